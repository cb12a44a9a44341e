"""Cost of anchor fitting on one MI355X.

python tools/anchor_fit_cost.py [reps]
    n = 1 M synthetic box sizes (four centres times exp(N(0, 0.25)), as the tests' mixture): y3_anchor_stats in per-anchor mode at
    (P, k) = (1, 9) -- a Lloyd step of one set, the report -- and (9, 9) -- the Lloyd step of fit_anchors' pool -- and in totals
    mode at (64, 9) -- one generation of the search -- beside the yardstick, a device-to-device copy_ of the same wh array; HIP
    event times (2 warm-up + reps launches each, one stream), then the NumPy path's wall time for the same three calls (once
    each).  Under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/anchor_fit_cost.py [reps]
    the kernel times are in the trace, and
python tools/anchor_fit_cost.py --trace DIR/.../*_kernel_trace.csv [reps]
    prints them per kernel and grid: launches, median, min and max in microseconds, the launches of one grid cut in launch order
    into parts of 2 + reps.
python tools/anchor_fit_cost.py --fit [gpu] [cpu]
    wall time of a whole fit_anchors(k=9, evolve=1000) on the same sizes, device 'gpu' then 'cpu', and of its Euclidean start
    (the host k-means both share); checks that the two fits are equal."""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

N = 1000000
WARMUP = 2
CASES = ((1, 9, 1), (9, 9, 1), (64, 9, 0))


def sizes(n=N, seed=0):
    rng = np.random.default_rng(seed)
    centres = np.array([(12, 12), (40, 90), (200, 60), (300, 300)], np.float64)
    c = centres[rng.integers(0, 4, n)]
    return np.maximum(np.rint(c * np.exp(rng.normal(0.0, 0.25, (n, 2)))), 1).astype(np.int32)


def candidates(P, k):
    return (np.random.default_rng(P * 100 + k).random((P, k, 2)) * 300 + 4).astype(np.float32)


def run(reps):
    import torch
    from yolo3 import _hip, anchors
    lib, check = _hip.lib, _hip.check
    st = torch.cuda.current_stream().cuda_stream
    wh = sizes()
    wh_dev = torch.from_numpy(wh).cuda()
    wh2 = torch.empty_like(wh_dev)
    print('# n = %d box sizes = %.2f MB of int32 (w, h)' % (N, wh.nbytes / 1e6))
    print('%-44s %14s %10s %10s' % ('entry', 'IoUs per call', 'median us', 'min us'))
    entries = [('copy_ of the wh array', lambda: wh2.copy_(wh_dev), 0)]
    keep = []
    for P, k, per_anchor in CASES:
        cand = torch.from_numpy(candidates(P, k)).cuda()
        out = torch.empty((P * k * 5 if per_anchor else P * 2) + 1, dtype=torch.int64, device='cuda')
        ws = torch.empty(int(lib.y3_anchor_stats_workspace_bytes(P, k)) // 8, dtype=torch.int64, device='cuda')
        keep.append((cand, out, ws))
        entries.append(('anchor_stats %s P = %d, k = %d' % ('per-anchor' if per_anchor else 'totals', P, k),
                        lambda cand=cand, out=out, ws=ws, P=P, k=k, per_anchor=per_anchor: check(lib.y3_anchor_stats(
                            wh_dev.data_ptr(), N, cand.data_ptr(), P, k, 1 << 23, per_anchor, out.data_ptr(), None, ws.data_ptr(), st)), N * P * k))
    for name, fn, work in entries:
        times = []
        for r in range(WARMUP + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                times.append(e0.elapsed_time(e1) * 1e3)
        print('%-44s %14d %10.1f %10.1f' % (name, work, np.median(times), min(times)))
    print('# the NumPy path, same calls, wall time of one call each')
    for P, k, per_anchor in CASES:
        t0 = time.perf_counter()
        anchors.anchor_stats(wh, candidates(P, k), per_anchor=bool(per_anchor), device='cpu')
        print('%-44s %14d %10.3f s' % ('numpy %s P = %d, k = %d' % ('per-anchor' if per_anchor else 'totals', P, k), N * P * k, time.perf_counter() - t0))


def fit(devices=('gpu', 'cpu')):
    import torch
    from yolo3 import anchors
    wh = sizes()
    t0 = time.perf_counter()
    anchors.kmeans(wh[:, ::-1].astype(np.float64), 9, np.random.default_rng(0))
    t_euclid = time.perf_counter() - t0
    print('Euclidean k-means start (host, inside both fits)   %8.2f s' % t_euclid)
    out = {}
    for device in devices:
        t0 = time.perf_counter()
        out[device] = anchors.fit_anchors(wh, 9, seed=0, evolve=1000, device=device)
        if device == 'gpu':
            torch.cuda.synchronize()
        t = time.perf_counter() - t0
        print('fit_anchors(k=9, evolve=1000, device=%r)           %8.2f s, of which not the Euclidean start %8.2f s; fitness %.6f'
              % (device, t, t - t_euclid, out[device]['fitness']))
    if len(out) == 2:
        print('the two fits are %s' % ('equal' if out['gpu'] == out['cpu'] else 'DIFFERENT'))


def from_trace(path, reps=None):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            key = (r['Kernel_Name'].split('(')[0][-60:], r.get('Grid_Size_X', r.get('Grid_Size', '')), r.get('Grid_Size_Y', ''), r.get('Grid_Size_Z', ''))
            groups.setdefault(key, []).append((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    print('%-60s %-18s %-6s %8s %10s %10s %10s' % ('kernel', 'grid', 'part', 'launches', 'median us', 'min us', 'max us'))
    for key in sorted(groups):
        us = [t for _, t in sorted(groups[key])]
        step = (WARMUP + reps) if reps else len(us)
        parts = [us[i:i + step] for i in range(0, len(us), step)]
        for p, part in enumerate(parts):
            print('%-60s %-18s %-6d %8d %10.2f %10.2f %10.2f' % (key[0], 'x'.join(k for k in key[1:] if k), p, len(part), np.median(part), min(part), max(part)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else None)
    elif args and args[0] == '--fit':
        fit(tuple(args[1:]) or ('gpu', 'cpu'))
    else:
        run(int(args[0]) if args else 20)
