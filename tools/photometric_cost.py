"""Cost of the opt-in colour / tone jitter and MixUp pass on one MI355X.

python tools/photometric_cost.py [reps]
    batches of 8 x 3 x 416^2 and 8 x 3 x 608^2 of float32 through y3_photometric_batch with three kinds of records -- identity
    (a copy through the kernel), matrix only (drawn hue / saturation / value, clamp on, no tone curve, no MixUp) and matrix + gamma
    + MixUp (every image changed, tone exponent 2^+-1, every image mixed: two source images read per output image) -- and two
    yardsticks that move the bytes of the identity case: a device-to-device copy_ and an elementwise multiply by one; the z-score
    of the same tensors for scale.  Prints the byte counts and HIP event times of the entries (2 warm-up + reps launches each, one
    stream); under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/photometric_cost.py [reps]
    the kernel times are in the trace, and
python tools/photometric_cost.py --trace DIR/.../*_kernel_trace.csv [reps]
    prints them per kernel and grid (the two sizes launch different grids): launches, median, min and max in microseconds.  With
    reps given, the launches of a grid are cut in launch order into parts of 2 + reps, so that the three photometric entries of one
    size (same grid) and the yardsticks can be told apart."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

N, C = 8, 3
SIDES = (416, 608)
WARMUP = 2


def run(reps):
    import torch
    from yolo3 import augment
    from yolo3.imagereader import photometric_device, zscore_normalize_device
    print('%-6s %-30s %12s %10s %10s' % ('side', 'entry', 'MB moved', 'median us', 'min us'))
    for side in SIDES:
        rng = np.random.default_rng(side)
        x = torch.from_numpy(rng.integers(0, 256, (N, C, side, side)).astype(np.float32)).cuda()
        ident = augment.photo_identity_records(N)
        matrix = augment.draw_photometric(0, 0, 0, N, C, 1.0, 0.015, 0.7, 0.4, 0.0, 255.0)
        full = augment.draw_mixup(augment.draw_photometric(0, 0, 0, N, C, 1.0, 0.015, 0.7, 0.4, 1.0, 255.0), 0, 0, 0, 1.0, 0.1)
        assert (matrix['gamma'] == 1).all() and (full['gamma'] != 1).all() and (full['lambda'] < 1).all()
        y = torch.empty_like(x)
        mb = 2 * x.numel() * 4 / 1e6
        entries = [('photometric, identity', lambda: photometric_device(x, ident), mb),
                   ('photometric, matrix only', lambda: photometric_device(x, matrix), mb),
                   ('photometric, matrix+gamma+mixup', lambda: photometric_device(x, full), 1.5 * mb),
                   ('copy_ (device to device)', lambda: y.copy_(x), mb),
                   ('multiply by one', lambda: torch.mul(x, 1.0, out=y), mb),
                   ('z-score', lambda: zscore_normalize_device(x), 1.5 * mb)]
        for name, fn, moved in entries:
            times = []
            for r in range(WARMUP + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= WARMUP:
                    times.append(e0.elapsed_time(e1) * 1e3)
            print('%-6d %-30s %12.2f %10.1f %10.1f' % (side, name[:30], moved, np.median(times), min(times)))
        assert torch.equal(photometric_device(x, ident).view(torch.int32), x.view(torch.int32))
        got = photometric_device(x[:2].contiguous(), matrix[:2]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), augment.photometric_reference(x[:2].cpu().numpy(), matrix[:2]).view(np.uint32))


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
        parts = [us[i:i + step] for i in range(0, len(us), step)]      # (a short last part: the launches of the closing checks)
        for p, part in enumerate(parts):
            print('%-60s %-18s %-6d %8d %10.2f %10.2f %10.2f' % (key[0], 'x'.join(k for k in key[1:] if k), p, len(part), np.median(part), min(part), max(part)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else None)
    else:
        run(int(args[0]) if args else 20)
