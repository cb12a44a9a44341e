"""Cost of the opt-in mosaic pass on one MI355X.

python tools/mosaic_cost.py [reps]
    batches of 8 x 3 x 416^2 and 8 x 3 x 608^2: the augmentation of a uint8 batch stored 40 pixels larger (every image with scale,
    flips, noise and blur, so all three augment kernels run), the mosaic of its result (records of draw_mosaic, prob = 1), the
    z-score, and two yardsticks that move the same bytes: a device-to-device copy_ and an elementwise multiply by one.  Prints
    the byte counts and HIP event times of the entries (2 warm-up + reps launches each, one stream); under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/mosaic_cost.py [reps]
    the kernel times are in the trace, and
python tools/mosaic_cost.py --trace DIR/.../*_kernel_trace.csv
    prints them per kernel and grid (the two sizes launch different grids): launches, median, min and max in microseconds."""
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
    from yolo3.imagereader import augment_device, mosaic_device, zscore_normalize_device
    print('%-6s %-22s %12s %10s %10s' % ('side', 'entry', 'MB moved', 'median us', 'min us'))
    for side in SIDES:
        rng = np.random.default_rng(side)
        stored = side + 40
        raw = torch.from_numpy(rng.integers(0, 256, (N, stored, stored, C), dtype=np.uint8)).cuda()
        np.random.seed(side)
        recs = np.concatenate([augment.draw_augmentation((stored, stored, C), None, crop_to=(side, side), reflection_flag=True,
                                                         noise_augmentation_severity=0.03, scale_augmentation_severity=0.1,
                                                         blur_augmentation_max_sigma=2)[0] for _ in range(N)])
        recs['blur_sigma'] = np.minimum(np.abs(recs['blur_sigma']) + 0.5, 2.0)      # every image blurred: the three-kernel case
        mrec = augment.draw_mosaic(0, 0, 0, N, (side, side), 1.0)
        x = augment_device(raw, recs, (side, side))
        y = torch.empty_like(x)
        mb = 2 * x.numel() * 4 / 1e6
        entries = [('augment (3 kernels)', lambda: augment_device(raw, recs, (side, side)), (raw.numel() + 5 * x.numel() * 4) / 1e6),
                   ('mosaic', lambda: mosaic_device(x, mrec), mb),
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
            print('%-6d %-22s %12.2f %10.1f %10.1f' % (side, name[:22], moved, np.median(times), min(times)))
        assert torch.equal(mosaic_device(x, mrec).view(torch.int32).cpu(), torch.from_numpy(augment.mosaic_reference(x.cpu().numpy(), mrec)).view(torch.int32))


def from_trace(path):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            key = (r['Kernel_Name'].split('(')[0][-60:], r.get('Grid_Size_X', r.get('Grid_Size', '')), r.get('Grid_Size_Y', ''), r.get('Grid_Size_Z', ''))
            groups.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('%-60s %-18s %8s %10s %10s %10s' % ('kernel', 'grid', 'launches', 'median us', 'min us', 'max us'))
    for key in sorted(groups):
        us = groups[key]
        print('%-60s %-18s %8d %10.2f %10.2f %10.2f' % (key[0], 'x'.join(k for k in key[1:] if k), len(us), np.median(us), min(us), max(us)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1])
    else:
        run(int(args[0]) if args else 20)
