"""Cost of tile test-time augmentation on one MI355X.

python tools/tile_tta_cost.py [images]
    bench.py's tiled_4k case (one synthetic 4096 x 4096 x 3 uint8 image, 608 x 608 tiles, random-init weights, bf16 convs, default
    schedule and host merge): the whole of inference_image_tiled per image, host clock around a device synchronise, with tile_tta
    none, hflip, flips and d4 ALTERNATED in one process after one warm-up image each.  Prints the median, minimum and maximum per
    setting; the `none` row is the yardstick.
python tools/tile_tta_cost.py --kernels [repetitions]
    The first 10 tiles of that image, first with the 4 views of `flips` (all repetitions), then with the 8 of `d4`: the fused
    gather (y3_tile_gather_zscore_views_nhwc), the three-launch composition it replaces (y3_tile_gather -> y3_zscore ->
    y3_tta_views_nhwc), y3_tile_gather_zscore_nhwc over the same tiles (k = 1) and a device-to-device copy (y3_copy) of the bytes
    the gather writes.  Checks that the two routes give the same bits.  Under
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/tile_tta_cost.py --kernels 5
    the kernel times are in the trace, and
python tools/tile_tta_cost.py --trace DIR/.../*_kernel_trace.csv [repetitions]
    prints them: per kernel the launches of the `flips` half and of the `d4` half, median, min and max in microseconds."""
import contextlib
import csv
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'object-detection-yolov3_amd'))
import numpy as np   # noqa: E402

K = 2
ANCHORS = [(64, 384), (384, 64)]      # bench.py's
TILE, NTILES = 608, 10


def _image():
    return np.random.default_rng(4).integers(0, 256, (4096, 4096, 3), dtype=np.uint8)


def run(images):
    import torch
    import inference_tiled
    from yolo3.model import YoloV3
    y = YoloV3(25, [TILE, TILE, 3], K, ANCHORS, seed=1, use_graph=True)
    y.inference_precision = 'bf16'
    mdl = y.get_keras_model()
    big = _image()
    settings = ('none', 'hflip', 'flips', 'd4')
    times = {s: [] for s in settings}
    found = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for s in settings:          # warm-up: code objects, plans, graphs, buffers
            found[s] = inference_tiled.inference_image_tiled(mdl, big, [TILE, TILE], 32, tile_tta=s).shape[0]
        torch.cuda.synchronize()
        for _ in range(images):
            for s in settings:
                t1 = time.perf_counter()
                inference_tiled.inference_image_tiled(mdl, big, [TILE, TILE], 32, tile_tta=s)
                torch.cuda.synchronize()
                times[s].append((time.perf_counter() - t1) * 1e3)
    print('detections: ' + ', '.join('%s %d' % (s, found[s]) for s in settings))
    print('%-8s %8s %10s %10s %10s %12s' % ('tile_tta', 'images', 'median ms', 'min ms', 'max ms', 'x none'))
    base = np.median(times['none'])
    for s in settings:
        t = times[s]
        print('%-8s %8d %10.2f %10.2f %10.2f %12.2f' % (s, len(t), np.median(t), min(t), max(t), np.median(t) / base))


def kernels(reps):
    import torch
    import inference_tiled
    from yolo3 import _hip, bbox_utils, imagereader
    lib, check = _hip.lib, _hip.check
    big = _image()
    table = torch.from_numpy(inference_tiled.tile_table(4096, 4096, [TILE, TILE])[0][:NTILES].copy()).cuda()
    img = torch.from_numpy(big).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(int(lib.y3_zscore_workspace_bytes(NTILES)) // 8 + 1, dtype=torch.float64, device='cuda')
    base = torch.empty(NTILES, TILE, TILE, 4, device='cuda')
    for name in ('flips', 'd4'):
        views = bbox_utils.TTA_VIEWS[name]
        k, codes = len(views), _hip.int_array(views)
        fused = torch.empty(NTILES * k, TILE, TILE, 4, device='cuda')
        split = torch.empty_like(fused)
        dup = torch.empty_like(fused)
        for _ in range(reps + 1):          # the first pass is the warm-up; --trace drops it
            check(lib.y3_tile_gather_zscore_views_nhwc(img.data_ptr(), 0, 4096, 4096, 3, table.data_ptr(), NTILES, TILE, TILE, codes, k,
                                                       fused.data_ptr(), 4, ws.data_ptr(), st), 'y3_tile_gather_zscore_views_nhwc')
            tiles = inference_tiled.tiles_to_device(img, 0, big.shape, table, 0, NTILES, [TILE, TILE])
            z = imagereader.zscore_normalize_device(tiles)
            check(lib.y3_tta_views_nhwc(z.data_ptr(), NTILES, 3, TILE, TILE, codes, k, _hip.view(split, NTILES * k, TILE, TILE, 4), st),
                  'y3_tta_views_nhwc')
            check(lib.y3_tile_gather_zscore_nhwc(img.data_ptr(), 0, 4096, 4096, 3, table.data_ptr(), NTILES, TILE, TILE, base.data_ptr(), 4,
                                                 ws.data_ptr(), st), 'y3_tile_gather_zscore_nhwc')
            check(lib.y3_copy(_hip.view(fused, NTILES * k, TILE, TILE, 4), _hip.view(dup, NTILES * k, TILE, TILE, 4), st), 'y3_copy')
        torch.cuda.synchronize()
        same = torch.equal(fused.view(torch.int32), split.view(torch.int32)) and torch.equal(fused.view(torch.int32), dup.view(torch.int32))
        print('%s: %d tiles x %d views, %.1f MB written, fused gather == three-launch composition: %s' % (
            name, NTILES, k, fused.numel() * 4 / 1e6, same))
        assert same


WANTED = ('tile_gather_views_kernel', 'tile_gather_norm_kernel', 'tile_gather_kernel', 'tile_stats_kernel', 'tile_stats_finalize_kernel',
          'zscore_partial_kernel', 'zscore_apply_kernel', 'tta_views_kernel', 'copy_add_kernel')


def from_trace(path, reps):
    groups = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r['Kernel_Name'].split('(')[0].split('<')[0].split()[-1]
            if name in WANTED:
                groups.setdefault(name, []).append((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    print('%-28s %-6s %8s %10s %10s %10s' % ('kernel', 'views', 'launches', 'median us', 'min us', 'max us'))
    for name in WANTED:
        runs = [us for _, us in sorted(groups.get(name, []))]
        half = len(runs) // 2          # kernels(): every `flips` launch comes before the first `d4` launch
        for label, part in (('flips', runs[:half]), ('d4', runs[half:])):
            part = part[len(part) // (reps + 1):]          # without the warm-up pass
            if part:
                print('%-28s %-6s %8d %10.2f %10.2f %10.2f' % (name, label, len(part), np.median(part), min(part), max(part)))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--trace':
        from_trace(args[1], int(args[2]) if len(args) > 2 else 5)
    elif args and args[0] == '--kernels':
        kernels(int(args[1]) if len(args) > 1 else 5)
    else:
        run(int(args[0]) if args else 7)
