"""CPU-only: the host side of fine-tuning -- load_pretrained's layer mapping, the trainable arena suffix and its
decay ranges, argument validation, the train.py flags, the data-parallel exchange of the suffix alone (gloo, two ranks), and the
float32 restatement of y3_bn_frozen_bwd against the fp64 one (tests/finetune_reference.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import finetune_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')


def _shapes(specs):
    return [(sp.k, sp.k, sp.cin, sp.cout) for sp in specs]


def _specs(classes=2, anchors=2, spp=False, channels=3):
    from yolo3.model import build_layer_specs
    return build_layer_specs(channels, anchors, classes, spp)[0]


def test_pretrained_map_by_role():
    from yolo3.model import pretrained_map, spp_transfer_map
    plain = _specs()
    heads = [i for i, sp in enumerate(plain) if not sp.bn]
    assert heads == [58, 66, 74]
    # equal heads: everything loads
    assert pretrained_map(plain, False, _shapes(plain), False) == (list(range(75)), [])
    # another class count, another anchor count: the three heads keep their initialisation, every other layer maps to itself
    for other in (_specs(classes=3), _specs(anchors=3)):
        mapping, kept = pretrained_map(other, False, _shapes(plain), False)
        assert kept == heads and [j for j in mapping if j is not None] == [i for i in range(75) if i not in heads]
        assert all(mapping[i] is None for i in heads)
    # plain file into an SPP model: spp_transfer_map, the layer behind the pools is fresh; with another class count the heads too
    spp = _specs(spp=True)
    mapping, kept = pretrained_map(spp, True, _shapes(plain), False)
    assert mapping == spp_transfer_map(spp) and kept == [mapping.index(None)] and len(spp) == 76
    spp3 = _specs(classes=3, spp=True)
    mapping, kept = pretrained_map(spp3, True, _shapes(plain), False)
    assert kept == sorted([spp_transfer_map(spp3).index(None)] + [i for i, sp in enumerate(spp3) if not sp.bn])
    # SPP file into an SPP model
    assert pretrained_map(spp, True, _shapes(spp), True)[1] == []


def test_pretrained_map_refuses():
    from yolo3.model import pretrained_map
    plain, spp = _specs(), _specs(spp=True)
    with pytest.raises(ValueError, match='SPP'):
        pretrained_map(plain, False, _shapes(spp), True)
    with pytest.raises(ValueError, match='input channels'):
        pretrained_map(plain, False, _shapes(_specs(channels=1)), False)
    with pytest.raises(ValueError, match='layers'):
        pretrained_map(plain, False, _shapes(plain)[:-1], False)
    body = _shapes(plain)
    body[10] = (1, 1, 128, 96)
    with pytest.raises(ValueError, match='layer 10'):
        pretrained_map(plain, False, body, False)


def test_trainable_suffix_and_decay_ranges():
    from yolo3.model import build_layer_specs, trainable_suffix, suffix_decay_ranges, decay_ranges, ALIGN, BACKBONE_LAYERS
    specs, arena, _, _ = build_layer_specs(3, 2, 2)
    assert BACKBONE_LAYERS == 52 and specs[51].k == 3 and specs[52].k == 1 and specs[52].cin == 1024      # the first yolo block starts there
    full = decay_ranges(specs)
    for n in (0, 1, 2, 52, len(specs) - 1):
        off, count = trainable_suffix(specs, arena, n)
        assert off == specs[n].w_off and off % ALIGN == 0 and off + count == arena
        assert (off == 0) == (n == 0)
        ranges = suffix_decay_ranges(specs, n)
        assert len(ranges) == len(specs) - n
        assert [(lo + off, hi + off) for lo, hi in ranges] == full[n:]
        assert ranges[0][0] == 0 and all(0 <= lo < hi <= count and lo % 4 == 0 and hi % 4 == 0 for lo, hi in ranges)
    assert suffix_decay_ranges(specs, 0) == full


def test_argument_validation():
    from yolo3.model import check_freeze_args, YoloV3
    check_freeze_args()
    check_freeze_args(52, True, 75)
    check_freeze_args(np.int64(74), np.bool_(False), 75)
    for bad in (-1, 75, 1.0, '2', None, True):
        with pytest.raises(ValueError, match='freeze_layers'):
            check_freeze_args(bad, False, 75)
    for bad in (2, 'yes', None, 0.0):
        with pytest.raises(ValueError, match='freeze_bn'):
            check_freeze_args(0, bad, 75)
    # the constructor checks before it needs a device: the SPP network has one layer more
    for kw in (dict(freeze_layers=75), dict(freeze_layers=76, spp=True), dict(freeze_layers=-1), dict(freeze_bn='1')):
        with pytest.raises(ValueError, match='freeze'):
            YoloV3(2, [64, 64, 3], 2, [(64, 384), (384, 64)], **kw)


def _parse(*extra):
    sys.path.insert(0, PKG)
    import train
    return train.build_parser().parse_args(['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c'] + list(extra))


def test_train_flags(capsys):
    a = _parse()
    assert (a.init_weights, a.init_optimizer, a.freeze_layers, a.freeze, a.freeze_bn) == (None, 0, 0, None, 0)
    a = _parse('--freeze', 'backbone', '--freeze_bn', '1', '--init_weights', 'w.npz', '--init_optimizer', '1')
    b = _parse('--freeze_layers', '52', '--freeze_bn', '1', '--init_weights', 'w.npz', '--init_optimizer', '1')
    assert a.freeze_layers == b.freeze_layers == 52 and a.freeze_bn == b.freeze_bn == 1 and a.init_weights == 'w.npz' and a.init_optimizer == 1
    assert _parse('--freeze', 'backbone', '--freeze_layers', '52').freeze_layers == 52
    for bad in (['--freeze', 'backbone', '--freeze_layers', '10'], ['--freeze_layers', '-1'], ['--freeze_layers', 'x'], ['--freeze', 'head'],
                ['--freeze_bn', '2'], ['--init_optimizer', '1']):
        with pytest.raises(SystemExit):
            _parse(*bad)
    capsys.readouterr()
    import train
    from yolo3.model import BACKBONE_LAYERS
    assert train.FREEZE_NAMES == {'backbone': BACKBONE_LAYERS}
    line = train.describe_freeze(_specs(), 52, True)
    assert '52 of 75 layers frozen' in line and '23 layers train' in line and 'stored statistics' in line
    specs = _specs()
    count = lambda sp: sp.k * sp.k * sp.cin * sp.cout + sp.cout * (3 if sp.bn else 1)
    assert '(%d parameters' % sum(count(sp) for sp in specs[:52]) in line and '(%d parameters)' % sum(count(sp) for sp in specs[52:]) in line
    with pytest.raises(ValueError, match='init_optimizer'):
        train.train_model(2, 1, 'a', 'b', 'c', 1, 1e-4, False, init_optimizer=True)


def test_float32_restatement_against_fp64():
    """dz of the float32 restatement is within its two roundings of the unrounded expression; slope decisions on +-0 go to alpha;
    the bound of the sums covers the difference between exact sums and plain fp64 accumulation in another order."""
    rng = np.random.default_rng(3)
    m, c = 257, 32
    dy = rng.standard_normal((m, c)).astype(np.float32)
    a = rng.standard_normal((m, c)).astype(np.float32)
    a[0, :] = 0.0
    a[1, :] = -0.0
    scale = rng.standard_normal(c).astype(np.float32)
    for alpha in (np.float32(0.2), np.float32(0.1)):
        dz32 = fr.frozen_dz_f32(dy, a, scale, alpha)
        dz64 = fr.frozen_dz_f64(dy, a, scale, alpha)
        assert dz32.dtype == np.float32
        assert (np.abs(dz32 - dz64) <= 2 * (2.0 ** -24) * np.abs(dz64) * (1 + 2.0 ** -23) + 2.0 ** -149).all()
        t = (dy[:2] * scale[None, :]).astype(np.float32)
        assert np.array_equal(dz32[:2], (t * alpha).astype(np.float32))
    assert np.array_equal(fr.frozen_dres_f32(dy, a, False), dy) and np.array_equal(fr.frozen_dres_f32(dy, a, True), a + dy)
    mean, var = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.01).astype(np.float32)
    dz32 = fr.frozen_dz_f32(dy, a, scale)
    S = fr.frozen_sums_f64(dy, a, dz32)
    want = fr.frozen_results_f64(*S, mean, var)
    bounds = fr.frozen_bounds(dy, a, dz32, mean, var)
    # plain fp64 accumulation in reversed row order, each result rounded to fp32 as the kernel does
    d64, a64 = dy.astype(np.float64)[::-1], a.astype(np.float64)[::-1]
    S1, S2, S3 = (np.add.reduce(x, 0) for x in (d64, d64 * a64, dz32.astype(np.float64)[::-1]))
    got = fr.frozen_results_f64(S1, S2, S3, mean, var)
    for g, w, b in zip(got, want, bounds):
        assert (np.abs(g.astype(np.float32).astype(np.float64) - w) <= b).all()
        assert (b <= 3 * (2.0 ** -24) * np.maximum(np.abs(w), 1e-3) + 1e-9).all()       # ... and is no looser than a few fp32 roundings here
    # fp32 accumulation is what the bound must NOT admit for the long sums
    bad = np.cumsum(dy, 0, dtype=np.float32)[-1].astype(np.float64)
    assert (np.abs(bad - want[1]) > bounds[1]).any()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, PKG)
    from yolo3.parallel import DataParallel
    from yolo3.model import build_layer_specs
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world)

    class Fake:
        pass
    m = Fake()
    m.specs, _, _, _ = build_layer_specs(3, 2, 2)
    lo = m.specs[-6].w_off                      # (the last six layers: light, as test_cpu_abi_and_dist does)
    m.specs = m.specs[-6:]
    for sp in m.specs:
        sp.w_off -= lo
        sp.end_off -= lo
    m.freeze_layers = 2
    m.grads = torch.randn(m.specs[-1].end_off, generator=torch.Generator().manual_seed(rank))
    mine = m.grads.clone()
    dp = DataParallel(bucket_mb=1.0).attach(m)
    dp.begin_step()
    for i in range(len(m.specs) - 1, m.freeze_layers - 1, -1):       # backward reports the trainable layers only
        dp.on_layer_done(i)
    dp.finish_step()
    q.put((rank, mine.numpy(), m.grads.numpy(), dp.buckets, m.specs[2].w_off))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_exchanges_the_trainable_suffix_only():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    off = res[0][4]
    total = res[0][1] + res[1][1]
    for _, mine, after, buckets, _ in res:
        assert np.array_equal(after[:off], mine[:off])                       # the frozen prefix never travels
        np.testing.assert_allclose(after[off:], total[off:], rtol=1e-6, atol=1e-6)
        assert buckets[-1][0] == off and buckets[0][1] == len(mine) and all(first >= 2 for _, _, first in buckets)
        assert sum(hi - lo for lo, hi, _ in buckets) == len(mine) - off
