"""GPU tests of the exponential moving average of the weights: the fused Adam + EMA kernel against y3_adam_step
and the NumPy float32 recurrence, bit for bit; a model with the EMA trains exactly like one without; ema_weights() swaps the
average in and restores every derived copy; the model-level recurrence, eager and graph; export; and train.py --ema_decay
against evaluate.py on the model it exported, in one process and under two gloo ranks."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _numpy_ema(e, x, omd):
    """The kernel's expression in float32 (the library is built with -ffp-contract=off)."""
    return (e + (x - e) * np.float32(omd)).astype(np.float32)


@pytest.mark.parametrize('count,mcount', [(1000003, 10001), (5, 7), (8, 3), (6, 40001)])
def test_fused_kernel_bits(count, mcount):
    from yolo3._hip import lib, check
    rng = np.random.default_rng(count + mcount)
    dev = torch.device('cuda')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    p0 = rng.standard_normal(count).astype(np.float32)
    m0 = (rng.standard_normal(count) * 1e-3).astype(np.float32)
    v0 = (rng.random(count) * 1e-5).astype(np.float32)
    e0 = (p0 + rng.standard_normal(count).astype(np.float32) * 1e-2).astype(np.float32)
    me0 = rng.random(mcount).astype(np.float32)
    p, m, v, e = t(p0), t(m0), t(v0), t(e0)
    rp, rm, rv = t(p0), t(m0), t(v0)                   # y3_adam_step on copies
    mov, emov = t(me0), t(me0 + 0.5)
    lr_dev, omd_dev = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    e_want, me_want = e0.copy(), (me0 + np.float32(0.5)).astype(np.float32)
    st = torch.cuda.current_stream().cuda_stream
    for step, (lr_t, omd) in enumerate([(1e-3, 0.75), (3.3e-4, np.float32(1 - 0.99 * (1 - np.exp(-2 / 4)))), (2e-3, 1e-4)]):
        g = t(rng.standard_normal(count) * 1e-2)
        mov.copy_(t(rng.random(mcount)))              # the forward pass's new moving statistics
        lr_dev.fill_(lr_t)
        omd_dev.fill_(float(np.float32(omd)))
        check(lib.y3_adam_step_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), count, lr_dev.data_ptr(), 0.9, 0.999, 1e-7,
                                   e.data_ptr(), mov.data_ptr(), emov.data_ptr(), mcount, omd_dev.data_ptr(), st), 'y3_adam_step_ema')
        check(lib.y3_adam_step(rp.data_ptr(), g.data_ptr(), rm.data_ptr(), rv.data_ptr(), count, lr_dev.data_ptr(), 0.9, 0.999, 1e-7, st),
              'y3_adam_step')
        torch.cuda.synchronize()
        assert torch.equal(p, rp) and torch.equal(m, rm) and torch.equal(v, rv), step
        e_want = _numpy_ema(e_want, rp.cpu().numpy(), omd)
        me_want = _numpy_ema(me_want, mov.cpu().numpy(), omd)
        assert np.array_equal(e.cpu().numpy(), e_want), step
        assert np.array_equal(emov.cpu().numpy(), me_want), step


def _case(seed=3, img=96, n=2):
    from dp_worker import make_case
    anchors, K, params, images, gts = make_case(img, n, seed)
    return anchors, K, params, images.cuda(), [torch.from_numpy(x).cuda() for x in gts]


def _model(case, **kw):
    from yolo3.model import YoloV3
    anchors, K, params, images, _ = case
    y = YoloV3(int(images.shape[0]), [int(images.shape[2]), int(images.shape[3]), 3], K, anchors, learning_rate=1e-3, **kw)
    y.set_weights(params)
    return y


def _live(y):
    """The arenas and every copy derived from them that inference or the next step reads."""
    return [x.clone() for x in (y.params, y.params_t, y.planes, y.planes_t, y.moving) if x is not None]


def test_ema_is_passive_and_the_swap_restores_everything():
    case = _case()
    images, gts = case[3], case[4]
    raw = _model(case)
    ema = _model(case, ema_decay=0.99, ema_warmup=4)
    assert raw.ema_params is None and ema.ema_params.numel() == ema.arena_floats
    assert torch.equal(ema.ema_params, ema.params) and torch.equal(ema.ema_moving, ema.moving)
    with pytest.raises(RuntimeError):
        with raw.ema_weights():
            pass
    for step in range(4):
        if step == 2:
            # warm the bf16 copy, then use the average through test_step and both predict precisions
            ema.predict(images, precision='bf16')
            live = _live(ema)
            raw_rows = ema.predict(images).clone()
            with ema.ema_weights():
                assert torch.equal(ema.params, ema.ema_params) and torch.equal(ema.moving, ema.ema_moving)
                float(ema.test_step((images, gts)))
                in_rows = ema.predict(images).clone()
                ema.predict(images, precision='bf16')
                with pytest.raises(RuntimeError):
                    ema.train_step((images, gts))
            assert not torch.equal(in_rows, raw_rows)            # the average really was in place
            for a, b in zip(live, _live(ema)):
                assert torch.equal(a, b)
        lr = float(raw.train_step((images, gts)))
        le = float(ema.train_step((images, gts)))
        torch.cuda.synchronize()
        assert lr == le, step
        for name in ('params', 'adam_m', 'adam_v', 'moving', 'grads'):
            assert torch.equal(getattr(raw, name), getattr(ema, name)), (step, name)
    assert not torch.equal(ema.ema_params, ema.params)
    for prec in ('fp32', 'bf16'):
        assert torch.equal(raw.predict(images, precision=prec), ema.predict(images, precision=prec)), prec


def test_model_recurrence_eager_and_graph():
    from yolo3.model import ema_one_minus_decay
    case = _case(seed=4)
    images, gts = case[3], case[4]
    eager = _model(case, ema_decay=0.99, ema_warmup=4)
    graph = _model(case, ema_decay=0.99, ema_warmup=4, use_graph=True)
    e_p, e_m = eager.params.cpu().numpy(), eager.moving.cpu().numpy()
    for t in range(1, 6):
        eager.train_step((images, gts))
        graph.train_step((images, gts))
        torch.cuda.synchronize()
        omd = ema_one_minus_decay(0.99, 4, t)
        assert float(eager.ema_omd_dev.item()) == float(omd)
        e_p = _numpy_ema(e_p, eager.params.cpu().numpy(), omd)
        e_m = _numpy_ema(e_m, eager.moving.cpu().numpy(), omd)
        assert np.array_equal(eager.ema_params.cpu().numpy(), e_p), t
        assert np.array_equal(eager.ema_moving.cpu().numpy(), e_m), t
        assert torch.equal(graph.ema_params, eager.ema_params) and torch.equal(graph.ema_moving, eager.ema_moving), t
        assert torch.equal(graph.params, eager.params), t
    # reset_ema restarts the average from the live weights
    eager.reset_ema()
    assert torch.equal(eager.ema_params, eager.params) and torch.equal(eager.ema_moving, eager.moving)


def test_export_inside_the_block(tmp_path):
    from yolo3.model import YoloV3
    case = _case(seed=5)
    images, gts = case[3], case[4]
    y = _model(case, ema_decay=0.9, ema_warmup=2)
    for _ in range(3):
        y.train_step((images, gts))
    path = os.path.join(str(tmp_path), 'ema.npz')
    with y.ema_weights():
        y.save_weights(path)
        want = y.predict(images).clone()
        weights = y.get_weights()
    raw_rows = y.predict(images).clone()
    got = YoloV3.from_file(path).predict(images)
    assert torch.equal(got, want) and not torch.equal(got, raw_rows)
    z = np.load(path)
    bn = next(k for k in sorted(z.files) if k.endswith('_mean'))
    assert np.array_equal(z['l000_W'], weights[0]['W']) and np.array_equal(z[bn], weights[int(bn[1:4])]['mean'])
    # the replacement moving statistics of ema_weights(moving=...) are the ones the block sees
    alt = y.ema_moving * 0.5 + 0.25
    with y.ema_weights(alt):
        assert torch.equal(y.moving, alt) and torch.equal(y.params, y.ema_params)


# ---- train.py --ema_decay -----------------------------------------------------------------------------------------------
def _exported(out):
    z = np.load(os.path.join(out, 'saved_model', 'yolov3.npz'))
    return {k: z[k] for k in z.files if k.startswith('l')}


def test_train_ema_one_process(tmp_path):
    from test_gpu_cli import _write_dataset
    from test_gpu_train_map import _train, _map_csv, _evaluate_cli, _check_row_against_evaluate
    tmp = str(tmp_path)
    _write_dataset(tmp, 15, (160, 160, 3))
    base = _train(tmp, os.path.join(tmp, 'base'), ['--test_map', '1', '--test_map_min_box_size', '8'])
    assert 'moving average' not in base.stdout
    out = os.path.join(tmp, 'ema')
    r = _train(tmp, out, ['--ema_decay', '0.9', '--test_map', '1', '--test_map_min_box_size', '8'])
    assert r.stdout.count('exponential moving average of the weights (decay 0.9,') == 1
    rows = _map_csv(out)
    assert [x[0] for x in rows] == [0, 1]
    losses = [float(v) for v in open(os.path.join(out, 'test_loss.csv')).read().split()]
    best = int(np.argmin(losses))
    _evaluate_cli(os.path.join(out, 'saved_model'), os.path.join(tmp, 'test-syn.lmdb'), 2, os.path.join(tmp, 'eval.csv'))
    _check_row_against_evaluate(rows[best], os.path.join(tmp, 'eval.csv'))
    a, b = _exported(os.path.join(tmp, 'base')), _exported(out)
    assert a.keys() == b.keys() and any(not np.array_equal(a[k], b[k]) for k in a)


def test_train_ema_two_gloo_ranks(tmp_path):
    from test_gpu_cli import _write_dataset
    from test_gpu_train_map import _train, _map_csv, _evaluate_cli, _check_row_against_evaluate
    tmp = str(tmp_path)
    _write_dataset(tmp, 15, (160, 160, 3))
    out = os.path.join(tmp, 'ema')
    r = _train(tmp, out, ['--ema_decay', '0.9', '--test_map', '1', '--test_map_min_box_size', '8'], ranks=2)
    assert r.stdout.count('exponential moving average of the weights') == 2        # one line per rank
    rows = _map_csv(out)
    assert [x[0] for x in rows] == [0, 1]
    losses = [float(v) for v in open(os.path.join(out, 'test_loss.csv')).read().split()]
    best = int(np.argmin(losses))
    _evaluate_cli(os.path.join(out, 'saved_model'), os.path.join(tmp, 'test-syn.lmdb'), 2, os.path.join(tmp, 'eval.csv'), ranks=2)
    _check_row_against_evaluate(rows[best], os.path.join(tmp, 'eval.csv'))
