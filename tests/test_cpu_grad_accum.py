"""Host side of gradient accumulation and global-norm gradient clipping: the new entry points' declarations,
exports, bindings and argument validation (no device needed: validation fails before any launch), the constructor's and
train.py's checks, and clip_scale() against its definition."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
sys.path.insert(0, PKG)

NEW = ('y3_grad_accumulate', 'y3_grad_sumsq', 'y3_grad_clip_scale', 'y3_grad_norm_workspace_bytes', 'y3_adam_step_scaled',
       'y3_adam_step_ema_scaled')
A = 1 << 20                # fake, 16-byte aligned addresses: validation fails before anything dereferences them


def test_entry_points_declared_exported_and_bound():
    from yolo3 import _hip
    hdr = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    so = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert ' %s(' % name in hdr, name
        assert name in _hip.SIGNATURES, name
        assert hasattr(so, name), name
    # the scaled kernels take the arguments of the unscaled ones plus the device scale
    for plain, scaled in (('y3_adam_step', 'y3_adam_step_scaled'), ('y3_adam_step_ema', 'y3_adam_step_ema_scaled')):
        assert len(_hip.SIGNATURES[scaled][1]) == len(_hip.SIGNATURES[plain][1]) + 1


def test_workspace_query_positive_and_monotone():
    from yolo3._hip import lib
    counts = [0, 1, 5, 8, 1000, 1000003, 61790400, 10 ** 9]
    sizes = [lib.y3_grad_norm_workspace_bytes(c) for c in counts]
    assert all(s > 0 and s % 8 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] < sizes[-1]


def test_accumulate_and_sumsq_argument_validation_without_device():
    from yolo3._hip import lib
    ok = dict(acc=A, g=2 * A, first=3 * A, ws=4 * A)

    def acc(**kw):
        d = dict(ok, **kw)
        return lib.y3_grad_accumulate(d['acc'], d['g'], 1000, d['first'], d['ws'], None)

    for k in ok:
        assert acc(**{k: None}) == -1, k
        assert b'null' in lib.y3_last_error(), k
    for k in ('acc', 'g'):
        assert acc(**{k: ok[k] + 4}) == -1, k
        assert b'aligned' in lib.y3_last_error(), k
    assert acc(ws=ok['ws'] + 4) == -1 and b'aligned' in lib.y3_last_error()
    assert lib.y3_grad_sumsq(None, 1000, A, None) == -1 and b'null' in lib.y3_last_error()
    assert lib.y3_grad_sumsq(A, 1000, None, None) == -1 and b'null' in lib.y3_last_error()
    assert lib.y3_grad_sumsq(A + 4, 1000, A, None) == -1 and b'aligned' in lib.y3_last_error()
    assert lib.y3_grad_sumsq(A, 1000, A + 4, None) == -1 and b'aligned' in lib.y3_last_error()


def test_clip_scale_argument_validation_without_device():
    from yolo3._hip import lib

    def call(ws=A, k=1, c=1.0, norm=2 * A, scale=3 * A):
        return lib.y3_grad_clip_scale(ws, 1000, k, c, norm, scale, None)

    for kw in (dict(ws=None), dict(norm=None), dict(scale=None)):
        assert call(**kw) == -1, kw
        assert b'null' in lib.y3_last_error(), kw
    assert call(ws=A + 4) == -1 and b'aligned' in lib.y3_last_error()
    for k in (0, -1):
        assert call(k=k) == -1, k
        assert b'accumulate_steps' in lib.y3_last_error(), k
    for c in (0.0, -1.0, -math.inf, math.nan):
        assert call(c=c) == -1, c
        assert b'clip_norm' in lib.y3_last_error(), c


def test_scaled_adam_argument_validation_without_device():
    from yolo3._hip import lib
    ok = dict(p=A, g=2 * A, m=3 * A, v=4 * A, lr=5 * A, e=6 * A, mv=7 * A, em=8 * A, omd=9 * A, s=10 * A)

    def plain(**kw):
        d = dict(ok, **kw)
        return lib.y3_adam_step_scaled(d['p'], d['g'], d['m'], d['v'], 1000, d['lr'], 0.9, 0.999, 1e-7, d['s'], None)

    def ema(**kw):
        d = dict(ok, **kw)
        return lib.y3_adam_step_ema_scaled(d['p'], d['g'], d['m'], d['v'], 1000, d['lr'], 0.9, 0.999, 1e-7, d['e'], d['mv'], d['em'], 37,
                                           d['omd'], d['s'], None)

    for k in ('p', 'g', 'm', 'v', 'lr', 's'):
        assert plain(**{k: None}) == -1, k
        assert b'null' in lib.y3_last_error(), k
    for k in ('p', 'g', 'm', 'v'):
        assert plain(**{k: ok[k] + 4}) == -1, k
        assert b'aligned' in lib.y3_last_error(), k
    for k in ('p', 'g', 'm', 'v', 'lr', 'e', 'omd', 's', 'mv', 'em'):
        assert ema(**{k: None}) == -1, k
        assert b'null' in lib.y3_last_error(), k
    for k in ('p', 'g', 'm', 'v', 'e', 'mv', 'em'):
        assert ema(**{k: ok[k] + 4}) == -1, k
        assert b'aligned' in lib.y3_last_error(), k
    # nothing to do: returns before launching
    assert lib.y3_adam_step_scaled(A, A, A, A, 0, A, 0.9, 0.999, 1e-7, A, None) == 0
    assert lib.y3_adam_step_ema_scaled(A, A, A, A, 0, A, 0.9, 0.999, 1e-7, A, None, None, 0, A, A, None) == 0


def test_check_grad_args():
    from yolo3.model import check_grad_args
    check_grad_args()
    for k, c in ((1, None), (1, 1.0), (4, 0.5), (64, 1e30), (np.int64(2), np.float32(3.0))):
        check_grad_args(k, c)
    for k in (0, -1, 1.5, 2.0, '2', None, True, math.nan):
        with pytest.raises(ValueError):
            check_grad_args(k, None)
    for c in (0, 0.0, -1.0, math.nan, math.inf, -math.inf, 'x', True):
        with pytest.raises(ValueError):
            check_grad_args(1, c)


@pytest.mark.parametrize('kw', [dict(accumulate_steps=0), dict(accumulate_steps=-2), dict(grad_clip_norm=0.0), dict(grad_clip_norm=-1.0),
                                dict(grad_clip_norm=math.nan), dict(grad_clip_norm=math.inf)])
def test_constructor_refuses_bad_values_before_it_needs_a_device(kw):
    from yolo3.model import YoloV3
    with pytest.raises(ValueError):
        YoloV3(2, [64, 64, 3], 2, **kw)


def test_clip_scale_against_its_definition():
    from yolo3.model import clip_scale
    for k in (1, 2, 3, 7, 64):
        for c in (1e-3, 1.0, 10.0):
            for norm in (0.0, c / 3, c):                            # below or at the bound: only the 1/k of the average
                got = clip_scale(norm, c, k)
                assert type(got) is np.float32 and got == np.float32(1.0 / k), (k, c, norm)
            assert clip_scale(4 * c, c, k) == np.float32(0.25 / k), (k, c)
            for norm in (1.7 * c, 123.456 * c):                    # the fp64 formula, rounded once
                assert clip_scale(norm, c, k) == np.float32((1.0 / k) * (c / max(norm, c)))
        assert clip_scale(5.0, None, k) == np.float32(1.0 / k)      # clipping off
        seq = [float(clip_scale(n, 1.0, k)) for n in np.linspace(0.0, 50.0, 2001)]
        assert all(a >= b for a, b in zip(seq, seq[1:]))             # monotone non-increasing in the norm
        assert 0.0 < seq[-1] < seq[0]
    # the scaled norm never exceeds the bound by more than the rounding of the factor
    for norm in (1.0, 3.0, 1e4):
        assert float(clip_scale(norm, 2.0, 1)) * norm <= 2.0 * (1 + 2.0 ** -23)


def _parse(extra):
    import train
    return train.build_parser().parse_args(['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c'] + extra)


def test_train_parser_flags():
    a = _parse([])
    assert a.accumulate_steps == 1 and a.grad_clip_norm is None
    b = _parse(['--accumulate_steps', '8', '--grad_clip_norm', '10'])
    assert b.accumulate_steps == 8 and type(b.accumulate_steps) is int and b.grad_clip_norm == 10.0
    for bad in (['--accumulate_steps', '0'], ['--accumulate_steps', '-3'], ['--accumulate_steps', '1.5'], ['--accumulate_steps', 'nan'],
                ['--grad_clip_norm', '0'], ['--grad_clip_norm', '-1'], ['--grad_clip_norm', 'nan'], ['--grad_clip_norm', 'inf'],
                ['--grad_clip_norm', '-inf']):
        with pytest.raises(SystemExit):
            _parse(bad)
    # the flags that were there keep their names and defaults
    assert (a.batch_size, a.learning_rate, a.test_every_n_steps, a.use_augmentation, a.ema_decay, a.box_loss) == (8, 1e-4, 1000, 1, 0.0, 'mse')


def test_train_model_validates_before_it_opens_anything():
    import train
    for kw in (dict(accumulate_steps=0), dict(grad_clip_norm=-1.0), dict(grad_clip_norm=math.nan)):
        with pytest.raises(ValueError):
            train.train_model(2, 2, '/nonexistent/a', '/nonexistent/b', '/nonexistent/c', 1, 1e-4, False, **kw)
