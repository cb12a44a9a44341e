"""Host side of the exponential moving average of the weights: the decay ramp, the constructor's checks, the
fused Adam + EMA entry point's declaration and argument validation, and train.py's --ema_decay flag."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
sys.path.insert(0, PKG)


def test_ramp_values_and_single_fp32_rounding():
    from yolo3.model import ema_one_minus_decay
    for decay, warmup in ((0.9999, 2000), (0.99, 4), (0.5, 1.0)):
        for t in (1, warmup, 10 ** 6):
            got = ema_one_minus_decay(decay, warmup, t)
            assert type(got) is np.float32
            want64 = 1.0 - decay * (1.0 - math.exp(-t / warmup))
            assert got == np.float32(want64)                     # fp64 formula, rounded once
    # t = 1: almost no averaging yet; t = warmup: 1 - d (1 - 1/e); t -> inf: 1 - d
    assert ema_one_minus_decay(0.9999, 2000, 1) == np.float32(1.0 - 0.9999 * (1.0 - math.exp(-1 / 2000)))
    assert abs(float(ema_one_minus_decay(0.9999, 2000, 1)) - (1 - 0.9999 / 2000)) < 1e-6
    assert abs(float(ema_one_minus_decay(0.9999, 2000, 2000)) - (1 - 0.9999 * (1 - math.exp(-1)))) < 1e-7
    assert ema_one_minus_decay(0.9999, 2000, 10 ** 6) == np.float32(1.0 - 0.9999)
    # the ramp only moves one way
    seq = [float(ema_one_minus_decay(0.999, 100, t)) for t in range(1, 2000)]
    assert all(a >= b for a, b in zip(seq, seq[1:]))


@pytest.mark.parametrize('bad', [-0.5, 1.0, 1.5, float('nan'), True])
def test_invalid_decay_is_refused(bad):
    """Checked before the constructor needs a device, so it raises ValueError here too."""
    from yolo3.model import YoloV3
    with pytest.raises(ValueError):
        YoloV3(2, [64, 64, 3], 2, ema_decay=bad)


def test_invalid_warmup_is_refused():
    from yolo3.model import YoloV3
    for w in (0, -3):
        with pytest.raises(ValueError):
            YoloV3(2, [64, 64, 3], 2, ema_decay=0.99, ema_warmup=w)


def test_adam_ema_entry_point_declared_and_exported():
    from yolo3 import _hip
    hdr = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    assert 'int y3_adam_step_ema(' in hdr
    assert 'y3_adam_step_ema' in _hip.SIGNATURES
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), 'y3_adam_step_ema')
    assert len(_hip.SIGNATURES['y3_adam_step_ema'][1]) == len(_hip.SIGNATURES['y3_adam_step'][1]) + 5


def test_adam_ema_argument_validation_without_device():
    """Null or misaligned arenas are refused on the host before any launch, with a message."""
    from yolo3 import _hip
    lib = _hip.lib
    a = 1 << 20            # fake, 16-byte aligned addresses: validation fails before anything dereferences them
    ok = dict(p=a, g=2 * a, m=3 * a, v=4 * a, lr=5 * a, e=6 * a, mv=7 * a, em=8 * a, omd=9 * a)

    def call(**kw):
        d = dict(ok, **kw)
        return lib.y3_adam_step_ema(d['p'], d['g'], d['m'], d['v'], 1000, d['lr'], 0.9, 0.999, 1e-7, d['e'], d['mv'], d['em'], 37,
                                    d['omd'], None)

    for k in ('p', 'g', 'm', 'v', 'lr', 'e', 'omd'):
        assert call(**{k: None}) == -1, k
        assert b'null' in lib.y3_last_error(), k
    for k in ('mv', 'em'):
        assert call(**{k: None}) == -1, k
        assert b'null' in lib.y3_last_error(), k
    for k in ('p', 'g', 'm', 'v', 'e', 'mv', 'em'):
        assert call(**{k: ok[k] + 4}) == -1, k
        assert b'aligned' in lib.y3_last_error(), k
    # nothing to do: returns before launching
    assert lib.y3_adam_step_ema(a, a, a, a, 0, a, 0.9, 0.999, 1e-7, a, None, None, 0, a, None) == 0


def _parse(extra):
    import train
    return train.build_parser().parse_args(['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c'] + extra)


def test_train_parser_ema_flag():
    a = _parse([])
    assert a.ema_decay == 0.0
    assert _parse(['--ema_decay', '0.9999']).ema_decay == 0.9999
    # the flags that were there keep their names and defaults
    assert (a.batch_size, a.learning_rate, a.test_every_n_steps, a.use_augmentation, a.test_map, a.model_selection) == (8, 1e-4, 1000, 1, 0, 'loss')
    assert a.terminate_after_num_epochs_without_test_loss_improvement == 10 and a.test_map_min_box_size == 32
