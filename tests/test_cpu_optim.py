"""CPU-only tests of the opt-in optimisers and learning-rate schedules: schedule values at hand-computed points,
the NumPy float32 restatement of y3_optim_step's rules (tests/optim_reference.py, which the GPU tests hold the kernel to bit
for bit) against independent fp64 yardsticks, the library's refusals, the train.py flags and the model's decay-range table.

ERROR BOUNDS of the restatement tests.  U = 2^-24 is the unit roundoff of fp32.  Both sides start from the same fp32 numbers; the
fp64 yardstick gets the fp32-rounded hyper-parameters, so what separates the two is the fp32 roundings alone, plus, for AdamW,
the constants the fp32 form cannot hold: o1 = 1 - b1 and o2 = 1 - b2 formed in fp32 (1 - fl(0.999) is 1.3e-5 off 0.001), eps and
lr_t rounded to fp32.  The bound of an element is carried from step to step beside the fp64 values: every fp32 operation adds
U times the magnitude of its result (for an add: of the sum of the absolute operands), and an error that is already there
passes through each expression with the absolute value of its derivative.  SECOND covers the products of two such first-order
terms (each below 1e-4 relative here).  Nothing is taken from what the restatement gives."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
for _p in (PKG, os.path.join(ROOT, 'tests'), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import optim_reference as R       # noqa: E402

U = 2.0 ** -24
SECOND = 1.01
F32 = np.float32


# ---- schedule -------------------------------------------------------------------------------------------------------------------
def test_schedule_values_at_hand_computed_points():
    from yolo3.schedule import LrSchedule
    W, T, f, s = 4, 12, 0.01, 0.25
    c = LrSchedule('cosine', warmup_steps=W, warmup_start_factor=s, total_steps=T, final_factor=f)
    assert c.factor(1) == s + (1 - s) * 1 / 4 == 0.4375
    assert c.factor(W) == 1.0
    assert c.factor(W + 1) == f + (1 - f) * 0.5 * (1 + math.cos(math.pi / 8))
    assert abs(c.factor(W + 1) - 0.962320369) < 1e-9                    # 0.01 + 0.99 * 0.5 * (1 + 0.923879533), cos 22.5 deg
    assert abs(c.factor(8) - (f + (1 - f) * 0.5)) < 1e-15               # the mid-point: cos(pi / 2) = 0 -> 0.505
    assert abs(c.factor(8) - 0.505) < 1e-15
    assert abs(c.factor(T) - f) < 1e-15 and c.factor(T + 1) == c.factor(T) == c.factor(10 * T)     # holds at f
    # W = 0: no warm-up, the first step is already on the curve
    c0 = LrSchedule('cosine', total_steps=10, final_factor=0.0)
    assert c0.factor(1) == 0.5 * (1 + math.cos(math.pi * 0.1)) and abs(c0.factor(5) - 0.5) < 1e-15 and abs(c0.factor(10)) < 1e-15
    k = LrSchedule('constant')
    assert [k.factor(t) for t in (1, 2, 1000)] == [1.0, 1.0, 1.0]
    kw = LrSchedule('constant', warmup_steps=5)                         # s = 0: t / W
    assert [kw.factor(t) for t in (1, 2, 5, 6)] == [0.2, 0.4, 1.0, 1.0]
    st = LrSchedule('step', warmup_steps=2, milestones=(5, 9), gamma=0.1)
    assert [st.factor(t) for t in (1, 2, 3, 4)] == [0.5, 1.0, 1.0, 1.0]
    assert st.factor(4) == 1.0 and st.factor(5) == 0.1                  # each side of every milestone
    assert st.factor(8) == 0.1 and st.factor(9) == 0.1 ** 2 and st.factor(10 ** 6) == 0.1 ** 2
    s0 = LrSchedule('step', milestones=(1,), gamma=0.5)
    assert s0.factor(1) == 0.5
    assert LrSchedule('step').factor(7) == 1.0


def test_schedule_is_monotone_inside_the_warmup_and_cosine_never_rises():
    from yolo3.schedule import LrSchedule
    for s in (0.0, 0.1, 1.0):
        c = LrSchedule('cosine', warmup_steps=50, warmup_start_factor=s, total_steps=200)
        v = [c.factor(t) for t in range(1, 260)]
        assert all(b >= a for a, b in zip(v[:50], v[1:50])) and v[49] == 1.0 and (s == 1.0 or v[0] > s)
        assert all(b <= a for a, b in zip(v[49:], v[50:])) and min(v[50:]) >= 0.01 - 1e-15
        assert all(isinstance(x, float) for x in v)


def test_schedule_rejects_bad_arguments():
    from yolo3.schedule import LrSchedule
    for kw in (dict(kind='linear'), dict(kind='cosine'), dict(kind='cosine', total_steps=5, warmup_steps=5),
               dict(kind='cosine', total_steps=4, warmup_steps=5), dict(kind='cosine', total_steps=10.5),
               dict(kind='cosine', total_steps=10, final_factor=-0.1), dict(kind='cosine', total_steps=10, final_factor=1.5),
               dict(kind='constant', warmup_steps=-1), dict(kind='constant', warmup_steps=1.5), dict(kind='constant', warmup_start_factor=-0.1),
               dict(kind='constant', warmup_start_factor=1.1), dict(kind='step', milestones=(5, 5)), dict(kind='step', milestones=(9, 5)),
               dict(kind='step', milestones=(0, 5)), dict(kind='step', milestones=(2,), gamma=0.0), dict(kind='step', milestones=(2,), gamma=float('inf'))):
        with pytest.raises(ValueError):
            LrSchedule(**kw)
    c = LrSchedule('constant')
    for t in (0, -1, 1.5):
        with pytest.raises(ValueError):
            c.factor(t)


# ---- the restatement against fp64 -------------------------------------------------------------------------------------------------
COUNT = 4096
LRS = (1e-3, 7e-4, 2e-3)
MU, WD = 0.9, 5e-4


def _data(seed):
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(COUNT)).astype(np.float32)
    gs = [(sc * rng.standard_normal(COUNT)).astype(np.float32) for sc in (1.0, 1e-2, 3.0)]
    D = R.mask_from_ranges(COUNT, [(0, 512), (1024, 1028), (2048, 4000)])          # mixed: decayed and undecayed stretches
    assert 0 < D.sum() < COUNT
    return p, gs, D


def _report(tag, err, bound):
    ratio = float(np.max(err / bound))
    print('%s: worst |fp32 - fp64| / bound = %.4f (max err %.3e)' % (tag, ratio, float(err.max())))
    return ratio


@pytest.mark.parametrize('nesterov', [False, True])
def test_sgd_restatement_against_torch_sgd_in_fp64(nesterov):
    p0, gs, D = _data(11)
    mu, wd = float(F32(MU)), float(F32(WD))
    # yardstick: torch.optim.SGD, fp64, two parameter groups
    tp = [torch.tensor(p0[D].astype(np.float64), requires_grad=True), torch.tensor(p0[~D].astype(np.float64), requires_grad=True)]
    opt = torch.optim.SGD([dict(params=[tp[0]], weight_decay=wd), dict(params=[tp[1]], weight_decay=0.0)], lr=1.0, momentum=mu,
                          dampening=0.0, nesterov=nesterov)
    p, m = p0.copy(), np.zeros(COUNT, np.float32)
    P, M = p0.astype(np.float64), np.zeros(COUNT)             # the fp64 mirror the bound's magnitudes come from
    e_p, e_m = np.zeros(COUNT), np.zeros(COUNT)
    for lr, g in zip(LRS, gs):
        lr = float(F32(lr))
        for grp in opt.param_groups:
            grp['lr'] = lr
        tp[0].grad, tp[1].grad = torch.tensor(g[D].astype(np.float64)), torch.tensor(g[~D].astype(np.float64))
        opt.step()
        p, m = R.sgd_step(p, m, g, lr, mu, wd, D, nesterov)
        G = g.astype(np.float64)
        dec = wd * P
        G1 = np.where(D, G + dec, G)
        e_g = np.where(D, wd * e_p + U * np.abs(dec) + U * (np.abs(G) + np.abs(dec)), 0.0)          # product, add
        Mn = mu * M + G1
        e_m = mu * e_m + e_g + U * np.abs(mu * M) + U * (np.abs(mu * M) + np.abs(G1))                # product, add
        M = Mn
        if nesterov:
            Uu = G1 + mu * M
            e_u = e_g + mu * e_m + U * np.abs(mu * M) + U * (np.abs(G1) + np.abs(mu * M))            # product, add
        else:
            Uu, e_u = M, e_m
        e_p = e_p + lr * e_u + U * np.abs(lr * Uu) + U * (np.abs(P) + np.abs(lr * Uu))               # product, subtract
        P = P - lr * Uu
    want = np.empty(COUNT)
    want[D], want[~D] = tp[0].detach().numpy(), tp[1].detach().numpy()
    want_m = np.empty(COUNT)
    want_m[D] = opt.state[tp[0]]['momentum_buffer'].numpy()
    want_m[~D] = opt.state[tp[1]]['momentum_buffer'].numpy()
    assert np.max(np.abs(P - want)) <= 1e-15 and np.max(np.abs(M - want_m)) <= 1e-13          # the mirror IS torch's SGD
    rp = _report('sgd%s p' % ('-nesterov' if nesterov else ''), np.abs(p - want), SECOND * e_p)
    rm = _report('sgd%s m' % ('-nesterov' if nesterov else ''), np.abs(m - want_m), SECOND * e_m)
    assert rp <= 1.0 and rm <= 1.0
    assert np.array_equal(R.sgd_step(p0, np.zeros_like(p0), gs[0], LRS[0], MU, 0.0, D)[0],
                          R.sgd_step(p0, np.zeros_like(p0), gs[0], LRS[0], MU, WD, np.zeros(COUNT, bool))[0])      # wd 0 = no mask


def test_adamw_restatement_against_the_oracle_adam_in_fp64():
    from oracle import model as om
    p0, gs, D = _data(12)
    wd = WD
    tp = torch.tensor(p0.astype(np.float64))
    adam = om.AdamState([tp], LRS[0])
    o1, o2, eps = float(F32(1) - F32(R.B1)), float(F32(1) - F32(R.B2)), float(F32(R.EPS))
    d_o1, d_o2, d_eps = abs(o1 - (1 - adam.b1)), abs(o2 - (1 - adam.b2)), abs(eps - adam.eps)
    p, m, v = p0.copy(), np.zeros(COUNT, np.float32), np.zeros(COUNT, np.float32)
    e_p, e_m, e_v = np.zeros(COUNT), np.zeros(COUNT), np.zeros(COUNT)
    for t, (lr, g) in enumerate(zip(LRS, gs), 1):
        lr_t, lw = R.adamw_hyper(lr, wd, t)
        lw64 = float(lw)
        P, M, V = tp.numpy().copy(), adam.m[0].numpy().copy(), adam.v[0].numpy().copy()          # fp64 state before the step
        # yardstick: the decay in fp64 on the decayed part, then the oracle's Keras Adam
        tp[torch.from_numpy(D)] -= lw64 * tp[torch.from_numpy(D)]
        adam.lr = lr
        adam.step([tp], [torch.tensor(g.astype(np.float64))])
        assert adam.t == t and abs(adam.lr_t() - float(lr_t)) <= U * adam.lr_t()
        p, m, v = R.adamw_step(p, m, v, g, lr_t, lw, D)
        # the bound, beside the fp64 values
        G = g.astype(np.float64)
        P1 = np.where(D, P - lw64 * P, P)
        e_p1 = e_p + np.where(D, lw64 * e_p + U * np.abs(lw64 * P) + U * (np.abs(P) + np.abs(lw64 * P)), 0.0)     # product, subtract
        dm = G - M
        Mn = M + dm * (1 - adam.b1)
        e_m = e_m * (1 + o1) + np.abs(dm) * d_o1 + U * np.abs(dm) + U * np.abs(dm * o1) + U * (np.abs(M) + np.abs(dm * o1))    # sub, mul, add
        dv = G * G - V
        Vn = V + dv * (1 - adam.b2)
        e_v = e_v * (1 + o2) + np.abs(dv) * d_o2 + o2 * U * G * G + U * np.abs(dv) + U * np.abs(dv * o2) + U * (np.abs(V) + np.abs(dv * o2))
        rt = np.sqrt(Vn)
        e_rt = np.where(rt > 0, np.minimum(e_v / np.maximum(rt, 1e-300), np.sqrt(e_v)), np.sqrt(e_v)) + U * rt       # |sqrt a - sqrt b| <= |a - b| / sqrt a
        den = rt + adam.eps
        e_den = e_rt + d_eps + U * den
        num = Mn * adam.lr_t()
        e_num = adam.lr_t() * e_m + 2 * U * np.abs(num)                                                              # lr_t in fp32, product
        assert np.all(e_den < 0.5 * den)
        q = num / den
        e_q = e_num / (den - e_den) + np.abs(num) * e_den / (den * (den - e_den)) + U * np.abs(q)
        e_p = e_p1 + e_q + U * (np.abs(P1) + np.abs(q))
        M, V = Mn, Vn
        assert np.max(np.abs((P1 - q) - tp.numpy())) <= 1e-15                                                         # the mirror IS the yardstick
    rp = _report('adamw p', np.abs(p - tp.numpy()), SECOND * e_p)
    rm = _report('adamw m', np.abs(m - adam.m[0].numpy()), SECOND * e_m)
    rv = _report('adamw v', np.abs(v - adam.v[0].numpy()), SECOND * e_v)
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0
    assert float(np.max(e_p)) < 1e-6          # the bound itself means something: three steps of 1e-3 move a weight by ~3e-3


def test_restatement_decays_only_inside_the_mask():
    p0, gs, D = _data(13)
    z = np.zeros(COUNT, np.float32)
    none = np.zeros(COUNT, bool)
    a = R.sgd_step(p0, z, gs[0], 1e-3, MU, WD, D)
    b = R.sgd_step(p0, z, gs[0], 1e-3, MU, WD, none)
    assert np.array_equal(a[0][~D], b[0][~D]) and not np.array_equal(a[0][D], b[0][D])
    lr_t, lw = R.adamw_hyper(1e-3, 0.05, 1)
    a = R.adamw_step(p0, z, z, gs[0], lr_t, lw, D)
    b = R.adamw_step(p0, z, z, gs[0], lr_t, lw, none)
    assert np.array_equal(a[0][~D], b[0][~D]) and not np.array_equal(a[0][D], b[0][D])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])            # decoupled: the moments never see the decay


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry():
    import re
    from yolo3 import _hip
    text = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    assert re.search(r'^int\s+y3_optim_step\s*\(const y3_optim_desc\* d, y3_stream_t stream\);', text, re.M)
    for name, val in (('Y3_OPT_SGD', 0), ('Y3_OPT_SGD_NESTEROV', 1), ('Y3_OPT_ADAMW', 2), ('Y3_OPT_MAX_RANGES', 128)):
        assert re.search(r'^#define %s %d$' % (name, val), text, re.M), name
    assert (_hip.OPT_SGD, _hip.OPT_SGD_NESTEROV, _hip.OPT_ADAMW, _hip.OPT_MAX_RANGES) == (0, 1, 2, 128)
    assert 'y3_optim_step' in _hip.SIGNATURES and hasattr(_hip.lib, 'y3_optim_step')
    # the ctypes struct has the header's members in the header's order
    body = re.search(r'typedef struct y3_optim_desc \{(.*?)\} y3_optim_desc;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', decl.strip())]
    assert names == [f[0] for f in _hip.OptimDesc._fields_], names
    n = len(re.findall(r'^(?:int|size_t|const char\*)\s+y3_\w+\s*\(', text, re.M))
    assert n == len(_hip.SIGNATURES) and '(%d extern "C" entry points' % n in open(os.path.join(ROOT, 'README.md')).read()


def _desc(**kw):
    """A descriptor whose every pointer is a small aligned integer: a launch would fault, so a clean return proves that the check
    came first."""
    import ctypes as C
    from yolo3 import _hip
    ranges = kw.pop('ranges', None)
    d = _hip.OptimDesc()
    d.kind, d.param, d.grad, d.m, d.v, d.count, d.hyper_dev = _hip.OPT_ADAMW, 64, 128, 192, 256, 1003, 320
    d.momentum, d.weight_decay, d.beta1, d.beta2, d.eps = 0.9, 5e-4, 0.9, 0.999, 1e-7
    for k, val in kw.items():
        setattr(d, k, val)
    if ranges is not None:
        d._keep = (C.c_longlong * max(1, 2 * len(ranges)))(*[x for r in ranges for x in r])
        d.decay_ranges_host = d._keep
        if 'n_ranges' not in kw:
            d.n_ranges = len(ranges)
    return d


def test_library_rejects_bad_arguments_before_launch():
    """Bad arguments are rejected on the host before any launch, with a message."""
    import ctypes as C
    from yolo3 import _hip
    lib = _hip.lib

    def bad(word, **kw):
        d = _desc(**kw)
        assert lib.y3_optim_step(C.byref(d), None) == -1, kw
        assert word in lib.y3_last_error(), (kw, lib.y3_last_error())

    assert lib.y3_optim_step(None, None) == -1 and b'null' in lib.y3_last_error()
    for name in ('param', 'grad', 'm', 'hyper_dev'):
        bad(b'null', **{name: None})
    bad(b'null', v=None)                                        # AdamW without v
    bad(b'AdamW', v=None)
    for name in ('param', 'grad', 'm', 'v'):
        bad(b'aligned', **{name: 68})
    bad(b'aligned', ema_param=68, omd_dev=64)
    bad(b'aligned', ema_param=64, omd_dev=64, moving=72, ema_moving=64, moving_count=8)
    for kind in (-1, 3, 99):
        bad(b'kind', kind=kind)
    for mu in (-0.1, 1.0, 1.5, float('nan'), float('inf')):
        bad(b'momentum', momentum=mu, kind=_hip.OPT_SGD, v=None)
    for wd in (-1e-6, -1.0, float('nan')):
        bad(b'weight_decay', weight_decay=wd, kind=_hip.OPT_SGD, v=None)
    for n in (-1, 129, 1000):
        bad(b'n_ranges', n_ranges=n, ranges=[(0, 4)])
    bad(b'null', n_ranges=2)                                    # ranges announced, no table
    # the range rules
    bad(b'sorted', ranges=[(8, 16), (0, 4)])
    bad(b'overlaps', ranges=[(0, 16), (8, 24)])
    bad(b'multiple of 4', ranges=[(2, 8)])
    bad(b'multiple of 4', ranges=[(0, 6)])
    bad(b'multiple of 4', ranges=[(0, 1002)])                   # not a multiple of 4 and not count
    bad(b'beyond count', ranges=[(0, 1004)])
    bad(b'beyond count', ranges=[(1000, 1008)])
    bad(b'empty', ranges=[(8, 8)])
    bad(b'empty', ranges=[(16, 8)])
    bad(b'empty', ranges=[(-4, 8)])
    # a partial set of EMA pointers
    bad(b'EMA', ema_param=64)
    bad(b'EMA', omd_dev=64)
    bad(b'EMA', ema_param=64, omd_dev=64, moving_count=8)
    bad(b'EMA', ema_param=64, omd_dev=64, moving_count=8, moving=64)
    bad(b'EMA', moving=64, ema_moving=64, moving_count=8)
    bad(b'EMA', moving_count=8)
    # count == 0: OK, nothing launched -- after the checks, which a bad argument still fails
    for kind in (_hip.OPT_SGD, _hip.OPT_SGD_NESTEROV, _hip.OPT_ADAMW):
        assert lib.y3_optim_step(C.byref(_desc(kind=kind, count=0)), None) == 0
    assert lib.y3_optim_step(C.byref(_desc(count=0, scale_dev=64, ema_param=64, omd_dev=64)), None) == 0
    bad(b'momentum', count=0, momentum=1.0)
    bad(b'beyond count', count=0, ranges=[(0, 4)])
    assert lib.y3_optim_step(C.byref(_desc(kind=_hip.OPT_SGD, v=None, count=0, ranges=[])), None) == 0
    # tables within the rules pass the range checks: the momentum check, which comes after them, is what refuses these (touching
    # ranges, a range from 0, one ending at the odd count, 128 ranges) -- and one range too many is refused for that
    for ranges in ([(0, 8), (8, 16)], [(0, 1003)], [(1000, 1003)], [(0, 4), (1000, 1003)], [(8 * i, 8 * i + 4) for i in range(125)]):
        bad(b'momentum', ranges=ranges, momentum=2.0)
    bad(b'momentum', count=2000, ranges=[(8 * i, 8 * i + 4) for i in range(128)], momentum=2.0)
    bad(b'n_ranges', count=2000, ranges=[(8 * i, 8 * i + 4) for i in range(129)], momentum=2.0)


# ---- train.py ---------------------------------------------------------------------------------------------------------------------
def test_train_parser_defaults_and_validators():
    import train
    parser = train.build_parser()
    base = ['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c']
    a = parser.parse_args(base)
    assert (a.optimizer, a.lr_schedule, a.weight_decay, a.momentum, a.nesterov) == ('adam', 'reference', 0.0, 0.9, 0)
    assert (a.lr_warmup_steps, a.lr_warmup_start_factor, a.lr_total_steps, a.lr_final_factor, a.lr_milestones, a.lr_gamma) == (0, 0.0, None, 0.01, [], 0.1)
    a = parser.parse_args(base + ['--optimizer', 'sgd', '--learning_rate', '1e-3', '--weight_decay', '5e-4', '--lr_schedule', 'cosine',
                                  '--lr_warmup_steps', '1000', '--lr_total_steps', '100000', '--nesterov', '1', '--momentum', '0.937'])
    assert (a.optimizer, a.weight_decay, a.lr_schedule, a.lr_warmup_steps, a.lr_total_steps, a.nesterov, a.momentum) == \
        ('sgd', 5e-4, 'cosine', 1000, 100000, 1, 0.937)
    a = parser.parse_args(base + ['--optimizer', 'adamw', '--weight_decay', '0.05', '--lr_schedule', 'step', '--lr_milestones', '10', '20', '--lr_gamma', '0.5'])
    assert a.lr_milestones == [10, 20] and a.lr_gamma == 0.5
    for bad in (['--optimizer', 'lamb'], ['--momentum', '1.0'], ['--momentum', '-0.1'], ['--momentum', 'x'], ['--weight_decay', '-1'],
                ['--weight_decay', 'inf'], ['--weight_decay', '5e-4'],                       # adam takes no decay
                ['--nesterov', '2'], ['--lr_schedule', 'linear'], ['--lr_schedule', 'cosine'],  # cosine needs --lr_total_steps
                ['--lr_schedule', 'cosine', '--lr_total_steps', '5', '--lr_warmup_steps', '5'], ['--lr_warmup_steps', '3'],   # reference takes none
                ['--lr_total_steps', '10'], ['--lr_milestones', '5'], ['--lr_gamma', '0.5'], ['--lr_final_factor', '0.1'],
                ['--lr_schedule', 'step', '--lr_milestones', '9', '5'], ['--lr_schedule', 'step', '--lr_milestones', '0'],
                ['--lr_schedule', 'step', '--lr_gamma', '0'], ['--lr_schedule', 'constant', '--lr_warmup_steps', '-1'],
                ['--lr_schedule', 'constant', '--lr_warmup_start_factor', '1.5'], ['--lr_schedule', 'cosine', '--lr_total_steps', '10', '--lr_final_factor', '2']):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    assert train.build_lr_schedule() is None
    s = train.build_lr_schedule('cosine', 3, 0.0, 8)
    assert s.factor(3) == 1.0 and abs(s.factor(8) - 0.01) < 1e-15
    for kw in (dict(optimizer='lamb'), dict(weight_decay=5e-4), dict(optimizer='sgd', momentum=1.0), dict(optimizer='sgd', weight_decay=-1.0),
               dict(lr_schedule='cosine'), dict(lr_warmup_steps=3), dict(optimizer='sgd', nesterov=2)):
        with pytest.raises(ValueError):      # checked before any reader or device is set up
            train.train_model(2, 3, 'a', 'b', 'c', 1, 1e-4, False, **kw)


# ---- the model's range table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spp, layers', [(False, 75), (True, 76)])
def test_decay_ranges_cover_the_kernels_only(spp, layers):
    from yolo3 import _hip
    from yolo3.model import build_layer_specs, decay_ranges
    specs, arena, _, _ = build_layer_specs(3, 2, 2, spp)
    ranges = decay_ranges(specs)
    assert len(ranges) == len(specs) == layers <= _hip.OPT_MAX_RANGES
    assert all(b % 4 == 0 and e % 4 == 0 and 0 <= b < e <= arena for b, e in ranges)
    assert all(e0 <= b1 for (_, e0), (b1, _) in zip(ranges, ranges[1:]))                  # sorted, disjoint
    D = R.mask_from_ranges(arena, ranges)
    assert np.array_equal(D, R.mask_from_specs(specs, arena))
    for sp in specs:
        assert D[sp.w_off:sp.w_off + sp.k * sp.k * sp.cin_pad * sp.cout].all()
        for off in [sp.b_off] + ([sp.g_off, sp.be_off] if sp.bn else []):
            assert not D[off:off + sp.cout].any() and not any(b <= off < e for b, e in ranges)
    assert D.sum() == sum(sp.k * sp.k * sp.cin_pad * sp.cout for sp in specs)
    # the library takes the table as it stands (count 0 would refuse it: the real count, and a null arena refused AFTER the ranges passed)
    import ctypes as C
    d = _desc(kind=_hip.OPT_SGD, v=None, count=arena, ranges=ranges, momentum=2.0)
    assert _hip.lib.y3_optim_step(C.byref(d), None) == -1 and b'momentum' in _hip.lib.y3_last_error()


def test_model_checks_the_optimizer_arguments_before_the_device():
    from yolo3.model import check_optimizer_args
    check_optimizer_args()
    check_optimizer_args('sgd', 0.9, True, 5e-4, None)
    check_optimizer_args('adamw', 0.0, False, 0.05, type('S', (), {'factor': lambda self, t: 1.0})())
    for args in (('rmsprop',), ('adam', 0.9, False, 5e-4), ('sgd', 1.0), ('sgd', -0.1), ('sgd', 'x'), ('sgd', 0.9, 2), ('sgd', 0.9, False, -1e-3),
                 ('sgd', 0.9, False, float('inf')), ('sgd', 0.9, False, True), ('sgd', 0.9, False, 0.0, object())):
        with pytest.raises(ValueError):
            check_optimizer_args(*args)
    with pytest.raises(ValueError) as e:
        check_optimizer_args('adam', 0.9, False, 5e-4)
    assert 'adamw' in str(e.value)
