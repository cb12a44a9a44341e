"""GPU tests of the opt-in optimisers: y3_optim_step bit for bit against the NumPy float32 restatement of its
rules (tests/optim_reference.py, which test_cpu_optim.py holds to fp64 yardsticks within derived bounds), its identities with the
Adam kernels, memory it must not touch, and the model, the captured graph, accumulation, clipping, the EMA, resume and train.py
on top of it.  Everything the optimiser computes is compared exactly: there is no tolerance to derive.  (The one inexact
comparison is of an INPUT: the clip scale the kernel read against its host restatement, within one fp32 ulp, because the order
of the device's fp64 sum of squares is not NumPy's; test_gpu_grad_accum.py pins that scale.)"""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
if os.path.join(ROOT, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tests'))

import optim_reference as R       # noqa: E402

F32 = np.float32
PAD = 8                                            # NaN canaries past `count` in every arena
PASS = 2048 * 256 * 4                              # floats one grid-stride pass of the full grid covers
BIG = 2 * PASS + 4 * 300 + 3                       # a second pass (and the start of a third) and a tail
COUNTS = [1, 3, 4, 5, 1023, 1028, BIG]
KINDS = [R.SGD, R.SGD_NESTEROV, R.ADAMW]
INSTANCES = [(k, e, s) for k in KINDS for e in (False, True) for s in (False, True)]
MU, WD = 0.9, 5e-4
# three steps, everything that lives in device memory changing: (lr or lr_t, lr * wd), 1 - decay, gradient scale
HYPER = [(1e-3, 5e-7), (7e-4, 3.5e-3), (2.5e-3, 1e-1)]
OMD = [0.5, 0.01, 0.25]
SCALE = [0.5, 0.3, 1.7]


def tables(count):
    """name -> range table for an arena of `count` floats: every table of the list that fits.  The arena of two passes takes the
    tables that need its size, the empty one and the one that ends in its tail; the others run at every smaller count."""
    c4 = count // 4 * 4
    t = {'empty': [], 'everything': [(0, count)]}
    if count % 4:
        t['ends at the odd count'] = [(c4, count)] if c4 else [(0, count)]
    if count > PASS + 16:
        del t['everything']        # (its last table below runs from inside the second pass to count)
        t['round the end of the first pass'] = [(PASS - 64, PASS - 4), (PASS + 4, PASS + 64), (2 * PASS - 8, 2 * PASS + 8), (2 * PASS + 1200, count)]
        t['across the first pass'] = [(0, 4), (PASS - 4, PASS + 4), (PASS + 256, 2 * PASS)]
        return t
    if count >= 8:
        t['begins at 0'] = [(0, 4)]
        t['touching'] = [(0, 4), (4, min(c4, 12))] if c4 >= 8 else [(0, 4)]
    if count >= 1020:
        t['128 of 4 with gaps of 4'] = [(8 * i, 8 * i + 4) for i in range(127)] + [(8 * 127, min(8 * 127 + 4, count))]
        t['inside a wavefront'] = [(40, 80), (280, 520), (520, 524), (760, 1016)]      # a wavefront spans 256 floats
        if count % 4:
            t['touching up to the odd count'] = [(512, 1000), (1000, count)]
    return t


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, pad=PAD):
    """a -> device arena with NaN canaries behind it"""
    t = torch.full((a.size + pad,), float('nan'), device='cuda')
    t[:a.size].copy_(torch.from_numpy(a))
    return t


def _host(t, n):
    h = t.cpu().numpy()
    assert np.isnan(h[n:]).all() and h.size == n + PAD, 'the canaries past count were written'
    return h[:n].copy()


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Run:
    """The arenas of one kernel test on the device, the same on the host, and one step of each."""

    def __init__(self, kind, ema, scaled, count, ranges, seed=0, mcount=37, wd=WD, mu=MU):
        from yolo3 import _hip
        rng = np.random.default_rng(seed + count)
        self.kind, self.ema, self.scaled, self.count, self.mcount, self.wd, self.mu = kind, ema, scaled, count, mcount, wd, mu
        self.D = R.mask_from_ranges(count, ranges)
        self.h = dict(p=(0.1 * rng.standard_normal(count)).astype(F32), m=(0.01 * rng.standard_normal(count)).astype(F32),
                      v=(1e-4 * rng.random(count)).astype(F32), e=(0.1 * rng.standard_normal(count)).astype(F32),
                      mv=rng.standard_normal(mcount).astype(F32), emv=rng.standard_normal(mcount).astype(F32))
        self.d = {k: _dev(a) for k, a in self.h.items()}
        self.g = None
        self.gd = torch.full((count + PAD,), float('nan'), device='cuda')
        self.hyper, self.omd, self.s = torch.zeros(2, device='cuda'), torch.zeros(1, device='cuda'), torch.zeros(1, device='cuda')
        self.table = (C.c_longlong * max(1, 2 * len(ranges)))(*[x for r in ranges for x in r])
        d = self.desc = _hip.OptimDesc()
        d.kind, d.count = kind, count
        d.param, d.grad, d.m = self.d['p'].data_ptr(), self.gd.data_ptr(), self.d['m'].data_ptr()
        d.v = self.d['v'].data_ptr() if kind == R.ADAMW else None
        d.hyper_dev, d.momentum, d.weight_decay = self.hyper.data_ptr(), mu, wd
        d.beta1, d.beta2, d.eps = R.B1, R.B2, R.EPS
        d.decay_ranges_host, d.n_ranges = self.table, len(ranges)
        if ema:
            d.ema_param, d.moving, d.ema_moving = self.d['e'].data_ptr(), self.d['mv'].data_ptr(), self.d['emv'].data_ptr()
            d.moving_count, d.omd_dev = mcount, self.omd.data_ptr()
        if scaled:
            d.scale_dev = self.s.data_ptr()

    def set(self, g, hyper, omd, s):
        self.g = g
        self.gd[:self.count].copy_(torch.from_numpy(g))
        self.hyper.copy_(torch.tensor([float(F32(hyper[0])), float(F32(hyper[1]))]))
        self.omd.fill_(float(F32(omd)))
        self.s.fill_(float(F32(s)))
        self.cur = (F32(hyper[0]), F32(hyper[1])), F32(omd), F32(s)

    def launch(self, stream=None):
        from yolo3._hip import lib, check
        check(lib.y3_optim_step(C.byref(self.desc), _stream() if stream is None else stream), 'y3_optim_step')

    def restate(self):
        hyper, omd, s = self.cur
        h = self.h
        with np.errstate(all='ignore'):
            p, m, v = R.step(self.kind, h['p'], h['m'], h['v'], self.g, hyper, self.D, self.mu, self.wd, s if self.scaled else None)
            if self.ema:
                h['e'] = R.ema_step(h['e'], p, omd)
                h['emv'] = R.ema_step(h['emv'], h['mv'], omd)
        h['p'], h['m'], h['v'] = p, m, v

    def device(self):
        torch.cuda.synchronize()
        out = {k: _host(t, self.mcount if k in ('mv', 'emv') else self.count) for k, t in self.d.items()}
        assert _same(_host(self.gd, self.count), self.g), 'the gradient was written'
        return out

    def check(self, what):
        got = self.device()
        for k in ('p', 'm', 'v', 'e', 'mv', 'emv'):       # v without AdamW, e / emv without the EMA: untouched
            assert _same(got[k], self.h[k]), (what, k, int(np.argmax(got[k].view(np.uint32) != self.h[k].view(np.uint32))))


def _grads(count, seed):
    rng = np.random.default_rng(1000 + seed + count)
    return [(sc * rng.standard_normal(count)).astype(F32) for sc in (1.0, 1e-2, 3.0)]


# ---- kernel: bit for bit against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, ema, scaled', INSTANCES)
def test_every_instantiation_matches_the_restatement_bit_for_bit(kind, ema, scaled):
    for count in COUNTS:
        gs = _grads(count, 0)
        for name, ranges in tables(count).items():
            run = Run(kind, ema, scaled, count, ranges, mcount=37 if count < BIG else 1027)
            for t in range(3):
                run.set(gs[t], HYPER[t], OMD[t], SCALE[t])
                run.launch()
                run.restate()
                run.check((count, name, t))
            assert run.D.any() == bool(ranges)


def test_tables_cover_the_cases():
    names = set()
    for count in COUNTS:
        for name, ranges in tables(count).items():
            names.add(name)
            assert len(ranges) <= 128 and all(b % 4 == 0 and b < e <= count and (e % 4 == 0 or e == count) for b, e in ranges), (count, name)
            assert all(e0 <= b1 for (_, e0), (b1, _) in zip(ranges, ranges[1:])), (count, name)
    assert len(names) == 10 and len(tables(1028)['128 of 4 with gaps of 4']) == 128
    assert BIG % 4 == 3 and BIG // 4 > 2 * 2048 * 256
    assert tables(BIG)['round the end of the first pass'][-1][1] == BIG and tables(1023)['touching up to the odd count'][-1][1] == 1023


# ---- identities with the Adam kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count', [5, 1023, PASS + 4 * 300 + 3])
def test_adamw_identities_with_the_adam_kernels(count):
    from yolo3._hip import lib, check
    gs = _grads(count, 1)
    ranges = [(0, count)]
    # no ranges == y3_adam_step; no ranges + EMA + scale == y3_adam_step_ema_scaled; lw = 0 with ranges == no ranges; s = 1 == unscaled
    plain, full = Run(R.ADAMW, False, False, count, []), Run(R.ADAMW, True, True, count, [])
    lw0, lw0_full = Run(R.ADAMW, False, False, count, ranges), Run(R.ADAMW, True, True, count, ranges)
    s1 = Run(R.ADAMW, False, True, count, [])
    ref, ref_full = Run(R.ADAMW, False, False, count, []), Run(R.ADAMW, True, True, count, [])
    for t in range(3):
        for r in (plain, full, ref, ref_full):
            r.set(gs[t], HYPER[t], OMD[t], SCALE[t])
        lw0.set(gs[t], (HYPER[t][0], 0.0), OMD[t], SCALE[t])
        lw0_full.set(gs[t], (HYPER[t][0], 0.0), OMD[t], SCALE[t])
        s1.set(gs[t], HYPER[t], OMD[t], 1.0)
        for r in (plain, full, lw0, lw0_full, s1):
            r.launch()
        d = ref.d
        check(lib.y3_adam_step(d['p'].data_ptr(), ref.gd.data_ptr(), d['m'].data_ptr(), d['v'].data_ptr(), count, ref.hyper.data_ptr(), R.B1, R.B2,
                               R.EPS, _stream()), 'y3_adam_step')
        d = ref_full.d
        check(lib.y3_adam_step_ema_scaled(d['p'].data_ptr(), ref_full.gd.data_ptr(), d['m'].data_ptr(), d['v'].data_ptr(), count,
                                          ref_full.hyper.data_ptr(), R.B1, R.B2, R.EPS, d['e'].data_ptr(), d['mv'].data_ptr(), d['emv'].data_ptr(),
                                          ref_full.mcount, ref_full.omd.data_ptr(), ref_full.s.data_ptr(), _stream()), 'y3_adam_step_ema_scaled')
        want, want_full = ref.device(), ref_full.device()
        for r, w in ((plain, want), (lw0, want), (s1, want), (full, want_full), (lw0_full, want_full)):
            got = r.device()
            for k in w:
                assert _same(got[k], w[k]), (t, k)


ADAM_ENTRIES = {(False, False): 'y3_adam_step', (False, True): 'y3_adam_step_scaled', (True, False): 'y3_adam_step_ema',
                (True, True): 'y3_adam_step_ema_scaled'}
# (count, moving_count): a tail alone, a body alone, both, a full grid-stride pass and a tail; with the EMA a grid sized by the moving
# statistics (their tail is the last block's), none of them (null pointers), them alone, and nothing at all
ADAM_SIZES = [(3, 37), (4, 37), (1023, 37), (PASS + 4 * 300 + 3, 37)]
ADAM_EMA_SIZES = [(6, 1027), (1023, 0), (0, 7), (0, 0)]


@pytest.mark.parametrize('ema, scaled', sorted(ADAM_ENTRIES))
def test_the_adam_entry_points_match_the_restatement_bit_for_bit(ema, scaled):
    """The four y3_adam_step* entry points themselves (the identities above compare them with y3_optim_step) against AdamW's
    restatement under an all-false decay mask, and the EMA's; lr_t in a tensor of ONE float, as the model passes it."""
    from yolo3._hip import lib, check
    name = ADAM_ENTRIES[ema, scaled]
    lr_t = torch.zeros(1, device='cuda')
    for count, mcount in ADAM_SIZES + (ADAM_EMA_SIZES if ema else [(0, 37)]):
        gs = _grads(count, 5)
        run = Run(R.ADAMW, ema, scaled, count, [], mcount=mcount)
        assert not run.D.any()
        d = run.d
        args = [d['p'].data_ptr(), run.gd.data_ptr(), d['m'].data_ptr(), d['v'].data_ptr(), count, lr_t.data_ptr(), R.B1, R.B2, R.EPS]
        if ema:
            args += [d['e'].data_ptr(), d['mv'].data_ptr() if mcount else None, d['emv'].data_ptr() if mcount else None, mcount, run.omd.data_ptr()]
        if scaled:
            args.append(run.s.data_ptr())
        for t in range(3):
            run.set(gs[t], HYPER[t], OMD[t], SCALE[t])
            lr_t.fill_(float(F32(HYPER[t][0])))
            check(getattr(lib, name)(*args, _stream()), name)
            run.restate()
            run.check((name, count, mcount, t))        # every arena, the ones this form leaves alone too, and the canaries past each


@pytest.mark.parametrize('kind', [R.SGD, R.SGD_NESTEROV])
def test_sgd_without_decay_or_with_unit_scale_gives_the_plain_bits(kind):
    count = 1023
    gs = _grads(count, 2)
    plain = Run(kind, False, False, count, [])
    wd0 = Run(kind, False, False, count, tables(count)['128 of 4 with gaps of 4'], wd=0.0)
    s1 = Run(kind, False, True, count, [])
    for t in range(3):
        for r in (plain, wd0, s1):
            r.set(gs[t], HYPER[t], OMD[t], 1.0)
            r.launch()
        want = plain.device()
        for r in (wd0, s1):
            got = r.device()
            assert all(_same(got[k], want[k]) for k in want), t


# ---- memory the kernel must not touch or mix -------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, ema, scaled', INSTANCES)
def test_nothing_leaks_across_a_range_boundary(kind, ema, scaled):
    """Non-finite values outside the ranges, finite ones inside: the decayed stretches come out finite and with the restatement's
    bits, so no lane took its neighbour's status or data.  (The canaries past count are checked by every read-back.)"""
    count = 1023
    ranges = [(40, 80), (280, 520), (520, 524), (1000, count)]
    run = Run(kind, ema, scaled, count, ranges, wd=0.05)
    D = run.D
    for k, bad in (('p', np.inf), ('m', -np.inf), ('v', np.inf), ('e', np.nan)):
        run.h[k][~D] = bad
        run.d[k][:count].copy_(torch.from_numpy(run.h[k]))
    g = _grads(count, 3)[0]
    g[~D] = np.nan
    run.set(g, HYPER[1], OMD[1], SCALE[1])
    run.launch()
    run.restate()
    got = run.device()
    for k in ('p', 'm') + (('v',) if kind == R.ADAMW else ()) + (('e',) if ema else ()):
        assert np.isfinite(got[k][D]).all() and not np.isfinite(got[k][~D]).any(), k
        assert _same(got[k][D], run.h[k][D]), k
        assert np.array_equal(np.isnan(got[k]), np.isnan(run.h[k])) and np.array_equal(got[k][~np.isnan(got[k])], run.h[k][~np.isnan(run.h[k])]), k


def test_same_bits_on_two_streams_and_on_repeated_launches():
    count = PASS + 4 * 300 + 3
    ranges = [(0, 4), (PASS - 4, PASS + 4), (PASS + 256, count)]
    side = torch.cuda.Stream()
    g = _grads(count, 4)[0]
    outs = []
    for kind, ema, scaled in ((R.SGD_NESTEROV, True, True), (R.ADAMW, True, True)):
        for rep in range(3):
            run = Run(kind, ema, scaled, count, ranges, mcount=1027)
            run.set(g, HYPER[0], OMD[0], SCALE[0])
            torch.cuda.synchronize()
            if rep == 2:
                with torch.cuda.stream(side):
                    run.launch(side.cuda_stream)
            else:
                run.launch()
            outs.append(run.device())
        a, b, c = outs[-3:]
        assert all(_same(a[k], b[k]) and _same(a[k], c[k]) for k in a), kind
        run.restate()
        assert all(_same(c[k], run.h[k]) for k in c)


# ---- model -------------------------------------------------------------------------------------------------------------------------
IMG, N, LR = 64, 2, 1e-3
MODELS = [dict(optimizer='sgd'), dict(optimizer='sgd', nesterov=True), dict(optimizer='adamw')]
IDS = ['sgd', 'sgd-nesterov', 'adamw']


@pytest.fixture(scope='module')
def case():
    from dp_worker import make_case
    anchors, K, params, images, gts = make_case(IMG, 2 * N, 31)
    return anchors, K, params, images.cuda(), [torch.from_numpy(x).cuda() for x in gts]


def _model(case, **kw):
    from yolo3.model import YoloV3
    anchors, K, params, _, _ = case
    kw.setdefault('weight_decay', WD if kw.get('optimizer', 'adam') != 'adam' else 0.0)
    y = YoloV3(N, [IMG, IMG, 3], K, anchors, learning_rate=LR, **kw)
    y.set_weights(params)
    return y


def _batch(case, j=0):
    sl = slice(j * N, (j + 1) * N)
    return case[3][sl], [x[sl] for x in case[4]]


def _np(t):
    return t.detach().cpu().numpy().copy()


def _kind(y):
    return R.ADAMW if y.optimizer_kind == 'adamw' else R.SGD_NESTEROV if y.nesterov else R.SGD


def _hyper(y, t):
    """The device pair of optimiser step t, from the rules: fp64, rounded once."""
    lr = y.learning_rate * (y.lr_schedule.factor(t) if y.lr_schedule is not None else 1.0)
    return R.adamw_hyper(lr, y.weight_decay, t) if y.optimizer_kind == 'adamw' else (F32(lr), F32(0.0))


def _state(y):
    z = np.zeros(y.arena_floats, F32)
    return _np(y.params), _np(y.adam_m), _np(y.adam_v) if y.adam_v is not None else z


def _expect_step(y, before, g, t, s=None):
    hyper = _hyper(y, t)
    assert _same(_np(y.hyper_dev), np.asarray(hyper, F32))
    D = R.mask_from_specs(y.specs, y.arena_floats)
    want = R.step(_kind(y), *before, g, hyper, D, y.momentum, y.weight_decay, s)
    got = _state(y)
    for name, a, b in zip(('params', 'adam_m', 'adam_v'), got, want):
        assert _same(a, b), name
    return want


@pytest.mark.parametrize('kw', MODELS, ids=IDS)
def test_one_train_step_is_the_restatement_on_the_models_own_gradients(case, kw):
    y = _model(case, **kw)
    assert (y.adam_v is None) == (kw['optimizer'] == 'sgd')                       # SGD has no second-moment arena
    assert len(y.decay_ranges) == len(y.specs) == 75 and y._adam_call[0].__name__ == 'y3_optim_step'
    before = _state(y)
    for t in (1, 2):
        y.train_step(_batch(case))
        torch.cuda.synchronize()
        want = _expect_step(y, before, _np(y.grads), t)
        assert not np.array_equal(want[0], before[0]) and y.iterations == t
        before = want
    # alignment padding stays zero
    used = np.zeros(y.arena_floats, bool)
    for sp in y.specs:
        used[sp.w_off:sp.w_off + sp.k * sp.k * sp.cin_pad * sp.cout] = True
        for off in [sp.b_off] + ([sp.g_off, sp.be_off] if sp.bn else []):
            used[off:off + sp.cout] = True
    assert (~used).any()
    for a in _state(y):
        assert not a[~used].any()
    assert y.current_learning_rate() == LR and y.get_learning_rate() == LR


def test_the_default_model_launches_the_adam_kernel_with_todays_arguments(case):
    from yolo3._hip import lib
    y = _model(case)
    fn, args = y._adam_call
    assert fn.__name__ == 'y3_adam_step' and y.optimizer_kind == 'adam' and y.adam_v is not None
    assert args == (y.params.data_ptr(), y.grads.data_ptr(), y.adam_m.data_ptr(), y.adam_v.data_ptr(), y.arena_floats, y.lr_t_dev.data_ptr(),
                    y.beta1, y.beta2, y.adam_eps)
    assert _model(case, ema_decay=0.9)._adam_call[0].__name__ == 'y3_adam_step_ema'
    assert _model(case, ema_decay=0.9, accumulate_steps=2)._adam_call[0].__name__ == 'y3_adam_step_ema_scaled'
    assert not hasattr(y, '_optim_desc') and lib.y3_optim_step is not None
    with pytest.raises(ValueError):
        _model(case, weight_decay=5e-4)                                           # 'adam' takes no decay: 'adamw'


def test_a_schedule_drives_the_default_adam_too(case):
    from yolo3.schedule import LrSchedule
    sched = LrSchedule('cosine', warmup_steps=1, warmup_start_factor=0.5, total_steps=4)
    y = _model(case, lr_schedule=sched)
    assert y._adam_call[0].__name__ == 'y3_adam_step'
    for t in (1, 2, 3):
        y.train_step(_batch(case))
        assert y.current_learning_rate() == LR * sched.factor(t)
        assert _same(_np(y.lr_t_dev), np.asarray([R.adamw_hyper(LR * sched.factor(t), 0.0, t)[0]], F32))
    y.set_learning_rate(2 * LR)                                                    # sets the base rate
    assert y.current_learning_rate() == 2 * LR * sched.factor(3)


@pytest.mark.parametrize('kw', MODELS, ids=IDS)
def test_graph_replay_equals_the_eager_step_under_a_cosine_schedule(case, kw):
    from yolo3.schedule import LrSchedule
    sched = LrSchedule('cosine', warmup_steps=1, warmup_start_factor=0.5, total_steps=5)
    host, graph = _model(case, lr_schedule=sched, **kw), _model(case, lr_schedule=sched, use_graph=True, **kw)
    seen = set()
    for t in range(1, 4):
        a, b = float(host.train_step(_batch(case, t % 2))), float(graph.train_step(_batch(case, t % 2)))
        torch.cuda.synchronize()
        assert a == b, t
        for name in ('params', 'adam_m', 'moving', 'grads', 'params_t', 'hyper_dev') + (('adam_v',) if host.adam_v is not None else ()):
            assert torch.equal(getattr(host, name), getattr(graph, name)), (t, name)
        assert _same(_np(graph.hyper_dev), np.asarray(_hyper(graph, t), F32))
        seen.add(float(graph.hyper_dev[0]))
    assert len(seen) == 3 and graph._plan(N, True).graph is not None                # the rate changed every step, one graph served them


@pytest.mark.parametrize('kw', MODELS, ids=IDS)
def test_accumulation_clipping_and_ema_against_the_restatement(case, kw):
    from yolo3.model import clip_scale, ema_one_minus_decay
    probe = _model(case, grad_clip_norm=1e30, **kw)
    probe.train_step(_batch(case))
    c = 0.01 * float(probe.last_grad_norm)                                         # bites
    y = _model(case, accumulate_steps=2, grad_clip_norm=c, ema_decay=0.99, ema_warmup=4, **kw)
    before, e_p, e_m = _state(y), _np(y.params), _np(y.moving)
    for t in (1, 2):
        y.train_step(_batch(case, 0))
        torch.cuda.synchronize()
        assert y.micro_step == 1 and y.iterations == t - 1
        assert all(_same(a, b) for a, b in zip(_state(y), before)) and _same(_np(y.ema_params), e_p)      # a micro-step updates nothing
        y.train_step(_batch(case, 1))
        torch.cuda.synchronize()
        acc = _np(y.grad_acc)
        # the scale the kernel read (pinned to clip_scale bit for bit in test_gpu_grad_accum.py; the order of the device's fp64 sum
        # may move its last bit against NumPy's here)
        s, s_host = _np(y.grad_scale_dev), clip_scale(float(np.sqrt(np.sum(acc.astype(np.float64) ** 2)) / 2), c, 2)
        assert abs(float(s) - float(s_host)) <= 2.0 ** -23 * float(s_host) and s < 0.5
        before = _expect_step(y, before, acc, t, s)
        omd = ema_one_minus_decay(0.99, 4, t)
        e_p, e_m = R.ema_step(e_p, before[0], omd), R.ema_step(e_m, _np(y.moving), omd)
        assert _same(_np(y.ema_params), e_p) and _same(_np(y.ema_moving), e_m), t


@pytest.mark.parametrize('kw', MODELS, ids=IDS)
def test_resume_continues_the_uninterrupted_run_bit_for_bit(case, kw, tmp_path):
    from yolo3.model import YoloV3
    from yolo3.schedule import LrSchedule
    sched = LrSchedule('cosine', warmup_steps=2, total_steps=6)
    path = os.path.join(str(tmp_path), 'w.npz')
    a = _model(case, lr_schedule=sched, **kw)
    for t in range(2):
        a.train_step(_batch(case, t))
    a.save_weights(path)
    z = np.load(path)
    assert str(z['meta_optimizer']) == kw['optimizer'] and ('opt_v' in z) == (kw['optimizer'] != 'sgd')
    a.train_step(_batch(case, 0))
    b = YoloV3.from_file(path, lr_schedule=sched)
    assert (b.optimizer_kind, b.nesterov, b.momentum, b.weight_decay) == (a.optimizer_kind, a.nesterov, a.momentum, a.weight_decay)
    assert b.iterations == 0
    b.load_weights(path, load_optimizer=True)
    assert b.iterations == 2 and b.current_learning_rate() == LR * sched.factor(2)
    b.train_step(_batch(case, 0))
    torch.cuda.synchronize()
    for name in ('params', 'adam_m', 'moving', 'hyper_dev') + (('adam_v',) if a.adam_v is not None else ()):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.current_learning_rate() == b.current_learning_rate() == LR * sched.factor(3)
    # across kinds: the weights load, the optimiser state does not
    other = _model(case, **(MODELS[2] if kw['optimizer'] == 'sgd' else MODELS[0]))
    other.load_weights(path)
    with pytest.raises(ValueError):
        other.load_weights(path, load_optimizer=True)
    with pytest.raises(ValueError):
        _model(case).load_weights(path, load_optimizer=True)


def test_a_default_models_file_has_no_optimizer_entry_and_loads_as_adam(case, tmp_path):
    from yolo3.model import YoloV3
    path = os.path.join(str(tmp_path), 'd.npz')
    y = _model(case)
    y.train_step(_batch(case))
    y.save_weights(path)
    z = np.load(path)
    assert 'meta_optimizer' not in z and 'meta_optimizer_args' not in z and 'opt_v' in z and 'opt_m' in z
    b = YoloV3.from_file(path)
    assert b.optimizer_kind == 'adam' and b._adam_call[0].__name__ == 'y3_adam_step'
    b.load_weights(path, load_optimizer=True)
    assert torch.equal(b.adam_v, y.adam_v) and b.iterations == 1
    with pytest.raises(ValueError):
        _model(case, optimizer='sgd').load_weights(path, load_optimizer=True)


def test_spp_model_has_76_ranges_and_its_step_matches(case):
    from yolo3.model import YoloV3
    # (the case's weights are the plain network's 75 layers: this one starts from its own seeded initialisation)
    y = YoloV3(N, [IMG, IMG, 3], case[1], case[0], learning_rate=LR, seed=5, optimizer='sgd', weight_decay=WD, spp=True)
    assert len(y.decay_ranges) == len(y.specs) == 76 and y._optim_desc.n_ranges == 76
    before = _state(y)
    y.train_step(_batch(case))
    torch.cuda.synchronize()
    _expect_step(y, before, _np(y.grads), 1)


def test_twenty_sgd_steps_on_one_batch_lower_the_loss(case):
    y = _model(case, optimizer='sgd')
    losses = [float(y.train_step(_batch(case))) for _ in range(20)]
    print('loss %.6f -> %.6f' % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


# ---- train.py ---------------------------------------------------------------------------------------------------------------------
def test_train_cli_with_sgd_and_a_cosine_schedule(tmp_path):
    from test_gpu_cli import _write_dataset
    from yolo3.model import YoloV3
    from yolo3.schedule import LrSchedule
    tmp = str(tmp_path)
    _write_dataset(tmp, 15, (160, 160, 3))
    out = os.path.join(tmp, 'out')
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    args = [os.path.join(PKG, 'train.py'), '--batch_size', '2', '--test_every_n_steps', '4', '--train_database', os.path.join(tmp, 'train-syn.lmdb'),
            '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out, '--early_stopping', '5', '--use_augmentation', '0',
            '--max_epochs', '1', '--reader_count', '1', '--learning_rate', '1e-3', '--optimizer', 'sgd', '--weight_decay', '5e-4',
            '--lr_schedule', 'cosine', '--lr_warmup_steps', '3', '--lr_total_steps', '8']
    r = subprocess.run(['timeout', '-k', '10', '900', sys.executable] + args, env=env, capture_output=True, text=True, timeout=960)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Performing Adam Optimizer learning rate warmup' not in r.stdout and r.stdout.count('Optimizer: sgd (momentum 0.9)') == 1
    scalars, = glob.glob(os.path.join(out, 'scalars-*'))
    train = open(os.path.join(scalars, 'train.csv')).read().splitlines()
    steps = len(train) - 1
    assert steps == 5                                                   # the full epoch size from epoch 0 on: steps 0 .. 4
    assert all(np.isfinite(float(v)) for ln in train[1:] for v in ln.split(',')[1:])
    test = open(os.path.join(scalars, 'test.csv')).read().splitlines()
    assert len(test) == 2 and all(np.isfinite(float(v)) for v in test[1].split(',')[1:])
    rows = open(os.path.join(scalars, 'lr.csv')).read().splitlines()
    assert rows[0] == 'step,lr' and len(rows) - 1 == steps
    sched = LrSchedule('cosine', warmup_steps=3, total_steps=8)
    for t, ln in enumerate(rows[1:], 1):
        step, lr = ln.split(',')
        assert int(step) == t and float(lr) == 1e-3 * sched.factor(t), ln
    y = YoloV3.from_file(os.path.join(out, 'saved_model', 'yolov3.npz'))
    assert y.optimizer_kind == 'sgd' and y.weight_decay == 5e-4 and y.momentum == 0.9 and not y.nesterov and y.adam_v is None
