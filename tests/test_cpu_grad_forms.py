"""The generated lists of gradient-form representatives (tests/grad_forms.py) that test_gpu_grad_forms.py runs: they must not silently
shrink, and their data must make a border or run-boundary bug visible.  Host only: the plan queries launch nothing.  Run with -s to
see the counts the README quotes.

Found at this commit (printed by the tests below; the floors are these counts rounded down to a multiple of 5):
    wgrad    760 envelope launches, 75 classes  -> floor 75;  dgrad2   180 envelope launches, 22 classes  -> floor 20
    longest pixel run of the kernel gradient in the envelope, and among the representatives: f32 2016, x3 2016, of a pixel table
    (Y3_WG_TABLE, out8[7] of y3_conv2d_wgrad_plan_x) of 2048."""
import os

import pytest
import torch

import grad_forms as gf
import plan_forms as pf

pytestmark = pytest.mark.skipif(bool(os.environ.get('Y3_NO_FAST')), reason='Y3_NO_FAST=1 changes the data-gradient classes')

CLASS_FLOOR = {'wgrad': 75, 'dgrad2': 20}
WGRAD_TOL, DGRAD_TOL = 5e-5, 2e-5      # the bounds of test_gpu_grad_forms.py


def _param_list(fn, name):
    return [m.args[1] for m in fn.pytestmark if m.name == 'parametrize' and m.args[0] == name][0]


def test_dgrad_plan_query_agrees_with_the_older_queries():
    """y3_conv2d_dgrad_plan_x: stride 1 answers what y3_conv2d_plan_x answers; the rows are y3_conv2d_dgrad_bn_tiles_x; the bytes are
    y3_conv2d_dgrad_workspace_x for every launch but the merged f32 one (which needs none: the older query keeps a loose bound)."""
    from yolo3 import _hip
    for shape in pf.layer_shapes((1, 8), (320, 416)) + gf.OFF_NETWORK:
        n, h, w, cin, cout, k, s = shape
        if cin == 4:
            continue
        dd, ds = _hip.Tensor(0, n, -(-h // s), -(-w // s), cout, gf.src_ld(cout)), _hip.Tensor(0, n, h, w, cin, gf.dst_ld(cin))
        for flags in (0, _hip.CONV_X3):
            if flags and not _hip.lib.y3_conv2d_dgrad_x3_ok(dd, k, s, ds):
                continue
            how, rows, cls, ws = gf.dgrad_plan(shape, flags)
            assert rows == _hip.lib.y3_conv2d_dgrad_bn_tiles_x(dd, k, s, ds, flags), shape
            if s == 1:
                p, pws = pf.plan(n * h * w, cout, k, cin, flags)
                assert how == 'single' and len(cls) == 1 and gf._class_plan13(cls[0])[:9] == p[:9] and (cls[0]['fast'], cls[0]['nk']) == (p[11], p[12]), shape
                assert cls[0]['taps'] == k * k and cls[0]['m'] == n * h * w and ws == pws, shape
            else:
                assert how in ('merged-f32', 'merged-x3') and [c['taps'] for c in cls] == [4, 2, 2, 1], shape
                assert sum(c['m'] for c in cls) == n * h * w and rows == sum(-(-c['m'] // c['bm']) for c in cls), shape
                assert (ws == 0) == all(c['s0'] == 1 for c in cls), shape
                if how == 'merged-x3':
                    assert ws == _hip.lib.y3_conv2d_dgrad_workspace_x(dd, k, s, ds, flags), shape
                else:
                    assert ws == 0
    o = (gf.C.c_int * 51)()
    assert _hip.lib.y3_conv2d_dgrad_plan_x(_hip.Tensor(0, 1, 8, 8, 64, 64), 3, 2, _hip.Tensor(0, 1, 13, 13, 64, 64), 0, o) == 0 and o[0] == -1      # geometry mismatch


@pytest.mark.parametrize('entry', gf.ENTRIES)
def test_every_class_has_a_unique_representative_within_the_cap(entry, capsys):
    reps, left = gf.representatives(entry)
    again, left2 = gf.representatives(entry)
    assert [(s, mb.shape(), mb.arith) for s, mb in reps] == [(s, mb.shape(), mb.arith) for s, mb in again] and left == left2
    cls = gf.classes(entry)
    assert len(set(s for s, _ in reps)) == len(reps) and set(s for s, _ in reps) | set(left) == set(cls) and not set(left) & set(s for s, _ in reps)
    cases = gf.cases(entry)
    assert len(set(mb.id() for _, mb in cases)) == len(cases)
    layers = set(pf.layer_shapes())
    for sig, mb in reps:
        assert mb.signature() == sig and mb.within_cap(), mb
        assert mb.key() == cls[sig][0].key() or not cls[sig][0].within_cap(), 'not the cheapest member: %r' % mb
        assert mb.shape() in layers, 'not a layer of the network: %r' % mb
    off = gf.off_network(entry)
    for sig, mb in off:
        assert mb.signature() == sig and mb.within_cap() and mb.shape() in gf.OFF_NETWORK, mb
    if entry == 'dgrad2':
        # what the odd sizes are there for: unequal parity classes (signature bit), on both arithmetics and both x3 tiles
        assert cases[:len(reps)] == reps and len(off) == 4 and not any(s[10] for s in cls)
        assert set(s[1] for s, _ in off if s[10]) == set(gf.ARITHS) and set(s[4] for s, _ in off if s[1] == 'x3') == {64, 128}
    for sig in left:
        assert not any(mb.within_cap() for mb in cls[sig]), gf.sig_id(sig)
    assert len(left) <= gf.MAX_LEFT_OUT * len(cls), [gf.sig_id(s) for s in left]
    assert len(cls) >= CLASS_FLOOR[entry], 'the envelope lost classes: %d' % len(cls)
    with capsys.disabled():
        print('\n%s forms: %d envelope launches, %d classes, %d representatives (+ %d off the network; %.0f GFLOP of fp64 reference, largest %.1f), left out: %s'
              % (entry, len(gf.envelope(entry)), len(cls), len(reps), len(off), sum(mb.ref_flop() for _, mb in reps) / 1e9,
                 max(mb.ref_flop() for _, mb in reps) / 1e9, [gf.sig_id(s) for s in left] or 'none'))


def test_wgrad_representatives_reach_the_longest_run_every_tile_and_every_form(capsys):
    """Per arithmetic: the longest pixel run (`chunk`) among the representatives is the longest of the envelope -- that member runs
    the kernels' LDS pixel table nearly full --, and every f32 tile of y3_conv2d_wgrad_x's dispatch and every reduction form that
    occurs in the envelope occurs among the representatives.  Which (tile, form) pairs the planner cannot produce, and why:
    grad_forms' docstring; the pairs that do occur are printed."""
    reps, _ = gf.representatives('wgrad')
    lines = []
    for arith in gf.ARITHS:
        env = [mb.plan()[0] for mb in gf.envelope('wgrad') if mb.arith == arith]
        got = [mb.plan()[0] for s, mb in reps if s[1] == arith]
        table = set(p[7] for p in env)
        assert len(table) == 1
        table = table.pop()
        longest = max(p[3] for p in env)
        assert longest <= table and max(p[3] for p in got) == longest, (arith, longest, max(p[3] for p in got))
        assert longest > 0.95 * table, 'no launch of the envelope fills the pixel table any more: %d of %d' % (longest, table)
        assert set((p[0], p[1]) for p in got) == set((p[0], p[1]) for p in env), arith
        assert set(gf.wgrad_form(p) for p in got) == set(gf.wgrad_form(p) for p in env) == set(gf.WG_FORMS), arith
        pairs = sorted(set((p[0], p[1], gf.wgrad_form(p)) for p in env))
        assert set((p[0], p[1], gf.wgrad_form(p)) for p in got) == set(pairs), arith
        if arith == 'f32':
            assert set((p[0], p[1]) for p in env) == set(gf.F32_WG_TILES), 'a tile of the f32 dispatch no longer occurs in the envelope'
        else:
            assert set((p[0], p[1]) for p in env) == {(128, 128)}
        lines.append('wgrad %s: longest pixel run %d of a table of %d (Y3_WG_TABLE); tile x form: %s'
                     % (arith, longest, table, ', '.join('%dx%d %s' % p for p in pairs)))
    # the bits of the signature all occur: a ragged K tile / column tile / last run, the padded XCD grid, both strides, both kernel sizes
    sigs = [s for s, _ in reps]
    for arith in gf.ARITHS:
        mine = [s for s in sigs if s[1] == arith]
        assert all(any(s[i] for s in mine) and any(not s[i] for s in mine) for i in (7, 10)), arith
        assert any(s[9] for s in mine) and set(s[5] for s in mine) == {1, 3} and set(s[6] for s in mine) == {1, 2}, arith
    assert any(s[8] for s in sigs if s[1] == 'f32')      # cout % bn: the 14-channel heads (x3 wants cout >= 128, a power-of-two network: never ragged)
    with capsys.disabled():
        print('\n' + '\n'.join(lines))


def test_representatives_cover_the_training_size_wgrad_cases():
    """test_gpu_wgrad.CASES pin error and determinism at training size; every class they run is a class of the list here"""
    import test_gpu_wgrad as tw
    shapes = [(n, hw, hw, cin, cout, k, s) for n, hw, cin, cout, k, s in tw.CASES]
    theirs = gf.covered_by(shapes, 'wgrad')
    mine = set(s for s, _ in gf.representatives('wgrad')[0])
    assert theirs <= mine, sorted(gf.sig_id(s) for s in theirs - mine)
    # and the name of each reduction form is theirs
    assert len(tw.FORMS) == len(gf.WG_FORMS)
    for case in tw.CASES:
        n, hw, cin, cout, k, s, oh, m = tw._geom(case)
        p, _ = gf.wgrad_plan(m, cin, k, cout, 0)
        assert tw.FORMS.index(tw._form(p)) == gf.WG_FORMS.index(gf.wgrad_form(p))


def _older_coverage(entry):
    """the envelope classes the shape lists of the older GPU tests reach"""
    import test_gpu_kernels as tk
    import test_gpu_wgrad as tw
    app = [(1 if hw >= 104 else 2, hw, hw, cin, cout, k, s) for hw, cin, cout, k, s in tk.APP_A]      # test_conv_x3_error_against_fp64_...
    if entry == 'wgrad':
        shapes = [(n, hw, hw, cin, cout, k, s) for n, hw, cin, cout, k, s in tw.CASES] + list(_param_list(tk.test_conv_wgrad, 'case'))
    else:
        shapes = list(tk.DGRAD_CASES) + [tuple(s) for s in _param_list(tk.test_conv_dgrad_bn_epilogue_stats, 'shape') if len(s) > 6]
        shapes += [(8, hw, hw, cin, cout, k, s) for hw, cin, cout, k, s in tw.DGRAD_S2] + app
    got = gf.covered_by(shapes, entry)
    for side, n in ((96, 4), (416, 8), (320, 8)):          # the teacher-forced training steps, layer by layer
        got |= gf.step_classes(side, n, entry)
    return got & set(gf.classes(entry))


@pytest.mark.parametrize('entry', gf.ENTRIES)
def test_report_what_the_older_shape_lists_reach(entry, capsys):
    """Printed, not asserted: the figure README quotes."""
    cls = set(gf.classes(entry))
    old = _older_coverage(entry)
    with capsys.disabled():
        print('\n%s forms: the older GPU shape lists reach %d of %d envelope classes; reached by test_gpu_grad_forms.py alone: %s'
              % (entry, len(old), len(cls), ', '.join(sorted(gf.sig_id(s) for s in cls - old)) or 'none'))
    assert old <= cls


def _three_cheapest(entry):
    return sorted((mb for _, mb in gf.representatives(entry)[0]), key=gf.Member.key)[:3]


@pytest.mark.parametrize('mb', _three_cheapest('wgrad'), ids=gf.Member.id)
def test_the_data_show_a_dropped_last_pixel_of_the_last_run(mb):
    """A kernel gradient that loses the last pixel of its last run (a run boundary off by one) differs from the fp64 reference by
    more than the bound: what the pixel contributes is its source patch (x) its gradient row, computed here directly."""
    n, h, w, cin, cout, k, s = mb.shape()
    x, dy = gf.wgrad_inputs(mb.shape())
    ref = gf.wgrad_reference(x, dy, k, s)
    xp, _, _ = gf.pad_same(x.double(), k, s)
    oh, ow = mb.oh, mb.ow
    patch = xp[n - 1, :, (oh - 1) * s:(oh - 1) * s + k, (ow - 1) * s:(ow - 1) * s + k]                 # [cin, k, k]
    delta = patch.permute(1, 2, 0)[..., None] * dy[n - 1, :, oh - 1, ow - 1].double()                  # [k, k, cin, cout]
    dy2 = dy.clone()
    dy2[n - 1, :, oh - 1, ow - 1] = 0
    dropped = gf.wgrad_reference(x, dy2, k, s)
    assert float((ref - dropped - delta).abs().max()) <= 1e-9 * float(ref.abs().max())                 # the direct formula is what the reference loses
    assert float(delta.abs().max()) > WGRAD_TOL * float(ref.abs().max()), (float(delta.abs().max()), float(ref.abs().max()))


@pytest.mark.parametrize('mb', _three_cheapest('dgrad2'), ids=gf.Member.id)
def test_the_data_show_a_missing_border_tap(mb):
    """A stride-2 data gradient that loses ONE tap at the border (a wrong validity mask: here the first and the last kernel tap, whose
    contribution at the last / first rows and columns runs into the SAME pad) differs from the reference by more than the bound
    already on the border pixels alone."""
    n, h, w, cin, cout, k, s = mb.shape()
    dy, wk, _, _ = gf.dgrad2_inputs(mb.shape())
    ref = gf.dgrad2_reference(mb.shape(), dy, wk)
    bound = DGRAD_TOL * float(ref.abs().max())
    for tap in ((0, 0), (k - 1, k - 1)):
        d = (ref - gf.dgrad2_reference(mb.shape(), dy, wk, drop_tap=tap)).abs()
        border = torch.cat([d[:, :2].flatten(), d[:, -2:].flatten(), d[:, :, :2].flatten(), d[:, :, -2:].flatten()])
        assert float(border.max()) > bound, (tap, float(border.max()), bound)
