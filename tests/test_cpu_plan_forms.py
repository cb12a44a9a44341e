"""The generated list of plan-form representatives (tests/plan_forms.py) that test_gpu_plan_forms.py runs: it must not silently
shrink.  Host only: the plan queries launch nothing.  Run with -s to see the counts the README quotes."""
import os

import pytest

import plan_forms as pf

pytestmark = pytest.mark.skipif(bool(os.environ.get('Y3_NO_FAST')), reason='Y3_NO_FAST=1 leaves the generic-kernel classes only')


def _param_list(fn, name):
    return [m.args[1] for m in fn.pytestmark if m.name == 'parametrize' and m.args[0] == name][0]


def test_layer_table_is_the_appendix_a_table():
    import test_gpu_kernels as tk
    assert pf.APP_A == tk.APP_A


def test_every_split_form_and_tile_occurs_in_both_arithmetics():
    """Every split form the planner of an arithmetic can produce (plan_forms' docstring says which it cannot, and why), every tile
    of pick_tile / plan_conv_x3, the generic kernel, ragged row and column tiles: all among the representatives."""
    reps, _ = pf.representatives()
    for entry in pf.ENTRIES:
        for arith, only_other, tiles in (('f32', pf.X3_ONLY_FORMS, pf.F32_TILES), ('x3', pf.F32_ONLY_FORMS, pf.X3_TILES)):
            sigs = [s for s, _ in reps if s[0] == entry and s[1] == arith]
            assert set(s[5] for s in sigs) == set(pf.FORMS) - set(only_other), (entry, arith, sorted(set(s[5] for s in sigs)))
            assert set((s[3], s[4]) for s in sigs if s[2]) == set(tiles), (entry, arith)
            assert any(s[6] for s in sigs) and any(s[6] and s[5] != 'whole' for s in sigs), (entry, arith)
            # a ragged column tile: the 14-channel heads (forward), 32 columns on the 64-column x3 tile; pick_tile gives the f32 data
            # gradient into 32 / 64 channels a tile of exactly that width
            assert any(s[7] for s in sigs) == ((entry, arith) != ('dgrad', 'f32')), (entry, arith)
            assert any(not s[2] for s in sigs) == (arith == 'f32'), 'the generic kernel is f32-only'
    # a split on the 32-column tile of the 14-channel heads, and two slice counts on the 128 x 64 tile of the x3 data gradient
    assert any(s[:2] == ('fwd', 'f32') and s[4] == 32 and s[5] != 'whole' for s, _ in reps)
    assert any(s[:2] == ('dgrad', 'x3') and s[4] == 64 and s[5] == 'mixed' for s, _ in reps)


def test_every_class_has_a_unique_representative_within_the_cap(capsys):
    reps, left = pf.representatives()
    again, left2 = pf.representatives()
    assert [(s, mb.shape(), mb.entry, mb.arith) for s, mb in reps] == [(s, mb.shape(), mb.entry, mb.arith) for s, mb in again] and left == left2
    cls = pf.classes()
    assert len(set(s for s, _ in reps)) == len(reps) and set(s for s, _ in reps) | set(left) == set(cls) and not set(left) & set(s for s, _ in reps)
    assert len(set(mb.id() for _, mb in reps)) == len(reps)
    for sig, mb in reps:
        assert mb.signature() == sig and mb.within_cap(), mb
        assert mb.key() == cls[sig][0].key() or not cls[sig][0].within_cap(), 'not the cheapest member: %r' % mb
        n, h, w, cin, cout, k, s = mb.shape()
        assert mb.shape() in set(pf.layer_shapes()), 'not a layer of the network: %r' % mb
    for sig in left:
        assert not any(mb.within_cap() for mb in cls[sig]), pf.sig_id(sig)
    assert len(left) <= pf.MAX_LEFT_OUT * len(cls), [pf.sig_id(s) for s in left]
    assert len(cls) >= 100, 'the envelope lost classes: %d' % len(cls)
    with capsys.disabled():
        print('\nplan forms: %d envelope launches, %d classes, %d representatives (%.0f GFLOP of fp64 reference, largest %.1f), left out: %s'
              % (len(pf.envelope()), len(cls), len(reps), sum(mb.ref_flop() for _, mb in reps) / 1e9, max(mb.ref_flop() for _, mb in reps) / 1e9,
                 [pf.sig_id(s) for s in left] or 'none'))


def _older_coverage():
    """the envelope classes the shape lists of the older GPU tests reach (test_gpu_kernels.py, and the model tests' sizes)"""
    import test_gpu_kernels as tk
    fwd = list(tk.CONV_CASES) + list(_param_list(tk.test_conv_fwd_fused_inference_epilogue, 'shape'))
    fwd += [(n, h, w, cin, cout, 1, 1) for n, h, w, cin, cout in _param_list(tk.test_conv_fwd_detection_head, 'shape')]
    dgrad = list(tk.DGRAD_CASES) + [tuple(s[:6]) + (s[6] if len(s) > 6 else 1,) for s in _param_list(tk.test_conv_dgrad_bn_epilogue_stats, 'shape')]
    app = [(1 if hw >= 104 else 2, hw, hw, cin, cout, k, s) for hw, cin, cout, k, s in tk.APP_A]
    got = pf.covered_by(fwd, ('fwd',)) | pf.covered_by(dgrad, ('dgrad',)) | pf.covered_by(app)
    for side, n in ((96, 4), (96, 3), (416, 1), (416, 8)):          # the training step and inference, layer by layer
        got |= pf.step_classes(side, n)
    got |= pf.step_classes(608, 2, ('fwd',))                        # inference only
    return got & set(pf.classes())


def test_report_what_the_older_shape_lists_reach(capsys):
    """Printed, not asserted: the figure README quotes.  Also the (image side, batch) choice of the two added teacher-forced cases."""
    cls = set(pf.classes())
    old = _older_coverage()
    miss = cls - old
    lines = ['plan forms: the older GPU shape lists reach %d of %d envelope classes, %d are reached by test_gpu_plan_forms.py alone' % (len(old), len(cls), len(miss))]
    for side in pf.SIDES:
        lines.append('  step at side %d, classes no older list reaches, by batch: ' % side +
                     ', '.join('%d: %d' % (n, len(pf.step_classes(side, n) & miss)) for n in pf.BATCHES))
    lines.append('  inference at batch 4, forward classes no older list reaches: ' +
                 ', '.join('%d: %d' % (side, len(pf.step_classes(side, 4, ('fwd',)) & miss)) for side in (512, 608)))
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    assert old <= cls
