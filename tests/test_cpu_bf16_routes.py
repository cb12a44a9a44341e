"""The generated list of bf16 route representatives (tests/bf16_routes.py) that test_gpu_bf16_routes.py runs: it must cover every
kernel route of y3_conv2d_fwd_bf16_ws and must not silently change.  Host only: y3_conv2d_fwd_bf16_plan launches nothing.  Run
with -s to see the counts the README quotes."""
import bf16_routes as br

# The representatives at the commit that added the query, by id (class + layer shape).  A dispatch threshold of
# describe_bf16 or BF16_PATCH_MIN_BYTES (yolo3/model.py) that moves shows up here: look at what migrated, check that every
# kernel still has its fp64 case in test_gpu_bf16_routes.py, then regenerate with `python tests/bf16_routes.py`.
EXPECTED = [
    'c32128x64k32-s2-whole-n10_608x608_32_64_k3_s2',
    'c32256x64k32-s1r-whole-n16_256x256_32_64_k3_s1',
    'c64128x128k64-s1-whole-raggedM-n25_152x152_64_128_k3_s1',
    'c6464x128k64-s2-whole-n25_304x304_64_128_k3_s2',
    'pp256x256k64-whole-n16_40x40_128_256_k3_s1',
    'pp256x256k64-whole-raggedM-n25_38x38_256_256_k1_s1',
    'ring128x128k32-whole-n16_76x76_256_128_k1_s1',
    'ring128x128k32-whole-raggedM-n25_76x76_256_128_k1_s1',
    'ring128x128k32-whole-raggedM-raggedN-f32-n10_76x76_256_255_k1_s1',
    'ring128x128k32-whole-raggedN-f32-n16_52x52_256_255_k1_s1',
    'ring128x32k32-whole-n1_160x160_64_32_k1_s1',
    'ring128x32k32-whole-raggedM-raggedN-f32-n1_10x10_1024_14_k1_s1',
    'ring128x32k32-whole-raggedN-f32-n1_16x16_1024_14_k1_s1',
    'ring128x64k32-whole-n1_80x80_128_64_k1_s1',
    'ring128x64k32-whole-raggedM-n1_104x104_128_64_k1_s1',
    'ring256x128k64-whole-n16_52x52_256_128_k1_s1',
    'ring256x128k64-whole-raggedM-n8_76x76_256_128_k1_s1',
    'ring256x128k64-whole-raggedM-raggedN-f32-n8_52x52_256_255_k1_s1',
    'ring256x128k64-whole-raggedN-f32-n16_40x40_256_255_k1_s1',
    'ring64x64k32-short-last-raggedM-n4_13x13_512_1024_k3_s1',
    'ring64x64k32-uniform-n1_16x16_1024_512_k1_s1',
    'ring64x64k32-uniform-raggedM-n1_10x10_1024_512_k1_s1',
    'ring64x64k32-uniform-raggedM-raggedN-f32-n1_10x10_1024_255_k1_s1',
    'ring64x64k32-uniform-raggedN-f32-n1_16x16_1024_255_k1_s1',
    'ring64x64k32-whole-n1_40x40_256_128_k1_s1',
    'ring64x64k32-whole-raggedM-n1_10x10_512_512_k1_s1',
    'ring64x64k32-whole-raggedM-raggedN-f32-n1_20x20_512_255_k1_s1',
    'ring64x64k32-whole-raggedN-f32-n1_40x40_256_255_k1_s1',
]
EXPECTED_EXTRA = ['c32128x64k32-s2r-whole-n10_608x608_32_64_k3_s2', 'c32256x64k32-s1-whole-n10_304x304_32_64_k3_s1']
CLASS_FLOOR = 28       # what the query returned for the envelope at the commit that added it


def _param_list(fn, name):
    return [m.args[1] for m in fn.pytestmark if m.name == 'parametrize' and m.args[0] == name][0]


def test_the_restated_network_is_the_models_layer_list():
    """cin, cout, ksize, stride of bf16_routes.network() against yolo3.model.build_layer_specs, layer by layer (the pitches, the
    residuals and the flags are held to the model's launch list on the GPU: test_gpu_model.py)"""
    from yolo3.model import build_layer_specs, YoloV3
    assert (br.FILTERS, br.BLOCKS) == (YoloV3.FILTER_COUNT, YoloV3.BLOCK_COUNT)
    for head, (anchors, classes) in zip(br.HEADS, ((2, 2), (3, 80))):
        specs = build_layer_specs(3, anchors, classes)[0]
        net = br.network(head)
        assert len(net) == len(specs) - 1 == 74
        assert [(l[1], l[2], l[3], l[4], l[8]) for l in net] == [(sp.cin_pad, sp.cout, sp.k, sp.s, not sp.bn) for sp in specs[1:]]
    assert sum(1 for l in br.network(14) if l[5]) == 1 + 2 + 8 + 8 + 4


def test_the_300_mb_rule_restated():
    """no_patch() by hand at the 32 -> 64 layers of 608^2 tiles: the stride-2 one moves 2 * n * 304^2 * (4 * 32 + 64) bytes and
    crosses 300 MB between 8 and 10 tiles, the stride-1 one with its residual 2 * n * 304^2 * (32 + 2 * 64): between 10 and 11"""
    assert 2 * 8 * 304 * 304 * 192 < 300e6 <= 2 * 10 * 304 * 304 * 192
    assert br.no_patch(8 * 304 * 304, 32, 64, 2, False) and not br.no_patch(10 * 304 * 304, 32, 64, 2, False)
    assert 2 * 10 * 304 * 304 * 160 < 300e6 <= 2 * 11 * 304 * 304 * 160
    assert br.no_patch(10 * 304 * 304, 32, 64, 1, True) and not br.no_patch(11 * 304 * 304, 32, 64, 1, True)
    assert br.no_patch(2 * 152 * 152, 64, 128, 1, True) and not br.no_patch(45 * 152 * 152, 64, 128, 1, True)


def test_query_binding_and_refusal():
    """the query is a dry run of the entry point: it refuses what the entry point refuses (route 0, the reason in
    y3_last_error), reads no memory behind its pointers (they are made-up addresses here), and needs no GPU"""
    hip = br._lib()
    p, used = br.plan(2, 13, 13, 128, 256, 3, 1, flags=hip.EPI_LRELU)
    assert dict(zip(br.OUT_NAMES, p))['route'] == hip.BF16_ROUTE_RING and p[1:4] == [64, 64, 32] and used == 0
    p, used = br.plan(2, 13, 13, 48, 128, 3, 1)                         # Cin not a multiple of 32
    assert p == [0] * 12 and used == 0 and b'Cin=48' in hip.lib.y3_last_error()
    p, used = br.plan(91, 608, 608, 32, 64, 3, 2)                       # src of 2.15 GB
    assert p[0] == 0 and b'2 GiB' in hip.lib.y3_last_error()
    assert br.plan(90, 608, 608, 32, 64, 3, 2, flags=hip.EPI_LRELU)[0][0] == hip.BF16_ROUTE_C32
    assert br.plan(90, 608, 608, 32, 64, 3, 2, flags=hip.EPI_LRELU | hip.BF16_NO_PATCH)[0][:3] == [hip.BF16_ROUTE_RING, 128, 64]
    # the workspace decides the split, to the byte
    need = int(hip.lib.y3_conv2d_fwd_bf16_workspace(8 * 169, 512, 3, 1024))
    assert need > 256 * 1024
    full, used = br.plan(8, 13, 13, 512, 1024, 3, 1, ws_bytes=need)
    assert used == need and full[6] > 1 and full[4] == full[6] * 22 * 16
    for short in (need - 1, 0):
        one, used = br.plan(8, 13, 13, 512, 1024, 3, 1, ws_bytes=short)
        assert used == 0 and one[6] == 1 and one[4] == 22 * 16 and one[:4] == full[:4]


def test_alignment_and_alpha_move_a_launch_off_its_kernel():
    """vec_ok (16-byte rows of dst / resid) and alpha outside [0, 1] are part of the route: the shapes that otherwise take the
    ping-pong or a patch kernel fall back to the ring kernel"""
    hip = br._lib()
    L = hip.EPI_LRELU
    pp = (16, 40, 40, 128, 256, 3, 1)
    assert br.plan(*pp, flags=L)[0][0] == hip.BF16_ROUTE_PP
    for kw in (dict(dst_ld=258), dict(dst_ptr=br.FAKE + 4), dict(resid=True, resid_ptr=br.FAKE + 4), dict(resid=True, resid_ld=258)):
        p = br.plan(*pp, flags=L, **kw)[0]
        assert p[0] == hip.BF16_ROUTE_RING and p[8] == 0, kw
    for shape, route in (((10, 304, 304, 32, 64, 3, 1), hip.BF16_ROUTE_C32), ((25, 152, 152, 64, 128, 3, 1), hip.BF16_ROUTE_C64)):
        assert br.plan(*shape, flags=L, alpha=0.2)[0][0] == route and br.plan(*shape, flags=L, alpha=1.0)[0][0] == route
        assert br.plan(*shape, flags=0, alpha=1.5)[0][0] == route             # linear: alpha is not read
        for alpha in (1.5, -0.1):
            assert br.plan(*shape, flags=L, alpha=alpha)[0][0] == hip.BF16_ROUTE_RING
        assert br.plan(*shape, flags=L, dst_ld=shape[4] + 2)[0][0] == hip.BF16_ROUTE_RING
        assert br.plan(*shape, flags=L, wt_ptr=br.FAKE + 8)[0][0] == hip.BF16_ROUTE_RING
        assert br.plan(*shape, flags=L, out_f32=True)[0][0] == hip.BF16_ROUTE_RING
        assert br.plan(*shape, flags=L, bias=False)[0][0] == route


def test_the_variant_table_names_the_routes_it_takes():
    """test_gpu_bf16_routes.VARIANTS: every case really takes the kernel, tile and epilogue path it is named after (the GPU test asks
    again with the real pointers), and the table enters each branch the model never enters"""
    import test_gpu_bf16_routes as tg
    seen = set()
    for name, shape, expect, kw in tg.VARIANTS:
        c = tg.variant_case(name, shape, kw)
        p, used = tg.host_plan(c)
        assert (br.route_names().get(p[0]), p[1], p[2], p[8], p[6] > 1) == expect, (name, dict(zip(br.OUT_NAMES, p)))
        n, h, w, cin, cout, k, s = shape
        assert 2.0 * n * h * w * cin * cout * k * k / (s * s) <= br.CAP_FLOP / 10, 'a variant is a small shape with a full fp64 reference'
        seen.add((expect[0], expect[1], expect[2], 'vec' if p[8] else 'novec', 'f32' if c.out_f32 else 'bf16', 'resid' if c.resid else '-'))
        seen.add(('flags', c.flags, c.out_f32))
        seen.add(('alpha', expect[0], cin, c.alpha))
        seen.add(('ptrs', expect[0], c.bias, c.affine, c.resid))
        seen.add(('ws', c.ws, p[6] > 1))
        if cout % 8 and p[8] and not c.out_f32 and c.resid:
            seen.add('ragged group, bf16 out, residual')
    for tile in ((64, 64), (128, 128), (256, 128)):
        for resid in ('resid', '-'):
            assert ('ring',) + tile + ('novec', 'bf16', resid) in seen
    assert ('ring', 128, 32, 'novec', 'f32', '-') in seen and 'ragged group, bf16 out, residual' in seen
    assert ('flags', 0, False) in seen and ('flags', 0, True) in seen
    for cin in (32, 64):
        assert ('alpha', 'ring', cin, 1.5) in seen and ('alpha', 'ring', cin, -0.1) in seen and ('alpha', 'c%d' % cin, cin, 0.2) in seen
    assert ('ptrs', 'ring', True, False, True) in seen and ('ptrs', 'pp', True, False, True) in seen          # no scale / shift, with a residual
    assert ('ptrs', 'ring', False, True, False) in seen and ('ptrs', 'c32', False, True, False) in seen       # no bias
    assert ('ws', 'query', True) in seen and ('ws', 'plain', False) in seen and ('ws', 'short', False) in seen and ('ws', 'none', False) in seen


def test_every_class_has_a_unique_representative_within_the_cap(capsys):
    reps, left = br.representatives()
    again, left2 = br.representatives()
    assert [(s, mb.args()) for s, mb in reps] == [(s, mb.args()) for s, mb in again] and left == left2
    cls = br.classes()
    assert len(left) <= br.MAX_LEFT_OUT * len(cls) and not left, [br.sig_id(s) for s in left]
    assert len(set(s for s, _ in reps)) == len(reps) and set(s for s, _ in reps) == set(cls)
    assert len(set(mb.id() for _, mb in reps)) == len(reps)
    env = set(mb.args() for mb in br.envelope())
    for sig, mb in reps:
        assert mb.signature() == sig and mb.within_cap() and mb.args() in env, mb
        assert mb.key() == cls[sig][0].key(), 'not the cheapest member: %r' % mb
        assert len(mb.subset()) <= br.SUBSET and mb.subset() == sorted(set(mb.subset())) and {0, mb.n - 1} <= set(mb.subset())
        assert mb.n <= br.SUBSET or any(b - a == 1 for a, b in zip(mb.subset()[1:-1], mb.subset()[2:-1]))       # the adjacent middle pair
        assert (mb.plan()[1] > 0) == (sig[5] != 'whole') and mb.plan()[1] in (0, mb.workspace_bytes())
    assert len(cls) >= CLASS_FLOOR, 'the envelope lost classes: %d' % len(cls)
    with capsys.disabled():
        print('\nbf16 routes: %d envelope launches, %d classes, %d representatives + %d off-network patch instantiations (%.0f GFLOP of fp64 '
              'reference, largest %.1f), left out: none' % (len(env), len(cls), len(reps), len(br.extra_members()),
                                                             sum(mb.ref_flop() for _, mb in reps) / 1e9, max(mb.ref_flop() for _, mb in reps) / 1e9))


def test_the_representative_list_is_the_recorded_one():
    """Moving a threshold of the dispatch chain (the 96 ping-pong tiles, the 150..300 tiles of 256 x 128, the 512 of 128 x 128, the
    split-K plan) or BF16_PATCH_MIN_BYTES moves launches between kernels: the list changes, and this test says which way."""
    got = [mb.id() for _, mb in br.representatives()[0]]
    assert got == EXPECTED, 'representatives changed: gone %s, new %s' % (sorted(set(EXPECTED) - set(got)), sorted(set(got) - set(EXPECTED)))
    assert sorted(mb.id() for _, mb in br.extra_members()) == EXPECTED_EXTRA


def test_every_route_tile_and_form_occurs():
    hip = br._lib()
    sigs = [s for s, _ in br.representatives()[0]]
    assert set(s[0] for s in sigs) == {hip.BF16_ROUTE_PP, hip.BF16_ROUTE_C32, hip.BF16_ROUTE_C64, hip.BF16_ROUTE_RING}
    # patch instantiations: the network launches four of the six the library compiles (its stride-1 32 -> 64 layer always has a
    # residual, its stride-2 one never); extra_members() are the other two, and test_gpu_bf16_routes.py runs all six
    net = set((s[0],) + s[4] for s in sigs if s[4])
    assert net == {(hip.BF16_ROUTE_C32, 1, 1), (hip.BF16_ROUTE_C32, 2, 0), (hip.BF16_ROUTE_C64, 1, 0), (hip.BF16_ROUTE_C64, 2, 0)}
    extra = set((s[0],) + s[4] for s, _ in br.extra_members())
    assert extra == {(hip.BF16_ROUTE_C32, 1, 0), (hip.BF16_ROUTE_C32, 2, 1)} and len(net | extra) == 6
    assert not any(s in set(sigs) for s, _ in br.extra_members())
    ring = [s for s in sigs if s[0] == hip.BF16_ROUTE_RING]
    assert set((s[1], s[2]) for s in ring) == set(br.RING_TILES)
    assert set(s[3] for s in ring if (s[1], s[2]) == (256, 128)) == {64} and set(s[3] for s in ring if (s[1], s[2]) != (256, 128)) == {32}
    assert set(s[5] for s in ring if (s[1], s[2]) == (64, 64)) == set(br.SPLIT_FORMS)
    assert all(s[5] == 'whole' for s in sigs if (s[1], s[2]) != (64, 64) or s[0] != hip.BF16_ROUTE_RING)
    # a ragged last row tile on every tile route (the ping-pong kernel and the five ring tiles), and on a split launch
    for tile in set(br.RING_TILES) | {(256, 256)}:
        assert any(s[6] for s in sigs if (s[1], s[2]) == tile), tile
    assert any(s[6] and s[5] != 'whole' for s in sigs)
    # a ragged, fp32-output column tile (the 255-channel head) on the big tiles of the ring kernel
    for tile in ((256, 128), (128, 128)):
        assert any(s[7] and s[8] for s in sigs if (s[1], s[2]) == tile), tile
    assert all(s[9] == 1 for s in sigs), 'the model aligns every row: vec_ok == 0 is test_gpu_bf16_routes.py\'s variants'


def test_report_what_the_older_tests_reach(capsys):
    """Printed, not asserted: which classes test_gpu_kernels.BF16_CASES and the (side, batch) pairs of the model tests reach."""
    import test_gpu_kernels as tk
    cls = set(br.classes())
    cases = br.covered_by(tk.BF16_CASES) & cls
    model = set()
    for side, n in ((96, 2), (96, 3), (416, 1), (608, 2)):       # test_bf16_layers_teacher_forced / test_bf16_inference_matches_bf16_oracle before this file
        model |= br.forward_classes(side, n)
    tiled = set()
    for n in (10, 45):                                             # test_tiled_4k_bf16_against_fp32: detections only, end to end
        tiled |= br.forward_classes(608, n)
    lines = ['bf16 routes: of %d envelope classes BF16_CASES reach %d, the per-layer model tests at batch <= 3 reach %d, together %d'
             % (len(cls), len(cases), len(model & cls), len((cases | model) & cls)),
             '  reached by neither: ' + ', '.join(sorted(br.sig_id(s) for s in cls - cases - model)),
             '  of those, run (unchecked per layer) by the 4096^2 tiled test: ' + ', '.join(sorted(br.sig_id(s) for s in (cls - cases - model) & tiled)),
             '  the teacher-forced cases (608, 10) and (608, 45) reach %d and %d classes' % (len(br.forward_classes(608, 10) & cls), len(br.forward_classes(608, 45) & cls))]
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    assert model <= cls | br.forward_classes(96, 2) | br.forward_classes(96, 3)
