"""Per-scale anchor assignment on the GPU: y3_format_labels_scales, y3_decode_fwd_scales, y3_truth_boxes_scales and
YoloV3(anchor_scales=...).

Everything rests on one identity: in both modes a box goes to the same cell and to its globally best anchor, so for every scale s
    labels_scale[s] == labels_all[s][..., mask_s, :]
bit for bit, collisions included (tests/anchor_scales_cases.py).  The decode rows are those of three one-scale y3_decode_fwd calls
with each scale's anchors, the truth gather is the concatenation of three y3_truth_boxes calls: all bit for bit.

Gradients: tests/teacher_forced.py builds oracle.model.Net with ONE anchor count for all three heads and checks the loss with all
anchors on every scale, so it cannot express per-scale heads without modification.  As the issue provides for that case, the head
gradients are held against fp64 instead, with teacher_forced.BOUNDS unchanged: dfm and loss4 against autograd of the existing
loss restatement (oracle.model.loss_layer, given each scale's anchors in slot order), the heads' kernel, bias and data gradients
against the fp64 products of the step's own activations.  Everything behind the heads is the code the existing tests cover.

Not covered here: the mAP effect (no real dataset)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import anchor_scales_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
PAD_HEAD, PAD_TAIL = 5, 7          # floats of NaN canary in front of and behind every output: the outputs start 4-byte aligned only


@pytest.fixture(scope='module')
def hip():
    from yolo3 import _hip
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return _hip


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- 1. y3_format_labels_scales --------------------------------------------------------------------------------------------------
def _labels_scales(hip, boxes, counts, size, anchors, K, table):
    """-> (three label tensors [n, G, G, A_s, 5+K] cut out of NaN-filled buffers, the buffers)"""
    n, m = boxes.shape[0], boxes.shape[1]
    shapes = [(n, size // (32 >> s), size // (32 >> s), table.count(s), 5 + K) for s in range(3)]
    bufs = [torch.full((PAD_HEAD + int(np.prod(sh)) + PAD_TAIL,), float('nan'), device='cuda') for sh in shapes]
    ptr = [b.data_ptr() + 4 * PAD_HEAD for b in bufs]
    hip.check(hip.lib.y3_format_labels_scales(boxes.data_ptr() if m else None, counts.data_ptr(), n, m,
                                              hip.float_array([v for a in anchors for v in a]), hip.int_array(table), len(anchors), K, size, size,
                                              ptr[0], ptr[1], ptr[2], _stream()), 'y3_format_labels_scales')
    torch.cuda.synchronize()
    return [b[PAD_HEAD:PAD_HEAD + int(np.prod(sh))].view(sh) for b, sh in zip(bufs, shapes)], bufs


def _check_labels(hip, boxes, counts, size, anchors, K, table, host=True):
    from yolo3.imagereader import format_boxes, format_labels_device
    b, c = torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda()
    got, bufs = _labels_scales(hip, b, c, size, anchors, K, table)
    for buf in bufs:      # canaries on both sides untouched
        assert bool(torch.isnan(buf[:PAD_HEAD]).all()) and bool(torch.isnan(buf[-PAD_TAIL:]).all())
    for g in got:         # every word written, zeros included
        assert not bool(torch.isnan(g).any())
    full = format_labels_device(b, c, (size, size, 3), anchors, K)
    masks = C.masks_of(table)
    written = 0
    for s in range(3):
        want = full[s][:, :, :, masks[s], :]
        assert _same(got[s], want), 'scale %d differs from the gather of y3_format_labels' % s
        written += int((got[s][..., 4] != 0).sum())
    if host:
        for i in range(boxes.shape[0]):
            twin = format_boxes(boxes[i, :counts[i]].copy(), (size, size, 3), anchors, K, anchor_scale=table)
            for s in range(3):
                assert _same(got[s][i].cpu(), torch.from_numpy(twin[s])), 'image %d scale %d differs from the host twin' % (i, s)
    again, _ = _labels_scales(hip, b, c, size, anchors, K, table)
    for s in range(3):
        assert _same(got[s], again[s])
    # the API wrapper is the same launch
    api = format_labels_device(b, c, (size, size, 3), anchors, K, anchor_scale=table)
    for s in range(3):
        assert _same(got[s], api[s])
    return written


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('size', [64, 96])
@pytest.mark.parametrize('name', sorted(C.PARTITIONS))
def test_labels_equal_the_gather_and_the_host_twin(hip, name, size, K):
    anchors, table = C.PARTITIONS[name]
    boxes, counts = C.box_batch(size, K, seed=size + K)          # image 0: 300 boxes (two chunk passes), image 1: none
    assert counts.tolist() == [300, 0]
    written = _check_labels(hip, boxes, counts, size, anchors, K, table)
    assert written > 20


def test_labels_eighty_classes_cross_run_boundaries(hip):
    """K = 80 with three anchors per scale: AD = 255, a run is 64 cells, and the 288 fine cells of two 96^2 images cross several
    run boundaries at an unaligned head."""
    anchors, table = C.PARTITIONS['3/3/3']
    boxes, counts = C.box_batch(96, 80, seed=7, per_image=(300, 40))
    assert 16384 // (3 * 85) == 64 and 2 * 12 * 12 > 4 * 64
    assert _check_labels(hip, boxes, counts, 96, anchors, 80, table) > 40


def test_labels_collisions(hip):
    anchors, table = C.PARTITIONS['1/2/3']
    for boxes in (C.collision_same_anchor(anchors), C.collision_other_scale(anchors, table)):
        b = np.zeros((2, len(boxes), 5), np.int32)
        b[0] = boxes
        b[1] = boxes[::-1]                                       # the other input order: the other box's coordinates win
        _check_labels(hip, b, np.array([len(boxes)] * 2, np.int32), 64, anchors, 3, table)


def test_labels_edges(hip):
    anchors, table = C.PARTITIONS['shuffled']
    K = 3
    # no boxes at all, and max_boxes = 0 with a null pointer
    _check_labels(hip, np.zeros((2, 4, 5), np.int32), np.zeros(2, np.int32), 64, anchors, K, table)
    _check_labels(hip, np.zeros((2, 0, 5), np.int32), np.zeros(2, np.int32), 64, anchors, K, table)
    # a box whose cell or class is outside the tensor writes nothing (the host loop raises or wraps there: no host twin)
    boxes = np.array([[[200, 10, 9, 9, 0], [10, 300, 9, 9, 1], [-90, 10, 9, 9, 1], [10, 10, 9, 9, K], [10, 10, 9, 9, -1], [20, 20, 12, 12, 2]]] * 2, np.int32)
    assert _check_labels(hip, boxes, np.array([6, 6], np.int32), 64, anchors, K, table, host=False) == 2
    # counts above max_boxes and below zero are clamped
    _check_labels(hip, boxes, np.array([9, -3], np.int32), 64, anchors, K, table, host=False)


def test_entry_points_refuse_bad_arguments(hip):
    lib = hip.lib
    anc = hip.float_array([4, 4, 8, 8, 16, 16, 32, 32])
    out = torch.zeros(4096, device='cuda')
    cnt = torch.zeros(2, dtype=torch.int32, device='cuda')
    p = out.data_ptr()

    def labels(table, A=4, K=1, size=64, anchors=anc, counts=cnt.data_ptr(), o3=p):
        return lib.y3_format_labels_scales(None, counts, 2, 0, anchors, None if table is None else hip.int_array(table), A, K, size, size, p, p, o3, None)
    for kw in (dict(table=[0, 1, 1, 1]), dict(table=[0, 1, 2, 3]), dict(table=[0, 1, 2, -1]), dict(table=None), dict(table=[0, 1, 2, 2], A=17),
               dict(table=[0, 1], A=2), dict(table=[0, 1, 2, 2], K=0), dict(table=[0, 1, 2, 2], size=48), dict(table=[0, 1, 2, 2], counts=None),
               dict(table=[0, 1, 2, 2], o3=None)):
        assert labels(**kw) == -1 and b'format_labels_scales' in lib.y3_last_error(), kw
    fm = (hip.Tensor * 3)(*[hip.Tensor(p, 1, g, g, 6, 8) for g in (1, 2, 4)])
    tab = hip.int_array([0, 1, 2])
    assert lib.y3_decode_fwd_scales(fm, anc, hip.int_array([0, 0, 1]), 3, 1, 32, 32, p, None) == -1 and b'every scale' in lib.y3_last_error()
    assert lib.y3_decode_fwd_scales(fm, anc, tab, 3, 2, 32, 32, p, None) == -1 and b'geometry' in lib.y3_last_error()       # c != A_s (5+K)
    assert lib.y3_decode_fwd_scales(fm, anc, None, 3, 1, 32, 32, p, None) == -1 and b'null' in lib.y3_last_error()
    assert lib.y3_decode_fwd_scales(fm, anc, hip.int_array([0, 1]), 2, 1, 32, 32, p, None) == -1
    short = (hip.Tensor * 3)(*[hip.Tensor(p, 1, g, g, 6, 5) for g in (1, 2, 4)])                                         # ld < c
    assert lib.y3_decode_fwd_scales(short, anc, tab, 3, 1, 32, 32, p, None) == -1 and b'geometry' in lib.y3_last_error()
    ip = cnt.data_ptr()
    for args in ((None, p, p, 2, 4, 4, 4, 6, p, ip, 8), (p, p, p, 0, 4, 4, 4, 6, p, ip, 8), (p, p, p, 2, 0, 4, 4, 6, p, ip, 8),
                 (p, p, p, 2, 4, 4, 4, 4, p, ip, 8), (p, p, p, 2, 4, 4, 4, 6, p, ip, 0), (p, p, p, 2, 4, 4, 4, 6, p, None, 8),
                 (p, p, p, 2, 4, 4, 1 << 31, 6, p, ip, 8)):
        assert lib.y3_truth_boxes_scales(*args, None) == -1 and b'truth_boxes_scales' in lib.y3_last_error(), args
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and int(cnt.abs().sum()) == 0          # nothing was launched


# ---- 2. y3_decode_fwd_scales -----------------------------------------------------------------------------------------------------
def _decode_case(hip, n, grids, anchors, table, K, img, seed):
    """Random feature maps with ld > c -> (rows of y3_decode_fwd_scales, rows of three y3_decode_fwd(nscales=1) calls concatenated)"""
    g = torch.Generator().manual_seed(seed)
    masks = C.masks_of(table)
    D = 5 + K
    bufs, views = [], []
    for s, G in enumerate(grids):
        c = len(masks[s]) * D
        ld = c + 3
        buf = (torch.randn(n * G * G * ld, generator=g) * 1.2).cuda()
        bufs.append(buf)
        views.append(hip.Tensor(buf.data_ptr(), n, G, G, c, ld))
    nb = sum(G * G * len(m) for G, m in zip(grids, masks))
    out = torch.full((n, nb, D), float('nan'), device='cuda')
    arr = (hip.Tensor * 3)(*views)
    hip.check(hip.lib.y3_decode_fwd_scales(arr, hip.float_array([v for a in anchors for v in a]), hip.int_array(table), len(anchors), K, img, img,
                                           out.data_ptr(), _stream()), 'y3_decode_fwd_scales')
    parts = []
    for s, G in enumerate(grids):
        sub = [anchors[a] for a in masks[s]]
        o = torch.full((n, G * G * len(sub), D), float('nan'), device='cuda')
        one = (hip.Tensor * 1)(views[s])
        hip.check(hip.lib.y3_decode_fwd(one, 1, hip.float_array([v for a in sub for v in a]), len(sub), K, img, img, o.data_ptr(), _stream()), 'y3_decode_fwd')
        parts.append(o)
    torch.cuda.synchronize()
    return out, torch.cat(parts, dim=1)


@pytest.mark.parametrize('size', [64, 96])
@pytest.mark.parametrize('name', sorted(C.PARTITIONS))
def test_decode_equals_three_one_scale_calls(hip, name, size):
    anchors, table = C.PARTITIONS[name]
    K = 2                                                        # D_s = 7 A_s: 7, 14, 21 -- no multiple of 4, and ld = c + 3
    got, want = _decode_case(hip, 2, [size // 32, size // 16, size // 8], anchors, table, K, size, seed=size)
    assert not bool(torch.isnan(got).any()) and _same(got, want)


def test_decode_second_pass_of_the_grid_stride_loop(hip):
    """N * nb = 34 * 16128 = 548352 rows > 2048 blocks x 256 threads: the last rows are the second trip of the loop."""
    anchors, table = C.PARTITIONS['3/3/3']
    got, want = _decode_case(hip, 34, [16, 32, 64], anchors, table, 2, 512, seed=3)
    assert got.shape[0] * got.shape[1] > 2048 * 256
    assert not bool(torch.isnan(got).any()) and _same(got, want)


# ---- 3. y3_truth_boxes_scales ----------------------------------------------------------------------------------------------------
def _truth_case(seed, n, cas, d):
    rng = np.random.default_rng(seed)
    gts = []
    for ca in cas:
        g = rng.standard_normal((n, ca, d)).astype(np.float32)
        g[..., 4] = (rng.random((n, ca)) < 0.2).astype(np.float32)
        gts.append(torch.from_numpy(g).cuda())
    return gts


def _truth_scales(hip, gts, cap):
    n, d = gts[0].shape[0], gts[0].shape[2]
    boxes = torch.full((n, cap, 4), float('nan'), device='cuda')
    counts = torch.full((n,), -77, dtype=torch.int32, device='cuda')
    hip.check(hip.lib.y3_truth_boxes_scales(gts[0].data_ptr(), gts[1].data_ptr(), gts[2].data_ptr(), n, gts[0].shape[1], gts[1].shape[1],
                                            gts[2].shape[1], d, boxes.data_ptr(), counts.data_ptr(), cap, _stream()), 'y3_truth_boxes_scales')
    torch.cuda.synchronize()
    return boxes, counts


@pytest.mark.parametrize('cas', [(4, 32, 192), (9, 72, 432), (1, 255, 257), (300, 1, 64)])
def test_truth_gather_equals_three_calls(hip, cas):
    n, d = 2, 7
    gts = _truth_case(sum(cas), n, cas, d)
    singles = []
    for g in gts:
        b = torch.full((n, g.shape[1], 4), float('nan'), device='cuda')
        c = torch.zeros(n, dtype=torch.int32, device='cuda')
        hip.check(hip.lib.y3_truth_boxes(g.data_ptr(), n, g.shape[1], d, b.data_ptr(), c.data_ptr(), g.shape[1], _stream()), 'y3_truth_boxes')
        singles.append((b, c))
    torch.cuda.synchronize()
    totals = sum(c for _, c in singles)
    lists = [torch.cat([b[i, :int(c[i])] for b, c in singles]) for i in range(n)]
    assert int(totals.min()) > 3
    for cap in (int(totals.max()), int(totals.min()) - 2, 1):              # exactly the total (of the longest list); smaller than every total
        boxes, counts = _truth_scales(hip, gts, cap)
        assert torch.equal(counts, totals)                                 # the TRUE count, also above cap
        for i in range(n):
            m = min(cap, int(totals[i]))
            assert _same(boxes[i, :m], lists[i][:m])
            assert bool(torch.isnan(boxes[i, m:]).all())                   # nothing past the list, nothing past cap
    again = _truth_scales(hip, gts, int(totals.max()))
    first = _truth_scales(hip, gts, int(totals.max()))
    assert torch.equal(_bits(again[0]), _bits(first[0]))


# ---- 4. the model ----------------------------------------------------------------------------------------------------------------
MODELS = {'A6 1/2/3': ('1/2/3', 2), 'A9 3/3/3': ('3/3/3', 2)}
IMG, N = 64, 2


def _model(name, **kw):
    from yolo3.model import YoloV3
    anchors, table = C.PARTITIONS[MODELS[name][0]]
    return YoloV3(N, [IMG, IMG, 3], MODELS[name][1], anchors, learning_rate=1e-3, seed=11, anchor_scales=table, **kw)


def _inputs(name, seed=5, per_image=(5, 3)):
    anchors, table = C.PARTITIONS[MODELS[name][0]]
    K = MODELS[name][1]
    images = torch.randn(N, 3, IMG, IMG, generator=torch.Generator().manual_seed(seed)).cuda()
    gts = C.label_batch(IMG, K, anchors, table, seed, per_image)
    return images, [torch.from_numpy(g).cuda() for g in gts]


@pytest.mark.parametrize('name', sorted(MODELS))
def test_model_shapes_predict_and_loss(hip, name):
    from yolo3.model import YoloV3
    lib = hip.lib
    anchors, table = C.PARTITIONS[MODELS[name][0]]
    K = MODELS[name][1]
    masks = C.masks_of(table)
    yolo = _model(name)
    assert yolo.anchor_scale == table and yolo.scale_anchor_counts == [len(m) for m in masks]
    assert [sp.cout for sp in yolo.specs if not sp.bn] == [len(m) * (5 + K) for m in masks]
    nb = sum(len(m) * (IMG // (32 >> s)) ** 2 for s, m in enumerate(masks))
    assert yolo.number_output_boxes == nb
    images, gts = _inputs(name)
    # three index lists and 'auto' name the same network where they describe the same table
    assert YoloV3(N, [IMG, IMG, 3], K, anchors, anchor_scales=masks).anchor_scale == table
    # predict rows == y3_decode_fwd_scales on feature_maps()
    rows = yolo.predict(images).clone()
    assert tuple(rows.shape) == (N, nb, 5 + K)
    fms = [f.permute(0, 2, 3, 1).contiguous() for f in yolo.feature_maps(images)]
    arr = (hip.Tensor * 3)(*[hip.Tensor(f.data_ptr(), N, f.shape[1], f.shape[2], f.shape[3], f.shape[3]) for f in fms])
    out = torch.empty_like(rows)
    hip.check(lib.y3_decode_fwd_scales(arr, yolo.anchors_c, yolo.anchor_scale_c, len(anchors), K, IMG, IMG, out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _same(rows, out)
    # the loss of train_step == the three direct loss calls on its own feature maps
    plan = yolo._plan(N, True)
    assert plan.decode_call[0] == lib.y3_decode_fwd_scales and [c[0] for c in plan.loss_calls] == [lib.y3_loss_fwd_bwd] * 3
    loss = yolo.train_step((images, gts))
    torch.cuda.synchronize()
    loss4 = torch.zeros(4, device='cuda')
    keep = []
    for s, f in enumerate(plan.fms):
        c = len(masks[s]) * (5 + K)
        ld = (c + 3) // 4 * 4
        assert (f.c, f.ld) == (c, ld) and tuple(plan.gt[s].shape) == (N, f.h, f.w, len(masks[s]), 5 + K)
        dfm = torch.full((N * f.h * f.w * ld,), -7.0, device='cuda')
        ws = torch.zeros(int(lib.y3_loss_workspace_bytes()) // 4 + 4, device='cuda')
        sub = hip.float_array([v for a in masks[s] for v in anchors[a]])
        hip.check(lib.y3_loss_fwd_bwd(f.v, gts[s].data_ptr(), sub, len(masks[s]), K, IMG, IMG, float(N), loss4.data_ptr(),
                                      hip.Tensor(dfm.data_ptr(), N, f.h, f.w, c, ld), ws.data_ptr(), _stream()))
        torch.cuda.synchronize()
        keep.append((dfm, ws, sub))
        got = f.grad.buf.view(N, f.h, f.w, ld)[..., :c]
        assert _same(got, dfm.view(N, f.h, f.w, ld)[..., :c]), 'dfm of scale %d' % s
    assert _same(plan.loss4, loss4)
    assert torch.equal(loss, loss4.sum() / float(N))
    # test_step: the same labels, inference-mode BatchNorm
    assert np.isfinite(float(yolo.test_step((images, gts))))


@pytest.mark.parametrize('name', sorted(MODELS))
def test_model_head_gradients_against_fp64(hip, name):
    """teacher_forced.BOUNDS, unchanged, on what the per-scale heads change: dfm and loss4 against fp64 autograd of the loss
    restatement with each scale's anchors, and the head's kernel / bias / data gradient against fp64 products of the step's own
    activations (the input of a head feeds nothing else, so its gradient is the head's data gradient alone)."""
    import teacher_forced as tf
    from oracle import model as om
    anchors, table = C.PARTITIONS[MODELS[name][0]]
    K = MODELS[name][1]
    masks = C.masks_of(table)
    yolo = _model(name, conv_arithmetic='f32')
    images, gts = _inputs(name)
    pre = yolo.params.clone()
    yolo.train_step((images, gts))
    torch.cuda.synchronize()
    plan = yolo._plan(N, True)
    heads = [op for op in plan.ops if op[0] == 'head']
    assert len(heads) == 3
    rep = tf.Report('anchor scales ' + name)
    W = tf.unpack(pre, yolo.specs)
    G = tf.unpack(yolo.grads, yolo.specs)
    want4 = torch.zeros(4, dtype=torch.float64)
    for s, (_, i, src, fm, _) in enumerate(heads):
        sub = [anchors[a] for a in masks[s]]
        x = fm.torch_view().permute(0, 3, 1, 2).cpu().double().requires_grad_(True)
        parts = om.loss_layer(x, gts[s].cpu().double(), (IMG, IMG, 3), sub, K)
        (sum(parts) / float(N)).backward()
        want4 += torch.stack([p.detach() for p in parts])
        dfm = fm.grad.torch_view().cpu().double()                                   # [N, G, G, D_s]
        rep.add('dfm', i, dfm.permute(0, 3, 1, 2), x.grad)
        a = src.torch_view().cpu().double()                                          # [N, G, G, Cin]
        rep.add('head_dW', i, G[i]['W'].cpu()[0, 0], torch.einsum('nhwi,nhwo->io', a, dfm))
        rep.add('head_db', i, G[i]['b'].cpu(), dfm.sum(dim=(0, 1, 2)), atol=tf.BOUNDS['head_db'] * max(float(dfm.abs().sum(dim=(0, 1, 2)).max()), 1e-30))
        rep.add('dact', i, src.grad.torch_view().cpu(), torch.einsum('nhwo,io->nhwi', dfm, W[i]['W'].cpu().double()[0, 0]))
    rep.add('loss4', 'all', plan.loss4.cpu(), want4)
    rep.print()
    assert not rep.failures, rep.failures


@pytest.mark.parametrize('name', sorted(MODELS))
def test_model_captured_step_equals_eager(name):
    eager, graph = _model(name), _model(name, use_graph=True)
    for step in range(3):
        images, gts = _inputs(name, seed=20 + step, per_image=(4, step))          # changing labels; step 0: an image without boxes
        le, lg = eager.train_step((images, gts)), graph.train_step((images, gts))
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (step, float(le), float(lg))
        for attr in ('grads', 'params', 'moving', 'adam_m', 'adam_v'):
            assert torch.equal(getattr(eager, attr), getattr(graph, attr)), (step, attr)
    assert graph._plan(N, True).graph is not None
    images, _ = _inputs(name)
    assert _same(eager.predict(images), graph.predict(images))


@pytest.mark.parametrize('name', sorted(MODELS))
def test_model_truth_mask_gathers_from_all_scales(hip, name):
    import ignore_mask_reference as M
    from test_gpu_ignore_mask import _compare_gradient, _compare_parts
    anchors, table = C.PARTITIONS[MODELS[name][0]]
    K = MODELS[name][1]
    masks = C.masks_of(table)
    thr = 0.3
    yolo = _model(name, ignore_mask='truth', ignore_thresh=thr, max_truth_boxes=16)
    images, gts = _inputs(name, seed=9, per_image=(6, 0))
    yolo.train_step((images, gts))
    torch.cuda.synchronize()
    plan = yolo._plan(N, True)
    assert plan.truth_call[0] == hip.lib.y3_truth_boxes_scales and [c[0] for c in plan.loss_calls] == [hip.lib.y3_loss_fwd_bwd_truth] * 3
    per_scale = [M.truth_boxes(g.cpu()) for g in gts]
    truth = [torch.cat([per_scale[s][i] for s in range(3)]) for i in range(N)]       # coarse -> fine, each in index order
    assert plan.truth_counts.cpu().tolist() == [t.shape[0] for t in truth] and truth[0].shape[0] >= 4 and truth[1].shape[0] == 0
    for i, t in enumerate(truth):
        assert _same(plan.truth_boxes[i, :t.shape[0]].cpu(), t.float())
    # a box lives on one scale: no single label tensor holds the whole list
    assert all(per_scale[s][0].shape[0] < truth[0].shape[0] for s in range(3))
    want, want_ignored, n_band = np.zeros(4), 0, 0
    for s, f in enumerate(plan.fms):
        sub = [anchors[a] for a in masks[s]]
        x = f.torch_view().permute(0, 3, 1, 2).cpu().double().requires_grad_(True)
        info = {}
        parts = M.loss_layer_truth(x, gts[s].cpu().double(), (IMG, IMG, 3), sub, K, 'mse', 1.0, [t.double() for t in truth], thr, info)
        (sum(parts) / float(N)).backward()
        want += np.array([float(p.detach()) for p in parts])
        want_ignored += int(info['ignored'].sum())
        shape = (N, f.h, f.w, len(sub), 5 + K)
        got = f.grad.torch_view().cpu().reshape(shape)
        n_band += _compare_gradient(got, x.grad.permute(0, 2, 3, 1).reshape(shape), info, thr, '%s scale %d dfm' % (name, s))
    _compare_parts(plan.loss4.cpu().numpy(), want, name + ' loss4')
    got_ignored = float(yolo.last_ignored)
    print('%s: ignored %r, NumPy / fp64 count %d, band members %d, longest list %d' % (name, got_ignored, want_ignored, n_band, int(yolo.last_truth_max)))
    assert abs(got_ignored - want_ignored) <= n_band and int(yolo.last_truth_max) == truth[0].shape[0]


def test_model_other_losses_and_accumulation_run(hip):
    """box_loss, focal loss, gradient accumulation, SPP and bf16 inference work on rows or on the spec list: they run and agree
    with themselves (a second model, the same bits)."""
    name = 'A6 1/2/3'
    images, gts = _inputs(name)
    kw = dict(box_loss='ciou', focal_gamma=2.0, focal_alpha=0.25, accumulate_steps=2, grad_clip_norm=10.0, spp=True)
    a, b = _model(name, **kw), _model(name, **kw)
    for step in range(2):
        la, lb = a.train_step((images, gts)), b.train_step((images, gts))
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and bool(torch.isfinite(la))
    assert a.iterations == 1 and torch.equal(a.params, b.params)
    rows = a.predict(images, precision='bf16')
    assert bool(torch.isfinite(rows).all()) and rows.shape[1] == a.number_output_boxes


def test_model_file_round_trip_and_table_mismatch(tmp_path, hip):
    from yolo3.model import YoloV3
    name = 'A6 1/2/3'
    anchors, table = C.PARTITIONS[MODELS[name][0]]
    yolo = _model(name)
    images, gts = _inputs(name)
    yolo.train_step((images, gts))
    path = str(tmp_path / 'w.npz')
    yolo.save_weights(path)
    assert np.load(path)['meta_anchor_scale'].tolist() == table
    back = YoloV3.from_file(path)
    assert back.anchor_scale == table
    assert _same(back.predict(images), yolo.predict(images))
    other = C.PARTITIONS['shuffled'][1]
    assert sorted(other) == sorted(table) and other != table                 # the same head widths, another owner table
    with pytest.raises(ValueError) as e:
        YoloV3(N, [IMG, IMG, 3], 2, anchors, anchor_scales=other).load_weights(path)
    assert str(table) in str(e.value) and str(other) in str(e.value)
    with pytest.raises(ValueError) as e:
        YoloV3(N, [IMG, IMG, 3], 2, anchors).load_weights(path)
    assert str(table) in str(e.value) and 'None' in str(e.value)
    plain = YoloV3(N, [IMG, IMG, 3], 2, anchors)
    plain_path = str(tmp_path / 'p.npz')
    plain.save_weights(plain_path)
    assert 'meta_anchor_scale' not in np.load(plain_path)                   # a file of the reference's network has no such entry
    with pytest.raises(ValueError):
        _model(name).load_weights(plain_path)
    kept = _model(name).load_pretrained(plain_path)                          # heads of another shape keep their initialisation
    assert kept == [i for i, sp in enumerate(yolo.specs) if not sp.bn]


# ---- 5. the default is unchanged -------------------------------------------------------------------------------------------------
def test_default_call_lists_are_the_parents(hip, monkeypatch):
    """A model and a label build without the new arguments launch what they launched before the feature: the recorded entry-point
    names of construction, one train_step, one test_step and one predict (tests/golden/anchor_scales_default_calls.json, recorded on
    the parent commit), and none of the three new entries."""
    from yolo3 import imagereader
    from yolo3.model import YoloV3
    calls = []

    def wrap(fname, fn):
        def recorded(*args):
            calls.append(fname)
            return fn(*args)
        recorded.__name__ = fname
        return recorded
    for fname in hip.SIGNATURES:
        monkeypatch.setattr(hip.lib, fname, wrap(fname, getattr(hip.lib, fname)))
    got = C.default_call_lists(YoloV3, imagereader, calls)
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'anchor_scales_default_calls.json')))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
        assert not any(n.endswith('_scales') for n in got[key])


# ---- 6. the command lines --------------------------------------------------------------------------------------------------------
def test_cli_train_evaluate_infer(tmp_path):
    from PIL import Image
    from test_gpu_box_loss import _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp, 12, (256, 256, 3))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = os.path.join(tmp, 'out')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--batch_size', '2', '--test_every_n_steps', '2', '--train_database',
                        os.path.join(tmp, 'train-syn.lmdb'), '--test_database', os.path.join(tmp, 'test-syn.lmdb'), '--output_dir', out,
                        '--early_stopping', '1', '--use_augmentation', '1', '--max_epochs', '1', '--learning_rate', '1e-4',
                        '--auto_anchors', '9', '--auto_anchors_evolve', '0', '--anchor_assignment', 'scale'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Per-scale anchor assignment' in r.stdout
    rec = json.load(open(os.path.join(out, 'anchor_scales.json')))
    fit = json.load(open(os.path.join(out, 'anchors.json')))
    assert rec['anchors'] == fit['anchors'] and sorted(rec['anchor_scale']) == [0] * 3 + [1] * 3 + [2] * 3
    model_file = os.path.join(out, 'saved_model', 'yolov3.npz')
    assert np.load(model_file)['meta_anchor_scale'].tolist() == rec['anchor_scale']
    imgs, gt = os.path.join(tmp, 'imgs'), os.path.join(tmp, 'gt')
    os.makedirs(imgs)
    os.makedirs(gt)
    rng = np.random.default_rng(3)
    for stem in ('p', 'q'):
        Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(os.path.join(imgs, stem + '.png'))
        with open(os.path.join(gt, stem + '.csv'), 'w') as fh:
            fh.write('X,Y,W,H,C\n5,5,60,60,0\n')
    common = ['--saved-model-filepath', model_file, '--image-folder', imgs, '--image-format', 'png', '--min-box-size', '4']       # no anchor flag
    res = os.path.join(tmp, 'eval.json')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'evaluate.py')] + common + ['--csv-folder', gt, '--output-file', res],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and os.path.exists(res), r.stdout[-3000:] + r.stderr[-3000:]
    det = os.path.join(tmp, 'det')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'inference.py')] + common + ['--output-folder', det],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sorted(os.listdir(det)) == ['p.csv', 'q.csv']
