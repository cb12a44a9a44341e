"""YOLOv3-SPP without a GPU: the spec list and its arena offsets with the option off and on, the restatement of
the block (tests/spp_reference.py) against brute-force window loops, why the forward kernel may cascade 5 o 5, the oracle
network with the block against the plain oracle, the library's exports and plan queries for the new layer's GEMM shape, the
command-line flag, the weight-file entry and the layer map of load_weights(transfer=True)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spp_reference as sr
from oracle import model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
FIELDS = ('cin', 'cin_pad', 'cout', 'k', 's', 'bn', 'w_off', 'b_off', 'g_off', 'be_off', 'end_off', 'bn_idx', 'ch_off', 'mv_off')


def _offsets(specs, align=64):
    """the arena layout rule of build_layer_specs restated over oracle specs: rows of FIELDS and the three totals"""
    up = lambda v: (v + align - 1) // align * align
    rows, off, bn_idx, ch, mv = [], 0, 0, 0, 0
    for sp in specs:
        cin_pad = (sp['cin'] + 3) // 4 * 4
        w_off = off
        b_off = up(w_off + sp['k'] ** 2 * cin_pad * sp['cout'])
        off = up(b_off + sp['cout'])
        if sp['bn']:
            g_off, be_off = off, up(off + sp['cout'])
            off = up(be_off + sp['cout'])
            rows.append((sp['cin'], cin_pad, sp['cout'], sp['k'], sp['s'], True, w_off, b_off, g_off, be_off, off, bn_idx, ch, mv))
            bn_idx, ch, mv = bn_idx + 1, up(ch + 7 * sp['cout']), up(mv + sp['cout'])
        else:
            rows.append((sp['cin'], cin_pad, sp['cout'], sp['k'], sp['s'], False, w_off, b_off, -1, -1, off, -1, -1, -1))
    return rows, (off, ch, mv)


def _rows(specs):
    return [tuple(getattr(sp, f) for f in FIELDS) for sp in specs]


def test_spec_list_with_spp_off_is_the_plain_network():
    from yolo3.model import build_layer_specs
    for cin, a, k in ((3, 2, 2), (1, 3, 80)):
        default = build_layer_specs(cin, a, k)
        off = build_layer_specs(cin, a, k, spp=False)
        want, totals = _offsets(om.layer_specs(cin, a, k))
        assert len(off[0]) == 75
        assert _rows(off[0]) == _rows(default[0]) == want
        assert off[1:] == default[1:] == totals
    assert build_layer_specs(3, 2, 2, spp=False)[1] == 61790400


def test_spec_list_with_spp_on():
    from yolo3.model import ALIGN, build_layer_specs
    specs, arena, chan, moving = build_layer_specs(3, 2, 2, spp=True)
    plain = build_layer_specs(3, 2, 2)[0]
    assert len(specs) == 76
    assert sum(4 if sp.bn else 2 for sp in specs) == 298 and sum(4 if sp.bn else 2 for sp in plain) == 294
    count = lambda L: sum(sp.k * sp.k * sp.cin * sp.cout + sp.cout * (3 if sp.bn else 1) for sp in L)
    assert count(specs) == 62839882 and count(plain) == 61789770
    want, totals = _offsets(sr.spp_layer_specs(3, 2, 2))
    assert _rows(specs) == want and (arena, chan, moving) == totals
    new = specs[sr.spp_layer_index(om.layer_specs(3, 2, 2))]
    assert (new.cin, new.cout, new.k, new.s, new.bn) == (2048, 512, 1, 1, True)
    # the layers around it: 1x1 1024->512, 3x3 512->1024, 1x1 1024->512, [new], 3x3 512->1024, 1x1 1024->512, 3x3 512->1024, head
    assert [(sp.cin, sp.cout, sp.k) for sp in specs[52:60]] == [(1024, 512, 1), (512, 1024, 3), (1024, 512, 1), (2048, 512, 1), (512, 1024, 3),
                                                                 (1024, 512, 1), (512, 1024, 3), (1024, 14, 1)]
    last = 0
    for sp in specs:
        offs = [sp.w_off, sp.b_off] + ([sp.g_off, sp.be_off] if sp.bn else []) + [sp.end_off]
        assert all(o % ALIGN == 0 for o in offs) and offs == sorted(offs) and offs[0] == last and len(set(offs)) == len(offs)
        last = sp.end_off
    assert last == arena
    with pytest.raises(TypeError):
        build_layer_specs(3, 2, 2, True, True)


def _window_data():
    g = torch.Generator().manual_seed(3)
    tied = torch.tensor([-1.0, 0.0, 2.0])[torch.randint(0, 3, (9, 11), generator=g)].double()
    normal = torch.randn(7, 16, generator=g).double()
    flat = torch.zeros(15, 15).double()                      # every window all ties: the first pixel of each window wins
    inf = torch.randn(8, 8, generator=g).double()
    inf[:, :7] = -math.inf                                   # windows that hold nothing but -inf
    inf[2, 7] = math.inf
    row = torch.randn(1, 20, generator=g).double()
    return dict(tied=tied, normal=normal, flat=flat, inf=inf, row=row, single=torch.tensor([[3.0]]).double())


@pytest.mark.parametrize('name', sorted(_window_data()))
def test_restatement_against_window_loops(name):
    """values, and the gradient routed to the FIRST maximum in row-major order of every clipped window"""
    x = _window_data()[name]
    h, w = x.shape
    val, arg = sr.brute_force(x.numpy())
    got = sr.spp_forward(x.reshape(1, h, w, 1))
    assert np.array_equal(got[0].permute(2, 0, 1).numpy(), val)
    g = torch.Generator().manual_seed(h * w)
    dd = torch.randint(-3, 4, (1, h, w, 3), generator=g).double()
    want = np.zeros(h * w)
    for b in range(3):
        np.add.at(want, arg[b].ravel(), dd[0, :, :, b].numpy().ravel())
    ds, terms, mag = sr.spp_backward(x.reshape(1, h, w, 1), dd)
    assert np.array_equal(ds.reshape(-1).numpy(), want)
    cnt = np.zeros(h * w)
    for b in range(3):
        np.add.at(cnt, arg[b].ravel(), 1.0)
    assert np.array_equal(terms.reshape(-1).numpy(), cnt) and float(terms.sum()) == 3 * h * w
    if name == 'flat':      # a 13-window clipped at the top-left corner names pixel (0, 0); one in the middle its own corner
        assert arg[2, 3, 3] == 0 and arg[2, 8, 8] == 2 * 15 + 2 and arg[0, 8, 8] == 6 * 15 + 6


def test_restatement_propagates_nan_and_keeps_infinities():
    x = sr.make_input((2, 9, 10, 4), 'nan')
    val = sr.spp_forward(x)
    for i in range(2):
        for c in range(4):
            want, _ = sr.brute_force(x[i, :, :, c].double().numpy())
            got = val[i, :, :, c::4].permute(2, 0, 1).numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0))
    assert int(torch.isnan(val).sum()) > 2 * 25                 # each NaN spreads over its windows
    x = sr.make_input((1, 8, 8, 4), 'inf')
    val = sr.spp_forward(x)
    assert bool((val[0, :, :, 0] == -math.inf).all()) and bool((val == math.inf).any()) and not bool(torch.isnan(val).any())
    xb = x.to(torch.bfloat16)
    assert torch.equal(sr.spp_forward(xb).float(), val)          # bf16 storage: the same values


@pytest.mark.parametrize('kind', ['normal', 'tied'])
def test_pool5_cascade_gives_pool9_and_pool13(kind):
    """why the forward kernel may compute pool9 = pool5 o pool5 and pool13 = pool5 o pool9: clipped windows of clipped windows
    are the clipped window of the summed radius.  (Not so for the argmax on ties: the backward kernel scans x.)"""
    import torch.nn.functional as F
    for case in ((2, 19, 19, 4), (1, 7, 3, 4), (1, 13, 20, 4)):
        x = sr.make_input(case, kind).permute(0, 3, 1, 2)
        p5, p9, p13 = sr.pools_nchw(x)
        assert torch.equal(F.max_pool2d(p5, 5, 1, 2), p9) and torch.equal(F.max_pool2d(p9, 5, 1, 2), p13)
    # the argmax of the cascade differs on ties: two equal maxima, the later one nearer to the centre of the inner window
    x = torch.zeros(1, 1, 9, 9, dtype=torch.float64)
    x[0, 0, 0, 8] = x[0, 0, 4, 0] = 1.0
    t = x.clone().requires_grad_(True)
    F.max_pool2d(F.max_pool2d(t, 5, 1, 2), 5, 1, 2)[0, 0, 4, 4].backward()
    d = x.clone().requires_grad_(True)
    F.max_pool2d(d, 9, 1, 4)[0, 0, 4, 4].backward()
    assert float(d.grad[0, 0, 0, 8]) == 1.0 and float(t.grad[0, 0, 0, 8]) != 1.0


def test_spp_net_with_identity_pools_is_the_plain_oracle():
    """SppNet whose pools return copies of x and whose new layer passes slice 0 through unchanged computes the plain oracle's
    feature maps on the same remaining weights.  A conv_layer is conv -> leaky-relu -> BatchNorm: with the kernel an identity on
    slice 0, bias B above every |x| (the leaky-relu sees positive numbers only) and BatchNorm(mean B, var 1 - eps, gamma 1,
    beta 0) it returns (x + B) - B."""
    plain = om.init_params(3, 2, 2, seed=4, randomize_bn=True)
    at = sr.spp_layer_index(om.layer_specs(3, 2, 2))
    c, B = 512, 64.0
    W = np.zeros((1, 1, 4 * c, c))
    W[0, 0, :c, :] = np.eye(c)
    ident = dict(W=W, b=np.full(c, B), gamma=np.ones(c), beta=np.zeros(c), mean=np.full(c, B), var=np.full(c, 1.0 - om.BN_EPS))
    net = sr.SppNet(plain[:at] + [ident] + plain[at:], 3, 2, 2, dtype=torch.float64)
    assert len(net.specs) == 76 and net.specs[at]['cin'] == 2048
    seen = []

    def copies(x):
        seen.append(float(x.abs().max()))
        return [x, x, x]
    net.pools = copies
    ref = om.Net(plain, 3, 2, 2, dtype=torch.float64)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        got, want = net.feature_maps(x, training=False), ref.feature_maps(x, training=False)
    assert len(seen) == 1 and seen[0] < B
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())
    # a kernel that reads the pooled slices too, with the real pools: the coarsest map moves, the block is in the graph
    net.p[at]['W'][0, 0, c:, :] = 0.01
    net.pools = sr.pools_nchw
    with torch.no_grad():
        other = net.feature_maps(x, training=False)
    assert float((other[0] - want[0]).abs().max()) > 1e-6 * float(want[0].abs().max())


def test_library_exports_and_plans_the_new_gemm_shape():
    from yolo3 import _hip
    for name in ('y3_spp_fwd', 'y3_spp_fwd_bf16', 'y3_spp_bwd'):
        assert hasattr(_hip.lib, name) and name in _hip.SIGNATURES
    import bf16_routes as br
    import grad_forms as gf
    import plan_forms as pf
    reps = sr.gemm_representatives()
    for entry, ident in (('fwd', pf.sig_id), ('dgrad', pf.sig_id), ('wgrad', gf.sig_id), ('bf16', br.sig_id)):
        assert reps[entry], entry
        for sig, mb in reps[entry]:
            print('%-6s %-60s first at n=%d grid=%d' % (entry, ident(sig), mb.n, mb.h))
    # every (batch, grid) is planned by every entry point in both arithmetics it has (gemm_representatives asserts the rest)
    for n in sr.GEMM_BATCHES:
        for g in sr.GEMM_GRIDS:
            m = n * g * g
            for flags in (0, _hip.CONV_X3):
                p, ws = pf.plan(m, sr.GEMM_CIN, 1, sr.GEMM_COUT, flags)
                assert p[0] > 0 and p[1] > 0 and p[3] == -(-m // p[0]) * -(-sr.GEMM_COUT // p[1]), (n, g, p)
                p, ws = pf.plan(m, sr.GEMM_COUT, 1, sr.GEMM_CIN, flags)
                assert p[3] == -(-m // p[0]) * -(-sr.GEMM_CIN // p[1]), (n, g, p)
                p, ws = gf.wgrad_plan(m, sr.GEMM_CIN, 1, sr.GEMM_COUT, flags)
                assert p[0] > 0 and p[1] > 0 and p[2] >= 1, (n, g, p)
            assert _hip.lib.y3_conv2d_fwd_bf16_workspace(m, sr.GEMM_CIN, 1, sr.GEMM_COUT) >= 0


def test_kernel_arguments_are_checked_on_the_host():
    """refused through the error channel before any launch (no device needed): null tensors, geometry, alignment, the plane limit"""
    from yolo3 import _hip
    lib = _hip.lib
    T = _hip.Tensor
    ok_s, ok_d = T(256, 1, 4, 4, 8, 8), T(512, 1, 4, 4, 24, 24)
    assert lib.y3_spp_fwd(None, ok_d, None) == -1 and b'null' in lib.y3_last_error()
    assert lib.y3_spp_fwd(ok_s, T(512, 1, 4, 4, 16, 16), None) == -1 and b'geometry' in lib.y3_last_error()
    assert lib.y3_spp_fwd(ok_s, T(512, 1, 4, 5, 24, 24), None) == -1
    assert lib.y3_spp_fwd(T(256, 1, 4, 4, 6, 8), T(512, 1, 4, 4, 18, 24), None) == -1 and b'multiples of 4' in lib.y3_last_error()
    assert lib.y3_spp_fwd(T(260, 1, 4, 4, 8, 8), ok_d, None) == -1
    assert lib.y3_spp_fwd_bf16(T(258, 1, 4, 4, 8, 8), ok_d, None) == -1
    assert lib.y3_spp_fwd(ok_s, T(512, 1, 4, 4, 24, 20), None) == -1
    for n, h, w, c in sr.REFUSED_CASES:
        assert h * w > sr.MAX_PLANE
        assert lib.y3_spp_fwd(T(256, n, h, w, c, c), T(512, n, h, w, 3 * c, 3 * c), None) == -1 and str(sr.MAX_PLANE).encode() in lib.y3_last_error()
        assert lib.y3_spp_bwd(T(256, n, h, w, c, c), T(512, n, h, w, 3 * c, 3 * c), T(1024, n, h, w, c, c), 0, None) == -1
    assert lib.y3_spp_bwd(ok_s, ok_d, None, 0, None) == -1 and b'dsrc' in lib.y3_last_error()
    assert lib.y3_spp_bwd(ok_s, ok_d, T(1024, 1, 4, 4, 4, 8), 1, None) == -1
    text = open(os.path.join(ROOT, 'include', 'yolo3hip.h')).read()
    assert '#define Y3_SPP_MAX_PLANE %d' % sr.MAX_PLANE in text
    # the case list has a plane on each side of every boundary of the implementation
    planes = {h * w for _, h, w, _ in sr.KERNEL_CASES}
    for edge in (sr.SMALL_PLANE, sr.LDS_DEFAULT_PIXELS):
        assert edge in planes and any(edge < p <= edge + 64 for p in planes), edge
    assert sr.MAX_PLANE in planes and all(p <= sr.MAX_PLANE for p in planes)
    src = open(os.path.join(PKG, 'csrc', 'spp.hip')).read()
    assert '#define SPP_SMALL_OWN 2' in src and '#define SPP_THREADS 256' in src and '#define SPP_DEFAULT_LDS 65536' in src
    assert sr.SMALL_PLANE == 2 * 256 and sr.LDS_DEFAULT_PIXELS * 32 == 65536


def test_train_cli_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--help'], capture_output=True, text=True, check=True).stdout
    assert '--spp {0,1}' in out
    sys.path.insert(0, PKG)
    import train
    p = train.build_parser()
    acts = {a.dest: a for a in p._actions}
    assert acts['spp'].default == 0 and tuple(acts['spp'].choices) == (0, 1)
    import inspect
    assert inspect.signature(train.train_model).parameters['spp'].default is False
    for cli in ('inference.py', 'inference_tiled.py', 'evaluate.py'):      # they take the setting from the saved model
        assert '--spp' not in open(os.path.join(PKG, cli)).read()


class _Stub:
    """what YoloV3.save_weights / load_weights read before they touch a device"""

    def __init__(self, spp):
        self.spp = spp
        self.img_size, self.number_classes, self.anchors = [64, 64, 3], 2, [(64, 384), (384, 64)]
        self.global_batch_size, self.learning_rate, self.iterations = 2, 1e-4, 0
        self.adam_m = self.adam_v = torch.zeros(4)

    def get_weights(self, moving=None):
        return [dict(W=np.zeros((1, 1, 1, 1), np.float32), b=np.zeros(1, np.float32))]

    def focal_args(self):
        return None


def test_weight_file_records_the_setting(tmp_path):
    from yolo3.model import YoloV3
    for spp in (False, True):
        path = str(tmp_path / ('w%d.npz' % spp))
        YoloV3.save_weights(_Stub(spp), path)
        z = np.load(path)
        assert ('meta_spp' in z) == spp and YoloV3._spp_meta(z) is spp      # a file without the entry is the plain network
    for mine, theirs in ((False, True), (True, False)):
        with pytest.raises(ValueError) as e:
            YoloV3.load_weights(_Stub(mine), str(tmp_path / ('w%d.npz' % theirs)))
        assert 'spp=%s' % theirs in str(e.value) and 'spp=%s' % mine in str(e.value)
    with pytest.raises(ValueError):      # transfer goes one way: a plain file into an SPP model
        YoloV3.load_weights(_Stub(False), str(tmp_path / 'w0.npz'), transfer=True)
    with pytest.raises(ValueError):
        YoloV3.load_weights(_Stub(True), str(tmp_path / 'w1.npz'), transfer=True)


def test_transfer_maps_layers_by_role():
    from yolo3.model import build_layer_specs, spp_transfer_map
    for cin, a, k in ((3, 2, 2), (3, 2, 59), (1, 3, 80)):      # (2 anchors x 64 = 128 head channels: 4 x 128 = 512, a lateral layer's width)
        new, old = build_layer_specs(cin, a, k, spp=True)[0], build_layer_specs(cin, a, k)[0]
        m = spp_transfer_map(new)
        assert len(m) == 76 and m.count(None) == 1
        fresh = m.index(None)
        assert fresh == 55 and (new[fresh].cin, new[fresh].cout, new[fresh].k) == (2048, 512, 1)
        assert m[:fresh] == list(range(fresh)) and m[fresh + 1:] == list(range(fresh, 75))
        for i, j in enumerate(m):
            if j is not None:
                assert (new[i].cin, new[i].cout, new[i].k, new[i].s, new[i].bn) == (old[j].cin, old[j].cout, old[j].k, old[j].s, old[j].bn)
    with pytest.raises(ValueError):
        spp_transfer_map(build_layer_specs(3, 2, 2)[0])


def test_constructor_checks_the_keyword_before_the_device():
    from yolo3.model import YoloV3
    with pytest.raises(ValueError):
        YoloV3(2, [64, 64, 3], 2, spp='yes')
    with pytest.raises(ValueError):
        YoloV3(2, [64, 64, 3], 2, spp=2)
