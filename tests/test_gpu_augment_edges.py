"""y3_augment_batch (csrc/augment.hip) at its edges, through the C ABI with buffers the test owns: every case table of
tests/augment_edges.py against the fp64 restatement of include/yolo3hip.h within the derived per-element bound; the min / max
keys; a 256-byte canary behind `out` and behind the workspace; NaN pre-fill (every element is written); bits where the contract
says bits (exact copies, radius 0, u_noise = 0.5, a constant image under noise, a record alone against the same record in a
batch of 40, a second run).

Y3_AUGMENT_ERR=<file> writes the worst error / bound of every (table, pass) of the run and the measured worst
|device normal - fp64 twin| to <file> (profiles/augment_edges_err.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

import augment_edges as ae

pytestmark = pytest.mark.gpu
CANARY = 256


@pytest.fixture(scope='module')
def hip():
    from yolo3 import _hip
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    yield _hip
    path = os.environ.get('Y3_AUGMENT_ERR')
    if path:
        with open(path, 'w') as f:
            f.write('# worst |error| / bound per table and pass, and the case, record and element (ch, y, x) that gave it (tests/test_gpu_augment_edges.py)\n')
            for (table, name), (r, cid, rec_i, where) in sorted(ae.RATIOS.items()):
                f.write('%-8s %-12s %.3f  %-34s record %-3d %s\n' % (table, name, r, cid, rec_i, where))
            f.write('\n# worst |device normal - fp64 twin| over the noise-only records with |s| >= 1 % of the range, and the resolution of the\n'
                    '# measurement (the fp32 roundings of s and of x + s z, divided by |s|)\n')
            for cid, (dev, res) in sorted(ae.NORMAL_DEV.items()):
                f.write('%-34s %.3e  (resolution %.1e)\n' % (cid, dev, res))
            if ae.NORMAL_DEV:
                f.write('%-34s %.3e\n' % ('all', max(d for d, _ in ae.NORMAL_DEV.values())))


def _ids(cases):
    return [c['id'] for c in cases]


def _run(hip, case, only=None):
    """One y3_augment_batch call on buffers of the test's own: `out` pre-filled with NaN, the workspace with 0xFF, each followed
    by 256 bytes of 0xA5 that must survive.  only: run record `only` alone, in a batch of one.
    Returns out [n, C, H, W] float32 (numpy), max [n], min [n] (decoded keys)."""
    lib = hip.lib
    idx = list(range(len(case['records']))) if only is None else [only]
    recs = np.ascontiguousarray(np.stack([case['records'][i] for i in idx]))
    imgs = np.ascontiguousarray(ae.case_images(case)[idx])
    n, (H, W), C = len(idx), case['crop'], case['C']
    src = torch.from_numpy(imgs.view(np.uint8).reshape(-1).copy()).cuda()
    out_bytes = n * C * H * W * 4
    outb = torch.full((out_bytes + CANARY,), 0xA5, dtype=torch.uint8, device='cuda')
    outb[:out_bytes].view(torch.float32).fill_(float('nan'))
    ws_bytes = int(lib.y3_augment_workspace_bytes(n, H, W, C))
    assert ws_bytes >= 8 * n + out_bytes
    ws = torch.full((ws_bytes + CANARY,), 0xA5, dtype=torch.uint8, device='cuda')
    ws[:ws_bytes] = 0xFF
    st = torch.cuda.current_stream().cuda_stream
    hip.check(lib.y3_augment_batch(src.data_ptr(), ae.DTYPE_CODE[case['dtype']], n, case['h_in'], case['w_in'], C, recs.ctypes.data, H, W, outb.data_ptr(),
                                   ws.data_ptr(), st), 'y3_augment_batch ' + case['id'])
    torch.cuda.synchronize()
    assert bool((outb[out_bytes:] == 0xA5).all()), case['id'] + ': wrote behind out'
    assert bool((ws[ws_bytes:] == 0xA5).all()), case['id'] + ': wrote behind the workspace'
    out = outb[:out_bytes].view(torch.float32).view(n, C, H, W).cpu().numpy()
    assert np.isfinite(out).all(), case['id'] + ': an output element was not written'
    keys = ws[:8 * n].cpu().numpy().view(np.uint32).reshape(n, 2)
    return out, ae.decode_key(keys[:, 0]), -ae.decode_key(keys[:, 1])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _compare(case, out, mx, mn):
    """every record of the batch against chain_full, its keys against the intervals, the bit-exact relations of its flags"""
    fails = []
    for i, flags in enumerate(case['flags']):
        full = ae.case_full(case, i)
        ae.check(case['table'], full['kind'], case['id'], i, out[i], full['want'], full['bound'], fails)
        for name, got, (lo, hi) in (('max', float(mx[i]), full['mx_iv']), ('min', float(mn[i]), full['mn_iv'])):
            mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
            ae.check(case['table'], 'minmax', case['id'], i, np.array([got]), np.array([mid]), np.array([half]), fails)
        if flags.get('exact_copy') and not np.array_equal(_bits(out[i]), _bits(ae.exact_copy_bits(case, i))):
            fails.append('%s record %d: an exact copy is not bit-exact' % (case['id'], i))
        j = flags.get('same_bits_as')
        if j is not None and not np.array_equal(_bits(out[i]), _bits(out[j])):
            fails.append('%s record %d: not the bits of record %d' % (case['id'], i, j))
    return fails


def _run_and_compare(hip, case):
    out, mx, mn = _run(hip, case)
    fails = _compare(case, out, mx, mn)
    assert not fails, '\n'.join(fails)
    return out


@pytest.mark.parametrize('case', ae.SEAM_CASES, ids=_ids(ae.SEAM_CASES))
def test_row_pass_across_the_segment_seams(hip, case):
    _run_and_compare(hip, case)


@pytest.mark.parametrize('case', ae.COLUMN_CASES, ids=_ids(ae.COLUMN_CASES))
def test_column_pass_across_the_tile_edges(hip, case):
    _run_and_compare(hip, case)


@pytest.mark.parametrize('case', ae.TINY_CASES, ids=_ids(ae.TINY_CASES))
def test_axes_shorter_than_the_blur_radius(hip, case):
    _run_and_compare(hip, case)


@pytest.mark.parametrize('case', ae.SOURCE_CASES, ids=_ids(ae.SOURCE_CASES))
def test_tiny_unaligned_and_far_rescaled_sources(hip, case):
    _run_and_compare(hip, case)


def test_the_largest_accepted_source_row(hip):
    """one pixel more is refused: tests/test_cpu_augment_device.py"""
    _run_and_compare(hip, ae.WIDE_CASE)


@pytest.mark.parametrize('case', ae.SIGNED_CASES, ids=_ids(ae.SIGNED_CASES))
def test_signed_and_constant_images(hip, case):
    out = _run_and_compare(hip, case)
    if case['source'].startswith('const'):
        assert np.unique(out[0]).tolist() == [37.5 if case['source'] == 'const+' else -37.5]


@pytest.mark.parametrize('case', ae.NOISE_CASES, ids=_ids(ae.NOISE_CASES))
def test_noise_index_over_dtypes_channels_flips_and_seeds(hip, case):
    """and the device's N(0,1) against the fp64 twin: (noisy - the same record without noise) / s, where |s| is large enough
    for the fp32 roundings of s and of x + s z to stay three orders below NORMAL_TOL"""
    out, mx, mn = _run(hip, case)
    fails = _compare(case, out, mx, mn)
    worst, res = 0.0, 0.0
    for i, flags in enumerate(case['flags']):
        full = ae.case_full(case, i)
        rng = full['mx'] - full['mn']
        if full['kind'] != 'noise' or abs(full['s']) < 0.01 * rng:
            continue
        z = (out[i].astype(np.float64) - out[flags['plain']]) / full['s']
        worst = max(worst, float(np.abs(z - full['z']).max()))
        width = (full['mx_iv'][1] - full['mx_iv'][0]) + (full['mn_iv'][1] - full['mn_iv'][0])
        res = max(res, float(((np.abs(full['base']) + np.abs(full['s'] * full['z'])) * ae.ku(1) / abs(full['s']) + np.abs(full['z']) * (ae.ku(3) + width / rng)).max()))
    ae.NORMAL_DEV[case['id']] = (worst, res)
    assert worst <= ae.NORMAL_TOL, (case['id'], worst)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('case', ae.RADIUS_CASES, ids=_ids(ae.RADIUS_CASES))
def test_every_radius_step(hip, case):
    """sigma 2.125 (radius 9) is refused: tests/test_cpu_augment_device.py"""
    _run_and_compare(hip, case)


@pytest.mark.parametrize('case', ae.MIXED_BATCH, ids=_ids(ae.MIXED_BATCH))
def test_second_launch_chunk_with_every_kind_of_record(hip, case):
    """40 images: each against the restatement, and bit for bit against the same record alone in a batch of one"""
    out, mx, mn = _run(hip, case)
    fails = _compare(case, out, mx, mn)
    for i in range(len(case['records'])):
        solo, smx, smn = _run(hip, case, only=i)
        if not (np.array_equal(_bits(solo[0]), _bits(out[i])) and _bits(smx)[0] == _bits(mx[i:i + 1])[0] and _bits(smn)[0] == _bits(mn[i:i + 1])[0]):
            fails.append('%s record %d (%s): the batch of 40 and the batch of one differ' % (case['id'], i, case['flags'][i]['kind']))
    assert not fails, '\n'.join(fails)


def test_the_same_input_gives_the_same_bits(hip):
    """a second run on fresh buffers: the mixed batch (in-place noise-only records, blurred ones through the workspace), a seam
    case and a noise case"""
    for case in (ae.MIXED_BATCH[2], ae.CASES_BY_ID['seam-3x513-c3'], ae.NOISE_CASES[1]):
        a, amx, amn = _run(hip, case)
        b, bmx, bmn = _run(hip, case)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(amx), _bits(bmx)) and np.array_equal(_bits(amn), _bits(bmn)), case['id']
