"""CPU tests of anchor fitting: yolo3/anchors.py on device='cpu' against imagereader.format_boxes (the assignment)
and tests/anchors_reference.py (the sums), the fit's guarantees, the files and flags, the refused C-ABI calls that need no device,
and the unchanged default mode of find_anchor_sizes.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import anchors_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'object-detection-yolov3_amd')
Q1 = 1 << 24


def _format_boxes_slot(w, h, anchors):
    """The anchor slot imagereader.format_boxes sets for one box of size (w, h) in a frame large enough to hold it."""
    from yolo3.imagereader import format_boxes
    side = 32 * (max(int(w), int(h)) // 32 + 2)
    labels = format_boxes(np.array([[0, 0, w, h, 0]], np.int32), (side, side, 3), anchors, 1)
    slots = np.nonzero(labels[0][..., 4].sum(axis=(0, 1)))[0]
    assert len(slots) == 1
    for lab in labels[1:]:
        assert np.array_equal(np.nonzero(lab[..., 4].sum(axis=(0, 1)))[0], slots)      # the SAME slot at all three scales
    return int(slots[0])


@pytest.mark.parametrize('k', [1, 2, 9, 16])
def test_labels_are_the_slots_format_boxes_sets(k):
    from yolo3.anchors import anchor_stats
    rng = np.random.default_rng(100 + k)
    wh = rng.integers(1, 400, (60, 2))
    anchors = (rng.random((k, 2)) * 300 + 2).astype(np.float32)
    _, skipped, labels = anchor_stats(wh, anchors, labels=True)
    assert skipped == 0
    for (w, h), lab in zip(wh.tolist(), labels.tolist()):
        assert lab == _format_boxes_slot(w, h, [tuple(a) for a in anchors.tolist()])


def test_ties_take_the_first_anchor():
    from yolo3.anchors import anchor_stats
    # a 100 x 100 box overlaps (64, 384) and (384, 64) equally: format_boxes (np.argmax) takes slot 0
    pair = [(64, 384), (384, 64)]
    st, _, labels = anchor_stats(np.array([[100, 100]]), pair, per_anchor=True, labels=True)
    assert labels.tolist() == [0] and _format_boxes_slot(100, 100, pair) == 0
    assert st[0, :, 0].tolist() == [1, 0]
    # a box equal to two identical anchors (q = 2^24 for both): slot 1 is the first of the two
    trio = [(10, 10), (30, 50), (30, 50)]
    st, _, labels = anchor_stats(np.array([[30, 50]]), trio, per_anchor=True, labels=True, thr_q=Q1)
    assert labels.tolist() == [1] and _format_boxes_slot(30, 50, trio) == 1
    assert st[0, 1].tolist() == [1, 30, 50, Q1, 1]


@pytest.mark.parametrize('thr_q', [0, 1 << 23, 1 << 24])
@pytest.mark.parametrize('P,k', [(1, 1), (1, 16), (3, 9), (5, 2)])
def test_stats_equal_the_plain_loop_reference(P, k, thr_q):
    from yolo3.anchors import anchor_stats
    rng = np.random.default_rng(7 * P + k)
    cands = (rng.random((P, k, 2)) * 200 + 1).astype(np.float32)
    cands[0, 0] = (37, 21)                                      # an anchor that a box equals: q = 2^24, counted at thr_q = 2^24
    wh = np.concatenate([rng.integers(1, 300, (150, 2)), [[37, 21], [1, 1], [65535, 65535], [1, 65535], [65535, 1]],
                         [[0, 5], [5, 0], [-3, 7], [7, -1], [65536, 10], [10, 65536]]]).astype(np.int64)
    wh = wh[rng.permutation(len(wh))]
    for per_anchor in (True, False):
        want, want_skipped, want_labels = ref.stats(wh, cands, thr_q, per_anchor)
        if P == 1:
            got, skipped, labels = anchor_stats(wh, cands, per_anchor=per_anchor, labels=True, thr_q=thr_q)
            assert labels.dtype == np.uint8 and labels.tolist() == want_labels
        else:
            got, skipped = anchor_stats(wh, cands, per_anchor=per_anchor, thr_q=thr_q)
        assert got.dtype == np.int64 and got.shape == ((P, k, 5) if per_anchor else (P, 2))
        assert got.tolist() == want and skipped == want_skipped == 6
    hit = ref.stats(np.array([[37, 21]]), cands[:1], thr_q, False)[0]
    assert hit[0] == [Q1, 1]


def test_iou_q_is_the_reference_expression():
    from yolo3.anchors import iou_q
    rng = np.random.default_rng(3)
    wh = rng.integers(1, 2000, (40, 2))
    anchors = (rng.random((5, 2)) * 500 + 1).astype(np.float32)
    q = iou_q(wh, anchors)
    assert q.shape == (40, 5) and q.dtype == np.int32
    for i in range(40):
        for a in range(5):
            assert int(q[i, a]) == ref.q_of(ref.iou(wh[i, 0], wh[i, 1], anchors[a, 0], anchors[a, 1]))


def test_fit_recovers_three_exact_sizes():
    from yolo3.anchors import fit_anchors
    wh = np.array([(12, 12)] * 50 + [(40, 90)] * 31 + [(200, 60)] * 7)
    wh = wh[np.random.default_rng(1).permutation(len(wh))]
    fit = fit_anchors(wh, 3)
    assert fit['anchors'] == [[12.0, 12.0], [40.0, 90.0], [200.0, 60.0]]
    assert fit['fitness'] == 1.0 and fit['recall'] == 1.0 and fit['sum_q'] == len(wh) * Q1
    assert [r['count'] for r in fit['table']] == [50, 31, 7]


@pytest.fixture(scope='module')
def mixture():
    return ref.mixture()


@pytest.fixture(scope='module')
def mixture_fit(mixture):
    from yolo3.anchors import fit_anchors
    return fit_anchors(mixture, 4, seed=0)


def test_fit_on_the_mixture_never_loses_ground(mixture, mixture_fit):
    """20 000 sizes around four centres (anchors_reference.mixture), k = 4, seed 0, the default settings.  Checked on the CPU for this
    seed before relying on the strict inequalities: the Euclidean centres score sum q / (n 2^24) = 0.48525, IoU k-means reaches
    0.69179 and the 1000-mutant search 0.69220 (16 generations, the elite improved in several of them)."""
    from yolo3.anchors import anchor_stats
    fit = mixture_fit
    n = len(mixture)
    hist = fit['history']
    assert len(hist) == 16 and all(b >= a for a, b in zip(hist, hist[1:])) and hist[0] >= fit['lloyd_sum_q']
    assert fit['sum_q'] == hist[-1] and fit['fitness'] == fit['sum_q'] / (n * float(Q1))
    assert len(fit['start_sum_q']) == 9 and all(fit['sum_q'] >= s for s in fit['start_sum_q'])
    euclid = fit['start_sum_q'][-1]
    assert fit['sum_q'] > euclid
    assert fit['sum_q'] > fit['lloyd_sum_q']                                        # the search alone gained
    # the Euclidean start set is what find_anchor_sizes' kmeans returns, and the report is what anchor_stats says of the result
    import find_anchor_sizes
    centers = find_anchor_sizes.kmeans(mixture[:, ::-1].astype(np.float64), 4, np.random.default_rng(0))[0]
    st, _ = anchor_stats(mixture, centers[:, ::-1].astype(np.float32))
    assert int(st[0, 0]) == euclid
    st, _ = anchor_stats(mixture, fit['anchors'], per_anchor=True)
    assert int(st[0, :, 3].sum()) == fit['sum_q'] and [int(c) for c in st[0, :, 0]] == [r['count'] for r in fit['table']]
    assert fit['recall'] == int(st[0, :, 4].sum()) / n
    areas = [a[0] * a[1] for a in fit['anchors']]
    assert areas == sorted(areas)


def test_fit_is_reproducible_and_seeded(mixture, mixture_fit):
    from yolo3.anchors import fit_anchors
    small = mixture[:3000]
    a = fit_anchors(small, 4, seed=5, evolve=256)
    b = fit_anchors(small, 4, seed=5, evolve=256)
    c = fit_anchors(small, 4, seed=6, evolve=256)
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert a['history'] != c['history'] or a['start_sum_q'] != c['start_sum_q']
    assert fit_anchors(small, 4, seed=5, evolve=0)['history'] == []
    # sizes times 2, fitted: the same as fitting with scale = 2
    assert fit_anchors(small * 2, 4, seed=5, evolve=64)['anchors'] == fit_anchors(small, 4, seed=5, evolve=64, scale=2.0)['anchors']


def test_fit_refuses_too_few_distinct_sizes():
    from yolo3.anchors import fit_anchors
    wh = np.array([(10, 10)] * 5 + [(20, 30)] * 5)
    with pytest.raises(ValueError, match='distinct'):
        fit_anchors(wh, 3)
    assert len(fit_anchors(wh, 2)['anchors']) == 2
    with pytest.raises(ValueError):
        fit_anchors(wh, 17)
    with pytest.raises(ValueError):
        fit_anchors(wh, 2, population=1024)


def test_anchor_files_and_flags(tmp_path, mixture_fit):
    from yolo3.anchors import anchors_flag, load_anchors, parse_anchor_args, save_anchors
    path = str(tmp_path / 'anchors.json')
    save_anchors(path, mixture_fit)
    assert load_anchors(path) == mixture_fit
    assert isinstance(json.load(open(path)), dict)
    # the printed flag reads back as the same float32 anchors
    flag = anchors_flag(mixture_fit['anchors']).split()
    assert flag[0] == '--anchors'
    assert np.array_equal(np.asarray(parse_anchor_args(flag[1:]), np.float32), np.asarray(mixture_fit['anchors'], np.float32))
    assert parse_anchor_args(['10,14', '23,27']) == [(10, 14), (23, 27)]
    assert parse_anchor_args(['10.5,14']) == [(10.5, 14)]
    for bad in (['10'], ['10,14,3'], ['a,b'], ['10,'], ['0,5'], ['-3,5'], ['5,nan'], ['5,inf'], [], ['3,4'] * 17):
        with pytest.raises(ValueError):
            parse_anchor_args(bad)
    assert len(parse_anchor_args(['3,4'] * 16)) == 16
    (tmp_path / 'bad.json').write_text('{"settings": {}}')
    with pytest.raises(ValueError):
        load_anchors(str(tmp_path / 'bad.json'))


def test_train_flags_exclude_each_other(tmp_path, capsys):
    import train
    base = ['--train_database', 'a', '--test_database', 'b', '--output_dir', 'c']
    p = train.build_parser()
    a = p.parse_args(base)
    assert a.anchors is None and a.anchors_file is None and a.auto_anchors is None
    assert p.parse_args(base + ['--anchors', '20,30', '60,40']).anchors == ['20,30', '60,40']
    assert p.parse_args(base + ['--auto_anchors', '3', '--auto_anchors_device', 'gpu', '--auto_anchors_evolve', '0']).auto_anchors == 3
    for bad in (['--anchors', '20,30', '--anchors_file', 'f.json'], ['--anchors', '20,30', '--auto_anchors', '3'],
                ['--anchors_file', 'f.json', '--auto_anchors', '3'], ['--anchors', '20;30'], ['--anchors', '0,3'], ['--auto_anchors', '17'],
                ['--auto_anchors', '0'], ['--auto_anchors_evolve', '10'], ['--auto_anchors_device', 'gpu'], ['--anchors'] + ['3,4'] * 17):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
    capsys.readouterr()
    # the resolution train_model runs before its readers: the reference's pair by default, the flag's, a file's, a host fit
    out = str(tmp_path)
    assert train.resolve_anchors(None, None, None, 'unused', out) == [(64, 384), (384, 64)]
    assert train.resolve_anchors(['20,30', '60,40'], None, None, 'unused', out) == [(20, 30), (60, 40)]
    assert train.resolve_anchors([(20, 30), (60, 40)], None, None, 'unused', out) == [(20, 30), (60, 40)]
    with pytest.raises(ValueError):
        train.resolve_anchors(['20,30'], 'f.json', None, 'unused', out)
    with pytest.raises(ValueError):
        train.train_model(2, 1, 'a', 'b', out, 1, 1e-4, False, anchors=['1,2'], auto_anchors=2)


def test_auto_anchors_on_the_host_reads_the_training_lmdb(tmp_path, capsys):
    import train
    from test_cpu_dataplane import _make_db
    from yolo3.anchors import fit_anchors, load_anchors, load_sizes_lmdb
    path, truth = _make_db(tmp_path, n=12, size=(64, 64, 3), seed=3)
    wh = load_sizes_lmdb(path)
    want = np.concatenate([np.asarray(truth[k][1]).reshape(-1, 5)[:, 2:4] for k in sorted(truth)])
    assert np.array_equal(wh, want) and len(wh) > 3
    out = tmp_path / 'out'
    out.mkdir()
    got = train.resolve_anchors(None, None, 2, path, str(out), evolve=128, seed=4)
    fit = fit_anchors(wh, 2, seed=4, evolve=128)
    assert got == [tuple(a) for a in fit['anchors']]
    assert load_anchors(str(out / 'anchors.json')) == fit
    assert '--anchors ' in capsys.readouterr().out
    # another rank computes the same anchors and writes nothing
    other = tmp_path / 'other'
    other.mkdir()
    assert train.resolve_anchors(None, None, 2, path, str(other), rank=1, evolve=128, seed=4) == got and not os.listdir(str(other))
    assert train.resolve_anchors(None, str(out / 'anchors.json'), None, 'unused', str(other)) == got


def test_refused_calls_launch_nothing():
    """Every refusal is decided before the first HIP call: -1 and a message, without a device."""
    from yolo3._hip import lib
    one = ctypes.c_void_p(4096)          # never dereferenced: the calls below are refused first

    def call(wh=one, n=10, cand=one, P=1, k=2, thr_q=0, per_anchor=1, out=one, labels=None, ws=one):
        return lib.y3_anchor_stats(wh, n, cand, P, k, thr_q, per_anchor, out, labels, ws, None), lib.y3_last_error().decode()

    for kw, word in ((dict(k=0), 'k 0'), (dict(k=17), 'k 17'), (dict(P=0), 'P 0'), (dict(P=1025, k=1), 'P * k'), (dict(P=65, k=16), 'P * k'),
                     (dict(n=0), 'n 0'), (dict(n=1 << 31), 'n 2147483648'), (dict(thr_q=-1), 'thr_q'), (dict(thr_q=(1 << 24) + 1), 'thr_q'),
                     (dict(labels=one, P=2), 'labels'), (dict(wh=None), 'null'), (dict(cand=None), 'null'), (dict(out=None), 'null'),
                     (dict(ws=None), 'null'), (dict(wh=ctypes.c_void_p(4100)), 'aligned')):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert lib.y3_anchor_stats_workspace_bytes(1, 1) == 512 * 6 * 8
    assert lib.y3_anchor_stats_workspace_bytes(64, 16) == 512 * (64 * 16 * 5 + 1) * 8
    assert lib.y3_anchor_stats_workspace_bytes(65, 16) == 0 and lib.y3_anchor_stats_workspace_bytes(1, 17) == 0


def _write_csv_folder(folder):
    """The folder of test_cpu_dataplane.test_find_anchor_sizes_recovers_clusters."""
    from yolo3 import bbox_utils
    rng = np.random.default_rng(0)
    true = np.array([[40, 30], [120, 200], [300, 280]])
    for f in range(4):
        rows = []
        for c, (h, w) in enumerate(true):
            for _ in range(25):
                rows.append([int(rng.integers(0, 500)), int(rng.integers(0, 500)), int(w + rng.integers(-5, 6)), int(h + rng.integers(-5, 6)), c])
        bbox_utils.write_boxes_from_xywhc(np.asarray(rows, np.int32), os.path.join(folder, 'a%d.csv' % f))


def test_tool_without_new_flags_prints_what_it_printed(tmp_path):
    """find_anchor_sizes.py --csv_dirpath F (seed 0): the score lines and centres below were printed by the tool before it learnt
    --metric iou."""
    _write_csv_folder(str(tmp_path))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'find_anchor_sizes.py'), '--csv_dirpath', str(tmp_path)], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if 'matplotlib is not installed' not in ln]
    assert lines == LEGACY_LINES
    # the new flags are refused without --metric iou, and the new mode needs --k
    import find_anchor_sizes
    for extra in (['--k', '3'], ['--device', 'cpu'], ['--output', 'x.json'], ['--metric', 'iou'], ['--metric', 'iou', '--k', '3', '--database', 'd']):
        with pytest.raises(SystemExit) as e:
            find_anchor_sizes.main(['--csv_dirpath', str(tmp_path)] + extra)
        assert e.value.code == 2, extra


def test_tool_iou_mode_prints_the_table_and_the_flag(tmp_path, capsys):
    import find_anchor_sizes
    from yolo3.anchors import fit_anchors, load_anchors, load_sizes_csv
    _write_csv_folder(str(tmp_path))
    out = str(tmp_path / 'anchors.json')
    fit = find_anchor_sizes.main(['--csv_dirpath', str(tmp_path), '--metric', 'iou', '--k', '3', '--evolve', '128', '--seed', '2', '--output', out])
    wh = load_sizes_csv(str(tmp_path))
    assert wh.shape == (300, 2) and np.array_equal(wh[:, ::-1], find_anchor_sizes.load_sizes(str(tmp_path)).astype(np.int64))
    assert fit == fit_anchors(wh, 3, seed=2, evolve=128) == load_anchors(out)
    text = capsys.readouterr().out
    assert 'mean IoU' in text and text.count(' x ') == 1 + 3 and '\n--anchors ' in text      # the header and one row per anchor
    centres = np.asarray(fit['anchors'])
    assert np.abs(centres - np.array([[30, 40], [200, 120], [280, 300]])).max() < 4.0


_VIEW = 'View the scatterplot and determine if the clusters look appropriate. You generally want a small, medium, and large anchor for Yolo.'
LEGACY_LINES = [
    'score for 2-means = -1765952.005', '  centers = [[ 80.31  114.775]', ' [299.84  279.53 ]]', _VIEW,
    'score for 3-means = -6008.84', '  centers = [[120.45 199.56]', ' [ 40.17  29.99]', ' [299.84 279.53]]', _VIEW,
    'score for 4-means = -5131.217998130342', '  centers = [[299.84       279.53      ]', ' [ 41.55769231  32.46153846]',
    ' [120.45       199.56      ]', ' [ 38.66666667  27.3125    ]]', _VIEW,
    'score for 5-means = -4301.547222474924', '  centers = [[ 38.95918367  27.2244898 ]', ' [299.84       279.53      ]',
    ' [122.63333333 200.33333333]', ' [ 41.33333333  32.64705882]', ' [117.175      198.4       ]]', _VIEW,
    'score for 6-means = -3833.237733415044', '  centers = [[123.19230769 199.82692308]', ' [299.84       279.53      ]',
    ' [ 38.7755102   27.30612245]', ' [ 41.50980392  32.56862745]', ' [117.65384615 196.38461538]', ' [117.27272727 202.68181818]]', _VIEW,
    'score for 7-means = -3062.480531729889', '  centers = [[ 38.88        27.32      ]', ' [297.63636364 280.83636364]',
    ' [123.23809524 198.9047619 ]', ' [ 41.46        32.66      ]', ' [119.19354839 203.09677419]', ' [302.53333333 277.93333333]',
    ' [117.55555556 196.51851852]]', _VIEW]
