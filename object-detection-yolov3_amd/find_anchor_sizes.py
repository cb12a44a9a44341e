#!/usr/bin/env python3
"""find_anchor_sizes.py -- cluster the (height, width) of every annotated box to suggest YOLO anchors.
Reference: find_anchor_sizes.py:19-66 (same flag, same printed lines: a score and the centres for k = 2..7).

The reference delegates to sklearn.cluster.KMeans (unseeded) and saves matplotlib scatter plots.  This is an offline
host utility outside the GPU path, so it is plain NumPy: k-means++ seeding + Lloyd iterations, best of `n_init`
restarts, `score` = minus the within-cluster sum of squares (what KMeans.score returns).  Being unseeded in the
reference, its centres are only defined up to the usual k-means local optima; here the seed is a flag.  Plots are
written only when matplotlib is importable.

Addition (--metric iou): Euclidean distance favours large boxes, and it is not the criterion that assigns a box to an
anchor in training (the IoU of the co-centred sizes).  `--metric iou --k K` fits K anchors to that criterion with
yolo3.anchors.fit_anchors (IoU k-means, then a mutation search; scored on the host or, --device gpu, by a HIP kernel with the same
result) and prints the --anchors string for train.py.  Without --metric the tool does exactly what it did."""
import argparse
import os

import numpy as np

from yolo3 import bbox_utils
from yolo3.anchors import kmeans      # noqa: F401  (the Euclidean k-means of this tool: fit_anchors puts its centres into the start pool)


def load_sizes(csv_dirpath):
    """[n,2] = (H, W) of every box of every csv in the folder (find_anchor_sizes.py:20-30)."""
    h_list, w_list = [], []
    for fn in sorted(f for f in os.listdir(csv_dirpath) if f.endswith('.csv')):
        boxes = bbox_utils.load_boxes_to_xywhc(os.path.join(csv_dirpath, fn))
        w_list.extend(boxes[:, 2].tolist())
        h_list.extend(boxes[:, 3].tolist())
    return np.stack([np.asarray(h_list, np.float64), np.asarray(w_list, np.float64)], axis=1).reshape(-1, 2)


def find_anchors(csv_dirpath, seed=0, plot=True):
    X = load_sizes(csv_dirpath)
    rng = np.random.default_rng(seed)
    plt = None
    if plot:
        try:
            import matplotlib
            matplotlib.use('Agg')
            import matplotlib.pyplot as plt
        except ImportError:
            print('matplotlib is not installed: scatter plots skipped')
    out = {}
    for k in range(2, 8):
        centers, labels, inertia = kmeans(X, k, rng)
        out[k] = centers
        print('score for {}-means = {}'.format(k, -inertia))
        print('  centers = {}'.format(centers))
        if plt is not None:
            fig = plt.figure(figsize=(16, 9), dpi=200)
            plt.scatter(X[:, 0], X[:, 1], c=labels, cmap='viridis')
            plt.xlabel('Width')           # axis labels as in the reference (its columns are H, W)
            plt.ylabel('Height')
            plt.scatter(centers[:, 0], centers[:, 1], c='black', s=200, alpha=0.5)
            plt.savefig('scatterplot_{}_clusters.png'.format(k))
            plt.close(fig)
        print('View the scatterplot and determine if the clusters look appropriate. You generally want a small, medium, and large anchor for Yolo.')
    return out


def load_box_sizes(csv_dirpath=None, database=None):
    """int64 [n, 2] = (w, h) of every box of a folder of csv files or of an lmdb (exactly one of the two)."""
    from yolo3 import anchors
    if (csv_dirpath is None) == (database is None):
        raise ValueError('give exactly one of csv_dirpath and database')
    return anchors.load_sizes_csv(csv_dirpath) if database is None else anchors.load_sizes_lmdb(database)


def find_anchors_iou(wh, k, seed=0, evolve=1000, population=64, thr=0.5, scale=1.0, device='cpu', output=None):
    """--metric iou: yolo3.anchors.fit_anchors on the sizes wh (w, h); prints the per-anchor table and the --anchors string for
    train.py; writes the fit as JSON when `output` is given.  -> the fit."""
    from yolo3 import anchors
    fit = anchors.fit_anchors(wh, k, seed=seed, evolve=evolve, population=population, thr=thr, scale=scale, device=device)
    for line in anchors.format_fit(fit):
        print(line)
    if output:
        # with at least one anchor per scale the file also records which scale owns each (train.py --anchor_assignment scale)
        anchors.save_anchors(output, fit, anchors.default_anchor_scales(fit['anchors']) if len(fit['anchors']) >= 3 else None)
        print('anchors written to {}'.format(output))
    return fit


def build_parser():
    parser = argparse.ArgumentParser(prog='find_anchor_sizes', description='Script to determine what anchors to use with yolov3.')
    parser.add_argument('--csv_dirpath', dest='csv_dirpath', type=str, default=None,
                        help='Filepath to the directory containing annotation csv files with columns [X,Y,W,H]')
    parser.add_argument('--seed', type=int, default=0, help='k-means seed (extension; the reference is unseeded)')
    parser.add_argument('--metric', choices=('euclidean', 'iou'), default='euclidean',
                        help='(addition) euclidean (default): the reference\'s k-means on (H, W) for k = 2..7; iou: k anchors fitted to the '
                             'criterion that assigns boxes to anchors in training, IoU k-means and a mutation search (needs --k)')
    parser.add_argument('--k', type=int, default=None, help='(addition, --metric iou) number of anchors, 1..16')
    parser.add_argument('--database', type=str, default=None,
                        help='(addition, --metric iou) lmdb written by build_lmdb.py to take the boxes from, instead of --csv_dirpath')
    parser.add_argument('--evolve', type=int, default=None, help='(addition, --metric iou) mutants tried by the search (default 1000; 0: IoU k-means alone)')
    parser.add_argument('--population', type=int, default=None, help='(addition, --metric iou) mutants per generation, scored in one call (default 64)')
    parser.add_argument('--thr', type=float, default=None, help='(addition, --metric iou) IoU at which a box counts as recalled in the report (default 0.5)')
    parser.add_argument('--scale', type=float, default=None,
                        help='(addition, --metric iou) factor applied to every size first, for images that are resized before training (default 1)')
    parser.add_argument('--device', choices=('cpu', 'gpu'), default=None,
                        help='(addition, --metric iou) where the candidate sets are scored: cpu (NumPy, default) or gpu (HIP kernel); same result')
    parser.add_argument('--output', type=str, default=None, help='(addition, --metric iou) write the fit as JSON (train.py --anchors_file reads it)')
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    extra = [f for f in ('k', 'database', 'evolve', 'population', 'thr', 'scale', 'device', 'output') if getattr(args, f) is not None]
    if args.metric == 'euclidean':
        if extra:
            parser.error('--{} needs --metric iou'.format(extra[0]))
        if args.csv_dirpath is None:
            parser.error('the following arguments are required: --csv_dirpath')
        find_anchors(args.csv_dirpath, args.seed)
        return None
    if args.k is None:
        parser.error('--metric iou needs --k')
    if (args.csv_dirpath is None) == (args.database is None):
        parser.error('--metric iou needs exactly one of --csv_dirpath and --database')
    try:
        wh = load_box_sizes(args.csv_dirpath, args.database)
        if wh.shape[0] == 0:
            raise ValueError('no boxes found')
        return find_anchors_iou(wh, args.k, args.seed, 1000 if args.evolve is None else args.evolve, 64 if args.population is None else args.population,
                                0.5 if args.thr is None else args.thr, 1.0 if args.scale is None else args.scale, args.device or 'cpu', args.output)
    except ValueError as e:
        parser.error(str(e))


if __name__ == '__main__':
    main()
