"""NumPy restatement of the letterbox front end in fp64, for tests/test_cpu_letterbox.py and
tests/test_gpu_letterbox.py: the record geometry, the antialiased triangle-filter weight matrices (the function of torch's
interpolate(mode='bilinear', antialias=True, align_corners=False)), the un-normalised frame with the quantities its error bound
needs, the z-score over the content, and the unmap in fp64 and in float32."""
import math
from fractions import Fraction

import numpy as np

RECORD = np.dtype([('src_offset', '<u8'), ('src_h', '<i4'), ('src_w', '<i4'), ('new_h', '<i4'), ('new_w', '<i4'), ('pad_y', '<i4'),
                   ('pad_x', '<i4')])
U = 2.0 ** -24          # unit roundoff of fp32


def record(h, w, H, W, src_offset=0):
    """The issue's geometry, in Python integers and fp64."""
    r = min(H / h, W / w)
    new_h = min(H, max(1, int(math.floor(h * r + 0.5))))
    new_w = min(W, max(1, int(math.floor(w * r + 0.5))))
    rec = np.zeros(1, RECORD)
    rec[0] = (src_offset, h, w, new_h, new_w, (H - new_h) // 2, (W - new_w) // 2)
    return rec


def hand_record(h, w, new_h, new_w, pad_y, pad_x, src_offset=0):
    rec = np.zeros(1, RECORD)
    rec[0] = (src_offset, h, w, new_h, new_w, pad_y, pad_x)
    return rec


def axis_weights(n_in, n_out):
    """[n_out][n_in] fp64: s = in / out, support u = max(s, 1), centre ctr = s (o + 0.5), taps lo = max(0, int(ctr - u + 0.5)) up to
    hi = min(in, int(ctr + u + 0.5)) -- exact: the bounds are ratios of integers -- weights max(0, 1 - |(j - ctr + 0.5) / u|)
    normalised by their sum."""
    s = Fraction(n_in, n_out)
    u = max(s, Fraction(1))
    m = np.zeros((n_out, n_in), np.float64)
    for o in range(n_out):
        ctr = s * (o + Fraction(1, 2))
        lo = max(0, int(ctr - u + Fraction(1, 2)))
        hi = min(n_in, int(ctr + u + Fraction(1, 2)))
        w = np.array([max(Fraction(0), 1 - abs((j - ctr + Fraction(1, 2)) / u)) for j in range(lo, hi)], dtype=object)
        tot = sum(w)
        m[o, lo:hi] = [float(v / tot) for v in w]
    return m


def resize(img_chw, new_h, new_w):
    """fp64 [c][h][w] -> [c][new_h][new_w]"""
    wy, wx = axis_weights(img_chw.shape[1], new_h), axis_weights(img_chw.shape[2], new_w)
    return np.einsum('oi,cij,pj->cop', wy, img_chw.astype(np.float64), wx)


def frames(images, records, H, W, fill):
    """images: HWC arrays; -> (frame fp64 [n][c][H][W], mag = sum |wy wx tap| on the content and 0 elsewhere, taps = Tx + Ty: the
    non-zero taps of each content element's column and row, 0 elsewhere, content mask)."""
    n, c = len(images), images[0].shape[2]
    out = np.full((n, c, H, W), fill, np.float64)
    mag = np.zeros((n, c, H, W), np.float64)
    taps = np.zeros((n, c, H, W), np.int64)
    mask = np.zeros((n, c, H, W), bool)
    for i, (im, r) in enumerate(zip(images, records)):
        x = np.ascontiguousarray(im.transpose(2, 0, 1)).astype(np.float64)
        wy, wx = axis_weights(x.shape[1], int(r['new_h'])), axis_weights(x.shape[2], int(r['new_w']))
        ys, xs = slice(int(r['pad_y']), int(r['pad_y'] + r['new_h'])), slice(int(r['pad_x']), int(r['pad_x'] + r['new_w']))
        with np.errstate(invalid='ignore'):
            out[i, :, ys, xs] = np.einsum('oi,cij,pj->cop', wy, x, wx)
            mag[i, :, ys, xs] = np.einsum('oi,cij,pj->cop', wy, np.abs(x), wx)
        taps[i, :, ys, xs] = ((wy > 0).sum(1)[:, None] + (wx > 0).sum(1)[None, :])[None]
        mask[i, :, ys, xs] = True
    return out, mag, taps, mask


def content_stats(frame, rec):
    """(mu, sd) as the kernels round them: fp64 mean and population std of the content of one frame [c][H][W], then float32."""
    ys, xs = slice(int(rec['pad_y']), int(rec['pad_y'] + rec['new_h'])), slice(int(rec['pad_x']), int(rec['pad_x'] + rec['new_w']))
    v = frame[:, ys, xs].astype(np.float64)
    mean = v.sum() / v.size
    var = max(0.0, (v * v).sum() / v.size - mean * mean)
    return np.float32(mean), np.float32(math.sqrt(var))


def zscore_content(frames_f32, records):
    """fp64 [n][H][W][c]: sd <= 1 ? x - mu : (x - mu) / sd on the content, 0 on the padding; also the per-element error bound of
    the fp32 evaluation (see test_gpu_letterbox.py) and the (mu, sd) pairs."""
    n, c, H, W = frames_f32.shape
    out = np.zeros((n, H, W, c), np.float64)
    bound = np.zeros((n, H, W, c), np.float64)
    stats = []
    for i, r in enumerate(records):
        mu, sd = content_stats(frames_f32[i], r)
        stats.append((mu, sd))
        ys, xs = slice(int(r['pad_y']), int(r['pad_y'] + r['new_h'])), slice(int(r['pad_x']), int(r['pad_x'] + r['new_w']))
        x = frames_f32[i, :, ys, xs].astype(np.float64).transpose(1, 2, 0)
        if sd <= 1:
            t = x - float(mu)
            b = U * np.abs(t) + 2 * U * abs(float(mu))
        else:
            t = (x - float(mu)) / float(sd)
            b = 4 * U * np.abs(t) + 2 * U * abs(float(mu)) / float(sd)
        out[i, ys, xs] = t
        bound[i, ys, xs] = b * (1 + 2.0 ** -20)
    return out, bound, stats


def scales(rec):
    return np.float32(float(rec['src_w']) / float(rec['new_w'])), np.float32(float(rec['src_h']) / float(rec['new_h']))


def unmap64(rows, records, clip):
    """fp64 statement of the unmap on rows [n][nb][ld] (corners first)."""
    out = rows.astype(np.float64).copy()
    for i, r in enumerate(records):
        sx, sy = float(r['src_w']) / float(r['new_w']), float(r['src_h']) / float(r['new_h'])
        for q in range(4):
            pad, s, lim = (r['pad_x'], sx, r['src_w']) if q % 2 == 0 else (r['pad_y'], sy, r['src_h'])
            v = (out[i, :, q] - float(pad)) * s
            out[i, :, q] = np.where(v < 0, 0.0, np.where(v > float(lim), float(lim), v)) if clip else v
    return out


def unmap32(rows, records, clip):
    """The float32 restatement: one fp32 subtraction, one fp32 multiplication, then v < 0 ? 0 : v > lim ? lim : v."""
    out = np.array(rows, np.float32, copy=True)
    for i, r in enumerate(records):
        sx, sy = scales(r)
        for q in range(4):
            pad, s, lim = (r['pad_x'], sx, r['src_w']) if q % 2 == 0 else (r['pad_y'], sy, r['src_h'])
            with np.errstate(invalid='ignore', over='ignore'):
                v = (out[i, :, q] - np.float32(pad)) * np.float32(s)
                if clip:
                    lim = np.float32(lim)
                    v = np.where(v < 0, np.float32(0), np.where(v > lim, lim, v))
            out[i, :, q] = v
    return out
