// Detection-side kernels: anchor decode (model.py:122-212), the YOLO loss with its
// analytic backward (model.py:230-354) and class-wise NMS (bbox_utils.py:200-281).
// Compiled with -ffp-contract=off: the NMS arithmetic must round exactly like the
// reference's NumPy float32 elementwise ops so the integer keep indices match.
#include <float.h>
#include <stdlib.h>

#include "common.h"

#define Y3_MAX_ANCHORS 16
#define Y3_MAX_SCALES 4

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
struct DecodeArgs {
    const float* fm[Y3_MAX_SCALES];
    int ld[Y3_MAX_SCALES], gh[Y3_MAX_SCALES], gw[Y3_MAX_SCALES], start[Y3_MAX_SCALES + 1];
    float sx[Y3_MAX_SCALES], sy[Y3_MAX_SCALES];
    float aw[Y3_MAX_ANCHORS], ah[Y3_MAX_ANCHORS];
    int nscales, A, K, N, nb;
    float* out;
};

__global__ void decode_kernel(const DecodeArgs p) {
    const long long total = (long long)p.N * p.nb;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int D = 5 + p.K;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int n = (int)(i / p.nb);
        const int b = (int)(i - (long long)n * p.nb);
        int s = 0;
        while (s + 1 < p.nscales && b >= p.start[s + 1]) ++s;
        const int r = b - p.start[s];
        const int a = r % p.A;
        const int cell = r / p.A;
        const int gy = cell / p.gw[s], gx = cell - gy * p.gw[s];
        const float* t = p.fm[s] + ((long long)n * p.gh[s] * p.gw[s] + cell) * p.ld[s] + a * D;
        // reorg_layer: box_xy = (sigmoid(t_xy) + offset) * stride ; box_wh = exp(t_wh) * anchor
        const float cx = (sigmoidf_(t[0]) + (float)gx) * p.sx[s];
        const float cy = (sigmoidf_(t[1]) + (float)gy) * p.sy[s];
        const float w = expf(t[2]) * p.aw[a];
        const float h = expf(t[3]) * p.ah[a];
        float* o = p.out + i * D;
        o[0] = cx - w / 2.0f;
        o[1] = cy - h / 2.0f;
        o[2] = cx + w / 2.0f;
        o[3] = cy + h / 2.0f;
        o[4] = sigmoidf_(t[4]);
        for (int k = 0; k < p.K; ++k) o[5 + k] = sigmoidf_(t[5 + k]);
    }
}

extern "C" int y3_decode_fwd(const y3_tensor* fm, int nscales, const float* anchors_host, int num_anchors, int num_classes, int img_h,
                             int img_w, float* out, y3_stream_t stream) {
    Y3_CHECK_ARG(fm && anchors_host && out, "decode_fwd: null pointer");
    Y3_CHECK_ARG(nscales >= 1 && nscales <= Y3_MAX_SCALES, "decode_fwd: nscales %d", nscales);
    Y3_CHECK_ARG(num_anchors >= 1 && num_anchors <= Y3_MAX_ANCHORS && num_classes >= 1, "decode_fwd: anchors/classes");
    DecodeArgs p = {};
    p.nscales = nscales;
    p.A = num_anchors;
    p.K = num_classes;
    p.N = fm[0].n;
    int nb = 0;
    for (int s = 0; s < nscales; ++s) {
        Y3_CHECK_ARG(fm[s].ptr && fm[s].n == p.N && fm[s].c == num_anchors * (5 + num_classes) && fm[s].ld >= fm[s].c, "decode_fwd: feature map %d geometry", s);
        p.fm[s] = fm[s].ptr;
        p.ld[s] = fm[s].ld;
        p.gh[s] = fm[s].h;
        p.gw[s] = fm[s].w;
        p.start[s] = nb;
        nb += fm[s].h * fm[s].w * num_anchors;
        // Q6: stride = img_size[0:2] // grid = (s_y, s_x) multiplies (x, y)
        p.sx[s] = (float)(img_h / fm[s].h);
        p.sy[s] = (float)(img_w / fm[s].w);
    }
    p.start[nscales] = nb;
    p.nb = nb;
    for (int a = 0; a < num_anchors; ++a) {
        p.aw[a] = anchors_host[2 * a];
        p.ah[a] = anchors_host[2 * a + 1];
    }
    p.out = out;
    const long long total = (long long)p.N * nb;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    Y3_CHECK_LAUNCH("decode");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// loss forward + backward, one scale
// ---------------------------------------------------------------------------
struct LossArgs {
    const float* fm;
    const float* gt;
    float* dfm;
    int fm_ld, dfm_ld;
    int N, G_h, G_w, A, K;
    float sx, sy;
    float aw[Y3_MAX_ANCHORS], ah[Y3_MAX_ANCHORS];
    float inv_b, gscale;  // 1/local batch, 1/(local batch * global batch)
    float box_weight;     // factor of the box term of the IoU kinds (y3_loss_fwd_bwd_ex); the mse kernel does not read it
    int* present;         // [A] flags: anchor a has at least one GT cell in this batch
    float* partials;      // [blocks][4]; truth variant: [N][blocks per image][5]
    // truth variant only (y3_loss_fwd_bwd_truth).  Behind every field of the reference's kernel: its loads keep their offsets
    const float* truth_boxes;  // [N][truth_cap][4] centre x, centre y, w, h in pixels
    const int* truth_counts;   // [N] boxes found per image; may exceed truth_cap
    int truth_cap;
    float ignore_thresh;
    // focal variant only (y3_loss_fwd_bwd_focal).  Behind the truth fields, for the same reason
    float gamma_obj, alpha_obj;  // objectness term: focusing exponent >= 0, balancing factor (0 = none)
    float gamma_cls, alpha_cls;  // class term
    float label_smoothing;       // class labels g -> g (1 - eps) + eps / 2
};

__global__ void loss_present_kernel(const float* __restrict__ gt, long long ncell_anchor, int A, int D, int* present) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < ncell_anchor; i += stride)
        if (gt[i * D + 4] != 0.f) atomicOr(&present[i % A], 1);
}

__device__ __forceinline__ float sig_ce(float z, float x) {  // labels z, logits x (App. C6)
    return fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
}

// Focal form of sig_ce (Lin et al. 2017): returns w m^gamma ce and writes its derivative in x to *dx.
//   m = z sigmoid(-x) + (1 - z) sigmoid(x) is 1 - p_t, formed without that subtraction: at a saturated logit sigmoid(-x) keeps the small
//   side's digits where 1 - sigmoid(x) is 0.  w = alpha z + (1 - alpha)(1 - z), or 1 for alpha == 0.
//   d/dx = w [m^gamma (p - z) + gamma m^gamma r (1 - 2z) ce], r = p (1 - p) / m <= 1 (m >= min(p, 1 - p) >= p (1 - p)), r = 0 where m = 0:
//   m^(gamma - 1) is never formed, so both values are finite for every gamma >= 0 and every logit.  powf(0, 0) = 1.
__device__ __forceinline__ float focal_ce(float z, float x, float gamma, float alpha, float* dx) {
    const float ps = sigmoidf_(x), qs = sigmoidf_(-x);
    const float ce = sig_ce(z, x);
    const float m = z * qs + (1.f - z) * ps;
    const float w = alpha != 0.f ? alpha * z + (1.f - alpha) * (1.f - z) : 1.f;
    const float mg = powf(m, gamma);
    const float r = m > 0.f ? (ps * qs) / m : 0.f;
    *dx = w * (mg * (ps - z) + gamma * mg * r * (1.f - 2.f * z) * ce);
    return w * mg * ce;
}

// The box term of the opt-in IoU losses (Y3_BOX_LOSS_GIOU / DIOU / CIOU) for one positive (cell, anchor): returns 1 - X and
// writes d(1 - X)/d(bx, by, bw, bh) to gb[0..3].  Reverse mode by hand: every `a_q` is dX/dq.  min / max / the clamp at 0 hand the
// gradient to the selected operand.  U, C, c2 reach 1e32 at a logit of 30, so none of them is squared: q / U^2 is (q / U) / U.
template <int BOX>
__device__ __forceinline__ float iou_box_loss(float bx, float by, float bw, float bh, const float* __restrict__ g, float* gb) {
    const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
    const float px0 = bx - bw / 2.0f, px1 = bx + bw / 2.0f, py0 = by - bh / 2.0f, py1 = by + bh / 2.0f;
    const float gx0 = g0 - g2 / 2.0f, gx1 = g0 + g2 / 2.0f, gy0 = g1 - g3 / 2.0f, gy1 = g1 + g3 / 2.0f;
    const float ixr = fminf(px1, gx1) - fmaxf(px0, gx0), iyr = fminf(py1, gy1) - fmaxf(py0, gy0);
    const float ix = fmaxf(ixr, 0.f), iy = fmaxf(iyr, 0.f);
    const float inter = ix * iy;
    const float U = bw * bh + g2 * g3 - inter;
    const float iou = inter / U;
    const float cw = fmaxf(px1, gx1) - fminf(px0, gx0), ch = fmaxf(py1, gy1) - fminf(py0, gy0);
    float X = iou;
    float a_U = -(iou / U);             // through IoU = inter / U
    float a_cw, a_ch;
    float a_bx = 0.f, a_by = 0.f, a_bw = 0.f, a_bh = 0.f;
    if (BOX == Y3_BOX_LOSS_GIOU) {
        const float C = cw * ch;
        X = iou - (C - U) / C;
        a_U += 1.0f / C;
        const float a_C = -((U / C) / C);
        a_cw = a_C * ch;
        a_ch = a_C * cw;
    } else {
        const float c2 = cw * cw + ch * ch;
        const float dx = bx - g0, dy = by - g1;
        const float rho2 = dx * dx + dy * dy;
        X = iou - rho2 / c2;
        const float a_c2 = (rho2 / c2) / c2;
        a_cw = a_c2 * (2.0f * cw);
        a_ch = a_c2 * (2.0f * ch);
        a_bx = -(2.0f * dx) / c2;
        a_by = -(2.0f * dy) / c2;
        if (BOX == Y3_BOX_LOSS_CIOU) {
            const float k = 0.40528473456935109f;  // 4 / pi^2
            const float da = atanf(g2 / g3) - atanf(bw / bh);
            const float v = k * (da * da);
            const float alpha = v / ((1.0f - iou) + v + 1e-7f);  // a constant of the backward pass
            X = X - alpha * v;
            // dv/d atan(bw/bh) = -2 k da ;  d atan(bw/bh) / d(bw, bh) = (bh, -bw) / (bw^2 + bh^2)
            const float a_at = alpha * (2.0f * k * da);
            const float q = bw * bw + bh * bh;
            a_bw = a_at * (bh / q);
            a_bh = -(a_at * (bw / q));
        }
    }
    const float a_inter = 1.0f / U - a_U;  // U = bw bh + g2 g3 - inter
    a_bw += a_U * bh;
    a_bh += a_U * bw;
    const float a_ixr = ixr >= 0.f ? a_inter * iy : 0.f, a_iyr = iyr >= 0.f ? a_inter * ix : 0.f;
    // corners: the intersection takes the inner edge of each pair, the enclosing box the outer one
    const float a_px1 = px1 < gx1 ? a_ixr : (px1 > gx1 ? a_cw : 0.5f * (a_ixr + a_cw));
    const float a_px0 = px0 > gx0 ? -a_ixr : (px0 < gx0 ? -a_cw : -0.5f * (a_ixr + a_cw));
    const float a_py1 = py1 < gy1 ? a_iyr : (py1 > gy1 ? a_ch : 0.5f * (a_iyr + a_ch));
    const float a_py0 = py0 > gy0 ? -a_iyr : (py0 < gy0 ? -a_ch : -0.5f * (a_iyr + a_ch));
    gb[0] = -(a_bx + (a_px0 + a_px1));
    gb[1] = -(a_by + (a_py0 + a_py1));
    gb[2] = -(a_bw + (a_px1 - a_px0) / 2.0f);
    gb[3] = -(a_bh + (a_py1 - a_py0) / 2.0f);
    return 1.0f - X;
}

// BOX == Y3_BOX_LOSS_MSE is the reference's loss; the other kinds replace its xy and wh terms by iou_box_loss and leave the rest alone.
// TRUTH == false is the reference's ignore mask (Q7) on a 1-D grid over the whole batch.  TRUTH == true masks against the
// ground-truth boxes of the prediction's own image: grid (blocks per image, N), the image's box list staged in LDS Y3_TRUTH_CHUNK boxes
// at a time, a fifth partial sum (the ignored negatives).  Everything TRUTH adds is behind `if (TRUTH)`, a compile-time constant: the
// TRUTH == false instantiations keep the instructions they had.
// FOCAL == true replaces sig_ce by focal_ce in the objectness and class terms, each with its own (gamma, alpha), the class
// labels smoothed first.  A neutral term (gamma 0, alpha 0, and for class no smoothing) takes the plain expressions behind a uniform
// branch: its loss part and gradient channels keep the plain kernel's bits.  Everything FOCAL adds is behind `if (FOCAL)`.
template <int BOX, bool TRUTH, bool FOCAL>
__global__ __launch_bounds__(256) void loss_kernel(const LossArgs p) {
    constexpr int NP = TRUTH ? 5 : 4;
    __shared__ float sm[NP][256];
    __shared__ float4 tb[TRUTH ? Y3_TRUTH_CHUNK : 1];
    const int D = 5 + p.K;
    // TRUTH: one image per workgroup row; j runs over the image's (cell, anchor) slots, i = first + j over the batch's
    const long long total = TRUTH ? (long long)p.G_h * p.G_w * p.A : (long long)p.N * p.G_h * p.G_w * p.A;
    const long long first = TRUTH ? (long long)blockIdx.y * total : 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    float l_xy = 0.f, l_wh = 0.f, l_obj = 0.f, l_cls = 0.f, l_ign = 0.f;
    int cnt = 0;
    const float* tbox = nullptr;
    if (TRUTH) {
        cnt = p.truth_counts[blockIdx.y];
        cnt = cnt < 0 ? 0 : (cnt > p.truth_cap ? p.truth_cap : cnt);
        tbox = p.truth_boxes + (long long)blockIdx.y * p.truth_cap * 4;
        if (cnt <= Y3_TRUTH_CHUNK) {  // the whole list fits: staged once, outside the prediction loop
            if ((int)threadIdx.x < cnt) {
                const float* b = tbox + (long long)threadIdx.x * 4;
                tb[threadIdx.x] = make_float4(b[0], b[1], b[2], b[3]);
            }
            __syncthreads();
        }
    }
    // TRUTH: the loop holds barriers when the list is longer than one chunk, so its bound is the workgroup's first slot (uniform); a
    // thread past the end of the image decodes the image's last slot, takes part in the staging and leaves before anything is written
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; TRUTH ? j - threadIdx.x < total : j < total; j += stride) {
        const bool active = !TRUTH || j < total;
        const long long i = TRUTH ? first + (active ? j : total - 1) : j;
        const int a = (int)(i % p.A);
        const long long cell = i / p.A;  // n*G*G + gy*G + gx
        const int gx = (int)(cell % p.G_w);
        const int gy = (int)((cell / p.G_w) % p.G_h);
        const float* t = p.fm + cell * p.fm_ld + a * D;
        const float* g = p.gt + i * D;
        float* d = p.dfm + cell * p.dfm_ld + a * D;
        const float aw = p.aw[a], ah = p.ah[a];
        const float offx = (float)gx, offy = (float)gy;
        const float sgx = sigmoidf_(t[0]), sgy = sigmoidf_(t[1]);
        const float bx = (sgx + offx) * p.sx, by = (sgy + offy) * p.sy;
        const float ew = expf(t[2]), eh = expf(t[3]);
        const float bw = ew * aw, bh = eh * ah;
        const float gm = g[4];

        float best = -INFINITY;
        if (!TRUTH) {
            // ignore mask (Q7): best IoU against origin-centred anchor-sized boxes of the anchors present in the batch
            for (int q = 0; q < p.A; ++q) {
                if (!p.present[q]) continue;
                const float tw = p.aw[q], th = p.ah[q];
                const float ix = fmaxf(fminf(bx + bw / 2.0f, tw / 2.0f) - fmaxf(bx - bw / 2.0f, -tw / 2.0f), 0.f);
                const float iy = fmaxf(fminf(by + bh / 2.0f, th / 2.0f) - fmaxf(by - bh / 2.0f, -th / 2.0f), 0.f);
                const float inter = ix * iy;
                const float iou = inter / (bw * bh + tw * th - inter);
                best = fmaxf(best, iou);
            }
        } else {
            // ignore mask of the paper: best IoU against the ground-truth boxes of this image.  tb[q] is one broadcast ds_read_b128
            const float px0 = bx - bw / 2.0f, px1 = bx + bw / 2.0f, py0 = by - bh / 2.0f, py1 = by + bh / 2.0f;
            const float parea = bw * bh;
            for (int c0 = 0; c0 < cnt; c0 += Y3_TRUTH_CHUNK) {
                const int m = cnt - c0 < Y3_TRUTH_CHUNK ? cnt - c0 : Y3_TRUTH_CHUNK;
                if (cnt > Y3_TRUTH_CHUNK) {  // uniform: cnt is the workgroup's
                    __syncthreads();         // every reader of the chunk before is done
                    if ((int)threadIdx.x < m) {
                        const float* b = tbox + (long long)(c0 + threadIdx.x) * 4;
                        tb[threadIdx.x] = make_float4(b[0], b[1], b[2], b[3]);
                    }
                    __syncthreads();
                }
                for (int q = 0; q < m; ++q) {
                    const float4 b = tb[q];
                    const float ix = fmaxf(fminf(px1, b.x + b.z / 2.0f) - fmaxf(px0, b.x - b.z / 2.0f), 0.f);
                    const float iy = fmaxf(fminf(py1, b.y + b.w / 2.0f) - fmaxf(py0, b.y - b.w / 2.0f), 0.f);
                    const float inter = ix * iy;
                    const float iou = inter / (parea + b.z * b.w - inter);
                    best = fmaxf(best, iou);
                }
            }
            if (!active) continue;  // behind the last barrier of this pass
        }
        const float ignore = best < (TRUTH ? p.ignore_thresh : 0.5f) ? 1.f : 0.f;
        if (TRUTH) l_ign += (gm == 0.f && ignore == 0.f) ? 1.f : 0.f;
        const float valid = gm + (1.f - gm) * ignore;

        // objectness
        if (FOCAL && !(p.gamma_obj == 0.f && p.alpha_obj == 0.f)) {
            float dx;
            l_obj += valid * focal_ce(gm, t[4], p.gamma_obj, p.alpha_obj, &dx);
            d[4] = valid * dx * p.gscale;
        } else {
            l_obj += valid * sig_ce(gm, t[4]);
            d[4] = valid * (sigmoidf_(t[4]) - gm) * p.gscale;
        }
        // class
        if (FOCAL && !(p.gamma_cls == 0.f && p.alpha_cls == 0.f && p.label_smoothing == 0.f)) {
            for (int k = 0; k < p.K; ++k) {
                const float z = g[5 + k] * (1.f - p.label_smoothing) + 0.5f * p.label_smoothing;
                float dx;
                l_cls += gm * focal_ce(z, t[5 + k], p.gamma_cls, p.alpha_cls, &dx);
                d[5 + k] = gm * dx * p.gscale;
            }
        } else {
            for (int k = 0; k < p.K; ++k) {
                l_cls += gm * sig_ce(g[5 + k], t[5 + k]);
                d[5 + k] = gm * (sigmoidf_(t[5 + k]) - g[5 + k]) * p.gscale;
            }
        }
        // xy: squared error in logit space of the clipped in-cell position
        if (BOX == Y3_BOX_LOSS_MSE) {
            const float txr = g[0] / p.sx - offx, tyr = g[1] / p.sy - offy;
            const float pxr = bx / p.sx - offx, pyr = by / p.sy - offy;
            const float tx = fminf(fmaxf(txr, 0.01f), 0.99f), ty = fminf(fmaxf(tyr, 0.01f), 0.99f);
            const float px = fminf(fmaxf(pxr, 0.01f), 0.99f), py = fminf(fmaxf(pyr, 0.01f), 0.99f);
            const float ltx = -logf(1.0f / tx - 1.0f), lty = -logf(1.0f / ty - 1.0f);
            const float lpx = -logf(1.0f / px - 1.0f), lpy = -logf(1.0f / py - 1.0f);
            const float ex = ltx - lpx, ey = lty - lpy;
            l_xy += (ex * ex + ey * ey) * gm;
            // d/dt: -2*e * dlogit/dp * [clip passes] * sigmoid'(t)     (the *stride /stride pair is the identity)
            const float gx_ = (pxr >= 0.01f && pxr <= 0.99f) ? (sgx * (1.f - sgx)) / (px * (1.f - px)) : 0.f;
            const float gy_ = (pyr >= 0.01f && pyr <= 0.99f) ? (sgy * (1.f - sgy)) / (py * (1.f - py)) : 0.f;
            d[0] = gm * (-2.f * ex) * gx_ * p.gscale;
            d[1] = gm * (-2.f * ey) * gy_ * p.gscale;
        }
        // wh: squared error of log(size / anchor)
        if (BOX == Y3_BOX_LOSS_MSE) {
            float tw = g[2] / aw, th = g[3] / ah;
            float pw = bw / aw, ph = bh / ah;
            const bool pw_nz = pw != 0.f, ph_nz = ph != 0.f;
            if (tw == 0.f) tw = 1.f;
            if (th == 0.f) th = 1.f;
            if (!pw_nz) pw = 1.f;
            if (!ph_nz) ph = 1.f;
            const float ltw = logf(fminf(fmaxf(tw, 1e-9f), 1e9f)), lth = logf(fminf(fmaxf(th, 1e-9f), 1e9f));
            const float lpw = logf(fminf(fmaxf(pw, 1e-9f), 1e9f)), lph = logf(fminf(fmaxf(ph, 1e-9f), 1e9f));
            const float ew_ = ltw - lpw, eh_ = lth - lph;
            l_wh += (ew_ * ew_ + eh_ * eh_) * gm;
            // d log(clip(q))/dt = [q in range, q != 0] * (dq/dt)/q = 1
            const float gw_ = (pw_nz && pw >= 1e-9f && pw <= 1e9f) ? 1.f : 0.f;
            const float gh_ = (ph_nz && ph >= 1e-9f && ph <= 1e9f) ? 1.f : 0.f;
            d[2] = gm * (-2.f * ew_) * gw_ * p.gscale;
            d[3] = gm * (-2.f * eh_) * gh_ * p.gscale;
        }
        // IoU-family box term in place of xy + wh, accumulated in the xy slot.  A branch, not a product with gm: a cell without an
        // object writes +0 whatever its logits are (expf may have overflowed there).  Positives are tens per batch, so the few lanes
        // that take the branch cost one divergent pass per wave that holds one.
        if (BOX != Y3_BOX_LOSS_MSE) {
            float gb[4] = {0.f, 0.f, 0.f, 0.f};
            if (gm != 0.f) {
                const float w = gm * p.box_weight;
                l_xy += w * iou_box_loss<BOX>(bx, by, bw, bh, g, gb);
                // d(bx)/dt0 = sx * sigmoid'(t0) ;  d(bw)/dt2 = bw
                gb[0] = w * (gb[0] * (p.sx * (sgx * (1.f - sgx)))) * p.gscale;
                gb[1] = w * (gb[1] * (p.sy * (sgy * (1.f - sgy)))) * p.gscale;
                gb[2] = w * (gb[2] * bw) * p.gscale;
                gb[3] = w * (gb[3] * bh) * p.gscale;
            }
            d[0] = gb[0];
            d[1] = gb[1];
            d[2] = gb[2];
            d[3] = gb[3];
        }
    }
    sm[0][threadIdx.x] = l_xy;
    sm[1][threadIdx.x] = l_wh;
    sm[2][threadIdx.x] = l_obj;
    sm[3][threadIdx.x] = l_cls;
    if (TRUTH) sm[NP - 1][threadIdx.x] = l_ign;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
#pragma unroll
            for (int j = 0; j < NP; ++j) sm[j][threadIdx.x] += sm[j][threadIdx.x + o];
        __syncthreads();
    }
    if (!TRUTH) {
        if (threadIdx.x < 4) p.partials[blockIdx.x * 4 + threadIdx.x] = sm[threadIdx.x][0] * p.inv_b;
    } else if (threadIdx.x < NP) {  // the count is not a loss term: unscaled
        p.partials[((long long)blockIdx.y * gridDim.x + blockIdx.x) * NP + threadIdx.x] = sm[threadIdx.x][0] * (threadIdx.x < 4 ? p.inv_b : 1.f);
    }
}

__global__ void loss_clear_kernel(int* present) {
    if (threadIdx.x < Y3_MAX_ANCHORS) present[threadIdx.x] = 0;
}
__global__ void loss_finalize_kernel(const float* partials, int nblocks, float* loss4) {
    if (threadIdx.x < 4) {
        float s = 0.f;
        for (int b = 0; b < nblocks; ++b) s += partials[b * 4 + threadIdx.x];
        loss4[threadIdx.x] += s;
    }
}

// Truth variant: partials [N][bpi][5] -> loss4[0..3] and *ignored, in a fixed order.  Thread (slot, j) adds up, image after image and
// block after block, the j-th partial of the images slot, slot + 32, ...; thread j then adds the 32 slots in order.
__global__ __launch_bounds__(256) void loss_finalize_truth_kernel(const float* partials, int n, int bpi, float* loss4, float* ignored) {
    __shared__ float slots[32][8];
    const int j = threadIdx.x & 7, slot = threadIdx.x >> 3;
    float s = 0.f;
    if (j < 5)
        for (int img = slot; img < n; img += 32)
            for (int b = 0; b < bpi; ++b) s += partials[((long long)img * bpi + b) * 5 + j];
    slots[slot][j] = s;
    __syncthreads();
    if (threadIdx.x < 5) {
        float t = 0.f;
        for (int q = 0; q < 32; ++q) t += slots[q][threadIdx.x];
        if (threadIdx.x < 4)
            loss4[threadIdx.x] += t;
        else if (ignored)
            *ignored += t;
    }
}

#define Y3_LOSS_BLOCKS 64
extern "C" size_t y3_loss_workspace_bytes(void) { return (Y3_MAX_ANCHORS + Y3_LOSS_BLOCKS * 4) * sizeof(float); }

#define Y3_LOSS_TRUTH_BLOCKS 16  // workgroups per image of the truth variant, at most
extern "C" size_t y3_loss_truth_workspace_bytes(int n) {
    if (n < 1) return 0;
    return (size_t)n * Y3_LOSS_TRUTH_BLOCKS * 5 * sizeof(float);
}

// What y3_loss_fwd_bwd_truth adds to the arguments of y3_loss_fwd_bwd_ex
struct LossTruth {
    const float* boxes;
    const int* counts;
    int cap;
    float thresh;
    float* ignored;
};

// What y3_loss_fwd_bwd_focal adds to the arguments of y3_loss_fwd_bwd_truth
struct LossFocal {
    float gamma_obj, alpha_obj, gamma_cls, alpha_cls, label_smoothing;
};

template <bool TRUTH, bool FOCAL>
static void loss_kernel_launch_kind(int box_loss, dim3 grid, hipStream_t st, const LossArgs& p) {
    if (box_loss == Y3_BOX_LOSS_MSE)
        hipLaunchKernelGGL((loss_kernel<Y3_BOX_LOSS_MSE, TRUTH, FOCAL>), grid, dim3(256), 0, st, p);
    else if (box_loss == Y3_BOX_LOSS_GIOU)
        hipLaunchKernelGGL((loss_kernel<Y3_BOX_LOSS_GIOU, TRUTH, FOCAL>), grid, dim3(256), 0, st, p);
    else if (box_loss == Y3_BOX_LOSS_DIOU)
        hipLaunchKernelGGL((loss_kernel<Y3_BOX_LOSS_DIOU, TRUTH, FOCAL>), grid, dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL((loss_kernel<Y3_BOX_LOSS_CIOU, TRUTH, FOCAL>), grid, dim3(256), 0, st, p);
}

template <bool TRUTH>
static void loss_kernel_launch(int box_loss, bool focal, dim3 grid, hipStream_t st, const LossArgs& p) {
    if (focal)
        loss_kernel_launch_kind<TRUTH, true>(box_loss, grid, st, p);
    else
        loss_kernel_launch_kind<TRUTH, false>(box_loss, grid, st, p);
}

static int loss_launch(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors, int num_classes, int img_h, int img_w,
                       float global_batch, int box_loss, float box_weight, const LossTruth* truth, const LossFocal* focal, float* loss4,
                       const y3_tensor* dfm, void* workspace, y3_stream_t stream) {
    bool use_focal = false;  // both terms neutral: the FOCAL == false kernel, the launch of y3_loss_fwd_bwd_ex / _truth
    if (focal) {
        const float go = focal->gamma_obj, ao = focal->alpha_obj, gc = focal->gamma_cls, ac = focal->alpha_cls, ls = focal->label_smoothing;
        Y3_CHECK_ARG(go >= 0.f && go <= FLT_MAX && gc >= 0.f && gc <= FLT_MAX, "loss_fwd_bwd_focal: gamma must be finite and >= 0 (got %g, %g)",
                     (double)go, (double)gc);
        Y3_CHECK_ARG((ao == 0.f || (ao > 0.f && ao < 1.f)) && (ac == 0.f || (ac > 0.f && ac < 1.f)),
                     "loss_fwd_bwd_focal: alpha must be 0 (no balancing factor) or in (0, 1) (got %g, %g)", (double)ao, (double)ac);
        Y3_CHECK_ARG(ls >= 0.f && ls < 1.f, "loss_fwd_bwd_focal: label_smoothing must be in [0, 1) (got %g)", (double)ls);
        use_focal = !(go == 0.f && ao == 0.f && gc == 0.f && ac == 0.f && ls == 0.f);
    }
    if (truth) {
        Y3_CHECK_ARG(truth->thresh > 0.f && truth->thresh <= 1.f, "loss_fwd_bwd_truth: ignore_thresh must be finite and in (0, 1] (got %g)",
                     (double)truth->thresh);
        Y3_CHECK_ARG(truth->cap >= 1, "loss_fwd_bwd_truth: truth_cap %d (at least 1)", truth->cap);
        Y3_CHECK_ARG(truth->boxes && truth->counts, "loss_fwd_bwd_truth: null pointer (truth_boxes, truth_counts)");
    }
    Y3_CHECK_ARG(box_loss >= Y3_BOX_LOSS_MSE && box_loss <= Y3_BOX_LOSS_CIOU, "loss_fwd_bwd: unknown box_loss %d", box_loss);
    Y3_CHECK_ARG(box_weight > 0.f && box_weight <= FLT_MAX, "loss_fwd_bwd: box_weight must be finite and > 0 (got %g)", (double)box_weight);
    Y3_CHECK_ARG(box_loss != Y3_BOX_LOSS_MSE || box_weight == 1.f, "loss_fwd_bwd: box_weight %g needs an IoU box_loss (mse takes 1)",
                 (double)box_weight);
    Y3_CHECK_ARG(fm && fm->ptr && dfm && dfm->ptr && gt && anchors_host && loss4 && workspace, "loss_fwd_bwd: null pointer");
    Y3_CHECK_ARG(num_anchors >= 1 && num_anchors <= Y3_MAX_ANCHORS && num_classes >= 1, "loss_fwd_bwd: anchors/classes");
    const int D = num_anchors * (5 + num_classes);
    Y3_CHECK_ARG(fm->c == D && dfm->c == D && fm->ld >= D && dfm->ld >= D && dfm->n == fm->n && dfm->h == fm->h && dfm->w == fm->w, "loss_fwd_bwd: geometry");
    hipStream_t st = (hipStream_t)stream;
    LossArgs p = {};
    p.fm = fm->ptr;
    p.gt = gt;
    p.dfm = dfm->ptr;
    p.fm_ld = fm->ld;
    p.dfm_ld = dfm->ld;
    p.N = fm->n;
    p.G_h = fm->h;
    p.G_w = fm->w;
    p.A = num_anchors;
    p.K = num_classes;
    p.sx = (float)(img_h / fm->h);  // Q6
    p.sy = (float)(img_w / fm->w);
    for (int a = 0; a < num_anchors; ++a) {
        p.aw[a] = anchors_host[2 * a];
        p.ah[a] = anchors_host[2 * a + 1];
    }
    p.inv_b = 1.f / (float)fm->n;
    p.gscale = 1.f / ((float)fm->n * global_batch);
    p.box_weight = box_weight;
    if (use_focal) {
        p.gamma_obj = focal->gamma_obj;
        p.alpha_obj = focal->alpha_obj;
        p.gamma_cls = focal->gamma_cls;
        p.alpha_cls = focal->alpha_cls;
        p.label_smoothing = focal->label_smoothing;
    }
    if (truth) {
        // one image per workgroup row; the anchor-present pass is not needed
        Y3_CHECK_ARG(fm->n <= 65535, "loss_fwd_bwd_truth: batch %d (at most 65535 images per call)", fm->n);
        const long long per_image = (long long)p.G_h * p.G_w * p.A;
        int bpi = (int)((per_image + 255) / 256);
        if (bpi > Y3_LOSS_TRUTH_BLOCKS) bpi = Y3_LOSS_TRUTH_BLOCKS;
        p.partials = (float*)workspace;
        p.truth_boxes = truth->boxes;
        p.truth_counts = truth->counts;
        p.truth_cap = truth->cap;
        p.ignore_thresh = truth->thresh;
        loss_kernel_launch<true>(box_loss, use_focal, dim3(bpi, p.N), st, p);
        Y3_CHECK_LAUNCH("loss (truth mask)");
        hipLaunchKernelGGL(loss_finalize_truth_kernel, dim3(1), dim3(256), 0, st, (const float*)p.partials, p.N, bpi, loss4, truth->ignored);
        Y3_CHECK_LAUNCH("loss_finalize (truth mask)");
        return Y3_OK;
    }
    p.present = (int*)workspace;
    p.partials = (float*)workspace + Y3_MAX_ANCHORS;
    // (a kernel, not hipMemsetAsync: as a memset NODE of a captured graph the clear was not reliably ordered against the loss kernels of
    // the previous scale, which read the same flags -- a replayed training step computed a wrong loss after the GPU had idled)
    hipLaunchKernelGGL(loss_clear_kernel, dim3(1), dim3(64), 0, st, p.present);
    Y3_CHECK_LAUNCH("loss_clear");
    const long long total = (long long)p.N * p.G_h * p.G_w * p.A;
    int pb = (int)((total + 255) / 256);
    if (pb > 256) pb = 256;
    hipLaunchKernelGGL(loss_present_kernel, dim3(pb), dim3(256), 0, st, gt, total, num_anchors, 5 + num_classes, p.present);
    Y3_CHECK_LAUNCH("loss_present");
    int blocks = (int)((total + 255) / 256);
    if (blocks > Y3_LOSS_BLOCKS) blocks = Y3_LOSS_BLOCKS;
    loss_kernel_launch<false>(box_loss, use_focal, dim3(blocks), st, p);
    Y3_CHECK_LAUNCH("loss");
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, st, (const float*)p.partials, blocks, loss4);
    Y3_CHECK_LAUNCH("loss_finalize");
    return Y3_OK;
}

extern "C" int y3_loss_fwd_bwd(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors, int num_classes, int img_h,
                               int img_w, float global_batch, float* loss4, const y3_tensor* dfm, void* workspace, y3_stream_t stream) {
    return loss_launch(fm, gt, anchors_host, num_anchors, num_classes, img_h, img_w, global_batch, Y3_BOX_LOSS_MSE, 1.f, nullptr, nullptr, loss4,
                       dfm, workspace, stream);
}

extern "C" int y3_loss_fwd_bwd_ex(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors, int num_classes, int img_h,
                                  int img_w, float global_batch, int box_loss, float box_weight, float* loss4, const y3_tensor* dfm,
                                  void* workspace, y3_stream_t stream) {
    return loss_launch(fm, gt, anchors_host, num_anchors, num_classes, img_h, img_w, global_batch, box_loss, box_weight, nullptr, nullptr, loss4,
                       dfm, workspace, stream);
}

extern "C" int y3_loss_fwd_bwd_truth(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors, int num_classes,
                                     int img_h, int img_w, float global_batch, int box_loss, float box_weight, const float* truth_boxes,
                                     const int* truth_counts, int truth_cap, float ignore_thresh, float* loss4, float* ignored,
                                     const y3_tensor* dfm, void* workspace, y3_stream_t stream) {
    const LossTruth truth = {truth_boxes, truth_counts, truth_cap, ignore_thresh, ignored};
    return loss_launch(fm, gt, anchors_host, num_anchors, num_classes, img_h, img_w, global_batch, box_loss, box_weight, &truth, nullptr, loss4,
                       dfm, workspace, stream);
}

extern "C" int y3_loss_fwd_bwd_focal(const y3_tensor* fm, const float* gt, const float* anchors_host, int num_anchors, int num_classes,
                                     int img_h, int img_w, float global_batch, int box_loss, float box_weight, const float* truth_boxes,
                                     const int* truth_counts, int truth_cap, float ignore_thresh, float* loss4, float* ignored,
                                     const y3_tensor* dfm, void* workspace, float gamma_obj, float alpha_obj, float gamma_cls,
                                     float alpha_cls, float label_smoothing, y3_stream_t stream) {
    const LossTruth truth = {truth_boxes, truth_counts, truth_cap, ignore_thresh, ignored};
    const LossFocal focal = {gamma_obj, alpha_obj, gamma_cls, alpha_cls, label_smoothing};
    // no lists at all: the reference mask (Q7) and its workspace layout; one list without the other is the truth variant's null-pointer error
    const bool reference_mask = !truth_boxes && !truth_counts;
    return loss_launch(fm, gt, anchors_host, num_anchors, num_classes, img_h, img_w, global_batch, box_loss, box_weight,
                       reference_mask ? nullptr : &truth, &focal, loss4, dfm, workspace, stream);
}

// ---------------------------------------------------------------------------
// per-image ground-truth box lists from a dense label tensor (the truth ignore mask)
// ---------------------------------------------------------------------------
// One 256-thread workgroup per image.  The rows with gt[..., 4] != 0 go out in index order: ballot prefix inside a wave, the four
// waves' counts in LDS (as tile_merge_kernel).  No atomics; the loop bound is the kernel argument, the same in every thread.
__global__ __launch_bounds__(256) void truth_boxes_kernel(const float* __restrict__ gt, int ca, int d, float* __restrict__ boxes,
                                                         int* __restrict__ counts, int cap) {
    __shared__ int wave_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* g = gt + (long long)blockIdx.x * ca * d;
    float* out = boxes + (long long)blockIdx.x * cap * 4;
    int base = 0;
    for (int r0 = 0; r0 < ca; r0 += 256) {
        const int r = r0 + tid;
        const float* row = g + (long long)(r < ca ? r : 0) * d;
        const bool keep = r < ca && row[4] != 0.f;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && pos < cap) {
            float* dst = out + (long long)pos * 4;
            dst[0] = row[0];
            dst[1] = row[1];
            dst[2] = row[2];
            dst[3] = row[3];
        }
        base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = base;
}

extern "C" int y3_truth_boxes(const float* gt, int n, long long cells_anchors, int d, float* boxes, int* counts, int cap, y3_stream_t stream) {
    Y3_CHECK_ARG(gt && boxes && counts, "truth_boxes: null pointer");
    Y3_CHECK_ARG(n >= 1 && cells_anchors >= 1 && cells_anchors < (1LL << 31) - 256 && d >= 5 && cap >= 1,
                 "truth_boxes: bad sizes (n %d, cells_anchors %lld, d %d, cap %d)", n, cells_anchors, d, cap);
    hipLaunchKernelGGL(truth_boxes_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, gt, (int)cells_anchors, d, boxes, counts, cap);
    Y3_CHECK_LAUNCH("truth_boxes");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// class-wise NMS: one 1024-thread workgroup per (image, class)
// ---------------------------------------------------------------------------
struct NmsArgs {
    const float* rows;
    int nb, D, K;
    float min_box, score_thr, iou_thr, clip_w, clip_h;
    int* keep_idx;
    int* keep_cnt;
    float* keep_score;
    int max_keep;
    int raw;  // 1: rows are [x0,y0,x1,y1,score] and the score is used as is (single_class_nms); 2: [x0,y0,x1,y1,score,class], the
              // score as is, and a row is a candidate of its own class only (y3_nms_labelled)
    int cap;  // capacity (power of two) of the per-block key array
    unsigned char* ws;
    size_t ws_per_block;
    int soft_gauss;  // soft_nms_kernel: 1 = Gaussian decay, 0 = linear
    float sigma;     // Gaussian decay parameter
};

// IoU in the reference's operation order (bbox_utils.py:200-214), float32, no contraction
__device__ __forceinline__ bool nms_suppressed(float kx0, float ky0, float kx1, float ky1, float karea, float x0, float y0, float x1, float y1,
                                               float area, float thr) {
    const float xl = fmaxf(kx0, x0), yt = fmaxf(ky0, y0);
    const float xr = fminf(kx1, x1), yb = fminf(ky1, y1);
    const float inter = fmaxf(yb - yt, 0.f) * fmaxf(xr - xl, 0.f);
    const float uni = (karea + area) - inter;
    const float iou = inter / uni;
    return !(iou <= thr);  // survivors satisfy iou <= thr; NaN is dropped, as np.where(iou <= thr) drops it
}

// The same IoU as nms_suppressed, returned (soft-NMS decays by it); k is the picked box
__device__ __forceinline__ float nms_iou(float kx0, float ky0, float kx1, float ky1, float karea, float x0, float y0, float x1, float y1,
                                        float area) {
    const float xl = fmaxf(kx0, x0), yt = fmaxf(ky0, y0);
    const float xr = fminf(kx1, x1), yb = fminf(ky1, y1);
    const float inter = fmaxf(yb - yt, 0.f) * fmaxf(xr - xl, 0.f);
    const float uni = (karea + area) - inter;
    return inter / uni;
}

// DIoU-NMS survival test (Y3_NMS_DIOU, yolo3hip.h): iou - rho2 / c2 <= thr survives, NaN is dropped
__device__ __forceinline__ bool nms_suppressed_diou(float kx0, float ky0, float kx1, float ky1, float karea, float x0, float y0, float x1,
                                                    float y1, float area, float thr) {
    const float iou = nms_iou(kx0, ky0, kx1, ky1, karea, x0, y0, x1, y1, area);
    const float dx = (x0 + x1) * 0.5f - (kx0 + kx1) * 0.5f;
    const float dy = (y0 + y1) * 0.5f - (ky0 + ky1) * 0.5f;
    const float rho2 = dx * dx + dy * dy;
    const float ex = fmaxf(kx1, x1) - fminf(kx0, x0);
    const float ey = fmaxf(ky1, y1) - fminf(ky0, y0);
    const float c2 = ex * ex + ey * ey;
    return !(iou - rho2 / c2 <= thr);
}

template <int CRIT>
__device__ __forceinline__ bool nms_test(float kx0, float ky0, float kx1, float ky1, float karea, float x0, float y0, float x1, float y1,
                                         float area, float thr) {
    if (CRIT == Y3_NMS_DIOU) return nms_suppressed_diou(kx0, ky0, kx1, ky1, karea, x0, y0, x1, y1, area, thr);
    return nms_suppressed(kx0, ky0, kx1, ky1, karea, x0, y0, x1, y1, area, thr);
}

// bbox_utils.filter_small_boxes (bbox_utils.py:274-281): indices of the rows with (x1 - x0) > min AND (y1 - y0) > min (strict),
// in row order.  One 1024-thread workgroup: per-chunk ballots + an exclusive scan over the 16 waves keep the order.
__global__ __launch_bounds__(1024) void filter_small_kernel(const float* __restrict__ rows, int m, int ld, float min_size, int* __restrict__ idx,
                                                            int* __restrict__ count) {
    __shared__ int wave_cnt[16];
    __shared__ int base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int r0 = 0; r0 < m; r0 += 1024) {
        const int r = r0 + threadIdx.x;
        bool keep = false;
        if (r < m) {
            const float* b = rows + (size_t)r * ld;
            keep = (b[2] - b[0]) > min_size && (b[3] - b[1]) > min_size;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int wv = 0; wv < wave; ++wv) off += wave_cnt[wv];
        if (keep) idx[off + __popcll(bal & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int wv = 0; wv < 16; ++wv) t += wave_cnt[wv];
            base += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}
extern "C" int y3_filter_small_boxes(const float* rows, int m, int ld, float min_size, int* keep_idx, int* keep_cnt, y3_stream_t stream) {
    Y3_CHECK_ARG(rows && keep_idx && keep_cnt && m > 0 && ld >= 4, "filter_small_boxes: bad args");
    hipLaunchKernelGGL(filter_small_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, m, ld, min_size, keep_idx, keep_cnt);
    Y3_CHECK_LAUNCH("filter_small_boxes");
    return Y3_OK;
}

// bbox_utils.compute_iou (bbox_utils.py:200-214): IoU of one corner box against m boxes, same operation order as above
__global__ void compute_iou_kernel(const float* __restrict__ box, const float* __restrict__ boxes, int m, int ld, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const float kx0 = box[0], ky0 = box[1], kx1 = box[2], ky1 = box[3];
    const float* b = boxes + (size_t)i * ld;
    const float x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
    const float karea = (kx1 - kx0) * (ky1 - ky0), area = (x1 - x0) * (y1 - y0);
    const float xl = fmaxf(kx0, x0), yt = fmaxf(ky0, y0);
    const float xr = fminf(kx1, x1), yb = fminf(ky1, y1);
    const float inter = fmaxf(yb - yt, 0.f) * fmaxf(xr - xl, 0.f);
    out[i] = inter / ((karea + area) - inter);
}
extern "C" int y3_compute_iou(const float* box4, const float* boxes, int m, int ld, float* iou, y3_stream_t stream) {
    Y3_CHECK_ARG(box4 && boxes && iou && m > 0 && ld >= 4, "compute_iou: bad args");
    hipLaunchKernelGGL(compute_iou_kernel, dim3(y3_cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, box4, boxes, m, ld, iou);
    Y3_CHECK_LAUNCH("compute_iou");
    return Y3_OK;
}

// A row's box, clipped to [0,clip_w]x[0,clip_h] when clip_w > 0
__device__ __forceinline__ void nms_load_box(const NmsArgs& p, const float* r, float& x0, float& y0, float& x1, float& y1) {
    x0 = r[0];
    y0 = r[1];
    x1 = r[2];
    y1 = r[3];
    if (p.clip_w > 0.f) {
        x0 = fminf(fmaxf(x0, 0.f), p.clip_w);
        x1 = fminf(fmaxf(x1, 0.f), p.clip_w);
        y0 = fminf(fmaxf(y0, 0.f), p.clip_h);
        y1 = fminf(fmaxf(y1, 0.f), p.clip_h);
    }
}

// The candidate test every NMS method shares: clip, small-box filter (strict >), score = sqrt(cls*obj) >= thr
__device__ __forceinline__ bool nms_candidate(const NmsArgs& p, const float* r, int cls, float& x0, float& y0, float& x1, float& y1,
                                              float& score) {
    nms_load_box(p, r, x0, y0, x1, y1);
    const float w = x1 - x0, h = y1 - y0;
    score = p.raw ? r[4] : sqrtf(r[5 + cls] * r[4]);
    // labelled rows: column 5 names the one class the row belongs to; the order key is the score's bit pattern, so only a
    // positive score is a candidate (0 would give row 0 the padding key, a negative one would sort first; NaN fails too)
    if (p.raw == 2 && !(r[5] == (float)cls && score > 0.f)) return false;
    return w > p.min_box && h > p.min_box && score >= p.score_thr;
}

// CRIT: Y3_NMS_HARD (nms_suppressed) or Y3_NMS_DIOU (nms_suppressed_diou); the greedy rounds are the same.  Y3_NMS_NONE (y3_nms_labelled
// only): sort, then every candidate is kept
template <bool LDS_KEYS, int CRIT>
__global__ __launch_bounds__(1024) void nms_kernel(const NmsArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_count, s_kept, s_nk;
    __shared__ float s_kb[5][64];

    const int tid = threadIdx.x;
    const int img = blockIdx.x / p.K, cls = blockIdx.x % p.K;
    const float* rows = p.rows + (long long)img * p.nb * p.D;
    unsigned char* wsb = p.ws + (size_t)blockIdx.x * p.ws_per_block;
    // workspace layout per block: boxes SoA [5][cap] floats | keys [cap] u64 | dead [cap] bytes  (keys/dead only when !LDS_KEYS)
    float* bx0 = (float*)wsb;
    float* by0 = bx0 + p.cap;
    float* bx1 = by0 + p.cap;
    float* by1 = bx1 + p.cap;
    float* bar = by1 + p.cap;
    unsigned long long* keys = LDS_KEYS ? (unsigned long long*)smem : (unsigned long long*)(wsb + (size_t)p.cap * 20);
    unsigned char* dead = LDS_KEYS ? (smem + (size_t)p.cap * 8) : (wsb + (size_t)p.cap * 28);

    if (tid == 0) {
        s_count = 0;
        s_kept = 0;
    }
    __syncthreads();

    // 1. candidates: small-box filter (strict >), score = sqrt(cls*obj) >= thr
    for (int i = tid; i < p.nb; i += 1024) {
        float x0, y0, x1, y1, score;
        if (nms_candidate(p, rows + (long long)i * p.D, cls, x0, y0, x1, y1, score)) {
            const int slot = atomicAdd(&s_count, 1);
            keys[slot] = ((unsigned long long)__float_as_uint(score) << 32) | (unsigned)i;
        }
    }
    __syncthreads();
    const int count = s_count;
    int n2 = 1;
    while (n2 < count) n2 <<= 1;
    for (int i = count + tid; i < n2; i += 1024) keys[i] = 0ull;
    for (int i = tid; i < n2; i += 1024) dead[i] = 0;
    __syncthreads();

    // 2. bitonic sort, descending on (score bits, row index): ties -> higher row index first
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += 1024) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // index with bit j clear
                const int hi = lo | j;
                const bool desc = (lo & k) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a < b) == desc) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }

    // Y3_NMS_NONE: the sorted candidates are the keep list (no IoU is formed, so degenerate boxes cannot drop anything); the greedy
    // rounds are not instantiated
    if constexpr (CRIT == Y3_NMS_NONE) {
        int* o_idx = p.keep_idx + (long long)blockIdx.x * p.max_keep;
        float* o_sc = p.keep_score + (long long)blockIdx.x * p.max_keep;
        const int m = count < p.max_keep ? count : p.max_keep;
        for (int i = tid; i < m; i += 1024) {
            o_idx[i] = (int)(unsigned)(keys[i] & 0xffffffffull);
            o_sc[i] = __uint_as_float((unsigned)(keys[i] >> 32));
        }
        if (tid == 0) p.keep_cnt[blockIdx.x] = m;
    } else {
        // 3. gather the sorted boxes (SoA) and their areas
        for (int i = tid; i < count; i += 1024) {
            float x0, y0, x1, y1;
            nms_load_box(p, rows + (long long)(unsigned)(keys[i] & 0xffffffffull) * p.D, x0, y0, x1, y1);
            bx0[i] = x0;
            by0[i] = y0;
            bx1[i] = x1;
            by1[i] = y1;
            bar[i] = (x1 - x0) * (y1 - y0);
        }
        __syncthreads();

        // 4. greedy suppression in sorted order, 64 candidates per round
        int* out_idx = p.keep_idx + (long long)blockIdx.x * p.max_keep;
        float* out_sc = p.keep_score + (long long)blockIdx.x * p.max_keep;
        for (int base = 0; base < count; base += 64) {
            if (tid < 64) {
                const int j = base + tid;
                const bool valid = j < count;
                bool alive = valid && !dead[j];
                float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f, ar = 0.f;
                if (valid) {
                    x0 = bx0[j];
                    y0 = by0[j];
                    x1 = bx1[j];
                    y1 = by1[j];
                    ar = bar[j];
                }
                unsigned long long mask = __ballot(alive);
                unsigned long long kept = 0ull;
                while (mask) {
                    const int k = __ffsll((long long)mask) - 1;
                    kept |= 1ull << k;
                    const float kx0 = __shfl(x0, k), ky0 = __shfl(y0, k), kx1 = __shfl(x1, k), ky1 = __shfl(y1, k), kar = __shfl(ar, k);
                    if (alive && tid > k && nms_test<CRIT>(kx0, ky0, kx1, ky1, kar, x0, y0, x1, y1, ar, p.iou_thr)) alive = false;
                    mask = __ballot(alive) & ~((2ull << k) - 1ull);
                }
                const int nk = __popcll(kept);
                if ((kept >> tid) & 1ull) {
                    const int rank = __popcll(kept & ((1ull << tid) - 1ull));
                    s_kb[0][rank] = x0;
                    s_kb[1][rank] = y0;
                    s_kb[2][rank] = x1;
                    s_kb[3][rank] = y1;
                    s_kb[4][rank] = ar;
                    const int o = s_kept + rank;
                    if (o < p.max_keep) {
                        out_idx[o] = (int)(unsigned)(keys[j] & 0xffffffffull);
                        out_sc[o] = __uint_as_float((unsigned)(keys[j] >> 32));
                    }
                }
                if (tid == 0) s_nk = nk;
            }
            __syncthreads();
            const int nk = s_nk;
            if (tid == 0) s_kept += nk;
            if (nk > 0) {
                for (int j = base + 64 + tid; j < count; j += 1024) {
                    if (dead[j]) continue;
                    const float x0 = bx0[j], y0 = by0[j], x1 = bx1[j], y1 = by1[j], ar = bar[j];
                    for (int q = 0; q < nk; ++q)
                        if (nms_test<CRIT>(s_kb[0][q], s_kb[1][q], s_kb[2][q], s_kb[3][q], s_kb[4][q], x0, y0, x1, y1, ar, p.iou_thr)) {
                            dead[j] = 1;
                            break;
                        }
                }
            }
            __syncthreads();
        }
        if (tid == 0) p.keep_cnt[blockIdx.x] = s_kept < p.max_keep ? s_kept : p.max_keep;
    }
}

// ---------------------------------------------------------------------------
// Soft-NMS (Y3_NMS_SOFT_LINEAR / Y3_NMS_SOFT_GAUSSIAN, yolo3hip.h): one 1024-thread workgroup per (image, class), no sort.
// Candidate state (box, current score) of R > 0: thread t owns rows t + 1024 r (r < R) in registers, rows that are no
// candidate start dead (nb <= 1024 R).  R == 0: the candidates are compacted into the workspace, SoA x0,y0,x1,y1,score,row
// [cap] each, and thread t owns slots t + 1024 r; the slot order does not matter, the key carries the row.
// One emission = the previous pick's decay and prune fused with each thread's argmax of its live keys, a wave max, one LDS
// entry per wave in the half chosen by the emission's parity, ONE barrier, and every thread reducing the 16 wave entries
// itself.  (A wave writes half e&1 at emission e; it can only write that half again at e+2, after the barrier of e+1, which
// every thread reaches only once it has read half e&1 of emission e.)  A dead candidate has score 0: a live one is >= score_thr > 0.
// ---------------------------------------------------------------------------
#define Y3_SOFT_REG_ROWS 8192  // rows above this: candidate state in the workspace (16 rows per thread in registers spill)

__device__ __forceinline__ float soft_decay(float s, float iou, const NmsArgs& p) {
    float t;
    if (p.soft_gauss)
        t = s * expf(-(iou * iou) / p.sigma);
    else
        t = iou > p.iou_thr ? s * (1.0f - iou) : s;
    return (iou != iou || !(t >= p.score_thr)) ? 0.f : t;
}

__device__ __forceinline__ unsigned long long soft_key(float s, int row) {
    return s > 0.f ? ((unsigned long long)__float_as_uint(s) << 32) | (unsigned)row : 0ull;
}

template <int R>
__global__ __launch_bounds__(1024) void soft_nms_kernel(const NmsArgs p) {
    __shared__ unsigned long long s_key[2][16];
    __shared__ float s_box[2][16][4];
    __shared__ int s_count;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.x / p.K, cls = blockIdx.x % p.K;
    const float* rows = p.rows + (long long)img * p.nb * p.D;
    constexpr int NR = R > 0 ? R : 1;
    float cx0[NR], cy0[NR], cx1[NR], cy1[NR], cs[NR];
    // R == 0: workspace SoA
    unsigned char* wsb = p.ws + (size_t)blockIdx.x * p.ws_per_block;
    float* gx0 = (float*)wsb;
    float* gy0 = gx0 + p.cap;
    float* gx1 = gy0 + p.cap;
    float* gy1 = gx1 + p.cap;
    float* gs = gy1 + p.cap;
    int* grow = (int*)(gs + p.cap);
    int count = 0;

    if (R > 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int i = tid + 1024 * r;
            float sc = 0.f;
            cx0[r] = cy0[r] = cx1[r] = cy1[r] = 0.f;
            if (i < p.nb && !nms_candidate(p, rows + (long long)i * p.D, cls, cx0[r], cy0[r], cx1[r], cy1[r], sc)) sc = 0.f;
            cs[r] = sc;
        }
    } else {
        if (tid == 0) s_count = 0;
        __syncthreads();
        for (int i = tid; i < p.nb; i += 1024) {
            float x0, y0, x1, y1, sc;
            if (nms_candidate(p, rows + (long long)i * p.D, cls, x0, y0, x1, y1, sc)) {
                const int slot = atomicAdd(&s_count, 1);
                gx0[slot] = x0;
                gy0[slot] = y0;
                gx1[slot] = x1;
                gy1[slot] = y1;
                gs[slot] = sc;
                grow[slot] = i;
            }
        }
        __syncthreads();
        count = s_count;
    }

    int* out_idx = p.keep_idx + (long long)blockIdx.x * p.max_keep;
    float* out_sc = p.keep_score + (long long)blockIdx.x * p.max_keep;
    float px0 = 0.f, py0 = 0.f, px1 = 0.f, py1 = 0.f, parea = 0.f;
    int prow = -1, emitted = 0;
    for (int e = 0;; ++e) {
        unsigned long long best = 0ull;
        float bx0 = 0.f, by0 = 0.f, bx1 = 0.f, by1 = 0.f;
        if (R > 0) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int row = tid + 1024 * r;
                float sc = cs[r];
                if (sc > 0.f) {
                    if (row == prow)
                        sc = 0.f;
                    else if (prow >= 0)
                        sc = soft_decay(sc, nms_iou(px0, py0, px1, py1, parea, cx0[r], cy0[r], cx1[r], cy1[r], (cx1[r] - cx0[r]) * (cy1[r] - cy0[r])), p);
                    cs[r] = sc;
                }
                const unsigned long long key = soft_key(sc, row);
                if (key > best) {
                    best = key;
                    bx0 = cx0[r];
                    by0 = cy0[r];
                    bx1 = cx1[r];
                    by1 = cy1[r];
                }
            }
        } else {
            for (int j = tid; j < count; j += 1024) {
                float sc = gs[j];
                if (!(sc > 0.f)) continue;
                const int row = grow[j];
                const float x0 = gx0[j], y0 = gy0[j], x1 = gx1[j], y1 = gy1[j];
                if (row == prow)
                    sc = 0.f;
                else if (prow >= 0)
                    sc = soft_decay(sc, nms_iou(px0, py0, px1, py1, parea, x0, y0, x1, y1, (x1 - x0) * (y1 - y0)), p);
                gs[j] = sc;
                const unsigned long long key = soft_key(sc, row);
                if (key > best) {
                    best = key;
                    bx0 = x0;
                    by0 = y0;
                    bx1 = x1;
                    by1 = y1;
                }
            }
        }
        unsigned long long wmax = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(wmax, o);
            wmax = v > wmax ? v : wmax;
        }
        const int par = e & 1;
        if (wmax != 0ull ? best == wmax : lane == 0) {  // live keys are unique (they carry the row)
            s_key[par][wave] = wmax;
            s_box[par][wave][0] = bx0;
            s_box[par][wave][1] = by0;
            s_box[par][wave][2] = bx1;
            s_box[par][wave][3] = by1;
        }
        __syncthreads();
        unsigned long long k = s_key[par][0];
        int w = 0;
#pragma unroll
        for (int q = 1; q < 16; ++q) {
            const unsigned long long v = s_key[par][q];
            if (v > k) {
                k = v;
                w = q;
            }
        }
        if (k == 0ull) break;  // no live candidate left
        px0 = s_box[par][w][0];
        py0 = s_box[par][w][1];
        px1 = s_box[par][w][2];
        py1 = s_box[par][w][3];
        parea = (px1 - px0) * (py1 - py0);
        prow = (int)(unsigned)(k & 0xffffffffull);
        if (tid == 0) {
            out_idx[emitted] = prow;
            out_sc[emitted] = __uint_as_float((unsigned)(k >> 32));
        }
        if (++emitted == p.max_keep) break;  // later emissions would be truncated anyway
    }
    if (tid == 0) p.keep_cnt[blockIdx.x] = emitted;
}

static int nms_cap(int nb) {
    int c = 64;
    while (c < nb) c <<= 1;
    return c;
}
static bool nms_soft(int method) { return method == Y3_NMS_SOFT_LINEAR || method == Y3_NMS_SOFT_GAUSSIAN; }
static size_t nms_ws_per_block(int nb, int method) {
    return nms_soft(method) ? (((size_t)nms_cap(nb) * 24 + 255) & ~(size_t)255) : (((size_t)nms_cap(nb) * 29 + 255) & ~(size_t)255);
}
extern "C" size_t y3_nms_workspace_bytes(int n, int nb, int num_classes) {
    return nms_ws_per_block(nb, Y3_NMS_HARD) * (size_t)n * (size_t)num_classes;
}
extern "C" size_t y3_nms_workspace_bytes_ex(int n, int nb, int num_classes, int method) {
    if (nms_soft(method) && nb <= Y3_SOFT_REG_ROWS) return 0;  // candidate state in registers
    return nms_ws_per_block(nb, method) * (size_t)n * (size_t)num_classes;
}

template <int CRIT>
static void nms_greedy_launch(const NmsArgs& p, int blocks, hipStream_t st, bool* attr_failed) {
    if (p.cap <= 16384) {
        const size_t lds = (size_t)p.cap * 9;  // keys + dead flags, <= 144 KiB of the CU's 160 KiB
        static bool attr_set = false;
        if (!attr_set) {
            if (hipFuncSetAttribute((const void*)nms_kernel<true, CRIT>, hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * 9) != hipSuccess) {
                *attr_failed = true;
                return;
            }
            attr_set = true;
        }
        hipLaunchKernelGGL((nms_kernel<true, CRIT>), dim3(blocks), dim3(1024), lds, st, p);
    } else {
        hipLaunchKernelGGL((nms_kernel<false, CRIT>), dim3(blocks), dim3(1024), 0, st, p);
    }
}

static int nms_launch(const float* rows, int n, int nb, int num_classes, int raw, int method, float min_box, float score_thr, float iou_thr,
                      float sigma, float clip_w, float clip_h, int* keep_idx, int* keep_cnt, float* keep_score, int max_keep, void* workspace,
                      size_t workspace_bytes, y3_stream_t stream) {
    Y3_CHECK_ARG(method >= Y3_NMS_HARD && method <= (raw == 2 ? Y3_NMS_NONE : Y3_NMS_SOFT_GAUSSIAN), "nms: unknown method %d", method);
    Y3_CHECK_ARG(!nms_soft(method) || score_thr > 0.f, "nms: soft-NMS needs score_thr > 0 (got %g)", (double)score_thr);
    Y3_CHECK_ARG(method != Y3_NMS_SOFT_GAUSSIAN || sigma > 0.f, "nms: Gaussian soft-NMS needs sigma > 0 (got %g)", (double)sigma);
    const size_t need = y3_nms_workspace_bytes_ex(n, nb, num_classes, method);
    Y3_CHECK_ARG(rows && keep_idx && keep_cnt && keep_score && (workspace || need == 0), "nms: null pointer");
    Y3_CHECK_ARG(n > 0 && nb > 0 && num_classes > 0 && max_keep > 0, "nms: bad sizes");
    Y3_CHECK_ARG(workspace_bytes >= need, "nms: workspace too small");
    NmsArgs p = {};
    p.rows = rows;
    p.nb = nb;
    p.D = raw == 1 ? 5 : (raw == 2 ? 6 : 5 + num_classes);
    p.K = num_classes;
    p.raw = raw;
    p.min_box = min_box;
    p.score_thr = score_thr;
    p.iou_thr = iou_thr;
    p.clip_w = clip_w;
    p.clip_h = clip_h;
    p.keep_idx = keep_idx;
    p.keep_cnt = keep_cnt;
    p.keep_score = keep_score;
    p.max_keep = max_keep;
    p.cap = nms_cap(nb);
    p.ws = (unsigned char*)workspace;
    p.ws_per_block = nms_ws_per_block(nb, method);
    p.soft_gauss = method == Y3_NMS_SOFT_GAUSSIAN;
    p.sigma = sigma;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = n * num_classes;
    bool attr_failed = false;
    if (method == Y3_NMS_HARD)
        nms_greedy_launch<Y3_NMS_HARD>(p, blocks, st, &attr_failed);
    else if (method == Y3_NMS_DIOU)
        nms_greedy_launch<Y3_NMS_DIOU>(p, blocks, st, &attr_failed);
    else if (method == Y3_NMS_NONE)
        nms_greedy_launch<Y3_NMS_NONE>(p, blocks, st, &attr_failed);
    else if (nb <= Y3_SOFT_REG_ROWS)
        hipLaunchKernelGGL((soft_nms_kernel<Y3_SOFT_REG_ROWS / 1024>), dim3(blocks), dim3(1024), 0, st, p);
    else
        hipLaunchKernelGGL((soft_nms_kernel<0>), dim3(blocks), dim3(1024), 0, st, p);
    if (attr_failed) {
        y3_set_error("nms_per_class: cannot raise dynamic LDS limit");
        return Y3_ELAUNCH;
    }
    Y3_CHECK_LAUNCH("nms");
    return Y3_OK;
}

extern "C" int y3_nms_per_class(const float* rows, int n, int nb, int num_classes, float min_box, float score_thr, float iou_thr,
                                float clip_w, float clip_h, int* keep_idx, int* keep_cnt, float* keep_score, int max_keep, void* workspace,
                                size_t workspace_bytes, y3_stream_t stream) {
    return nms_launch(rows, n, nb, num_classes, 0, Y3_NMS_HARD, min_box, score_thr, iou_thr, 0.f, clip_w, clip_h, keep_idx, keep_cnt,
                      keep_score, max_keep, workspace, workspace_bytes, stream);
}

extern "C" int y3_nms_per_class_ex(const float* rows, int n, int nb, int num_classes, int method, float min_box, float score_thr,
                                   float iou_thr, float sigma, float clip_w, float clip_h, int* keep_idx, int* keep_cnt, float* keep_score,
                                   int max_keep, void* workspace, size_t workspace_bytes, y3_stream_t stream) {
    return nms_launch(rows, n, nb, num_classes, 0, method, min_box, score_thr, iou_thr, sigma, clip_w, clip_h, keep_idx, keep_cnt,
                      keep_score, max_keep, workspace, workspace_bytes, stream);
}

extern "C" int y3_nms_single_class(const float* rows5, int m, float iou_thr, int* keep_idx, int* keep_cnt, float* keep_score, void* workspace,
                                   size_t workspace_bytes, y3_stream_t stream) {
    return nms_launch(rows5, 1, m, 1, 1, Y3_NMS_HARD, -INFINITY, -INFINITY, iou_thr, 0.f, -1.f, -1.f, keep_idx, keep_cnt, keep_score, m,
                      workspace, workspace_bytes, stream);
}

// Class-wise NMS over a pool of labelled detections (the merged tiles of one image): block c takes the rows whose column 5 == c
extern "C" int y3_nms_labelled(const float* pool, int m, int num_classes, int method, float score_thr, float iou_thr, float sigma,
                               int* keep_idx, int* keep_cnt, float* keep_score, int max_keep, void* workspace, size_t workspace_bytes,
                               y3_stream_t stream) {
    return nms_launch(pool, 1, m, num_classes, 2, method, -INFINITY, score_thr, iou_thr, sigma, -1.f, -1.f, keep_idx, keep_cnt, keep_score,
                      max_keep, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------
// box voting over the pooled views of test-time augmentation (y3_box_vote, yolo3hip.h)
// ---------------------------------------------------------------------------
#define Y3_VOTE_CHUNK 256  // candidates staged in LDS per pass = threads per workgroup
#define Y3_VOTE_WAVES 4    // keeps of one (image, class) a workgroup votes at a time, one wave each
#define Y3_VOTE_GRID_X 32  // workgroups per (image, class) at most; each strides over the keeps

struct VoteArgs {
    NmsArgs nms;  // rows, sizes, the candidate test's parameters and the keep lists (read only here)
    float vote_iou;
    int views, rows_per_view;
    float* out;     // [n][K][max_keep][6]
    float* cand;    // [n * K][6][nb]: x0, y0, x1, y1, score, row (as int bits) of the candidates, row order
    int* cand_cnt;  // [n * K]
};

// Pass 1, one 256-thread workgroup per (image, class): the candidates nms_candidate accepts, compacted in row order (ballot
// prefix inside a wave, the four waves' counts in LDS, as truth_boxes_kernel).  No atomics.
__global__ __launch_bounds__(256) void vote_compact_kernel(const VoteArgs a) {
    __shared__ int wave_cnt[4];
    const NmsArgs& p = a.nms;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x, img = seg / p.K, cls = seg - img * p.K;
    const float* rows = p.rows + (long long)img * p.nb * p.D;
    float* out = a.cand + (long long)seg * 6 * p.nb;
    int base = 0;
    for (int r0 = 0; r0 < p.nb; r0 += 256) {
        const int r = r0 + tid;
        float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f, score = 0.f;
        const bool keep = r < p.nb && nms_candidate(p, rows + (long long)r * p.D, cls, x0, y0, x1, y1, score);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
        if (keep) {
            out[pos] = x0;
            out[p.nb + pos] = y0;
            out[2 * p.nb + pos] = x1;
            out[3 * p.nb + pos] = y1;
            out[4 * p.nb + pos] = score;
            out[5 * p.nb + pos] = __int_as_float(r);
        }
        base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    if (tid == 0) a.cand_cnt[seg] = base;
}

// Pass 2, one wave per keep, Y3_VOTE_WAVES keeps of one (image, class) per workgroup: they share the candidate list, staged through
// LDS Y3_VOTE_CHUNK entries at a time.  Candidate p of the list always goes to lane p % 64, a lane adds its members in increasing p,
// and the lanes are combined by the xor butterfly of y3_wave_sum_d: the same bits on every run.  The keep loop and the chunk loop
// are uniform over the workgroup (both bounds come from memory every thread reads alike), so every thread meets every barrier.
template <bool CONSENSUS>
__global__ __launch_bounds__(256) void vote_kernel(const VoteArgs a) {
    __shared__ float s_c[6][Y3_VOTE_CHUNK];
    const NmsArgs& p = a.nms;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.y, img = seg / p.K, cls = seg - img * p.K;
    int cnt = p.keep_cnt[seg];
    cnt = cnt < 0 ? 0 : (cnt > p.max_keep ? p.max_keep : cnt);
    int ncand = a.cand_cnt[seg];
    ncand = ncand > p.nb ? p.nb : ncand;
    const float* cand = a.cand + (long long)seg * 6 * p.nb;
    const float* rows = p.rows + (long long)img * p.nb * p.D;
    for (int j0 = blockIdx.x * Y3_VOTE_WAVES; j0 < cnt; j0 += gridDim.x * Y3_VOTE_WAVES) {
        const int j = j0 + wave;
        const long long e = (long long)seg * p.max_keep + j;
        const int row = j < cnt ? p.keep_idx[e] : -1;
        const bool active = row >= 0 && row < p.nb;  // anything else is never produced by the NMS kernels; nothing outside `rows` is read
        float kx0 = 0.f, ky0 = 0.f, kx1 = 0.f, ky1 = 0.f;
        if (active) nms_load_box(p, rows + (long long)row * p.D, kx0, ky0, kx1, ky1);
        const float karea = (kx1 - kx0) * (ky1 - ky0);
        double ax0 = 0., ay0 = 0., ax1 = 0., ay1 = 0., as = 0.;
        int members = 0;
        float vmax[Y3_TTA_MAX_VIEWS];
#pragma unroll
        for (int v = 0; v < Y3_TTA_MAX_VIEWS; ++v) vmax[v] = 0.f;
        for (int c0 = 0; c0 < ncand; c0 += Y3_VOTE_CHUNK) {
            __syncthreads();  // the chunk before this one has been read by every wave
            if (c0 + tid < ncand) {
#pragma unroll
                for (int f = 0; f < 6; ++f) s_c[f][tid] = cand[(long long)f * p.nb + c0 + tid];
            }
            __syncthreads();
            const int m = ncand - c0 < Y3_VOTE_CHUNK ? ncand - c0 : Y3_VOTE_CHUNK;
            if (active) {
                for (int t = lane; t < m; t += 64) {
                    const float x0 = s_c[0][t], y0 = s_c[1][t], x1 = s_c[2][t], y1 = s_c[3][t], s = s_c[4][t];
                    const float iou = nms_iou(kx0, ky0, kx1, ky1, karea, x0, y0, x1, y1, (x1 - x0) * (y1 - y0));
                    if (iou >= a.vote_iou) {  // NaN: no member
                        const double w = (double)s;
                        ax0 += w * (double)x0;
                        ay0 += w * (double)y0;
                        ax1 += w * (double)x1;
                        ay1 += w * (double)y1;
                        as += w;
                        ++members;
                        if (CONSENSUS) {
                            const int view = __float_as_int(s_c[5][t]) / a.rows_per_view;
#pragma unroll
                            for (int v = 0; v < Y3_TTA_MAX_VIEWS; ++v)
                                if (v == view) vmax[v] = fmaxf(vmax[v], s);
                        }
                    }
                }
            }
        }
        ax0 = y3_wave_sum_d(ax0);
        ay0 = y3_wave_sum_d(ay0);
        ax1 = y3_wave_sum_d(ax1);
        ay1 = y3_wave_sum_d(ay1);
        as = y3_wave_sum_d(as);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) members += __shfl_xor(members, o);
        float score = active ? p.keep_score[e] : 0.f;
        if (CONSENSUS) {
            score = 0.f;
#pragma unroll
            for (int v = 0; v < Y3_TTA_MAX_VIEWS; ++v) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) vmax[v] = fmaxf(vmax[v], __shfl_xor(vmax[v], o));
                if (v < a.views) score += vmax[v];  // fp32, increasing view
            }
            score = score / (float)a.views;
        }
        if (active && lane == 0) {
            float* o = a.out + e * 6;
            const bool own = members == 0 || !(as > 0.);  // a degenerate own box (0 / 0 IoU), or members whose scores are all zero
            o[0] = own ? kx0 : (float)(ax0 / as);
            o[1] = own ? ky0 : (float)(ay0 / as);
            o[2] = own ? kx1 : (float)(ax1 / as);
            o[3] = own ? ky1 : (float)(ay1 / as);
            o[4] = score;
            o[5] = (float)cls;
        }
    }
}

extern "C" size_t y3_box_vote_workspace_bytes(int n, int nb, int num_classes) {
    if (n < 1 || nb < 1 || num_classes < 1) return 0;
    return (size_t)n * (size_t)num_classes * ((size_t)nb * 24 + 4);
}

extern "C" int y3_box_vote(const float* rows, int n, int nb, int num_classes, const int* keep_idx, const int* keep_cnt, const float* keep_score,
                           int max_keep, float min_box, float score_thr, float clip_w, float clip_h, float vote_iou, int views,
                           int rows_per_view, int score_mode, float* out, void* workspace, size_t workspace_bytes, y3_stream_t stream) {
    Y3_CHECK_ARG(rows && keep_idx && keep_cnt && keep_score && out && workspace, "box_vote: null pointer");
    Y3_CHECK_ARG(n >= 1 && nb >= 1 && num_classes >= 1 && max_keep >= 1, "box_vote: bad sizes (n %d, nb %d, classes %d, max_keep %d)", n, nb,
                 num_classes, max_keep);
    Y3_CHECK_ARG((long long)n * num_classes <= 65535, "box_vote: n * classes = %lld (at most 65535 per call)", (long long)n * num_classes);
    Y3_CHECK_ARG((long long)n * num_classes * max_keep * 6 < (1LL << 31), "box_vote: n * classes * max_keep * 6 overflows");
    Y3_CHECK_ARG(views >= 1 && views <= Y3_TTA_MAX_VIEWS && rows_per_view >= 1 && (long long)views * rows_per_view == nb,
                 "box_vote: %d views of %d rows are not the %d rows of an image (1 .. %d views)", views, rows_per_view, nb, Y3_TTA_MAX_VIEWS);
    Y3_CHECK_ARG(vote_iou > 0.f && vote_iou <= 1.f, "box_vote: vote_iou %g outside (0, 1]", (double)vote_iou);
    Y3_CHECK_ARG(score_mode == Y3_VOTE_SCORE_KEEP || score_mode == Y3_VOTE_SCORE_CONSENSUS, "box_vote: unknown score mode %d", score_mode);
    Y3_CHECK_ARG(workspace_bytes >= y3_box_vote_workspace_bytes(n, nb, num_classes), "box_vote: workspace too small");
    VoteArgs a = {};
    a.nms.rows = rows;
    a.nms.nb = nb;
    a.nms.D = 5 + num_classes;
    a.nms.K = num_classes;
    a.nms.min_box = min_box;
    a.nms.score_thr = score_thr;
    a.nms.clip_w = clip_w;
    a.nms.clip_h = clip_h;
    a.nms.keep_idx = const_cast<int*>(keep_idx);
    a.nms.keep_cnt = const_cast<int*>(keep_cnt);
    a.nms.keep_score = const_cast<float*>(keep_score);
    a.nms.max_keep = max_keep;
    a.vote_iou = vote_iou;
    a.views = views;
    a.rows_per_view = rows_per_view;
    a.out = out;
    a.cand = (float*)workspace;
    a.cand_cnt = (int*)((float*)workspace + (size_t)n * num_classes * 6 * nb);
    hipStream_t st = (hipStream_t)stream;
    const int segs = n * num_classes;
    hipLaunchKernelGGL(vote_compact_kernel, dim3(segs), dim3(256), 0, st, a);
    Y3_CHECK_LAUNCH("box_vote (candidates)");
    const int per = y3_cdiv(max_keep, Y3_VOTE_WAVES);
    const dim3 grid(per < Y3_VOTE_GRID_X ? per : Y3_VOTE_GRID_X, segs);
    if (score_mode == Y3_VOTE_SCORE_CONSENSUS)
        hipLaunchKernelGGL(vote_kernel<true>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(vote_kernel<false>, grid, dim3(256), 0, st, a);
    Y3_CHECK_LAUNCH("box_vote");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// ground-truth label tensors (ImageReader.__format_boxes, imagereader.py:252-324)
// ---------------------------------------------------------------------------
// One launch writes the three label tensors [N, G, G, A, 5+K] completely.  The flat tensor of a scale is cut into runs of whole
// cells; a workgroup owns one run: it zero-fills it (16-byte stores between an unaligned head and tail), then walks the boxes of the
// images its run touches, Y3_LABEL_CHUNK at a time and in input order, and writes the rows of the boxes whose cell lies in the run.
// Nothing outside the run is written, so no workgroup depends on another and the result does not depend on the order waves run in.
// Within a chunk the objectness and class stores all write 1.0 (any order gives the same bits); the four coordinates of a
// (cell, anchor) are stored by the LAST box of the chunk that lands there (the keys of the chunk sit in LDS), and a barrier
// between chunks puts a later chunk's stores after an earlier one's: the state the host's sequential loop leaves.
//
// Arithmetic: every step is the float32 operation NumPy performs in format_boxes, in its order, under -ffp-contract=off:
// centre = floor(xy + (wh - 1) / 2); the anchor IoU as min / max / product / (sum - inter) / quotient with the first maximum
// winning (np.argmax); the cell index as floor((c / size) * G) with `size` and `G` converted to float32 and an IEEE division
// followed by an IEEE multiplication -- the FLOAT32 evaluation of `boxes[t, 1] / image_size[0] * g[0]` (NumPy 2 keeps a float32
// scalar float32 against a Python int), which is neither c // stride nor the float64 evaluation: side 352, stride 16, centre
// 208 gives cell 12, not 13.  No reciprocal, no fast-math.
#define Y3_LABEL_CHUNK 256          // boxes per pass = threads per workgroup; max_boxes is not bounded by it
#define Y3_LABEL_RUN_FLOATS 16384   // floats a workgroup owns (rounded to whole cells): 16 x 16-byte stores per thread

struct LabelArgs {
    const int* boxes;   // [N][max_boxes][5]
    const int* counts;  // [N]
    float* out[3];
    int gh[3], gw[3];
    int block_start[4];  // first workgroup of each scale
    int N, max_boxes, A, K;
    int cells_per_block;
    float img_h, img_w;
    float aw[Y3_MAX_ANCHORS], ah[Y3_MAX_ANCHORS];
};

__global__ __launch_bounds__(Y3_LABEL_CHUNK) void format_labels_kernel(const LabelArgs p) {
    __shared__ int key[Y3_LABEL_CHUNK];
    const int tid = threadIdx.x;
    int s = 0;
    while (s < 2 && (int)blockIdx.x >= p.block_start[s + 1]) ++s;
    const int gh = p.gh[s], gw = p.gw[s];
    const int D = 5 + p.K, AD = p.A * D;
    const long long cells = (long long)gh * gw;
    const long long total = cells * p.N;
    const long long c0 = (long long)((int)blockIdx.x - p.block_start[s]) * p.cells_per_block;
    const long long c1 = c0 + p.cells_per_block < total ? c0 + p.cells_per_block : total;
    float* const base = p.out[s];

    // zero fill of [c0, c1) cells
    {
        float* f = base + c0 * AD;
        const long long cnt = (c1 - c0) * AD;
        long long head = (long long)(((16u - (unsigned)((uintptr_t)f & 15u)) & 15u) >> 2);
        if (head > cnt) head = cnt;
        const long long nv = (cnt - head) >> 2;
        float4* v = reinterpret_cast<float4*>(f + head);
        for (long long i = tid; i < nv; i += Y3_LABEL_CHUNK) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < head) f[tid] = 0.f;
        const long long tail0 = head + (nv << 2);
        if (tail0 + tid < cnt) f[tail0 + tid] = 0.f;      // < 4 floats
    }
    __syncthreads();

    const int n0 = (int)(c0 / cells), n1 = (int)((c1 - 1) / cells);
    for (int n = n0; n <= n1; ++n) {
        int cnt = p.counts[n];
        cnt = cnt < 0 ? 0 : (cnt > p.max_boxes ? p.max_boxes : cnt);
        const int* bx = p.boxes + (long long)n * p.max_boxes * 5;
        for (int t0 = 0; t0 < cnt; t0 += Y3_LABEL_CHUNK) {
            const int t = t0 + tid;
            int k = -1, cls = 0;
            float cx = 0.f, cy = 0.f, w = 0.f, h = 0.f;
            if (t < cnt) {
                const float x = (float)bx[t * 5 + 0], y = (float)bx[t * 5 + 1];
                w = (float)bx[t * 5 + 2];
                h = (float)bx[t * 5 + 3];
                cls = bx[t * 5 + 4];
                cx = floorf(x + (w - 1.f) / 2.0f);
                cy = floorf(y + (h - 1.f) / 2.0f);
                int best = 0;
                float best_iou = 0.f;
                for (int a = 0; a < p.A; ++a) {
                    const float aw = p.aw[a], ah = p.ah[a];
                    const float iw = fmaxf(fminf(w / 2.0f, aw / 2.0f) - fmaxf(-w / 2.0f, -aw / 2.0f), 0.0f);
                    const float ih = fmaxf(fminf(h / 2.0f, ah / 2.0f) - fmaxf(-h / 2.0f, -ah / 2.0f), 0.0f);
                    const float inter = iw * ih;
                    const float iou = inter / (w * h + aw * ah - inter);
                    if (a == 0 || iou > best_iou) {
                        best = a;
                        best_iou = iou;
                    }
                }
                const float fi = floorf(cy / p.img_h * (float)gh);
                const float fj = floorf(cx / p.img_w * (float)gw);
                // a cell or class outside the tensor (where the host loop raises or wraps around) writes nothing
                if (fi >= 0.f && fi < (float)gh && fj >= 0.f && fj < (float)gw && cls >= 0 && cls < p.K) {
                    const long long cell = (long long)n * cells + (long long)((int)fi * gw + (int)fj);
                    if (cell >= c0 && cell < c1) k = (int)(cell - c0) * p.A + best;
                }
            }
            key[tid] = k;
            __syncthreads();
            if (k >= 0) {
                float* row = base + c0 * AD + (long long)k * D;
                bool last = true;
                const int lim = cnt - t0 < Y3_LABEL_CHUNK ? cnt - t0 : Y3_LABEL_CHUNK;
                for (int u = tid + 1; u < lim; ++u) last = last && key[u] != k;
                if (last) {
                    row[0] = cx;
                    row[1] = cy;
                    row[2] = w;
                    row[3] = h;
                }
                row[4] = 1.0f;
                row[5 + cls] = 1.0f;
            }
            __syncthreads();      // the next chunk's stores (and its keys) come after this chunk's
        }
    }
}

extern "C" int y3_format_labels(const int* boxes, const int* counts, int n, int max_boxes, const float* anchors_host, int num_anchors,
                                int num_classes, int img_h, int img_w, float* out1, float* out2, float* out3, y3_stream_t stream) {
    Y3_CHECK_ARG(counts && anchors_host && out1 && out2 && out3, "format_labels: null pointer");
    Y3_CHECK_ARG(max_boxes >= 0 && (boxes || max_boxes == 0), "format_labels: max_boxes %d%s", max_boxes, boxes ? "" : " with null boxes");
    Y3_CHECK_ARG(n >= 1 && num_anchors >= 1 && num_anchors <= Y3_MAX_ANCHORS && num_classes >= 1, "format_labels: n %d anchors %d classes %d", n,
                 num_anchors, num_classes);
    Y3_CHECK_ARG(img_h >= 32 && img_w >= 32 && img_h % 32 == 0 && img_w % 32 == 0 && img_h < (1 << 24) && img_w < (1 << 24),
                 "format_labels: image %dx%d (multiples of 32)", img_h, img_w);
    Y3_CHECK_ARG((long long)n * max_boxes * 5 < (1LL << 31), "format_labels: %d x %d boxes too many", n, max_boxes);
    LabelArgs p = {};
    p.boxes = boxes;
    p.counts = counts;
    p.out[0] = out1;
    p.out[1] = out2;
    p.out[2] = out3;
    p.N = n;
    p.max_boxes = max_boxes;
    p.A = num_anchors;
    p.K = num_classes;
    p.img_h = (float)img_h;
    p.img_w = (float)img_w;
    const int AD = num_anchors * (5 + num_classes);
    p.cells_per_block = Y3_LABEL_RUN_FLOATS / AD > 0 ? Y3_LABEL_RUN_FLOATS / AD : 1;
    Y3_CHECK_ARG((long long)p.cells_per_block * AD < (1LL << 31), "format_labels: %d classes too many", num_classes);
    long long blocks = 0;
    for (int s = 0; s < 3; ++s) {
        p.gh[s] = img_h / (32 >> s);
        p.gw[s] = img_w / (32 >> s);
        p.block_start[s] = (int)blocks;
        blocks += ((long long)n * p.gh[s] * p.gw[s] + p.cells_per_block - 1) / p.cells_per_block;
        Y3_CHECK_ARG(blocks < (1LL << 31), "format_labels: labels too large");
    }
    p.block_start[3] = (int)blocks;
    for (int a = 0; a < num_anchors; ++a) {
        p.aw[a] = anchors_host[2 * a];
        p.ah[a] = anchors_host[2 * a + 1];
    }
    hipLaunchKernelGGL(format_labels_kernel, dim3((unsigned)blocks), dim3(Y3_LABEL_CHUNK), 0, (hipStream_t)stream, p);
    Y3_CHECK_LAUNCH("format_labels");
    return Y3_OK;
}
