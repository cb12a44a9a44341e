// Detection accuracy on the device: matching of NMS keep lists against ground truth and 101-point AP (yolo3hip.h,
// DESIGN §3.6).  Compiled with -ffp-contract=off: the IoU must round exactly like compute_iou_kernel (detect.hip) and the
// NumPy float32 mirror of the tests, so the TP bits are reproducible bit for bit.
#include "common.h"

#define Y3_EVAL_MAX_GT 4096   // ground-truth boxes of one (image, class) staged in LDS: 20 B each -> 80 KiB
#define Y3_EVAL_MAX_THR 32    // IoU thresholds: one bit each of the uint32 TP mask

// ---------------------------------------------------------------------------
// pool offsets: exclusive prefix over the (image, class) keep counts, image-major
// ---------------------------------------------------------------------------
__device__ __forceinline__ int eval_kept(const int* keep_cnt, int seg, int max_keep, int max_det) {
    int c = keep_cnt[seg];
    c = c < max_keep ? c : max_keep;
    c = c < max_det ? c : max_det;
    return c > 0 ? c : 0;
}

// One 1024-thread workgroup: per-chunk wave prefix (shuffles) + an exclusive scan over the 16 wave totals.
__global__ __launch_bounds__(1024) void eval_offsets_kernel(const int* __restrict__ keep_cnt, int nseg, int max_keep, int max_det,
                                                            int* __restrict__ offsets) {
    __shared__ int wave_tot[16];
    __shared__ int base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int s0 = 0; s0 < nseg; s0 += 1024) {
        const int s = s0 + threadIdx.x;
        const int v = s < nseg ? eval_kept(keep_cnt, s, max_keep, max_det) : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wave_tot[w];
        if (s < nseg) offsets[s] = off + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += wave_tot[w];
            base += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[nseg] = base;
}

extern "C" int y3_eval_offsets(const int* keep_cnt, int nseg, int max_keep, int max_det, int* offsets, y3_stream_t stream) {
    Y3_CHECK_ARG(keep_cnt && offsets, "eval_offsets: null pointer");
    Y3_CHECK_ARG(nseg >= 1 && max_keep >= 1 && max_det >= 1, "eval_offsets: bad sizes (nseg %d, max_keep %d, max_det %d)", nseg, max_keep,
                 max_det);
    hipLaunchKernelGGL(eval_offsets_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, keep_cnt, nseg, max_keep, max_det, offsets);
    Y3_CHECK_LAUNCH("eval_offsets");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// matching: one workgroup per (image, class), one wave per IoU threshold
// ---------------------------------------------------------------------------
struct EvalMatchArgs {
    const float* rows;
    int nb, ld, K;
    float clip_w, clip_h;
    const int* keep_idx;
    const int* keep_cnt;
    const float* keep_score;
    int max_keep, max_det;
    const float* gt;
    const int* gt_cnt;
    int max_gt, cap;  // cap: LDS slots per coordinate (>= the caller's per-(image, class) bound, multiple of 64)
    float thr[Y3_EVAL_MAX_THR];
    int T;
    const int* offsets;
    long long* pool_key;
    unsigned* pool_tp;
    long long pool_capacity;
};

// order-preserving map of a float onto uint32 (ascending float -> ascending key)
__device__ __forceinline__ unsigned eval_mono(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(1024) void eval_match_kernel(const EvalMatchArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sg[];  // SoA [5][cap]: x0, y0, x1, y1, area of the class's GT boxes
    __shared__ int s_ng;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int seg = blockIdx.x;
    const int img = seg / p.K, cls = seg - img * p.K;
    float* gx0 = sg;
    float* gy0 = gx0 + p.cap;
    float* gx1 = gy0 + p.cap;
    float* gy1 = gx1 + p.cap;
    float* gar = gy1 + p.cap;

    const int cnt = eval_kept(p.keep_cnt, seg, p.max_keep, p.max_det);
    const long long out0 = p.offsets[seg];
    // 1. pool entries of this (image, class): sort key (class asc, score desc) and a cleared TP mask
    for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
        const long long o = out0 + j;
        if (o < p.pool_capacity) {
            const float sc = p.keep_score[(long long)seg * p.max_keep + j];
            p.pool_key[o] = ((long long)cls << 32) | (long long)(unsigned)~eval_mono(sc);
            p.pool_tp[o] = 0u;
        }
    }
    // 2. wave 0 compacts the image's GT boxes of this class into LDS, in GT order (ballot + popcount)
    if (wave == 0) {
        int ng = p.gt_cnt[img];
        ng = ng < p.max_gt ? ng : p.max_gt;
        const float* g = p.gt + (long long)img * p.max_gt * 5;
        int base = 0;
        for (int g0 = 0; g0 < ng; g0 += 64) {
            const int i = g0 + lane;
            float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
            bool mine = false;
            if (i < ng) {
                const float* b = g + (long long)i * 5;
                x0 = b[0];
                y0 = b[1];
                x1 = b[2];
                y1 = b[3];
                mine = b[4] == (float)cls;
            }
            const unsigned long long bal = __ballot(mine);
            const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
            if (mine && pos < p.cap) {
                gx0[pos] = x0;
                gy0[pos] = y0;
                gx1[pos] = x1;
                gy1[pos] = y1;
                gar[pos] = (x1 - x0) * (y1 - y0);
            }
            base += __popcll(bal);
        }
        if (lane == 0) s_ng = base < p.cap ? base : p.cap;
    }
    __syncthreads();
    const int G = s_ng;
    if (cnt == 0) return;
    const float* rows = p.rows + (long long)img * p.nb * p.ld;
    const int* kidx = p.keep_idx + (long long)seg * p.max_keep;

    // 3. greedy matching in keep order, one wave per threshold; no barriers from here on.  Lane l owns GT boxes
    //    l, l + 64, ...; their matched flags are the bits of one 64-bit register (G <= 4096 = 64 x 64).
    for (int t = wave; t < p.T; t += nwaves) {
        const float thr = p.thr[t];
        unsigned long long matched = 0ull;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            // lane l stages detection j0 + l (clipped like y3_nms_per_class / bbox_utils.detect_async)
            const int j = j0 + lane;
            float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
            bool ok = false;
            if (j < cnt) {
                const int r = kidx[j];
                if (r >= 0 && r < p.nb) {
                    const float* b = rows + (long long)r * p.ld;
                    x0 = b[0];
                    y0 = b[1];
                    x1 = b[2];
                    y1 = b[3];
                    if (p.clip_w > 0.f) {
                        x0 = fminf(fmaxf(x0, 0.f), p.clip_w);
                        x1 = fminf(fmaxf(x1, 0.f), p.clip_w);
                        y0 = fminf(fmaxf(y0, 0.f), p.clip_h);
                        y1 = fminf(fmaxf(y1, 0.f), p.clip_h);
                    }
                    ok = true;
                }
            }
            const float ar = (x1 - x0) * (y1 - y0);
            const unsigned long long okmask = __ballot(ok);
            const int nj = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int k = 0; k < nj; ++k) {
                if (!((okmask >> k) & 1ull)) continue;
                const float kx0 = __shfl(x0, k), ky0 = __shfl(y0, k), kx1 = __shfl(x1, k), ky1 = __shfl(y1, k), kar = __shfl(ar, k);
                // key = (IoU bits << 32) | (g + 1): IoU >= thr > 0 makes the bits monotone; the max takes the highest g on ties
                unsigned long long best = 0ull;
                int bit = 0;
                for (int g = lane; g < G; g += 64, ++bit) {
                    if ((matched >> bit) & 1ull) continue;
                    const float xl = fmaxf(kx0, gx0[g]), yt = fmaxf(ky0, gy0[g]);
                    const float xr = fminf(kx1, gx1[g]), yb = fminf(ky1, gy1[g]);
                    const float inter = fmaxf(yb - yt, 0.f) * fmaxf(xr - xl, 0.f);
                    const float iou = inter / ((kar + gar[g]) - inter);
                    if (iou >= thr) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)(g + 1);
                        best = key > best ? key : best;
                    }
                }
                if (!__ballot(best != 0ull)) continue;  // no candidate anywhere (an FP): skip the reduction
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long other = __shfl_xor(best, o);
                    best = other > best ? other : best;
                }
                if (best) {
                    const int g = (int)(unsigned)(best & 0xffffffffull) - 1;
                    if (lane == (g & 63)) matched |= 1ull << (g >> 6);
                    const long long o = out0 + j0 + k;
                    if (lane == 0 && o < p.pool_capacity) atomicOr(&p.pool_tp[o], 1u << t);
                }
            }
        }
    }
}

extern "C" int y3_eval_match(const float* rows, int n, int nb, int ld, int num_classes, float clip_w, float clip_h, const int* keep_idx,
                             const int* keep_cnt, const float* keep_score, int max_keep, int max_det, const float* gt, const int* gt_cnt,
                             int max_gt, int max_gt_per_class, const float* iou_thr_host, int num_thr, const int* offsets,
                             long long* pool_key, unsigned* pool_tp, long long pool_capacity, y3_stream_t stream) {
    Y3_CHECK_ARG(rows && keep_idx && keep_cnt && keep_score && gt && gt_cnt && iou_thr_host && offsets && pool_key && pool_tp,
                 "eval_match: null pointer");
    Y3_CHECK_ARG(n >= 1 && nb >= 1 && ld >= 4 && num_classes >= 1 && max_keep >= 1 && max_det >= 1 && max_gt >= 1 && pool_capacity >= 0,
                 "eval_match: bad sizes (n %d, nb %d, ld %d, classes %d, max_keep %d, max_det %d, max_gt %d)", n, nb, ld, num_classes,
                 max_keep, max_det, max_gt);
    Y3_CHECK_ARG(num_thr >= 1 && num_thr <= Y3_EVAL_MAX_THR, "eval_match: %d IoU thresholds (1..%d)", num_thr, Y3_EVAL_MAX_THR);
    Y3_CHECK_ARG(max_gt_per_class >= 0 && max_gt_per_class <= Y3_EVAL_MAX_GT,
                 "eval_match: %d ground-truth boxes in one (image, class); at most %d fit the LDS stage", max_gt_per_class,
                 Y3_EVAL_MAX_GT);
    Y3_CHECK_ARG((long long)n * num_classes <= 0x7fffffffLL, "eval_match: n * classes overflows");
    EvalMatchArgs p = {};
    for (int t = 0; t < num_thr; ++t) {
        const float v = iou_thr_host[t];
        Y3_CHECK_ARG(v > 0.f && v <= 1.f, "eval_match: IoU threshold %d = %g outside (0, 1]", t, (double)v);
        p.thr[t] = v;
    }
    p.rows = rows;
    p.nb = nb;
    p.ld = ld;
    p.K = num_classes;
    p.clip_w = clip_w;
    p.clip_h = clip_h;
    p.keep_idx = keep_idx;
    p.keep_cnt = keep_cnt;
    p.keep_score = keep_score;
    p.max_keep = max_keep;
    p.max_det = max_det;
    p.gt = gt;
    p.gt_cnt = gt_cnt;
    p.max_gt = max_gt;
    p.cap = max_gt_per_class < 64 ? 64 : (max_gt_per_class + 63) & ~63;
    p.T = num_thr;
    p.offsets = offsets;
    p.pool_key = pool_key;
    p.pool_tp = pool_tp;
    p.pool_capacity = pool_capacity;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)eval_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Y3_EVAL_MAX_GT * 20) !=
            hipSuccess) {
            y3_set_error("eval_match: cannot raise the dynamic LDS limit");
            return Y3_ELAUNCH;
        }
        attr_set = true;
    }
    const int waves = num_thr < 16 ? num_thr : 16;
    hipLaunchKernelGGL(eval_match_kernel, dim3(n * num_classes), dim3(64 * waves), (size_t)p.cap * 20, (hipStream_t)stream, p);
    Y3_CHECK_LAUNCH("eval_match");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// AP: one 256-thread workgroup per (class, threshold) over the class-sorted pool
// ---------------------------------------------------------------------------
__device__ __forceinline__ long long eval_lower_bound(const long long* keys, long long m, long long v) {
    long long lo = 0, hi = m;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void eval_ap_kernel(const long long* __restrict__ keys, const unsigned* __restrict__ tp, long long m, int T,
                                                      const int* __restrict__ npos_dev, float* __restrict__ ws, float* __restrict__ ap,
                                                      float* __restrict__ recall, int* __restrict__ tp_out, int* __restrict__ fp_out) {
    __shared__ long long s_range[2];
    __shared__ int wtot[4];
    __shared__ float wmax[4];
    __shared__ double terms[101];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cls = blockIdx.x / T, t = blockIdx.x - cls * T;
    if (threadIdx.x < 2) s_range[threadIdx.x] = eval_lower_bound(keys, m, (long long)(cls + threadIdx.x) << 32);
    __syncthreads();
    const long long s = s_range[0], e = s_range[1];
    const int npos = npos_dev[cls];
    float* prec = ws + (long long)t * m + s;  // precision at the q-th TP, then its suffix max (the envelope)

    // 1. tp_cum by a chunked block scan of the TP bits; precision = tp_cum / (rank + 1) at every TP
    long long ntp = 0;
    for (long long b0 = s; b0 < e; b0 += 256) {
        const long long i = b0 + threadIdx.x;
        const bool hit = i < e && ((tp[i] >> t) & 1u);
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        long long q = ntp + __popcll(bal & ((1ull << lane) - 1ull)) + 1;
        for (int w = 0; w < wave; ++w) q += wtot[w];
        if (hit) prec[q - 1] = (float)q / (float)(i - s + 1);
        ntp += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    // 2. envelope: reverse max-scan over the TP precisions, chunks from the end
    float carry = 0.f;
    for (long long end = ntp; end > 0; end -= 256) {
        const long long st = end - 256 > 0 ? end - 256 : 0;
        const long long i = st + threadIdx.x;
        float v = i < end ? prec[i] : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float u = __shfl_down(v, o);
            if (lane + o < 64) v = fmaxf(v, u);
        }
        if (lane == 0) wmax[wave] = v;
        __syncthreads();
        for (int w = wave + 1; w < 4; ++w) v = fmaxf(v, wmax[w]);
        v = fmaxf(v, carry);
        if (i < end) prec[i] = v;
        carry = fmaxf(carry, fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
        __syncthreads();
    }
    // 3. 101 points: recall j/100 is first reached at the ceil(j npos / 100)-th TP (index 0 when that is 0)
    if (threadIdx.x <= 100) {
        const long long need = ((long long)threadIdx.x * npos + 99) / 100;
        float v = 0.f;
        if (e > s) {
            if (need == 0) v = ntp > 0 ? prec[0] : 0.f;
            else if (need <= ntp) v = prec[need - 1];
        }
        terms[threadIdx.x] = (double)v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int j = 0; j <= 100; ++j) sum += terms[j];
        const int o = cls * T + t;
        ap[o] = npos > 0 ? (float)(sum / 101.0) : __builtin_nanf("");
        recall[o] = npos > 0 ? (float)ntp / (float)npos : __builtin_nanf("");
        tp_out[o] = (int)ntp;
        fp_out[o] = (int)((e - s) - ntp);
    }
}

extern "C" size_t y3_eval_ap_workspace_bytes(long long m, int num_thr) {
    if (m < 0 || num_thr < 1) return 0;
    return (size_t)m * (size_t)num_thr * sizeof(float);
}

extern "C" int y3_eval_ap(const long long* keys, const unsigned* tp, long long m, int num_classes, int num_thr, const int* npos,
                          void* workspace, size_t workspace_bytes, float* ap, float* recall, int* tp_count, int* fp_count,
                          y3_stream_t stream) {
    Y3_CHECK_ARG(npos && ap && recall && tp_count && fp_count, "eval_ap: null pointer");
    Y3_CHECK_ARG(m >= 0 && m < 0x7fffffffLL && num_classes >= 1, "eval_ap: bad sizes (m %lld, classes %d)", m, num_classes);
    Y3_CHECK_ARG(m == 0 || (keys && tp && workspace), "eval_ap: null pool or workspace");
    Y3_CHECK_ARG(num_thr >= 1 && num_thr <= Y3_EVAL_MAX_THR, "eval_ap: %d IoU thresholds (1..%d)", num_thr, Y3_EVAL_MAX_THR);
    Y3_CHECK_ARG(workspace_bytes >= y3_eval_ap_workspace_bytes(m, num_thr), "eval_ap: workspace too small");
    Y3_CHECK_ARG((long long)num_classes * num_thr <= 0x7fffffffLL, "eval_ap: classes * thresholds overflows");
    hipLaunchKernelGGL(eval_ap_kernel, dim3(num_classes * num_thr), dim3(256), 0, (hipStream_t)stream, keys, tp, m, num_thr, npos,
                       (float*)workspace, ap, recall, tp_count, fp_count);
    Y3_CHECK_LAUNCH("eval_ap");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// matching by area range: one workgroup per (image, class), the waves walk the (range, threshold) pairs
// ---------------------------------------------------------------------------
#define Y3_EVAL_MAX_RANGES 8  // area ranges: pool_tp / pool_ign hold one mask word per entry and range

struct EvalMatchRangesArgs {
    EvalMatchArgs m;
    float lo[Y3_EVAL_MAX_RANGES], hi[Y3_EVAL_MAX_RANGES];
    int A;
    unsigned* pool_ign;
};

__global__ __launch_bounds__(1024) void eval_match_ranges_kernel(const EvalMatchRangesArgs q) {
    extern __shared__ __attribute__((aligned(16))) float sg[];  // SoA [5][cap], as eval_match_kernel
    __shared__ int s_ng;
    const EvalMatchArgs& p = q.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int seg = blockIdx.x;
    const int img = seg / p.K, cls = seg - img * p.K;
    const int A = q.A;
    float* gx0 = sg;
    float* gy0 = gx0 + p.cap;
    float* gx1 = gy0 + p.cap;
    float* gy1 = gx1 + p.cap;
    float* gar = gy1 + p.cap;

    const int cnt = eval_kept(p.keep_cnt, seg, p.max_keep, p.max_det);
    const long long out0 = p.offsets[seg];
    // 1. pool entries of this (image, class): the sort key and cleared TP / ignore masks, one word per range
    for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
        const long long o = out0 + j;
        if (o < p.pool_capacity) {
            const float sc = p.keep_score[(long long)seg * p.max_keep + j];
            p.pool_key[o] = ((long long)cls << 32) | (long long)(unsigned)~eval_mono(sc);
            for (int a = 0; a < A; ++a) {
                p.pool_tp[o * A + a] = 0u;
                q.pool_ign[o * A + a] = 0u;
            }
        }
    }
    // 2. wave 0 compacts the image's GT boxes of this class into LDS, in GT order
    if (wave == 0) {
        int ng = p.gt_cnt[img];
        ng = ng < p.max_gt ? ng : p.max_gt;
        const float* g = p.gt + (long long)img * p.max_gt * 5;
        int base = 0;
        for (int g0 = 0; g0 < ng; g0 += 64) {
            const int i = g0 + lane;
            float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
            bool mine = false;
            if (i < ng) {
                const float* b = g + (long long)i * 5;
                x0 = b[0];
                y0 = b[1];
                x1 = b[2];
                y1 = b[3];
                mine = b[4] == (float)cls;
            }
            const unsigned long long bal = __ballot(mine);
            const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
            if (mine && pos < p.cap) {
                gx0[pos] = x0;
                gy0[pos] = y0;
                gx1[pos] = x1;
                gy1[pos] = y1;
                gar[pos] = (x1 - x0) * (y1 - y0);
            }
            base += __popcll(bal);
        }
        if (lane == 0) s_ng = base < p.cap ? base : p.cap;
    }
    __syncthreads();
    const int G = s_ng;
    if (cnt == 0) return;
    const float* rows = p.rows + (long long)img * p.nb * p.ld;
    const int* kidx = p.keep_idx + (long long)seg * p.max_keep;

    // 3. greedy matching in keep order, one wave per (range, threshold) pair at a time; no barriers from here on
    const int P = A * p.T;
    for (int pr = wave; pr < P; pr += nwaves) {
        const int a = pr / p.T, t = pr - a * p.T;
        const float thr = p.thr[t], lo = q.lo[a], hi = q.hi[a];
        unsigned long long matched = 0ull;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + lane;
            float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
            bool ok = false;
            if (j < cnt) {
                const int r = kidx[j];
                if (r >= 0 && r < p.nb) {
                    const float* b = rows + (long long)r * p.ld;
                    x0 = b[0];
                    y0 = b[1];
                    x1 = b[2];
                    y1 = b[3];
                    if (p.clip_w > 0.f) {
                        x0 = fminf(fmaxf(x0, 0.f), p.clip_w);
                        x1 = fminf(fmaxf(x1, 0.f), p.clip_w);
                        y0 = fminf(fmaxf(y0, 0.f), p.clip_h);
                        y1 = fminf(fmaxf(y1, 0.f), p.clip_h);
                    }
                    ok = true;
                }
            }
            const float ar = (x1 - x0) * (y1 - y0);
            const unsigned long long okmask = __ballot(ok);
            const int nj = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int k = 0; k < nj; ++k) {
                if (!((okmask >> k) & 1ull)) continue;
                const float kx0 = __shfl(x0, k), ky0 = __shfl(y0, k), kx1 = __shfl(x1, k), ky1 = __shfl(y1, k), kar = __shfl(ar, k);
                // key = (in range << 63) | (IoU bits << 32) | (g + 1): an IoU in (0, 1] never sets bit 31 of its float bits, so
                // one max yields the in-range best if there is one, else the out-of-range best; ties take the highest g
                unsigned long long best = 0ull;
                int bit = 0;
                for (int g = lane; g < G; g += 64, ++bit) {
                    if ((matched >> bit) & 1ull) continue;
                    const float xl = fmaxf(kx0, gx0[g]), yt = fmaxf(ky0, gy0[g]);
                    const float xr = fminf(kx1, gx1[g]), yb = fminf(ky1, gy1[g]);
                    const float inter = fmaxf(yb - yt, 0.f) * fmaxf(xr - xl, 0.f);
                    const float ga = gar[g];
                    const float iou = inter / ((kar + ga) - inter);
                    if (iou >= thr) {
                        const unsigned long long in = (lo <= ga && ga <= hi) ? 1ull << 63 : 0ull;
                        const unsigned long long key = in | ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)(g + 1);
                        best = key > best ? key : best;
                    }
                }
                const long long o = out0 + j0 + k;
                if (!__ballot(best != 0ull)) {  // no candidate anywhere: ignored if the detection's own area is out of range, else an FP
                    if (lane == 0 && !(lo <= kar && kar <= hi) && o < p.pool_capacity) atomicOr(&q.pool_ign[o * A + a], 1u << t);
                    continue;
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    const unsigned long long other = __shfl_xor(best, s);
                    best = other > best ? other : best;
                }
                const int g = (int)(unsigned)(best & 0xffffffffull) - 1;
                if (lane == (g & 63)) matched |= 1ull << (g >> 6);  // consumed in both tiers
                if (lane == 0 && o < p.pool_capacity) atomicOr((best >> 63) ? &p.pool_tp[o * A + a] : &q.pool_ign[o * A + a], 1u << t);
            }
        }
    }
}

extern "C" int y3_eval_match_ranges(const float* rows, int n, int nb, int ld, int num_classes, float clip_w, float clip_h, const int* keep_idx,
                                    const int* keep_cnt, const float* keep_score, int max_keep, int max_det, const float* gt,
                                    const int* gt_cnt, int max_gt, int max_gt_per_class, const float* iou_thr_host, int num_thr,
                                    const float* area_lo_host, const float* area_hi_host, int num_ranges, const int* offsets,
                                    long long* pool_key, unsigned* pool_tp, unsigned* pool_ign, long long pool_capacity, y3_stream_t stream) {
    Y3_CHECK_ARG(rows && keep_idx && keep_cnt && keep_score && gt && gt_cnt && iou_thr_host && area_lo_host && area_hi_host && offsets &&
                     pool_key && pool_tp && pool_ign,
                 "eval_match_ranges: null pointer");
    Y3_CHECK_ARG(n >= 1 && nb >= 1 && ld >= 4 && num_classes >= 1 && max_keep >= 1 && max_det >= 1 && max_gt >= 1 && pool_capacity >= 0,
                 "eval_match_ranges: bad sizes (n %d, nb %d, ld %d, classes %d, max_keep %d, max_det %d, max_gt %d)", n, nb, ld,
                 num_classes, max_keep, max_det, max_gt);
    Y3_CHECK_ARG(num_thr >= 1 && num_thr <= Y3_EVAL_MAX_THR, "eval_match_ranges: %d IoU thresholds (1..%d)", num_thr, Y3_EVAL_MAX_THR);
    Y3_CHECK_ARG(num_ranges >= 1 && num_ranges <= Y3_EVAL_MAX_RANGES, "eval_match_ranges: %d area ranges (1..%d)", num_ranges,
                 Y3_EVAL_MAX_RANGES);
    Y3_CHECK_ARG(max_gt_per_class >= 0 && max_gt_per_class <= Y3_EVAL_MAX_GT,
                 "eval_match_ranges: %d ground-truth boxes in one (image, class); at most %d fit the LDS stage", max_gt_per_class,
                 Y3_EVAL_MAX_GT);
    Y3_CHECK_ARG((long long)n * num_classes <= 0x7fffffffLL, "eval_match_ranges: n * classes overflows");
    EvalMatchRangesArgs q = {};
    EvalMatchArgs& p = q.m;
    for (int t = 0; t < num_thr; ++t) {
        const float v = iou_thr_host[t];
        Y3_CHECK_ARG(v > 0.f && v <= 1.f, "eval_match_ranges: IoU threshold %d = %g outside (0, 1]", t, (double)v);
        p.thr[t] = v;
    }
    for (int a = 0; a < num_ranges; ++a) {
        const float lo = area_lo_host[a], hi = area_hi_host[a];
        Y3_CHECK_ARG(lo < hi, "eval_match_ranges: area range %d = [%g, %g] needs lo < hi (no NaN)", a, (double)lo, (double)hi);
        q.lo[a] = lo;
        q.hi[a] = hi;
    }
    q.A = num_ranges;
    q.pool_ign = pool_ign;
    p.rows = rows;
    p.nb = nb;
    p.ld = ld;
    p.K = num_classes;
    p.clip_w = clip_w;
    p.clip_h = clip_h;
    p.keep_idx = keep_idx;
    p.keep_cnt = keep_cnt;
    p.keep_score = keep_score;
    p.max_keep = max_keep;
    p.max_det = max_det;
    p.gt = gt;
    p.gt_cnt = gt_cnt;
    p.max_gt = max_gt;
    p.cap = max_gt_per_class < 64 ? 64 : (max_gt_per_class + 63) & ~63;
    p.T = num_thr;
    p.offsets = offsets;
    p.pool_key = pool_key;
    p.pool_tp = pool_tp;
    p.pool_capacity = pool_capacity;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)eval_match_ranges_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Y3_EVAL_MAX_GT * 20) !=
            hipSuccess) {
            y3_set_error("eval_match_ranges: cannot raise the dynamic LDS limit");
            return Y3_ELAUNCH;
        }
        attr_set = true;
    }
    const int pairs = num_ranges * num_thr;
    const int waves = pairs < 16 ? pairs : 16;
    hipLaunchKernelGGL(eval_match_ranges_kernel, dim3(n * num_classes), dim3(64 * waves), (size_t)p.cap * 20, (hipStream_t)stream, q);
    Y3_CHECK_LAUNCH("eval_match_ranges");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// AP by area range, best-F1 cut and PR curve: one 256-thread workgroup per (class, range, threshold)
// ---------------------------------------------------------------------------
// inverse of the pool key's score part (eval_mono)
__device__ __forceinline__ float eval_key_score(long long key) {
    const unsigned mono = ~(unsigned)(key & 0xffffffffLL);
    return __uint_as_float((mono & 0x80000000u) ? (mono & 0x7fffffffu) : ~mono);
}

struct EvalCut {  // a candidate score cut: the first k non-ignored entries, tp of them TPs, key of the k-th
    double f1;
    int k, tp;
    long long key;
};

__device__ __forceinline__ void eval_cut_max(EvalCut& b, double f1, int k, int tp, long long key) {
    if (f1 > b.f1 || (f1 == b.f1 && k < b.k)) {
        b.f1 = f1;
        b.k = k;
        b.tp = tp;
        b.key = key;
    }
}

__global__ __launch_bounds__(256) void eval_ap_ranges_kernel(const long long* __restrict__ keys, const unsigned* __restrict__ tp,
                                                             const unsigned* __restrict__ ign, long long m, int A, int T,
                                                             const int* __restrict__ npos_dev, float* __restrict__ ws,
                                                             float* __restrict__ ap, float* __restrict__ recall, int* __restrict__ tp_out,
                                                             int* __restrict__ fp_out, int* __restrict__ ign_out, int* __restrict__ best_n,
                                                             int* __restrict__ best_tp, float* __restrict__ best_score,
                                                             float* __restrict__ pr_prec, float* __restrict__ pr_score) {
    __shared__ long long s_range[2];
    __shared__ int wtp[4], wva[4];
    __shared__ long long wlast[4];
    __shared__ float wmax[4];
    __shared__ double terms[101];
    __shared__ float s_first;
    __shared__ EvalCut wcut[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int o = blockIdx.x;  // (cls * A + a) * T + t
    const int t = o % T, a = (o / T) % A, cls = o / (T * A);
    if (threadIdx.x < 2) s_range[threadIdx.x] = eval_lower_bound(keys, m, (long long)(cls + threadIdx.x) << 32);
    __syncthreads();
    const long long s = s_range[0], e = s_range[1];
    const int npos = npos_dev[cls * A + a];
    float* prec = ws + (long long)(a * T + t) * 2 * m + s;  // precision at the q-th TP, then its suffix max (the envelope)
    float* scr = prec + m;                                  // score of the q-th TP

    // 1. tp_cum and the non-ignored rank by a chunked block scan; precision = tp_cum / rank at every TP.  A cut between two
    //    non-ignored neighbours of different score is a candidate operating point; every thread keeps its best F1.
    const float nanv = __builtin_nanf("");
    EvalCut cut = {-1.0, 0x7fffffff, 0, 0ll};
    long long ntp = 0, nva = 0, carry = -1;  // carry: key of the last non-ignored entry so far (keys are >= 0)
    for (long long b0 = s; b0 < e; b0 += 256) {
        const long long i = b0 + threadIdx.x;
        const bool in = i < e;
        const bool val = in && !((ign[i * A + a] >> t) & 1u);
        const bool hit = val && ((tp[i * A + a] >> t) & 1u);
        const long long key = in ? keys[i] : 0ll;
        const unsigned long long balh = __ballot(hit), balv = __ballot(val);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int hl = balv ? 63 - __clzll((long long)balv) : 0;         // the wave's last non-ignored lane
        const int pl = (balv & below) ? 63 - __clzll((long long)(balv & below)) : 0;  // the nearest one below this lane
        const long long lastk = __shfl(key, hl);
        long long pk = __shfl(key, pl);
        if (lane == 0) {
            wtp[wave] = __popcll(balh);
            wva[wave] = __popcll(balv);
            wlast[wave] = balv ? lastk : -1;
        }
        __syncthreads();
        long long qx = ntp + __popcll(balh & below);  // TPs / non-ignored entries before this one
        long long rx = nva + __popcll(balv & below);
        long long before = carry;
        for (int w = 0; w < wave; ++w) {
            qx += wtp[w];
            rx += wva[w];
            if (wlast[w] >= 0) before = wlast[w];
        }
        if (!(balv & below)) pk = before;
        if (hit) {
            prec[qx] = (float)(qx + 1) / (float)(rx + 1);
            scr[qx] = eval_key_score(key);
        }
        if (val) {
            if (rx == 0) s_first = eval_key_score(key);
            else if (pk != key && npos > 0) eval_cut_max(cut, 2.0 * (double)qx / (double)(rx + npos), (int)rx, (int)qx, pk);
        }
        for (int w = 0; w < 4; ++w) {
            ntp += wtp[w];
            nva += wva[w];
            if (wlast[w] >= 0) carry = wlast[w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && nva > 0 && npos > 0)  // the cut after the last entry
        eval_cut_max(cut, 2.0 * (double)ntp / (double)(nva + npos), (int)nva, (int)ntp, carry);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) eval_cut_max(cut, __shfl_xor(cut.f1, d), __shfl_xor(cut.k, d), __shfl_xor(cut.tp, d), __shfl_xor(cut.key, d));
    if (lane == 0) wcut[wave] = cut;
    // 2. envelope: reverse max-scan over the TP precisions, chunks from the end
    float carry_max = 0.f;
    for (long long end = ntp; end > 0; end -= 256) {
        const long long st = end - 256 > 0 ? end - 256 : 0;
        const long long i = st + threadIdx.x;
        float v = i < end ? prec[i] : 0.f;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float u = __shfl_down(v, d);
            if (lane + d < 64) v = fmaxf(v, u);
        }
        if (lane == 0) wmax[wave] = v;
        __syncthreads();
        for (int w = wave + 1; w < 4; ++w) v = fmaxf(v, wmax[w]);
        v = fmaxf(v, carry_max);
        if (i < end) prec[i] = v;
        carry_max = fmaxf(carry_max, fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
        __syncthreads();
    }
    // 3. 101 points: recall j/100 is first reached at the ceil(j npos / 100)-th TP (the first entry when that is 0)
    if (threadIdx.x <= 100) {
        const long long need = ((long long)threadIdx.x * npos + 99) / 100;
        float v = 0.f, sc = nanv;
        if (nva > 0) {
            if (need == 0) {
                v = ntp > 0 ? prec[0] : 0.f;
                sc = s_first;
            } else if (need <= ntp) {
                v = prec[need - 1];
                sc = scr[need - 1];
            }
        }
        terms[threadIdx.x] = (double)v;
        if (pr_prec) pr_prec[(long long)o * 101 + threadIdx.x] = npos > 0 ? v : nanv;
        if (pr_score) pr_score[(long long)o * 101 + threadIdx.x] = npos > 0 ? sc : nanv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int j = 0; j <= 100; ++j) sum += terms[j];
        ap[o] = npos > 0 ? (float)(sum / 101.0) : nanv;
        recall[o] = npos > 0 ? (float)ntp / (float)npos : nanv;
        tp_out[o] = (int)ntp;
        fp_out[o] = (int)(nva - ntp);
        ign_out[o] = (int)((e - s) - nva);
        for (int w = 1; w < 4; ++w) eval_cut_max(cut, wcut[w].f1, wcut[w].k, wcut[w].tp, wcut[w].key);
        const bool any = cut.f1 >= 0.0;
        best_n[o] = any ? cut.k : 0;
        best_tp[o] = any ? cut.tp : 0;
        best_score[o] = any ? eval_key_score(cut.key) : nanv;
    }
}

extern "C" size_t y3_eval_ap_ranges_workspace_bytes(long long m, int num_ranges, int num_thr) {
    if (m < 0 || num_ranges < 1 || num_thr < 1) return 0;
    return (size_t)m * (size_t)num_ranges * (size_t)num_thr * 2 * sizeof(float);
}

extern "C" int y3_eval_ap_ranges(const long long* keys, const unsigned* tp, const unsigned* ign, long long m, int num_classes, int num_ranges,
                                 int num_thr, const int* npos, void* workspace, size_t workspace_bytes, float* ap, float* recall,
                                 int* tp_count, int* fp_count, int* ign_count, int* best_n, int* best_tp, float* best_score,
                                 float* pr_precision, float* pr_score, y3_stream_t stream) {
    Y3_CHECK_ARG(npos && ap && recall && tp_count && fp_count && ign_count && best_n && best_tp && best_score, "eval_ap_ranges: null pointer");
    Y3_CHECK_ARG(m >= 0 && m < 0x7fffffffLL && num_classes >= 1, "eval_ap_ranges: bad sizes (m %lld, classes %d)", m, num_classes);
    Y3_CHECK_ARG(m == 0 || (keys && tp && ign && workspace), "eval_ap_ranges: null pool or workspace");
    Y3_CHECK_ARG(num_thr >= 1 && num_thr <= Y3_EVAL_MAX_THR, "eval_ap_ranges: %d IoU thresholds (1..%d)", num_thr, Y3_EVAL_MAX_THR);
    Y3_CHECK_ARG(num_ranges >= 1 && num_ranges <= Y3_EVAL_MAX_RANGES, "eval_ap_ranges: %d area ranges (1..%d)", num_ranges,
                 Y3_EVAL_MAX_RANGES);
    Y3_CHECK_ARG(workspace_bytes >= y3_eval_ap_ranges_workspace_bytes(m, num_ranges, num_thr), "eval_ap_ranges: workspace too small");
    Y3_CHECK_ARG((long long)num_classes * num_ranges * num_thr <= 0x7fffffffLL / 101, "eval_ap_ranges: classes * ranges * thresholds overflows");
    hipLaunchKernelGGL(eval_ap_ranges_kernel, dim3(num_classes * num_ranges * num_thr), dim3(256), 0, (hipStream_t)stream, keys, tp, ign, m,
                       num_ranges, num_thr, npos, (float*)workspace, ap, recall, tp_count, fp_count, ign_count, best_n, best_tp, best_score,
                       pr_precision, pr_score);
    Y3_CHECK_LAUNCH("eval_ap_ranges");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// per-class score cut on keep lists: one wave per (image, class) segment
// ---------------------------------------------------------------------------
// The lists are in keep order with non-increasing scores, but the kernel takes the longest passing PREFIX and relies on nothing
// more: per 64-entry chunk a ballot of "inside the list and score >= threshold" and the count of its trailing ones.
__global__ __launch_bounds__(256) void keep_cut_kernel(const float* __restrict__ keep_score, int* __restrict__ keep_cnt, int nseg, int K,
                                                       int max_keep, const float* __restrict__ class_thr) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (s >= nseg) return;  // wave-uniform
    int m = keep_cnt[s];
    m = m < max_keep ? m : max_keep;
    m = m > 0 ? m : 0;
    const float thr = class_thr[s % K];
    const float* sc = keep_score + (long long)s * max_keep;
    int kept = 0;
    for (int j0 = 0; j0 < m; j0 += 64) {
        const int j = j0 + lane;
        const bool pass = j < m && sc[j] >= thr;
        const unsigned long long fail = ~__ballot(pass);
        const int run = fail ? __builtin_ctzll(fail) : 64;
        kept += run;
        if (run < 64) break;
    }
    if (lane == 0) keep_cnt[s] = kept;
}

extern "C" int y3_keep_cut(const float* keep_score, int* keep_cnt, int nseg, int num_classes, int max_keep, const float* class_thr,
                           y3_stream_t stream) {
    Y3_CHECK_ARG(keep_score && keep_cnt && class_thr, "keep_cut: null pointer");
    Y3_CHECK_ARG(nseg >= 1 && num_classes >= 1 && max_keep >= 1, "keep_cut: bad sizes (nseg %d, classes %d, max_keep %d)", nseg, num_classes,
                 max_keep);
    Y3_CHECK_ARG(nseg % num_classes == 0, "keep_cut: %d segments are not whole images of %d classes", nseg, num_classes);
    hipLaunchKernelGGL(keep_cut_kernel, dim3((nseg + 3) / 4), dim3(256), 0, (hipStream_t)stream, keep_score, keep_cnt, nseg, num_classes,
                       max_keep, class_thr);
    Y3_CHECK_LAUNCH("keep_cut");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// confusion matrix: class-agnostic matching, one workgroup per image, one wave per IoU threshold
// ---------------------------------------------------------------------------
struct EvalConfusionArgs {
    EvalMatchArgs m;              // pool_key / pool_tp unused; cap: LDS slots per field for the image's GT boxes of ALL classes
    int* order;                   // [total]: at offsets[img * K] + pooled rank, the entry's class * max_keep + keep rank
    long long total;
    unsigned long long* counts;   // [T][K + 1][K + 1], rows true, columns predicted, index K = background; added to
};

// entries of the non-increasing list a[0..m) that precede score s: those > s, with `ties` also those == s
__device__ __forceinline__ int eval_count_before(const float* a, int m, float s, bool ties) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float v = a[mid];
        if (ties ? v >= s : v > s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The pooled order of an image's entries: score descending, ties: lower class first, then keep rank.  An entry's rank is its keep
// rank plus, per other class, the entries of that class's list that precede it (>= for lower classes, > for higher ones).
__global__ __launch_bounds__(256) void eval_pool_rank_kernel(const EvalConfusionArgs q) {
    const EvalMatchArgs& p = q.m;
    const int img = blockIdx.x, K = p.K;
    const int* off = p.offsets + (long long)img * K;
    const int first = off[0], count = off[K] - first;
    for (int e = threadIdx.x; e < count; e += blockDim.x) {
        // the segment of entry e: the last class c with off[c] <= first + e (empty segments share their successor's offset)
        int lo = 0, hi = K;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= first + e) lo = mid;
            else hi = mid;
        }
        const int c = lo, j = first + e - off[c];
        const float s = p.keep_score[((long long)img * K + c) * p.max_keep + j];
        int rank = j;
        for (int o = 0; o < K; ++o) {
            if (o == c) continue;
            const int m = off[o + 1] - off[o];
            if (m > 0) rank += eval_count_before(p.keep_score + ((long long)img * K + o) * p.max_keep, m, s, o < c);
        }
        const long long at = (long long)first + rank;
        if (rank < count && at < q.total) q.order[at] = c * p.max_keep + j;
    }
}

__global__ __launch_bounds__(1024) void eval_confusion_kernel(const EvalConfusionArgs q) {
    extern __shared__ __attribute__((aligned(16))) float sg[];  // SoA [6][cap]: x0, y0, x1, y1, area, class of the image's GT boxes
    const EvalMatchArgs& p = q.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int img = blockIdx.x, K = p.K, K1 = p.K + 1;
    float* gx0 = sg;
    float* gy0 = gx0 + p.cap;
    float* gx1 = gy0 + p.cap;
    float* gy1 = gx1 + p.cap;
    float* gar = gy1 + p.cap;
    int* gcl = (int*)(gar + p.cap);

    // 1. the image's GT boxes of every class into LDS, in GT order
    int G = p.gt_cnt[img];
    G = G < p.max_gt ? G : p.max_gt;
    G = G < p.cap ? G : p.cap;
    G = G > 0 ? G : 0;
    const float* gt = p.gt + (long long)img * p.max_gt * 5;
    for (int i = threadIdx.x; i < G; i += blockDim.x) {
        const float* b = gt + (long long)i * 5;
        const float x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
        const int c = (int)b[4];
        gx0[i] = x0;
        gy0[i] = y0;
        gx1[i] = x1;
        gy1[i] = y1;
        gar[i] = (x1 - x0) * (y1 - y0);
        gcl[i] = c < 0 ? 0 : (c < K ? c : K - 1);
    }
    __syncthreads();
    const int first = p.offsets[(long long)img * K];
    const int cnt = p.offsets[(long long)img * K + K] - first;
    const float* rows = p.rows + (long long)img * p.nb * p.ld;

    // 2. greedy matching in pooled order, one wave per threshold; no barriers from here on.  Lane l owns GT boxes l, l + 64, ...;
    //    their matched flags are the bits of one 64-bit register (G <= 4096 = 64 x 64).
    for (int t = wave; t < p.T; t += nwaves) {
        const float thr = p.thr[t];
        unsigned long long* M = q.counts + (long long)t * K1 * K1;
        unsigned long long matched = 0ull;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            // lane l stages pooled entry j0 + l (clipped like eval_match_kernel)
            const int j = j0 + lane;
            float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
            int cls = -1;  // < 0: an entry the rank kernel did not place (scores out of order); skipped
            bool ok = false;
            if (j < cnt && (long long)first + j < q.total) {
                const int v = q.order[first + j];
                const int c = v / p.max_keep, slot = v - c * p.max_keep;
                if (v >= 0 && c < K && slot < eval_kept(p.keep_cnt, img * K + c, p.max_keep, p.max_det)) {
                    cls = c;
                    const int r = p.keep_idx[((long long)img * K + c) * p.max_keep + slot];
                    if (r >= 0 && r < p.nb) {
                        const float* b = rows + (long long)r * p.ld;
                        x0 = b[0];
                        y0 = b[1];
                        x1 = b[2];
                        y1 = b[3];
                        if (p.clip_w > 0.f) {
                            x0 = fminf(fmaxf(x0, 0.f), p.clip_w);
                            x1 = fminf(fmaxf(x1, 0.f), p.clip_w);
                            y0 = fminf(fmaxf(y0, 0.f), p.clip_h);
                            y1 = fminf(fmaxf(y1, 0.f), p.clip_h);
                        }
                        ok = true;
                    }
                }
            }
            const float ar = (x1 - x0) * (y1 - y0);
            const unsigned long long okmask = __ballot(ok);
            const int nj = cnt - j0 < 64 ? cnt - j0 : 64;
            for (int k = 0; k < nj; ++k) {
                const int pc = __shfl(cls, k);
                if (pc < 0) continue;
                unsigned long long best = 0ull;
                if ((okmask >> k) & 1ull) {  // a keep row outside the rows is background, as eval_match_kernel never makes it a TP
                    const float kx0 = __shfl(x0, k), ky0 = __shfl(y0, k), kx1 = __shfl(x1, k), ky1 = __shfl(y1, k), kar = __shfl(ar, k);
                    // key = (IoU bits << 32) | (g + 1): IoU >= thr > 0 makes the bits monotone; the max takes the highest g on ties
                    int bit = 0;
                    for (int g = lane; g < G; g += 64, ++bit) {
                        if ((matched >> bit) & 1ull) continue;
                        const float xl = fmaxf(kx0, gx0[g]), yt = fmaxf(ky0, gy0[g]);
                        const float xr = fminf(kx1, gx1[g]), yb = fminf(ky1, gy1[g]);
                        const float inter = fmaxf(yb - yt, 0.f) * fmaxf(xr - xl, 0.f);
                        const float iou = inter / ((kar + gar[g]) - inter);
                        if (iou >= thr) {
                            const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)(g + 1);
                            best = key > best ? key : best;
                        }
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned long long other = __shfl_xor(best, o);
                        best = other > best ? other : best;
                    }
                }
                int row = K;  // background: a false positive
                if (best) {
                    const int g = (int)(unsigned)(best & 0xffffffffull) - 1;
                    if (lane == (g & 63)) matched |= 1ull << (g >> 6);
                    row = gcl[g];
                }
                if (lane == 0) atomicAdd(&M[(long long)row * K1 + pc], 1ull);
            }
        }
        // 3. the GT boxes nobody took: missed
        int bit = 0;
        for (int g = lane; g < G; g += 64, ++bit)
            if (!((matched >> bit) & 1ull)) atomicAdd(&M[(long long)gcl[g] * K1 + K], 1ull);
    }
}

extern "C" size_t y3_eval_confusion_workspace_bytes(long long total) { return total > 0 ? (size_t)total * sizeof(int) : 0; }

extern "C" int y3_eval_confusion(const float* rows, int n, int nb, int ld, int num_classes, float clip_w, float clip_h, const int* keep_idx,
                                 const int* keep_cnt, const float* keep_score, int max_keep, int max_det, const float* gt,
                                 const int* gt_cnt, int max_gt, int max_gt_per_image, const float* iou_thr_host, int num_thr,
                                 const int* offsets, long long total, void* workspace, size_t workspace_bytes, long long* confusion,
                                 y3_stream_t stream) {
    Y3_CHECK_ARG(rows && keep_idx && keep_cnt && keep_score && gt && gt_cnt && iou_thr_host && offsets && confusion,
                 "eval_confusion: null pointer");
    Y3_CHECK_ARG(n >= 1 && nb >= 1 && ld >= 4 && num_classes >= 1 && max_keep >= 1 && max_det >= 1 && max_gt >= 1 && total >= 0,
                 "eval_confusion: bad sizes (n %d, nb %d, ld %d, classes %d, max_keep %d, max_det %d, max_gt %d, total %lld)", n, nb, ld,
                 num_classes, max_keep, max_det, max_gt, total);
    Y3_CHECK_ARG(num_thr >= 1 && num_thr <= Y3_EVAL_MAX_THR, "eval_confusion: %d IoU thresholds (1..%d)", num_thr, Y3_EVAL_MAX_THR);
    Y3_CHECK_ARG(max_gt_per_image >= 0 && max_gt_per_image <= Y3_EVAL_MAX_GT,
                 "eval_confusion: %d ground-truth boxes in one image; at most %d fit the LDS stage", max_gt_per_image, Y3_EVAL_MAX_GT);
    Y3_CHECK_ARG((long long)n * num_classes <= 0x7fffffffLL && (long long)num_classes * max_keep <= 0x7fffffffLL && total <= 0x7fffffffLL,
                 "eval_confusion: n * classes, classes * max_keep or total overflows");
    Y3_CHECK_ARG(total == 0 || (workspace && workspace_bytes >= y3_eval_confusion_workspace_bytes(total)),
                 "eval_confusion: workspace missing or too small");
    EvalConfusionArgs q = {};
    EvalMatchArgs& p = q.m;
    for (int t = 0; t < num_thr; ++t) {
        const float v = iou_thr_host[t];
        Y3_CHECK_ARG(v > 0.f && v <= 1.f, "eval_confusion: IoU threshold %d = %g outside (0, 1]", t, (double)v);
        p.thr[t] = v;
    }
    p.rows = rows;
    p.nb = nb;
    p.ld = ld;
    p.K = num_classes;
    p.clip_w = clip_w;
    p.clip_h = clip_h;
    p.keep_idx = keep_idx;
    p.keep_cnt = keep_cnt;
    p.keep_score = keep_score;
    p.max_keep = max_keep;
    p.max_det = max_det;
    p.gt = gt;
    p.gt_cnt = gt_cnt;
    p.max_gt = max_gt;
    p.cap = max_gt_per_image < 64 ? 64 : (max_gt_per_image + 63) & ~63;
    p.T = num_thr;
    p.offsets = offsets;
    q.order = (int*)workspace;
    q.total = total;
    q.counts = (unsigned long long*)confusion;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)eval_confusion_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Y3_EVAL_MAX_GT * 24) !=
            hipSuccess) {
            y3_set_error("eval_confusion: cannot raise the dynamic LDS limit");
            return Y3_ELAUNCH;
        }
        attr_set = true;
    }
    if (total > 0) {
        hipLaunchKernelGGL(eval_pool_rank_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, q);
        Y3_CHECK_LAUNCH("eval_confusion (pooled order)");
    }
    const int waves = num_thr < 16 ? num_thr : 16;
    hipLaunchKernelGGL(eval_confusion_kernel, dim3(n), dim3(64 * waves), (size_t)p.cap * 24, (hipStream_t)stream, q);
    Y3_CHECK_LAUNCH("eval_confusion");
    return Y3_OK;
}
