// Anchor fitting on the device: y3_anchor_stats scores P candidate anchor sets of k anchors each against n box
// sizes in one launch -- the Lloyd step (per-anchor sums), the mutation search (totals) and the report of yolo3/anchors.py.
// Compiled with -ffp-contract=off: the IoU below is the fp32 expression of format_labels_kernel (detect.hip), one rounding per
// step and in its order, so the anchor a box scores best against here is the slot the label builder gives it later.
//
// Everything that is accumulated is an integer (the score is q = rint(iou * 2^24)), so the sums do not depend on the order they
// are taken in: workgroups add into LDS with integer atomics, write one partial row each into the workspace, and a second
// kernel adds the rows.  No float atomics, no global atomics, nothing to zero beforehand.
//
// Shape of the main kernel: a thread keeps two neighbouring boxes in registers (one 16-byte load: the pair grid is shifted by one
// box when wh_dev is only 8-byte aligned, and the boxes at the two ragged ends come in as 8-byte loads) and walks the P * k
// candidates, which sit in LDS as (w / 2, h / 2, w * h) and are read as broadcasts.  The grid is capped; a workgroup strides.
#include "common.h"

#define Y3_ANCHOR_THREADS 256
static_assert(Y3_ANCHOR_THREADS * 2 == Y3_ANCHOR_BLOCK_BOXES, "two boxes per thread");
#define Y3_ANCHOR_ACC 4   // LDS words (64-bit) per (set, anchor) in per-anchor mode: count | count_thr << 32, sum w, sum h, sum q

struct AnchorArgs {
    const int* wh;  // [n][2]
    const float* cand;  // [P][k][2]
    long long n;
    long long nv;   // box pairs of the shifted pair grid
    int head;       // 1: wh is 8 mod 16, pair v holds boxes 2v - 1 and 2v
    int P, k, thr_q, per_anchor;
    int words;      // 64-bit words of the output, the skipped-box counter included
    unsigned char* labels;
    long long* partial;  // [gridDim.x][words]
};

struct AnchorBox {
    float w2, h2, area;  // w / 2, h / 2, w * h
    int w, h;
    bool ok;  // inside n and not skipped
};

__device__ __forceinline__ AnchorBox anchor_box(int w, int h, bool inside) {
    AnchorBox b;
    b.w = w;
    b.h = h;
    b.ok = inside && w >= 1 && w <= 65535 && h >= 1 && h <= 65535;
    const float fw = (float)w, fh = (float)h;
    b.w2 = fw / 2.0f;
    b.h2 = fh / 2.0f;
    b.area = fw * fh;
    return b;
}

// q of one box against one anchor c = (aw / 2, ah / 2, aw * ah): the iw / ih / inter / iou lines of format_labels_kernel
__device__ __forceinline__ float anchor_iou(const AnchorBox& b, const float4 c) {
    const float iw = fmaxf(fminf(b.w2, c.x) - fmaxf(-b.w2, -c.x), 0.0f);
    const float ih = fmaxf(fminf(b.h2, c.y) - fmaxf(-b.h2, -c.y), 0.0f);
    const float inter = iw * ih;
    return inter / (b.area + c.z - inter);
}

__device__ __forceinline__ int anchor_q(float iou) {
    const int q = (int)rintf(iou * 16777216.0f);
    return q < 0 ? 0 : (q > (1 << 24) ? (1 << 24) : q);     // (only a candidate that is not a positive finite size gets here out of range)
}

__device__ __forceinline__ unsigned anchor_wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

__global__ __launch_bounds__(Y3_ANCHOR_THREADS) void anchor_stats_kernel(const AnchorArgs p) {
    __shared__ float4 cand[Y3_ANCHOR_MAX_CANDIDATES];
    __shared__ unsigned long long acc[Y3_ANCHOR_MAX_CANDIDATES * Y3_ANCHOR_ACC];
    __shared__ unsigned long long skipped;
    const int tid = threadIdx.x;
    const int PK = p.P * p.k;
    const int nacc = p.per_anchor ? PK * Y3_ANCHOR_ACC : p.P * 2;
    for (int i = tid; i < PK; i += Y3_ANCHOR_THREADS) {
        const float aw = p.cand[2 * i], ah = p.cand[2 * i + 1];
        cand[i] = make_float4(aw / 2.0f, ah / 2.0f, aw * ah, 0.0f);
    }
    for (int i = tid; i < nacc; i += Y3_ANCHOR_THREADS) acc[i] = 0ull;
    if (tid == 0) skipped = 0ull;
    __syncthreads();

    unsigned long long my_skipped = 0ull;     // (whole wave's count, kept by every lane)
    const long long step = (long long)gridDim.x * Y3_ANCHOR_THREADS;
    for (long long base = (long long)blockIdx.x * Y3_ANCHOR_THREADS; base < p.nv; base += step) {      // uniform over the workgroup
        const long long v = base + tid;
        const long long u0 = 2 * v - p.head, u1 = u0 + 1;
        const bool in0 = v < p.nv && u0 >= 0, in1 = v < p.nv && u1 < p.n;
        int w0 = 0, h0 = 0, w1 = 0, h1 = 0;
        if (in0 && in1) {
            const int4 t = *reinterpret_cast<const int4*>(p.wh + 2 * u0);      // 16-byte aligned: u0 + head is even
            w0 = t.x;
            h0 = t.y;
            w1 = t.z;
            h1 = t.w;
        } else if (in0) {
            const int2 t = *reinterpret_cast<const int2*>(p.wh + 2 * u0);
            w0 = t.x;
            h0 = t.y;
        } else if (in1) {
            const int2 t = *reinterpret_cast<const int2*>(p.wh + 2 * u1);
            w1 = t.x;
            h1 = t.y;
        }
        const AnchorBox b0 = anchor_box(w0, h0, in0), b1 = anchor_box(w1, h1, in1);
        my_skipped += (unsigned long long)(__popcll(__ballot(in0 && !b0.ok)) + __popcll(__ballot(in1 && !b1.ok)));

        for (int s = 0; s < p.P; ++s) {
            const float4* cs = cand + s * p.k;
            int best0 = 0, best1 = 0;
            float iou0 = 0.f, iou1 = 0.f;
            for (int a = 0; a < p.k; ++a) {
                const float4 c = cs[a];
                const float i0 = anchor_iou(b0, c), i1 = anchor_iou(b1, c);
                if (a == 0 || i0 > iou0) {
                    best0 = a;
                    iou0 = i0;
                }
                if (a == 0 || i1 > iou1) {
                    best1 = a;
                    iou1 = i1;
                }
            }
            const int q0 = b0.ok ? anchor_q(iou0) : 0, q1 = b1.ok ? anchor_q(iou1) : 0;
            const bool t0 = b0.ok && q0 >= p.thr_q, t1 = b1.ok && q1 >= p.thr_q;
            if (p.per_anchor) {
                if (b0.ok) {
                    unsigned long long* r = acc + (s * p.k + best0) * Y3_ANCHOR_ACC;
                    atomicAdd(r + 0, 1ull | ((unsigned long long)t0 << 32));
                    atomicAdd(r + 1, (unsigned long long)b0.w);
                    atomicAdd(r + 2, (unsigned long long)b0.h);
                    atomicAdd(r + 3, (unsigned long long)q0);
                }
                if (b1.ok) {
                    unsigned long long* r = acc + (s * p.k + best1) * Y3_ANCHOR_ACC;
                    atomicAdd(r + 0, 1ull | ((unsigned long long)t1 << 32));
                    atomicAdd(r + 1, (unsigned long long)b1.w);
                    atomicAdd(r + 2, (unsigned long long)b1.h);
                    atomicAdd(r + 3, (unsigned long long)q1);
                }
            } else {
                // 128 boxes of a wave: sum q <= 2^31 fits 32 bits
                const unsigned sq = anchor_wave_sum_u32((unsigned)(q0 + q1));
                const int cnt = __popcll(__ballot(t0)) + __popcll(__ballot(t1));
                if ((tid & 63) == 0) {
                    atomicAdd(acc + 2 * s, (unsigned long long)sq);
                    atomicAdd(acc + 2 * s + 1, (unsigned long long)cnt);
                }
            }
            if (p.labels && s == 0) {     // (P == 1)
                if (in0) p.labels[u0] = b0.ok ? (unsigned char)best0 : (unsigned char)255;
                if (in1) p.labels[u1] = b1.ok ? (unsigned char)best1 : (unsigned char)255;
            }
        }
    }
    if ((tid & 63) == 0 && my_skipped) atomicAdd(&skipped, my_skipped);
    __syncthreads();

    long long* row = p.partial + (long long)blockIdx.x * p.words;
    if (p.per_anchor) {
        for (int i = tid; i < PK * 5; i += Y3_ANCHOR_THREADS) {
            const int pa = i / 5, f = i - pa * 5;
            const unsigned long long c = acc[pa * Y3_ANCHOR_ACC];
            row[i] = (long long)(f == 0 ? (c & 0xffffffffull) : f == 4 ? (c >> 32) : acc[pa * Y3_ANCHOR_ACC + f]);
        }
    } else {
        for (int i = tid; i < p.P * 2; i += Y3_ANCHOR_THREADS) row[i] = (long long)acc[i];
    }
    if (tid == 0) row[p.words - 1] = (long long)skipped;
}

// out[j] = sum over the workgroups' partial rows (integers: any order gives the same word).  A workgroup owns 16 words; 16 threads
// per word each take every 16th row, eight loads in flight, and LDS adds the 16 lanes up.  (One thread per word walking all the
// rows measured 118 us for 512 rows -- a chain of load latencies -- beside 18 us for the main kernel at P = 1, k = 9, n = 1 M.)
#define Y3_ANCHOR_FIN_WORDS 16
#define Y3_ANCHOR_FIN_LANES (Y3_ANCHOR_THREADS / Y3_ANCHOR_FIN_WORDS)
__global__ __launch_bounds__(Y3_ANCHOR_THREADS) void anchor_stats_finalize_kernel(const long long* __restrict__ partial, int rows, int words,
                                                                                  long long* __restrict__ out) {
    __shared__ long long part[Y3_ANCHOR_FIN_LANES][Y3_ANCHOR_FIN_WORDS];
    const int jw = threadIdx.x % Y3_ANCHOR_FIN_WORDS, lane = threadIdx.x / Y3_ANCHOR_FIN_WORDS;
    const int j = blockIdx.x * Y3_ANCHOR_FIN_WORDS + jw;
    long long s = 0;
    if (j < words) {
#pragma unroll 8
        for (int r = lane; r < rows; r += Y3_ANCHOR_FIN_LANES) s += partial[(long long)r * words + j];
    }
    part[lane][jw] = s;
    __syncthreads();
    if (lane == 0 && j < words) {
        long long t = 0;
#pragma unroll
        for (int l = 0; l < Y3_ANCHOR_FIN_LANES; ++l) t += part[l][jw];
        out[j] = t;
    }
}

static int anchor_words(int P, int k, int per_anchor) { return (per_anchor ? P * k * 5 : P * 2) + 1; }

static bool anchor_shape_ok(int P, int k) {
    return k >= 1 && k <= Y3_ANCHOR_MAX_K && P >= 1 && (long long)P * k <= Y3_ANCHOR_MAX_CANDIDATES;
}

extern "C" size_t y3_anchor_stats_workspace_bytes(int P, int k) {
    if (!anchor_shape_ok(P, k)) return 0;
    return (size_t)Y3_ANCHOR_MAX_BLOCKS * (size_t)anchor_words(P, k, 1) * sizeof(long long);     // (per-anchor rows are the longer ones)
}

extern "C" int y3_anchor_stats(const int* wh_dev, long long n, const float* cand_dev, int P, int k, int thr_q, int per_anchor,
                               long long* out_dev, unsigned char* labels_dev, void* workspace, y3_stream_t stream) {
    Y3_CHECK_ARG(k >= 1 && k <= Y3_ANCHOR_MAX_K, "anchor_stats: k %d outside 1..%d", k, Y3_ANCHOR_MAX_K);
    Y3_CHECK_ARG(P >= 1, "anchor_stats: P %d < 1", P);
    Y3_CHECK_ARG((long long)P * k <= Y3_ANCHOR_MAX_CANDIDATES, "anchor_stats: P * k = %lld above %d", (long long)P * k, Y3_ANCHOR_MAX_CANDIDATES);
    Y3_CHECK_ARG(n >= 1 && n <= 2147483647LL, "anchor_stats: n %lld outside 1..2^31-1", n);
    Y3_CHECK_ARG(thr_q >= 0 && thr_q <= (1 << 24), "anchor_stats: thr_q %d outside 0..2^24", thr_q);
    Y3_CHECK_ARG(!labels_dev || P == 1, "anchor_stats: labels need P == 1, got %d", P);
    Y3_CHECK_ARG(wh_dev && cand_dev && out_dev && workspace, "anchor_stats: null pointer");
    Y3_CHECK_ARG(((uintptr_t)wh_dev & 7u) == 0 && ((uintptr_t)out_dev & 7u) == 0 && ((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)cand_dev & 3u) == 0,
                 "anchor_stats: wh, out and workspace must be 8-byte aligned, candidates 4-byte");
    AnchorArgs a = {};
    a.wh = wh_dev;
    a.cand = cand_dev;
    a.n = n;
    a.head = (int)(((uintptr_t)wh_dev >> 3) & 1u);
    a.nv = (n + a.head + 1) / 2;
    a.P = P;
    a.k = k;
    a.thr_q = thr_q;
    a.per_anchor = per_anchor ? 1 : 0;
    a.words = anchor_words(P, k, a.per_anchor);
    a.labels = labels_dev;
    a.partial = (long long*)workspace;
    long long blocks = (a.nv + Y3_ANCHOR_THREADS - 1) / Y3_ANCHOR_THREADS;
    if (blocks > Y3_ANCHOR_MAX_BLOCKS) blocks = Y3_ANCHOR_MAX_BLOCKS;
    hipLaunchKernelGGL(anchor_stats_kernel, dim3((unsigned)blocks), dim3(Y3_ANCHOR_THREADS), 0, (hipStream_t)stream, a);
    Y3_CHECK_LAUNCH("anchor_stats");
    hipLaunchKernelGGL(anchor_stats_finalize_kernel, dim3((unsigned)y3_cdiv(a.words, Y3_ANCHOR_FIN_WORDS)), dim3(Y3_ANCHOR_THREADS), 0,
                       (hipStream_t)stream, a.partial, (int)blocks, a.words, out_dev);
    Y3_CHECK_LAUNCH("anchor_stats finalize");
    return Y3_OK;
}
