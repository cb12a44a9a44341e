// Opt-in per-scale anchor assignment: every anchor is owned by ONE of the three scales.  The owner table
// anchor_scale[A] gives each anchor's scale (0 coarse, stride 32 .. 2 fine, stride 8); an anchor's slot is its rank among the
// anchors of its scale, in index order; scale s has A_s anchors and tensors of A_s * (5 + K) floats per cell.
// Three kernels beside their all-scales counterparts of detect.hip (format_labels_kernel, decode_kernel, truth_boxes_kernel),
// whose code is not touched.  Compiled with -ffp-contract=off like detect.hip: the label arithmetic is NumPy's float32.
#include <float.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"

#define Y3_MAX_ANCHORS 16

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// owner table -> per-scale counts, slot of every anchor, anchors of every scale in slot order; false on a bad table
struct ScaleTable {
    int count[3];
    int slot[Y3_MAX_ANCHORS];
    int member[3][Y3_MAX_ANCHORS];
};

static bool scale_table(const int* anchor_scale, int A, ScaleTable* t) {
    t->count[0] = t->count[1] = t->count[2] = 0;
    for (int a = 0; a < A; ++a) {
        const int s = anchor_scale[a];
        if (s < 0 || s > 2) return false;
        t->slot[a] = t->count[s];
        t->member[s][t->count[s]++] = a;
    }
    return t->count[0] >= 1 && t->count[1] >= 1 && t->count[2] >= 1;
}

// ---------------------------------------------------------------------------
// ground-truth label tensors, one scale per anchor
// ---------------------------------------------------------------------------
// format_labels_kernel with two differences: a scale's cell holds A_s rows, so the run of whole cells a workgroup owns has a
// length per scale; and a box whose best anchor (over ALL anchors) another scale owns leaves no key in this scale's runs.
#define Y3_LABEL_CHUNK 256          // boxes per pass = threads per workgroup
#define Y3_LABEL_RUN_FLOATS 16384   // floats a workgroup owns (rounded to whole cells)

struct LabelScaleArgs {
    const int* boxes;   // [N][max_boxes][5]
    const int* counts;  // [N]
    float* out[3];
    int gh[3], gw[3];
    int block_start[4];  // first workgroup of each scale
    int cells_per_block[3];
    int As[3];
    int N, max_boxes, A, K;
    float img_h, img_w;
    float aw[Y3_MAX_ANCHORS], ah[Y3_MAX_ANCHORS];
    int owner[Y3_MAX_ANCHORS], slot[Y3_MAX_ANCHORS];
};

__global__ __launch_bounds__(Y3_LABEL_CHUNK) void format_labels_scales_kernel(const LabelScaleArgs p) {
    __shared__ int key[Y3_LABEL_CHUNK];
    const int tid = threadIdx.x;
    int s = 0;
    while (s < 2 && (int)blockIdx.x >= p.block_start[s + 1]) ++s;
    const int gh = p.gh[s], gw = p.gw[s];
    const int As = p.As[s], cpb = p.cells_per_block[s];
    const int D = 5 + p.K, AD = As * D;
    const long long cells = (long long)gh * gw;
    const long long total = cells * p.N;
    const long long c0 = (long long)((int)blockIdx.x - p.block_start[s]) * cpb;
    const long long c1 = c0 + cpb < total ? c0 + cpb : total;
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
                for (int a = 0; a < p.A; ++a) {      // ALL anchors: the best one decides the scale
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
                // a cell or class outside the tensor writes nothing, as in format_labels_kernel; nor does another scale's anchor
                if (p.owner[best] == s && fi >= 0.f && fi < (float)gh && fj >= 0.f && fj < (float)gw && cls >= 0 && cls < p.K) {
                    const long long cell = (long long)n * cells + (long long)((int)fi * gw + (int)fj);
                    if (cell >= c0 && cell < c1) k = (int)(cell - c0) * As + p.slot[best];
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

extern "C" int y3_format_labels_scales(const int* boxes, const int* counts, int n, int max_boxes, const float* anchors_host,
                                       const int* anchor_scale_host, int num_anchors, int num_classes, int img_h, int img_w, float* out1,
                                       float* out2, float* out3, y3_stream_t stream) {
    Y3_CHECK_ARG(counts && anchors_host && anchor_scale_host && out1 && out2 && out3, "format_labels_scales: null pointer");
    Y3_CHECK_ARG(max_boxes >= 0 && (boxes || max_boxes == 0), "format_labels_scales: max_boxes %d%s", max_boxes, boxes ? "" : " with null boxes");
    Y3_CHECK_ARG(n >= 1 && num_anchors >= 3 && num_anchors <= Y3_MAX_ANCHORS && num_classes >= 1,
                 "format_labels_scales: n %d anchors %d (3..16) classes %d", n, num_anchors, num_classes);
    Y3_CHECK_ARG(img_h >= 32 && img_w >= 32 && img_h % 32 == 0 && img_w % 32 == 0 && img_h < (1 << 24) && img_w < (1 << 24),
                 "format_labels_scales: image %dx%d (multiples of 32)", img_h, img_w);
    Y3_CHECK_ARG((long long)n * max_boxes * 5 < (1LL << 31), "format_labels_scales: %d x %d boxes too many", n, max_boxes);
    ScaleTable tab;
    Y3_CHECK_ARG(scale_table(anchor_scale_host, num_anchors, &tab),
                 "format_labels_scales: anchor_scale entries must be 0, 1 or 2 and every scale must own an anchor");
    LabelScaleArgs p = {};
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
    long long blocks = 0;
    for (int s = 0; s < 3; ++s) {
        const long long AD = (long long)tab.count[s] * (5 + num_classes);
        Y3_CHECK_ARG(AD < (1LL << 31), "format_labels_scales: %d classes too many", num_classes);
        p.As[s] = tab.count[s];
        p.cells_per_block[s] = Y3_LABEL_RUN_FLOATS / AD > 0 ? (int)(Y3_LABEL_RUN_FLOATS / AD) : 1;
        p.gh[s] = img_h / (32 >> s);
        p.gw[s] = img_w / (32 >> s);
        p.block_start[s] = (int)blocks;
        blocks += ((long long)n * p.gh[s] * p.gw[s] + p.cells_per_block[s] - 1) / p.cells_per_block[s];
        Y3_CHECK_ARG(blocks < (1LL << 31), "format_labels_scales: labels too large");
    }
    p.block_start[3] = (int)blocks;
    for (int a = 0; a < num_anchors; ++a) {
        p.aw[a] = anchors_host[2 * a];
        p.ah[a] = anchors_host[2 * a + 1];
        p.owner[a] = anchor_scale_host[a];
        p.slot[a] = tab.slot[a];
    }
    hipLaunchKernelGGL(format_labels_scales_kernel, dim3((unsigned)blocks), dim3(Y3_LABEL_CHUNK), 0, (hipStream_t)stream, p);
    Y3_CHECK_LAUNCH("format_labels_scales");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// decode, A_s boxes per cell of scale s
// ---------------------------------------------------------------------------
struct DecodeScaleArgs {
    const float* fm[3];
    int ld[3], gh[3], gw[3], As[3], start[4];
    float sx[3], sy[3];
    float aw[3][Y3_MAX_ANCHORS], ah[3][Y3_MAX_ANCHORS];   // the anchors of each scale in slot order
    int K, N, nb;
    float* out;
};

// decode_kernel gives a row to one thread, which stores its 5 + K floats one after the other: at K = 80 neighbouring lanes write 340
// bytes apart.  Here a wave takes 64 / D consecutive rows (one row when D >= 64) and a lane one channel of one of them (every 64th
// channel of the row when D > 64): the out rows are dense, so a wave's stores are one contiguous stretch, and so are its loads
// within a cell.  Each value is decode_kernel's expression, operand for operand, so the bits are the same.
__global__ __launch_bounds__(256) void decode_scales_kernel(const DecodeScaleArgs p) {
    const long long total = (long long)p.N * p.nb;
    const int D = 5 + p.K;
    const int rpw = D >= 64 ? 1 : 64 / D;                       // rows per wave and trip
    const int lane = threadIdx.x & 63;
    const int sub = rpw == 1 ? 0 : lane / D;                    // which of the wave's rows
    const int ch0 = rpw == 1 ? lane : lane - sub * D;           // first channel of this lane
    if (sub >= rpw) return;                                     // lanes past the last whole row of the wave (no barrier below)
    const long long waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long i0 = ((((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6)) * rpw; i0 < total; i0 += waves * rpw) {
        const long long i = i0 + sub;
        if (i >= total) continue;
        const int n = (int)(i / p.nb);
        const int b = (int)(i - (long long)n * p.nb);
        int s = 0;
        while (s + 1 < 3 && b >= p.start[s + 1]) ++s;
        const int r = b - p.start[s];
        const int a = r % p.As[s];
        const int cell = r / p.As[s];
        const int gy = cell / p.gw[s], gx = cell - gy * p.gw[s];
        const float* t = p.fm[s] + ((long long)n * p.gh[s] * p.gw[s] + cell) * p.ld[s] + a * D;
        float* o = p.out + i * D;
        for (int ch = ch0; ch < D; ch += 64) {
            float v;
            if (ch >= 4) {
                v = sigmoidf_(t[ch]);
            } else if ((ch & 1) == 0) {
                // reorg_layer, in decode_kernel's expression order
                const float cx = (sigmoidf_(t[0]) + (float)gx) * p.sx[s];
                const float w = expf(t[2]) * p.aw[s][a];
                v = ch == 0 ? cx - w / 2.0f : cx + w / 2.0f;
            } else {
                const float cy = (sigmoidf_(t[1]) + (float)gy) * p.sy[s];
                const float h = expf(t[3]) * p.ah[s][a];
                v = ch == 1 ? cy - h / 2.0f : cy + h / 2.0f;
            }
            o[ch] = v;
        }
    }
}

extern "C" int y3_decode_fwd_scales(const y3_tensor* fm, const float* anchors_host, const int* anchor_scale_host, int num_anchors,
                                    int num_classes, int img_h, int img_w, float* out, y3_stream_t stream) {
    Y3_CHECK_ARG(fm && anchors_host && anchor_scale_host && out, "decode_fwd_scales: null pointer");
    Y3_CHECK_ARG(num_anchors >= 3 && num_anchors <= Y3_MAX_ANCHORS && num_classes >= 1, "decode_fwd_scales: anchors %d (3..16) classes %d",
                 num_anchors, num_classes);
    ScaleTable tab;
    Y3_CHECK_ARG(scale_table(anchor_scale_host, num_anchors, &tab),
                 "decode_fwd_scales: anchor_scale entries must be 0, 1 or 2 and every scale must own an anchor");
    DecodeScaleArgs p = {};
    p.K = num_classes;
    p.N = fm[0].n;
    Y3_CHECK_ARG(p.N >= 1, "decode_fwd_scales: batch %d", p.N);
    long long nb = 0;
    for (int s = 0; s < 3; ++s) {
        const int As = tab.count[s];
        Y3_CHECK_ARG(fm[s].ptr && fm[s].n == p.N && fm[s].h >= 1 && fm[s].w >= 1 && fm[s].c == As * (5 + num_classes) && fm[s].ld >= fm[s].c,
                     "decode_fwd_scales: feature map %d geometry (%d anchors of this scale need %d channels)", s, As, As * (5 + num_classes));
        p.fm[s] = fm[s].ptr;
        p.ld[s] = fm[s].ld;
        p.gh[s] = fm[s].h;
        p.gw[s] = fm[s].w;
        p.As[s] = As;
        p.start[s] = (int)nb;
        nb += (long long)fm[s].h * fm[s].w * As;
        Y3_CHECK_ARG(nb < (1LL << 31), "decode_fwd_scales: too many boxes per image");
        // Q6: stride = img_size[0:2] // grid = (s_y, s_x) multiplies (x, y)
        p.sx[s] = (float)(img_h / fm[s].h);
        p.sy[s] = (float)(img_w / fm[s].w);
        for (int j = 0; j < As; ++j) {
            p.aw[s][j] = anchors_host[2 * tab.member[s][j]];
            p.ah[s][j] = anchors_host[2 * tab.member[s][j] + 1];
        }
    }
    p.start[3] = (int)nb;
    p.nb = (int)nb;
    p.out = out;
    const long long total = (long long)p.N * nb;
    const int D = 5 + num_classes;
    const int rows_per_block = 4 * (D >= 64 ? 1 : 64 / D);      // four waves, 64 / D rows each (decode_scales_kernel)
    long long blocks = (total + rows_per_block - 1) / rows_per_block;
    if (blocks > 2048) blocks = 2048;                           // the waves stride over the rest
    hipLaunchKernelGGL(decode_scales_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    Y3_CHECK_LAUNCH("decode_scales");
    return Y3_OK;
}

// ---------------------------------------------------------------------------
// per-image ground-truth box lists gathered from the three label tensors (the truth ignore mask)
// ---------------------------------------------------------------------------
// truth_boxes_kernel's ordered append (ballot prefix inside a wave, the four waves' counts in LDS; no atomics), run over the
// three tensors coarse -> fine with the running base carried from one tensor to the next.  Loop bounds are kernel arguments.
struct TruthScaleArgs {
    const float* gt[3];
    int ca[3];      // rows per image: cells x anchors of the scale
    int d, cap;
    float* boxes;
    int* counts;
};

__global__ __launch_bounds__(256) void truth_boxes_scales_kernel(const TruthScaleArgs p) {
    __shared__ int wave_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* out = p.boxes + (long long)blockIdx.x * p.cap * 4;
    int base = 0;
    for (int s = 0; s < 3; ++s) {
        const int ca = p.ca[s];
        const float* g = p.gt[s] + (long long)blockIdx.x * ca * p.d;
        for (int r0 = 0; r0 < ca; r0 += 256) {
            const int r = r0 + tid;
            const float* row = g + (long long)(r < ca ? r : 0) * p.d;
            const bool keep = r < ca && row[4] != 0.f;
            const unsigned long long bal = __ballot(keep);
            if (lane == 0) wave_cnt[wave] = __popcll(bal);
            __syncthreads();
            int off = base;
            for (int w = 0; w < wave; ++w) off += wave_cnt[w];
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && pos < p.cap) {
                float* dst = out + (long long)pos * 4;
                dst[0] = row[0];
                dst[1] = row[1];
                dst[2] = row[2];
                dst[3] = row[3];
            }
            base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
            __syncthreads();
        }
    }
    if (tid == 0) p.counts[blockIdx.x] = base;
}

extern "C" int y3_truth_boxes_scales(const float* gt1, const float* gt2, const float* gt3, int n, long long cells_anchors1,
                                     long long cells_anchors2, long long cells_anchors3, int d, float* boxes, int* counts, int cap,
                                     y3_stream_t stream) {
    Y3_CHECK_ARG(gt1 && gt2 && gt3 && boxes && counts, "truth_boxes_scales: null pointer");
    const long long ca[3] = {cells_anchors1, cells_anchors2, cells_anchors3};
    long long sum = 0;
    for (int s = 0; s < 3; ++s) {
        Y3_CHECK_ARG(ca[s] >= 1 && ca[s] < (1LL << 31) - 256, "truth_boxes_scales: cells_anchors %lld of tensor %d", ca[s], s);
        sum += ca[s];
    }
    // the total is an int in the kernel
    Y3_CHECK_ARG(n >= 1 && sum < (1LL << 31) - 256 && d >= 5 && cap >= 1, "truth_boxes_scales: bad sizes (n %d, rows %lld, d %d, cap %d)", n, sum, d,
                 cap);
    TruthScaleArgs p = {};
    p.gt[0] = gt1;
    p.gt[1] = gt2;
    p.gt[2] = gt3;
    for (int s = 0; s < 3; ++s) p.ca[s] = (int)ca[s];
    p.d = d;
    p.cap = cap;
    p.boxes = boxes;
    p.counts = counts;
    hipLaunchKernelGGL(truth_boxes_scales_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, p);
    Y3_CHECK_LAUNCH("truth_boxes_scales");
    return Y3_OK;
}
