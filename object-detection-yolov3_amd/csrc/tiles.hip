// Tiled inference, after the per-tile NMS: ghost-band rejection, shift to image coordinates, rounding, the centre-outside-image
// test, the clamp and the ordered append of the survivors to one device pool (inference_tiled.py:230-301; the host restatement
// is merge_tile_detections + finalize_predictions of this project's inference_tiled.py).
// Compiled with -ffp-contract=off: every fp32 step below is the one NumPy performs, in its order.
#include <limits.h>

#include "common.h"

struct TileMergeArgs {
    const float* rows;  // [n][nb][ld]
    const int* keep_idx;
    const int* keep_cnt;
    const float* keep_score;
    const int* table;  // [n][6] = {y0, ny, pre_y, x0, nx, pre_x}
    int n, nb, ld, K, max_keep;
    int img_h, img_w;
    float edge, lo_y, hi_y, lo_x, hi_x;  // E;  E - margin;  th - E + margin;  E - margin;  tw - E + margin
    float far_y, far_x;                  // H - E, W - E
    float* pool;                         // [cap][6]
    int cap;
    int* pool_count;  // {rows written, rows needed}
    int* ws;          // [0] = rows needed before this batch, [1 + s] = survivors of segment s = tile * K + class
    const float* voted;  // VOTED kernels only: [n][K][max_keep][6], y3_box_vote's out (box and score of entry e at voted + e * 6)
};

// np.round(...).astype(np.int32) of one float32: half-to-even, then the conversion NumPy performs on x86-64 (cvttss2si: anything
// outside int32, NaN included, becomes INT_MIN)
__device__ __forceinline__ int tile_round_i32(float v) {
    const float r = rintf(v);
    return (r >= -2147483648.f && r < 2147483648.f) ? (int)r : INT_MIN;
}
__device__ __forceinline__ int tile_clamp(int v, int lim) { return v < 0 ? 0 : (v >= lim ? lim - 1 : v); }

// Entry j of segment (tile t, class c): does it survive, and as which pool row.  VOTED: the box and the score come from p.voted
// (tile test-time augmentation with box voting) instead of rows[keep_idx] and keep_score; nothing else differs.
template <bool VOTED>
__device__ __forceinline__ bool tile_merge_entry(const TileMergeArgs& p, int t, int c, int j, float ty, float tx, float* out) {
    const long long e = ((long long)t * p.K + c) * p.max_keep + j;
    const int row = p.keep_idx[e];
    if (row < 0 || row >= p.nb) return false;  // never produced by the NMS kernels; nothing outside `rows` is read
    const float* r = VOTED ? p.voted + e * 6 : p.rows + ((long long)t * p.nb + row) * p.ld;
    const float b0 = r[0], b1 = r[1], b2 = r[2], b3 = r[3];
    const float cx = (b2 + b0) / 2.0f, cy = (b3 + b1) / 2.0f;
    const float cxg = cx + tx, cyg = cy + ty;
    const bool ghost = (cyg > p.edge && cy < p.lo_y) || (cyg <= p.far_y && cy >= p.hi_y) || (cxg > p.edge && cx < p.lo_x) ||
                       (cxg <= p.far_x && cx >= p.hi_x);
    if (ghost) return false;
    const int x0 = tile_round_i32(b0 + tx), y0 = tile_round_i32(b1 + ty), x1 = tile_round_i32(b2 + tx), y1 = tile_round_i32(b3 + ty);
    // (x1 + x0) / 2.0 < 0 or >= W, decided on the int32 sum (which wraps as NumPy's does)
    const int sx = (int)((unsigned)x1 + (unsigned)x0), sy = (int)((unsigned)y1 + (unsigned)y0);
    if (sx < 0 || (long long)sx >= 2LL * p.img_w || sy < 0 || (long long)sy >= 2LL * p.img_h) return false;
    out[0] = (float)tile_clamp(x0, p.img_w);
    out[1] = (float)tile_clamp(y0, p.img_h);
    out[2] = (float)tile_clamp(x1, p.img_w);
    out[3] = (float)tile_clamp(y1, p.img_h);
    out[4] = VOTED ? r[4] : p.keep_score[e];
    out[5] = (float)c;
    return true;
}

// One 256-thread workgroup per segment.  WRITE == false: count the segment's survivors into ws[1 + s]; workgroup 0 also copies
// the rows needed so far into ws[0] (pool_count is only read by this launch).  WRITE == true: the segment starts at ws[0] + the
// sum of the counts before it and its survivors go out in keep order (ballot prefix inside a wave, the four waves' counts in
// LDS); workgroup 0 stores the new totals (pool_count is only written by this launch).  No atomics: the positions are sums.
template <bool WRITE, bool VOTED>
__global__ __launch_bounds__(256) void tile_merge_kernel(const TileMergeArgs p) {
    __shared__ int wave_cnt[4];
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, t = s / p.K, c = s - t * p.K;
    const int nseg = p.n * p.K;
    long long base = 0;  // 64-bit: the rows needed so far plus this batch's may pass 2^31 (the stored total then saturates)
    if (WRITE) {
        int part = 0, all = 0;
        for (int i = tid; i < nseg; i += 256) {
            const int v = p.ws[1 + i];
            all += v;
            if (i < s) part += v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            part += __shfl_xor(part, o);
            all += __shfl_xor(all, o);
        }
        if (lane == 0) {
            wave_cnt[wave] = part;
            red[wave] = all;
        }
        __syncthreads();
        const int before = p.ws[0];
        base = (long long)before + (wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]);
        if (s == 0 && tid == 0) {
            const long long need = (long long)before + (red[0] + red[1] + red[2] + red[3]);
            p.pool_count[1] = need > INT_MAX ? INT_MAX : (int)need;
            p.pool_count[0] = need < p.cap ? (int)need : p.cap;
        }
        __syncthreads();
    } else if (s == 0 && tid == 0) {
        p.ws[0] = p.pool_count[1];
    }
    int cnt = p.keep_cnt[s];
    cnt = cnt < 0 ? 0 : (cnt > p.max_keep ? p.max_keep : cnt);
    const float ty = (float)p.table[t * 6 + 0], tx = (float)p.table[t * 6 + 3];
    int total = 0;
    for (int j0 = 0; j0 < cnt; j0 += 256) {
        const int j = j0 + tid;
        float o[6];
        const bool keep = j < cnt && tile_merge_entry<VOTED>(p, t, c, j, ty, tx, o);
        const unsigned long long bal = __ballot(keep);
        if (WRITE) {
            if (lane == 0) wave_cnt[wave] = __popcll(bal);
            __syncthreads();
            long long off = base;
            for (int w = 0; w < wave; ++w) off += wave_cnt[w];
            const long long pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && pos < p.cap) {
                float* dst = p.pool + pos * 6;
#pragma unroll
                for (int q = 0; q < 6; ++q) dst[q] = o[q];
            }
            base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
            __syncthreads();
        } else {
            total += lane == 0 ? __popcll(bal) : 0;
        }
    }
    if (!WRITE) {
        if (lane == 0) wave_cnt[wave] = total;
        __syncthreads();
        if (tid == 0) p.ws[1 + s] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    }
}

extern "C" size_t y3_tile_merge_workspace_bytes(int n, int num_classes) {
    if (n < 1 || num_classes < 1) return 0;
    return ((size_t)n * (size_t)num_classes + 1) * sizeof(int);
}

// rows / keep_score (voted == nullptr) or voted (rows == nullptr): the one difference between the two entry points
static int tile_merge_launch(const char* what, const float* rows, int n, int nb, int ld, int num_classes, const int* keep_idx, const int* keep_cnt,
                             const float* keep_score, const float* voted, int max_keep, const int* table_dev, int tile_h, int tile_w, int img_h,
                             int img_w, int edge, float margin, float* pool, int cap, int* pool_count, void* workspace, size_t workspace_bytes,
                             y3_stream_t stream) {
    Y3_CHECK_ARG((voted || (rows && keep_score)) && keep_idx && keep_cnt && table_dev && pool && pool_count && workspace, "%s: null pointer", what);
    Y3_CHECK_ARG(n >= 1 && nb >= 1 && ld >= 4 && num_classes >= 1 && max_keep >= 1 && cap >= 1,
                 "%s: bad sizes (n %d, nb %d, ld %d, classes %d, max_keep %d, cap %d)", what, n, nb, ld, num_classes, max_keep, cap);
    // every workgroup of the write launch adds up the counts before its segment itself: fine for the few hundred segments of a batch
    // of tiles, quadratic beyond
    Y3_CHECK_ARG((long long)n * num_classes <= Y3_TILE_MERGE_MAX_SEGMENTS, "%s: n * classes = %lld segments (at most %d per call)", what,
                 (long long)n * num_classes, Y3_TILE_MERGE_MAX_SEGMENTS);
    Y3_CHECK_ARG((long long)n * num_classes * max_keep < (1LL << 31), "%s: n * classes * max_keep overflows", what);
    // rounded, clamped coordinates are stored as fp32: exact below 2^24
    Y3_CHECK_ARG(img_h >= 1 && img_w >= 1 && img_h <= (1 << 24) && img_w <= (1 << 24), "%s: image %d x %d (sides 1 .. 2^24)", what, img_h, img_w);
    Y3_CHECK_ARG(tile_h >= 1 && tile_w >= 1 && tile_h <= (1 << 24) && tile_w <= (1 << 24), "%s: tile %d x %d", what, tile_h, tile_w);
    Y3_CHECK_ARG(edge >= 0 && edge <= (1 << 20), "%s: edge %d", what, edge);
    Y3_CHECK_ARG((margin >= 0.f && margin < (float)edge) || (edge == 0 && margin == 0.f), "%s: margin %g outside [0, edge = %d)", what,
                 (double)margin, edge);
    Y3_CHECK_ARG(workspace_bytes >= y3_tile_merge_workspace_bytes(n, num_classes), "%s: workspace too small", what);
    TileMergeArgs p = {};
    p.rows = rows;
    p.voted = voted;
    p.keep_idx = keep_idx;
    p.keep_cnt = keep_cnt;
    p.keep_score = keep_score;
    p.table = table_dev;
    p.n = n;
    p.nb = nb;
    p.ld = ld;
    p.K = num_classes;
    p.max_keep = max_keep;
    p.img_h = img_h;
    p.img_w = img_w;
    p.edge = (float)edge;
    p.lo_y = p.lo_x = (float)edge - margin;
    p.hi_y = (float)(tile_h - edge) + margin;
    p.hi_x = (float)(tile_w - edge) + margin;
    p.far_y = (float)(img_h - edge);
    p.far_x = (float)(img_w - edge);
    p.pool = pool;
    p.cap = cap;
    p.pool_count = pool_count;
    p.ws = (int*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(n * num_classes), block(256);
    if (voted) {
        hipLaunchKernelGGL((tile_merge_kernel<false, true>), grid, block, 0, st, p);
        Y3_CHECK_LAUNCH("tile_merge_voted (count)");
        hipLaunchKernelGGL((tile_merge_kernel<true, true>), grid, block, 0, st, p);
        Y3_CHECK_LAUNCH("tile_merge_voted (write)");
    } else {
        hipLaunchKernelGGL((tile_merge_kernel<false, false>), grid, block, 0, st, p);
        Y3_CHECK_LAUNCH("tile_merge (count)");
        hipLaunchKernelGGL((tile_merge_kernel<true, false>), grid, block, 0, st, p);
        Y3_CHECK_LAUNCH("tile_merge (write)");
    }
    return Y3_OK;
}

extern "C" int y3_tile_merge(const float* rows, int n, int nb, int ld, int num_classes, const int* keep_idx, const int* keep_cnt,
                             const float* keep_score, int max_keep, const int* table_dev, int tile_h, int tile_w, int img_h, int img_w,
                             int edge, float margin, float* pool, int cap, int* pool_count, void* workspace, size_t workspace_bytes,
                             y3_stream_t stream) {
    return tile_merge_launch("tile_merge", rows, n, nb, ld, num_classes, keep_idx, keep_cnt, keep_score, nullptr, max_keep, table_dev, tile_h,
                             tile_w, img_h, img_w, edge, margin, pool, cap, pool_count, workspace, workspace_bytes, stream);
}

extern "C" int y3_tile_merge_voted(const float* voted, int n, int nb, int num_classes, const int* keep_idx, const int* keep_cnt, int max_keep,
                                   const int* table_dev, int tile_h, int tile_w, int img_h, int img_w, int edge, float margin, float* pool,
                                   int cap, int* pool_count, void* workspace, size_t workspace_bytes, y3_stream_t stream) {
    Y3_CHECK_ARG(voted, "tile_merge_voted: null pointer");
    return tile_merge_launch("tile_merge_voted", nullptr, n, nb, 6, num_classes, keep_idx, keep_cnt, nullptr, voted, max_keep, table_dev, tile_h,
                             tile_w, img_h, img_w, edge, margin, pool, cap, pool_count, workspace, workspace_bytes, stream);
}
