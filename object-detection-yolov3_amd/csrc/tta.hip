// Test-time augmentation: the flipped / transposed views of a batch written straight into the network's NHWC input,
// and the decode rows of every view mapped back to the frame of the image.  Both are data movement or one fp32 operation per
// value; compiled with -ffp-contract=off like the rest of the library.
#include "common.h"

#define Y3_TTA_TILE 32                 // source pixels per tile side
#define Y3_TTA_PITCH (Y3_TTA_TILE + 1)  // LDS row pitch in dwords: a column read (transposed views) walks banks 33 apart

int y3_tta_check_views(const int* views, int k, int h, int w, const char* what, TtaViews* out) {
    Y3_CHECK_ARG(views && k >= 1 && k <= Y3_TTA_MAX_VIEWS, "%s: 1 .. %d views (got %d)", what, Y3_TTA_MAX_VIEWS, k);
    unsigned seen = 0;
    for (int v = 0; v < k; ++v) {
        Y3_CHECK_ARG(views[v] >= 0 && views[v] < 8, "%s: view code %d outside 0 .. 7", what, views[v]);
        Y3_CHECK_ARG(!(seen & (1u << views[v])), "%s: view code %d given twice", what, views[v]);
        Y3_CHECK_ARG(!(views[v] & Y3_TTA_TRANSPOSE) || h == w, "%s: view code %d transposes, which needs a square image (got %d x %d)", what,
                     views[v], h, w);
        seen |= 1u << views[v];
        out->code[v] = views[v];
    }
    for (int v = k; v < Y3_TTA_MAX_VIEWS; ++v) out->code[v] = 0;
    out->k = k;
    return Y3_OK;
}

// One 256-thread workgroup per 32 x 32 source tile of one image.  Four channel planes at a time (the one pass of a network input of
// up to four channels) are read once (rows of 128 bytes, coalesced along W) into LDS planes of pitch 33 dwords; every view then
// reads them back and stores whole 16-byte pixels.  A straight view reads LDS along a row and thread x walks the destination row
// (forwards or, flipped, backwards: the same cache lines either way); a transposed view reads LDS along a column -- pitch 33
// keeps the 32 lanes of a half wave on 32 different banks -- so thread x again walks the DESTINATION row.  Values travel as 32-bit
// integers: a copy, bit for bit, NaN payloads included.  The channel loop's bound is a kernel argument: every thread meets
// every barrier.
__global__ __launch_bounds__(256) void tta_views_kernel(const unsigned* __restrict__ src, int C, int H, int W, unsigned* __restrict__ dst, int dC,
                                                        int ld, const TtaViews vw) {
    __shared__ unsigned tile[4][Y3_TTA_TILE][Y3_TTA_PITCH];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int x0 = blockIdx.x * Y3_TTA_TILE, y0 = blockIdx.y * Y3_TTA_TILE, img = blockIdx.z;
    const long long hw = (long long)H * W;
    const unsigned* s = src + (long long)img * C * hw;
    for (int c0 = 0; c0 < dC; c0 += 4) {
        const int cn = C - c0 < 4 ? C - c0 : 4;  // source planes of this group of four destination channels (<= 0: all padding)
        if (c0) __syncthreads();                 // the group before this one has been stored by every thread
        for (int c = 0; c < cn; ++c)
#pragma unroll
            for (int r = ty; r < Y3_TTA_TILE; r += 8) {
                const int y = y0 + r, x = x0 + tx;
                if (y < H && x < W) tile[c][r][tx] = s[(c0 + c) * hw + (long long)y * W + x];
            }
        __syncthreads();
        for (int v = 0; v < vw.k; ++v) {
            const int code = vw.code[v];
            const bool tr = code & Y3_TTA_TRANSPOSE, fx = code & Y3_TTA_FLIP_X, fy = code & Y3_TTA_FLIP_Y;
            unsigned* d = dst + ((long long)img * vw.k + v) * hw * ld + c0;  // a transposing view is square: the view is H x W as well
#pragma unroll
            for (int r = ty; r < Y3_TTA_TILE; r += 8) {
                // (ly, lx): the tile entry this thread moves; (vy, vx): where it lands in the view before the flips
                const int ly = tr ? tx : r, lx = tr ? r : tx;
                const int sy = y0 + ly, sx = x0 + lx;
                if (sy >= H || sx >= W) continue;
                int vy = tr ? sx : sy, vx = tr ? sy : sx;
                if (fx) vx = W - 1 - vx;
                if (fy) vy = H - 1 - vy;
                uint4 px;
                px.x = cn > 0 ? tile[0][ly][lx] : 0u;
                px.y = cn > 1 ? tile[1][ly][lx] : 0u;
                px.z = cn > 2 ? tile[2][ly][lx] : 0u;
                px.w = cn > 3 ? tile[3][ly][lx] : 0u;
                *(uint4*)(d + ((long long)vy * W + vx) * ld) = px;
            }
        }
    }
}

extern "C" int y3_tta_views_nhwc(const float* src, int n, int c, int h, int w, const int* views, int k, const y3_tensor* dst,
                                 y3_stream_t stream) {
    Y3_CHECK_ARG(src && dst && dst->ptr, "tta_views: null pointer");
    Y3_CHECK_ARG(n >= 1 && c >= 1 && h >= 1 && w >= 1, "tta_views: bad source (n %d, c %d, %d x %d)", n, c, h, w);
    TtaViews vw;
    if (int e = y3_tta_check_views(views, k, h, w, "tta_views", &vw)) return e;
    Y3_CHECK_ARG((long long)n * k <= 65535, "tta_views: n * k = %lld images (at most 65535)", (long long)n * k);
    Y3_CHECK_ARG(dst->n == n * k && dst->h == h && dst->w == w, "tta_views: destination %d x %d x %d, expected %d x %d x %d", dst->n, dst->h,
                 dst->w, n * k, h, w);
    Y3_CHECK_ARG(dst->c >= c && (dst->c & 3) == 0 && dst->ld >= dst->c && (dst->ld & 3) == 0 && ((uintptr_t)dst->ptr & 15) == 0,
                 "tta_views: destination needs at least the source's %d channels, c and ld multiples of 4 and 16-byte alignment (c %d, ld %d)", c,
                 dst->c, dst->ld);
    Y3_CHECK_ARG(y3_cdiv(h, Y3_TTA_TILE) <= 65535, "tta_views: image too tall");
    const dim3 grid(y3_cdiv(w, Y3_TTA_TILE), y3_cdiv(h, Y3_TTA_TILE), n);
    hipLaunchKernelGGL(tta_views_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned*)src, c, h, w, (unsigned*)dst->ptr, dst->c,
                       dst->ld, vw);
    Y3_CHECK_LAUNCH("tta_views");
    return Y3_OK;
}

// One thread per decode row: un-flip, then transpose back.  Each value is ONE fp32 subtraction (or none).
__global__ __launch_bounds__(256) void tta_unmap_kernel(float* __restrict__ rows, long long total, int nb, int ld, float fw, float fh,
                                                        const TtaViews vw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int code = vw.code[(int)((i / nb) % vw.k)];
    if (code == 0) return;
    float* r = rows + i * ld;
    float x0 = r[0], y0 = r[1], x1 = r[2], y1 = r[3];
    if (code & Y3_TTA_FLIP_X) {
        const float a = fw - x1, b = fw - x0;
        x0 = a;
        x1 = b;
    }
    if (code & Y3_TTA_FLIP_Y) {
        const float a = fh - y1, b = fh - y0;
        y0 = a;
        y1 = b;
    }
    if (code & Y3_TTA_TRANSPOSE) {
        const float a = x0, b = x1;
        x0 = y0;
        x1 = y1;
        y0 = a;
        y1 = b;
    }
    r[0] = x0;
    r[1] = y0;
    r[2] = x1;
    r[3] = y1;
}

extern "C" int y3_tta_unmap(float* rows, int n_views, int nb, int ld, const int* views, int k, int img_h, int img_w, y3_stream_t stream) {
    Y3_CHECK_ARG(rows, "tta_unmap: null pointer");
    Y3_CHECK_ARG(nb >= 1 && ld >= 4 && img_h >= 1 && img_w >= 1 && img_h <= (1 << 24) && img_w <= (1 << 24),
                 "tta_unmap: bad sizes (nb %d, ld %d, image %d x %d)", nb, ld, img_h, img_w);
    TtaViews vw;
    if (int e = y3_tta_check_views(views, k, img_h, img_w, "tta_unmap", &vw)) return e;
    Y3_CHECK_ARG(n_views >= k && n_views % k == 0, "tta_unmap: %d images are no multiple of %d views", n_views, k);
    const long long total = (long long)n_views * nb;
    Y3_CHECK_ARG(total < (1LL << 31), "tta_unmap: %lld rows (fewer than 2^31)", total);
    hipLaunchKernelGGL(tta_unmap_kernel, dim3(y3_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, rows, total, nb, ld, (float)img_w,
                       (float)img_h, vw);
    Y3_CHECK_LAUNCH("tta_unmap");
    return Y3_OK;
}
