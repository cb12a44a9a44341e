// Letterbox front end of inference: a ragged batch of HWC images of any size and dtype -> antialiased (triangle
// filtered, separable) resample with the aspect ratio kept -> padded network frame, un-normalised (y3_letterbox_batch) or z-scored
// on the content alone and written as the network's NHWC input (y3_letterbox_zscore_nhwc); and the decode rows mapped back to each
// image's own frame (y3_letterbox_unmap).  Compiled with -ffp-contract=off: every fp32 step below is one rounding, in the order
// yolo3hip.h states.
//
// The weights.  For one axis with in / out = a / b in lowest terms and D = 2 max(a, b), tap j of output o has the weight
//   max(0, 1 - |(j - ctr + 0.5) / u|) = max(0, D - |(2j + 1) b - (2o + 1) a|) / D,        ctr = (a / b)(o + 0.5), u = max(a / b, 1)
// so the numerator wn is an integer <= D <= 65536, D cancels in the normalisation, and sum(wn) <= 2 a (a / b) <= 2^22 when
// a / b <= 64 (<= 2 b <= 2^16 when enlarging): weights and their sum are EXACT in fp32, a zero weight is decided in integers.
#include "common.h"

#define Y3_LB_ROWS 8        // output rows per workgroup (a band)
#define Y3_LB_COLS 256      // output elements (column x channel) per workgroup: one per thread
#define Y3_LB_CHUNK 16384   // bytes of an LDS stage (whole rows, or one chunk of a long row): four 16-byte loads per thread
#define Y3_LB_MAX_SIDE 32768
#define Y3_LB_MAX_SCALE 64
#define Y3_LB_ZS_BLOCKS 128  // partition of the content statistics: that of y3_zscore

struct LbAxis {
    int a, b, den;  // in / out in lowest terms, 2 max(a, b)
    int in, out;
};
struct LbImage {
    unsigned long long off;
    int pad_y, pad_x;
    float sy, sx;
    LbAxis ay, ax;
};
struct LbBatch {
    LbImage im[Y3_LETTERBOX_MAX_IMAGES];
};

static int lb_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}
static LbAxis lb_axis(int in, int out) {
    const int g = lb_gcd(in, out);
    LbAxis A;
    A.a = in / g;
    A.b = out / g;
    A.den = 2 * (A.a > A.b ? A.a : A.b);
    A.in = in;
    A.out = out;
    return A;
}

// first tap and one past the last: floor(ctr - u + 0.5) and floor(ctr + u + 0.5) as ratios of integers over 2 b.  a <= 2^15 and
// 2o + 1 < 2^16: the numerators fit 32 unsigned bits, and the divisions are 32-bit ones
__device__ __forceinline__ int lb_lo(const LbAxis& A, int o) {
    const unsigned t = (unsigned)A.a * (unsigned)(2 * o + 1) + (unsigned)A.b, d = (unsigned)A.den;
    return t <= d ? 0 : (int)((t - d) / (2u * (unsigned)A.b));
}
__device__ __forceinline__ int lb_hi(const LbAxis& A, int o) {
    const unsigned t = (unsigned)A.a * (unsigned)(2 * o + 1) + (unsigned)A.den + (unsigned)A.b;
    const unsigned h = t / (2u * (unsigned)A.b);
    return h < (unsigned)A.in ? (int)h : A.in;
}
// (2j + 1) b - (2o + 1) a for a tap within reach of o: below 2^18 in magnitude
__device__ __forceinline__ int lb_num(const LbAxis& A, int o, int j) { return (int)((long long)(2 * j + 1) * A.b - (long long)(2 * o + 1) * A.a); }
__device__ __forceinline__ int lb_weight(const LbAxis& A, int num) {
    const int w = A.den - (num < 0 ? -num : num);
    return w > 0 ? w : 0;
}

// One 16-byte slot of a row stage: relative byte `rel` of source row `row` (row + rel is a multiple of 16).  The last slot of an
// image may reach past its end: those bytes are not read.
__device__ __forceinline__ uint4 lb_load_slot(const unsigned char* __restrict__ img, size_t img_bytes, size_t row, int rel) {
    const size_t at = row + (long long)rel;
    if (at + 16 <= img_bytes) return *(const uint4*)(img + at);
    union {
        uint4 v;
        unsigned char b[16];
    } u;
    u.v = make_uint4(0u, 0u, 0u, 0u);
    for (int q = 0; q < 16; ++q)
        if (at + q < img_bytes) u.b[q] = img[at + q];
    return u.v;
}

// One 256-thread workgroup per (band of 8 output rows, group of 256 output ELEMENTS -- column x channel, channel fastest --,
// image); one element per thread.  Every source row the band's filter reaches is read from memory once per workgroup (so once per
// band and per element group, the groups of a band sharing only the filter support at their seams), in 16-byte slots from the
// 16-byte boundary below its first needed byte, and staged in LDS in stages of 16 KiB: as many whole rows as fit, or one chunk of
// a row too long for that.  The stages are double buffered: the loads of the next one are in flight while this one is reduced.
// The thread that owns an output element reduces its taps horizontally, ascending (neighbouring threads read neighbouring LDS
// bytes: the channels of a pixel); across the chunks of a long row the partial sum is carried in the same register, so the order
// of the additions does not depend on where the chunks fall.  The reduced value stays in a register and is accumulated, rows
// ascending, into the (at most 8) output rows it contributes to.  Neighbouring bands re-read the rows of the filter support
// only; nothing of size [src_h][new_w] exists anywhere.  The taps lo .. hi-1 of an output have positive weight except possibly
// the last ones (lo = floor(ctr - u + 0.5) > ctr - u - 0.5): the thread trims those once, and no tap of weight zero is read
// afterwards.  Every thread meets every barrier: the loop bounds are workgroup-uniform.
template <typename T, int C>
__global__ __launch_bounds__(256) void letterbox_resample_kernel(const unsigned char* __restrict__ src, const LbBatch B, float* __restrict__ out,
                                                                 int H, int W) {
    __shared__ uint4 stage[2][Y3_LB_CHUNK / 16];
    const LbImage& I = B.im[blockIdx.z];
    const LbAxis ay = I.ay, ax = I.ax;
    const int o0 = blockIdx.y * Y3_LB_ROWS, e0 = blockIdx.x * Y3_LB_COLS, ne = ax.out * C;
    if (o0 >= ay.out || e0 >= ne) return;  // uniform: this image's content is smaller than the grid
    const int o1 = min(o0 + Y3_LB_ROWS, ay.out), e1 = min(e0 + Y3_LB_COLS, ne);
    const int tid = threadIdx.x, e = e0 + tid;
    const bool active = e < e1;
    const int x = e / C, ch = e - x * C;
    constexpr int SZ = (int)sizeof(T), PX = C * SZ;  // bytes of an element, of a pixel

    int jlo = 0, jhi = 0, num0 = 0, wsum_x = 1;
    if (active) {
        jlo = lb_lo(ax, x);
        jhi = lb_hi(ax, x);
        num0 = lb_num(ax, x, jlo);
        while (lb_weight(ax, num0 + 2 * ax.b * (jhi - 1 - jlo)) == 0) --jhi;  // tap jlo has positive weight: this ends
        wsum_x = 0;
        for (int j = jlo, num = num0; j < jhi; ++j, num += 2 * ax.b) wsum_x += lb_weight(ax, num);
    }
    const float wsum_xf = (float)wsum_x, denf = (float)ax.den, stepf = (float)(2 * ax.b);
    const int rb0 = lb_lo(ax, e0 / C) * PX, rb1 = lb_hi(ax, (e1 - 1) / C) * PX;  // the row bytes this workgroup needs
    const int i0 = lb_lo(ay, o0), i1 = lb_hi(ay, o1 - 1);
    const size_t row_bytes = (size_t)ax.in * PX, img_bytes = (size_t)ay.in * row_bytes;
    const unsigned char* img = src + I.off;

    float acc[Y3_LB_ROWS];
    int vsum[Y3_LB_ROWS];
#pragma unroll
    for (int r = 0; r < Y3_LB_ROWS; ++r) {
        vsum[r] = 0;
        acc[r] = 0.f;
    }

    // A stage is Y3_LB_CHUNK bytes of LDS.  Where the bytes a row contributes (at any alignment: span16) fit more than once, a
    // stage holds R whole rows, row rr at byte rr * span16 -- many rows' loads in flight together, one barrier for all of them;
    // otherwise it holds chunk k of one row: the row-relative bytes [ra + k * CHUNK, ra + (k + 1) * CHUNK).  Slot s of a stage
    // (16 bytes) is loaded by thread s % 256; its row within the stage and slot within the row are fixed for the walk.
    constexpr int SLOTS = Y3_LB_CHUNK / 16 / 256;
    const int span16 = ((rb1 - rb0 + 30) >> 4) << 4;
    const bool multi = span16 <= Y3_LB_CHUNK;
    const int nsr = multi ? span16 >> 4 : Y3_LB_CHUNK / 16, R = multi ? Y3_LB_CHUNK / span16 : 1, row_lds = multi ? span16 : 0;
    int srow[SLOTS], ssl[SLOTS];
#pragma unroll
    for (int m = 0; m < SLOTS; ++m) {
        srow[m] = (tid + 256 * m) / nsr;
        ssl[m] = (tid + 256 * m) - srow[m] * nsr;
    }
    auto row_start = [&](int row) { return rb0 - (int)(((size_t)row * row_bytes + rb0) & 15); };  // 16-byte boundary below the row's first byte
    uint4 regs[SLOTS];
    auto load_stage = [&](int si, int sk) {
        const int nrows = min(R, i1 - si);
#pragma unroll
        for (int m = 0; m < SLOTS; ++m) {
            const int row = si + srow[m], rel = row_start(row) + sk * Y3_LB_CHUNK + ssl[m] * 16;
            if (srow[m] < nrows && rel < rb1) regs[m] = lb_load_slot(img, img_bytes, (size_t)row * row_bytes, rel);
        }
    };
    auto store_stage = [&](int si, int sk, int buf) {
        const int nrows = min(R, i1 - si);
#pragma unroll
        for (int m = 0; m < SLOTS; ++m) {
            const int row = si + srow[m], rel = row_start(row) + sk * Y3_LB_CHUNK + ssl[m] * 16;
            if (srow[m] < nrows && rel < rb1) stage[buf][tid + 256 * m] = regs[m];
        }
    };

    int i = i0, k = 0, cur = 0;
    load_stage(i, k);
    store_stage(i, k, 0);
    __syncthreads();
    float hacc = 0.f;
    while (i < i1) {
        const int nrows = min(R, i1 - i);
        // the stage after this one
        int ni = i + nrows, nk = 0;
        if (!multi && row_start(i) + (k + 1) * Y3_LB_CHUNK < rb1) {
            ni = i;
            nk = k + 1;
        }
        const bool more = ni < i1;
        if (more) load_stage(ni, nk);
        for (int rr = 0; rr < nrows; ++rr) {
            const int row = i + rr;
            // the taps of this thread's element that lie in this part of the row (element j * PX + ch * SZ in [cb0, cb1)), ascending
            const int cb0 = row_start(row) + k * Y3_LB_CHUNK, cb1 = cb0 + (multi ? span16 : Y3_LB_CHUNK);
            if (active) {
                const T* l = (const T*)((const unsigned char*)stage[cur] + rr * row_lds) + (ch * SZ - cb0) / SZ;  // element of pixel j at l[j * C]
                const int ja = max(jlo, (max(cb0 - ch * SZ, 0) + PX - 1) / PX), jb = min(jhi, (cb1 - ch * SZ + PX - 1) / PX);
                // the weight in fp32: den - |num| of integers below 2^24, every step exact (no tap here: ja >= jb, nothing is formed)
                float numf = ja < jb ? (float)(num0 + 2 * ax.b * (ja - jlo)) : 0.f;
                int j = ja;
                if (j == jlo && j < jb) {  // the first product starts the sum
                    hacc = (denf - fabsf(numf)) * (float)l[j * C];
                    numf += stepf;
                    ++j;
                }
#pragma unroll 4
                for (; j < jb; ++j, numf += stepf) hacc += (denf - fabsf(numf)) * (float)l[j * C];
            }
            if (ni != i) {
                // the row is complete: normalise, then accumulate it into the output rows of the band it reaches
                const float hn = hacc / wsum_xf;
#pragma unroll
                for (int r = 0; r < Y3_LB_ROWS; ++r) {
                    const int o = o0 + r;
                    if (o >= o1) continue;
                    const int wy = lb_weight(ay, lb_num(ay, o, row));  // uniform over the workgroup
                    if (wy == 0) continue;
                    const float p = (float)wy * hn;
                    acc[r] = vsum[r] ? acc[r] + p : p;
                    vsum[r] += wy;
                }
            }
        }
        if (more) store_stage(ni, nk, cur ^ 1);
        __syncthreads();
        cur ^= 1;
        i = ni;
        k = nk;
    }
    if (!active) return;
    float* dst = out + ((size_t)blockIdx.z * C + ch) * H * W + (size_t)(I.pad_y + o0) * W + I.pad_x + x;
#pragma unroll
    for (int r = 0; r < Y3_LB_ROWS; ++r)
        if (o0 + r < o1) dst[(size_t)r * W] = acc[r] / (float)vsum[r];
}

// the frame outside the content
__global__ __launch_bounds__(256) void letterbox_fill_kernel(const LbBatch B, int C, int H, int W, float fill, float* __restrict__ out) {
    const LbImage& I = B.im[blockIdx.z];
    const int y = blockIdx.y;
    const bool row_in = y >= I.pad_y && y < I.pad_y + I.ay.out;
    for (int x = blockIdx.x * 256 + threadIdx.x; x < W; x += gridDim.x * 256) {
        if (row_in && x >= I.pad_x && x < I.pad_x + I.ax.out) continue;
        for (int c = 0; c < C; ++c) out[(((size_t)blockIdx.z * C + c) * H + y) * W + x] = fill;
    }
}

// sum and sum of squares of the content of every frame, in fp64: the content as a [c][new_h][new_w] tensor in the partition and
// tree of zscore_partial_kernel (pointwise.hip), so that a content which fills the frame gives the partials of y3_zscore
__global__ __launch_bounds__(256) void letterbox_stats_kernel(const float* __restrict__ frames, const LbBatch B, int C, int H, int W,
                                                              double* __restrict__ ws) {
    __shared__ double sm[2][256];
    const int img = blockIdx.y;
    const LbImage& I = B.im[img];
    const unsigned nw = (unsigned)I.ax.out, plane = (unsigned)I.ay.out * nw, count = plane * (unsigned)C;
    const float* f = frames + (size_t)img * C * H * W;
    double s = 0.0, q = 0.0;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += (unsigned)Y3_LB_ZS_BLOCKS * 256u) {
        const unsigned c = i / plane, r = i - c * plane;
        const unsigned y = r / nw, x = r - y * nw;
        const double v = (double)f[((size_t)c * H + I.pad_y + y) * W + I.pad_x + x];
        s += v;
        q += v * v;
    }
    sm[0][threadIdx.x] = s;
    sm[1][threadIdx.x] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            sm[0][threadIdx.x] += sm[0][threadIdx.x + o];
            sm[1][threadIdx.x] += sm[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ws[((size_t)img * Y3_LB_ZS_BLOCKS + blockIdx.x) * 2 + 0] = sm[0][0];
        ws[((size_t)img * Y3_LB_ZS_BLOCKS + blockIdx.x) * 2 + 1] = sm[1][0];
    }
}
// {mean, std} of every image: the expressions of tile_stats_finalize_kernel / zscore_apply_kernel, the partials in their order
__global__ void letterbox_finalize_kernel(const double* __restrict__ ws, const LbBatch B, int n, int C, float* __restrict__ mvsd) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= n) return;
    double s = 0.0, q = 0.0;
    for (int b = 0; b < Y3_LB_ZS_BLOCKS; ++b) {
        s += ws[((size_t)img * Y3_LB_ZS_BLOCKS + b) * 2 + 0];
        q += ws[((size_t)img * Y3_LB_ZS_BLOCKS + b) * 2 + 1];
    }
    const double count = (double)C * (double)B.im[img].ay.out * (double)B.im[img].ax.out;
    const double mean = s / count;
    double var = q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    mvsd[2 * img] = (float)mean;
    mvsd[2 * img + 1] = (float)sqrt(var);
}
// One thread per frame pixel: the content normalised, the padding and the spare channels zero, whole 16-byte pixels stored.
__global__ __launch_bounds__(256) void letterbox_apply_kernel(const float* __restrict__ frames, const LbBatch B, int C, int H, int W,
                                                              const float* __restrict__ mvsd, float* __restrict__ dst, int dC, int ld) {
    const int img = blockIdx.z, y = blockIdx.y;
    const LbImage& I = B.im[img];
    const float mv = mvsd[2 * img], sd = mvsd[2 * img + 1];
    const bool divide = !(sd <= 1.0f);
    const bool row_in = y >= I.pad_y && y < I.pad_y + I.ay.out;
    const float* f = frames + ((size_t)img * C * H + y) * W;
    float* d = dst + ((size_t)img * H + y) * W * ld;
    for (int x = blockIdx.x * 256 + threadIdx.x; x < W; x += gridDim.x * 256) {
        const bool in = row_in && x >= I.pad_x && x < I.pad_x + I.ax.out;
        for (int c0 = 0; c0 < dC; c0 += 4) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (in) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c0 + c < C) {
                        const float t = f[(size_t)(c0 + c) * H * W + x] - mv;
                        v[c] = divide ? t / sd : t;
                    }
            }
            *reinterpret_cast<float4*>(d + (size_t)x * ld + c0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// Validates a call's records on the host and turns them into kernel arguments.  frame: H, W > 0 for the two image calls (the
// content must lie inside), 0 for the unmap (which knows no frame).
static int lb_check(const char* what, int n, const y3_letterbox_record* rec, int H, int W, bool image, LbBatch* B, int* max_h, int* max_w) {
    Y3_CHECK_ARG(n >= 1 && n <= Y3_LETTERBOX_MAX_IMAGES, "%s: %d images (1 .. %d per call)", what, n, Y3_LETTERBOX_MAX_IMAGES);
    Y3_CHECK_ARG(rec, "%s: null pointer", what);
    *max_h = *max_w = 0;
    for (int i = 0; i < n; ++i) {
        const y3_letterbox_record& r = rec[i];
        Y3_CHECK_ARG(r.src_h >= 1 && r.src_w >= 1 && r.src_h <= Y3_LB_MAX_SIDE && r.src_w <= Y3_LB_MAX_SIDE,
                     "%s: record %d: source %d x %d (sides 1 .. %d)", what, i, r.src_h, r.src_w, Y3_LB_MAX_SIDE);
        Y3_CHECK_ARG(r.new_h >= 1 && r.new_w >= 1 && r.new_h <= Y3_LB_MAX_SIDE && r.new_w <= Y3_LB_MAX_SIDE,
                     "%s: record %d: content %d x %d (sides 1 .. %d)", what, i, r.new_h, r.new_w, Y3_LB_MAX_SIDE);
        Y3_CHECK_ARG(r.pad_y >= 0 && r.pad_x >= 0 && r.pad_y <= Y3_LB_MAX_SIDE && r.pad_x <= Y3_LB_MAX_SIDE, "%s: record %d: padding %d, %d",
                     what, i, r.pad_y, r.pad_x);
        if (image) {
            Y3_CHECK_ARG(r.pad_y + r.new_h <= H && r.pad_x + r.new_w <= W,
                         "%s: record %d: content %d x %d at (%d, %d) does not fit the %d x %d frame", what, i, r.new_h, r.new_w, r.pad_y, r.pad_x, H,
                         W);
            Y3_CHECK_ARG((r.src_offset & 15) == 0, "%s: record %d: source offset %llu is no multiple of 16", what, i,
                         (unsigned long long)r.src_offset);
            Y3_CHECK_ARG((long long)r.src_h <= (long long)Y3_LB_MAX_SCALE * r.new_h && (long long)r.src_w <= (long long)Y3_LB_MAX_SCALE * r.new_w,
                         "%s: record %d: %d x %d -> %d x %d reduces an axis by more than %d", what, i, r.src_h, r.src_w, r.new_h, r.new_w,
                         Y3_LB_MAX_SCALE);
        }
        LbImage& I = B->im[i];
        I.off = r.src_offset;
        I.pad_y = r.pad_y;
        I.pad_x = r.pad_x;
        I.sy = (float)((double)r.src_h / (double)r.new_h);
        I.sx = (float)((double)r.src_w / (double)r.new_w);
        I.ay = lb_axis(r.src_h, r.new_h);
        I.ax = lb_axis(r.src_w, r.new_w);
        if (r.new_h > *max_h) *max_h = r.new_h;
        if (r.new_w > *max_w) *max_w = r.new_w;
    }
    for (int i = n; i < Y3_LETTERBOX_MAX_IMAGES; ++i) B->im[i] = B->im[0];
    return Y3_OK;
}
static int lb_check_source(const char* what, const void* src, int dtype, int c, int H, int W) {
    Y3_CHECK_ARG(src, "%s: null pointer", what);
    Y3_CHECK_ARG(dtype >= 0 && dtype <= 2, "%s: dtype %d (0 = u8, 1 = u16, 2 = f32)", what, dtype);
    Y3_CHECK_ARG(c == 1 || c == 3, "%s: %d channels (1 or 3)", what, c);
    Y3_CHECK_ARG(H >= 1 && W >= 1 && H <= Y3_LB_MAX_SIDE && W <= Y3_LB_MAX_SIDE, "%s: frame %d x %d (sides 1 .. %d)", what, H, W, Y3_LB_MAX_SIDE);
    Y3_CHECK_ARG(((uintptr_t)src & 15) == 0, "%s: the source buffer must be 16-byte aligned", what);
    return Y3_OK;
}

static void lb_launch_resample(const void* src, int dtype, int c, int n, const LbBatch& B, int max_h, int max_w, int H, int W, float* out,
                               hipStream_t st) {
    const dim3 grid(y3_cdiv((long long)max_w * c, Y3_LB_COLS), y3_cdiv(max_h, Y3_LB_ROWS), n), block(256);
    const unsigned char* s = (const unsigned char*)src;
#define Y3_LB_LAUNCH(T, C) hipLaunchKernelGGL((letterbox_resample_kernel<T, C>), grid, block, 0, st, s, B, out, H, W)
    if (c == 1) {
        if (dtype == 0) Y3_LB_LAUNCH(unsigned char, 1);
        else if (dtype == 1) Y3_LB_LAUNCH(unsigned short, 1);
        else Y3_LB_LAUNCH(float, 1);
    } else {
        if (dtype == 0) Y3_LB_LAUNCH(unsigned char, 3);
        else if (dtype == 1) Y3_LB_LAUNCH(unsigned short, 3);
        else Y3_LB_LAUNCH(float, 3);
    }
#undef Y3_LB_LAUNCH
}

extern "C" int y3_letterbox_batch(const void* src, int dtype, int c, int n, const y3_letterbox_record* records, int H, int W, float fill,
                                  float* out, y3_stream_t stream) {
    if (int e = lb_check_source("letterbox_batch", src, dtype, c, H, W)) return e;
    Y3_CHECK_ARG(out, "letterbox_batch: null pointer");
    LbBatch B;
    int max_h, max_w;
    if (int e = lb_check("letterbox_batch", n, records, H, W, true, &B, &max_h, &max_w)) return e;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(letterbox_fill_kernel, dim3(y3_cdiv(W, 256), H, n), dim3(256), 0, st, B, c, H, W, fill, out);
    Y3_CHECK_LAUNCH("letterbox_batch (fill)");
    lb_launch_resample(src, dtype, c, n, B, max_h, max_w, H, W, out, st);
    Y3_CHECK_LAUNCH("letterbox_batch");
    return Y3_OK;
}

// workspace: [n][128][2] fp64 partials, [n][2] floats {mean, std} (padded to 16 bytes), [n][c][H][W] floats of un-normalised frames
static size_t lb_stats_bytes(int n) { return (size_t)n * Y3_LB_ZS_BLOCKS * 2 * sizeof(double) + (((size_t)n * 2 * sizeof(float) + 15) & ~(size_t)15); }
extern "C" size_t y3_letterbox_workspace_bytes(int n, int H, int W, int c) {
    if (n < 1 || H < 1 || W < 1 || c < 1) return 0;
    return lb_stats_bytes(n) + (size_t)n * c * H * W * sizeof(float);
}

extern "C" int y3_letterbox_zscore_nhwc(const void* src, int dtype, int c, int n, const y3_letterbox_record* records, const y3_tensor* dst,
                                        void* workspace, y3_stream_t stream) {
    Y3_CHECK_ARG(dst && dst->ptr && workspace, "letterbox_zscore_nhwc: null pointer");
    const int H = dst->h, W = dst->w;
    if (int e = lb_check_source("letterbox_zscore_nhwc", src, dtype, c, H, W)) return e;
    LbBatch B;
    int max_h, max_w;
    if (int e = lb_check("letterbox_zscore_nhwc", n, records, H, W, true, &B, &max_h, &max_w)) return e;
    Y3_CHECK_ARG(dst->n == n, "letterbox_zscore_nhwc: destination of %d images, expected %d", dst->n, n);
    Y3_CHECK_ARG(dst->c >= c && (dst->c & 3) == 0 && dst->ld >= dst->c && (dst->ld & 3) == 0 && ((uintptr_t)dst->ptr & 15) == 0,
                 "letterbox_zscore_nhwc: destination needs at least the source's %d channels, c and ld multiples of 4 and 16-byte alignment (c %d, "
                 "ld %d)",
                 c, dst->c, dst->ld);
    Y3_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "letterbox_zscore_nhwc: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    float* mvsd = (float*)(ws + (size_t)n * Y3_LB_ZS_BLOCKS * 2);
    float* frames = (float*)((char*)workspace + lb_stats_bytes(n));
    lb_launch_resample(src, dtype, c, n, B, max_h, max_w, H, W, frames, st);
    Y3_CHECK_LAUNCH("letterbox_zscore_nhwc (resample)");
    hipLaunchKernelGGL(letterbox_stats_kernel, dim3(Y3_LB_ZS_BLOCKS, n), dim3(256), 0, st, (const float*)frames, B, c, H, W, ws);
    Y3_CHECK_LAUNCH("letterbox_zscore_nhwc (statistics)");
    hipLaunchKernelGGL(letterbox_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, B, n, c, mvsd);
    Y3_CHECK_LAUNCH("letterbox_zscore_nhwc (finalize)");
    hipLaunchKernelGGL(letterbox_apply_kernel, dim3(y3_cdiv(W, 256), H, n), dim3(256), 0, st, (const float*)frames, B, c, H, W, (const float*)mvsd,
                       (float*)dst->ptr, dst->c, dst->ld);
    Y3_CHECK_LAUNCH("letterbox_zscore_nhwc (apply)");
    return Y3_OK;
}

// One thread per decode row: out of the frame, into the image.  One fp32 subtraction and one fp32 multiplication per value.
__global__ __launch_bounds__(256) void letterbox_unmap_kernel(float* __restrict__ rows, long long total, int nb, int ld, int clip, const LbBatch B) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const LbImage& I = B.im[(int)(i / nb)];
    const float px = (float)I.pad_x, py = (float)I.pad_y, w = (float)I.ax.in, h = (float)I.ay.in;
    float* r = rows + i * ld;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool isx = !(q & 1);
        float v = (r[q] - (isx ? px : py)) * (isx ? I.sx : I.sy);
        if (clip) {
            const float lim = isx ? w : h;
            v = v < 0.f ? 0.f : (v > lim ? lim : v);
        }
        r[q] = v;
    }
}

extern "C" int y3_letterbox_unmap(float* rows, int n, int nb, int ld, const y3_letterbox_record* records, int clip, y3_stream_t stream) {
    Y3_CHECK_ARG(rows, "letterbox_unmap: null pointer");
    Y3_CHECK_ARG(nb >= 1 && ld >= 4, "letterbox_unmap: bad sizes (nb %d, ld %d)", nb, ld);
    Y3_CHECK_ARG(clip == 0 || clip == 1, "letterbox_unmap: clip %d (0 or 1)", clip);
    LbBatch B;
    int max_h, max_w;
    if (int e = lb_check("letterbox_unmap", n, records, 0, 0, false, &B, &max_h, &max_w)) return e;
    const long long total = (long long)n * nb;
    Y3_CHECK_ARG(total < (1LL << 31), "letterbox_unmap: %lld rows (fewer than 2^31)", total);
    hipLaunchKernelGGL(letterbox_unmap_kernel, dim3(y3_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, rows, total, nb, ld, clip, B);
    Y3_CHECK_LAUNCH("letterbox_unmap");
    return Y3_OK;
}
