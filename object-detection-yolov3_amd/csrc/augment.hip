// Training augmentation on the device (augment.py:30-125, 275-297; imagereader.py:369-391): bilinear rescale + crop + flips,
// Gaussian noise scaled by the crop's range, 3-axis Gaussian blur, HWC -> CHW float32.  The random decisions are drawn on
// the host (yolo3/augment.py draw_augmentation) and arrive as one y3_aug_record per image; semantics in yolo3hip.h.
//
// Passes (one launch each per chunk of up to Y3_AUG_CHUNK images):
//   aug_resample  one workgroup per output row: the two source rows the row interpolates between are staged in LDS with
//                 4-byte loads, every output column is two LDS lookups per row; writes CHW float32 into `out` and folds the
//                 row's min / max into two order-preserving words per image (atomicMax).
//   aug_row       only for images with noise or blur: one workgroup per (row, 256-column segment).  Loads the segment and its
//                 reflect halo, adds the noise on the load (the halo gets the same counter-based draws as the element it
//                 mirrors), filters along W and mixes the channels with the folded C x C matrix.  Without blur it writes
//                 back in place, with blur into the workspace.
//   aug_col       only for images with blur: 64-column x 32-row tiles with a row halo in LDS, filter along H -> `out`.
//
// Mosaic (not in the reference; y3_mosaic_batch, semantics in yolo3hip.h): a second, separate pass that recombines
// the augmented batch, four windows of four images per output image.
//   mosaic        one thread per 16-byte-aligned group of four destination floats of one (image, channel) plane.  A group that
//                 lies inside one span (one row, one side of the seam column) is one 16-byte load at 4-byte alignment -- the
//                 source is shifted against the destination by ox - qx, any residue mod 4 -- and one aligned 16-byte store; the
//                 at most three groups a row has at its seam and its ends copy their floats one by one.
//
// Affine warp (not in the reference; y3_affine_batch, semantics in yolo3hip.h): a third, separate pass that resamples
// every image of the batch through its own inverse affine map.
//   affine        one thread per output pixel and all its channels, 32 x 32 pixels per workgroup: fp32 coordinates in a stated
//                 unfused order, four taps gathered straight from global memory (the two of a row as one 8-byte load in the
//                 interior), `fill` outside the image, taps of weight zero never read.
//
// Colour / tone jitter and MixUp (not in the reference; y3_photometric_batch, semantics in yolo3hip.h): a fourth,
// separate pass, elementwise over the batch.
//   photometric   one thread per 16-byte-aligned group of four pixels and all their channel planes (planes of a multiple of four
//                 elements; one pixel per thread otherwise): colour matrix with scalar branches on the record's zeros, clamp,
//                 tone curve as exp2(gamma * log2(t / white)) only for images whose record asks for it, and the blend with the
//                 partner image evaluated under the partner's own record.  Streaming: each source element is read once (twice
//                 for a mixed image) with 16-byte loads at 4-byte alignment, each output element stored once, aligned.
#include "common.h"
#include <math.h>
#include <algorithm>

#define Y3_AUG_CHUNK 32        // images per launch: the per-image table travels as a kernel argument (32 x 48 B)
#define Y3_AUG_MAX_RADIUS 8    // int(4 sigma + 0.5) <= 8, i.e. sigma < 2.125 (the reader draws |sigma| <= 2)
#define Y3_AUG_STAGE_BYTES 61440   // dynamic LDS for the two staged source rows (+ static scratch < 64 KiB)

struct AugImg {                // 48 bytes
    int rows, cols, dy, dx;
    int flags;                 // 1 = reflect_x, 2 = reflect_y
    int radius;                // blur radius, 0 = no blur
    float sigma;               // blur sigma (radius > 0)
    float noise;               // severity * (2 u_noise - 1): noise sigma = noise * (max - min); 0 = no noise
    unsigned seed_lo, seed_hi;
    int pad0, pad1;
};
struct AugTable {
    AugImg img[Y3_AUG_CHUNK];
};

// order-preserving float <-> uint (x < y <=> enc(x) < enc(y)); 0 is below every encoded value, so a zeroed word is "empty"
__device__ __forceinline__ unsigned aug_enc(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float aug_dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// scipy mode='mirror' (= numpy 'reflect'): whole-sample symmetric, period 2(n-1), no edge repeat
__device__ __forceinline__ int aug_mirror(int p, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int q = p % period;
    if (q < 0) q += period;
    return q < n ? q : period - q;
}
// scipy mode='reflect' (= numpy 'symmetric'): half-sample symmetric, period 2n, the edge repeats
__device__ __forceinline__ int aug_reflect(int p, int n) {
    const int period = 2 * n;
    int q = p % period;
    if (q < 0) q += period;
    return q < n ? q : period - 1 - q;
}

// Source coordinate of rescaled index o: ((2o + 1) n_in - n_res) / (2 n_res), as an exact integer floor i0 and the fraction
// of the remainder (numerator < 2^31 is checked on the host)
__device__ __forceinline__ void aug_coord(int o, int n_in, int n_res, int& i0, float& f) {
    const int num = (2 * o + 1) * n_in - n_res, den = 2 * n_res;
    i0 = num >= 0 ? num / den : -((den - 1 - num) / den);
    f = (float)(num - i0 * den) / (float)den;
}

__device__ __forceinline__ float aug_lerp(float a, float b, float f) { return f == 0.f ? a : (1.f - f) * a + f * b; }

// Philox4x32-10 (Salmon et al., SC'11): counter (e, 0, 0, 0), key (seed_lo, seed_hi); Box-Muller on the first two words
__device__ __forceinline__ float aug_normal(unsigned e, unsigned k0, unsigned k1) {
    unsigned c0 = e, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const float u1 = (float)((c0 >> 8) + 1u) * 5.9604644775390625e-8f;    // (0, 1]
    const float u2 = (float)(c1 >> 8) * 5.9604644775390625e-8f;           // [0, 1)
    return sqrtf(-2.f * logf(u1)) * cosf(6.2831853071795865f * u2);
}

// Normalised Gaussian weights w[0..radius] (scipy _gaussian_kernel1d: exp(-x^2 / 2 sigma^2) / sum over -r..r, in double) and,
// when mix != nullptr, the C x C channel matrix of the same 1-D filter folded through mode='reflect' on an axis of length C.
// Called by the whole workgroup (two barriers).
__device__ void aug_weights(const AugImg& a, float* wgt, float* mix, int C) {
    __shared__ double phi[Y3_AUG_MAX_RADIUS + 1];
    const int r = a.radius;
    if ((int)threadIdx.x <= r) {
        const double s = (double)a.sigma, x = (double)threadIdx.x;
        phi[threadIdx.x] = exp(-0.5 / (s * s) * x * x);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = phi[0];
        for (int k = 1; k <= r; ++k) sum += 2.0 * phi[k];
        double w[Y3_AUG_MAX_RADIUS + 1];
        for (int k = 0; k <= r; ++k) {
            w[k] = phi[k] / sum;
            wgt[k] = (float)w[k];
        }
        if (mix)
            for (int co = 0; co < C; ++co) {
                double m[3] = {0.0, 0.0, 0.0};
                for (int k = -r; k <= r; ++k) m[aug_reflect(co + k, C)] += w[k < 0 ? -k : k];
                for (int ci = 0; ci < C; ++ci) mix[co * C + ci] = (float)m[ci];
            }
    }
    __syncthreads();
}

// ---- pass 1: resample + crop + flips -> CHW, per-image min / max ---------------------------------------------------------
template <typename T>
__device__ __forceinline__ void aug_stage_row(const T* __restrict__ src, int elems, unsigned char* dst) {
    const unsigned char* s = (const unsigned char*)src;
    const int bytes = elems * (int)sizeof(T);
    if ((((size_t)s) & 3) == 0 && (bytes & 3) == 0) {
        const unsigned* s4 = (const unsigned*)s;
        unsigned* d4 = (unsigned*)dst;
        for (int i = threadIdx.x; i < (bytes >> 2); i += blockDim.x) d4[i] = s4[i];
    } else {
        T* d = (T*)dst;
        for (int i = threadIdx.x; i < elems; i += blockDim.x) d[i] = src[i];
    }
}

template <typename T, int C>
__global__ __launch_bounds__(256) void aug_resample_kernel(const T* __restrict__ src, int Hin, int Win, AugTable tab, int Hout, int Wout,
                                                           float* __restrict__ out, unsigned* __restrict__ minmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    __shared__ float red[2][4];
    const AugImg& a = tab.img[blockIdx.y];
    const int r = blockIdx.x;
    const int rr = (a.flags & 2) ? Hout - 1 - r : r;
    int y0;
    float fy;
    aug_coord(rr + a.dy, Hin, a.rows, y0, fy);
    const int ya = aug_mirror(y0, Hin), yb = fy == 0.f ? ya : aug_mirror(y0 + 1, Hin);
    const int rowElems = Win * C;
    const T* img = src + (size_t)blockIdx.y * Hin * rowElems;
    const size_t rowBytes = ((size_t)rowElems * sizeof(T) + 15) & ~(size_t)15;
    const T* la = (const T*)stage;
    const T* lb = (const T*)(stage + rowBytes);
    aug_stage_row(img + (size_t)ya * rowElems, rowElems, stage);
    if (yb != ya) aug_stage_row(img + (size_t)yb * rowElems, rowElems, stage + rowBytes);
    else lb = la;
    __syncthreads();
    const size_t plane = (size_t)Hout * Wout;
    float* o = out + (size_t)blockIdx.y * C * plane + (size_t)r * Wout;
    float lo = INFINITY, hi = -INFINITY;
    for (int c = threadIdx.x; c < Wout; c += blockDim.x) {
        const int cc = (a.flags & 1) ? Wout - 1 - c : c;
        int x0;
        float fx;
        aug_coord(cc + a.dx, Win, a.cols, x0, fx);
        const int xa = aug_mirror(x0, Win) * C, xb = (fx == 0.f ? aug_mirror(x0, Win) : aug_mirror(x0 + 1, Win)) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const float top = aug_lerp((float)la[xa + ch], (float)la[xb + ch], fx);
            const float bot = aug_lerp((float)lb[xa + ch], (float)lb[xb + ch], fx);
            const float v = aug_lerp(top, bot, fy);
            o[ch * plane + c] = v;
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, s));
        hi = fmaxf(hi, __shfl_xor(hi, s));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            lo = fminf(lo, red[0][w]);
            hi = fmaxf(hi, red[1][w]);
        }
        atomicMax(minmax + 2 * blockIdx.y, aug_enc(hi));
        atomicMax(minmax + 2 * blockIdx.y + 1, aug_enc(-lo));
    }
}

// ---- pass 2: noise + blur along W + channel mix ---------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void aug_row_kernel(float* __restrict__ io, float* __restrict__ tmp, AugTable tab, int Hout, int Wout, int nseg,
                                                      const unsigned* __restrict__ minmax) {
    __shared__ float row[C][256 + 2 * Y3_AUG_MAX_RADIUS];
    __shared__ float wgt[Y3_AUG_MAX_RADIUS + 1];
    __shared__ float mix[C * C];
    const AugImg& a = tab.img[blockIdx.y];
    if (a.noise == 0.f && a.radius == 0) return;
    const int R = a.radius;
    if (R > 0) aug_weights(a, wgt, C > 1 ? mix : nullptr, C);
    const int h = blockIdx.x / nseg, x0 = (blockIdx.x - h * nseg) * 256;
    const size_t plane = (size_t)Hout * Wout;
    const float* s = io + (size_t)blockIdx.y * C * plane + (size_t)h * Wout;
    const float sig = a.noise * (aug_dec(minmax[2 * blockIdx.y]) + aug_dec(minmax[2 * blockIdx.y + 1]));   // noise * (max - min)
    const bool noisy = a.noise != 0.f;
    const int span = min(256, Wout - x0) + 2 * R;
    for (int ch = 0; ch < C; ++ch)
        for (int i = threadIdx.x; i < span; i += blockDim.x) {
            const int x = aug_reflect(x0 - R + i, Wout);
            float v = s[ch * plane + x];
            if (noisy) v += sig * aug_normal((unsigned)(((size_t)ch * Hout + h) * Wout + x), a.seed_lo, a.seed_hi);
            row[ch][i] = v;
        }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= Wout) return;
    float b[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const float* p = &row[ch][threadIdx.x + R];
        if (R == 0) {
            b[ch] = p[0];
        } else {
            float acc = wgt[0] * p[0];
            for (int k = 1; k <= R; ++k) acc += wgt[k] * (p[-k] + p[k]);      // scipy correlate1d's symmetric form
            b[ch] = acc;
        }
    }
    float* d = (R > 0 ? tmp : io) + (size_t)blockIdx.y * C * plane + (size_t)h * Wout + x;
#pragma unroll
    for (int co = 0; co < C; ++co) {
        float v = b[co];
        if (C > 1 && R > 0) {
            v = 0.f;
#pragma unroll
            for (int ci = 0; ci < C; ++ci) v += mix[co * C + ci] * b[ci];
        }
        d[co * plane] = v;
    }
}

// ---- pass 3: blur along H --------------------------------------------------------------------------------------------------
#define AUG_COL_TW 64
#define AUG_COL_TH 32
__global__ __launch_bounds__(256) void aug_col_kernel(const float* __restrict__ tmp, float* __restrict__ out, AugTable tab, int C, int Hout, int Wout,
                                                      int tilesx, int tilesy) {
    __shared__ float col[AUG_COL_TH + 2 * Y3_AUG_MAX_RADIUS][AUG_COL_TW];
    __shared__ float wgt[Y3_AUG_MAX_RADIUS + 1];
    const AugImg& a = tab.img[blockIdx.y];
    if (a.radius == 0) return;
    const int R = a.radius;
    aug_weights(a, wgt, nullptr, C);
    const int t = blockIdx.x, tx = t % tilesx, ty = (t / tilesx) % tilesy, ch = t / (tilesx * tilesy);
    const int lane = threadIdx.x & (AUG_COL_TW - 1), grp = threadIdx.x / AUG_COL_TW;
    const int x = tx * AUG_COL_TW + lane, y0 = ty * AUG_COL_TH;
    const size_t plane = (size_t)Hout * Wout;
    const float* s = tmp + ((size_t)blockIdx.y * C + ch) * plane;
    const int rowsIn = min(AUG_COL_TH, Hout - y0) + 2 * R;
    for (int i = grp; i < rowsIn; i += 256 / AUG_COL_TW) col[i][lane] = x < Wout ? s[(size_t)aug_reflect(y0 - R + i, Hout) * Wout + x] : 0.f;
    __syncthreads();
    if (x >= Wout) return;
    float* d = out + ((size_t)blockIdx.y * C + ch) * plane + x;
    for (int i = grp; i < AUG_COL_TH && y0 + i < Hout; i += 256 / AUG_COL_TW) {
        float acc = wgt[0] * col[i + R][lane];
        for (int k = 1; k <= R; ++k) acc += wgt[k] * (col[i + R - k][lane] + col[i + R + k][lane]);
        d[(size_t)(y0 + i) * Wout] = acc;
    }
}

// ---- host entry ------------------------------------------------------------------------------------------------------------
static size_t aug_minmax_bytes(int n) { return ((size_t)n * 2 * sizeof(unsigned) + 255) & ~(size_t)255; }

extern "C" size_t y3_augment_workspace_bytes(int n, int h_out, int w_out, int c) {
    if (n <= 0 || h_out <= 0 || w_out <= 0 || c <= 0) return 0;
    return aug_minmax_bytes(n) + (size_t)n * c * h_out * w_out * sizeof(float);
}

static int aug_blur_radius(float sigma) { return sigma > 0.f ? (int)(4.0 * (double)sigma + 0.5) : 0; }

template <typename T, int C>
static void aug_launch_resample(const void* src, int h_in, int w_in, const AugTable& tab, int nb, int h_out, int w_out, float* out,
                                unsigned* mm, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((aug_resample_kernel<T, C>), dim3(h_out, nb), dim3(256), lds, st, (const T*)src, h_in, w_in, tab, h_out, w_out, out, mm);
}

extern "C" int y3_augment_batch(const void* src, int dtype, int n, int h_in, int w_in, int c, const y3_aug_record* records, int h_out,
                                int w_out, float* out, void* workspace, y3_stream_t stream) {
    Y3_CHECK_ARG(src && records && out && workspace, "augment_batch: null pointer");
    Y3_CHECK_ARG(dtype >= 0 && dtype <= 2, "augment_batch: dtype %d (0 = u8, 1 = u16, 2 = f32)", dtype);
    Y3_CHECK_ARG(c == 1 || c == 3, "augment_batch: channels %d (1 or 3)", c);
    Y3_CHECK_ARG(n > 0 && h_in > 0 && w_in > 0 && h_out > 0 && w_out > 0, "augment_batch: bad dims n %d in %dx%d out %dx%d", n, h_in, w_in, h_out, w_out);
    Y3_CHECK_ARG((long long)h_out * w_out * c < (1LL << 31) && h_out <= 65535, "augment_batch: output %dx%dx%d too large", h_out, w_out, c);
    const size_t esize = dtype == 0 ? 1 : dtype == 1 ? 2 : 4;
    const size_t rowBytes = ((size_t)w_in * c * esize + 15) & ~(size_t)15;
    Y3_CHECK_ARG(2 * rowBytes <= Y3_AUG_STAGE_BYTES, "augment_batch: source rows of %d x %d x %zu bytes exceed the LDS row stage", w_in, c, esize);
    for (int i = 0; i < n; ++i) {
        const y3_aug_record& r = records[i];
        Y3_CHECK_ARG(r.src_h == h_in && r.src_w == w_in, "augment_batch: record %d: source %dx%d, batch %dx%d", i, r.src_h, r.src_w, h_in, w_in);
        Y3_CHECK_ARG(r.rows >= 1 && r.cols >= 1, "augment_batch: record %d: rescaled size %dx%d", i, r.rows, r.cols);
        Y3_CHECK_ARG((long long)2 * r.rows * h_in < (1LL << 31) && (long long)2 * r.cols * w_in < (1LL << 31), "augment_batch: record %d: rescaled size %dx%d too large",
                     i, r.rows, r.cols);
        Y3_CHECK_ARG(r.dy >= 0 && r.dx >= 0 && (long long)r.dy + h_out <= r.rows && (long long)r.dx + w_out <= r.cols,
                     "augment_batch: record %d: crop %d+%d x %d+%d outside the rescaled %dx%d", i, r.dy, h_out, r.dx, w_out, r.rows, r.cols);
        Y3_CHECK_ARG((r.reflect_x == 0 || r.reflect_x == 1) && (r.reflect_y == 0 || r.reflect_y == 1), "augment_batch: record %d: reflect flags %d %d", i,
                     r.reflect_x, r.reflect_y);
        Y3_CHECK_ARG(isfinite(r.noise_severity) && r.noise_severity >= 0.f && isfinite(r.u_noise) && r.u_noise >= 0.f && r.u_noise <= 1.f,
                     "augment_batch: record %d: noise severity %g, u_noise %g", i, (double)r.noise_severity, (double)r.u_noise);
        Y3_CHECK_ARG(isfinite(r.blur_sigma) && aug_blur_radius(r.blur_sigma) <= Y3_AUG_MAX_RADIUS, "augment_batch: record %d: blur sigma %g (radius <= %d)", i,
                     (double)r.blur_sigma, Y3_AUG_MAX_RADIUS);
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned* mm = (unsigned*)workspace;
    float* tmp = (float*)((char*)workspace + aug_minmax_bytes(n));
    const hipError_t e = hipMemsetAsync(mm, 0, (size_t)n * 2 * sizeof(unsigned), st);
    if (e != hipSuccess) {
        y3_set_error("augment_batch: memset: %s", hipGetErrorString(e));
        return Y3_ELAUNCH;
    }
    const size_t plane = (size_t)h_out * w_out;
    for (int base = 0; base < n; base += Y3_AUG_CHUNK) {
        const int nb = std::min(Y3_AUG_CHUNK, n - base);
        AugTable tab = {};
        bool any_row = false, any_blur = false;
        for (int i = 0; i < nb; ++i) {
            const y3_aug_record& r = records[base + i];
            AugImg& a = tab.img[i];
            a.rows = r.rows;
            a.cols = r.cols;
            a.dy = r.dy;
            a.dx = r.dx;
            a.flags = (r.reflect_x ? 1 : 0) | (r.reflect_y ? 2 : 0);
            a.radius = aug_blur_radius(r.blur_sigma);
            a.sigma = r.blur_sigma;
            a.noise = (float)((double)r.noise_severity * (2.0 * (double)r.u_noise - 1.0));
            a.seed_lo = (unsigned)(r.seed & 0xffffffffu);
            a.seed_hi = (unsigned)(r.seed >> 32);
            any_row |= a.noise != 0.f || a.radius > 0;
            any_blur |= a.radius > 0;
        }
        const void* s = (const char*)src + (size_t)base * h_in * w_in * c * esize;
        float* o = out + (size_t)base * c * plane;
        float* t = tmp + (size_t)base * c * plane;
        unsigned* m = mm + 2 * base;
        const size_t lds = 2 * rowBytes;
        switch (dtype * 4 + c) {
            case 0 * 4 + 1: aug_launch_resample<unsigned char, 1>(s, h_in, w_in, tab, nb, h_out, w_out, o, m, lds, st); break;
            case 0 * 4 + 3: aug_launch_resample<unsigned char, 3>(s, h_in, w_in, tab, nb, h_out, w_out, o, m, lds, st); break;
            case 1 * 4 + 1: aug_launch_resample<unsigned short, 1>(s, h_in, w_in, tab, nb, h_out, w_out, o, m, lds, st); break;
            case 1 * 4 + 3: aug_launch_resample<unsigned short, 3>(s, h_in, w_in, tab, nb, h_out, w_out, o, m, lds, st); break;
            case 2 * 4 + 1: aug_launch_resample<float, 1>(s, h_in, w_in, tab, nb, h_out, w_out, o, m, lds, st); break;
            default: aug_launch_resample<float, 3>(s, h_in, w_in, tab, nb, h_out, w_out, o, m, lds, st); break;
        }
        Y3_CHECK_LAUNCH("augment_batch: resample");
        if (any_row) {
            const int nseg = y3_cdiv(w_out, 256);
            if (c == 1) hipLaunchKernelGGL(aug_row_kernel<1>, dim3(nseg * h_out, nb), dim3(256), 0, st, o, t, tab, h_out, w_out, nseg, (const unsigned*)m);
            else hipLaunchKernelGGL(aug_row_kernel<3>, dim3(nseg * h_out, nb), dim3(256), 0, st, o, t, tab, h_out, w_out, nseg, (const unsigned*)m);
            Y3_CHECK_LAUNCH("augment_batch: noise / row blur");
        }
        if (any_blur) {
            const int tilesx = y3_cdiv(w_out, AUG_COL_TW), tilesy = y3_cdiv(h_out, AUG_COL_TH);
            hipLaunchKernelGGL(aug_col_kernel, dim3(tilesx * tilesy * c, nb), dim3(256), 0, st, (const float*)t, o, tab, c, h_out, w_out, tilesx, tilesy);
            Y3_CHECK_LAUNCH("augment_batch: column blur");
        }
    }
    return Y3_OK;
}

// ---- mosaic: four windows of four augmented images per output image (not in the reference) ---------------------------------
struct MosImg {                // 48 bytes
    long long delta[4];        // quadrant q: source element = delta[q] + ch * h * w + (y * w + x); src * c * h * w + (oy - qy) * w + ox - qx
    int cy, cx;
    int pad0, pad1;
};
struct MosTable {
    MosImg img[Y3_AUG_CHUNK];
};
typedef float mos_f4 __attribute__((ext_vector_type(4)));
typedef float mos_f4u __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at 4-byte alignment: one global_load_dwordx4

// grid (groups of a plane / 256, c, images of the chunk).  `out` is the chunk's first output image, `src` the whole batch.
// e / W for 0 <= e < 2^31 is (e * div_mul) >> div_shift (Granlund & Montgomery, PLDI'94: l = ceil(log2 W), div_mul =
// floor(2^(31+l) / W) + 1 < 2^32, div_shift = 31 + l), a multiply in place of the division every thread would start with.
__global__ __launch_bounds__(256) void mosaic_kernel(const float* __restrict__ src, float* __restrict__ out, MosTable tab, int C, int H, int W,
                                                     unsigned div_mul, int div_shift) {
    const MosImg& m = tab.img[blockIdx.z];
    const int P = H * W;
    float* o = out + ((size_t)blockIdx.z * C + blockIdx.y) * (size_t)P;
    const float* s = src + (size_t)blockIdx.y * (size_t)P;
    const float *s0 = s + m.delta[0], *s1 = s + m.delta[1], *s2 = s + m.delta[2], *s3 = s + m.delta[3];      // uniform: scalar registers
#define MOS_SRC(row, x) ((row) >= m.cy ? ((x) >= m.cx ? s3 : s2) : ((x) >= m.cx ? s1 : s0))
    const int a = (int)(((size_t)o >> 2) & 3);                     // the plane starts `a` floats into a 16-byte group
    const int e0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4 - a;  // first element of this thread's group, -3 .. P-1
    if (e0 >= P) return;
    const int e = max(e0, 0), end = min(e0 + 4, P);
    int row = (int)(((unsigned long long)(unsigned)e * div_mul) >> div_shift), x = e - row * W;
    const bool whole = e0 >= 0 && e0 + 4 <= P && x + 4 <= W && (x + 4 <= m.cx || x >= m.cx);      // one span: y * w + x = e0 on both sides
    mos_f4 v;
    if (whole) {
        v = *(const mos_f4u*)(MOS_SRC(row, x) + e0);
    } else {                                                        // a row end, the seam, or the plane's first / last group:
#pragma unroll
        for (int k = 0; k < 4; ++k)                                 // its (up to) four loads issued back to back, its stores after them
            if (e0 + k >= e && e0 + k < end) {
                v[k] = MOS_SRC(row, x)[e0 + k];
                if (++x == W) {
                    x = 0;
                    ++row;
                }
            }
    }
    if (whole) {
        *(mos_f4*)(o + e0) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e0 + k >= e && e0 + k < end) o[e0 + k] = v[k];
    }
#undef MOS_SRC
}

extern "C" int y3_mosaic_batch(const float* src, int n, int c, int h, int w, const y3_mosaic_record* records, float* out, y3_stream_t stream) {
    Y3_CHECK_ARG(src && records && out, "mosaic_batch: null pointer");
    Y3_CHECK_ARG(c == 1 || c == 3, "mosaic_batch: channels %d (1 or 3)", c);
    Y3_CHECK_ARG(n > 0 && h > 0 && w > 0, "mosaic_batch: bad dims n %d, %dx%d", n, h, w);
    Y3_CHECK_ARG((long long)h * w < (1LL << 31) - 8, "mosaic_batch: plane %dx%d too large", h, w);
    const size_t plane = (size_t)h * w, image = plane * c, bytes = (size_t)n * image * sizeof(float);
    Y3_CHECK_ARG((((size_t)src | (size_t)out) & 3) == 0, "mosaic_batch: src / out not 4-byte aligned");
    Y3_CHECK_ARG((size_t)src + bytes <= (size_t)out || (size_t)out + bytes <= (size_t)src, "mosaic_batch: src and out overlap (the pass cannot run in place)");
    for (int i = 0; i < n; ++i) {
        const y3_mosaic_record& r = records[i];
        Y3_CHECK_ARG(r.cy >= 0 && r.cy <= h && r.cx >= 0 && r.cx <= w, "mosaic_batch: record %d: seam (%d, %d) outside [0, %d] x [0, %d]", i, r.cy, r.cx, h, w);
        Y3_CHECK_ARG(r.reserved[0] == 0 && r.reserved[1] == 0, "mosaic_batch: record %d: reserved words %d %d", i, r.reserved[0], r.reserved[1]);
        for (int q = 0; q < 4; ++q) {
            const int qh = (q & 2) ? h - r.cy : r.cy, qw = (q & 1) ? w - r.cx : r.cx;
            if (qh == 0 || qw == 0) continue;
            Y3_CHECK_ARG(r.src[q] >= 0 && r.src[q] < n, "mosaic_batch: record %d: quadrant %d: source image %d of %d", i, q, r.src[q], n);
            Y3_CHECK_ARG(r.oy[q] >= 0 && r.ox[q] >= 0 && (long long)r.oy[q] + qh <= h && (long long)r.ox[q] + qw <= w,
                         "mosaic_batch: record %d: quadrant %d: window %d+%d x %d+%d leaves the %dx%d source", i, q, r.oy[q], qh, r.ox[q], qw, h, w);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int groups = y3_cdiv((long long)plane + 3, 4);
    const int div_shift = 31 + y3_ilog2(w);
    const unsigned div_mul = (unsigned)((1ULL << div_shift) / (unsigned long long)w + 1);
    for (int base = 0; base < n; base += Y3_AUG_CHUNK) {
        const int nb = std::min(Y3_AUG_CHUNK, n - base);
        MosTable tab = {};
        for (int i = 0; i < nb; ++i) {
            const y3_mosaic_record& r = records[base + i];
            MosImg& m = tab.img[i];
            m.cy = r.cy;
            m.cx = r.cx;
            for (int q = 0; q < 4; ++q) {
                const int qy = (q & 2) ? r.cy : 0, qx = (q & 1) ? r.cx : 0;
                if (((q & 2) ? h - r.cy : r.cy) == 0 || ((q & 1) ? w - r.cx : r.cx) == 0) continue;      // empty: no element selects it
                m.delta[q] = (long long)r.src[q] * (long long)image + ((long long)r.oy[q] - qy) * w + ((long long)r.ox[q] - qx);
            }
        }
        hipLaunchKernelGGL(mosaic_kernel, dim3(y3_cdiv(groups, 256), c, nb), dim3(256), 0, st, src, out + (size_t)base * image, tab, c, h, w, div_mul, div_shift);
        Y3_CHECK_LAUNCH("mosaic_batch");
    }
    return Y3_OK;
}

// ---- affine warp: every output pixel gathers four taps of its own image (not in the reference) -----------------------------
#define Y3_AFF_TILE 32             // a 256-thread workgroup covers 32 x 32 output pixels: 32 columns x 8 rows of threads, 4 rows each
#define Y3_AFF_MAX_COORD 1073741824.0      // 2^30: bound on |m0| (w-1) + |m1| (h-1) + |m2| (y alike), so (int)floorf(s) is defined

struct AffImg {                    // 32 bytes
    float m[6];
    float fill;
    int pad0;
};
struct AffTable {
    AffImg img[Y3_AUG_CHUNK];
};
typedef float aff_f2u __attribute__((ext_vector_type(2), aligned(4)));      // 8 bytes at 4-byte alignment: one global_load_dwordx2

// aug_lerp's form with the second weight-zero case: f == 1 happens (sx = -1e-9 has floor -1 and the fp32 fraction 1), and then `a`
// must not be touched either.  Roundings: g (1), g * a (1), f * b (1), the sum (1): a's term carries 3, b's term 2, and a lerp of
// two lerps twice that, so the worst tap of a bilinear value carries 6 fp32 roundings (the bound of tests/affine_reference.py).
__device__ __forceinline__ float aff_lerp(float a, float b, float f) {
    const float g = 1.f - f;
    return f == 0.f ? a : g == 0.f ? b : g * a + f * b;
}

// grid (tiles of a plane, 1, images of the chunk); `src` and `out` are the chunk's first image.  Thread t owns column
// tile_x + (t & 31) of rows tile_y + (t >> 5) + {0, 8, 16, 24}: a wave stores two 128-byte row pieces per channel plane and its
// taps lie in two short source segments.  A tap that is outside the image or has weight zero is not read: it takes `fill`, which
// aff_lerp then uses (outside) or drops (weight zero).  Where all four taps are inside and live -- every pixel of a rotated or
// scaled image but those at its border -- the two taps of a row are one global_load_dwordx2 at 4-byte alignment: six loads per
// pixel of three channels instead of twelve (profiles/affine_cost.txt has both forms).
template <int C>
__global__ __launch_bounds__(256) void affine_kernel(const float* __restrict__ src, float* __restrict__ out, AffTable tab, int H, int W, int tilesx) {
    const AffImg& a = tab.img[blockIdx.z];
    const int ty = (int)blockIdx.x / tilesx, tx = (int)blockIdx.x - ty * tilesx;
    const int x = tx * Y3_AFF_TILE + (int)(threadIdx.x & 31);
    if (x >= W) return;
    const size_t plane = (size_t)H * W;
    const float* s = src + (size_t)blockIdx.z * C * plane;
    float* o = out + (size_t)blockIdx.z * C * plane;
    const float xf = (float)x, fill = a.fill;
    const float ax = a.m[0] * xf, bx = a.m[3] * xf;
#pragma unroll
    for (int k = 0; k < Y3_AFF_TILE / 8; ++k) {
        const int y = ty * Y3_AFF_TILE + (int)(threadIdx.x >> 5) + 8 * k;
        if (y >= H) break;
        const float yf = (float)y;
        const float sx = (ax + a.m[1] * yf) + a.m[2];      // unfused, in this order (-ffp-contract=off): augment.affine_coords
        const float sy = (bx + a.m[4] * yf) + a.m[5];
        const float flx = floorf(sx), fly = floorf(sy);
        const float fx = sx - flx, fy = sy - fly;
        const int x0 = (int)flx, y0 = (int)fly;             // |s| <= 2^30 (1 + 2^-22): checked on the host
        const bool cl = fx != 1.f, cr = fx != 0.f, rt = fy != 1.f, rb = fy != 0.f;      // the column / row has a non-zero weight
        const bool inl = (unsigned)x0 < (unsigned)W, inr = (unsigned)(x0 + 1) < (unsigned)W;
        const bool int_ = (unsigned)y0 < (unsigned)H, inb = (unsigned)(y0 + 1) < (unsigned)H;
        const unsigned e = (unsigned)y0 * (unsigned)W + (unsigned)x0;      // mod 2^32; a tap inside the image has 0 <= index < H * W < 2^31
        const bool r00 = cl && rt && inl && int_, r01 = cr && rt && inr && int_, r10 = cl && rb && inl && inb, r11 = cr && rb && inr && inb;
        float v[C][4];
        if (r00 && r01 && r10 && r11) {                      // the interior: the two taps of a row are one 8-byte load at 4-byte alignment
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {                 // all loads of the pixel issued before the first use
                const float* p = s + ch * plane + e;
                const aff_f2u top = *(const aff_f2u*)p, bot = *(const aff_f2u*)(p + W);
                v[ch][0] = top.x;
                v[ch][1] = top.y;
                v[ch][2] = bot.x;
                v[ch][3] = bot.y;
            }
        } else {                                             // an edge of the image or a weight of zero
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float* p = s + ch * plane;
                v[ch][0] = r00 ? p[e] : fill;
                v[ch][1] = r01 ? p[e + 1] : fill;
                v[ch][2] = r10 ? p[e + W] : fill;
                v[ch][3] = r11 ? p[e + W + 1] : fill;
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
            o[ch * plane + (size_t)y * W + x] = aff_lerp(aff_lerp(v[ch][0], v[ch][1], fx), aff_lerp(v[ch][2], v[ch][3], fx), fy);
    }
}

extern "C" int y3_affine_batch(const float* src, int n, int c, int h, int w, const y3_affine_record* records, float* out, y3_stream_t stream) {
    Y3_CHECK_ARG(src && records && out, "affine_batch: null pointer");
    Y3_CHECK_ARG(c == 1 || c == 3, "affine_batch: channels %d (1 or 3)", c);
    Y3_CHECK_ARG(n > 0 && h > 0 && w > 0, "affine_batch: bad dims n %d, %dx%d", n, h, w);
    Y3_CHECK_ARG((long long)h * w < (1LL << 31) - 8, "affine_batch: plane %dx%d too large", h, w);
    const size_t plane = (size_t)h * w, image = plane * c, bytes = (size_t)n * image * sizeof(float);
    Y3_CHECK_ARG((((size_t)src | (size_t)out) & 3) == 0, "affine_batch: src / out not 4-byte aligned");
    Y3_CHECK_ARG((size_t)src + bytes <= (size_t)out || (size_t)out + bytes <= (size_t)src, "affine_batch: src and out overlap (the pass cannot run in place)");
    for (int i = 0; i < n; ++i) {
        const y3_affine_record& r = records[i];
        Y3_CHECK_ARG(r.reserved == 0, "affine_batch: record %d: reserved word %d", i, r.reserved);
        bool finite = isfinite(r.fill);
        for (int k = 0; k < 6; ++k) finite = finite && isfinite(r.m[k]);
        Y3_CHECK_ARG(finite, "affine_batch: record %d: non-finite coefficient or fill", i);
        for (int k = 0; k < 6; k += 3) {
            const double reach = fabs((double)r.m[k]) * (w - 1) + fabs((double)r.m[k + 1]) * (h - 1) + fabs((double)r.m[k + 2]);
            Y3_CHECK_ARG(reach <= Y3_AFF_MAX_COORD, "affine_batch: record %d: source %s coordinate reaches %g at a corner of the output (limit 2^30)", i,
                         k ? "y" : "x", reach);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int tilesx = y3_cdiv(w, Y3_AFF_TILE), tilesy = y3_cdiv(h, Y3_AFF_TILE);
    Y3_CHECK_ARG((long long)tilesx * tilesy <= (1LL << 23), "affine_batch: %dx%d needs more than 2^23 tiles of %d x %d", h, w, Y3_AFF_TILE, Y3_AFF_TILE);
    for (int base = 0; base < n; base += Y3_AUG_CHUNK) {
        const int nb = std::min(Y3_AUG_CHUNK, n - base);
        AffTable tab = {};
        for (int i = 0; i < nb; ++i) {
            const y3_affine_record& r = records[base + i];
            for (int k = 0; k < 6; ++k) tab.img[i].m[k] = r.m[k];
            tab.img[i].fill = r.fill;
        }
        const dim3 grid((unsigned)((long long)tilesx * tilesy), 1, nb);
        if (c == 1) hipLaunchKernelGGL(affine_kernel<1>, grid, dim3(256), 0, st, src + (size_t)base * image, out + (size_t)base * image, tab, h, w, tilesx);
        else hipLaunchKernelGGL(affine_kernel<3>, grid, dim3(256), 0, st, src + (size_t)base * image, out + (size_t)base * image, tab, h, w, tilesx);
        Y3_CHECK_LAUNCH("affine_batch");
    }
    return Y3_OK;
}

// ---- colour matrix, clamp, tone curve and MixUp: one elementwise pass (not in the reference) --------------------------------
#define Y3_PHO_CHUNK 16            // images per launch: 16 x 128 B of table travel as a kernel argument

struct PhoOp {                     // 56 bytes: the photometric part of one y3_photo_record
    float m[9];
    float bias[3];
    float gamma, white;
};
struct PhoImg {                    // 128 bytes, one per OUTPUT image
    PhoOp self, other;             // its own record's and its partner's record's operator (`other` unused when lambda == 1)
    long long own, partner;        // element offsets of the image and of its partner from `src` (the whole batch)
};
struct PhoTable {
    PhoImg img[Y3_PHO_CHUNK];
    float lambda[Y3_PHO_CHUNK];
};
typedef float pho_f4 __attribute__((ext_vector_type(4)));
typedef float pho_f4u __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at 4-byte alignment: one global_load_dwordx4

// P_r of the G pixels e0 .. e0 + G - 1 of the image at `p` (planes of P elements) -> v[channel][pixel].  Only the pixels in
// [lo, hi) are read (`whole`: all G = 4 of them, as one 16-byte load per plane); the others come out as P_r(0) and are never
// stored.  Every branch on the record is uniform over the workgroup (the record is per image): scalar branches.  fp32, one
// rounding per operation in the order of yolo3hip.h (-ffp-contract=off), which augment.photometric_reference restates:
//   matrix   a term with coefficient 0 is skipped, and a channel no row uses is not loaded; a coefficient of exactly 1 passes its
//            channel unmultiplied; a zero bias is not added; a row without terms and bias is +0
//   clamp    selects, not max / min: NaN stays NaN (and -0.0 stays -0.0)
//   curve    s = t / white (IEEE division), white * exp2f(gamma * log2f(s)); s == 0 gives 0 and s == 1 gives 1 (log2f(1) = 0,
//            exp2f(0) = 1), so both ends are exact; exp2f / log2f are the device library's (they scale denormals around the
//            hardware v_exp_f32 / v_log_f32); the accuracy relied on is the measured one of profiles/photometric_err.txt
template <int C, int G>
__device__ __forceinline__ void pho_eval(const PhoOp& r, const float* __restrict__ p, int P, int e0, bool whole, int lo, int hi, float (&v)[C][G]) {
    float c[C][G];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        bool used = false;
#pragma unroll
        for (int k = 0; k < C; ++k) used = used || r.m[3 * k + j] != 0.f;
#pragma unroll
        for (int i = 0; i < G; ++i) c[j][i] = 0.f;
        if (!used) continue;
        const float* q = p + (size_t)j * (size_t)P;
        if (G == 4 && whole) {
            const pho_f4u t = *(const pho_f4u*)(q + e0);
#pragma unroll
            for (int i = 0; i < G; ++i) c[j][i] = t[i];
        } else {
#pragma unroll
            for (int i = 0; i < G; ++i)
                if (e0 + i >= lo && e0 + i < hi) c[j][i] = q[e0 + i];
        }
    }
    const bool clamp = r.white > 0.f, curve = r.gamma != 1.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const float* mk = r.m + 3 * k;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            float acc = 0.f;
            bool started = false;
#pragma unroll
            for (int j = 0; j < C; ++j)
                if (mk[j] != 0.f) {
                    const float t = mk[j] == 1.f ? c[j][i] : mk[j] * c[j][i];
                    acc = started ? acc + t : t;
                    started = true;
                }
            if (r.bias[k] != 0.f) acc = started ? acc + r.bias[k] : r.bias[k];
            if (clamp) acc = acc < 0.f ? 0.f : (acc > r.white ? r.white : acc);
            if (curve) {
                const float s = acc / r.white;
                acc = r.white * (s == 0.f ? 0.f : exp2f(r.gamma * log2f(s)));
            }
            v[k][i] = acc;
        }
    }
}

// grid (groups of a plane / 256, 1, images of the chunk).  `out` is the chunk's first output image, `src` the whole batch.  G = 4:
// thread t of the grid owns the 16-byte-aligned group of four output floats that starts e0 = 4 t - a elements into each plane of
// its image, a = the plane's offset into a 16-byte group (the same for every plane: P is a multiple of 4); the first and last group
// of a plane may be partial and go float by float.  G = 1 (P no multiple of 4): one pixel per thread.
template <int C, int G>
__global__ __launch_bounds__(256) void photometric_kernel(const float* __restrict__ src, float* __restrict__ out, PhoTable tab, int P) {
    const PhoImg& r = tab.img[blockIdx.z];
    const float lambda = tab.lambda[blockIdx.z];
    float* o = out + (size_t)blockIdx.z * C * (size_t)P;
    const int a = G == 4 ? (int)(((size_t)o >> 2) & 3) : 0;
    const int e0 = (int)((blockIdx.x * 256u + threadIdx.x) * (unsigned)G) - a;      // -3 .. P-1
    if (e0 >= P) return;
    const int lo = max(e0, 0), hi = min(e0 + G, P);
    const bool whole = e0 >= 0 && e0 + G <= P;
    float v[C][G];
    pho_eval<C, G>(r.self, src + r.own, P, e0, whole, lo, hi, v);
    if (lambda != 1.f) {                                         // uniform: an image that is not mixed never reads a partner
        float u[C][G];
        pho_eval<C, G>(r.other, src + r.partner, P, e0, whole, lo, hi, u);
        const float rest = 1.f - lambda;
#pragma unroll
        for (int k = 0; k < C; ++k)
#pragma unroll
            for (int i = 0; i < G; ++i) v[k][i] = (lambda * v[k][i]) + (rest * u[k][i]);
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        float* q = o + (size_t)k * (size_t)P;
        if (G == 4 && whole) {
            pho_f4 t;
#pragma unroll
            for (int i = 0; i < G; ++i) t[i] = v[k][i];
            *(pho_f4*)(q + e0) = t;
        } else {
#pragma unroll
            for (int i = 0; i < G; ++i)
                if (e0 + i >= lo && e0 + i < hi) q[e0 + i] = v[k][i];
        }
    }
}

extern "C" int y3_photometric_batch(const float* src, int n, int c, int h, int w, const y3_photo_record* records, float* out, y3_stream_t stream) {
    Y3_CHECK_ARG(src && records && out, "photometric_batch: null pointer");
    Y3_CHECK_ARG(c == 1 || c == 3, "photometric_batch: channels %d (1 or 3)", c);
    Y3_CHECK_ARG(n > 0 && h > 0 && w > 0, "photometric_batch: bad dims n %d, %dx%d", n, h, w);
    Y3_CHECK_ARG((long long)h * w < (1LL << 31) - 8, "photometric_batch: plane %dx%d too large", h, w);
    const size_t plane = (size_t)h * w, image = plane * c, bytes = (size_t)n * image * sizeof(float);
    Y3_CHECK_ARG((((size_t)src | (size_t)out) & 3) == 0, "photometric_batch: src / out not 4-byte aligned");
    Y3_CHECK_ARG((size_t)src + bytes <= (size_t)out || (size_t)out + bytes <= (size_t)src, "photometric_batch: src and out overlap (the pass cannot run in place)");
    for (int i = 0; i < n; ++i) {
        const y3_photo_record& r = records[i];
        bool finite = isfinite(r.gamma) && isfinite(r.white) && isfinite(r.lambda);
        for (int k = 0; k < 9; ++k) finite = finite && isfinite(r.m[k]);
        for (int k = 0; k < 3; ++k) finite = finite && isfinite(r.bias[k]);
        Y3_CHECK_ARG(finite, "photometric_batch: record %d: non-finite coefficient, bias, gamma, white or lambda", i);
        Y3_CHECK_ARG(r.gamma > 0.f, "photometric_batch: record %d: gamma %g (must be > 0)", i, r.gamma);
        Y3_CHECK_ARG(r.white >= 0.f, "photometric_batch: record %d: white %g (must be >= 0)", i, r.white);
        Y3_CHECK_ARG(r.white > 0.f || r.gamma == 1.f, "photometric_batch: record %d: gamma %g needs white > 0 (the tone curve is scaled by it)", i, r.gamma);
        Y3_CHECK_ARG(r.lambda >= 0.f && r.lambda <= 1.f, "photometric_batch: record %d: lambda %g outside [0, 1]", i, r.lambda);
        Y3_CHECK_ARG(r.lambda == 1.f || (r.partner >= 0 && r.partner < n), "photometric_batch: record %d: partner image %d of %d", i, r.partner, n);
    }
    hipStream_t st = (hipStream_t)stream;
    const int g = (plane & 3) == 0 ? 4 : 1;
    const int groups = g == 4 ? y3_cdiv((long long)plane + 3, 4) : (int)plane;
    auto op = [](const y3_photo_record& r) {
        PhoOp p;
        for (int k = 0; k < 9; ++k) p.m[k] = r.m[k];
        for (int k = 0; k < 3; ++k) p.bias[k] = r.bias[k];
        p.gamma = r.gamma;
        p.white = r.white;
        return p;
    };
    for (int base = 0; base < n; base += Y3_PHO_CHUNK) {
        const int nb = std::min(Y3_PHO_CHUNK, n - base);
        PhoTable tab = {};
        for (int i = 0; i < nb; ++i) {
            const y3_photo_record& r = records[base + i];
            const bool mixed = r.lambda != 1.f;
            tab.img[i].self = op(r);
            tab.img[i].other = op(mixed ? records[r.partner] : r);
            tab.img[i].own = (long long)(base + i) * (long long)image;
            tab.img[i].partner = mixed ? (long long)r.partner * (long long)image : tab.img[i].own;
            tab.lambda[i] = r.lambda;
        }
        for (int i = nb; i < Y3_PHO_CHUNK; ++i) tab.lambda[i] = 1.f;
        const dim3 grid((unsigned)y3_cdiv(groups, 256), 1, nb);
        float* o = out + (size_t)base * image;
        if (c == 1 && g == 4) hipLaunchKernelGGL((photometric_kernel<1, 4>), grid, dim3(256), 0, st, src, o, tab, (int)plane);
        else if (c == 1) hipLaunchKernelGGL((photometric_kernel<1, 1>), grid, dim3(256), 0, st, src, o, tab, (int)plane);
        else if (g == 4) hipLaunchKernelGGL((photometric_kernel<3, 4>), grid, dim3(256), 0, st, src, o, tab, (int)plane);
        else hipLaunchKernelGGL((photometric_kernel<3, 1>), grid, dim3(256), 0, st, src, o, tab, (int)plane);
        Y3_CHECK_LAUNCH("photometric_batch");
    }
    return Y3_OK;
}
