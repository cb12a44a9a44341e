// Spatial pyramid pooling of YOLOv3-SPP: the three stride-1 SAME max pools 5 / 9 / 13 of one NHWC tensor in one
// launch, and their gradient in one launch.
//
// A workgroup owns one image and one group of 4 channels: the H x W plane of that group (16 bytes per pixel) is read from HBM
// once into LDS, every pool is computed there, and only results go back.  4 channels is the smallest group a 16-byte access
// allows and gives N * C / 4 workgroups (128 per image at C = 512), so that even one image covers half the machine's 256 CUs and
// two cover it; the plane of the largest grid of the model (19 x 19 at 608^2) is 5.6 KiB.  Source and destination may be disjoint
// channel ranges of one allocation: a workgroup has its whole source plane in LDS before its first store, and no workgroup stores
// to a channel another one loads.
#include "common.h"

typedef unsigned short u16;

#define SPP_THREADS 256
#define SPP_MAX_OWN (Y3_SPP_MAX_PLANE / SPP_THREADS)   // pixels of the largest plane per thread
#define SPP_SMALL_OWN 2                                // ... of a plane of up to 512 pixels (22 x 22: every grid of the model)
#define SPP_DEFAULT_LDS 65536   // dynamic LDS a kernel may ask for without hipFuncAttributeMaxDynamicSharedMemorySize

// max that keeps a NaN of either side (fmaxf drops it): a diverged run must still show
__device__ __forceinline__ float spp_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float4 spp_max4(const float4 a, const float4 b) {
    return make_float4(spp_max(a.x, b.x), spp_max(a.y, b.y), spp_max(a.z, b.z), spp_max(a.w, b.w));
}

// 4 channels of one pixel, fp32 in registers; bf16 <-> fp32 is exact both ways for values that came from bf16 (NaNs included)
template <bool BF16>
__device__ __forceinline__ float4 spp_load4(const void* base, long long off) {
    if (BF16) {
        const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const u16*>(base) + off);
        return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                           __uint_as_float(v.y & 0xffff0000u));
    }
    return *reinterpret_cast<const float4*>(static_cast<const float*>(base) + off);
}
template <bool BF16>
__device__ __forceinline__ void spp_store4(void* base, long long off, const float4 v) {
    if (BF16) {
        uint2 o;
        o.x = (__float_as_uint(v.x) >> 16) | (__float_as_uint(v.y) & 0xffff0000u);
        o.y = (__float_as_uint(v.z) >> 16) | (__float_as_uint(v.w) & 0xffff0000u);
        *reinterpret_cast<uint2*>(static_cast<u16*>(base) + off) = o;
    } else {
        *reinterpret_cast<float4*>(static_cast<float*>(base) + off) = v;
    }
}

// ---------------------------------------------------------------------------
// forward: pool5 as a row pass and a column pass over the LDS plane; pool9 = pool5 o pool5 and pool13 = pool5 o pool9 (exact for
// the values, borders included: a clipped window of clipped windows is the clipped window of the sum of the radii)
// ---------------------------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(SPP_THREADS) void spp_fwd_kernel(const void* src, int s_ld, void* dst, int d_ld, int C, int H, int W, int groups) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spp_lds[];
    const int HW = H * W;
    float4* A = reinterpret_cast<float4*>(spp_lds);      // [HW]
    float4* B = A + HW;                                   // [HW]
    const int n = blockIdx.x / groups;
    const int c0 = (blockIdx.x - n * groups) * 4;
    const long long pix0 = (long long)n * HW;
    for (int p = threadIdx.x; p < HW; p += SPP_THREADS) A[p] = spp_load4<BF16>(src, (pix0 + p) * s_ld + c0);
    __syncthreads();
    for (int lvl = 0; lvl < 3; ++lvl) {
        for (int p = threadIdx.x; p < HW; p += SPP_THREADS) {
            const int i = p / W, j = p - i * W;
            const int jlo = max(j - 2, 0), jhi = min(j + 2, W - 1);
            float4 m = A[i * W + jlo];
            for (int jj = jlo + 1; jj <= jhi; ++jj) m = spp_max4(m, A[i * W + jj]);
            B[p] = m;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < HW; p += SPP_THREADS) {
            const int i = p / W, j = p - i * W;
            const int ilo = max(i - 2, 0), ihi = min(i + 2, H - 1);
            float4 m = B[ilo * W + j];
            for (int ii = ilo + 1; ii <= ihi; ++ii) m = spp_max4(m, B[ii * W + j]);
            A[p] = m;
            spp_store4<BF16>(dst, (pix0 + p) * d_ld + (long long)lvl * C + c0, m);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// backward: dsrc[p] (+)= sum over k = 5, 9, 13 and the pixels q whose k x k window has its FIRST maximum (row-major) at p of
// ddst_k[q].  The first maximum is separable: in every row of the window the first column that holds the row's maximum, then the
// first row whose maximum is the window's.  It is NOT what the 5 o 5 cascade of the forward pass would pick on ties, so every k
// scans the source plane itself.  Per pixel, channel and k one byte (row offset << 4 | column offset, each 0 .. k - 1) names the
// winner; the gather of an input pixel then walks its windows in a fixed order (k ascending, q row-major) and adds the ddst of
// the q that name it: no atomics, the same bits on every run.  src, ddst and dsrc each cross HBM once: ddst is staged in LDS, one
// pool's block at a time, in the space of the source plane, which the winners have made redundant by then.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned spp_byte(unsigned v, int c) { return (v >> (8 * c)) & 0xffu; }

// OWN: pixels per thread the gather keeps sums for, 2 (planes of up to 512 pixels: every grid of the model) or SPP_MAX_OWN
template <int OWN>
__global__ __launch_bounds__(SPP_THREADS) void spp_bwd_kernel(const float* src, int s_ld, const float* ddst, int dd_ld, float* dsrc, int ds_ld,
                                                               int C, int H, int W, int groups, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spp_lds[];
    const int HW = H * W;
    float4* X = reinterpret_cast<float4*>(spp_lds);                 // [HW]     source plane, later one ddst block
    const float* Xs = reinterpret_cast<const float*>(spp_lds);
    unsigned* rowj = reinterpret_cast<unsigned*>(X + HW);           // [HW]     per channel: column offset of the row window's first maximum
    unsigned* win = rowj + HW;                                      // [3][HW]  per channel: the winner of the k x k window
    const int n = blockIdx.x / groups;
    const int c0 = (blockIdx.x - n * groups) * 4;
    const long long pix0 = (long long)n * HW;
    for (int p = threadIdx.x; p < HW; p += SPP_THREADS) X[p] = *reinterpret_cast<const float4*>(src + (pix0 + p) * s_ld + c0);
    __syncthreads();
    for (int lvl = 0; lvl < 3; ++lvl) {
        const int r = 2 + 2 * lvl;
        for (int p = threadIdx.x; p < HW; p += SPP_THREADS) {
            const int i = p / W, j = p - i * W;
            const int jlo = max(j - r, 0), jhi = min(j + r, W - 1);
            float4 best = X[i * W + jlo];
            unsigned b0 = (unsigned)(jlo - j + r), b1 = b0, b2 = b0, b3 = b0;
            for (int jj = jlo + 1; jj <= jhi; ++jj) {
                const float4 v = X[i * W + jj];
                const unsigned d = (unsigned)(jj - j + r);
                if (v.x > best.x) { best.x = v.x; b0 = d; }
                if (v.y > best.y) { best.y = v.y; b1 = d; }
                if (v.z > best.z) { best.z = v.z; b2 = d; }
                if (v.w > best.w) { best.w = v.w; b3 = d; }
            }
            rowj[p] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        }
        __syncthreads();
        for (int p = threadIdx.x; p < HW; p += SPP_THREADS) {
            const int i = p / W, j = p - i * W;
            const int ilo = max(i - r, 0), ihi = min(i + r, H - 1);
            unsigned packed = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float best = 0.f;
                unsigned code = 0;
                for (int ii = ilo; ii <= ihi; ++ii) {
                    const unsigned dj = spp_byte(rowj[ii * W + j], c);
                    const float v = Xs[(ii * W + j + (int)dj - r) * 4 + c];
                    if (ii == ilo || v > best) {
                        best = v;
                        code = ((unsigned)(ii - i + r) << 4) | dj;
                    }
                }
                packed |= code << (8 * c);
            }
            win[lvl * HW + p] = packed;
        }
        __syncthreads();
    }
    // gather.  The source plane is dead: its LDS holds one pool's ddst block at a time, loaded once with 16-byte accesses.  A thread
    // owns the pixels threadIdx.x + 256 s and keeps their sums in registers across the three pools (s is unrolled: static indices).
    float acc[OWN][4];
#pragma unroll
    for (int s = 0; s < OWN; ++s) acc[s][0] = acc[s][1] = acc[s][2] = acc[s][3] = 0.f;
    for (int lvl = 0; lvl < 3; ++lvl) {
        const int r = 2 + 2 * lvl;
        for (int p = threadIdx.x; p < HW; p += SPP_THREADS)
            X[p] = *reinterpret_cast<const float4*>(ddst + (pix0 + p) * dd_ld + (long long)lvl * C + c0);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < OWN; ++s) {
            const int p = (int)threadIdx.x + s * SPP_THREADS;
            if (p < HW) {
                const int i = p / W, j = p - i * W;
                const int ilo = max(i - r, 0), ihi = min(i + r, H - 1), jlo = max(j - r, 0), jhi = min(j + r, W - 1);
                for (int ii = ilo; ii <= ihi; ++ii)
                    for (int jj = jlo; jj <= jhi; ++jj) {
                        const unsigned me = ((unsigned)(i - ii + r) << 4) | (unsigned)(j - jj + r);      // how (ii, jj) would name this pixel
                        const unsigned x = win[lvl * HW + ii * W + jj] ^ (me * 0x01010101u);             // a zero byte: that channel names it
                        if ((x - 0x01010101u) & ~x & 0x80808080u) {
                            const float4 g = X[ii * W + jj];
                            if ((x & 0x000000ffu) == 0) acc[s][0] += g.x;
                            if ((x & 0x0000ff00u) == 0) acc[s][1] += g.y;
                            if ((x & 0x00ff0000u) == 0) acc[s][2] += g.z;
                            if ((x & 0xff000000u) == 0) acc[s][3] += g.w;
                        }
                    }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < OWN; ++s) {
        const int p = (int)threadIdx.x + s * SPP_THREADS;
        if (p < HW) {
            float* out = dsrc + (pix0 + p) * ds_ld + c0;
            float4 o = make_float4(acc[s][0], acc[s][1], acc[s][2], acc[s][3]);
            if (accumulate) {
                const float4 old = *reinterpret_cast<const float4*>(out);
                o.x = old.x + o.x;
                o.y = old.y + o.y;
                o.z = old.z + o.z;
                o.w = old.w + o.w;
            }
            *reinterpret_cast<float4*>(out) = o;
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// src: N x H x W x C, wide: N x H x W x 3C; elem: bytes per element (4-channel accesses: 16 bytes fp32, 8 bytes bf16)
static int spp_check(const char* what, const y3_tensor* src, const y3_tensor* wide, int elem) {
    Y3_CHECK_ARG(src && src->ptr && wide && wide->ptr, "%s: null tensor", what);
    Y3_CHECK_ARG(src->n > 0 && src->h > 0 && src->w > 0 && src->c > 0 && src->ld >= src->c && wide->ld >= wide->c, "%s: bad dims", what);
    Y3_CHECK_ARG(wide->n == src->n && wide->h == src->h && wide->w == src->w && wide->c == 3 * src->c,
                 "%s: geometry (the pooled tensor is N x H x W x 3C of the source's N x H x W x C)", what);
    const uintptr_t mask = (uintptr_t)(4 * elem - 1);
    Y3_CHECK_ARG((src->c & 3) == 0 && (src->ld & 3) == 0 && (wide->ld & 3) == 0 && ((uintptr_t)src->ptr & mask) == 0 && ((uintptr_t)wide->ptr & mask) == 0,
                 "%s: needs c, ld multiples of 4 and %d-byte alignment", what, 4 * elem);
    Y3_CHECK_ARG((long long)src->h * src->w <= Y3_SPP_MAX_PLANE, "%s: plane %d x %d has more than %d pixels (the plane of 4 channels is staged in LDS)",
                 what, src->h, src->w, Y3_SPP_MAX_PLANE);
    Y3_CHECK_ARG((long long)src->n * (src->c / 4) < 0x7fffffffLL, "%s: too many workgroups", what);
    return 0;
}

// planes above 64 KiB of LDS (more than 45 x 45 cells: no grid of the model) raise the kernel's limit first
static int spp_lds_limit(const char* what, const void* kernel, size_t lds) {
    if (lds <= SPP_DEFAULT_LDS) return 0;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        y3_set_error("%s: cannot raise the dynamic LDS limit to %zu bytes", what, lds);
        return Y3_ELAUNCH;
    }
    return 0;
}

template <bool BF16>
static int spp_fwd(const char* what, const y3_tensor* src, const y3_tensor* dst, y3_stream_t stream) {
    if (int e = spp_check(what, src, dst, BF16 ? 2 : 4)) return e;
    const int groups = src->c / 4;
    const size_t lds = (size_t)src->h * src->w * 32;
    if (int e = spp_lds_limit(what, (const void*)spp_fwd_kernel<BF16>, lds)) return e;
    hipLaunchKernelGGL(spp_fwd_kernel<BF16>, dim3((unsigned)(src->n * groups)), dim3(SPP_THREADS), lds, (hipStream_t)stream, (const void*)src->ptr, src->ld,
                       (void*)dst->ptr, dst->ld, src->c, src->h, src->w, groups);
    Y3_CHECK_LAUNCH(what);
    return Y3_OK;
}
extern "C" int y3_spp_fwd(const y3_tensor* src, const y3_tensor* dst, y3_stream_t stream) { return spp_fwd<false>("spp_fwd", src, dst, stream); }
extern "C" int y3_spp_fwd_bf16(const y3_tensor* src, const y3_tensor* dst, y3_stream_t stream) { return spp_fwd<true>("spp_fwd_bf16", src, dst, stream); }

extern "C" int y3_spp_bwd(const y3_tensor* src, const y3_tensor* ddst, const y3_tensor* dsrc, int accumulate, y3_stream_t stream) {
    if (int e = spp_check("spp_bwd", src, ddst, 4)) return e;
    Y3_CHECK_ARG(dsrc && dsrc->ptr, "spp_bwd: null dsrc");
    Y3_CHECK_ARG(dsrc->n == src->n && dsrc->h == src->h && dsrc->w == src->w && dsrc->c == src->c && dsrc->ld >= dsrc->c, "spp_bwd: dsrc geometry");
    Y3_CHECK_ARG((dsrc->ld & 3) == 0 && ((uintptr_t)dsrc->ptr & 15) == 0, "spp_bwd: dsrc needs ld a multiple of 4 and 16-byte alignment");
    const int groups = src->c / 4;
    const size_t lds = (size_t)src->h * src->w * 32;      // plane 16 + row winners 4 + window winners 3 x 4 bytes per pixel
    const bool small = src->h * src->w <= SPP_SMALL_OWN * SPP_THREADS;
    auto kernel = small ? spp_bwd_kernel<SPP_SMALL_OWN> : spp_bwd_kernel<SPP_MAX_OWN>;
    if (int e = spp_lds_limit("spp_bwd", (const void*)kernel, lds)) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(src->n * groups)), dim3(SPP_THREADS), lds, (hipStream_t)stream, (const float*)src->ptr, src->ld,
                       (const float*)ddst->ptr, ddst->ld, (float*)dsrc->ptr, dsrc->ld, src->c, src->h, src->w, groups, accumulate);
    Y3_CHECK_LAUNCH("spp_bwd");
    return Y3_OK;
}
