// SGD with momentum (plain and Nesterov) and AdamW over the whole parameter arena, with weight decay on some segments of it
// (DESIGN §3.19).  Streaming kernels of adam_kernel's shape (pointwise.hip): 256 threads, 16-byte accesses, a grid-stride loop,
// a scalar tail for count & 3; everything that changes per step is read from device memory, so the launch is graph-replayable.
#include "common.h"
#include "adam_update.h"

// The decay ranges travel by value in the kernel arguments as 2 * n sorted boundaries in FLOAT4 units (begin / 4, ceil(end / 4):
// the host has checked that a float4 is wholly inside or wholly outside a range, and the tail counts as the float4 at count / 4).
// A float4 index i is decayed when the number of boundaries <= i is odd; touching ranges give two equal boundaries, which cancel.
struct OptimRanges {
    unsigned b[2 * Y3_OPT_MAX_RANGES];
};
#define Y3_OPT_NO_BOUNDARY 0xFFFFFFFFu      // above every float4 index the host lets through
static_assert(2 * Y3_OPT_MAX_RANGES == 256, "a block of 256 threads stages one boundary per thread");

// one element of one float4 lane f.  D: the float4 lies in a decay range.  Each line is one fp32 expression (-ffp-contract=off).
// torch.optim.SGD with dampening 0 and coupled L2: the decay joins the gradient, so the momentum buffer carries it
#define Y3_SGD1(f)                                                          \
    if (D) gg.f = gg.f + wd * pp.f;                                         \
    mm.f = mu * mm.f + gg.f;                                                \
    pp.f = pp.f - h0 * (KIND == Y3_OPT_SGD_NESTEROV ? gg.f + mu * mm.f : mm.f);
// AdamW: decoupled decay first (as Keras and PyTorch do), then the text of the Adam kernels
#define Y3_ADAMW1(f)                     \
    if (D) pp.f = pp.f - lw * pp.f;      \
    Y3_ADAM1(f)

template <int KIND, bool EMA, bool SCALED>
__global__ void __launch_bounds__(256)
optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t count4, size_t count,
             const float* __restrict__ hyper_dev, float mu, float wd, float b1, float b2, float eps, const OptimRanges tab, int nb,
             float* __restrict__ ema_p, const float* __restrict__ mv, float* __restrict__ ema_mv, size_t mcount4, size_t mcount,
             const float* __restrict__ omd_dev, const float* __restrict__ scale_dev) {
    constexpr bool ADAMW = KIND == Y3_OPT_ADAMW;
    // the boundaries in LDS, closed by a sentinel so that the cursor below needs no bound of its own
    __shared__ unsigned sb[2 * Y3_OPT_MAX_RANGES + 1];
    sb[threadIdx.x] = (int)threadIdx.x < nb ? tab.b[threadIdx.x] : Y3_OPT_NO_BOUNDARY;
    if (threadIdx.x == 0) sb[2 * Y3_OPT_MAX_RANGES] = Y3_OPT_NO_BOUNDARY;
    __syncthreads();
    const float h0 = hyper_dev[0];                 // lr (SGD) or lr_t (AdamW)
    const float lr_t = h0;                         // the name Y3_ADAM1 reads
    const float lw = ADAMW ? hyper_dev[1] : 0.f;   // lr * weight_decay
    const float omd = EMA ? *omd_dev : 0.f;
    const float s = SCALED ? *scale_dev : 1.f;
    const float o1 = 1.f - b1, o2 = 1.f - b2;
    (void)lr_t, (void)lw, (void)omd, (void)s, (void)o1, (void)o2;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // a thread's float4 indices only grow, so a cursor over the boundaries serves all its iterations: it advances at most
    // 2 * n_ranges times over the whole loop, and an iteration that crosses no boundary costs one LDS read
    unsigned cur = 0;
    for (size_t i = tid; i < count4; i += stride) {
        while (sb[cur] <= (unsigned)i) ++cur;
        const bool D = cur & 1;
        float4 pp = reinterpret_cast<float4*>(p)[i];
        float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv, ee;
        if constexpr (ADAMW) vv = reinterpret_cast<float4*>(v)[i];
        if constexpr (EMA) ee = reinterpret_cast<float4*>(ema_p)[i];
        if constexpr (SCALED) gg.x *= s, gg.y *= s, gg.z *= s, gg.w *= s;
        if constexpr (ADAMW) {
            Y3_ADAMW1(x) Y3_ADAMW1(y) Y3_ADAMW1(z) Y3_ADAMW1(w)
        } else {
            Y3_SGD1(x) Y3_SGD1(y) Y3_SGD1(z) Y3_SGD1(w)
        }
        if constexpr (EMA) {
            ee.x += (pp.x - ee.x) * omd;
            ee.y += (pp.y - ee.y) * omd;
            ee.z += (pp.z - ee.z) * omd;
            ee.w += (pp.w - ee.w) * omd;
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        if constexpr (ADAMW) reinterpret_cast<float4*>(v)[i] = vv;
        if constexpr (EMA) reinterpret_cast<float4*>(ema_p)[i] = ee;
    }
    if constexpr (EMA) {
        for (size_t i = tid; i < mcount4; i += stride) {
            const float4 s4 = reinterpret_cast<const float4*>(mv)[i];
            float4 ee = reinterpret_cast<float4*>(ema_mv)[i];
            ee.x += (s4.x - ee.x) * omd;
            ee.y += (s4.y - ee.y) * omd;
            ee.z += (s4.z - ee.z) * omd;
            ee.w += (s4.w - ee.w) * omd;
            reinterpret_cast<float4*>(ema_mv)[i] = ee;
        }
    }
    // tails: lane x of a float4 through the same update text; the tail is decayed when the last range ends at count
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) {
        const size_t i = (count4 << 2) + threadIdx.x;
        unsigned c = 0;
        while (sb[c] <= (unsigned)count4) ++c;
        const bool D = c & 1;
        float4 pp, gg, mm, vv;
        pp.x = p[i], gg.x = g[i], mm.x = m[i];
        if constexpr (ADAMW) vv.x = v[i];
        if constexpr (SCALED) gg.x *= s;
        if constexpr (ADAMW) {
            Y3_ADAMW1(x)
        } else {
            Y3_SGD1(x)
        }
        p[i] = pp.x;
        m[i] = mm.x;
        if constexpr (ADAMW) v[i] = vv.x;
        if constexpr (EMA) ema_p[i] += (pp.x - ema_p[i]) * omd;
    }
    if constexpr (EMA) {
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x < (mcount & 3)) {
            const size_t i = (mcount4 << 2) + threadIdx.x;
            ema_mv[i] += (mv[i] - ema_mv[i]) * omd;
        }
    }
}

template <int KIND, bool EMA, bool SCALED>
static void optim_launch(const y3_optim_desc* d, const OptimRanges& tab, hipStream_t stream) {
    const size_t mcount = EMA ? d->moving_count : 0;
    const long long items = (long long)((d->count > mcount ? d->count : mcount) / 4 + 1);
    hipLaunchKernelGGL((optim_kernel<KIND, EMA, SCALED>), dim3(stream_blocks(items, 256)), dim3(256), 0, stream, d->param, d->grad, d->m, d->v,
                       d->count / 4, d->count, d->hyper_dev, d->momentum, d->weight_decay, d->beta1, d->beta2, d->eps, tab, 2 * d->n_ranges,
                       d->ema_param, d->moving, d->ema_moving, mcount / 4, mcount, d->omd_dev, d->scale_dev);
}

extern "C" int y3_optim_step(const y3_optim_desc* d, y3_stream_t stream) {
    Y3_CHECK_ARG(d, "optim_step: null descriptor");
    Y3_CHECK_ARG(d->kind == Y3_OPT_SGD || d->kind == Y3_OPT_SGD_NESTEROV || d->kind == Y3_OPT_ADAMW, "optim_step: unknown kind %d", d->kind);
    const bool adamw = d->kind == Y3_OPT_ADAMW;
    Y3_CHECK_ARG(d->param && d->grad && d->m && d->hyper_dev, "optim_step: null pointer");
    Y3_CHECK_ARG(!adamw || d->v, "optim_step: AdamW needs the second-moment arena v (null pointer)");
    const bool ema = d->ema_param || d->moving || d->ema_moving || d->omd_dev || d->moving_count;
    Y3_CHECK_ARG(!ema || (d->ema_param && d->omd_dev && (d->moving_count == 0 || (d->moving && d->ema_moving))),
                 "optim_step: partial set of EMA pointers (ema_param, omd_dev, and moving / ema_moving with moving_count, or none)");
    Y3_CHECK_ARG((((uintptr_t)d->param | (uintptr_t)d->grad | (uintptr_t)d->m | (uintptr_t)d->v | (uintptr_t)d->ema_param | (uintptr_t)d->moving |
                   (uintptr_t)d->ema_moving) & 15) == 0,
                 "optim_step: arenas must be 16-byte aligned");
    Y3_CHECK_ARG(d->n_ranges >= 0 && d->n_ranges <= Y3_OPT_MAX_RANGES, "optim_step: n_ranges must be in 0..%d, got %d", Y3_OPT_MAX_RANGES,
                 d->n_ranges);
    Y3_CHECK_ARG(d->n_ranges == 0 || d->decay_ranges_host, "optim_step: null decay_ranges_host with n_ranges = %d", d->n_ranges);
    // the kernel keeps float4 indices in 32 bits, Y3_OPT_NO_BOUNDARY above them all
    Y3_CHECK_ARG(d->count / 4 < (size_t)Y3_OPT_NO_BOUNDARY - 1, "optim_step: count %zu is beyond the 2^34 floats one launch takes", d->count);
    OptimRanges tab;
    long long prev_end = 0;
    for (int r = 0; r < d->n_ranges; ++r) {
        const long long b = d->decay_ranges_host[2 * r], e = d->decay_ranges_host[2 * r + 1];
        Y3_CHECK_ARG(b >= 0 && b < e, "optim_step: decay range %d [%lld, %lld) is empty or negative", r, b, e);
        Y3_CHECK_ARG((unsigned long long)e <= d->count, "optim_step: decay range %d [%lld, %lld) ends beyond count %zu", r, b, e, d->count);
        Y3_CHECK_ARG(b >= prev_end, "optim_step: decay range %d [%lld, %lld) is not sorted or overlaps the one before it", r, b, e);
        Y3_CHECK_ARG((b & 3) == 0 && ((e & 3) == 0 || (unsigned long long)e == d->count),
                     "optim_step: decay range %d [%lld, %lld) must begin on a multiple of 4 and end on one or at count", r, b, e);
        tab.b[2 * r] = (unsigned)(b / 4);
        tab.b[2 * r + 1] = (unsigned)((e + 3) / 4);
        prev_end = e;
    }
    for (int i = 2 * d->n_ranges; i < 2 * Y3_OPT_MAX_RANGES; ++i) tab.b[i] = Y3_OPT_NO_BOUNDARY;
    // (NaN fails both)
    Y3_CHECK_ARG(d->momentum >= 0.f && d->momentum < 1.f, "optim_step: momentum must be in [0, 1), got %g", (double)d->momentum);
    Y3_CHECK_ARG(d->weight_decay >= 0.f, "optim_step: weight_decay must be >= 0, got %g", (double)d->weight_decay);
    if (d->count == 0) return Y3_OK;
    const hipStream_t st = (hipStream_t)stream;
    const bool scaled = d->scale_dev != nullptr;
#define Y3_OPT_CASE(K)                                                     \
    case K:                                                                \
        if (ema && scaled) optim_launch<K, true, true>(d, tab, st);        \
        else if (ema) optim_launch<K, true, false>(d, tab, st);            \
        else if (scaled) optim_launch<K, false, true>(d, tab, st);         \
        else optim_launch<K, false, false>(d, tab, st);                    \
        break;
    switch (d->kind) {
        Y3_OPT_CASE(Y3_OPT_SGD)
        Y3_OPT_CASE(Y3_OPT_SGD_NESTEROV)
        Y3_OPT_CASE(Y3_OPT_ADAMW)
    }
#undef Y3_OPT_CASE
    Y3_CHECK_LAUNCH("optim_step");
    return Y3_OK;
}
