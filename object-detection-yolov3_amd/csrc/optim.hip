// Everything between the gradients and the new weights: the optimiser step over the whole parameter arena -- the reference's Adam
// (y3_adam_step and its EMA / scaled forms) and SGD with momentum (plain and Nesterov) and AdamW with weight
// decay on some segments of the arena (y3_optim_step), all instantiations of one kernel template -- and, at the
// end, gradient accumulation and the global gradient norm.  Streaming kernels: 256 threads, 16-byte accesses, a grid-stride
// loop, a scalar tail for count & 3; everything that changes per step is read from device memory, so the launch is graph-replayable.
#include "common.h"

// A fourth kind beside the public Y3_OPT_*: Keras Adam (App. C5), which knows no decay.  Only the y3_adam_step* entry points
// ask for it; y3_optim_step refuses it like any other unknown kind.
#define Y3_OPT_ADAM_PRIVATE 3
static_assert(Y3_OPT_ADAM_PRIVATE > Y3_OPT_SGD && Y3_OPT_ADAM_PRIVATE > Y3_OPT_SGD_NESTEROV && Y3_OPT_ADAM_PRIVATE > Y3_OPT_ADAMW, "no public kind");

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
// Adam; o1 = 1 - b1, o2 = 1 - b2.  One text for Adam and AdamW, plain, EMA and scaled, so all give the same bits
#define Y3_ADAM1(f)                              \
    mm.f += (gg.f - mm.f) * o1;                  \
    vv.f += (gg.f * gg.f - vv.f) * o2;           \
    pp.f -= (mm.f * lr_t) / (sqrtf(vv.f) + eps);
// AdamW: decoupled decay first (as Keras and PyTorch do), then Adam.  In the Adam kind D is constant false
#define Y3_ADAMW1(f)                     \
    if (D) pp.f = pp.f - lw * pp.f;      \
    Y3_ADAM1(f)

// EMA: after the step, ema_p += (p_new - ema_p) * omd over the arena and the same update of ema_mv towards the BatchNorm moving
// statistics mv (a second, small segment, written by this step's forward pass), two more fp32 streams per element.
// SCALED: the gradient operand is g * *scale_dev, one fp32 multiply in front of the update text; s = 1 gives the unscaled bits
// (gradient accumulation and global-norm clipping).
template <int KIND, bool EMA, bool SCALED>
__global__ void __launch_bounds__(256)
optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t count4, size_t count,
             const float* __restrict__ hyper_dev, float mu, float wd, float b1, float b2, float eps, const OptimRanges tab, int nb,
             float* __restrict__ ema_p, const float* __restrict__ mv, float* __restrict__ ema_mv, size_t mcount4, size_t mcount,
             const float* __restrict__ omd_dev, const float* __restrict__ scale_dev) {
    constexpr bool ADAMW = KIND == Y3_OPT_ADAMW;
    constexpr bool HAS_V = ADAMW || KIND == Y3_OPT_ADAM_PRIVATE;     // the second-moment arena and the text of Y3_ADAM1
    constexpr bool DECAY = KIND != Y3_OPT_ADAM_PRIVATE;              // Adam: no boundaries, no LDS, no barrier, no cursor
    // the boundaries in LDS, closed by a sentinel so that the cursor below needs no bound of its own
    __shared__ unsigned sb[2 * Y3_OPT_MAX_RANGES + 1];
    if constexpr (DECAY) {
        sb[threadIdx.x] = (int)threadIdx.x < nb ? tab.b[threadIdx.x] : Y3_OPT_NO_BOUNDARY;
        if (threadIdx.x == 0) sb[2 * Y3_OPT_MAX_RANGES] = Y3_OPT_NO_BOUNDARY;
        __syncthreads();
    }
    const float h0 = hyper_dev[0];                 // lr (SGD) or lr_t (Adam, AdamW)
    const float lr_t = h0;                         // the name Y3_ADAM1 reads
    float lw = 0.f;                                // lr * weight_decay
    if constexpr (ADAMW) lw = hyper_dev[1];        // AdamW alone: the lr_t_dev of y3_adam_step* is ONE float
    const float omd = EMA ? *omd_dev : 0.f;
    const float s = SCALED ? *scale_dev : 1.f;
    const float o1 = 1.f - b1, o2 = 1.f - b2;
    (void)lr_t, (void)lw, (void)omd, (void)s, (void)o1, (void)o2;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // a thread's float4 indices only grow, so a cursor over the boundaries serves all its iterations: it advances at most
    // 2 * n_ranges times over the whole loop, and an iteration that crosses no boundary costs one LDS read
    unsigned cur = 0;
    (void)cur;
    for (size_t i = tid; i < count4; i += stride) {
        bool D = false;
        if constexpr (DECAY) {
            while (sb[cur] <= (unsigned)i) ++cur;
            D = cur & 1;
        }
        float4 pp = reinterpret_cast<float4*>(p)[i];
        float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv, ee;
        if constexpr (HAS_V) vv = reinterpret_cast<float4*>(v)[i];
        if constexpr (EMA) ee = reinterpret_cast<float4*>(ema_p)[i];
        if constexpr (SCALED) gg.x *= s, gg.y *= s, gg.z *= s, gg.w *= s;
        if constexpr (HAS_V) {
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
        if constexpr (HAS_V) reinterpret_cast<float4*>(v)[i] = vv;
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
        bool D = false;
        if constexpr (DECAY) {
            unsigned c = 0;
            while (sb[c] <= (unsigned)count4) ++c;
            D = c & 1;
        }
        float4 pp, gg, mm, vv;
        pp.x = p[i], gg.x = g[i], mm.x = m[i];
        if constexpr (HAS_V) vv.x = v[i];
        if constexpr (SCALED) gg.x *= s;
        if constexpr (HAS_V) {
            Y3_ADAMW1(x)
        } else {
            Y3_SGD1(x)
        }
        p[i] = pp.x;
        m[i] = mm.x;
        if constexpr (HAS_V) v[i] = vv.x;
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

// The checks every kind shares, the choice of the instantiation and the launch.  kind: Y3_OPT_* or Y3_OPT_ADAM_PRIVATE, checked by
// the caller; ema, scaled: the form the entry point `who` asks for, whose pointers must then be there.
static int optim_run(const char* who, int kind, bool ema, bool scaled, const y3_optim_desc* d, const OptimRanges& tab, y3_stream_t stream) {
    const bool has_v = kind == Y3_OPT_ADAMW || kind == Y3_OPT_ADAM_PRIVATE;
    Y3_CHECK_ARG(d->param && d->grad && d->m && d->hyper_dev && (!has_v || d->v) && (!ema || (d->ema_param && d->omd_dev)) &&
                     (!scaled || d->scale_dev),
                 "%s: null pointer", who);
    Y3_CHECK_ARG(!ema || d->moving_count == 0 || (d->moving && d->ema_moving), "%s: null moving-statistics pointer", who);
    Y3_CHECK_ARG((((uintptr_t)d->param | (uintptr_t)d->grad | (uintptr_t)d->m | (uintptr_t)d->v | (uintptr_t)d->ema_param | (uintptr_t)d->moving |
                   (uintptr_t)d->ema_moving) & 15) == 0,
                 "%s: arenas must be 16-byte aligned", who);
    // nothing to do.  With no parameters the Adam entry points still average the moving statistics; y3_optim_step never has
    if (d->count == 0 && (kind != Y3_OPT_ADAM_PRIVATE || !ema || d->moving_count == 0)) return Y3_OK;
    const hipStream_t st = (hipStream_t)stream;
#define Y3_OPT_CASE(K)                                                     \
    case K:                                                                \
        if (ema && scaled) optim_launch<K, true, true>(d, tab, st);        \
        else if (ema) optim_launch<K, true, false>(d, tab, st);            \
        else if (scaled) optim_launch<K, false, true>(d, tab, st);         \
        else optim_launch<K, false, false>(d, tab, st);                    \
        break;
    switch (kind) {
        Y3_OPT_CASE(Y3_OPT_SGD)
        Y3_OPT_CASE(Y3_OPT_SGD_NESTEROV)
        Y3_OPT_CASE(Y3_OPT_ADAMW)
        Y3_OPT_CASE(Y3_OPT_ADAM_PRIVATE)
    }
#undef Y3_OPT_CASE
    Y3_CHECK_LAUNCH(who);
    return Y3_OK;
}

extern "C" int y3_optim_step(const y3_optim_desc* d, y3_stream_t stream) {
    Y3_CHECK_ARG(d, "optim_step: null descriptor");
    Y3_CHECK_ARG(d->kind == Y3_OPT_SGD || d->kind == Y3_OPT_SGD_NESTEROV || d->kind == Y3_OPT_ADAMW, "optim_step: unknown kind %d", d->kind);
    Y3_CHECK_ARG(d->kind != Y3_OPT_ADAMW || d->v, "optim_step: AdamW needs the second-moment arena v (null pointer)");
    const bool ema = d->ema_param || d->moving || d->ema_moving || d->omd_dev || d->moving_count;
    Y3_CHECK_ARG(!ema || (d->ema_param && d->omd_dev && (d->moving_count == 0 || (d->moving && d->ema_moving))),
                 "optim_step: partial set of EMA pointers (ema_param, omd_dev, and moving / ema_moving with moving_count, or none)");
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
    return optim_run("optim_step", d->kind, ema, d->scale_dev != nullptr, d, tab, stream);
}

// The four Adam entry points: a descriptor of the private kind.  Unlike y3_optim_step, which takes the form from the pointers
// it is given, each of them states its form, so a null ema_param, omd_dev or scale_dev is an error there.
static int adam_run(const char* who, bool ema, bool scaled, float* param, const float* grad, float* m, float* v, size_t count,
                    const float* lr_t_dev, float beta1, float beta2, float eps, float* ema_param, const float* moving, float* ema_moving,
                    size_t moving_count, const float* omd_dev, const float* scale_dev, y3_stream_t stream) {
    y3_optim_desc d = {};
    d.kind = Y3_OPT_ADAM_PRIVATE;
    d.param = param, d.grad = grad, d.m = m, d.v = v, d.count = count;
    d.hyper_dev = lr_t_dev;
    d.beta1 = beta1, d.beta2 = beta2, d.eps = eps;
    d.ema_param = ema_param, d.moving = moving, d.ema_moving = ema_moving, d.moving_count = moving_count, d.omd_dev = omd_dev;
    d.scale_dev = scale_dev;
    return optim_run(who, d.kind, ema, scaled, &d, OptimRanges(), stream);      // the table: unread by this kind
}
extern "C" int y3_adam_step(float* param, const float* grad, float* m, float* v, size_t count, const float* lr_t_dev, float beta1, float beta2,
                            float eps, y3_stream_t stream) {
    return adam_run("adam_step", false, false, param, grad, m, v, count, lr_t_dev, beta1, beta2, eps, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                    stream);
}
extern "C" int y3_adam_step_scaled(float* param, const float* grad, float* m, float* v, size_t count, const float* lr_t_dev, float beta1,
                                   float beta2, float eps, const float* scale_dev, y3_stream_t stream) {
    return adam_run("adam_step_scaled", false, true, param, grad, m, v, count, lr_t_dev, beta1, beta2, eps, nullptr, nullptr, nullptr, 0, nullptr,
                    scale_dev, stream);
}
extern "C" int y3_adam_step_ema(float* param, const float* grad, float* m, float* v, size_t count, const float* lr_t_dev, float beta1,
                                float beta2, float eps, float* ema_param, const float* moving, float* ema_moving, size_t moving_count,
                                const float* omd_dev, y3_stream_t stream) {
    return adam_run("adam_step_ema", true, false, param, grad, m, v, count, lr_t_dev, beta1, beta2, eps, ema_param, moving, ema_moving,
                    moving_count, omd_dev, nullptr, stream);
}
extern "C" int y3_adam_step_ema_scaled(float* param, const float* grad, float* m, float* v, size_t count, const float* lr_t_dev, float beta1,
                                       float beta2, float eps, float* ema_param, const float* moving, float* ema_moving, size_t moving_count,
                                       const float* omd_dev, const float* scale_dev, y3_stream_t stream) {
    return adam_run("adam_step_ema_scaled", true, true, param, grad, m, v, count, lr_t_dev, beta1, beta2, eps, ema_param, moving, ema_moving,
                    moving_count, omd_dev, scale_dev, stream);
}

// ---------------------------------------------------------------------------
// Gradient accumulation and the global gradient norm, over the whole gradient arena
// ---------------------------------------------------------------------------
// ACC: acc = *first_dev ? g : acc + g (plain fp32; the first micro-step does not read acc), and the block's sum of squares of the
// RESULT.  !ACC: the sum of squares of g alone.  Squares and sums in fp64 (an fp32 x fp32 product is exact there); a thread adds
// its elements in loop order, the block a fixed LDS tree, and EVERY block writes its partial, so nothing needs zeroing and the
// bits do not depend on the run.  `first` comes from device memory so a replayed graph serves every micro-step.
#define Y3_GN_SQ(f) q += (double)aa.f * (double)aa.f;
template <bool ACC>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(float* __restrict__ acc, const float* __restrict__ g, size_t count4, size_t count,
                                                         const int* __restrict__ first_dev, double* __restrict__ partials) {
    __shared__ double sm[256];
    bool first = true;
    if constexpr (ACC) first = *first_dev != 0;
    double q = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count4; i += stride) {
        float4 aa = reinterpret_cast<const float4*>(g)[i];
        if constexpr (ACC) {
            if (!first) {
                const float4 gg = aa;
                aa = reinterpret_cast<float4*>(acc)[i];
                aa.x += gg.x, aa.y += gg.y, aa.z += gg.z, aa.w += gg.w;
            }
            reinterpret_cast<float4*>(acc)[i] = aa;
        }
        Y3_GN_SQ(x) Y3_GN_SQ(y) Y3_GN_SQ(z) Y3_GN_SQ(w)
    }
    // tail: lane x of a float4 through the same text
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) {
        const size_t i = (count4 << 2) + threadIdx.x;
        float4 aa;
        aa.x = g[i];
        if constexpr (ACC) {
            if (!first) {
                const float gx = aa.x;
                aa.x = acc[i];
                aa.x += gx;
            }
            acc[i] = aa.x;
        }
        Y3_GN_SQ(x)
    }
    sm[threadIdx.x] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = sm[0];
}
// One workgroup: the partials staged in LDS, added by one lane in index order; norm = sqrt(S) / k and
// s = (1/k) * (clip / max(norm, clip)) (1/k with clipping off) in fp64, each rounded once to fp32.
#define Y3_GN_MAX_BLOCKS 2048      // the cap of stream_blocks today; y3_grad_clip_scale refuses more partials than this LDS array holds
__global__ __launch_bounds__(256) void grad_clip_scale_kernel(const double* __restrict__ partials, int nblocks, int k, double clip, int clip_on,
                                                              float* __restrict__ norm_dev, float* __restrict__ scale_dev) {
    __shared__ double sm[Y3_GN_MAX_BLOCKS];
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) sm[b] = partials[b];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double S = 0.0;
    for (int b = 0; b < nblocks; ++b) S += sm[b];
    const double norm = sqrt(S) / (double)k;
    double s = 1.0 / (double)k;
    if (clip_on) s = s * (clip / (norm > clip ? norm : clip));
    *norm_dev = (float)norm;
    *scale_dev = (float)s;
}
static inline int grad_norm_blocks(size_t count) { return stream_blocks((long long)(count / 4 + 1), 256); }
extern "C" size_t y3_grad_norm_workspace_bytes(size_t count) { return (size_t)grad_norm_blocks(count) * sizeof(double); }
extern "C" int y3_grad_accumulate(float* acc, const float* grad, size_t count, const int* first_dev, void* workspace, y3_stream_t stream) {
    Y3_CHECK_ARG(acc && grad && first_dev && workspace, "grad_accumulate: null pointer");
    Y3_CHECK_ARG((((uintptr_t)acc | (uintptr_t)grad) & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
                 "grad_accumulate: arenas must be 16-byte aligned, the workspace 8-byte");
    hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(grad_norm_blocks(count)), dim3(256), 0, (hipStream_t)stream, acc, grad, count / 4, count,
                       first_dev, (double*)workspace);
    Y3_CHECK_LAUNCH("grad_accumulate");
    return Y3_OK;
}
extern "C" int y3_grad_sumsq(const float* grad, size_t count, void* workspace, y3_stream_t stream) {
    Y3_CHECK_ARG(grad && workspace, "grad_sumsq: null pointer");
    Y3_CHECK_ARG(((uintptr_t)grad & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
                 "grad_sumsq: the arena must be 16-byte aligned, the workspace 8-byte");
    hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(grad_norm_blocks(count)), dim3(256), 0, (hipStream_t)stream, (float*)nullptr, grad,
                       count / 4, count, (const int*)nullptr, (double*)workspace);
    Y3_CHECK_LAUNCH("grad_sumsq");
    return Y3_OK;
}
extern "C" int y3_grad_clip_scale(const void* workspace, size_t count, int accumulate_steps, double clip_norm, float* norm_dev,
                                  float* scale_dev, y3_stream_t stream) {
    Y3_CHECK_ARG(workspace && norm_dev && scale_dev, "grad_clip_scale: null pointer");
    Y3_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "grad_clip_scale: the workspace must be 8-byte aligned");
    Y3_CHECK_ARG(accumulate_steps >= 1, "grad_clip_scale: accumulate_steps %d (needs >= 1)", accumulate_steps);
    const bool off = clip_norm == Y3_GRAD_CLIP_OFF;      // +infinity: no bound
    Y3_CHECK_ARG(off || (clip_norm > 0.0 && clip_norm < Y3_GRAD_CLIP_OFF), "grad_clip_scale: clip_norm %g (needs finite > 0, or Y3_GRAD_CLIP_OFF)",
                 clip_norm);
    Y3_CHECK_ARG(grad_norm_blocks(count) <= Y3_GN_MAX_BLOCKS, "grad_clip_scale: %d partial sums (the finalize kernel holds %d)",
                 grad_norm_blocks(count), Y3_GN_MAX_BLOCKS);
    hipLaunchKernelGGL(grad_clip_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, grad_norm_blocks(count),
                       accumulate_steps, off ? 1.0 : clip_norm, off ? 0 : 1, norm_dev, scale_dev);
    Y3_CHECK_LAUNCH("grad_clip_scale");
    return Y3_OK;
}
