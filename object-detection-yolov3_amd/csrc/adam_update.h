// The Adam update of one element, shared by pointwise.hip (adam_kernel, adam_ema_kernel and their scaled forms) and optim.hip
// (the AdamW kernels): one text, so all give the same bits.
#pragma once

// one element of one float4 lane f; the caller has pp, gg, mm, vv (float4) and o1 = 1 - b1, o2 = 1 - b2, lr_t, eps in scope
#define Y3_ADAM1(f)                              \
    mm.f += (gg.f - mm.f) * o1;                  \
    vv.f += (gg.f * gg.f - vv.f) * o2;           \
    pp.f -= (mm.f * lr_t) / (sqrtf(vv.f) + eps);
