// Host-side helpers of libyolo3hip.so that need no HIP header: the error channel, argument checks and integer arithmetic.
#pragma once
#include <stdio.h>
#include "../../include/yolo3hip.h"

void y3_set_error(const char* fmt, ...);

#define Y3_CHECK_ARG(cond, ...)          \
    do {                                 \
        if (!(cond)) {                   \
            y3_set_error(__VA_ARGS__);   \
            return Y3_EINVAL;            \
        }                                \
    } while (0)

// A checked test-time augmentation view list as a kernel argument (tta.hip; the tile gather of pointwise.hip writes views too)
struct TtaViews {
    int k;
    int code[Y3_TTA_MAX_VIEWS];
};
// 1 .. Y3_TTA_MAX_VIEWS distinct codes 0 .. 7, a transposing one only for h == w: Y3_EINVAL + message otherwise (tta.hip)
int y3_tta_check_views(const int* views, int k, int h, int w, const char* what, TtaViews* out);

static inline int y3_ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
static inline bool y3_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int y3_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// TF padding='same': pad_before for one spatial axis
static inline int y3_same_pad_before(int size, int k, int s) {
    int out = (size + s - 1) / s;
    int total = (out - 1) * s + k - size;
    if (total < 0) total = 0;
    return total / 2;
}

// x / d for 0 <= x < 2^31 without a divide: the compiler's sequence for a run-time divisor is ~30 dependent instructions
// (float reciprocal + two correction steps), and the index decode of a workgroup needs five of them before its first load.
//   d == 1: mul == 0 (identity);  d == 2^k: shift = k - 1, mul = 2^31 + 1;  else shift = floor(log2 d), mul = floor(2^(32+shift) / d) + 1
// (error term mul * d - 2^(32+shift) <= d, so floor is exact while x * d < 2^(32+shift), i.e. for every x < 2^31).
struct Y3Div {
    unsigned mul;
    int shift;
};
static inline Y3Div y3_make_div(int d) {
    Y3Div r = {0u, 0};
    if (d <= 1) return r;
    int s = 0;
    while ((2LL << s) <= d) ++s;      // floor(log2 d)
    if ((1LL << s) == d) {
        r.shift = s - 1;
        r.mul = 0x80000001u;
    } else {
        r.shift = s;
        r.mul = (unsigned)(((1ULL << (32 + s)) / (unsigned long long)d) + 1ULL);
    }
    return r;
}
