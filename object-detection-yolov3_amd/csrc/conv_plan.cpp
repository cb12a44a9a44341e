// The launch planners of the convolutions: which kernel runs, on which tile, cut how along K, with how much workspace -- decided
// from shapes alone (no pointer is read, no HIP function is called).  The plan queries answer from these descriptions; conv.hip issues them.
#include <stdlib.h>
#include "host.h"
#include "conv_plan.h"

// Tile choice from a measured sweep over the tile sizes (MI355X): a launch wants >= ~600 workgroups
// (256 CUs x 2-3 resident); prefer the largest tile that still gives that many, else 64x64 (+ split-K).
static TileCfg pick_tile(int M, int Nout) {
    TileCfg t;
    if (Nout <= 32)
        t = {128, 32, 16};
    else if (Nout <= 64)
        t = {128, 64, 16};
    else {
        const long long t128 = (long long)y3_cdiv(M, 128) * y3_cdiv(Nout, 128);
        const long long t64x128 = (long long)y3_cdiv(M, 64) * y3_cdiv(Nout, 128);
        if (t128 >= 600)
            t = {128, 128, 16};
        else if (t64x128 >= 600)
            t = {64, 128, 16};
        else
            t = {64, 64, 16};
    }
    return t;
}
// No tile is cut: every tile is one slice of `chunk` K steps, and the launch needs no slabs.  Where the planners start, and what
// a plan falls back to when its slabs have no room.
void whole_tiles(ConvPlan& pl, int chunk) {
    pl.f = pl.tiles;
    pl.s0 = pl.s1 = 1;
    pl.chunk0 = pl.chunk1 = chunk;
    pl.ws_bytes = 0;
}
// The end of both planners: the workspace a split plan needs (ticket header + one slab per slice of a cut tile).  Slab offsets
// are 32-bit buffer offsets: a plan whose slabs would not fit them falls back to whole tiles of `whole_chunk` steps.
static void size_slabs(ConvPlan& pl, int whole_chunk) {
    const long long split_items = pl.s0 > 1 ? (long long)pl.f * pl.s0 + (long long)(pl.tiles - pl.f) * pl.s1 : (pl.s1 > 1 ? (long long)(pl.tiles - pl.f) * pl.s1 : 0);
    const long long slab_bytes = split_items * pl.t.bm * pl.t.bn * 4;
    if (slab_bytes >= 0x7ff00000LL)
        whole_tiles(pl, whole_chunk);
    else
        pl.ws_bytes = split_items > 0 ? (size_t)Y3_WS_HEADER + (size_t)slab_bytes : 0;
}
// The caller's workspace cannot hold the `need` bytes of a split plan (the launch then runs whole_tiles)
bool no_room(size_t need, const void* workspace, size_t workspace_bytes) {
    return need > 0 && (workspace == nullptr || workspace_bytes < need);
}
// The x3 kernels (conv_x3.hip): 128 x 128 tiles (128 x 64 for <= 64 output columns), two to three workgroups per CU.  Every
// launch of the layers they are used for is cut along K into slices of >= 12 K steps so that ~700 workgroups share the work
// evenly -- 2.7 per CU, dealt out as slots free up -- e.g. 338 tiles x 2, 172 x 4, 88 x 8 slices of 36 steps for the 3x3 layers
// of the 52 / 26 / 13 grids at batch 8.
static bool x3_shape_ok(int C, int Nout, int K, int ntaps) {
    return C % 16 == 0 && K % 16 == 0 && (ntaps == 1 || y3_is_pow2(C)) && Nout >= 32 && K / 16 >= 2;
}
static ConvPlan plan_conv_x3(int M, int Nout, int K, int ntaps) {
    ConvPlan pl;
    pl.t = {128, Nout <= 64 ? 64 : 128, 16};
    const int tiles = y3_cdiv(M, pl.t.bm) * y3_cdiv(Nout, pl.t.bn);
    const int nk = K / 16;
    pl.tiles = tiles;
    whole_tiles(pl, even_steps(nk));
    constexpr int min_steps = 12;
    // slices are whole units of K steps: 3x3 launches in units of 18 (two 16-channel chunks of nine taps: the patch kernel's loop
    // body, conv_x3.hip), the others in pairs of steps
    const int unit = ntaps == 9 ? 18 : 2;
    if (tiles <= Y3_MAX_TICKETS && tiles > 256) {
        // more tiles than CUs but too few to balance by themselves (338 tiles: a third of the CUs would carry two): whole rounds of
        // tiles stay whole -- no slabs for them -- and only the remainder round is cut, so that its pieces spread evenly
        const int F = tiles / 256 * 256, R = tiles - F;
        int best = 1;
        double best_cost = 1.0;
        for (int S = 2; S <= 6; ++S) {
            const int ch = y3_cdiv(y3_cdiv(nk, S), unit) * unit;
            if (ch * S != nk || ch < min_steps) continue;             // equal slices only
            const double cost = (double)y3_cdiv((long long)R * S, 256) / S + 0.03 * (S - 1);
            if (cost < best_cost - 1e-9) {
                best_cost = cost;
                best = S;
            }
        }
        if (R > 0 && best > 1) {
            pl.f = F;
            pl.chunk1 = nk / best;
            pl.s1 = best;
        }
    } else if (tiles <= Y3_MAX_TICKETS && tiles <= 256) {
        // Fewer tiles than CUs: cut along K so that the launch fills the chip's workgroup slots ONCE, two per CU -- a lone workgroup
        // (one wave per SIMD) runs its loop at a third of the MFMA rate, and a second, partly filled round costs a whole round
        // (measured with a K-slice sweep: 507 pieces 78 us, 338 pieces 97 us, 676 pieces 103 us on the same launch).
        // The slice counts a launch can have are ceil(nk / c) for c a multiple of the unit; take the largest count s_lo with
        // tiles * s_lo <= slots and give the next larger one, s_hi, to as many tiles as fill the rest of the slots.
        auto count_for = [&](int c) { return y3_cdiv(nk, c); };
        int c_lo = 0, c_hi = 0;      // chunk lengths of the counts s_lo <= slots / tiles < s_hi
        for (int c = y3_cdiv(nk, unit) * unit; c >= unit && c >= min_steps; c -= unit) {      // slice counts grow as c shrinks
            const int sc = count_for(c);
            if (sc > 16) break;
            if ((long long)tiles * sc <= x3_slots)
                c_lo = c;
            else if (c_hi == 0 && (c_lo == 0 || sc > count_for(c_lo)))
                c_hi = c;
        }
        const int s_lo = c_lo > 0 ? count_for(c_lo) : 1;
        if (s_lo > 1) {
            pl.s0 = pl.s1 = s_lo;
            pl.chunk0 = pl.chunk1 = c_lo;
        }
        // Overflow by SHORT slices: when the next larger count leaves a last slice of at most a third of the others, every tile
        // takes that count although the launch then has a few blocks more than slots: the items are dealt so that every XCD's
        // blocks END with short slices (conv_fast_decode<SHORTLAST>), i.e. the blocks beyond the slots are short ones that start as
        // the first short ones finish -- and no tile needs the longer slices of s_lo (13x13 forward: 88 x 6 = 528 pieces of 54 / 18
        // steps instead of 80 x 6 + 8 x 4 with 72-step pieces: 92 -> 82 us).
        if (c_hi > 0 && ntaps == 9) {
            const int s_hi = count_for(c_hi), last = nk - (s_hi - 1) * c_hi;
            if ((long long)tiles * s_hi <= x3_slots + x3_slots / 16 && 3 * last <= c_hi) {
                pl.f = tiles;
                pl.s0 = pl.s1 = s_hi;
                pl.chunk0 = pl.chunk1 = c_hi;
                pl.short_last = 1;
                c_hi = 0;
            }
        }
        if (c_hi > 0) {      // tiles [0, f) take the next larger count: f * s_hi + (tiles - f) * s_lo <= slots
            const int s_hi = count_for(c_hi);
            const int f = (int)((x3_slots - (long long)tiles * s_lo) / (s_hi - s_lo));
            if (f > 0) {
                pl.f = f < tiles ? f : tiles;
                pl.s0 = s_hi;
                pl.chunk0 = c_hi;
            }
        }
    }
    pl.stats_tiles = y3_cdiv(M, pl.t.bm);
    size_slabs(pl, even_steps(nk));
    return pl;
}
// fast_ok: the launch qualifies for conv_igemm_fast_kernel (the only kernel with split-K)
static ConvPlan plan_conv(int M, int Nout, int K, bool fast_ok) {
    ConvPlan pl;
    pl.t = pick_tile(M, Nout);
    const int tiles = y3_cdiv(M, pl.t.bm) * y3_cdiv(Nout, pl.t.bn);
    const int nk = K / pl.t.bk;                                   // K steps (fast path: K % bk == 0)
    const int whole = nk > 0 ? nk : 1;
    pl.tiles = tiles;
    whole_tiles(pl, whole);
    constexpr int want = 2000;    // workgroups to aim for (swept with tools/fwd_time.py: 1000 / 1400 / 2000 / 2800)
    constexpr int min_k = 256;    // shortest K slice worth a launch
    constexpr int cus = 256;
    // measured (tools/fixed_cost.py, layer_times.py): a 676-tile launch (2.6 workgroups per CU) is better left whole unless
    // K is long; at <= 512 tiles the extra workgroups win over the slab round trip
    constexpr int few_max = 512;
    const bool few_tiles = tiles <= few_max || ((long long)tiles * 2 <= want && K >= 2048);
    if (fast_ok && tiles <= Y3_MAX_TICKETS && few_tiles && K >= 2 * min_k) {
        int ks = (int)((want + tiles / 2) / tiles);
        const int maxs = K / min_k;
        if (ks > maxs) ks = maxs;
        if (ks > 16) ks = 16;
        if (ks > 1) {
            pl.chunk0 = even_steps(y3_cdiv(nk, ks));
            pl.s0 = y3_cdiv(nk, pl.chunk0);
        }
    } else if (fast_ok && tiles <= Y3_MAX_TICKETS && tiles > cus && nk >= 8) {
        // whole rounds of tiles stay whole; the remainder round is cut along K so that its pieces spread evenly over the CUs:
        // load per CU = full rounds + ceil(R * S / CUs) / S tiles against tiles / CUs ideal
        const int F = tiles / cus * cus, R = tiles - F;
        if (R > 0) {
            int best = 1;
            double best_cost = 1.0;
            for (int S = 2; S <= 6 && S * 4 <= nk; ++S) {
                const double cost = (double)y3_cdiv((long long)R * S, cus) / S + 0.03 * (S - 1);
                if (cost < best_cost - 1e-9) {
                    best_cost = cost;
                    best = S;
                }
            }
            if (best > 1) {
                pl.f = F;
                pl.chunk1 = even_steps(y3_cdiv(nk, best));
                pl.s1 = y3_cdiv(nk, pl.chunk1);
            }
        }
    }
    pl.stats_tiles = y3_cdiv(M, pl.t.bm);
    size_slabs(pl, whole);
    return pl;
}
static bool fast_shape_ok(int C, int Nout, int K, int ntaps) {
    return !getenv("Y3_NO_FAST") && C % 16 == 0 && K % 16 == 0 && (ntaps == 1 || y3_is_pow2(C));
}
static GemmDesc describe_gemm(int M, int C, int ntaps, int Nout, unsigned flags) {
    GemmDesc d;
    const int K = ntaps * C;
    d.x3 = (flags & Y3_CONV_X3) && x3_shape_ok(C, Nout, K, ntaps);
    d.fast = d.x3 || fast_shape_ok(C, Nout, K, ntaps);
    d.pl = d.x3 ? plan_conv_x3(M, Nout, K, ntaps) : plan_conv(M, Nout, K, d.fast);
    return d;
}

extern "C" int y3_conv2d_x3_ok(int m, int c, int ntaps, int nout) {
    return (m > 0 && (ntaps == 1 || ntaps == 9 || ntaps == 2 || ntaps == 4) && x3_shape_ok(c, nout, ntaps * c, ntaps)) ? 1 : 0;
}
extern "C" int y3_conv2d_stats_tiles_x(int m, int cin, int ksize, int cout, unsigned flags) {
    return describe_gemm(m, cin, ksize * ksize, cout, flags).pl.stats_tiles;
}
extern "C" size_t y3_conv2d_fwd_workspace_x(int m, int cin, int ksize, int cout, unsigned flags) {
    return describe_gemm(m, cin, ksize * ksize, cout, flags).pl.ws_bytes;
}
extern "C" int y3_conv2d_stats_tiles(int m, int cin, int ksize, int cout) { return y3_conv2d_stats_tiles_x(m, cin, ksize, cout, 0u); }
extern "C" size_t y3_conv2d_fwd_workspace(int m, int cin, int ksize, int cout) { return y3_conv2d_fwd_workspace_x(m, cin, ksize, cout, 0u); }

// Diagnostics (include/yolo3hip.h): the plan behind y3_conv2d_fwd / stride-1 y3_conv2d_dgrad for an M x cout x (ksize^2 cin) GEMM
extern "C" size_t y3_conv2d_plan(int m, int cin, int ksize, int cout, int* out13) { return y3_conv2d_plan_x(m, cin, ksize, cout, 0u, out13); }
extern "C" size_t y3_conv2d_plan_x(int m, int cin, int ksize, int cout, unsigned flags, int* out13) {
    const GemmDesc d = describe_gemm(m, cin, ksize * ksize, cout, flags);
    const ConvPlan& pl = d.pl;
    if (out13) {
        const int v[13] = {pl.t.bm, pl.t.bn, pl.t.bk, pl.tiles, pl.f, pl.s0, pl.s1, pl.chunk0, pl.chunk1,
                           pl.f * pl.s0 + (pl.tiles - pl.f) * pl.s1, pl.stats_tiles, (d.fast ? 1 : 0) | (pl.short_last ? 2 : 0), ksize * ksize * cin / pl.t.bk};
        for (int i = 0; i < 13; ++i) out13[i] = v[i];
    }
    return pl.ws_bytes;
}

// Geometry only (no data pointer is read); false if the launch does not qualify for the fast kernels: 2 GiB buffer limits, tap grid.
bool fast_geom(const ConvArgs& a, int ntaps, int bk, FastGeom* g) {
    // Nout need not be a multiple of 4 (the detection heads): a weight-row load that runs past column Nout - 1 picks up the
    // head of the next row (zeros past the end of the buffer) into accumulator columns >= Nout, which the epilogue never stores
    if (a.C % bk != 0 || a.K % bk != 0) return false;
    if (ntaps > 1 && !y3_is_pow2(a.C)) return false;
    // bias the base pointer by the most negative tap offset so that scalar offsets stay non-negative
    g->min_off = 0;
    for (int t = 0; t < ntaps; ++t) {
        const int code = (int)((a.tap_dhdw >> (4 * t)) & 15ull);
        g->dh[t] = (code & 3) - 1;
        g->dw[t] = (code >> 2) - 1;
        const int off = (g->dh[t] * a.W + g->dw[t]) * a.src_ld;
        if (off < g->min_off) g->min_off = off;
    }
    const long long total = (long long)a.src_n * a.H * a.W * a.src_ld - g->min_off;
    const long long wtotal = (long long)(a.wt_rows) * a.Nout;
    // x3: three bf16 piece planes of the K-contiguous copy (y3_x3_split_weights): 6 bytes per element, same 2 GiB limit
    if (total * 4 >= 0x7fffffffLL || wtotal * (a.x3 ? 6 : 4) >= 0x7fffffffLL) return false;
    g->src_bytes = (unsigned)(total * 4);
    g->wt_bytes = (unsigned)(wtotal * (a.x3 ? 6 : 4));
    for (int t = 0; t < ntaps; ++t) {
        g->off[t] = ((g->dh[t] * a.W + g->dw[t]) * a.src_ld - g->min_off) * 4;
        g->wrow[t] = (int)((a.tap_wsel >> (4 * t)) & 15ull) * a.C;
    }
    // the tap list as a (rows x nx) grid: nx = length of the first run of equal dh
    int nx = 1;
    while (nx < ntaps && g->dh[nx] == g->dh[0]) ++nx;
    if (ntaps % nx != 0 || nx > 3) return false;
    g->nx = nx;
    const int offx = nx > 1 ? g->off[1] - g->off[0] : 0, wx = nx > 1 ? g->wrow[1] - g->wrow[0] : 0;
    const int offy = ntaps > nx ? g->off[nx] - g->off[0] : 0, wy = ntaps > nx ? g->wrow[nx] - g->wrow[0] : 0;
    for (int t = 0; t < ntaps; ++t)
        if (g->off[t] != g->off[0] + (t / nx) * offy + (t % nx) * offx || g->wrow[t] != g->wrow[0] + (t / nx) * wy + (t % nx) * wx)
            return false;   // not a grid: the generic kernel takes it
    const long long dpix = a.dense_dst ? (long long)a.M : (long long)a.src_n * a.DH * a.DW;
    const long long db = dpix * a.dst_ld * 4, rb = dpix * (long long)a.resid_ld * 4;
    if (db >= 0x7fffffffLL || rb >= 0x7fffffffLL) return false;
    g->dst_bytes = (unsigned)db;
    g->resid_bytes = (unsigned)rb;
    return true;
}

GemmDesc describe_gemm(const ConvArgs& a) { return describe_gemm(a.M, a.C, a.K / a.C, a.Nout, a.x3 ? Y3_CONV_X3 : 0u); }

int set_channels(int C, int taps, int* logC, int* cmask) {
    if (taps == 1) {
        *logC = 31;
        *cmask = 0x7fffffff;
        return 0;
    }
    Y3_CHECK_ARG(y3_is_pow2(C) && C >= 4, "3x3 conv needs power-of-two channels >= 4 (got %d)", C);
    *logC = y3_ilog2(C);
    *cmask = C - 1;
    return 0;
}

// f32: whole tiles of one size for all classes
static bool plan_dgrad_multi_f32(const ConvArgs* cls, int ncls, MultiPlan* pl) {
    int mmax = 0;
    for (int c = 0; c < ncls; ++c) mmax = cls[c].M > mmax ? cls[c].M : mmax;
    TileCfg t = pick_tile(mmax * ncls, cls[0].Nout);   // the classes share one grid: size the tile for their sum
    if (t.bm == 128 && t.bn == 128) t.bm = 64;          // launch_fast_multi has no 128 x 128
    pl->rows = 0;
    pl->ws = 0;
    for (int c = 0; c < ncls; ++c) {
        if (!fast_shape_ok(cls[c].C, cls[c].Nout, cls[c].K, cls[c].K / cls[c].C)) return false;
        ConvPlan& q = pl->c[c];
        q.t = t;
        q.stats_tiles = y3_cdiv(cls[c].M, t.bm);
        q.tiles = q.stats_tiles * y3_cdiv(cls[c].Nout, t.bn);
        whole_tiles(q, cls[c].K / t.bk);
        pl->rows += q.stats_tiles;
    }
    return true;
}
// x3 (conv_x3_multi_kernel).  The classes carry 1 / 2 / 2 / 4 taps, i.e. K steps in the ratio 1 : 2 : 2 : 4, and the x3 loop wants
// the launch to fill the 512 workgroup slots once: every class is cut along K into slices of about the same length L -- the
// smallest L for which the launch still fits the slots.
static bool plan_dgrad_multi_x3(const ConvArgs* cls, int ncls, MultiPlan* pl) {
    const int Nout = cls[0].Nout;
    if (Nout < 64) return false;
    const TileCfg t = {128, Nout >= 128 ? 128 : 64, 16};
    int steps[4], tsum = 0, smax = 0;
    long long total = 0;
    pl->rows = 0;
    for (int c = 0; c < ncls; ++c) {
        if (cls[c].Nout != Nout || !x3_shape_ok(cls[c].C, Nout, cls[c].K, cls[c].K / cls[c].C)) return false;
        ConvPlan& q = pl->c[c];
        q.t = t;
        q.stats_tiles = y3_cdiv(cls[c].M, t.bm);
        q.tiles = q.stats_tiles * y3_cdiv(Nout, t.bn);
        steps[c] = cls[c].K / 16;
        whole_tiles(q, even_steps(steps[c]));
        pl->rows += q.stats_tiles;
        tsum += q.tiles;
        total += (long long)q.tiles * steps[c];
        smax = steps[c] > smax ? steps[c] : smax;
    }
    if (tsum < x3_slots && tsum <= Y3_MAX_TICKETS) {
        int L = even_steps(y3_cdiv(total, x3_slots));
        if (L < 12) L = 12;
        for (; L < smax; L += 2) {
            long long g = 0;
            for (int c = 0; c < ncls; ++c) g += (long long)pl->c[c].tiles * y3_cdiv(steps[c], L);
            if (g <= x3_slots) break;
        }
        for (int c = 0; c < ncls; ++c) {
            const int sc = y3_cdiv(steps[c], L);
            if (sc > 1) {
                ConvPlan& q = pl->c[c];
                q.chunk0 = q.chunk1 = even_steps(y3_cdiv(steps[c], sc));
                q.s0 = q.s1 = y3_cdiv(steps[c], q.chunk0);
            }
        }
    }
    size_t slab = 0;
    for (int c = 0; c < ncls; ++c)
        if (pl->c[c].s0 > 1) slab += (size_t)pl->c[c].tiles * pl->c[c].s0 * t.bm * t.bn * 4;
    pl->ws = slab ? (size_t)Y3_WS_HEADER + slab : 0;
    return true;
}
// false if the classes do not qualify for one merged launch (they are then launched one by one)
static bool plan_dgrad_multi(const ConvArgs* cls, int ncls, MultiPlan* pl) {
    if (ncls < 2 || ncls > 4) return false;
    if (!(cls[0].x3 ? plan_dgrad_multi_x3(cls, ncls, pl) : plan_dgrad_multi_f32(cls, ncls, pl))) return false;
    FastGeom g;
    for (int c = 0; c < ncls; ++c)
        if (!fast_geom(cls[c], cls[c].K / cls[c].C, 16, &g)) return false;
    return true;
}

// shapes the x3 data gradient takes: stride 1 as the forward; stride 2 (3x3, the merged launch of the parity classes): >= 64 input
// channels of the layer (output columns of the GEMM), its output channels a power of two
bool dgrad_x3(unsigned flags, const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc) {
    if (!(flags & Y3_CONV_X3) || !ddst || !dsrc) return false;
    if (stride == 1) return x3_shape_ok(ddst->c, dsrc->c, ksize * ksize * ddst->c, ksize * ksize);
    return stride == 2 && ksize == 3 && dsrc->c >= 64 && y3_is_pow2(ddst->c) && x3_shape_ok(ddst->c, dsrc->c, ddst->c, 1);
}
extern "C" int y3_conv2d_dgrad_x3_ok(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc) {
    return dgrad_x3(Y3_CONV_X3, ddst, ksize, stride, dsrc) ? 1 : 0;
}

// Y3_CONV_X3 in `flags` counts where dgrad_x3 takes the shape (the entry points refuse the others before they come here).
int describe_dgrad(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags, DgradDesc* d) {
    Y3_CHECK_ARG(ksize == 1 || ksize == 3, "conv2d_dgrad: ksize %d unsupported", ksize);
    Y3_CHECK_ARG(stride == 1 || stride == 2, "conv2d_dgrad: stride %d unsupported", stride);
    const int OH = (dsrc->h + stride - 1) / stride, OW = (dsrc->w + stride - 1) / stride;
    Y3_CHECK_ARG(ddst->n == dsrc->n && ddst->h == OH && ddst->w == OW, "conv2d_dgrad: geometry mismatch");
    const int pbh = y3_same_pad_before(dsrc->h, ksize, stride), pbw = y3_same_pad_before(dsrc->w, ksize, stride);
    // the contraction runs over (tap, cout): channels of ddst
    ConvArgs base = {};
    base.H = ddst->h;
    base.W = ddst->w;
    base.C = ddst->c;
    base.src_ld = ddst->ld;
    base.dst_ld = dsrc->ld;
    base.Nout = dsrc->c;
    base.flags = flags & ~Y3_CONV_X3;
    base.x3 = dgrad_x3(flags, ddst, ksize, stride, dsrc) ? 1 : 0;
    base.DH = dsrc->h;
    base.DW = dsrc->w;
    base.sh = base.sw = 1;
    base.src_n = ddst->n;
    base.wt_rows = ksize * ksize * ddst->c;
    d->ncls = 0;
    d->rows = 0;
    d->ws_bytes = 0;
    if (stride == 1) {
        ConvArgs& p = d->cls[0];
        p = base;
        d->ncls = 1;
        const int taps = ksize * ksize;
        if (int e = set_channels(ddst->c, taps, &p.logC, &p.cmask)) return e;
        for (int kh = 0; kh < ksize; ++kh)
            for (int kw = 0; kw < ksize; ++kw) {
                const int t = kh * ksize + kw;
                const int dh = pbh - kh, dw = pbw - kw;  // dsrc[i] += ddst[i + pad - k] * w[k]
                p.tap_dhdw |= (unsigned long long)((dh + 1) | ((dw + 1) << 2)) << (4 * t);
                p.tap_wsel |= (unsigned long long)t << (4 * t);
            }
        p.OH = dsrc->h;
        p.OW = dsrc->w;
        p.dsh = p.dsw = 1;
        p.dense_dst = 1;
        p.K = taps * ddst->c;
        p.M = dsrc->n * p.OH * p.OW;
        d->how = DGRAD_SINGLE;
        d->g[0] = describe_gemm(p);
        d->ws_bytes = d->g[0].pl.ws_bytes;
        // the statistics live in the dense fast kernels: the launch itself must take them too (2 GiB buffer limits, tap grid)
        FastGeom fg;
        if (d->g[0].fast && d->g[0].pl.t.bk == 16 && fast_geom(p, taps, 16, &fg)) d->rows = d->g[0].pl.stats_tiles;
        return Y3_OK;
    }
    // stride 2: forward out o reads in[2o + k - pad]; input pixel i = 2q + par receives from the taps with
    // (par + pad - k) even, at o = q + (par + pad - k)/2.  One class per (row parity, col parity).
    ConvArgs* cls = d->cls;
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            ConvArgs p = base;
            int nt = 0;
            for (int kh = 0; kh < ksize; ++kh) {
                if ((ph + pbh - kh) & 1) continue;
                for (int kw = 0; kw < ksize; ++kw) {
                    if ((pw + pbw - kw) & 1) continue;
                    const int dh = (ph + pbh - kh) / 2, dw = (pw + pbw - kw) / 2;  // exact: numerator even (may be negative)
                    Y3_CHECK_ARG(dh >= -1 && dh <= 2 && dw >= -1 && dw <= 2, "conv2d_dgrad: tap offset out of range");
                    p.tap_dhdw |= (unsigned long long)((dh + 1) | ((dw + 1) << 2)) << (4 * nt);
                    p.tap_wsel |= (unsigned long long)(kh * ksize + kw) << (4 * nt);
                    ++nt;
                }
            }
            p.OH = (dsrc->h - ph + 1) / 2;
            p.OW = (dsrc->w - pw + 1) / 2;
            if (p.OH <= 0 || p.OW <= 0) continue;
            p.dsh = p.dsw = 2;
            p.doh = ph;
            p.dow = pw;
            p.dense_dst = 0;
            p.M = dsrc->n * p.OH * p.OW;
            // no tap reaches this parity class (1x1 stride 2): gradient is zero there
            Y3_CHECK_ARG(nt > 0, "conv2d_dgrad: 1x1 stride-2 not supported");
            if (int e = set_channels(ddst->c, nt == 1 ? 1 : 9, &p.logC, &p.cmask)) return e;   // single tap: plain k = c (no power-of-two requirement)
            p.K = nt * ddst->c;
            cls[d->ncls++] = p;
        }
    // longest contraction first, so that the 4-tap workgroups of a merged launch start before the 1-tap ones
    for (int i = 1; i < d->ncls; ++i)
        for (int j = i; j > 0 && cls[j].K > cls[j - 1].K; --j) {
            const ConvArgs tmp = cls[j];
            cls[j] = cls[j - 1];
            cls[j - 1] = tmp;
        }
    if (plan_dgrad_multi(cls, d->ncls, &d->multi)) {
        d->how = base.x3 ? DGRAD_MERGED_X3 : DGRAD_MERGED_F32;
        d->rows = d->multi.rows;
        d->ws_bytes = d->multi.ws;
        return Y3_OK;
    }
    d->how = DGRAD_BY_CLASS;
    for (int c = 0; c < d->ncls; ++c) {
        d->g[c] = describe_gemm(cls[c]);
        if (d->g[c].pl.ws_bytes > d->ws_bytes) d->ws_bytes = d->g[c].pl.ws_bytes;
    }
    return Y3_OK;
}

extern "C" size_t y3_conv2d_dgrad_workspace(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc) {
    return y3_conv2d_dgrad_workspace_x(ddst, ksize, stride, dsrc, 0u);
}
extern "C" size_t y3_conv2d_dgrad_workspace_x(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags) {
    if (stride == 1) return describe_gemm(dsrc->n * dsrc->h * dsrc->w, ddst->c, ksize * ksize, dsrc->c, flags).pl.ws_bytes;
    DgradDesc d;
    if (describe_dgrad(ddst, ksize, stride, dsrc, flags, &d) == Y3_OK && d.how == DGRAD_MERGED_X3) return d.ws_bytes;   // slabs of all classes behind one ticket header
    // Every other stride-2 launch: a deliberately loose bound, kept as it has always been answered -- every parity class (1, 2, 2
    // and 4 taps of a 3x3 kernel) planned as an f32 launch of its own with the M of the largest class, although the merged f32
    // launch needs no workspace at all (d.ws_bytes is the exact figure).
    size_t best = 0;
    for (int nt = 1; nt <= 4; nt *= 2) {
        const size_t b = describe_gemm(dsrc->n * ((dsrc->h + 1) / 2) * ((dsrc->w + 1) / 2), ddst->c, nt, dsrc->c, 0u).pl.ws_bytes;
        if (b > best) best = b;
    }
    return best;
}

// Row tiles of the partial statistics y3_conv2d_dgrad_bn writes for this shape, 0 if the shape does not qualify (channel counts
// off the fast path; stride 2: no merged launch): the caller then runs y3_bn_bwd_stats on the finished gradient instead.
extern "C" int y3_conv2d_dgrad_bn_tiles(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc) {
    return y3_conv2d_dgrad_bn_tiles_x(ddst, ksize, stride, dsrc, 0u);
}
extern "C" int y3_conv2d_dgrad_bn_tiles_x(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags) {
    DgradDesc d;
    return ddst && dsrc && describe_dgrad(ddst, ksize, stride, dsrc, flags, &d) == Y3_OK ? d.rows : 0;
}

// Diagnostics (include/yolo3hip.h): how y3_conv2d_dgrad / y3_conv2d_dgrad_bn send this data gradient out, class by class
extern "C" size_t y3_conv2d_dgrad_plan_x(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags, int* out51) {
    DgradDesc d;
    if (!ddst || !dsrc || describe_dgrad(ddst, ksize, stride, dsrc, flags, &d) != Y3_OK) {
        if (out51) out51[0] = -1;
        return 0;
    }
    if (out51) {
        for (int i = 0; i < 51; ++i) out51[i] = 0;
        out51[0] = (int)d.how;
        out51[1] = d.ncls;
        out51[2] = d.rows;
        const bool merged = d.how == DGRAD_MERGED_F32 || d.how == DGRAD_MERGED_X3;
        for (int c = 0; c < d.ncls; ++c) {
            const ConvPlan& pl = merged ? d.multi.c[c] : d.g[c].pl;
            const int fast = merged ? 1 : ((d.g[c].fast ? 1 : 0) | (pl.short_last ? 2 : 0));
            const int v[12] = {d.cls[c].K / d.cls[c].C, d.cls[c].M, pl.t.bm, pl.t.bn, pl.tiles, pl.f, pl.s0, pl.s1, pl.chunk0, pl.chunk1,
                               d.cls[c].K / pl.t.bk, fast};
            for (int i = 0; i < 12; ++i) out51[3 + 12 * c + i] = v[i];
        }
    }
    return d.ws_bytes;
}

static WgradPlan plan_wgrad(int K, int Nout, int M, int taps) {
    WgradPlan w;
    w.bkr = (K <= 64) ? 64 : 128;
    w.bn = (Nout <= 32) ? 32 : (Nout <= 64 ? 64 : 128);
    // Measured per shape (a sweep over the tile sizes, batch 8 at 416^2): the 1x1 layers (8-11 K steps per split, slab
    // traffic as large as the operands) run 20-25 % faster on 64x64 tiles; the 3x3 layers with large kernel matrices (26x26 and
    // 13x13 grids: K*Nout >= 1M) 5-10 % faster on 128x64, the 104x104 layer (K = 576) 6 % faster on 64x128.
    if (w.bkr == 128 && w.bn == 128) {
        if (taps == 1) {
            w.bkr = 64;
            w.bn = 64;
        } else if ((long long)K * Nout >= (1 << 20)) {
            w.bn = 64;
        } else if (K <= 576) {
            w.bkr = 64;
        }
    }
    w.tiles = y3_cdiv(K, w.bkr) * y3_cdiv(Nout, w.bn);
    // aim at ~16 waves per CU overall (these launches are latency / HBM bound per workgroup), at least 128 pixels per split
    constexpr int want_waves = 4096;
    const int waves_per_wg = (w.bkr == 64 && w.bn == 32) ? 2 : 4;
    int splits = y3_cdiv(want_waves, w.tiles * waves_per_wg);
    const int maxs = y3_cdiv(M, 128);
    if (splits > maxs) splits = maxs;
    if (splits < 1) splits = 1;
    if (splits < y3_cdiv(M, Y3_WG_TABLE - 32)) splits = y3_cdiv(M, Y3_WG_TABLE - 32);   // a split's pixels fit the kernel's LDS pixel table
    int chunk = y3_cdiv(M, splits);
    chunk = y3_cdiv(chunk, 32) * 32;                   // an even number of 16-pixel steps (the kernel runs its steps in pairs)
    w.splits = y3_cdiv(M, chunk);
    w.chunk = chunk;
    return w;
}

// The x3 kernel gradient (conv_x3.hip: conv_wgrad_x3_kernel): 128 x 128 tiles, two workgroups per CU (64 KB of LDS each), six
// steps of 16 pixels per loop iteration.  ~480 workgroups per launch -- one round of the 512 slots.
static bool wgrad_x3_shape_ok(int K, int Nout, int taps, int cin) {
    return cin % 4 == 0 && K >= 128 && Nout >= 128 && (taps == 1 || y3_is_pow2(cin));
}
static WgradPlan plan_wgrad_x3(int K, int Nout, int M) {
    WgradPlan w;
    w.bkr = 128;
    w.bn = 128;
    w.tiles = y3_cdiv(K, 128) * y3_cdiv(Nout, 128);
    constexpr int want = 480;
    int splits = want / w.tiles;
    if (splits < 1) splits = 1;
    // more tiles than CUs (13x13 3x3 layers: 288): one pixel run per tile leaves most CUs with a lone workgroup; two runs are a
    // round and an eighth; three (864 workgroups of ~28 steps, reduced in the kernel) measured best: 98 -> 87 us
    if (w.tiles > 256 && splits < 3) splits = 3;
    const int maxs = y3_cdiv(M, 192);
    if (splits > maxs) splits = maxs;
    if (splits < y3_cdiv(M, Y3_WG_TABLE - 96)) splits = y3_cdiv(M, Y3_WG_TABLE - 96);       // a split's pixels fit the LDS pixel table
    int chunk = y3_cdiv(M, splits);
    chunk = y3_cdiv(chunk, 96) * 96;                  // whole loop iterations: six steps of 16 pixels
    w.splits = y3_cdiv(M, chunk);
    w.chunk = chunk;
    return w;
}

// splits <= Y3_WG_FANIN: the reduction runs inside the kernel (one level: tickets + fragment-order slabs behind the header);
// more splits: natural-layout slabs [split][K][Nout] + slab_reduce_kernel (measured: a multi-level in-kernel tree costs more
// than the streaming reduce when every split is only a few K steps long)
static bool wgrad_in_kernel(const WgradPlan& w) {
    return w.splits > 1 && w.splits <= Y3_WG_FANIN && w.tiles <= Y3_MAX_TICKETS;
}
static size_t wgrad_ws_bytes(const WgradPlan& w, int K, int Nout) {
    if (w.splits <= 1) return 0;
    if (wgrad_in_kernel(w)) return (size_t)Y3_WS_HEADER + (size_t)w.tiles * w.splits * w.bkr * w.bn * sizeof(float);
    return (size_t)Y3_WS_HEADER + (size_t)w.splits * K * Nout * sizeof(float);
}
// The plan of a kernel gradient from its shape alone: the queries read it, y3_conv2d_wgrad_x issues it
WgradPlan describe_wgrad(int M, int cin, int taps, int Nout, unsigned flags) {
    const bool x3 = (flags & Y3_CONV_X3) && wgrad_x3_shape_ok(taps * cin, Nout, taps, cin);
    WgradPlan w = x3 ? plan_wgrad_x3(taps * cin, Nout, M) : plan_wgrad(taps * cin, Nout, M, taps);
    w.x3 = x3;
    w.grid = (w.splits >= 32 ? y3_cdiv(w.splits, 8) * 8 : w.splits) * w.tiles;
    w.in_kernel = wgrad_in_kernel(w);
    w.ws_bytes = wgrad_ws_bytes(w, taps * cin, Nout);
    return w;
}

// Diagnostics (include/yolo3hip.h): the plan behind y3_conv2d_wgrad
extern "C" size_t y3_conv2d_wgrad_plan(int m, int cin, int ksize, int cout, int* out8) { return y3_conv2d_wgrad_plan_x(m, cin, ksize, cout, 0u, out8); }
extern "C" size_t y3_conv2d_wgrad_plan_x(int m, int cin, int ksize, int cout, unsigned flags, int* out8) {
    const WgradPlan w = describe_wgrad(m, cin, ksize * ksize, cout, flags);
    if (out8) {
        const int v[8] = {w.bkr, w.bn, w.splits, w.chunk, w.tiles, w.in_kernel ? 1 : 0, w.grid, Y3_WG_TABLE};
        for (int i = 0; i < 8; ++i) out8[i] = v[i];
    }
    return w.ws_bytes;
}

extern "C" int y3_conv2d_wgrad_x3_ok(int m, int cin, int ksize, int cout) {
    return (m > 0 && wgrad_x3_shape_ok(ksize * ksize * cin, cout, ksize * ksize, cin)) ? 1 : 0;
}
extern "C" size_t y3_conv2d_wgrad_workspace_x(const y3_tensor* src, const y3_tensor* ddst, int ksize, int stride, unsigned flags) {
    (void)stride;
    return describe_wgrad(ddst->n * ddst->h * ddst->w, src->c, ksize * ksize, ddst->c, flags).ws_bytes;
}
extern "C" size_t y3_conv2d_wgrad_workspace(const y3_tensor* src, const y3_tensor* ddst, int ksize, int stride) {
    return y3_conv2d_wgrad_workspace_x(src, ddst, ksize, stride, 0u);
}
