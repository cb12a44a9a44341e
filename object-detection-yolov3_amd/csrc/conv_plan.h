// Descriptions of the convolution launches (conv_plan.cpp plans them, conv.hip issues them): ConvArgs -- the argument of the generic
// kernel and what the planners read of a launch --, the plans, and the constants planners and kernels share.  Plain C++, no HIP header.
#pragma once
#include "host.h"

struct ConvArgs {
    const float* src;
    const float* wt;
    float* dst;
    const float* bias;
    const float* scale;
    const float* shift;
    const float* resid;
    float* stats;
    unsigned long long tap_dhdw;  // 4 bits per tap: (dh+1) | (dw+1) << 2
    unsigned long long tap_wsel;  // 4 bits per tap: weight slice
    int H, W, C, logC, cmask, src_ld;
    int OH, OW, sh, sw;
    int DH, DW, dsh, dsw, doh, dow, dst_ld, dense_dst;
    int resid_ld;
    int Nout, K, M;
    unsigned flags;
    float alpha;
    int nbn;
    int src_n, wt_rows;  // host-side only: batch of src, rows of the weight matrix (descriptor sizes)
    const float* bn_a;   // data gradient with BatchNorm-backward statistics in the epilogue (y3_conv2d_dgrad_bn): the activation `a`
    float* bn_part;      // ... and the partial sums [row tile][6][Nout]
    int bn_a_ld;
    int x3;              // Y3_CONV_X3: the launch runs conv_x3.hip and `wt` is the copy with K contiguous per output column
};

struct TileCfg {
    int bm, bn, bk;
};
#define Y3_WS_HEADER (256 * 1024)   // bytes of tile tickets in front of the slabs (65 536 tiles)
#define Y3_MAX_TICKETS (Y3_WS_HEADER / 4)
static constexpr int x3_slots = 512;   // workgroup slots the x3 launches fill once: two workgroups of the patch kernel per CU
struct ConvPlan {
    TileCfg t;
    int f, s0, s1, chunk0, chunk1;   // FastArgs::sk_*: tiles [0,f) in s0 slices of chunk0 K steps, the rest in s1 of chunk1
    int tiles, stats_tiles;
    size_t ws_bytes;
    int short_last = 0;              // x3 overflow plan: deal the short last slices to the blocks the dispatcher starts last (FastArgs::x3_mode bit 3)
};
// The K loop of conv_fast_body runs its steps in pairs (an odd count is padded with a dead step): slices get an even step count.
static inline int even_steps(int chunk) { return chunk + (chunk & 1); }

// One gather-GEMM launch (the forward, a stride-1 data gradient, one parity class of a stride-2 one) described from its shape
// alone: M rows, ntaps * C contracted, Nout columns.  The queries read this description, launch_igemm issues it.
struct GemmDesc {
    bool x3;        // Y3_CONV_X3 was asked for and the x3 kernels take the shape
    bool fast;      // x3, or conv_igemm_fast_kernel; false: the generic kernel, whole tiles
    ConvPlan pl;
};

// What the fast kernels' arguments need from the geometry of a launch: the tap list as the kernels address it and the extents
// of the buffer descriptors.
struct FastGeom {
    int min_off;                   // most negative tap offset (floats): the source pointer is biased by it
    int dh[9], dw[9], off[9], wrow[9];
    int nx;                        // the tap list as a (rows x nx) grid
    unsigned src_bytes, wt_bytes, dst_bytes, resid_bytes;
};

// The merged launch of the parity classes of a stride-2 data gradient (conv_igemm_fast_multi_kernel, conv_x3_multi_kernel): one
// plan per class, each with ONE slice count for all its tiles (f32: whole tiles, no workspace)
struct MultiPlan {
    ConvPlan c[4];      // c[].ws_bytes is not used: the classes share one workspace
    int rows;           // row tiles over all classes: rows of the partial statistics
    size_t ws;          // ticket header + the slabs of all cut classes
};

// A data gradient described from the geometry of its tensors alone (no data pointer is read or needed).  The queries read the
// description; y3_conv2d_dgrad / y3_conv2d_dgrad_bn build it once, fill in the pointers and issue it (issue_dgrad).
enum DgradHow {
    DGRAD_SINGLE,        // stride 1: one launch_igemm
    DGRAD_MERGED_F32,    // stride 2: the parity classes in one launch of conv_igemm_fast_multi_kernel
    DGRAD_MERGED_X3,     // ... of conv_x3_multi_kernel
    DGRAD_BY_CLASS       // stride 2 off the fast path: one launch_igemm per parity class
};
struct DgradDesc {
    ConvArgs cls[4];     // one per launch or parity class, longest K first; src / wt / dst / bn_* stay null until issue_dgrad
    int ncls;
    DgradHow how;
    GemmDesc g[4];       // DGRAD_SINGLE (g[0]), DGRAD_BY_CLASS: the plan of each launch
    MultiPlan multi;     // DGRAD_MERGED_*
    int rows;            // rows of partial statistics y3_conv2d_dgrad_bn writes (row tiles over all classes); 0: it does not take the shape
    size_t ws_bytes;     // workspace the launches use at most
};

// kernel gradient (conv.hip: conv_wgrad_kernel; conv_x3.hip: conv_wgrad_x3_kernel)
#define Y3_WG_FANIN 8      // slab reduction: fan-in of the in-kernel tree
#define Y3_WG_TABLE 2048   // pixels per split the LDS pixel table holds (plan_wgrad keeps chunks below it)
struct WgradPlan {
    int bkr, bn, splits, chunk, tiles;
    bool x3;          // Y3_CONV_X3 was asked for and conv_wgrad_x3_kernel takes the shape
    int grid;         // workgroups of the launch
    bool in_kernel;   // the reduction over the splits runs inside the kernel (wgrad_in_kernel)
    size_t ws_bytes;  // ticket header + slabs; 0: one split, no workspace
};

// conv_plan.cpp, as far as conv.hip calls it to issue a launch
void whole_tiles(ConvPlan& pl, int chunk);
bool no_room(size_t need, const void* workspace, size_t workspace_bytes);
bool fast_geom(const ConvArgs& a, int ntaps, int bk, FastGeom* g);
int set_channels(int C, int taps, int* logC, int* cmask);
GemmDesc describe_gemm(const ConvArgs& a);
bool dgrad_x3(unsigned flags, const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc);
int describe_dgrad(const y3_tensor* ddst, int ksize, int stride, const y3_tensor* dsrc, unsigned flags, DgradDesc* d);
WgradPlan describe_wgrad(int M, int cin, int taps, int Nout, unsigned flags);
