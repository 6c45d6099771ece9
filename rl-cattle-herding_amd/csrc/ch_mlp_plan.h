// ch_mlp_plan.h -- what the host and the device sides of the policy forward must agree on: the tile constants, the
// kernel table (one row per instantiation of k_mlp2 / k_mlp, with what each tolerates) and the planner that picks a
// row for a launch (ch_mlp_plan.cpp).  Plain C++: no HIP runtime call, usable from host and device code.
#pragma once
#include <stddef.h>

#ifdef __HIP__   // compiled as HIP (ch_mlp2_dev.h's device code calls these too)
#define CH_PLAN_HD __host__ __device__
#define CH_PLAN_INLINE __forceinline__
#else
#define CH_PLAN_HD
#define CH_PLAN_INLINE inline
#endif

namespace ch {

constexpr int kTM = 16;            // rows per row tile
constexpr int kKC = 64;            // k_mlp: K chunk
constexpr int kKS = kKC + 4;       // k_mlp: LDS row stride of a chunk (conflict-free operand reads)
constexpr int kWMax = 256;         // widest layer
constexpr int kD2 = 4;             // k_mlp2: K pairs in flight per wave
constexpr int kMaxPair0 = 36;      // k_mlp2: first-layer live width <= 1152 (else k_mlp)
constexpr int kLdsMax2 = 160 * 1024 - 1024;   // k_mlp2 dynamic LDS cap (the static kmax word included)
// k_mlp's dynamic LDS: one chunk of the input rows and of the weights, two hidden buffers
constexpr int kLdsMlp1 = (int)sizeof(float) * (kTM * kKS + kWMax * kKS + 2 * kTM * (kWMax + 4));

CH_PLAN_HD CH_PLAN_INLINE int pad_pairs(int k) { return ((k + 31) / 32 + kD2 - 1) / kD2 * kD2; }

// mlp2_body's staging ring: 4 NW threads share an input row, each holding kQ float4 registers per pass.  A pass must
// cover a whole row tile's padded width 32 np0 (the store loop walks the ring once per pass), so a kernel takes only
// first layers with ceil(8 np0 / (4 NW)) <= kQ.  <8, *, *> rings hold kMaxPair0 pairs; the <4, 4, *, RT > 1> ones
// (8 registers, to stay inside their register budget) hold 16 pairs = 512 columns: the kernel table's max_pair0, so
// that mlp_plan gives wider first layers one row tile per workgroup.
template <int NW, int RT> constexpr int mlp2_stage_regs() { return RT > 1 && NW < 8 ? 8 : 8 * kMaxPair0 / (4 * NW); }
template <int NW, int RT> CH_PLAN_HD constexpr bool mlp2_stage_fits(int np0) {
    return (8 * np0 + 4 * NW - 1) / (4 * NW) <= mlp2_stage_regs<NW, RT>();
}
// the most first-layer pairs k_mlp2<NW, *, *, RT> stages
template <int NW, int RT> constexpr int mlp2_stage_pairs() {
    int np0 = kMaxPair0;
    while (np0 > 0 && !mlp2_stage_fits<NW, RT>(np0)) np0 -= kD2;
    return np0;
}

// ---- the kernel table ----------------------------------------------------------------------------------------------
// kMlp2_<NW>_<TW>[s][_r<RT>] = k_mlp2<NW, TW, SHARE, RT>; kMlp1_<NW>_<TWMAX>_<DEPTH> = k_mlp<NW, TWMAX, DEPTH>.  The
// values are ch__mlp_last_launch's kernel numbers and index kMlpTable and ch_policy.hip's array of kernels.
enum MlpKernel {
    kMlpNone = 0, kMlp2_8_1 = 1, kMlp2_8_2 = 2, kMlp2_4_2 = 3, kMlp2_8_1s = 4, kMlp2_8_1_r2 = 5, kMlp2_4_4_r2 = 6,
    kMlp2_4_4_r4 = 7, kMlp1_8_1_2 = 8, kMlp1_8_2_2 = 9, kMlp1_4_4_1 = 10, kMlpKernels = 11
};
enum MlpFamily { kFamNone = 0, kFamMlp2 = 2, kFamMlp1 = 1 };   // k_mlp2: one launch over all segments; k_mlp: one per net
enum MlpAb { kAbNone = 0, kAbNw4, kAbWide4 };   // the A/B switch that puts a row in place of its class's default rows
struct MlpKernelInfo {
    const char* name;    // cattleherd/_lib.py MLP_KERNELS
    int family;          // MlpFamily
    int nw, tw;          // waves (64 nw threads) and 16-column tiles per wave: layers up to 16 nw tw wide
    bool share;          // k_mlp2 SHARE: two workgroups per CU, the multi-segment launches
    int rt;              // row tiles of 16 per workgroup
    int ab;              // MlpAb
    // what the kernel tolerates
    bool packed_only;    // reads ch_mlp.packed only (mlp2_body's PKO)
    int max_pair0;       // the most first-layer K pairs (of the live width kcap) its staging holds
    bool raw_ragged;     // raw weights with a hidden width that is no multiple of 16
    constexpr int width() const { return 16 * nw * tw; }
    constexpr int lds_attr() const { return family == kFamMlp2 ? kLdsMax2 : kLdsMlp1; }   // the dynamic-LDS opt-in
};
constexpr bool mlp2_pko(int nw, int rt) { return nw == 4 && rt > 1; }
template <int NW, int TW, bool SHARE, int RT> constexpr MlpKernelInfo mlp2_row(const char* name, int ab = kAbNone) {
    return {name, kFamMlp2, NW, TW, SHARE, RT, ab, mlp2_pko(NW, RT), mlp2_stage_pairs<NW, RT>(), false};
}
// k_mlp streams its input in chunks (any width) and masks a ragged layer's columns in its epilogue
constexpr MlpKernelInfo mlp1_row(const char* name, int nw, int twmax, int ab = kAbNone) {
    return {name, kFamMlp1, nw, twmax, false, 1, ab, false, 1 << 24, true};
}
constexpr MlpKernelInfo kMlpTable[kMlpKernels] = {
    {"none", kFamNone, 0, 0, false, 0, kAbNone, false, 0, false},
    mlp2_row<8, 1, false, 1>("k_mlp2<8,1>"),
    mlp2_row<8, 2, false, 1>("k_mlp2<8,2>"),
    mlp2_row<4, 2, false, 1>("k_mlp2<4,2>", kAbNw4),
    mlp2_row<8, 1, true, 1>("k_mlp2<8,1,true>"),
    mlp2_row<8, 1, false, 2>("k_mlp2<8,1,false,2>"),
    mlp2_row<4, 4, false, 2>("k_mlp2<4,4,false,2>"),
    mlp2_row<4, 4, false, 4>("k_mlp2<4,4,false,4>"),
    mlp1_row("k_mlp<8,1,2>", 8, 1),
    mlp1_row("k_mlp<8,2,2>", 8, 2),
    mlp1_row("k_mlp<4,4,1>", 4, 4, kAbWide4),
};
static_assert(kMlpTable[kMlp2_8_2].max_pair0 == kMaxPair0 && kMlpTable[kMlp2_4_4_r4].max_pair0 == 16,
              "<8, *> rings hold every first layer k_mlp2 takes, the 8-register rings 512 columns");

// ch__mlp_last_launch: the forward kernel launch_mlp_multi launched last -- host side only
struct MlpLaunch {
    int kernel;   // MlpKernel (kMlpNone: no row to compute, nothing launched)
    int rt;       // row tiles of 16 per workgroup it ended with
    int grid;     // workgroups
    int lds;      // dynamic LDS bytes
};

// ---- the planner (ch_mlp_plan.cpp): a pure function of the nets, the row counts, the CU count and the switches ------
struct MlpArgs;
struct MlpSwitches { bool v1, nw4, wide4; int rt; };   // CH_MLP_V1, CH_MLP2_NW4, CH_MLP_WIDE4, CH_MLP_RT
struct MlpPlan {
    bool v2;                 // one k_mlp2 launch over all segments; false: one k_mlp launch per net
    int n;                   // segments with rows > 0, in order
    int src[3];              // their indices in the caller's array
    int kernel[3], grid[3];  // v2: kernel[0] and the total grid (start[n]) are what is launched
    int start[4], rt, lda, ldh, lds;   // first workgroup of each segment; row tiles; LDS strides (floats); LDS bytes
};
MlpPlan mlp_plan(const MlpArgs* segs, int nseg, int cus, const MlpSwitches& sw);

}  // namespace ch
