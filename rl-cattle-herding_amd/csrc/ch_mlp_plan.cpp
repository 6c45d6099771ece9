// ch_mlp_plan.cpp -- which forward kernel a launch gets (ch_mlp_plan.h): a pure function of the nets, their row
// counts, the device's CU count and the A/B switches.  No getenv, no HIP call, no global state: ch_policy.hip's
// launch_mlp_multi executes the plan, ch__mlp_plan (ch_api_policy.cpp) shows it to the CPU tests.
#include <algorithm>

#include "ch_internal.h"

namespace ch {
namespace {

// LDS floats of k_mlp2's tile: RT == 1 input rows and two hidden buffers; RT > 1 the odd layers' hidden buffer in the
// input rows' region (dead after layer 0)
size_t mlp2_lds_floats(int rt, int lda, int ldh) {
    return rt == 1 ? (size_t)kTM * (lda + 2 * ldh) : (size_t)kTM * rt * ((lda > ldh ? lda : ldh) + ldh);
}

// what the table's tolerances are held against: the widest layer, the first layer's live K pairs, the LDS strides
// (the live input width rounded to whole K pairs, rows padded to 4 mod 64 floats), packed or raw weights
struct Shape {
    int maxw = 0, np0 = 0, lda = 0, ldh = 0;
    bool packed = true;
    // Raw weights and a hidden width that is no multiple of 16: k_mlp2's last tile of the layer clamps its rows past
    // the width to the last weight row (packed weights hold zero rows there), so its epilogue writes non-zero
    // activations into the columns [N, 16 nt) that other waves zero for the next layer, with no barrier between the
    // two.  k_mlp masks the columns in its epilogue.
    bool raw_ragged = false;
    void add(const MlpArgs& a) {
        int maxhid = 32;
        bool ragged = false;
        for (int i = 1; i <= a.layers; ++i) {
            maxw = std::max(maxw, a.dims[i]);
            maxhid = std::max(maxhid, a.dims[i]);   // (the output too: the sampling epilogue stages there)
            ragged |= i < a.layers && a.dims[i] % 16 != 0;
        }
        const int p = pad_pairs(std::max(a.kcap, 1));
        np0 = std::max(np0, p);
        lda = std::max(lda, (32 * p + 63) / 64 * 64 + 4);
        ldh = std::max(ldh, (std::max(maxhid, 32 * kD2) + 32 * kD2 - 1) / (32 * kD2) * (32 * kD2) + 4);
        packed &= a.packed != nullptr;
        raw_ragged |= !a.packed && ragged;
    }
    bool lds_fits(int rt) const { return sizeof(float) * mlp2_lds_floats(rt, lda, ldh) <= (size_t)kLdsMax2; }
};

bool tolerates(const MlpKernelInfo& k, const Shape& sh) {
    return (sh.packed || !k.packed_only) && sh.np0 <= k.max_pair0 && (!sh.raw_ragged || k.raw_ragged);
}

bool ab_on(int ab, const MlpSwitches& sw) { return ab == kAbNw4 ? sw.nw4 : (ab == kAbWide4 ? sw.wide4 : false); }

// The row of `family` for layers up to `maxw` wide and at most `rt` row tiles that tolerates `sh` and whose tile fits
// the LDS: the one with the most row tiles (kMlpNone: no row).  The width class is the narrowest the table has for
// maxw; an A/B row whose switch is set stands in for its class's default rows, one whose switch is not is left out.
int pick(int family, int maxw, int rt, bool share, const Shape& sh, const MlpSwitches& sw) {
    int width = 1 << 30;
    bool ab = false;
    for (const MlpKernelInfo& k : kMlpTable)
        if (k.family == family && k.width() >= maxw) width = std::min(width, k.width());
    for (const MlpKernelInfo& k : kMlpTable) ab |= k.family == family && k.width() == width && ab_on(k.ab, sw);
    int best = kMlpNone;
    for (int i = 0; i < kMlpKernels; ++i) {
        const MlpKernelInfo& k = kMlpTable[i];
        if (k.family != family || k.width() != width || k.share != share || k.rt > rt) continue;
        if (ab ? !ab_on(k.ab, sw) : k.ab != kAbNone) continue;
        if (!tolerates(k, sh) || (family == kFamMlp2 && !sh.lds_fits(k.rt))) continue;
        if (best == kMlpNone || k.rt > kMlpTable[best].rt) best = i;
    }
    return best;
}

}  // namespace

MlpPlan mlp_plan(const MlpArgs* segs, int nseg, int cus, const MlpSwitches& sw) {
    MlpPlan p = {};
    Shape sh;
    long long rows_all = 0;
    for (int s = 0; s < nseg && s < 3; ++s) {
        if (segs[s].rows <= 0) continue;
        p.src[p.n++] = s;
        sh.add(segs[s]);
        rows_all += segs[s].rows;
    }
    p.rt = 1;
    if (p.n == 0) return p;   // kMlpNone: nothing to launch
    p.lda = sh.lda;
    p.ldh = sh.ldh;
    // 1. the row tiles asked for: the most (1, 2 or 4 tiles of 16 rows) that still leave a workgroup for every CU across
    // the launch's segments -- each weight pair a workgroup streams then feeds RT times the MFMAs, and the forward of
    // a chip-filling batch waits on that stream, not on the matrix cores; CH_MLP_RT overrides
    int want = 1;
    if (sw.rt == 1 || sw.rt == 2 || sw.rt == 4) want = sw.rt;
    else
        for (int r : {4, 2})
            if (rows_all >= (long long)kTM * r * cus) { want = r; break; }
    // 2. + 3. the k_mlp2 rows of the nets' width class that tolerate them (packed or raw weights, the first layer's
    // pairs, ragged hidden widths) and, among those, the most row tiles <= want whose tile fits the LDS (a row tile
    // count the class has no row for, or whose rows do not take these nets, falls to the next lower one)
    int k2 = sw.v1 ? kMlpNone : pick(kFamMlp2, sh.maxw, want, false, sh, sw);
    // 4. two or three segments at one row tile: the SHARE variant, two workgroups per CU, where the class has one
    if (k2 != kMlpNone && p.n > 1 && kMlpTable[k2].rt == 1) {
        const int ks = pick(kFamMlp2, sh.maxw, 1, true, sh, sw);
        if (ks != kMlpNone) k2 = ks;
    }
    p.v2 = k2 != kMlpNone;
    if (p.v2) {
        p.rt = kMlpTable[k2].rt;
        p.lds = (int)(sizeof(float) * mlp2_lds_floats(p.rt, p.lda, p.ldh));
    } else {
        p.lds = kLdsMlp1;
    }
    // 5. no such row (a first layer past kMaxPair0 pairs, ragged raw weights) or CH_MLP_V1: k_mlp, one launch per net,
    // each by its own width
    for (int i = 0; i < p.n; ++i) {
        const MlpArgs& a = segs[p.src[i]];
        Shape own;
        own.add(a);
        p.kernel[i] = p.v2 ? k2 : pick(kFamMlp1, own.maxw, 1, false, own, sw);
        p.grid[i] = (int)((a.rows + kTM * p.rt - 1) / (kTM * p.rt));
        p.start[i + 1] = p.start[i] + p.grid[i];
    }
    return p;
}

// k_mlp2's one-tile shape for the step kernel's fused forward (ch_step.hip): the same tolerances as a one-row-tile
// kernel of CH_V2_MAX_BLOCK / 64 waves with one column tile each
bool mlp2_fused_tile(const MlpArgs& a, int& lda, int& ldh, size_t& bytes) {
    Shape sh;
    sh.add(a);
    lda = sh.lda;
    ldh = sh.ldh;
    if (sh.np0 > kMaxPair0 || sh.raw_ragged || !sh.lds_fits(1) || sh.maxw > 16 * (CH_V2_MAX_BLOCK / 64)) return false;
    if (a.rows_dev || a.row_mask || a.rows_per_env != 1) return false;
    bytes = sizeof(float) * mlp2_lds_floats(1, lda, ldh);
    return true;
}

}  // namespace ch
