// ch_step_plan.cpp -- which kernels a handle's env step runs, at what geometry (ch_step_plan.h): a pure function of
// the shape, the device's CU count and LDS budget, and the diagnostics overrides.  No getenv, no HIP call, no global
// state: ch_api.cpp stores the plan on the handle and launches its rows, ch__step_plan shows it to the CPU tests.
#include <algorithm>

#include "ch_step_plan.h"

namespace ch {
namespace {

struct Geometry {
    int kernel = 2, G = 1, block = 64;
    size_t lds = 0;
    bool pw = false, sep = false;
};
struct Ctx {
    const StepShape& s;
    int cus, P, rb;
    size_t budget;
    bool pyb() const { return s.physics == CH_PHYS_PYB; }
    // V2Layout's bytes for G envs per workgroup: W per-wave tables, or the shared tables with / without `sep`
    size_t bytes(int G, int W = 0, bool sep = false) const { return V2Layout(G, s.N, s.M, P, s.mode, rb, W, sep).bytes(); }
};

// The geometry rules: each returns whether it changed `g`.  They run in the table's order and a later one
// may undo an earlier one; the order and the results are ch_create's of old.

// v2 geometry: G envs per workgroup with all G*N drone chains in wave 0, the LDS carve within the per-CU budget, and at
// least one workgroup per CU when E allows it.
bool rule_generic(const Ctx& c, Geometry& g) {
    // a drone wave (G*N <= 64 drone chains) plus three cow waves (G*M cows, one per lane when it fits)
    int G = std::max(1, std::min(64 / c.s.N, 192 / c.s.M));
    G = (int)std::min<long long>(G, std::max<long long>(1, c.s.E / std::max(c.cus, 1)));
    while (G & (G - 1)) G &= G - 1;   // power of two: whole workgroups per CU at E = 2^k
    while (G > 1 && c.bytes(G) > c.budget) --G;
    g.G = G;
    g.lds = c.bytes(G);
    g.block = 256;
    return true;
}

// measured (tools/geom_sweep.py, profiles/r02/geom_*.log): at 4 drones x 16 cattle one workgroup
// of 16 envs per CU (a full 64-drone wave + cow waves sharing the work counters) beats two of 8
// envs, and 11 cow waves (768 threads, 3 waves per SIMD) edge out 7 (24.1 vs 24.8 us at 4096 envs);
// the physics variants keep 512 (their register use allows 2 waves per SIMD)
bool rule_4x16(const Ctx& c, Geometry& g) {
    if (!(c.s.mode == CH_MODE_CTDE && c.s.N == 4 && c.s.M == 16 && c.s.E >= 16 * (long long)c.cus && c.bytes(16) <= c.budget))
        return false;
    g.G = 16;
    g.lds = c.bytes(16);
    // f32: 512 threads (tools/f32_geom_probe.py: 419 vs 273 M env-steps/s at 262144 envs, 1.5 % slower
    // at 4096; f64 keeps 768, 230 vs 225 M at 262144 and 1 % faster at 4096)
    g.block = (c.pyb() && c.rb == 8) ? CH_V2_MAX_BLOCK : CH_V2_MAX_BLOCK_PW;
    return true;
}

// 2 drones x 8 cattle (configs[1]/[2]), f64: 16 envs / 512 threads per workgroup from 1024 envs up, also when
// that leaves CUs idle (configs[1]: 64 workgroups) -- tools/multi_geom.py, profiles/r06/ab/r6y_*: at 1024 envs
// 78.1 vs 76.4 M env-steps/s (ch_step_n) and 61.8 vs 58.5 M (ch_step) against 4 envs / 256 threads; at 4096
// envs 311.9 vs 311.0 M and 238.3 vs 229.4 M against 16 envs / 256 threads
bool rule_2x8(const Ctx& c, Geometry& g) {
    if (!(c.s.mode == CH_MODE_CTDE && c.s.N == 2 && c.s.M == 8 && c.rb == 8 && c.pyb() && c.s.E >= 1024 &&
          c.bytes(16) <= c.budget))
        return false;
    g.G = 16;
    g.lds = c.bytes(16);
    g.block = CH_V2_MAX_BLOCK_PW;
    return true;
}

// measured (tools/ab/marl.py, MI355X, 4096 envs): the dataflow kernel wins for every CTDE size
// (2x8 19.4 vs 41.1 us, 8x16 39.7 vs 55.8, 12x16 59.9 vs 67.1) and for MARL with up to 16
// cattle (3x8 25.8 vs 43.2).  Above 16 cows one shared pair table per workgroup (15.9 KB per
// env at 32 cows) leaves room for 4 envs per CU; the per-wave env tables (V2Layout W) keep a
// CU's 16 envs in one workgroup instead.
bool rule_per_wave(const Ctx& c, Geometry& g) {
    if (c.s.M < kPwMinCattle) return false;
    g.kernel = 1;   // unless a per-wave geometry fits (physics variants stay on v1)
    if (!c.pyb()) return true;
    const int cand[][2] = {{16, 512}, {8, 512}, {8, 256}, {4, 256}, {2, 128}, {1, 128}};
    for (const auto& gb : cand) {
        const int G = gb[0], blk = gb[1];
        if (G * c.s.N > 64 || G * c.s.M > 3 * (blk - 64)) continue;
        if (G > 1 && c.s.E < (long long)G * c.cus) continue;
        const size_t l = c.bytes(G, blk / 64 - 1);
        if (l > c.budget) continue;
        g.G = G; g.block = blk; g.lds = l; g.pw = true; g.kernel = 2;
        break;
    }
    return true;
}

// shared tables: the shepherd terms in their own region when it fits, so they need not wait for every
// alpha row to have read the pair table
bool rule_sep(const Ctx& c, Geometry& g) {
    if (g.pw) return false;
    const size_t l = c.bytes(g.G, 0, true);
    if (l > c.budget) return false;
    g.sep = true;
    g.lds = l;
    return true;
}

// one env's pair table alone exceeds the budget
bool rule_v1_fallback(const Ctx& c, Geometry& g) {
    if (g.lds <= c.budget) return false;
    g.kernel = 1;
    return true;
}

constexpr struct { const char* name; bool (*apply)(const Ctx&, Geometry&); } kRules[kStepRules] = {
    {"generic", rule_generic},       {"4x16", rule_4x16}, {"2x8", rule_2x8},
    {"per_wave", rule_per_wave},     {"sep", rule_sep},   {"v1_fallback", rule_v1_fallback},
};

// ch__set_geometry: G envs per workgroup and `block` threads in place of the rules' (pw stays what they chose)
int override_geometry(const Ctx& c, int G, int block, Geometry& g) {
    if (G < 1 || G > 64 || G * c.s.N > 64 || block < 128 || block % 64 || block > step_max_block(!c.pyb(), g.pw))
        return CH_ERR_INVALID;
    if (G * c.s.M > 3 * (block - 64)) return CH_ERR_UNSUPPORTED;   // the cow waves prefetch <= 3 spawn slots per lane
    size_t lds = c.bytes(G, g.pw ? block / 64 - 1 : 0);
    if (lds > c.budget) return CH_ERR_UNSUPPORTED;
    g.G = G; g.block = block; g.lds = lds; g.sep = false;
    rule_sep(c, g);
    return CH_OK;
}

int find_row(int family, int prec, int mode, int gt, int nt, int mt, bool phys, bool pw, int tobs_wpe) {
    for (int i = 0; i < kStepKernels; ++i)
        if (step_row_is(i, family, prec, mode, gt, nt, mt, phys, pw, tobs_wpe)) return i;
    return kStepNoRow;
}

}  // namespace

const char* const kStepRuleNames[kStepRules] = {kRules[0].name, kRules[1].name, kRules[2].name,
                                                kRules[3].name, kRules[4].name, kRules[5].name};

// ch_step_n's f32 kernel takes the registers of 4 waves per SIMD (WPE = 4: two workgroups per CU) once the grid has more
// workgroups than this: MI355X's CU count, written as a literal -- not the device's -- because that is what was measured
// (ch_step_multi.hip) and the choice must not move with the planner.
constexpr long long kMultiWpe4Grid = 256;

StepPlan step_plan(const StepShape& s, int cus, size_t lds_budget, const StepOverrides& ov) {
    StepPlan p = {};
    p.step_row[0] = p.step_row[1] = p.multi_row = p.actor_row[0] = p.actor_row[1] = kStepNoRow;
    const Ctx c{s, cus, s.M * (s.M - 1) / 2, s.precision == CH_PREC_F64 ? 8 : 4, lds_budget};
    Geometry g;
    for (int r = 0; r < kStepRules; ++r)
        if (kRules[r].apply(c, g)) p.rules |= 1u << r;
    if (ov.geometry)
        if ((p.error = override_geometry(c, ov.G, ov.block, g))) return p;
    if (ov.kernel) {   // ch__set_kernel
        if (ov.kernel != 1 && ov.kernel != 2) { p.error = CH_ERR_INVALID; return p; }
        if (ov.kernel == 2 && g.lds > lds_budget) { p.error = CH_ERR_UNSUPPORTED; return p; }
        g.kernel = ov.kernel;
    }
    p.kernel = g.kernel; p.G = g.G; p.block = g.block; p.lds = g.lds; p.pw = g.pw; p.sep = g.sep;
    if (g.kernel != 2) return p;

    // k_step2: the body specialised for this geometry where the table has one, else the runtime-geometry body; the
    // terminal observations from their producers (TOBS) where the table has that twin
    const bool phys = !c.pyb();
    auto row_of = [&](int family, int tobs_wpe) {
        const int r = find_row(family, s.precision, s.mode, g.G, s.N, s.M, phys, g.pw, tobs_wpe);
        return r != kStepNoRow || family != kStepFamStep ? r : find_row(family, s.precision, s.mode, 0, 0, 0, phys, g.pw, tobs_wpe);
    };
    p.step_row[0] = row_of(kStepFamStep, 0);
    p.step_row[1] = row_of(kStepFamStep, 1);
    if (p.step_row[1] == kStepNoRow) p.step_row[1] = p.step_row[0];
    if (ov.phase_mask) return p;

    // k_step2_multi: the BASELINE geometries under PYB only; WPE = 4 where the table has it and the grid is large
    int m = row_of(kStepFamMulti, 1);
    const int m4 = row_of(kStepFamMulti, 4);
    if (m4 != kStepNoRow && (s.E + g.G - 1) / g.G > kMultiWpe4Grid) m = m4;
    if (m != kStepNoRow) {
        const StepKernelInfo& k = kStepTable[m];
        // The handle's block is clamped to the instantiation's launch bound: 8 waves where the step loop needs the
        // registers of 2 waves per SIMD, 10 for the pipelined instantiation, whose loop fits 3 per SIMD.  The cow waves
        // share their work out dynamically, so the outputs do not depend on how many of them run.
        const int blk = std::min(g.block, k.max_block);
        size_t lds = g.lds;
        bool ok = true;
        if (k.pipelined) {
            // two drone waves and at least two cow waves that hold the workgroup's cows (three spawn slots per lane); the
            // fast reset path (sep); room for the hand-off behind the carve
            lds += v2_pipe_bytes(c.rb);
            ok = blk >= 256 && g.G * s.M <= 3 * (blk - 128) && g.sep && lds <= lds_budget;
        }
        if (ok) { p.multi_row = m; p.multi_block = blk; p.multi_lds = lds; }
    }
    // k_step2_actor: the shape's half of the fused step's conditions (the net's: launch_step_v2_actor)
    if (g.block == CH_V2_MAX_BLOCK) {
        p.actor_row[0] = row_of(kStepFamActor, 0);
        p.actor_row[1] = row_of(kStepFamActor, 1);
    }
    return p;
}

}  // namespace ch

// ---- host-only introspection (cattleherd/_lib.py step_plan, step_kernel_table, step_rules) ---------------------------
void ch::step_plan_out(const StepPlan& p, int64_t out[13]) {
    const int64_t v[13] = {p.kernel, p.G, p.block, (int64_t)p.lds, p.pw, p.sep, p.step_row[0], p.step_row[1], p.multi_row,
                           p.multi_block, (int64_t)p.multi_lds, p.actor_row[0] != kStepNoRow, (int64_t)p.rules};
    std::copy(v, v + 13, out);
}

extern "C" {

/* Internal (tests / diagnostics): what ch_create would plan for a handle of this shape on a device of `cus` compute
 * units and `lds_budget` bytes of LDS per workgroup -- step_plan on the host, no device touched.  out = {kernel
 * version, G, block, lds, pw, sep, k_step2's row without and with terminal observations, ch_step_n's k_step2_multi row,
 * its block, its lds, whether the shape takes the fused actor step, the geometry rules that fired (bit r: rule r of
 * ch__step_rule)}; rows index the kernel table (ch__step_kernel), -1 = none.  set_kernel / set_G / set_block (0: none)
 * plan as after ch__set_kernel and ch__set_geometry, whose status is returned. */
int ch__step_plan(int32_t mode, int32_t N, int32_t M, int32_t precision, int32_t physics, int64_t E, int32_t cus,
                  int64_t lds_budget, int32_t set_kernel, int32_t set_G, int32_t set_block, int64_t out[13]) {
    using namespace ch;
    if (!out || N < 1 || N > kNMax || M < 1 || M > kMMax || E < 1 || cus < 1 || lds_budget < 1) return CH_ERR_INVALID;
    StepOverrides ov;
    ov.kernel = set_kernel;
    ov.geometry = set_G || set_block; ov.G = set_G; ov.block = set_block;
    const StepPlan p = step_plan({mode, N, M, precision, physics, E}, cus, (size_t)lds_budget, ov);
    if (!p.error) step_plan_out(p, out);
    return p.error;
}

/* Internal (tests / diagnostics): row `row` of the step kernels' table (ch_step_plan.h kStepTable): its name (NULL past
 * the table) and, if `out` is given, {family (0 k_step2, 1 k_step2_multi, 2 k_step2_actor), precision, MODE, GT, NT,
 * MT, PHYS, PW, TOBS (k_step2_multi: WPE), launch bound, pipelined}. */
const char* ch__step_kernel(int32_t row, int32_t out[11]) {
    if (row < 0 || row >= ch::kStepKernels) return nullptr;
    const ch::StepKernelInfo& k = ch::kStepTable[row];
    const int32_t v[11] = {k.family, k.precision, k.mode, k.gt, k.nt, k.mt, k.phys, k.pw, k.tobs_wpe, k.max_block, k.pipelined};
    if (out) std::copy(v, v + 11, out);
    return k.name;
}

/* Internal (tests / diagnostics): the name of geometry rule `rule`, in the order the planner applies them (NULL past the
 * last). */
const char* ch__step_rule(int32_t rule) { return rule >= 0 && rule < ch::kStepRules ? ch::kStepRuleNames[rule] : nullptr; }

}  // extern "C"
