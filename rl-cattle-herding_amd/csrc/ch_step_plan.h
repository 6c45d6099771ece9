// ch_step_plan.h -- what runs for a handle's env step, decided in one place: the kernel table (one row per
// instantiation of k_step2, k_step2_multi and k_step2_actor that ch_step.hip and ch_step_multi.hip emit) and the planner
// (ch_step_plan.cpp) that gives a shape its kernel version, its geometry and its rows.  Plain C++: no HIP runtime call.
// ch_create stores the plan on the handle, ch__set_kernel / ch__set_geometry / ch__set_phase_mask replan through the
// overrides, the launchers of the two .hip files take a row and launch it, ch__step_plan shows it to the CPU tests.
#pragma once
#include "ch_internal.h"

// 512 threads: 2 waves per SIMD (A/B)
#ifndef CH_MULTI_MAX_BLOCK
#define CH_MULTI_MAX_BLOCK CH_V2_MAX_BLOCK_PW
#endif
// The pipelined instantiation's own bound: 2 drone waves + 8 cow waves.  Its step loop compiles to 161 VGPRs and no
// scratch under this bound too (tools/res_usage.sh), inside the 168 registers of 3 waves per SIMD, and the extra cow
// waves shorten the cow side, which is that loop's critical path (640 beat 576 beat 512).  The other
// instantiations take 171 VGPRs, which do not fit 3 waves per SIMD: they keep CH_MULTI_MAX_BLOCK.
#ifndef CH_MULTI_PIPE_MAX_BLOCK
#define CH_MULTI_PIPE_MAX_BLOCK 640
#endif

namespace ch {

// ---- the kernel table ----------------------------------------------------------------------------------------------
enum StepFamily { kStepFamStep = 0, kStepFamMulti = 1, kStepFamActor = 2 };   // k_step2, k_step2_multi, k_step2_actor
struct StepKernelInfo {
    const char* name;     // the template-id, trailing default arguments left out (cattleherd/_lib.py STEP_KERNELS)
    int family;           // StepFamily
    int precision;        // CH_PREC_F64 / CH_PREC_F32: the kernel's R
    int mode;             // MODE: CH_MODE_CTDE / CH_MODE_MARL
    int gt, nt, mt;       // GT, NT, MT: the geometry the body is specialised for; all 0: read at run time
    bool phys, pw;        // PHYS: the physics variants' body; PW: per-wave env tables
    int tobs_wpe;         // k_step2, k_step2_actor: TOBS (terminal observations from their producers); k_step2_multi: WPE
    int max_block;        // the instantiation's __launch_bounds__
    bool pipelined;       // k_step2_multi: the step loop pipelined over two drone waves (ch_step_multi.hip)
};
// k_step2's launch bound
constexpr int step_max_block(bool phys, bool pw) { return (pw || phys) ? CH_V2_MAX_BLOCK_PW : CH_V2_MAX_BLOCK; }
// The k_step2_multi instantiation whose step loop is pipelined over two drone waves (configs[3], f64), and the launch
// bound of each (ch_step_multi.hip)
constexpr bool multi_pipelined(int precision, int mode, int gt, int nt, int mt, bool phys, bool pw, int wpe) {
    return precision == CH_PREC_F64 && mode == 0 && gt == 16 && nt == 4 && mt == 16 && !phys && !pw && wpe == 1;
}
constexpr int multi_max_block(bool pipelined, bool pw) {
    return pipelined ? CH_MULTI_PIPE_MAX_BLOCK : pw ? CH_V2_MAX_BLOCK_PW : CH_MULTI_MAX_BLOCK;
}
constexpr StepKernelInfo step_row(const char* name, int prec, int mode, int gt, int nt, int mt, bool phys = false,
                                  bool pw = false, bool tobs = false) {
    return {name, kStepFamStep, prec, mode, gt, nt, mt, phys, pw, tobs, step_max_block(phys, pw), false};
}
constexpr StepKernelInfo multi_row(const char* name, int prec, int mode, int gt, int nt, int mt, bool phys = false,
                                   bool pw = false, int wpe = 1) {
    const bool pipe = multi_pipelined(prec, mode, gt, nt, mt, phys, pw, wpe);
    return {name, kStepFamMulti, prec, mode, gt, nt, mt, phys, pw, wpe, multi_max_block(pipe, pw), pipe};
}
constexpr StepKernelInfo actor_row(const char* name, bool tobs) {
    return {name, kStepFamActor, CH_PREC_F64, 0, 16, 4, 16, false, false, tobs, CH_V2_MAX_BLOCK, false};
}
// k_step2's instantiations, the same for each precision; the BASELINE configs at their default geometry have bodies of
// their own
#define CH_STEP2_ROWS(R, PREC)                                                                   \
    step_row("k_step2<" #R ",1,0,0,0,true>", PREC, 1, 0, 0, 0, true),                            \
    step_row("k_step2<" #R ",0,16,4,16,true>", PREC, 0, 16, 4, 16, true),              /* configs[3] */ \
    step_row("k_step2<" #R ",0,0,0,0,true>", PREC, 0, 0, 0, 0, true),                            \
    step_row("k_step2<" #R ",1,16,4,32,false,true>", PREC, 1, 16, 4, 32, false, true), /* configs[4] */ \
    step_row("k_step2<" #R ",1,0,0,0,false,true>", PREC, 1, 0, 0, 0, false, true),               \
    step_row("k_step2<" #R ",0,0,0,0,false,true>", PREC, 0, 0, 0, 0, false, true),               \
    step_row("k_step2<" #R ",1,0,0,0>", PREC, 1, 0, 0, 0),                                       \
    step_row("k_step2<" #R ",0,8,4,16>", PREC, 0, 8, 4, 16),                           /* configs[3] */ \
    step_row("k_step2<" #R ",0,16,4,16,false,false,true>", PREC, 0, 16, 4, 16, false, false, true), \
    step_row("k_step2<" #R ",0,16,4,16>", PREC, 0, 16, 4, 16),                         /* configs[3] */ \
    step_row("k_step2<" #R ",0,16,2,8>", PREC, 0, 16, 2, 8),                           /* configs[2] */ \
    step_row("k_step2<" #R ",0,4,2,8>", PREC, 0, 4, 2, 8),                             /* configs[1] */ \
    step_row("k_step2<" #R ",0,0,0,0>", PREC, 0, 0, 0, 0)
constexpr StepKernelInfo kStepTable[] = {
    CH_STEP2_ROWS(double, CH_PREC_F64),
    CH_STEP2_ROWS(float, CH_PREC_F32),
    // ch_step_n's kernel: the BASELINE geometries under PYB
    multi_row("k_step2_multi<double,1,16,4,32,false,true>", CH_PREC_F64, 1, 16, 4, 32, false, true),   // configs[4]
    multi_row("k_step2_multi<double,0,16,4,16>", CH_PREC_F64, 0, 16, 4, 16),                          // configs[3]
    multi_row("k_step2_multi<double,0,8,4,16>", CH_PREC_F64, 0, 8, 4, 16),                            // configs[3], 2 per CU
    multi_row("k_step2_multi<double,0,16,2,8>", CH_PREC_F64, 0, 16, 2, 8),                            // configs[2]
    multi_row("k_step2_multi<double,0,4,2,8>", CH_PREC_F64, 0, 4, 2, 8),                              // configs[1]
    multi_row("k_step2_multi<float,0,16,4,16,false,false,4>", CH_PREC_F32, 0, 16, 4, 16, false, false, 4),
    multi_row("k_step2_multi<float,0,16,4,16>", CH_PREC_F32, 0, 16, 4, 16),
    // ch_rollout_collect's fused step
    actor_row("k_step2_actor<double,0,16,4,16,false>", false),
    actor_row("k_step2_actor<double,0,16,4,16,true>", true),
};
#undef CH_STEP2_ROWS
constexpr int kStepKernels = (int)(sizeof(kStepTable) / sizeof(kStepTable[0]));
constexpr int kStepNoRow = -1;
template <class R> constexpr int kPrecision = sizeof(R) == 8 ? CH_PREC_F64 : CH_PREC_F32;   // the table's column for a kernel's R
// rows of `family` and `precision`, and the first of them: each (family, precision) is one run of the table, which
// the launcher arrays of the .hip files are indexed against
constexpr int step_rows(int family, int precision, bool first = false) {
    int n = 0;
    for (int i = 0; i < kStepKernels; ++i)
        if (kStepTable[i].family == family && kStepTable[i].precision == precision) {
            if (first) return i;
            ++n;
        }
    return first ? kStepNoRow : n;
}
// row `i` is the instantiation with these template arguments (the launcher arrays' build-time check)
constexpr bool step_row_is(int i, int family, int precision, int mode, int gt, int nt, int mt, bool phys, bool pw,
                           int tobs_wpe) {
    const StepKernelInfo& k = kStepTable[i];
    return k.family == family && k.precision == precision && k.mode == mode && k.gt == gt && k.nt == nt && k.mt == mt &&
           k.phys == phys && k.pw == pw && k.tobs_wpe == tobs_wpe;
}

// the pipelined step loop's LDS hand-off behind the carve (V2Pipe, ch_step_sync.h: kBytes); rb = sizeof(R)
constexpr int kPipeMetG = 16;      // envs per workgroup of the pipelined instantiation
constexpr int kPipeCounters = 8;   // its launch-long counters
constexpr size_t v2_pipe_bytes(int rb) {
    return (size_t)(kDroneComps + 1 + 7) * 64 * rb + (size_t)kMetricRows * kPipeMetG * sizeof(double) +
           (2 * 64 + kV2Flags + kPipeCounters) * sizeof(int);
}

// ---- the planner (ch_step_plan.cpp): a pure function of the shape, the CU count, the LDS budget and the overrides ----
struct StepShape {
    int mode, N, M;       // CH_MODE_*, num_drones, num_cattle
    int precision;        // CH_PREC_*
    int physics;          // CH_PHYS_*
    long long E;          // envs
};
// what the diagnostics entry points impose on a handle (0: nothing)
struct StepOverrides {
    int kernel = 0;       // ch__set_kernel: 1 or 2
    bool geometry = false;   // ch__set_geometry: G envs per workgroup, `block` threads
    int G = 0, block = 0;
    int phase_mask = 0;   // ch__set_phase_mask: a handle that skips phases takes neither ch_step_n's kernel nor the fused step
};
// the geometry rules, in the order they are applied; a later rule may undo an earlier one
enum StepRule { kRuleGeneric = 0, kRule4x16, kRule2x8, kRulePerWave, kRuleSep, kRuleV1Fallback, kStepRules };
extern const char* const kStepRuleNames[kStepRules];
struct StepPlan {
    int error;            // CH_OK, or why the overrides were refused (CH_ERR_INVALID / CH_ERR_UNSUPPORTED; the rest unset)
    int kernel;           // 1 = team-per-env (ch_kernels.hip), 2 = role-split (ch_step.hip)
    int G, block;         // v2: envs per workgroup, threads
    size_t lds;           // v2: dynamic LDS bytes (V2Layout)
    bool pw, sep;         // v2: per-wave env tables; shared tables with the shepherd terms in their own region
    int step_row[2];      // k_step2's row without / with terminal observations (kStepNoRow on the v1 kernel)
    int multi_row;        // ch_step_n's k_step2_multi row, or kStepNoRow: n launches of the step
    int multi_block;      // its block, clamped to the row's launch bound
    size_t multi_lds;     // its LDS, with the pipelined row's hand-off
    int actor_row[2];     // k_step2_actor's rows without / with terminal observations, or kStepNoRow: the shape does not
                          // take the fused actor step (whether the net does: launch_step_v2_actor)
    unsigned rules;       // bit r: StepRule r changed the geometry
};
StepPlan step_plan(const StepShape& s, int cus, size_t lds_budget, const StepOverrides& ov);
// ch__step_plan's and ch__step_plan_of's `out`
void step_plan_out(const StepPlan& p, int64_t out[13]);

}  // namespace ch
