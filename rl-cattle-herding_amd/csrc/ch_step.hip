// ch_step.hip — the kernels and launchers of the fused env-step, v2: k_step2 and k_step2_actor around step2_body
// (ch_step_body.h, which holds the design comment; ch_step_sync.h the hand-off primitives, ch_step_flock.h the flock
// math) and one launcher per row of the kernel table (ch_step_plan.h): which row a handle runs is the planner's choice.
#include "ch_step_body.h"
#include "ch_mlp2_dev.h"   // mlp2_body (k_step2_actor)

namespace ch {

template <class R, int MODE, int GT, int NT, int MT, bool PHYS = false, bool PW = false, bool TOBS = false>
__global__ __launch_bounds__((PW || PHYS) ? CH_V2_MAX_BLOCK_PW : CH_V2_MAX_BLOCK)
__attribute__((amdgpu_waves_per_eu((sizeof(R) == 4 && GT > 0 && !PW && !PHYS) ? 4 : 1)))
void k_step2(StepParams<R> p) {
    step2_body<R, MODE, GT, NT, MT, PHYS, PW, TOBS>(p);
}

// The PPO collection step with the actor forward of the next step fused in (ch_rollout_collect, CH_FUSED_ACTOR /
// ch__set_rollout_path bit 2): the workgroup steps its 16 envs, then -- once every wave has written its observation
// stores -- runs the SB3 actor (k_mlp2's body, one 16-row tile, 12 waves of which 8 carry the 128-wide layers' column
// tiles) on the 16 observation rows it has just written, with the sampling epilogue (kRoleSample: actions,
// log-probabilities, the next step's env actions).  The rows are read back through the CU's caches (the stores of
// this workgroup; a workgroup-scope release before the barrier, a workgroup-scope acquire after it),
// the weights stream from L2 as in the separate launch; the LDS of the step is dead by then and the forward's tile
// reuses it.  The critic and its value epilogue stay a separate launch.  Same arithmetic as the separate forward
// (the K order of each output does not depend on the wave count): bit-identical rollouts.
constexpr int kFusedLdsMax = 160 * 1024 - 256;   // k_step2_actor's dynamic LDS cap
struct FusedActor {
    MlpArgs a;
    RolloutArgs ro;
    int lda, ldh;
};
template <class R, int MODE, int GT, int NT, int MT, bool TOBS>
__global__ __launch_bounds__(CH_V2_MAX_BLOCK)
void k_step2_actor(StepParams<R> p, FusedActor f) {
    // diagnostics (ch__set_mlp_tstamp): wall clocks of the workgroup's start, barrier and end in slots 13-15
    long long* ts = f.a.tstamp && threadIdx.x == 0 ? f.a.tstamp + (long long)blockIdx.x * 16 : nullptr;
    if (ts) ts[13] = (long long)wall_clock64();
    step2_body<R, MODE, GT, NT, MT, false, false, TOBS>(p);
    // workgroup scope both ways: the waves of a workgroup share the CU's vector L1, so the release's store-counter
    // wait makes every observation store visible to the forward's loads after the barrier (an agent-scope acquire
    // would also invalidate this XCD's L2 -- measured: the forward's first weight loads then waited ~17 us)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    __builtin_amdgcn_s_setprio(0);   // (the drone wave's raised priority)
    if (ts) ts[14] = (long long)wall_clock64();
    mlp2_body<CH_V2_MAX_BLOCK / 64, 1, 1>(f.a, (long long)blockIdx.x, f.lda, f.ldh, kRoleSample, f.ro, StepOfRo{f.ro});
    if (ts) ts[15] = (long long)wall_clock64();
}

template <class R, int MODE, int GT, int NT, int MT, bool PHYS = false, bool PW = false, bool TOBS = false>
static hipError_t launch_v2_kernel(const StepParams<R>& p, int block, size_t lds, hipStream_t st, bool launch) {
    // opt-in to > 64 KiB of dynamic LDS, once per device (the attribute is per device context)
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_relaxed) & bit)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step2<R, MODE, GT, NT, MT, PHYS, PW, TOBS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStepLdsMax);
        if (e != hipSuccess) return e;
        attr_set.fetch_or(bit, std::memory_order_relaxed);
    }
    if (!launch) return hipSuccess;
    dim3 grid((p.E + p.G - 1) / p.G);
    hipLaunchKernelGGL((k_step2<R, MODE, GT, NT, MT, PHYS, PW, TOBS>), grid, dim3(block), lds, st, p);
    return hipGetLastError();
}

// k_step2's launchers, one per row of kStepTable's run for R, in the table's order; each is checked against its row
template <class R> using StepLauncher = hipError_t (*)(const StepParams<R>&, int, size_t, hipStream_t, bool);
template <int I, class R, int MODE, int GT, int NT, int MT, bool PHYS = false, bool PW = false, bool TOBS = false>
constexpr StepLauncher<R> step_entry() {
    static_assert(step_row_is(step_rows(kStepFamStep, kPrecision<R>, true) + I, kStepFamStep, kPrecision<R>, MODE, GT, NT,
                              MT, PHYS, PW, TOBS), "the launcher is its table row's instantiation");
    return &launch_v2_kernel<R, MODE, GT, NT, MT, PHYS, PW, TOBS>;
}
template <class R>
constexpr StepLauncher<R> kStepLaunchers[] = {
    step_entry<0, R, 1, 0, 0, 0, true>(),           step_entry<1, R, 0, 16, 4, 16, true>(),
    step_entry<2, R, 0, 0, 0, 0, true>(),           step_entry<3, R, 1, 16, 4, 32, false, true>(),
    step_entry<4, R, 1, 0, 0, 0, false, true>(),    step_entry<5, R, 0, 0, 0, 0, false, true>(),
    step_entry<6, R, 1, 0, 0, 0>(),                 step_entry<7, R, 0, 8, 4, 16>(),
    step_entry<8, R, 0, 16, 4, 16, false, false, true>(), step_entry<9, R, 0, 16, 4, 16>(),
    step_entry<10, R, 0, 16, 2, 8>(),               step_entry<11, R, 0, 4, 2, 8>(),
    step_entry<12, R, 0, 0, 0, 0>(),
};
static_assert(sizeof(kStepLaunchers<double>) / sizeof(void*) == step_rows(kStepFamStep, CH_PREC_F64) &&
              sizeof(kStepLaunchers<float>) / sizeof(void*) == step_rows(kStepFamStep, CH_PREC_F32),
              "one launcher per k_step2 row");

template <class R>
hipError_t launch_step_v2(const StepParams<R>& p, int row, int block, size_t lds, hipStream_t st, bool launch) {
    const int i = row - step_rows(kStepFamStep, kPrecision<R>, true);
    if (i < 0 || i >= step_rows(kStepFamStep, kPrecision<R>)) return hipErrorInvalidValue;
    return kStepLaunchers<R>[i](p, block, lds, st, launch);
}
template hipError_t launch_step_v2<double>(const StepParams<double>&, int, int, size_t, hipStream_t, bool);

template <class R, bool TOBS>
static hipError_t launch_actor_kernel(const StepParams<R>& p, int block, size_t lds, hipStream_t st, const FusedActor& f,
                                      bool launch) {
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_relaxed) & bit)) {
        // (the forward's static words -- kmax, kany, the row slots -- sit beside the dynamic LDS)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step2_actor<R, 0, 16, 4, 16, TOBS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kFusedLdsMax);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        attr_set.fetch_or(bit, std::memory_order_relaxed);
    }
    if (!launch) return hipSuccess;
    hipLaunchKernelGGL((k_step2_actor<R, 0, 16, 4, 16, TOBS>), dim3((p.E + 15) / 16), dim3(block), lds, st, p, f);
    return hipGetLastError();
}

constexpr hipError_t (*kActorLaunchers[])(const StepParams<double>&, int, size_t, hipStream_t, const FusedActor&, bool) = {
    &launch_actor_kernel<double, false>, &launch_actor_kernel<double, true>};
static_assert(sizeof(kActorLaunchers) / sizeof(void*) == step_rows(kStepFamActor, CH_PREC_F64) &&
              step_row_is(step_rows(kStepFamActor, CH_PREC_F64, true), kStepFamActor, CH_PREC_F64, 0, 16, 4, 16, false, false, 0) &&
              step_row_is(step_rows(kStepFamActor, CH_PREC_F64, true) + 1, kStepFamActor, CH_PREC_F64, 0, 16, 4, 16, false, false, 1),
              "one launcher per k_step2_actor row: <double, 0, 16, 4, 16, TOBS>");

// the shape's half of the fused step's conditions is the planner's (StepPlan::actor_row); the net's is here
hipError_t launch_step_v2_actor(const StepParams<double>& p, int row, int block, size_t lds, hipStream_t st,
                                const MlpArgs& a, const RolloutArgs& ro, bool launch) {
    const int i = row - step_rows(kStepFamActor, CH_PREC_F64, true);
    if (i < 0 || i >= step_rows(kStepFamActor, CH_PREC_F64)) return hipErrorInvalidValue;
    if (a.rows != p.E) return hipErrorNotSupported;
    FusedActor f;
    size_t mb = 0;
    if (!mlp2_fused_tile(a, f.lda, f.ldh, mb)) return hipErrorNotSupported;
    f.a = a;
    // (diagnostics, ch__set_mlp_tstamp: the forward's phase clocks in the buffer's second half, rows [grid, 2 grid),
    // so that the separate launches of the same collection, which use the first, do not overwrite them)
    f.a.tstamp = g_mlp_tstamp ? g_mlp_tstamp + 16LL * ((p.E + 15) / 16) : nullptr;
    f.ro = ro;
    const size_t l = lds > mb ? lds : mb;
    if (l > (size_t)kFusedLdsMax) return hipErrorNotSupported;
    return kActorLaunchers[i](p, block, l, st, f, launch);
}

#ifdef CH_COUNT_SPINS
// (diagnostic builds) read and clear the k_step2 spin counters: out[0..3] = drone-wave sleeps, cow-wave sleeps,
// drone-wave waits, cow-wave waits
extern "C" int ch__spin_counts(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ch_spins), sizeof(g_ch_spins)) != hipSuccess) return -1;
    const unsigned long long z[4] = {0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_ch_spins), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

template hipError_t launch_step_v2<float>(const StepParams<float>&, int, int, size_t, hipStream_t, bool);

}  // namespace ch
