// ch_step_multi.hip — ch_step_n's kernel: n consecutive steps of a handle in one launch (k_step2_multi).
//
// The step is step2_body (ch_step_body.h), the same function k_step2 runs.  This translation unit is compiled with
// machine LICM off (cattleherd/_build.py): with it, the step loop hoisted the body's loop-invariant values (LDS
// addresses, constants) to the loop preheader and held them across the whole step, and configs[3]'s instantiation
// spilled 80-145 VGPRs; without it the body keeps k_step2's register allocation (173 VGPRs, no scratch).
#include "ch_step_body.h"

namespace ch {

// n consecutive steps of the same io in one launch (ch_step_n): each workgroup steps its G envs n times back to back.
// The env groups are independent, so no workgroup waits for another between steps: the launch gap, the wait of every
// step on the grid's slowest workgroup, and the state loads' first-touch latency at workgroup start are paid once per
// launch instead of once per step.  Between two steps a workgroup-scope release (the step's global stores complete),
// s_barrier (every wave is done with the step's LDS) and a workgroup-scope acquire: the waves of a workgroup share the
// CU's vector L1, so the next step's loads see this step's stores (as k_step2_actor's forward does).  Every step is the
// full step2_body: the outputs, the auto-resets and the state are those of n ch_step calls (test_gpu_runtime.py).
// One step.  The parameters come from a device copy (ch_step_n uploads them before the launch): the pointer is made
// uniform (readfirstlane) and read through the constant address space, so every parameter read is a scalar load where
// the step uses it, as from k_step2's kernel arguments (the address of a by-value kernel argument would be a private
// copy).
template <class R>
__device__ __forceinline__ const StepParams<R>& uniform_params(const StepParams<R>* p) {
    const unsigned long long a = (unsigned long long)(uintptr_t)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    using KP = const __attribute__((address_space(4))) StepParams<R>*;
    const KP kp = (KP)(((unsigned long long)hi << 32) | lo);
    return *(const StepParams<R>*)kp;
}
template <class R, int MODE, int GT, int NT, int MT, bool PHYS, bool PW, int ROLE = 0>
__device__ __forceinline__ void step2_once(const StepParams<R>* p, int salt, int kstep = 0) {
    step2_body<R, MODE, GT, NT, MT, PHYS, PW, false, ROLE>(uniform_params(p), salt, kstep);
}

// The instantiation whose step loop is pipelined over two drone waves (configs[3], f64): step k+1's drone chain needs
// only the bodies after chain k and step k's reset decision, so a second drone wave starts it as soon as R_k is
// published, while the first still closes the books of step k (reward, metrics, env write-back) -- see V2Pipe and
// step2_body's ROLE in ch_step_body.h; the counters that replace the barrier between two steps: V2Pipe, ch_step_sync.h.
// Which instantiation that is, and every instantiation's launch bound (CH_MULTI_MAX_BLOCK, CH_MULTI_PIPE_MAX_BLOCK),
// are the kernel table's (ch_step_plan.h multi_pipelined, multi_max_block).
template <class R, int MODE, int GT, int NT, int MT, bool PHYS, bool PW, int WPE>
constexpr bool kMultiPipelined = multi_pipelined(kPrecision<R>, MODE, GT, NT, MT, PHYS, PW, WPE);
// n consecutive steps in one launch (ch_step_n); `pd`: the step's parameters in device memory
// WPE: the waves per SIMD the registers are allocated for (4: two workgroups per CU, for grids of more workgroups than
// CUs -- the f32 mode at 262 144 envs: 395.5 vs 294.4 M env-steps/s; at 4096 envs, one workgroup per CU, the register
// cap only spills: 261.9 vs 297.2 M, profiles/r06/ab/r6n_*)
template <class R, int MODE, int GT, int NT, int MT, bool PHYS, bool PW, int WPE>
constexpr int kMultiMaxBlock = multi_max_block(kMultiPipelined<R, MODE, GT, NT, MT, PHYS, PW, WPE>, PW);
template <class R, int MODE, int GT, int NT, int MT, bool PHYS = false, bool PW = false, int WPE = 1>
__global__ __launch_bounds__((kMultiMaxBlock<R, MODE, GT, NT, MT, PHYS, PW, WPE>))
__attribute__((amdgpu_waves_per_eu(WPE)))
void k_step2_multi(const StepParams<R>* __restrict__ pd, int n_steps) {
    if constexpr (kMultiPipelined<R, MODE, GT, NT, MT, PHYS, PW, WPE>) {
        // Waves 0 and 1 are the drone waves: wave 0 runs the drone role of steps 0, 2, ..., wave 1 of steps 1, 3, ...;
        // the other waves run the cow role of every step.  One barrier per launch (step2_pipe_init); inside the loops
        // every sync is a bounded LDS-counter wait, so an expired wait leaves no wave waiting for another.
        step2_pipe_init<R, MODE, GT, NT, MT>(uniform_params(pd));
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (wave < 2) {
            for (int k = wave; k < n_steps; k += 2) {
                int salt = 0;
                const StepParams<R>* q = pd;
                asm volatile("" : "+s"(salt), "+s"(q));   // (as below)
                step2_once<R, MODE, GT, NT, MT, PHYS, PW, 1>(q, salt, k);
                __builtin_amdgcn_s_setprio(0);   // raised only inside the chain and the books, not while it waits for P_N
            }
        } else {
            for (int k = 0; k < n_steps; ++k) {
                int salt = 0;
                const StepParams<R>* q = pd;
                asm volatile("" : "+s"(salt), "+s"(q));   // (as below)
                step2_once<R, MODE, GT, NT, MT, PHYS, PW, 2>(q, salt, k);
            }
        }
    } else {
    for (int k = 0; k < n_steps; ++k) {
        int salt = 0;
        const StepParams<R>* q = pd;
        asm volatile("" : "+s"(salt), "+s"(q));   // an opaque 0 (step2_body's salt) and parameter pointer, per step
        step2_once<R, MODE, GT, NT, MT, PHYS, PW>(q, salt);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_s_setprio(0);   // (the drone wave's raised priority)
    }
    }
}

// launches row's instantiation with the plan's block (clamped to the launch bound) and LDS (with the pipelined
// instantiation's hand-off): StepPlan::multi_block, multi_lds
template <class R, int MODE, int GT, int NT, int MT, bool PHYS = false, bool PW = false, int WPE = 1>
static hipError_t launch_v2_multi_kernel(const StepParams<R>& p, const StepParams<R>* pd, int block, size_t lds,
                                         hipStream_t st, int n_steps) {
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_relaxed) & bit)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step2_multi<R, MODE, GT, NT, MT, PHYS, PW, WPE>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStepLdsMax);
        if (e != hipSuccess) return e;
        attr_set.fetch_or(bit, std::memory_order_relaxed);
    }
    if (block > kMultiMaxBlock<R, MODE, GT, NT, MT, PHYS, PW, WPE>) return hipErrorInvalidValue;
    dim3 grid((p.E + p.G - 1) / p.G);
    hipLaunchKernelGGL((k_step2_multi<R, MODE, GT, NT, MT, PHYS, PW, WPE>), grid, dim3(block), lds, st, pd, n_steps);
    return hipGetLastError();
}

// k_step2_multi's launchers, one per row of kStepTable's run for R, in the table's order; each is checked against its row
template <class R> using MultiLauncher = hipError_t (*)(const StepParams<R>&, const StepParams<R>*, int, size_t, hipStream_t, int);
template <int I, class R, int MODE, int GT, int NT, int MT, bool PHYS = false, bool PW = false, int WPE = 1>
constexpr MultiLauncher<R> multi_entry() {
    constexpr int row = step_rows(kStepFamMulti, kPrecision<R>, true) + I;
    static_assert(step_row_is(row, kStepFamMulti, kPrecision<R>, MODE, GT, NT, MT, PHYS, PW, WPE) &&
                      kStepTable[row].max_block == kMultiMaxBlock<R, MODE, GT, NT, MT, PHYS, PW, WPE>,
                  "the launcher is its table row's instantiation");
    return &launch_v2_multi_kernel<R, MODE, GT, NT, MT, PHYS, PW, WPE>;
}
template <class R> struct MultiLaunchers;   // (static members: emitted for the host only, where they are used)
template <> struct MultiLaunchers<double> {
    static constexpr MultiLauncher<double> rows[] = {
        multi_entry<0, double, 1, 16, 4, 32, false, true>(), multi_entry<1, double, 0, 16, 4, 16>(),
        multi_entry<2, double, 0, 8, 4, 16>(), multi_entry<3, double, 0, 16, 2, 8>(), multi_entry<4, double, 0, 4, 2, 8>()};
};
template <> struct MultiLaunchers<float> {
    static constexpr MultiLauncher<float> rows[] = {multi_entry<0, float, 0, 16, 4, 16, false, false, 4>(),
                                                    multi_entry<1, float, 0, 16, 4, 16>()};
};
static_assert(sizeof(MultiLaunchers<double>::rows) / sizeof(void*) == step_rows(kStepFamMulti, CH_PREC_F64) &&
              sizeof(MultiLaunchers<float>::rows) / sizeof(void*) == step_rows(kStepFamMulti, CH_PREC_F32),
              "one launcher per k_step2_multi row");

template <class R>
hipError_t launch_step_v2_multi(const StepParams<R>& p, const StepParams<R>* pd, int row, int block, size_t lds,
                                hipStream_t st, int n_steps) {
    const int i = row - step_rows(kStepFamMulti, kPrecision<R>, true);
    if (i < 0 || i >= step_rows(kStepFamMulti, kPrecision<R>)) return hipErrorInvalidValue;
    return MultiLaunchers<R>::rows[i](p, pd, block, lds, st, n_steps);
}

template hipError_t launch_step_v2_multi<double>(const StepParams<double>&, const StepParams<double>*, int, int, size_t,
                                                 hipStream_t, int);
template hipError_t launch_step_v2_multi<float>(const StepParams<float>&, const StepParams<float>*, int, int, size_t,
                                                hipStream_t, int);

}  // namespace ch
