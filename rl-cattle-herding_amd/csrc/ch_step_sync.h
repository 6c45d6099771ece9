// ch_step_sync.h — the step kernels' synchronisation: LDS-only barriers and hand-off counters, the diagnostics' stamp
// macros, and the pipelined step loop's launch-long protocol (V2Pipe).  Included by ch_step_body.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ch_step_plan.h"   // (ch_internal.h; the kernel table and v2_pipe_bytes)

namespace ch {


// workgroup barrier that orders LDS only (no wait for outstanding global stores)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// LDS writes of this wave visible to its other lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// called convergently by a whole wave: its LDS writes are published, then the counter is bumped once
__device__ __forceinline__ void lds_signal(int* f) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(f, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int lds_peek(int* f) {
    return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// a hand-off that never completed: the kernel goes on (never a hang) and the handle's device error
// word records it; ch_metrics / ch_get_state / ch_sync return CH_ERR_DEVICE from then on
__device__ __forceinline__ void handoff_failed(int* err) {
    if (err && (threadIdx.x & 63) == 0) atomicOr(err, CH_DEVERR_HANDOFF);
}
// diagnostics (-DCH_COUNT_SPINS builds only, tools/spin_split.py): sleep iterations of the hand-off waits, per wave
// kind (drone wave, cow waves), and the number of waits, summed over every k_step2 launch since the last read
#ifdef CH_COUNT_SPINS
static __device__ unsigned long long g_ch_spins[4];
__device__ __forceinline__ void spin_note(int n) {
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x < 64 ? 0 : 1;
        atomicAdd(&g_ch_spins[w], (unsigned long long)n);
        atomicAdd(&g_ch_spins[2 + w], 1ull);
    }
}
#else
__device__ __forceinline__ void spin_note(int) {}
#endif
// spin until *f >= target (bounded, about 0.1 s)
__device__ __forceinline__ void lds_wait(int* f, int target, int* err) {
    int spins = 0;
    while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target && ++spins < (1 << 22))
        __builtin_amdgcn_s_sleep(1);
    if (spins >= (1 << 22)) handoff_failed(err);
    spin_note(spins);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Dynamic share-out of a cow-wave loop: each call hands the calling wave the next n items of the
// counter.  The cow waves do not run at equal speed (one of them shares its SIMD with the other
// resident workgroup's prioritised drone wave), so a static lane -> item split leaves the slowest
// wave with as many items as the fastest.
__device__ __forceinline__ int grab(int* ctr, int n, bool skip = false) {
    if (skip) return 1 << 28;   // (wave-uniform) this wave takes no more items of the loop
    int b = 0;
    if ((threadIdx.x & 63) == 0) b = atomicAdd(ctr, n);
    return __builtin_amdgcn_readfirstlane(b);
}

// barrier among the cow waves only (the drone wave keeps running); `global` also publishes their
// global stores (needed before other cow lanes rewrite the same state)
__device__ __forceinline__ void cow_sync(int* f, int waves, bool global, int* err) {
    if (global) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    lds_signal(f);
    lds_wait(f, waves, err);
    if (global) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// diagnostics: per-workgroup timestamps (slots: 0/1 wall clock at start/end, 2 shader clock at start,
// 3 after the first barrier, 4 drone chain done, 5 reward terms done, 6 herded flags received,
// 7 bookkeeping done, 8 cow waves: alpha rows done, 9 drone positions received, 10 velocity update
// done, 11 obs copy done, 12 CU id, 13 second barrier, 14 end)
#define TS(slot, val) do { if (!PIPE && p.tstamp) p.tstamp[(long long)blockIdx.x * 128 + (slot)] = (val); } while (0)
// diagnostics: per cow wave 1..6, chunks taken and cycles spent in each dynamic loop (slots 64 + 10 (w - 1) + 2 loop)
#define CHUNK_T0 const long long ck0_ = (!PIPE && p.tstamp) ? (long long)clock64() : 0
// diagnostics: the latest of the cow waves at a point (per-workgroup max of the shader clock in slot `slot`)
#define TS_MAX(slot) do { if (!PIPE && p.tstamp && (threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned long long*>(p.tstamp + (long long)blockIdx.x * 128 + (slot)), (unsigned long long)clock64()); } while (0)
#define CHUNK_T1(loop) do { if (!PIPE && p.tstamp && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) <= 6) { long long* q_ = p.tstamp + (long long)blockIdx.x * 128 + 64 + 10 * ((threadIdx.x >> 6) - 1) + 2 * (loop); q_[0] += 1; q_[1] += (long long)clock64() - ck0_; } } while (0)

// (step2_body's PIPE instantiations write none of the slots above: its waves are in different steps at once.)  The
// pipelined step loop's own stamps, 16 slots per step for the first 8 steps of a launch (slot 16 k + i), shader clock:
//   drone wave of step k: 0 at the P_N wait (step 0: launch start), 1 chain start, 2 D published, 3 H received,
//   4 R published, 5 P_N signalled, 6 env scalars written back (P_B), 7 books closed (P_K), with the wave's SIMD in
//   bits 62-63
//   cow waves: 8 first cow wave enters step k (at the P_B wait), 9 past P_B and P_C, 10 waits for D, 11 D seen,
//   12 flock work done, waits for R (first cow wave), 13 the same, latest cow wave, 14 R seen (first cow wave),
//   15 step end, latest cow wave
#define PTS(i, val) do { if (PIPE && p.tstamp && kstep < 8) p.tstamp[(long long)blockIdx.x * 128 + 16 * kstep + (i)] = (val); } while (0)
// The first cow wave's split of "enters step k" .. "waits for D", in a second table behind the first (the pipelined
// kernel's stamp buffer is [2 grid][128]: row grid + workgroup, slot 16 k + i): 0 staging done (past F_E), 1 its cheap
// pass done, 2 its full pass done, 3 its first alpha-row chunk taken (0: none before D)
#define PTSS(i, val) do { if (PIPE && p.tstamp && kstep < 8) p.tstamp[((long long)gridDim.x + blockIdx.x) * 128 + 16 * kstep + (i)] = (val); } while (0)
#define PTS_MAX(i) do { if (PIPE && p.tstamp && kstep < 8 && (threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned long long*>(p.tstamp + (long long)blockIdx.x * 128 + 16 * kstep + (i)), (unsigned long long)clock64()); } while (0)

// LDS of the pipelined step loop (k_step2_multi, configs[3] f64), placed after the V2Layout carve:
//   ho   [27][64]  per drone lane: the 26 state reals after the chain (a reset env: its new body; rows kRowPos .. kRowLink,
//                  ch_internal.h) and evald's accumulator (kRowEvalDist)
//   hoi  [2][64]   NUM_DRONES of the lane's env for the next step, the Philox step counter
//   d1   [7][64]   the odd steps' copy of S.dx, dy, dz, dq (the even steps use the V2Layout arrays)
//   met  [kMetricRows][16]  the metric rows of the workgroup's envs, owned by the books waves for the length of the
//                  launch: staged from global memory by the cow waves in step 0 only (before F_E of step 0), then read,
//                  updated and written back by the books wave of every step (which also stores them to global memory
//                  every step).  The cow waves never touch them after step 0.
//   flags1 [kV2Flags]  the odd steps' hand-off and work counters (the even steps: S.flags)
//   sync           counters that run over the whole launch, never cleared inside it:
//       P_N  = steps whose hand-off is final       (drone wave k -> drone wave k+1; target k+1)
//       P_B  = steps whose env scalars are written back (drone wave k -> cow waves; target k+1).  It guards the global
//              rows envi / envr / stale / obs_tag, which the cow waves load on entering step k+1, and the LDS rows they
//              restage there (S.ei, S.prev, S.clock and the cow and pair tables): the books wave of step k reads none
//              of them after this signal.  It does not say that the books are closed.
//       P_C  = cow waves done with a step, summed  (cow waves among themselves; target W1 (k+1))
//       P_K  = steps whose books are closed        (drone wave k -> cow waves and drone wave k+1; target k+1): the
//              reward, term / trunc, metrics and episode records of step k are stored (released at workgroup scope) and
//              that wave is done with S.dcow (the closest-cow search) and X.met.  The cow waves wait for it before the
//              per-cow pass of step k+1, the first thing that overwrites S.dcow; the books wave of step k+1 waits for
//              it before it touches X.met or stores to the rows above.
//       P_SIMD + w = 1 + the SIMD of drone wave w
// Invariant: step k uses counter set k & 1; that set is zero when step k's first signal can arrive (step 0 and 1: cleared
// before the launch's only barrier; step k >= 2: cleared by the cow waves on entering step k-1, step2_body's phase 0).
// S.LT and S.pl (the curriculum table and the pair list) are constant: staged once per launch (step2_pipe_init), so the
// books wave may read LT whatever step the cow waves are in.
//
// The protocol.  No workgroup barrier separates two steps; three orderings replace it, carried by the members below and by
// the two waits on entering a step (step2_body's phase 0: the cow waves' P_B and P_C with the clear, the drone wave's P_N;
// as members they changed the pipelined kernel's generated code, so they stay written out there):
//   (a) step k's loads come after step k-1's stores.  The cow waves enter step k behind P_B of step k-1 (the books wave's
//       write-back of envi, envr, stale, obs_tag, released at workgroup scope by a wave that reads none of the LDS rows
//       the cow waves restage after it) and behind P_C (a cow-wave barrier that publishes every cow wave's global stores
//       of its final pass).  The drone wave enters step k behind P_N of step k-1 (the chain state in ho / hoi is final).
//       The books of step k-1 may still be open then: their wave reads only its registers, the constant S.LT, met (never
//       touched by the cow waves after step 0) and S.dcow, which step k overwrites only behind its P_K wait.
//   (b) the counter set of step k-1 is cleared for step k+1 once every wave is done with it: the cow waves by P_C, the
//       books wave by P_B (behind it that wave signals only P_K, a launch-long counter).  Step k+1's drone wave touches
//       the set only after R of step k, which follows step k's F_E and F_H, which follow the clear.
//   (c) the outputs of step k are ordered after those of step k-1 through P_K: the cow waves wait for it ahead of step
//       k's cow items (F_H), which the books of step k wait for, and the books wave of step k waits for P_K itself
//       before its output stores.
// What a drone wave does between its P_N wait and its P_K signal is step2_body's drone part; the members are called there in
// the order (P_N wait), publish_next, publish_scalars, await_prev_books, close_books.
template <class R> struct V2Smem;
template <class R>
struct V2Pipe {
    enum { P_N = 0, P_B, P_C, P_SIMD, P_K = P_SIMD + 2, P_COUNT = kPipeCounters };
    static_assert(P_K < P_COUNT, "launch-long counters");
    static constexpr int kMetG = kPipeMetG;   // envs per workgroup of the pipelined instantiation
    static constexpr int kHoRows = kDroneComps + 1;   // the chain state's rows and kRowEvalDist
    // (kHoRows + 7) * 64 reals, the metric rows, 2 * 64 + kV2Flags + P_COUNT ints: sized where the planner reads it too
    static constexpr size_t kBytes = v2_pipe_bytes(sizeof(R));
    R *ho, *d1;
    double* met;
    int *hoi, *flags1, *sync;
    __device__ explicit V2Pipe(unsigned char* base) {
        ho = (R*)base; d1 = ho + kHoRows * 64;
        met = (double*)(d1 + 7 * 64);
        hoi = (int*)(met + kMetricRows * kMetG); flags1 = hoi + 2 * 64; sync = flags1 + kV2Flags;
    }
    // An odd step's copy of the arrays the cow waves read from the drone wave (S.dx, dy, dz, dq), and its set of hand-off
    // counters; an even step uses the V2Layout arrays and S.flags.  GN = G * N.
    __device__ __forceinline__ void select_step(V2Smem<R>& S, int kstep, int GN) const {
        if (kstep & 1) {
            S.dx = d1; S.dy = S.dx + GN; S.dz = S.dy + GN; S.dq = S.dz + GN;
            S.dxd = (double*)S.dx; S.dyd = (double*)S.dy;
            S.flags = flags1;
        }
    }
    // P_N: the hand-off is final (R_k is known, the reset envs' new bodies are in) -- the other drone wave starts chain
    // k+1.  A workgroup-scope release: this wave's stores of step k to the drone state and the observation rows are
    // complete before that wave stores step k+1's to the same addresses.
    __device__ __forceinline__ void publish_next() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        lds_signal(sync + P_N);
    }
    // P_B: the env scalars of step k are written back (released at workgroup scope) and this wave reads none of S.ei,
    // S.prev, S.clock or the cow tables any more: the cow waves may load step k+1's env scalars and restage those rows.
    // The books stay open (see P_K).
    __device__ __forceinline__ void publish_scalars() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        lds_signal(sync + P_B);
    }
    // P_K of step k-1, waited for by both roles of step k > 0 (expected never to spin: those books closed a whole chain
    // ago, within a fraction of a step).  Drone wave, ahead of its books: the other drone wave stored to the addresses
    // this wave stores to next (reward, term, trunc, metrics, episode records) and owned met until then.  Cow waves, ahead
    // of the per-cow pass: it is the first thing in the step that overwrites S.dcow, which that books wave's closest-cow
    // search reads; and since F_H of this step is signalled behind this wait, every output store of the books of step k
    // follows those of step k-1 (c).
    __device__ __forceinline__ void await_prev_books(int kstep, int* err) const {
        if (kstep > 0) {
            lds_wait(sync + P_K, kstep, err);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
    // P_K: the books of step k are closed -- every output store of this step is released at workgroup scope, met holds the
    // step's rows and this wave is done with S.dcow.
    __device__ __forceinline__ void close_books() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        lds_signal(sync + P_K);
    }
};

}  // namespace ch
