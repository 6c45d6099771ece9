// ch_eval_log.hip — the device-side evaluator log (include/cattleherd.h ch_eval_log_*): one row per logged env and
// step of what the reference logs while is_evaluating is set.
//
// Reference: BaseAviary.update_evaluation_metrics (sb3_envs/BaseAviary.py:1406-1437: drone xy poses and velocities,
// cattle poses and velocities, the per-drone distances, evaluate_herding_effectiveness, ep_time) and the time-out
// evaluation_episode_trigger of CattleAviary._computeTruncated (CattleAviary.py:513-548), as
// cattleherd/evaluation.py restates them (herding_effectiveness, failure_truncation, EvalTracker.after_step).
//
// One wave per logged env, four waves per workgroup: lanes are cows (M <= 64) for the cattle columns and the winding
// number, lanes < N are drones.  A logged env's rows are owned by its wave, so every store is a plain vector store.
// The arithmetic whose sign or comparison decides a logged value is written as evaluation.py writes it, with FP
// contraction off, so it agrees with numpy bit for bit.  (The step kernels keep their own copy of the winding test:
// their device assembly does not depend on this file.)
#include <hip/hip_runtime.h>

#include "ch_internal.h"

namespace ch {

constexpr int kLogWaves = 4, kLogThreads = 64 * kLogWaves;
// _computeTruncated's thresholds (CattleAviary.py:94-97, 513-542; evaluation.py failure_truncation's defaults)
constexpr double kLogTargetAlt = 0.45, kLogMaxAltError = 0.27, kLogCollision = 0.2, kLogMaxFormation = 8.0,
                 kLogMissionBoundary = 15.0;

__global__ __launch_bounds__(kLogThreads) void k_eval_log_begin(EvalLogArgs a) {
    const int s = (int)(blockIdx.x * kLogThreads + threadIdx.x);
    if (s >= a.S) return;
    a.rows[s] = 0;
    a.dropped[s] = 0;
}

// the logged env of this wave: -1 when the wave has none or its index is out of range (error word set)
__device__ __forceinline__ long long log_env(const EvalLogArgs& a, int s, int lane) {
    if (s >= a.S) return -1;
    const long long e = a.sel[s];
    if (e < 0 || e >= a.E) {
        if (lane == 0) atomicOr(a.err, CH_DEVERR_LOG_INDEX);
        return -1;
    }
    return e;
}

// before a step: the cattle velocities the reference's read-back of that step returns, and step_counter (ep_time)
template <class R>
__global__ __launch_bounds__(kLogThreads) void k_eval_log_mark(EvalLogArgs a) {
    const int lane = threadIdx.x & 63;
    const int s = (int)(blockIdx.x * kLogWaves + (threadIdx.x >> 6));
    const long long e = log_env(a, s, lane);
    if (e < 0) return;
    const R* cattle = static_cast<const R*>(a.cattle);
    if (lane < a.M) {
        const double vx = (double)cattle[(2 * a.E + e) * a.M + lane], vy = (double)cattle[(3 * a.E + e) * a.M + lane];
        reinterpret_cast<double2*>(a.start_vxy)[(long long)s * a.M + lane] = make_double2(vx, vy);
    }
    if (lane == 0) a.start_counter[s] = a.envi[1 * a.E + e];
}

#pragma clang fp contract(off)
// evaluate_herding_effectiveness (evaluation.py herding_effectiveness): this lane's cow (px, py) has a non-zero winding
// number w.r.t. the polygon of the first n drones in index order; (dx, dy): lane i holds drone i.  Every lane of the
// wave calls it (the shuffles read the drone lanes).
__device__ __forceinline__ bool log_inside(double px, double py, double dx, double dy, int n) {
    int wn = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const double x1 = __shfl(dx, i), y1 = __shfl(dy, i), x2 = __shfl(dx, j), y2 = __shfl(dy, j);
        const double t1 = (x2 - x1) * (py - y1);
        const double t2 = (px - x1) * (y2 - y1);
        const double il = t1 - t2;
        wn += ((y1 <= py) && (y2 > py) && (il > 0.0)) ? 1 : 0;
        wn -= ((y1 > py) && (y2 <= py) && (il < 0.0)) ? 1 : 0;
    }
    return wn != 0;
}

// conditions 1-4 of _computeTruncated (evaluation.py failure_truncation) for the n live drones: lane i < n holds drone
// i's position, lane j < m cow j's.  Every lane of the wave calls it; every lane returns the env's answer.
__device__ __forceinline__ bool log_failure(double dx, double dy, double dz, double cx, double cy, int n, int m,
                                            int lane) {
    const bool live = lane < n;
    // 1. altitude
    const bool alt = live && fabs(dz - kLogTargetAlt) > kLogMaxAltError;
    // 2. a pair closer than the collision threshold; 3. a drone farther than max_formation from all the others (the
    // distance to itself counts as infinite)
    bool coll = false, iso = true;
    for (int j = 0; j < n; ++j) {
        const double ex = dx - __shfl(dx, j), ey = dy - __shfl(dy, j);
        const double sx = ex * ex, sy = ey * ey;
        const double d = sqrt(sx + sy);
        if (j != lane) {
            coll = coll || d < kLogCollision;
            iso = iso && d > kLogMaxFormation;
        }
    }
    // 4. the two centroids (means in index order) more than mission_boundary apart
    double sdx = 0.0, sdy = 0.0, scx = 0.0, scy = 0.0;
    for (int i = 0; i < n; ++i) { sdx += __shfl(dx, i); sdy += __shfl(dy, i); }
    for (int j = 0; j < m; ++j) { scx += __shfl(cx, j); scy += __shfl(cy, j); }
    const double gx = sdx / (double)n - scx / (double)m, gy = sdy / (double)n - scy / (double)m;
    const double g2x = gx * gx, g2y = gy * gy;
    const bool far = sqrt(g2x + g2y) > kLogMissionBoundary;
    return __any((int)(alt || (live && coll) || (live && iso))) != 0 || far;
}

// after a step (without auto-reset): the row of every logged env, and done_mask for every env
template <class R>
__global__ __launch_bounds__(kLogThreads) void k_eval_log_record(EvalLogArgs a) {
    if (a.done_mask) {   // one thread per env
        const long long g = (long long)blockIdx.x * kLogThreads + threadIdx.x;
        if (g < a.E) a.done_mask[g] = (uint8_t)((a.term[g] | a.trunc[g]) ? 1 : 0);
    }
    const int lane = threadIdx.x & 63;
    const int s = (int)(blockIdx.x * kLogWaves + (threadIdx.x >> 6));
    const long long e = log_env(a, s, lane);
    if (e < 0) return;
    const int r = a.rows[s];
    if (r < 0 || r >= a.T) {   // full: count the step, write nothing
        if (lane == 0) a.dropped[s] = a.dropped[s] + 1;
        return;
    }
    const int N = a.NC, M = a.M;
    const long long E = a.E;
    int n = a.envi[0 * E + e];
    n = n < 0 ? 0 : (n > N ? N : n);
    const R* drone = static_cast<const R*>(a.drone);
    const R* cattle = static_cast<const R*>(a.cattle);
    // this lane's drone and cow (f32 handles: the positions the step carries in f64)
    double dx = 0.0, dy = 0.0, dz = 0.0, dvx = 0.0, dvy = 0.0, dist = 0.0, cx = 0.0, cy = 0.0;
    if (lane < n) {
        const long long i = e * N + lane;
        if constexpr (sizeof(R) == 8) {
            dx = drone[(kRowPos + 0) * E * N + i]; dy = drone[(kRowPos + 1) * E * N + i]; dz = drone[(kRowPos + 2) * E * N + i];
        } else {
            dx = a.pos64[0 * E * N + i]; dy = a.pos64[1 * E * N + i]; dz = a.pos64[2 * E * N + i];
        }
        dvx = (double)drone[(kRowVel + 0) * E * N + i]; dvy = (double)drone[(kRowVel + 1) * E * N + i];
        dist = a.evald[i];
    }
    if (lane < M) {
        const long long j = e * M + lane;
        if constexpr (sizeof(R) == 8) { cx = cattle[0 * E * M + j]; cy = cattle[1 * E * M + j]; }
        else { cx = a.cpos64[0 * E * M + j]; cy = a.cpos64[1 * E * M + j]; }
    }
    const bool inside = log_inside(cx, cy, dx, dy, n);
    const int count = __popcll(__ballot(lane < M && inside));
    const bool failure = log_failure(dx, dy, dz, cx, cy, n, M, lane);
    const long long row = (long long)s * a.T + r;
    if (lane < N) {   // (the slots i >= NUM_DRONES hold zeros)
        reinterpret_cast<double2*>(a.drone_xy)[row * N + lane] = make_double2(dx, dy);
        reinterpret_cast<double2*>(a.drone_vxy)[row * N + lane] = make_double2(dvx, dvy);
        a.drone_dist[row * N + lane] = dist;
    }
    if (lane < M) {
        reinterpret_cast<double2*>(a.cattle_xy)[row * M + lane] = make_double2(cx, cy);
        reinterpret_cast<double2*>(a.cattle_vxy)[row * M + lane] =
            reinterpret_cast<const double2*>(a.start_vxy)[(long long)s * M + lane];
    }
    if (lane == 0) {
        const double ep_time = (double)a.start_counter[s] / (double)a.ctrl_freq;
        const double ratio = (double)count / (double)M;
        a.time[row] = ep_time;
        a.eff[row] = ratio * 100.0;
        a.num_drones[row] = n;
        a.episode[row] = a.envi[8 * E + e];
        a.flags[row] = (uint8_t)((a.term[e] ? 1 : 0) | (a.trunc[e] ? 2 : 0) | ((ep_time > a.episode_len && !failure) ? 4 : 0));
        a.rows[s] = r + 1;
    }
}

// waves: one per logged env and, for the done mask, one per 64 envs
static unsigned log_grid(const EvalLogArgs& a, bool mask) {
    const long long waves_mask = mask ? (a.E + 63) / 64 : 0;
    const long long waves = a.S > waves_mask ? a.S : waves_mask;
    return (unsigned)((waves + kLogWaves - 1) / kLogWaves);
}

hipError_t launch_eval_log_begin(const EvalLogArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_log_begin, dim3((unsigned)((a.S + kLogThreads - 1) / kLogThreads)), dim3(kLogThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_eval_log_mark(const EvalLogArgs& a, bool f32, hipStream_t st) {
    if (f32) hipLaunchKernelGGL(k_eval_log_mark<float>, dim3(log_grid(a, false)), dim3(kLogThreads), 0, st, a);
    else hipLaunchKernelGGL(k_eval_log_mark<double>, dim3(log_grid(a, false)), dim3(kLogThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_eval_log_record(const EvalLogArgs& a, bool f32, hipStream_t st) {
    const unsigned grid = log_grid(a, a.done_mask != nullptr);
    if (f32) hipLaunchKernelGGL(k_eval_log_record<float>, dim3(grid), dim3(kLogThreads), 0, st, a);
    else hipLaunchKernelGGL(k_eval_log_record<double>, dim3(grid), dim3(kLogThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace ch
