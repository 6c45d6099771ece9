// ch_norm.hip -- the device side of VecNormalize for the CTDE PPO path (include/cattleherd.h ch_norm_*): running
// float64 statistics of the observations and of the discounted returns, and the elementwise normalisation.
//
// Reference: stable_baselines3 RunningMeanStd.update / update_from_moments and VecNormalize.step_wait / reset /
// normalize_obs / normalize_reward.  (SB3 is not installed here: restated from its source, "parity unpinned".)
//
// Order and determinism.  No floating-point atomics, no grid barrier: every all-to-all seam is a launch boundary, and
// every sum has a fixed order -- a thread adds its rows in row order, one thread adds the row lanes in lane order, the
// sub-blocks of a chunk and then the chunks are merged in index order (Chan's formula).  The same state and input give
// the same bits.  The running statistics are written by one kernel only (k_norm_merge / the reward kernel's one
// thread), in a launch of its own, so no workgroup reads them while another writes them.
//
// Cancellation.  The variance is two-pass inside a 64-row sub-block (the rows stay in registers between the passes)
// and Chan-merged above it, and every moment is taken of x - pivot, the pivot of a column being its first row's value:
// the chunk means are then of the spread's size, not of the offset's, and so is their rounding, which is what the
// between-chunk term delta^2 n_a n_b / n multiplies.  (A column at 1e3 +- 1e-3 otherwise loses ~1e-10 of its variance.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ch_norm.h"

namespace ch {

namespace {

// Chan: the moments (n, m, q = sum of squared deviations) of a set joined with (nb, mb, qb); n, nb > 0
__device__ __forceinline__ void chan_merge(double n, double& m, double& q, double nb, double mb, double qb) {
    const double tot = n + nb, d = mb - m;
    m = m + d * nb / tot;
    q = q + qb + d * d * n * nb / tot;
}

// RunningMeanStd.update_from_moments, operation for operation
__device__ __forceinline__ void update_from_moments(double& mean, double& var, double& count, double bm, double bv,
                                                    double bn) {
    const double delta = bm - mean, tot = count + bn;
    const double m_a = var * count, m_b = bv * bn;
    const double m2 = m_a + m_b + delta * delta * count * bn / tot;
    mean = mean + delta * bn / tot;
    var = m2 / tot;
    count = tot;
}

// np.clip, then the float32 cast (NaN stays NaN)
__device__ __forceinline__ float clip_cast(double q, double c) {
    q = q < -c ? -c : (q > c ? c : q);
    return (float)q;
}

// The thread layout of the two obs kernels: a tile of kNormTile columns, CPT per thread (float4 or scalar loads along
// dim: a row lane reads 256 contiguous bytes), RY row lanes.
template <bool VEC>
struct Lay {
    static constexpr int CPT = VEC ? 4 : 1;
    static constexpr int CX = kNormTile / CPT;
    static constexpr int RY = kNormThreads / CX;
    static constexpr int RPT = kNormBlockRows / RY;
};

template <bool VEC>
__device__ __forceinline__ void load_cols(const float* p, float (&v)[Lay<VEC>::CPT]) {
    if constexpr (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
        v[0] = *p;
    }
}

// ---- batch moments ---------------------------------------------------------------------------------------------
// grid (column tiles, row chunks).  Workgroup (tile, g) leaves the mean and the sum of squared deviations of
// x[rows of chunk g][its columns] - pivot in part_mean[g][col], part_m2[g][col]; tile 0 leaves part_n[g], and
// workgroup (0, 0) the running count as it was (k_norm_merge reads it there, and writes the new one).
template <bool VEC>
__global__ __launch_bounds__(kNormThreads) void k_norm_moments(NormObsArgs a) {
    using L = Lay<VEC>;
    constexpr int CPT = L::CPT, RY = L::RY, RPT = L::RPT;
    __shared__ double sh[RY][kNormTile];
    const int tx = threadIdx.x % L::CX, ry = threadIdx.x / L::CX, lc = tx * CPT;
    const long long col = (long long)blockIdx.x * kNormTile + lc;
    const bool live = col < a.dim;   // (VEC: dim % 4 == 0, so a thread's four columns are live together)
    const long long lo = (long long)blockIdx.y * a.chunk_rows, hi = lo + a.chunk_rows < a.rows ? lo + a.chunk_rows : a.rows;
    double piv[CPT], rm[CPT], rq[CPT];
    {
        float p[CPT];
        for (int c = 0; c < CPT; ++c) p[c] = 0.0f;
        if (live) load_cols<VEC>(a.x + col, p);
        for (int c = 0; c < CPT; ++c) { piv[c] = (double)p[c]; rm[c] = 0.0; rq[c] = 0.0; }
    }
    double rn = 0.0;
    for (long long sb = lo; sb < hi; sb += kNormBlockRows) {
        const long long end = sb + kNormBlockRows < hi ? sb + kNormBlockRows : hi;
        const double nb = (double)(end - sb);
        double v[RPT][CPT], s[CPT];
        for (int c = 0; c < CPT; ++c) s[c] = 0.0;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const long long r = sb + ry + k * RY;
            float f[CPT];
            for (int c = 0; c < CPT; ++c) f[c] = 0.0f;
            const bool ok = live && r < end;
            if (ok) load_cols<VEC>(a.x + r * a.dim + col, f);
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                v[k][c] = ok ? (double)f[c] - piv[c] : 0.0;
                s[c] += v[k][c];
            }
        }
        for (int c = 0; c < CPT; ++c) sh[ry][lc + c] = s[c];
        __syncthreads();
        double m[CPT];
        for (int c = 0; c < CPT; ++c) {
            double t = 0.0;
            for (int y = 0; y < RY; ++y) t += sh[y][lc + c];
            m[c] = t / nb;
        }
        __syncthreads();
        double q[CPT];
        for (int c = 0; c < CPT; ++c) q[c] = 0.0;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (sb + ry + k * RY < end) {
#pragma unroll
                for (int c = 0; c < CPT; ++c) {
                    const double d = v[k][c] - m[c];
                    q[c] += d * d;
                }
            }
        }
        for (int c = 0; c < CPT; ++c) sh[ry][lc + c] = q[c];
        __syncthreads();
        if (ry == 0) {
            for (int c = 0; c < CPT; ++c) {
                double t = 0.0;
                for (int y = 0; y < RY; ++y) t += sh[y][lc + c];
                if (rn == 0.0) { rm[c] = m[c]; rq[c] = t; }
                else chan_merge(rn, rm[c], rq[c], nb, m[c], t);
            }
            rn += nb;
        }
        __syncthreads();
    }
    double* pm = a.scratch + (long long)blockIdx.y * a.dim;
    double* pq = pm + (long long)a.chunks * a.dim;
    if (ry == 0 && live)
        for (int c = 0; c < CPT; ++c) { pm[col + c] = rm[c]; pq[col + c] = rq[c]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double* pn = a.scratch + 2LL * a.chunks * a.dim;
        pn[blockIdx.y] = (double)(hi - lo);
        if (blockIdx.y == 0) pn[a.chunks] = *a.count;
    }
}

// One thread per column: the chunks in index order, then the running update.  The only writer of the running
// statistics; it reads the old count from the scratch (k_norm_moments put it there), so column 0's thread can write
// the new one while other workgroups are still merging.
__global__ __launch_bounds__(kNormTile) void k_norm_merge(NormObsArgs a) {
    const long long col = (long long)blockIdx.x * kNormTile + threadIdx.x;
    if (col >= a.dim) return;
    const long long plane = (long long)a.chunks * a.dim;
    const double *pm = a.scratch, *pq = a.scratch + plane, *pn = a.scratch + 2 * plane;
    double n = pn[0], m = pm[col], q = pq[col];
    for (int g = 1; g < a.chunks; ++g) {
        const double nb = pn[g];
        chan_merge(n, m, q, nb, pm[(long long)g * a.dim + col], pq[(long long)g * a.dim + col]);
        n += nb;
    }
    double mean = a.mean[col], var = a.var[col], count = pn[a.chunks];
    update_from_moments(mean, var, count, (double)a.x[col] + m, q / n, n);
    a.mean[col] = mean;
    a.var[col] = var;
    if (col == 0) *a.count = count;
}

// ---- apply -----------------------------------------------------------------------------------------------------
// grid (column tiles, row blocks of kNormApplyRows).  A thread keeps its columns' mean and sqrt(var + eps) in
// registers over its rows; the quotient is an IEEE float64 division (no reciprocal), as numpy's.
template <bool VEC>
__global__ __launch_bounds__(kNormThreads) void k_norm_apply(NormObsArgs a) {
    using L = Lay<VEC>;
    constexpr int CPT = L::CPT, RY = L::RY;
    const int tx = threadIdx.x % L::CX, ry = threadIdx.x / L::CX;
    const long long col = (long long)blockIdx.x * kNormTile + tx * CPT;
    if (col >= a.dim) return;
    const long long lo = (long long)blockIdx.y * kNormApplyRows, hi = lo + kNormApplyRows < a.rows ? lo + kNormApplyRows : a.rows;
    double mean[CPT], sd[CPT];
    for (int c = 0; c < CPT; ++c) {
        mean[c] = a.passthrough ? 0.0 : a.mean[col + c];
        sd[c] = a.passthrough ? 1.0 : sqrt(a.var[col + c] + a.eps);
    }
    for (long long r = lo + ry; r < hi; r += RY) {
        if (a.row_mask && !a.row_mask[r]) continue;
        float f[CPT], o[CPT];
        load_cols<VEC>(a.x + r * a.dim + col, f);
        for (int c = 0; c < CPT; ++c) o[c] = a.passthrough ? f[c] : clip_cast(((double)f[c] - mean[c]) / sd[c], a.clip);
        float* y = a.y + r * a.dim + col;
        if constexpr (VEC) *reinterpret_cast<float4*>(y) = make_float4(o[0], o[1], o[2], o[3]);
        else *y = o[0];
    }
}

// ---- the reward kernel -----------------------------------------------------------------------------------------
// the workgroup's sum in every thread: a fixed tree over the threads' values
__device__ __forceinline__ double reward_tree(double* sh, double v) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int w = kRewardThreads / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// the pivot of the returns' moments: env 0's new return (from values no launch has written yet)
__device__ __forceinline__ double reward_pivot(const NormRewardArgs& a) { return a.ret[0] * a.gamma + (double)a.reward[0]; }

// ret' = ret gamma + reward of the workgroup's envs (base + t + k * kRewardThreads) into r, and their moments about
// `piv`: count, mean and sum of squared deviations of ret' - piv, in every thread
__device__ __forceinline__ void reward_moments(const NormRewardArgs& a, long long base, double piv, double* sh,
                                               double (&r)[kRewardPer], double& n, double& m, double& q) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kRewardPer; ++k) {
        const long long e = base + threadIdx.x + (long long)k * kRewardThreads;
        r[k] = e < a.n ? a.ret[e] * a.gamma + (double)a.reward[e] : 0.0;
        if (e < a.n) s += r[k] - piv;
    }
    const long long left = a.n - base;
    n = (double)(left < (long long)kRewardThreads * kRewardPer ? left : (long long)kRewardThreads * kRewardPer);
    m = reward_tree(sh, s) / n;
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < kRewardPer; ++k) {
        const long long e = base + threadIdx.x + (long long)k * kRewardThreads;
        if (e < a.n) {
            const double d = (r[k] - piv) - m;
            d2 += d * d;
        }
    }
    q = reward_tree(sh, d2);
}

// steps 4 and 6 for the workgroup's envs: the normalised reward from `var`, ret' stored, zero where done
__device__ __forceinline__ void reward_finish(const NormRewardArgs& a, long long base, const double (&r)[kRewardPer],
                                              double var) {
    const double sd = sqrt(var + a.eps);
#pragma unroll
    for (int k = 0; k < kRewardPer; ++k) {
        const long long e = base + threadIdx.x + (long long)k * kRewardThreads;
        if (e >= a.n) continue;
        const float rw = a.reward[e];
        a.reward_out[e] = a.norm_reward ? clip_cast((double)rw / sd, a.clip) : rw;
        a.ret[e] = (a.terminated[e] | a.truncated[e]) ? 0.0 : r[k];
    }
}

// up to kRewardThreads * kRewardPer envs, training: steps 3, 4 and 6 in one workgroup
__global__ __launch_bounds__(kRewardThreads) void k_norm_reward_one(NormRewardArgs a) {
    __shared__ double sh[kRewardThreads];
    __shared__ double var_now;
    const double piv = reward_pivot(a);
    double r[kRewardPer], n, m, q;
    reward_moments(a, 0, piv, sh, r, n, m, q);   // (its barriers stand between the read of ret[0] above and the stores below)
    if (threadIdx.x == 0) {
        double mean = a.stats[0], var = a.stats[1], count = a.stats[2];
        update_from_moments(mean, var, count, piv + m, q / n, n);
        a.stats[0] = mean; a.stats[1] = var; a.stats[2] = count;
        var_now = var;
    }
    __syncthreads();
    reward_finish(a, 0, r, var_now);
}

// beyond that, three launches: the chunks' moments (nothing of ret or of the statistics is written) ...
__global__ __launch_bounds__(kRewardThreads) void k_norm_reward_part(NormRewardArgs a) {
    __shared__ double sh[kRewardThreads];
    double r[kRewardPer], n, m, q;
    reward_moments(a, (long long)blockIdx.x * kRewardThreads * kRewardPer, reward_pivot(a), sh, r, n, m, q);
    if (threadIdx.x == 0) {
        double* p = a.scratch + 3LL * blockIdx.x;
        p[0] = n; p[1] = m; p[2] = q;
    }
}

// ... one thread merges them in index order and updates the running statistics ...
__global__ void k_norm_reward_merge(NormRewardArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double n = a.scratch[0], m = a.scratch[1], q = a.scratch[2];
    for (int g = 1; g < a.chunks; ++g) {
        const double* p = a.scratch + 3LL * g;
        chan_merge(n, m, q, p[0], p[1], p[2]);
        n += p[0];
    }
    double mean = a.stats[0], var = a.stats[1], count = a.stats[2];
    update_from_moments(mean, var, count, reward_pivot(a) + m, q / n, n);
    a.stats[0] = mean; a.stats[1] = var; a.stats[2] = count;
}

// ... and the elementwise rest (update: ret' is formed again, the same bits; 0: training off, ret stays but for the
// zeroing)
__global__ __launch_bounds__(kRewardThreads) void k_norm_reward_apply(NormRewardArgs a, int update) {
    const long long base = (long long)blockIdx.x * kRewardThreads * kRewardPer;
    double r[kRewardPer];
#pragma unroll
    for (int k = 0; k < kRewardPer; ++k) {
        const long long e = base + threadIdx.x + (long long)k * kRewardThreads;
        r[k] = e < a.n ? (update ? a.ret[e] * a.gamma + (double)a.reward[e] : a.ret[e]) : 0.0;
    }
    reward_finish(a, base, r, a.stats[1]);
}

__global__ __launch_bounds__(kNormThreads) void k_norm_begin(NormBeginArgs a) {
    const long long i = (long long)blockIdx.x * kNormThreads + threadIdx.x;
    if (i < a.dim) { a.mean[i] = 0.0; a.var[i] = 1.0; }
    if (i < a.n) a.ret[i] = 0.0;
    if (i == 0) {
        *a.count = 1e-4;
        a.stats[0] = 0.0; a.stats[1] = 1.0; a.stats[2] = 1e-4;
    }
}

bool vec_ok(const NormObsArgs& a) {
    return a.dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.y)) & 15) == 0;
}

}  // namespace

hipError_t launch_norm_begin(const NormBeginArgs& a, hipStream_t st) {
    const long long n = std::max<long long>(a.dim, std::max<long long>(a.n, 1));
    hipLaunchKernelGGL(k_norm_begin, dim3((unsigned)((n + kNormThreads - 1) / kNormThreads)), dim3(kNormThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_norm_obs_update(const NormObsArgs& a, hipStream_t st) {
    const unsigned tiles = (unsigned)((a.dim + kNormTile - 1) / kNormTile);
    const dim3 grid(tiles, (unsigned)a.chunks);
    if (vec_ok(a)) hipLaunchKernelGGL(k_norm_moments<true>, grid, dim3(kNormThreads), 0, st, a);
    else hipLaunchKernelGGL(k_norm_moments<false>, grid, dim3(kNormThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_norm_merge, dim3(tiles), dim3(kNormTile), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_norm_obs_apply(const NormObsArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.dim + kNormTile - 1) / kNormTile), (unsigned)((a.rows + kNormApplyRows - 1) / kNormApplyRows));
    if (vec_ok(a)) hipLaunchKernelGGL(k_norm_apply<true>, grid, dim3(kNormThreads), 0, st, a);
    else hipLaunchKernelGGL(k_norm_apply<false>, grid, dim3(kNormThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_norm_reward(const NormRewardArgs& a, hipStream_t st) {
    if (!a.training) {
        hipLaunchKernelGGL(k_norm_reward_apply, dim3(a.chunks), dim3(kRewardThreads), 0, st, a, 0);
        return hipGetLastError();
    }
    if (a.chunks == 1) {
        hipLaunchKernelGGL(k_norm_reward_one, dim3(1), dim3(kRewardThreads), 0, st, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_norm_reward_part, dim3(a.chunks), dim3(kRewardThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_norm_reward_merge, dim3(1), dim3(64), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_norm_reward_apply, dim3(a.chunks), dim3(kRewardThreads), 0, st, a, 1);
    return hipGetLastError();
}

}  // namespace ch
