// ch_ppo.hip -- one minibatch step of SB3 PPO.train for the CTDE driver's ActorCriticPolicy
// (CTDECattleHerder.py:107-150; cattleherd/ppo.py restates it: _loss, evaluate_actions, _sgd), float32 on the matrix
// cores (v_mfma_f32_16x16x4_f32: exact f32 products, a k-ordered fma chain per output element, ch_policy.hip's
// operand maps).  Weights are read and written in nn.Linear layout, in place.
//
// Three launches per step, one per all-to-all seam (no grid barrier, no atomics on floats, every sum in a fixed
// order: two runs from the same state give the same bits):
//   k_ppo_fb    one workgroup per (16-row tile, net): advantage statistics, gather by index, forward with the
//               hidden activations in LDS, the loss gradient, backward to every layer's dZ; hidden activations and dZ
//               go to scratch, with per-tile partial sums of the loss terms and of the log_std gradient.
//   k_ppo_dw    one workgroup per (layer, 16 output rows, 256 input columns): dW = dZ^T A over the minibatch rows (A
//               gathered from obs again for the first layer), the bias gradient, log_std's gradient in a workgroup
//               of its own; each workgroup writes the sum of squares of what it produced.
//   k_ppo_adam  every workgroup sums those partials in the same order, forms clip_grad_norm_'s coefficient and runs
//               torch's Adam on its slice.  The step count was incremented by k_ppo_dw, so the loop over minibatches
//               is stream-ordered with no host sync.
//
// The three kernels take a compile-time flavour (ch_ppo.h).  kPpoRllib is the minibatch step of RLlib's PPO learner for
// the DTDE driver's shared policy (cattleherd/marl_ppo.py restates it): the head is [mean, raw log_std], the loss adds
// the KL penalty against the gathered old dist inputs and clips the value error, k_ppo_dw has no log_std workgroup and
// k_ppo_adam a no-clip mode and five statistics.  kPpoSb3 is the step described above; for
// ch_ppo_train_log a third k_ppo_fb instantiation (kFbSb3Log) also leaves per-tile sums of SB3's two diagnostics
// (approx_kl, clip_fraction), which k_ppo_adam turns into two more statistics.  For
// ch_marl_ppo_train_log a fourth flavour (kPpoRllibLog) of k_ppo_fb and k_ppo_adam adds RLlib's vf_loss_unclipped,
// total_loss and vf_explained_var.
//
// MFMA operand map (16x16x4 f32): lane l gives A[row l & 15][k slot l >> 4] and B[k slot l >> 4][col l & 15]; it
// holds C/D[row 4 (l >> 4) + r][col l & 15] in register r.  Which k a slot stands for is free as long as A and B
// agree, so a lane loads four consecutive k as one float4 and feeds element j to the j-th MFMA of the chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "ch_ppo.h"

namespace ch {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kFbWaves = 8;              // k_ppo_fb: 512 threads, one 16-column tile per wave and pass
constexpr int kLdh = kPpoMaxHidden + 4;  // LDS row stride of the hidden buffers (16-byte aligned rows)
constexpr int kLdo = kPpoMaxAct + 4;     // of the head's output
constexpr int kDwWaves = 4;              // k_ppo_dw: 256 threads, 64 input columns per wave
constexpr int kDwCols = 64 * kDwWaves;
constexpr float kHalfLog2Pi = 0.91893853320467274178f;   // log(sqrt(2 pi))
constexpr double kHalfLog2Pi64 = 0.91893853320467274178;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// every lane gets the wave's sum, added in the butterfly's fixed order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sum in every thread: waves in index order
__device__ __forceinline__ float block_sum(float v, float* red, int nw) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.0f;
    for (int i = 0; i < nw; ++i) s += red[i];
    __syncthreads();
    return s;
}

// p[k .. k + 3] of a row of K floats starting at p, zero past K: clamped (always valid) addresses and a select, so
// that the loops below stay branch-free and unroll.  VEC: K % 4 == 0 and p 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* p, int k, int K) {
    if constexpr (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(p + min(k, K - 4));
        return k < K ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        const float x = p[min(k, K - 1)], y = p[min(k + 1, K - 1)], z = p[min(k + 2, K - 1)], w = p[min(k + 3, K - 1)];
        return make_float4(k < K ? x : 0.0f, k + 1 < K ? y : 0.0f, k + 2 < K ? z : 0.0f, k + 3 < K ? w : 0.0f);
    }
}

// C[16][16] = A[16][K] W[col0 .. col0 + 15][K]^T: `arow` is this lane's row (l & 15) of A, `wrow` its row of W
template <bool VEC>
__device__ __forceinline__ f32x4 fwd_tile_t(const float* arow, const float* wrow, int K) {
    const int g = (threadIdx.x & 63) >> 4;
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    // four chunks of 16 k per pass, their loads issued before the first multiply (chunks past K load zeros)
    // (trip counts are wave-uniform: an MFMA needs every lane, so the lane's k offset is added inside)
    for (int k0 = 0; k0 < K; k0 += 64) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = ld4<VEC>(arow, k0 + 16 * u + 4 * g, K);
            b[u] = ld4<VEC>(wrow, k0 + 16 * u + 4 * g, K);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = mfma4(a[u].x, b[u].x, acc0);
            acc1 = mfma4(a[u].y, b[u].y, acc1);
            acc0 = mfma4(a[u].z, b[u].z, acc0);
            acc1 = mfma4(a[u].w, b[u].w, acc1);
        }
    }
    return acc0 + acc1;
}

__device__ __forceinline__ f32x4 fwd_tile(const float* arow, const float* wrow, bool vec, int K) {
    return vec ? fwd_tile_t<true>(arow, wrow, K) : fwd_tile_t<false>(arow, wrow, K);
}

// C[16][16] = dZ[16][N] W[N][col0 .. col0 + 15]: dz in LDS (row stride ld), W in nn.Linear layout [N][H]
__device__ __forceinline__ f32x4 bwd_tile(const float* dz, int ld, int N, const float* W, int H, int col0) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int n0 = 0; n0 < N; n0 += 32) {   // 32 rows of W per pass (rows past N: clamped loads, zero dz)
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int n = n0 + 4 * u + g, cn = min(n, N - 1);
            av[u] = dz[c * ld + cn];
            bv[u] = W[(long long)cn * H + col0 + c];
            av[u] = n < N ? av[u] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            acc0 = mfma4(av[u], bv[u], acc0);
            acc1 = mfma4(av[u + 1], bv[u + 1], acc1);
        }
    }
    return acc0 + acc1;
}

struct FbArgs {
    PpoNet n;
    PpoData d;
    const long long* idx;
    long long batch;
    float* scratch;
    PpoScratch s;
    float clip_range, vf_coef;
    int normalize;
    int vec_obs;       // obs rows take float4 loads
    int vec_w[2][3];   // so do layer li's weight rows of net ni
    // kPpoRllib
    float ent_coef, vf_clip, ls_clip;
    const float* kl_coeff_dev;
};

// k_ppo_fb's third flavour (ch_ppo_train_log): kPpoSb3 plus the per-tile sums of SB3's two diagnostics.  A kernel of
// its own, so that ch_ppo_train's carries none of the float64 code.
constexpr int kFbSb3Log = 2;
// the fourth, of k_ppo_fb and of the Adam kernel (ch_marl_ppo_train_log): kPpoRllib plus what RLlib's learner record
// lacks in the five statistics -- the critic workgroups leave the loss's coefficients, each tile's sum of unclipped
// squared value errors and each row's (value, target) in the scratch region `misc` (unused by kPpoRllib otherwise:
// [4] coefficients, [tiles] sums, [bp][2] rows), and k_ppo_adam turns them into vf_loss_unclipped, total_loss and
// vf_explained_var.
// Kernels of their own, so that ch_marl_ppo_train launches what it launched before.
constexpr int kPpoRllibLog = 3;
constexpr bool ppo_rllib(int F) { return F == kPpoRllib || F == kPpoRllibLog; }

// per-tile loss partials: the surrogate and the squared value error; kPpoRllib adds the entropy and the KL
template <int F>
constexpr int kStat = ppo_rllib(F) ? 4 : 2;

template <int F>
__global__ __launch_bounds__(64 * kFbWaves) void k_ppo_fb(FbArgs a) {
    [[maybe_unused]] constexpr bool kLog = F == kFbSb3Log;
    __shared__ __align__(16) float hs[2][kPpoTile * kLdh];   // hidden activations
    __shared__ __align__(16) float dzs[kPpoTile * kLdh];     // dZ of the last hidden layer
    __shared__ __align__(16) float os[kPpoTile * kLdo];      // the head's output, then its dZ
    __shared__ float tmp[kPpoTile * kLdo];                   // per-row log_std gradient terms
    __shared__ float red[kFbWaves];
    __shared__ float rowstat[kPpoTile];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, ni = blockIdx.y;
    const PpoMlp& net = a.n.net[ni];
    const int L = net.layers, B = (int)a.batch;
    const long long row0 = (long long)tile * kPpoTile;
    const float inv_b = 1.0f / (float)B;

    // the minibatch's advantage statistics (policy net only): torch's mean and unbiased std, two passes
    float adv_mean = 0.0f, adv_scale = 1.0f;
    if (ni == 0 && a.normalize && B > 1) {
        float s = 0.0f;
        for (int i = tid; i < B; i += 64 * kFbWaves) s += a.d.advantages[a.idx[i]];
        adv_mean = block_sum(s, red, kFbWaves) * inv_b;
        float q = 0.0f;
        for (int i = tid; i < B; i += 64 * kFbWaves) {
            const float t = a.d.advantages[a.idx[i]] - adv_mean;
            q += t * t;
        }
        const float var = block_sum(q, red, kFbWaves) / (float)(B - 1);
        adv_scale = 1.0f / (sqrtf(var) + 1e-8f);
    }

    // forward.  Rows past the minibatch read its last row: finite values that meet dZ = 0.
    const long long my_row = a.idx[min(row0 + c, a.batch - 1)];
    const float* xrow = a.d.obs + my_row * a.n.obs_dim;
    for (int li = 0; li < L; ++li) {
        const int K = net.dims[li], N = net.dims[li + 1];
        const bool head = li == L - 1;
        const float* arow = li == 0 ? xrow : hs[li - 1] + c * kLdh;
        // (hidden activations: aligned LDS rows; readfirstlane: the branch around the MFMA loop stays scalar)
        const bool vec = __builtin_amdgcn_readfirstlane(a.vec_w[ni][li] && (li > 0 || a.vec_obs)) != 0;
        for (int t = wave; t < (N + 15) / 16; t += kFbWaves) {
            const int col = t * 16 + c;
            const f32x4 acc = fwd_tile(arow, net.w[li] + (long long)min(col, N - 1) * K, vec, K);
            if (col < N) {
                const float bv = net.b[li][col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * g + r;
                    const float z = acc[r] + bv;
                    if (head) {
                        os[row * kLdo + col] = z;
                    } else {
                        const float h = tanhf(z);
                        hs[li][row * kLdh + col] = h;
                        a.scratch[a.s.act[ni][li] + (row0 + row) * N + col] = h;
                    }
                }
            }
        }
        __syncthreads();
    }

    // the loss and its gradient with respect to the head's output, rows past the minibatch 0
    const int NO = net.dims[L];
    if constexpr (ppo_rllib(F)) {
        if (ni == 0) {
            // 16 lanes per row.  The head is [mean (A), raw log_std (A)], log_std = the raw value clamped to +-ls_clip
            // (torch.clamp: the gradient passes inside the closed range).  Per row: the log-probability of the stored
            // action, the entropy, and KL(sampling policy || this one) against the gathered old dist inputs.
            const int row = tid >> 4, sub = tid & 15, A = NO >> 1;
            if (row < kPpoTile) {
                const bool valid = row0 + row < a.batch;
                const long long src = a.idx[min(row0 + row, a.batch - 1)];
                float lp = 0.0f, ent = 0.0f, kl = 0.0f;
                for (int j = sub; j < A; j += 16) {
                    const float mu = os[row * kLdo + j];
                    const float ls = fminf(fmaxf(os[row * kLdo + A + j], -a.ls_clip), a.ls_clip);
                    const float mu_p = a.d.old_dist[src * NO + j], ls_p = a.d.old_dist[src * NO + A + j];
                    const float var = expf(2.0f * ls), dlt = a.d.actions[src * A + j] - mu, dm = mu_p - mu;
                    lp += -(dlt * dlt) / (2.0f * var) - ls - kHalfLog2Pi;
                    ent += ls + 0.5f + kHalfLog2Pi;
                    kl += ls - ls_p + (expf(2.0f * ls_p) + dm * dm) / (2.0f * var) - 0.5f;
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    lp += __shfl_xor(lp, o);
                    ent += __shfl_xor(ent, o);
                    kl += __shfl_xor(kl, o);
                }
                const float adv = a.d.advantages[src];   // standardised once per training iteration by the caller
                const float ratio = expf(lp - a.d.old_log_prob[src]);
                const float s1 = adv * ratio;
                const float s2 = adv * fminf(fmaxf(ratio, 1.0f - a.clip_range), 1.0f + a.clip_range);
                const float dlp = valid && s1 <= s2 ? -inv_b * adv * ratio : 0.0f;   // (torch.min: see kPpoSb3 below)
                const float klc = valid ? *a.kl_coeff_dev * inv_b : 0.0f, entc = valid ? a.ent_coef * inv_b : 0.0f;
                if (sub == 0) {
                    rowstat[row] = valid ? fminf(s1, s2) : 0.0f;
                    tmp[row] = valid ? ent : 0.0f;
                    tmp[kPpoTile + row] = valid ? kl : 0.0f;
                }
                for (int j = sub; j < A; j += 16) {   // (each lane reads, then overwrites, its own columns)
                    const float mu = os[row * kLdo + j], raw = os[row * kLdo + A + j];
                    const float ls = fminf(fmaxf(raw, -a.ls_clip), a.ls_clip);
                    const float mu_p = a.d.old_dist[src * NO + j], ls_p = a.d.old_dist[src * NO + A + j];
                    const float var = expf(2.0f * ls), dlt = a.d.actions[src * A + j] - mu, dm = mu_p - mu;
                    const float dls = dlp * (dlt * dlt / var - 1.0f) - entc + klc * (1.0f - (expf(2.0f * ls_p) + dm * dm) / var);
                    os[row * kLdo + j] = dlp * dlt / var - klc * dm / var;
                    os[row * kLdo + A + j] = raw >= -a.ls_clip && raw <= a.ls_clip ? dls : 0.0f;
                }
            }
        } else if (tid < kPpoTile) {
            // clamp((V - R)^2, 0, vf_clip): the gradient passes where the squared error is inside the closed range
            const bool valid = row0 + tid < a.batch;
            const long long src = a.idx[min(row0 + tid, a.batch - 1)];
            const float err = os[tid * kLdo] - a.d.returns[src], e2 = err * err;
            if constexpr (F == kPpoRllibLog) {
                // the training log's share of the row: the squared error before the clamp (`tmp` is free in a critic
                // workgroup), and the value and its target as the loss used them, for the explained variance
                tmp[tid] = valid ? e2 : 0.0f;
                float* vy = a.scratch + a.s.misc + 4 + a.s.tiles + 2 * (row0 + tid);
                vy[0] = os[tid * kLdo];
                vy[1] = a.d.returns[src];
            }
            rowstat[tid] = valid ? fminf(e2, a.vf_clip) : 0.0f;
            os[tid * kLdo] = valid && e2 <= a.vf_clip ? a.vf_coef * 2.0f * err * inv_b : 0.0f;
        }
        __syncthreads();
        if (tid == 0) {
            float s = 0.0f, e = 0.0f, k = 0.0f;
            for (int r = 0; r < kPpoTile; ++r) s += rowstat[r];
            a.scratch[a.s.tile_stat + 4 * tile + ni] = s;
            if (ni == 0) {
                for (int r = 0; r < kPpoTile; ++r) {
                    e += tmp[r];
                    k += tmp[kPpoTile + r];
                }
                a.scratch[a.s.tile_stat + 4 * tile + 2] = e;
                a.scratch[a.s.tile_stat + 4 * tile + 3] = k;
            }
            if (F == kPpoRllibLog && ni == 1) {   // the tile's unclipped squared errors, rows in order
                float u = 0.0f;
                for (int r = 0; r < kPpoTile; ++r) u += tmp[r];
                a.scratch[a.s.misc + 4 + tile] = u;
                if (tile == 0) {   // and the loss's coefficients, as this kernel used them
                    a.scratch[a.s.misc] = a.vf_coef;
                    a.scratch[a.s.misc + 1] = a.ent_coef;
                    a.scratch[a.s.misc + 2] = *a.kl_coeff_dev;
                }
            }
        }
    } else {
        if (ni == 0) {
            // 16 lanes per row: log-probability of the stored action under N(mean, exp(log_std))
            const int row = tid >> 4, sub = tid & 15;
            if (row < kPpoTile) {
                const bool valid = row0 + row < a.batch;
                const long long src = a.idx[min(row0 + row, a.batch - 1)];
                float lp = 0.0f;
                // (lp64, kFbSb3Log: the same log-probability from the same float32 mean, widened exactly and summed in
                // float64, for approx_kl alone -- see below; the loss keeps the float32 one)
                double lp64 = 0.0;
                for (int j = sub; j < NO; j += 16) {
                    const float ls = a.n.log_std[j], dlt = a.d.actions[src * NO + j] - os[row * kLdo + j];
                    lp += -(dlt * dlt) / (2.0f * expf(2.0f * ls)) - ls - kHalfLog2Pi;
                    if constexpr (kLog) {
                        const double ls64 = ls, d64 = (double)a.d.actions[src * NO + j] - (double)os[row * kLdo + j];
                        lp64 += -(d64 * d64) / (2.0 * exp(2.0 * ls64)) - ls64 - kHalfLog2Pi64;
                    }
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    lp += __shfl_xor(lp, o);
                    if constexpr (kLog) lp64 += __shfl_xor(lp64, o);
                }
                float adv = a.d.advantages[src];
                if (a.normalize && B > 1) adv = (adv - adv_mean) * adv_scale;
                const float log_ratio = lp - a.d.old_log_prob[src];
                const float ratio = expf(log_ratio);
                const float s1 = adv * ratio;
                const float s2 = adv * fminf(fmaxf(ratio, 1.0f - a.clip_range), 1.0f + a.clip_range);
                // torch.min's gradient goes to the smaller branch (both when they tie: inside the clip range, where the
                // clamp passes it on); the clamped branch outside the range has none
                const float dlp = valid && s1 <= s2 ? -inv_b * adv * ratio : 0.0f;
                if (sub == 0) {
                    rowstat[row] = valid ? fminf(s1, s2) : 0.0f;
                    if constexpr (kLog) {
                        // SB3's diagnostics of the row (PPO.train's approx_kl_divs and clip_fractions), in the two
                        // columns of `tmp` past the widest head: (ratio - 1) - log_ratio, and |ratio - 1| > clip_range
                        // as 0 / 1.  The first cancels: it is ~log_ratio^2 / 2, so the float32 rounding of a
                        // log-probability of magnitude 10-20 and of the ratio is ~1e-5 of it in a one-row minibatch.
                        // It is evaluated in float64 from lp64 and rounded once; the clip test is the loss's own ratio.
                        const double lr64 = lp64 - (double)a.d.old_log_prob[src];
                        tmp[row * kLdo + kPpoMaxAct] = valid ? (float)(expm1(lr64) - lr64) : 0.0f;
                        tmp[row * kLdo + kPpoMaxAct + 1] = valid && fabsf(ratio - 1.0f) > a.clip_range ? 1.0f : 0.0f;
                    }
                }
                for (int j = sub; j < NO; j += 16) {
                    const float var = expf(2.0f * a.n.log_std[j]);
                    const float dlt = a.d.actions[src * NO + j] - os[row * kLdo + j];
                    tmp[row * kLdo + j] = dlp * (dlt * dlt / var - 1.0f);
                    os[row * kLdo + j] = dlp * dlt / var;   // d loss / d mean (each lane its own columns)
                }
            }
        } else if (tid < kPpoTile) {
            const bool valid = row0 + tid < a.batch;
            const long long src = a.idx[min(row0 + tid, a.batch - 1)];
            const float err = os[tid * kLdo] - a.d.returns[src];
            rowstat[tid] = valid ? err * err : 0.0f;
            os[tid * kLdo] = valid ? a.vf_coef * 2.0f * err * inv_b : 0.0f;
        }
        __syncthreads();
        if (tid == 0) {
            float s = 0.0f;
            for (int r = 0; r < kPpoTile; ++r) s += rowstat[r];
            a.scratch[a.s.tile_stat + 2 * tile + ni] = s;
            if (kLog && ni == 0) {   // the tile's diagnostics, rows in order, behind the [tiles][2] loss partials
                float kl = 0.0f, cf = 0.0f;
                for (int r = 0; r < kPpoTile; ++r) {
                    kl += tmp[r * kLdo + kPpoMaxAct];
                    cf += tmp[r * kLdo + kPpoMaxAct + 1];
                }
                a.scratch[a.s.tile_stat + 2 * a.s.tiles + 2 * tile] = kl;
                a.scratch[a.s.tile_stat + 2 * a.s.tiles + 2 * tile + 1] = cf;
            }
            if (ni == 0 && tile == 0) {
                float e = 0.0f;
                for (int j = 0; j < NO; ++j) e += 0.5f + kHalfLog2Pi + a.n.log_std[j];
                a.scratch[a.s.misc] = e;   // the entropy is the same for every row
            }
        }
        if (ni == 0 && tid < NO) {
            float s = 0.0f;
            for (int r = 0; r < kPpoTile; ++r) s += tmp[r * kLdo + tid];
            a.scratch[a.s.tile_dls + (long long)tile * NO + tid] = s;
        }
    }
    for (int i = tid; i < kPpoTile * NO; i += 64 * kFbWaves) {
        const int r = i / NO, j = i - r * NO;
        a.scratch[a.s.dz[ni][L - 1] + (row0 + r) * NO + j] = os[r * kLdo + j];
    }

    // backward through the hidden layers: dZ[li] = (dZ[li + 1] W[li + 1]) (1 - h^2)
    for (int li = L - 2; li >= 0; --li) {
        const int H = net.dims[li + 1], N = net.dims[li + 2];
        const float* dz_in = li == L - 2 ? os : dzs;
        const int ld_in = li == L - 2 ? kLdo : kLdh;
        for (int t = wave; t < H / 16; t += kFbWaves) {
            const int col = t * 16 + c;
            const f32x4 acc = bwd_tile(dz_in, ld_in, N, net.w[li + 1], H, t * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const float h = hs[li][row * kLdh + col];
                const float dz = acc[r] * (1.0f - h * h);
                if (li > 0) dzs[row * kLdh + col] = dz;   // (read by the next pass: the first pass reads `os`)
                a.scratch[a.s.dz[ni][li] + (row0 + row) * H + col] = dz;
            }
        }
        __syncthreads();
    }
}

// one weight matrix's gradient: dW[N][K] = dz[bp][N]^T act[bp][K]
struct DwGemm {
    const float* dz;
    const float* act;     // NULL: rows of obs gathered by idx
    float* gw;
    float* gb;
    int N, K;
    int vec_act, vec_out;
    int wg0, kgroups;     // its workgroups are [wg0, wg0 + tiles(N) * kgroups)
};

struct DwArgs {
    DwGemm g[6];
    int ng, wg_ls;        // the workgroup of log_std's gradient
    const float* obs;
    const long long* idx;
    long long batch;
    int bp, tiles, act_dim;
    const float* tile_dls;
    float* g_ls;
    float ent_coef;
    float* partial;
    long long* step_dev;
};

// A operand: dz[b][n0 + c]; B operand: act[b][kw0 + 4 c + j] for the j-th accumulator, so register r of accumulator j
// is dW[n0 + 4 g + r][kw0 + 4 c + j]; bsum: this lane's share of the column sum of dz (the bias gradient)
template <bool VEC, bool GATHER>
__device__ __forceinline__ void dw_loop(const DwArgs& a, const DwGemm& G, int n0, int kw0, f32x4 (&acc)[4], float& bsum) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int N = G.N, K = G.K, ncol = min(n0 + c, N - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    bsum = 0.0f;
    for (int b0 = 0; b0 < a.bp; b0 += 16) {   // bp is a multiple of 16: four chunks of 4 rows per pass
        float dz[4];
        float4 av[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long b = b0 + 4 * u + g;
            dz[u] = G.dz[b * N + ncol];
            const float* arow = GATHER ? a.obs + a.idx[min(b, a.batch - 1)] * K : G.act + b * K;
            av[u] = ld4<VEC>(arow, kw0 + 4 * c, K);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bsum += dz[u];
            acc[0] = mfma4(dz[u], av[u].x, acc[0]);
            acc[1] = mfma4(dz[u], av[u].y, acc[1]);
            acc[2] = mfma4(dz[u], av[u].z, acc[2]);
            acc[3] = mfma4(dz[u], av[u].w, acc[3]);
        }
    }
}

template <int F>
__global__ __launch_bounds__(64 * kDwWaves) void k_ppo_dw(DwArgs a) {
    __shared__ float red[kDwWaves];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x;
    if (wg == 0 && tid == 0 && a.step_dev) *a.step_dev += 1;   // the Adam step this gradient is for
    float ss = 0.0f;
    if (F == kPpoSb3 && wg == a.wg_ls) {   // (kPpoRllib: log_std is a head output, its gradient part of the GEMMs)
        // log_std: the tiles' partials in order, and the entropy bonus (-ent_coef * mean entropy: -ent_coef each)
        if (tid < a.act_dim) {
            float s = 0.0f;
            for (int t = 0; t < a.tiles; ++t) s += a.tile_dls[(long long)t * a.act_dim + tid];
            s -= a.ent_coef;
            a.g_ls[tid] = s;
            ss = s * s;
        }
    } else {
        int gi = 0;
        for (int i = 1; i < a.ng; ++i)
            if (wg >= a.g[i].wg0) gi = i;
        const DwGemm& G = a.g[gi];
        const int local = wg - G.wg0, nt = local / G.kgroups, kg = local - nt * G.kgroups;
        // wave-uniform by construction (blockIdx, kernel arguments); readfirstlane keeps the branches around the
        // MFMA loops scalar, so that every lane takes part in them
        const int N = __builtin_amdgcn_readfirstlane(G.N), K = __builtin_amdgcn_readfirstlane(G.K);
        const bool gather = __builtin_amdgcn_readfirstlane(G.act == nullptr) != 0;
        const bool vec_act = __builtin_amdgcn_readfirstlane(G.vec_act) != 0;
        const int n0 = 16 * nt, kw0 = __builtin_amdgcn_readfirstlane(kg * kDwCols + wave * 64);
        if (kw0 < K) {
            f32x4 acc[4];   // (dw_loop: register r of accumulator j is dW[n0 + 4 g + r][kw0 + 4 c + j])
            float bsum;
            if (gather) {
                if (vec_act) dw_loop<true, true>(a, G, n0, kw0, acc, bsum);
                else dw_loop<false, true>(a, G, n0, kw0, acc, bsum);
            } else if (vec_act) {
                dw_loop<true, false>(a, G, n0, kw0, acc, bsum);
            } else {
                dw_loop<false, false>(a, G, n0, kw0, acc, bsum);
            }
            const int k = kw0 + 4 * c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 4 * g + r;
                if (n >= N) continue;
                float* dst = G.gw + (long long)n * K + k;
                if (G.vec_out && k < K) {
                    *reinterpret_cast<float4*>(dst) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k + j < K) dst[j] = acc[j][r];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k + j < K) ss += acc[j][r] * acc[j][r];
            }
            // the bias: the column sums of dz, the four row classes in the order (0 + 1) + (2 + 3)
            float t = bsum + __shfl_xor(bsum, 16);
            t += __shfl_xor(t, 32);
            if (kg == 0 && wave == 0 && g == 0 && n0 + c < N) {
                G.gb[n0 + c] = t;
                ss += t * t;
            }
        }
    }
    const float total = block_sum(ss, red, kDwWaves);
    if (tid == 0) a.partial[wg] = total;
}

// the sum-of-squares partials of a given flat gradient (ch_ppo_adam)
__global__ __launch_bounds__(256) void k_ppo_sumsq(const float* __restrict__ grad, long long n, float* partial,
                                                   long long* step_dev) {
    __shared__ float red[4];
    if (blockIdx.x == 0 && threadIdx.x == 0 && step_dev) *step_dev += 1;
    float s = 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += grad[i] * grad[i];
    const float total = block_sum(s, red, 4);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

struct AdamSeg {
    float* p;
    long long off, n;
};

struct AdamArgs {
    AdamSeg seg[kPpoMaxSeg];
    int nseg;
    long long n_params;
    const float* grad;
    float* m;
    float* v;
    const long long* step_dev;
    const float* partial;
    int n_partials;
    double lr, beta1, beta2, eps, max_grad_norm;   // kPpoRllib: max_grad_norm <= 0 is no clip (coefficient exactly 1)
    // statistics (stats4 NULL: none): [policy loss, value loss, mean entropy, unclipped gradient norm]; kPpoRllib has
    // five: [policy loss, clipped value loss, mean entropy, mean KL, unclipped gradient norm]
    float* stats4;
    const float* tile_stat;
    const float* misc;
    int tiles;
    long long batch;
    int update;           // 0: statistics only; kPpoSb3: bit 1 set = stats4 is [CH_PPO_LOG_STATS], with approx_kl and
                          // clip_fraction (ch_ppo_train_log)
};

// the workgroup's two sums in sy[0], sd[0]: a fixed tree over its 256 threads
__device__ __forceinline__ void tree_sum2(double* sy, double* sd, double y, double d) {
    const int t = threadIdx.x;
    sy[t] = y; sd[t] = d;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { sy[t] += sy[t + w]; sd[t] += sd[t + w]; }
        __syncthreads();
    }
}

// The three statistics ch_marl_ppo_train_log adds, by workgroup 0 (all of its threads get here) after stats4[0..4]:
// vf_loss_unclipped from the tiles' sums in index order; total_loss as the reference's _loss forms it, in float64
// from the four float32 means; vf_explained_var = max(-1, 1 - var(y - v) / (var(y) + 1e-6)) with unbiased variances
// (RLlib's explained_variance(value_targets, values)).  The differences cancel, so both variances are two-pass float64
// sums over the exactly widened float32 y and v, thread t adding rows t, t + 256, ... and a fixed tree the threads;
// a one-row minibatch gives 0 / 0 = NaN, which the comparison below keeps (fmax would not).  Everything comes from the
// scratch region `misc` as k_ppo_fb<kPpoRllibLog> left it: the loss's three coefficients, the tiles' sums, the rows.
__device__ __forceinline__ void rllib_log_stats(const AdamArgs& a) {
    __shared__ double sy[256], sd[256];
    const int tid = threadIdx.x;
    const float* log = a.misc + 4;
    const float* vy = log + a.tiles;
    double y = 0.0, d = 0.0;
    for (long long i = tid; i < a.batch; i += 256) {
        const double v = vy[2 * i], r = vy[2 * i + 1];
        y += r; d += r - v;
    }
    tree_sum2(sy, sd, y, d);
    const double my = sy[0] / (double)a.batch, md = sd[0] / (double)a.batch;
    __syncthreads();
    y = 0.0; d = 0.0;
    for (long long i = tid; i < a.batch; i += 256) {
        const double v = vy[2 * i], r = vy[2 * i + 1];
        y += (r - my) * (r - my); d += (r - v - md) * (r - v - md);
    }
    tree_sum2(sy, sd, y, d);
    if (tid != 0) return;
    float u = 0.0f;
    for (int t = 0; t < a.tiles; ++t) u += log[t];
    a.stats4[5] = u / (float)a.batch;
    a.stats4[6] = (float)((double)a.stats4[0] + (double)a.misc[0] * (double)a.stats4[1] -
                          (double)a.misc[1] * (double)a.stats4[2] +
                          (double)a.misc[2] * (double)a.stats4[3]);   // (thread 0 wrote the four just above)
    const double n1 = (double)(a.batch - 1);
    const double ev = 1.0 - (sd[0] / n1) / (sy[0] / n1 + 1e-6);
    a.stats4[7] = (float)(ev < -1.0 ? -1.0 : ev);
}

template <int F>
__global__ __launch_bounds__(256) void k_ppo_adam(AdamArgs a) {
    __shared__ float red[4];
    __shared__ float sc[4];
    const int tid = threadIdx.x;
    float s = 0.0f;
    for (int i = tid; i < a.n_partials; i += 256) s += a.partial[i];
    const float sumsq = block_sum(s, red, 4);
    const float norm = sqrtf(sumsq);
    if (blockIdx.x == 0 && tid == 0 && a.stats4) {
        float pl = 0.0f, vl = 0.0f, en = 0.0f, kl = 0.0f;
        for (int t = 0; t < a.tiles; ++t) {
            pl += a.tile_stat[kStat<F> * t];
            vl += a.tile_stat[kStat<F> * t + 1];
            if constexpr (ppo_rllib(F)) {
                en += a.tile_stat[4 * t + 2];
                kl += a.tile_stat[4 * t + 3];
            }
        }
        a.stats4[0] = -pl / (float)a.batch;
        a.stats4[1] = vl / (float)a.batch;
        if constexpr (ppo_rllib(F)) {
            a.stats4[2] = en / (float)a.batch;
            a.stats4[3] = kl / (float)a.batch;
            a.stats4[4] = norm;
        } else {
            a.stats4[2] = a.misc[0];
            a.stats4[3] = norm;
            if (a.update & 2) {   // the tiles' diagnostics in index order (k_ppo_fb wrote them behind the loss partials)
                float akl = 0.0f, cf = 0.0f;
                for (int t = 0; t < a.tiles; ++t) {
                    akl += a.tile_stat[2 * a.tiles + 2 * t];
                    cf += a.tile_stat[2 * a.tiles + 2 * t + 1];
                }
                a.stats4[4] = akl / (float)a.batch;
                a.stats4[5] = cf / (float)a.batch;
            }
        }
    }
    if constexpr (F == kPpoRllibLog) {
        if (blockIdx.x == 0 && (a.update & 2)) rllib_log_stats(a);   // (ch_marl_ppo_train_log: stats4 is required)
    }
    if (!a.update) return;
    if (tid == 0) {
        // torch Adam's scalars in double, as its (non-capturable) step computes them on the host
        const double t = (double)*a.step_dev;
        const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
        sc[0] = (float)fmin(1.0, a.max_grad_norm / ((double)norm + 1e-6));   // clip_grad_norm_
        if (ppo_rllib(F) && !(a.max_grad_norm > 0.0)) sc[0] = 1.0f;     // grad_clip None
        sc[1] = (float)(a.lr / bc1);
        sc[2] = (float)(1.0 / sqrt(bc2));
    }
    __syncthreads();
    const float coef = sc[0], step_size = sc[1], inv_sqrt_bc2 = sc[2];
    const float b2 = (float)a.beta2, w1 = (float)(1.0 - a.beta1), w2 = (float)(1.0 - a.beta2);
    const float eps = (float)a.eps;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < a.n_params; i += (long long)gridDim.x * 256) {
        int si = 0;
        for (int j = 1; j < a.nseg; ++j)
            if (i >= a.seg[j].off) si = j;
        float* p = a.seg[si].p + (i - a.seg[si].off);
        const float gr = a.grad[i] * coef;
        const float m = a.m[i] + (gr - a.m[i]) * w1;          // exp_avg.lerp_(grad, 1 - beta1)
        const float v = a.v[i] * b2 + w2 * gr * gr;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        a.m[i] = m;
        a.v[i] = v;
        const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
        *p = *p - step_size * (m / denom);
    }
}

int dw_tiles(int n) { return (n + 15) / 16; }
int dw_kgroups(int k) { return (k + kDwCols - 1) / kDwCols; }

int dw_workgroups(const PpoNet& n) {
    int wg = n.flavour == kPpoSb3 ? 1 : 0;   // log_std
    for (int ni = 0; ni < 2; ++ni)
        for (int li = 0; li < n.net[ni].layers; ++li) wg += dw_tiles(n.net[ni].dims[li + 1]) * dw_kgroups(n.net[ni].dims[li]);
    return wg;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int kSumsqGrid = 128;

}  // namespace

void ppo_scratch_layout(const PpoNet& n, long long batch, PpoScratch& s) {
    std::memset(&s, 0, sizeof(s));
    s.tiles = (int)((batch + kPpoTile - 1) / kPpoTile);
    s.bp = s.tiles * kPpoTile;
    long long o = 0;
    auto take = [&](long long floats) { const long long at = o; o += (floats + 3) / 4 * 4; return at; };   // 16-byte steps
    for (int ni = 0; ni < 2; ++ni) {
        const PpoMlp& m = n.net[ni];
        for (int li = 0; li < m.layers; ++li) {
            if (li < m.layers - 1) s.act[ni][li] = take((long long)s.bp * m.dims[li + 1]);
            s.dz[ni][li] = take((long long)s.bp * m.dims[li + 1]);
        }
    }
    s.tile_stat = take(4LL * s.tiles);
    s.tile_dls = take(n.flavour == kPpoSb3 ? (long long)s.tiles * n.act_dim : 0);
    s.misc = take(n.flavour == kPpoSb3 ? 4 : 4 + s.tiles + 2LL * s.bp);
    s.partial = take(std::max(dw_workgroups(n), kSumsqGrid));
    s.grad = take(n.n_params);
    s.total = o;
}

hipError_t ppo_launch_grad(const PpoNet& n, const PpoHp& hp, const PpoData& d, const long long* idx, long long batch,
                           float* grad, float* scratch, const PpoScratch& s, long long* step_dev, int* n_partials,
                           hipStream_t st, bool log_stats) {
    FbArgs f;
    std::memset(&f, 0, sizeof(f));
    f.n = n; f.d = d; f.idx = idx; f.batch = batch; f.scratch = scratch; f.s = s;
    f.clip_range = (float)hp.clip_range; f.vf_coef = (float)hp.vf_coef;
    f.normalize = hp.normalize_advantage;
    f.ent_coef = (float)hp.ent_coef; f.vf_clip = (float)hp.vf_clip; f.ls_clip = (float)hp.log_std_clip;
    f.kl_coeff_dev = hp.kl_coeff_dev;
    f.vec_obs = n.obs_dim % 4 == 0 && aligned16(d.obs);
    for (int ni = 0; ni < 2; ++ni)
        for (int li = 0; li < n.net[ni].layers; ++li) f.vec_w[ni][li] = n.net[ni].dims[li] % 4 == 0 && aligned16(n.net[ni].w[li]);
    const bool rllib = n.flavour == kPpoRllib;
    hipLaunchKernelGGL(rllib ? (log_stats ? k_ppo_fb<kPpoRllibLog> : k_ppo_fb<kPpoRllib>)
                             : (log_stats ? k_ppo_fb<kFbSb3Log> : k_ppo_fb<kPpoSb3>),
                       dim3((unsigned)s.tiles, 2), dim3(64 * kFbWaves), 0, st, f);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    DwArgs w;
    std::memset(&w, 0, sizeof(w));
    int wg = 0;
    for (int ni = 0; ni < 2; ++ni) {
        const PpoMlp& m = n.net[ni];
        for (int li = 0; li < m.layers; ++li) {
            DwGemm& G = w.g[w.ng++];
            G.dz = scratch + s.dz[ni][li];
            G.act = li == 0 ? nullptr : scratch + s.act[ni][li - 1];
            G.gw = grad + m.goff_w[li];
            G.gb = grad + m.goff_b[li];
            G.N = m.dims[li + 1]; G.K = m.dims[li];
            G.vec_act = li == 0 ? f.vec_obs : (aligned16(G.act) ? 1 : 0);
            G.vec_out = G.K % 4 == 0 && aligned16(G.gw);
            G.wg0 = wg; G.kgroups = dw_kgroups(G.K);
            wg += dw_tiles(G.N) * G.kgroups;
        }
    }
    w.wg_ls = rllib ? -1 : wg++;
    w.obs = d.obs; w.idx = idx; w.batch = batch; w.bp = s.bp; w.tiles = s.tiles; w.act_dim = n.act_dim;
    w.tile_dls = scratch + s.tile_dls; w.g_ls = grad + n.goff_log_std; w.ent_coef = (float)hp.ent_coef;
    w.partial = scratch + s.partial; w.step_dev = step_dev;
    hipLaunchKernelGGL(rllib ? k_ppo_dw<kPpoRllib> : k_ppo_dw<kPpoSb3>, dim3((unsigned)wg), dim3(64 * kDwWaves), 0, st, w);
    *n_partials = wg;
    return hipGetLastError();
}

hipError_t ppo_launch_sumsq(const PpoNet& n, const float* grad, float* scratch, const PpoScratch& s, long long* step_dev,
                            int* n_partials, hipStream_t st) {
    hipLaunchKernelGGL(k_ppo_sumsq, dim3(kSumsqGrid), dim3(256), 0, st, grad, n.n_params, scratch + s.partial, step_dev);
    *n_partials = kSumsqGrid;
    return hipGetLastError();
}

static void adam_common(AdamArgs& a, const PpoNet& n, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                        float* stats) {
    std::memset(&a, 0, sizeof(a));
    for (int ni = 0; ni < 2; ++ni) {
        const PpoMlp& m = n.net[ni];
        for (int li = 0; li < m.layers; ++li) {
            a.seg[a.nseg++] = AdamSeg{m.w[li], m.goff_w[li], (long long)m.dims[li + 1] * m.dims[li]};
            a.seg[a.nseg++] = AdamSeg{m.b[li], m.goff_b[li], (long long)m.dims[li + 1]};
        }
    }
    if (n.flavour == kPpoSb3) a.seg[a.nseg++] = AdamSeg{n.log_std, n.goff_log_std, (long long)n.act_dim};
    // by offset, for the kernel's scan (the flat order interleaves the two nets' heads after both MLPs)
    std::sort(a.seg, a.seg + a.nseg, [](const AdamSeg& x, const AdamSeg& y) { return x.off < y.off; });
    a.n_params = n.n_params;
    a.partial = scratch + s.partial; a.n_partials = n_partials;
    a.stats4 = stats; a.tile_stat = scratch + s.tile_stat; a.misc = scratch + s.misc; a.tiles = s.tiles; a.batch = batch;
}

hipError_t ppo_launch_adam(const PpoNet& n, const PpoHp& hp, const float* grad, float* m, float* v,
                           const long long* step_dev, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                           float* stats, hipStream_t st, bool log_stats) {
    AdamArgs a;
    adam_common(a, n, scratch, s, n_partials, batch, stats);
    a.grad = grad; a.m = m; a.v = v; a.step_dev = step_dev;
    a.lr = hp.lr; a.beta1 = hp.beta1; a.beta2 = hp.beta2; a.eps = hp.eps; a.max_grad_norm = hp.max_grad_norm;
    a.update = log_stats ? 3 : 1;
    const unsigned grid = (unsigned)std::min<long long>((n.n_params + 1023) / 1024, 512);
    hipLaunchKernelGGL(n.flavour != kPpoRllib ? k_ppo_adam<kPpoSb3> : log_stats ? k_ppo_adam<kPpoRllibLog> : k_ppo_adam<kPpoRllib>,
                       dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t ppo_launch_stats(const PpoNet& n, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                            float* stats, hipStream_t st) {
    AdamArgs a;
    adam_common(a, n, scratch, s, n_partials, batch, stats);
    hipLaunchKernelGGL(n.flavour == kPpoRllib ? k_ppo_adam<kPpoRllib> : k_ppo_adam<kPpoSb3>, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace ch
