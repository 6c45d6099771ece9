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
// The kernels take a compile-time flavour F (ch_ppo.h lists the six and what each adds to its base).  The three bodies
// live in ch_ppo_{fb,dw,adam}_body.inc, included into the plain kernels and into ch_ppo_train_opt's (*_opt, which take
// an option struct behind the plain arguments: DESIGN.md 4.11, Options).  The 14 instantiations, one row of kPpoTable
// each; ppo_plan (ch_ppo.h) picks the rows an ABI entry launches:
//
//   kernel          | kPpoSb3 0 | kPpoRllib 1 | kFbSb3Log 2 | kPpoRllibLog 3 | kFbSb3Opt 4 | kFbSb3OptVf 5
//   k_ppo_fb        |     x     |      x      |      x      |       x        |             |
//   k_ppo_fb_opt    |           |             |             |                |      x      |       x
//   k_ppo_dw        |     x     |      x      |             |                |             |
//   k_ppo_dw_opt    |  x + gate |             |             |                |             |
//   k_ppo_adam      |     x     |      x      |             |       x        |             |
//   k_ppo_adam_opt  |  x + gate |             |             |                |             |
//   k_ppo_sumsq     no flavour: ch_ppo_adam's sum of squares of a given gradient
//
// The population kernels (k_ppo_{fb,dw,adam}_pop, ch_ppo_train_pop: P members per launch, the same bodies over a
// device table of arguments) follow the solo kernels below and have a table of their own, kPpoPopTable.
//
// (k_ppo_dw is the same for a base and its log flavour; k_ppo_adam<kPpoSb3> writes kFbSb3Log's two statistics under a
// run-time bit of AdamArgs::update.  DESIGN.md 4.12 - 4.14 describe the flavours.)
//
// MFMA operand map (16x16x4 f32): lane l gives A[row l & 15][k slot l >> 4] and B[k slot l >> 4][col l & 15]; it
// holds C/D[row 4 (l >> 4) + r][col l & 15] in register r.  Which k a slot stands for is free as long as A and B
// agree, so a lane loads four consecutive k as one float4 and feeds element j to the j-th MFMA of the chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

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

// What ch_ppo_train_opt's kernels take beside the arguments of the plain ones.  NoOpt: the plain
// kernels, whose bodies compile to what they were.
struct NoOpt {};
// NoOpt as a type that depends on the flavour, so that a plain kernel's discarded `if constexpr` branches, which name
// the options' members, are not looked up in it
template <int F, class Opt>
using PlainOpt = std::conditional_t<(F >= 0), NoOpt, Opt>;
struct FbOpt {
    const int32_t* stop;       // NULL: no gate
    const float* old_values;   // kFbSb3OptVf: [rows], the rollout's value predictions
    float clip_vf;             // kFbSb3OptVf: clip_range_vf
};
// The KL gate.  `stop` is the call's stop word (NULL: no gate): non-zero means an earlier minibatch tripped, and every
// launch returns at entry.  Otherwise a workgroup that needs this minibatch's decision forms it itself with
// gate_trips: the same float32 sums over the same scratch values in the same order as the approx_kl statistic, so all
// of them -- the weight-gradient launch's thread that counts the Adam step, every Adam workgroup -- agree without
// waiting for one another.
struct GateArgs {
    int32_t* stop;
    const float* tile_stat;    // this minibatch's tile partials (k_ppo_fb wrote them; a kernel boundary lies between)
    double threshold;          // 1.5 * target_kl
};

// approx_kl exactly as k_ppo_adam's statistic: the tiles' sums in index order, divided by the batch, compared in float64
__device__ __forceinline__ bool gate_trips(const GateArgs& g, int tiles, long long batch) {
    if (!g.stop) return false;
    float akl = 0.0f;
    for (int t = 0; t < tiles; ++t) akl += g.tile_stat[2 * tiles + 2 * t];
    return (double)(akl / (float)batch) > g.threshold;
}

// per-tile loss partials: the surrogate and the squared value error; kPpoRllib adds the entropy and the KL
template <int F>
constexpr int kStat = ppo_rllib(F) ? 4 : 2;

template <int F>
__global__ __launch_bounds__(64 * kFbWaves) void k_ppo_fb(FbArgs a) {
    [[maybe_unused]] constexpr PlainOpt<F, FbOpt> o{};
#include "ch_ppo_fb_body.inc"
}

template <int F>
__global__ __launch_bounds__(64 * kFbWaves) void k_ppo_fb_opt(FbArgs a, FbOpt o) {
#include "ch_ppo_fb_body.inc"
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
// (Args: DwArgs, or the population kernel's view of a table entry)
template <bool VEC, bool GATHER, class Args>
__device__ __forceinline__ void dw_loop(const Args& a, const DwGemm& G, int n0, int kw0, f32x4 (&acc)[4], float& bsum) {
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
    using Gate = PlainOpt<F, GateArgs>;
    [[maybe_unused]] constexpr Gate gate{};
#include "ch_ppo_dw_body.inc"
}

__global__ __launch_bounds__(64 * kDwWaves) void k_ppo_dw_opt(DwArgs a, GateArgs gate) {
    using Gate = GateArgs;
    constexpr int F = kPpoSb3;
#include "ch_ppo_dw_body.inc"
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
template <class Args>
__device__ __forceinline__ void rllib_log_stats(const Args& a) {
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
    using Gate = PlainOpt<F, GateArgs>;
    [[maybe_unused]] constexpr Gate gate{};
#include "ch_ppo_adam_body.inc"
}

__global__ __launch_bounds__(256) void k_ppo_adam_opt(AdamArgs a, GateArgs gate) {
    using Gate = GateArgs;
    constexpr int F = kPpoSb3;
#include "ch_ppo_adam_body.inc"
}

// ---- the population kernels (ch_ppo_train_pop) -----------------------------------------------------
// P members of one architecture in one launch.  A workgroup's member is a grid coordinate -- blockIdx.z of
// k_ppo_fb_pop, blockIdx.y of the other two; the bodies use blockIdx.x, blockIdx.y (fb) and gridDim.x only -- and its
// arguments are that member's entry of a device table: the structs k_ppo_*_opt take as kernel arguments, built by the
// same host code.  The body sees them as `a` through a view, references into the entry (the arrays the bodies index
// at run time stay in memory, as they stay in the kernel-argument segment) with the step's two offsets added: the
// minibatch's place in the member's idx, the statistics row.  The table is read-only and `__restrict__`, the member
// wave-uniform, so the entry's fields come by scalar loads and every branch on them stays uniform.  Members share
// nothing: each entry points into its member's own weights, moments, scratch, statistics and stop word.
struct PopFb { FbArgs a; FbOpt o; };
struct PopDw { DwArgs a; GateArgs gate; };
struct PopAdam { AdamArgs a; GateArgs gate; };

struct FbView {
    const PpoNet& n;
    const PpoData& d;
    const long long* idx;
    long long batch;
    float* scratch;
    const PpoScratch& s;
    float clip_range, vf_coef;
    int normalize, vec_obs;
    const int (&vec_w)[2][3];
    float ent_coef, vf_clip, ls_clip;
    const float* kl_coeff_dev;
    __device__ FbView(const FbArgs& t, long long idx_off)
        : n(t.n), d(t.d), idx(t.idx + idx_off), batch(t.batch), scratch(t.scratch), s(t.s), clip_range(t.clip_range),
          vf_coef(t.vf_coef), normalize(t.normalize), vec_obs(t.vec_obs), vec_w(t.vec_w), ent_coef(t.ent_coef),
          vf_clip(t.vf_clip), ls_clip(t.ls_clip), kl_coeff_dev(t.kl_coeff_dev) {}
};

struct DwView {
    const DwGemm (&g)[6];
    int ng, wg_ls;
    const float* obs;
    const long long* idx;
    long long batch;
    int bp, tiles, act_dim;
    const float* tile_dls;
    float* g_ls;
    float ent_coef;
    float* partial;
    long long* step_dev;
    __device__ DwView(const DwArgs& t, long long idx_off)
        : g(t.g), ng(t.ng), wg_ls(t.wg_ls), obs(t.obs), idx(t.idx + idx_off), batch(t.batch), bp(t.bp), tiles(t.tiles),
          act_dim(t.act_dim), tile_dls(t.tile_dls), g_ls(t.g_ls), ent_coef(t.ent_coef), partial(t.partial),
          step_dev(t.step_dev) {}
};

struct AdamView {
    const AdamSeg (&seg)[kPpoMaxSeg];
    int nseg;
    long long n_params;
    const float* grad;
    float* m;
    float* v;
    const long long* step_dev;
    const float* partial;
    int n_partials;
    double lr, beta1, beta2, eps, max_grad_norm;
    float* stats4;
    const float* tile_stat;
    const float* misc;
    int tiles;
    long long batch;
    int update;
    __device__ AdamView(const AdamArgs& t, long long stats_off)   // (the population's statistics are required)
        : seg(t.seg), nseg(t.nseg), n_params(t.n_params), grad(t.grad), m(t.m), v(t.v), step_dev(t.step_dev),
          partial(t.partial), n_partials(t.n_partials), lr(t.lr), beta1(t.beta1), beta2(t.beta2), eps(t.eps),
          max_grad_norm(t.max_grad_norm), stats4(t.stats4 + stats_off), tile_stat(t.tile_stat), misc(t.misc),
          tiles(t.tiles), batch(t.batch), update(t.update) {}
};

// F: kFbSb3Opt, kFbSb3OptVf (a later RLlib population is a flavour with options of its own, and a table row)
template <int F>
__global__ __launch_bounds__(64 * kFbWaves) void k_ppo_fb_pop(const PopFb* __restrict__ tab, long long idx_off) {
    const PopFb& e = tab[blockIdx.z];
    const FbView a(e.a, idx_off);
    const FbOpt o = e.o;
#include "ch_ppo_fb_body.inc"
}

// F: the base flavour, kPpoSb3 (with the gate, as k_ppo_dw_opt)
template <int F>
__global__ __launch_bounds__(64 * kDwWaves) void k_ppo_dw_pop(const PopDw* __restrict__ tab, long long idx_off) {
    using Gate = GateArgs;
    const PopDw& e = tab[blockIdx.y];
    const DwView a(e.a, idx_off);
    const GateArgs gate = e.gate;
#include "ch_ppo_dw_body.inc"
}

template <int F>
__global__ __launch_bounds__(256) void k_ppo_adam_pop(const PopAdam* __restrict__ tab, long long stats_off) {
    using Gate = GateArgs;
    const PopAdam& e = tab[blockIdx.y];
    const AdamView a(e.a, stats_off);
    const GateArgs gate = e.gate;
#include "ch_ppo_adam_body.inc"
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

// The kernel table, by PpoKernel: an instantiation's name (cattleherd/_lib.py ppo_kernel_table), its host handle and
// its workgroup size.
struct PpoKernelRow { const char* name; const void* fn; unsigned block; };
#define CH_ROW(KERNEL, BLOCK) {#KERNEL, reinterpret_cast<const void*>(&KERNEL), BLOCK}
const PpoKernelRow kPpoTable[kPpoKernels] = {   // in PpoKernel's order
    {"none", nullptr, 0},
    CH_ROW(k_ppo_fb<0>, 64 * kFbWaves), CH_ROW(k_ppo_fb<1>, 64 * kFbWaves), CH_ROW(k_ppo_fb<2>, 64 * kFbWaves),
    CH_ROW(k_ppo_fb<3>, 64 * kFbWaves), CH_ROW(k_ppo_fb_opt<4>, 64 * kFbWaves), CH_ROW(k_ppo_fb_opt<5>, 64 * kFbWaves),
    CH_ROW(k_ppo_dw<0>, 64 * kDwWaves), CH_ROW(k_ppo_dw<1>, 64 * kDwWaves), CH_ROW(k_ppo_dw_opt, 64 * kDwWaves),
    CH_ROW(k_ppo_sumsq, 256),
    CH_ROW(k_ppo_adam<0>, 256), CH_ROW(k_ppo_adam<1>, 256), CH_ROW(k_ppo_adam<3>, 256), CH_ROW(k_ppo_adam_opt, 256),
};
// the population kernels' table, by PpoPopKernel
const PpoKernelRow kPpoPopTable[kPpoPopKernels] = {
    CH_ROW(k_ppo_fb_pop<4>, 64 * kFbWaves), CH_ROW(k_ppo_fb_pop<5>, 64 * kFbWaves),
    CH_ROW(k_ppo_dw_pop<0>, 64 * kDwWaves), CH_ROW(k_ppo_adam_pop<0>, 256),
};
#undef CH_ROW

hipError_t launch_row(const PpoKernelRow& k, dim3 grid, void** args, hipStream_t st) {
    (void)hipLaunchKernel(k.fn, grid, dim3(k.block), args, 0, st);
    return hipGetLastError();
}

// launches row `k` over the kernel's arguments (an option kernel's struct last: a plain kernel does not read it)
hipError_t launch(int k, dim3 grid, void** args, hipStream_t st) { return launch_row(kPpoTable[k], grid, args, st); }

}  // namespace

PpoLastStep g_ppo_last_step = {kPpoNone, kPpoNone, kPpoNone, 0, 0};

const char* ppo_kernel_name(int row) { return row >= 0 && row < kPpoKernels ? kPpoTable[row].name : nullptr; }

void ppo_scratch_layout(const PpoNet& n, long long batch, PpoScratch& s) {
    std::memset(&s, 0, sizeof(s));
    s = ppo_scratch_for(s, batch);
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

namespace {

void fb_args(FbArgs& f, const PpoNet& n, const PpoHp& hp, const PpoData& d, const long long* idx, long long batch,
             float* scratch, const PpoScratch& s) {
    std::memset(&f, 0, sizeof(f));
    f.n = n; f.d = d; f.idx = idx; f.batch = batch; f.scratch = scratch; f.s = s;
    f.clip_range = (float)hp.clip_range; f.vf_coef = (float)hp.vf_coef;
    f.normalize = hp.normalize_advantage;
    f.ent_coef = (float)hp.ent_coef; f.vf_clip = (float)hp.vf_clip; f.ls_clip = (float)hp.log_std_clip;
    f.kl_coeff_dev = hp.kl_coeff_dev;
    f.vec_obs = n.obs_dim % 4 == 0 && aligned16(d.obs);
    for (int ni = 0; ni < 2; ++ni)
        for (int li = 0; li < n.net[ni].layers; ++li) f.vec_w[ni][li] = n.net[ni].dims[li] % 4 == 0 && aligned16(n.net[ni].w[li]);
}

// returns the weight-gradient grid: one sum-of-squares partial per workgroup
int dw_args(DwArgs& w, const FbArgs& f, const PpoNet& n, const PpoHp& hp, const PpoData& d, const long long* idx,
            long long batch, float* grad, float* scratch, const PpoScratch& s, long long* step_dev) {
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
    w.wg_ls = n.flavour == kPpoRllib ? -1 : wg++;
    w.obs = d.obs; w.idx = idx; w.batch = batch; w.bp = s.bp; w.tiles = s.tiles; w.act_dim = n.act_dim;
    w.tile_dls = scratch + s.tile_dls; w.g_ls = grad + n.goff_log_std; w.ent_coef = (float)hp.ent_coef;
    w.partial = scratch + s.partial; w.step_dev = step_dev;
    return wg;
}

// the gate as ch_ppo_train_opt's weight-gradient and Adam kernels take it (a plain kernel's plan: no options, unused)
GateArgs gate_args(const PpoPlan& p, const PpoOpt* opt, float* scratch, const PpoScratch& s) {
    return p.opts ? GateArgs{ppo_stop(*opt), scratch + s.tile_stat, 1.5 * opt->target_kl} : GateArgs{};
}

// the forward-backward kernel's options (a plain kernel's plan: unused)
FbOpt fb_opt_args(const PpoPlan& p, const PpoOpt* opt) {
    return p.opts ? FbOpt{ppo_stop(*opt), opt->old_values, (float)opt->clip_range_vf} : FbOpt{};
}

// the Adam launch's arguments; returns its grid.  `hp` NULL: the statistics alone, by one workgroup
unsigned adam_args(AdamArgs& a, const PpoPlan& p, const PpoNet& n, const PpoHp* hp, const float* grad, float* m, float* v,
                   const long long* step_dev, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                   float* stats) {
    std::memset(&a, 0, sizeof(a));
    for (int ni = 0; ni < 2; ++ni) {
        const PpoMlp& mlp = n.net[ni];
        for (int li = 0; li < mlp.layers; ++li) {
            a.seg[a.nseg++] = AdamSeg{mlp.w[li], mlp.goff_w[li], (long long)mlp.dims[li + 1] * mlp.dims[li]};
            a.seg[a.nseg++] = AdamSeg{mlp.b[li], mlp.goff_b[li], (long long)mlp.dims[li + 1]};
        }
    }
    if (n.flavour == kPpoSb3) a.seg[a.nseg++] = AdamSeg{n.log_std, n.goff_log_std, (long long)n.act_dim};
    // by offset, for the kernel's scan (the flat order interleaves the two nets' heads after both MLPs)
    std::sort(a.seg, a.seg + a.nseg, [](const AdamSeg& x, const AdamSeg& y) { return x.off < y.off; });
    a.n_params = n.n_params;
    a.partial = scratch + s.partial; a.n_partials = n_partials;
    a.stats4 = stats; a.tile_stat = scratch + s.tile_stat; a.misc = scratch + s.misc; a.tiles = s.tiles; a.batch = batch;
    if (!hp) return 1;
    a.grad = grad; a.m = m; a.v = v; a.step_dev = step_dev;
    a.lr = hp->lr; a.beta1 = hp->beta1; a.beta2 = hp->beta2; a.eps = hp->eps; a.max_grad_norm = hp->max_grad_norm;
    a.update = p.update;
    return (unsigned)std::min<long long>((n.n_params + 1023) / 1024, 512);
}

}  // namespace

hipError_t ppo_launch_grad(const PpoPlan& p, const PpoNet& n, const PpoHp& hp, const PpoData& d, const PpoOpt* opt,
                           const long long* idx, long long batch, float* grad, float* scratch, const PpoScratch& s,
                           long long* step_dev, int* n_partials, hipStream_t st) {
    FbArgs f;
    fb_args(f, n, hp, d, idx, batch, scratch, s);
    FbOpt fo = fb_opt_args(p, opt);
    void* fb[] = {&f, &fo};
    g_ppo_last_step.fb = p.fb; g_ppo_last_step.dw = p.dw;
    hipError_t e = launch(p.fb, dim3((unsigned)s.tiles, 2), fb, st);
    if (e != hipSuccess) return e;

    GateArgs gate = gate_args(p, opt, scratch, s);
    DwArgs w;
    const int wg = dw_args(w, f, n, hp, d, idx, batch, grad, scratch, s, step_dev);
    void* dw[] = {&w, &gate};
    *n_partials = wg;
    return launch(p.dw, dim3((unsigned)wg), dw, st);
}

hipError_t ppo_launch_sumsq(const PpoNet& n, const float* grad, float* scratch, const PpoScratch& s, long long* step_dev,
                            int* n_partials, hipStream_t st) {
    long long count = n.n_params;
    float* partial = scratch + s.partial;
    void* args[] = {&grad, &count, &partial, &step_dev};
    g_ppo_last_step.fb = kPpoNone; g_ppo_last_step.dw = kPpoSumsq;
    *n_partials = kSumsqGrid;
    return launch(kPpoSumsq, dim3(kSumsqGrid), args, st);
}

// `hp` NULL: the statistics alone, by one workgroup (ppo_launch_stats)
hipError_t ppo_launch_adam(const PpoPlan& p, const PpoNet& n, const PpoHp* hp, const PpoOpt* opt, const float* grad,
                           float* m, float* v, const long long* step_dev, float* scratch, const PpoScratch& s,
                           int n_partials, long long batch, float* stats, hipStream_t st) {
    AdamArgs a;
    const unsigned grid = adam_args(a, p, n, hp, grad, m, v, step_dev, scratch, s, n_partials, batch, stats);
    GateArgs gate = gate_args(p, opt, scratch, s);
    void* args[] = {&a, &gate};
    g_ppo_last_step.adam = p.adam; g_ppo_last_step.update = a.update; g_ppo_last_step.adam_grid = (int)grid;
    return launch(p.adam, dim3(grid), args, st);
}

const char* ppo_pop_kernel_name(int row) { return row >= 0 && row < kPpoPopKernels ? kPpoPopTable[row].name : nullptr; }

PpoPopSizes ppo_pop_entry_sizes() { return {sizeof(PopFb), sizeof(PopDw), sizeof(PopAdam)}; }

void ppo_pop_fill(const PpoPopTables& host, int i, const PpoMember& mb, long long batch, const PpoScratch& s, PpoPopGeom* g) {
    // ch_ppo_train_opt's plan (the gate and the clip do not change the arguments' build, only what the options hold)
    const PpoPlan p = ppo_plan(kPpoSb3, false, true, mb.o.target_kl > 0.0, mb.o.clip_range_vf > 0.0);
    float* grad = mb.scratch + s.grad;
    PopFb& f = static_cast<PopFb*>(host.fb)[i];
    PopDw& w = static_cast<PopDw*>(host.dw)[i];
    PopAdam& a = static_cast<PopAdam*>(host.adam)[i];
    fb_args(f.a, mb.n, mb.hp, mb.d, mb.idx, batch, mb.scratch, s);
    f.o = fb_opt_args(p, &mb.o);
    g->tiles = s.tiles;
    g->dw_grid = dw_args(w.a, f.a, mb.n, mb.hp, mb.d, mb.idx, batch, grad, mb.scratch, s, mb.step_dev);
    w.gate = gate_args(p, &mb.o, mb.scratch, s);
    g->adam_grid = (int)adam_args(a.a, p, mb.n, &mb.hp, grad, mb.m, mb.v, mb.step_dev, mb.scratch, s, g->dw_grid, batch, mb.stats);
    a.gate = w.gate;
}

hipError_t ppo_pop_launch(const PpoPopPlan& p, const PpoPopTables& dev, const PpoPopGeom& g, int members,
                          long long idx_off, long long stats_off, hipStream_t st) {
    const unsigned P = (unsigned)members;
    void* fb[] = {const_cast<void**>(&dev.fb), &idx_off};
    hipError_t e = launch_row(kPpoPopTable[p.fb], dim3((unsigned)g.tiles, 2, P), fb, st);
    if (e != hipSuccess) return e;
    void* dw[] = {const_cast<void**>(&dev.dw), &idx_off};
    e = launch_row(kPpoPopTable[p.dw], dim3((unsigned)g.dw_grid, P), dw, st);
    if (e != hipSuccess) return e;
    void* adam[] = {const_cast<void**>(&dev.adam), &stats_off};
    return launch_row(kPpoPopTable[p.adam], dim3((unsigned)g.adam_grid, P), adam, st);
}

}  // namespace ch
