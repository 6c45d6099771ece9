// ch_ppo_fb_body.inc -- the body of k_ppo_fb and k_ppo_fb_opt (ch_ppo.hip), included into both: `F` the flavour, `a`
// the FbArgs, `o` the options (NoOpt in k_ppo_fb, whose instantiations compile to the code they were before the
// options existed -- a shared __device__ function does not give that).
    [[maybe_unused]] constexpr bool kLog = F == kFbSb3Log || fb_opt(F);
    if constexpr (fb_opt(F)) {
        if (o.stop && *o.stop) return;   // an earlier minibatch tripped the gate: nothing of this one runs
    }
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
            if constexpr (F == kFbSb3OptVf) {
                // SB3's clip_range_vf: old + clamp(v - old, +-c) in the squared error; torch.clamp's gradient passes
                // inside the closed range, so a row strictly outside it gives the value head none
                const float old = o.old_values[src], dv = os[tid * kLdo] - old;
                const float err = old + fminf(fmaxf(dv, -o.clip_vf), o.clip_vf) - a.d.returns[src];
                rowstat[tid] = valid ? err * err : 0.0f;
                os[tid * kLdo] = valid && dv >= -o.clip_vf && dv <= o.clip_vf ? a.vf_coef * 2.0f * err * inv_b : 0.0f;
            } else {
                const float err = os[tid * kLdo] - a.d.returns[src];
                rowstat[tid] = valid ? err * err : 0.0f;
                os[tid * kLdo] = valid ? a.vf_coef * 2.0f * err * inv_b : 0.0f;
            }
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
