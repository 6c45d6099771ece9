// ch_ppo_dw_body.inc -- the body of k_ppo_dw and k_ppo_dw_opt (ch_ppo.hip), included into both: `F` the flavour, `a` the
// DwArgs, `gate` of type `Gate` the KL gate (NoOpt in k_ppo_dw; see ch_ppo_fb_body.inc).
    constexpr bool kGate = !std::is_same_v<Gate, NoOpt>;
    __shared__ float red[kDwWaves];
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x;
    if constexpr (kGate) {
        if (gate.stop && *gate.stop) return;
        // the Adam step is counted only for a minibatch that will be applied; the gradient of a tripping one is still
        // formed, for its norm in the statistics row
        if (wg == 0 && tid == 0 && a.step_dev && !gate_trips(gate, a.tiles, a.batch)) *a.step_dev += 1;
    } else {
        if (wg == 0 && tid == 0 && a.step_dev) *a.step_dev += 1;   // the Adam step this gradient is for
    }
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
