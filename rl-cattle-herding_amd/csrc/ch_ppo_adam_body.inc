// ch_ppo_adam_body.inc -- the body of k_ppo_adam and k_ppo_adam_opt (ch_ppo.hip), included into both: `F` the flavour,
// `a` the AdamArgs, `gate` of type `Gate` the KL gate (NoOpt in k_ppo_adam; see ch_ppo_fb_body.inc).
// Gate = GateArgs (k_ppo_adam_opt, ch_ppo_train_opt): stats4 is a row of CH_PPO_OPT_STATS, its last column the step's
// state -- 1 applied, 0 this minibatch tripped the gate (statistics written, nothing updated), -1 not run because an
// earlier one had (the other columns NaN).  Workgroup 0's first thread sets the stop word on a trip, a plain store that
// the next step's launches see through the kernel boundary.  That store can land while a late workgroup of this same
// launch is at its entry test, so the test is made once per workgroup: thread 0 reads the word into LDS and every wave
// branches on that copy behind a barrier.  A workgroup that sees the fresh 1 returns as a whole, where it would have
// returned as a whole a few lines further down on the decision it forms itself; waves of one workgroup never part.
    constexpr bool kGate = !std::is_same_v<Gate, NoOpt>;
    __shared__ float red[4];
    __shared__ float sc[4];
    const int tid = threadIdx.x;
    if constexpr (kGate) {
        if (tid == 0) sc[3] = gate.stop && *gate.stop ? 1.0f : 0.0f;
        __syncthreads();
        if (sc[3] != 0.0f) {   // (sc[3] is written again only behind block_sum's barriers)
            if (blockIdx.x == 0 && tid < 7) a.stats4[tid] = tid < 6 ? __builtin_nanf("") : -1.0f;
            return;
        }
    }
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
        if constexpr (kGate) sc[3] = gate_trips(gate, a.tiles, a.batch) ? 1.0f : 0.0f;
    }
    __syncthreads();
    if constexpr (kGate) {
        const bool trip = sc[3] != 0.0f;
        if (blockIdx.x == 0 && tid == 0) {
            a.stats4[6] = trip ? 0.0f : 1.0f;
            if (trip) *gate.stop = 1;
        }
        if (trip) return;   // before the moments and the weights: *step_dev was not counted either (k_ppo_dw_opt)
    }
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
