// ch_step_flock.h — the cow waves' flock math (flockUtils.py:237-348): the alpha pair table in its shared and per-wave
// forms, the alpha rows, the shepherd / predator terms and the velocity update.  A part of ch_step_body.h, included
// there behind V2Smem, the LDS flag enums and the store helpers it uses; not a header to include on its own.
#pragma once

namespace ch {


// flock alpha term, pair form, for every flocking env (flockUtils.py:237-258, 327-337; MathUtils 11-58):
// one table of the workgroup's unordered cow pairs, evaluated in the bump's support only.  The bump is
// exactly 0 for sigma_norm(|z|) / r_alpha > 1 (beyond the lattice range d_alpha = 1.2 m); such a pair adds
// +-0 to both rows, which leaves a row sum that starts at +0 unchanged.  A cheap pass over every pair (no
// square root) marks the pairs with |z|^2 <= 1.44 (1 + 1e-9) -- a superset of the support, see
// kAlphaSupport2 -- in both cows' neighbour masks and appends them to a queue; the full evaluation runs on
// full waves of queued pairs; the rows visit the masked neighbours in ascending order like the dense loop.
constexpr double kAlphaSupport2 = 1.44 * (1.0 + 1e-9);

// |z| <= 999 (the sensing range) from |z|^2 without the square root away from the boundary: sqrt is
// correctly rounded and monotonic, and sqrt(998001) = 999 exactly
template <class R> __device__ __forceinline__ bool in_sensing(R n2) {
    bool s = n2 <= R(998001.0);
    if (!s && n2 < R(998010.0)) s = sqrt(n2) <= R(999);
    return s;
}

// Cow j of env g has another cow of its env within sensing range (flockUtils.py:237-258: the alpha sums run over the
// neighbours inside r = 999 m; with none, its alpha term is 0).  One partner decides it almost always -- the next cow --
// and only a cow out of that one's range scans the rest, with the pair's difference taken in the pair list's order
// (the same n2 as the cheap pass).  Evaluated by the row instead of marked by the cheap pass: those byte stores (many
// lanes of a pass chunk on the same cow) took ~40 % of the pass (tools/wg_trace.py, profiles/r04/zc).
template <class R>
__device__ __forceinline__ bool has_sensing_neighbour(const V2Smem<R>& S, int M, int g, int j) {
    auto ins = [&](int k) {
        const int lo = g * M + min(j, k), hi = g * M + max(j, k);
        const R zx = S.cx[hi] - S.cx[lo], zy = S.cy[hi] - S.cy[lo];
        return in_sensing(zx * zx + zy * zy);
    };
    bool has = M > 1 && ins(j + 1 < M ? j + 1 : 0);
    if (!has)
        for (int k = 0; k < M; ++k)
            if (k != j && ins(k)) { has = true; break; }
    return has;
}

template <class R>
__device__ __forceinline__ void alpha_cheap(V2Smem<R>& S, int* fl, int M, int P, int nf, const int* flist, bool skip) {
    const float rP = 1.0f / (float)P;
    const int lane = threadIdx.x & 63;
    for (;;) {
        const int b = grab(fl + C_PAIRS, 64, skip);
        if (b >= nf * P) break;
        const int q = b + lane;
        bool cand = false;
        int gi = 0;
        if (q < nf * P) {
            const int f = qdiv(q, P, rP), r = q - f * P, g = flist[f];
            const uint32_t pr = S.pl[r];
            const int li = pr & 0xff, hi = pr >> 8;
            const int bi = g * M + li, bj = g * M + hi;
            const R zx = S.cx[bj] - S.cx[bi], zy = S.cy[bj] - S.cy[bi];
            const R n2 = zx * zx + zy * zy;
            cand = n2 <= R(kAlphaSupport2);
            if (cand) {
                atomicOr(&S.nbm[bi], 1ull << hi);
                atomicOr(&S.nbm[bj], 1ull << li);
            }
            gi = g * P + r;
        }
        const unsigned long long m = __ballot(cand);
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(fl + Q_LEN, (int)__popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (cand) S.queue[base + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)gi;
    }
}

// The same pass for the pipelined step loop's geometry (compile-time G, M and P; NC = the pass's 64-pair chunks), one
// unit per flocking env instead of one per 64 queue positions: C_PAIRS counts envs.  The lane's pair words are read
// once per step, ahead of the first grab (a pair past P repeats pair 0 and is masked out by r < P), and so is the
// flock list (lane f holds env f; the unit's env is a readlane); every chunk's position loads are issued before any
// test, and one returning add on Q_LEN reserves the env's slots, filled in (chunk, lane) order.  A unit is three
// dependent LDS round trips (grab, positions, reservation) where alpha_cheap's 64-pair chunk is five, and an env is
// one unit where it was two chunks.  The queue's order differs from alpha_cheap's; nothing read from it depends on
// the order: the masks are ORs, the pair table is indexed by the pair (gi) and the rows walk the masks in ascending
// order.
template <class R, int G, int M, int P>
__device__ __forceinline__ void alpha_cheap_env(V2Smem<R>& S, int* fl, int nf, const int* flist, bool skip) {
    constexpr int NC = (P + 63) / 64;
    static_assert(G <= 64 && (G & (G - 1)) == 0, "the flock list is held one env per lane");
    const int lane = threadIdx.x & 63;
    uint32_t prw[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int r = 64 * c + lane;
        prw[c] = S.pl[r < P ? r : 0];
    }
    const int flv = flist[lane & (G - 1)];   // (entries past nf are stale and never selected)
    for (;;) {
        const int f = grab(fl + C_PAIRS, 1, skip);
        if (f >= nf) break;
        const int g = __builtin_amdgcn_readlane(flv, f & (G - 1));
        R n2[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const uint32_t pr = prw[c];
            const int bi = g * M + (pr & 0xff), bj = g * M + (pr >> 8);
            const R zx = S.cx[bj] - S.cx[bi], zy = S.cy[bj] - S.cy[bi];
            n2[c] = zx * zx + zy * zy;
        }
        bool cand[NC];
        unsigned long long m[NC];
        int tot = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const uint32_t pr = prw[c];
            const int li = pr & 0xff, hi = pr >> 8;
            cand[c] = 64 * c + lane < P && n2[c] <= R(kAlphaSupport2);
            if (cand[c]) {
                atomicOr(&S.nbm[g * M + li], 1ull << hi);
                atomicOr(&S.nbm[g * M + hi], 1ull << li);
            }
            m[c] = __ballot(cand[c]);
            tot += (int)__popcll(m[c]);
        }
        int base = 0;
        if (lane == 0 && tot) base = atomicAdd(fl + Q_LEN, tot);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (cand[c]) S.queue[base + __popcll(m[c] & ((1ull << lane) - 1ull))] = (uint16_t)(g * P + 64 * c + lane);
            base += (int)__popcll(m[c]);
        }
    }
}

// The full evaluation of the queued pairs, streamed (the barrier form is in DESIGN_HISTORY.md): a wave
// that runs out of cheap-pass chunks starts on the queue at once instead of waiting at a pass-wide barrier for
// the other waves' last cheap chunks.  Every queue slot starts as kQEmpty (phase 0); a chunk of 64 slots is taken
// when all of them are reserved (Q_LEN) or the cheap pass is complete (F_C counts the waves done with it, so
// Q_LEN is then final), and each lane waits for its own slot's pair index to be written -- a per-slot ready mark.
constexpr uint16_t kQEmpty = 0xFFFF;
template <class R>
__device__ __forceinline__ void alpha_full(V2Smem<R>& S, int* fl, int M, int P, bool skip, int W1, int* err) {
    const R ra = sigma_norm_n(R(1.2)), da = ra;
    const float rP = 1.0f / (float)P;
    const int lane = threadIdx.x & 63;
    for (;;) {
        const int b = grab(fl + C_QUEUE, 64, skip);
        if (b >= (1 << 28)) break;   // (skip)
        int qn = 0;
        bool done = false;
        int spins = 0;
        for (;; ++spins) {
            done = lds_peek(fl + F_C) >= W1;      // F_C before Q_LEN: once every wave is done, Q_LEN is final
            qn = lds_peek(fl + Q_LEN);
            if (done || qn >= b + 64) break;
            if (spins >= (1 << 22)) { handoff_failed(err); done = true; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        spin_note(spins);
        if (b >= qn) break;   // done: no slot of this chunk was ever reserved
        if (b + lane < qn) {
            int gi = kQEmpty;
            for (int spins = 0; spins < (1 << 22); ++spins) {
                gi = *reinterpret_cast<volatile const uint16_t*>(&S.queue[b + lane]);
                if (gi != kQEmpty) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (gi == kQEmpty) { handoff_failed(err); gi = 0; }
            const int g = qdiv(gi, P, rP), r = gi - g * P;
            const uint32_t pr = S.pl[r];
            const int bi = g * M + (pr & 0xff), bj = g * M + (pr >> 8);
            const R zx = S.cx[bj] - S.cx[bi], zy = S.cy[bj] - S.cy[bi];
            const R nrm = sqrt(zx * zx + zy * zy);
            R gx = 0, gy = 0, cx = 0, cy = 0;
            pair_terms_n(nrm, zx, zy, S.cvx[bi], S.cvy[bi], S.cvx[bj], S.cvy[bj], ra, da, gx, gy, cx, cy);
            S.tgx[gi] = gx; S.tgy[gi] = gy; S.tcx[gi] = cx; S.tcy[gi] = cy;
        }
    }
}

// alpha row of cow u = g*M + j in neighbour order over its masked neighbours, scaled by c2_alpha
// (flockUtils.py:237-258); the two directed contributions of a pair are exact negations
template <class R>
__device__ __forceinline__ void alpha_row(V2Smem<R>& S, int M, int P, int u, int g, int j) {
    const R C2A = R(2 * 1.7320508075688772);
    R gx = 0, gy = 0, cxx = 0, cyy = 0, ux = 0, uy = 0;
    const int pb = g * P;
    // Four neighbours per round, branch-free: the table loads of a round are issued together (an empty slot
    // reads the env's first pair), then summed in neighbour order.  An empty slot adds +0, which leaves the
    // sum unchanged: it starts at +0 and a round-to-nearest sum is -0 only if both addends are.
    for (unsigned long long m = S.nbm[u]; m;) {
        R t[4][4];
        bool v[4], fwd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[r] = m != 0;
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            fwd[r] = j < k;
            const int idx = v[r] ? pb + tri(min(j, k), max(j, k), M) : pb;
            t[r][0] = S.tgx[idx]; t[r][1] = S.tgy[idx]; t[r][2] = S.tcx[idx]; t[r][3] = S.tcy[idx];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gx += v[r] ? (fwd[r] ? t[r][0] : -t[r][0]) : R(0); gy += v[r] ? (fwd[r] ? t[r][1] : -t[r][1]) : R(0);
            cxx += v[r] ? (fwd[r] ? t[r][2] : -t[r][2]) : R(0); cyy += v[r] ? (fwd[r] ? t[r][3] : -t[r][3]) : R(0);
        }
    }
    if (has_sensing_neighbour(S, M, g, j)) { ux = C2A * gx + C2A * cxx; uy = C2A * gy + C2A * cyy; }
    S.aux[u] = ux; S.auy[u] = uy;
}

// ---- per-wave env tables (V2Layout W > 0, large herds) ---------------------------------------------
// Env g's alpha pair table in the calling wave's slot: gradient x, y and the bump b per pair
// (flockUtils.py:237-258, 327-337).  The consensus term b (p_hi - p_lo) is not stored: alpha_row_pw
// recomputes it from the velocities with the same rounding.
//
// Sparse in the bump's support.  The bump is exactly 0 for sigma_norm(|z|) / r_alpha > 1, i.e. beyond
// the lattice range d_alpha = 1.2 m, and such a pair adds +-0 to both rows, which leaves a row sum that
// starts at +0 unchanged.  A cheap pass over all pairs (no square root) queues the pairs with
// |z|^2 <= 1.44 (1 + 1e-9) -- a superset of the support: any pair beyond it has z > 1 + 5e-10 exactly and
// z > 1 as computed -- and marks them in both cows' neighbour masks; the full evaluation (square roots,
// the bump's cos, sigma_1, divisions) runs on full waves of queued pairs only, and the rows visit only
// masked neighbours, in ascending neighbour order like the dense loop.
template <class R>
__device__ __forceinline__ void alpha_cheap_pw(V2Smem<R>& S, int M, int P, int g, uint16_t* qu, int& qn) {
    const int lane = threadIdx.x & 63;
    for (int r0 = 0; r0 < P; r0 += 64) {
        const int r = r0 + lane;
        bool cand = false;
        if (r < P) {
            const uint32_t pr = S.pl[r];
            const int li = pr & 0xff, hi = pr >> 8;
            const int bi = g * M + li, bj = g * M + hi;
            const R zx = S.cx[bj] - S.cx[bi], zy = S.cy[bj] - S.cy[bi];
            const R n2 = zx * zx + zy * zy;
            cand = n2 <= R(kAlphaSupport2);
            if (cand) {
                atomicOr(&S.nbm[bi], 1ull << hi);
                atomicOr(&S.nbm[bj], 1ull << li);
            }
        }
        const unsigned long long m = __ballot(cand);
        if (cand) qu[qn + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)r;
        qn += __popcll(m);
    }
}

// The same pass for a geometry-specialised herd (NC = the pass's 64-pair chunks, a compile-time count): the lane's
// pair words come from registers (prw, read from LDS once per kernel) and every chunk's position loads are issued
// before any chunk's test, so the pass costs about one LDS round trip instead of one per chunk.  The queue and
// masks are filled in the same (chunk, lane) order as alpha_cheap_pw.
template <class R, int NC>
__device__ __forceinline__ void alpha_cheap_pw_b(V2Smem<R>& S, int M, int P, int g, uint16_t* qu, int& qn,
                                                 const uint32_t (&prw)[NC]) {
    const int lane = threadIdx.x & 63;
    R n2[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const uint32_t pr = prw[c];
        const int bi = g * M + (pr & 0xff), bj = g * M + (pr >> 8);
        const R zx = S.cx[bj] - S.cx[bi], zy = S.cy[bj] - S.cy[bi];
        n2[c] = zx * zx + zy * zy;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int r = 64 * c + lane;
        bool cand = false;
        if (r < P) {
            const uint32_t pr = prw[c];
            const int li = pr & 0xff, hi = pr >> 8;
            const int bi = g * M + li, bj = g * M + hi;
            cand = n2[c] <= R(kAlphaSupport2);
            if (cand) {
                atomicOr(&S.nbm[bi], 1ull << hi);
                atomicOr(&S.nbm[bj], 1ull << li);
            }
        }
        const unsigned long long m = __ballot(cand);
        if (cand) qu[qn + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)r;
        qn += __popcll(m);
    }
}

template <class R>
__device__ __forceinline__ void alpha_full_pw(V2Smem<R>& S, int M, int P, int g, int q0, int qn, R* tb,
                                              const uint16_t* qu) {
    const R ra = sigma_norm_n(R(1.2)), da = ra;
    const int q = q0 + (threadIdx.x & 63);
    if (q >= qn) return;
    const int r = qu[q];
    const uint32_t pr = S.pl[r];
    const int bi = g * M + (pr & 0xff), bj = g * M + (pr >> 8);
    const R zx = S.cx[bj] - S.cx[bi], zy = S.cy[bj] - S.cy[bi];
    const R nrm = sqrt(zx * zx + zy * zy);
    R gx = 0, gy = 0, cx = 0, cy = 0;
    const R b = pair_terms_n(nrm, zx, zy, R(0), R(0), R(0), R(0), ra, da, gx, gy, cx, cy);
    tb[r] = gx; tb[P + r] = gy; tb[2 * P + r] = b;
}

// alpha row of cow j of env g from the wave's slot, in neighbour order (as alpha_row), visiting the
// masked neighbours only.  The pair's consensus term is b * (p_hi - p_lo), hi/lo the pair's cows,
// exactly as the shared table holds it.
template <class R>
__device__ __forceinline__ void alpha_row_pw(V2Smem<R>& S, int M, int P, int g, int j, const R* tb) {
    const R C2A = R(2 * 1.7320508075688772);
    const int u = g * M + j;
    R gx = 0, gy = 0, cxx = 0, cyy = 0, ux = 0, uy = 0;
    const R pjx = S.cvx[u], pjy = S.cvy[u];
    // four neighbours per round, branch-free as in alpha_row (an empty slot reads pair 0 / cow j, adds +0)
    for (unsigned long long m = S.nbm[u]; m;) {
        R t[4][5];
        bool v[4], fwd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[r] = m != 0;
            const int k = v[r] ? __ffsll((long long)m) - 1 : j;
            m &= m - 1;
            fwd[r] = j < k;
            const int idx = v[r] ? tri(min(j, k), max(j, k), M) : 0;
            t[r][0] = tb[idx]; t[r][1] = tb[P + idx]; t[r][2] = tb[2 * P + idx];
            t[r][3] = S.cvx[g * M + k]; t[r][4] = S.cvy[g * M + k];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const R b = t[r][2], pkx = t[r][3], pky = t[r][4];
            const R dvx = fwd[r] ? pkx - pjx : pjx - pkx, dvy = fwd[r] ? pky - pjy : pjy - pky;
            const R tcx = b * dvx, tcy = b * dvy;
            gx += v[r] ? (fwd[r] ? t[r][0] : -t[r][0]) : R(0); gy += v[r] ? (fwd[r] ? t[r][1] : -t[r][1]) : R(0);
            cxx += v[r] ? (fwd[r] ? tcx : -tcx) : R(0); cyy += v[r] ? (fwd[r] ? tcy : -tcy) : R(0);
        }
    }
    if (has_sensing_neighbour(S, M, g, j)) { ux = C2A * gx + C2A * cxx; uy = C2A * gy + C2A * cyy; }
    S.aux[u] = ux; S.auy[u] = uy;
}

// the shepherd term of a drone closer than 1 m (mu < 1: the projected agent q_ik lies between cow and drone),
// the general pair_terms evaluation.  Rare, so it is kept out of line: inlined at each of the unrolled drone
// slots of shepherd_sum it would add ~1.2k instructions to the kernel's instruction-cache footprint.
template <class R> struct Terms4 { R gx, gy, cx, cy; };
template <class R>
__device__ __noinline__ Terms4<R> near_drone_terms(R qix, R qiy, R pix, R piy, R yx, R yy, R mu, R pkx, R pky) {
    const R ra_b = sigma_norm_n(R(1.0)), da_b = ra_b;
    R qkx = mu * qix + (R(1) - mu) * yx, qky = mu * qiy + (R(1) - mu) * yy;
    Terms4<R> t = {0, 0, 0, 0};
    pair_terms(qix, qiy, pix, piy, qkx, qky, pkx, pky, ra_b, da_b, t.gx, t.gy, t.cx, t.cy);
    return t;
}

// shepherd (delta, flockUtils.py:271-317) and predator (343-348) terms of drone k on cow u = g*M + j:
// t[0..3] the delta gradient and consensus parts, t[4..5] the predator push; returns in-range | predator << 1
template <class R>
__device__ __forceinline__ int delta_vals(const V2Smem<R>& S, int N, int u, int g, int k, R t[6]) {
    const R qix = S.cx[u], qiy = S.cy[u], pix = S.cvx[u], piy = S.cvy[u];
    const R yx = S.dx[g * N + k], yy = S.dy[g * N + k];
    const R ex = yx - qix, ey = yy - qiy;
    const R dn = sqrt(ex * ex + ey * ey);   // = the distance table entry
    const bool in = dn <= R(999 + 2), pr = dn <= R(1.1);
#pragma unroll
    for (int c = 0; c < 6; ++c) t[c] = 0;
    if (in) {
        R difx = qix - yx, dify = qiy - yy;
        R d = dn + R(1e-6);
        R mu = d / R(1.0) < R(1.0) ? d / R(1.0) : R(1.0);
        R akx = difx / d, aky = dify / d;
        R P00 = R(1) - akx * akx, P01 = R(0) - akx * aky, P10 = R(0) - aky * akx, P11 = R(1) - aky * aky;
        R pkx = mu * (P00 * pix + P01 * piy), pky = mu * (P10 * pix + P11 * piy);
        if (mu == R(1) && isfinite(yx) && isfinite(yy) && isfinite(qix) && isfinite(qiy)) {
            // a drone 1 m away or more: q_ik = 1 q_i + 0 y_k = q_i exactly, so pair_terms sees z = +0:
            // |z| = 0, den = 1, sigma_norm = 0, bump(0) = 1, gradient ph * (0 / 1) = +-0 (+0 in the table),
            // consensus 1 * (p_ik - p_i) -- the same values without the square roots and divisions
            t[2] = pkx - pix;
            t[3] = pky - piy;
        } else {
            const Terms4<R> n4 = near_drone_terms(qix, qiy, pix, piy, yx, yy, mu, pkx, pky);
            t[0] = n4.gx; t[1] = n4.gy; t[2] = n4.cx; t[3] = n4.cy;
        }
    }
    if (pr) {
        R d3 = cube(dn);
        t[4] = R(-650000.0) * ex / d3;
        t[5] = R(-650000.0) * ey / d3;
    }
    return (int)in | ((int)pr << 1);
}

// the same terms, one (cow, drone) item per lane, stored in the term table for flock_combine
template <class R>
__device__ __forceinline__ void delta_term(V2Smem<R>& S, int N, int u, int g, int k, R* td, uint8_t* tdf, int i,
                                           int T) {
    R t[6];
    const int f = delta_vals(S, N, u, g, k, t);
#pragma unroll
    for (int c = 0; c < 6; ++c) td[c * T + i] = t[c];
    tdf[i] = (uint8_t)f;
}

// the shepherd/predator sum of cow u over its env's n live drones in drone order (flockUtils.py:271-348),
// one cow per lane with the drone terms in registers: delta = c2_beta (sum grad + sum consensus) over the
// drones in range, plus the predator pushes.  A term out of range is +0, which leaves a sum that starts at
// +0 unchanged (the same sums flock_combine forms from the term table).
template <class R, int NT>
__device__ __forceinline__ void shepherd_sum(const V2Smem<R>& S, int N, int u, int g, int n, R& ddx, R& ddy) {
    const R C2B = R(2 * 4.47213595499958);
    R gx = 0, gy = 0, cxx = 0, cyy = 0, sx = 0, sy = 0;
    int nb = 0;
    constexpr int NK = NT ? NT : 64;
    CH_UNROLL for (int k = 0; k < NK; ++k) {
        if (k >= N || k >= n) break;
        R t[6];
        const int f = delta_vals(S, N, u, g, k, t);
        if (f & 1) { ++nb; gx += t[0]; gy += t[1]; cxx += t[2]; cyy += t[3]; }
        if (f & 2) { sx += t[4]; sy += t[5]; }
    }
    ddx = 0; ddy = 0;
    if (nb > 0) { ddx = C2B * gx + C2B * cxx; ddy = C2B * gy + C2B * cyy; }
    ddx += sx; ddy += sy;
}

// gamma term (flockUtils.py:150-160, 340-341) and the velocity update with the speed clip
// (BaseAviary.py:1384-1400) of cow u from its alpha row (aux, auy) and shepherd sum (ddx, ddy)
// nv != nullptr: the new velocity goes to LDS (nv[u], nv[GM + u]) instead of HBM
template <class R>
__device__ __forceinline__ void velocity_update(const StepParams<R>& p, const V2Smem<R>& S, int M, int e0, int u, R ddx,
                                                R ddy, R* nv = nullptr, int GM = 0) {
    const long long CS = (long long)p.E * M;
    const R C1G = R(5), C2G = R(0.2 * 2.23606797749979);
    const R qix = S.cx[u], qiy = S.cy[u], pix = S.cvx[u], piy = S.cvy[u];
    R gmx = -C1G * sigma_1(qix - R(1)) - C2G * pix, gmy = -C1G * sigma_1(qiy - R(1)) - C2G * piy;
    R qx = (S.aux[u] + ddx) + gmx, qy = (S.auy[u] + ddy) + gmy;
    const R dt_sqr = R(0.05 * 0.05);
    R vx = pix + qx * dt_sqr, vy = piy + qy * dt_sqr;
    R sp = norm2(vx, vy);
    if (sp > R(kMaxVelCattle)) { R f = R(kMaxVelCattle) / sp; vx *= f; vy *= f; }
    if (nv) { nv[u] = vx; nv[GM + u] = vy; return; }
    const long long ci = (long long)e0 * M + u;
    CH_STS(&p.cattle[2 * CS + ci], vx); CH_STS(&p.cattle[3 * CS + ci], vy);
}

// the drone terms of cow u from the term table summed in drone order, then the velocity update.  A term
// out of range is +0 in the table, and adding +0 to a sum that starts at +0 leaves it unchanged, so only
// the count needs the flag.
template <class R>
__device__ __forceinline__ void flock_combine(const StepParams<R>& p, V2Smem<R>& S, int N, int M, int e0, int u, int n,
                                              const R* td, const uint8_t* tdf, int ib, int T) {
    const R C2B = R(2 * 4.47213595499958);
    R ddx = 0, ddy = 0, sx = 0, sy = 0, gx = 0, gy = 0, cxx = 0, cyy = 0;
    int nb = 0;
    CH_UNROLL for (int k = 0; k < N; ++k) {
        if (k >= n) break;
        const int i = ib + k;
        const int f = tdf[i];
        if (f & 1) { ++nb; gx += td[i]; gy += td[T + i]; cxx += td[2 * T + i]; cyy += td[3 * T + i]; }
        if (f & 2) { sx += td[4 * T + i]; sy += td[5 * T + i]; }
    }
    if (nb > 0) { ddx = C2B * gx + C2B * cxx; ddy = C2B * gy + C2B * cyy; }
    ddx += sx; ddy += sy;
    velocity_update(p, S, M, e0, u, ddx, ddy);
}

}  // namespace ch
