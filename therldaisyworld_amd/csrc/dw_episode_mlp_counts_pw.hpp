// dw_episode_mlp_counts_pw.hpp — dw_run_episode_mlp_counts: MLP episodes in which world b has its own number of agents,
// n_active[b] of the handle's N (the agent-count scans of the reference's title notebook,
// notebooks/daisy_world_existential_risk_and_agency.ipynb cells fd8ad489 .. 227e4895: n_agents over 1, 31, .. 271 on 16x16).
// In world b only agents [0, n_active[b]) exist: the others are neither observed nor stamped into channel 4 (ref forward
// :454-459 stamps dead agents too, so an absent agent is NOT a dead one), their state is 0, their action 0, reward 0, done 1.
//
//   episode_mlp_counts_pw<EXACT>   K steps in one launch with the worlds in LDS (H*W <= 4096): episode_mlp's step with
//                                  an LDS footprint of ~20 bytes per agent (dw_counts_plan.hpp) and a per-cell stamp map
//                                  in place of its O(N) search per patch cell
//   observe_counts_pw<PrevT, POST> `observe` with the stamp loop bounded by the world's count and all-zero rows for absent
//                                  agents (zero rows -> zero logits -> policy_mlp writes action 0): the launches per step
//   zero_absent_states_pw          the states of absent agents to 0.0 at the start of a call
//
// Barriers of episode_mlp_counts_pw: every __syncthreads() below sits in code all 256 threads run - outside every
// `if (valid)` / `if (on)` - and the only loops that hold one are the step loop (K, a kernel argument) and the pass loop,
// whose trip count `npass` derives from the LARGEST count among the workgroup's worlds (an invalid world b >= B counts 0)
// and is computed by every thread from the same global words.  Lanes without an agent idle through the passes.
#pragma once
#include "dw_agents.hpp"
#include "dw_counts_plan.hpp"
#include "dw_episode.hpp"

namespace dw {

static_assert(kCountsFixCap == kEpFixCap, "ep_forward's near-tie list");

__global__ void zero_absent_states_pw(double* __restrict__ st, const int* __restrict__ n_active, int B, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * N) return;
    const int b = i / N;
    if (i - b * N >= n_active[b]) st[i] = 0.0;
}

// `observe` (dw_agents.hpp) for worlds with n_active[b] of N agents; no reward / done tail
template <typename PrevT, bool POST>
__global__ void observe_counts_pw(const PrevT* __restrict__ pL, const PrevT* __restrict__ pD,
                                  const plane_t* __restrict__ cL, const plane_t* __restrict__ cD,
                                  const int* __restrict__ idx, const double* __restrict__ st,
                                  const int* __restrict__ n_active, int B, int N, int H, int W, PhysF64 P, int mask,
                                  double* __restrict__ obs) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * N * 9) return;
    const int k = gid % 9, an = gid / 9;       // patch cell, flat agent id
    const int b = an / N;
    const int na = n_active[b];
    double* o7 = obs + (size_t)an * 63 + k;    // channel stride 9
    if (an - b * N >= na || !((mask >> k) & 1)) {
#pragma unroll
        for (int ch = 0; ch < 7; ++ch) o7[ch * 9] = 0.0;
        return;
    }
    const int ar = idx[(size_t)an * 2], ac = idx[(size_t)an * 2 + 1];
    const int r = (ar + (k / 3 - 1) + H) % H, c = (ac + (k % 3 - 1) + W) % W;
    const size_t n = (size_t)H * W, woff = (size_t)b * n;
    double l9[9], d9[9];
    gather9(pL + woff, H, W, r, c, l9);
    gather9(pD + woff, H, W, r, c, d9);
    const CellF64 o = cell_f64(P, l9, d9);
    double v[7];
    if (POST) {
        v[0] = dw_div1000(dw_round3_k(P.p - o.nl - o.nd));
        v[1] = to_natural(cL[woff + (size_t)r * W + c]);
        v[2] = to_natural(cD[woff + (size_t)r * W + c]);
        v[3] = dw_div1000(dw_round3_k(o.T));
        v[4] = dw_div1000(dw_round3_k(o.Tl));
        v[5] = dw_div1000(dw_round3_k(o.Td));
    } else {
        v[0] = P.p - l9[4] - d9[4]; v[1] = l9[4]; v[2] = d9[4];
        v[3] = o.T; v[4] = o.Tl; v[5] = o.Td;
    }
    v[6] = 0.0;
    if (POST) {   // ref forward :454-459, the world's own agents only
        for (int a = 0; a < na; ++a) {
            const int rr = idx[((size_t)b * N + a) * 2], cc = idx[((size_t)b * N + a) * 2 + 1];
            if (rr == r && cc == c) v[4] = st[(size_t)b * N + a];
        }
    }
#pragma unroll
    for (int ch = 0; ch < 7; ++ch) o7[ch * 9] = v[ch];
}

struct EpisodeMlpCountsArgs {
    EpisodeMlpIO io;                // as episode_mlp's
    const int* n_active;            // [B]
    StatsDev* trace;                // [K][B] out, or null
    int B, N, H, W, wpb, K, obs_mask, split;
    double agent_gamma, L_prev0;
    PhysF64 P64;
};

template <bool EXACT>
__global__ __launch_bounds__(kCountsThreads) void episode_mlp_counts_pw(EpisodeMlpCountsArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_mlp[kCountsGroups][kCountsBlockDoubles];   // one block per 16-lane group: x 64 | h1 16 | h2 32 | logits 16
    const EpisodeMlpIO& io = A.io;
    const int B = A.B, N = A.N, H = A.H, W = A.W, wpb = A.wpb, K = A.K;
    const int C = H * W;
    const int tpw = kCountsThreads / wpb;                        // threads per world
    const int tid = threadIdx.x, w = tid / tpw, lt = tid - w * tpw;
    const int b = blockIdx.x * wpb + w;
    const bool valid = b < B;
    const int k = valid ? A.n_active[b] : 0;                     // this world's agents: [0, k)
    const size_t world_bytes = episode_mlp_counts_world_bytes(C, N);
    unsigned char* base = smem + (size_t)w * world_bytes;
    float* planes = reinterpret_cast<float*>(base);
    double* ast = reinterpret_cast<double*>(base + (size_t)16 * C);
    int* aidx = reinterpret_cast<int*>(ast + N);
    int* act = aidx + 2 * N;
    int* stamp = act + N;                                        // [C]: the last agent on the cell, -1: none
    unsigned int* red = reinterpret_cast<unsigned int*>(stamp + C);
    unsigned short* fixlist = reinterpret_cast<unsigned short*>(red + 8);
    float* curL = planes;
    float* curD = planes + C;
    float* nxtL = planes + 2 * C;                                // holds the PREVIOUS state between the steps
    float* nxtD = planes + 3 * C;

    // passes of the policy: the same number for every thread of the workgroup
    const int ngrp = tpw >> 4;
    int kmax = 0;
    for (int ww = 0; ww < wpb; ++ww) {
        const int bb = blockIdx.x * wpb + ww;
        const int kk = bb < B ? A.n_active[bb] : 0;
        kmax = kk > kmax ? kk : kmax;
    }
    const int npass = (kmax + ngrp - 1) / ngrp;

    if (valid) {
        for (int c = lt; c < C; c += tpw) {
            curL[c] = (float)io.L[(size_t)b * C + c];
            curD[c] = (float)io.D[(size_t)b * C + c];
            nxtL[c] = (float)io.prevL[(size_t)b * C + c];
            nxtD[c] = (float)io.prevD[(size_t)b * C + c];
        }
        for (int n = lt; n < k; n += tpw) {
            ast[n] = io.st[(size_t)b * N + n];
            aidx[2 * n] = io.idx[((size_t)b * N + n) * 2];
            aidx[2 * n + 1] = io.idx[((size_t)b * N + n) * 2 + 1];
        }
        if (lt < 8) red[lt] = 0;
    }
    __syncthreads();
    const int bc = valid ? b : 0;
    const double* Wa = io.weights + (io.member_a ? (size_t)io.member_a[bc] * 1808 : 0);
    const double* Wb = io.weights + (io.member_b ? (size_t)io.member_b[bc] * 1808 : 0);
    double L_prev = A.L_prev0;
    const int j = lt & 15, g0 = lt >> 4;
    double* x = s_mlp[tid >> 4];

    for (int t = 0; t < K; ++t) {
        // ---- stamps (ref forward :454-459): the highest index on a cell is the reference's "last stamp wins" ----
        if (valid)
            for (int c = lt; c < C; c += tpw) stamp[c] = -1;
        __syncthreads();
        if (valid)
            for (int n = lt; n < k; n += tpw) {
                const int r = aidx[2 * n], c = aidx[2 * n + 1];
                if ((unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W) atomicMax(&stamp[r * W + c], n);
            }
        __syncthreads();
        // ---- policy: one agent per 16-lane group and pass ----
        PhysF64 Qp = A.P64;
        Qp.L = L_prev;
        for (int pass = 0; pass < npass; ++pass) {
            const int n = pass * ngrp + g0;
            const bool on = valid && n < k;
            const double* Wn = n >= A.split ? Wb : Wa;
            const double* W1 = Wn;                 // [63][16]
            const double* W2 = Wn + 63 * 16;       // [16][32]
            const double* W3 = W2 + 16 * 32;      // [32][9]
            // observe (ref get_obs :246-263; `observe<.., POST = true>`'s arithmetic): lane j < 9 owns patch cell j
            if (on && j < 9) {
                if (!((A.obs_mask >> j) & 1)) {
#pragma unroll
                    for (int ch = 0; ch < 7; ++ch) x[ch * 9 + j] = 0.0;
                } else {
                    const int r = (aidx[2 * n] + (j / 3 - 1) + H) % H, c = (aidx[2 * n + 1] + (j % 3 - 1) + W) % W;
                    const int ru = r == 0 ? H - 1 : r - 1, rd = r == H - 1 ? 0 : r + 1;
                    const int cl = c == 0 ? W - 1 : c - 1, cr = c == W - 1 ? 0 : c + 1;
                    const int rows[3] = {ru, r, rd}, cols[3] = {cl, c, cr};
                    double l9[9], d9[9];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int e = 0; e < 3; ++e) {
                            l9[a * 3 + e] = dw_permille_to_natural((double)nxtL[rows[a] * W + cols[e]]);
                            d9[a * 3 + e] = dw_permille_to_natural((double)nxtD[rows[a] * W + cols[e]]);
                        }
                    const CellF64 o = cell_f64(Qp, l9, d9);
                    double v4 = dw_div1000(dw_round3_k(o.Tl));
                    const int s = stamp[r * W + c];
                    if (s >= 0) v4 = ast[s];
                    x[0 * 9 + j] = dw_div1000(dw_round3_k(Qp.p - o.nl - o.nd));
                    x[1 * 9 + j] = dw_permille_to_natural((double)curL[r * W + c]);
                    x[2 * 9 + j] = dw_permille_to_natural((double)curD[r * W + c]);
                    x[3 * 9 + j] = dw_div1000(dw_round3_k(o.T));
                    x[4 * 9 + j] = v4;
                    x[5 * 9 + j] = dw_div1000(dw_round3_k(o.Td));
                    x[6 * 9 + j] = 0.0;
                }
            }
            __syncthreads();
            // the three layers: `policy_mlp`'s sequential fma in index order
            if (on) {
                double h = 0.0;
                for (int i = 0; i < 63; ++i) h = __builtin_fma(x[i], W1[i * 16 + j], h);
                x[64 + j] = h * (h > 0.0 ? 1.0 : 0.0);
            }
            __syncthreads();
            if (on) {
                double u = 0.0, v = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const double hi = x[64 + i];
                    u = __builtin_fma(hi, W2[i * 32 + j], u);
                    v = __builtin_fma(hi, W2[i * 32 + j + 16], v);
                }
                x[80 + j] = u * (u > 0.0 ? 1.0 : 0.0);
                x[80 + j + 16] = v * (v > 0.0 ? 1.0 : 0.0);
            }
            __syncthreads();
            if (on && j < 9) {
                double o = 0.0;
#pragma unroll
                for (int i = 0; i < 32; ++i) o = __builtin_fma(x[80 + i], W3[i * 9 + j], o);
                x[112 + j] = o;
            }
            __syncthreads();
            if (on && j == 0) {
                int best = 0;
                double bestv = x[112];
#pragma unroll
                for (int q = 1; q < 9; ++q) {
                    const double o = x[112 + q];
                    if (o > bestv) { best = q; bestv = o; }    // first maximum, as np.argmax
                }
                act[n] = best;
            }
        }
        __syncthreads();
        // ---- update_agents over the world's k agents: one lane per world, agents in order ----
        if (valid && lt == 0 && k > 0) ep_update_agents(ast, aidx, act, curL, curD, k, H, W, A.agent_gamma);
        __syncthreads();
        // ---- the step's reward / done (ref step :486-492) of all N agents, spread over the lanes ----
        if (valid) {
            for (int n = lt; n < N; n += tpw) {
                const double s = n < k ? ast[n] : 0.0;
                const double rw = s * (s > 0.0 ? 1.0 : 0.0);
                io.reward[((size_t)t * B + b) * N + n] = rw;
                io.done[((size_t)t * B + b) * N + n] = rw < 0.1 ? 1 : 0;
                if (t == K - 1 && io.action) io.action[(size_t)b * N + n] = n < k ? act[n] : 0;
            }
        }
        // ---- forward ----
        const PhysF32 P = io.P32[t];
        PhysF64 Q = A.P64;
        Q.L = io.Ls[t];
        ep_forward<EXACT>(P, Q, curL, curD, nxtL, nxtD, H, W, C, lt, tpw, tid, valid, red, fixlist);
        { float* xx = curL; curL = nxtL; nxtL = xx; xx = curD; curD = nxtD; nxtD = xx; }
        L_prev = io.Ls[t];
        if (valid && lt == 0) {
            if (A.trace) A.trace[(size_t)t * B + b] = StatsDev{red[0], 0u, red[1], red[2]};
            if (t == K - 1) {
                io.stats[b].max_k = red[0];
                io.stats[b].sum_l = red[1];
                io.stats[b].sum_d = red[2];
                if (EXACT && red[3]) atomicAdd(io.fixups, (unsigned long long)red[3]);
            }
        }
        __syncthreads();
        if (valid && lt < 4) red[lt] = 0;
        __syncthreads();
    }

    if (valid) {
        for (int c = lt; c < C; c += tpw) {
            io.L[(size_t)b * C + c] = (plane_t)curL[c];
            io.D[(size_t)b * C + c] = (plane_t)curD[c];
            io.prevL[(size_t)b * C + c] = (plane_t)nxtL[c];
            io.prevD[(size_t)b * C + c] = (plane_t)nxtD[c];
        }
        for (int n = lt; n < k; n += tpw) {
            io.st[(size_t)b * N + n] = ast[n];
            io.idx[((size_t)b * N + n) * 2] = aidx[2 * n];
            io.idx[((size_t)b * N + n) * 2 + 1] = aidx[2 * n + 1];
        }
    }
}

}  // namespace dw
