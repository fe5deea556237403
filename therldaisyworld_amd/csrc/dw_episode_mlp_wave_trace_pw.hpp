// dw_episode_mlp_wave_trace_pw.hpp — episode_mlp_wave_trace_pw: episode_mlp_wave (dw_episode_wave.hpp: K environment
// steps with MLP policies in one launch, one WAVE per world, H*W <= 256 and 16 N <= 64) that also RECORDS, for every step,
// what dw_reduce would report after it and, on demand, the statistics of the temperature field that step computes
// (dw_run_episode_mlp_trace: the curves the reference's trained-agent demo appends after every env.step(action) while an
// MLP grazes - env.grid[:,1].mean(), env.grid[:,2].mean(), temp.mean(), temp.std(), daisy/notebook_helpers.py:210-223
// `update_fig_agent`; the field is ref daisy_world_rl.py:410,415 `self.temp`).
#pragma once
#include "dw_episode_wave_temp_pw.hpp"

namespace dw {

// ---------------------------------------------------------------------------------------------
// What differs from episode_mlp_wave (which is held to its recorded instructions, DESIGN.md 7.0000, and is not edited):
//  * the forward pass is ew_forward_stats (!TEMPS) or ew_forward_temp_pw (TEMPS): the cell arithmetic of ew_forward,
//    line by line, with the lane's sums and maximum of what it wrote and, TEMPS, the float64 temperature of each of the
//    lane's cells - after ew_update_agents, grazed cells zeroed, before anything is written.
//  * the step's cover record is ew_wave_stats' (packed DPP sums, the maximum); lane 0 parks it in the world's own LDS
//    area of kEwSeg x 12 bytes behind episode_mlp_wave's world area; after each 64-step segment lane i writes step
//    t0 + i's row (reserved = 0).  The launch's final io.stats are the last step's record, `reserved` the fixup count.
//  * TEMPS: the step's temperature row is ew_wave_temp_pw's - temp_moments_pw's order, the same doubles - from the handle's
//    float64 set at the step's luminosity, which the near-tie repair takes too; lane 0 stores the 32-byte row straight to
//    temps[t][b].  The set is hot in either variant: the observation evaluates cell_f64 with it every step.
// Observe, the sixteen-lanes-per-agent policy, reward / done and the write-back are written out as in episode_mlp_wave;
// ew_cells_init, ew_reach and ew_update_agents are called.  Between the phases there is nothing but the wave's own fences
// and barriers; the two workgroup barriers around a segment's shared rows are met by every wave, valid or not.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t episode_mlp_wave_trace_world_bytes(int C, int N) {
    return episode_mlp_wave_world_bytes(C, N) + kEwRecBytes;    // (both multiples of 16)
}
__host__ __device__ constexpr size_t episode_mlp_wave_trace_lds_bytes(int C, int N) {
    return episode_wave_shared_bytes() + 4 * episode_mlp_wave_trace_world_bytes(C, N);
}
// the largest launch (256 cells, 4 agents: 44 864 bytes) stays under the 64 KB a launch may ask for without a function attribute
static_assert(episode_mlp_wave_trace_lds_bytes(kEwMaxCells, 4) <= 64 * 1024, "episode_mlp_wave_trace_pw: LDS above the default limit");

// episode_mlp_wave's argument struct and the records' destinations
struct EpisodeMlpWaveTraceArgs {
    EpisodeMlpIO io;
    StatsDev* trace;                                            // [K][B] out: row t = dw_reduce after step t, reserved = 0
    TempStatsDev* temps;                                        // [K][B] out (TEMPS): row t = the temperature field step t computes
    int B, N, H, W, K, obs_mask, split;
    double agent_gamma, L_prev0;
    PhysF64 P64;                                                // (L: replaced by the step's)
};

template <bool EXACT, bool TEMPS>
__global__ __launch_bounds__(256) void episode_mlp_wave_trace_pw(EpisodeMlpWaveTraceArgs A) {
    const EpisodeMlpIO& io = A.io;
    const int B = A.B, N = A.N, H = A.H, W = A.W, K = A.K, obs_mask = A.obs_mask, split = A.split;
    const double agent_gamma = A.agent_gamma;
    const double cells = (double)A.H * (double)A.W;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int C = H * W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x * 4 + wv;
    const bool valid = b < B;                                   // (invalid waves still meet the segment barriers)
    PhysF32* const sP32 = reinterpret_cast<PhysF32*>(smem);
    double* const sLs = reinterpret_cast<double*>(smem + (size_t)kEwSeg * sizeof(PhysF32));
    unsigned char* const wbase = smem + episode_wave_shared_bytes() + (size_t)wv * episode_mlp_wave_trace_world_bytes(C, N);
    float2* const planes = reinterpret_cast<float2*>(wbase);    // [2][C]: current | previous (they swap every step)
    double* const mlp = reinterpret_cast<double*>(wbase + (size_t)16 * C);              // [N][128]
    double* const sSt = mlp + (size_t)N * 128;                                           // [N] agent states
    int* const sIdx = reinterpret_cast<int*>(wbase + (size_t)16 * C + (size_t)N * 1024 + ((size_t)8 * N + 15) / 16 * 16);   // [N][2]
    unsigned int* const sRec = reinterpret_cast<unsigned int*>(wbase + episode_mlp_wave_world_bytes(C, N));   // [kEwSeg][3]

    EwCells G;
    ew_cells_init(G, lane, C, H, W, valid);
    int cur = 0;
    if (valid) {
#pragma unroll
        for (int j = 0; j < kEwSlots; ++j)
            if (G.own[j]) {
                const int c = lane + 64 * j;
                planes[c] = make_float2((float)io.L[(size_t)b * C + c], (float)io.D[(size_t)b * C + c]);
                planes[C + c] = make_float2((float)io.prevL[(size_t)b * C + c], (float)io.prevD[(size_t)b * C + c]);
            }
    }
    const bool is_agent = valid && lane < N;
    double ast = 0.0;
    int ar = 0, ac = 0;
    if (is_agent) {
        ast = io.st[(size_t)b * N + lane];
        ar = io.idx[((size_t)b * N + lane) * 2];
        ac = io.idx[((size_t)b * N + lane) * 2 + 1];
        sSt[lane] = ast; sIdx[2 * lane] = ar; sIdx[2 * lane + 1] = ac;
    }
    const int bc = valid ? b : 0;
    const double* const Wa = io.weights + (io.member_a ? (size_t)io.member_a[bc] * 1808 : 0);
    const double* const Wb = io.weights + (io.member_b ? (size_t)io.member_b[bc] * 1808 : 0);
    // sixteen lanes per agent: lane = 16 * agent + j
    const int gj = lane & 15, gn = lane >> 4;
    const bool mlp_on = valid && gn < N;
    const double* const Wn = (split >= 0 && gn >= split) ? Wb : Wa;
    const double* const W1 = Wn;                 // [63][16]
    const double* const W2 = Wn + 63 * 16;       // [16][32]
    const double* const W3 = W2 + 16 * 32;       // [32][9]
    double* const xg = mlp + (size_t)(mlp_on ? gn : 0) * 128;
    // observation lane i < 9 N: patch cell k of agent n
    const int on_ = lane / 9, ok_ = lane - on_ * 9;
    const bool obs_on = valid && lane < 9 * N;
    double L_prev = A.L_prev0;
    unsigned int last_fix = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    for (int t0 = 0; t0 < K; t0 += kEwSeg) {
        const int seg = min(kEwSeg, K - t0);
        __syncthreads();                                        // (the previous segment's readers are done)
        for (int i = tid; i < seg * (int)(sizeof(PhysF32) / 4); i += 256)
            reinterpret_cast<unsigned int*>(sP32)[i] = reinterpret_cast<const unsigned int*>(io.P32 + t0)[i];
        for (int i = tid; i < seg; i += 256) sLs[i] = io.Ls[t0 + i];
        __syncthreads();

        for (int ts = 0; ts < seg; ++ts) {
            float2* const pc = planes + cur * C;                 // current state
            float2* const pp = planes + (1 - cur) * C;           // the state before the last step taken (becomes the new one)
            const PhysF32 P = sP32[ts];
            const EwReach R = ew_reach(pc, ar, ac, H, W);        // (pre-graze covers: what update_agents needs below)
            // ---- observe (ref get_obs :246-263; the `observe<.., POST = true>` kernel's arithmetic) ----
            if (obs_on) {
                double* x = mlp + (size_t)on_ * 128;
                const int k = ok_;
                if (!((obs_mask >> k) & 1)) {
#pragma unroll
                    for (int ch = 0; ch < 7; ++ch) x[ch * 9 + k] = 0.0;
                } else {
                    PhysF64 Qp = A.P64;
                    Qp.L = L_prev;
                    const int pr = sIdx[2 * on_], pcn = sIdx[2 * on_ + 1];
                    int r = pr + (k / 3 - 1), c = pcn + (k % 3 - 1);
                    r = r < 0 ? r + H : (r >= H ? r - H : r);
                    c = c < 0 ? c + W : (c >= W ? c - W : c);
                    const int ru = r == 0 ? H - 1 : r - 1, rd = r == H - 1 ? 0 : r + 1;
                    const int cl = c == 0 ? W - 1 : c - 1, cr = c == W - 1 ? 0 : c + 1;
                    const int rows[3] = {ru, r, rd}, cols[3] = {cl, c, cr};
                    double l9[9], d9[9];
#pragma unroll
                    for (int a3 = 0; a3 < 3; ++a3)
#pragma unroll
                        for (int e3 = 0; e3 < 3; ++e3) {
                            const float2 v = pp[rows[a3] * W + cols[e3]];
                            l9[a3 * 3 + e3] = dw_permille_to_natural((double)v.x);      // = (double)k / 1000.0 exactly
                            d9[a3 * 3 + e3] = dw_permille_to_natural((double)v.y);
                        }
                    const CellF64 o = cell_f64(Qp, l9, d9);
                    double v4 = dw_div1000(dw_round3_k(o.Tl));
                    for (int a2 = 0; a2 < N; ++a2)                // ref forward :454-459: agent states stamped, last wins
                        if (sIdx[2 * a2] == r && sIdx[2 * a2 + 1] == c) v4 = sSt[a2];
                    const float2 cc2 = pc[r * W + c];
                    x[0 * 9 + k] = dw_div1000(dw_round3_k(Qp.p - o.nl - o.nd));
                    x[1 * 9 + k] = dw_permille_to_natural((double)cc2.x);
                    x[2 * 9 + k] = dw_permille_to_natural((double)cc2.y);
                    x[3 * 9 + k] = dw_div1000(dw_round3_k(o.T));
                    x[4 * 9 + k] = v4;
                    x[5 * 9 + k] = dw_div1000(dw_round3_k(o.Td));
                    x[6 * 9 + k] = 0.0;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // ---- policy: 63 -> 16 -> 32 -> 9, ReLU, float64, sequential dot products ----
            int act = 0;
            {
                double h = 0.0;
                for (int i = 0; i < 63; ++i) h = __builtin_fma(xg[i], W1[i * 16 + gj], h);
                if (mlp_on) xg[64 + gj] = h * (h > 0.0 ? 1.0 : 0.0);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                double u = 0.0, v = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const double hi = xg[64 + i];
                    u = __builtin_fma(hi, W2[i * 32 + gj], u);
                    v = __builtin_fma(hi, W2[i * 32 + gj + 16], v);
                }
                if (mlp_on) {
                    xg[80 + gj] = u * (u > 0.0 ? 1.0 : 0.0);
                    xg[80 + gj + 16] = v * (v > 0.0 ? 1.0 : 0.0);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int gj9 = gj < 9 ? gj : 8;
                double o = 0.0;
#pragma unroll
                for (int i = 0; i < 32; ++i) o = __builtin_fma(xg[80 + i], W3[i * 9 + gj9], o);
                if (mlp_on && gj < 9) xg[112 + gj] = o;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                // agent lane n: first maximum of its nine logits, as np.argmax
                const double* lg = mlp + (size_t)(is_agent ? lane : 0) * 128 + 112;
                int best = 0;
                double bestv = lg[0];
#pragma unroll
                for (int k = 1; k < 9; ++k) {
                    const double ov = lg[k];
                    const bool bt = ov > bestv;
                    best = bt ? k : best;
                    bestv = bt ? ov : bestv;
                }
                act = best;
            }
            // ---- update_agents; the step's reward / done (ref step :486-492) ----
            ew_update_agents(act, R, is_agent, lane, N, W, agent_gamma, ast, ar, ac, pc);
            if (t0 + ts == K - 1 && is_agent && io.action) io.action[(size_t)b * N + lane] = act;
            if (is_agent) {
                sSt[lane] = ast; sIdx[2 * lane] = ar; sIdx[2 * lane + 1] = ac;
                const double rw = ast * (ast > 0.0 ? 1.0 : 0.0);
                io.reward[((size_t)(t0 + ts) * B + b) * N + lane] = rw;
                io.done[((size_t)(t0 + ts) * B + b) * N + lane] = rw < 0.1 ? 1 : 0;
            }
            // ---- forward: the current planes advance into the buffer of the previous state, with this lane's record of what
            //      it wrote and, TEMPS, the temperature of each of its cells (the field this step computes, ref :410,415) ----
            unsigned int nfix = 0;
            const double Lt = sLs[ts];
            EwLaneStats mine;
            if constexpr (TEMPS) {
                PhysF64 Q = A.P64;                               // the float64 set of this step: every cell's temperature needs it
                Q.L = Lt;
                double T[kEwSlots];
                mine = ew_forward_temp_pw<EXACT>(P, Q, pc, pp, G, C, lane, nfix, T);
                // the step's temperature record: wave-uniform, one 32-byte row from lane 0 (a store nobody waits for)
                const TempStatsDev trow = ew_wave_temp_pw(T, G, C, cells);
                if (valid && lane == 0) A.temps[(size_t)(t0 + ts) * B + b] = trow;
            } else {
                mine = ew_forward_stats<EXACT>(P, pc, pp, G, C, lane, [&]() { PhysF64 Q = A.P64; Q.L = Lt; return Q; }, nfix);
            }
            if (t0 + ts == K - 1) last_fix = nfix;
            // ---- the step's record (what dw_reduce reports after it) ----
            const EwStepStats rec = ew_wave_stats(mine);
            if (lane == 0) { sRec[3 * ts] = rec.m; sRec[3 * ts + 1] = rec.sl; sRec[3 * ts + 2] = rec.sd; }
            L_prev = Lt;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            cur = 1 - cur;
        }
        // ---- the segment's records (the wave's own LDS rows: no workgroup barrier in here) ----
        if (valid) {
            for (int i = lane; i < seg; i += 64) {
                StatsDev row;
                row.max_k = sRec[3 * i];
                row.reserved = 0u;
                row.sum_l = sRec[3 * i + 1];
                row.sum_d = sRec[3 * i + 2];
                A.trace[(size_t)(t0 + i) * B + b] = row;
            }
        }
    }

    // ---- back to global memory: planes, the state before the last step (after its grazing), agents, the last record ----
    if (valid) {
        const float2* const pc = planes + cur * C;
        const float2* const pp = planes + (1 - cur) * C;
#pragma unroll
        for (int j = 0; j < kEwSlots; ++j)
            if (G.own[j]) {
                const int c = lane + 64 * j;
                const float2 v = pc[c], w = pp[c];
                io.L[(size_t)b * C + c] = (plane_t)v.x;
                io.D[(size_t)b * C + c] = (plane_t)v.y;
                io.prevL[(size_t)b * C + c] = (plane_t)w.x;
                io.prevD[(size_t)b * C + c] = (plane_t)w.y;
            }
        if (is_agent) {
            io.st[(size_t)b * N + lane] = ast;
            io.idx[((size_t)b * N + lane) * 2] = ar;
            io.idx[((size_t)b * N + lane) * 2 + 1] = ac;
        }
        const unsigned int nf = (unsigned int)wave_sum((float)last_fix);
        if (lane == 0) {                                        // the world's whole record is ASSIGNED: no memset before the launch
            const unsigned int* const r = sRec + 3 * ((K - 1) % kEwSeg);    // the last step's record (K >= 1)
            if (b == 0) io.stats[B] = StatsDev{0u, 0u, 0ull, 0ull};   // ... and the counter record behind the worlds'
            io.stats[b].max_k = r[0];
            io.stats[b].reserved = EXACT ? nf : 0u;              // float64 re-evaluations of the last step (dw_last_fixup_count sums them)
            io.stats[b].sum_l = r[1];
            io.stats[b].sum_d = r[2];
        }
    }
}

}  // namespace dw
