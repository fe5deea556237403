// dw_episode_wave_stats_pw.hpp — episode_wave_stats_pw: episode_wave (dw_episode_wave.hpp: K environment steps in one
// launch, one WAVE per world, H*W <= 256 and N <= 64) that also RECORDS, for every step, what dw_reduce would report after
// it (dw_run_episode_trace: the daisy populations with grazing agents in them, ref daisy/notebook_helpers.py:218-223
// `update_fig_agent`, notebooks/rl_daisy_world.ipynb cells 12-16, notebooks/greedy_longevity_abatement.ipynb cells 10-15,
// which append env.grid[:,1].mean() / env.grid[:,2].mean() after every env.step(action)); and episode_stats_row_pw, the
// record row of one step for the shapes that take launches per step.
#pragma once
#include "dw_episode_wave.hpp"

namespace dw {

// ---------------------------------------------------------------------------------------------
// What differs from episode_wave:
//  * the forward pass (ew_forward_stats, a sibling of ew_forward: episode_wave itself is held to its recorded
//    instructions) also returns this lane's sums of the light and of the dark values it wrote and their maximum - after
//    the exact mode's float64 repair, owned cells only.  The values are per-mille integers <= 1000 held in floats and a
//    lane owns at most 4 cells: the lane sums (<= 4000) are exact.
//  * per step the three lane values are combined across the wave without LDS: the two sums travel as ONE 32-bit word
//    (light in bits 0-15, dark in bits 16-31) through four DPP adds inside each row of 16 lanes - a row's sum is at most
//    16 * 4000 = 64000 < 2^16, so no carry crosses the fields - the maximum through four DPP maxima; the four rows are
//    read with v_readlane and finished on the scalar unit (each sum <= 256000).  The record {max, sumL, sumD} is
//    wave-uniform: `alive` is max > thr - the same predicate as episode_wave's lane mask, every value being an integer.
//  * lane 0 keeps the step's record (three uint32) in the world's own LDS area of 64 x 12 B; after the segment lane i
//    writes step t0 + i's dw_world_stats row (reserved = 0) next to the segment's flags.  The launch's final io.stats are
//    the last step's record.
// The rest of the step is episode_wave's pieces, called: ew_cells_init, ew_reach, ew_policy_action, ew_update_agents.
// The prologue's loads, the table slice of a segment, the agents' flags and the write-back are written out as there, and
// ew_forward_stats stays next to ew_forward: shared, they changed episode_wave's instructions.
// The price of the records on every other shape is stated at run_episode_stepwise (dw_api.hip): launches per step, no
// fused step pairs, no LDS workgroup kernel.
// ---------------------------------------------------------------------------------------------
constexpr size_t kEwRecBytes = (size_t)kEwSeg * 12;             // a world's records of one segment: {max, sumL, sumD} uint32

__host__ __device__ constexpr size_t episode_wave_stats_world_bytes(int C, int N) {
    return episode_wave_world_bytes(C, N) + kEwRecBytes;        // (both multiples of 16)
}
__host__ __device__ constexpr size_t episode_wave_stats_lds_bytes(int C, int N) {
    return episode_wave_shared_bytes() + 4 * episode_wave_stats_world_bytes(C, N);
}
// the largest launch (256 cells, 64 agents) stays under the 64 KB a launch may ask for without a function attribute
static_assert(episode_wave_stats_lds_bytes(kEwMaxCells, 64) <= 64 * 1024, "episode_wave_stats_pw: LDS above the default limit");

struct EwLaneStats {
    float m, sl, sd;                                            // this lane's maximum / light sum / dark sum of the values it wrote
};

// ew_forward with the lane's record of what it wrote (see above); the arithmetic of a cell is ew_forward's, line by line.
template <bool EXACT, typename Q64>
__device__ __forceinline__ EwLaneStats ew_forward_stats(const PhysF32& P, const float2* pc, float2* pn, const EwCells& G, int C,
                                                        int lane, Q64 q64, unsigned int& nfix) {
    EwLaneStats S{0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kEwSlots; ++j) {
        if (j * 64 >= C) break;                                  // wave-uniform
        float2 nb[9];
        {
            const int rows[3] = {G.rowU[j], G.rowM[j], G.rowD[j]}, cols[3] = {G.colL[j], G.colM[j], G.colR[j]};
#pragma unroll
            for (int a3 = 0; a3 < 3; ++a3)
#pragma unroll
                for (int e3 = 0; e3 < 3; ++e3) nb[a3 * 3 + e3] = pc[rows[a3] + cols[e3]];
        }
        const float li = nb[4].x, di = nb[4].y;
        const float El = (nb[1].x + nb[7].x) + (nb[3].x + nb[5].x);
        const float Cl = (nb[0].x + nb[6].x) + (nb[2].x + nb[8].x);
        const float Ed = (nb[1].y + nb[7].y) + (nb[3].y + nb[5].y);
        const float Cd = (nb[0].y + nb[6].y) + (nb[2].y + nb[8].y);
        const GrowthF32 g = growth_f32<EXACT || kFastSplit>(P, li, di, El, Cl, Ed, Cd);
        float kl, kd;
        if (EXACT) {
            bool tl, td;
            kl = finish_exact(P, li, g.gql, g.dKl, g.oml, tl);
            kd = finish_exact(P, di, g.gqd, g.dKd, g.omd, td);
            const bool tie = G.own[j] && (tl || td);
            if (__builtin_amdgcn_ballot_w64(tie) != 0ull) {       // wave-uniform: rare
                if (tie) {
                    unsigned int wv9[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) wv9[i] = (unsigned)nb[i].x | ((unsigned)nb[i].y << 16);
                    const PhysF64 Q = q64();
                    const NewCoverF64 o64 = cell_f64_lean(Q, wv9);
                    kl = (float)dw_round3_k(o64.nl);
                    kd = (float)dw_round3_k(o64.nd);
                    ++nfix;
                }
            }
        } else {
            kl = finish_fast(li, g.dKl, g.fl);
            kd = finish_fast(di, g.dKd, g.fd);
        }
        if (G.own[j]) pn[lane + 64 * j] = make_float2(kl, kd);
        // (selects, not a branch: a lane that does not own the slot adds nothing)
        const float wl = G.own[j] ? kl : 0.f, wd = G.own[j] ? kd : 0.f;
        S.sl += wl;
        S.sd += wd;
        S.m = fmaxf(S.m, fmaxf(wl, wd));
    }
    return S;
}

// lane i of a row of 16 reads lane `CTRL`(i) of the same row: quad_perm [1,0,3,2] = 0xB1, quad_perm [2,3,0,1] = 0x4E,
// row_half_mirror = 0x141, row_mirror = 0x140 (every lane reads a lane of the wave: no bound to control)
template <int CTRL>
__device__ __forceinline__ unsigned int ew_dpp(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

struct EwStepStats {
    unsigned int m, sl, sd;                                     // wave-uniform: the world's record of a step
};
__device__ __forceinline__ EwStepStats ew_wave_stats(const EwLaneStats& S) {
    unsigned int p = (unsigned int)S.sl | ((unsigned int)S.sd << 16);      // lane sums <= 4000
    unsigned int m = (unsigned int)S.m;
    p += ew_dpp<0xB1>(p);    m = max(m, ew_dpp<0xB1>(m));       // pairs
    p += ew_dpp<0x4E>(p);    m = max(m, ew_dpp<0x4E>(m));       // quads: every lane of a quad holds the quad's
    p += ew_dpp<0x141>(p);   m = max(m, ew_dpp<0x141>(m));      // the other quad of the half row
    p += ew_dpp<0x140>(p);   m = max(m, ew_dpp<0x140>(m));      // the other half row: row sums <= 64000 per field
    const unsigned int p0 = (unsigned int)__builtin_amdgcn_readlane((int)p, 0), p1 = (unsigned int)__builtin_amdgcn_readlane((int)p, 16);
    const unsigned int p2 = (unsigned int)__builtin_amdgcn_readlane((int)p, 32), p3 = (unsigned int)__builtin_amdgcn_readlane((int)p, 48);
    const unsigned int m0 = (unsigned int)__builtin_amdgcn_readlane((int)m, 0), m1 = (unsigned int)__builtin_amdgcn_readlane((int)m, 16);
    const unsigned int m2 = (unsigned int)__builtin_amdgcn_readlane((int)m, 32), m3 = (unsigned int)__builtin_amdgcn_readlane((int)m, 48);
    EwStepStats R;
    R.sl = ((p0 & 0xffffu) + (p1 & 0xffffu)) + ((p2 & 0xffffu) + (p3 & 0xffffu));
    R.sd = ((p0 >> 16) + (p1 >> 16)) + ((p2 >> 16) + (p3 >> 16));
    R.m = max(max(m0, m1), max(m2, m3));
    return R;
}

// episode_wave's argument struct and the records' destination (the float64 constants stay last: cold, read from the
// kernarg segment inside the rare near-tie path)
struct EpisodeWaveStatsArgs {
    EpisodeIO io;
    StatsDev* trace;                                            // [K][B] out: row t = dw_reduce after step t, reserved = 0
    int B, N, H, W, K, policy_mode, obs_mask;
    unsigned int thr;
    double agent_gamma;
    PhysF64 P64;                                                // cold
};

template <bool EXACT>
__global__ __launch_bounds__(256) void episode_wave_stats_pw(EpisodeWaveStatsArgs A) {
    const EpisodeIO& io = A.io;
    const int B = A.B, N = A.N, H = A.H, W = A.W, K = A.K, policy_mode = A.policy_mode, obs_mask = A.obs_mask;
    const unsigned int thr = A.thr;
    const double agent_gamma = A.agent_gamma;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int C = H * W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x * 4 + wv;
    const bool valid = b < B;                                   // (invalid waves still meet the segment barriers)
    PhysF32* const sP32 = reinterpret_cast<PhysF32*>(smem);
    double* const sLs = reinterpret_cast<double*>(smem + (size_t)kEwSeg * sizeof(PhysF32));
    unsigned char* const sUT = smem + (size_t)kEwSeg * sizeof(PhysF32) + (size_t)kEwSeg * sizeof(double);
    unsigned char* const wbase = smem + episode_wave_shared_bytes() + (size_t)wv * episode_wave_stats_world_bytes(C, N);
    float2* const planes = reinterpret_cast<float2*>(wbase);    // [2][C]
    signed char* const sTab = reinterpret_cast<signed char*>(wbase + (size_t)16 * C);
    unsigned long long* const sOk = reinterpret_cast<unsigned long long*>(wbase + (size_t)16 * C + ((size_t)kEwSeg * N + 15) / 16 * 16);
    unsigned int* const sRec = reinterpret_cast<unsigned int*>(wbase + episode_wave_world_bytes(C, N));   // [kEwSeg][3]
    const bool with_agents = N > 0 && policy_mode != kPolicySkipAgents;
    const bool any_table = policy_mode == kPolicyTable || (policy_mode != kPolicyZeros && io.use_table != nullptr);

    EwCells G;
    ew_cells_init(G, lane, C, H, W, valid);
    int cur = 0;                                                // planes[cur*C ..]: the current state
    if (valid) {
#pragma unroll
        for (int j = 0; j < kEwSlots; ++j)
            if (G.own[j]) {
                const int c = lane + 64 * j;
                planes[c] = make_float2((float)io.L[(size_t)b * C + c], (float)io.D[(size_t)b * C + c]);
            }
    }
    // agent n lives in lane n
    const bool is_agent = valid && lane < N;
    const int alane = N > 0 ? min(lane, N - 1) : 0;             // (lanes without an agent shadow the last one's table entry)
    double ast = 0.0;
    int ar = 0, ac = 0;
    if (is_agent) {
        ast = io.st[(size_t)b * N + lane];
        ar = io.idx[((size_t)b * N + lane) * 2];
        ac = io.idx[((size_t)b * N + lane) * 2 + 1];
    }
    unsigned int last_fix = 0;                                  // float64 re-evaluations of the last step (this lane)

    for (int t0 = 0; t0 < K; t0 += kEwSeg) {
        const int seg = min(kEwSeg, K - t0);
        // ---- the segment's constants and this wave's slice of the action table into LDS ----
        __syncthreads();                                        // (the previous segment's readers are done)
        for (int i = tid; i < seg * (int)(sizeof(PhysF32) / 4); i += 256)
            reinterpret_cast<unsigned int*>(sP32)[i] = reinterpret_cast<const unsigned int*>(io.P32 + t0)[i];
        for (int i = tid; i < seg; i += 256) {
            sLs[i] = io.Ls[t0 + i];
            sUT[i] = (policy_mode != kPolicyZeros && io.use_table) ? io.use_table[t0 + i] : 0;
        }
        if (valid && with_agents && any_table && io.table)
            for (int i = lane; i < seg * N; i += 64) {
                const int tt = i / N, n = i - tt * N;
                sTab[i] = io.table[((size_t)(t0 + tt) * B + b) * N + n];
            }
        __syncthreads();
        unsigned long long alive_mask = 0ull, ok_mask = 0ull;   // bit i: step t0 + i (world: uniform; agent: this lane's)
        const unsigned long long ut_mask = __builtin_amdgcn_ballot_w64(lane < seg && sUT[lane] != 0);   // steps that take the table

        for (int ts = 0; ts < seg; ++ts) {
            float2* const pc = planes + cur * C;
            float2* const pn = planes + (1 - cur) * C;
            const PhysF32 P = sP32[ts];
            // ---- policy + update_agents ----
            if (with_agents) {
                const bool from_table = policy_mode == kPolicyTable || ((ut_mask >> ts) & 1ull);           // wave-uniform
                const int tab = (int)sTab[ts * N + alane];       // 0..8, or -1 / -2: (anti-)greedy choice (unused unless from_table)
                const EwReach R = ew_reach(pc, ar, ac, H, W);
                const int a = ew_policy_action(policy_mode, from_table, tab, R, obs_mask);
                if (t0 + ts == K - 1 && is_agent && io.action) io.action[(size_t)b * N + lane] = a;
                ew_update_agents(a, R, is_agent, lane, N, W, agent_gamma, ast, ar, ac, pc);
            }
            // ---- forward (ref :434-461) with this lane's record of what it wrote ----
            const bool last = t0 + ts == K - 1;
            unsigned int nfix = 0;
            const EwLaneStats mine = ew_forward_stats<EXACT>(P, pc, pn, G, C, lane, [&]() {
                const EpisodeWaveStatsArgs* cold = &kernarg_struct<EpisodeWaveStatsArgs>();
                asm volatile("" : "+s"(cold));                   // (keeps the 17 scalar loads inside the cold block)
                PhysF64 Q = cold->P64;
                Q.L = sLs[ts];
                return Q;
            }, nfix);
            if (last) last_fix = nfix;
            // ---- the step's record (what dw_reduce reports after it) and the flags of the lifespan harness ----
            const EwStepStats rec = ew_wave_stats(mine);
            if (lane == 0) { sRec[3 * ts] = rec.m; sRec[3 * ts + 1] = rec.sl; sRec[3 * ts + 2] = rec.sd; }
            if (rec.m > thr) alive_mask |= 1ull << ts;
            if (is_agent) {
                const double rw = ast * (ast > 0.0 ? 1.0 : 0.0);
                if (!(rw < 0.1)) ok_mask |= 1ull << ts;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // the new plane is complete before anyone reads it
            __builtin_amdgcn_wave_barrier();
            cur = 1 - cur;
        }
        // ---- the segment's flags and records ----
        if (valid) {
            for (int i = lane; i < seg; i += 64) {
                io.world_alive[(size_t)(t0 + i) * B + b] = (unsigned char)((alive_mask >> i) & 1ull);
                StatsDev row;
                row.max_k = sRec[3 * i];
                row.reserved = 0u;
                row.sum_l = sRec[3 * i + 1];
                row.sum_d = sRec[3 * i + 2];
                A.trace[(size_t)(t0 + i) * B + b] = row;
            }
            if (N > 0) {
                if (is_agent) sOk[lane] = ok_mask;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int i = lane; i < seg * N; i += 64) {
                    const int tt = i / N, n = i - tt * N;
                    io.agent_ok[((size_t)(t0 + tt) * B + b) * N + n] = (unsigned char)((sOk[n] >> tt) & 1ull);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
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

// The record row of one step where dw_run_episode_trace launches per step: the step kernel's reductions of the new state
// (stats [B]) into row [B] of the trace buffer, `reserved` zeroed.
__global__ void episode_stats_row_pw(const StatsDev* __restrict__ stats, int B, StatsDev* __restrict__ row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        const StatsDev s = stats[i];
        row[i] = StatsDev{s.max_k, 0u, s.sum_l, s.sum_d};
    }
}

}  // namespace dw
