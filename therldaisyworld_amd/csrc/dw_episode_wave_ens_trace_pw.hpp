// dw_episode_wave_ens_trace_pw.hpp — episode_wave_ens_trace_pw: episode_wave_pw (dw_episode_wave_pw.hpp: K environment
// steps in one launch, one WAVE per world, H*W <= 256 and N <= 64, the physics constants of a step taken from the wave's
// OWN world) that also RECORDS, for every step, what dw_reduce would report after it and - TEMPS - the statistics of the
// temperature field that step computes, as episode_wave_temp_pw (dw_episode_wave_temp_pw.hpp) does with one constant set
// (dw_run_episode_ensemble_trace: the population and temperature curves of every scenario of the reference's README -
// greedy, anti-greedy, random and no agents under light-and-dark and under neutral albedos - side by side from ONE
// device-resident run).
#pragma once
#include "dw_episode_wave_pw.hpp"
#include "dw_episode_wave_temp_pw.hpp"

namespace dw {

// ---------------------------------------------------------------------------------------------
// The data path is episode_wave_pw's: io.P32 and io.Ls are [K][B] tables, a wave stages the rows of ITS world for a
// 64-step segment in its own LDS region with 16-byte loads behind one workgroup barrier per segment.  The records are
// episode_wave_temp_pw's: ew_forward_temp_pw / ew_wave_temp_pw reduce the four 64-cell slots in temp_moments_pw's order,
// ew_wave_stats combines the lanes' sums and maximum by DPP, the cover records of a segment wait in the world's LDS area
// and are written next to the segment's flags, lane 0 stores each 32-byte temperature row straight to temps[t][b].
// What differs from both:
//  * a world's float64 set is fixed for the whole launch - make_f64(params, L) depends on L in its member L only - and
//    with TEMPS it is hot (every step, every cell).  P64[b] is loaded ONCE per launch, wave-uniformly (b is wave-uniform:
//    scalar loads into SGPRs; a wave beyond the last world reads world B - 1's and uses nothing of it); per step only
//    Q.L = sLs[ts] changes, and the near-tie repair takes the same Q.  Those are the operands a one-world handle that
//    carries worlds[b] passes to the same cell_f64: the same doubles.
//  * TEMPS == false evaluates no float64 field: ew_forward_stats with episode_wave_pw's cold-branch read of P64[b].
//  * LDS per workgroup: use_table of a segment + 4 x (a world's P32 | Ls rows + episode_wave_stats_pw's world area):
//    about 71 KB at 256 cells and 64 agents - above the 64 KB default, under a CU's 160 KB - asked for by function
//    attribute as episode_wave_pw does.
// The existing kernels are held to their recorded instructions: their pieces are called, their
// prologue, segment loads, write-out and write-back are written out again here.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t episode_wave_ens_trace_world_bytes(int C, int N) {
    return episode_wave_pw_const_bytes() + episode_wave_stats_world_bytes(C, N);       // (both multiples of 16)
}
__host__ __device__ constexpr size_t episode_wave_ens_trace_lds_bytes(int C, int N) {
    return episode_wave_pw_shared_bytes() + 4 * episode_wave_ens_trace_world_bytes(C, N);
}
static_assert(episode_wave_ens_trace_lds_bytes(kEwMaxCells, 64) <= 160 * 1024, "episode_wave_ens_trace_pw: LDS above a CU's 160 KB");

struct EpisodeWaveEnsTraceArgs {
    EpisodeIO io;                                               // P32: [K][B], Ls: [K][B]
    StatsDev* trace;                                            // [K][B] out: row t = dw_reduce after step t, reserved = 0
    TempStatsDev* temps;                                        // [K][B] out (TEMPS): row t = the temperature field step t computes
    const PhysF64* P64;                                         // [B]: world b's float64 set (its L is replaced per step)
    int B, N, H, W, K, policy_mode, obs_mask;
    unsigned int thr;
    double agent_gamma;
};

template <bool EXACT, bool TEMPS>
__global__ __launch_bounds__(256) void episode_wave_ens_trace_pw(EpisodeWaveEnsTraceArgs A) {
    const EpisodeIO& io = A.io;
    const int B = A.B, N = A.N, H = A.H, W = A.W, K = A.K, policy_mode = A.policy_mode, obs_mask = A.obs_mask;
    const unsigned int thr = A.thr;
    const double agent_gamma = A.agent_gamma;
    const double cells = (double)A.H * (double)A.W;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int C = H * W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x * 4 + wv;
    const bool valid = b < B;                                   // (invalid waves still meet the segment barriers)
    unsigned char* const sUT = smem;
    unsigned char* const cbase = smem + episode_wave_pw_shared_bytes() + (size_t)wv * episode_wave_ens_trace_world_bytes(C, N);
    PhysF32* const sP32 = reinterpret_cast<PhysF32*>(cbase);    // [kEwSeg]: this world's rows
    double* const sLs = reinterpret_cast<double*>(cbase + (size_t)kEwSeg * sizeof(PhysF32));
    unsigned char* const wbase = cbase + episode_wave_pw_const_bytes();
    float2* const planes = reinterpret_cast<float2*>(wbase);    // [2][C]
    signed char* const sTab = reinterpret_cast<signed char*>(wbase + (size_t)16 * C);
    unsigned long long* const sOk = reinterpret_cast<unsigned long long*>(wbase + (size_t)16 * C + ((size_t)kEwSeg * N + 15) / 16 * 16);
    unsigned int* const sRec = reinterpret_cast<unsigned int*>(wbase + episode_wave_world_bytes(C, N));   // [kEwSeg][3]
    const bool with_agents = N > 0 && policy_mode != kPolicySkipAgents;
    const bool any_table = policy_mode == kPolicyTable || (policy_mode != kPolicyZeros && io.use_table != nullptr);

    // the world's float64 set: wave-uniform, once per launch (TEMPS; without, it stays behind the cold branch)
    PhysF64 Q{};
    if (TEMPS) Q = A.P64[valid ? b : B - 1];

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
        // ---- the segment's rows of this wave's world, use_table, and the wave's slice of the action table into LDS ----
        __syncthreads();                                        // (the previous segment's readers are done)
        if (valid) {
            constexpr int kQ = (int)(sizeof(PhysF32) / 16);     // 16-byte words per row: eight lanes fetch one row
            for (int i = lane; i < seg * kQ; i += 64) {
                const int r = i / kQ, q = i - r * kQ;
                reinterpret_cast<uint4*>(sP32)[i] = reinterpret_cast<const uint4*>(io.P32 + ((size_t)(t0 + r) * B + b))[q];
            }
            for (int i = lane; i < seg; i += 64) sLs[i] = io.Ls[(size_t)(t0 + i) * B + b];
        }
        for (int i = tid; i < seg; i += 256) sUT[i] = (policy_mode != kPolicyZeros && io.use_table) ? io.use_table[t0 + i] : 0;
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
            // ---- forward (ref :434-461) at this world's constants, with this lane's record of what it wrote and (TEMPS)
            //      the temperature of each of its cells: the field this step computes, after its grazing, before its growth ----
            const bool last = t0 + ts == K - 1;
            unsigned int nfix = 0;
            EwLaneStats mine;
            if constexpr (TEMPS) {
                Q.L = sLs[ts];
                double T[kEwSlots];
                mine = ew_forward_temp_pw<EXACT>(P, Q, pc, pn, G, C, lane, nfix, T);
                // the step's temperature record: wave-uniform, one 32-byte row from lane 0 (a store nobody waits for)
                const TempStatsDev trow = ew_wave_temp_pw(T, G, C, cells);
                if (valid && lane == 0) A.temps[(size_t)(t0 + ts) * B + b] = trow;
            } else {
                mine = ew_forward_stats<EXACT>(P, pc, pn, G, C, lane, [&]() {
                    const PhysF64* cold = kernarg_struct<EpisodeWaveEnsTraceArgs>().P64 + b;   // (a tie implies an owned cell: b < B)
                    asm volatile("" : "+s"(cold));               // (keeps the scalar loads inside the cold block)
                    PhysF64 Qc = *cold;
                    Qc.L = sLs[ts];
                    return Qc;
                }, nfix);
            }
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

}  // namespace dw
