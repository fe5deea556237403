// dw_episode_wave_pw.hpp — episode_wave_pw: episode_wave (dw_episode_wave.hpp: K environment steps in one launch, one
// WAVE per world, H*W <= 256 and N <= 64) with the physics constants of a step taken from the wave's OWN world
// (dw_run_episode_ensemble: the reference's lifespan table, notebooks/greedy_longevity_abatement.ipynb, albedo settings x
// policies, or a lifespan-versus-q2 / gamma / temp_optimal scan, as ONE device-resident run).
#pragma once
#include "dw_episode_wave.hpp"

namespace dw {

// ---------------------------------------------------------------------------------------------
// What differs from episode_wave:
//  * io.P32 and io.Ls are [K][B] tables (row t, world b: derive_f32 / the luminosity of world b's params at step t, all
//    derived on the host in float64 - nothing is derived here).  A wave stages the rows of ITS world for a 64-step segment
//    in its own LDS region (8 KB + 512 B) with 16-byte loads, behind the same single workgroup barrier per segment;
//    episode_wave's block shares one copy of one row per step.  use_table stays one byte per step for the whole block.
//  * the float64 repair set of a near-tie cell is the world's own: P64[b] (read through a pointer by scalar loads, inside
//    the rare branch) with the step's luminosity from the wave's LDS rows.
// The step itself is episode_wave's pieces, called: ew_cells_init, ew_reach, ew_policy_action, ew_update_agents, ew_forward.
// The prologue's loads, the table slice of a segment, the flags' write-out and the write-back are written out as there: as
// helpers they changed the instructions of episode_wave, which is held to its recorded ones.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t episode_wave_pw_shared_bytes() { return kEwSeg; }        // use_table of one segment
__host__ __device__ constexpr size_t episode_wave_pw_const_bytes() {                           // a world's P32 | Ls rows of one segment
    return (size_t)kEwSeg * sizeof(PhysF32) + (size_t)kEwSeg * sizeof(double);
}
__host__ __device__ constexpr size_t episode_wave_pw_world_bytes(int C, int N) {
    return episode_wave_pw_const_bytes() + episode_wave_world_bytes(C, N);
}

struct EpisodeWavePwArgs {
    EpisodeIO io;                                               // P32: [K][B], Ls: [K][B]
    const PhysF64* P64;                                         // [B]: world b's float64 set (its L is replaced per step); cold
    int B, N, H, W, K, policy_mode, obs_mask;
    unsigned int thr;
    double agent_gamma;
};

template <bool EXACT>
__global__ __launch_bounds__(256) void episode_wave_pw(EpisodeWavePwArgs A) {
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
    unsigned char* const sUT = smem;
    unsigned char* const cbase = smem + episode_wave_pw_shared_bytes() + (size_t)wv * episode_wave_pw_world_bytes(C, N);
    PhysF32* const sP32 = reinterpret_cast<PhysF32*>(cbase);    // [kEwSeg]: this world's rows
    double* const sLs = reinterpret_cast<double*>(cbase + (size_t)kEwSeg * sizeof(PhysF32));
    unsigned char* const wbase = cbase + episode_wave_pw_const_bytes();
    float2* const planes = reinterpret_cast<float2*>(wbase);    // [2][C]
    signed char* const sTab = reinterpret_cast<signed char*>(wbase + (size_t)16 * C);
    unsigned long long* const sOk = reinterpret_cast<unsigned long long*>(wbase + (size_t)16 * C + ((size_t)kEwSeg * N + 15) / 16 * 16);
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
    const float thr_f = (float)thr;
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
            // ---- forward (ref :434-461) at this world's constants ----
            const bool last = t0 + ts == K - 1;
            unsigned int nfix = 0;
            const bool alive_here = ew_forward<EXACT>(P, pc, pn, G, C, lane, thr_f, [&]() {
                const PhysF64* cold = kernarg_struct<EpisodeWavePwArgs>().P64 + b;   // (a tie implies an owned cell: b < B)
                asm volatile("" : "+s"(cold));                   // (keeps the scalar loads inside the cold block)
                PhysF64 Q = *cold;
                Q.L = sLs[ts];
                return Q;
            }, nfix);
            if (last) last_fix = nfix;
            // ---- per-step flags of the lifespan harness (nb greedy cell 2:46-52) ----
            if (__builtin_amdgcn_ballot_w64(alive_here) != 0ull) alive_mask |= 1ull << ts;
            if (is_agent) {
                const double rw = ast * (ast > 0.0 ? 1.0 : 0.0);
                if (!(rw < 0.1)) ok_mask |= 1ull << ts;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // the new plane is complete before anyone reads it
            __builtin_amdgcn_wave_barrier();
            cur = 1 - cur;
        }
        // ---- the segment's flags ----
        if (valid) {
            for (int i = lane; i < seg; i += 64) io.world_alive[(size_t)(t0 + i) * B + b] = (unsigned char)((alive_mask >> i) & 1ull);
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

    // ---- back to global memory: planes, the state before the last step (after its grazing), agents, reductions ----
    if (valid) {
        const float2* const pc = planes + cur * C;
        const float2* const pp = planes + (1 - cur) * C;
        float m = 0.f, sl = 0.f, sd = 0.f;
#pragma unroll
        for (int j = 0; j < kEwSlots; ++j)
            if (G.own[j]) {
                const int c = lane + 64 * j;
                const float2 v = pc[c], w = pp[c];
                io.L[(size_t)b * C + c] = (plane_t)v.x;
                io.D[(size_t)b * C + c] = (plane_t)v.y;
                io.prevL[(size_t)b * C + c] = (plane_t)w.x;
                io.prevD[(size_t)b * C + c] = (plane_t)w.y;
                m = fmaxf(m, fmaxf(v.x, v.y));
                sl += v.x;
                sd += v.y;
            }
        if (is_agent) {
            io.st[(size_t)b * N + lane] = ast;
            io.idx[((size_t)b * N + lane) * 2] = ar;
            io.idx[((size_t)b * N + lane) * 2 + 1] = ac;
        }
        m = wave_max(m);
        sl = wave_sum(sl);                                       // integers < 2^24: exact in any order
        sd = wave_sum(sd);
        const unsigned int nf = (unsigned int)wave_sum((float)last_fix);
        if (lane == 0) {                                        // the world's whole record is ASSIGNED: no memset before the launch
            if (b == 0) io.stats[B] = StatsDev{0u, 0u, 0ull, 0ull};   // ... and the counter record behind the worlds'
            io.stats[b].max_k = (unsigned int)m;
            io.stats[b].reserved = EXACT ? nf : 0u;              // float64 re-evaluations of the last step (dw_last_fixup_count sums them)
            io.stats[b].sum_l = (unsigned long long)sl;
            io.stats[b].sum_d = (unsigned long long)sd;
        }
    }
}

}  // namespace dw
