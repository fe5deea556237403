// dw_episode_wave_temp_pw.hpp — episode_wave_temp_pw: episode_wave_stats_pw (dw_episode_wave_stats_pw.hpp: K environment
// steps in one launch, one WAVE per world, H*W <= 256 and N <= 64, with the record of every step) that also RECORDS, for
// every step, the statistics of the temperature field that step computes (dw_run_episode_trace_temperature: the curves
// temp.mean() / temp.std() that the reference's agent animation appends after every env.step(action),
// daisy/notebook_helpers.py:210-223 `update_fig_agent`; the field is ref daisy_world_rl.py:410,415 `self.temp`).
#pragma once
#include "dw_episode_wave_stats_pw.hpp"
#include "dw_temp_moments.hpp"

namespace dw {

// ---------------------------------------------------------------------------------------------
// What differs from episode_wave_stats_pw:
//  * the forward pass (ew_forward_temp_pw, a sibling of ew_forward_stats: the kernels there are held to their recorded
//    instructions) also evaluates, for each slot of the lane, cell_f64(Q, l9, d9).T of the 3x3
//    neighbourhood it has just loaded - after ew_update_agents, grazed cells zeroed, before anything is written - with
//    the per-mille floats converted as gather9 converts a binary16 plane (dw_permille_to_natural of the widened value)
//    and Q the handle's float64 set at this step's luminosity.  Those are the doubles temp_moments_pw computes from the
//    same state: the same inline function of the same operands.
//  * the statistics are REDUCED in temp_moments_pw's order, so the record is the same doubles, not merely close ones.
//    There thread i of a 256-thread workgroup holds cell i (a world of this form is one chunk), the four waves reduce by
//    the xor butterfly 32, 16, 8, 4, 2, 1, and thread 0 adds the waves as ((w0 + w1) + w2) + w3.  Here slot j of lane l is
//    cell l + 64 j: slot j IS wave j of that workgroup, lane for lane.  So each slot is reduced across the wave by the
//    same butterfly (wave_sum_f64 / wave_min_f64 / wave_max_f64 themselves) and the slots are combined in index order;
//    a slot the world does not reach contributes +0.0 to the sums and t_ref to the extrema, as a wave whose threads all
//    lie beyond the world's cells does there.  t_ref is lane 0's slot-0 temperature, broadcast: no second evaluation.
//    The finish is temp_moments_finish_pw's expressions for one chunk.
//  * the record is wave-uniform; lane 0 stores the 32-byte row of step t straight to temps[t][b].  Nothing waits for
//    that store, and the LDS of a launch stays episode_wave_stats_pw's.
// The float64 set is hot here (16 of its 32 words every step), so it is read as an ordinary argument and the near-tie
// path takes the same Q.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t episode_wave_temp_lds_bytes(int C, int N) { return episode_wave_stats_lds_bytes(C, N); }
// the largest launch (256 cells, 64 agents) stays under the 64 KB a launch may ask for without a function attribute
static_assert(episode_wave_temp_lds_bytes(kEwMaxCells, 64) <= 64 * 1024, "episode_wave_temp_pw: LDS above the default limit");
static_assert(sizeof(TempStatsDev) == 32, "a temperature record is a 32-byte row");

// ew_forward_stats with the temperature of each of the lane's cells (see above): T[j] for every slot j the world
// reaches (a lane that does not own the slot evaluates cell 0's neighbourhood; its value is never used).  The
// arithmetic of a cell's new cover is ew_forward's, line by line.
template <bool EXACT>
__device__ __forceinline__ EwLaneStats ew_forward_temp_pw(const PhysF32& P, const PhysF64& Q, const float2* pc, float2* pn,
                                                          const EwCells& G, int C, int lane, unsigned int& nfix, double* T) {
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
        {
            double l9[9], d9[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                l9[i] = dw_permille_to_natural((double)nb[i].x);
                d9[i] = dw_permille_to_natural((double)nb[i].y);
            }
            T[j] = cell_f64(Q, l9, d9).T;
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

// The world's temperature record from the lanes' T[j], in temp_moments_pw + temp_moments_finish_pw's order (see above).
// Every lane returns the same record.
__device__ __forceinline__ TempStatsDev ew_wave_temp_pw(const double* T, const EwCells& G, int C, double cells) {
    const long long t0bits = __double_as_longlong(T[0]);
    const double t_ref = __hiloint2double(__builtin_amdgcn_readlane((int)(t0bits >> 32), 0),
                                          __builtin_amdgcn_readlane((int)(t0bits & 0xffffffffll), 0));
    double ws[kEwSlots], wss[kEwSlots], wmn[kEwSlots], wmx[kEwSlots];
#pragma unroll
    for (int j = 0; j < kEwSlots; ++j) { ws[j] = 0.0; wss[j] = 0.0; wmn[j] = t_ref; wmx[j] = t_ref; }
#pragma unroll
    for (int j = 0; j < kEwSlots; ++j) {
        if (j * 64 >= C) break;                                  // wave-uniform
        // a thread of temp_moments_pw with one cell: s = 0.0 + d, ss = 0.0 + d * d, mn = fmin(t_ref, T); without: 0.0, t_ref
        const double d = T[j] - t_ref;
        double s = 0.0, ss = 0.0, mn = t_ref, mx = t_ref;
        s += d;
        ss += d * d;
        mn = fmin(mn, T[j]);
        mx = fmax(mx, T[j]);
        ws[j] = wave_sum_f64(G.own[j] ? s : 0.0);
        wss[j] = wave_sum_f64(G.own[j] ? ss : 0.0);
        wmn[j] = wave_min_f64(G.own[j] ? mn : t_ref);
        wmx[j] = wave_max_f64(G.own[j] ? mx : t_ref);
    }
    const double s = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    const double ss = ((wss[0] + wss[1]) + wss[2]) + wss[3];
    const double mn = fmin(fmin(wmn[0], wmn[1]), fmin(wmn[2], wmn[3]));
    const double mx = fmax(fmax(wmx[0], wmx[1]), fmax(wmx[2], wmx[3]));
    const double md = s / cells;
    const double var = ss / cells - md * md;
    TempStatsDev o;
    o.mean = t_ref + md;
    o.std = var > 0.0 ? sqrt(var) : 0.0;
    o.mn = mn;
    o.mx = mx;
    return o;
}
static_assert(kEwSlots == 4, "ew_wave_temp_pw combines four slots as temp_moments_pw combines four waves");

// episode_wave_stats_pw's argument struct and the temperature records' destination
struct EpisodeWaveTempArgs {
    EpisodeIO io;
    StatsDev* trace;                                            // [K][B] out: row t = dw_reduce after step t, reserved = 0
    TempStatsDev* temps;                                        // [K][B] out: row t = the temperature field step t computes
    int B, N, H, W, K, policy_mode, obs_mask;
    unsigned int thr;
    double agent_gamma;
    PhysF64 P64;                                                // (L: replaced by the step's)
};

template <bool EXACT>
__global__ __launch_bounds__(256) void episode_wave_temp_pw(EpisodeWaveTempArgs A) {
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
            // ---- forward (ref :434-461) with this lane's record of what it wrote, and the temperature of each of its cells:
            //      the field this step computes (ref :410,415), after its grazing and before its growth ----
            const bool last = t0 + ts == K - 1;
            unsigned int nfix = 0;
            PhysF64 Q = A.P64;                                   // the float64 set of this step: every cell's temperature needs it
            Q.L = sLs[ts];
            double T[kEwSlots];
            const EwLaneStats mine = ew_forward_temp_pw<EXACT>(P, Q, pc, pn, G, C, lane, nfix, T);
            if (last) last_fix = nfix;
            // ---- the step's record (what dw_reduce reports after it) and the flags of the lifespan harness ----
            const EwStepStats rec = ew_wave_stats(mine);
            if (lane == 0) { sRec[3 * ts] = rec.m; sRec[3 * ts + 1] = rec.sl; sRec[3 * ts + 2] = rec.sd; }
            // ---- the step's temperature record: wave-uniform, one 32-byte row from lane 0 (a store nobody waits for) ----
            const TempStatsDev trow = ew_wave_temp_pw(T, G, C, cells);
            if (valid && lane == 0) A.temps[(size_t)(t0 + ts) * B + b] = trow;
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
