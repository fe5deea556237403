// dw_episode_wave_frames_pw.hpp — episode_wave_frames_pw: episode_wave_temp_pw (dw_episode_wave_temp_pw.hpp: K environment
// steps in one launch, one WAVE per world, H*W <= 256 and N <= 64, with the record and the temperature record of every
// step) that also leaves, at every stride-th step of each SELECTED world, a FRAME (dw_run_episode_frames: the pictures of
// the reference's agent animation, daisy/notebook_helpers.py:180-258 `update_fig_agent` - env.grid[:, :3], env.temp and
// the agent channel env.grid[:, 4] after every env.step(action)); and frame_agents_pw, the agents' part of a frame for
// the shapes that take launches per step.
#pragma once
#include "dw_episode_wave_temp_pw.hpp"
#include "dw_tile_maps.hpp"

namespace dw {

// ---------------------------------------------------------------------------------------------
// What differs from episode_wave_temp_pw:
//  * FIELD says which steps evaluate the float64 temperature of every cell: 0 none (no temperature records and no
//    temperature tiles), 1 the frame steps of selected worlds only (tiles without records), 2 every step (records).  The
//    forward pass (ew_forward_frames_pw<EXACT, WITH_T>, a sibling of ew_forward_stats and ew_forward_temp_pw: the kernels
//    there are held to their recorded instructions) is theirs line by line, with or without T[j].
//  * a wave reads slot_of[b] once: the place of its world among the selected ones, -1 for a world without frames.  "This
//    is a frame step of a selected world" is a scalar, and everything below sits behind that one branch.  A launch starts
//    at a whole number of strides of its call, so its frame `fl` is the step (fl + 1) * stride - 1 of the launch, and the
//    launch's frames fit the device ring (the host splits the call: plan_frame_launches, dw_episode_staging.hpp).
//  * agents: behind ew_update_agents lane n < N stores {row, column, energy store} - what dw_download_agents returns
//    after this step - to the ring.
//  * cover tiles: behind the step's wave barrier the new plane is complete in LDS.  Lane i takes tiles i, i + 64, ... and
//    adds the tile's per-mille integers (exact in any order: tile_cover_pw adds them with atomics); at 1 x 1 tiles that is
//    the lane's own cells, one pair each.
//  * temperature tiles: the lanes' T[j] (cell lane + 64 j) are staged in a per-world LDS area of 8 C bytes and summed in
//    tile_temp_pw's order for the tile size (dw_tile_maps.hpp), "cell i" being the tile's i-th cell in row-major order:
//      MAP 0 (<= 16 cells)  lane i takes tiles i, i + 64, ...: sum = T(cell 0), then += T(cell 1), T(cell 2), ...;
//                           a 1 x 1 tile is the cell's double itself (one term, divided by 1.0)
//      MAP 1 (more)         the wave takes the tiles one after another: lane l adds cells l, l + 64, ... ascending from
//                           0.0, wave_sum_f64, lane 0 divides by the cell count
//    C <= 256 never reaches MAP 2.  T[j] are the doubles cell_temperature returns for the same state (the argument of
//    dw_episode_wave_temp_pw.hpp), so the means are tile_temp_pw's doubles, not merely close ones.
// Records go straight to the ring at frame fl, world slot_of[b]; nothing waits for those stores.
// ---------------------------------------------------------------------------------------------
struct AgentFrameDev { int row, col; double state; };            // mirrors dw_agent_frame

__host__ __device__ constexpr size_t episode_wave_frames_world_bytes(int C, int N) {
    return episode_wave_stats_world_bytes(C, N) + ((size_t)8 * C + 15) / 16 * 16;   // ... | T of every cell
}
__host__ __device__ constexpr size_t episode_wave_frames_lds_bytes(int C, int N) {
    return episode_wave_shared_bytes() + 4 * episode_wave_frames_world_bytes(C, N);
}
// the largest launch (256 cells, 64 agents) stays under the 64 KB a launch may ask for without a function attribute
static_assert(episode_wave_frames_lds_bytes(kEwMaxCells, 64) <= 64 * 1024, "episode_wave_frames_pw: LDS above the default limit");
static_assert(sizeof(AgentFrameDev) == 16, "an agent's frame record is a 16-byte row");
static_assert(kTileThreadCells < 64 && kEwMaxCells <= kTileWaveCells, "a world of this form reduces its tiles by MAP 0 or MAP 1");

// ew_forward_stats (WITH_T = false) / ew_forward_temp_pw (WITH_T = true: T[j] for every slot j the world reaches; a lane
// that does not own the slot evaluates cell 0's neighbourhood, its value is never used).  The arithmetic of a cell's new
// cover is ew_forward's, line by line; the near-tie path takes the same Q.
template <bool EXACT, bool WITH_T>
__device__ __forceinline__ EwLaneStats ew_forward_frames_pw(const PhysF32& P, const PhysF64& Q, const float2* pc, float2* pn,
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
        if constexpr (WITH_T) {
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

// where the frames of a launch go, and the tiles of a world (TileGeom's members the kernel needs)
struct EwFrameOut {
    const int* slot_of;                                         // [B]: the world's place among the selected ones, -1: no frames
    TileCoverDev* cover;                                        // rings [frames][S][TH * TW] / [frames][S][N]; null: not wanted
    double* tmean;
    AgentFrameDev* agents;
    int S, stride, th, tw, TW, tiles, map;
};

// cell i (row-major within the tile) of tile `tile`, as an index into the world's plane
__device__ __forceinline__ int ew_tile_cell(const EwFrameOut& F, int W, int tile, int i) {
    const int tr = tile / F.TW, tc = tile - tr * F.TW;
    const int ir = i / F.tw;
    return (tr * F.th + ir) * W + tc * F.tw + (i - ir * F.tw);
}

// the cover tiles of the complete plane `pn` into rec[tiles]
__device__ __forceinline__ void ew_tile_cover_pw(const EwFrameOut& F, const float2* pn, int W, int lane, TileCoverDev* rec) {
    const int n = F.th * F.tw;
    for (int tile = lane; tile < F.tiles; tile += 64) {
        unsigned int sl = 0u, sd = 0u;
        for (int i = 0; i < n; ++i) {
            const float2 v = pn[ew_tile_cell(F, W, tile, i)];
            sl += (unsigned int)v.x;
            sd += (unsigned int)v.y;
        }
        rec[tile] = TileCoverDev{sl, sd};
    }
}

// the temperature tiles from the staged doubles sT[C] into mean[tiles], in tile_temp_pw's order (see above); every lane
// of the wave is here
__device__ __forceinline__ void ew_tile_temp_pw(const EwFrameOut& F, const double* sT, int W, int lane, double* mean) {
    const int n = F.th * F.tw;
    const double cells = (double)n;
    if (F.map == 0) {
        for (int tile = lane; tile < F.tiles; tile += 64) {
            double sum = sT[ew_tile_cell(F, W, tile, 0)];
            for (int i = 1; i < n; ++i) sum += sT[ew_tile_cell(F, W, tile, i)];
            mean[tile] = sum / cells;
        }
    } else {
        for (int tile = 0; tile < F.tiles; ++tile) {            // wave-uniform
            double sum = 0.0;
            for (int i = lane; i < n; i += 64) sum += sT[ew_tile_cell(F, W, tile, i)];
            sum = wave_sum_f64(sum);
            if (lane == 0) mean[tile] = sum / cells;
        }
    }
}

// episode_wave_temp_pw's argument struct and the frames' destination
struct EpisodeWaveFramesArgs {
    EpisodeIO io;
    StatsDev* trace;                                            // [K][B] out: row t = dw_reduce after step t, reserved = 0
    TempStatsDev* temps;                                        // [K][B] out (FIELD == 2): row t = the temperature field step t computes
    EwFrameOut F;
    int B, N, H, W, K, policy_mode, obs_mask;
    unsigned int thr;
    double agent_gamma;
    PhysF64 P64;                                                // (L: replaced by the step's)
};

template <bool EXACT, int FIELD>
__global__ __launch_bounds__(256) void episode_wave_frames_pw(EpisodeWaveFramesArgs A) {
    const EpisodeIO& io = A.io;
    const EwFrameOut& F = A.F;
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
    unsigned char* const wbase = smem + episode_wave_shared_bytes() + (size_t)wv * episode_wave_frames_world_bytes(C, N);
    float2* const planes = reinterpret_cast<float2*>(wbase);    // [2][C]
    signed char* const sTab = reinterpret_cast<signed char*>(wbase + (size_t)16 * C);
    unsigned long long* const sOk = reinterpret_cast<unsigned long long*>(wbase + (size_t)16 * C + ((size_t)kEwSeg * N + 15) / 16 * 16);
    unsigned int* const sRec = reinterpret_cast<unsigned int*>(wbase + episode_wave_world_bytes(C, N));   // [kEwSeg][3]
    double* const sT = reinterpret_cast<double*>(wbase + episode_wave_stats_world_bytes(C, N));           // [C]
    const bool with_agents = N > 0 && policy_mode != kPolicySkipAgents;
    const bool any_table = policy_mode == kPolicyTable || (policy_mode != kPolicyZeros && io.use_table != nullptr);
    // this world's place among the selected ones (wave-uniform; -1: no frames), the launch's next frame and its step
    const int slot = valid ? __builtin_amdgcn_readfirstlane(F.slot_of[b]) : -1;
    int fl = 0, frame_at = F.stride - 1;

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
            const bool frame_step = t0 + ts == frame_at;         // scalar
            const bool frame = frame_step && slot >= 0;          // scalar: a frame step of a selected world
            const size_t fw = (size_t)fl * F.S + (size_t)(slot >= 0 ? slot : 0);   // this world of this frame, in ring records
            // ---- policy + update_agents ----
            if (with_agents) {
                const bool from_table = policy_mode == kPolicyTable || ((ut_mask >> ts) & 1ull);           // wave-uniform
                const int tab = (int)sTab[ts * N + alane];       // 0..8, or -1 / -2: (anti-)greedy choice (unused unless from_table)
                const EwReach R = ew_reach(pc, ar, ac, H, W);
                const int a = ew_policy_action(policy_mode, from_table, tab, R, obs_mask);
                if (t0 + ts == K - 1 && is_agent && io.action) io.action[(size_t)b * N + lane] = a;
                ew_update_agents(a, R, is_agent, lane, N, W, agent_gamma, ast, ar, ac, pc);
                // the agents of the frame: position and energy store after this step's update_agents
                if (frame && F.agents && is_agent) F.agents[fw * N + lane] = AgentFrameDev{ar, ac, ast};
            }
            // ---- forward (ref :434-461) with this lane's record of what it wrote and, where FIELD asks for it, the temperature
            //      of each of its cells: the field this step computes (ref :410,415), after its grazing and before its growth ----
            const bool last = t0 + ts == K - 1;
            unsigned int nfix = 0;
            PhysF64 Q = A.P64;                                   // the float64 set of this step
            Q.L = sLs[ts];
            double T[kEwSlots] = {0.0, 0.0, 0.0, 0.0};
            const bool tile_temps = frame && F.tmean;            // scalar
            EwLaneStats mine;
            if (FIELD == 2 || (FIELD == 1 && tile_temps)) mine = ew_forward_frames_pw<EXACT, true>(P, Q, pc, pn, G, C, lane, nfix, T);
            else mine = ew_forward_frames_pw<EXACT, false>(P, Q, pc, pn, G, C, lane, nfix, T);
            if (last) last_fix = nfix;
            // ---- the step's record (what dw_reduce reports after it) and the flags of the lifespan harness ----
            const EwStepStats rec = ew_wave_stats(mine);
            if (lane == 0) { sRec[3 * ts] = rec.m; sRec[3 * ts + 1] = rec.sl; sRec[3 * ts + 2] = rec.sd; }
            // ---- the step's temperature record: wave-uniform, one 32-byte row from lane 0 (a store nobody waits for) ----
            if (FIELD == 2) {
                const TempStatsDev trow = ew_wave_temp_pw(T, G, C, cells);
                if (valid && lane == 0) A.temps[(size_t)(t0 + ts) * B + b] = trow;
            }
            if (rec.m > thr) alive_mask |= 1ull << ts;
            if (is_agent) {
                const double rw = ast * (ast > 0.0 ? 1.0 : 0.0);
                if (!(rw < 0.1)) ok_mask |= 1ull << ts;
            }
            if (FIELD != 0 && tile_temps) {                      // the lanes' doubles, cell by cell, for the tile sums
#pragma unroll
                for (int j = 0; j < kEwSlots; ++j)
                    if (G.own[j]) sT[lane + 64 * j] = T[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // the new plane is complete before anyone reads it
            __builtin_amdgcn_wave_barrier();
            // ---- the frame's tiles: cover of the state this step left, means of the field it computed ----
            if (frame) {
                if (F.cover) ew_tile_cover_pw(F, pn, W, lane, F.cover + fw * F.tiles);
                if (FIELD != 0 && tile_temps) ew_tile_temp_pw(F, sT, W, lane, F.tmean + fw * F.tiles);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    // (sT is read before the next frame stages its own)
                __builtin_amdgcn_wave_barrier();
            }
            if (frame_step) { frame_at += F.stride; ++fl; }
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

// The agents' part of a frame where dw_run_episode_frames launches per step: agent n of selected world s (sel[s]; null: s
// itself) into out[s][n].  One thread per record.
__global__ __launch_bounds__(256) void frame_agents_pw(const int* __restrict__ idx, const double* __restrict__ st,
                                                       const int* __restrict__ sel, int S, int N, AgentFrameDev* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * N) return;
    const int s = i / N, n = i - s * N;
    const size_t a = (size_t)(sel ? sel[s] : s) * N + n;
    out[i] = AgentFrameDev{idx[a * 2], idx[a * 2 + 1], st[a]};
}

}  // namespace dw
