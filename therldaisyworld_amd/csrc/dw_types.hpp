// dw_types.hpp — the plain data that the host code and the kernels share: constant sets, launch geometry, capacities.
// No HIP header: dw_plan.hpp compiles with these alone under a host compiler (tests/test_plan_cpu.py) - the clang++ of
// ROCm, not g++: PhysF32 is built on clang's ext_vector_type.  Each struct is explained in the kernel header that uses it.
#pragma once

namespace dw {

typedef _Float16 plane_t;     // a cell of a quantised state (dw_common.hpp, "Plane formats")

struct PhysF64 {
    double p, g, S, sigma, gamma, q, q2, dt;
    double ab, al, ad, To;       // albedo bare/light/dark, optimal temperature
    double L;                    // luminosity of this pass
    double w0, w1, w2;           // daisy kernel centre / edge / corner (ref :270-273)
};

typedef float dw_f32x2 __attribute__((ext_vector_type(2)));
#define DW_PAIR(lo_name, hi_name, pair_name) \
    union { struct { float lo_name, hi_name; }; dw_f32x2 pair_name; }

struct PhysF32 {
    // e_x = c0x + a1*Sl8 + a2*Sd8 + a3*li + a4*di, coefficients split hi + lo (exact mode) ...
    DW_PAIR(a1h, a2h, a12h);
    DW_PAIR(a3h, a4h, a34h);
    DW_PAIR(a1l, a2l, a12l);
    DW_PAIR(a3l, a4l, a34l);
    DW_PAIR(c0lh, c0ll, c0l);    // constant for light: hi, lo (the lo part seeds the lo chain)
    DW_PAIR(c0dh, dc0l, c0d);    // constant for dark: hi, and (its lo part - light's lo part)
    // ... or rounded once (float32-only mode): a_i = fl(a_ih + a_il), c0x = fl(c0xh + c0xl)
    DW_PAIR(a1, a2, a12);
    DW_PAIR(a3, a4, a34);
    DW_PAIR(c0ls, c0ds, c0s);
    // dt * (daisy kernel weights): dK = dt * density comes straight out of the weighted sum
    DW_PAIR(dw0, dw1, dw01);
    DW_PAIR(dw2, kbeta, dw2kb);  // kbeta = 1 / sqrt(g * To^2):  beta = 1 - (((T-To)/To) / kbeta)^2
    DW_PAIR(p, ck, pck);         // bare fraction kb = p - (dKl + dKd) * ck,  ck = 0.001 / dt
    // exact-mode tie test (per-mille; om = 1 - beta = cbeta*((T-To)/To)^2 >= 0):
    //   |frac(gq)| > tie_lo - eA*|gq| - |dt*K|*(eK0 + eK1*om)   =>  re-evaluate in float64
    DW_PAIR(eK1s, eK0s, eKs);    // -sign(dt) * eK1, eK0: dK * (eK0s + eK1s*om) = -|dK| * (eK0 + eK1*om) (density >= 0)
    DW_PAIR(ngamma, tie_lo, gt); // -gamma; the tie threshold's constant part
    // the same bracket written in beta = 1 - om (the hot kernels have beta, not om):
    //   eK0s + eK1s*om = (eK0s + eK1s) + (-eK1s)*beta
    DW_PAIR(neK1s, eK01s, eKb);
    float eA;                    // used un-packed (|gq| source modifier); eK0 = |eK0s|, eK1 = |eK1s| (host, audit)
    int hi_bits;                 // the hi parts are multiples of 2^-hi_bits (host bookkeeping)
};
static_assert(sizeof(PhysF32) == 32 * sizeof(float), "PhysF32 layout");

struct PhysLumF32 {
    dw_f32x2 a12h, a12l, c0l, c0d, a12, c0s;
};

struct FirstStepBound {
    float a1, a2, a3, a4;         // |a_i| of the rounded coefficient set
    float c_de, c_c0;             // de = c_de * M + c_c0
    float eK0, eK1, cW, eA, cS, slack;
};

struct PairPw {               // the constants of a step pair of one world (dw_step_fused_pw.hpp)
    PhysF32 P1, P2;              // the sets of step 1 and step 2
};
static_assert(sizeof(PairPw) == 2 * sizeof(PhysF32), "PairPw layout");

struct StatsDev {             // mirrors dw_world_stats
    unsigned int max_k;
    unsigned int reserved;    // the one-wave-per-world episode kernels: float64 re-evaluations of the world's last step
    unsigned long long sum_l;
    unsigned long long sum_d;
};

// launch geometry: tiled (dw_step_tiled.hpp), wave-strip (dw_step_stream.hpp), step pairs (dw_step_fused.hpp), first step
// (dw_step_first.hpp)
struct Geom {
    int B, H, W;
    int Wq;                   // W / 4 (tiled kernel only)
    int tiles_r, tiles_c;     // tiles per world
    int ntiles;               // B * tiles_r * tiles_c
    int chunk;                // ceil(ntiles / 8): tiles per XCD
    int qcap;                 // near-tie LDS queue capacity in use (<= kMaxFix; tests shrink it)
};

struct StripGeom {
    int B, H, W;
    int SR;                   // rows per wave-strip
    int ncs, nrs;             // column / row strips per world
    int nstrips;              // B * nrs * ncs
    int nwg;                  // ceil(nstrips / 4) workgroups of 4 waves
    int chunk;                // ceil(nwg / 8): workgroups per XCD
    int qcap;                 // near-tie LDS queue capacity in use (<= kWaveQueueCap; tests shrink it)
    int lpw, wpr;             // packed mode (W < 256): lanes per world row (W/4), worlds per wave row (64 / lpw)
    int force_rescan;         // tests: every exact strip takes the maximum's re-scan path (see `rescan_max` in stream_body)
};

struct FusedGeom {
    int B, H, W;
    int SR;                   // output rows per wave-strip
    int ncs, nrs;             // column / row strips per world
    int nstrips, nwg, chunk;
    int cols_per_strip;       // 256 (ROT) or 248 (OVL)
    int qcap, mcap;           // queue / mismatch-list capacities in use (tests shrink them)
    int lpw, wpr;             // packed mode (W < 256): lanes per world row (W/4), worlds per wave row (64 / lpw)
    int sure_need;            // STATS: sure step-2 row groups after which a wave's count cannot matter any more:
                              // 9 per agent (patched cells) + 9 per possible step-1 mismatch (deducted) + 1
};

struct FirstGeom {
    int B, H, W;
    int SR;                   // rows per wave-strip (<= 64: a lane's partial sums stay exact in float32)
    int ncs, nrs;             // column (ceil(W / 256); packed: 1) and row strips per world (packed: per world GROUP)
    int nstrips;              // B (packed: world groups) * nrs * ncs
    int lpw, wpr;             // packed mode (W < 256): lanes per world row (W / 4), worlds per wave row (64 / lpw)
};

enum { kFusedOvl = 0, kFusedRot = 1, kFusedRing = 2 };   // strip layout of the step pairs (dw_step_fused.hpp)
// ... and, on overlapped strips, the strip form of the plain float32 format-access kernels (fused2_body, SEAM):
// kSeamStrip  252 output columns per wave: lanes 0..62 own four columns each, lane 63 holds the two halo columns on either
//             side of the strip (a FusedGeom with cols_per_strip = 252 and ncs = W / 252 whole strips)
// kSeamLeft   the W % 252 columns that whole seam strips leave: overlapped strips of W % 252 / 4 + 2 lanes, the same columns
//             of several row bands of one world side by side in a wave (a FusedGeom with lpw = lanes per row band, wpr = row
//             bands per wave, ncs = W / 252, nstrips = B * ceil(nrs / wpr))
enum { kSeamNone = 0, kSeamStrip = 1, kSeamLeft = 2 };
constexpr int kSeamCols = 252;              // output columns of a seam strip
constexpr int kWaveQueueCap = 256;          // near-tie entries per wave-strip held in LDS (48 B each)
constexpr int kMismatchCap = 64;            // float32 step-1 mismatches per wave-strip held in LDS
constexpr int kMaxFix = 1024;     // per-workgroup LDS queue of near-tie cells
constexpr int kNumQueues = 256;   // global queues (one counter cache line each)

}  // namespace dw
