// dw_plan.hpp — what the host decides before a launch, as pure functions of dw_params, the switches and plain structs:
// the experiment / test switches (read_switches: the one reader of the environment), which kernels take the steps and
// their launch geometry (plan_steps), and the constant sets of a step (make_f64, derive_f32, derive_f32_pair,
// derive_first_bound).  No HIP call and no HIP header: dw_api.hip includes it, and tests/test_plan_cpu.py compiles it alone
// with the host clang++ and holds every value it produces to a recorded fixture.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/daisyworld_hip.h"
#include "dw_types.hpp"

namespace dw {

// ---- switches ------------------------------------------------------------------------------------------------------
// Experiment and test switches (environment variables), read ONCE per handle at dw_create - a handle behaves the same for
// its whole life whatever the environment does afterwards - and reported by dw_kernel_info when any is set.  None changes
// results.  The DW_TEST_* hooks (shrunk queues, injected allocation failures, forced fallbacks) are honoured only when
// DW_TEST_HOOKS is set as well: a stray variable in a user's environment cannot inject failures.
//   DW_STRIP_ROWS=n        rows per wave-strip of the steady-state, step-pair AND first-step kernels instead of strip_rows()'s
//                          choice (the first-step kernel: at most 64, the height its float32 partial sums stay exact at)
//   DW_NO_FMT_PLANES=1     the plain overlapped-strip step pairs read and write their rows with ordinary global accesses
//                          instead of format buffer accesses (StepPlan::fmt_planes): an A/B in one process
//   DW_NO_SEAM_STRIPS=1    the format-access step pairs keep their overlapped 248-column strips instead of seam strips with
//                          packed leftover columns (StepPlan::seam_strips): an A/B in one process
//   DW_NO_ROW_LANDING=1    the seam-strip step pairs keep the kernels whose prefetched rows change registers once instead of
//                          those whose rows land in their window slots (StepPlan::row_landing): an A/B in one process
//   DW_TEST_TRACE_ROWS=n   (test hook) dw_step_n_trace holds n rows of the series on the device at a time (rounded down to
//                          even, at least 2) instead of 32 MiB of them: multi-chunk runs with a handful of worlds
//   DW_TEST_FRAME_RING=n   (test hook) dw_step_n_frames holds n frames on the device at a time instead of 32 MiB of them
struct Switches {
    bool no_sym = false, no_pack = false, no_fuse = false, no_ring = false, no_fmt_planes = false, no_seam_strips = false,
         no_row_landing = false,
         no_episode_kernel = false,
         no_episode_wave = false, no_agent_fuse = false, no_agent_preapply = false, first_f64 = false,
         first_generic = false, force_rescan = false, test_hooks = false;
    int pack_min_strips = -1, strip_rows = 0, tile_rpt = 0, queue_cap = -1, mismatch_cap = -1, trace_rows = 0, frame_ring = 0;
    double first_slack = -1.0;
    char kernel[16] = {0};           // DW_KERNEL: "tiled" | "stream"
    char text[256] = {0};            // what was set, for dw_kernel_info
};
inline const char* test_hook(const char* name) {              // a DW_TEST_* variable, only under DW_TEST_HOOKS
    return std::getenv("DW_TEST_HOOKS") ? std::getenv(name) : nullptr;
}
inline Switches read_switches() {
    Switches w;
    auto note = [&](const char* name, const char* val) {
        const size_t n = std::strlen(w.text);
        snprintf(w.text + n, sizeof(w.text) - n, "%s%s%s%s", n ? " " : "", name, val ? "=" : "", val ? val : "");
    };
    auto flag = [&](const char* name, bool& dst) { if (std::getenv(name)) { dst = true; note(name, nullptr); } };
    auto num = [&](const char* name, int& dst, bool test) {
        if (const char* e = test ? test_hook(name) : std::getenv(name)) { dst = std::atoi(e); note(name, e); }
    };
    w.test_hooks = std::getenv("DW_TEST_HOOKS") != nullptr;
    flag("DW_NO_SYM", w.no_sym); flag("DW_NO_PACK", w.no_pack); flag("DW_NO_FUSE", w.no_fuse); flag("DW_NO_RING", w.no_ring);
    flag("DW_NO_FMT_PLANES", w.no_fmt_planes); flag("DW_NO_SEAM_STRIPS", w.no_seam_strips);
    flag("DW_NO_ROW_LANDING", w.no_row_landing);
    flag("DW_NO_EPISODE_KERNEL", w.no_episode_kernel); flag("DW_NO_EPISODE_WAVE", w.no_episode_wave);
    flag("DW_NO_AGENT_FUSE", w.no_agent_fuse); flag("DW_NO_AGENT_PREAPPLY", w.no_agent_preapply);
    flag("DW_FIRST_STEP_F64", w.first_f64); flag("DW_FIRST_GENERIC", w.first_generic);
    num("DW_PACK_MIN_STRIPS", w.pack_min_strips, false); num("DW_STRIP_ROWS", w.strip_rows, false);
    num("DW_TILE_RPT", w.tile_rpt, false);
    num("DW_TEST_QUEUE_CAP", w.queue_cap, true); num("DW_TEST_MISMATCH_CAP", w.mismatch_cap, true);
    num("DW_TEST_TRACE_ROWS", w.trace_rows, true);
    num("DW_TEST_FRAME_RING", w.frame_ring, true);
    if (test_hook("DW_TEST_FORCE_RESCAN")) { w.force_rescan = true; note("DW_TEST_FORCE_RESCAN", nullptr); }
    if (const char* e = test_hook("DW_TEST_FIRST_SLACK")) { w.first_slack = std::atof(e); note("DW_TEST_FIRST_SLACK", e); }
    if (const char* e = std::getenv("DW_KERNEL")) { snprintf(w.kernel, sizeof(w.kernel), "%s", e); note("DW_KERNEL", e); }
    return w;
}

// ---- per-world constants (dw_step_n_trace_ensemble) ----------------------------------------------------------------
// A world of an ensemble call carries the twelve physics members of dw_params itself (dw_world_params).  Everything
// below - make_f64, derive_f32, derive_f32_pair, derive_first_bound - takes a dw_params: a world's constants are derived
// from the handle's params with those members replaced, by the same functions and nothing else.
inline dw_params with_world_params(dw_params p, const dw_world_params& w) {
    p.p = w.p; p.g = w.g; p.S = w.S; p.sigma = w.sigma; p.gamma = w.gamma; p.q = w.q; p.q2 = w.q2; p.dt = w.dt;
    p.albedo_bare = w.albedo_bare; p.albedo_light = w.albedo_light; p.albedo_dark = w.albedo_dark;
    p.temp_optimal = w.temp_optimal;
    return p;
}
inline dw_world_params world_params_of(const dw_params& p) {
    return dw_world_params{p.p, p.g, p.S, p.sigma, p.gamma, p.q, p.q2, p.dt, p.albedo_bare, p.albedo_light, p.albedo_dark,
                           p.temp_optimal};
}
// a_dark - a_bare == -(a_light - a_bare) exactly: the two-term coefficient chain (growth_t<.., SYM>) applies
inline bool albedo_symmetric(double bare, double light, double dark) { return (dark - bare) == -(light - bare); }
// ... for a whole call: the kernels are instantiated once per launch, so SYM holds only if EVERY world's set is symmetric
// (both instantiations give the same values; SYM = false costs instructions, never results)
inline bool worlds_symmetric(const dw_world_params* worlds, size_t B) {
    for (size_t b = 0; b < B; ++b)
        if (!albedo_symmetric(worlds[b].albedo_bare, worlds[b].albedo_light, worlds[b].albedo_dark)) return false;
    return true;
}

// ---- constants: float64 set and the per-step float32 set -----------------------------------------------------------
inline PhysF64 make_f64(const dw_params& p, double L) {
    PhysF64 P;
    P.p = p.p; P.g = p.g; P.S = p.S; P.sigma = p.sigma; P.gamma = p.gamma; P.q = p.q; P.q2 = p.q2;
    P.dt = p.dt; P.ab = p.albedo_bare; P.al = p.albedo_light; P.ad = p.albedo_dark;
    P.To = p.temp_optimal; P.L = L;
    // ref daisy_world_rl.py:270-273: ones*e^-1, centre 1, corners e^-2, normalised
    const double e1 = std::exp(-1.0), e2 = std::exp(-2.0);
    const double s = 1.0 + 4.0 * e1 + 4.0 * e2;
    P.w0 = 1.0 / s; P.w1 = e1 / s; P.w2 = e2 / s;
    return P;
}

// kbeta = 1 / sqrt(g To^2) in float64 (dw_physics.hpp); g = 0 (beta = 1 everywhere): a denominator so large that w^2
// vanishes.  g < 0 is refused for the float32 modes by check_params.
inline double cbeta_host(const dw_params& p) {
    const double cbeta = p.g * p.temp_optimal * p.temp_optimal;
    return cbeta > 1e-30 ? 1.0 / std::sqrt(cbeta) : 0x1p60;
}

inline void split_hi_lo(double v, double scale, float* hi, float* lo) {
    const double h = std::nearbyint(v * scale) / scale;
    *hi = (float)h;
    *lo = (float)(v - h);
}

inline float round_up(double v) {                             // never round a bound DOWN
    const float f = (float)v;
    return (double)f < v ? std::nextafterf(f, INFINITY) : f;
}

// The constants of e_x = c0x + a1*Sl8 + a2*Sd8 + a3*li + a4*di (x = light, dark; dw_physics.hpp) in float64
struct EConst { double c0l, c0d; };
inline EConst e_const(const dw_params& p, double L) {
    const double To4 = std::pow(p.temp_optimal, 4), K = p.S * L / p.sigma;
    const double e0 = K * (1.0 - p.albedo_bare * p.p) / To4 - 1.0;
    return EConst{e0 + p.q2 * (p.albedo_bare * p.p - p.albedo_light) / To4,
                  e0 + p.q2 * (p.albedo_bare * p.p - p.albedo_dark) / To4};
}

// What the two tie bounds below share: the admissible interval of e over all states with covers in [0, kmax], and
// the relative error `ew` of w.  Round-3 derivation (every step numbered there).  With
// v = 1 + e, s = sqrt(v), y = sqrt(s), D = kbeta (y+1)(s+1), w = e/D, om = w^2, the hardware's sqrt / rcp at 1 ulp
// (relative 2u) and every other operation correctly rounded (relative u):
//   rel(v)  <= u (1 + re) + de/vmin =: ev                 re = max |e| / (1 + e)
//   rel(D)  <= 3u + (ev/2 + 2u) sg + (ev/4 + 3u) et       sg = max s/(s+1), et = max y/(y+1)
//   rel(w)  <= 4u + rel(D) + de/|e| = ew + de/|e|
// a1 .. a4: the coefficients of e with their signs (light and dark cover are clipped separately: both may be full in the
// same cell); de: the absolute error of e.
struct TieChain {
    double emin, emax, vlo;       // vlo = max(1 + emin, 0.02)
    bool admissible;              // 1 + emin > 0.02; otherwise: flag every cell (float64 everywhere)
    double ew;
    double kbmax;                 // max |kb| over states with covers in [0, 1]: the two densities sum to [0, 2]
    double pu, safety;            // u |p| unless p is a float; the second-order terms dropped above (~u relative)
};
inline TieChain tie_chain(const dw_params& p, const EConst& c, double a1, double a2, double a3, double a4, double de) {
    const double u = std::ldexp(1.0, -24), kmax = 1000.0;
    TieChain t;
    const double pos = (std::fmax(a1, 0.0) + std::fmax(a2, 0.0)) * 8 * kmax + (std::fmax(a3, 0.0) + std::fmax(a4, 0.0)) * kmax;
    const double neg = (std::fmin(a1, 0.0) + std::fmin(a2, 0.0)) * 8 * kmax + (std::fmin(a3, 0.0) + std::fmin(a4, 0.0)) * kmax;
    t.emax = std::fmax(c.c0l, c.c0d) + pos;
    t.emin = std::fmin(c.c0l, c.c0d) + neg;
    const double vmin = 1.0 + t.emin, vmax = 1.0 + t.emax;
    t.admissible = vmin > 0.02;
    t.vlo = std::fmax(vmin, 0.02);
    const double smax = std::sqrt(std::fmax(vmax, t.vlo));
    const double ymax = std::sqrt(smax);
    const double sg = smax / (smax + 1.0), et = ymax / (ymax + 1.0);
    const double re = std::fmax(std::fabs(t.emin) / t.vlo, std::fabs(t.emax) / std::fmax(vmax, t.vlo));
    const double ev = u * (1.0 + re) + de / t.vlo;
    const double eD = 3.0 * u + (0.5 * ev + 2.0 * u) * sg + (0.25 * ev + 3.0 * u) * et;
    t.ew = 4.0 * u + eD;
    t.kbmax = std::fmax(std::fabs(p.p), std::fabs(p.p - 2.0));
    t.pu = (double)(float)p.p == p.p ? 0.0 : std::fabs(p.p);
    t.safety = 1.0 + 0x1p-7;
    return t;
}

// Derivation of the fused float32 coefficients (see dw_physics.hpp, PhysF32) and of the exact-mode
// tie bound (DESIGN.md §"Exact mode").  All in float64, rounded once.
inline PhysF32 derive_f32(const dw_params& p, double L, int hb_cap = 40) {
    const double To4 = std::pow(p.temp_optimal, 4);
    const double K = p.S * L / p.sigma;
    const double dal = p.albedo_light - p.albedo_bare, dad = p.albedo_dark - p.albedo_bare;
    const double a1 = (p.q - K) * dal / (8000.0 * To4);
    const double a2 = (p.q - K) * dad / (8000.0 * To4);
    const double a3 = (-p.q + p.q2) * dal / (1000.0 * To4);
    const double a4 = (-p.q + p.q2) * dad / (1000.0 * To4);
    const EConst c0 = e_const(p, L);
    const double c0l = c0.c0l, c0d = c0.c0d;
    // hi parts are multiples of 2^-hb with hb chosen so that every partial sum of the hi chain
    // (|.| <= maxsum) stays below 2^(24-hb): exactly representable in float32 for integer inputs.
    const double kmax = 1000.0;                                  // covers are clipped to [0, 1] whatever p is (ref :449)
    const double maxsum = std::fabs(a1) * 8 * kmax + std::fabs(a2) * 8 * kmax + std::fabs(a3) * kmax +
                          std::fabs(a4) * kmax + std::fmax(std::fabs(c0l), std::fabs(c0d));
    int hb = 23 - (int)std::ceil(std::log2(std::fmax(maxsum, 1e-30)));
    if (hb > hb_cap) hb = hb_cap;                               // a coarser split is always admissible
    if (hb < 0) hb = 0;
    const double scale = std::ldexp(1.0, hb);
    PhysF32 P;
    P.hi_bits = hb;
    split_hi_lo(a1, scale, &P.a1h, &P.a1l);
    split_hi_lo(a2, scale, &P.a2h, &P.a2l);
    split_hi_lo(a3, scale, &P.a3h, &P.a3l);
    split_hi_lo(a4, scale, &P.a4h, &P.a4l);
    split_hi_lo(c0l, scale, &P.c0lh, &P.c0ll);
    float c0dl;
    split_hi_lo(c0d, scale, &P.c0dh, &c0dl);
    P.dc0l = c0dl - P.c0ll;                                      // the lo chain carries light's lo constant
    // float32-only mode: every coefficient rounded once (= fl(hi + lo): the sum of two floats is exact in double)
    P.a1 = (float)((double)P.a1h + P.a1l); P.a2 = (float)((double)P.a2h + P.a2l);
    P.a3 = (float)((double)P.a3h + P.a3l); P.a4 = (float)((double)P.a4h + P.a4l);
    P.c0ls = (float)((double)P.c0lh + P.c0ll); P.c0ds = (float)((double)P.c0dh + c0dl);
    const double kbe = cbeta_host(p);                            // kbeta in float64
    P.kbeta = (float)kbe;
    const PhysF64 P64 = make_f64(p, L);
    // dt folded into the density weights (dK = dt * density is what the map needs); the bare fraction then is
    // kb = p - (dKl + dKd) * 0.001 / dt  (dt = 0: no growth at all - weights 0, kb = p)
    P.dw0 = (float)(p.dt * P64.w0); P.dw1 = (float)(p.dt * P64.w1); P.dw2 = (float)(p.dt * P64.w2);
    P.p = (float)p.p; P.ck = p.dt != 0.0 ? (float)(0.001 / p.dt) : 0.f;
    P.ngamma = (float)(-p.gamma);
    // ---- tie bound (per-mille), DESIGN.md "Exact mode":
    //   |gq32 - gq64| <= A0 + eA*|gq| + |dt*K| * (eK0 + eK1*om),   om = 1 - beta >= 0
    const double u = std::ldexp(1.0, -24);
    // absolute error of e: only the lo chain rounds (hi chain exact); lo coefficients <= 2^-(hb+1)
    const double lo_mag = std::ldexp(1.0, -(hb + 1)) * 18.0 * kmax + std::ldexp(1.0, -(hb + 1));
    const double de_abs = 6.0 * u * lo_mag + 1e-9;
    // the float64 coefficients; beyond TieChain's estimates:
    //   |beta^ - beta| <= 2 ew om + u (1 + om) + 2 de max(|e| / D^2)
    //   |kb^ - kb| <= pu + 6u Dt + u |kb|       (kb = p - Dt, Dt = ck S the summed densities: S carries 5u, ck u; pu = u|p|
    //                                             unless p is a float) <= pu + 6u|p| + 7u|kb| [kb < 0]
    //   |f^ - f| <= (pu + 6u|p|)(1 + om) + 7u (|f| + |gamma|) + kbmax (2 ew om + u (1 + om) + Ae) + u |gamma| + u |f|
    //               (|beta^| <= 1 + om; |kb beta| = |f + gamma|)
    //   |gq^ - gq| <= |K| |f^ - f| + 5u |gq|        (K carries 4u, the product u)
    const TieChain t = tie_chain(p, c0, a1, a2, a3, a4, de_abs);
    auto e_over_D2 = [&](double e) {
        const double v = std::fmax(1.0 + e, t.vlo), sv = std::sqrt(v), yv = std::sqrt(sv);
        const double D = kbe * (yv + 1.0) * (sv + 1.0);
        return std::fabs(e) / (D * D);
    };
    const double Ae = 2.0 * de_abs * std::fmax(e_over_D2(t.emin), e_over_D2(t.emax));
    double A0 = t.safety * (kmax * std::fabs(p.dt) * t.kbmax * Ae + 2e-6);   // 2e-6: the float32 arithmetic of the threshold
    if (!t.admissible) A0 = 1.0;                                  // tie_lo < 0: every cell goes to float64
    const double eA = t.safety * 13.0 * u;
    const double eK0d = t.safety * (6.0 * std::fabs(p.p) + t.pu + t.kbmax + 8.0 * std::fabs(p.gamma)) * u;
    const double eK1d = t.safety * ((6.0 * std::fabs(p.p) + t.pu) * u + t.kbmax * (u + 2.0 * t.ew));
    P.tie_lo = (float)(0.5 - A0);
    if ((double)P.tie_lo > 0.5 - A0) P.tie_lo = std::nextafterf(P.tie_lo, -INFINITY);
    P.eA = round_up(eA);
    const float eK0 = round_up(eK0d), eK1 = round_up(eK1d);
    P.eK0s = p.dt < 0.0 ? eK0 : -eK0;
    P.eK1s = p.dt < 0.0 ? eK1 : -eK1;
    P.neK1s = -P.eK1s;                                           // the bracket in beta: (eK0s + eK1s) - eK1s*beta
    P.eK01s = (float)((double)P.eK0s + (double)P.eK1s);
    if (std::fabs((double)P.eK01s) < std::fabs((double)P.eK0s + (double)P.eK1s))     // never round the bound DOWN
        P.eK01s = std::nextafterf(P.eK01s, P.eK01s < 0.f ? -1.f : 1.f);
    return P;
}

// Coefficient sets of the two steps of a fused exact launch, split at the SAME scale (the coarser of
// the two) and with the more conservative of the two tie thresholds: they then differ only in the
// luminosity-dependent members (PhysLumF32).
inline void derive_f32_pair(const dw_params& p, double L1, double L2, PhysF32* P1, PhysF32* P2) {
    const PhysF32 a = derive_f32(p, L1), b = derive_f32(p, L2);
    const int hb = a.hi_bits < b.hi_bits ? a.hi_bits : b.hi_bits;
    *P1 = derive_f32(p, L1, hb);
    *P2 = derive_f32(p, L2, hb);
    const float tie_lo = P1->tie_lo < P2->tie_lo ? P1->tie_lo : P2->tie_lo;
    P1->tie_lo = tie_lo;
    P2->tie_lo = tie_lo;
}

// Error bound of the float32 map on an UN-quantised state (step_generic<In, 3>, dw_step_generic.hpp; the first step of
// an episode in the exact mode).  Same chain of estimates as derive_f32's round-3 bound with: iota = u for a float64
// state (its values are rounded to float32 on the way in; the float64 re-evaluation reads the originals), 0 for a
// float32 state; stencil sums of non-integers round (2u per sum of four, 3u for the sum of eight); the density
// carries 5u + iota; the coefficient chain is the rounded one (no exact hi part): its absolute error is
// (8u + iota) M + u |c0| with the per-cell M the kernel evaluates.
inline FirstStepBound derive_first_bound(const dw_params& p, double L, const PhysF32& P, bool from_f64,
                                         double test_slack = -1.0) {
    const double u = std::ldexp(1.0, -24), iota = from_f64 ? u : 0.0;
    const double kmax = 1000.0;
    const double a1 = std::fabs((double)P.a1), a2 = std::fabs((double)P.a2), a3 = std::fabs((double)P.a3), a4 = std::fabs((double)P.a4);
    const EConst c0 = e_const(p, L);
    const double c0m = std::fmax(std::fabs(c0.c0l), std::fabs(c0.c0d));
    // the rounded coefficients; the worst-case absolute error of e
    const double Mmax = (a1 + a2) * 8 * kmax + (a3 + a4) * kmax;
    const double de_max = (8.0 * u + iota) * Mmax + u * c0m;
    const TieChain t = tie_chain(p, c0, P.a1, P.a2, P.a3, P.a4, de_max);
    const double kbe = cbeta_host(p);
    const double Dmin = kbe * (std::sqrt(std::sqrt(t.vlo)) + 1.0) * (std::sqrt(t.vlo) + 1.0);
    const double kK = 5.0 * u + iota;                             // relative error of a density
    const double safety = t.safety, pu = t.pu, kbmax = t.kbmax;
    FirstStepBound B;
    B.a1 = round_up(a1); B.a2 = round_up(a2); B.a3 = round_up(a3); B.a4 = round_up(a4);
    B.c_de = round_up(safety * (8.0 * u + iota) * (1.0 + 8.0 * u));     // (1 + 8u): M itself is a float32 chain
    B.c_c0 = round_up(safety * u * c0m);
    // |kb^ - kb| <= pu + (kK + 2u)|p| + (kK + 3u)|kb| [kb < 0];  |gq^ - gq| <= |K| |f^ - f| + (kK + u)|gq|
    B.eK0 = round_up(safety * (pu + (kK + 2.0 * u) * std::fabs(p.p) + kbmax * u + ((kK + 3.0 * u) + u) * std::fabs(p.gamma)));
    B.eK1 = round_up(safety * (pu + (kK + 2.0 * u) * std::fabs(p.p) + kbmax * (u + 2.0 * t.ew)));
    B.cW = round_up(safety * 2.0 * kbmax / Dmin);                       // 2 de |e| / D^2 <= 2 de |w| / Dmin
    B.eA = round_up(safety * ((kK + 3.0 * u) + u + (kK + u)));
    B.cS = round_up(safety * u);                                        // the sum k + gq rounds (u |sum|); a float64 k was rounded (u k)
    B.slack = t.admissible ? 4e-6f : 1.0f;                        // the float32 arithmetic of eps itself; inadmissible: all float64
    if (test_slack > (double)B.slack) B.slack = (float)test_slack;   // tests: a wider bracket flags many cells (list sweeps)
    return B;
}

// ---- kernel selection ----------------------------------------------------------------------------------------------
// Which kernels take the steps, and their launch geometry: a pure function of the parameters and the switches
// (plan_steps), computed when a handle is created or its parameters change and committed together with them.
enum StepKind { STEP_GENERIC, STEP_TILED, STEP_STREAM };
struct StepPlan {
    StepKind kind = STEP_GENERIC;     // the step from a quantised state (DW_PRECISION_F64: always generic)
    int halo = 0;                     // wave-strip halo form of the single-step kernels, first step included (halo_form)
    bool packed = false;              // STEP_STREAM with W < 256: several worlds side by side in a wave row
    bool allow_fuse = false;          // STEP_STREAM only: dw_step_n / dw_run_episode fuse pairs of steps ...
    int fused_mode = kFusedOvl;       // ... with this strip layout (packed worlds: kFusedRot)
    bool fmt_planes = false;          // ... whose plain (no STATS, no trace) float32 launches on overlapped strips take the
                                      // format buffer access kernel (step_stream_fused2_fmt_pw)
    bool seam_strips = false;         // ... in the seam-strip layout where that takes fewer waves (seam_layout): the launches
    FusedGeom seam_geom{}, left_geom{};   // of step_stream_fused2_seam_pw and, if columns are left over (left_geom.nstrips
                                      // != 0), of step_stream_fused2_left_pw
    bool row_landing = false;         // ... by the kernels whose input rows land in their window slots
                                      // (step_stream_fused2_land_seam_pw, step_stream_fused2_land_left_pw): same geometry
    bool trace_pairs = false;         // dw_step_n_trace records step pairs (trace_pair_fast / trace_pair_exact: un-packed
                                      // overlapped or rotating strips); otherwise single steps, a copy of B records each
    bool sym_albedo = false;          // a_dark - a_bare == -(a_light - a_bare) exactly: the exact wave-strip kernels use
                                      // the two-term coefficient chain (growth_t<.., SYM>)
    int tcq = 0, rpt = 0;             // STEP_TILED: tile columns (quads) and rows per thread
    Geom geom{};
    size_t tile_lds = 0;
    StripGeom sgeom{};                // STEP_STREAM
    FusedGeom fgeom{};
    int first_prec = 2;               // the first step from an un-quantised state: PREC of step_generic /
                                      // step_first_stream (1 float32, 2 float64, 3 float32 with the tie bound) ...
    bool first_stream = false;        // ... in the wave-strip form (step_first_stream)
    FirstGeom first_geom{};
    bool need_fixq = false;           // exact tiled steps: the global near-tie queues
    bool pw_stream = false;           // dw_step_n_trace_per_world: the wave-strip kernels with per-world constants
                                      // (un-packed strips: a wave works on one world); otherwise step_generic_pw
};

// Halo form of the wave-strip single-step kernels (HALO of step_stream_* and step_first_stream): 0 W == 256 (rotate),
// 1 another multiple of 256, 2 any other W >= 256, 3 packed worlds (W < 256)
inline int halo_form(int W) { return W < 256 ? 3 : (W == 256 ? 0 : (W % 256 == 0 ? 1 : 2)); }

// Rows per wave-strip: 64 (3 % halo re-reads) when `groups` columns of strips then make at least `target` strips; shorter
// strips for smaller jobs - a strip is a serial march of ~0.8 us per row, so with few strips the launch takes as long as
// ONE strip and most SIMDs idle.  Never more than the grid's height.
inline int strip_rows(long groups, int H, long target) {
    int sr = 64;
    while (sr > 8 && groups * ((H + sr - 1) / sr) < target) sr >>= 1;
    return H < sr ? H : sr;
}

// ... unless DW_STRIP_ROWS overrides (experiments, tests): that many rows, at most `cap` and the grid's height
inline int strip_rows_or_override(const Switches& sw, int cap, long groups, int H, long target) {
    if (sw.strip_rows < 1) return strip_rows(groups, H, target);
    const int want = sw.strip_rows < cap ? sw.strip_rows : cap;
    return H < want ? H : want;
}

// The seam-strip layout of a plan with format-access step pairs (un-packed float32 pairs on overlapped strips): whole
// strips of 252 output columns (the two halo columns on either side share ONE lane), and the L = W % 252 columns they leave
// as overlapped strips of L / 4 + 2 lanes, G = 64 / (L / 4 + 2) row bands of a world to a wave.  Taken where it needs fewer
// waves than the overlapped 248-column strips of f (W = 4096, 64 row bands: 64 * 16 + 22 = 1046 against 1088).
inline long seam_waves_per_world(int W, int nrs) {
    const int n_full = W / kSeamCols, L = W - kSeamCols * n_full;
    const int G = L ? 64 / (L / 4 + 2) : 1;
    return (long)nrs * n_full + (L ? (nrs + G - 1) / G : 0);
}
inline bool seam_layout(const FusedGeom& f, FusedGeom* seam, FusedGeom* left) {
    const int n_full = f.W / kSeamCols, L = f.W - kSeamCols * n_full;
    if (n_full < 1 || seam_waves_per_world(f.W, f.nrs) >= (long)f.nrs * f.ncs) return false;
    auto launch = [](FusedGeom& g, long nstrips) {
        g.nstrips = (int)nstrips;
        g.nwg = (g.nstrips + 3) / 4;
        g.chunk = (g.nwg + 7) / 8;
    };
    *seam = f;
    seam->cols_per_strip = kSeamCols;
    seam->ncs = n_full;
    launch(*seam, (long)f.B * f.nrs * n_full);
    *left = *seam;
    left->cols_per_strip = L;
    left->lpw = L ? L / 4 + 2 : 64;
    left->wpr = 64 / left->lpw;
    launch(*left, L ? (long)f.B * ((f.nrs + left->wpr - 1) / left->wpr) : 0);
    return true;
}

inline StepPlan plan_steps(const dw_params& p, const Switches& sw) {
    StepPlan s;
    s.sym_albedo = albedo_symmetric(p.albedo_bare, p.albedo_light, p.albedo_dark) && !sw.no_sym;
    s.halo = halo_form(p.width);
    // Packed mode of the wave-strip kernels: narrow worlds whose width divides 256 sit side by side in one 256-column wave
    // row (256/W worlds per wave) - only for ensembles with enough wave-strips to occupy the GPU: a lone strip is a serial
    // march down 64 rows, ~50 us, where the tiled kernel answers in ~9 us; DW_PACK_MIN_STRIPS overrides for tests.
    // Any width below 256 that is a multiple of 4, provided at least 70 % of the 64 lanes get columns (W = 96: 2 worlds on
    // 48 lanes; W = 132: one world on 33 lanes - left to the tiled kernel).
    const int lpw = p.width / 4, wpr = lpw ? 64 / lpw : 0;
    const bool pack_shape = p.width >= 8 && p.width < 256 && wpr >= 1 && wpr * lpw * 10 >= 64 * 7 && !sw.no_pack;
    const long pack_strips = pack_shape ? (long)((p.batch + wpr - 1) / wpr) * ((p.height + 63) / 64) : 0;
    const bool packable = pack_shape && pack_strips >= (sw.pack_min_strips >= 0 ? sw.pack_min_strips : 512);
    const bool quads = p.precision != DW_PRECISION_F64 && p.width % 4 == 0;
    // the wave-strip kernels take the step: W >= 256 or a packed ensemble, unless DW_KERNEL=tiled (A/B experiments)
    if (quads && (p.width >= 256 || packable) && std::strcmp(sw.kernel, "tiled") != 0) {
        s.kind = STEP_STREAM;
        s.packed = p.width < 256;
        StripGeom& g = s.sgeom;
        g.B = p.batch; g.H = p.height; g.W = p.width;
        g.ncs = (p.width + 255) / 256;
        g.lpw = s.packed ? lpw : 64;
        g.wpr = s.packed ? wpr : 1;
        const long groups = s.packed ? (p.batch + wpr - 1) / wpr : p.batch;
        g.SR = strip_rows_or_override(sw, INT_MAX, groups * g.ncs, p.height, 2048);   // two strips per SIMD
        g.nrs = (p.height + g.SR - 1) / g.SR;
        g.nstrips = (int)(groups * g.nrs * g.ncs);
        g.nwg = (g.nstrips + 3) / 4;
        g.chunk = (g.nwg + 7) / 8;
        g.qcap = kWaveQueueCap;
        int mcap = kMismatchCap;
        if (sw.queue_cap >= 0 && sw.queue_cap < kWaveQueueCap) g.qcap = sw.queue_cap;   // tests: force the overflow fallbacks
        if (sw.mismatch_cap >= 0 && sw.mismatch_cap < kMismatchCap) mcap = sw.mismatch_cap;
        g.force_rescan = sw.force_rescan ? 1 : 0;               // tests: the strip maximum's re-scan path
        s.allow_fuse = !sw.no_fuse;
        // W == 1024: one WORKGROUP per row strip, its four waves side by side (edge columns through LDS) instead of
        // five overlapped 248-column strips (DW_NO_RING: experiments)
        const bool ring = p.width == 1024 && !sw.no_ring;
        s.fused_mode = p.width <= 256 ? kFusedRot : (ring ? kFusedRing : kFusedOvl);
        FusedGeom& f = s.fgeom;
        f.B = p.batch; f.H = p.height; f.W = p.width;
        f.SR = g.SR;
        f.nrs = g.nrs;
        f.lpw = g.lpw; f.wpr = g.wpr;
        f.cols_per_strip = p.width <= 256 ? 256 : (ring ? 1024 : 248);
        f.ncs = s.packed ? 1 : (p.width + f.cols_per_strip - 1) / f.cols_per_strip;
        f.nstrips = (int)(groups * f.nrs * f.ncs);
        f.nwg = ring ? f.nstrips : (f.nstrips + 3) / 4;
        f.chunk = (f.nwg + 7) / 8;
        f.qcap = g.qcap;
        f.mcap = mcap;
        f.sure_need = 9 * p.n_agents + 9 * mcap + 1;            // (dw_step_fused.hpp, STATS)
        s.trace_pairs = s.allow_fuse && !s.packed && s.fused_mode != kFusedRing;
        // (a world's plane is addressed by 32-bit byte offsets there)
        s.fmt_planes = p.precision == DW_PRECISION_FAST && s.allow_fuse && !s.packed && s.fused_mode == kFusedOvl && !sw.no_fmt_planes &&
                       (size_t)p.height * p.width * sizeof(plane_t) < ((size_t)1 << 31);
        s.seam_strips = s.fmt_planes && !sw.no_seam_strips && seam_layout(f, &s.seam_geom, &s.left_geom);
        s.row_landing = s.seam_strips && !sw.no_row_landing;
    } else if (quads && p.width >= 64) {
        s.kind = STEP_TILED;
        const int Wq = p.width / 4;
        if (Wq >= 64) {
            s.tcq = 64; s.rpt = 4;
            if (sw.tile_rpt == 2 || sw.tile_rpt == 4 || sw.tile_rpt == 8) s.rpt = sw.tile_rpt;   // tuning experiments only
        }
        else if (Wq >= 32) { s.tcq = 32; s.rpt = 4; }
        else { s.tcq = 16; s.rpt = 2; }
        const int TR = (256 / s.tcq) * s.rpt;
        Geom& g = s.geom;
        g.B = p.batch; g.H = p.height; g.W = p.width; g.Wq = Wq;
        g.tiles_r = (p.height + TR - 1) / TR;
        g.tiles_c = (Wq + s.tcq - 1) / s.tcq;
        g.ntiles = p.batch * g.tiles_r * g.tiles_c;
        g.chunk = (g.ntiles + 7) / 8;
        g.qcap = kMaxFix;
        if (sw.queue_cap >= 0 && sw.queue_cap < kMaxFix) g.qcap = sw.queue_cap;   // tests: force the overflow fallbacks
        s.tile_lds = (size_t)2 * (TR + 2) * (s.tcq + 2) * 4 * sizeof(float);
    }                                                           // narrow grids and DW_PRECISION_F64: generic kernel
    s.need_fixq = p.precision == DW_PRECISION_EXACT && s.kind == STEP_TILED;
    s.pw_stream = s.kind == STEP_STREAM && !s.packed;
    // The first step from an un-quantised state reads it in its upload format: float32 (fast mode); exact mode: float32
    // with the tie bound for non-integer inputs, float64 only for the flagged cells (DW_FIRST_STEP_F64=1: every cell in
    // float64, as in round 2 - experiments); f64 mode: float64 (bit-identical to the reference's first step).
    s.first_prec = p.precision == DW_PRECISION_FAST ? 1 : (p.precision == DW_PRECISION_EXACT && !sw.first_f64 ? 3 : 2);
    // Every shape the steady-state wave-strip kernels take, and any multiple of 256: the wave-strip form of the same
    // arithmetic (dw_step_first.hpp; ~4x fewer vector instructions per cell).  DW_FIRST_GENERIC=1: the one-thread-per-cell
    // kernel (experiments, tests)
    s.first_stream = (p.width % 256 == 0 || s.kind == STEP_STREAM) && s.first_prec != 2 && !sw.first_generic;
    if (s.first_stream) {
        FirstGeom& fg = s.first_geom;
        fg.B = p.batch; fg.H = p.height; fg.W = p.width;
        fg.lpw = s.packed ? lpw : 64;
        fg.wpr = s.packed ? wpr : 1;
        fg.ncs = s.packed ? 1 : (p.width + 255) / 256;
        const long groups = s.packed ? (p.batch + fg.wpr - 1) / fg.wpr : p.batch;
        // four strips per SIMD; never above the 64 rows FirstGeom::SR allows
        fg.SR = strip_rows_or_override(sw, 64, groups * fg.ncs, p.height, 4096);
        fg.nrs = (p.height + fg.SR - 1) / fg.SR;
        fg.nstrips = (int)(groups * fg.nrs * fg.ncs);
    }
    return s;
}

}  // namespace dw
