// dw_step_generic.hpp — step_generic: one thread per cell, any grid shape, float64 or float32 arithmetic: the
// in-library reference, the first step from an un-quantised state (InT = double / float), odd shapes.
// Input: any plane format (dw_common.hpp); output: always the canonical binary16 planes.
#pragma once
#include "dw_common.hpp"
#include "dw_types.hpp"    // FirstStepBound

namespace dw {

// ---------------------------------------------------------------------------------------------
// step_generic: grid = (ceil(H*W/(256*cpt)), B), block = 256; a thread evaluates `cpt` cells (256 apart) and the
// wave issues ONE set of reduction atomics for all of them: with one set per 64 cells the first step of the
// north-star shape (2.7e8 waves x 3 atomics on 1024 x 3 addresses) took 0.65 s in either arithmetic.
// generic_cells_per_thread() picks cpt so that the launch still has a few thousand workgroups.
// PREC: 0 exact (quantised input), 1 fast, 2 f64, 3 exact from an UN-quantised input (the first step of an episode):
// float32 with a tie bound for non-integer inputs (FirstStepBound), the flagged cells of a workgroup collected in
// LDS and re-evaluated in float64 from the original inputs by densely packed lanes after the cell loop.
// ---------------------------------------------------------------------------------------------
// Error bound of the float32 map on NON-INTEGER inputs (no exact coefficient chain: every operation rounds).
// Derived like the bound of the quantised case (dw_plan.hpp derive_f32) with these changes: the
// inputs carry iota (u for a float64 state converted to float32, 0 for a float32 state), stencil sums 2u-3u, the
// density 5u + iota, and the absolute error of e is (8u + iota) * M + u |c0| with the per-cell magnitude
// M = |a1| Sl8 + |a2| Sd8 + |a3| li + |a4| di, which enters the growth curve as 2 de |e| / D^2 <= 2 de |w| / Dmin:
//   eps = |K| (eK0 + eK1 om + cW de |w|) + eA |gq| + cS (|k + gq| + k) + slack
constexpr int kFirstListCap = 1024;   // flagged cells per workgroup held in LDS (overflow: evaluated in line)

__host__ inline int generic_cells_per_thread(long long batch, long long cells_per_world) {
    long long cpt = batch * cells_per_world / (256LL * 8192);          // big jobs: still >= 8192 workgroups
    const long long few = cells_per_world / (256LL * 512);              // any job: <= 512 atomic sets per world
    cpt = cpt > few ? cpt : few;
    return (int)(cpt < 1 ? 1 : (cpt > 32 ? 32 : cpt));                   // <= 32: float partial sums stay exact
}

template <typename InT, int PREC>
__global__ __launch_bounds__(256) void step_generic(const InT* __restrict__ inL,
                                                    const InT* __restrict__ inD,
                                                    plane_t* __restrict__ outL,
                                                    plane_t* __restrict__ outD, int H, int W,
                                                    PhysF32 P, PhysF64 P64,
                                                    StatsDev* __restrict__ stats,
                                                    unsigned long long* __restrict__ fixups,
                                                    unsigned long long* __restrict__ zero_me,
                                                    int zero_n, int cpt = 1, FirstStepBound FB = FirstStepBound{}) {
#include "dw_step_generic_body.hpp"
}

}  // namespace dw
