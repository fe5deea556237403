// dw_step_fused_pw.hpp — the step pairs of dw_step_n_trace with the constants of each strip's own world
// (dw_step_n_trace_ensemble: a set of physics constants AND a luminosity per world).
//
// A pair's constants are one row of a device table, [B] entries of PairPw: the two float32 sets exactly as
// launch_forward_fused2 derives them for a one-world handle with that world's constants (derive_f32 at each luminosity).
// The kernels are fused2_body's trace form (dw_step_fused.hpp) handed the entry of the strip's world instead of by-value
// kernel arguments: a strip belongs to one world (un-packed overlapped or rotating strips), the index is wave-uniform and
// the table is read through the constant address space, so the constants arrive by scalar loads in front of the row loop
// and live in SGPRs as kernel arguments do (tests/test_ensemble_params_cpu.py holds the assembly to the shared-L kernels'
// registers, occupancy and row-loop instruction count).
// Float32-only mode only.  The exact form (trace_pair_exact with P1, lum_part(P2) and the cold float64 set read from the
// entry) does not keep the shared-L kernel's row loop: that kernel is at its SGPR limit and re-reads kernel arguments
// from the kernarg segment where it runs out, which a table entry does not allow - its constants are parked in VGPR lanes
// instead, 109-136 v_readlane per row-loop iteration against 46-67.  The exact mode takes single steps.
#pragma once
#include "dw_step_fused.hpp"
#include "dw_step_per_world.hpp"

namespace dw {

// The world of this wave's strip (strip_world: fused2_body numbers its un-packed strips as stream_body does), in a scalar
// register (the division by the strips per world runs on the vector unit).
__device__ __forceinline__ int pair_world(const FusedGeom& G) { return __builtin_amdgcn_readfirstlane(strip_world(G)); }

template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DW_TRACE_FAST_WAVES, DW_TRACE_FAST_WAVES)))
void trace_pair_fast_pw(const plane_t* __restrict__ inL, const plane_t* __restrict__ inD, plane_t* __restrict__ outL,
                        plane_t* __restrict__ outD, FusedGeom G, const PairPw* __restrict__ row,
                        unsigned long long* __restrict__ zero_me, int zero_n, StatsDev* __restrict__ trace) {
    static_assert(MODE != kFusedRing, "per-world constants: a wave's strip belongs to one world");
    const PairPw& E = table_entry(row, pair_world(G));
    const PhysF64 dummy{};
    const double zero = 0.0;
    fused2_body<MODE, false, false, false, false, plane_t, plane_t, true>(inL, inD, outL, outD, G, E.P1, E.P2, dummy, zero, zero,
                                                                           zero_me, zero_n, nullptr, 0.f, trace, 0);
}

}  // namespace dw
