// dw_step_per_world.hpp — single-step kernels whose constants differ from world to world (dw_step_n_trace_per_world:
// every world of a handle at a luminosity of its own, ref daisy_world_rl.py:405,408 is where L enters the map).
//
// The luminosity enters the coefficient chain (PhysLumF32) and, through the admissible interval of e, the tie bound;
// the float64 repair needs it in double.  So a step's constants are ONE ROW of a device table, [B] entries of
//   PhysF32 (128 B: the world's whole float32 set, tie bound included - exactly what derive_f32 (dw_plan.hpp) gives a one-world
//            handle at that luminosity, so the same cells are flagged and the fix-up counts agree)
//   PhysF64 (128 B: the float64 set of the repair path and of DW_PRECISION_F64)
// and the kernels below are the shared-L kernels' bodies (stream_body, dw_step_generic_body.hpp) handed `row[world]`
// instead of a by-value kernel argument.  In both forms the world is wave-uniform - a wave-strip belongs to one world (un-packed
// geometry), a workgroup of the generic kernel to the world blockIdx.y - and the table is read-only for the launch, so
// the constants arrive by scalar loads and live in SGPRs exactly as kernel arguments do: no extra VGPRs, nothing
// re-loaded in the row loop (tests/test_per_world_cpu.py holds the assembly to that).
#pragma once
#include "dw_step_generic.hpp"
#include "dw_step_stream.hpp"

namespace dw {

// tables are read through the constant address space: a uniform address there is always a scalar load
template <class T> using const_table = const __attribute__((address_space(4))) T*;
template <class T>
__device__ __forceinline__ const T& table_entry(const T* tab, int i) {
    return *(const T*)((const_table<T>)tab + i);
}

// The world of this wave's strip, with stream_body's own strip numbering (XCD-chunked workgroups of four strips); waves
// past the last strip - stream_body sends them home after workgroup 0's have cleared the old reductions - read the last
// strip's entry, so the index is always inside the table.  readfirstlane: the value is uniform, and says so.
// (StripGeom, and the FusedGeom of the un-packed step pairs - dw_step_fused_pw.hpp: fused2_body numbers its strips alike)
template <class StripGeomT>
__device__ __forceinline__ int strip_world(const StripGeomT& G) {
    const int bid = blockIdx.x;
    const int wg = (bid & 7) * G.chunk + (bid >> 3);
    const int s = __builtin_amdgcn_readfirstlane(wg * 4 + ((int)threadIdx.x >> 6));
    return min(s, G.nstrips - 1) / (G.nrs * G.ncs);
}

// HALO 0, 1, 2 only: packed strips hold several worlds in a wave row and go to step_generic_pw
template <int HALO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
void step_stream_fast_pw(const plane_t* __restrict__ inL, const plane_t* __restrict__ inD, plane_t* __restrict__ outL,
                         plane_t* __restrict__ outD, StripGeom G, const PhysF32* __restrict__ row32,
                         const PhysF64* __restrict__ row64, StatsDev* __restrict__ stats,
                         unsigned long long* __restrict__ fixups, unsigned long long* __restrict__ zero_me, int zero_n) {
    static_assert(HALO != 3, "per-world constants: un-packed strips only");
    const int b = strip_world(G);
    stream_body<false, HALO, DW_STREAM_RB_FAST>(inL, inD, outL, outD, G, table_entry(row32, b), table_entry(row64, b), stats,
                                                fixups, zero_me, zero_n);
}

struct StreamExactPwArgs {
    const plane_t* inL; const plane_t* inD; plane_t* outL; plane_t* outD;
    StripGeom G; const PhysF32* row32; const PhysF64* row64; StatsDev* stats; unsigned long long* fixups;
    unsigned long long* zero_me; int zero_n;
};

template <int HALO, bool SYM = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DW_STREAM_WAVES_EXACT, DW_STREAM_WAVES_EXACT)))
void step_stream_exact_pw(StreamExactPwArgs A) {
    static_assert(HALO != 3, "per-world constants: un-packed strips only");
    const int b = strip_world(A.G);
    // the float64 set is cold (the repair code after the row loop reads it where it needs it): only its address is live
    stream_body<true, HALO, DW_STREAM_RB_EXACT, SYM>(A.inL, A.inD, A.outL, A.outD, A.G, table_entry(A.row32, b), A.row64[b],
                                                     A.stats, A.fixups, A.zero_me, A.zero_n);
}

// step_generic with the constants of the workgroup's world: every shape, every input format, float64, the first step
// from an un-quantised state (PREC 3: `rowfb` holds that step's per-world FirstStepBound; otherwise unused, may be null)
template <typename InT, int PREC>
__global__ __launch_bounds__(256) void step_generic_pw(const InT* __restrict__ inL, const InT* __restrict__ inD,
                                                       plane_t* __restrict__ outL, plane_t* __restrict__ outD, int H, int W,
                                                       const PhysF32* __restrict__ row32, const PhysF64* __restrict__ row64,
                                                       const FirstStepBound* __restrict__ rowfb,
                                                       StatsDev* __restrict__ stats, unsigned long long* __restrict__ fixups,
                                                       unsigned long long* __restrict__ zero_me, int zero_n, int cpt) {
    const PhysF32& P = table_entry(row32, (int)blockIdx.y);
    const PhysF64& P64 = table_entry(row64, (int)blockIdx.y);
    const FirstStepBound none{};
    const FirstStepBound& FB = PREC == 3 ? table_entry(rowfb, (int)blockIdx.y) : none;
#include "dw_step_generic_body.hpp"
}

}  // namespace dw
