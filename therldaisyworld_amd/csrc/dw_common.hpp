// dw_common.hpp — shared device helpers of the RLDaisyWorld kernels (gfx950): per-world reduction record,
// wavefront reductions, input adaptors, and the four-cell row group (`Row4`, `cells4`) that the tiled,
// wave-strip and fused step kernels evaluate with packed float32 arithmetic.
#pragma once
#include <type_traits>

#include "dw_physics.hpp"
#include "dw_types.hpp"    // StatsDev, Geom, plane_t

namespace dw {

// ---------------------------------------------------------------------------------------------
// wave / workgroup reductions (wavefront shuffles, 64 lanes)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------
// Plane formats.
//   plane_t (binary16)  the canonical format of a QUANTISED state: k = 1000 * cover is an integer in [0, 1000]
//                       after any step (np.round(., 3), ref daisy_world_rl.py:452), and binary16 holds every
//                       integer up to 2048 exactly - lossless, 2 bytes per value, 8 bytes of HBM traffic per
//                       cell-update (2 planes read + 2 written).  Every step kernel reads and writes it.
//   float  (per-mille)  an UN-quantised state from dw_init_random / dw_upload_state_f32(quantised = 0)
//   double (natural)    an un-quantised state from dw_upload_state_f64 (the reference's own initial grid)
// The two un-quantised formats exist only until the first step has consumed them (then one step longer as the
// "previous state" observations are derived from); the adaptors below let the cold kernels read all three.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double to_natural(double x) { return x; }
__device__ __forceinline__ double to_natural(float k) { return (double)k / 1000.0; }
// (a binary16 plane holds per-mille INTEGERS: the division-free form is the correctly rounded k / 1000.0, dw_physics.hpp)
__device__ __forceinline__ double to_natural(plane_t k) { return dw_permille_to_natural((double)(float)k); }
__device__ __forceinline__ float to_permille(double x) { return (float)(x * 1000.0); }
__device__ __forceinline__ float to_permille(float k) { return k; }
__device__ __forceinline__ float to_permille(plane_t k) { return (float)k; }

// streaming accesses of four adjacent cells of a binary16 plane (8 bytes).  The new planes are not read again
// within the step, so they are stored non-temporally (measured -1.5 % / -6 % on C2; non-temporal LOADS were
// slower).  One v_cvt_pkrtz_f16_f32 packs two cells (exact whatever its rounding mode: integers <= 1000),
// v_cvt_f32_f16 with an SDWA half-select unpacks one.
typedef _Float16 dw_f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int dw_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ dw_f16x4 stream_load4_raw(const plane_t* p) { return *reinterpret_cast<const dw_f16x4*>(p); }
__device__ __forceinline__ float4 widen4(const dw_f16x4& v) { return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w); }
__device__ __forceinline__ float4 stream_load4(const plane_t* p) { return widen4(stream_load4_raw(p)); }
__device__ __forceinline__ void stream_store4(plane_t* p, const float4& v) {
    dw_u32x2 t;
    t.x = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_pkrtz(v.x, v.y));
    t.y = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_pkrtz(v.z, v.w));
    __builtin_nontemporal_store(t, reinterpret_cast<dw_u32x2*>(p));
}

// ---------------------------------------------------------------------------------------------
// Format buffer accesses of a binary16 plane: the memory path converts binary16 <-> float32 (four cells per access, as
// float32 in the registers) and the row's byte offset travels in a scalar register, so a row access costs the vector
// unit no conversion and no 64-bit address arithmetic.  Exact both ways: the loads widen, and the stored values are
// integers in [0, 1000], which binary16 holds whatever the rounding (0 is no denormal).
// The compiler has no builtin for them; the LLVM intrinsics are declared by their names, so its own s_waitcnt
// insertion tracks them like any other vector memory access.
// ---------------------------------------------------------------------------------------------
typedef float dw_fmt_f32x4 __attribute__((ext_vector_type(4)));
typedef int dw_i32x4 __attribute__((ext_vector_type(4)));
__device__ dw_fmt_f32x4 dw_buf_load_fmt4(dw_i32x4 rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.format.v4f32");
__device__ dw_f32x2 dw_buf_load_fmt2(dw_i32x4 rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.format.v2f32");
__device__ void dw_buf_store_fmt4(dw_fmt_f32x4 v, dw_i32x4 rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.store.format.v4f32");
constexpr int kBufAuxNonTemporal = 2;                           // the `nt` bit of a buffer access (as stream_store4's stores)
// The descriptor of ONE world's plane; `world` and `world_bytes` (H * W * 2 < 2^31) must be wave-uniform.  The base is a
// 64-bit scalar computation (a plane of the whole ensemble exceeds 4 GiB), the offsets within a world fit 32 bits.
//   word 0  base[31:0]       word 1  base[47:32], stride 0 (a raw buffer)       word 2  num_records = world_bytes
//   word 3  dst_sel x/y/z/w = 4/5/6/7 [11:0] | num_format FLOAT (7) [14:12] | data_format 16_16_16_16 (12) [18:15]
// An access whose VECTOR offset leaves the world reads zero / is dropped (the scalar offset takes no part in the
// range check: the callers' rows are wrapped onto the torus before they become one).
// kFmtRsrcPairs: data_format 16_16 (5) instead - an element is TWO cells, for the 2-component loads (fmt_load2x2).
constexpr int kFmtRsrcQuads = 0x00067FAC, kFmtRsrcPairs = 0x0002FFAC;
__device__ __forceinline__ dw_i32x4 fmt_plane_rsrc(const plane_t* plane, int world, unsigned int world_bytes,
                                                   int word3 = kFmtRsrcQuads) {
    const unsigned long long base = (unsigned long long)plane + (unsigned long long)world * world_bytes;
    dw_i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned int)base);
    r.y = __builtin_amdgcn_readfirstlane((int)(unsigned int)(base >> 32)) & 0xffff;
    r.z = __builtin_amdgcn_readfirstlane((int)world_bytes);
    r.w = word3;
    return r;
}
__device__ __forceinline__ float4 fmt_load4(const dw_i32x4& rsrc, int voff, int soff) {
    const dw_fmt_f32x4 v = dw_buf_load_fmt4(rsrc, voff, soff, 0);
    return make_float4(v.x, v.y, v.z, v.w);
}
// four cells as two pairs at byte offsets of their own (a kFmtRsrcPairs descriptor)
__device__ __forceinline__ float4 fmt_load2x2(const dw_i32x4& rsrc, int voff_a, int voff_b, int soff) {
    const dw_f32x2 a = dw_buf_load_fmt2(rsrc, voff_a, soff, 0), c = dw_buf_load_fmt2(rsrc, voff_b, soff, 0);
    return make_float4(a.x, a.y, c.x, c.y);
}
__device__ __forceinline__ void fmt_store4(const dw_i32x4& rsrc, int voff, int soff, const float4& v) {
    dw_buf_store_fmt4(dw_fmt_f32x4{v.x, v.y, v.z, v.w}, rsrc, voff, soff, kBufAuxNonTemporal);
}
// A prefetched row out of the load's registers into its slot of a register window: the window's slots rotate with the
// unrolled loop, the prefetch's registers do not, so the row has to move once - two cells per v_pk_mov_b32 (where the
// binary16 form paid one conversion per cell, which was that move).  Left to the compiler: one v_mov_b32 per cell.
__device__ __forceinline__ float4 widen4(const float4& v) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    unsigned long long lo, hi;                                  // (not float pairs: their sums would be formed as packed adds
    asm("v_pk_mov_b32 %0, %1, %1 op_sel:[0,1]" : "=v"(lo) : "v"(f2{v.x, v.y}));   //  across the window's register pairs)
    asm("v_pk_mov_b32 %0, %1, %1 op_sel:[0,1]" : "=v"(hi) : "v"(f2{v.z, v.w}));
    return make_float4(__uint_as_float((unsigned int)lo), __uint_as_float((unsigned int)(lo >> 32)),
                       __uint_as_float((unsigned int)hi), __uint_as_float((unsigned int)(hi >> 32)));
}

// Rows that land where they stay (fused2_body, LAND): the load names the window slot's own register pairs as its
// destination, so no move follows it.  The compiler cannot see such a load: the caller issues it only behind the last
// read of the slot's old row (a read the compiler placed later would make it copy the old row first) and orders the
// first read of the new row behind a counted wait (fmt_landed), through which the landed values pass as operands.
// Accesses the compiler does not count only make ITS waits stricter: vmcnt retires in issue order.
__device__ __forceinline__ void fmt_land2(dw_f32x2& dst, const dw_i32x4& rsrc, int voff, int soff) {
    asm volatile("buffer_load_format_xy %0, %1, %2, %3 offen" : "+v"(dst) : "v"(voff), "s"(rsrc), "s"(soff));
}
template <int IMM>                                              // (no scalar offset; IMM: the instruction's byte offset)
__device__ __forceinline__ void fmt_land2(dw_f32x2& dst, const dw_i32x4& rsrc, int voff) {
    asm volatile("buffer_load_format_xy %0, %1, %2, 0 offen offset:%3" : "+v"(dst) : "v"(voff), "s"(rsrc), "n"(IMM));
}
// YOUNGER: the vector memory accesses issued behind the landing loads that may still be in flight (the row stores).
// The landed pairs pass as 64-bit integers, as in widen4: typed as float pairs, the two middle pair sums of the row would
// be formed as one packed add and moved apart again.
template <int YOUNGER>
__device__ __forceinline__ void fmt_landed(unsigned long long& a, unsigned long long& b, unsigned long long& c,
                                           unsigned long long& d) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(YOUNGER));
}
__device__ __forceinline__ unsigned long long pair_bits(float lo, float hi) {
    return (unsigned long long)__float_as_uint(lo) | ((unsigned long long)__float_as_uint(hi) << 32);
}
__device__ __forceinline__ float4 pairs_float4(unsigned long long lo, unsigned long long hi) {
    return make_float4(__uint_as_float((unsigned int)lo), __uint_as_float((unsigned int)(lo >> 32)),
                       __uint_as_float((unsigned int)hi), __uint_as_float((unsigned int)(hi >> 32)));
}

// a coordinate at most one period outside [0, n) back onto the torus (agents move by one cell, stencils reach two)
__device__ __forceinline__ int wrap_near(int v, int n) { return v < 0 ? v + n : (v >= n ? v - n : v); }
// ... at most TWO periods outside (a repair reaches four rows beyond a strip of a world that may be only three rows tall)
__device__ __forceinline__ int wrap_near2(int v, int n) { return wrap_near(wrap_near(v, n), n); }

template <typename T>
__device__ __forceinline__ void gather9(const T* __restrict__ plane, int H, int W, int r, int c,
                                        double out[9]) {
    const int ru = r == 0 ? H - 1 : r - 1, rd = r == H - 1 ? 0 : r + 1;
    const int cl = c == 0 ? W - 1 : c - 1, cr = c == W - 1 ? 0 : c + 1;
    const int rows[3] = {ru, r, rd}, cols[3] = {cl, c, cr};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) out[a * 3 + b] = to_natural(plane[(size_t)rows[a] * W + cols[b]]);
}

struct Row4 {                 // 4 centre values of a row and the horizontal pair sums around them
    float x[4];
    float h2[4];              // h2[i] = x[i-1] + x[i+1]
};

__device__ __forceinline__ Row4 load_row(const float* __restrict__ lds_row_group) {
    // lds_row_group points at the float4 group LEFT of the thread's own group
    const float4 a = *reinterpret_cast<const float4*>(lds_row_group);
    const float4 m = *reinterpret_cast<const float4*>(lds_row_group + 4);
    const float4 c = *reinterpret_cast<const float4*>(lds_row_group + 8);
    Row4 r;
    r.x[0] = m.x; r.x[1] = m.y; r.x[2] = m.z; r.x[3] = m.w;
    r.h2[0] = a.w + m.y;
    r.h2[1] = m.x + m.z;
    r.h2[2] = m.y + m.w;
    r.h2[3] = m.z + c.x;
    return r;
}

// The map on the four cells of one row group: (up, mid, down) rows of both planes -> new values (and,
// in the exact mode, the near-tie flags).  Two cells per packed float32 lane pair (dw_physics.hpp).
// `tie`: per-lane bools (bool*), or - the wave-strip kernels - the wave's lane masks (unsigned long long*), which
// stay on the scalar unit from the compare to the queue push.
template <bool EXACT, bool SYM = false, typename F = bool>
__device__ __forceinline__ void cells4(const PhysF32& P, const Row4& upL, const Row4& miL, const Row4& dnL,
                                       const Row4& upD, const Row4& miD, const Row4& dnD, float* ol, float* od,
                                       F* tie) {
#pragma clang fp contract(off)
    using T = dw_f32x2;
    constexpr int N = Lanes<T>::N;
#pragma unroll
    for (int i = 0; i < 4; i += N) {
        auto pr = [&](const float* a) -> T { return Lanes<T>::load(a, i); };
        const T li = pr(miL.x), di = pr(miD.x);
        const T El = pr(miL.h2) + (pr(upL.x) + pr(dnL.x));
        const T Cl = pr(upL.h2) + pr(dnL.h2);
        const T Ed = pr(miD.h2) + (pr(upD.x) + pr(dnD.x));
        const T Cd = pr(upD.h2) + pr(dnD.h2);
        const GrowthT<T> g = growth_t<EXACT || kFastSplit, T, EXACT && SYM>(P, li, di, El, Cl, Ed, Cd);
        T vl, vd;
        if (EXACT) {
            F tl[N], td[N];
            if constexpr (DW_TIE_FROM_BETA || sizeof(F) == 8) {
                vl = finish_exact_beta_t<T, F>(P, li, g.gql, g.dKl, g.bl, tl);
                vd = finish_exact_beta_t<T, F>(P, di, g.gqd, g.dKd, g.bd, td);
            } else {
                vl = finish_exact_t<T>(P, li, g.gql, g.dKl, g.oml, tl);
                vd = finish_exact_t<T>(P, di, g.gqd, g.dKd, g.omd, td);
            }
#pragma unroll
            for (int e = 0; e < N; ++e) tie[i + e] = tl[e] | td[e];
        } else {
            vl = finish_fast_t<T>(li, g.dKl, g.fl);
            vd = finish_fast_t<T>(di, g.dKd, g.fd);
        }
#pragma unroll
        for (int e = 0; e < N; ++e) {
            ol[i + e] = Lanes<T>::get(vl, e);
            od[i + e] = Lanes<T>::get(vd, e);
        }
    }
}

// The float32-only map of cells4 in two parts: up_sums4 forms the four sums per plane that read the UP row (the same
// additions, in cells4's order), cells4_up the rest from them.  Between the two the up row is dead, which is where a
// kernel that lands its next input row in that row's registers issues the load (fused2_body, LAND).
struct UpSums4 { dw_f32x2 xl[2], cl[2], xd[2], cd[2]; };     // up.x + dn.x and up.h2 + dn.h2, light and dark
__device__ __forceinline__ UpSums4 up_sums4(const Row4& upL, const Row4& dnL, const Row4& upD, const Row4& dnD) {
#pragma clang fp contract(off)
    using T = dw_f32x2;
    UpSums4 s;
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
        auto pr = [&](const float* a) -> T { return Lanes<T>::load(a, i); };
        s.xl[i / 2] = pr(upL.x) + pr(dnL.x);
        s.cl[i / 2] = pr(upL.h2) + pr(dnL.h2);
        s.xd[i / 2] = pr(upD.x) + pr(dnD.x);
        s.cd[i / 2] = pr(upD.h2) + pr(dnD.h2);
    }
    return s;
}
__device__ __forceinline__ void cells4_up(const PhysF32& P, const UpSums4& s, const Row4& miL, const Row4& miD, float* ol,
                                          float* od) {
#pragma clang fp contract(off)
    using T = dw_f32x2;
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
        auto pr = [&](const float* a) -> T { return Lanes<T>::load(a, i); };
        const T li = pr(miL.x), di = pr(miD.x);
        const T El = pr(miL.h2) + s.xl[i / 2];
        const T Ed = pr(miD.h2) + s.xd[i / 2];
        const GrowthT<T> g = growth_t<kFastSplit, T, false>(P, li, di, El, s.cl[i / 2], Ed, s.cd[i / 2]);
        const T vl = finish_fast_t<T>(li, g.dKl, g.fl), vd = finish_fast_t<T>(di, g.dKd, g.fd);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            ol[i + e] = Lanes<T>::get(vl, e);
            od[i + e] = Lanes<T>::get(vd, e);
        }
    }
}

}  // namespace dw
