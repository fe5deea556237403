// dw_temp_moments.hpp — per-world statistics of the local temperature field `temp` (ref daisy_world_rl.py:410,415: the
// curve the reference's notebooks append after every step, daisy/notebook_helpers.py:50-52): mean, population standard
// deviation, minimum and maximum over the H*W cells of each world, in float64 whatever the handle's precision.
//
//   temp_moments_pw<InT, TABLE>   a workgroup reduces kTempChunk consecutive cells of world blockIdx.y into one partial
//   temp_moments_finish_pw        one thread per world combines the world's partials in index order
//
// ("_pw": per world.)  Every cell's temperature is cell_f64's `T` of the cell's 3x3 neighbourhood - the double that
// materialise writes into the `temps` cache; the outputs of cell_f64 that are not read fall to dead-code elimination.
//
// Deterministic by construction: a thread adds its cells in ascending order, the 64 lanes of a wave combine by an xor
// butterfly (both operands of every addition are the same pair of values in every lane), thread 0 adds the four waves in
// index order, the finishing thread adds the chunks in index order.  No atomics.  Nothing in that order depends on the
// number of worlds: world b of a B-world handle reduces exactly as it does alone.
//
// Stable by construction: the sums are taken of d = T - T_ref and d*d, T_ref the temperature of the world's own cell
// (0, 0) - recomputed by every thread, the loads are wave-uniform - so
//   mean = T_ref + sum(d)/n,   var = sum(d*d)/n - (sum(d)/n)^2  (clamped at 0),
// and no digits are lost to mean^2 ~ 9e4 K^2.  A uniform world has d == 0 in every cell: std == 0.0 and
// min == max == mean == T_ref exactly.
#pragma once
#include "dw_common.hpp"
#include "dw_step_per_world.hpp"   // table_entry

namespace dw {

constexpr int kTempChunk = 4096;                                // cells per workgroup: 16 per thread

struct TempPartial {                                            // one chunk of one world
    double sum_d, sum_dd, mn, mx;
    double t_ref;                                               // the world's T_ref (the same value in every chunk)
};

struct TempStatsDev { double mean, std, mn, mx; };              // mirrors dw_temp_stats

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// the temperature of cell (r, c) of one world's planes
template <typename InT>
__device__ __forceinline__ double cell_temperature(const PhysF64& P, const InT* __restrict__ wL, const InT* __restrict__ wD,
                                                   int H, int W, int r, int c) {
    double l9[9], d9[9];
    gather9(wL, H, W, r, c, l9);
    gather9(wD, H, W, r, c, d9);
    return cell_f64(P, l9, d9).T;
}

// grid (chunks, B), 256 threads.  TABLE: the constants of world b are row64[b] (the table dw_step_n_trace_per_world
// uploads for the step), otherwise the by-value set P0.  part: [B][gridDim.x].
template <typename InT, bool TABLE>
__global__ __launch_bounds__(256) void temp_moments_pw(const InT* __restrict__ L, const InT* __restrict__ D, int H, int W,
                                                       PhysF64 P0, const PhysF64* __restrict__ row64,
                                                       TempPartial* __restrict__ part) {
    const int b = blockIdx.y;
    const PhysF64& P = TABLE ? table_entry(row64, b) : P0;
    const int n = H * W;
    const size_t woff = (size_t)b * n;
    const InT* wL = L + woff;
    const InT* wD = D + woff;
    const double t_ref = cell_temperature(P, wL, wD, H, W, 0, 0);
    double s = 0.0, ss = 0.0, mn = t_ref, mx = t_ref;           // (t_ref is a cell of the world: neutral for min / max)
    const int cell0 = blockIdx.x * kTempChunk + threadIdx.x;
    for (int it = 0; it < kTempChunk / 256; ++it) {
        const int cell = cell0 + it * 256;
        if (cell >= n) break;
        const int r = cell / W, c = cell - r * W;
        const double T = cell_temperature(P, wL, wD, H, W, r, c);
        const double d = T - t_ref;
        s += d;
        ss += d * d;
        mn = fmin(mn, T);
        mx = fmax(mx, T);
    }
    s = wave_sum_f64(s);
    ss = wave_sum_f64(ss);
    mn = wave_min_f64(mn);
    mx = wave_max_f64(mx);
    __shared__ double red[4][4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wv] = s; red[1][wv] = ss; red[2][wv] = mn; red[3][wv] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        TempPartial o;
        o.sum_d = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        o.sum_dd = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        o.mn = fmin(fmin(red[2][0], red[2][1]), fmin(red[2][2], red[2][3]));
        o.mx = fmax(fmax(red[3][0], red[3][1]), fmax(red[3][2], red[3][3]));
        o.t_ref = t_ref;
        part[(size_t)b * gridDim.x + blockIdx.x] = o;
    }
}

// one thread per world: the world's `chunks` partials in index order -> out[b]
__global__ __launch_bounds__(64) void temp_moments_finish_pw(const TempPartial* __restrict__ part, int B, int chunks,
                                                             double cells, TempStatsDev* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const TempPartial* p = part + (size_t)b * chunks;
    double s = p[0].sum_d, ss = p[0].sum_dd, mn = p[0].mn, mx = p[0].mx;
    for (int i = 1; i < chunks; ++i) {
        s += p[i].sum_d;
        ss += p[i].sum_dd;
        mn = fmin(mn, p[i].mn);
        mx = fmax(mx, p[i].mx);
    }
    const double md = s / cells;
    const double var = ss / cells - md * md;
    TempStatsDev o;
    o.mean = p[0].t_ref + md;
    o.std = var > 0.0 ? sqrt(var) : 0.0;
    o.mn = mn;
    o.mx = mx;
    out[b] = o;
}

}  // namespace dw
