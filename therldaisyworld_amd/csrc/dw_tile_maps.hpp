// dw_tile_maps.hpp — spatial frames: per tile of tile_h x tile_w cells of each SELECTED world, the integer sums of the two
// per-mille cover planes and the float64 mean of the local temperature field (the image panels of the reference's figure,
// daisy/notebook_helpers.py `tensor_to_image(env.grid[:, :3])` / `tensor_to_image(env.temp)`).
//
//   tile_cover_pw<VEC>        sums of the two binary16 planes per tile: integers, exact and order-free (global atomics
//                             into records the host zeroed on the stream)
//   tile_temp_pw<InT, MAP>    the mean of cell_f64's `T` (cell_temperature, dw_temp_moments.hpp) per tile, fixed order
//   tile_temp_finish_pw       ... the partials of tiles above kTileChunk cells, in index order
//
// ("_pw": per world.)  World s of a launch is sel[s] (null: s itself): only the selected worlds are read.  Grids are
// (x, selected worlds), in slices of 65 535 worlds; world bases and record offsets are size_t, cell indices int.
//
// The order of the temperature sum depends on (tile_h, tile_w) alone - never on B, the selection or the caller:
//   MAP 0  (<= kTileThreadCells cells)  one thread per tile adds the tile's cells in row-major order; a 1 x 1 tile returns
//                                       the cell's double itself (one term, divided by 1.0)
//   MAP 1  (<= kTileWaveCells cells)    one wave per tile: lane l adds cells l, l + 64, ... ascending (a lane without a
//                                       cell holds 0.0), the lanes combine by wave_sum_f64's xor butterfly
//   MAP 2  (more)                       one workgroup per kTileChunk cells of a tile: thread i adds cells i, i + 256, ...
//                                       ascending, butterfly per wave, thread 0 adds the four waves in index order; a tile
//                                       of one chunk is divided and written at once, otherwise tile_temp_finish_pw adds the
//                                       tile's chunks in index order
// "cell i" of a tile is its i-th cell in row-major order WITHIN the tile.  No atomics on doubles anywhere.
#pragma once
#include "dw_common.hpp"
#include "dw_temp_moments.hpp"    // cell_temperature, wave_sum_f64

namespace dw {

constexpr int kTileThreadCells = 16;
constexpr int kTileWaveCells = 1024;
constexpr int kTileChunk = 4096;                                // cells per workgroup of MAP 2: 16 per thread

struct TileCoverDev { unsigned int sum_light_k, sum_dark_k; };   // mirrors dw_tile_cover

struct TileGeom {
    int H, W, th, tw;             // world and tile shape; th | H, tw | W
    int TH, TW;                   // tiles per world: H / th, W / tw
    int rpt;                      // tile_cover_pw: rows a thread adds, a divisor of th
    int chunks;                   // tile_temp_pw MAP 2: workgroups per tile
};

// ---- cover ----------------------------------------------------------------------------------------------------------
// A thread adds `rpt` rows of VEC consecutive columns (VEC == 8: one 16-byte load per row and plane; W is a multiple of 8
// and tw a multiple or a divisor of 8, so a thread's columns fall into whole tiles) and adds each tile's share to its
// record.  VEC == 1: any shape.  grid ((H / rpt) * (W / VEC) / 256, worlds), rec: [worlds][TH][TW], zeroed.
template <int VEC>
__global__ __launch_bounds__(256) void tile_cover_pw(const plane_t* __restrict__ L, const plane_t* __restrict__ D, TileGeom G,
                                                     const int* __restrict__ sel, int s0, TileCoverDev* __restrict__ rec) {
    const int s = s0 + blockIdx.y;
    const size_t woff = (size_t)(sel ? sel[s] : s) * G.H * G.W;
    const int groups = G.W / VEC;                               // threads per row band
    const int tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= (G.H / G.rpt) * groups) return;
    const int band = tid / groups, c0 = (tid - band * groups) * VEC, r0 = band * G.rpt;
    TileCoverDev* out = rec + ((size_t)s * G.TH + r0 / G.th) * G.TW;
    unsigned int al[VEC], ad[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) al[j] = ad[j] = 0u;
    for (int i = 0; i < G.rpt; ++i) {
        const size_t at = woff + (size_t)(r0 + i) * G.W + c0;
        if constexpr (VEC == 8) {
            typedef _Float16 h8 __attribute__((ext_vector_type(8)));
            const h8 vl = *reinterpret_cast<const h8*>(L + at), vd = *reinterpret_cast<const h8*>(D + at);
#pragma unroll
            for (int j = 0; j < 8; ++j) { al[j] += (unsigned int)(float)vl[j]; ad[j] += (unsigned int)(float)vd[j]; }
        } else {
            al[0] += (unsigned int)(float)L[at];
            ad[0] += (unsigned int)(float)D[at];
        }
    }
    const int span = G.tw < VEC ? G.tw : VEC;                   // columns of one tile among the thread's
    unsigned int sl = 0u, sd = 0u;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        sl += al[j];
        sd += ad[j];
        if ((j + 1) % span == 0) {
            TileCoverDev* o = out + (c0 + j) / G.tw;
            atomicAdd(&o->sum_light_k, sl);
            atomicAdd(&o->sum_dark_k, sd);
            sl = sd = 0u;
        }
    }
}

// ---- temperature ----------------------------------------------------------------------------------------------------
// the temperature of cell i (row-major within the tile) of tile (tr, tc)
template <typename InT>
__device__ __forceinline__ double tile_cell_temperature(const PhysF64& P, const InT* __restrict__ wL, const InT* __restrict__ wD,
                                                        const TileGeom& G, int tr, int tc, int i) {
    const int ir = i / G.tw;
    return cell_temperature(P, wL, wD, G.H, G.W, tr * G.th + ir, tc * G.tw + (i - ir * G.tw));
}

// MAP 0: grid (TH * TW / 256, worlds);  MAP 1: grid (TH * TW / 4, worlds);  MAP 2: grid (TH * TW * chunks, worlds).
// mean: [worlds][TH][TW]; part (MAP 2 with chunks > 1): [worlds][TH * TW][chunks].
template <typename InT, int MAP>
__global__ __launch_bounds__(256) void tile_temp_pw(const InT* __restrict__ L, const InT* __restrict__ D, TileGeom G, PhysF64 P,
                                                    const int* __restrict__ sel, int s0, double* __restrict__ mean,
                                                    double* __restrict__ part) {
    const int s = s0 + blockIdx.y;
    const size_t woff = (size_t)(sel ? sel[s] : s) * G.H * G.W;
    const InT* wL = L + woff;
    const InT* wD = D + woff;
    const int tiles = G.TH * G.TW, n = G.th * G.tw;
    const double cells = (double)n;
    if constexpr (MAP == 0) {
        const int tile = blockIdx.x * 256 + threadIdx.x;
        if (tile >= tiles) return;
        const int tr = tile / G.TW, tc = tile - tr * G.TW;
        double sum = tile_cell_temperature(P, wL, wD, G, tr, tc, 0);
        for (int i = 1; i < n; ++i) sum += tile_cell_temperature(P, wL, wD, G, tr, tc, i);
        mean[(size_t)s * tiles + tile] = sum / cells;
    } else if constexpr (MAP == 1) {
        const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (tile >= tiles) return;                              // (a whole wave: no barrier follows)
        const int tr = tile / G.TW, tc = tile - tr * G.TW;
        double sum = 0.0;
        for (int i = lane; i < n; i += 64) sum += tile_cell_temperature(P, wL, wD, G, tr, tc, i);
        sum = wave_sum_f64(sum);
        if (lane == 0) mean[(size_t)s * tiles + tile] = sum / cells;
    } else {
        const int tile = blockIdx.x / G.chunks, chunk = blockIdx.x - tile * G.chunks;
        const int tr = tile / G.TW, tc = tile - tr * G.TW;
        const int end = (chunk + 1) * kTileChunk < n ? (chunk + 1) * kTileChunk : n;
        double sum = 0.0;
        for (int i = chunk * kTileChunk + threadIdx.x; i < end; i += 256) sum += tile_cell_temperature(P, wL, wD, G, tr, tc, i);
        sum = wave_sum_f64(sum);
        __shared__ double red[4];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double t = ((red[0] + red[1]) + red[2]) + red[3];
            if (G.chunks == 1) mean[(size_t)s * tiles + tile] = t / cells;
            else part[((size_t)s * tiles + tile) * G.chunks + chunk] = t;
        }
    }
}

// one thread per tile of the launch's worlds: the tile's `chunks` partials in index order -> its mean
__global__ __launch_bounds__(256) void tile_temp_finish_pw(const double* __restrict__ part, size_t ntiles, int chunks, double cells,
                                                           double* __restrict__ mean) {
    const size_t tile = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (tile >= ntiles) return;
    const double* p = part + tile * chunks;
    double sum = p[0];
    for (int i = 1; i < chunks; ++i) sum += p[i];
    mean[tile] = sum / cells;
}

}  // namespace dw
