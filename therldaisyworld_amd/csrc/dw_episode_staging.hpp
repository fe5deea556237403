// dw_episode_staging.hpp — where an episode call keeps its inputs and results in the handle's staging buffer, as plain
// data: one layout for dw_run_episode, dw_run_episode_trace, dw_run_episode_ensemble (every form of each) and
// dw_run_episode_mlp.  No HIP call and no HIP header: dw_api.hip includes it, and tests/test_episode_staging_cpu.py
// compiles it alone (tests/episode_staging_driver.cpp).
#pragma once
#include <cstddef>
#include <vector>

#include "dw_plan.hpp"

namespace dw {

// The regions a call may have besides the action table and the flags (an absent one holds zero bytes)
struct EpisodeRegions {
    size_t rows = 0;            // steps whose P32 | Ls rows are on the device at a time (0: none - the launches per step derive their own)
    bool per_world = false;     // the rows are [rows][B], and the worlds' float64 sets P64 [B] follow them
    bool use_table = false;     // use_table [K] on the device (the LDS-resident kernels; the launches per step read the caller's)
    bool trace = false;         // the records of every step, [K][B]
    bool temps = false;         // ... followed by the temperature records of every step, [K][B] rows of 32 bytes (with `trace`)
    bool pairs = false;         // fused step pairs: the uniform action-code bytes [B*N] and the pair statistics [2*B] uint32
    bool mlp = false;           // dw_run_episode_mlp: member maps [B] x 2, reward and done [K][B*N]; no table, no flags
    size_t slack = 0;           // bytes behind the last region
};

// The regions in the order of the enumeration, each at a multiple of 256 bytes: inputs (a staged call uploads ONE prefix
// of the page-locked image), what the device writes (ONE download of WORLD_ALIVE .. TRACE), what only the device uses.
struct EpisodeStaging {
    enum Region { MEMBER_A, MEMBER_B, REWARD, DONE, P32, LS, P64, USE_TABLE, TABLE, WORLD_ALIVE, AGENT_OK, TRACE, CODE, PAIR_STATS, kRegions };
    static constexpr size_t kTempRow = 32;                      // a temperature record: four doubles (dw_temp_stats)
    size_t K, B, bn;
    size_t off[kRegions], bytes[kRegions], total;
    size_t stats_bytes, temps_bytes;                            // the two blocks of TRACE: [K][B] StatsDev | [K][B] temperature rows

    static size_t up(size_t v) { return (v + 255) / 256 * 256; }

    EpisodeStaging(size_t K_, size_t B_, size_t N, const EpisodeRegions& r) : K(K_), B(B_), bn(B_ * N) {
        const size_t per_row = r.per_world ? B : 1, flags = r.mlp ? 0 : 1;
        bytes[MEMBER_A] = bytes[MEMBER_B] = r.mlp ? sizeof(int) * B : 0;
        bytes[REWARD] = r.mlp ? sizeof(double) * K * bn : 0;
        bytes[DONE] = r.mlp ? K * bn : 0;
        bytes[P32] = sizeof(PhysF32) * r.rows * per_row;
        bytes[LS] = sizeof(double) * r.rows * per_row;
        bytes[P64] = r.per_world ? sizeof(PhysF64) * B : 0;
        bytes[USE_TABLE] = r.use_table ? K : 0;
        bytes[TABLE] = flags * K * bn;
        bytes[WORLD_ALIVE] = flags * K * B;
        bytes[AGENT_OK] = flags * K * bn;
        stats_bytes = r.trace ? sizeof(StatsDev) * K * B : 0;
        temps_bytes = r.trace && r.temps ? kTempRow * K * B : 0;
        bytes[TRACE] = stats_bytes + temps_bytes;
        bytes[CODE] = r.pairs ? bn : 0;
        bytes[PAIR_STATS] = r.pairs ? sizeof(unsigned int) * 2 * B : 0;
        size_t o = 0;
        for (int i = 0; i < kRegions; ++i) {
            off[i] = o;
            o = up(o + bytes[i]);
        }
        total = o + r.slack;
    }
    size_t end(Region r) const { return off[r] + bytes[r]; }
    // where the temperature rows start: 8-byte aligned, sizeof(StatsDev) * K * B being a multiple of 8
    size_t temps_off() const { return off[TRACE] + stats_bytes; }
    // the prefix a call's first upload covers: through the action table when the caller gave one, else through use_table
    size_t input_end(bool have_table) const { return have_table ? end(TABLE) : end(USE_TABLE); }
    // a page-locked image of the whole buffer is kept up to 64 MiB; beyond: straight from / to the caller's arrays
    bool fits_image() const { return total <= ((size_t)64 << 20); }
    template <class T>
    T* at(unsigned char* base, Region r) const { return reinterpret_cast<T*>(base + off[r]); }
};

// ---- the launches of an episode call with frames (dw_run_episode_frames, one wave per world) ---------------------------
// Step t of the call leaves a frame when (t + 1) % stride == 0, and at most `ring` frames (>= 1) wait on the device: the
// call is split into launches at whole strides, each of at most `ring` frames, the last one taking the steps behind the
// last frame too.  A launch continues from the planes and agents the one before it wrote back and writes its flags and
// records from row t0 of their blocks on; its frames are f0 .. f0 + frames - 1 of the call, at ring places 0 .. frames - 1.
struct FrameLaunch { size_t t0, steps, f0, frames; };

inline std::vector<FrameLaunch> plan_frame_launches(size_t K, size_t stride, size_t ring) {
    std::vector<FrameLaunch> out;
    const size_t F = K / stride;
    ring = ring < 1 ? 1 : ring;
    size_t t0 = 0, f0 = 0;
    while (F - f0 > ring) {
        out.push_back({t0, ring * stride, f0, ring});
        t0 += ring * stride;
        f0 += ring;
    }
    out.push_back({t0, K - t0, f0, F - f0});
    return out;
}

}  // namespace dw
