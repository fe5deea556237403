// dw_series.hpp — what the step-series and ensemble calls decide on the host between their launches, as plain data: the
// constants of every world of a step (WorldRows), where they sit in the per-world table (PwLayout), and which steps a call
// takes as pairs, in which chunks of the series and of the table, from which table row (plan_series).  No HIP call and no
// HIP header: dw_api.hip includes it, and tests/test_series_cpu.py compiles it alone (tests/series_driver.cpp).
#pragma once
#include <cstring>
#include <vector>

#include "dw_plan.hpp"

namespace dw {

// ---- the constants of the worlds of one step -----------------------------------------------------------------------
// World b's constants: from the handle's params with worlds[b]'s members (without `worlds`: the handle's own).  A world
// whose luminosity did not change since its last row keeps its sets (a sweep at fixed L derives B sets, not nsteps * B), a
// world whose set equals world b - 1's (a scenario's block of worlds) takes that world's at the same luminosity.
class WorldRows {
public:
    // f64: rows carry the float64 sets too (not for the wave episode kernel, which takes float32 rows only)
    WorldRows(const dw_params& p, const dw_world_params* worlds, size_t B, bool f64 = true)
        : f64_(f64), wp_(worlds ? B : 1, p), twin_(B, 0), lastL_(B, -1.0), last32_(B), last64_(f64 ? B : 0) {
        for (size_t b = 0; worlds && b < B; ++b) {
            wp_[b] = with_world_params(p, worlds[b]);
            twin_[b] = b > 0 && std::memcmp(&worlds[b], &worlds[b - 1], sizeof(dw_world_params)) == 0;
        }
    }
    size_t worlds() const { return twin_.size(); }
    const dw_params& params(size_t b) const { return wp_[wp_.size() > 1 ? b : 0]; }
    size_t derived_singles = 0, derived_pairs = 0;              // derivations that were not shared (tests)

    // one single-step row at Ls[B]; r64[B] with `f64` only (null without)
    void single(const double* Ls, PhysF32* r32, PhysF64* r64) {
        for (size_t b = 0; b < worlds(); ++b) {
            if (Ls[b] != lastL_[b]) {
                lastL_[b] = Ls[b];
                if (twin_[b] && lastL_[b - 1] == Ls[b]) {
                    last32_[b] = last32_[b - 1];
                    if (f64_) last64_[b] = last64_[b - 1];
                } else {
                    last32_[b] = derive_f32(params(b), Ls[b]);
                    if (f64_) last64_[b] = make_f64(params(b), Ls[b]);
                    ++derived_singles;
                }
            }
            r32[b] = last32_[b];
            if (f64_) r64[b] = last64_[b];
        }
    }
    // one pair row at the luminosities Ls[2][B]: the sets launch_forward_fused2 derives in the float32-only mode
    void pair(const double* Ls, PairPw* row) {
        const size_t B = worlds();
        if (last_pair_.empty()) { last_pair_.resize(B); lastLa_.assign(B, -1.0); lastLb_.assign(B, -1.0); }   // (the first pair)
        for (size_t b = 0; b < B; ++b) {
            if (Ls[b] != lastLa_[b] || Ls[B + b] != lastLb_[b]) {
                lastLa_[b] = Ls[b];
                lastLb_[b] = Ls[B + b];
                if (twin_[b] && lastLa_[b - 1] == Ls[b] && lastLb_[b - 1] == Ls[B + b]) {
                    last_pair_[b] = last_pair_[b - 1];
                } else {
                    last_pair_[b].P1 = derive_f32(params(b), Ls[b]);
                    last_pair_[b].P2 = derive_f32(params(b), Ls[B + b]);
                    ++derived_pairs;
                }
            }
            row[b] = last_pair_[b];
        }
    }
    // the bounds of a first step from an un-quantised state at Ls[B], whose float32 sets are r32[B]
    void first_bound(const double* Ls, const PhysF32* r32, bool from_f64, double test_slack, FirstStepBound* fb) const {
        for (size_t b = 0; b < worlds(); ++b)
            fb[b] = twin_[b] && Ls[b] == Ls[b - 1] ? fb[b - 1] : derive_first_bound(params(b), Ls[b], r32[b], from_f64, test_slack);
    }

private:
    bool f64_;
    std::vector<dw_params> wp_;
    std::vector<unsigned char> twin_;
    std::vector<double> lastL_, lastLa_, lastLb_;               // the luminosity world b's sets were derived at; its pair's two
    std::vector<PhysF32> last32_;
    std::vector<PhysF64> last64_;
    std::vector<PairPw> last_pair_;
};

// ---- the per-world table -------------------------------------------------------------------------------------------
// The constants of a chunk of steps: [rows][B] PhysF32 | [rows][B] PhysF64 | [B] FirstStepBound (the first step of a
// call from an un-quantised state in the exact mode; otherwise unused) | [prows][B] PairPw (the step pairs of
// dw_step_n_trace_ensemble, dw_step_fused_pw.hpp; otherwise none).  One device buffer, one page-locked image, one
// upload per part and chunk; a launch gets the addresses of its row.
struct PwLayout {
    size_t B, rows, prows, o64, ofb, opair, bytes;
    PwLayout(size_t B_, size_t rows_, size_t prows_ = 0) : B(B_), rows(rows_), prows(prows_) {
        o64 = sizeof(PhysF32) * rows * B;
        ofb = o64 + sizeof(PhysF64) * rows * B;
        opair = ofb + sizeof(FirstStepBound) * B;
        bytes = opair + sizeof(PairPw) * prows * B;
    }
    // row `row` of each part of the table that starts at `base` (the device buffer or its host image)
    PhysF32* p32(unsigned char* base, size_t row) const { return reinterpret_cast<PhysF32*>(base) + row * B; }
    PhysF64* p64(unsigned char* base, size_t row) const { return reinterpret_cast<PhysF64*>(base + o64) + row * B; }
    FirstStepBound* fb(unsigned char* base) const { return reinterpret_cast<FirstStepBound*>(base + ofb); }
    PairPw* pair(unsigned char* base, size_t row) const { return reinterpret_cast<PairPw*>(base + opair) + row * B; }
};

// ---- the schedule of a series --------------------------------------------------------------------------------------
struct SeriesSpec {
    int nsteps = 0;
    size_t B = 0, stats_bytes = 0, temp_bytes = 0;   // worlds; one world's record of each series
    int trace_rows = 0;               // Switches::trace_rows (DW_TEST_TRACE_ROWS; < 1: unset)
    bool always_even = false;         // chunks of the series are laid out for pairs even when the call takes none
    bool may_pair = false;            // the plan and the entry point take step pairs ...
    bool quantised = true;            // ... from a quantised state: the current one is
    bool temps = false;               // temperature records are wanted (reduced in front of every step: single steps only)
    const double* table_Ls = nullptr; // [nsteps][B]: the steps read their constants from the per-world table
    // frames (dw_step_n_frames): step t with (t + 1) % frame_stride == 0 leaves a frame - the tile maps of the state after
    // it and (frame_temps) of the temperature field it computes from the state before it.  < 1: no frames.
    int frame_stride = 0;
    bool frame_temps = false;
    bool is_frame(size_t t) const { return frame_stride >= 1 && (t + 1) % (size_t)frame_stride == 0; }
};

struct SeriesSchedule {
    size_t rows = 0;                          // rows of the series on the device at a time: step t fills row t % rows
    std::vector<unsigned char> is_pair;       // [nsteps] a step pair starts at t
    size_t npairs = 0;
    std::vector<unsigned char> is_frame;      // [nsteps] step t leaves a frame (none without SeriesSpec::frame_stride)
    size_t nframes = 0;
    bool frame_temps = false;                 // ... with the temperature map, reduced in front of the step
    bool even = false;                        // chunks laid out for pairs: an even number of rows, at least two, zeroed
    // the table (table_Ls): capacity in single-step and pair rows, the row step t (or the pair at t) reads, whether it is
    // the first to read it, and the chunks - the steps before `end` have their rows on the device after its upload
    size_t trows = 0, prows = 0;
    std::vector<size_t> row_of;
    std::vector<unsigned char> new_row;
    struct Chunk { int end; size_t singles, pairs; };
    std::vector<Chunk> chunks;
    int took(int t) const { return is_pair[(size_t)t] ? 2 : 1; }
};

inline SeriesSchedule plan_series(const SeriesSpec& s) {
    SeriesSchedule q;
    const size_t n = (size_t)s.nsteps, B = s.B;
    const bool hook = s.trace_rows >= 1;
    auto clamp = [](size_t v, size_t lo, size_t hi) { return v < lo ? lo : (v > hi ? hi : v); };
    const bool pairs = s.may_pair && !s.temps;
    q.even = s.always_even || pairs;
    // the whole run up to 32 MiB of the records that decide (512 steps of 1024 worlds: 12 MiB), longer runs in chunks
    size_t rows = hook ? (size_t)s.trace_rows : ((size_t)32 << 20) / ((s.temps ? s.temp_bytes : s.stats_bytes) * B);
    if (q.even) rows = (rows & ~(size_t)1) < 2 ? 2 : rows & ~(size_t)1;
    q.rows = rows = clamp(rows, 1, n);
    // A pair where dw_step_n would issue one - from a quantised state (a first single step makes it so), never the closing
    // one or two steps (the retained previous state stays the true predecessor) - with both rows in one chunk of the series
    // A frame step is a single launch (its input planes and its output planes are in HBM around it), and the steps
    // between two frames pair as a run of their number would: `end` is the frame step ahead, or the end of the run.
    q.is_pair.assign(n, 0);
    q.is_frame.assign(n, 0);
    q.frame_temps = s.frame_stride >= 1 && s.frame_temps;
    for (size_t t = 0; t < n; ++t) q.nframes += q.is_frame[t] = s.is_frame(t);
    bool quantised = s.quantised;
    for (size_t t = 0, end = 0; t < n;) {
        if (end <= t) for (end = t; end < n && !q.is_frame[end]; ++end) {}
        if (pairs && quantised && end - t >= 3 && t % rows + 2 <= rows) { q.is_pair[t] = 1; ++q.npairs; t += 2; }
        else { quantised = true; t += 1; }
    }
    if (!s.table_Ls) return q;
    // 8 MiB of single-step constants (256 B per step and world) and, with pairs, 8 MiB of theirs (256 B per pair and
    // world); under the test hook as many as trace rows hold
    q.trows = ((size_t)8 << 20) / ((sizeof(PhysF32) + sizeof(PhysF64)) * B);
    if (hook && q.trows > (size_t)s.trace_rows) q.trows = (size_t)s.trace_rows;
    q.trows = clamp(q.trows, 1, n);
    if (q.npairs) {
        q.prows = ((size_t)8 << 20) / (sizeof(PairPw) * B);
        if (hook && q.prows > (size_t)s.trace_rows / 2) q.prows = (size_t)s.trace_rows / 2;
        q.prows = clamp(q.prows, 1, q.npairs);
    }
    // A step whose luminosities all equal those of the step before it of its kind in the chunk shares that step's row (a
    // sweep at fixed luminosities: ONE row of each kind, one upload for the whole run); a chunk is the steps that `trows`
    // distinct single-step rows and `prows` distinct pair rows serve.
    q.row_of.assign(n, 0), q.new_row.assign(n, 0);
    for (size_t t = 0; t < n;) {
        size_t used[2] = {0, 0};                                // rows of each kind: single, pair
        const double* newest[2] = {nullptr, nullptr};           // the steps the newest row of each kind was built for
        while (t < n) {
            const int k = q.is_pair[t];
            const double* Ls = s.table_Ls + t * B;
            if (!newest[k] || std::memcmp(Ls, newest[k], sizeof(double) * (size_t)(k + 1) * B) != 0) {
                if (used[k] == (k ? q.prows : q.trows)) break;
                newest[k] = Ls;
                q.new_row[t] = 1;
                ++used[k];
            }
            q.row_of[t] = used[k] - 1;
            t += (size_t)k + 1;
        }
        q.chunks.push_back({(int)t, used[0], used[1]});
    }
    return q;
}

// The rows of chunk c (the steps from the chunk before it's end to its own), derived into the image of the table
inline void fill_chunk(const SeriesSchedule& q, size_t c, const double* Ls, WorldRows& w, const PwLayout& lay, unsigned char* img) {
    const size_t B = lay.B;
    for (int t = c ? q.chunks[c - 1].end : 0; t < q.chunks[c].end; t += q.took(t)) {
        if (!q.new_row[(size_t)t]) continue;
        const size_t r = q.row_of[(size_t)t];
        if (q.is_pair[(size_t)t]) w.pair(Ls + (size_t)t * B, lay.pair(img, r));
        else w.single(Ls + (size_t)t * B, lay.p32(img, r), lay.p64(img, r));
    }
}

}  // namespace dw
