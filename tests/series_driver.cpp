// series_driver.cpp — what csrc/dw_series.hpp computes, as one JSON document (tests/test_series_cpu.py).  Host C++17
// only: no HIP header, no device.
//   "world_rows"  per case (the parameter sets of ensemble_driver.cpp): every row WorldRows writes over a run of steps -
//                 single-step sets, float32-only sets, pair sets, first-step bounds - as hexadecimal words ("got") next to
//                 a cache-free derivation done here for that step and world ("want"), and how many derivations it made
//   "schedules"   plan_series over a grid of calls: chunk sizes, pair placement, table rows and chunks; "src": the step
//                 whose luminosities the table row a step reads was built from; "rows_ok": 1 per step whose table row, as
//                 fill_chunk derived it into an image, equals a fresh derivation at the step's own luminosities
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dw_series.hpp"

using namespace dw;

static dw_params base_params(int B) {                           // the values of dw_default_params
    dw_params p;
    std::memset(&p, 0, sizeof(p));
    p.abi_version = DW_ABI_VERSION;
    p.batch = B; p.height = 70; p.width = 320; p.n_agents = 0;
    p.precision = DW_PRECISION_EXACT; p.obs_mask = 0x0BA;
    p.p = 1.0; p.g = 0.003265; p.S = 1000.0; p.sigma = 5.67e-8; p.gamma = 0.25;
    p.q = 0.2 * p.S / p.sigma; p.q2 = p.q / 8.0; p.dt = 1.0;
    p.albedo_bare = 0.5; p.albedo_light = 0.75; p.albedo_dark = 0.25; p.temp_optimal = 295.5;
    p.agent_gamma = 0.05; p.food_chain_penalty = 0.5;
    p.initial_al = 0.2; p.initial_ad = 0.2; p.light_proportion = 0.33; p.dark_proportion = 0.33;
    return p;
}

static std::vector<dw_world_params> parameter_sets(const dw_params& base) {     // as tests/ensemble_driver.cpp
    const dw_world_params own = world_params_of(base);
    std::vector<dw_world_params> worlds{own};
    { dw_world_params w = own; w.q2 = 0.0; worlds.push_back(w); }
    { dw_world_params w = own; w.q2 = own.q / 64.0; worlds.push_back(w); }
    { dw_world_params w = own; w.albedo_light = 0.8; w.albedo_dark = 0.3; w.gamma = 0.3; worlds.push_back(w); }
    { dw_world_params w = own; w.temp_optimal = 290.0; w.dt = 0.5; worlds.push_back(w); }
    { dw_world_params w = own; w.p = 0.7; w.g = 0.004; w.S = 917.0; w.sigma = 5.5e-8; w.q = 0.15 * w.S / w.sigma; w.albedo_bare = 0.45;
      worlds.push_back(w); }
    return worlds;
}

template <class T>
static std::string words(const T& v) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    uint32_t w[sizeof(T) / 4];
    std::memcpy(w, &v, sizeof(T));
    std::string s;
    char buf[12];
    for (size_t i = 0; i < sizeof(T) / 4; ++i) { std::snprintf(buf, sizeof(buf), "%s%08x", i ? " " : "", w[i]); s += buf; }
    return s;
}

struct Pairs { std::vector<std::string> got, want; };
static void print_pairs(const char* key, const Pairs& v, bool last = false) {
    std::printf("    \"%s\": {", key);
    for (int side = 0; side < 2; ++side) {
        const auto& l = side ? v.want : v.got;
        std::printf("\"%s\": [", side ? "want" : "got");
        for (size_t i = 0; i < l.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", l[i].c_str());
        std::printf("]%s", side ? "" : ", ");
    }
    std::printf("}%s\n", last ? "" : ",");
}

// One run of `steps` rows through a WorldRows: world b at Ls[t][b], with the sets `sets` (null: the handle's own)
static void world_rows_case(const char* name, const dw_params& base, const dw_world_params* sets, size_t B, int steps,
                            const std::vector<double>& Ls, bool last) {
    auto fresh = [&](size_t b) { return sets ? with_world_params(base, sets[b]) : base; };
    WorldRows rows(base, sets, B), rows32(base, sets, B, false);
    Pairs f32, f64, only32, pair, fb64, fb32;
    std::vector<PhysF32> r32(B), o32(B);
    std::vector<PhysF64> r64(B);
    std::vector<PairPw> rp(B);
    std::vector<FirstStepBound> fb(B);
    for (int t = 0; t < steps; ++t) {
        const double* L = Ls.data() + (size_t)t * B;
        rows.single(L, r32.data(), r64.data());
        rows32.single(L, o32.data(), nullptr);
        if (t + 1 < steps) rows.pair(L, rp.data());
        for (size_t b = 0; b < B; ++b) {
            const dw_params p = fresh(b);
            f32.got.push_back(words(r32[b])); f32.want.push_back(words(derive_f32(p, L[b])));
            f64.got.push_back(words(r64[b])); f64.want.push_back(words(make_f64(p, L[b])));
            only32.got.push_back(words(o32[b])); only32.want.push_back(words(derive_f32(p, L[b])));
            if (t + 1 < steps) {
                const PairPw w{derive_f32(p, L[b]), derive_f32(p, L[B + b])};
                pair.got.push_back(words(rp[b])); pair.want.push_back(words(w));
            }
        }
        for (int from_f64 = 0; from_f64 < 2; ++from_f64) {     // (the call computes it for its first step only)
            rows.first_bound(L, r32.data(), from_f64 != 0, -1.0, fb.data());
            Pairs& out = from_f64 ? fb64 : fb32;
            for (size_t b = 0; b < B; ++b) {
                out.got.push_back(words(fb[b]));
                out.want.push_back(words(derive_first_bound(fresh(b), L[b], derive_f32(fresh(b), L[b]), from_f64 != 0)));
            }
        }
    }
    std::printf("  \"%s\": {\n    \"B\": %zu, \"steps\": %d, \"derived_singles\": %zu, \"derived_singles_f32_only\": %zu, \"derived_pairs\": %zu,\n",
                name, B, steps, rows.derived_singles, rows32.derived_singles, rows.derived_pairs);
    print_pairs("f32", f32); print_pairs("f64", f64); print_pairs("f32_only", only32); print_pairs("pair", pair);
    print_pairs("first_from_f64", fb64); print_pairs("first_from_f32", fb32, true);
    std::printf("  }%s\n", last ? "" : ",");
}

// the luminosity schedules of the grid: 0 constant, 1 all-distinct, 2 constant for the first five steps then distinct
static std::vector<double> schedule(int kind, int nsteps, size_t B) {
    std::vector<double> Ls((size_t)nsteps * B);
    for (int t = 0; t < nsteps; ++t) {
        const int k = kind == 0 ? 0 : (kind == 1 ? t : (t < 5 ? 0 : t));
        for (size_t b = 0; b < B; ++b) Ls[(size_t)t * B + b] = 0.8 + 0.01 * k + 0.001 * (double)(b % 7);
    }
    return Ls;
}

static void schedule_case(bool& first, const char* form, const SeriesSpec& spec, int kind, const dw_params& base, bool fill) {
    const SeriesSchedule q = plan_series(spec);
    const size_t n = (size_t)spec.nsteps, B = spec.B;
    std::printf("%s  {\"form\": \"%s\", \"nsteps\": %d, \"B\": %zu, \"trace_rows\": %d, \"always_even\": %d, \"may_pair\": %d, "
                "\"quantised\": %d, \"temps\": %d, \"schedule\": %d, \"even\": %d, \"rows\": %zu, \"npairs\": %zu, \"trows\": %zu, \"prows\": %zu, \"is_pair\": [",
                first ? "\n" : ",\n", form, spec.nsteps, B, spec.trace_rows, (int)spec.always_even, (int)spec.may_pair, (int)spec.quantised,
                (int)spec.temps, kind, (int)q.even, q.rows, q.npairs, q.trows, q.prows);
    first = false;
    for (size_t t = 0; t < n; ++t) std::printf("%s%d", t ? ", " : "", (int)q.is_pair[t]);
    std::printf("]");
    if (spec.table_Ls) {
        std::printf(", \"row_of\": [");
        for (size_t t = 0; t < n; ++t) std::printf("%s%zu", t ? ", " : "", q.row_of[t]);
        std::printf("], \"chunks\": [");
        for (size_t c = 0; c < q.chunks.size(); ++c)
            std::printf("%s[%d, %zu, %zu]", c ? ", " : "", q.chunks[c].end, q.chunks[c].singles, q.chunks[c].pairs);
        // what a step finds in its row: the step the row was built for (new_row), and with `fill` the row itself
        std::vector<int> src(n, -1), ok(n, -1);
        const PwLayout lay(B, q.trows, q.prows);
        std::vector<unsigned char> img(fill ? lay.bytes : 0);
        WorldRows rows(base, nullptr, B);
        for (size_t c = 0; c < q.chunks.size(); ++c) {
            std::vector<int> built[2] = {std::vector<int>(q.trows, -1), std::vector<int>(q.prows, -1)};
            if (fill) fill_chunk(q, c, spec.table_Ls, rows, lay, img.data());
            for (int t = c ? q.chunks[c - 1].end : 0; t < q.chunks[c].end; t += q.took(t)) {
                const int k = q.is_pair[(size_t)t];
                if (q.new_row[(size_t)t]) built[k][q.row_of[(size_t)t]] = t;
                src[(size_t)t] = built[k][q.row_of[(size_t)t]];
                if (!fill) continue;
                const double* L = spec.table_Ls + (size_t)t * B;
                ok[(size_t)t] = 1;
                for (size_t b = 0; b < B; ++b) {
                    if (k) {
                        const PairPw w{derive_f32(base, L[b]), derive_f32(base, L[B + b])};
                        ok[(size_t)t] &= std::memcmp(&w, lay.pair(img.data(), q.row_of[(size_t)t]) + b, sizeof(w)) == 0;
                    } else {
                        const PhysF32 w32 = derive_f32(base, L[b]);
                        const PhysF64 w64 = make_f64(base, L[b]);
                        ok[(size_t)t] &= std::memcmp(&w32, lay.p32(img.data(), q.row_of[(size_t)t]) + b, sizeof(w32)) == 0 &&
                                         std::memcmp(&w64, lay.p64(img.data(), q.row_of[(size_t)t]) + b, sizeof(w64)) == 0;
                    }
                }
            }
        }
        std::printf("], \"src\": [");
        for (size_t t = 0; t < n; ++t) std::printf("%s%d", t ? ", " : "", src[t]);
        std::printf("], \"rows_ok\": [");
        for (size_t t = 0; t < n; ++t) std::printf("%s%d", t ? ", " : "", ok[t]);
        std::printf("]");
    }
    std::printf("}");
}

int main() {
    std::printf("{\n\"world_rows\": {\n");
    {
        // a sweep: blocks of worlds with one set each (twins), luminosities that repeat and change, a twin (world 2) whose
        // luminosity differs from its neighbour's, one (world 4) that never changes and one (world 7) that always does
        const dw_params base = base_params(8);
        const std::vector<dw_world_params> s = parameter_sets(base);
        const std::vector<dw_world_params> sets{s[0], s[0], s[0], s[1], s[1], s[3], s[3], s[5]};
        const int steps = 12;
        std::vector<double> Ls((size_t)steps * 8);
        for (int t = 0; t < steps; ++t)
            for (int b = 0; b < 8; ++b) {
                const double L = t < 5 ? 0.8 : 0.8 + 0.01 * (t - 4);
                Ls[(size_t)t * 8 + b] = b == 2 ? L + 0.05 : (b == 4 ? 0.9 : (b == 7 ? 0.7 + 0.02 * t : L));
            }
        world_rows_case("sweep", base, sets.data(), 8, steps, Ls, false);
    }
    {
        const dw_params base = base_params(6);                   // no twins, no luminosity twice
        const std::vector<dw_world_params> sets = parameter_sets(base);
        const int steps = 12;
        std::vector<double> Ls((size_t)steps * 6);
        for (int t = 0; t < steps; ++t)
            for (int b = 0; b < 6; ++b) Ls[(size_t)t * 6 + b] = 0.7 + 0.01 * t + 0.13 * b;
        world_rows_case("distinct", base, sets.data(), 6, steps, Ls, false);
    }
    {
        const dw_params base = base_params(5);                   // without `worlds`: the handle's own set for every world
        world_rows_case("own", base, nullptr, 5, 12, schedule(2, 12, 5), true);
    }
    std::printf("},\n\"schedules\": [");
    bool first = true;
    const int nsteps_grid[] = {1, 2, 3, 4, 5, 7, 8, 11};
    const dw_params base = base_params(3);
    for (int nsteps : nsteps_grid)
        for (int trace_rows = 0; trace_rows <= 4; ++trace_rows)
            for (int may_pair = 0; may_pair < 2; ++may_pair)
                for (int quantised = 0; quantised < 2; ++quantised)
                    for (int temps = 0; temps < 2; ++temps)
                        for (int kind = 0; kind < 3; ++kind) {
                            const std::vector<double> Ls = schedule(kind, nsteps, 3);
                            SeriesSpec s;
                            s.nsteps = nsteps; s.B = 3; s.stats_bytes = sizeof(StatsDev); s.temp_bytes = 32;
                            s.trace_rows = trace_rows; s.quantised = quantised != 0; s.temps = temps != 0;
                            // the per-world table: the ensemble call (it passes "may pair" as its plan has it, also
                            // along with temperature records: the schedule itself takes single steps then)
                            s.may_pair = may_pair != 0;
                            s.table_Ls = Ls.data();
                            schedule_case(first, "table", s, kind, base, true);
                            if (kind) continue;
                            // shared L: dw_step_n_trace (always even chunks), dw_step_n_trace_temperature (single steps)
                            s.table_Ls = nullptr;
                            s.may_pair = may_pair != 0 && !temps; s.always_even = !temps;
                            schedule_case(first, temps ? "shared_temperature" : "shared", s, kind, base, false);
                        }
    // ensembles so large that the byte limits decide: 32 MiB of records, 8 MiB of table rows of each kind
    for (int may_pair = 0; may_pair < 2; ++may_pair)
        for (int temps = 0; temps < 2; ++temps)
            for (int kind = 0; kind < 3; ++kind) {
                const size_t B = 300000;
                const std::vector<double> Ls = schedule(kind, 11, B);
                SeriesSpec s;
                s.nsteps = 11; s.B = B; s.stats_bytes = sizeof(StatsDev); s.temp_bytes = 32;
                s.temps = temps != 0;
                s.may_pair = may_pair != 0;
                s.table_Ls = Ls.data();
                schedule_case(first, "table", s, kind, base, false);
            }
    std::printf("\n]\n}\n");
    return 0;
}
