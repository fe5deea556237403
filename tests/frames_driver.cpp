// frames_driver.cpp — the frame rule of csrc/dw_series.hpp's plan_series, as one JSON document (tests/test_frames_cpu.py).
// Host C++17 only: no HIP header, no device.
//   "frames"    plan_series as dw_step_n_frames calls it (shared luminosity, always even chunks) over
//               nsteps x stride x pairs allowed x quantised start x temperature frames
//   "plain"     the same spec WITHOUT frames for every run length 1..13: what a stretch between frames is held against
//   "defaults"  the shared-luminosity cases of tests/series_driver.cpp's grid, filled member by member as that driver fills
//               them (the new members stay at their defaults)
#include <cstdio>
#include <vector>

#include "dw_series.hpp"

using namespace dw;

static void print_list(const char* key, const std::vector<unsigned char>& v) {
    std::printf(", \"%s\": [", key);
    for (size_t t = 0; t < v.size(); ++t) std::printf("%s%d", t ? ", " : "", (int)v[t]);
    std::printf("]");
}

static SeriesSpec frames_call(int nsteps, bool may_pair, bool quantised) {      // dw_step_n_frames' spec without its frames
    SeriesSpec s;
    s.nsteps = nsteps; s.B = 3; s.stats_bytes = sizeof(StatsDev); s.temp_bytes = 32;
    s.always_even = true; s.may_pair = may_pair; s.quantised = quantised;
    return s;
}

int main() {
    std::printf("{\n\"frames\": [");
    bool first = true;
    const int nsteps_grid[] = {1, 2, 3, 4, 5, 7, 8, 11, 13};
    for (int nsteps : nsteps_grid)
        for (int stride = 1; stride <= 5; ++stride)
            for (int may_pair = 0; may_pair < 2; ++may_pair)
                for (int quantised = 0; quantised < 2; ++quantised)
                    for (int temps = 0; temps < 2; ++temps) {
                        SeriesSpec s = frames_call(nsteps, may_pair != 0, quantised != 0);
                        s.frame_stride = stride; s.frame_temps = temps != 0;
                        const SeriesSchedule q = plan_series(s);
                        std::printf("%s  {\"nsteps\": %d, \"stride\": %d, \"may_pair\": %d, \"quantised\": %d, \"frame_temps\": %d, "
                                    "\"rows\": %zu, \"npairs\": %zu, \"nframes\": %zu, \"plan_frame_temps\": %d",
                                    first ? "\n" : ",\n", nsteps, stride, may_pair, quantised, temps, q.rows, q.npairs, q.nframes,
                                    (int)q.frame_temps);
                        first = false;
                        print_list("is_pair", q.is_pair);
                        print_list("is_frame", q.is_frame);
                        std::printf("}");
                    }
    std::printf("\n],\n\"plain\": [");
    first = true;
    for (int nsteps = 1; nsteps <= 13; ++nsteps)
        for (int may_pair = 0; may_pair < 2; ++may_pair)
            for (int quantised = 0; quantised < 2; ++quantised) {
                const SeriesSchedule q = plan_series(frames_call(nsteps, may_pair != 0, quantised != 0));
                std::printf("%s  {\"nsteps\": %d, \"may_pair\": %d, \"quantised\": %d, \"nframes\": %zu", first ? "\n" : ",\n", nsteps,
                            may_pair, quantised, q.nframes);
                first = false;
                print_list("is_pair", q.is_pair);
                print_list("is_frame", q.is_frame);
                std::printf("}");
            }
    std::printf("\n],\n\"defaults\": [");
    first = true;
    const int series_grid[] = {1, 2, 3, 4, 5, 7, 8, 11};
    for (int nsteps : series_grid)
        for (int trace_rows = 0; trace_rows <= 4; ++trace_rows)
            for (int may_pair = 0; may_pair < 2; ++may_pair)
                for (int quantised = 0; quantised < 2; ++quantised)
                    for (int temps = 0; temps < 2; ++temps) {
                        SeriesSpec s;
                        s.nsteps = nsteps; s.B = 3; s.stats_bytes = sizeof(StatsDev); s.temp_bytes = 32;
                        s.trace_rows = trace_rows; s.quantised = quantised != 0; s.temps = temps != 0;
                        s.may_pair = may_pair != 0 && !temps; s.always_even = !temps;
                        const SeriesSchedule q = plan_series(s);
                        std::printf("%s  {\"form\": \"%s\", \"nsteps\": %d, \"B\": 3, \"trace_rows\": %d, \"always_even\": %d, "
                                    "\"may_pair\": %d, \"quantised\": %d, \"temps\": %d, \"schedule\": 0, \"even\": %d, \"rows\": %zu, "
                                    "\"npairs\": %zu, \"trows\": %zu, \"prows\": %zu, \"nframes\": %zu",
                                    first ? "\n" : ",\n", temps ? "shared_temperature" : "shared", nsteps, trace_rows,
                                    (int)s.always_even, (int)s.may_pair, quantised, temps, (int)q.even, q.rows, q.npairs, q.trows,
                                    q.prows, q.nframes);
                        first = false;
                        print_list("is_pair", q.is_pair);
                        std::printf("}");
                    }
    std::printf("\n]\n}\n");
    return 0;
}
