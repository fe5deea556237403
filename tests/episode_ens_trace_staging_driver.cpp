// episode_ens_trace_staging_driver.cpp — the layouts csrc/dw_episode_staging.hpp computes for dw_run_episode_ensemble_trace
// (per-world rows AND records), as one JSON document (tests/test_episode_ensemble_trace_cpu.py).  Host C++17 only: no HIP
// header, no device.  Per (K, B, N): the wave form of dw_run_episode_ensemble ("flags"), with the cover records ("trace")
// and with the temperature rows behind them ("temps"); "image_inputs_only" is what the page-locked image holds of a call
// beyond fits_image(): everything in front of WORLD_ALIVE.
#include <cstdio>

#include "dw_episode_staging.hpp"

using namespace dw;

static const char* kNames[EpisodeStaging::kRegions] = {"member_a", "member_b", "reward", "done", "p32", "ls", "p64", "use_table",
                                                       "table", "world_alive", "agent_ok", "trace", "code", "pair_stats"};

static size_t ensemble_rows(size_t K, size_t B) {
    size_t rows = ((size_t)32 << 20) / ((sizeof(PhysF32) + sizeof(double)) * B) / 64 * 64;
    rows = rows < 64 ? 64 : rows;
    return rows > K ? K : rows;
}

static void print_case(bool& first, const char* form, size_t K, size_t B, size_t N, bool trace, bool temps) {
    EpisodeRegions r;
    r.rows = ensemble_rows(K, B); r.per_world = true; r.use_table = true; r.trace = trace; r.temps = temps;
    const EpisodeStaging S(K, B, N, r);
    std::printf("%s  {\"form\": \"%s\", \"K\": %zu, \"B\": %zu, \"N\": %zu, \"rows\": %zu, \"total\": %zu, \"fits_image\": %d, "
                "\"input_end_table\": %zu, \"image_inputs_only\": %zu, \"stats_bytes\": %zu, \"temps_bytes\": %zu, \"temps_off\": %zu, "
                "\"regions\": [",
                first ? "\n" : ",\n", form, K, B, N, r.rows, S.total, (int)S.fits_image(), S.input_end(true),
                S.off[EpisodeStaging::WORLD_ALIVE], S.stats_bytes, S.temps_bytes, S.temps_off());
    first = false;
    for (int i = 0; i < EpisodeStaging::kRegions; ++i)
        std::printf("%s[\"%s\", %zu, %zu]", i ? ", " : "", kNames[i], S.off[i], S.bytes[i]);
    std::printf("]}");
}

int main() {
    const size_t grid[][3] = {{1, 1, 0}, {70, 6, 4}, {70, 2000, 2}, {64, 1000, 4}, {4096, 1000, 4}};
    std::printf("{\"sizes\": {\"StatsDev\": %zu, \"temp_row\": %zu, \"PhysF32\": %zu, \"PhysF64\": %zu},\n\"cases\": [", sizeof(StatsDev),
                EpisodeStaging::kTempRow, sizeof(PhysF32), sizeof(PhysF64));
    bool first = true;
    for (const auto& g : grid) {
        print_case(first, "flags", g[0], g[1], g[2], false, false);
        print_case(first, "trace", g[0], g[1], g[2], true, false);
        print_case(first, "temps", g[0], g[1], g[2], true, true);
    }
    std::printf("\n]}\n");
    return 0;
}
