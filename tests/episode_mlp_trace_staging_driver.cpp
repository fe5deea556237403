// episode_mlp_trace_staging_driver.cpp — the layouts csrc/dw_episode_staging.hpp computes for dw_run_episode_mlp ("mlp") and
// for dw_run_episode_mlp_trace with the cover records ("trace") and with the temperature rows behind them ("temps"), as one
// JSON document (tests/test_episode_mlp_trace_cpu.py).  Host C++17 only: no HIP header, no device.
#include <cstdio>

#include "dw_episode_staging.hpp"

using namespace dw;

static const char* kNames[EpisodeStaging::kRegions] = {"member_a", "member_b", "reward", "done", "p32", "ls", "p64", "use_table",
                                                       "table", "world_alive", "agent_ok", "trace", "code", "pair_stats"};

static void print_case(bool& first, const char* form, size_t K, size_t B, size_t N, bool trace, bool temps) {
    EpisodeRegions r;
    r.rows = K; r.mlp = true; r.trace = trace; r.temps = temps;
    const EpisodeStaging S(K, B, N, r);
    std::printf("%s  {\"form\": \"%s\", \"K\": %zu, \"B\": %zu, \"N\": %zu, \"total\": %zu, \"stats_bytes\": %zu, \"temps_bytes\": %zu, "
                "\"temps_off\": %zu, \"regions\": [",
                first ? "\n" : ",\n", form, K, B, N, S.total, S.stats_bytes, S.temps_bytes, S.temps_off());
    first = false;
    for (int i = 0; i < EpisodeStaging::kRegions; ++i)
        std::printf("%s[\"%s\", %zu, %zu]", i ? ", " : "", kNames[i], S.off[i], S.bytes[i]);
    std::printf("]}");
}

int main() {
    const size_t grid[][3] = {{1, 1, 1}, {70, 5, 4}, {65, 3, 2}, {64, 2048, 4}, {4096, 1000, 4}};
    std::printf("{\"sizes\": {\"StatsDev\": %zu, \"temp_row\": %zu, \"PhysF32\": %zu},\n\"cases\": [", sizeof(StatsDev),
                EpisodeStaging::kTempRow, sizeof(PhysF32));
    bool first = true;
    for (const auto& g : grid) {
        print_case(first, "mlp", g[0], g[1], g[2], false, false);
        print_case(first, "trace", g[0], g[1], g[2], true, false);
        print_case(first, "temps", g[0], g[1], g[2], true, true);
    }
    std::printf("\n]}\n");
    return 0;
}
