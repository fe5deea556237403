// episode_temp_staging_driver.cpp — the layouts csrc/dw_episode_staging.hpp computes with and without the temperature
// block of dw_run_episode_trace_temperature, as one JSON document (tests/test_episode_temperature_cpu.py).  Host C++17
// only: no HIP header, no device.  For every (K, B, N) of tests/episode_staging_driver.cpp's grid and each of its forms,
// the layout with EpisodeRegions::temps false and true ("temps_off": where the temperature rows start).
#include <cstdio>

#include "dw_episode_staging.hpp"

using namespace dw;

static const char* kNames[EpisodeStaging::kRegions] = {"member_a", "member_b", "reward", "done", "p32", "ls", "p64", "use_table",
                                                       "table", "world_alive", "agent_ok", "trace", "code", "pair_stats"};

static void print_case(bool& first, const char* form, size_t K, size_t B, size_t N, EpisodeRegions r, bool temps) {
    r.temps = temps;
    const EpisodeStaging S(K, B, N, r);
    std::printf("%s  {\"form\": \"%s\", \"temps\": %d, \"K\": %zu, \"B\": %zu, \"N\": %zu, \"total\": %zu, \"fits_image\": %d, "
                "\"input_end_table\": %zu, \"input_end_no_table\": %zu, \"stats_bytes\": %zu, \"temps_bytes\": %zu, "
                "\"temps_off\": %zu, \"regions\": [",
                first ? "\n" : ",\n", form, (int)temps, K, B, N, S.total, (int)S.fits_image(), S.input_end(true), S.input_end(false),
                S.stats_bytes, S.temps_bytes, S.temps_off());
    first = false;
    for (int i = 0; i < EpisodeStaging::kRegions; ++i)
        std::printf("%s[\"%s\", %zu, %zu]", i ? ", " : "", kNames[i], S.off[i], S.bytes[i]);
    std::printf("]}");
}

static size_t ensemble_rows(size_t K, size_t B) {
    size_t rows = ((size_t)32 << 20) / ((sizeof(PhysF32) + sizeof(double)) * B) / 64 * 64;
    rows = rows < 64 ? 64 : rows;
    return rows > K ? K : rows;
}

int main() {
    const size_t grid[][3] = {{1, 1, 0}, {11, 3, 2}, {64, 6, 2}, {130, 5, 64}, {4096, 3000, 8}};
    std::printf("{\"sizes\": {\"StatsDev\": %zu, \"temp_row\": %zu},\n\"cases\": [", sizeof(StatsDev), EpisodeStaging::kTempRow);
    bool first = true;
    for (const auto& g : grid) {
        const size_t K = g[0], B = g[1], N = g[2];
        for (int temps = 0; temps < 2; ++temps) {
            { EpisodeRegions r; r.rows = K; r.use_table = true; print_case(first, "episode", K, B, N, r, temps); }
            { EpisodeRegions r; r.rows = K; r.use_table = true; r.trace = true; print_case(first, "episode_trace", K, B, N, r, temps); }
            { EpisodeRegions r; r.rows = ensemble_rows(K, B); r.per_world = true; r.use_table = true; print_case(first, "ensemble_wave", K, B, N, r, temps); }
            { EpisodeRegions r; r.pairs = true; r.slack = 256; print_case(first, "stepwise", K, B, N, r, temps); }
            { EpisodeRegions r; r.trace = true; r.slack = 256; print_case(first, "stepwise_trace", K, B, N, r, temps); }
            { EpisodeRegions r; r.slack = 256; print_case(first, "stepwise_ensemble", K, B, N, r, temps); }
            { EpisodeRegions r; r.rows = K; r.mlp = true; print_case(first, "mlp", K, B, N, r, temps); }
        }
    }
    std::printf("\n]}\n");
    return 0;
}
