// episode_staging_driver.cpp — the layouts csrc/dw_episode_staging.hpp computes, as one JSON document
// (tests/test_episode_staging_cpu.py).  Host C++17 only: no HIP header, no device.
// For every (K, B, N) of the grid, the layout of each kind of call - "form", and which dw_api.hip function builds it:
//   "episode"           run_episode_impl: P32 | Ls rows of all K steps, use_table
//   "episode_trace"     ... with the records
//   "ensemble_wave"     dw_run_episode_ensemble, one wave per world: `rows` steps of [B] rows, P64 [B], use_table
//   "stepwise"          run_episode_stepwise without extras: the pair regions, 256 bytes of slack
//   "stepwise_trace"    ... with the records (no pair regions)
//   "stepwise_ensemble" ... with per-world rows (neither)
//   "mlp"               dw_run_episode_mlp
#include <cstdio>

#include "dw_episode_staging.hpp"

using namespace dw;

static const char* kNames[EpisodeStaging::kRegions] = {"member_a", "member_b", "reward", "done", "p32", "ls", "p64", "use_table",
                                                       "table", "world_alive", "agent_ok", "trace", "code", "pair_stats"};

static void print_case(bool& first, const char* form, size_t K, size_t B, size_t N, const EpisodeRegions& r) {
    const EpisodeStaging S(K, B, N, r);
    std::printf("%s  {\"form\": \"%s\", \"K\": %zu, \"B\": %zu, \"N\": %zu, \"rows\": %zu, \"total\": %zu, \"fits_image\": %d, "
                "\"input_end_table\": %zu, \"input_end_no_table\": %zu, \"regions\": [",
                first ? "\n" : ",\n", form, K, B, N, r.rows, S.total, (int)S.fits_image(), S.input_end(true), S.input_end(false));
    first = false;
    for (int i = 0; i < EpisodeStaging::kRegions; ++i)
        std::printf("%s[\"%s\", %zu, %zu]", i ? ", " : "", kNames[i], S.off[i], S.bytes[i]);
    std::printf("]}");
}

// the steps per launch of the ensemble's wave path (dw_run_episode_ensemble): 32 MiB of rows, whole 64-step segments
static size_t ensemble_rows(size_t K, size_t B) {
    size_t rows = ((size_t)32 << 20) / ((sizeof(PhysF32) + sizeof(double)) * B) / 64 * 64;
    rows = rows < 64 ? 64 : rows;
    return rows > K ? K : rows;
}

int main() {
    // the last case passes the 64 MiB of a page-locked image in every form with a table
    const size_t grid[][3] = {{1, 1, 0}, {11, 3, 2}, {64, 6, 2}, {130, 5, 64}, {4096, 3000, 8}};
    std::printf("{\"sizes\": {\"PhysF32\": %zu, \"PhysF64\": %zu, \"StatsDev\": %zu},\n\"cases\": [", sizeof(PhysF32), sizeof(PhysF64),
                sizeof(StatsDev));
    bool first = true;
    for (const auto& g : grid) {
        const size_t K = g[0], B = g[1], N = g[2];
        { EpisodeRegions r; r.rows = K; r.use_table = true; print_case(first, "episode", K, B, N, r); }
        { EpisodeRegions r; r.rows = K; r.use_table = true; r.trace = true; print_case(first, "episode_trace", K, B, N, r); }
        { EpisodeRegions r; r.rows = ensemble_rows(K, B); r.per_world = true; r.use_table = true; print_case(first, "ensemble_wave", K, B, N, r); }
        { EpisodeRegions r; r.pairs = true; r.slack = 256; print_case(first, "stepwise", K, B, N, r); }
        { EpisodeRegions r; r.trace = true; r.slack = 256; print_case(first, "stepwise_trace", K, B, N, r); }
        { EpisodeRegions r; r.slack = 256; print_case(first, "stepwise_ensemble", K, B, N, r); }
        { EpisodeRegions r; r.rows = K; r.mlp = true; print_case(first, "mlp", K, B, N, r); }
    }
    std::printf("\n]}\n");
    return 0;
}
