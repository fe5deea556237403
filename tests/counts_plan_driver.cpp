// counts_plan_driver.cpp — prints what csrc/dw_counts_plan.hpp decides for the shapes on the command line (the header alone,
// no HIP): tests/test_agent_counts_cpu.py holds the lines to a Python restatement.
//   counts_plan_driver C N f64 collision_mode no_episode_kernel [C N f64 collision_mode no_episode_kernel ...]
// One line per shape: C N worlds_per_block world_bytes dynamic_lds lds_bytes workgroup
#include <cstdio>
#include <cstdlib>

#include "dw_counts_plan.hpp"

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 1) % 5 != 0) {
        std::fprintf(stderr, "usage: %s C N f64 collision_mode no_episode_kernel ...\n", argv[0]);
        return 2;
    }
    std::printf("static %zu groups %d\n", dw::kCountsStaticLds, dw::kCountsGroups);
    for (int i = 1; i + 4 < argc; i += 5) {
        const int C = std::atoi(argv[i]), N = std::atoi(argv[i + 1]);
        const bool f64 = std::atoi(argv[i + 2]) != 0, nok = std::atoi(argv[i + 4]) != 0;
        const int cm = std::atoi(argv[i + 3]);
        std::printf("%d %d %d %zu %zu %zu %d\n", C, N, dw::counts_worlds_per_block(C), dw::episode_mlp_counts_world_bytes(C, N),
                    dw::episode_mlp_counts_dynamic_lds(C, N), dw::episode_mlp_counts_lds_bytes(C, N),
                    dw::episode_mlp_counts_workgroup(C, N, f64, cm, nok) ? 1 : 0);
    }
    return 0;
}
