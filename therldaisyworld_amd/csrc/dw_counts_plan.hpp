// dw_counts_plan.hpp — the form dw_run_episode_mlp_counts takes and the LDS its workgroup kernel asks for, as pure
// functions of the shape.  Plain C++ with no HIP header and no HIP call: dw_api.hip and dw_episode_mlp_counts_pw.hpp
// include it, and tests/counts_plan_driver.cpp compiles it alone (tests/test_agent_counts_cpu.py holds it to a Python
// restatement).
//
// episode_mlp_counts_pw keeps, per world, the two ping-pong states as float32 planes, the agents (state, position, action:
// 20 bytes each), a stamp map of one int per cell (the index of the last agent on that cell, -1: none), the reduction
// words and the step's near-tie list; and ONCE PER WORKGROUP, in static LDS, one observation / activation block of 128
// doubles for each of its sixteen 16-lane groups - not one per agent, as episode_mlp does.  A world of 16x16 with 271
// agents is 11 056 bytes (+ a quarter of the 16 KiB of blocks) where episode_mlp_world_bytes asks for 287 536.
#pragma once
#include <cstddef>

namespace dw {

constexpr int kCountsThreads = 256;                            // threads of a workgroup
constexpr int kCountsGroups = kCountsThreads / 16;             // its 16-lane groups: one agent each per policy pass
constexpr int kCountsBlockDoubles = 128;                       // x 64 | h1 16 | h2 32 | logits 16
constexpr size_t kCountsStaticLds = (size_t)kCountsGroups * kCountsBlockDoubles * 8;   // 16 384 bytes, whatever the shape
constexpr int kCountsFixCap = 240;                             // near-tie cells listed per step (kEpFixCap)
constexpr int kCountsMaxCells = 4096;                          // H*W an LDS-resident world may have
constexpr size_t kCountsLdsLimit = (size_t)160 * 1024;         // bytes of LDS a workgroup may hold (gfx950)

// worlds a workgroup holds: 256 / wpb threads per world (worlds_per_block of the other LDS-resident episode kernels)
constexpr int counts_worlds_per_block(int cells) { return cells <= 256 ? 4 : (cells <= 1024 ? 2 : 1); }

// dynamic LDS of one world: planes [2 states][2 species][C] floats | state doubles [N] | positions [N][2] | actions [N] |
// stamp map [C] ints | 8 reduction words | near-tie list
constexpr size_t episode_mlp_counts_world_bytes(int C, int N) {
    return ((size_t)16 * C + (size_t)N * (8 + 8 + 4) + (size_t)4 * C + 32 + 2 * kCountsFixCap + 15) / 16 * 16;
}

// dynamic LDS of a launch, and all the LDS of a workgroup
constexpr size_t episode_mlp_counts_dynamic_lds(int C, int N) {
    return episode_mlp_counts_world_bytes(C, N) * counts_worlds_per_block(C);
}
constexpr size_t episode_mlp_counts_lds_bytes(int C, int N) { return kCountsStaticLds + episode_mlp_counts_dynamic_lds(C, N); }

// true: the workgroup kernel takes the steps once the current and the retained previous state are quantised; false:
// launches per step throughout.  `f64`: DW_PRECISION_F64; `no_episode_kernel`: the DW_NO_EPISODE_KERNEL switch.
constexpr bool episode_mlp_counts_workgroup(int C, int N, bool f64, int collision_mode, bool no_episode_kernel) {
    return C <= kCountsMaxCells && episode_mlp_counts_lds_bytes(C, N) <= kCountsLdsLimit && !f64 && collision_mode == 0 &&
           !no_episode_kernel;
}

}  // namespace dw
