// episode_frames_driver.cpp — the launch split of dw_run_episode_frames' one-wave-per-world form (plan_frame_launches,
// csrc/dw_episode_staging.hpp) and the layout of dw_agent_frame, as one JSON document (tests/test_episode_frames_cpu.py).
// Host C++17 only: no HIP header, no device.
//   "record"    sizeof(dw_agent_frame) and the offsets of its members
//   "launches"  plan_frame_launches over K x stride x ring capacity (0 stands for "unlimited": more frames than any call has)
#include <cstddef>
#include <cstdio>

#include "../include/daisyworld_hip.h"
#include "dw_episode_staging.hpp"

using namespace dw;

int main() {
    std::printf("{\n\"record\": {\"size\": %zu, \"row\": %zu, \"col\": %zu, \"state\": %zu},\n\"launches\": [", sizeof(dw_agent_frame),
                offsetof(dw_agent_frame, row), offsetof(dw_agent_frame, col), offsetof(dw_agent_frame, state));
    const size_t Ks[] = {1, 2, 63, 64, 65, 130, 4096}, strides[] = {1, 3, 7, 64, 100}, rings[] = {1, 2, 5, 0};
    bool first = true;
    for (size_t K : Ks)
        for (size_t stride : strides)
            for (size_t ring : rings) {
                std::printf("%s  {\"K\": %zu, \"stride\": %zu, \"ring\": %zu, \"launches\": [", first ? "\n" : ",\n", K, stride, ring);
                first = false;
                bool head = true;
                for (const FrameLaunch& l : plan_frame_launches(K, stride, ring ? ring : (size_t)1 << 40)) {
                    std::printf("%s[%zu, %zu, %zu, %zu]", head ? "" : ", ", l.t0, l.steps, l.f0, l.frames);
                    head = false;
                }
                std::printf("]}");
            }
    std::printf("\n]\n}\n");
    return 0;
}
