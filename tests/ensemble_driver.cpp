// ensemble_driver.cpp — what csrc/dw_plan.hpp derives for a world of dw_step_n_trace_ensemble, as one JSON document
// (tests/test_ensemble_params_cpu.py).  Host C++17 only: no HIP header, no device.
//   "cases"  per parameter set and luminosity pair: the words of PhysF64, PhysF32, derive_f32_pair and FirstStepBound
//            derived "via_world" (the handle's params with the world's twelve members, with_world_params) and "direct"
//            (a dw_params assigned member by member here) - one derivation, so the two agree bit for bit
//   "round_trip"  world_params_of(with_world_params(base, w)) == w, as words
//   "sym"    the call-wide decision of worlds_symmetric for tables of worlds
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dw_plan.hpp"

using namespace dw;

static dw_params base_params() {                                // the values of dw_default_params, 3 worlds of 70 x 320
    dw_params p;
    std::memset(&p, 0, sizeof(p));
    p.abi_version = DW_ABI_VERSION;
    p.batch = 3; p.height = 70; p.width = 320; p.n_agents = 0;
    p.precision = DW_PRECISION_EXACT; p.obs_mask = 0x0BA;
    p.p = 1.0; p.g = 0.003265; p.S = 1000.0; p.sigma = 5.67e-8; p.gamma = 0.25;
    p.q = 0.2 * p.S / p.sigma; p.q2 = p.q / 8.0; p.dt = 1.0;
    p.albedo_bare = 0.5; p.albedo_light = 0.75; p.albedo_dark = 0.25; p.temp_optimal = 295.5;
    p.agent_gamma = 0.05; p.food_chain_penalty = 0.5;
    p.initial_al = 0.2; p.initial_ad = 0.2; p.light_proportion = 0.33; p.dark_proportion = 0.33;
    return p;
}

template <class T>
static void print_words(const char* key, const T& v, bool last = false) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    uint32_t w[sizeof(T) / 4];
    std::memcpy(w, &v, sizeof(T));
    std::printf("      \"%s\": \"", key);
    for (size_t i = 0; i < sizeof(T) / 4; ++i) std::printf("%s%08x", i ? " " : "", w[i]);
    std::printf("\"%s", last ? "\n" : ",\n");
}

static void print_derived(const char* key, const dw_params& p, double L1, double L2, bool last) {
    std::printf("    \"%s\": {\n", key);
    const PhysF32 P = derive_f32(p, L1);
    print_words("f64", make_f64(p, L1));
    print_words("f32", P);
    PhysF32 pair[2];
    derive_f32_pair(p, L1, L2, &pair[0], &pair[1]);
    print_words("pair", pair);
    print_words("first_from_f64", derive_first_bound(p, L1, P, true));
    print_words("first_from_f32", derive_first_bound(p, L1, P, false), true);
    std::printf("    }%s\n", last ? "" : ",");
}

int main() {
    const dw_params base = base_params();
    const dw_world_params own = world_params_of(base);
    std::vector<dw_world_params> worlds;
    worlds.push_back(own);
    { dw_world_params w = own; w.q2 = 0.0; worlds.push_back(w); }
    { dw_world_params w = own; w.q2 = own.q / 64.0; worlds.push_back(w); }
    { dw_world_params w = own; w.albedo_light = 0.8; w.albedo_dark = 0.3; w.gamma = 0.3; worlds.push_back(w); }
    { dw_world_params w = own; w.temp_optimal = 290.0; w.dt = 0.5; worlds.push_back(w); }
    { dw_world_params w = own; w.p = 0.7; w.g = 0.004; w.S = 917.0; w.sigma = 5.5e-8; w.q = 0.15 * w.S / w.sigma; w.albedo_bare = 0.45;
      worlds.push_back(w); }
    std::printf("{\n\"cases\": [\n");
    for (size_t i = 0; i < worlds.size(); ++i) {
        const dw_world_params& w = worlds[i];
        dw_params direct = base;                                // member by member, not through with_world_params
        direct.p = w.p; direct.g = w.g; direct.S = w.S; direct.sigma = w.sigma; direct.gamma = w.gamma; direct.q = w.q;
        direct.q2 = w.q2; direct.dt = w.dt; direct.albedo_bare = w.albedo_bare; direct.albedo_light = w.albedo_light;
        direct.albedo_dark = w.albedo_dark; direct.temp_optimal = w.temp_optimal;
        const dw_params via = with_world_params(base, w);
        const double L1 = 0.7 + 0.15 * (double)i, L2 = L1 + 0.75 / 512;
        std::printf("  {\n");
        print_derived("via_world", via, L1, L2, false);
        print_derived("direct", direct, L1, L2, false);
        std::printf("    \"round_trip\": {\n");
        print_words("in", w);
        print_words("out", world_params_of(via), true);
        std::printf("    },\n    \"shape_kept\": %d\n  }%s\n",
                    (int)(via.batch == base.batch && via.height == base.height && via.width == base.width &&
                          via.precision == base.precision && via.agent_gamma == base.agent_gamma),
                    i + 1 < worlds.size() ? "," : "");
    }
    std::printf("],\n");
    // the call-wide SYM decision: worlds 0, 1, 2, 4 are symmetric, 3 and 5 are not
    const std::vector<dw_world_params> symmetric = {worlds[0], worlds[1], worlds[2], worlds[4]};
    std::vector<dw_world_params> one_off = symmetric;
    one_off.push_back(worlds[3]);
    std::vector<dw_world_params> first_off = {worlds[5], worlds[0], worlds[1]};
    std::printf("\"sym\": {\"all_symmetric\": %d, \"last_asymmetric\": %d, \"first_asymmetric\": %d, \"single_asymmetric\": %d, "
                "\"plan_own\": %d}\n}\n",
                (int)worlds_symmetric(symmetric.data(), symmetric.size()), (int)worlds_symmetric(one_off.data(), one_off.size()),
                (int)worlds_symmetric(first_off.data(), first_off.size()), (int)worlds_symmetric(&worlds[3], 1),
                (int)plan_steps(base, Switches{}).sym_albedo);
    return 0;
}
