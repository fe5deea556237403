// plan_driver.cpp — prints what csrc/dw_plan.hpp computes, as one JSON document (tests/test_plan_cpu.py holds it
// against tests/golden/plan_constants.json).  Host C++17 only: no HIP header, no device.
//   "plan"       every scalar of StepPlan and of its four geometry structs (names: "plan_fields"), per shape, precision
//                and switch setting
//   "constants"  PhysF64, PhysF32, FirstStepBound (from a float64 and from a float32 state) and derive_f32_pair as the
//                hexadecimal words of the structs, per parameter set and luminosity
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dw_plan.hpp"

using namespace dw;

static dw_params params(int B, int H, int W, int precision) {   // the values of dw_default_params
    dw_params p;
    std::memset(&p, 0, sizeof(p));
    p.abi_version = DW_ABI_VERSION;
    p.batch = B; p.height = H; p.width = W; p.n_agents = 2;
    p.precision = precision; p.obs_mask = 0x0BA;
    p.p = 1.0; p.g = 0.003265; p.S = 1000.0; p.sigma = 5.67e-8; p.gamma = 0.25;
    p.q = 0.2 * p.S / p.sigma; p.q2 = p.q / 8.0; p.dt = 1.0;
    p.albedo_bare = 0.5; p.albedo_light = 0.75; p.albedo_dark = 0.25; p.temp_optimal = 295.5;
    p.agent_gamma = 0.05; p.food_chain_penalty = 0.5;
    p.initial_al = 0.2; p.initial_ad = 0.2; p.light_proportion = 0.33; p.dark_proportion = 0.33;
    return p;
}

static const char* sep(bool& first) { const char* s = first ? "\n" : ",\n"; first = false; return s; }

// ---- plans ---------------------------------------------------------------------------------------------------------
#define PLAN_FIELDS(X)                                                                                                  \
    X(kind) X(halo) X(packed) X(allow_fuse) X(fused_mode) X(fmt_planes) X(trace_pairs) X(sym_albedo) X(tcq) X(rpt)      \
    X(geom.B) X(geom.H) X(geom.W) X(geom.Wq) X(geom.tiles_r) X(geom.tiles_c) X(geom.ntiles) X(geom.chunk) X(geom.qcap)  \
    X(tile_lds)                                                                                                         \
    X(sgeom.B) X(sgeom.H) X(sgeom.W) X(sgeom.SR) X(sgeom.nrs) X(sgeom.ncs) X(sgeom.nstrips) X(sgeom.nwg) X(sgeom.chunk) \
    X(sgeom.qcap) X(sgeom.force_rescan) X(sgeom.lpw) X(sgeom.wpr)                                                       \
    X(fgeom.B) X(fgeom.H) X(fgeom.W) X(fgeom.SR) X(fgeom.nrs) X(fgeom.ncs) X(fgeom.cols_per_strip) X(fgeom.nstrips)     \
    X(fgeom.nwg) X(fgeom.chunk) X(fgeom.qcap) X(fgeom.mcap) X(fgeom.sure_need) X(fgeom.lpw) X(fgeom.wpr)                \
    X(first_prec) X(first_stream)                                                                                       \
    X(first_geom.B) X(first_geom.H) X(first_geom.W) X(first_geom.SR) X(first_geom.nrs) X(first_geom.ncs)                \
    X(first_geom.nstrips) X(first_geom.lpw) X(first_geom.wpr)                                                           \
    X(need_fixq) X(pw_stream)

static void print_plan(bool& first, const std::string& name, const dw_params& p, const Switches& sw) {
    const StepPlan s = plan_steps(p, sw);
    std::printf("%s  \"%s\": [", sep(first), name.c_str());
    bool f = true;
#define X(field) std::printf("%s%lld", f ? "" : ", ", (long long)s.field); f = false;
    PLAN_FIELDS(X)
#undef X
    std::printf("]");
}

struct Variant { const char* name; Switches sw; };

static std::vector<Variant> variants() {
    std::vector<Variant> v;
    auto add = [&](const char* name, auto&& set) { Variant x{name, Switches{}}; set(x.sw); v.push_back(x); };
    add("default", [](Switches&) {});
    add("no_fuse", [](Switches& w) { w.no_fuse = true; });
    add("no_ring", [](Switches& w) { w.no_ring = true; });
    add("no_fmt_planes", [](Switches& w) { w.no_fmt_planes = true; });
    add("no_pack", [](Switches& w) { w.no_pack = true; });
    add("no_sym", [](Switches& w) { w.no_sym = true; });
    add("kernel=tiled", [](Switches& w) { std::snprintf(w.kernel, sizeof(w.kernel), "tiled"); });
    add("kernel=tiled,tile_rpt=8", [](Switches& w) { std::snprintf(w.kernel, sizeof(w.kernel), "tiled"); w.tile_rpt = 8; });
    add("strip_rows=8", [](Switches& w) { w.strip_rows = 8; });
    add("strip_rows=64", [](Switches& w) { w.strip_rows = 64; });
    add("strip_rows=128", [](Switches& w) { w.strip_rows = 128; });
    add("tile_rpt=8", [](Switches& w) { w.tile_rpt = 8; });
    add("queue_cap=4", [](Switches& w) { w.queue_cap = 4; });
    add("mismatch_cap=3,force_rescan", [](Switches& w) { w.mismatch_cap = 3; w.force_rescan = true; });
    add("pack_min_strips=1", [](Switches& w) { w.pack_min_strips = 1; });
    add("first_f64", [](Switches& w) { w.first_f64 = true; });
    add("first_generic", [](Switches& w) { w.first_generic = true; });
    return v;
}

static void print_plans() {
    static const int shapes[][3] = {{2, 16, 16},   {2, 40, 64},   {2, 40, 128},   {2, 40, 132},    {2, 96, 256},
                                    {2, 96, 512},  {2, 96, 1000}, {2, 96, 1024},  {2, 96, 1280},   {4096, 16, 64},
                                    {4096, 16, 96}, {8, 16, 64},  {1, 40000, 32768}};
    static const char* prec[] = {"exact", "fast", "f64"};
    std::printf("\"plan_fields\": [");
    bool f = true;
#define X(field) std::printf("%s\"%s\"", f ? "" : ", ", #field); f = false;
    PLAN_FIELDS(X)
#undef X
    std::printf("],\n\"plan\": {");
    bool first = true;
    for (const Variant& v : variants())
        for (const auto& sh : shapes)
            for (int pr = 0; pr < 3; ++pr) {
                char name[96];
                std::snprintf(name, sizeof(name), "%dx%dx%d %s %s", sh[0], sh[1], sh[2], prec[pr], v.name);
                print_plan(first, name, params(sh[0], sh[1], sh[2], pr), v.sw);
            }
    // a non-symmetric albedo triple: the two-term coefficient chain is off
    dw_params p = params(2, 96, 512, DW_PRECISION_EXACT);
    p.albedo_light = 0.8;
    print_plan(first, "2x96x512 exact default albedo=0.5/0.8/0.25", p, Switches{});
    std::printf("\n}");
}

// ---- constants -----------------------------------------------------------------------------------------------------
template <class T>
static void print_words(const char* key, const T& v, bool last = false) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    uint32_t w[sizeof(T) / 4];
    std::memcpy(w, &v, sizeof(T));
    std::printf("    \"%s\": \"", key);
    for (size_t i = 0; i < sizeof(T) / 4; ++i) std::printf("%s%08x", i ? " " : "", w[i]);
    std::printf("\"%s", last ? "" : ",\n");
}

static void print_constants_of(bool& first, const std::string& name, const dw_params& p, double L, double L2) {
    std::printf("%s  \"%s L=%g\": {\n", sep(first), name.c_str(), L);
    const PhysF32 P = derive_f32(p, L);
    print_words("f64", make_f64(p, L));
    print_words("cbeta", cbeta_host(p));
    print_words("f32", P);
    print_words("f32_hb12", derive_f32(p, L, 12));
    print_words("first_from_f64", derive_first_bound(p, L, P, true));
    print_words("first_from_f32", derive_first_bound(p, L, P, false));
    print_words("first_test_slack", derive_first_bound(p, L, P, false, 0.25));
    PhysF32 pair[2];
    derive_f32_pair(p, L, L2, &pair[0], &pair[1]);
    print_words("pair", pair, true);
    std::printf("\n  }");
}

static void print_constants() {
    std::printf("\"constants\": {");
    bool first = true;
    const dw_params d = params(2, 96, 512, DW_PRECISION_EXACT);
    for (double L : {0.6, 1.0, 1.4}) print_constants_of(first, "default", d, L, L + 0.75 / 512);
    print_constants_of(first, "default", d, 0.1, 0.3);          // 1 + e can reach 0: the inadmissible branch of both bounds
    dw_params p = d; p.dt = 0.0;
    print_constants_of(first, "dt=0", p, 1.0, 1.2);
    p = d; p.dt = -1.0;
    print_constants_of(first, "dt=-1", p, 1.0, 1.2);
    p = d; p.g = 0.0;
    print_constants_of(first, "g=0", p, 1.0, 1.2);
    p = d; p.albedo_bare = 0.45; p.albedo_light = 0.8; p.albedo_dark = 0.2;
    print_constants_of(first, "albedo=0.45/0.8/0.2", p, 0.9, 1.3);
    p = d; p.p = 0.7;
    print_constants_of(first, "p=0.7", p, 1.0, 0.8);
    p = d; p.p = 0.7; p.gamma = 0.3; p.dt = 0.5; p.temp_optimal = 290.0; p.q = 0.15 * p.S / p.sigma; p.q2 = p.q / 6.0;
    print_constants_of(first, "p=0.7 gamma=0.3 dt=0.5 To=290 q=0.15 q2=q/6", p, 1.1, 0.7);
    std::printf("\n}");
}

int main() {
    std::printf("{\n");
    print_plans();
    std::printf(",\n");
    print_constants();
    std::printf("\n}\n");
    return 0;
}
