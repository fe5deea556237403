// constant_edges_driver.cpp — which branches of csrc/dw_plan.hpp a constant set reaches (tests/test_constant_edges_cpu.py).
// Host C++17 only, built as tests/plan_driver.cpp is.  Reads lines of thirteen numbers from standard input,
//   p g S sigma gamma q q2 dt albedo_bare albedo_light albedo_dark temp_optimal L
// and prints one JSON object per line: what tie_chain, derive_f32, derive_first_bound and albedo_symmetric say.
#include <cstdio>
#include <cstring>

#include "dw_plan.hpp"

using namespace dw;

int main() {
    double v[13];
    std::printf("[");
    bool first = true;
    while (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6],
                      &v[7], &v[8], &v[9], &v[10], &v[11], &v[12]) == 13) {
        dw_params p;
        std::memset(&p, 0, sizeof(p));
        p.abi_version = DW_ABI_VERSION;
        p.batch = 2; p.height = 12; p.width = 256; p.precision = DW_PRECISION_EXACT;
        p.p = v[0]; p.g = v[1]; p.S = v[2]; p.sigma = v[3]; p.gamma = v[4]; p.q = v[5]; p.q2 = v[6]; p.dt = v[7];
        p.albedo_bare = v[8]; p.albedo_light = v[9]; p.albedo_dark = v[10]; p.temp_optimal = v[11];
        const double L = v[12];
        // the chain exactly as derive_f32 feeds it (the same a1 .. a4; de does not enter `admissible`)
        const double To4 = std::pow(p.temp_optimal, 4), K = p.S * L / p.sigma;
        const double dal = p.albedo_light - p.albedo_bare, dad = p.albedo_dark - p.albedo_bare;
        const TieChain t = tie_chain(p, e_const(p, L), (p.q - K) * dal / (8000.0 * To4), (p.q - K) * dad / (8000.0 * To4),
                                     (-p.q + p.q2) * dal / (1000.0 * To4), (-p.q + p.q2) * dad / (1000.0 * To4), 0.0);
        const PhysF32 P = derive_f32(p, L);
        const FirstStepBound fb = derive_first_bound(p, L, P, true);
        std::printf("%s\n{\"admissible\": %d, \"one_plus_emin\": %.17g, \"tie_lo\": %.9g, \"eK0s\": %.9g, \"eK1s\": %.9g, "
                    "\"ck\": %.9g, \"hi_bits\": %d, \"symmetric\": %d, \"kbeta\": %.17g, \"p_f32\": %.9g, \"pu\": %.17g, "
                    "\"kbmax\": %.17g, \"a3\": %.9g, \"a4\": %.9g, \"first_slack\": %.9g}",
                    first ? "" : ",", t.admissible ? 1 : 0, 1.0 + t.emin, (double)P.tie_lo, (double)P.eK0s, (double)P.eK1s,
                    (double)P.ck, P.hi_bits, albedo_symmetric(p.albedo_bare, p.albedo_light, p.albedo_dark) ? 1 : 0,
                    (double)P.kbeta, (double)P.p, t.pu, t.kbmax, (double)P.a3, (double)P.a4, (double)fb.slack);
        first = false;
    }
    std::printf("\n]\n");
    return 0;
}
