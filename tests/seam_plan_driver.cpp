// seam_plan_driver.cpp — prints the seam-strip layout that csrc/dw_plan.hpp plans (StepPlan::seam_strips, seam_geom,
// left_geom) as one JSON document, for tests/test_seam_plan_cpu.py.  Host C++17 only: no HIP header, no device.
// Arguments: any number of "B H W precision strip_rows no_seam no_fmt" septuples (integers; strip_rows 0: the plan's choice).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dw_plan.hpp"

using namespace dw;

int main(int argc, char** argv) {
    std::printf("[");
    for (int a = 1; a + 6 < argc; a += 7) {
        dw_params p;
        std::memset(&p, 0, sizeof(p));
        p.abi_version = DW_ABI_VERSION;
        p.batch = std::atoi(argv[a]); p.height = std::atoi(argv[a + 1]); p.width = std::atoi(argv[a + 2]);
        p.precision = std::atoi(argv[a + 3]);
        p.p = 1.0; p.albedo_bare = 0.5; p.albedo_light = 0.75; p.albedo_dark = 0.25;
        Switches sw;
        sw.strip_rows = std::atoi(argv[a + 4]);
        sw.no_seam_strips = std::atoi(argv[a + 5]) != 0;
        sw.no_fmt_planes = std::atoi(argv[a + 6]) != 0;
        const StepPlan s = plan_steps(p, sw);
        const FusedGeom &f = s.fgeom, &g = s.seam_geom, &l = s.left_geom;
        std::printf("%s\n{\"fmt_planes\": %d, \"seam_strips\": %d, \"fused_mode\": %d, \"nrs\": %d, \"old_ncs\": %d, \"old_nstrips\": %d, "
                    "\"n_full\": %d, \"seam_cols\": %d, \"seam_nstrips\": %d, \"seam_nwg\": %d, \"seam_chunk\": %d, "
                    "\"left_cols\": %d, \"left_lanes\": %d, \"left_bands\": %d, \"left_nstrips\": %d, \"left_nwg\": %d, "
                    "\"left_chunk\": %d, \"waves_per_world\": %ld}",
                    a > 1 ? "," : "", (int)s.fmt_planes, (int)s.seam_strips, s.fused_mode, f.nrs, f.ncs, f.nstrips, g.ncs,
                    g.cols_per_strip, g.nstrips, g.nwg, g.chunk, l.cols_per_strip, l.lpw, l.wpr, l.nstrips, l.nwg, l.chunk,
                    seam_waves_per_world(p.width, f.nrs));
    }
    std::printf("\n]\n");
    return 0;
}
