"""The seam-strip form of the float32 step-pair kernel (step_stream_fused2_seam_pw), checked on the assembly hipcc emits
(no GPU needed; one compilation of csrc/dw_api.hip with --save-temps), in the style of tests/test_isa_format_planes.py.

The layout pays only if a wave of 63 writing lanes costs what a wave of 62 costs: the seam kernel's row loop may hold no more
vector instructions than the row loop of the kernel it replaces IN THE SAME assembly (step_stream_fused2_fmt_pw<0>: 738 for 24
cell-evaluations), the same 144 transcendentals, no conversion, and it keeps the register budget of 4 waves per SIMD (at most
128 VGPRs) without scratch memory.  Its rows arrive as two 2-component format loads per plane and row (the seam lane's two
halves are not adjacent in memory) and leave as one 4-component format store, as before.

The leftover kernel (step_stream_fused2_left_pw: 2 % of the headline's waves) addresses rows per lane, which costs vector
instructions by design; it is held to the register budget and to the map's arithmetic only.
"""
import re

import pytest

from test_isa_format_planes import _count, _hot_loop, kernels  # noqa: F401  (kernels: the module's fixture)

FMT_LOOP_VALU = 738                                             # step_stream_fused2_fmt_pw<0>, 24 cell-evaluations


def _one(kernels, part):
    names = [n for n in kernels if part in n]
    assert len(names) == 1, (part, names)
    return kernels[names[0]]


def _valu(loop):
    return sum(1 for ln in loop if ln.startswith("\tv_"))


@pytest.mark.parametrize("name", ("step_stream_fused2_seam_pw", "step_stream_fused2_left_pw"))
def test_register_budget_of_four_waves_and_no_scratch(kernels, name):
    info, _ = _one(kernels, name)
    print(f"{name}: {info['NumVgprs']} VGPRs, {info['TotalNumSgprs']} SGPRs, {info['ScratchSize']} scratch bytes")
    assert info["NumVgprs"] <= 128 and info["Occupancy"] >= 4, info
    assert info["ScratchSize"] == 0, info


def test_seam_row_loop_costs_no_more_than_the_overlapped_one(kernels):
    _, body = _one(kernels, "step_stream_fused2_seam_pw")
    _, old_body = _one(kernels, "step_stream_fused2_fmt_pwILi0E")
    loop, old_loop = _hot_loop(body), _hot_loop(old_body)
    assert loop and old_loop
    print(f"row loop VALU instructions: overlapped {_valu(old_loop)}, seam {_valu(loop)}")
    assert _valu(old_loop) == FMT_LOOP_VALU                     # the premise
    assert _valu(loop) <= FMT_LOOP_VALU
    assert _count(loop, r"v_(sqrt|rcp)_f32") == 144 == _count(old_loop, r"v_(sqrt|rcp)_f32")
    assert _count(loop, r"v_cvt") == 0
    assert _count(loop, r"v_lshl_add_u64") == 0
    # three rows, two planes: two pair loads each; one quad store each
    assert _count(loop, r"buffer_load_format_xy ") == 12 and _count(loop, r"buffer_load_format_xyzw") == 0
    assert _count(loop, r"buffer_store_format_xyzw") == 6
    assert _count(loop, r"(global|flat)_(load|store)") == 0
    assert _count(loop, r"s_(buffer_)?load") == 0
    assert _count(loop, r"scratch_") == 0
    assert _count(loop, r"v_readfirstlane") == 0                # wave-uniform descriptors: no waterfall loop
    assert _count(loop, r"(ds_|s_barrier)") == 0                # nothing is exchanged between waves
    # the horizontal neighbours: rotations folded into the pair sums, 24 as in the overlapped loop's shifts
    assert _count(loop, r"v_add_f32_dpp .*wave_ro[lr]:1") == 24
    assert _count(loop, r"v_mov_b32_dpp") == 0


def test_leftover_row_loop_keeps_the_map(kernels):
    _, body = _one(kernels, "step_stream_fused2_left_pw")
    loop = _hot_loop(body)
    assert loop
    print(f"leftover row loop VALU instructions: {_valu(loop)}")
    assert _count(loop, r"v_(sqrt|rcp)_f32") == 144
    assert _count(loop, r"v_cvt") == 0
    assert _count(loop, r"buffer_load_format_xyzw") == 6 and _count(loop, r"buffer_store_format_xyzw") == 6
    assert _count(loop, r"(global|flat)_(load|store)") == 0
    assert _count(loop, r"scratch_") == 0
    assert _count(loop, r"(ds_|s_barrier)") == 0
    # per-lane row addressing and the per-lane band height: a few instructions per row, not a second map
    assert _valu(loop) <= FMT_LOOP_VALU + 60
