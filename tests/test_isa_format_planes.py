"""The format-buffer-access form of the float32 step-pair kernel on overlapped strips (step_stream_fused2_fmt_pw), checked
on the assembly hipcc emits (no GPU needed; one compilation of csrc/dw_api.hip with --save-temps).

The kernel is VALU-issue-bound, so what it saves is counted in instructions, against the kernel it replaces IN THE SAME
assembly (step_stream_fused2<0, false, false>), not against fixed numbers: its row loop holds no binary16 conversion and
no 64-bit vector address arithmetic, reads and writes its rows with six format loads and six format stores, keeps the 144
transcendentals of 24 cell-evaluations, and keeps the register budget of 4 waves per SIMD.

There is no exact form of the kernel: with four buffer descriptors the exact kernels spill scalar registers inside the row
loop, so the assembly must not hold one that the dispatch could never choose.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_fmt"))
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        m = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        if m and info:
            out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, m.group(1))
    return out


def _hot_loop(body):
    """the loop with the most packed float32 instructions: the row loop"""
    lines = body.split("\n")
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\.LBB\S+):", ln)] if m}
    best, best_pk = None, -1
    for i, ln in enumerate(lines):
        m = re.match(r"\ts_c?branch\S* (\.LBB\S+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            npk = sum(1 for x in lines[labels[m.group(1)]:i + 1] if x.startswith("\tv_pk_"))
            if npk > best_pk:
                best, best_pk = (labels[m.group(1)], i), npk
    return lines[best[0]:best[1] + 1] if best else []


def _pair(kernels):
    new = [n for n in kernels if "step_stream_fused2_fmt_pwILi0E" in n]
    old = [n for n in kernels if "step_stream_fused2ILi0ELb0ELb0E" in n]
    assert len(new) == 1 and len(old) == 1, (new, old)
    return kernels[new[0]], kernels[old[0]]


def _count(loop, pattern):
    return sum(1 for ln in loop if re.match(r"\t" + pattern, ln))


def test_row_loop_has_no_conversions_and_no_vector_addresses(kernels):
    (_, body), (_, old_body) = _pair(kernels)
    loop, old_loop = _hot_loop(body), _hot_loop(old_body)
    assert loop and old_loop
    # what the old loop pays (the premise): 24 un-packing conversions, 12 packing ones, 12 row addresses
    assert _count(old_loop, r"v_cvt_f32_f16") == 24 and _count(old_loop, r"v_cvt_pkrtz_f16_f32") == 12
    assert _count(old_loop, r"v_lshl_add_u64") == 12
    for op in (r"v_cvt_f32_f16", r"v_cvt_pkrtz_f16_f32", r"v_lshl_add_u64"):
        assert _count(loop, op) == 0, op
    assert _count(loop, r"buffer_load_format_xyzw") == 6 and _count(loop, r"buffer_store_format_xyzw") == 6
    assert _count(loop, r"(global|flat)_(load|store)") == 0
    assert _count(loop, r"v_(sqrt|rcp)_f32") == 144           # 24 cell-evaluations x 6
    assert _count(loop, r"s_(buffer_)?load") == 0             # the descriptors and constants are loaded once
    assert _count(loop, r"scratch_") == 0
    # the descriptors are provably wave-uniform: no waterfall loop around an access
    assert _count(loop, r"v_readfirstlane") == 0


def test_row_loop_is_at_least_40_vector_instructions_shorter(kernels):
    """48 instructions leave (36 conversions, 12 addresses); the prefetched rows, which no conversion moves into their
    window slots any more, cost 12 packed moves back.  Required: 40 fewer (the issue's margin for column / row-wrap
    arithmetic that may move)."""
    (_, body), (_, old_body) = _pair(kernels)
    valu = lambda loop: sum(1 for ln in loop if ln.startswith("\tv_"))
    new, old = valu(_hot_loop(body)), valu(_hot_loop(old_body))
    print(f"row loop VALU instructions: {old} -> {new} ({old / 24:.2f} -> {new / 24:.2f} per cell-evaluation)")
    assert new <= old - 40, (new, old)


def test_register_budget_of_four_waves(kernels):
    (info, _), (old_info, _) = _pair(kernels)
    print(f"VGPRs {old_info['NumVgprs']} -> {info['NumVgprs']}, SGPRs {old_info['TotalNumSgprs']} -> {info['TotalNumSgprs']}")
    assert info["NumVgprs"] <= 128 and info["Occupancy"] >= 4, info
    assert info["ScratchSize"] == old_info["ScratchSize"], (info["ScratchSize"], old_info["ScratchSize"])


def test_no_exact_format_kernel_is_built(kernels):
    assert not [n for n in kernels if "fused2_exact_fmt" in n]
