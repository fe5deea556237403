"""The step-pair kernels whose input rows land in their window slots (step_stream_fused2_land_seam_pw and
step_stream_fused2_land_left_pw), checked on the assembly hipcc emits (no GPU needed; the one compilation of
tests/test_isa_format_planes.py, its recipe and its `kernels` fixture).

The seam kernel is VALU-issue-bound and its map is frozen, so what the new form saves is the 18 register moves of the old
row loop (24 cell-evaluations): 12 `v_pk_mov_b32` that carried a prefetched row from the load's registers into its window
slot, and 6 `v_mov_b64` that copied the bare-fraction constant pair out of scalar registers in front of a packed fma.  The
old kernel IN THE SAME assembly is the yardstick: it still has 738 vector instructions, the new one at most 720, none of
them a move, with the same 144 transcendentals, the same 24 rotations folded into `v_add_f32_dpp`, the same accesses, no
scratch memory anywhere in the kernel, and the register budget of 4 waves per SIMD.

The loads are inline assembly behind the compiler's back, so the order the counted waits rely on is checked here too: in the
row loop every `s_waitcnt vmcnt(2)` stands behind four landing loads and the two row stores issued after them, and nothing
else touches vector memory in between.

The leftover kernel (2 % of the headline's waves) runs the same body: no moves, and a loop no longer than the old leftover
loop and at most 18 instructions shorter - the moves, not the map.
"""
import re

from test_isa_format_planes import _count, _hot_loop, kernels  # noqa: F401  (kernels: the module's fixture)

OLD_SEAM_LOOP_VALU = 738                                        # step_stream_fused2_seam_pw, 24 cell-evaluations
MOVES = r"v_(pk_mov_b32|mov_b64|mov_b32)"


def _one(kernels, part):
    names = [n for n in kernels if part in n]
    assert len(names) == 1, (part, names)
    return kernels[names[0]]


def _valu(loop):
    return sum(1 for ln in loop if ln.startswith("\tv_"))


def test_names_keep_the_old_kernels_unique(kernels):
    for part in ("step_stream_fused2_seam_pw", "step_stream_fused2_left_pw", "step_stream_fused2_fmt_pw"):
        assert len([n for n in kernels if part in n]) == 1, part
    for part in ("step_stream_fused2_land_seam_pw", "step_stream_fused2_land_left_pw"):
        name = [n for n in kernels if part in n]
        assert len(name) == 1 and "step_stream_fused2I" not in name[0], (part, name)


def test_seam_row_loop_has_no_moves(kernels):
    _, body = _one(kernels, "step_stream_fused2_land_seam_pw")
    _, old_body = _one(kernels, "step_stream_fused2_seam_pw")
    loop, old_loop = _hot_loop(body), _hot_loop(old_body)
    assert loop and old_loop
    print(f"row loop VALU instructions: seam {_valu(old_loop)} ({_count(old_loop, MOVES)} moves), "
          f"landing {_valu(loop)} ({_count(loop, MOVES)} moves)")
    assert _valu(old_loop) == OLD_SEAM_LOOP_VALU                # the premise
    assert _count(old_loop, r"v_pk_mov_b32") == 12 and _count(old_loop, r"v_mov_b64") == 6
    assert _count(loop, MOVES) == 0
    assert _valu(loop) <= 720
    assert _count(loop, r"v_(sqrt|rcp)_f32") == 144
    assert _count(loop, r"v_add_f32_dpp .*wave_ro[lr]:1") == 24
    assert _count(loop, r"v_cvt") == 0
    assert _count(loop, r"v_mov_b32_dpp") == 0
    assert _count(loop, r"buffer_load_format_xy ") == 12 and _count(loop, r"buffer_load_format_xyzw") == 0
    assert _count(loop, r"buffer_store_format_xyzw") == 6
    assert _count(loop, r"(global|flat)_(load|store)") == 0
    assert _count(loop, r"(scratch_|ds_|s_barrier)") == 0


def test_seam_kernel_register_budget_and_no_scratch_anywhere(kernels):
    info, body = _one(kernels, "step_stream_fused2_land_seam_pw")
    print(f"{info['NumVgprs']} VGPRs, {info['TotalNumSgprs']} SGPRs, {info['ScratchSize']} scratch bytes")
    assert info["NumVgprs"] <= 128 and info["Occupancy"] == 4, info
    assert info["ScratchSize"] == 0, info
    assert not re.search(r"\n\tscratch_", "\n" + body)


def test_counted_waits_follow_four_loads_and_two_stores(kernels):
    """vmcnt retires in issue order: a wait for all but the 2 youngest accesses covers the landing loads exactly if the
    two row stores, and nothing else, were issued behind them.  Rotated to start at a wait, the loop is three times
    (4 loads, 2 stores, wait)."""
    _, body = _one(kernels, "step_stream_fused2_land_seam_pw")
    loop = _hot_loop(body)
    seq = []
    for ln in loop:
        m = re.match(r"\t(buffer_load_format_xy|buffer_store_format_xyzw|s_waitcnt vmcnt\((\d+)\))", ln)
        if m:
            seq.append("L" if "load" in m.group(1) else ("S" if "store" in m.group(1) else "W" + m.group(2)))
        assert not re.match(r"\t(global_|flat_|scratch_|buffer_(?!load_format_xy |store_format_xyzw ))", ln), ln
    assert seq.count("W2") == 3 and not [s for s in seq if s.startswith("W") and s != "W2"], seq
    k = seq.index("W2") + 1
    assert seq[k:] + seq[:k] == ["L", "L", "L", "L", "S", "S", "W2"] * 3, seq
    # the loaded registers are read only behind the wait: every load's destination pair is no operand of an instruction
    # between the load and the next wait
    n = len(loop)
    for i, ln in enumerate(loop):
        m = re.match(r"\tbuffer_load_format_xy v\[(\d+):(\d+)\]", ln)
        if not m:
            continue
        regs = {int(m.group(1)), int(m.group(2))}
        for d in range(1, n):
            nxt = loop[(i + d) % n]
            if nxt.startswith("\ts_waitcnt vmcnt(2)"):
                break
            if nxt.startswith(("\tv_", "\tbuffer_")):
                used = set()
                for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", nxt):
                    used.update(range(int(a), int(b) + 1))
                used.update(int(a) for a in re.findall(r"\bv(\d+)\b", nxt))
                assert not (regs & used), (ln, nxt)
        else:
            raise AssertionError("no wait behind " + ln)


def test_leftover_row_loop_has_no_moves(kernels):
    info, body = _one(kernels, "step_stream_fused2_land_left_pw")
    _, old_body = _one(kernels, "step_stream_fused2_left_pw")
    loop, old_loop = _hot_loop(body), _hot_loop(old_body)
    assert loop and old_loop
    print(f"leftover row loop VALU instructions: {_valu(old_loop)} -> {_valu(loop)}; {info['NumVgprs']} VGPRs")
    # the 18 register moves are gone; what is left of the old loop's `v_mov_b32` copies the grid height out of a scalar
    # register for the lane's own row wrap (per-lane row addressing, as before: it is no move of a row or a constant pair)
    assert _count(loop, r"v_(pk_mov_b32|mov_b64)") == 0
    assert _count(old_loop, r"v_pk_mov_b32") == 12 and _count(old_loop, r"v_mov_b64") == 6
    assert _count(loop, r"v_mov_b32_e32 v\d+, v\d+") == 0
    assert _count(loop, r"v_mov_b32") == _count(old_loop, r"v_mov_b32") == _count(loop, r"v_mov_b32_e32 v\d+, s\d+")
    assert _valu(old_loop) - 18 <= _valu(loop) <= _valu(old_loop)
    assert _count(loop, r"v_(sqrt|rcp)_f32") == 144
    assert _count(loop, r"v_cvt") == 0 and _count(loop, r"v_mov_b32_dpp") == 0
    assert _count(loop, r"buffer_store_format_xyzw") == 6
    assert _count(loop, r"(global|flat)_(load|store)") == 0
    assert _count(loop, r"(scratch_|ds_|s_barrier)") == 0
    # the leftover waves' stores are per band: their waits are for everything
    assert _count(loop, r"s_waitcnt vmcnt\(0\)") == 3
    assert info["NumVgprs"] <= 128 and info["Occupancy"] == 4 and info["ScratchSize"] == 0, info
