"""The per-world constant rows and the schedule of a step series (csrc/dw_series.hpp), without a GPU.

tests/series_driver.cpp includes only dw_series.hpp and is compiled here as plain C++17 by the clang++ that ships with
ROCm (the recipe of test_plan_cpu.py; once more with -fsanitize=address,undefined where that clang++ links its sanitizer
runtime).  There is no recorded fixture: this logic had no form of its own before it moved into the header, so the
expectations are computed independently -

  * WorldRows: every word it writes (PhysF32, PhysF64, PairPw, FirstStepBound) next to a derivation without cache and
    without twin reuse that the driver makes for the same step and world;
  * plan_series: the rules restated below in Python (_expected), over the grid the driver prints.
"""
import json
import os
import subprocess

import pytest

from test_plan_cpu import CSRC, ROOT, _rocm_clang

STATS_BYTES, TEMP_BYTES = 24, 32            # one world's record of the two series
SINGLE_ROW, PAIR_ROW = 256, 256             # bytes per world of a table row: PhysF32 + PhysF64, PairPw


def _build(tmp, extra=()):
    exe = tmp / ("series_driver" + ("_san" if extra else ""))
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", *extra, "-I", CSRC,
                           os.path.join(ROOT, "tests", "series_driver.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    if _rocm_clang() is None:
        pytest.skip("the clang++ of ROCm is not installed")
    return tmp_path_factory.mktemp("series")


@pytest.fixture(scope="module")
def driver_output(build_dir):
    out = subprocess.run([str(_build(build_dir))], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


# ---- WorldRows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sweep", "distinct", "own"])
def test_world_rows_write_what_a_fresh_derivation_writes(driver_output, case):
    c = driver_output["world_rows"][case]
    per_step = c["steps"] * c["B"]
    sizes = {"f32": (per_step, 32), "f64": (per_step, 32), "f32_only": (per_step, 32), "pair": (per_step - c["B"], 64),
             "first_from_f64": (per_step, 12), "first_from_f32": (per_step, 12)}
    for key, (n, nwords) in sizes.items():
        got, want = c[key]["got"], c[key]["want"]
        assert len(got) == len(want) == n, key
        assert all(len(w.split()) == nwords for w in want), key
        wrong = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not wrong, f"{case}: {key} differs at (step, world) {[divmod(i, c['B']) for i in wrong[:5]]}"
    # the cases are worth something: the rows change along the run and differ between worlds
    assert len(set(c["f32"]["want"])) > c["steps"]


def test_sharing_saves_derivations_and_nothing_else(driver_output):
    rows = driver_output["world_rows"]
    sweep, distinct, own = rows["sweep"], rows["distinct"], rows["own"]
    for key in ("derived_singles", "derived_singles_f32_only"):
        assert distinct[key] == distinct["steps"] * distinct["B"]      # no twins, no luminosity twice: nothing to share
        assert 0 < sweep[key] < sweep["steps"] * sweep["B"]
        assert own[key] < own["steps"] * own["B"]
    assert distinct["derived_pairs"] == (distinct["steps"] - 1) * distinct["B"]
    assert 0 < sweep["derived_pairs"] < (sweep["steps"] - 1) * sweep["B"]
    # the sweep, counted by hand: worlds 0, 3, 5 derive at step 0 and at each of the 7 changes, world 1 is world 0's twin
    # throughout, world 2 has a luminosity of its own, world 4 derives once, world 6 is 5's twin, world 7 changes always
    assert sweep["derived_singles"] == 3 * 8 + 8 + 1 + 12


# ---- plan_series -------------------------------------------------------------------------------------------------------
def _luminosity(kind, t):
    """what distinguishes step t's luminosities in the driver's schedules: constant | all-distinct | constant for five steps"""
    return 0 if kind == 0 else (t if kind == 1 else (0 if t < 5 else t))


def _expected(c):
    """The rules of the series calls, restated."""
    n, B, hook = c["nsteps"], c["B"], c["trace_rows"] >= 1
    rows = c["trace_rows"] if hook else (32 << 20) // ((TEMP_BYTES if c["temps"] else STATS_BYTES) * B)
    pairs = bool(c["may_pair"]) and not c["temps"]           # single steps along with temperature records
    even = bool(c["always_even"]) or pairs                   # dw_step_n_trace: always; the ensemble call: with pairs
    if even:
        rows = max(rows - rows % 2, 2)
    rows = max(1, min(rows, n))
    is_pair, t, quantised = [0] * n, 0, bool(c["quantised"])
    while t < n:
        if pairs and quantised and n - t >= 3 and t // rows == (t + 1) // rows:
            is_pair[t] = 1
            t += 2
        else:
            quantised = True                                 # a single step leaves a quantised state
            t += 1
    want = {"rows": rows, "is_pair": is_pair, "npairs": sum(is_pair), "even": int(even)}
    if c["form"] != "table":
        return want
    limit = [(8 << 20) // (SINGLE_ROW * B), (8 << 20) // (PAIR_ROW * B)]
    if hook:
        limit = [min(limit[0], c["trace_rows"]), min(limit[1], c["trace_rows"] // 2)]
    limit = [max(1, min(limit[0], n)), max(1, min(limit[1], sum(is_pair))) if sum(is_pair) else 0]
    row_of, chunks, t = [0] * n, [], 0
    lum = lambda t, k: tuple(_luminosity(c["schedule"], t + i) for i in range(k + 1))
    while t < n:
        built = [[], []]                                     # the luminosities of the rows of each kind in this chunk
        while t < n:
            k = is_pair[t]
            if not built[k] or built[k][-1] != lum(t, k):
                if len(built[k]) == limit[k]:
                    break
                built[k].append(lum(t, k))
            row_of[t] = len(built[k]) - 1
            t += k + 1
        chunks.append([t, len(built[0]), len(built[1])])
    want.update(trows=limit[0], prows=limit[1], row_of=row_of, chunks=chunks)
    return want


def test_the_grid_is_the_one_asked_for(driver_output):
    cases = driver_output["schedules"]
    table = [c for c in cases if c["form"] == "table" and c["B"] == 3]
    combos = {(c["nsteps"], c["trace_rows"], c["may_pair"], c["quantised"], c["temps"], c["schedule"]) for c in table}
    assert len(combos) == 8 * 5 * 2 * 2 * 2 * 3 and {c["nsteps"] for c in table} == {1, 2, 3, 4, 5, 7, 8, 11}
    assert {c["form"] for c in cases} == {"table", "shared", "shared_temperature"}
    assert any(c["B"] > 100000 for c in cases)               # ... and calls whose chunks the byte limits decide


def test_schedules_follow_the_rules(driver_output):
    for c in driver_output["schedules"]:
        want = _expected(c)
        for key, value in want.items():
            assert c[key] == value, (key, c)


def test_schedules_have_the_properties_the_calls_rely_on(driver_output):
    seen_straddle_candidates = 0
    for c in driver_output["schedules"]:
        n, rows, is_pair = c["nsteps"], c["rows"], c["is_pair"]
        # every step is taken exactly once
        taken = [0] * n
        t = 0
        while t < n:
            for i in range(is_pair[t] + 1):
                taken[t + i] += 1
            t += is_pair[t] + 1
        assert taken == [1] * n and t == n, c
        starts = [t for t in range(n) if is_pair[t]]
        assert all(not is_pair[t + 1] for t in starts)
        # chunks of the series: even and at least two where pairs may land in them, never above the run
        assert 1 <= rows <= n
        if c["even"] and n >= 2:
            assert rows % 2 == 0 or rows == n, c
        # pairs: never with temperature records or where the call may not take them, never the closing one or two steps,
        # never across two chunks of the series, never from an un-quantised state
        if c["temps"] or not c["may_pair"]:
            assert not starts, c
        assert all(n - t >= 3 and t // rows == (t + 1) // rows for t in starts), c
        assert c["quantised"] or not is_pair[0]
        seen_straddle_candidates += sum(1 for t in range(n - 2) if t % rows == rows - 1 and c["may_pair"])
        if c["form"] != "table":
            continue
        # the table: no chunk above its limits, every step's row built from exactly its own luminosities
        begin = 0
        for end, singles, pairs in c["chunks"]:
            assert begin < end and 0 < singles + pairs and singles <= c["trows"] and pairs <= c["prows"], c
            in_chunk = [t for t in range(begin, end) if not (t and is_pair[t - 1])]      # (not a pair's second step)
            assert {c["row_of"][t] for t in in_chunk if not is_pair[t]} == set(range(singles)), c
            assert {c["row_of"][t] for t in in_chunk if is_pair[t]} == set(range(pairs)), c
            assert all(begin <= c["src"][t] <= t for t in in_chunk), c
            begin = end
        assert begin == n
        for t in range(n):
            if t and is_pair[t - 1]:
                continue                                     # the second step of a pair: the pair's row serves it
            k = is_pair[t]
            assert is_pair[c["src"][t]] == k, c
            assert all(_luminosity(c["schedule"], t + i) == _luminosity(c["schedule"], c["src"][t] + i) for i in range(k + 1)), c
            assert c["rows_ok"][t] == (1 if c["B"] == 3 else -1), c
        if c["schedule"] == 0:                               # a constant schedule: one row of each kind for the whole run
            assert len(c["chunks"]) == 1 and c["chunks"][0][1] == 1 and c["chunks"][0][2] == (1 if starts else 0), c
    assert seen_straddle_candidates > 100                    # the grid does put steps where a pair would straddle


def test_driver_is_clean_under_the_sanitizers(build_dir, driver_output):
    """The same stand-alone host program with -fsanitize=address,undefined: same answers, nothing reported."""
    probe = build_dir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run([_rocm_clang(), "-fsanitize=address,undefined", str(probe), "-o", str(build_dir / "probe")],
                         capture_output=True).returncode == 0
    if not can:
        pytest.skip("this clang++ does not link its sanitizer runtime")
    exe = _build(build_dir, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert got["schedules"] == driver_output["schedules"]
    # (the two builds fold the driver's own luminosity arithmetic differently, to the last bit: each is held to itself)
    for name, case in got["world_rows"].items():
        for key, value in case.items():
            if isinstance(value, dict):
                assert value["got"] == value["want"], (name, key)
            else:
                assert value == driver_output["world_rows"][name][key], (name, key)
