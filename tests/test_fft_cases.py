"""The FFT case tables (tests/fft_cases.py) held to the rule they are drawn from: a case for every kernel family, every seam
case across its seam, the f32 rule equal to the one the library runs (csrc/fft_plan.hpp, executed at every length), and every
threshold of the f64 rule still in the source it restates.  No GPU."""
import os
import subprocess

import pytest

import fft_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """tests/fft_plan_test.cpp -- the library's own rule (csrc/fft_plan.hpp) and table builder (csrc/roots.hpp), nothing else of
    it -- built with AddressSanitizer and UBSan and run once as a program of its own: ({name: value}, {section: {n: label}})."""
    exe = str(tmp_path_factory.mktemp("fft_plan") / "fft_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "comms_rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fft_plan_test.cpp"), "-o", exe], timeout=300)
    out = subprocess.run([exe, str(fc.NUM_CU)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    consts, forms, roots = {}, {}, None
    for line in out.stdout.splitlines():
        f = line.split("\t")
        if f[0] == "const":
            consts[f[1]] = int(f[2])
        elif f[0] == "form":
            forms.setdefault(f[1], {})[int(f[2])] = f[3]
        elif f[0] == "roots":
            roots = (int(f[1]), int(f[2]))
    assert roots is not None and roots[0] > 40000 and roots[1] == 0, (roots, out.stderr[-4000:])
    return consts, forms


def test_family_f32_is_the_rule_the_library_runs(plan):
    """family_f32(n) against fft_form / pow2_form themselves, at every length 1 ... 70000 and around every power of two up to
    2^25: the same label, and a refusal exactly where family_f32 raises."""
    _, forms = plan
    default = forms["default"]
    assert set(range(1, 70001)) <= set(default)
    assert {(1 << k) + d for k in range(1, 26) for d in (-1, 0, 1)} <= set(default)
    for n, label in default.items():
        try:
            want = fc.family_f32(n)
        except ValueError:
            want = "refused"
        assert label == want or (want == "refused" and label.startswith("refused: ")), (n, label, want)
    assert default[1 << 25] == "refused: power-of-two FFT supports up to 2^24 points (got 2^25)"
    assert default[fc.F32_REFUSED] == "refused: FFT length %d too large" % fc.F32_REFUSED


def test_batching_constants_are_the_headers(plan):
    consts, _ = plan
    assert consts == {"tile_points": fc.F32_TILE_POINTS, "blu_chunk_points": fc.F32_BLU_CHUNK_POINTS, "blu_max_n": fc.F32_BLU_MAX_N,
                      "small_dft_grid_cap": fc.F32_DIRECT_GROUP_CAP, "small_dft_lanes": fc.F32_SMALL_DFT_LANES,
                      "small_dft_max": fc.F32_SMALL_DFT_MAX, "direct_max": fc.F32_DIRECT_MAX, "direct_max_cap": fc.F32_DIRECT_MAX_CAP}


def test_selectors_move_their_cases_to_the_forms_they_name(plan):
    """Under each selector of FALLBACKS every one of its cases leaves its default form, for the form the comment beside the
    selector names."""
    _, forms = plan
    assert set(forms) == {"default"} | {"%s=%s" % (name, value) for name, (value, _) in fc.FALLBACKS.items()}
    named = {
        # the generic tile kernel; Bluestein unfused on it
        "COMMS_FFT_NO_RX": lambda n: "pow2_tile_2p%d" % fc.ilog2(n) if fc.is_pow2(n) else "blu_tile_M2p%d" % fc.ilog2(fc.padded(n)),
        "COMMS_FFT_NO_RX32K": lambda n: "pow2_tile_2p15",                     # 32 x 1024 on the tile kernel + rows
        "COMMS_FFT_NO_COLS": lambda n: "pow2_tile_2p%d" % fc.ilog2(n),        # column pass on the tile kernel
        "COMMS_FFT_BLU_UNFUSED": lambda n: "blu_unfused_rx_M%d" % fc.padded(n),  # pre / mul / post around the single-pass kernel
        # dft_small_kernel at 65 ... 128, dft_direct_kernel above
        "COMMS_FFT_DIRECT_MAX": lambda n: "direct" if n <= fc.F32_SMALL_DFT_MAX else "direct_large",
    }
    assert set(named) == set(fc.FALLBACKS)
    for name, (value, cases) in fc.FALLBACKS.items():
        under = forms["%s=%s" % (name, value)]
        for n, _ in cases:
            assert under[n] != forms["default"][n], (name, n)
            assert under[n] == named[name](n), (name, n, under[n])
        # ... and moves nothing but what it names: every other length keeps its label's family
        moved = {n for n in under if under[n] != forms["default"][n]}
        assert all("tile" in under[n] or "unfused" in under[n] or under[n].startswith("direct") for n in moved), name


def test_thresholds_still_stand_in_the_source():
    """Each rule of family_f64 (and NUM_CU) names the source text it restates; a threshold that moves takes its text along."""
    texts = {}
    for path, where, text in fc.ANCHORS:
        if path not in texts:
            with open(os.path.join(ROOT, path)) as f:
                texts[path] = f.read()
        assert text in texts[path], "%s (%s) no longer reads %r: restate the rule in tests/fft_cases.py" % (path, where, text)


def test_seam_enumeration_finds_every_family():
    """all_families() samples the lengths around 2^k and the direct threshold; a sweep of every length up to 70000 (and the
    band around 4096, where the f64 rule turns) finds nothing more below those lengths' families."""
    for family in (fc.family_f32, fc.family_f64):
        swept = {family(n) for n in range(1, 70001)}
        assert swept <= fc.all_families(family)
        assert swept == fc.all_families(family, limit=1 << 16)


def test_expected_labels():
    f32, f64 = fc.all_families(fc.family_f32), fc.all_families(fc.family_f64)
    assert {"direct", "blu_fused_M256", "blu_fused_M512", "blu_fused_M16384", "blu_rx32k", "blu_cols_M2p17", "blu_fast_M2p20",
            "blu_gather_M2p22", "blu_three_M2p24", "pow2_copy", "pow2_tiny", "pow2_rx64", "pow2_rx32k", "pow2_three_2p24"} <= f32
    assert len(f32) == 1 + 7 + 1 + 4 + 1 + 3 + 1 + (1 + 1 + 9 + 1 + 4 + 1 + 3 + 1)  # direct, Bluestein by M, powers of two
    assert f64 == ({"lds", "dft_sum"} | {"four_step_%d" % k for k in range(13, 25)} | {"blu_P2p%d" % k for k in range(14, 25)})
    assert fc.family_f32(129) == fc.family_f32(255) == "blu_fused_M512"
    assert fc.family_f32(64) == "pow2_rx64" and fc.family_f32(63) == "direct" and fc.family_f32(65) == "blu_fused_M256"
    for refused, family in ((fc.F32_REFUSED, fc.family_f32), (fc.F64_REFUSED, fc.family_f64), (1 << 25, fc.family_f32), (0, fc.family_f64)):
        with pytest.raises(ValueError):
            family(refused)
    assert fc.family_f32(fc.F32_REFUSED - 2) == "blu_three_M2p24" and fc.family_f64(fc.F64_REFUSED - 2) == "blu_P2p24"


def test_every_family_has_a_case():
    have32 = {fc.family_f32(n) for n, _, _ in fc.F32_CASES}
    assert fc.all_families(fc.family_f32) - have32 == set()
    have64 = {fc.family_f64(n) for n, _, _ in fc.F64_CASES} | set(fc.F64_COVERED_ELSEWHERE)
    assert fc.all_families(fc.family_f64) - have64 == set()
    for label, test_id in fc.F64_COVERED_ELSEWHERE.items():  # ... and the test named for it is there
        module, name = test_id.split("::")
        with open(os.path.join(ROOT, "tests", module)) as f:
            assert "def %s(" % name in f.read(), (label, test_id)


def test_every_seam_case_crosses_its_seam():
    tables = {"f32": fc.F32_GROUPS, "f64": fc.F64_GROUPS}
    for (table, group), crosses in fc.SEAMS.items():
        cases = tables[table][group]
        assert cases
        for n, batches, _ in cases:
            for b in batches:
                assert crosses(n, b), (table, group, n, b)
    # the Bluestein chunk seams: one per form of the loop body
    assert [fc.family_f32(n) for n, _, _ in fc.F32_GROUPS["blu_chunk_seams"]] == ["blu_fused_M16384", "blu_rx32k", "blu_cols_M2p17"]
    # the batches around a tile are around it: below, one past, and past two tiles with a ragged third
    for n, batches, _ in fc.F32_GROUPS["blu_fused"]:
        xpt = fc.tile_xforms(n)
        assert fc.padded(n) * xpt == fc.F32_TILE_POINTS or xpt == 1
        assert {1, xpt + 1, 2 * xpt + 3} <= set(batches) and (xpt == 1 or xpt - 1 in batches)
    # both edges of every fused padded length
    assert sorted(fc.FUSED_LENGTHS) == sorted(v for m in (256, 512, 1024, 2048, 4096, 8192, 16384) for v in (m // 4 + 1, m // 2 - 1))
    # the smallest batch past launch_rx's grid: one tile fewer is not past it
    for n, (b,), _ in fc.F32_GROUPS["blu_fused_grid"]:
        assert (b - 1) * fc.padded(n) // fc.F32_TILE_POINTS <= fc.F32_RX_GRID
    # the direct DFT at every length it serves, two full groups and a ragged one
    assert [n for n, _, _ in fc.F32_GROUPS["direct_every_length"]] == [n for n in range(3, 64) if n & (n - 1)]
    assert len(fc.F32_GROUPS["direct_every_length"]) == 57
    for n, (b,), _ in fc.F32_GROUPS["direct_every_length"]:
        assert fc.family_f32(n) == "direct" and b == 2 * (256 // n) + 1


def test_fallback_cases_reach_the_forms_they_are_for():
    f = fc.FALLBACKS
    assert all(fc.family_f32(n).startswith(("pow2_rx", "blu_fused")) and fc.family_f32(n) != "pow2_rx32k" for n, _ in f["COMMS_FFT_NO_RX"][1])
    assert all(fc.family_f32(n) == "pow2_rx32k" for n, _ in f["COMMS_FFT_NO_RX32K"][1])
    assert all(fc.family_f32(n).startswith("pow2_cols") for n, _ in f["COMMS_FFT_NO_COLS"][1])
    assert all(fc.family_f32(n).startswith("blu_fused") for n, _ in f["COMMS_FFT_BLU_UNFUSED"][1])
    value, cases = f["COMMS_FFT_DIRECT_MAX"]
    assert all(fc.F32_DIRECT_MAX < n <= int(value) <= 4096 and n & (n - 1) for n, _ in cases)
    assert any(n <= 128 for n, _ in cases) and any(n > 128 for n, _ in cases)  # dft_small_kernel and dft_direct_kernel


def test_sizes_stay_small():
    """No case above ~6 M points of f32 or 2^23 points of f64 in one call, apart from the 2^24 power of two."""
    for n, batches, _ in fc.F32_CASES:
        assert n * max(batches) <= (1 << 24), (n, batches)
    for n, batches, _ in fc.F64_CASES:
        assert n * max(batches) <= (1 << 23), (n, batches)
