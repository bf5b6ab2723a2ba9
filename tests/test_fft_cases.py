"""The FFT case tables (tests/fft_cases.py) held to the rule they are drawn from: a case for every kernel family, every seam
case across its seam, and every threshold of the rule still in the source it restates.  No GPU."""
import os

import pytest

import fft_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thresholds_still_stand_in_the_source():
    """Each rule of family_f32 / family_f64 names the source text it restates; a threshold that moves takes its text along."""
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
