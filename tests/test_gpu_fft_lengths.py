"""The f32 and f64 FFT nodes off their tuned sizes (-m gpu): every kernel family of tests/fft_cases.py at its edge lengths,
every batch loop past its first piece, the limits, and the fallback forms of the diagnostic build.

Reference: numpy's f64 FFT of the same input (the CPU suite ties numpy to the oracle), and the oracle itself for the first
transform where n <= 2048.  Measure: the relative L2 error of each transform, ||got_b - want_b|| / ||want_b||, maximised over
the batch -- one bad transform is named rather than averaged away.  Bounds: TOL = 1e-5 for f32 (test_gpu_parity.py) and
1e-12 for f64 (fft_f64.hip, test_gpu_f64_fft.py).  Each case prints its figure (pytest -s), both directions."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fft_cases as fc
import oracle
from test_gpu_parity import DIAG_LIB, ROOT, TOL, rand_c

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
DIRECTIONS = (False, True)


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def rand_z(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def reference(x, n, inverse):
    """numpy's f64 transform of every row, unnormalised in both directions (rustfft's convention)."""
    xr = np.asarray(x).astype(np.complex128).reshape(-1, n)
    return np.fft.ifft(xr, axis=1) * n if inverse else np.fft.fft(xr, axis=1)


def worst(got, want):
    """(largest relative L2 error of a transform, its index)."""
    got = np.asarray(got).astype(np.complex128).reshape(want.shape)
    d = np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    b = int(np.argmax(d))
    return float(d[b]), b


def check(family, n, batch, inverse, got, x, tol):
    want = reference(x, n, inverse)
    err, b = worst(got, want)
    print("%-18s n=%-8d batch=%-7d %s err=%.3e (transform %d)" % (family, n, batch, "inv" if inverse else "fwd", err, b))
    assert err <= tol, (family, n, batch, inverse, err, b)
    if 1 < n <= 2048:  # the oracle's own transform of the first one
        o = oracle.fft(np.ascontiguousarray(np.asarray(x).reshape(-1, n)[0]), inverse)
        e0, _ = worst(np.asarray(got).reshape(-1, n)[:1], o.astype(np.complex128).reshape(1, n))
        assert e0 <= tol, (family, n, batch, inverse, "oracle", e0)
    return err


def host_f32(c, n, batch, inverse, seed):
    x = rand_c(np.random.default_rng(seed), n * batch)
    got = c.FFTBatchNode(n, inverse).run(x)
    assert got.shape == (n * batch,)
    return check(fc.family_f32(n), n, batch, inverse, got, x, TOL)


def dev_f32(c, n, batch, inverse, seed, in_place):
    """Device-resident: out of place against numpy, then (where asked) in place, bitwise equal to the out-of-place result."""
    import torch

    total = n * batch
    x = torch.empty(total, dtype=torch.complex64, device="cuda:0")
    c.synth_iq_dev(x.data_ptr(), total, 0, seed)
    y = torch.full_like(x, float("nan"))  # a transform that is never written shows
    s = torch.cuda.current_stream().cuda_stream
    node = c.FFTBatchNode(n, inverse)
    node.run_dev(x.data_ptr(), total, y.data_ptr(), s)
    torch.cuda.synchronize()
    err = check(fc.family_f32(n), n, batch, inverse, y.cpu().numpy(), c.synth_iq(total, 0, seed), TOL)
    if in_place:
        node.run_dev(x.data_ptr(), total, x.data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(x), torch.view_as_real(y)), (n, batch, inverse, "in place differs")
    return err


def host_f64(c, n, batch, inverse, seed):
    x = rand_z(np.random.default_rng(seed), n * batch)
    got = c.FFTBatchNodeF64(n, inverse).run(x)
    assert got.dtype == np.complex128 and got.shape == (n * batch,)
    return check(fc.family_f64(n), n, batch, inverse, got, x, TOL64)


def dev_f64(c, n, batch, inverse, seed, in_place):
    import torch

    total = n * batch
    xh = rand_z(np.random.default_rng(seed), total)
    x = torch.from_numpy(xh).to("cuda:0")
    y = torch.full_like(x, float("nan"))
    s = torch.cuda.current_stream().cuda_stream
    node = c.FFTBatchNodeF64(n, inverse)
    node.run_dev(x.data_ptr(), total, y.data_ptr(), s)
    torch.cuda.synchronize()
    err = check(fc.family_f64(n), n, batch, inverse, y.cpu().numpy(), xh, TOL64)
    if in_place:
        node.run_dev(x.data_ptr(), total, x.data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(x), torch.view_as_real(y)), (n, batch, inverse, "in place differs")
    return err


def ids(cases):
    return ["%d" % n for n, _, _ in cases]


# ------------------------------------------------------------------ f32
def test_f32_direct_dft_every_length(c):
    """dft_small_kernel at every length it serves (57 of them), two full groups of G = 256 / n transforms and a ragged one."""
    for n, batches, _ in fc.F32_GROUPS["direct_every_length"]:
        for batch in batches:
            for inverse in DIRECTIONS:
                host_f32(c, n, batch, inverse, 1000 + n)


@pytest.mark.parametrize("n,batches,in_place", fc.F32_GROUPS["direct_grid_cap"], ids=ids(fc.F32_GROUPS["direct_grid_cap"]))
def test_f32_direct_dft_past_the_grid_cap(c, n, batches, in_place):
    """More groups than the 8 * kNumCU workgroups of the launch: every workgroup's second trip through the group loop."""
    for batch in batches:
        for inverse in DIRECTIONS:
            dev_f32(c, n, batch, inverse, 1100 + n, in_place)


@pytest.mark.parametrize("n,batches,in_place", fc.F32_GROUPS["blu_fused"], ids=ids(fc.F32_GROUPS["blu_fused"]))
def test_f32_fused_bluestein_edge_lengths_around_a_tile(c, n, batches, in_place):
    """Both edge lengths of every fused padded length M = 256 ... 16384, at batch counts below, one past and several past a
    tile's worth of padded transforms: the partly filled tile and the compacted m < n store."""
    for batch in batches:
        for inverse in DIRECTIONS:
            host_f32(c, n, batch, inverse, 1200 + n + batch)


@pytest.mark.parametrize("n,batches,in_place", fc.F32_GROUPS["blu_fused_grid"], ids=ids(fc.F32_GROUPS["blu_fused_grid"]))
def test_f32_fused_bluestein_more_tiles_than_workgroups(c, n, batches, in_place):
    for batch in batches:
        for inverse in DIRECTIONS:
            dev_f32(c, n, batch, inverse, 1300 + n, in_place)


@pytest.mark.parametrize("n,batches,in_place", fc.F32_GROUPS["blu_unfused"] + fc.F32_GROUPS["blu_unfused_large"],
                         ids=ids(fc.F32_GROUPS["blu_unfused"] + fc.F32_GROUPS["blu_unfused_large"]))
def test_f32_unfused_bluestein_every_padded_length(c, n, batches, in_place):
    """M = 2^15 (one pass), 2^16 ... 2^20 (four-step with work2), 2^21 ... 2^23 (gathered columns), 2^24 (three launches),
    each under blu_pre / blu_mul / blu_post."""
    for batch in batches:
        for inverse in DIRECTIONS:
            host_f32(c, n, batch, inverse, 1400 + n % 1000)


@pytest.mark.parametrize("n,batches,in_place", fc.F32_GROUPS["blu_chunk_seams"], ids=ids(fc.F32_GROUPS["blu_chunk_seams"]))
def test_f32_bluestein_second_chunk(c, n, batches, in_place):
    """batch * M > 2^24: the loop's `in + b0 * N`, `o + b0 * N` and the reuse of the work buffers by a second chunk, in each
    form of the loop body."""
    for batch in batches:
        for inverse in DIRECTIONS:
            dev_f32(c, n, batch, inverse, 1500 + n % 1000, in_place)


@pytest.mark.parametrize("n,batches,in_place", fc.F32_GROUPS["pow2"], ids=ids(fc.F32_GROUPS["pow2"]))
def test_f32_power_of_two_families(c, n, batches, in_place):
    for batch in batches:
        for inverse in DIRECTIONS:
            dev_f32(c, n, batch, inverse, 1600 + fc.ilog2(n), in_place)


def test_f32_refuses_above_2p23_and_leaves_nothing_behind(c):
    """fft_setup refuses before it builds a table: code 1 (the caller's data), no device memory kept (the chirp alone would
    be 64 MiB, the padded spectrum 256 MiB), and the next node works."""
    import torch

    c.FFTBatchNode(1000, False).run(rand_c(np.random.default_rng(1), 1000))  # (the library's one-off allocations first)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for inverse in DIRECTIONS:
        with pytest.raises(c.CommsError) as e:
            c.FFTBatchNode(fc.F32_REFUSED, inverse)
        assert e.value.code == 1
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (32 << 20), (free0, free1)
    assert fc.family_f32(fc.F32_REFUSED - 2).startswith("blu_three")  # (the longest accepted odd length is a family of the table)
    host_f32(c, 1000, 3, False, 1700)


# ------------------------------------------------------------------ f64
def test_f64_one_pass_every_size(c):
    """fft_f64_lds_kernel at every log2 N = 1 ... 12: two full workgroups of B transforms and a ragged one."""
    for n, batches, _ in fc.F64_GROUPS["one_pass"]:
        for batch in batches:
            for inverse in DIRECTIONS:
                host_f64(c, n, batch, inverse, 2000 + n)


@pytest.mark.parametrize("n,batches,in_place", fc.F64_GROUPS["four_step"], ids=ids(fc.F64_GROUPS["four_step"]))
def test_f64_four_step_every_size(c, n, batches, in_place):
    """log2 P = 13 ... 23: the split logN1 = (logP + 1) / 2 and the twiddle split h = logP / 2 of every size."""
    for batch in batches:
        for inverse in DIRECTIONS:
            host_f64(c, n, batch, inverse, 2100 + fc.ilog2(n))


@pytest.mark.parametrize("n,batch", [(n, b) for n, batches, _ in fc.F64_GROUPS["seams"] for b in batches])
def test_f64_second_piece_of_the_batch_loops(c, n, batch):
    """Four-step past 64 transforms (one and two further pieces), one pass past 2^20: out of place against numpy, then in
    place, bitwise equal."""
    for inverse in DIRECTIONS:
        dev_f64(c, n, batch, inverse, 2200 + batch % 1000, True)


@pytest.mark.parametrize("n,batches,in_place", fc.F64_GROUPS["seam_dft_sum"], ids=ids(fc.F64_GROUPS["seam_dft_sum"]))
def test_f64_dft_sum_second_launch(c, n, batches, in_place):
    for batch in batches:
        for inverse in DIRECTIONS:
            dev_f64(c, n, batch, inverse, 2300 + n, in_place)


def test_f64_dft_sum_lengths(c):
    for n, batches, _ in fc.F64_GROUPS["dft_sum"]:
        for batch in batches:
            for inverse in DIRECTIONS:
                host_f64(c, n, batch, inverse, 2400 + n)


F64_BLU = fc.F64_GROUPS["bluestein"] + fc.F64_GROUPS["bluestein_other_p"] + fc.F64_GROUPS["bluestein_large"]


@pytest.mark.parametrize("n,batches,in_place", F64_BLU, ids=ids(F64_BLU))
def test_f64_bluestein_every_padded_length(c, n, batches, in_place):
    for batch in batches:
        for inverse in DIRECTIONS:
            host_f64(c, n, batch, inverse, 2500 + n % 1000)


# ------------------------------------------------------------------ the fallback forms (diagnostic build, one process each)
CHILD = r'''
import sys; sys.path.insert(0, %r)
import numpy as np, comms_rs_amd as c
rng = np.random.default_rng(7)
for n, batch in %r:
    for inverse in (False, True):
        x = (rng.uniform(-1, 1, n * batch) + 1j * rng.uniform(-1, 1, n * batch)).astype(np.complex64)
        got = c.FFTBatchNode(n, inverse).run(x).astype(np.complex128).reshape(batch, n)
        xr = x.astype(np.complex128).reshape(batch, n)
        want = np.fft.ifft(xr, axis=1) * n if inverse else np.fft.fft(xr, axis=1)
        d = float(np.max(np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)))
        print("n=%%d batch=%%d %%s err=%%.3e" %% (n, batch, "inv" if inverse else "fwd", d))
        assert d <= %r, (n, batch, inverse, d)
print("ok")
'''


@pytest.mark.parametrize("selector", sorted(fc.FALLBACKS))
def test_f32_fallback_forms(selector):
    """The forms behind the diagnostic build's selectors -- what every A/B figure of NOTES.md was measured against.  A selector
    is read once per process: own process."""
    value, cases = fc.FALLBACKS[selector]
    env = dict(os.environ, COMMS_HIP_LIB=DIAG_LIB)  # kernel selectors exist in the diagnostic build only
    env[selector] = value
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, cases, TOL)], env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr
