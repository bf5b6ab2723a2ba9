"""The f64 timing estimator and the NCO (csrc/demod.hip) at their tile, pass and scan seams, on the full grid.  Inputs,
references and bounds are tests/demod_ref.py's; tests/test_demod_ref.py holds them to their conditions without a GPU.

NCO: every output against the exact int64 / np.longdouble phase at 1e-9 (small shapes in full; past the grid at every tile
seam and at random places, plus out[i] conj(out[i-1]) and |out[i]| over the whole length on the device); outputs bit for bit
the same however the stream is cut into calls; argument refusals that leave the phase alone.

Timing estimator: filters of one tap to three passes, blocks on n d, n d + 1 and the tile multiples, shaped QPSK under noise
and sparse impulses on the tile edges, against the oracle at the angle the existing tests hold n = 10 to.

Largest distances seen on an MI355X: NCO 1.0e-12 from the exact values on the small shapes (the negative dphase, which
Nco::new wraps by fl(2 pi) with one rounding: ~2.4e-16 a sample; 5e-16 with the positive one), 8.3e-15 past the grid, adjacent
ratio 4.7e-16, modulus 2.2e-16; timing estimate 1.4e-12 rad of the sum (bound 6.28e-10)."""
import re

import numpy as np
import pytest

import demod_ref as dr

pytestmark = pytest.mark.gpu

ERR_ARG = 1   # COMMS_ERR_ARG


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    return c


def fields(name):
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}


def new_nco(c, d, p0):
    return c.NcoNode(float(dr.rad(d)), float(dr.rad(p0)))


def phase_distance(node, k_end):
    return abs(np.exp(1j * node.phase) - dr.rotor_exact(np.array([k_end]))[0])


# ------------------------------------------------------------------ NCO
def test_nco_small_shapes_against_the_exact_phase(c):
    """Largest distance seen: 1.0e-12 (n = 4097 with the negative dphase)."""
    worst = 0.0
    for name, d, p0, e in dr.small_cases():
        node = new_nco(c, d, p0)
        assert fields(node.kernel(e.size))["tiles"] == -(-e.size // dr.TILE)
        got = node.run(dr.rad(e))
        want, k_end = dr.nco_exact(p0, d, e)
        err = max(float(np.max(np.abs(got - want))), phase_distance(node, k_end))
        worst = max(worst, err)
        assert got.shape == want.shape and err <= dr.NCO_TOL, (name, err)
    print("NCO small shapes: largest distance from the exact values %.3e (tolerance %.0e)" % (worst, dr.NCO_TOL))


@pytest.mark.parametrize("kind", dr.KINDS)
def test_nco_outputs_do_not_depend_on_how_the_stream_is_cut(c, kind):
    d, p0, e = dr.cut_stream(kind)
    x = dr.rad(e)
    whole = new_nco(c, d, p0)
    uncut = whole.run(x)
    want, k_end = dr.nco_exact(p0, d, e)
    assert float(np.max(np.abs(uncut - want))) <= dr.NCO_TOL
    for name, cuts in dr.CUTS.items():
        node = new_nco(c, d, p0)
        edges = [0] + list(cuts) + [x.size]
        got = np.concatenate([node.run(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
        assert got.tobytes() == uncut.tobytes(), (kind, name, int(np.flatnonzero(got != uncut)[0]))
        assert node.phase == whole.phase, (kind, name)
    assert phase_distance(whole, k_end) <= dr.NCO_TOL


def check_device_block(torch, out, perr, dphase, idx, want):
    """The absolute check at idx, and over the whole length on the device: adjacent ratio and modulus."""
    got = out[torch.from_numpy(idx).cuda()].cpu().numpy()
    err = float(np.max(np.abs(got - want)))
    step = torch.polar(torch.ones_like(perr[1:]), perr[1:] + dphase)
    ratio = float(torch.max(torch.abs(out[1:] * torch.conj(out[:-1]) - step)))
    modulus = float(torch.max(torch.abs(torch.abs(out) - 1.0)))
    return err, ratio, modulus


def test_nco_past_the_grid(c):
    """8 * 256 + 3 tiles and five samples of varying errors, most of them several turns: every workgroup of the sum and apply kernels takes a
    second tile.  Largest distances seen: 8.3e-15 from the exact values, ratio 4.7e-16, modulus 2.2e-16."""
    import torch

    d, p0, e = dr.big_stream()
    n = e.size
    perr = torch.from_numpy(dr.rad(e)).cuda()
    out = torch.empty(n, dtype=torch.complex128, device="cuda:0")
    node = new_nco(c, d, p0)
    k = fields(node.kernel(n))
    assert k["tiles"] == dr.GRID + 4 and k["grid"] == dr.GRID and k["scan_sweeps"] == 1
    node.run_dev(perr.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    idx = dr.seam_indices(n)
    want, k_end = dr.nco_exact(p0, d, e, idx)
    err, ratio, modulus = check_device_block(torch, out, perr, float(dr.rad(d)), idx, want)
    print("NCO past the grid: %d samples, %d checked absolutely: %.3e from the exact values (tolerance %.0e); adjacent ratio off by %.3e, "
          "modulus by %.3e (tolerance %.0e)" % (n, idx.size, err, dr.NCO_TOL, ratio, modulus, dr.RATIO_TOL))
    assert err <= dr.NCO_TOL and phase_distance(node, k_end) <= dr.NCO_TOL
    assert ratio <= dr.RATIO_TOL and modulus <= dr.RATIO_TOL


def test_nco_refusals_leave_the_phase_alone(c):
    d, p0, e = dr.D_POS, dr.P_QUARTER, dr.nco_errors("large", 2 * dr.TILE + 3, 700)
    n = e.size
    x = dr.rad(e)
    want, k_end = dr.nco_exact(p0, d, np.concatenate([e, e]))
    node = new_nco(c, d, p0)
    d_in, d_out = c.DeviceBuf(8 * n + 16).upload(x), c.DeviceBuf(16 * n + 16)
    both = c.DeviceBuf(24 * n + 32).upload(x)
    assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0 and both.ptr % 16 == 0

    def refused(perr_ptr, count, out_ptr):
        before = node.phase
        with pytest.raises(c.CommsError) as err:
            node.run_dev(perr_ptr, count, out_ptr)
        assert err.value.code == ERR_ARG, err.value
        assert node.phase == before

    for call in range(2):
        refused(d_in.ptr + 8, n - 1, d_out.ptr)             # d_perr at 8 mod 16
        refused(d_in.ptr, n, d_out.ptr + 8)                 # d_out at 8 mod 16
        refused(both.ptr, n, both.ptr + 16)                 # the output begins inside the input
        refused(both.ptr + 16 * n - 16, n, both.ptr)        # the input begins inside the output
        refused(0, n, d_out.ptr)                            # NULL with n > 0
        refused(d_in.ptr, n, 0)
        node.run_dev(d_in.ptr, n, d_out.ptr)
        _ = node.phase                                      # synchronises
        got = d_out.download(np.complex128, n)
        assert float(np.max(np.abs(got - want[call * n: (call + 1) * n]))) <= dr.NCO_TOL, call
    node.run_dev(0, 0, 0)                                   # an empty call takes NULL
    assert phase_distance(node, k_end) <= dr.NCO_TOL


# ------------------------------------------------------------------ timing estimator
@pytest.mark.parametrize("n,d", dr.FILTERS)
def test_timing_filter_and_block_lengths(c, n, d):
    """Largest angle seen over all filters: 1.4e-12 rad, at (n, d) = (1, 509) (bound 6.28e-10)."""
    node = c.TimingEstimatorNode(n, d, dr.ALPHA)
    k = fields(node.kernel(dr.TILE + 1))
    assert k["taps"] == 2 * n * d + 1 and k["filter_passes"] == len(dr.pass_lengths(n, d)) and k["tile"] == dr.TILE and k["tiles"] == 2
    worst = 0.0
    for kind in dr.KINDS_T:
        for ln in dr.block_lengths(n, d):
            x = dr.timing_block(kind, n, d, ln)
            want = dr.timing_reference(kind, n, d, ln)
            got = node.run(x)
            if ln <= n * d:                                   # no product: the oracle's -0.0
                assert got == 0.0 and np.signbit(got) == np.signbit(want), (kind, ln, got, want)
            else:
                err = dr.angle_error(got, want, n)
                worst = max(worst, err)
                assert err <= dr.ANGLE_TOL, (kind, n, d, ln, got, want, err)
            assert np.float64(node.run(x)).tobytes() == np.float64(got).tobytes(), (kind, ln)     # fresh state on every push
            if ln:                                            # the device entry: the host entry's bits
                buf = c.DeviceBuf(16 * ln).upload(x)
                assert np.float64(node.run_dev(buf.ptr, ln)).tobytes() == np.float64(got).tobytes(), (kind, ln)
    print("timing n=%d d=%d (%d taps, passes %s): largest angle from the oracle %.3e rad (bound %.3e)"
          % (n, d, 2 * n * d + 1, dr.pass_lengths(n, d), worst, dr.ANGLE_TOL))


def test_timing_refusals_do_not_disturb_the_next_push(c):
    n, d = 10, 51                                             # two passes: the qacc scratch is in use
    ln = 2 * dr.TILE + n * d + 1
    x = dr.timing_block("qpsk", n, d, ln)
    node = c.TimingEstimatorNode(n, d, dr.ALPHA)
    buf = c.DeviceBuf(16 * ln + 16).upload(x)
    first = node.run_dev(buf.ptr, ln)
    assert dr.angle_error(first, dr.timing_reference("qpsk", n, d, ln), n) <= dr.ANGLE_TOL
    for ptr, count in ((buf.ptr + 8, ln - 1), (0, ln)):       # 8 mod 16; NULL with len > 0
        with pytest.raises(c.CommsError) as err:
            node.run_dev(ptr, count)
        assert err.value.code == ERR_ARG, err.value
        assert np.float64(node.run_dev(buf.ptr, ln)).tobytes() == np.float64(first).tobytes()
    empty = node.run_dev(0, 0)                                # an empty push takes NULL
    assert empty == 0.0 and np.signbit(empty)
