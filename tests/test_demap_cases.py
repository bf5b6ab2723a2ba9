"""tests/demap_cases.py held to its rules, and on its tables the contract's choice of the split and the per-axis identities of
demap_axis_kernel against the brute-force definition (tests/symmap_ref.py) at all 44 splits.  What is asserted about the inputs
are conditions the GPU test rests on, not measurements of a kernel.  No GPU."""
import numpy as np
import pytest

import demap_cases as dc
import symmap_ref as sr

f32 = np.float32
N_IDENTITY = 2048
TINY = np.finfo(f32).tiny                      # 2^-126, the smallest normal


def levels_of(table, split):
    mI, mQ = split
    return table.real[: 1 << mI].copy(), table.imag[np.arange(1 << mQ) << mI].copy()


def check_identities(name, table, split, z):
    mI, mQ = split
    pI, pQ = levels_of(table, split)
    assert sr.same_floats(sr.axis_llr(z, mI, pI, pQ, dc.LLR_SCALE), sr.ref_llr(z, table, dc.LLR_SCALE)), name
    want = sr.ref_index(z, table)
    assert np.array_equal(sr.axis_index(z, mI, pI, pQ), want), name
    return int(np.count_nonzero(sr.naive_axis_index(z, mI, pI, pQ) != want))


# ------------------------------------------------------------------ the case table itself
def test_there_is_a_table_for_every_split_and_no_name_twice():
    assert len(dc.SPLITS) == len(set(dc.SPLITS)) == 44
    assert set(dc.SPLITS) == {(i, m - i) for m in range(1, 9) for i in range(m + 1)}
    t = dc.tables()
    assert len(t) == 44 + 1 + len(dc.ambiguous()) + len(dc.scaled())
    for name, (m, table, split) in t.items():
        assert table.dtype == np.complex64 and table.shape == (1 << m,) and np.isfinite(table.view(f32)).all(), name
        assert split is None or sum(split) == m, name
    assert {t[dc.split_name(*s)][0] for s in dc.SEP7} == {7} and t["rand7"][0] == 7
    assert sorted(m for m, _, _ in dc.ambiguous().values() if m in (3, 4, 7))[-1] == 7


@pytest.mark.parametrize("mI,mQ", dc.SPLITS)
def test_split_tables_have_distinct_unordered_levels(mI, mQ):
    pI, pQ = dc.split_levels(mI, mQ)
    for p, k, step in ((pI, mI, 0.375), (pQ, mQ, 0.5)):
        assert p.dtype == f32 and p.size == 1 << k == np.unique(p).size
        assert np.all(np.diff(np.sort(p)) == step)                             # a ladder, exact in f32, its own step per axis
        assert not np.array_equal(np.sort(-p), np.sort(p))                     # not symmetric
        order = np.argsort(p)                                                  # the indices from the lowest level up
        if k >= 3:                                                             # neighbours more than one bit apart: not Gray
            assert any(bin(int(a) ^ int(b)).count("1") != 1 for a, b in zip(order[:-1], order[1:]))
    table = dc.split_table(mI, mQ)
    assert np.unique(table).size == table.size


# ------------------------------------------------------------------ the choice of the split
@pytest.mark.parametrize("mI,mQ", dc.SPLITS)
def test_the_only_separable_split_is_found(mI, mQ):
    table = dc.split_table(mI, mQ)
    got = sr.find_split(table)
    pI, pQ = dc.split_levels(mI, mQ)
    assert got is not None and got[0] == mI and got[1].tobytes() == pI.tobytes() and got[2].tobytes() == pQ.tobytes()
    m, v = mI + mQ, np.arange(table.size)
    for k in range(m + 1):                                                     # no other split holds
        holds = np.array_equal(table.real, table.real[v & ((1 << k) - 1)]) and np.array_equal(table.imag, table.imag[(v >> k) << k])
        assert holds == (k == mI), (mI, mQ, k)


@pytest.mark.parametrize("name", list(dc.ambiguous()))
def test_the_contracts_choice_among_several_splits(name):
    m, table, split = dc.ambiguous()[name]
    got = sr.find_split(table)
    v = np.arange(table.size)
    holding = [k for k in range(m + 1)
               if np.array_equal(table.real, table.real[v & ((1 << k) - 1)]) and np.array_equal(table.imag, table.imag[(v >> k) << k])]
    if split is None:
        assert got is None and not holding
        assert np.unique(table).size < table.size                              # repeated points
        return
    assert len(holding) > 1, "the table is meant to leave a choice"
    cost = {k: (1 << k) + (1 << (m - k)) for k in holding}
    assert split[0] == min(holding, key=lambda k: (cost[k], k))                # the hand-written split is the contract's
    assert got is not None and (got[0], m - got[0]) == split
    rebuilt = sr.separable_table(got[1], got[2])
    assert np.array_equal(rebuilt, table)                                      # (as floats: +0.0 == -0.0)


def test_the_ambiguous_tables_are_the_kinds_asked_for():
    a = dc.ambiguous()
    assert [a["equal%d" % m][2][0] for m in (3, 4, 7)] == [1, 2, 3]
    for m in (3, 4, 7):
        assert np.unique(a["equal%d" % m][1]).size == 1
    pI, pQ = levels_of(a["repeat22"][1], a["repeat22"][2])
    assert pI.tolist() == [1, -1, 1, -1] and pQ.tolist() == [2, 2, -2, 0.5]
    z = a["zero_signs"][1]
    assert set(np.signbit(z.real).tolist()) == {True, False} and not z.real.any()
    pI, _ = levels_of(z, (1, 2))
    assert pI.view(np.uint32).tolist() == [0, 0x80000000]                      # one level, once as +0.0 and once as -0.0
    assert sr.find_split(a["repeated_points"][1]) is None


# ------------------------------------------------------------------ the per-axis identities
@pytest.mark.parametrize("mI,mQ", dc.SPLITS)
def test_per_axis_identities_equal_the_brute_force_at_every_split(mI, mQ):
    table = dc.split_table(mI, mQ)
    wrong = check_identities((mI, mQ), table, (mI, mQ), sr.demap_input(table, N_IDENTITY, 100 * mI + mQ))
    print("split (%d,%d): the naive per-axis argmin differs in %d of %d" % (mI, mQ, wrong, N_IDENTITY))
    if mI >= 1 and mQ >= 1:
        assert wrong > 0, "the input no longer catches a naive per-axis argmin"


@pytest.mark.parametrize("name", [n for n, (_, _, s) in {**dc.ambiguous(), **dc.scaled()}.items() if s is not None])
def test_per_axis_identities_on_ambiguous_and_scaled_tables(name):
    m, table, split = dc.tables()[name]
    check_identities(name, table, split, sr.demap_input(table, N_IDENTITY, 7 + m))


# ------------------------------------------------------------------ conditions on the inputs of the GPU test
def gpu_input(name):
    m, table, _ = dc.tables()[name]
    return table, np.concatenate([dc.case_input(table, F, frames) for F in dc.lengths(m) for frames in dc.FRAME_COUNTS])


@pytest.mark.parametrize("name", list(dc.tables()))
def test_half_of_every_input_has_finite_llrs(name):
    table, z = gpu_input(name)
    finite = np.isfinite(sr.ref_llr(z, table, dc.LLR_SCALE)).all(axis=1)
    assert 2 * np.count_nonzero(finite) >= z.size, (name, np.count_nonzero(finite), z.size)
    assert not finite.all()                                                    # and the other kind is there too


def flushed_llr(z, table, scale):
    """symmap_ref.ref_llr with every subnormal product dx dx, dy dy taken as zero: what a build that flushed f32 denormals
    would compute at best."""
    c = np.asarray(table, np.complex64)
    m = c.size.bit_length() - 1
    with np.errstate(all="ignore"):
        dx = z.real.astype(f32)[:, None] - c.real[None, :]
        dy = z.imag.astype(f32)[:, None] - c.imag[None, :]
        xx, yy = (dx * dx).astype(f32), (dy * dy).astype(f32)
        xx[np.abs(xx) < TINY] = 0
        yy[np.abs(yy) < TINY] = 0
        d = (xx + yy).astype(f32)
        i = np.arange(c.size)
        out = np.zeros((z.size, m), f32)
        for b in range(m):
            d0, _ = sr._scan_min(d[:, ((i >> b) & 1) == 0])
            d1, _ = sr._scan_min(d[:, ((i >> b) & 1) == 1])
            out[:, b] = f32(scale) * (d1 - d0).astype(f32)
    return out


@pytest.mark.parametrize("name", ["sep_small", "rand_small"])
def test_small_tables_put_subnormals_into_the_llrs(name):
    table, z = gpu_input(name)
    d = sr.distances(z, table)
    sub = (d != 0) & (np.abs(d) < TINY)
    assert sub.any() and np.count_nonzero(sub.any(axis=1)) >= z.size // 4
    want = sr.ref_llr(z, table, dc.LLR_SCALE)
    unit = dc.scaled_by(table, -dc.SMALL_EXP)                                  # at the unit scale flushing changes nothing
    z1 = sr.demap_input(unit, 512, 3)
    assert sr.same_floats(flushed_llr(z1, unit, dc.LLR_SCALE), sr.ref_llr(z1, unit, dc.LLR_SCALE))
    changed = want.view(np.uint32) != flushed_llr(z, table, dc.LLR_SCALE).view(np.uint32)
    print("%s: %d of %d symbols have a subnormal distance, flushing changes %d of %d LLR words" %
          (name, np.count_nonzero(sub.any(axis=1)), z.size, np.count_nonzero(changed), changed.size))
    assert changed.any()
    assert np.count_nonzero(sr.ref_index(z, table)) > 0


@pytest.mark.parametrize("name", ["sep_large", "rand_large"])
def test_large_tables_keep_their_own_distances_finite(name):
    m, table, _ = dc.tables()[name]
    assert np.isfinite(sr.distances(table, table)).all() and np.abs(table).min() > 2.0 ** 30
    assert np.isfinite(sr.ref_llr(sr.noisy_points(table, 500, 1), table, dc.LLR_SCALE)).all()


def test_scaled_tables_are_exact_copies_of_the_unit_ones():
    s = dc.scaled()
    for tag, e in (("small", dc.SMALL_EXP), ("large", dc.LARGE_EXP)):
        for name, base in (("sep_", dc.split_table(*dc.SCALED_SPLIT)), ("rand_", sr.random_table(5, dc.SCALED_RAND_SEED))):
            t = s[name + tag][1].astype(np.complex128) * 2.0 ** -e
            assert np.array_equal(t, base.astype(np.complex128))
    assert sr.find_split(s["rand_small"][1]) is None and sr.find_split(s["rand_large"][1]) is None
    assert sr.find_split(dc.rand7()) is None


# ------------------------------------------------------------------ known decisions
@pytest.mark.parametrize("m", range(1, 9))
def test_pattern_symbols_decode_to_their_indices(m):
    table = dc.pack_table(m)
    assert np.unique(table).size == table.size and sr.find_split(table)[0] == m // 2
    Fs = dc.pack_lengths(m)
    assert Fs[:3] == [64, 65, 129] and Fs[3] * m % 32 == (31 if m % 2 else 32 - np.gcd(m, 32))
    mask = (1 << m) - 1
    for F in Fs:
        for kind in dc.PATTERNS:
            z, v = dc.pattern_symbols(table, F, kind)
            assert z.shape == v.shape == (F,) and np.array_equal(sr.ref_index(z, table), v), (m, F, kind)
            rec = dc.index_records(v, m, F)
            assert rec.shape == (1, sr.record_bytes(F * m)) and np.array_equal(rec, sr.ref_bits_records(z, table, F))
            bits = sr.unpack_records(rec, F * m)[0].reshape(F, m)
            if kind == "ones":
                assert bits.all() and not np.unpackbits(rec, axis=1, bitorder="little")[0, F * m:].any()
            elif kind == "zeros":
                assert not rec.any()
            elif kind == "alternate":
                assert set(v.tolist()) == {0x55 & mask, 0xAA & mask} and v[0] == 0x55 & mask and v[1] == 0xAA & mask
            else:
                assert (bits.sum(axis=1) == 1).all() and np.array_equal(np.argmax(bits, axis=1), np.arange(F) % m)


def test_lengths_reach_the_seams_and_three_chunks():
    for m in range(1, 9):
        Fs = dc.lengths(m)
        assert set(sr.demap_lengths(m)) <= set(Fs) and max(Fs) >= 129 and max(Fs) % 64
        for F in Fs:
            P = dc.weight_periods(F)
            assert P[0] == 1 and P[-1] == F and (F < 3 or 1 < P[1] < F)


def test_symbols_on_repeated_points_decide_for_the_first_of_them():
    """What the GPU test's run on the points themselves rests on: the definition's index of a point that occurs more than once
    (as floats, +0.0 == -0.0) is its lowest index."""
    for name, (m, table, _) in dc.ambiguous().items():
        first = np.array([int(np.flatnonzero(table == p)[0]) for p in table])
        assert np.array_equal(sr.ref_index(table, table), first), name
        assert (first != np.arange(table.size)).any(), name
