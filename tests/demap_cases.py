"""The case table of the soft demapper's split and seven-bit tests: a separable table for every split mI + mQ = m of every
m = 1 ... 8 (the 44 instantiations of demap_axis_kernel), tables at seven bits per symbol, tables on which more than one split is
separable, tables with repeated levels and points, tables scaled by a large and by a small power of two, symbols that sit on
table points in the bit patterns that show a misplaced field of a packed record, and the lengths and inputs of every run.
tests/test_demap_cases.py (no GPU) holds this module to its rules; tests/test_gpu_demap_splits.py runs the kernels on it
against tests/symmap_ref.py's brute force.  Nothing here touches the library."""
import functools
from math import gcd

import numpy as np

import symmap_ref as sr

f32 = np.float32

# ------------------------------------------------------------------ a table for every split
SPLITS = [(mI, m - mI) for m in range(1, sr.MAX_BITS + 1) for mI in range(m + 1)]


def split_levels(mI, mQ):
    """(pI, pQ): 2^mI and 2^mQ distinct levels, each a seeded permutation of an arithmetic ladder -- step 3/8 around +1/16 on
    the real axis, step 1/2 around -1/8 on the imaginary one (every level exact in f32): not Gray-ordered, not symmetric."""
    rng = np.random.default_rng(1000 + 16 * mI + mQ)
    nI, nQ = 1 << mI, 1 << mQ
    pI = (rng.permutation(nI) - (nI - 1) / 2.0) * 0.375 + 0.0625
    pQ = (rng.permutation(nQ) - (nQ - 1) / 2.0) * 0.5 - 0.125
    return pI.astype(f32), pQ.astype(f32)


def split_table(mI, mQ):
    """The separable table of split_levels(mI, mQ).  Its levels are distinct, so (mI, mQ) is its only separable split."""
    return sr.separable_table(*split_levels(mI, mQ))


def split_name(mI, mQ):
    return "split_%d_%d" % (mI, mQ)


# ------------------------------------------------------------------ seven bits per symbol
RAND7_SEED = 47
SEP7 = ((3, 4), (4, 3))


def rand7():
    return sr.random_table(7, RAND7_SEED)


# ------------------------------------------------------------------ tables on which the choice of the split is a choice
def _all_equal(m):
    return np.full(1 << m, 0.5 - 0.25j, np.complex64)


def _zero_signs():
    """m = 3, (pI, pQ) = ((+-0.0), 4 distinct levels): the real part is +0.0 or -0.0 from point to point in no pattern.  Floats
    compare exactly (0.0 == -0.0), so the splits (0,3) and (1,2) hold and (1,2) has fewer levels; compared as bit patterns no
    split would hold.  The points v and v ^ 1 are at the same distance from everything: the lower index wins."""
    re = np.array([0.0, -0.0, -0.0, 0.0, 0.0, 0.0, -0.0, -0.0], f32)
    t = np.empty(8, np.complex64)                    # (re + 1j * im would add +0.0 to the real part: the signs would go)
    t.real, t.imag = re, np.array([0.75, -0.5, 1.5, -1.25], f32)[np.arange(8) >> 1]
    return t


def _repeated_points():
    """16 points with no structure, five of which repeat an earlier or a later one."""
    t = sr.random_table(4, 64).copy()
    t[5] = t[2]
    t[9] = t[2]
    t[14] = t[7]
    t[0] = t[11]
    t[15] = t[11]
    return t


@functools.lru_cache(maxsize=None)
def ambiguous():
    """name -> (m, table, the contract's split (mI, mQ) or None): the smallest 2^mI + 2^mQ among the separable splits, the lowest
    mI on a tie.  Worked out by hand here; test_demap_cases.py holds symmap_ref.find_split to it."""
    return {
        # every split is separable: 2 + 4 = 4 + 2 -> mI = 1; 4 + 4 -> mI = 2; 8 + 16 = 16 + 8 -> mI = 3
        "equal3": (3, _all_equal(3), (1, 2)),
        "equal4": (4, _all_equal(4), (2, 2)),
        "equal7": (7, _all_equal(7), (3, 4)),
        # pI has period 2 and pQ a repeated level: (1,3) with 2 + 8 levels and (2,2) with 4 + 4 are separable
        "repeat22": (4, sr.separable_table([1, -1, 1, -1], [2, 2, -2, 0.5]), (2, 2)),
        # built as (1,2) with pQ = (c, c, d, d): (2,1) is separable too, 2 + 4 = 4 + 2 -> mI = 1
        "tie12": (3, sr.separable_table([0.75, -1.25], [0.5, 0.5, -1.0, -1.0]), (1, 2)),
        # a constant real part: (0,4), (1,3), (2,2) are separable with 17, 10 and 8 levels
        "flat_re": (4, sr.separable_table([0.25, 0.25, 0.25, 0.25], [1.5, -0.5, 0.5, -1.5]), (2, 2)),
        "zero_signs": (3, _zero_signs(), (1, 2)),
        "repeated_points": (4, _repeated_points(), None),
    }


# ------------------------------------------------------------------ scaled tables
# Levels of order 1 times 2^-70: a squared difference between a symbol and a neighbouring point is of order 2^-140 ... 2^-146,
# below f32's smallest normal 2^-126 and above its smallest subnormal 2^-149.  Times 2^40: squared differences of order 2^86 and
# the adversarial set's symbols at up to 2^29 points' lengths, squared 2^140 -- beyond f32, which is the set's purpose, while
# every distance between the table's own points and the noisy half of the input stays finite.
SMALL_EXP, LARGE_EXP = -70, 40
SCALED_SPLIT = (2, 3)
SCALED_RAND_SEED = 55


def scaled_by(table, e):
    """table * 2^e, each component on its own: exact."""
    t = np.empty(len(table), np.complex64)
    t.real, t.imag = np.ldexp(table.real, e), np.ldexp(table.imag, e)
    return t


@functools.lru_cache(maxsize=None)
def scaled():
    """name -> (m, table, split or None)."""
    out = {}
    for tag, e in (("small", SMALL_EXP), ("large", LARGE_EXP)):
        out["sep_" + tag] = (5, scaled_by(split_table(*SCALED_SPLIT), e), SCALED_SPLIT)
        out["rand_" + tag] = (5, scaled_by(sr.random_table(5, SCALED_RAND_SEED), e), None)
    return out


@functools.lru_cache(maxsize=None)
def tables():
    """Every table of the module: name -> (m, table, split (mI, mQ) the library must choose or None for the table form)."""
    out = {split_name(mI, mQ): (mI + mQ, split_table(mI, mQ), (mI, mQ)) for mI, mQ in SPLITS}
    out["rand7"] = (7, rand7(), None)
    out.update(ambiguous())
    out.update(scaled())
    for _, t, _ in out.values():
        t.setflags(write=False)
    return out


# ------------------------------------------------------------------ lengths and inputs
LONG_F = 131        # two full 64-symbol chunks and a partial one
LLR_SCALE = 0.37    # not a power of two: the product rounds
FRAME_COUNTS = (1, 3)


def lengths(m):
    return sorted(set(sr.demap_lengths(m)) | {LONG_F})


def case_input(table, F, frames):
    """The symbols of one run of the GPU test: symmap_ref.demap_input, seeded by the shape."""
    return sr.demap_input(table, frames * F, 1000 * F + frames)


def weight_periods(F):
    """P = 1, one period between, P = F."""
    return sorted({1, (F + 2) // 3, F})


# ------------------------------------------------------------------ known decisions for the BITS packing
PATTERNS = ("ones", "zeros", "alternate", "walk")


def pattern_indices(m, F, kind):
    """(F,) point indices: all ones (2^m - 1), all zeros, the fields 0x55.. / 0xAA.. in turn, a single bit that walks through
    the field from symbol to symbol."""
    j = np.arange(F)
    mask = (1 << m) - 1
    if kind == "ones":
        return np.full(F, mask, np.int64)
    if kind == "zeros":
        return np.zeros(F, np.int64)
    if kind == "alternate":
        return np.where(j % 2 == 0, 0x55 & mask, 0xAA & mask).astype(np.int64)
    if kind == "walk":
        return (1 << (j % m)).astype(np.int64)
    raise ValueError(kind)


def pattern_symbols(table, F, kind):
    """(symbols (F,) complex64 exactly on table points, their indices (F,)).  With distinct points the decision is the index:
    the distance to that point is +0.0 and every other one is greater."""
    c = np.asarray(table, np.complex64)
    v = pattern_indices(c.size.bit_length() - 1, F, kind)
    return c[v].copy(), v


def index_records(v, m, F):
    """Point indices (frames * F,) -> the BITS records (frames, record bytes) that hold them."""
    v = np.asarray(v, np.int64).reshape(-1, F)
    bits = ((v[:, :, None] >> np.arange(m)) & 1).astype(np.uint8).reshape(v.shape[0], F * m)
    return sr.pack_records(bits)


def pack_table(m):
    """The table of the packing runs: distinct points, separable at (m // 2, m - m // 2)."""
    return split_table(m // 2, m - m // 2)


def pack_lengths(m):
    """F = 64 (whole words at every m), 65, 129, and the first F past 65 whose F m bits end as close below a word's end as m
    allows: one bit short where m is odd, gcd(m, 32) bits short otherwise."""
    short = next(F for F in range(66, 66 + 32) if F * m % 32 == 32 - gcd(m, 32))
    return [64, 65, 129, short]


# ------------------------------------------------------------------ several passes per lane at m = 7
PASS_F = 67
PASS_DISTINCT = 30000      # distinct input symbols; the stream repeats them
