"""
CPU: the shapes and tables tests/test_gpu_ensemble_reduce_shapes.py reaches okx_ensemble_reduce with, and the proof that what it
expects of them does not depend on the order ensemble_stats.reduce_host happens to add in.

The tables are integers (``integer_table``: values in [-1024, 1024], shift in [-8, 8], factors in [-256, 256], at most 1024
geometries), so |d| <= 1032 and every sum the accumulator holds - of d, d^2, f d, f, f f' - stays below 1024 * 1032^2 < 2^31, far below
2^53: each partial sum of each addition order is an integer fp64 holds exactly, and the device, the host and an int64 restatement must
agree to the last bit.  ``test_reduce_host_equals_the_integer_restatement`` pins reduce_host to that restatement on every case.

The shapes are chosen from the launch plan of the reduction (okx_ensemble.hip, enstable::slab_plan), restated here in ``slab_plan`` and
``quarters``: a lane owns one of 64 entries of a tile; the geometries are cut into slabs - as many as 512 workgroups over the tiles ask
for, none shorter than 16 geometries, equal lengths rounded up -; the four wavefronts of a workgroup take the four contiguous quarters of
a slab (rounded up, the last ones short or empty), wave 0 merges them and a second kernel merges the slabs.

Where the ties lie (``tie_plan``), in terms of that plan: the column minimum -1024 (no draw reaches it) stands at the first two
geometries of the first quarter that has two, and again at the table's last geometry; the column maximum 1024 at the first two
geometries of the NEXT quarter that has two, and again at the last geometry but one.  So the in-lane comparison, the merge of the
quarters in LDS and - from 17 geometries on, where the last geometry lies in another slab - the merge of the slabs each meet a tie,
and the expected index is the first of the pair.  Tables of fewer than five geometries have no quarter of two: the minimum stands at
geometry 0 and at the last one, the maximum at what is left between them.  The ties are planted in the first entry, the last entry and
entries 63 and 64 (the last lane of the first tile, the first of the second), those of the rejected step left out.
"""

import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

from open_kinematics_amd.ensemble_stats import (ENS_ARGMAX, ENS_ARGMIN, ENS_COUNT, ENS_FIELDS, ENS_MAX, ENS_MIN, ENS_REJECTED, ENS_SUM, ENS_SUMSQ,
                                                EnsembleAccumulator, clean_shift, reduce_host)
from test_ensemble_stats import cross_bound, sum_bounds

TILE, MIN_SLAB, WANT_GROUPS, WAVES = 64, 16, 512, 4  # okx_ensemble.hip: kTile, kMinSlab, kWantGroups, kWaves
OFFSET = 2 ** 40

ACCEPTED = np.array([1, 9, 17, 33, 65, 129, 249], dtype=np.uint8)      # low three bits == 1, any advisory bit
REJECTED = np.array([0, 2, 3, 4, 5, 7, 131, 255], dtype=np.uint8)

# ---- the cases (G, S, K, P): one axis at a time around the base ----

BASE = (33, 5, 13, 9)  # 65 entries: a second tile with ONE live lane; three slabs of 11 geometries
GEOMETRY_CASES = [(g, 5, 13, 9) for g in (1, 2, 3, 4, 5, 15, 16, 17, 33, 64, 65, 257, 1000)]
ENTRY_CASES = [(33, s, k, 9) for s, k in ((1, 1), (7, 9), (8, 8), (5, 13), (2, 65), (130, 1), (1, 130))]
FACTOR_CASES = [(g, 5, 13, p) for g in (1, 5, 33) for p in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100)] + [(3, 2, 3, 1024)]
TILE_CAPPED_CASES = [(40, 300, 64, 3), (40, 600, 64, 0)]  # 300 / 600 tiles: two slabs of 20, one slab of 40
CASES = list(dict.fromkeys(GEOMETRY_CASES + ENTRY_CASES + FACTOR_CASES + TILE_CAPPED_CASES))  # (the base and two more stand in several lists)


def case_id(case):
    return "G{}-S{}-K{}-P{}".format(*case)


def case_seed(case):
    g, s, k, p = case
    return 100000 * g + 1000 * s + 10 * k + p


# ---- the plan, restated ----

def slab_plan(g, n_entries):
    """``(n_slabs, slab_len)`` of a call over ``g`` geometries and ``n_entries`` entries."""
    tiles = max(1, -(-n_entries // TILE))
    slabs = max(1, min(-(-WANT_GROUPS // tiles), -(-g // MIN_SLAB)))
    slab_len = -(-g // slabs)
    return -(-g // slab_len), slab_len


def quarters(g, n_entries):
    """``[(first, end)]`` of the geometries every wavefront walks, ascending, the empty ones left out."""
    n_slabs, slab_len = slab_plan(g, n_entries)
    out = []
    for slab in range(n_slabs):
        g0, g1 = slab * slab_len, min(g, (slab + 1) * slab_len)
        quarter = -(-(g1 - g0) // WAVES)
        for wave in range(WAVES):
            a = min(g0 + wave * quarter, g1)
            b = min(a + quarter, g1)
            if b > a:
                out.append((a, b))
    return out


TiePlan = namedtuple("TiePlan", "entries lowest highest rejected_step lone_entry lone_geometry")


def tie_plan(g, s, k):
    """Where ``integer_table`` plants what (module docstring): the ``entries`` with ties, the geometries that hold the column's
    minimum (``lowest``) and maximum (``highest``, may be empty), ascending; the step every geometry rejects (S >= 2: the middle one,
    never the first or - from three steps on - the last); the entry with ONE accepted state and the geometry that has it (G >= 2 and
    an entry to spare)."""
    n = s * k
    rejected = None if s < 2 else (1 if s == 2 else s // 2)
    entries = [e for e in sorted({0, 63, 64, n - 1}) if e < n and (rejected is None or e // k != rejected)]
    pairs = [q for q in quarters(g, n) if q[1] - q[0] >= 2]
    if len(pairs) >= 2:
        lowest, highest = [pairs[0][0], pairs[0][0] + 1], [pairs[1][0], pairs[1][0] + 1]
    else:
        lowest, highest = [0], ([1] if g >= 3 else [])
    if g - 1 not in lowest + highest:
        lowest.append(g - 1)
    if highest and g - 2 not in lowest + highest:
        highest.append(g - 2)
    spare = [e for e in range(min(n, 4)) if e not in entries and (rejected is None or e // k != rejected)]
    lone = spare[0] if g >= 2 and spare else None
    return TiePlan(entries, sorted(lowest), sorted(highest), rejected, lone, g // 2)


# ---- the tables ----

def integer_table(g, s, k, p, seed):
    """``(values [G, S, K], status [G, S] uint8, factors [G, P], shift [S, K])``, integer-valued doubles: values in [-1024, 1024]
    (drawn in [-1023, 1023]; +-1024 are the planted extremes of ``tie_plan``), the shift in [-8, 8], the factors in [-256, 256].
    Seeded tampering: about 5 % of the values NaN and one more at a cell of its own, one +inf and one -inf (G >= 3) under accepted
    status bytes; status bytes from ``ACCEPTED``, about a fifth of them from ``REJECTED``; one whole step rejected (S >= 2); one entry
    with a single accepted state (G >= 2)."""
    rng = np.random.default_rng(seed)
    plan = tie_plan(g, s, k)
    shift = rng.integers(-8, 9, (s, k)).astype(np.float64)
    values = rng.integers(-1023, 1024, (g, s, k)).astype(np.float64)
    factors = rng.integers(-256, 257, (g, p)).astype(np.float64)
    values[rng.random((g, s, k)) < 0.05] = np.nan
    status = rng.choice(ACCEPTED, (g, s))
    bad = rng.random((g, s)) < 0.2
    status[bad] = rng.choice(REJECTED, int(bad.sum()))
    if plan.rejected_step is not None:
        status[:, plan.rejected_step] = rng.choice(REJECTED, g)

    def accept(i, step):
        if (status[i, step] & 7) != 1:
            status[i, step] = rng.choice(ACCEPTED)

    if plan.lone_entry is not None:
        step, col = divmod(plan.lone_entry, k)
        values[:, step, col] = np.nan
        values[plan.lone_geometry, step, col] = float(rng.integers(-1023, 1024))
        accept(plan.lone_geometry, step)
    for e in plan.entries:
        step, col = divmod(e, k)
        for where, v in ((plan.lowest, -1024.0), (plan.highest, 1024.0)):
            for i in where:
                values[i, step, col] = v
                accept(i, step)
    # one +inf, one -inf, one NaN at cells of their own: no planted extreme, not the lone entry, not the rejected step
    taken = set()
    for v in ([np.inf, -np.inf] if g >= 3 else []) + ([np.nan] if g * s * k >= 2 else []):
        for _ in range(10000):
            i, e = int(rng.integers(g)), int(rng.integers(s * k))
            step, col = divmod(e, k)
            if (i, e) in taken or e == plan.lone_entry or step == plan.rejected_step or (e in plan.entries and i in plan.lowest + plan.highest):
                continue
            taken.add((i, e))
            values[i, step, col] = v
            accept(i, step)
            break
        else:
            raise AssertionError("no free cell")
    return values, status, factors, shift


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case_tables(case):
    """``(values, status, factors or None, shift, reduce_host's accumulator at OFFSET)`` of a case, made once and read-only."""
    g, s, k, p = case
    values, status, factors, shift = frozen(*integer_table(g, s, k, p, case_seed(case)))
    want = reduce_host(values, status, factors if p else None, shift, OFFSET)
    frozen(want.acc, want.shift, *([want.factor_acc] if p else []))
    return values, status, factors if p else None, shift, want


def accepted(values, status):
    return np.isfinite(values) & ((status & 7) == 1)[:, :, None]


def integer_restatement(values, status, factors, shift, offset):
    """The accumulator from boolean and int64 arithmetic alone: ``(acc [S, K, 8 + P], factor_acc or None)`` as float64."""
    g, s, k = values.shape
    ok = accepted(values, status)
    d = np.where(ok, np.nan_to_num(values, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64) - shift.astype(np.int64)[None], 0)
    p = 0 if factors is None else factors.shape[1]
    acc = np.zeros((s, k, ENS_FIELDS + p), dtype=np.float64)
    count = ok.sum(axis=0)
    sums = [count, g - count, d.sum(axis=0), (d * d).sum(axis=0)]
    for field, table in zip((ENS_COUNT, ENS_REJECTED, ENS_SUM, ENS_SUMSQ), sums):
        assert table.dtype.kind in "iu" and np.abs(table).max() < 2 ** 40
        acc[..., field] = table
    some = ok.any(axis=0)
    for value, arg, masked, extreme in ((ENS_MIN, ENS_ARGMIN, np.where(ok, values, np.inf), np.min), (ENS_MAX, ENS_ARGMAX, np.where(ok, values, -np.inf), np.max)):
        best = extreme(masked, axis=0)
        first = np.argmax(masked == best[None], axis=0)  # the FIRST geometry that holds it
        acc[..., value] = best
        acc[..., arg] = np.where(some, offset + first, -1)
    if not p:
        return acc, None
    f = factors.astype(np.int64)
    cross = np.einsum("gsk,gp->skp", d, f)
    rows, cols = np.tril_indices(p)
    moments = np.concatenate([f.sum(axis=0), (f[:, rows] * f[:, cols]).sum(axis=0), [g]])
    assert cross.dtype == np.int64 and moments.dtype == np.int64 and max(np.abs(cross).max(), np.abs(moments).max()) < 2 ** 40
    acc[..., ENS_FIELDS:] = cross
    return acc, moments.astype(np.float64)


# ---- the chunked table and the real table of the GPU tests ----

CHUNK_SHAPE = (300, 5, 13, 9)
CHUNK_EDGES = [[0, 300], [0, 149, 300], [0, 1, 2, 130, 130, 300], [0, 64, 128, 192, 256, 300]]
CHUNK_OFFSET = 2 ** 53 - 300  # the last geometry's index is 2^53 - 1, the largest a double holds next to its neighbours
CHUNK_TIES = ((1, 2, (129, 130)), (3, 5, (200, 201)))  # (step, column, geometries): across the cut at 130, and inside a chunk of every partition


@functools.lru_cache(maxsize=None)
def chunk_tables():
    """The integer table of ``CHUNK_SHAPE`` with two more minimum ties (``CHUNK_TIES``), read-only."""
    g, s, k, p = CHUNK_SHAPE
    values, status, factors, shift = integer_table(g, s, k, p, 300)
    plan = tie_plan(g, s, k)
    for step, col, where in CHUNK_TIES:
        assert step != plan.rejected_step and step * k + col not in plan.entries + [plan.lone_entry]
        for i in where:
            values[i, step, col] = -1024.0
            status[i, step] = 1
    return frozen(values, status, factors, shift)


def host_chunks(values, status, factors, shift, edges, order=1, onto=None):
    """The host ``merge()`` of the per-chunk ``reduce_host`` results, the chunks taken in ``order`` (1 ascending, -1 descending)."""
    merged = onto
    for a, b in list(zip(edges[:-1], edges[1:]))[::order]:
        part = reduce_host(values[a:b], status[a:b], factors[a:b], shift, CHUNK_OFFSET + a)
        merged = part if merged is None else merged.merge(part)
    return merged


REAL_SHAPE = (257, 5, 13, 9)


@functools.lru_cache(maxsize=None)
def real_tables():
    """``(values, status, factors, shift, (sum d, sum d^2 [S, K], sum f d [S, K, P]) as Fractions)``: values 1e6 + normal * 10^uniform(-3, 3)
    per entry, the tampering of the integer table of the same shape (its status bytes, its NaN and infinities where it has them, its ties
    as 1e6 -+ 1e5), normal factors, the shift geometry 0.  d = values - shift is ONE fp64 rounding, the device's own; the sums of d,
    d d and f d are then taken exactly."""
    g, s, k, p = REAL_SHAPE
    tampered, status, _, _ = integer_table(g, s, k, p, 257)
    rng = np.random.default_rng(2570)
    values = 1e6 + rng.normal(size=(g, s, k)) * (10.0 ** rng.uniform(-3.0, 3.0, (s, k)))[None]
    values[~np.isfinite(tampered)] = tampered[~np.isfinite(tampered)]
    values[tampered == -1024.0], values[tampered == 1024.0] = 1e6 - 1e5, 1e6 + 1e5
    factors = rng.normal(size=(g, p))
    shift = clean_shift(values[0])
    d = np.where(accepted(values, status), values - shift[None], 0.0)
    exact = np.frompyfunc(Fraction, 1, 1)
    df, ff = exact(d), exact(factors)
    sums = (df.sum(axis=0), (df * df).sum(axis=0), np.stack([(df * ff[:, j][:, None, None]).sum(axis=0) for j in range(p)], axis=2))
    return frozen(values, status, factors, shift) + (sums,)


def real_bounds(values, status, factors, shift):
    """``(E1, E2, cross)`` of tests/test_ensemble_stats.py, ONCE: the reference is exact, and n u sum |t| bounds a sum of n terms
    in any order (Higham (4.4)), the device's slab-and-quarter order included."""
    ok = accepted(values, status)
    return sum_bounds(values, ok, shift) + (cross_bound(values, ok, shift, factors),)


def within(got, exact, bound):
    """|got - exact| <= bound elementwise, compared in rationals; the largest ratio for the record."""
    worst = 0.0
    for x, y, b in zip(np.asarray(got).reshape(-1), np.asarray(exact, dtype=object).reshape(-1), np.asarray(bound).reshape(-1)):
        err = abs(Fraction(float(x)) - y)
        if err > Fraction(float(b)):
            return False, float(err), float(b)
        worst = max(worst, float(err / Fraction(float(b))) if b > 0 else 0.0)
    return True, worst, None


# ---- the tests ----

def test_the_restated_plan_gives_the_slabs_the_shapes_were_chosen_for():
    n = 5 * 13
    assert slab_plan(33, n) == (3, 11) and slab_plan(17, n) == (2, 9) and slab_plan(65, n) == (5, 13)
    assert slab_plan(257, n) == (17, 16) and quarters(257, n)[-1] == (256, 257)         # a last slab of one geometry
    assert slab_plan(1000, n) == (63, 16) and 1000 - 62 * 16 == 8
    assert quarters(5, n) == [(0, 2), (2, 4), (4, 5)]                                   # quarters of 2, 2, 1, 0
    assert quarters(17, n) == [(0, 3), (3, 6), (6, 9), (9, 11), (11, 13), (13, 15), (15, 17)]  # slabs of 9 + 8
    assert [len(quarters(g, n)) for g in (1, 2, 3, 4)] == [1, 2, 3, 4]                  # fewer geometries than wavefronts
    assert slab_plan(40, 300 * 64) == (2, 20) and slab_plan(40, 600 * 64) == (1, 40)    # capped by the tile count, although G > 16
    assert slab_plan(256, 2) == (16, 16) and slab_plan(300, n) == (19, 16)
    assert (BASE in GEOMETRY_CASES and BASE in ENTRY_CASES and BASE in FACTOR_CASES) and len(CASES) == 13 + 7 + 46 + 2 - 4


def test_tie_plans():
    assert tie_plan(33, 5, 13) == ([0, 63, 64], [0, 1, 32], [3, 4, 31], 2, 1, 16)
    assert tie_plan(5, 5, 13)[1:3] == ([0, 1, 4], [2, 3]) and tie_plan(17, 5, 13)[1:3] == ([0, 1, 16], [3, 4, 15])
    assert [tie_plan(g, 5, 13)[1:3] for g in (1, 2, 3, 4)] == [([0], []), ([0, 1], []), ([0, 2], [1]), ([0, 3], [1, 2])]
    assert tie_plan(33, 2, 65)[0] == [0, 63, 64] and tie_plan(33, 2, 65).rejected_step == 1
    assert tie_plan(33, 1, 1) == ([0], [0, 1, 32], [3, 4, 31], None, None, 16)
    assert tie_plan(33, 130, 1)[0] == [0, 63, 64, 129] and tie_plan(33, 1, 130)[0] == [0, 63, 64, 129]
    for case in CASES:
        g, s, k, _ = case
        plan = tie_plan(g, s, k)
        assert plan.entries and not set(plan.lowest) & set(plan.highest) and max(plan.lowest + plan.highest) < g
        if g >= 5:  # a pair inside ONE quarter for each extreme, the minimum's third in another quarter
            for pair in (plan.lowest[:2], plan.highest[:2]):
                assert any(a <= pair[0] and pair[1] == pair[0] + 1 and pair[1] < b for a, b in quarters(g, s * k))
            assert plan.lowest[2] == g - 1 and not any(a <= plan.lowest[0] and g - 1 < b for a, b in quarters(g, s * k))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reduce_host_equals_the_integer_restatement(case):
    g, s, k, p = case
    values, status, factors, shift, want = case_tables(case)
    assert values.shape == (g, s, k) and status.shape == (g, s) and status.dtype == np.uint8 and shift.shape == (s, k)
    finite = values[np.isfinite(values)]
    assert np.array_equal(finite, np.round(finite)) and np.abs(finite).max(initial=0) <= 1024 and np.abs(shift).max() <= 8
    if p:
        assert factors.shape == (g, p) and np.array_equal(factors, np.round(factors)) and np.abs(factors).max() <= 256
    acc, moments = integer_restatement(values, status, factors, shift, OFFSET)
    for field in range(ENS_FIELDS):
        assert np.array_equal(want.acc[..., field], acc[..., field]), field
    assert np.array_equal(want.acc, acc) and np.array_equal(want.shift, shift)
    assert (want.factor_acc is None and moments is None) if not p else np.array_equal(want.factor_acc, moments)
    # the case is worth running
    plan = tie_plan(g, s, k)
    ok = accepted(values, status)
    if g * s * k >= 2:
        assert np.isnan(values).any()
    if g >= 3:
        assert (values == np.inf).sum() == 1 and (values == -np.inf).sum() == 1
        gi, si, _ = np.nonzero(np.isinf(values))
        assert np.all((status[gi, si] & 7) == 1)  # rejected for what they are, not for their status byte
    if g >= 5:  # bytes of both lists, the more of each the more states there are
        seen = set(status.reshape(-1).tolist())
        assert len(seen & set(ACCEPTED.tolist())) >= min(len(ACCEPTED), g * s // 16) >= 1
        assert len(seen & set(REJECTED.tolist())) >= min(len(REJECTED), g * s // 16) >= 1
        assert 0 < ok.sum() < ok.size and not set(np.unique(status).tolist()) - set(ACCEPTED.tolist()) - set(REJECTED.tolist())
    if plan.rejected_step is not None:
        r = plan.rejected_step
        assert not acc[r, :, ENS_COUNT].any() and np.all(acc[r, :, ENS_MIN] == np.inf) and np.all(acc[r, :, ENS_MAX] == -np.inf)
        assert np.all(acc[r, :, ENS_ARGMIN] == -1) and np.all(acc[r, :, ENS_ARGMAX] == -1) and np.all(acc[r, :, ENS_REJECTED] == g)
    if plan.lone_entry is not None:
        step, col = divmod(plan.lone_entry, k)
        assert acc[step, col, ENS_COUNT] == 1 and acc[step, col, ENS_ARGMIN] == acc[step, col, ENS_ARGMAX] == OFFSET + plan.lone_geometry
    assert g < 2 or s * k < 2 or plan.lone_entry is not None
    for e in plan.entries:  # each planted tie is the column's extreme, held by all its geometries, and the first of them is expected
        step, col = divmod(e, k)
        column = np.where(ok[:, step, col], values[:, step, col], np.nan)
        assert np.flatnonzero(column == np.nanmin(column)).tolist() == plan.lowest and acc[step, col, ENS_MIN] == -1024
        assert acc[step, col, ENS_ARGMIN] == OFFSET + plan.lowest[0]
        if plan.highest:
            assert np.flatnonzero(column == np.nanmax(column)).tolist() == plan.highest and acc[step, col, ENS_MAX] == 1024
            assert acc[step, col, ENS_ARGMAX] == OFFSET + plan.highest[0]


def test_the_issue_s_own_shapes():
    """(1, 1, 1, 1), (5, 7, 9, 33), (257, 5, 13, 64), (3, 2, 3, 1024) and (65, 10, 13, 17), the shapes the check was proposed with."""
    for g, s, k, p in ((1, 1, 1, 1), (5, 7, 9, 33), (257, 5, 13, 64), (3, 2, 3, 1024), (65, 10, 13, 17)):
        values, status, factors, shift = integer_table(g, s, k, p, 1)
        want = reduce_host(values, status, factors, shift, OFFSET)
        acc, moments = integer_restatement(values, status, factors, shift, OFFSET)
        assert np.array_equal(want.acc, acc) and np.array_equal(want.factor_acc, moments)


@pytest.mark.parametrize("edges", CHUNK_EDGES, ids=lambda e: "-".join(map(str, e)))
def test_host_chunks_merge_to_the_single_run_exactly(edges):
    values, status, factors, shift = chunk_tables()
    g, s, k, p = CHUNK_SHAPE
    whole = reduce_host(values, status, factors, shift, CHUNK_OFFSET)
    acc, moments = integer_restatement(values, status, factors, shift, CHUNK_OFFSET)
    assert np.array_equal(whole.acc, acc) and np.array_equal(whole.factor_acc, moments)
    for step, col, where in CHUNK_TIES:
        assert acc[step, col, ENS_MIN] == -1024 and acc[step, col, ENS_ARGMIN] == CHUNK_OFFSET + where[0]
    index = acc[..., ENS_ARGMIN:ENS_FIELDS][acc[..., ENS_ARGMIN:ENS_FIELDS] >= 0]
    assert index.min() == CHUNK_OFFSET and int(index.max()) < 2 ** 53 and (index.astype(np.int64) % 2 == 1).any()  # odd indices: all 53 bits in use
    for order, onto in ((1, None), (-1, None), (1, EnsembleAccumulator.empty(s, k, p, shift))):
        merged = host_chunks(values, status, factors, shift, edges, order, onto)
        assert np.array_equal(merged.acc, whole.acc) and np.array_equal(merged.factor_acc, whole.factor_acc)


def test_real_table_reference():
    """reduce_host itself against the exact sums, within the bounds the device is held to; the first sum against math.fsum."""
    values, status, factors, shift, (s1, s2, cross) = real_tables()
    e1, e2, fe = real_bounds(values, status, factors, shift)
    d = np.where(accepted(values, status), values - shift[None], 0.0)
    g, s, k, p = REAL_SHAPE
    for step in range(s):
        for col in range(k):
            assert Fraction(math.fsum(d[:, step, col])) == Fraction(float(s1[step, col]))  # fsum: the exact sum, rounded once
    host = reduce_host(values, status, factors, shift, 0)
    for got, exact, bound in ((host.acc[..., ENS_SUM], s1, e1), (host.acc[..., ENS_SUMSQ], s2, e2), (host.acc[..., ENS_FIELDS:], cross, fe)):
        assert within(got, exact, bound)[0]
    # a sum that squares before it shifts, or forgets the shift, misses by orders of magnitude
    ok = accepted(values, status)
    assert not within(np.where(ok, values * values, 0.0).sum(axis=0) - 2 * shift * np.where(ok, values, 0.0).sum(axis=0) + ok.sum(axis=0) * shift * shift, s2, e2)[0]
    assert not within(np.where(ok, values, 0.0).sum(axis=0), s1, e1)[0]
