"""
GPU: okx_ensemble_reduce (DeviceProgram.reduce_ensemble) at the edges of its launch plan - tiles of 64 entries, slabs of geometries,
the four quarters of a slab, blocks of 8 / 16 / 32 factors - against ensemble_stats.reduce_host and EnsembleAccumulator.merge.

The cases, the tables and the placement of the ties are those of tests/test_ensemble_reduce_shapes.py, where reduce_host is pinned to an
int64 restatement on every one of them: the tables are integers whose sums fp64 holds exactly in every order, so every comparison
here is an equality (``np.array_equal`` per field).  The one exception is ``test_real_table_against_exact_sums``: sums of real values
against their exact rational sums, within the bounds derived in tests/test_ensemble_stats.py from the number format and the term
count, taken once.

Tables go up the way tests/test_gpu_ensemble_effects.py uploads them: values as a [G S, K] view of a [G S, K + 3] tensor padded with
NaN, the status byte as byte 32 of 40-byte records whose other bytes read "residual exceeded".  Accumulators are the middle of larger
tensors filled with a sentinel; the rows before and behind must keep it.

What each test is there for was checked by changing the kernels one value at a time (never an address) and running this file and
tests/test_gpu_ensemble_stats.py against each changed library:

  mutation                                                fails here                                                            fails in test_gpu_ensemble_stats.py
  (a) lane loop: v < mn -> v <= mn                        exact tables with G >= 5 (45 of 64), chunks (4 of 4), end of           test_full_size_ensemble only
                                                          allocation at G = 5, limits, real table
  (b) take_extreme's tie clause: i < held_i -> i > held_i exact tables with G >= 2 (49), chunks (4), end of allocation at        test_full_size_ensemble only
                                                          G = 2 and 5, limits, real table
  (c) quarter merge loop: kWaves - 1 -> kWaves - 2        exact tables (31: those with a fourth quarter), chunks (4), real     every test that reduces
                                                          table, status bytes
  (d) quarter rounded down                                exact tables (58), chunks (3), end of allocation (15), limits,         test_few_factors_at_the_end_of_their_allocation only
                                                          real table
  (e) merge ignores accumulate for the sum of squares     chunks (the three partitions of more than one chunk)                   test_full_size_ensemble only
  (f) partial's store guard: p < np -> p < np - 1         exact tables with P >= 1 (60), chunks (4), end of allocation (15),     few_factors, full size, the fixture
                                                          limits, real table
  (g) acceptance compares the whole status byte with 1    every test of the file: exact tables (64), chunks (4), end of          test_full_size_ensemble only
                                                          allocation (15), limits, real table, status bytes
  (h) entry_values: n_columns in place of ld              exact tables (60), chunks (4), end of allocation (15),                 test_strided_views_of_evaluation_rows only
                                                          limits, real table

(test_gpu_ensemble_stats.py was run without its two tests that start child processes.)  Four of the eight are caught there by
test_full_size_ensemble alone, a million-state run; here each is caught by tables of a few thousand doubles, with the failing field
and entry in the message.
"""

import numpy as np
import pytest
import torch

from conftest import gpu_available
from open_kinematics_amd.ensemble_stats import (ENS_ARGMAX, ENS_ARGMIN, ENS_COUNT, ENS_FIELDS, ENS_MAX, ENS_MIN, ENS_REJECTED, ENS_SUM, ENS_SUMSQ,
                                                EnsembleAccumulator, factor_moment_count, reduce_host)
from test_ensemble_reduce_shapes import (CASES, CHUNK_EDGES, CHUNK_OFFSET, CHUNK_SHAPE, CHUNK_TIES, OFFSET, REAL_SHAPE, case_id, case_tables, chunk_tables,
                                         host_chunks, integer_table, real_bounds, real_tables, tie_plan, within)
from test_ensemble_stats import U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL, OTHER = -12345.5, 54321.25  # (no accumulator of an integer table holds a half or a quarter)
FIELD_NAMES = ("count", "rejected", "sum", "sumsq", "min", "max", "argmin", "argmax")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def dp():
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.workloads import bump_sweep_problem

    program, _ = bump_sweep_problem(4)
    return DeviceProgram(program, DEV)


def upload(values, status, pad=3, stride=40):
    """The table with ``ld = K + pad`` and its status bytes ``stride`` apart, the rest filled with what must never be read as data."""
    g, s, k = values.shape
    wide = torch.full((g * s, k + pad), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :k] = torch.as_tensor(np.array(values).reshape(g * s, k), device=DEV)  # (np.array: a copy, the shared tables are read-only)
    st = None
    if status is not None:
        info = torch.full((g * s, stride), 2, dtype=torch.uint8, device=DEV)
        info[:, 32 % stride] = torch.as_tensor(np.array(status).reshape(-1), device=DEV)
        st = info[:, 32 % stride]
    return wide[:, :k], st


def on_device(table):
    return None if table is None else torch.as_tensor(np.array(table), device=DEV)


class Guarded:
    """An accumulator [S, K, 8 + P] (and its factor moments) as the middle of larger tensors filled with ``SENTINEL``."""

    ROWS, MOMENTS = 2, 64

    def __init__(self, s, k, p, shift):
        n = factor_moment_count(p)
        self.around = torch.full((s + 2 * self.ROWS, k, ENS_FIELDS + p), SENTINEL, dtype=torch.float64, device=DEV)
        self.around_moments = torch.full((n + 2 * self.MOMENTS,), SENTINEL, dtype=torch.float64, device=DEV) if p else None
        self.out = EnsembleAccumulator(self.around[self.ROWS : self.ROWS + s], on_device(shift), self.around_moments[self.MOMENTS : self.MOMENTS + n] if p else None)
        assert self.out.acc.is_contiguous()

    def fill(self, value):
        self.out.acc.fill_(value)
        if self.out.factor_acc is not None:
            self.out.factor_acc.fill_(value)

    def bits(self):
        torch.cuda.synchronize()
        moments = self.out.factor_acc
        return self.out.acc.view(torch.int64).clone(), None if moments is None else moments.view(torch.int64).clone()

    def same_bits(self, bits):
        mine = self.bits()
        return torch.equal(mine[0], bits[0]) and (bits[1] is None or torch.equal(mine[1], bits[1]))

    def untouched(self):
        """Everything, the accumulator too, still holds the sentinel."""
        torch.cuda.synchronize()
        return bool((self.around == SENTINEL).all()) and (self.around_moments is None or bool((self.around_moments == SENTINEL).all()))

    def guards_kept(self):
        torch.cuda.synchronize()
        r, m = self.ROWS, self.MOMENTS
        kept = bool((self.around[:r] == SENTINEL).all()) and bool((self.around[-r:] == SENTINEL).all())
        if self.around_moments is not None:
            kept = kept and bool((self.around_moments[:m] == SENTINEL).all()) and bool((self.around_moments[-m:] == SENTINEL).all())
        return kept


def assert_same(got: EnsembleAccumulator, want: EnsembleAccumulator, what=""):
    """Every field of ``acc``, all of ``factor_acc`` and the shift, by value."""
    torch.cuda.synchronize()
    a, b = got.numpy(), want.numpy()
    assert a.acc.shape == b.acc.shape
    for field in range(a.acc.shape[2]):
        name = FIELD_NAMES[field] if field < ENS_FIELDS else f"cross sum of factor {field - ENS_FIELDS}"
        bad = np.argwhere(a.acc[..., field] != b.acc[..., field])
        assert bad.size == 0, (what, name, bad[:6].tolist(), a.acc[..., field][tuple(bad[0])], b.acc[..., field][tuple(bad[0])])
    assert np.array_equal(a.shift, b.shift), what
    assert (a.factor_acc is None) == (b.factor_acc is None), what
    if a.factor_acc is not None:
        bad = np.flatnonzero(a.factor_acc != b.factor_acc)
        assert bad.size == 0, (what, "factor moments", bad[:6].tolist(), a.factor_acc[bad[:6]].tolist(), b.factor_acc[bad[:6]].tolist())


# ---- every case, exactly ----

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exact_integer_tables(dp, case):
    g, s, k, p = case
    values, status, factors, shift, want = case_tables(case)
    v, st = upload(values, status)
    assert g * s == 1 or (v.stride(0) == k + 3 and st.stride(0) == 40)
    f = on_device(factors)
    held = Guarded(s, k, p, shift)
    got = dp.reduce_ensemble(v, steps_per_geometry=s, status=st, factors=f, geometry_offset=OFFSET, out=held.out)
    assert got is held.out
    assert_same(got, want, case_id(case))
    assert held.guards_kept()
    # again into the same tables, over another sentinel: the same bytes
    first = held.bits()
    held.fill(OTHER)
    dp.reduce_ensemble(v, steps_per_geometry=s, status=st, factors=f, geometry_offset=OFFSET, out=held.out)
    assert held.same_bits(first) and held.guards_kept()


# ---- the acceptance rule over every byte ----

def test_status_bytes(dp):
    g = 256
    rng = np.random.default_rng(256)
    status = np.arange(g, dtype=np.uint8).reshape(g, 1)
    values = rng.integers(-100, 101, (g, 1, 2)).astype(np.float64)
    values[0, 0, 0], values[255, 0, 0] = -1000.0, 1000.0  # the extremes of ALL rows stand under rejected bytes (0 and 255)
    values[1::2, 0, 1] = np.nan                           # column 1: every accepted byte is odd, so nothing of it counts
    shift = np.array([[3.0, -2.0]])
    ok_bytes = (np.arange(g) & 7) == 1
    assert ok_bytes.sum() == 32 and ok_bytes[[1, 9, 17, 33, 65, 129, 249]].all() and not ok_bytes[[0, 2, 3, 4, 5, 7, 131, 255]].any()
    v, st = upload(values, status)
    acc = dp.reduce_ensemble(v, steps_per_geometry=1, status=st, shift=shift, geometry_offset=OFFSET)
    assert_same(acc, reduce_host(values, status, None, shift, OFFSET))
    a = acc.numpy().acc[0]
    assert a[0, ENS_COUNT] == 32 and a[0, ENS_REJECTED] == g - 32 and a[1, ENS_COUNT] == 0 and a[1, ENS_REJECTED] == g
    assert a[1, ENS_ARGMIN] == -1 and a[1, ENS_ARGMAX] == -1 and a[1, ENS_MIN] == np.inf and a[1, ENS_MAX] == -np.inf
    column = np.where(ok_bytes, values[:, 0, 0], np.nan)
    for field, arg, best in ((ENS_MIN, ENS_ARGMIN, np.nanmin(column)), (ENS_MAX, ENS_ARGMAX, np.nanmax(column))):
        row = int(a[0, arg]) - OFFSET
        assert ok_bytes[row] and a[0, field] == best == values[row, 0, 0] and row == int(np.flatnonzero(column == best)[0])
    # no status bytes: every finite value counts
    plain = dp.reduce_ensemble(v, steps_per_geometry=1, shift=shift, geometry_offset=OFFSET)
    assert_same(plain, reduce_host(values, None, None, shift, OFFSET))
    b = plain.numpy().acc[0]
    assert b[0, ENS_COUNT] == g and b[1, ENS_COUNT] == g // 2 and b[1, ENS_REJECTED] == g // 2
    assert (b[0, ENS_ARGMIN], b[0, ENS_ARGMAX]) == (OFFSET, OFFSET + 255) and int(b[1, ENS_ARGMIN]) % 2 == 0


# ---- chunks ----

@pytest.mark.parametrize("edges", CHUNK_EDGES, ids=lambda e: "-".join(map(str, e)))
def test_chunks_accumulate_exactly(dp, edges):
    g, s, k, p = CHUNK_SHAPE
    values, status, factors, shift = chunk_tables()
    v, st = upload(values, status)
    f = on_device(factors)
    whole = dp.reduce_ensemble(v, steps_per_geometry=s, status=st, factors=f, shift=shift, geometry_offset=CHUNK_OFFSET)
    assert_same(whole, reduce_host(values, status, factors, shift, CHUNK_OFFSET), "one call")
    a = whole.numpy().acc
    for step, col, where in CHUNK_TIES:
        assert a[step, col, ENS_MIN] == -1024 and int(a[step, col, ENS_ARGMIN]) == CHUNK_OFFSET + where[0]
    plan = tie_plan(g, s, k)
    assert int(a[0, 0, ENS_ARGMIN]) == CHUNK_OFFSET + plan.lowest[0] and plan.lowest[-1] == g - 1  # (the tie at index 2^53 - 1 loses)
    chunks = list(zip(edges[:-1], edges[1:]))

    def run(order=1, onto=None, moments_once=False):
        held = Guarded(s, k, p, shift)
        if onto is not None:
            held.out.acc.copy_(onto.acc)
            held.out.factor_acc.copy_(onto.factor_acc)
        for i, (lo, hi) in enumerate(chunks[::order]):
            before = held.bits() if lo == hi else None
            dp.reduce_ensemble(v[lo * s : hi * s], steps_per_geometry=s, status=st[lo * s : hi * s], factors=f[lo:hi], geometry_offset=CHUNK_OFFSET + lo,
                               out=held.out, accumulate=onto is not None or i > 0, factor_moments=not (moments_once and i > 0))
            assert before is None or held.same_bits(before)  # the empty chunk changes nothing
        assert held.guards_kept()
        return held.out

    empty = EnsembleAccumulator.empty(s, k, p, shift)
    for what, order, onto, host_onto in (("ascending", 1, None, None), ("descending", -1, None, None), ("onto the neutral accumulator", 1, empty.to(DEV), empty)):
        got = run(order, onto)
        assert_same(got, whole, what)
        assert_same(got, host_chunks(values, status, factors, shift, edges, order, host_onto), what)
    # the factor moments taken with the first chunk only
    got = run(moments_once=True)
    lo, hi = chunks[0]
    first = reduce_host(values[lo:hi], status[lo:hi], factors[lo:hi], shift, CHUNK_OFFSET + lo)
    assert np.array_equal(got.numpy().acc, whole.numpy().acc) and np.array_equal(got.numpy().factor_acc, first.factor_acc)


# ---- real values against exact sums ----

def test_real_table_against_exact_sums(dp):
    g, s, k, p = REAL_SHAPE
    values, status, factors, shift, (s1, s2, cross) = real_tables()
    e1, e2, fe = real_bounds(values, status, factors, shift)
    v, st = upload(values, status)
    f = on_device(factors)
    acc = dp.reduce_ensemble(v, steps_per_geometry=s, status=st, factors=f, shift=shift, geometry_offset=OFFSET)
    torch.cuda.synchronize()
    got, host = acc.numpy(), reduce_host(values, status, factors, shift, OFFSET)
    for field in (ENS_COUNT, ENS_REJECTED, ENS_MIN, ENS_MAX, ENS_ARGMIN, ENS_ARGMAX):
        assert np.array_equal(got.acc[..., field], host.acc[..., field]), FIELD_NAMES[field]
    checks = [within(got.acc[..., ENS_SUM], s1, e1), within(got.acc[..., ENS_SUMSQ], s2, e2), within(got.acc[..., ENS_FIELDS:], cross, fe)]
    print("sum d, sum d^2, sum f d: (inside the bound, largest error / bound or the first miss and its bound)", checks)
    assert all(c[0] for c in checks), checks
    # (two roundings of the same sums of G terms: the bound of tests/test_gpu_ensemble_stats.py)
    assert got.factor_acc[-1] == g and np.allclose(got.factor_acc, host.factor_acc, rtol=0, atol=2 * (g + 1) * U * np.abs(host.factor_acc).max())
    again = dp.reduce_ensemble(v, steps_per_geometry=s, status=st, factors=f, shift=shift, geometry_offset=OFFSET)
    torch.cuda.synchronize()
    assert torch.equal(again.acc.view(torch.int64), acc.acc.view(torch.int64)) and torch.equal(again.factor_acc.view(torch.int64), acc.factor_acc.view(torch.int64))


# ---- the wide factor reads with few geometries ----

@pytest.fixture(scope="module")
def allocation():
    return torch.empty(32 * 1024 * 1024 // 8, dtype=torch.float64, device=DEV)  # (large enough to be an allocation of its own)


@pytest.mark.parametrize("g", [1, 2, 5])
@pytest.mark.parametrize("p", [1, 8, 17, 33, 100])
def test_factor_table_at_the_end_of_its_allocation(dp, allocation, g, p):
    """tests/test_gpu_ensemble_stats.py::test_few_factors_at_the_end_of_their_allocation with fewer geometries than a block has factors:
    the reads of a whole block must end inside the [G][P] table, which is the tail of its allocation."""
    s, k = 5, 3
    values, status, factors, shift = integer_table(g, s, k, p, 40 + 7 * g + p)
    tail = allocation[allocation.numel() - g * p :].view(g, p)
    tail.copy_(torch.as_tensor(np.array(factors)))
    assert tail.data_ptr() + 8 * g * p == allocation.data_ptr() + 8 * allocation.numel()
    v, st = upload(values, status)
    acc = dp.reduce_ensemble(v, steps_per_geometry=s, status=st, factors=tail, shift=shift, geometry_offset=5)
    assert_same(acc, reduce_host(values, status, factors, shift, 5))


# ---- the limits ----

def test_limits_launch_nothing(dp):
    g, s, k, p = 5, 3, 3, 4
    values, status, factors, shift = integer_table(g, s, k, p, 53)
    plan = tie_plan(g, s, k)
    assert plan.rejected_step == 1 and 2 not in plan.entries + [plan.lone_entry]
    values[g - 1, 0, 2], status[g - 1, 0] = 1024.0, 1  # entry 2: its maximum at the last geometry
    v, st = upload(values, status)
    f = on_device(factors)
    held, wide = Guarded(s, k, p, shift), Guarded(s, k, 1025, shift)
    kw = dict(steps_per_geometry=s, status=st)
    with pytest.raises(ValueError, match=r"geometry indices beyond 2\^53"):
        dp.reduce_ensemble(v, factors=f, geometry_offset=2 ** 53 + 1 - g, out=held.out, **kw)
    with pytest.raises(ValueError, match="at most 1024 factors"):
        dp.reduce_ensemble(v, factors=torch.zeros((g, 1025), dtype=torch.float64, device=DEV), out=wide.out, **kw)
    with pytest.raises(ValueError, match=r"factors must be \[G, P\]"):
        dp.reduce_ensemble(v, factors=f[: g - 1], out=held.out, **kw)
    with pytest.raises(ValueError, match="out must hold contiguous device tables"):
        dp.reduce_ensemble(v, factors=f[:, : p - 1], out=held.out, **kw)
    with pytest.raises(ValueError, match="accumulate=True needs"):
        dp.reduce_ensemble(v, factors=f, accumulate=True, **kw)
    assert held.untouched() and wide.untouched()
    # the last index a double holds exactly is allowed, and comes back exact
    low = 2 ** 53 - g
    got = dp.reduce_ensemble(v, factors=f, geometry_offset=low, out=held.out, **kw)
    assert_same(got, reduce_host(values, status, factors, shift, low))
    a = got.numpy().acc
    assert a[0, 2, ENS_MAX] == 1024 and int(a[0, 2, ENS_ARGMAX]) == 2 ** 53 - 1 and a[0, 2, ENS_ARGMAX] == float(2 ** 53 - 1)
    index = a[..., ENS_ARGMIN:ENS_FIELDS]
    assert np.all((index == -1) | ((index >= low) & (index < 2.0 ** 53) & (index == np.round(index))))
    assert held.guards_kept()
