"""
Sobol' indices of a pick-freeze ensemble, CPU: the family draw (ensemble_sample.FamilyPlan / families_host), the accumulator's NumPy
definition (ensemble_stats.sobol_host) against a plain-loop restatement on small-integer tables, the exact zeros the pick-freeze
structure forces, the finalization, chunk_pieces(align=) and the Sobol stage of ShardedEnsemble on the stand-in program of
tests/test_dist.py.

Integer tables: values - shift in [-8, 8] over at most 67 families, so every difference (<= 16), product (<= 256) and partial sum
(< 2^15) is an integer fp64 holds - every addition order gives the same bits and the comparisons are array_equal.
U = 2^-53; ``term_bound`` is the recursive-summation bound 2 (n + 1) U sum |term| over the host's own terms, for the real tables.
"""

import dataclasses
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from open_kinematics_amd import ensemble_sample as smp
from open_kinematics_amd import ensemble_stats as es
from open_kinematics_amd.ensemble_sample import GUARD_SIGN, IID, LHS, NORMAL, TRUNCATED, UNIFORM, FamilyPlan, SamplePlan, families_host, sample_host
from open_kinematics_amd.ensemble_stats import (SOBOL_COUNT, SOBOL_DROPPED, SOBOL_FIELDS, SobolAccumulator, sobol_host, sobol_terms)

U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def family_plan(z=6, n_families=5, *, stratify=IID, mixing=False, guard=True, seed=21, n_groups=None):
    """A family plan over ``z`` latents (kinds cycling): without ``mixing`` one coordinate per latent, with it 9 coordinates mixed from
    the latents.  Groups: latent ``i`` is in group ``i % D`` with ``D = min(3, z)``, and - from four latents on - the LAST latent is
    in no group (-1).  ``guard``: a SIGN guard on the first perturbed coordinate, whose nominal value is 0: about half the rows fail."""
    rng = np.random.default_rng(100 * z + 7)
    f = 9 if mixing else z
    p = (f + 2) // 3 + 1
    nominal = rng.normal(0.0, 50.0, (p, 3))
    coords = np.arange(f, dtype=np.int32)
    kind = np.asarray([(NORMAL, UNIFORM, TRUNCATED)[i % 3] for i in range(z)], dtype=np.int32)
    guards = ()
    if guard:
        nominal.reshape(-1)[0] = 0.0
        guards = ((GUARD_SIGN, 0, 1.0, 0.0),)
    plan = SamplePlan(nominal, coords, kind, 0.5 + 2.0 * rng.random(z), rng.normal(0.0, 1.0, (f, z)) if mixing else None,
                      None if mixing else 0.25 + rng.random(f), stratify, 0, seed, guards, 1)
    d = min(3, z) if n_groups is None else n_groups
    group = np.arange(z) % d
    if z >= 4:
        group[-1] = -1
    return FamilyPlan(plan, group, n_families)


# ---- the family draw ----

@pytest.mark.parametrize("stratify", [IID, LHS])
@pytest.mark.parametrize("mixing", [False, True])
def test_family_draw_properties(stratify, mixing):
    n = 23
    fp = family_plan(7, n, stratify=stratify, mixing=mixing)
    d, m, z = fp.n_groups, fp.family_size, fp.n_latents
    assert (d, m, fp.n_total) == (3, 5, n * 5) and fp.group[-1] == -1
    whole = families_host(fp)
    source = sample_host(fp.source_plan())
    assert fp.source_plan().n_total == 2 * n and fp.plan.n_total == 0
    # members 0 / 1 are rows 2 i / 2 i + 1 of the plain ensemble of 2 N rows, all four outputs
    for got, want in zip(whole, source):
        fam = got.reshape((n, m) + got.shape[1:])
        assert np.array_equal(fam[:, 0].view(np.uint8), want[0::2].view(np.uint8)) and np.array_equal(fam[:, 1].view(np.uint8), want[1::2].view(np.uint8))
    # an arbitrary unaligned range equals the slice of the whole
    for lo, hi in ((3, 3), (3, 4), (7, 58), (m * n - 1, m * n)):
        part = families_host(fp, lo, hi)
        assert all(np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b[lo:hi]) if b.dtype == np.float64 else b[lo:hi]) for a, b in zip(part, whole))
        assert all(a.shape[0] == hi - lo for a in part)
    lat = whole[1].reshape(n, m, z)
    a, b = lat[:, 0], lat[:, 1]
    assert not np.any(a == b)  # (two draws of a continuous variable)
    for j in range(d):
        inside = fp.group == j
        assert np.array_equal(bits(lat[:, 2 + j][:, inside]), bits(b[:, inside])) and np.array_equal(bits(lat[:, 2 + j][:, ~inside]), bits(a[:, ~inside]))
    never = fp.group == -1
    for member in (0, *range(2, m)):
        assert np.array_equal(bits(lat[:, member][:, never]), bits(a[:, never]))
    # a guard that fails sets bit 0, never changes the row; bits 4-7 stay 0
    flags = whole[3]
    assert set(np.unique(flags)) == {0, 1}
    free = families_host(FamilyPlan(dataclasses.replace(fp.plan, guards=()), fp.group, n))
    assert not free[3].any() and all(np.array_equal(bits(x), bits(y)) for x, y in zip(free[:3], whole[:3]))
    assert np.array_equal(flags == 1, ~(whole[0].reshape(n * m, -1)[:, 0] > 0.0))
    if stratify == LHS:  # A and B together are ONE Latin hypercube of the 2 N source rows
        keys = smp.stratum(fp.plan.seed, 2 * n, np.arange(2 * n, dtype=np.uint64)[:, None], np.arange(z, dtype=np.uint64)[None])
        assert all(sorted(keys[:, i].tolist()) == list(range(2 * n)) for i in range(z))


def test_family_plan_checks():
    fp = family_plan(6, 4)
    base = fp.plan
    with pytest.raises(ValueError, match="max_attempts is 2; a family is drawn once"):
        FamilyPlan(dataclasses.replace(base, max_attempts=2), fp.group, 4)
    with pytest.raises(ValueError, match=r"group 1 is -2, outside \[-1, 3\)"):
        FamilyPlan(base, [0, -2, 1, 2, 0, 1], 4)
    with pytest.raises(ValueError, match="group 1 has no latent"):
        FamilyPlan(base, [0, 0, 2, 2, 2, -1], 4)
    with pytest.raises(ValueError, match="5 groups for 6 latents"):
        FamilyPlan(base, [0, 0, 1, 1, 2], 4)
    with pytest.raises(ValueError, match="0 groups, 1 to 288 allowed"):
        FamilyPlan(base, [-1] * 6, 4)
    with pytest.raises(ValueError, match="negative"):
        FamilyPlan(base, fp.group, -1)
    with pytest.raises(ValueError, match=r"geometries \[0, 21\) lie outside the 4 families of 5"):
        families_host(FamilyPlan(dataclasses.replace(base, stratify=LHS), fp.group, 4), 0, 21)
    assert families_host(fp, 3, 3)[0].shape == (0, base.n_points, 3)
    group, names = smp.group_by_point(family_plan(6, 4).plan)
    assert group.tolist() == [0, 0, 0, 1, 1, 1] and names == ("point0", "point1")


def test_constants_match_the_header():
    with open(os.path.join(REPO, "include", "okx.h"), "r", encoding="utf-8") as fh:
        text = fh.read()
    for name in ("COUNT", "DROPPED", "SUM_A", "SUM_B", "SUMSQ_A", "SUMSQ_B", "FIELDS"):
        assert int(re.search(rf"OKX_SOBOL_{name} = (\d+)", text).group(1)) == getattr(es, f"SOBOL_{name}")
    assert int(re.search(r"OKX_ENS_SOBOL_MAX_GROUPS = (\d+)", text).group(1)) == es.SOBOL_MAX_GROUPS == smp.SOBOL_MAX_GROUPS


# ---- sobol_host on small-integer tables ----

def integer_table(n, d, s, k, seed, with_mask=True):
    """``(values [N M, S, K], status [N M, S], mask [N M] or None, shift [S, K])``: integers with |value - shift| <= 8.  From two
    families on, one member of family 1 is rejected at ONE step (status byte, then a NaN in one column) and - with a mask - one
    member of the last family is masked; larger tables get a sprinkling of both."""
    rng = np.random.default_rng(seed)
    m = d + 2
    shift = rng.integers(-5, 6, (s, k)).astype(np.float64)
    values = shift[None] + rng.integers(-8, 9, (n * m, s, k)).astype(np.float64)
    status = np.ones((n * m, s), dtype=np.uint8)
    mask = np.zeros(n * m, dtype=np.uint8) if with_mask else None
    if n >= 2:
        status[m + 1 + (d > 1), s - 1] = 2
        values[m, 0, k - 1] = np.nan
        if with_mask:
            mask[(n - 1) * m + m - 1] = 1
    for _ in range(n // 12):
        status[rng.integers(0, n * m), rng.integers(0, s)] = rng.choice(np.array([0, 3, 5, 9], dtype=np.uint8))  # (9: advisory bit, still accepted)
        values[rng.integers(0, n * m), rng.integers(0, s), rng.integers(0, k)] = rng.choice([np.inf, -np.inf, np.nan])
        if with_mask:
            mask[rng.integers(0, n * m)] = rng.choice(np.array([1, 2, 17], dtype=np.uint8))  # (2: bit 0 clear, the member counts)
    return values, status, mask, shift


def plain_loops(values, status, mask, d, shift):
    """The accumulator restated with Python floats, one family, entry and member at a time."""
    g, s, k = values.shape
    m = d + 2
    acc = np.zeros((s, k, SOBOL_FIELDS + 3 * d))
    for i in range(g // m):
        for si in range(s):
            for ki in range(k):
                counts = True
                for b in range(m):
                    row = i * m + b
                    counts = counts and math.isfinite(values[row, si, ki]) and (status is None or (int(status[row, si]) & 7) == 1) \
                        and (mask is None or (int(mask[row]) & 1) == 0)
                cell = acc[si, ki]
                if not counts:
                    cell[SOBOL_DROPPED] += 1.0
                    continue
                cell[SOBOL_COUNT] += 1.0
                sh = float(shift[si, ki])
                da, db = float(values[i * m, si, ki]) - sh, float(values[i * m + 1, si, ki]) - sh
                cell[es.SOBOL_SUM_A] += da
                cell[es.SOBOL_SUM_B] += db
                cell[es.SOBOL_SUMSQ_A] += da * da
                cell[es.SOBOL_SUMSQ_B] += db * db
                for j in range(d):
                    dj = float(values[i * m + 2 + j, si, ki]) - sh
                    cell[SOBOL_FIELDS + 3 * j] += db * (dj - da)
                    cell[SOBOL_FIELDS + 3 * j + 1] += (da - dj) * (da - dj)
                    cell[SOBOL_FIELDS + 3 * j + 2] += (db - dj) * (db - dj)
    return acc


INTEGER_CASES = [(n, d, s, k) for n in (1, 2, 67) for d in (1, 3) for s, k in ((1, 1), (3, 5))]


@pytest.mark.parametrize("n,d,s,k", INTEGER_CASES)
def test_sobol_host_equals_plain_loops_on_integer_tables(n, d, s, k):
    for with_mask in (False, True):
        values, status, mask, shift = integer_table(n, d, s, k, 1000 * n + 10 * d + s, with_mask)
        got = sobol_host(values, status, mask, d, shift)
        want = plain_loops(values, status, mask, d, shift)
        assert got.n_groups == d and np.array_equal(got.acc, want) and np.array_equal(got.shift, shift)
        assert np.all(got.acc[..., SOBOL_COUNT] + got.acc[..., SOBOL_DROPPED] == n)
        # merging two halves (whole families) equals the whole exactly
        cut = (n // 2) * (d + 2)
        halves = [sobol_host(values[a:b], status[a:b], None if mask is None else mask[a:b], d, shift) for a, b in ((0, cut), (cut, values.shape[0]))]
        assert np.array_equal(halves[0].merge(halves[1]).acc, want)
        assert np.array_equal(SobolAccumulator.empty(s, k, d, shift).merge(got).acc, want)
        if n < 2:
            continue
        m = d + 2
        dropped = got.acc[..., SOBOL_DROPPED]
        if n == 2:
            # family 1: one rejected member drops it at that step only, a NaN at that entry only; a masked member at every entry
            want_dropped = np.zeros((s, k))
            want_dropped[s - 1, :] = 1
            want_dropped[0, k - 1] = 1
            if with_mask:
                want_dropped[:] = 1  # (the last family IS family 1)
            assert np.array_equal(dropped, want_dropped)
        else:
            assert dropped.min() >= (1 if with_mask else 0) and 0 < dropped.max() < n
    with pytest.raises(ValueError, match="no whole families"):
        sobol_host(values[:-1], status[:-1], None, d, shift)
    with pytest.raises(ValueError, match="different shifts"):
        got.merge(sobol_host(values, status, mask, d, shift + 1.0))
    with pytest.raises(ValueError, match="0 groups, 1 to 288 allowed"):
        sobol_host(values, status, mask, 0, shift)


def term_bound(values, status, mask, d, shift):
    """``[S, K, fields]``: 2 (n + 1) U sum |term| - two recursive sums of the same n terms, each within (n + 1) U sum |term| of the
    exact sum whatever its order (Higham, Accuracy and Stability, (4.4) with gamma_n <= (n + 1) U for n U << 1)."""
    _, terms, _ = sobol_terms(values, status, mask, d, shift)
    return 2.0 * (terms.shape[0] + 1) * U * np.abs(terms).sum(axis=0)


# ---- exact zeros end to end: the drawn latents as the value table ----

@pytest.mark.parametrize("stratify", [IID, LHS])
def test_exact_zeros_with_the_latents_as_the_table(stratify):
    fp = family_plan(7, 40, stratify=stratify, guard=False)
    lat = families_host(fp)[1]
    acc = sobol_host(lat[:, None, :], None, None, fp.n_groups).acc[0]   # S = 1, K = Z
    check_exact_zeros(acc, fp.group)
    out = SobolAccumulator(acc[None], np.zeros((1, lat.shape[1]))).finalize()
    assert np.all(out.total[0][fp.group == -1] == 0.0)


def check_exact_zeros(acc, group):
    """``acc [Z, fields]`` of the latents' table: column z of group j has R_j == 0 and P_m == Q_m == 0 for every m != j; a -1 column
    every Q (and P) zero - and the sums that need not vanish do not."""
    d = int(group.max()) + 1
    p, q, r = (acc[:, SOBOL_FIELDS + f :: 3] for f in range(3))
    for z, j in enumerate(group.tolist()):
        for other in range(d):
            if other == j:
                assert r[z, other] == 0.0 and q[z, other] > 0.0
            else:
                assert q[z, other] == 0.0 and p[z, other] == 0.0 and r[z, other] > 0.0
    assert np.all(acc[:, SOBOL_DROPPED] == 0)


# ---- finalize ----

def test_finalize():
    d, s, k, n = 2, 2, 3, 50
    rng = np.random.default_rng(3)
    shift = rng.normal(0.0, 10.0, (s, k))
    values = shift[None] + rng.normal(0.0, 1.0, (n * (d + 2), s, k))
    values[:, 1, 0] = shift[1, 0]   # a constant column: every d is 0 and V = 0 exactly
    values[::4, 1, 1] = np.nan   # member 0 of every family is undefined: n = 0
    acc = sobol_host(values, None, None, d, shift, ("a", "b"))
    out = acc.finalize()
    assert out.group_names == ["a", "b"] and out.first.shape == (s, k, d)
    assert out.count[1, 1] == 0 and out.dropped[1, 1] == n and out.count[0, 0] == n
    for table in (out.first, out.first_jansen, out.total):
        assert np.all(np.isnan(table[1, 0])) and np.all(np.isnan(table[1, 1])) and np.all(np.isfinite(table[0]))
    assert np.isnan(out.mean[1, 1]) and np.isnan(out.variance[1, 0]) and out.mean[1, 0] == shift[1, 0]
    # mean undoes the shift; the formulas as the header states them
    fam = values.reshape(n, d + 2, s, k)
    ab = fam[:, :2].reshape(2 * n, s, k)
    assert np.allclose(out.mean[0], ab.mean(axis=0)[0], rtol=0, atol=1e-12)
    assert np.allclose(out.variance[0], ab.var(axis=0)[0], rtol=1e-10, atol=0)
    v = ab.var(axis=0)[0]
    dev = fam - shift[None, None]  # (P_j is taken about the shift: sum dB (dj - dA) moves with it by shift-of-B times sum (dj - dA))
    da, db, dj = dev[:, 0, 0], dev[:, 1, 0], np.moveaxis(dev[:, 2:, 0], 1, -1)
    assert np.allclose(out.first[0], (db[..., None] * (dj - da[..., None])).mean(axis=0) / v[:, None], rtol=1e-9, atol=1e-12)
    assert np.allclose(out.total[0], ((da[..., None] - dj) ** 2).mean(axis=0) / (2 * v[:, None]), rtol=1e-9, atol=1e-12)
    assert np.allclose(out.first_jansen[0], 1.0 - ((db[..., None] - dj) ** 2).mean(axis=0) / (2 * v[:, None]), rtol=1e-9, atol=1e-12)
    assert es.SobolAccumulator.empty(s, k, d, shift).finalize().count.sum() == 0


def test_indices_of_a_known_response():
    """y = sum c_z x_z + 0.3 x_2 x_3 over independent standard normals, groups {0, 1}, {2}, {3, 4}, latent 5 free: the indices are
    known in closed form; 4096 families put the estimates within 0.1 of them (standard errors of a few hundredths)."""
    group = np.array([0, 0, 1, 2, 2, -1])
    plan = SamplePlan(np.zeros((2, 3)), np.arange(6), np.full(6, NORMAL), stratify=LHS, seed=77)
    fp = FamilyPlan(plan, group, 4096)
    lat = families_host(fp)[1]
    c = np.array([1.0, 2.0, 0.5, 1.0, 1.0, 0.0])
    y = lat @ c + 0.3 * lat[:, 2] * lat[:, 3]
    out = sobol_host(y[:, None, None], None, None, 3).finalize()
    var, inter = np.array([5.0, 0.25, 2.0]), 0.09
    want_first, want_total = var / (var.sum() + inter), (var + [0.0, inter, inter]) / (var.sum() + inter)
    assert np.abs(out.first[0, 0] - want_first).max() < 0.1 and np.abs(out.first_jansen[0, 0] - want_first).max() < 0.1
    assert np.abs(out.total[0, 0] - want_total).max() < 0.1 and abs(out.mean[0, 0]) < 0.1 and abs(out.variance[0, 0] - 7.34) < 0.5


# ---- chunk_pieces(align=) ----

def test_chunk_pieces_in_units_of_a_family():
    from open_kinematics_amd.dist import chunk_pieces, shard_range

    for n_geom, world, chunks in ((4099, 3, 4), (5, 8, 2)):
        today = []
        for c in range(chunks):
            row = []
            for r in range(world):
                lo, hi = shard_range(n_geom, r, world)
                a, b = shard_range(hi - lo, c, chunks)
                row.append((lo + a, lo + b))
            today.append(row)
        assert chunk_pieces(n_geom, world, chunks) == chunk_pieces(n_geom, world, chunks, 1) == today
    for n_fam, m, world, chunks in ((7, 5, 3, 2), (2, 4, 3, 2), (4096, 12, 8, 2), (1, 3, 1, 1)):
        pieces = chunk_pieces(n_fam * m, world, chunks, align=m)
        flat = sorted(span for row in pieces for span in row if span[1] > span[0])
        assert all(a % m == 0 and b % m == 0 for row in pieces for a, b in row)
        assert flat[0][0] == 0 and flat[-1][1] == n_fam * m and all(x[1] == y[0] for x, y in zip(flat, flat[1:]))
        for r in range(world):  # a rank's chunks are consecutive runs of its shard
            mine = [pieces[c][r] for c in range(chunks)]
            assert all(x[1] == y[0] for x, y in zip(mine, mine[1:]))


# ---- the Sobol stage of ShardedEnsemble on host stand-ins ----

STEPS = 6


def integer_stand_in():
    """tests/test_dist.py's stand-in program (with the status bytes of tests/test_ensemble_stats.py) whose evaluation rows are rounded
    to integers: every sum of the Sobol stage is exact, so chunked and unchunked runs must agree bit for bit."""
    from test_ensemble_stats import _stand_in

    base = _stand_in()

    class _Integer(type(base)):
        def solve_evaluated(self, targets, **kw):
            res = super().solve_evaluated(targets, **kw)
            res.eval.copy_(torch.clamp(torch.round(res.eval), -64.0, 64.0))
            return res

    return _Integer()


def stand_in_families(n_families, stratify=LHS):
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(1, STEPS)
    plan = SamplePlan(table[0].numpy(), np.arange(9), NORMAL, scale=2.0, stratify=stratify, seed=9, guards=((GUARD_SIGN, 7, 1.0, float(table[0, 2, 1])),))
    return FamilyPlan(plan, [0, 0, 0, 1, 1, 1, 2, -1, 2], n_families, ("lower", "middle", "upper")), relative


def test_sobol_stage_chunked_equals_unchunked():
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_ensemble_stats import COLUMNS

    fp, relative = stand_in_families(9)
    shift = np.zeros((STEPS, len(COLUMNS)))
    runs = {}
    for chunks in (1, 2, 4):
        pipe = ShardedEnsemble(integer_stand_in(), fp, relative, STEPS, chunks=chunks, metric_columns=COLUMNS, reduce=True, sobol=True, shift=shift)
        pipe.step()
        assert all(a % 5 == 0 and b % 5 == 0 for row in pipe.pieces for a, b in row) and pipe.sobol_exchange_bytes_per_rank == 0
        runs[chunks] = pipe
    one = runs[1]
    acc = one.sobol_accumulator.acc.numpy()
    assert all(np.array_equal(runs[c].sobol_accumulator.acc.numpy(), acc) for c in (2, 4))
    values = one.metric_local.numpy().reshape(45, STEPS, len(COLUMNS))
    assert np.array_equal(values, np.round(values))  # the table is one of integers
    flags = families_host(fp)[3]
    assert 0 < flags.sum() < flags.size and torch.equal(one.sampled_flags, torch.as_tensor(flags))
    want = sobol_host(values, one.info_local[:, 32].numpy().reshape(45, STEPS), flags, 3, shift)
    assert np.array_equal(acc, want.acc)
    out = one.sobol()
    assert np.all(out.count + out.dropped == 9) and out.count.max() > 0 and out.dropped.max() > 0 and out.group_names == ["lower", "middle", "upper"]
    again = one.step() and one.sobol_accumulator.acc.numpy()
    assert np.array_equal(again, acc)  # a second step starts from nothing


def test_sobol_needs_a_family_plan():
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_ensemble_stats import COLUMNS, _stand_in

    fp, relative = stand_in_families(3)
    with pytest.raises(ValueError, match="pass an ensemble_sample.FamilyPlan"):
        ShardedEnsemble(_stand_in(), torch.as_tensor(families_host(fp)[0]), relative, STEPS, metric_columns=COLUMNS, reduce=True, sobol=True)
    with pytest.raises(ValueError, match="pass an ensemble_sample.FamilyPlan"):
        ShardedEnsemble(_stand_in(), fp.source_plan(), relative, STEPS, metric_columns=COLUMNS, reduce=True, sobol=True)
    with pytest.raises(ValueError, match="needs reduce=True"):
        ShardedEnsemble(_stand_in(), fp, relative, STEPS, metric_columns=COLUMNS, sobol=True)
    plain = ShardedEnsemble(_stand_in(), fp, relative, STEPS, metric_columns=COLUMNS, reduce=True)  # a family plan is a table like any other
    assert plain.n_geom == 15 and plain.align == 1
    with pytest.raises(ValueError, match="needs sobol=True"):
        plain.sobol()
