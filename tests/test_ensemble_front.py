"""
CPU: the nondominated (Pareto) front of an ensemble (ensemble_stats.front_host, the definition okx_ensemble_front is compared
with) against a plain double loop over pairs, its properties on hand-made rows, the merge rule front(A u B) = front(front(A) u
front(B)) over random splits, every message of check_front_arguments, and the Front stage of ShardedEnsemble(reduce=True,
front=...) on a CPU ensemble - one process and two gloo ranks, the stand-in program of tests/test_dist.py.

front_case is what tests/test_gpu_ensemble_front.py feeds the device pass with.  Every comparison is exact: integers, or the bits
of table values.  No tolerance appears anywhere.
"""

import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from open_kinematics_amd.ensemble_stats import (CURVE_C0, CURVE_C1, CURVE_MAX, FRONT_MAX, FRONT_MAX_GEOMETRIES, FRONT_MIN, FRONT_TARGET, EnsembleFront,
                                                check_front_arguments, curves_host, front_dominated, front_host, front_objectives, screen_host)
from test_ensemble_stats import COLUMNS, _stand_in


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_front(got: EnsembleFront, want: EnsembleFront, *, dominated: bool = True) -> bool:
    """Integers equal, values equal by their bits."""
    if dominated and not (got.dominated is not None and got.dominated.dtype == np.int32 and np.array_equal(got.dominated, want.dominated)):
        return False
    return bool(np.array_equal(got.tally, want.tally) and got.index.dtype == np.int64 and np.array_equal(got.index, want.index)
                and got.values.shape == want.values.shape and np.array_equal(bits(got.values), bits(want.values)))


def senses_of(m: int, mixed: bool):
    return [("min", "max", "target")[i % 3] if mixed else "min" for i in range(m)]


def front_case(g: int, m: int, levels: int, *, s: int = 1, k: int | None = None, mixed: bool = False, spoil: bool = True, with_status: bool = False,
               with_mask: bool = False):
    """
    ``(values [G, S, K], status [G, S] or None, objectives, mask [G] or None)``.  The M selected entries - M distinct entries of
    the ``S K``, not in order - hold ``default_rng(1000 G + 10 M + levels).integers(0, levels, (G, M))`` (``levels`` 4 or 16: ties
    and duplicate vectors are common) or, with ``levels = 0``, continuous values; the other entries hold noise.  ``mixed``: the
    senses cycle min, max, target (the target is the middle level); else all min.  ``spoil``: about one geometry in 16 carries a
    NaN, a +-inf or (``with_status``) a rejected state in a SELECTED entry and about one in 8 in an unselected one;
    ``with_mask``: about one in 5 is masked out, with the byte values the screen writes (1, 2, 3).
    """
    k = m if k is None else k
    rng = np.random.default_rng(1000 * g + 10 * m + levels)
    picked = rng.integers(0, levels, (g, m)).astype(np.float64) if levels else rng.standard_normal((g, m))
    side = np.random.default_rng(7 + g + m)  # (everything else comes from a second stream: the drawn objective values stay as stated)
    entries = side.permutation(s * k)[:m]
    table = side.standard_normal((g, s * k))
    table[:, entries] = picked
    objectives = []
    for i, (e, sense) in enumerate(zip(entries, senses_of(m, mixed))):
        objectives.append((int(e) // k, int(e) % k, sense) + ((float(levels // 2) + 0.5 * (i % 2),) if sense == "target" else ()))
    status = None
    if with_status:
        status = np.ones((g, s), dtype=np.uint8)
        status[side.random((g, s)) < 0.3] = 9  # (bits above the low three do not matter)
    if spoil and g:
        others = np.setdiff1d(np.arange(s * k), entries)
        for gi in np.flatnonzero(side.random(g) < 1.0 / 16.0):
            e = entries[side.integers(0, m)]
            what = side.integers(0, 4 if with_status else 3)
            if what < 3:
                table[gi, e] = (np.nan, np.inf, -np.inf)[what]
            else:
                status[gi, e // k] = (2, 4, 0, 3)[side.integers(0, 4)]
        for gi in np.flatnonzero(side.random(g) < 1.0 / 8.0):
            if others.size:
                table[gi, others[side.integers(0, others.size)]] = (np.nan, np.inf, -np.inf)[side.integers(0, 3)]
        if with_status:  # rejected states at steps no objective reads
            free = np.setdiff1d(np.arange(s), entries // k)
            if free.size:
                status[side.random(g) < 0.25, free[0]] = 6
    mask = None
    if with_mask:
        mask = np.where(side.random(g) < 0.2, side.integers(1, 4, g), 0).astype(np.uint8)
    return table.reshape(g, s, k), status, objectives, mask


def brute_force(values, status, objectives, mask=None, index=None, geometry_offset=0) -> EnsembleFront:
    """The contract as a plain double loop over pairs."""
    g = values.shape[0]
    vectors, raw = [], []
    for gi in range(g):
        ok = mask is None or mask[gi] == 0
        o, r = [], []
        for step, column, sense, *target in objectives:
            v = float(values[gi, step, column])
            if not math.isfinite(v) or (status is not None and (int(status[gi, step]) & 7) != 1):
                ok = False
            r.append(v)
            o.append(v if sense == "min" else -v if sense == "max" else abs(v - target[0]))
        vectors.append(o if ok else None)
        raw.append(r)
    dominated = np.full(g, -1, dtype=np.int32)
    for b in range(g):
        if vectors[b] is None:
            continue
        count = 0
        for a in range(g):
            if vectors[a] is not None and all(x <= y for x, y in zip(vectors[a], vectors[b])) and any(x < y for x, y in zip(vectors[a], vectors[b])):
                count += 1
        dominated[b] = count
    keep = np.flatnonzero(dominated == 0)
    ids = np.arange(g, dtype=np.int64) + geometry_offset if index is None else np.asarray(index, dtype=np.int64)
    tally = np.array([g, int((dominated >= 0).sum()), keep.size], dtype=np.int64)
    _, sense, target = check_front_arguments(objectives, values.shape[1], values.shape[2])
    return EnsembleFront(dominated, tally, ids[keep], np.array([raw[i] for i in keep], dtype=np.float64).reshape(keep.size, len(objectives)), sense, target)


def worth(front: EnsembleFront):
    """``(front members, dominated geometries, front members whose objective vector another member shares)``."""
    o = front_objectives(front.values, front.sense, front.target)
    _, counts = np.unique(o, axis=0, return_counts=True) if o.shape[0] else (None, np.zeros(0, dtype=np.int64))
    return int(front.tally[2]), int((front.dominated > 0).sum()), int(counts[counts > 1].sum())


def assert_worth(runs, levels: int) -> None:
    """The inputs of a parametrised case are worth the test: over its runs (``worth`` of each) at G >= 37 there is a front with more
    than one member, at least one dominated geometry and, for levels = 4, at least two front members with equal vectors."""
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 3)
    assert (runs[:, 0] > 1).any() and runs[:, 1].sum() >= 1, runs
    if levels == 4:
        assert runs[:, 2].sum() >= 2, runs


@pytest.mark.parametrize("levels", [4, 16, 0])
def test_front_host_equals_the_double_loop(levels):
    runs = []
    for m in (1, 2, 3, 5, 8):
        for g in (0, 1, 2, 37, 50, 65):
            for mixed, shape in ((False, dict()), (True, dict(s=3, k=4, with_status=True, with_mask=True))):
                values, status, objectives, mask = front_case(g, m, levels, mixed=mixed, **shape)
                index = None if not mixed else np.random.default_rng(g).permutation(g).astype(np.int64) * 3 + 11
                got = front_host(values, status, objectives, mask, index, 0 if mixed else 1000)
                want = brute_force(values, status, objectives, mask, index, 0 if mixed else 1000)
                assert same_front(got, want), (g, m, levels, mixed)
                assert got.tally[0] == g and (got.dominated == -1).sum() == g - got.tally[1]
                if g >= 37:
                    runs.append(worth(got))
    assert_worth(runs, levels)


def test_what_the_generator_promises():
    """With levels = 4, G >= 37 gives tied front members for M <= 2 and a dominated majority for M <= 3; continuous values
    and M = 8 put most of the ensemble on the front (545 of 1031)."""
    for g in (37, 65, 255):
        for m in (1, 2, 3):
            front = front_host(*front_case(g, m, 4, spoil=False)[:3])
            members, dominated, tied = worth(front)
            assert dominated > g // 2, (g, m)
            if m <= 2:
                assert tied >= 2, (g, m)
    assert front_host(*front_case(1031, 8, 0, spoil=False)[:3]).tally[2] == 545


# ---- properties on hand-made rows ----

def one_step(rows):
    return np.asarray(rows, dtype=np.float64)[:, None, :]


ALL_MIN3 = [(0, 0, "min"), (0, 1, "min"), (0, 2, "min")]


def special_rows(g: int):
    """``{name: (values [G, 1, 3], objectives, dominated [G])}``: all rows equal, a strict chain, an antichain."""
    i = np.arange(g, dtype=np.float64)
    return {"equal": (one_step(np.tile([1.5, -2.0, 0.25], (g, 1))), ALL_MIN3, np.zeros(g, dtype=np.int32)),
            "chain": (one_step(np.stack([i, 2.0 * i, i * i], axis=1)), ALL_MIN3, np.arange(g, dtype=np.int32)),
            "antichain": (one_step(np.stack([i, -i, np.zeros(g)], axis=1)), ALL_MIN3, np.zeros(g, dtype=np.int32))}


@pytest.mark.parametrize("name", ["equal", "chain", "antichain"])
def test_equal_rows_a_chain_and_an_antichain(name):
    g = 131
    values, objectives, dominated = special_rows(g)[name]
    front = front_host(values, None, objectives)
    assert np.array_equal(front.dominated, dominated) and front.dominated.dtype == np.int32
    members = 1 if name == "chain" else g
    assert list(front.tally) == [g, g, members] and np.array_equal(front.index, np.arange(members))
    assert np.array_equal(bits(front.values), bits(values[:members, 0, :]))


def test_one_objective_is_the_competition_rank():
    v = np.random.default_rng(3).integers(0, 9, 200).astype(np.float64)
    front = front_host(v[:, None, None], None, [(0, 0, "min")])
    assert np.array_equal(front.dominated, [(v < x).sum() for x in v])
    assert np.array_equal(front.index, np.flatnonzero(v == v.min())) and front.tally[2] > 1
    best = front_host(v[:, None, None], None, [(0, 0, FRONT_MAX)])
    assert np.array_equal(best.dominated, [(v > x).sum() for x in v]) and np.array_equal(best.values[:, 0], np.full(best.tally[2], v.max()))


def signed_zero_rows():
    """-0.0 and +0.0 tie: rows 0 and 1 are equal vectors, row 2 is dominated by both, under min and under max alike."""
    return one_step([[0.0, -0.0], [-0.0, 0.0], [0.0, 1.0]]), [(0, 0, "max"), (0, 1, "min")], [0, 0, 2]


def target_rounding_rows():
    """|v - t| with the subtraction rounded ONCE: 3 + 2^-51 and 3 are at different distances from 3, but at the same distance
    from t = 1e16 once the difference is rounded (doubles are 2 apart there: both differences round to 1e16 - 4, while the
    exact ones differ)."""
    t = 1.0e16
    rows = one_step([[3.0 + 2.0 ** -51, 3.0, 0.0], [3.0, 3.0, 0.0], [0.0, 3.0, 1.0]])
    near = [(0, 0, "target", 3.0), (0, 1, "target", t)]  # row 1 is nearer to 3 than row 0: it dominates it
    far = [(0, 0, "target", t), (0, 1, "min")]           # row 0 - t and row 1 - t round to the same double: they tie
    assert rows[0, 0, 0] != rows[1, 0, 0] and abs(rows[0, 0, 0] - t) == abs(rows[1, 0, 0] - t) == 9999999999999996.0
    return rows, near, [1, 0, 2], far, [0, 0, 2]


def test_signed_zeros_tie_and_the_target_difference_is_rounded_once():
    values, objectives, dominated = signed_zero_rows()
    front = front_host(values, None, objectives)
    assert list(front.dominated) == dominated and list(front.index) == [0, 1]
    assert np.array_equal(bits(front.values), bits(values[:2, 0, :]))  # the raw bits: the zeros keep their signs
    rows, near, d_near, far, d_far = target_rounding_rows()
    assert list(front_host(rows, None, near).dominated) == d_near
    got = front_host(rows, None, far)
    assert list(got.dominated) == d_far and np.array_equal(bits(got.values), bits(rows[:2, 0, :2]))


def test_what_removes_a_geometry():
    base = one_step(np.random.default_rng(5).standard_normal((12, 4)))
    objectives = [(0, 0, "min"), (0, 2, "max")]
    want = front_host(base, None, objectives)
    assert want.tally[1] == 12
    for bad in (np.nan, np.inf, -np.inf):
        for column, removed in ((0, True), (2, True), (1, False), (3, False)):
            v = base.copy()
            v[4, 0, column] = bad
            got = front_host(v, None, objectives)
            assert (got.dominated[4] == -1) == removed and got.tally[1] == 12 - removed
            if not removed:
                assert np.array_equal(got.dominated, want.dominated)
    two = np.concatenate([base, base[:, :, ::-1]], axis=1)  # two steps
    for st, removed in ((1, False), (9, False), (2, True), (3, True), (5, True), (0, True)):
        status = np.ones((12, 2), dtype=np.uint8)
        status[4, 0] = st
        got = front_host(two, status, objectives)
        assert (got.dominated[4] == -1) == removed
        status = np.ones((12, 2), dtype=np.uint8)
        status[4, 1] = st  # a step no objective reads
        assert np.array_equal(front_host(two, status, objectives).dominated, want.dominated)
    mask = np.zeros(12, dtype=np.uint8)
    mask[[0, 4, 7]] = (1, 2, 3)
    got = front_host(base, None, objectives, mask)
    keep = np.flatnonzero(mask == 0)
    sub = front_host(base[keep], None, objectives)
    assert np.array_equal(got.dominated[keep], sub.dominated) and (got.dominated[mask != 0] == -1).all() and got.tally[1] == 9
    assert np.array_equal(got.index, keep[sub.index]) and np.array_equal(bits(got.values), bits(sub.values))


def test_ids_follow_index_and_offset():
    values, _, objectives, _ = front_case(40, 2, 4, spoil=False)
    plain = front_host(values, None, objectives)
    assert np.array_equal(front_host(values, None, objectives, None, None, 700).index, plain.index + 700)
    ids = np.random.default_rng(1).permutation(40).astype(np.int64) * 1_000_000_007
    named = front_host(values, None, objectives, None, ids, 700)  # (the offset is not used beside an index)
    assert np.array_equal(named.index, ids[plain.index]) and np.array_equal(bits(named.values), bits(plain.values))


# ---- merge ----

def merged_in_chunks(values, status, objectives, mask, pieces, order):
    g = values.shape[0]
    cuts = np.sort(np.random.default_rng(pieces + g).choice(np.arange(1, g), pieces - 1, replace=False)) if pieces > 1 else []
    spans = list(zip([0, *cuts], [*cuts, g]))
    total = None
    for at in order(len(spans)):
        a, b = spans[at]
        part = front_host(values[a:b], None if status is None else status[a:b], objectives, None if mask is None else mask[a:b], None, a)
        total = part if total is None else total.merge(part)
    return total


@pytest.mark.parametrize("pieces", [2, 3, 7])
@pytest.mark.parametrize("with_mask", [False, True])
def test_chunks_merge_to_the_one_call(pieces, with_mask):
    found = np.zeros(3, dtype=np.int64)
    for g, m, levels in ((37, 2, 4), (64, 3, 16), (130, 5, 0), (257, 2, 4)):
        values, status, objectives, mask = front_case(g, m, levels, s=2, k=4, mixed=True, with_status=True, with_mask=with_mask)
        whole = front_host(values, status, objectives, mask)
        found += worth(whole)
        orders = (lambda n: range(n), lambda n: reversed(range(n)), lambda n: np.random.default_rng(n).permutation(n))
        for order in orders:
            got = merged_in_chunks(values, status, objectives, mask, pieces, order)
            assert got.dominated is None and np.array_equal(got.tally, whole.tally)
            by_id = np.argsort(got.index, kind="stable")
            assert np.array_equal(got.index[by_id], whole.index) and np.array_equal(bits(got.values[by_id]), bits(whole.values))
    assert found[0] > 4 and found[1] > 0 and found[2] >= 2
    with pytest.raises(ValueError, match="different objectives"):
        front_host(values, status, objectives).merge(front_host(values, status, objectives[:1]))


# ---- argument checks ----

GOOD = [(0, 1, "min"), (2, 0, "max"), (1, 2, "target", 0.5)]
MESSAGES = [
    ([], "0 objectives, 1 to 8 allowed"),
    ([(0, 0, "min")] * 9, "9 objectives, 1 to 8 allowed"),
    ([(3, 0, "min")], r"entry 0 is \(step 3, column 0\), outside"),
    (GOOD[:2] + [(0, 3, "min")], r"entry 2 is \(step 0, column 3\), outside"),
    ([(-1, 0, "min")], "entry 0 is"),
    (GOOD + [(2, 0, "min")], r"entry 3 repeats entry 1 \(index 6\)"),
    ([(0, 0, "best")], "sense 0 is 'best', not 0"),
    ([(0, 0, 3)], "sense 0 is 3, not 0"),
    ([(0, 0, "target")], "objective 0 aims at a target and no target"),
    (GOOD[:1] + [(1, 1, "target", float("nan"))], "target 1 is nan, not finite"),
    ([(0, 0, FRONT_TARGET, float("inf"))], "target 0 is inf, not finite"),
    ([(0, 0, "min", 1.0)], "gives a target and does not aim at one"),
    ([(0.5, 0, "min")], "step and column must be integers"),
    ([(0, 0)], "must be"),
]


@pytest.mark.parametrize("objectives,message", MESSAGES)
def test_every_message_of_check_front_arguments(objectives, message):
    with pytest.raises(ValueError, match=message):
        check_front_arguments(objectives, 3, 3)
    with pytest.raises(ValueError, match=message):
        front_host(np.zeros((2, 3, 3)), None, objectives)


def test_the_cap_and_the_normalised_arguments():
    with pytest.raises(ValueError, match="65537 geometries, at most 65536"):
        check_front_arguments(GOOD, 3, 3, FRONT_MAX_GEOMETRIES + 1)
    entries, sense, target = check_front_arguments(GOOD, 3, 3, FRONT_MAX_GEOMETRIES)
    assert entries.dtype == np.int32 and sense.dtype == np.int32 and target.dtype == np.float64
    assert list(entries) == [1, 6, 5] and list(sense) == [FRONT_MIN, FRONT_MAX, FRONT_TARGET] and list(target) == [0.0, 0.0, 0.5]
    with pytest.raises(ValueError, match="objectives are needed"):
        front_host(np.zeros((2, 3, 3)))


def test_the_header_and_the_library_agree_with_the_host():
    """The constants of include/okx.h, and okx_ensemble_front_check's words (it needs no GPU) against check_front_arguments'."""
    import ctypes as C
    import re

    from open_kinematics_amd import _lib, ensemble_stats as es

    with open(os.path.join(REPO, "include", "okx.h"), "r", encoding="utf-8") as fh:
        header = fh.read()
    for name, value in (("OKX_FRONT_MIN", es.FRONT_MIN), ("OKX_FRONT_MAX", es.FRONT_MAX), ("OKX_FRONT_TARGET", es.FRONT_TARGET),
                        ("OKX_ENS_FRONT_MAX_OBJECTIVES", es.FRONT_MAX_OBJECTIVES), ("OKX_ENS_FRONT_MAX_GEOMETRIES", es.FRONT_MAX_GEOMETRIES)):
        assert int(re.search(name + r" = (\d+)", header).group(1)) == value
    lib = _lib.load()

    def check(n_geom, entries, sense, target):
        e, s = np.asarray(entries, dtype=np.int32), np.asarray(sense, dtype=np.int32)
        t = None if target is None else np.asarray(target, dtype=np.float64)
        return lib.okx_ensemble_front_check(n_geom, 3, 3, e.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                                            None if t is None else t.ctypes.data_as(C.c_void_p), len(entries))

    assert check(65536, [1, 6, 5], [0, 1, 2], [0.0, 0.0, 0.5]) == 0 and check(0, [8], [1], None) == 0
    inf, nan = float("inf"), float("nan")
    for args, message in (((65537, [0], [0], None), "65537 geometries, at most 65536"),
                          ((4, [], [], None), "0 objectives, 1 to 8 allowed"),
                          ((4, [0] * 9, [0] * 9, None), "9 objectives, 1 to 8 allowed"),
                          ((4, [9], [0], None), r"entry 0 is 9, outside \[0, 9\)"),
                          ((4, [0, -1], [0, 0], None), r"entry 1 is -1, outside"),
                          ((4, [1, 6, 5, 6], [0] * 4, None), r"entry 3 repeats entry 1 \(index 6\)"),
                          ((4, [0], [3], None), "sense 0 is 3, not 0"),
                          ((4, [0], [-1], None), "sense 0 is -1, not 0"),
                          ((4, [0], [2], None), "objective 0 aims at a target and no target"),
                          ((4, [0, 1], [0, 2], [0.0, nan]), "target 1 is nan, not finite"),
                          ((4, [0], [2], [inf]), "target 0 is inf, not finite")):
        assert check(*args) == -1 and re.search(message, _lib.last_error()), (args, _lib.last_error())
    assert isinstance(lib.okx_ensemble_front, C._CFuncPtr) and lib.okx_ensemble_front_scratch_bytes(4099, 3) == 8 * 4160 * 4


# ---- the Front stage on a CPU ensemble ----

STEPS = 6
CURVES = dict(abscissa=1, origin=0.5, scale=4.0, degree=2, window=(-20.0, 20.0))
TABLE_OBJECTIVES = [(0, 0, "min"), (3, 2, "max"), (5, 3, "target", 0.0)]
CURVE_OBJECTIVES = [(0, CURVE_C1, "min"), (2, CURVE_MAX, "max"), (3, CURVE_C0, "target", 0.25)]
VARIANTS = {"table": dict(objectives=TABLE_OBJECTIVES), "curves": dict(objectives=CURVE_OBJECTIVES, source="curves"),
            "screened": dict(objectives=TABLE_OBJECTIVES[:2], source="table", screened=True),
            "screened curves": dict(objectives=CURVE_OBJECTIVES[:2], source="curves", screened=True)}
N_GEOM = (23, 1)


def _one_process_table(n_geom: int):
    """``(values [G, S, K], status [G, S])`` of the gathered table of the same ensemble in one process."""
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(n_geom, STEPS)
    plain = ShardedEnsemble(_stand_in(), table, relative, STEPS, metric_columns=COLUMNS)
    full = plain.step()
    return full.numpy().reshape(n_geom, STEPS, len(COLUMNS)).copy(), plain.status_full.numpy().reshape(n_geom, STEPS).copy()


def _limits():
    """The 20 % - 80 % band of what counts of column 0 at step 2 of the 64-geometry table; every other entry is not looked at."""
    values, status = _one_process_table(64)
    column = values[:, 2, 0][np.isfinite(values[:, 2, 0]) & ((status[:, 2] & 7) == 1)]
    limits = np.full((STEPS, len(COLUMNS), 2), (-np.inf, np.inf))
    limits[2, 0] = np.quantile(column, 0.2), np.quantile(column, 0.8)
    return limits


def _front_ensemble(n_geom: int, chunks: int, variant: str, limits):
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(n_geom, STEPS)
    pipe = ShardedEnsemble(_stand_in(), table, relative, STEPS, chunks=chunks, metric_columns=COLUMNS, reduce=True, curves=CURVES, limits=limits,
                           screen=True, front=VARIANTS[variant])
    pipe.step()
    pipe.step()  # a second step starts from nothing
    return pipe


def host_chain(values, status, variant: str, limits) -> EnsembleFront:
    """curves_host -> screen_host -> front_host on the one-process table."""
    spec = VARIANTS[variant]
    mask = screen_host(values, status, limits).flags if spec.get("screened") else None
    if spec.get("source") == "curves":
        features = curves_host(values, status, **CURVES).table()
        return front_host(features[:, None, :], None, [(0, c * 12 + f) + tuple(rest) for c, f, *rest in spec["objectives"]], mask)
    return front_host(values, status, spec["objectives"], mask)


def _tables(front: EnsembleFront) -> dict:
    return {"tally": front.tally, "index": front.index, "values": front.values}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_stage_in_one_process(variant):
    limits = _limits()
    n_geom = N_GEOM[0]
    values, status = _one_process_table(n_geom)
    want = host_chain(values, status, variant, limits)
    # worth it: a front of several, dominated geometries and (but for the features alone: every fit succeeds) geometries that are no candidates
    assert 1 < want.tally[2] < want.tally[1] and (want.tally[1] < n_geom or variant == "curves"), want.tally
    for chunks in (1, 3):
        pipe = _front_ensemble(n_geom, chunks, variant, limits)
        got = pipe.front()
        assert same_front(got, want, dominated=chunks == 1) and pipe.front_exchange_bytes_per_rank == 0
        assert (got.dominated is None) == (chunks > 1) and pipe.front_local() is got


def test_the_constructor_refuses():
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    def make(n_geom=2, **kw):
        table, relative = _ensemble_inputs(n_geom, STEPS)
        return ShardedEnsemble(_stand_in(), table, relative, STEPS, metric_columns=COLUMNS, **kw)

    front = dict(objectives=TABLE_OBJECTIVES)
    with pytest.raises(ValueError, match="needs reduce=True"):
        make(front=front)
    with pytest.raises(ValueError, match=r"front= takes objectives .*got \['best', 'objectives'\]"):
        make(reduce=True, front=dict(front, best=1))
    with pytest.raises(ValueError, match="front= takes objectives"):
        make(reduce=True, front=dict(source="table"))
    with pytest.raises(ValueError, match="front= takes objectives"):
        make(reduce=True, front=dict(front, source="features"))
    with pytest.raises(ValueError, match="needs curves="):
        make(reduce=True, front=dict(front, source="curves"))
    with pytest.raises(ValueError, match="needs screen=True"):
        make(reduce=True, front=dict(front, screened=True))
    with pytest.raises(ValueError, match="at most 65536 geometries, the ensemble has 65537"):
        make(65537, reduce=True, front=front)
    with pytest.raises(ValueError, match=r"entry 0 is \(step 6, column 0\)"):
        make(reduce=True, front=dict(objectives=[(6, 0, "min")]))
    with pytest.raises(ValueError, match=r"a curves objective is \(column, field, sense ...\)"):
        make(reduce=True, curves=CURVES, front=dict(objectives=[(0, 12, "min")], source="curves"))
    with pytest.raises(ValueError, match="needs front="):
        make(reduce=True).front()


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    limits = _limits()
    out = {}
    for n_geom in N_GEOM:
        for chunks in (1, 2):
            for variant in VARIANTS:
                pipe = _front_ensemble(n_geom, chunks, variant, limits)
                local = pipe.front_local()
                out[n_geom, chunks, variant] = {"range": pipe.geometry_range, "front": _tables(pipe.front()), "local": _tables(local),
                                                "sent": pipe.front_exchange_bytes_per_rank}
    torch.save(out, os.path.join(out_dir, f"front{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_one_process_front(tmp_path):
    """23 geometries shard 12 + 11; one geometry leaves rank 1 without any, and it still joins the all-gather.  Every rank runs the
    pass over the gathered front rows, so front() is the host chain on the one-process table bit for bit, on both ranks and with
    one chunk or two; a rank's own front is the front of its shard."""
    world = 2
    port = 36100 + (os.getpid() + 31 * world) % 2000
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"front{r}.pt"), weights_only=False) for r in range(world)]
    limits = _limits()
    for n_geom in N_GEOM:
        values, status = _one_process_table(n_geom)
        for variant, spec in VARIANTS.items():
            want = host_chain(values, status, variant, limits)
            one_process = _front_ensemble(n_geom, 1, variant, limits).front()
            assert same_front(one_process, want)
            for chunks in (1, 2):
                one, two = got[0][n_geom, chunks, variant], got[1][n_geom, chunks, variant]
                assert (one["range"], two["range"]) == ({23: (0, 12), 1: (0, 1)}[n_geom], {23: (12, 23), 1: (1, 1)}[n_geom])
                for rank in (one, two):
                    for key, table in _tables(want).items():
                        same = np.array_equal(bits(rank["front"][key]), bits(table)) if key == "values" else np.array_equal(rank["front"][key], table)
                        assert same and rank["front"][key].dtype == table.dtype, (n_geom, chunks, variant, key)
                    lo, hi = rank["range"]
                    shard = host_chain(values[lo:hi], status[lo:hi], variant, limits)
                    assert np.array_equal(rank["local"]["index"], shard.index + lo) and np.array_equal(bits(rank["local"]["values"]), bits(shard.values))
                    assert rank["sent"] == 8 * ({23: 12, 1: 1}[n_geom] + 1) * (len(spec["objectives"]) + 2)
