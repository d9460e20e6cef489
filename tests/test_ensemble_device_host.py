"""
CPU: the host layer of the device ensemble passes (open_kinematics_amd/ensemble_device.py), without a GPU.  A stand-in takes the
place of ``DeviceProgram``: the real library (its host-side ``*_check`` / ``*_scratch_bytes`` functions need no device), CPU tensors,
and an ``_ensemble_call`` that checks every launch's arguments against the entry point's ``argtypes`` and records the launch
instead of making it.  What is pinned here: which entry point every wrapper reaches and with which tables; that every table of
every pass's ``out=`` is refused - before any launch - when its dtype, its shape or its layout is wrong; the argument errors and
their texts; and ``merge`` / ``numpy()`` of the four accumulators.

The shapes are the smallest that take every branch: 6 geometries of 2 steps and 2 columns (Sobol': two families of three, D = 1,
and one of six, D = 4), 3 replicates, 4 weight rows, 2 factors.

Two cases of the tamper table cannot be built as "one extra or one missing element" / "a non-contiguous view", and are replaced
or counted, never dropped: the length of the screen's ``pass_index`` IS its capacity (any length is a valid table; what is refused
is a second dimension), and a one-element table (the screen's ``pass_count [1]``) has no non-contiguous view.
"""

import ctypes as C

import numpy as np
import pytest
import torch

from open_kinematics_amd import _lib
from open_kinematics_amd.ensemble_device import EnsembleReductions
from open_kinematics_amd.ensemble_stats import (CovarianceAccumulator, EnsembleAccumulator, SobolAccumulator, SobolBootstrapAccumulator,
                                                factor_moment_count)
from test_ensemble_sample import IID, NORMAL, make_plan
from test_ensemble_sobol import family_plan

G, S, K, P, R = 6, 2, 2, 2, 3
VALUES = torch.arange(G * S * K, dtype=torch.float64).reshape(G * S, K)
FACTORS = torch.arange(G * P, dtype=torch.float64).reshape(G, P)
LIMITS = [-1.0, 100.0]
PLAN = make_plan(p=1, f=1, kinds=(NORMAL,), stratify=IID, n_total=3)  # "one coordinate" of test_gpu_ensemble_sample.py
FAMILIES = family_plan(1, 1)  # the smallest of test_gpu_ensemble_sobol.py: one latent, one family of three


class Recorder(EnsembleReductions):
    """``self.calls``: every launch as ``(name, args)``; ``self.specs``: the tables the checker was last given."""

    def __init__(self):
        self.lib, self.device, self.calls, self.specs = _lib.load(), torch.device("cpu"), [], None

    def _ensemble_call(self, name, *args):
        fn = getattr(self.lib, name)
        assert len(args) + 1 == len(fn.argtypes), name
        for kind, arg in zip(fn.argtypes, args):
            kind.from_param(arg)
        self.calls.append((name, args))

    def _check_tables(self, message, tables, optional=()):
        self.specs = [*tables, *optional]
        super()._check_tables(message, tables, optional)


def select_round(call):
    def run(dp, out):
        out = dp.select_prepare(S, K, [0.25, 0.5], LIMITS, rounds=True) if out is None else out
        call(dp, out)
        return out
    return run


# pass: (the entry point it reaches, call(dp, out) -> out, the tables its checker is given by the attribute that holds them)
PASSES = {
    "reduce": ("okx_ensemble_reduce", lambda dp, out: dp.reduce_ensemble(VALUES, steps_per_geometry=S, factors=FACTORS, out=out),
               {"acc", "shift", "factor_acc"}),
    "select": ("okx_ensemble_select", lambda dp, out: dp.select_ensemble(VALUES, steps_per_geometry=S, out=out,
                                                                         **({} if out else dict(probs=[0.25, 0.5], limits=LIMITS))),
               {"probs", "limits", "order", "count", "outside"}),
    "select_begin": ("okx_ensemble_select_begin", select_round(lambda dp, run: dp.select_begin(run)),
                     {"probs", "limits", "order", "count", "outside", "state", "hist"}),
    "select_count": ("okx_ensemble_select_count", select_round(lambda dp, run: dp.select_count(run, 0, VALUES, steps_per_geometry=S)),
                     {"probs", "limits", "order", "count", "outside", "state", "hist"}),
    "select_descend": ("okx_ensemble_select_descend", select_round(lambda dp, run: dp.select_descend(run, 0)),
                       {"probs", "limits", "order", "count", "outside", "state", "hist"}),
    "select_finish": ("okx_ensemble_select_finish", select_round(lambda dp, run: dp.select_finish(run)),
                      {"probs", "limits", "order", "count", "outside", "state", "hist"}),
    "screen": ("okx_ensemble_screen", lambda dp, out: dp.screen_ensemble(VALUES, steps_per_geometry=S, out=out, **({} if out else dict(limits=LIMITS))),
               {"limits", "flags", "margin", "entry", "tally", "blame", "pass_index", "pass_count"}),  # (scale: None)
    "covariance": ("okx_ensemble_covariance", lambda dp, out: dp.covariance_ensemble(VALUES, steps_per_geometry=S, out=out,
                                                                                     **({} if out else dict(entries=[0, 3]))),
                   {"gram", "sum", "counts", "shift", "entries"}),
    "curves": ("okx_ensemble_curves", lambda dp, out: dp.curves_ensemble(VALUES, steps_per_geometry=S, out=out,
                                                                         **({} if out else dict(abscissa=[0.0, 1.0], scale=1.0, degree=1))),
               {"features", "count", "abscissa"}),
    "front": ("okx_ensemble_front", lambda dp, out: dp.front_ensemble(VALUES, steps_per_geometry=S, out=out,
                                                                      **({} if out else dict(objectives=[(0, 0, "min"), (1, 1, "max")]))),
              {"dominated", "tally", "front_index", "front_values"}),
    "sample": ("okx_ensemble_sample", lambda dp, out: dp.sample_ensemble(PLAN, 0, 3, latents=True, out=out), {"hardpoints", "latents", "flags"}),
    "sample_families": ("okx_ensemble_sample_families", lambda dp, out: dp.sample_families(FAMILIES, latents=True, delta=True, out=out),
                        {"hardpoints", "latents", "delta", "flags"}),
    "sobol, D = 1": ("okx_ensemble_sobol", lambda dp, out: dp.sobol_ensemble(VALUES, steps_per_geometry=S, n_groups=1, out=out), {"acc", "shift"}),
    "sobol, D = 4": ("okx_ensemble_sobol", lambda dp, out: dp.sobol_ensemble(VALUES, steps_per_geometry=S, n_groups=4, out=out), {"acc", "shift"}),
    "bootstrap_weights": ("okx_ensemble_bootstrap_weights", lambda dp, out: dp.bootstrap_weights(4, R, 5, out=out), {"out"}),
    "sobol_bootstrap": ("okx_ensemble_sobol_bootstrap",
                        lambda dp, out: dp.sobol_bootstrap_ensemble(VALUES, steps_per_geometry=S, n_groups=1, n_replicates=R, seed=5, out=out),
                        {"acc", "shift"}),
}
NONE_PAIRS = {"screen": 1, "sample": 1}  # scale; delta
HANDS_ALL = set(PASSES) - {"select", "select_begin", "select_count", "select_descend", "select_finish"}  # (these hand on what they work on)


def pointers(args) -> set:
    return {a.value for a in args if isinstance(a, C.c_void_p) and a.value}


def holder(out, table) -> str:
    """The attribute of ``out`` that holds ``table``; "out" when ``out`` is the table."""
    return "out" if out is table else next(name for name, value in vars(out).items() if value is table)


@pytest.mark.parametrize("name", list(PASSES))
def test_every_wrapper_reaches_its_entry_point_and_out_is_reused(name):
    entry, call, names = PASSES[name]
    dp = Recorder()
    first = call(dp, None)
    assert [c[0] for c in dp.calls] == [entry]
    assert call(dp, first) is first and [c[0] for c in dp.calls] == [entry, entry]
    tables = [t for t, _, _ in dp.specs if t is not None]
    assert {holder(first, t) for t in tables} == names and len(dp.specs) - len(tables) == NONE_PAIRS.get(name, 0)
    handed, owned = pointers(dp.calls[1][1]), {t.data_ptr() for t in tables}
    assert handed == pointers(dp.calls[0][1])  # nothing was reallocated, the scratch included
    assert owned <= handed if name in HANDS_ALL else owned & handed


def test_the_select_rounds_entry():
    dp = Recorder()
    assert dp.select_rounds == int(dp.lib.okx_ensemble_select_rounds()) > 0 and not dp.calls


# how the shape of a table is spoiled: one element more in the last dimension, unless ...
SHAPE = {"state": "shorter",  # ... the table has a least size, not a shape,
         "dominated": "shorter",  # (as here: one row per geometry of the call or more)
         "pass_index": "wider"}  # ... or its length is free - it is the capacity - and only a second dimension is wrong


def spoiled(table, how):
    if how == "dtype":
        return table.to(torch.float32)
    if how == "shape":
        return torch.cat([table, table.narrow(-1, 0, 1)], dim=-1)
    if how == "shorter":
        return table[:-1].clone()
    if how == "wider":
        return torch.stack([table, table], dim=-1).contiguous()
    return torch.stack([table, table], dim=-1)[..., 0]  # "layout": same shape and dtype, every element two apart


def test_every_table_of_every_out_is_checked():
    tried = pairs = absent = impossible = 0
    for name, (_, call, _) in PASSES.items():
        dp = Recorder()
        out = call(dp, call(dp, None))
        launches, specs = len(dp.calls), list(dp.specs)
        for table, _, _ in specs:
            pairs += 1
            if table is None:
                absent += 1
                continue
            where = holder(out, table)
            for how in ("dtype", SHAPE.get(where, "shape"), "layout"):
                bad = spoiled(table, how)
                if how == "layout" and table.numel() == 1:
                    assert bad.is_contiguous()  # a one-element table has no other layout: the case does not exist
                    impossible += 1
                    continue
                assert bad.dtype != table.dtype or bad.shape != table.shape or not bad.is_contiguous()
                with pytest.raises(ValueError):
                    call(dp, bad) if where == "out" else (setattr(out, where, bad), call(dp, out))
                assert len(dp.calls) == launches, (name, where, how)
                tried += 1
            if where != "out":
                setattr(out, where, table)
        assert call(dp, out) is out and len(dp.calls) == launches + 1  # the tables put back: accepted again
    assert pairs == sum(len(names) + NONE_PAIRS.get(name, 0) for name, (_, _, names) in PASSES.items())
    assert absent == sum(NONE_PAIRS.values()) and impossible == 1  # (pass_count [1])
    assert tried == 3 * (pairs - absent) - impossible


def test_outside_goes_with_limits():
    dp = Recorder()
    out = dp.select_ensemble(VALUES, steps_per_geometry=S, probs=[0.5], limits=LIMITS)
    out.outside = None
    with pytest.raises(ValueError, match="out must hold contiguous device tables"):
        dp.select_ensemble(VALUES, steps_per_geometry=S, out=out)
    assert len(dp.calls) == 1
    plain = dp.select_ensemble(VALUES, steps_per_geometry=S, probs=[0.5])
    assert plain.limits is None and plain.outside is None and dp.select_ensemble(VALUES, steps_per_geometry=S, out=plain) is plain


def test_argument_errors_keep_their_texts():
    dp = Recorder()
    sobol = dict(steps_per_geometry=S, n_groups=1)
    boot = dict(steps_per_geometry=S, n_groups=1, n_replicates=R, seed=1)
    shift = torch.zeros((S, K), dtype=torch.float64)
    mask = torch.zeros(G, dtype=torch.uint8)
    cases = [
        ("okx_ensemble_sobol: 6 geometries are no whole families of 4", lambda: dp.sobol_ensemble(VALUES, steps_per_geometry=S, n_groups=2)),
        ("okx_ensemble_sobol_bootstrap: 6 geometries are no whole families of 4",
         lambda: dp.sobol_bootstrap_ensemble(VALUES, **{**boot, "n_groups": 2})),
        ("okx_ensemble_sobol: 0 groups, 1 to ", lambda: dp.sobol_ensemble(VALUES, steps_per_geometry=S, n_groups=0)),
        (r"accumulate=True needs the accumulator to merge into \(out=\)", lambda: dp.sobol_ensemble(VALUES, accumulate=True, **sobol)),
        (r"accumulate=True needs the accumulator to merge into \(out=\)", lambda: dp.sobol_bootstrap_ensemble(VALUES, accumulate=True, **boot)),
        (r"accumulate=True needs the accumulator to merge into \(out=\)", lambda: dp.reduce_ensemble(VALUES, steps_per_geometry=S, accumulate=True)),
        (r"accumulate=True needs the accumulator to merge into \(out=\)", lambda: dp.covariance_ensemble(VALUES, steps_per_geometry=S, accumulate=True)),
        ("accumulate=True adds to out=", lambda: dp.screen_ensemble(VALUES, steps_per_geometry=S, limits=LIMITS, accumulate=True)),
        ("out= carries its own shift$", lambda: dp.sobol_ensemble(VALUES, shift=shift, out=dp.sobol_ensemble(VALUES, **sobol), **sobol)),
        ("out= carries its own shift$", lambda: dp.sobol_bootstrap_ensemble(VALUES, shift=shift, out=dp.sobol_bootstrap_ensemble(VALUES, **boot), **boot)),
        ("out= carries its own shift$", lambda: dp.reduce_ensemble(VALUES, steps_per_geometry=S, shift=shift,
                                                                   out=dp.reduce_ensemble(VALUES, steps_per_geometry=S))),
        ("out= carries its own shift and entries", lambda: dp.covariance_ensemble(VALUES, steps_per_geometry=S, entries=[0],
                                                                                  out=dp.covariance_ensemble(VALUES, steps_per_geometry=S))),
        ("out= carries its own probabilities and limits", lambda: dp.select_ensemble(VALUES, steps_per_geometry=S, probs=[0.5],
                                                                                     out=dp.select_ensemble(VALUES, steps_per_geometry=S, probs=[0.5]))),
        ("out= carries its own limits, scale and capacity", lambda: dp.screen_ensemble(
            VALUES, steps_per_geometry=S, capacity=1, out=dp.screen_ensemble(VALUES, steps_per_geometry=S, limits=LIMITS))),
        ("out= carries its own abscissa, origin, scale, degree and window", lambda: dp.curves_ensemble(
            VALUES, steps_per_geometry=S, degree=1, out=dp.curves_ensemble(VALUES, steps_per_geometry=S, abscissa=0, scale=1.0))),
        ("out= carries its own objectives and capacity", lambda: dp.front_ensemble(
            VALUES, steps_per_geometry=S, capacity=1, out=dp.front_ensemble(VALUES, steps_per_geometry=S, objectives=[(0, 0, "min")]))),
        (r"probs is needed \(or out=, which carries its own\)", lambda: dp.select_ensemble(VALUES, steps_per_geometry=S)),
        (r"limits are needed \(or out=, which carries its own\)", lambda: dp.screen_ensemble(VALUES, steps_per_geometry=S)),
        (r"abscissa and scale are needed \(or out=, which carries its own\)", lambda: dp.curves_ensemble(VALUES, steps_per_geometry=S)),
        (r"objectives are needed \(or out=, which carries its own\)", lambda: dp.front_ensemble(VALUES, steps_per_geometry=S)),
        ("mask must be a contiguous uint8 .G. device tensor", lambda: dp.sobol_ensemble(VALUES, mask=torch.zeros(2 * G, dtype=torch.uint8)[::2], **sobol)),
        ("mask must be a contiguous uint8 .G. device tensor", lambda: dp.sobol_bootstrap_ensemble(VALUES, mask=mask.to(torch.int8), **boot)),
        ("mask must be a uint8 .G. device tensor", lambda: dp.front_ensemble(VALUES, steps_per_geometry=S, objectives=[(0, 0, "min")], mask=mask[:5])),
        ("mask must have a positive stride", lambda: dp.front_ensemble(VALUES, steps_per_geometry=S, objectives=[(0, 0, "min")],
                                                                       mask=mask[:1].expand(G))),
        (r"okx_ensemble_sample: bad range \[5, 4\)", lambda: dp.sample_ensemble(PLAN, 5, 4)),
        (r"okx_ensemble_sample_families: bad range \[-1, 2\)", lambda: dp.sample_families(FAMILIES, -1, 2)),
        (r"okx_ensemble_bootstrap_weights: bad range \[-1, 3\)", lambda: dp.bootstrap_weights(4, R, 1, row_offset=-1)),
        ("okx_ensemble_sobol_bootstrap: negative family_offset", lambda: dp.sobol_bootstrap_ensemble(VALUES, family_offset=-1, **boot)),
        ("okx_ensemble_sobol_bootstrap: 1025 replicates, 1 to 1024 allowed", lambda: dp.sobol_bootstrap_ensemble(VALUES, **{**boot, "n_replicates": 1025})),
        ("okx_ensemble_bootstrap_weights: 0 replicates, 1 to 1024 allowed", lambda: dp.bootstrap_weights(4, 0, 1)),
        ("out= was taken with seed 1, not 2", lambda: dp.sobol_bootstrap_ensemble(VALUES, out=dp.sobol_bootstrap_ensemble(VALUES, **boot),
                                                                                 **{**boot, "seed": 2})),
        (r"out was prepared for \[S, K\] = \[1, 2\]", lambda: dp.select_ensemble(VALUES, steps_per_geometry=S, out=dp.select_prepare(1, K, [0.5]))),
        (r"out was prepared for \[S, K\] = \[1, 2\]", lambda: dp.screen_ensemble(VALUES, steps_per_geometry=S, out=dp.screen_prepare(1, K, LIMITS, None, G))),
        (r"the select was prepared for \[S, K\] = \[1, 2\]", lambda: dp.select_count(dp.select_prepare(1, K, [0.5], rounds=True), 0, VALUES,
                                                                                    steps_per_geometry=S)),
        (r"out holds 6 geometries: rows \[1, 7\) do not fit", lambda: dp.screen_ensemble(VALUES, steps_per_geometry=S, first_row=1,
                                                                                        out=dp.screen_prepare(S, K, LIMITS, None, G))),
        ("out holds no hardpoint table", lambda: dp.sample_ensemble(PLAN, 0, 3, out=type(dp.sample_ensemble(PLAN, 0, 3))(None, None, None, None))),
    ]
    for message, call in cases:
        dp.calls.clear()
        with pytest.raises(ValueError, match=message):
            call()
        assert len(dp.calls) <= 1, message  # (the call that made the out= of the refused one)


def test_a_mask_may_be_strided_for_the_front_alone():
    dp = Recorder()
    wide = torch.zeros((G, 5), dtype=torch.uint8)
    dp.front_ensemble(VALUES, steps_per_geometry=S, objectives=[(0, 0, "min")], mask=wide[:, 2])
    args = dp.calls[-1][1]
    at = [i for i, a in enumerate(args) if isinstance(a, C.c_void_p) and a.value == wide[:, 2].data_ptr()]
    assert len(at) == 1 and args[at[0] + 1] == 5  # the mask and, after it, its stride
    dp.front_ensemble(VALUES[:S], steps_per_geometry=S, objectives=[(0, 0, "min")], mask=wide[:1, 2])
    assert dp.calls[-1][1][at[0] + 1] == 1  # one geometry: stride 1


def test_a_plans_tables_are_made_once_and_leave_with_the_plan():
    import gc

    dp = Recorder()
    plan, families = make_plan(p=1, f=1, kinds=(NORMAL,), n_total=3), family_plan(1, 1)
    first = dp._sample_tables(plan)
    assert dp._sample_tables(plan) is first and dp._family_tables(families) is dp._family_tables(families)
    assert len(dp._sample_plans) == 3  # the plan, the family plan and the plan it wraps
    del plan, families, first
    gc.collect()
    assert len(dp._sample_plans) == 0


# ---- the accumulators (ensemble_stats.py) ----

class NoCompareArray(np.ndarray):
    def __eq__(self, other):
        raise AssertionError("the tables were compared")

    def __array_function__(self, func, types, args, kwargs):
        if func in (np.array_equal, np.array_equiv, np.allclose, np.equal):
            raise AssertionError("the tables were compared")
        return super().__array_function__(func, types, args, kwargs)


class NoCompareTensor(torch.Tensor):
    __module__ = "torch.stand_in"  # (ensemble_stats tells a tensor by its type's module, without importing torch)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if func in (torch.equal, torch.eq, torch.Tensor.eq, torch.Tensor.__eq__):
            raise AssertionError("the tables were compared")
        return super().__torch_function__(func, types, args, kwargs or {})


def guarded(table):
    return table.as_subclass(NoCompareTensor) if isinstance(table, torch.Tensor) else table.view(NoCompareArray)


def accumulators(xp, shift, entries, seed=3):
    """One of each class over ``[S, K]`` entries, tables of ``xp`` (torch or numpy) filled with distinct values."""
    def table(*shape, dtype="float64"):
        return (1 + xp.arange(int(np.prod(shape)))).reshape(shape).astype(dtype) if xp is np \
            else (1 + torch.arange(int(np.prod(shape)))).reshape(shape).to(getattr(torch, dtype))

    return {
        "reduce": EnsembleAccumulator(table(S, K, 8 + P), shift, table(factor_moment_count(P)), ["a", "b"]),
        "covariance": CovarianceAccumulator(table(2, 2), table(2), table(2, dtype="int64"), shift, entries, table(G, dtype="uint8"), natural=True),
        "sobol": SobolAccumulator(table(S, K, 9), shift, ["g"]),
        "bootstrap": SobolBootstrapAccumulator(table(R, S, K, 9), shift, seed, ["g"]),
    }


@pytest.mark.parametrize("xp", [np, torch])
def test_merge_of_one_shift_object_compares_nothing(xp):
    shift = guarded(xp.zeros((S, K), dtype=xp.float64))
    entries = guarded(xp.zeros(2, dtype=xp.int32))
    other = guarded(xp.zeros((S, K), dtype=xp.float64))
    for name, a in accumulators(xp, shift, entries).items():
        b = accumulators(xp, shift, entries)[name]
        merged = a.merge(b)
        assert merged.shift is shift and type(merged) is type(a), name
        first = "gram" if name == "covariance" else "acc"
        assert bool((getattr(merged, first) == 2 * getattr(a, first)).all()) or name == "reduce"  # (reduce: extremes are no sums)
        with pytest.raises(AssertionError, match="the tables were compared"):  # another object: by content, which these tables refuse
            a.merge(accumulators(xp, other, entries)[name])


@pytest.mark.parametrize("xp", [np, torch])
def test_merge_refusals_keep_their_texts(xp):
    zeros, ones = xp.zeros((S, K), dtype=xp.float64), xp.ones((S, K), dtype=xp.float64)
    entries, others = xp.zeros(2, dtype=xp.int32), xp.ones(2, dtype=xp.int32)
    for name, a in accumulators(xp, zeros, entries).items():
        with pytest.raises(ValueError, match="accumulators taken with different shifts cannot be merged"):
            a.merge(accumulators(xp, ones, entries)[name])
        assert a.merge(accumulators(xp, xp.zeros((S, K), dtype=xp.float64), entries)[name]) is not a  # equal content: merged
    a = accumulators(xp, zeros, entries)
    with pytest.raises(ValueError, match="accumulators of different entries cannot be merged"):
        a["covariance"].merge(accumulators(xp, zeros, others)["covariance"])
    with pytest.raises(ValueError, match="accumulators taken with different seeds cannot be merged"):
        a["bootstrap"].merge(accumulators(xp, zeros, entries, seed=4)["bootstrap"])
    for name, wrong in (("reduce", EnsembleAccumulator(xp.zeros((S, K, 9)), zeros)), ("sobol", SobolAccumulator(xp.zeros((S, K, 12)), zeros)),
                        ("bootstrap", SobolBootstrapAccumulator(xp.zeros((R + 1, S, K, 9)), zeros, 3))):
        with pytest.raises(ValueError, match="accumulators of different shapes"):
            a[name].merge(wrong)


def test_numpy_of_a_torch_accumulator_keeps_every_field():
    shift, entries = torch.full((S, K), 0.5, dtype=torch.float64), torch.tensor([0, 3], dtype=torch.int32)
    for name, a in accumulators(torch, shift, entries).items():
        host = a.numpy()
        assert type(host) is type(a) and host.numpy() is host, name
        for table in a.TABLES:
            got, want = getattr(host, table), getattr(a, table)
            assert isinstance(got, np.ndarray) and got.dtype == want.numpy().dtype and np.array_equal(got, want.numpy()), (name, table)
        for field in a.CARRIED:
            assert getattr(host, field) == (False if field in a.DEVICE_ONLY else getattr(a, field)), (name, field)
        back = host.to("cpu")
        assert all(torch.equal(getattr(back, table), getattr(a, table)) for table in a.TABLES), name
    assert accumulators(torch, shift, entries)["covariance"].to("cpu").natural is True
    bare = EnsembleAccumulator(torch.zeros((S, K, 8)), shift).numpy()
    assert bare.factor_acc is None and bare.factor_names is None
