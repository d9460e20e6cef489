"""
Per-geometry problem emission ON THE DEVICE (``okx_rebind_design``) and everything that reads its tables - the absolute
targets, every solve kernel family, the expand kernels - against the real reference on every topology: the
``rebind_<name>.npz`` fixtures (oracle/gen_golden_rebind.py; tests/rebind_reference.py for the bounds).  Four geometries of
five steps each: the smallest batch that still runs pair mode, the three-joining-row programs and the derived chains.

Measured on an MI355X when the module was written (worst over geometries, line modes and chain lengths; mm):

  topology               rebind pos  row param  families run           solved: rack pickup / other points
  (bound)                1e-12       1e-14                             6e-8 / 1e-8   (u_*: 1e-9)
  t_axle_dw              1.1e-13     2.1e-16    single quad            1.3e-8 / 3.8e-9
  t_axle_dw_explicit     1.1e-13     2.0e-16    single quad            1.8e-8 / 4.0e-9
  t_axle_macpherson      1.1e-13     4.6e-16    single quad            3.2e-8 / 7.1e-9
  t_corner_rocker        1.1e-13     1.4e-15    single packed quad     1.9e-8 / 4.7e-9
  t_corner_strut         1.1e-13     2.2e-16    single packed quad     1.8e-8 / 4.3e-9
  t_corner_strut_rocker  1.1e-13     7.9e-16    single quad            1.7e-8 / 4.7e-9
  t_axle_t_bar_bump      2.3e-13     8.7e-16    single quad            2.1e-8 / 5.4e-9
  t_axle_t_bar_roll      1.1e-13     1.7e-15    single quad            2.0e-8 / 4.5e-9
  t_axle_heave_link      1.1e-13     7.4e-16    single quad            2.1e-8 / 4.8e-9
  t_axle_t_bar_heave     2.3e-13     7.4e-16    single quad            2.1e-8 / 6.5e-9
  c3_axle_grid           1.1e-13     8.2e-16    single quad            1.4e-8 / 4.2e-9
  c4_macpherson_grid     1.1e-13     4.6e-16    single packed quad lane  2.2e-8 / 4.8e-9
  u_macpherson           1.1e-13     5.1e-16    single packed quad lane  - / 8.9e-12 (single), 1.9e-12 (quad)
  u_axle                 1.1e-13     7.4e-16    single                 - / 2.7e-10

Within a topology the families agree in every printed digit but the last.  A family is missing where the program has no
such kernel (the planner's answer, printed with the generator's notes): here the packed kernel is offered up to 8 free
points, the lane kernel up to 6 free points and not in pair mode, and u_axle has no quad kernel (no row joins its halves).
max_residual against the reference's: <= 5.7e-13 everywhere (bound 1e-8); absolute targets: 0; expand against the
reference's records: 2.3e-13 (bound 1e-11).
"""

import numpy as np
import pytest
import torch

from conftest import gpu_available, load_golden
from rebind_reference import (FREE_CLAMP, G, LINE_MODES, MACPHERSON, NAMES, PARAM_REL, POS_TOL, S, TARGET_TOL,
                              all_classes_table, clamp_contract, fixture, geometries, numpy_row_targets, param_error,
                              rack_outputs, reference_program, sweep_bounds, table)

pytestmark = pytest.mark.gpu

FAMILIES = ["single", "packed", "quad", "lane"]   # the kernel= values of DeviceProgram.solve
CHAIN_LENS = [1, -1]
_programs = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    yield
    for dp in _programs.values():
        dp.close()
    _programs.clear()


def _dp(name: str, line_mode: str):
    from open_kinematics_amd.batch import DeviceProgram

    if (name, line_mode) not in _programs:
        _programs[name, line_mode] = DeviceProgram(fixture(name)[1].with_line_mode(line_mode), "cuda:0")
    return _programs[name, line_mode]


def _rebound(name: str, line_mode: str):
    dp = _dp(name, line_mode)
    gpos, gparam = dp.rebind(torch.as_tensor(table(name), device="cuda:0"))
    return dp, gpos, gparam


def _offered(dp, family: str, chain_len: int) -> bool:
    """Whether a launch of the G x S batch with per-geometry tables can run on ``family`` (the planner's own answer)."""
    try:
        got, _ = dp.plan_launch(G * S, steps_per_geometry=S, geometry_tables=True, kernel=family, chain_len=chain_len)
    except (ValueError, RuntimeError):
        return False
    return got == family


@pytest.mark.parametrize("line_mode", LINE_MODES)
@pytest.mark.parametrize("name", NAMES)
def test_device_rebind_matches_reference_and_oracle(name, line_mode):
    from oracle.oracle import Oracle

    arrays, program = fixture(name)
    dp, gpos, gparam = _rebound(name, line_mode)
    pos, rp = gpos.cpu().numpy(), gparam.cpu().numpy()
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(rp)) and np.abs(pos).max() < 1e4, "the sentinel reached an output"
    worst_pos, worst_param = 0.0, 0.0
    for g in geometries(name):
        ref = reference_program(name, g, line_mode)
        worst_pos = max(worst_pos, float(np.max(np.abs(pos[g] - ref.design_pos))))
        worst_param = max(worst_param, param_error(rp[g], ref.row_param))
    print(f"device rebind {name} {line_mode}: positions {worst_pos:.2e} (<= {POS_TOL}), row parameters {worst_param:.2e} (<= {PARAM_REL})")
    assert worst_pos <= POS_TOL
    assert worst_param <= PARAM_REL
    orc = Oracle(program.with_line_mode(line_mode))
    for g in range(G):   # the oracle shares the documented contract: the freely moved clamp too
        pos_o, rp_o = orc.rebind(arrays["hardpoints"][g])
        assert np.max(np.abs(pos[g] - pos_o)) <= POS_TOL
        assert param_error(rp[g], rp_o) <= PARAM_REL
    # the same bits: one geometry at a time, a pinned host table, another value at the ignored entries
    host = table(name)
    for g in range(G):
        one_pos, one_rp = dp.rebind(torch.as_tensor(host[g:g + 1], device="cuda:0"))
        assert torch.equal(one_pos[0], gpos[g]) and torch.equal(one_rp[0], gparam[g])
    pin_pos, pin_rp = dp.rebind(torch.as_tensor(host).pin_memory())
    assert pin_pos.is_cuda and torch.equal(pin_pos, gpos) and torch.equal(pin_rp, gparam)
    alt_pos, alt_rp = dp.rebind(torch.as_tensor(table(name, sentinel=-3.0e5), device="cuda:0"))
    assert torch.equal(alt_pos, gpos) and torch.equal(alt_rp, gparam)


@pytest.mark.parametrize("name", NAMES)
def test_device_ensemble_targets_match_reference(name):
    arrays, _ = fixture(name)
    dp, gpos, _ = _rebound(name, "pinned")
    targets = dp.ensemble_targets(gpos, torch.as_tensor(arrays["targets_rel"], device="cuda:0"))
    assert targets.shape == (G * S, arrays["targets_abs"].shape[2])
    worst = float(np.max(np.abs(targets.cpu().numpy().reshape(G, S, -1) - arrays["targets_abs"])))
    print(f"device targets {name}: {worst:.2e} (<= {TARGET_TOL})")
    assert worst <= TARGET_TOL


@pytest.mark.parametrize("name", NAMES)
def test_every_kernel_family_solves_the_rebound_ensemble(name):
    """The G x S batch with the per-geometry tables through every family the program offers, independent and chained."""
    arrays, program = fixture(name)
    dp, gpos, gparam = _rebound(name, "pinned")
    targets = torch.as_tensor(np.ascontiguousarray(arrays["targets_abs"]).reshape(G * S, -1), device="cuda:0")
    rack_bound, other_bound = sweep_bounds(name, program)
    rack = rack_outputs(program)
    keep = geometries(name)   # a freely moved clamp is solved too, but it is another mechanism than the reference's
    ran, skipped, results = [], [], {}
    for family in FAMILIES:
        for chain_len in CHAIN_LENS:
            if not _offered(dp, family, chain_len):
                skipped.append((family, chain_len))
                continue
            res = dp.solve(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=S, kernel=family,
                           chain_len=chain_len)
            torch.cuda.synchronize()
            info = res.info()
            pos = res.positions.cpu().numpy().reshape(G, S, -1, 3)
            diff = np.abs(pos - arrays["ref_tight_pos"])[keep]
            on_rack = float(diff[:, :, rack].max()) if rack else 0.0
            elsewhere = float(np.delete(diff, rack, axis=2).max())
            maxres = float(np.max(np.abs(info["max_residual"].reshape(G, S) - arrays["ref_tight_maxres"])[keep]))
            print(f"solve {name} {family} chain_len={chain_len}: rack pickups {on_rack:.2e} (<= {rack_bound}), other points "
                  f"{elsewhere:.2e} (<= {other_bound}), max_residual {maxres:.2e} (<= 1e-8)")
            assert np.all((info["flags"] & 7) == 1), f"{family} chain_len={chain_len}: not every problem accepted"
            assert on_rack <= rack_bound and elsewhere <= other_bound
            assert maxres <= 1e-8
            results[family, chain_len] = pos
            ran.append((family, chain_len))
    print(f"families {name}: ran {sorted({f for f, _ in ran})}, not offered {sorted({f for f, _ in skipped})}"
          f" (quad: {dp.kernel_note or 'loaded'}; lane: {dp.lane_note or 'loaded'})")
    assert {f for f, _ in ran} >= {"single"}, "every program has the interpreter kernel"
    first = results[ran[0]]
    for key in ran[1:]:
        assert float(np.max(np.abs(results[key] - first))) <= 1e-9, f"{key} against {ran[0]}"


@pytest.mark.parametrize("name", NAMES)
def test_expand_rebuilds_records_from_the_geometry_tables(name):
    """Fixed points from the table, derived points re-evaluated: from the REFERENCE's free coordinates its own records, and
    from a solve's free coordinates that solve's records (interpreter form on the composed axles, generated form elsewhere)."""
    arrays, program = fixture(name)
    dp, gpos, gparam = _rebound(name, "pinned")
    index = dp.free_out_index
    keep = geometries(name)
    ref = torch.as_tensor(np.ascontiguousarray(arrays["ref_tight_pos"]).reshape(G * S, -1, 3), device="cuda:0")
    rebuilt = dp.expand(ref[:, index].contiguous(), geom_pos=gpos, steps_per_geometry=S)
    worst_ref = float((rebuilt - ref).abs().reshape(G, S, -1)[keep].max())
    targets = torch.as_tensor(np.ascontiguousarray(arrays["targets_abs"]).reshape(G * S, -1), device="cuda:0")
    res = dp.solve(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=S)
    again = dp.expand(res.positions[:, index].contiguous(), geom_pos=gpos, steps_per_geometry=S)
    worst_own = float((again - res.positions).abs().max())
    print(f"expand {name}: reference records {worst_ref:.2e}, solved records {worst_own:.2e} (<= 1e-11)")
    assert worst_ref <= 1e-11
    assert worst_own <= 1e-11


@pytest.mark.parametrize("line_mode", LINE_MODES)
@pytest.mark.parametrize("name", MACPHERSON)
def test_macpherson_clamp_offset_is_a_program_constant_on_device(name, line_mode):
    """Geometry 3 moved the authored clamp freely: the device keeps the program's offset d0 (okx.h) and ``strict`` says so."""
    arrays, program = fixture(name)
    dp, gpos, _ = _rebound(name, line_mode)
    contract = clamp_contract(name, gpos[FREE_CLAMP].cpu().numpy())
    print(f"device clamp {name} {line_mode}: {contract}")
    assert contract["on_axis"] <= 1e-12
    assert contract["from_reference"] <= 1e-12
    host = table(name)
    with pytest.raises(ValueError, match="strut_bottom"):
        dp.rebind(torch.as_tensor(host, device="cuda:0"), strict=True)
    ok_pos, _ = dp.rebind(torch.as_tensor(host[geometries(name)], device="cuda:0"), strict=True)
    assert torch.equal(ok_pos, gpos[geometries(name)])


@pytest.mark.parametrize("line_mode", LINE_MODES)
def test_every_row_class_rebinds_to_its_definition_on_device(line_mode):
    """The three-point angle row (no reference topology emits one) and every other class, against the reference's definitions."""
    from open_kinematics_amd.batch import DeviceProgram

    program = load_golden("rows_all_classes")[1].with_line_mode(line_mode)
    dp = DeviceProgram(program, "cuda:0")
    hard = all_classes_table()
    gpos, gparam = dp.rebind(torch.as_tensor(hard, device="cuda:0"))
    assert np.array_equal(gpos.cpu().numpy(), hard)
    for g in range(len(hard)):
        assert param_error(gparam[g].cpu().numpy(), numpy_row_targets(program, hard[g])) <= PARAM_REL
    dp.close()
