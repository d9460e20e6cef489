"""
The launch planner (csrc/okx_launch.cpp) through okx_debug_plan_launch: which kernel family, chain length and start mode a
launch resolves to, from hand-made capabilities - no device.

The expected (status, family, chain length, error text) of every row below were recorded from the selection as it stood
BEFORE the planner was split out of solve_impl (that code run on the same capabilities through a throw-away hook), not from
the planner; the start mode / auto-cold / confirm columns of the rows that name them follow from reading that code.
"""

import ctypes as C

import pytest

from conftest import gpu_available, load_golden
from open_kinematics_amd import _lib
from open_kinematics_amd._abi import LaunchCaps, SolveOpts

INTERPRETER, PACKED, QUAD, LANE = 1, 2, 3, 4
COLD, CHAIN, NESTED, REFINED = 0, 1, 2, 3

# a double-wishbone corner (18 unknowns; the lane kernel's chain body is not for auto selection) and a MacPherson strut
# (15 unknowns, both lane bodies) on 256 compute units
DW = dict(lane_min_problems=256 * 64 + 1, n_cu=256, n=18, nreg=18, n_targets=1, blocks_per_cu=8, packed_blocks_per_cu=8, groups=3,
          has_packed=1, has_quad=1, quad_ppw=16, quad_waves_per_cu=4, has_head=1, has_cold=1, has_lane=1, lane_cold_ok=1,
          lane_chain_ok=0, has_nest=1)
MAC = dict(DW, n=15, nreg=15, groups=4, lane_chain_ok=1)
BASES = {"DW": DW, "MAC": MAC}

# (id, base, capability overrides, n_problems, geometry tables, evaluated, option overrides,
#  (status, family, chain length as okx_plan_launch reports it, error text))
ROWS = [
    ('independent_16384_stays_on_quad', 'DW', {}, 16384, 0, 0, {'chain_len': 1},
     (0, 3, 1, '')),
    ('independent_16385_goes_to_lane', 'DW', {}, 16385, 0, 0, {'chain_len': 1},
     (0, 4, 1, '')),
    ('ensemble_of_4_steps_back_to_quad', 'DW', {}, 32768, 1, 0, {'steps_per_geometry': 4, 'chain_len': 1},
     (0, 3, 1, '')),
    ('ensemble_of_256_steps_on_lane', 'DW', {}, 1048576, 1, 0, {'steps_per_geometry': 256, 'chain_len': 1},
     (0, 4, 1, '')),
    ('auto_cold_where_chain_body_spills', 'DW', {'has_nest': 0}, 65536, 1, 0, {'steps_per_geometry': 64, 'chain_len': -1},
     (0, 4, 1, '')),
    ('auto_chain_without_cold_body_goes_to_quad', 'DW', {'has_nest': 0, 'lane_cold_ok': 0}, 65536, 1, 0, {'steps_per_geometry': 64, 'chain_len': -1},
     (0, 3, 4, '')),
    ('nested_span_256', 'DW', {}, 1048576, 1, 0, {'steps_per_geometry': 256, 'chain_len': -1},
     (0, 4, -1, '')),
    ('nested_span_2048', 'DW', {}, 131072, 1, 0, {'steps_per_geometry': 2048, 'chain_len': -1},
     (0, 4, -1, '')),
    ('nested_span_3000_is_long_enough', 'DW', {}, 192000, 1, 0, {'steps_per_geometry': 3000, 'chain_len': -1},
     (0, 4, -1, '')),
    ('not_nested_span_1000', 'DW', {}, 64000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1},
     (0, 4, 1, '')),
    ('not_nested_when_evaluated', 'DW', {'ev_enabled': 1, 'ev_lane': 1}, 1048576, 1, 1, {'steps_per_geometry': 256, 'chain_len': -1},
     (0, 4, 1, '')),
    ('refine_present', 'DW', {'has_nest': 0, 'has_refine': 1}, 64000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1},
     (0, 4, 1, '')),
    ('refine_absent', 'MAC', {'has_nest': 0, 'has_refine': 0}, 64000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1},
     (0, 4, 1, '')),
    ('refine_not_with_output_none', 'MAC', {'has_nest': 0, 'has_refine': 1}, 64000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1, 'output': 2},
     (0, 4, 1, '')),
    ('refine_not_with_gradient_stop', 'MAC', {'has_nest': 0, 'has_refine': 1}, 64000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1, 'grad_tol': 1e-09},
     (0, 4, 1, '')),
    ('kernel_4_without_lane', 'DW', {'has_lane': 0}, 100000, 0, 0, {'kernel': 4},
     (-1, 0, 0, 'lane kernel requested but not available: lane note')),
    ('kernel_4_with_predictor', 'DW', {}, 100000, 0, 0, {'kernel': 4, 'predictor': 1},
     (-1, 0, 0, 'lane kernel requested but not available: lane note')),
    ('kernel_3_without_quad', 'DW', {'has_quad': 0, 'has_lane': 0}, 1000, 0, 0, {'kernel': 3},
     (-1, 0, 0, 'quad kernel requested but not available: quad note')),
    ('kernel_4_forces_lane_below_threshold', 'DW', {}, 64, 0, 0, {'kernel': 4, 'chain_len': 1},
     (0, 4, 1, '')),
    ('trace_keeps_quad', 'DW', {'trace': 1}, 100000, 0, 0, {'chain_len': 1},
     (0, 3, 1, '')),
    ('evaluated_without_enable', 'DW', {}, 1000, 0, 1, {},
     (-1, 0, 0, 'evaluated solves need okx_program_enable_evaluation first: evaluation note')),
    ('evaluated_on_interpreter_refused', 'DW', {'ev_enabled': 1}, 1000, 0, 1, {'kernel': 1},
     (-1, 0, 0, 'evaluated solves run the generated kernels only (kernel = 0, 3 or 4)')),
    ('evaluated_independent_on_lane', 'DW', {'ev_enabled': 1, 'ev_lane': 1}, 100000, 0, 1, {'chain_len': 1},
     (0, 4, 1, '')),
    ('evaluated_chain_goes_to_quad', 'MAC', {'ev_enabled': 1, 'ev_lane': 1}, 1048576, 1, 1, {'steps_per_geometry': 256, 'chain_len': 8},
     (0, 3, 8, '')),
    ('evaluated_kernel_4_chain_refused', 'MAC', {'ev_enabled': 1, 'ev_lane': 1}, 1048576, 1, 1, {'steps_per_geometry': 256, 'chain_len': 8, 'kernel': 4},
     (-1, 0, 0, 'no evaluated lane kernel for this launch: chains')),
    ('evaluated_kernel_4_without_lane_form', 'MAC', {'ev_enabled': 1, 'ev_lane': 0}, 100000, 0, 1, {'chain_len': 1, 'kernel': 4},
     (-1, 0, 0, 'no evaluated lane kernel for this launch: evaluation note')),
    ('packed_auto_nreg_15', 'MAC', {'has_quad': 0, 'has_lane': 0}, 16384, 0, 0, {},
     (0, 2, 1, '')),
    ('packed_auto_nreg_15_below_8_per_slot', 'MAC', {'has_quad': 0, 'has_lane': 0}, 16383, 0, 0, {},
     (0, 1, 1, '')),
    ('packed_auto_not_for_nreg_18', 'DW', {'has_quad': 0, 'has_lane': 0}, 16384, 0, 0, {},
     (0, 1, 1, '')),
    ('packed_forced_nreg_18', 'DW', {'has_quad': 0, 'has_lane': 0}, 1000, 0, 0, {'kernel': 2},
     (0, 2, 1, '')),
    ('packed_request_without_packed_kernel', 'DW', {'has_quad': 0, 'has_lane': 0, 'has_packed': 0}, 1000, 0, 0, {'kernel': 2},
     (0, 1, 1, '')),
    ('interpreter_forced_on_quad_program', 'DW', {}, 1000, 0, 0, {'kernel': 1, 'chain': 1},
     (0, 1, 1000, '')),
    ('auto_chain_len_lane_multiples_of_64', 'MAC', {'has_nest': 0}, 512000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1},
     (0, 4, 8, '')),
    ('auto_chain_len_lane_rounds_67_chains_to_128', 'MAC', {'has_nest': 0}, 983000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1},
     (0, 4, 8, '')),
    ('auto_chain_len_quad_same_batch', 'MAC', {'has_nest': 0}, 983000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1, 'kernel': 3},
     (0, 3, 59, '')),
    ('auto_chain_len_quad_no_rounding', 'MAC', {'has_nest': 0, 'has_lane': 0}, 512000, 1, 0, {'steps_per_geometry': 1000, 'chain_len': -1},
     (0, 3, 32, '')),
    ('auto_chain_len_single_sweep', 'MAC', {'has_nest': 0}, 1048576, 0, 0, {'chain_len': -1},
     (0, 4, 16, '')),
    ('auto_chain_len_small_batch_is_cold', 'MAC', {}, 1000, 0, 0, {'chain_len': -1},
     (0, 3, 1, '')),
    ('chain_flag_whole_span', 'MAC', {}, 1616, 1, 0, {'steps_per_geometry': 101, 'chain': 1},
     (0, 3, 101, '')),
    ('chain_len_beyond_span_is_clamped', 'MAC', {}, 1024, 1, 0, {'steps_per_geometry': 64, 'chain_len': 1000000},
     (0, 3, 64, '')),
    ('confirm_forced_by_line_row', 'DW', {'line_row': 1}, 1000, 0, 0, {'chain_len': 1},
     (0, 3, 1, '')),
]

# start mode, auto-cold and confirm of the rows that are about them
MODES = {
    "independent_16385_goes_to_lane": (COLD, 0, 0),
    "auto_cold_where_chain_body_spills": (COLD, 1, 0),
    "auto_chain_without_cold_body_goes_to_quad": (CHAIN, 0, 0),
    "nested_span_256": (NESTED, 0, 0),
    "nested_span_2048": (NESTED, 0, 0),
    "nested_span_3000_is_long_enough": (NESTED, 0, 0),
    "not_nested_span_1000": (COLD, 1, 0),
    "refine_present": (REFINED, 1, 0),
    "refine_absent": (COLD, 0, 0),
    "refine_not_with_output_none": (COLD, 0, 0),
    "refine_not_with_gradient_stop": (COLD, 0, 0),
    "evaluated_chain_goes_to_quad": (CHAIN, 0, 0),
    "confirm_forced_by_line_row": (COLD, 0, 1),
    "independent_16384_stays_on_quad": (COLD, 0, 0),
}


NOTES = (b"quad note", b"lane note", b"evaluation note")  # what the rows' program says about its missing kernels


def _plan(caps: dict, n_problems: int, geometry_tables: int, evaluated: int, options: dict, notes=NOTES):
    lib = _lib.load()
    lib.okx_debug_plan_notes(*notes)
    opts = SolveOpts()
    lib.okx_default_opts(C.byref(opts))
    for key, value in options.items():
        setattr(opts, key, value)
    out = (C.c_int32 * 6)()
    rc = lib.okx_debug_plan_launch(C.byref(LaunchCaps(**caps)), C.byref(opts), n_problems, geometry_tables, evaluated, C.byref(out))
    return rc, list(out), (_lib.last_error() if rc else "")


@pytest.mark.parametrize("row", ROWS, ids=[row[0] for row in ROWS])
def test_plan_matches_the_selection_before_the_split(row):
    name, base, over, n_problems, geometry_tables, evaluated, options, expected = row
    rc, out, error = _plan(dict(BASES[base], **over), n_problems, geometry_tables, evaluated, options)
    assert (rc, out[0], out[1], error) == expected
    if name in MODES:
        assert tuple(out[2:5]) == MODES[name]
    if rc == 0:
        assert out[5] >= 1


def test_error_texts_of_a_program_without_notes():
    """A program whose kernels all attached has empty notes: the refusals then end differently (read off the selection
    before the split: `lane_note[0] ? lane_note : "predictor / trace in use"`, `ev_note[0] ? ": " : ""`)."""
    empty = (b"", None, b"")
    assert _plan(DW, 100000, 0, 0, dict(kernel=4, predictor=1), empty) == (
        -1, [0] * 6, "lane kernel requested but not available: predictor / trace in use")
    assert _plan(dict(DW, trace=1), 100000, 0, 0, dict(kernel=4), empty)[2] == "lane kernel requested but not available: predictor / trace in use"
    assert _plan(DW, 1000, 0, 1, {}, empty) == (-1, [0] * 6, "evaluated solves need okx_program_enable_evaluation first")
    assert _plan(dict(DW, has_quad=0, has_lane=0), 1000, 0, 0, dict(kernel=3), empty)[2] == "quad kernel requested but not available: "
    assert _plan(dict(MAC, ev_enabled=1), 100000, 0, 1, dict(chain_len=1, kernel=4), empty)[2] == "no evaluated lane kernel for this launch: "


def test_refined_rows_differ_only_in_the_start_mode():
    """refine present against absent on the same program: same family; present resolves to four strided cold launches"""
    caps = dict(MAC, has_nest=0, lane_chain_ok=0)
    options = dict(steps_per_geometry=1000, chain_len=-1)
    _, absent, _ = _plan(dict(caps, has_refine=0), 64000, 1, 0, options)
    _, present, _ = _plan(dict(caps, has_refine=1), 64000, 1, 0, options)
    assert absent[:4] == [LANE, 1, COLD, 1] and present[:4] == [LANE, 1, REFINED, 1]


def test_grid_sizes():
    """one wavefront per SIMD for the lane kernel, quad_waves_per_cu per CU for the quad kernel, never an empty grid"""
    assert _plan(DW, 16385, 0, 0, dict(chain_len=1))[1][5] == (16385 + 63) // 64
    assert _plan(DW, 1 << 20, 0, 0, dict(chain_len=1))[1][5] == 256 * 4
    assert _plan(DW, 100, 0, 0, dict(chain_len=1))[1][5] == (100 + 15) // 16
    assert _plan(DW, 16384, 0, 0, dict(chain_len=1))[1][5] == 256 * 4
    assert _plan(dict(DW, has_quad=0, has_lane=0), 5, 0, 0, {})[1][5] == 5


def _evaluate(caps: dict, n_problems: int, steps_per_geometry: int = 0):
    out = (C.c_int32 * 2)()
    assert _lib.load().okx_debug_plan_evaluate(C.byref(LaunchCaps(**caps)), n_problems, steps_per_geometry, C.byref(out)) == 0
    return out[0]


def test_evaluate_batch_lane_or_quad():
    """okx_evaluate_batch: the lane form once every SIMD has a wave unit (units >= 4 n_cu) whose lanes are at least 3/4 full
    (n >= 48 units); read off the entry point as it stood before the split."""
    caps = dict(DW, ev_enabled=1, ev_lane=1, ev_lane_pos=1)
    simds = 4 * 256
    assert _evaluate(caps, 64 * simds) == 1
    assert _evaluate(caps, 64 * (simds - 1)) == 0                        # units = 4 n_cu - 1
    assert _evaluate(caps, 64 * (simds - 1) + 1) == 1                    # units = 4 n_cu
    assert _evaluate(caps, 48 * 2048, steps_per_geometry=48) == 1        # n = 48 units
    assert _evaluate(caps, 47 * 2048, steps_per_geometry=47) == 0        # n = 47 units
    assert _evaluate(dict(caps, ev_lane_pos=0), 64 * simds) == 0         # no lane form of the epilogue
    assert _evaluate(dict(caps, evaluate_quad=1), 64 * simds) == 0       # developer switches
    assert _evaluate(dict(caps, evaluate_lane=1), 64) == 1
    assert _evaluate(dict(caps, evaluate_lane=1, evaluate_quad=1), 64) == 0


def test_hook_rejects_bad_requests():
    assert _plan(DW, 0, 0, 0, {})[0] == -1
    assert _plan(DW, 10, 0, 0, dict(steps_per_geometry=3))[2] == "n_problems must be a multiple of steps_per_geometry"
    assert _plan(dict(DW, quad_ppw=0), 10, 0, 0, {})[0] == -1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c1_dw_corner", "c4_macpherson_grid", "c3_axle_grid"])
def test_program_caps_plan_like_okx_plan_launch(name):
    """The capabilities the launch path fills for a live program, planned through the hook, against okx_plan_launch on
    the program itself: same status, same (family, chain length).  Nothing is launched."""
    if not gpu_available():
        pytest.skip("no GPU")
    from open_kinematics_amd.batch import DeviceProgram

    _, program = load_golden(name)
    dp = DeviceProgram(program, "cuda:0")
    lib = _lib.load()
    caps = LaunchCaps()
    assert lib.okx_debug_program_caps(dp._handle, C.byref(caps)) == 0, _lib.last_error()
    assert caps.n_cu > 0 and caps.n == program.n_vars
    seen = set()
    for n in (1, 16, 16384, 16385, 65536):
        for spg in (0, 4, 256):
            for tables in (0, 1):
                for chain_len in (-1, 0, 1):
                    opts = dp.default_opts()
                    opts.steps_per_geometry, opts.chain_len = spg, chain_len
                    out6, out2 = (C.c_int32 * 6)(), (C.c_int32 * 2)()
                    rc_hook = lib.okx_debug_plan_launch(C.byref(caps), C.byref(opts), n, tables, 0, C.byref(out6))
                    rc_live = lib.okx_plan_launch(dp._handle, C.byref(opts), n, tables, 0, C.byref(out2))
                    assert (rc_hook, out6[0], out6[1]) == (rc_live, out2[0], out2[1]), (n, spg, tables, chain_len)
                    seen.add((rc_live, out2[0]))
    assert (0, QUAD) in seen
