"""
Prints the NOISE / AXLE_NOISE tables of tests/test_gpu_metric_derivatives.py: per derivative column, the largest
|float64 - 50-digit| of the oracle's duals relative to max(1, |d|), over the states, directions and role sets that module
uses - for the axle-scope columns also every state of the four axle fixtures' own sweeps, which
tests/test_gpu_axle_evaluated.py evaluates (the oracle's tangents and sweep states stand in for the device's, which agree
with them to 1e-9).  CPU only, needs mpmath:

    python -m oracle.measure_metric_noise
"""

from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main() -> None:
    import mpmath

    import test_gpu_metric_derivatives as cases
    import test_metrics_oracle as shared
    from conftest import load_golden
    from oracle.metrics_oracle import AXLE_METRIC_NAMES, METRIC_NAMES, axle_metric_duals, catalog_duals
    from oracle.oracle import Oracle

    mpmath.mp.dps = 50
    noise, axle_noise = dict.fromkeys(METRIC_NAMES, 0.0), dict.fromkeys(AXLE_METRIC_NAMES, 0.0)

    def measure(table, names, fn):
        _, d64 = fn(float)
        _, dmp = fn(mpmath.mpf)
        for k, name in enumerate(names):
            if not np.isnan(dmp[k]):
                table[name] = max(table[name], abs(d64[k] - dmp[k]) / max(1.0, abs(dmp[k])))

    def corner(spec, states, fields):
        for s in range(states.shape[0]):
            for vel in fields(s):
                measure(noise, METRIC_NAMES, lambda number: catalog_duals(spec, states[s], vel, number))

    golden = lambda name: load_golden(name)  # noqa: E731
    for name in cases.CORNER_CASES:
        program, _, spec, states = cases.corner_case(golden, name)
        n = min(states.shape[0], 65)
        rnd = cases.random_velocities((n, program.n_targets, program.n_out, 3), 20)
        corner(spec, states, lambda s: list(shared.oracle_tangents(program, states[s])) + (list(rnd[s]) if s < n else []))
    for name, (spec, states) in cases.c1_role_sets(golden).items():
        program, _, _, solved = cases.corner_case(golden, "c1_dw_corner")
        sign = np.array([1.0, -1.0 if name == "mirrored" else 1.0, 1.0])
        corner(spec, states, lambda s: list(shared.oracle_tangents(program, solved[s]) * sign))
    for name, base in shared.AXLE_GOLDENS.items():
        arrays, program = load_golden(base)
        mg = shared.load_metrics_golden(name)
        names, design, states = shared.out_names(program), program.design_pos[program.out_point], mg["pos"]
        left, right = (shared.corner_spec(names, design, mg, f"{tag}_", f"{tag}_") for tag in ("left", "right"))
        rnd = cases.random_velocities((states.shape[0], program.n_targets, program.n_out, 3), 21)
        for s in range(states.shape[0]):
            tangents = list(shared.oracle_tangents(program, states[s]))
            for vel in tangents:
                measure(axle_noise, AXLE_METRIC_NAMES, lambda number: axle_metric_duals(left, right, states[s], vel, number))
            if name in ("axle_c3", "axle_t_bar_roll"):
                for spec in (left, right):
                    for vel in tangents + (list(rnd[s]) if name == "axle_c3" else []):
                        measure(noise, METRIC_NAMES, lambda number: catalog_duals(spec, states[s], vel, number))
        # ... and every state of the fixture's own sweep (tests/test_gpu_axle_evaluated.py evaluates the solved sweep)
        sweep = Oracle(program).sweep(arrays["targets_abs"], 1e-15, 1e-15, 1e-15, warm_start=True).positions
        for row in sweep:
            for vel in shared.oracle_tangents(program, row):
                measure(axle_noise, AXLE_METRIC_NAMES, lambda number: axle_metric_duals(left, right, row, vel, number))
    # the rotation / hardware roles of the two axles whose blocks the module compares whole
    from oracle.metrics_oracle import ROLE_KINDS, role_dual

    role_noise = dict.fromkeys(ROLE_KINDS, 0.0)
    for name in ("axle_c3", "axle_t_bar_roll"):
        arrays, program = load_golden(shared.AXLE_GOLDENS[name])
        states = shared.load_metrics_golden(name)["pos"]
        for _, kind, a, b, *rest in shared.fixture_roles(arrays, program):
            for row in states:
                for vel in shared.oracle_tangents(program, row):
                    measure(role_noise, [kind], lambda number: [np.array([x]) for x in role_dual(kind, row[a], vel[a], row[b], vel[b], *rest, number=number)])
    for title, table in (("NOISE", noise), ("AXLE_NOISE", axle_noise), ("ROLE_NOISE", role_noise)):
        print(title, "= {" + ", ".join(f'"{k}": {v:.1e}' for k, v in table.items()) + "}")


if __name__ == "__main__":
    main()
