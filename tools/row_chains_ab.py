#!/usr/bin/env python3
"""A/B of the batched norm chains: the serial text (OKX_DEV=quad_serial_chains) against the default build as two programs of
one process, builds alternated, kernel = quad: five repetitions each of bench.time_launches after 60 ms of the same launch,
and the outputs of the two compared bit for bit.  Cases: c2 (the headline launch), c2_chained, mac16k, c3, c3_chained, tbar,
c4_quad.  Both texts should be in the kernel cache (build() compiles the serial text of the corner, MacPherson and axle
programs), or the first creation compiles in place.
   python3 tools/row_chains_ab.py out.json c2 c3 tbar"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import bench
from open_kinematics_amd.batch import DeviceProgram
from open_kinematics_amd.workloads import axle_grid_problem, bump_sweep_problem, macpherson_grid_problem

dev = torch.device("cuda:0")
out_path, serial, names = sys.argv[1], "quad_serial_chains", sys.argv[2:]
REPS, STEPS = 5, 2000


def fixture_line(name, n=16384):
    from conftest import load_golden
    arrays, program = load_golden(name)
    program = program.with_line_mode("pinned")
    t = arrays["targets_abs"].reshape(-1, program.n_targets)
    lo, hi = t.min(axis=0), t.max(axis=0)
    return program, lo + np.linspace(0.1, 0.9, n)[:, None] * (hi - lo)


CASES = {"c2": (lambda: bump_sweep_problem(16384), 1, STEPS), "c2_chained": (lambda: bump_sweep_problem(16384), 16, STEPS),
         "c3": (lambda: axle_grid_problem(256, 256), 1, 200), "c3_chained": (lambda: axle_grid_problem(256, 256), -1, 200),
         "tbar": (lambda: fixture_line("t_axle_t_bar_roll"), 1, 500),
         "c4_quad": (lambda: macpherson_grid_problem(512, 512), 1, 50), "mac16k": (lambda: macpherson_grid_problem(128, 128), 1, STEPS)}
record = {}
for name in names:
    make, chain_len, steps = CASES[name]
    program, t = make()
    targets = torch.as_tensor(t, device=dev)
    n = targets.shape[0]
    built = {}
    for tag, switch in (("serial", serial), ("default", "")):
        os.environ["OKX_DEV"] = switch
        t0 = time.perf_counter()
        dp = DeviceProgram(program, dev)
        assert dp.kernel == "quad", dp.kernel_note
        out = torch.zeros((n, program.n_out, 3), dtype=torch.float64, device=dev)
        info = torch.zeros((n, 40), dtype=torch.uint8, device=dev)
        launch = dp.plan(targets, out=out, info_out=info, chain_len=chain_len, predictor=False, kernel="quad")
        launch()
        torch.cuda.synchronize()
        built[tag] = (dp, out, info, launch, time.perf_counter() - t0)
    os.environ["OKX_DEV"] = ""
    same = bool(torch.equal(built["serial"][1], built["default"][1]) and torch.equal(built["serial"][2], built["default"][2]))
    ms = {"serial": [], "default": []}
    for rep in range(REPS):
        for tag in ("serial", "default"):
            launch = built[tag][3]
            until = time.perf_counter() + 0.06
            while time.perf_counter() < until:
                launch()
                torch.cuda.synchronize()
            ms[tag].append(bench.time_launches(launch, steps, 10, dev)[1])
    nfev, ok = bench.info_summary(built["default"][2])
    gain = 1.0 - float(np.median(ms["default"])) / float(np.median(ms["serial"]))
    record[name] = {"problems": n, "chain_len": chain_len, "steps": steps, "serial_ms": ms["serial"], "default_ms": ms["default"],
                    "median_gain": gain, "slowest_default_beats_fastest_serial": max(ms["default"]) < min(ms["serial"]),
                    "outputs_bit_equal": same, "lm_evaluations_mean": nfev, "all_converged": ok,
                    "create_s": {k: v[4] for k, v in built.items()}}
    print(name, json.dumps(record[name]), flush=True)
    for dp, *_ in built.values():
        dp.close()
    with open(out_path, "w") as fh:
        json.dump(record, fh, indent=1)
