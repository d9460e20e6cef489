#!/usr/bin/env python3
"""The sweep-diagnostics pass (okx_diagnose_sweeps_batch) on BASELINE config 5's solved records - 4096 perturbed
double-wishbone geometries x 256 steps, 1 048 576 states - timed with HIP events after warm-up:
  (a) the pass over records [B][n_out][3] and over free coordinates [B][n_free][3], with the solve's okx_info and every
      geometry's own design table;
  (b) okx_corner_metrics_batch on the same records: a kernel that streams the same bytes per state once - the yardstick
      (the pass over records should take at most twice its time);
  (c) the host NumPy path (diagnostics.diagnose_arrays) on the same data, copy from the device included and apart.
Prints a table and, with --json PATH, writes the figures (implied bytes/s against the HBM rate given by --hbm-gbs).
   python3 tools/diagnose_rate.py [--geometries 4096] [--steps 256] [--json profiles/diagnose_rate.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from open_kinematics_amd import diagnostics as dg
from open_kinematics_amd.batch import DeviceProgram
from open_kinematics_amd.input import load_geometry
from open_kinematics_amd.metrics import corner_roles, corner_state_metrics
from open_kinematics_amd.workloads import ensemble_problem, geometry_path

ap = argparse.ArgumentParser()
ap.add_argument("--geometries", type=int, default=4096)
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate the implied bytes/s are set against (peak: 8000)")
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


G, S = args.geometries, args.steps
program, table, rel = ensemble_problem(G, S)
dp = DeviceProgram(program, dev)
gpos, gparam = dp.rebind(torch.as_tensor(table, device=dev))
targets = dp.ensemble_targets(gpos, torch.as_tensor(rel, device=dev))
res = dp.solve(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=S, chain_len=-1)
pos, info = res.positions, res.info_raw
free = pos[:, dp.free_out_index].contiguous()
sus = load_geometry(geometry_path("geometry.yaml"))
roles = dg.diag_roles(sus, program)
n = G * S
out = (torch.empty((G, 80), dtype=torch.uint8, device=dev), torch.empty((4096, 40), dtype=torch.uint8, device=dev),
       torch.empty(1, dtype=torch.int64, device=dev))
rows = {}


def row(name, ms, bytes_per_state):
    gbs = bytes_per_state * n / ms / 1e6
    rows[name] = {"ms": round(ms, 4), "states_per_s": n / ms * 1e3, "bytes_per_state": bytes_per_state,
                  "implied_gbs": round(gbs, 1), "hbm_frac": round(gbs / args.hbm_gbs, 3)}
    print(f"{name:44s} {ms:9.4f} ms  {n / ms * 1e3:10.3g} states/s  {bytes_per_state:4d} B/state  {gbs:7.0f} GB/s  {gbs / args.hbm_gbs:.3f} of {args.hbm_gbs:.0f} GB/s")


ms_records = timed(lambda: dp.diagnose(pos, info, steps_per_sweep=S, roles=roles, geom_pos=gpos, out=out), args.reps)
row("diagnose, records (+ info)", ms_records, 24 * program.n_out + 40)
ms = timed(lambda: dp.diagnose(free, info, steps_per_sweep=S, layout="free", roles=roles, geom_pos=gpos, out=out), args.reps)
row("diagnose, free coordinates (+ info)", ms, 24 * program.n_free + 40)
ms = timed(lambda: dp.diagnose(pos, None, steps_per_sweep=S, roles=roles, geom_pos=gpos, out=out), args.reps)
row("diagnose, records, no info", ms, 24 * program.n_out)
croles = corner_roles(sus, program)
ms_metrics = timed(lambda: corner_state_metrics(croles, pos, None), args.reps)
row("okx_corner_metrics_batch (yardstick)", ms_metrics, 24 * program.n_out + 8 * 19)
found = int(out[2].item())

out_rows = [int(k) for k in program.out_point]
rows_np = dg.DiagRoles([out_rows.index(int(p)) for p in roles.points], roles.names)
t0 = time.perf_counter()
host_pos = pos.cpu().numpy()
host_info = res.info()
t1 = time.perf_counter()
summary, records = dg.diagnose_arrays(host_pos, rows_np, np.zeros((program.n_out, 3)), steps_per_sweep=S,
                                      converged=res.converged(host_info), max_residual=host_info["max_residual"])
t2 = time.perf_counter()
print(f"{'host NumPy path':44s} {1e3 * (t2 - t1):9.1f} ms  (+ {1e3 * (t1 - t0):.1f} ms device -> host copy of {host_pos.nbytes / 1e6:.0f} MB); "
      f"{len(records)} issues on the host, {found} on the device")
ratio = ms_records / ms_metrics
print(f"diagnose over records / okx_corner_metrics_batch = {ratio:.2f}  (yardstick: at most 2)")
if args.json:
    with open(args.json, "w", encoding="utf-8") as fh:
        json.dump({"geometries": G, "steps": S, "states": n, "tracked_points": len(roles.points), "reps": args.reps,
                   "device": torch.cuda.get_device_name(dev), "kernels": rows, "ratio_to_corner_metrics": round(ratio, 3),
                   "host_numpy_ms": round(1e3 * (t2 - t1), 1), "host_copy_ms": round(1e3 * (t1 - t0), 1),
                   "issues_found": found}, fh, indent=1)
        fh.write("\n")
