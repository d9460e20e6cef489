"""
What the tools/ensemble_*_rate.py share: the timers (device events, the interquartile spread, a host-timed step), the
alternated-blocks loop, the set-up of a rehearsal rank and the launch of the rehearsal's child processes, the common options
and the tail of ``main``.  A tool keeps what is its own: its workload, what it measures, its JSON, its port base.
"""

from __future__ import annotations

import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(REPO, "tools"), REPO):
    if path not in sys.path:
        sys.path.insert(0, path)


def events(fn, n: int) -> list:
    """The runs [us] of ``fn`` between device events, one pair per repetition."""
    import torch

    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def spread(runs) -> float:
    """The interquartile range."""
    q = statistics.quantiles(runs, n=4)
    return q[2] - q[0]


def step_ms(fn, n: int) -> float:
    """The host time [ms] of one of ``n`` calls of ``fn``, the device drained before and after."""
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def alternated(passes: dict, reps: int, warm: int = 5) -> dict:
    """The runs [us] of every pass of ``passes``: ``warm`` calls of each, then four blocks of ``reps // 4`` repetitions, the passes
    alternated block by block so that a drift hits all of them alike."""
    import torch

    for fn in passes.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in passes}
    for _ in range(4):
        for name, fn in passes.items():
            runs[name] += events(fn, max(1, reps // 4))
    return runs


def timed(passes: dict, reps: int) -> dict:
    """``alternated`` after three warm-up calls, every pass as ``{"median", "interquartile", "runs"}``."""
    return {name: {"median": statistics.median(r), "interquartile": spread(r), "runs": r} for name, r in alternated(passes, reps, warm=3).items()}


@contextlib.contextmanager
def rank(args):
    """Rank ``args.rank`` of ``args.rehearse`` over gloo at ``args.port``, every rank on ``cuda:0`` (the device is yielded); a barrier
    and the group's end after the body."""
    import torch
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(args.port)
    dist.init_process_group("gloo", rank=args.rank, world_size=args.rehearse)
    yield torch.device("cuda:0")
    dist.barrier()
    dist.destroy_process_group()


def rehearse(args, script: str, base_port: int, extra_argv, span: int = 2000) -> int:
    """``args.rehearse`` fresh child processes of ``script``, one per rank, at a port of the tool's own range; the largest exit
    status, 124 when a child outlives ``args.timeout`` (then all are killed)."""
    port = base_port + os.getpid() % span
    procs = [subprocess.Popen([sys.executable, os.path.abspath(script), "--rehearse", str(args.rehearse), "--rank", str(r), "--port", str(port),
                               *(str(a) for a in extra_argv), "--out", args.out])
             for r in range(args.rehearse)]
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=args.timeout))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            return 124
    return max(abs(c) for c in codes)


def parser(rehearsal: bool = True, timeout: float = 500.0, **sizes) -> argparse.ArgumentParser:
    """The options the tools share: ``--out``; with ``rehearsal`` ``--rehearse``, ``--rank``, ``--port`` and ``--timeout``; and one
    integer option per entry of ``sizes`` (``steps_per_geometry=256``: ``--steps-per-geometry``), in that order."""
    ap = argparse.ArgumentParser()
    for name, default in sizes.items():
        ap.add_argument("--" + name.replace("_", "-"), type=int, default=default)
    ap.add_argument("--out", default="")
    if rehearsal:
        ap.add_argument("--rehearse", type=int, default=0)
        ap.add_argument("--rank", type=int, default=-1)
        ap.add_argument("--port", type=int, default=0)
        ap.add_argument("--timeout", type=float, default=timeout)
    return ap


def run(args, measure, summary=None, rank_main=None, rehearse_main=None, echo: bool = True) -> int:
    """The tail of every tool's ``main``: a rehearsal rank, the rehearsal, or the measurement - its JSON printed (``echo``) and
    written to ``args.out``, its summary (where the tool has one) printed and written beside it as ``.txt``."""
    if getattr(args, "rehearse", 0):
        if args.rank >= 0:
            rank_main(args)
            return 0
        return rehearse_main(args)
    result = measure(args)
    text = json.dumps(result, indent=1)
    if echo:
        print(text)
    if summary is not None:
        print(summary(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")
        if summary is not None:
            with open(os.path.splitext(args.out)[0] + ".txt", "w", encoding="utf-8") as fh:
                fh.write(summary(result))
    return 0
