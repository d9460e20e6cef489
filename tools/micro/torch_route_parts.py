"""Where the torch comparison route of tools/ensemble_surface_rate.py spends its time: its operations one by one on synthetic tensors of
the measured shapes (S = 256, K = 4; status as byte 32 of 40-byte records), device events, median of 20 after 3 warm-up calls."""
import statistics
import sys

import torch

dev = torch.device("cuda:0")
s, k = 256, 4


def med(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


lines = []
for g in (4096, 131072):
    table = torch.randn((g * s, k), dtype=torch.float64, device=dev)
    info = torch.ones((g * s, 40), dtype=torch.uint8, device=dev)
    status = info[:, 32]
    for t, n in ((66, 36), (66, 1024), (496, 36), (496, 1024)):
        phi = torch.randn((g, t), dtype=torch.float64, device=dev)
        index = torch.arange(n, device=dev) if n == s * k else torch.as_tensor([st * k + c for st in range(0, s, s // 9)[:9] for c in range(k)], device=dev)
        shift = torch.zeros(n, dtype=torch.float64, device=dev)
        step_of = index // k
        d = table.reshape(g, s * k)[:, index] - shift
        okay = (status.reshape(g, s) & 7) == 1
        used = torch.isfinite(d).all(dim=1) & okay[:, step_of].all(dim=1)
        f = phi * used[:, None]
        parts = {
            "gather - shift": lambda: table.reshape(g, s * k)[:, index] - shift,
            "status vote [G, S]": lambda: (status.reshape(g, s) & 7) == 1,
            "used": lambda: torch.isfinite(d).all(dim=1) & okay[:, step_of].all(dim=1),
            "mask D and Phi": lambda: (torch.where(used[:, None], d, torch.zeros_like(d)), phi * used[:, None]),
            "Phi.T @ Phi": lambda: f.t() @ f,
            "Phi.T @ D": lambda: f.t() @ d,
            "sum d d": lambda: (d * d).sum(dim=0),
        }
        got = {name: med(fn) for name, fn in parts.items()}
        lines.append(f"G = {g}, T = {t}, N = {n}: " + ", ".join(f"{name} {us:.1f} us" for name, us in got.items()) + f"; sum {sum(got.values()):.1f} us")
text = "\n".join(lines) + "\n"
print(text)
open(sys.argv[1], "w").write(text)
