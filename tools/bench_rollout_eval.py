"""Monte-Carlo policy evaluation, two ways to the same numbers, timed against each other on the GPU:
  (a) BatchedI2c.evaluate(R, seed): noise drawn in the kernel, costs and moments reduced on the device (i2c_rollout_eval);
  (b) what there was before it: torch.randn of the noise, BatchedI2c.rollout, the reductions in torch on the device.
The two sides alternate, each is repeated, and the table states median and spread (min .. max) of each, the peak allocation torch
measured next to the bytes computed from the shapes, and a sweep of `parts` at one shape.
    python tools/bench_rollout_eval.py [--reps 7] [--quick] [--out profiles/rollout_eval_times.txt]
    python tools/bench_rollout_eval.py --bytes      # the allocation table alone, from shapes (no GPU needed)"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd")]

# (model, T, B, R, moments)
SHAPES = [("PendulumKnown", 200, 4096, 64, True), ("PendulumKnown", 200, 64, 4096, True), ("PendulumKnown", 200, 1, 65536, True),
          ("DoubleCartpoleKnown", 300, 4096, 16, True), ("DoubleCartpoleKnown", 300, 4096, 16, False)]
SWEEPS = [("PendulumKnown", 200, 64, 4096, (1, 4, 16, 64, 256, None)), ("PendulumKnown", 200, 1, 65536, (1024, 8192, None))]
DIMS = {"PendulumKnown": (2, 1, 4, 3), "DoubleCartpoleKnown": (6, 1, 9, 8)}  # nx, nu, nz, nzt


def sym(n):
    return n * (n + 1) // 2


def parts_rule(B, R):
    return min(R, max(1, -(-65536 // B)))


def bytes_evaluate(model, T, B, R, moments, parts=None):
    """fp64 bytes evaluate() allocates: the costs, their statistics and count, and with moments the workspace and the two outputs"""
    nx, nu, _, _ = DIMS[model]
    d = nx + nu
    P = parts or parts_rule(B, R)
    n = R * B * 8 + 4 * B * 8 + B * 4
    if moments:
        n += P * T * (d + sym(d)) * B * 8 + T * (d + sym(d)) * B * 8
    return n


def bytes_rollout_way(model, T, B, R, moments):
    """fp64 bytes of the noise rollout() is handed and of the trajectories it writes (the reductions' temporaries come on top)"""
    nx, nu, nz, nzt = DIMS[model]
    N = R * B
    return T * nx * N * 8, ((T * (nx + nu) * N if moments else 0) + T * nz * N + nzt * N) * 8


def make_engine(pkg, model, T, B, device):
    from i2c.known_models import make_env_model
    rng = np.random.default_rng(0)
    m = make_env_model(model)
    if model == "PendulumKnown":
        Q, R = np.diag([1.0, 100.0, 1.0]), np.diag([2.0])
        x0 = np.array([np.pi, 0.0]) + 1e-2 * rng.normal(size=(B, 2))
        eng = pkg.BatchedI2c(m, T, Q, R, Q, 100.0, 0.0, 1e-2 * rng.normal(size=(B, T, 1)), 2.0 * np.eye(1), x0=x0, device=device,
                             keep_zpost=False, keep_xm=False)
    else:
        Q, R = 1e-3 * np.diag([1.0, 1.0, 100.0, 1.0, 100.0, 10.0, 1.0, 1.0]), 1e-3 * np.diag([0.1])
        x0 = np.asarray(m.x0, float).reshape(1, -1) + 1e-3 * rng.normal(size=(B, m.dim_x))
        eng = pkg.BatchedI2c(m, T, Q, R, Q, 0.05, 0.99, 1e-2 * rng.normal(size=(B, T, 1)), np.eye(1), x0=x0, device=device,
                             keep_zpost=False, keep_xm=False)
    eng.learn(3)
    return eng


def way_a(eng, R, moments, parts=None, seed=0):
    return eng.evaluate(R, seed=seed, moments=moments, parts=parts)


def way_b(eng, R, moments):
    """the same numbers from rollout(): noise by torch.randn, reductions in torch"""
    N, T, dt, dev = R * eng.B, eng.H, eng.dtype, eng.device
    eps = torch.randn(T, eng.nx, N, dtype=dt, device=dev)
    res = eng.rollout(R, eps_x=eps, want=("xu", "z", "z_term") if moments else ("z", "z_term"))
    QR = torch.as_tensor(eng.QR, dtype=dt, device=dev)
    e = res["z"] - torch.as_tensor(eng.zg, dtype=dt, device=dev)
    cost = torch.einsum("rbti,ij,rbtj->rb", e, QR, e)
    if eng.has_Qf:
        et = res["z_term"] - torch.as_tensor(eng.zg_term, dtype=dt, device=dev)
        cost = cost + torch.einsum("rbi,ij,rbj->rb", et, torch.as_tensor(eng.Qf, dtype=dt, device=dev), et)
    out = {"cost": cost, "cost_mean": cost.mean(0), "cost_var": cost.var(0, unbiased=True), "cost_min": cost.min(0).values,
           "cost_max": cost.max(0).values, "cost_percentiles": eng._cost_quantiles(cost, torch.tensor([0.1, 0.9], dtype=dt, device=dev))}
    if moments:
        xu = res["xu"]
        mean = xu.mean(0)
        c = xu - mean
        out["xu_mean"], out["xu_cov"] = mean, torch.einsum("rbti,rbtj->btij", c, c) / (R - 1)
    return out


def timed(fn, sync):
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    ms = (time.perf_counter() - t0) * 1e3
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return ms, peak


def spread(v):
    return f"{statistics.median(v):9.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the command, not a measurement")
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    shapes = [(m, 20, min(B, 64), min(R, 8), mo) for m, _, B, R, mo in SHAPES] if a.quick else SHAPES
    sweeps = [("PendulumKnown", 20, 8, 64, (1, 4, None))] if a.quick else SWEEPS
    say("bytes from shapes (fp64): evaluate() allocates | rollout way: noise in + trajectories out")
    for m, T, B, R, mo in shapes:
        nin, nout = bytes_rollout_way(m, T, B, R, mo)
        say(f"  {m} T={T} B={B} R={R} moments={mo}: {bytes_evaluate(m, T, B, R, mo) / 1e6:10.2f} MB | {nin / 1e6:10.2f} + {nout / 1e6:10.2f} MB")
    if a.bytes:
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_eval.py times the GPU and found none (use --bytes for the allocation table)")
    pkg = importlib.import_module("input-inference-for-control_amd")
    sync = torch.cuda.synchronize
    say(f"\n(a) evaluate(R, seed) against (b) torch.randn + rollout + torch reductions; {a.reps} alternating repetitions, median (min .. max)")
    engines = {}
    for m, T, B, R, mo in shapes:
        eng = engines.get((m, T, B)) or engines.setdefault((m, T, B), make_engine(pkg, m, T, B, "cuda:0"))
        fa, fb = (lambda: way_a(eng, R, mo)), (lambda: way_b(eng, R, mo))
        for _ in range(2):
            timed(fa, sync), timed(fb, sync)
        ta, tb, pa, pb = [], [], 0, 0
        for i in range(a.reps):
            ms, pk = timed(fa, sync)
            ta.append(ms)
            pa = max(pa, pk)
            ms, pk = timed(fb, sync)
            tb.append(ms)
            pb = max(pb, pk)
        say(f"  {m} T={T} B={B} R={R} moments={mo} parts={way_a(eng, R, mo)['parts']}")
        say(f"    (a) {spread(ta)}  peak {pa / 1e6:10.2f} MB (from shapes {bytes_evaluate(m, T, B, R, mo) / 1e6:.2f}; the workspace is kept between calls)")
        say(f"    (b) {spread(tb)}  peak {pb / 1e6:10.2f} MB (noise + trajectories from shapes {sum(bytes_rollout_way(m, T, B, R, mo)) / 1e6:.2f})")
        say(f"    (a) / (b) = {statistics.median(ta) / statistics.median(tb):.3f}")
    for m, T, B, R, parts in sweeps:
        eng = engines.get((m, T, B)) or make_engine(pkg, m, T, B, "cuda:0")
        say(f"\nparts sweep, {m} T={T} B={B} R={R} (None = the rule, {parts_rule(B, R)})")
        times = {p: [] for p in parts}
        for p in parts:
            timed(lambda: way_a(eng, R, True, p), sync)
        for i in range(a.reps):
            for p in parts:
                times[p].append(timed(lambda: way_a(eng, R, True, p), sync)[0])
        for p in parts:
            say(f"    parts={p}: {spread(times[p])}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
