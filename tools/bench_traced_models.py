"""A model written in Python against the hand-written functor of the same math, sweep by sweep (sibling of tools/bench_models.py):
python tools/bench_traced_models.py [B] [T=<n>] [repeats=<n>] [out=<file>]

PyCartpole (tests/plugins/py_models.py, traced and generated) against the in-tree Cartpole at the reference's experiment settings:
forward and backward sweep on the lane kernels and on the quad kernels (group_lanes = -1 / 64), and the Linearize() forward sweep
with the emitted Jacobian, with jacobian=False (dual numbers) and on the hand-written functor. Every variant is timed `repeats` times
(default 5), the variants ALTERNATING inside a repeat; a repeat is the mean of 10 sweeps between device events after 3 warm-up
iterations. Prints, per variant, the repeats, their median and max - min, and the ratio of medians traced / hand-written."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd"), os.path.join(ROOT, "tests", "plugins")]
pkg = importlib.import_module("input-inference-for-control_amd")
import py_models  # noqa: E402
from bench_models import CONFIGS  # noqa: E402
from i2c.known_models import make_env_model  # noqa: E402


def engine(model, B, T, **kw):
    cfg = CONFIGS["CartpoleKnown"]
    rng = np.random.default_rng(0)
    x0 = np.asarray(model.x0, float).reshape(1, -1) + 1e-3 * rng.normal(size=(B, model.dim_x))
    mu_u = cfg["mu_u"] * rng.normal(size=(B, T, 1))
    eng = pkg.BatchedI2c(model, T, cfg["Q"], cfg["R"], cfg["Q"], cfg["alpha"], cfg["tol"], mu_u, cfg["sig_u"] * np.eye(1), x0=x0,
                         keep_zpost=False, keep_xm=False, **kw)
    for _ in range(3):
        eng.learn_msgs()
    return eng


def time_sweeps(eng, iters=10):
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    torch.cuda.synchronize()
    for e in ev:
        e[0].record(); eng.forward_sweep(); e[1].record(); eng.backward_sweep(); e[2].record(); eng.maximize()
    torch.cuda.synchronize()
    return [float(np.mean([e[j].elapsed_time(e[j + 1]) for e in ev])) for j in range(2)]


def main(argv):
    B = ([int(a) for a in argv if a.isdigit()] or [4096])[0]
    opt = {a.split("=")[0]: a.split("=")[1] for a in argv if "=" in a}
    T, repeats = int(opt.get("T", 500)), int(opt.get("repeats", 5))
    hand = make_env_model("CartpoleKnown")
    lines = [f"PyCartpole (generated functor) against Cartpole (hand-written), B = {B}, T = {T}, fp64, ms per sweep; {repeats} repeats of 10 sweeps"]
    legs = [("cubature lane", dict(group_lanes=-1), [("hand-written", hand), ("traced", py_models.PyCartpole())]),
            ("cubature quad", dict(group_lanes=64), [("hand-written", hand), ("traced", py_models.PyCartpole())]),
            ("linearize lane", dict(group_lanes=-1, inference="linearize"),
             [("hand-written", hand), ("traced, emitted Jacobian", py_models.PyCartpole()), ("traced, dual numbers", py_models.PyCartpole(jacobian=False))])]
    for leg, kw, variants in legs:
        engs = [(name, engine(m, B, T, **kw)) for name, m in variants]
        times = {name: [] for name, _ in engs}
        for _ in range(repeats):
            for name, e in engs:
                times[name].append(time_sweeps(e))
        fam = f"{engs[0][1].forward_family}/{engs[0][1].backward_family} {engs[0][1].backward_schedule}"
        assert all(e.failures() == [] and e.forward_family == engs[0][1].forward_family for _, e in engs)
        for j, sweep in enumerate(("forward", "backward")):
            if sweep == "backward" and "linearize" in leg:
                continue  # (the issue's question is the forward sweep: two transforms per cell against the backward cell's one)
            base = float(np.median([t[j] for t in times["hand-written"]]))
            for name, _ in engs:
                t = [x[j] for x in times[name]]
                lines.append(f"{leg:15s} {sweep:8s} [{fam:22s}] {name:26s} " + " ".join(f"{x:7.3f}" for x in t)
                             + f" | median {np.median(t):7.3f}  max - min {max(t) - min(t):6.3f}  ratio to hand-written {np.median(t) / base:5.3f}")
        del engs
    text = "\n".join(lines)
    print(text)
    if "out" in opt:
        os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
        with open(opt["out"], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
