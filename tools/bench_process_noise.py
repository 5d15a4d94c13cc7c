"""What the optional process_noise member of a functor costs, sweep by sweep (sibling of tools/bench_traced_models.py):
python tools/bench_process_noise.py [repeats=<n>] [out=<file>]

  lane forward sweep:  the pendulum with input noise (tests/plugins/pendulum_input_noise.hpp) against the in-tree Pendulum, T = 200, B = 4096
  quad forward sweep:  the cartpole with input noise (tests/plugins/cartpole_input_noise.hpp) against the in-tree Cartpole, T = 100, B = 1024
  and three more: the d = 5 lane sweep (cartpole, T = 100, B = 4096), and the first two with general cubature weights (1.2, 0.44, 0.5)
at the reference's experiment settings. Every variant is timed `repeats` times (default 5), the variants ALTERNATING inside a repeat; a
repeat is the mean of 20 forward sweeps between device events after 3 warm-up iterations. Prints the repeats, their median and max - min,
and the ratio of medians with / without the term. (The in-tree model's sweep under i2c_learn may take the helper wave; a stand-alone
forward sweep, timed here, is plain k_forward / k_quad_forward for both.)"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd"), os.path.join(ROOT, "tests")]
pkg = importlib.import_module("input-inference-for-control_amd")
from bench_models import CONFIGS  # noqa: E402
from i2c.known_models import make_env_model  # noqa: E402
from noise_models import CartpoleInputNoiseKnown, PendulumInputNoiseKnown  # noqa: E402


def engine(model, name, B, T, **kw):
    cfg = CONFIGS[name]
    rng = np.random.default_rng(0)
    x0 = np.asarray(model.x0, float).reshape(1, -1) + 1e-3 * rng.normal(size=(B, model.dim_x))
    mu_u = cfg["mu_u"] * rng.normal(size=(B, T, 1))
    eng = pkg.BatchedI2c(model, T, cfg["Q"], cfg["R"], cfg["Q"], cfg["alpha"], cfg["tol"], mu_u, cfg["sig_u"] * np.eye(1), x0=x0,
                         keep_zpost=False, keep_xm=False, **kw)
    for _ in range(3):
        eng.learn_msgs()
    return eng


def time_forward(eng, iters=20):
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(iters)]
    torch.cuda.synchronize()
    for e in ev:
        e[0].record(); eng.forward_sweep(); e[1].record(); eng.backward_sweep(); eng.maximize()
    torch.cuda.synchronize()
    return float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))


def main(argv):
    opt = {a.split("=")[0]: a.split("=")[1] for a in argv if "=" in a}
    repeats = int(opt.get("repeats", 5))
    lines = [f"forward sweep with / without the process_noise member, fp64, ms per sweep; {repeats} repeats of 20 sweeps, variants alternating"]
    general = dict(quad=(1.2, 0.44, 0.5))  # weights that do not sum to one: the general cell / the GENERAL quad variant
    legs = [("lane", "PendulumKnown", PendulumInputNoiseKnown, 4096, 200, dict(group_lanes=-1)),
            ("quad", "CartpoleKnown", CartpoleInputNoiseKnown, 1024, 100, dict(group_lanes=pkg._native.LANES_QUAD)),
            ("lane", "CartpoleKnown", CartpoleInputNoiseKnown, 4096, 100, dict(group_lanes=-1)),
            ("lane", "PendulumKnown", PendulumInputNoiseKnown, 4096, 200, dict(group_lanes=-1, **general)),
            ("quad", "CartpoleKnown", CartpoleInputNoiseKnown, 1024, 100, dict(group_lanes=pkg._native.LANES_QUAD, **general))]
    for fam, name, noisy, B, T, kw in legs:
        engs = [("in-tree " + name, engine(make_env_model(name), name, B, T, **kw)), ("with process_noise", engine(noisy(), name, B, T, **kw))]
        assert all(e.forward_family == fam for _, e in engs)
        times = {n: [] for n, _ in engs}
        for _ in range(repeats):
            for n, e in engs:
                times[n].append(time_forward(e))
        assert all(e.failures() == [] for _, e in engs)
        base = float(np.median(times[engs[0][0]]))
        for n, _ in engs:
            t = times[n]
            lines.append(f"{fam} forward{', general weights' if 'quad' in kw else ''}, T = {T}, B = {B}: {n:24s} " + " ".join(f"{x:7.4f}" for x in t)
                         + f" | median {np.median(t):7.4f}  max - min {max(t) - min(t):6.4f}  ratio {np.median(t) / base:5.3f}")
        del engs
    text = "\n".join(lines)
    print(text)
    if "out" in opt:
        os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
        with open(opt["out"], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
