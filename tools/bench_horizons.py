"""What per-trajectory horizons (BatchedI2c(horizons=...), I2cProblem.horizons) cost and save on the headline workload.

    python tools/bench_horizons.py [--steps K] [--warmup W] [--batch B] [--horizon T]

Pendulum, T = 200 allocated cells, B = 4096, one EM iteration (forward sweep, backward sweep, M-step: the K iterations of one
i2c_learn call, as bench.py times them), three legs on the same inputs:
  mixed     horizons drawn uniformly from 20 .. T (default_rng(0)): the one-lane kernels with the fused backward walk
  sorted    the same horizons in ascending order over the batch: the lanes of a wavefront then end together
  full      every horizon equal to T: the same kernels doing all the work -- what the feature's only schedule costs
  default   no horizons at all: the default schedule of this batch size (the chunked backward sweep, helper wave)
and, for the fused walk alone, `fused`: no horizons, group_lanes = -1, backward_mode = "fused" (what `full` is to be compared with).
Prints one JSON line: per leg the median and the spread (min, max) of the per-iteration milliseconds over `--repeats` timed calls.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "input-inference-for-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

pkg = importlib.import_module("input-inference-for-control_amd")
from i2c.known_models import make_env_model  # noqa: E402


def make_engine(B, T, horizons=None, **kw):
    rng = np.random.default_rng(1234)
    x0 = np.array([np.pi, 0.0]) + 1e-2 * rng.normal(size=(B, 2))
    mu_u = 1e-2 * rng.normal(size=(B, T, 1))
    Q, R = np.diag([1.0, 100.0, 1.0]), np.diag([2.0])
    return pkg.BatchedI2c(make_env_model("PendulumKnown"), T, Q, R, Q, 100.0, 0.0, mu_u, 2.0 * np.eye(1), x0=x0, device="cuda",
                          keep_zpost=False, keep_xm=False, horizons=horizons, **kw)


def time_leg(eng, steps, warmup, repeats):
    for _ in range(warmup):
        eng.learn_msgs()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.learn(steps)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    assert eng.failures() == [], "failed trajectories"
    return {"ms_per_iteration": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)),
            "forward": eng.forward_family, "backward": f"{eng.backward_family}/{eng.backward_schedule}"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=200)
    a = ap.parse_args()
    B, T = a.batch, a.horizon
    mixed = np.random.default_rng(0).integers(min(20, T), T + 1, size=B)
    # (a wavefront runs as long as its longest lane: the same horizons sorted, so that the 64 lanes of a wave end together)
    legs = [("mixed_20_to_T", dict(horizons=mixed)), ("mixed_20_to_T_sorted", dict(horizons=np.sort(mixed))),
            ("full_T", dict(horizons=np.full(B, T))), ("default_no_horizons", {}),
            ("fused_no_horizons", dict(group_lanes=-1, backward_mode="fused"))]
    out = {"workload": f"pendulum T={T} B={B}, one EM iteration", "cells_mixed": int(mixed.sum()), "cells_full": B * T}
    for name, kw in legs:
        out[name] = time_leg(make_engine(B, T, **kw), a.steps, a.warmup, a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
