"""Same-box check that two builds of the library give bit-identical results (pure addressing / scheduling changes):
python tools/ab_bitexact.py <other_lib.so> [model] [B] [group_lanes]   (group_lanes: a kernel-family request, e.g. 64 = the wave / quad kernels,
16 = the group kernels of the 12-state quadrotor; default 0 = what the model runs by default)"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd"), os.path.join(ROOT, "tools")]
pkg = importlib.import_module("input-inference-for-control_amd")
from bench_models import CONFIGS  # noqa: E402
from i2c.known_models import make_env_model  # noqa: E402

other = sys.argv[1]
name = sys.argv[2] if len(sys.argv) > 2 else "PendulumKnown"
B = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
lanes = int(sys.argv[4]) if len(sys.argv) > 4 else 0
cfg = CONFIGS[name]
model = make_env_model(name)
T, nu = cfg["T"], model.dim_u
rng = np.random.default_rng(0)
x0 = np.asarray(model.x0, float).reshape(1, -1) + 1e-3 * rng.normal(size=(B, model.dim_x))
mu_u = cfg["mu_u"] * rng.normal(size=(B, T, nu))
res = []
for lib in (None, pkg.load_library(other)):
    for mode in ("chunked", "two_pass", "fused"):
        eng = pkg.BatchedI2c(model, T, cfg["Q"], cfg["R"], cfg["Q"], cfg["alpha"], cfg["tol"], mu_u, cfg["sig_u"] * np.eye(nu), x0=x0,
                             backward_mode=mode, lib=lib, group_lanes=lanes)
        for _ in range(4):
            eng.learn_msgs()
        torch.cuda.synchronize()
        res.append((mode, eng.post.clone(), eng.alpha.clone(), eng.zpost.clone() if eng.zpost is not None else None, eng.backward_schedule))
n = len(res) // 2
for (m, p, a, z, sch), (m2, p2, a2, z2, _) in zip(res[:n], res[n:]):
    print(f"{name} B={B} lanes={lanes} {m:8s} [{sch}]: post {'bit-identical' if torch.equal(p, p2) else 'DIFFERENT %.3e' % float((p - p2).abs().max())}, "
          f"alpha {'bit-identical' if torch.equal(a, a2) else 'DIFFERENT'}, zpost {'bit-identical' if z is None or torch.equal(z, z2) else 'DIFFERENT'}")
