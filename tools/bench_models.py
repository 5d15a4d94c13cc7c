"""Time one EM iteration (forward / backward / M-step) for any model:
python tools/bench_models.py [model ...] [B ...] [two_pass|fused|chunked ...] [f64] [f32s] [group] [lane] [wave] [quad] [grid] [gh<n>] [T=<n>]
`group` runs the group kernels (G lanes per trajectory) as well where a model has both forms; `lane` forces one lane per
trajectory for every sweep (the default runs the forward sweep of the d >= 7 models on the group kernels at small batches);
`wave` runs the matrix-instruction kernels where a model has them (group_lanes = 64: one wavefront per trajectory for the 12-state
quadrotor, four trajectories per wavefront -- forward sweep -- for the d <= 8 models). `gh<n>` (e.g. gh3) times every run under
GaussHermiteQuadrature(n) instead of the cubature rule; `grid` adds the grid family (one wavefront per trajectory, group_lanes = 64
under that rule; degree 3 unless gh<n> says otherwise), so `lane grid gh3 f64` prints the two forms of the rule side by side.
`T=<n>` overrides the horizon of the reference's experiment file."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd")]
pkg = importlib.import_module("input-inference-for-control_amd")
from i2c.known_models import make_env_model  # noqa: E402

CONFIGS = {  # hyper-parameters of the reference's experiment files
    "PendulumKnown": dict(T=200, Q=np.diag([1, 100.0, 1]), R=np.diag([2.0]), alpha=100.0, tol=0.0, sig_u=2.0, mu_u=1e-2),
    "CartpoleKnown": dict(T=500, Q=np.diag([1.0, 1.0, 100.0, 10.0, 1.0]), R=np.diag([1.0]), alpha=80.0, tol=0.0, sig_u=1.0, mu_u=1e-3),
    "DoubleCartpoleKnown": dict(T=300, Q=1e-3 * np.diag([1.0, 1.0, 100.0, 1.0, 100.0, 10.0, 1.0, 1.0]), R=1e-3 * np.diag([0.1]),
                                alpha=0.05, tol=0.99, sig_u=1.0, mu_u=1e-2),
    "PlanarQuadrotor": dict(T=50, Q=np.diag([1e3, 1e3, 1e3, 1, 1, 1]) / 1e3, R=np.diag([1e-3, 1e-3]), alpha=1.0, tol=1.0,
                            sig_u=1e-2, mu_u=0.0),
    "Quadrotor12": dict(T=50, Q=np.diag([10.0] * 3 + [1.0] * 3 + [0.1] * 6), R=1e-2 * np.eye(4), alpha=1.0, tol=0.5, sig_u=1e-2,
                        mu_u=1e-2),
}


def run(name, B, dtype, iters=10, mode="auto", group=0, storage=None, gh=0, T=None):
    cfg = CONFIGS[name]
    model = make_env_model(name)
    T, nu = T or cfg["T"], model.dim_u
    rng = np.random.default_rng(0)
    x0 = np.asarray(model.x0, float).reshape(1, -1) + 1e-3 * rng.normal(size=(B, model.dim_x))
    base = {"PlanarQuadrotor": 0.5, "Quadrotor12": 0.25}.get(name, 0.0) * getattr(model, "gravity", 0.0)
    mu_u = base + cfg["mu_u"] * rng.normal(size=(B, T, nu))
    try:
        eng = pkg.BatchedI2c(model, T, cfg["Q"], cfg["R"], cfg["Q"], cfg["alpha"], cfg["tol"], mu_u, cfg["sig_u"] * np.eye(nu), x0=x0,
                             dtype=dtype, keep_zpost=False, keep_xm=False, backward_mode=mode, group_lanes=group, allow_inexact=True,
                             **({"storage_dtype": storage} if storage is not None else {}),
                             **({"inference": "gauss_hermite", "gh_degree": gh} if gh else {}),
                             lib=pkg.load_library(os.environ["I2C_BENCH_LIB"]) if os.environ.get("I2C_BENCH_LIB") else None)
    except (RuntimeError, ValueError) as e:  # a combination the library refuses (e.g. fp32 arithmetic on the d = 16 model)
        print(f"{name:22s} B={B:6d} T={T:3d} {str(dtype)[6:]:8s} refused: {str(e)[:90]}")
        return
    for _ in range(3):
        eng.learn_msgs()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]
    torch.cuda.synchronize()
    for i in range(iters):
        ev[i][0].record(); eng.forward_sweep(); ev[i][1].record(); eng.backward_sweep(); ev[i][2].record(); eng.maximize(); ev[i][3].record()
    torch.cuda.synchronize()
    ms = [np.mean([ev[i][j].elapsed_time(ev[i][j + 1]) for i in range(iters)]) for j in range(3)]
    d = eng.dims
    w = 4 if (storage == torch.float32 or dtype != torch.float64) else 8
    el = (d.e_post - nu - nu * (nu + 1) // 2) + 2 * d.e_fwd + d.e_post
    tot = sum(ms)
    print(f"{name:22s} B={B:6d} T={T:3d} {f'gh{gh} ' if gh else ''}{('f64/f32s' if storage == torch.float32 else str(dtype)[6:]):8s} fwd {ms[0]:8.3f} bwd {ms[1]:8.3f} mstep {ms[2]:6.3f} ms | "
          f"[{eng.backward_schedule:8s} {eng.forward_family:5s}/{eng.backward_family:5s}] {B * T / tot * 1e3:10.3e} msg/s | {el * w * B * T / tot / 1e6:8.1f} GB/s | fails {len(eng.failures())}")


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if a in CONFIGS] or list(CONFIGS)
    Bs = [int(a) for a in sys.argv[1:] if a.isdigit()] or [4096]
    modes = [a for a in sys.argv[1:] if a in ("auto", "two_pass", "fused", "chunked")] or ["auto"]
    dts = (torch.float64,) if "f64" in sys.argv[1:] else (torch.float64, torch.float32)
    groups = (0, True) if "group" in sys.argv[1:] else (0,)
    if "wave" in sys.argv[1:]:
        groups = groups + (64,)
    if "quad" in sys.argv[1:]:  # the quad forward kernel of a model that also has wave kernels (the 12-state quadrotor)
        groups = groups + (164,)
    grid = "grid" in sys.argv[1:]
    gh = ([int(a[2:]) for a in sys.argv[1:] if a.startswith("gh") and a[2:].isdigit()] or [3 if grid else 0])[0]
    T = ([int(a[2:]) for a in sys.argv[1:] if a.startswith("T=")] or [None])[0]
    if "lane" in sys.argv[1:]:  # one lane per trajectory for every sweep (no group forward for the d >= 7 models)
        groups = (-1,) + groups[1:]
    for n in names:
        for B in Bs:
            for dt in dts:
                for m in modes:
                    for grp in groups:
                        if grp is True and (dt != torch.float64 or m != modes[0]):
                            continue
                        if grp == 164 and (n != "Quadrotor12" or dt != torch.float64 or m != modes[0]):
                            continue
                        if grp == 64 and (dt != torch.float64 or m != modes[0]):
                            continue  # (64: the wave kernels of the 12-state quadrotor, the quad forward kernel of the d <= 8 models)
                        if grp == 0 and n == "Quadrotor12" and 64 in groups and B <= 1024:
                            continue  # up to 1024 trajectories the default IS the wave family
                        if grp == -1 and n == "Quadrotor12":
                            grp = 0
                        run(n, B, dt, mode=m, group=grp, gh=gh, T=T)
                        if grid and dt == torch.float64 and m == modes[0] and grp in (0, -1):  # the same rule on the grid family
                            run(n, B, dt, mode=m, group=64, gh=gh, T=T)
                        if "f32s" in sys.argv[1:] and dt == torch.float64 and grp in (0, 64, 164):  # fp64 arithmetic on fp32-stored messages
                            run(n, B, dt, mode=m, group=grp, storage=torch.float32, T=T)
