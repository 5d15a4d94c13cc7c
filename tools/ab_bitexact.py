"""Same-box check that two builds of the library give bit-identical results (pure addressing / scheduling / dispatch changes):
python tools/ab_bitexact.py <other_lib.so> [model] [B] [group_lanes] [T] [inference] [storage]
group_lanes: a kernel-family request, e.g. 64 = the wave / quad kernels, 16 = the group kernels of the 12-state quadrotor; default 0 =
what the model runs by default ("G": the model's group width). T: default the horizon of the model's config. inference: cubature
(default) | linearize | gauss_hermite (degree 3, degree 2 for d > 5). storage: fp64 (default) | fp32 (fp64 arithmetic on fp32-stored messages) | f32a (fp32 ARITHMETIC and storage). B, group_lanes, T,
inference and storage each take a comma-separated list: every combination runs in this one process. A request the engine refuses
prints one "refused" line. Exit status 1 if any line differs; the last line counts lines, refusals and differences.
I2C_AB_LIB=<lib.so>: the library compared against (default: the in-tree build); I2C_AB_NO_WORK=1: run without the chunk workspace;
I2C_AB_PER_TRAJ=1: pass per-trajectory model parameters (models that have parameters); I2C_AB_LEARN=1: the four EM iterations by ONE
i2c_learn call (eng.learn(4): the M-step on the reduction kernels, deferred into the next forward sweep, the helper wave) instead of
four learn_msgs(), which never enter it."""
import importlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd"), os.path.join(ROOT, "tools")]
pkg = importlib.import_module("input-inference-for-control_amd")
from bench_models import CONFIGS  # noqa: E402
from i2c.known_models import make_env_model  # noqa: E402


def arg(i, default):
    return sys.argv[i].split(",") if len(sys.argv) > i else [default]


# the three in-tree models tools/bench_models.py has no experiment for, with the parameters the parity tests run them with
# (tests/test_hip_full_configs.py; tests/golden em_linear_T60, lin_covctrl_T50); term = (mu_x_terminal, sig_x_terminal); noise: the
# shipped LinearKnown has degenerate noise (1e-20), the golden run replaces it
CONFIGS = dict(CONFIGS)
CONFIGS["PendulumKnownActReg"] = dict(T=60, Q=None, Qf=None, R=np.diag([1.0]), alpha=300.0, tol=1.0, sig_u=0.5, mu_u=1e-2,
                                      term=(np.array([0.0, 0.0]), np.diag([1e-3, 1e-3])))
CONFIGS["LinearKnown"] = dict(T=60, Q=np.diag([10.0, 10.0]), R=np.diag([1.0]), alpha=800.0, tol=0.0, sig_u=1.0, mu_u=1e-2, noise=1e-4)
CONFIGS["LinearKnownMinimumEnergy"] = dict(T=50, Q=None, Qf=None, R=np.diag([1.0]), alpha=1e9, tol=1.0, sig_u=100.0, mu_u=1e-2,
                                           term=(np.array([-5.0, -5.0]), 2.0 * np.eye(2)))

name = arg(2, "PendulumKnown")[0]
cfg, model = CONFIGS[name], make_env_model(name)
if "noise" in cfg:
    model.sig_x0 = model.sig_eta = cfg["noise"] * np.eye(model.dim_x)
base = os.environ.get("I2C_AB_LIB")
libs = (pkg.load_library(base) if base else pkg.load_library(), pkg.load_library(sys.argv[1]))
group = libs[0].query(pkg._native.MODEL_IDS[name]).group_lanes or 4  # (4: a width a model without group kernels must refuse)
nu = model.dim_u
gh_degree = 3 if model.dim_x + nu <= 5 else 2  # (a grid of at most 256 points per cell)


def run(lib, mode, B, lanes, T, inference, storage, x0, mu_u):
    extra = {"storage_dtype": torch.float32} if storage == "fp32" else {"dtype": torch.float32, "allow_inexact": True} if storage == "f32a" else {}
    if os.environ.get("I2C_AB_PER_TRAJ"):  # the per-trajectory-parameter tables, every trajectory with the model's own parameters
        extra["model_params"] = np.tile(np.asarray(model.device_params(), float), (B, 1))
    eng = pkg.BatchedI2c(model, T, cfg["Q"], cfg["R"], cfg.get("Qf", cfg["Q"]), cfg["alpha"], cfg["tol"], mu_u, cfg["sig_u"] * np.eye(nu),
                         *cfg.get("term", ()), x0=x0,
                         backward_mode=mode, lib=lib, group_lanes=lanes, inference=inference, gh_degree=gh_degree if inference == "gauss_hermite" else None, **extra)
    if os.environ.get("I2C_AB_NO_WORK"):  # a chunked answer falls back to two-pass (which needs cell_stats) or fused
        # (relies on engine.py internals: BatchedI2c.work / ._problem.work hold the chunk workspace, .cell_stats is the [T][2][B]
        #  arithmetic-typed buffer of the two-pass schedule handed to i2c_learn -- keep in step with BatchedI2c.__init__)
        eng.work = eng._problem.work = None
        if eng.cell_stats is None:
            eng.cell_stats = torch.zeros(T, 2, B, dtype=eng.dtype, device=eng.device)
    if os.environ.get("I2C_AB_LEARN"):
        eng.learn(4)
    else:
        for _ in range(4):
            eng.learn_msgs()
    if eng.post.is_cuda:
        torch.cuda.synchronize()
    return eng.post.clone(), eng.alpha.clone(), eng.zpost.clone() if eng.zpost is not None else None, eng.backward_schedule


lines = refused = bad = 0
for B, lanes, T, inference, storage in itertools.product(arg(3, "4096"), arg(4, "0"), arg(5, str(cfg["T"])), arg(6, "cubature"), arg(7, "fp64")):
    B, T, lanes = int(B), int(T), group if lanes == "G" else int(lanes)
    tag = f"{name} B={B} T={T} lanes={lanes} {inference} {storage}"
    rng = np.random.default_rng(0)
    x0 = np.asarray(model.x0, float).reshape(1, -1) + 1e-3 * rng.normal(size=(B, model.dim_x))
    mu_u = cfg["mu_u"] * rng.normal(size=(B, T, nu))
    for mode in ("chunked", "two_pass", "fused"):
        out = []
        for lib in libs:
            try:
                out.append(run(lib, mode, B, lanes, T, inference, storage, x0, mu_u))
            except (ValueError, NotImplementedError, RuntimeError) as e:
                if "illegal memory access" in str(e) or "HIP error" in str(e):
                    raise
                out.append(f"{type(e).__name__}: {e}")
        if isinstance(out[0], str) or isinstance(out[1], str):  # refused: by both alike, or a difference
            alike = out[0] == out[1]
            refused += alike
            bad += not alike
            print(f"{tag} {mode:8s}: " + (f"refused by both ({out[0][:70]})" if alike else f"DIFFERENT outcome: {out[0]!s:.80} | {out[1]!s:.80}"))
            continue
        (p, a, z, sch), (p2, a2, z2, _) = out
        same = (torch.equal(p, p2), torch.equal(a, a2), z is None or torch.equal(z, z2))
        lines += 1
        bad += not all(same)
        print(f"{tag} {mode:8s} [{sch}]: post {'bit-identical' if same[0] else 'DIFFERENT %.3e' % float((p - p2).abs().max())}, "
              f"alpha {'bit-identical' if same[1] else 'DIFFERENT'}, zpost {'bit-identical' if same[2] else 'DIFFERENT'}", flush=True)
print(f"{name}: {lines} lines compared, {refused} refused by the engine, {bad} DIFFERENT")
sys.exit(1 if bad else 0)
