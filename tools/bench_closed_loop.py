"""Per-control-step time of a CLOSED MPC loop at the shapes of BASELINE config 4 (H = 50, two EM iterations per step, cubature
Kalman state estimation; scripts/mpc_state_est/mpc_quad.py:559, 638-664), three ways on the same problem:
    bare     eng.mpc_step with a constant (y, u): the control step alone, what tools/bench_mpc12.py times -- the yardstick
    episode  eng.run_closed_loop: control step + plant step on the device, N steps in one library call (i2c_mpc_episode)
    host     the loop a user writes without it: eng.mpc_step per step, the action read back, the NumPy plant and measurement,
             (y, u) staged up again through a page-locked buffer
    python tools/bench_closed_loop.py [Quadrotor12|PlanarQuadrotor] [B ...]"""
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd")]
pkg = importlib.import_module("input-inference-for-control_amd")
from i2c.known_models import make_env_model  # noqa: E402


def engine(name, B, T, rng):
    m = make_env_model(name)
    nx, nu = m.dim_x, m.dim_u
    if name == "Quadrotor12":
        Q, R, ny = np.diag([10.0] * 3 + [1.0] * 3 + [0.1] * 6), 1e-2 * np.eye(4), 9
        args = (Q / 10.0, 0.02, 1.0)
    else:
        Q, R, ny = np.diag([10.0, 10.0, 1.0, 0.1, 0.1, 0.1]), 1e-2 * np.eye(2), 8
        args = (Q, 1.0, 1.0)
    hover = m.gravity / nu
    x0 = 1e-2 * rng.normal(size=(B, nx))
    mu_u = hover + 1e-2 * rng.normal(size=(B, T, nu))
    target = np.concatenate((np.asarray(m.zg, float).reshape(-1)[:nx], hover * np.ones(nu)))
    eng = pkg.BatchedI2c(m, T, Q, R, *args, mu_u, 1e-2 * np.eye(nu), x0=x0, keep_zpost=False, keep_xm=False,
                         z_traj=np.broadcast_to(target, (T, nx + nu)))
    eng.tau = T - 1
    eng.enable_per_cell_alpha()
    return m, eng, x0, 1e-4 * np.eye(ny), target


def run(name, B, T=50, n_iter=2, N=20, warm=3):
    rng = np.random.default_rng(7)
    sync = torch.cuda.synchronize

    # bare control step, constant (y, u)
    m, eng, x0, sig_zeta, target = engine(name, B, T, rng)
    y = torch.as_tensor(np.ascontiguousarray(m.measure(x0).T), dtype=torch.float64, device=eng.device)
    u = torch.full((eng.nu, B), float(m.gravity / eng.nu), dtype=torch.float64, device=eng.device)
    for _ in range(warm):
        eng.mpc_step(n_iter, y, u, sig_zeta)
    sync()
    t0 = time.perf_counter()
    for _ in range(N):
        eng.mpc_step(n_iter, y, u, sig_zeta)
    sync()
    bare = (time.perf_counter() - t0) / N * 1e3

    # the episode call
    m, eng, x0, sig_zeta, target = engine(name, B, T, np.random.default_rng(7))
    gen = torch.Generator(device=eng.device).manual_seed(1)
    r = eng.run_closed_loop(warm, n_iter, sig_zeta, x_true=x0, generator=gen, z_traj=target[None], keep=())
    sync()
    t0 = time.perf_counter()
    r = eng.run_closed_loop(N, n_iter, sig_zeta, x_true=r["x_true"], generator=gen, z_traj=target[None], keep=())
    sync()
    episode = (time.perf_counter() - t0) / N * 1e3
    fails_e, cost_e = len(eng.failures()), float(r["cost"].mean()) / N

    # today's loop: NumPy plants between the control steps
    m, eng, x0, sig_zeta, target = engine(name, B, T, np.random.default_rng(7))
    ny, nu = eng.dims.ny, eng.nu
    Le, Lz = np.linalg.cholesky(np.asarray(m.sig_eta, float)), np.linalg.cholesky(sig_zeta)
    stage = torch.empty(ny + nu, B, dtype=torch.float64).pin_memory()
    stage_dev = torch.empty(ny + nu, B, dtype=torch.float64, device=eng.device)
    act = torch.empty(nu, B, dtype=torch.float64).pin_memory()
    hrng = np.random.default_rng(1)
    x, cost = x0.copy(), np.zeros(B)

    def host_step(k):
        nonlocal x
        if k == 0:
            eng.mpc_step(n_iter)
        else:
            stage_dev.copy_(stage, non_blocking=True)
            eng.mpc_step(n_iter, stage_dev[:ny], stage_dev[ny:], sig_zeta)
        act.copy_(eng._mpc_action[:nu])  # blocks until the step has run
        uu = act.numpy().T
        xu = np.concatenate((x, uu), axis=1)
        err = m.observe(xu) - target
        cost[:] += np.einsum("bi,ij,bj->b", err, eng.QR, err)
        x = m.forward(xu)[0] + hrng.normal(size=x.shape) @ Le.T
        stage.numpy()[:ny] = (m.measure(x) + hrng.normal(size=(B, ny)) @ Lz.T).T
        stage.numpy()[ny:] = uu.T

    for k in range(warm):
        host_step(k)
    sync()
    t0 = time.perf_counter()
    for k in range(warm, warm + N):
        host_step(k)
    sync()
    host = (time.perf_counter() - t0) / N * 1e3
    print(f"{name} closed loop H={T} n_iter={n_iter} B={B:6d} [{eng.forward_family}/{eng.backward_family}, filter {eng.kernel_family('filter')}]: "
          f"bare {bare:7.3f} ms | episode {episode:7.3f} ms ({(episode / bare - 1) * 100:+5.1f} %) | host loop {host:8.3f} ms "
          f"({host / episode:5.1f}x) per control step; episode cost/step {cost_e:.3e}, fails {fails_e} / {len(eng.failures())}")


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.isdigit()]
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()]
    for name, default in (("Quadrotor12", [1024, 8192]), ("PlanarQuadrotor", [1024])):
        if not names or name in names:
            for B in sizes or default:
                run(name, B)
