"""Closed-loop MPC episodes on the device (ABI v9): the plant step (i2c_plant_step, BatchedI2c.plant_step) and the episode call
(i2c_mpc_episode, BatchedI2c.run_closed_loop) that chains N control steps with the noisy plants in between -- the loop of the
reference's scripts/mpc_state_est/mpc_quad.py:638-664 for B systems at once, with no host round trip.

  1. the plant step against the models' own NumPy forward / observe / measure;
  2. the episode against a loop of its pieces (mpc_step + plant_step on a second engine), bit for bit;
  3. the episode against today's host-driven loop (mpc_step + NumPy plant);
  4. batch independence and failure isolation;
  5. plant parameters that differ from the planner's;
  6. the ABI.
Each check runs on the host simulation of the kernels and, with `-m gpu`, on the MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import assert_close
from test_model_params_batch import linear_model, param_rows, problem, with_params
from test_model_plugin import VanDerPolKnown

pkg = parity.pkg
from i2c.known_models import make_env_model  # noqa: E402

_native = pkg._native
IN_TREE = ["PendulumKnown", "PendulumKnownActReg", "CartpoleKnown", "DoubleCartpoleKnown", "LinearKnown", "LinearKnownMinimumEnergy",
           "PlanarQuadrotor", "Quadrotor12"]


def _model(name):
    if name == "VanDerPol":
        return make_env_model(VanDerPolKnown())
    return linear_model() if name == "LinearKnown" else make_env_model(name)


def _spd(rng, n, scale):
    a = rng.normal(size=(n, n))
    return scale * (a @ a.T / n + np.eye(n))


def _dev(a, eng):
    """(B, n) array -> [n][B] device tensor."""
    return torch.as_tensor(np.array(np.asarray(a, np.float64).T, order="C"), dtype=eng.dtype, device=eng.device)


def _generic_engine(model, B, lib, device, rng, T=3):
    """Any model with a full (non-diagonal) cost weight: only the plant step is exercised."""
    nx, nu, nz, nzt = model.dim_x, model.dim_u, model.dim_z, (model.dim_z_term or 0)
    Q = _spd(rng, nz - nu, 1.0) if nz > nu else None
    Rm = _spd(rng, nu, 0.5)
    Qf = np.eye(nzt) if nzt else None
    x0 = np.asarray(model.x0, float).reshape(1, nx) + 0.3 * rng.normal(size=(B, nx))
    return pkg.BatchedI2c(model, T, Q, Rm, Qf, 1.0, 0.0, np.zeros((B, T, nu)), np.eye(nu), x0=x0, device=device, lib=lib)


def _numpy_plant(model, x, u, sig_eta, sig_zeta, eps_x, eps_y, QR, z_ref):
    """(x', y, stage cost) of one plant step per row, from the model's own NumPy functions (known_models.py)."""
    xu = np.concatenate((x, u), axis=1)
    z = np.asarray(model.observe(xu)).reshape(x.shape[0], -1)
    xn = np.asarray(model.forward(xu)[0]).reshape(x.shape)
    if eps_x is not None:
        xn = xn + eps_x @ np.linalg.cholesky(sig_eta).T
    y = np.asarray(model.measure(xn)).reshape(x.shape[0], -1)
    if eps_y is not None:
        y = y + eps_y @ np.linalg.cholesky(sig_zeta).T
    err = z - z_ref
    return xn, y, np.einsum("bi,ij,bj->b", err, QR, err)


# ---- 1. plant step against the NumPy models ---------------------------------------------------------------------------------
def _check_plant_step(name, lib, device, noise, B=5):
    rng = np.random.default_rng(11)
    model = _model(name)
    eng = _generic_engine(model, B, lib, device, rng)
    nx, nu, ny = eng.nx, eng.nu, eng.dims.ny
    x = np.asarray(model.x0, float).reshape(1, nx) + 0.3 * rng.normal(size=(B, nx))
    u = 0.5 * rng.normal(size=(B, nu))
    if name in ("PlanarQuadrotor", "Quadrotor12"):
        u += model.gravity / nu  # around hover thrust, some rows beyond the clip
    sig_zeta = _spd(rng, ny, 1e-3)
    sig_eta = np.asarray(model.sig_eta, float)
    ex, ey = (rng.normal(size=(B, nx)), rng.normal(size=(B, ny))) if noise else (None, None)
    z_ref = rng.normal(size=(B, eng.nz))
    xd, cost = _dev(x, eng), torch.full((B,), 0.25, dtype=eng.dtype, device=eng.device)
    y = eng.plant_step(xd, _dev(u, eng), sig_zeta, None if ex is None else _dev(ex, eng), None if ey is None else _dev(ey, eng),
                       z_ref=_dev(z_ref, eng), cost=cost)
    xn, yn, cn = _numpy_plant(model, x, u, sig_eta, sig_zeta, ex, ey, eng.QR, z_ref)
    what = f"{name} plant step ({'noisy' if noise else 'noise-free'})"
    assert_close(parity.np_(xd).T, xn, 1e-10, what + " x'")
    assert_close(parity.np_(y).T, yn, 1e-10, what + " y")
    assert_close(parity.np_(cost), 0.25 + cn, 1e-10, what + " cost (accumulated)")
    # the default cost reference is sys.zg; the fully observed mode hands the state to the belief mean and measures nothing
    xd2, cost2 = _dev(x, eng), torch.zeros(B, dtype=eng.dtype, device=eng.device)
    assert eng.plant_step(xd2, _dev(u, eng), eps_x=None if ex is None else _dev(ex, eng), observe_state=True, cost=cost2) is None
    assert torch.equal(xd2, xd) and torch.equal(eng.x0, xd)
    _, _, cg = _numpy_plant(model, x, u, sig_eta, sig_zeta, ex, None, eng.QR, np.asarray(model.zg, float).reshape(1, -1))
    assert_close(parity.np_(cost2), cg, 1e-10, what + " cost against zg")


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("name", IN_TREE + ["VanDerPol"])
def test_plant_step_matches_numpy_model_cpu(name, noise):
    _check_plant_step(name, hostsim.load(), "cpu", noise)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("name", IN_TREE + ["VanDerPol"])
def test_plant_step_matches_numpy_model_gpu(name, noise):
    _check_plant_step(name, None, "cuda", noise)


def _check_plant_step_params(name, lib, device, B=4):
    """plant_params: row b against the NumPy functions of with_params(model, row_b); for the Van der Pol plugin, whose NumPy twin
    has fixed constants, against the oscillator's step written out here with the row's (mu, dt, u_max)."""
    rng = np.random.default_rng(5)
    model = _model(name)
    eng = _generic_engine(model, B, lib, device, np.random.default_rng(6))
    nx, nu, ny = eng.nx, eng.nu, eng.dims.ny
    rows = param_rows(model, B, 3)
    x = np.asarray(model.x0, float).reshape(1, nx) + 0.3 * rng.normal(size=(B, nx))
    u = 0.5 * rng.normal(size=(B, nu)) + (model.gravity / nu if hasattr(model, "gravity") else 0.0)
    sig_zeta, ex, ey = _spd(rng, ny, 1e-3), rng.normal(size=(B, nx)), rng.normal(size=(B, ny))
    xd, cost = _dev(x, eng), torch.zeros(B, dtype=eng.dtype, device=eng.device)
    y = eng.plant_step(xd, _dev(u, eng), sig_zeta, _dev(ex, eng), _dev(ey, eng), cost=cost, plant_params=rows)
    zg = np.asarray(model.zg, float).reshape(1, -1)
    for b in range(B):
        mb = with_params(model, rows[b])
        s = slice(b, b + 1)
        if name == "VanDerPol":  # tests/plugins/van_der_pol.hpp in NumPy, with this row's constants
            mu, dt, u_max = rows[b]
            v = x[s, 1] + dt * (mu * (1.0 - x[s, 0] ** 2) * x[s, 1] - x[s, 0] + np.clip(u[s, 0], -u_max, u_max))
            xn = np.stack((x[s, 0] + dt * v, v), axis=1) + ex[s] @ np.linalg.cholesky(np.asarray(model.sig_eta, float)).T
            yn = xn + ey[s] @ np.linalg.cholesky(sig_zeta).T
            err = np.asarray(model.observe(np.concatenate((x[s], u[s]), axis=1))).reshape(1, -1) - zg
            cn = np.einsum("bi,ij,bj->b", err, eng.QR, err)
        else:
            xn, yn, cn = _numpy_plant(mb, x[s], u[s], np.asarray(mb.sig_eta, float), sig_zeta, ex[s], ey[s], eng.QR, zg)
        assert_close(parity.np_(xd).T[s], xn, 1e-10, f"{name} plant_params row {b} x'")
        assert_close(parity.np_(y).T[s], yn, 1e-10, f"{name} plant_params row {b} y")
        assert_close(parity.np_(cost)[s], cn, 1e-10, f"{name} plant_params row {b} cost")
    assert np.abs(parity.np_(xd).T[0] - _numpy_plant(model, x[:1], u[:1], np.asarray(model.sig_eta, float), sig_zeta, ex[:1], None,
                                                    eng.QR, zg)[0]).max() > 0  # the rows do differ from the nominal plant


PARAMETERISED = ["LinearKnown", "PlanarQuadrotor", "Quadrotor12", "VanDerPol"]


@pytest.mark.parametrize("name", PARAMETERISED)
def test_plant_step_per_trajectory_plants_cpu(name):
    _check_plant_step_params(name, hostsim.load(), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARAMETERISED)
def test_plant_step_per_trajectory_plants_gpu(name):
    _check_plant_step_params(name, None, "cuda")


def test_plant_step_refuses_what_it_cannot_do():
    lib = hostsim.load()
    eng = _generic_engine(_model("PendulumKnown"), 2, lib, "cpu", np.random.default_rng(0))
    x, u = eng.x0.clone(), torch.zeros(1, 2, dtype=eng.dtype)
    with pytest.raises(ValueError):  # a model without parameters has no other plant
        eng.plant_step(x, u, plant_params=np.zeros((2, 1)))
    with pytest.raises(ValueError):  # measurement noise without its covariance
        eng.plant_step(x, u, eps_y=torch.zeros(3, 2, dtype=eng.dtype))
    with pytest.raises(RuntimeError):  # ... or with one that is not positive definite: I2C_EINVAL
        eng.plant_step(x, u, -np.eye(3), eps_y=torch.zeros(3, 2, dtype=eng.dtype))
    # the plant step reads no device buffer of the problem: a problem with its scalar fields and constants alone is enough
    p = eng._make_problem()
    p.x0 = p.sig_x0 = p.alpha = p.feedforward = p.temp = None
    x1 = eng.x0.clone()
    assert lib.i2c_plant_step(C.byref(p), None, x1.data_ptr(), u.data_ptr(), None, None, None, None, None, None, None) == 0
    x2 = eng.x0.clone()
    eng.plant_step(x2, u, observe_state=True)
    assert torch.equal(x1, x2)
    p.B = 0
    assert lib.i2c_plant_step(C.byref(p), None, x1.data_ptr(), u.data_ptr(), None, None, None, None, None, None, None) == -1


# ---- the MPC engines of checks 2 - 6 -----------------------------------------------------------------------------------------
def _mpc_engine(name, B, T, lib, device, seed=0, z_rows=None, x0=None, mu_u=None, sig_x0=None, **kw):
    """An engine set up for the receding-horizon loop (per-cell temperatures, feedback from the first iteration) on the small
    problem of tests/test_model_params_batch.py, trajectories perturbed per row; z_rows: per-cell targets (T, nz)."""
    model = _model(name)
    p = problem(model, T)
    rng = np.random.default_rng(seed)
    if x0 is None:
        x0 = np.tile(p["x0"], (B, 1)) + 1e-2 * rng.normal(size=(B, model.dim_x))
    if mu_u is None:
        mu_u = np.broadcast_to(p["mu_u"], (B, T, model.dim_u)) + 1e-2 * rng.normal(size=(B, T, model.dim_u))
    eng = pkg.BatchedI2c(model, T, p["Q"], p["R"], p["Qf"], p["alpha"], p["tol"], mu_u, p["sig_u"], x0=x0, sig_x0=sig_x0, device=device,
                         lib=lib, z_traj=z_rows, **kw)
    eng.tau = T - 1
    eng.enable_per_cell_alpha()
    return eng


def _targets(model, n_z, rng):
    """A slowly moving reference around the model's goal, (n_z, nz)."""
    zg = np.asarray(model.zg, float).reshape(1, -1)
    return zg + 0.05 * np.cumsum(rng.normal(size=(n_z, zg.shape[1])), axis=0) / np.sqrt(n_z)


def _loop_of_pieces(eng, N, n_iter, sig_zeta, x_true, eps_x, eps_y, zt, observe_state, plant_params=None):
    """The episode written out with the single calls: mpc_step, then plant_step, per control step."""
    nu = eng.nu
    x = x_true.clone()
    cost = torch.zeros(eng.B, dtype=eng.dtype, device=eng.device)
    hist = {k: [] for k in ("x", "u", "y", "mu")}
    y = u = None
    for k in range(N):
        z_new = None if zt is None else zt[min(k + eng.H, zt.shape[0] - 1)]
        if y is None:
            eng.mpc_step(n_iter, z_new=z_new)
        else:
            eng.mpc_step(n_iter, y, u, sig_zeta, z_new=z_new)
        u = eng._mpc_action[:nu].clone()
        hist["mu"].append(eng.x0.clone())
        hist["x"].append(x.clone())
        hist["u"].append(u)
        y = eng.plant_step(x, u, sig_zeta, None if eps_x is None else eps_x[k], None if eps_y is None else eps_y[k],
                           observe_state=observe_state, z_ref=None if zt is None else zt[min(k, zt.shape[0] - 1)], cost=cost,
                           plant_params=plant_params)
        if y is not None:
            hist["y"].append(y.clone())
    out = {k: torch.stack(v).permute(2, 0, 1) for k, v in hist.items() if v}
    out.update(cost=cost, x_true=x.T)
    return out


SIG_ZETA = {"PendulumKnown": 1e-4 * np.eye(3), "PlanarQuadrotor": 1e-4 * np.eye(8), "Quadrotor12": 1e-4 * np.eye(9),
            "LinearKnown": 1e-4 * np.eye(2), "VanDerPol": 1e-4 * np.eye(2)}
STATE = ("post", "x0", "sig_x0", "alpha_cell", "status", "feedforward", "z")


def _check_episode_is_its_pieces(name, lib, device, observe_state, z_len, B=3, T=5, N=7, n_iter=2, **kw):
    """z_len: None (no per-cell targets), "short" (n_z < N + T: the last row repeats) or "long" (n_z > N + T)."""
    rng = np.random.default_rng(2)
    model = _model(name)
    z = None if z_len is None else _targets(model, T + 3 if z_len == "short" else N + T + 4, rng)
    a = _mpc_engine(name, B, T, lib, device, z_rows=None if z is None else z[:T], **kw)
    b = _mpc_engine(name, B, T, lib, device, z_rows=None if z is None else z[:T], **kw)
    sig_zeta = SIG_ZETA[name]
    gen = torch.Generator(device=a.device).manual_seed(5)
    x_true = parity.np_(a.x0).T + 1e-2 * rng.normal(size=(B, a.nx))
    keep = ("x", "u", "mu") + (() if observe_state else ("y",))
    ra = a.run_closed_loop(N, n_iter, sig_zeta, x_true=x_true, generator=gen, z_traj=z, observe_state=observe_state, keep=keep)
    assert ra["eps_x"].shape == (N, a.nx, B) and (ra["eps_y"] is None) == bool(observe_state)
    zt = None if z is None else torch.as_tensor(np.broadcast_to(z[:, :, None], z.shape + (B,)).copy(), dtype=a.dtype, device=a.device)
    rb = _loop_of_pieces(b, N, n_iter, sig_zeta, _dev(x_true, b), ra["eps_x"], ra["eps_y"], zt, observe_state)
    what = f"{name} {'observed' if observe_state else 'filtered'} z={z_len} [{a.forward_family}/{a.backward_family}]"
    assert a.failures() == [] and b.failures() == [], what
    for k in keep + ("cost", "x_true"):
        assert torch.equal(ra[k], rb[k]), f"{what}: {k} of the episode differs from the loop of its pieces"
    for k in STATE:
        ta, tb = getattr(a, k), getattr(b, k)
        assert (ta is None and tb is None) or torch.equal(ta, tb), f"{what}: engine.{k}"
    assert (a.t0, a.terminal_cell) == (b.t0, b.terminal_cell) == (N % T, -1), what
    assert (a._problem.t0, a._problem.terminal_cell) == (a.t0, a.terminal_cell)
    assert bool(torch.all(torch.isfinite(ra["cost"]))) and float(ra["cost"].min()) > 0.0
    # ... and the engine goes on where the episode left it: one more single control step on both
    ua, ub = a.mpc_step(n_iter)[0].clone(), b.mpc_step(n_iter)[0].clone()
    assert torch.equal(ua, ub) and torch.equal(a.post, b.post), what + ": the step after the episode"
    return a


EPISODES = [
    ("PendulumKnown", False, "short", {}),
    ("PendulumKnown", True, "long", {}),
    ("PendulumKnown", False, None, {}),
    ("PendulumKnown", False, "long", dict(inference="linearize")),
    ("PlanarQuadrotor", False, "long", dict(group_lanes=64)),
    ("PlanarQuadrotor", True, "short", dict(group_lanes=64)),
    ("Quadrotor12", False, "short", {}),
    ("Quadrotor12", True, None, {}),
    ("Quadrotor12", False, "long", dict(group_lanes=_native.LANES_QUAD)),
    # fp32 arithmetic (4-byte rows in the episode's history / noise / target offsets, the noise factors narrowed to float)
    ("PendulumKnown", False, "short", dict(dtype=torch.float32, allow_inexact=True)),
    ("LinearKnown", True, "long", dict(dtype=torch.float32, allow_inexact=True)),
]
FAMILY = {"PendulumKnown": "lane", "LinearKnown": "lane", "PlanarQuadrotor": "quad", "Quadrotor12": "wave"}


def _episode_case(name, observe_state, z_len, kw, lib, device):
    eng = _check_episode_is_its_pieces(name, lib, device, observe_state, z_len, **kw)
    assert eng.forward_family == ("quad" if kw.get("group_lanes") == _native.LANES_QUAD else FAMILY[name])


@pytest.mark.parametrize("name,observe_state,z_len,kw", EPISODES)
def test_episode_is_its_pieces_cpu(name, observe_state, z_len, kw):
    _episode_case(name, observe_state, z_len, kw, hostsim.load(), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name,observe_state,z_len,kw", EPISODES)
def test_episode_is_its_pieces_gpu(name, observe_state, z_len, kw):
    _episode_case(name, observe_state, z_len, kw, None, "cuda")


# ---- 3. against today's host-driven loop --------------------------------------------------------------------------------------
HOST_LOOP_SEEDS = (0, 1, 2)
# Worst max-norm relative deviation (over x, u, y, mu and the cost, over HOST_LOOP_SEEDS) between the episode and the loop a
# user writes today, measured on the host simulation with N = 8, B = 4, T = 10, two iterations per step:
#   LinearKnown 1.02e-13 (the action of seed 2; states, measurements, beliefs and cost stay below 4e-15),
#   PlanarQuadrotor 7.66e-15
# (the two plants differ in the last bits and the loop feeds that back through the controller gain). The bound is ten times
# the worst of them, far inside the replay tests' 1e-6.
HOST_LOOP_TOL = 1.02e-12


def _check_against_host_loop(name, lib, device, seed, B=4, T=10, N=8, n_iter=2):
    """mpc_step per step, the action read back, the NumPy plant and measurement of check 1, (y, u) staged up again."""
    model = _model(name)
    a = _mpc_engine(name, B, T, lib, device, seed=seed)
    b = _mpc_engine(name, B, T, lib, device, seed=seed)
    sig_zeta, sig_eta = SIG_ZETA[name], np.asarray(model.sig_eta, float)
    rng = np.random.default_rng(100 + seed)
    x = parity.np_(a.x0).T + 1e-3 * rng.normal(size=(B, a.nx))
    ra = a.run_closed_loop(N, n_iter, sig_zeta, x_true=x, generator=torch.Generator(device=a.device).manual_seed(seed),
                           keep=("x", "u", "y", "mu"))
    ex, ey = parity.np_(ra["eps_x"]), parity.np_(ra["eps_y"])
    zg = np.asarray(model.zg, float).reshape(1, -1)
    hist, cost, y, u = {k: [] for k in ("x", "u", "y", "mu")}, np.zeros(B), None, None
    for k in range(N):
        mu_u = b.mpc_step(n_iter)[0] if y is None else b.mpc_step(n_iter, _dev(y, b), _dev(u, b), sig_zeta)[0]
        u = parity.np_(mu_u).copy()  # (on the host simulation np_ is a view of the engine's action row)
        hist["mu"].append(parity.np_(b.x0).T.copy())
        hist["x"].append(x)
        hist["u"].append(u)
        x, y, c = _numpy_plant(model, x, u, sig_eta, sig_zeta, ex[k].T, ey[k].T, b.QR, zg)
        cost += c
        hist["y"].append(y)
    assert a.failures() == [] and b.failures() == []
    worst = 0.0
    for k, v in hist.items():
        ref = np.stack(v, axis=1)
        dev = float(np.max(np.abs(parity.np_(ra[k]) - ref)) / np.max(np.abs(ref)))
        print(f"closed loop vs host loop, {name} seed {seed}: {k} deviates by {dev:.2e}")
        worst = max(worst, dev)
    dev = float(np.max(np.abs(parity.np_(ra["cost"]) - cost)) / np.max(np.abs(cost)))
    print(f"closed loop vs host loop, {name} seed {seed}: cost deviates by {dev:.2e}")
    worst = max(worst, dev)
    assert worst <= HOST_LOOP_TOL, f"{name} seed {seed}: {worst:.2e} > {HOST_LOOP_TOL:.1e}"
    # the loop is closed: the plants stay where the controller holds them
    assert np.max(np.abs(parity.np_(ra["x"])[:, -1] - parity.np_(ra["mu"])[:, -1])) < 0.1


@pytest.mark.parametrize("seed", HOST_LOOP_SEEDS)
@pytest.mark.parametrize("name", ["LinearKnown", "PlanarQuadrotor"])
def test_episode_matches_host_driven_loop_cpu(name, seed):
    _check_against_host_loop(name, hostsim.load(), "cpu", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", HOST_LOOP_SEEDS)
@pytest.mark.parametrize("name", ["LinearKnown", "PlanarQuadrotor"])
def test_episode_matches_host_driven_loop_gpu(name, seed):
    _check_against_host_loop(name, None, "cuda", seed)


# ---- 4. batch independence and failure isolation ------------------------------------------------------------------------------
def _episode_rows(eng, N, n_iter, name, x_true, eps_x, eps_y, **kw):
    r = eng.run_closed_loop(N, n_iter, SIG_ZETA[name], x_true=x_true, eps_x=eps_x, eps_y=eps_y, keep=("x", "u", "y", "mu"), **kw)
    return {k: r[k] for k in ("x", "u", "y", "mu", "cost", "x_true")}


def _check_batch_independence(name, lib, device, B=67, row=41, T=6, N=4, n_iter=2):
    rng = np.random.default_rng(9)
    model = _model(name)
    p = problem(model, T)
    x0 = np.tile(p["x0"], (B, 1)) + 1e-2 * rng.normal(size=(B, model.dim_x))
    mu_u = np.broadcast_to(p["mu_u"], (B, T, model.dim_u)) + 1e-2 * rng.normal(size=(B, T, model.dim_u))
    big = _mpc_engine(name, B, T, lib, device, x0=x0, mu_u=mu_u, deterministic_family=True)
    one = _mpc_engine(name, 1, T, lib, device, x0=x0[row:row + 1], mu_u=mu_u[row:row + 1], deterministic_family=True)
    ny = big.dims.ny
    ex = torch.as_tensor(rng.normal(size=(N, big.nx, B)), dtype=big.dtype, device=big.device)
    ey = torch.as_tensor(rng.normal(size=(N, ny, B)), dtype=big.dtype, device=big.device)
    xt = x0 + 1e-2 * rng.normal(size=(B, big.nx))
    rb = _episode_rows(big, N, n_iter, name, xt, ex, ey)
    r1 = _episode_rows(one, N, n_iter, name, xt[row:row + 1], ex[:, :, row:row + 1], ey[:, :, row:row + 1])
    assert big.failures() == [] and one.failures() == []
    for k in rb:
        assert torch.equal(rb[k][row], r1[k][0]), f"{name}: {k} of trajectory {row} depends on its neighbours"
    assert torch.equal(big.post[:, :, row], one.post[:, :, 0])


# B = 1 against the same row inside B = 67. On the host simulation the 12-state model runs a smaller batch (B = 9: its wave kernels
# are simulated with 64 threads per trajectory and cell, and B = 67 would take minutes); the `gpu` form runs B = 67 for every model.
@pytest.mark.parametrize("name", ["PendulumKnown", "PlanarQuadrotor", "Quadrotor12"])
def test_episode_batch_independence_cpu(name):
    _check_batch_independence(name, hostsim.load(), "cpu", **(dict(B=9, row=5, T=5, N=3) if name == "Quadrotor12" else {}))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["PendulumKnown", "PlanarQuadrotor", "Quadrotor12"])
def test_episode_batch_independence_gpu(name):
    _check_batch_independence(name, None, "cuda")


def _check_failure_isolation(name, lib, device, B=5, bad_row=2, T=6, N=4, n_iter=2):
    """One trajectory fails numerically through its inputs (an indefinite sig_x0: a status word, as tests/test_edge_cases.py):
    it is flagged; every other row of every output is bit-identical to the run without the failure."""
    model = _model(name)
    rng = np.random.default_rng(4)
    sig_x0 = np.broadcast_to(np.asarray(model.sig_x0, float), (B, model.dim_x, model.dim_x)).copy()
    good = _mpc_engine(name, B, T, lib, device, sig_x0=sig_x0.copy())
    sig_x0[bad_row] = -sig_x0[bad_row]
    bad = _mpc_engine(name, B, T, lib, device, sig_x0=sig_x0)
    ny = good.dims.ny
    ex = torch.as_tensor(rng.normal(size=(N, good.nx, B)), dtype=good.dtype, device=good.device)
    ey = torch.as_tensor(rng.normal(size=(N, ny, B)), dtype=good.dtype, device=good.device)
    xt = parity.np_(good.x0).T.copy()
    rg, rb = _episode_rows(good, N, n_iter, name, xt, ex, ey), _episode_rows(bad, N, n_iter, name, xt, ex, ey)
    assert good.failures() == []
    fails = bad.failures()
    assert [f[0] for f in fails] == [bad_row] and int(bad.status[bad_row]) != 0, fails
    keep = [b for b in range(B) if b != bad_row]
    for k in rg:
        assert torch.equal(rg[k][keep], rb[k][keep]), f"{name}: {k} of the healthy trajectories changed"
    assert torch.equal(good.post[:, :, keep], bad.post[:, :, keep]) and torch.equal(good.x0[:, keep], bad.x0[:, keep])
    assert not bool(torch.all(torch.isfinite(rb["u"][bad_row])))  # the failed plant stepped on what its action row held


@pytest.mark.parametrize("name", ["PendulumKnown", "PlanarQuadrotor"])
def test_episode_failure_isolation_cpu(name):
    _check_failure_isolation(name, hostsim.load(), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["PendulumKnown", "PlanarQuadrotor", "Quadrotor12"])
def test_episode_failure_isolation_gpu(name):
    _check_failure_isolation(name, None, "cuda")


# ---- 5. plant != model --------------------------------------------------------------------------------------------------------
def _check_plant_not_model(name, lib, device, B=4, T=6, N=5, n_iter=2, row=1):
    model = _model(name)
    rng = np.random.default_rng(8)
    base = np.tile(np.asarray(model.device_params(), np.float64), (B, 1))
    ex = torch.as_tensor(rng.normal(size=(N, model.dim_x, B)))
    engs = [_mpc_engine(name, B, T, lib, device) for _ in range(3)]
    ny = engs[0].dims.ny
    ey = torch.as_tensor(rng.normal(size=(N, ny, B)))
    xt = parity.np_(engs[0].x0).T.copy()
    r_none = _episode_rows(engs[0], N, n_iter, name, xt, ex, ey)
    r_same = _episode_rows(engs[1], N, n_iter, name, xt, ex, ey, plant_params=base)
    other = base.copy()
    other[row] = param_rows(model, 1, 12)[0]
    r_other = _episode_rows(engs[2], N, n_iter, name, xt, ex, ey, plant_params=other)
    assert all(e.failures() == [] for e in engs)
    keep = [b for b in range(B) if b != row]
    for k in r_none:
        assert torch.equal(r_none[k], r_same[k]), f"{name}: {k} with the planner's own parameters as plant_params"
        assert torch.equal(r_none[k][keep], r_other[k][keep]), f"{name}: {k} of an unperturbed row"
    assert not torch.equal(r_none["x_true"][row], r_other["x_true"][row]) and not torch.equal(r_none["u"][row], r_other["u"][row])
    assert engs[2].model_params is None  # the planner's model is untouched


@pytest.mark.parametrize("name", ["LinearKnown", "PlanarQuadrotor", "VanDerPol"])
def test_episode_plant_differs_from_model_cpu(name):
    _check_plant_not_model(name, hostsim.load(), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["LinearKnown", "PlanarQuadrotor", "Quadrotor12", "VanDerPol"])
def test_episode_plant_differs_from_model_gpu(name):
    _check_plant_not_model(name, None, "cuda")


def test_episode_plant_params_need_a_parameterised_model():
    eng = _mpc_engine("PendulumKnown", 2, 5, hostsim.load(), "cpu")
    with pytest.raises(ValueError):
        eng.run_closed_loop(2, 1, SIG_ZETA["PendulumKnown"], plant_params=np.zeros((2, 1)))
    # ... and the C entry point itself answers I2C_EINVAL to a plant-parameter pointer on such a model
    st, ep = _native.I2cMpcStep(), _native.I2cEpisode()
    eng._fill_mpc_step(st, 1)
    buf = torch.zeros(8, 2, dtype=eng.dtype)
    ep.n_steps, ep.x_true, ep.y, ep.u, ep.cost = 1, buf[0:2].data_ptr(), buf[2:5].data_ptr(), buf[5:6].data_ptr(), buf[6].data_ptr()
    ep.plant_params_b = buf[7].data_ptr()
    assert eng.lib.i2c_mpc_episode(C.byref(eng._problem), C.byref(st), C.byref(ep), None) == -1
    assert eng.t0 == 0 and eng.failures() == []


# ---- 6. ABI -------------------------------------------------------------------------------------------------------------------
def _check_abi(lib, device):
    assert lib.i2c_abi_version() == 9 == _native.ABI_VERSION
    assert lib.i2c_problem_size() == C.sizeof(_native.I2cProblem)
    for name in ("i2c_plant_step", "i2c_mpc_episode"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    # the Van der Pol plugin, rebuilt against v9, runs an episode; the tables of a v8 model library are refused
    eng = _mpc_engine("VanDerPol", 3, 6, lib, device)
    assert eng.model_id >= _native.PLUGIN_BASE
    r = eng.run_closed_loop(8, 2, SIG_ZETA["VanDerPol"], generator=torch.Generator(device=eng.device).manual_seed(1), keep=("x", "u", "y", "mu"))
    assert eng.failures() == [] and all(bool(torch.all(torch.isfinite(r[k]))) for k in ("x", "u", "y", "mu", "cost"))
    assert r["x"].shape == (3, 8, 2) and r["u"].shape == (3, 8, 1) and r["y"].shape == (3, 8, 2) and eng.t0 == 8 % 6
    assert float(r["x"][:, -1].abs().max()) < float(r["x"][:, 0].abs().max())  # the oscillator is being driven to the origin
    from i2c.known_models import KnownModel  # noqa: F401  (the plugin's library was built by resolve_model_id)
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("i2c_amd_build", os.path.join(os.path.dirname(pkg.__file__), "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    path = build.model_lib_path("van_der_pol", host_sim=lib.is_host_sim, out_dir=os.path.dirname(lib.path) if lib.is_host_sim else None)
    dll = C.CDLL(path)
    dll.i2c_model_ops.restype, dll.i2c_model_ops.argtypes = C.c_void_p, [C.c_int]
    assert dll.i2c_model_abi_version() == 9
    ops = [dll.i2c_model_ops(k) for k in range(3)]
    assert lib.i2c_register_model(9, ops[0], ops[1], ops[2], None) == eng.model_id
    assert lib.i2c_register_model(8, ops[0], ops[1], ops[2], None) == -1  # I2C_EINVAL: a model library of ABI v8


def test_abi_v9_cpu():
    _check_abi(hostsim.load(), "cpu")


@pytest.mark.gpu
def test_abi_v9_gpu():
    _check_abi(pkg.load_library(), "cuda")


def test_run_closed_loop_is_reproducible_from_a_seed():
    lib = hostsim.load()
    runs = []
    for _ in range(2):
        eng = _mpc_engine("PendulumKnown", 3, 5, lib, "cpu")
        runs.append(eng.run_closed_loop(6, 1, SIG_ZETA["PendulumKnown"], generator=torch.Generator().manual_seed(3), keep=("x", "u", "y")))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in ("x", "u", "y", "cost", "eps_x", "eps_y"))
    eng = _mpc_engine("PendulumKnown", 3, 5, lib, "cpu")
    quiet = eng.run_closed_loop(6, 1, SIG_ZETA["PendulumKnown"], process_noise=False, measurement_noise=False, keep=("x",))
    assert quiet["eps_x"] is None and quiet["eps_y"] is None and not torch.equal(quiet["x"], runs[0]["x"])
    with pytest.raises(ValueError):
        eng.run_closed_loop(1, 1, SIG_ZETA["PendulumKnown"], observe_state=True, keep=("y",))
