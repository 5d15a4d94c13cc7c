"""Models with STATE-ACTION-DEPENDENT process noise: a functor's optional `process_noise` member (csrc/i2c_cell.hpp, INTEGRATION.md
section 3) -- the reference's `sys.forward(x_pts) -> (means, one covariance PER POINT)`, summed over the sigma points with the rule's
covariance weights (i2c/inference/quadrature.py:46-58, i2c/policy/mpc.py:131-137).

  (a) the test-side twin (tests/noise_oracle.py) against goldens captured from the real reference on wrapped models
      (tools/gen_golden_process_noise.py);
  (b) the kernels against those goldens: lane kernels, and the quad forward sweep (group_lanes = 164);
  (c) the kernels against the twin on ragged batches with per-trajectory inputs: lane and quad forward, chunked and fused backward,
      learn(n) against stepwise learn_msgs(), fp32-stored messages;
  (e) the sampling kernels (rollout, plant_step, the episode call) with given eps_x: chol(sig_eta + Q(x, u)) factored per step;
  (f) failure isolation: one trajectory whose Q is indefinite through its parameter;
  (g) what the resolver and the engine refuse for such a model.
Without the feature a model that overrides process_noise is silently solved with constant noise: (b), (c) and (e) fail.
CPU: the host simulation of the kernels; `-m gpu`: the library on the MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import assert_close, load_case
from noise_models import CARTPOLE_Q, MODELS, PENDULUM_Q
from noise_oracle import NoiseOracle, ckf_filter, sample_step
from oracle.i2c_numpy import CubatureRule
from parity import close, np_

pkg = parity.pkg
_native = pkg._native
GENERAL = (1.2, 0.44, 0.5)
KIND_OF = {"PendulumKnown": "pendulum", "CartpoleKnown": "cartpole"}
HYPER = {  # (Q, R, Qf, alpha, tol, sig_u, x0 scale, mu_u scale): gen_golden.case_pendulum / case_cartpole
    "pendulum": (np.diag([1, 100.0, 1]), np.diag([2.0]), np.diag([1, 100.0, 1]), 100.0, 0.0, 2.0 * np.eye(1), 1e-2, 1e-2),
    "cartpole": (np.diag([1.0, 1.0, 100.0, 10.0, 1.0]), np.diag([1.0]), np.diag([1.0, 1.0, 100.0, 10.0, 1.0]), 80.0, 0.0, np.eye(1), 1e-2, 0.3),
}
HYPER["pendulum_expanded"] = HYPER["pendulum"]  # (the same model in the code generator's order of operations: tests/test_process_noise_traced.py)


def _lib(device):
    return hostsim.load() if device == "cpu" else pkg.load_library()


def _models(kind):
    known, twin = MODELS[kind]
    return known(), twin()


# ---- (a), (b): goldens from the reference ---------------------------------------------------------------------------------------
def _twin_from_case(case, **over):
    """golden_util.oracle_from_case for these cases: the twin model and the twin oracle"""
    meta = case.meta
    coef = meta["process_noise"]
    kind = KIND_OF[meta["model"]]
    assert {k: (tuple(v) if isinstance(v, list) else v) for k, v in coef.items()} == {"pendulum": PENDULUM_Q, "cartpole": CARTPOLE_Q}[kind]
    o = NoiseOracle(_models(kind)[1], meta["T"], case.get("Q"), case["R"], case.get("Qf"), meta["alpha"], meta["tol"], case["mu_u"], case["sig_u"],
                    None, None, CubatureRule(*meta["quad"]), **over)
    if meta.get("propagate"):
        o._propagate = True
    if "use_expert_controller" in meta:
        o.use_expert_controller = bool(meta["use_expert_controller"])
    return o


EM_GOLDENS = ["em_pendulum_noise_T40", "em_pendulum_noise_T40_general", "em_cartpole_noise_T40", "em_pendulum_noise_T40_propagate"]


@pytest.mark.parametrize("name", EM_GOLDENS)
def test_twin_against_reference(name, monkeypatch):
    import test_oracle_golden

    monkeypatch.setattr(test_oracle_golden, "oracle_from_case", _twin_from_case)
    test_oracle_golden._run_and_check(name, 1e-8, 1e-7)


def test_twin_filter_against_reference():
    """the filter step of the twin on the reference's own measurement stream: every step's belief from the step before (the policy
    filters from the second step on, mpc.py:156-158), all steps as one batch"""
    g = load_case("mpc_pendulum_noise_fb")
    twin = _models("pendulum")[1]
    twin.measure = twin.observe_terminal
    mu, cov = ckf_filter(twin, g["mu"][:-1], g["covar"][:-1], g["u_prev"][1:], g["y"][1:], g["sig_zeta"])
    assert_close(mu, g["mu"][1:], 1e-9, "filtered means")
    assert_close(cov, g["covar"][1:], 1e-8, "filtered covariances")


def _noise_product_model(case):
    return _models(KIND_OF[case.meta["model"]])[0]


def _kernels_against_golden(name, device, monkeypatch, **kw):
    monkeypatch.setattr(parity, "product_model", _noise_product_model)
    return parity.check_against_golden(name, _lib(device), device, **kw)


LANE_AND_QUAD = [(-1, "lane"), (_native.LANES_QUAD, "quad")]  # (-1: the quad forward sweep is the d = 5 cartpole's default)


@pytest.mark.parametrize("lanes,family", LANE_AND_QUAD, ids=["lane", "quad"])
@pytest.mark.parametrize("name", EM_GOLDENS[:3])
def test_kernels_against_reference_cpu(name, lanes, family, monkeypatch):
    eng = _kernels_against_golden(name, "cpu", monkeypatch, group_lanes=lanes)
    assert eng.forward_family == family


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,family", LANE_AND_QUAD, ids=["lane", "quad"])
@pytest.mark.parametrize("name", EM_GOLDENS[:3])
def test_kernels_against_reference_gpu(name, lanes, family, monkeypatch):
    eng = _kernels_against_golden(name, "cuda", monkeypatch, group_lanes=lanes)
    assert eng.forward_family == family


def test_propagation_against_reference_cpu(monkeypatch):
    eng = _kernels_against_golden(EM_GOLDENS[3], "cpu", monkeypatch)
    assert eng.kernel_family("propagate") == "lane"


@pytest.mark.gpu
def test_propagation_against_reference_gpu(monkeypatch):
    _kernels_against_golden(EM_GOLDENS[3], "cuda", monkeypatch)


def _mpc_replay(device, tol, monkeypatch):
    import test_mpc

    monkeypatch.setattr(parity, "product_model", _noise_product_model)
    pol = test_mpc._replay("mpc_pendulum_noise_fb", _lib(device), device, tol)
    assert pol.engine.kernel_family("filter") == "lane"


def test_mpc_against_reference_cpu(monkeypatch):
    _mpc_replay("cpu", 1e-7, monkeypatch)


@pytest.mark.gpu
def test_mpc_against_reference_gpu(monkeypatch):
    _mpc_replay("cuda", 1e-6, monkeypatch)


# ---- (c): ragged batches against the twin ------------------------------------------------------------------------------------------
def problem(kind, B, T, seed=3):
    Q, R, Qf, alpha, tol, sig_u, sx, su = HYPER[kind]
    known, twin = _models(kind)
    rng = np.random.default_rng(seed)
    x0 = np.asarray(twin.x0, float).reshape(1, -1) + sx * rng.normal(size=(B, twin.dim_x))
    mu_u = su * rng.normal(size=(B, T, 1))
    return known, twin, dict(T=T, Q=Q, R=R, Qf=Qf, alpha=alpha, tol=tol, mu_u=mu_u, sig_u=sig_u, x0=x0)


def engine(known, p, device, **kw):
    return pkg.BatchedI2c(known, p["T"], p["Q"], p["R"], p["Qf"], p["alpha"], p["tol"], p["mu_u"], p["sig_u"], x0=p["x0"], device=device,
                          lib=_lib(device), **kw)


def twin_oracle(twin, p, quad=(1, 0, 0)):
    return NoiseOracle(twin, p["T"], p["Q"], p["R"], p["Qf"], p["alpha"], p["tol"], p["mu_u"], p["sig_u"], rule=CubatureRule(*quad), x0=p["x0"])


def against_twin(device, kind, B, T, n_iters=3, quad=(1, 0, 0), tol=1e-8, **kw):
    known, twin, p = problem(kind, B, T)
    eng, ora = engine(known, p, device, quad=quad, **kw), twin_oracle(twin, p, quad)
    for it in range(1, n_iters + 1):
        eng.learn_msgs()
        ora.learn_msgs()
        what = f"{kind} B={B} T={T} {quad} ({eng.forward_family}/{eng.backward_family}) it{it}"
        f = eng.forward_messages()
        for k in parity.FWD:
            close(np_(f[k]), getattr(ora, k), tol, f"{what} {k}")
        mu, sig = eng.marginal_state_action()
        close(np_(mu), ora.mu_xu0_m, tol, what + " mu_xu0_m")
        close(np_(sig), ora.sig_xu0_m, tol, what + " sig_xu0_m")
        K, k, sigK = eng.local_linear_policy()
        close(np_(K), ora.K, tol * 10, what + " K")
        close(np_(k), ora.k, tol * 10, what + " k")
        close(np_(sigK), ora.sigK, tol * 10, what + " sigK")
        close(np_(eng.alpha), ora.alpha, tol, what + " alpha")
        close(np_(eng.costs_m[-1]), ora.costs_m[-1], tol, what + " cost")
    assert eng.failures() == []
    return eng, ora


# (kind, B, T, rule, group_lanes, backward_mode): B = 1, 5, 67 (more than one wavefront of lanes, a ragged last one; 67 = 16 quad
# wavefronts and three trajectories in the seventeenth), T = 12 and 40, both rules, lane and quad forward, chunked and fused backward
RAGGED = [("pendulum", 1, 12, (1, 0, 0), 0, "auto"), ("pendulum", 5, 40, GENERAL, 0, "fused"), ("pendulum", 67, 40, (1, 0, 0), 0, "chunked"),
          ("pendulum", 67, 12, GENERAL, _native.LANES_QUAD, "auto"), ("pendulum", 5, 40, (1, 0, 0), _native.LANES_QUAD, "chunked"),
          ("cartpole", 1, 40, (1, 0, 0), 0, "auto"), ("cartpole", 67, 12, (1, 0, 0), -1, "fused"), ("cartpole", 5, 40, GENERAL, -1, "chunked"),
          ("cartpole", 67, 12, GENERAL, 0, "auto"), ("cartpole", 5, 40, (1, 0, 0), _native.LANES_QUAD, "fused")]
RAGGED_IDS = [f"{k}-B{B}-T{T}-{'general' if q != (1, 0, 0) else 'unit'}-{'quad' if (g > 0 or (k == 'cartpole' and g == 0)) else 'lane'}-{m}" for k, B, T, q, g, m in RAGGED]


def _ragged(device, kind, B, T, quad, lanes, mode):
    eng, _ = against_twin(device, kind, B, T, quad=quad, group_lanes=lanes, backward_mode=mode)
    # d = 5: the quad forward sweep is the cartpole's default; the lane kernels are asked for with -1
    want = "quad" if (lanes > 0 or (kind == "cartpole" and lanes == 0)) else "lane"
    assert eng.forward_family == want, eng.forward_family


@pytest.mark.parametrize("kind,B,T,quad,lanes,mode", RAGGED, ids=RAGGED_IDS)
def test_ragged_batch_against_twin_cpu(kind, B, T, quad, lanes, mode):
    _ragged("cpu", kind, B, T, quad, lanes, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,T,quad,lanes,mode", RAGGED, ids=RAGGED_IDS)
def test_ragged_batch_against_twin_gpu(kind, B, T, quad, lanes, mode):
    _ragged("cuda", kind, B, T, quad, lanes, mode)


def _learn_equals_stepwise(device, kind, B, T, **kw):
    """learn(n) (one library call: no helper wave, no deferred M-step for such a model) == n x learn_msgs(), bit for bit"""
    known, _, p = problem(kind, B, T)
    a, b = engine(known, p, device, **kw), engine(known, p, device, **kw)
    a.learn(3)
    for _ in range(3):
        b.learn_msgs()
    assert a.failures() == [] and b.failures() == []
    for x, y in zip(a.marginal_state_action() + a.local_linear_policy() + (a.alpha,), b.marginal_state_action() + b.local_linear_policy() + (b.alpha,)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind,B,T", [("pendulum", 67, 40), ("cartpole", 5, 12)])
def test_learn_equals_stepwise_cpu(kind, B, T):
    _learn_equals_stepwise("cpu", kind, B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,T", [("pendulum", 67, 40), ("pendulum", 4096, 12), ("cartpole", 5, 12)])
def test_learn_equals_stepwise_gpu(kind, B, T):
    """(B = 4096: the batch from which an in-tree d <= 5 model's sweep takes the helper wave)"""
    _learn_equals_stepwise("cuda", kind, B, T)


def _propagation_against_twin(device):
    """closed-loop propagation on a ragged batch, general weights (W != 1: the weights of Q are the rule's own)"""
    known, twin, p = problem("pendulum", 5, 12)
    eng, ora = engine(known, p, device, quad=GENERAL), twin_oracle(twin, p, GENERAL)
    eng._propagate = ora._propagate = True
    for _ in range(2):
        eng.learn_msgs()
        ora.learn_msgs()
    pr = eng.propagated()
    for key in ("mu_xu0_pf", "sig_xu0_pf", "mu_x3_pf", "sig_x3_pf"):
        close(np_(pr[key]), getattr(ora, key), 1e-8, "propagation " + key)
    assert eng.failures() == []


def test_propagation_against_twin_cpu():
    _propagation_against_twin("cpu")


@pytest.mark.gpu
def test_propagation_against_twin_gpu():
    _propagation_against_twin("cuda")


def _filter_against_twin(device, B=37):
    known, twin, p = problem("pendulum", B, 4)
    twin.measure = twin.observe_terminal
    eng = engine(known, p, device)
    rng = np.random.default_rng(5)
    mu = np.asarray(twin.x0) + 0.1 * rng.normal(size=(B, 2))
    A = rng.normal(size=(B, 2, 2))
    cov = 1e-3 * (A @ np.swapaxes(A, -1, -2)) + 1e-5 * np.eye(2)
    u, sig_zeta = rng.normal(size=(B, 1)), np.diag([1e-4, 1e-4, 1e-3])
    y = twin.measure(mu) + 0.01 * rng.normal(size=(B, 3))
    eng.set_initial_state(mu, cov)
    dev = lambda a: torch.as_tensor(np.array(a.T, order="C"), dtype=eng.dtype, device=eng.device)  # noqa: E731
    m, c = eng.ckf_filter(dev(y), dev(u), sig_zeta)
    mu_o, cov_o = ckf_filter(twin, mu, cov, u, y, sig_zeta)
    assert_close(np_(m).T, mu_o, 1e-9, "filtered mean")
    assert_close(np_(pkg.engine.unpack_sym(c.T, 2)), cov_o, 1e-8, "filtered covariance")
    assert eng.failures() == []


def test_filter_against_twin_cpu():
    _filter_against_twin("cpu")


@pytest.mark.gpu
def test_filter_against_twin_gpu():
    _filter_against_twin("cuda")


def _mixed_precision(device, kind, lanes, family):
    """fp32-stored messages against the engine's own fp64 run, inside MIXED_BOUNDS["em_pendulum_T200"] as tests/test_precision.py defines
    and measures them, at every iteration: (median over the batch of the per-trajectory posterior-mean deviation, its 99th percentile,
    median cost deviation). Lane kernels and the quad forward sweep (QuadDynamicsNoiseF in k_quad_forward<.., float>: asked for on the
    pendulum, the default of the d = 5 cartpole)."""
    from test_precision import MIXED_BOUNDS, _rel_per_traj

    b_med, b_p99, b_cost = MIXED_BOUNDS["em_pendulum_T200"]
    known, _, p = problem(kind, 5, 40)
    e64, e32 = engine(known, p, device, group_lanes=lanes), engine(known, p, device, group_lanes=lanes, storage_dtype=torch.float32)
    assert e32.mixed and e32.fwd.dtype == torch.float32 and e32.forward_family == e64.forward_family == family
    for it in range(3):
        e64.learn_msgs()
        e32.learn_msgs()
        dm = _rel_per_traj(e32.marginal_state_action()[0], e64.marginal_state_action()[0])
        dc = (e32.costs_m[-1].double() - e64.costs_m[-1]).abs() / e64.costs_m[-1].abs()
        row = dict(it=it, mean_median=float(dm.median()), mean_p99=float(dm.quantile(0.99)), cost_median=float(dc.median()))
        print(f"fp32-stored {kind} {family}: {row}")
        assert row["mean_median"] <= b_med and row["mean_p99"] <= b_p99 and row["cost_median"] <= b_cost, row
    assert e64.failures() == [] and e32.failures() == []


MIXED = [("pendulum", 0, "lane"), ("pendulum", _native.LANES_QUAD, "quad"), ("cartpole", 0, "quad")]


@pytest.mark.parametrize("kind,lanes,family", MIXED)
def test_mixed_precision_cpu(kind, lanes, family):
    _mixed_precision("cpu", kind, lanes, family)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lanes,family", MIXED)
def test_mixed_precision_gpu(kind, lanes, family):
    _mixed_precision("cuda", kind, lanes, family)


def _quad_both_sweeps(device):
    """group_lanes = 64 on such a model: the quad forward sweep AND the quad backward walk (which reads what the forward sweep stored)"""
    eng, _ = against_twin(device, "cartpole", 5, 12, group_lanes=64)
    assert (eng.forward_family, eng.backward_family) == ("quad", "quad")


def test_quad_both_sweeps_cpu():
    _quad_both_sweeps("cpu")


@pytest.mark.gpu
def test_quad_both_sweeps_gpu():
    _quad_both_sweeps("cuda")


def test_twin_without_the_term_is_the_oracle():
    """NoiseOracle restates two methods of I2cOracle for one line each: with Q = 0 it must BE the oracle, bit for bit (a drift alarm)"""
    from oracle.i2c_numpy import I2cOracle

    class ZeroNoise(type(_models("pendulum")[1])):
        def process_noise(self, xu):
            return np.zeros(np.shape(xu)[:-1] + (2, 2))

    _, twin, p = problem("pendulum", 3, 12)
    args = (p["T"], p["Q"], p["R"], p["Qf"], p["alpha"], 0.5, p["mu_u"], p["sig_u"])
    a = NoiseOracle(ZeroNoise(), *args, rule=CubatureRule(*GENERAL), x0=p["x0"])
    b = I2cOracle(twin, *args, rule=CubatureRule(*GENERAL), x0=p["x0"])
    a._propagate = b._propagate = True
    for _ in range(3):
        a.learn_msgs()
        b.learn_msgs()
    for k in parity.FWD + ["mu_xu0_m", "sig_xu0_m", "K", "k", "sigK", "mu_x3_pf", "sig_x3_pf", "alpha"]:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


# ---- (e): sampling ---------------------------------------------------------------------------------------------------------------
def _rollout(device, kind):
    B, T, NR = 5, 12, 2
    known, twin, p = problem(kind, B, T)
    eng = engine(known, p, device)
    eng.learn(2)
    rng = np.random.default_rng(11)
    nx, N = twin.dim_x, NR * B
    eps = rng.normal(size=(T, nx, N))
    out = eng.rollout(NR, eps_x=eps, want=("xu", "x_final"))
    K, k, _ = (np_(t) for t in eng.local_linear_policy())
    x = np.tile(p["x0"], (NR, 1))  # rollout n = r * B + b
    for t in range(T):
        u = np.einsum("nij,nj->ni", np.tile(K[:, t], (NR, 1, 1)), x) + np.tile(k[:, t], (NR, 1))
        assert_close(np_(out["xu"]).reshape(N, T, -1)[:, t], np.concatenate((x, u), axis=-1), 1e-12, f"{kind} rollout xu, step {t}")
        x = sample_step(twin, x, u, eps[t].T)
    assert_close(np_(out["x_final"]).reshape(N, -1), x, 1e-12, f"{kind} rollout final state")
    # one plant whose sig_eta + Q(x, u) is not positive definite (its sign parameter): both of its rollouts are NaN from the first step
    # on, the others are what they were, bit for bit
    sign = np.ones((B, 1))
    sign[3] = -1e3
    bad = eng.rollout(NR, eps_x=eps, want=("xu", "x_final"), model_params=sign)
    assert torch.isnan(bad["x_final"][:, 3]).all() and torch.isnan(bad["xu"][:, 3, 1:, :nx]).all()
    assert torch.equal(bad["xu"][:, 3, 0], out["xu"][:, 3, 0])  # (the state BEFORE the first step is recorded)
    keep = torch.as_tensor(np.delete(np.arange(B), 3), device=eng.device)
    assert torch.equal(bad["x_final"][:, keep], out["x_final"][:, keep]) and torch.equal(bad["xu"][:, keep], out["xu"][:, keep])


@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_rollout_cpu(kind):
    _rollout("cpu", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_rollout_gpu(kind):
    _rollout("cuda", kind)


def _plant_step(device, kind):
    B = 37
    known, twin, p = problem(kind, B, 4)
    eng = engine(known, p, device)
    rng = np.random.default_rng(13)
    nx = twin.dim_x
    x = np.asarray(twin.x0) + 0.3 * rng.normal(size=(B, nx))
    u, eps = rng.normal(size=(B, 1)), rng.normal(size=(B, nx))
    dev = lambda a: torch.as_tensor(np.array(a.T, order="C"), dtype=eng.dtype, device=eng.device)  # noqa: E731
    xd = dev(x)
    eng.plant_step(xd, dev(u), eps_x=dev(eps), observe_state=True)
    assert_close(np_(xd).T, sample_step(twin, x, u, eps), 1e-12, f"{kind} plant step")
    # a step whose sig_eta + Q(x, u) is not positive definite (the sign parameter of that plant) leaves that lane's state NaN
    sign = np.ones((B, 1))
    sign[3] = -1.0
    xd = dev(x)
    eng.plant_step(xd, dev(u), eps_x=dev(eps), observe_state=True, plant_params=sign)
    got = np_(xd).T
    assert np.all(np.isnan(got[3])) and np.all(np.isfinite(np.delete(got, 3, axis=0)))
    assert_close(np.delete(got, 3, axis=0), np.delete(sample_step(twin, x, u, eps), 3, axis=0), 1e-12, f"{kind} plant step, the other lanes")


@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_plant_step_cpu(kind):
    _plant_step("cpu", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_plant_step_gpu(kind):
    _plant_step("cuda", kind)


def _episode(device):
    """an episode of 6 steps == mpc_step + plant_step one by one, bit for bit (fully observed loop, given eps_x)"""
    B, T, N = 5, 10, 6
    known, _, p = problem("pendulum", B, T)
    a, b = engine(known, p, device), engine(known, p, device)
    for e in (a, b):
        e.learn(2)
    eps = torch.as_tensor(np.random.default_rng(17).normal(size=(N, 2, B)), dtype=a.dtype, device=a.device)
    out = a.run_closed_loop(N, 2, observe_state=True, eps_x=eps, keep=("x", "u"))
    x = b.x0.clone()
    for k in range(N):
        assert torch.equal(out["x"][:, k], x.T)
        u, _ = b.mpc_step(2)
        assert torch.equal(out["u"][:, k], u)
        b.plant_step(x, u.T.contiguous(), eps_x=eps[k], observe_state=True)
    assert torch.equal(out["x_true"], x.T) and a.failures() == [] and b.failures() == []


def test_episode_equals_steps_cpu():
    _episode("cpu")


@pytest.mark.gpu
def test_episode_equals_steps_gpu():
    _episode("cuda")


# ---- (f): failure isolation --------------------------------------------------------------------------------------------------------
def _failure_isolation(device, kind, lanes):
    B, T, bad = 67, 12, 41
    known, _, p = problem(kind, B, T)
    sign = np.ones((B, 1))
    clean = engine(known, p, device, group_lanes=lanes, model_params=sign)
    sign[bad] = -1e3  # (far beyond what the transform's own covariance absorbs: sig_y + sig_eta + sum_p w_p Q(x_p) is indefinite)
    eng = engine(known, p, device, group_lanes=lanes, model_params=sign)
    for e in (clean, eng):
        for _ in range(2):
            e.learn_msgs()
    assert clean.failures() == []
    fails = eng.failures()
    assert [f[0] for f in fails] == [bad], fails
    keep = torch.as_tensor(np.delete(np.arange(B), bad), device=eng.device)
    for x, y in zip(eng.marginal_state_action() + eng.local_linear_policy(), clean.marginal_state_action() + clean.local_linear_policy()):
        assert torch.equal(x[keep], y[keep])


@pytest.mark.parametrize("kind,lanes", [("pendulum", 0), ("pendulum", _native.LANES_QUAD), ("cartpole", -1), ("cartpole", 0)])
def test_failure_isolation_cpu(kind, lanes):
    _failure_isolation("cpu", kind, lanes)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lanes", [("pendulum", 0), ("pendulum", _native.LANES_QUAD), ("cartpole", -1), ("cartpole", 0)])
def test_failure_isolation_gpu(kind, lanes):
    _failure_isolation("cuda", kind, lanes)


# ---- (g): refusals -------------------------------------------------------------------------------------------------------------------
def _refusals(device):
    lib = _lib(device)
    known, _, p = problem("pendulum", 5, 12)
    mid = known.resolve_model_id(lib)
    pr = _native.I2cProblem()
    pr.abi_version, pr.model_id, pr.B, pr.T, pr.quad_alpha = _native.ABI_VERSION, mid, 64, 40, 1.0
    sweeps = (_native.SWEEP_FORWARD, _native.SWEEP_BACKWARD, _native.SWEEP_PROPAGATE, _native.SWEEP_FILTER)

    def families(lanes, inference=_native.INF_CUBATURE):
        pr.group_lanes, pr.inference = lanes, inference
        if inference == _native.INF_GAUSS_HERMITE:
            pr.gh_degree = 3
        return [lib.i2c_kernel_family(C.byref(pr), s) for s in sweeps]

    L, Q, NO = _native.FAMILY_LANE, _native.FAMILY_QUAD, -2  # (I2C_ENOTSUP, include/i2c_hip.h)
    assert families(0) == [L, L, L, L] and families(-1) == [L, L, L, L]
    assert families(_native.LANES_QUAD)[0] == Q and families(_native.LANES_QUAD)[2:] == [L, L]
    assert families(4) == [NO] * 4                               # the group kernels the in-tree pendulum has
    assert families(0, _native.INF_LINEARIZE) == [NO] * 4
    assert families(0, _native.INF_GAUSS_HERMITE) == [NO] * 4
    assert families(64, _native.INF_GAUSS_HERMITE) == [NO] * 4   # the grid family
    # the engine refuses the same before it allocates
    for kw in (dict(inference="linearize"), dict(inference="gauss_hermite", gh_degree=3), dict(group_lanes=4), dict(group_lanes=True)):
        with pytest.raises(ValueError, match="process_noise"):
            engine(known, p, device, **kw)
    # the Riccati messages read the constant sig_eta alone
    eng = engine(known, p, device)
    pl = eng._make_problem()
    pl.inference = _native.INF_LINEARIZE  # (the call's own precondition; the model's table answers before anything is launched)
    buf, st = eng._ptr(eng.fwd), eng._ptr(eng.status)
    assert lib.i2c_riccati_sweep(C.byref(pl), buf, buf, buf, buf, buf, st, eng._stream()) == NO
    # the engine asks the LIBRARY whether the functor has the member: an override over a functor without it (here the in-tree pendulum's
    # model_id kept) would be solved with constant noise and is refused; a header with the member under a class without the override
    # is a model with the term all the same
    from i2c.known_models import PendulumKnown

    class OverrideOnly(PendulumKnown):
        def process_noise(self, xu):
            return np.zeros((np.shape(xu)[0], 2, 2))

    class HeaderOnly(PendulumKnown):
        model_id, hip_header = None, known.hip_header

        def device_params(self):
            return [1.0]

    with pytest.raises(ValueError, match="no process_noise member"):
        engine(OverrideOnly(), p, device)
    assert not HeaderOnly().has_process_noise and engine(HeaderOnly(), p, device).has_process_noise
    with pytest.raises(ValueError, match="process_noise"):
        engine(HeaderOnly(), p, device, inference="linearize")
    assert not engine(PendulumKnown(), p, device, inference="linearize").has_process_noise
    # a model without the member resolves as before: the in-tree pendulum keeps its group kernels
    pr.model_id = 0
    assert families(4)[0] == _native.FAMILY_GROUP


def test_refusals_cpu():
    _refusals("cpu")


@pytest.mark.gpu
def test_refusals_gpu():
    _refusals("cuda")


def test_host_model_contract():
    """KnownModel.forward returns sig_eta + process_noise(xu) per point -- the reference's contract -- and only for a model that has it"""
    from i2c.known_models import PendulumKnown

    known, twin = _models("pendulum")
    xu = np.random.default_rng(0).normal(size=(7, 3))
    xn, cov = known.forward(xu)
    assert cov.shape == (7, 2, 2) and known.has_process_noise and not PendulumKnown().has_process_noise
    assert_close(cov, known.sig_eta + twin.process_noise(xu), 1e-15, "per-point covariance")
    assert_close(xn, twin.dynamics(xu), 1e-15, "means")
    assert np.array_equal(PendulumKnown().forward(xu)[1], np.broadcast_to(known.sig_eta, (7, 2, 2)))
