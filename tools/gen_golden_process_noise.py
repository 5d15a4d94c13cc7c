"""TEST INFRASTRUCTURE ONLY -- golden vectors for models with STATE-ACTION-DEPENDENT process noise, captured from the REAL reference
(imported through oracle/ref_shim.py, with the helpers of oracle/gen_golden.py). Runs only where the reference exists; no test imports it.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 python tools/gen_golden_process_noise.py [case ...]

The reference's own PendulumKnown / CartpoleKnown are wrapped so that `forward(x_pts)` returns one covariance PER POINT,
sig_eta + Q(x_p) -- its model contract (i2c/model.py:154-156, 205-207), which QuadratureInference.forward_gaussian
(i2c/inference/quadrature.py:46-58) and the MPC filter (i2c/policy/mpc.py:131-137) sum with the rule's covariance weights:
    Q(xu) = s2 u^2 b b^T + c xu[k]^2 e_k e_k^T      (tests/plugins/*_input_noise.hpp, tests/noise_models.py)
The coefficients are recorded in each file's meta["process_noise"]. Every case is run a second time with the constant noise alone, and the
generator asserts that the two runs differ by at least 50x the tolerance the tests compare at (1e-8 on means and covariances, 1e-7 on
the gain, max-norm relative): a kernel that ignores the term cannot pass. Data only is written, under tests/golden/."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G  # noqa: E402  (installs the shim and imports the reference)

import numpy as np  # noqa: E402
from i2c.exp_types import CubatureQuadrature  # noqa: E402  (the reference)
from i2c.i2c import I2cGraph  # noqa: E402
from i2c.model import make_env_model  # noqa: E402

PENDULUM_Q = dict(s2=1e-2, c=1e-3, b=(0.05, 1.0), k=1, iu=2)
CARTPOLE_Q = dict(s2=1e-3, c=1e-4, b=(0.0, 0.0, 1.0, 0.5), k=3, iu=4)
MARGIN = 50.0


def input_noise(xu, coef):
    xu = np.asarray(xu, float)
    b = np.asarray(coef["b"], float)
    e = np.zeros(b.size)
    e[coef["k"]] = 1.0
    a = coef["s2"] * xu[:, coef["iu"]] ** 2
    v = coef["c"] * xu[:, coef["k"]] ** 2
    return a[:, None, None] * np.outer(b, b) + v[:, None, None] * np.outer(e, e)


def noisy(model_name, coef):
    """the reference's model; with `coef`, its forward returns per-point covariances"""
    model = make_env_model(model_name, None)
    if coef is not None:
        base = model.forward

        def forward(xu):
            xn, cov = base(xu)
            return xn, cov + input_noise(xu, coef)

        model.forward = forward
    return model


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, float) - np.asarray(b, float))) / np.max(np.abs(np.asarray(b, float))))


def assert_moves(name, out, base):
    d = {k: rel(out[k], base[k]) for k in ("final/mu_xu0_m", "final/sig_xu0_m", "final/K")}
    print(f"{name}: against the constant-noise run: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert d["final/mu_xu0_m"] >= MARGIN * 1e-8 and d["final/sig_xu0_m"] >= MARGIN * 1e-8 and d["final/K"] >= MARGIN * 1e-7, (name, d)


def em_case(name, model_name, coef, T, hyper, seed, mu_scale, quad=(1, 0, 0), n_detail=2, n_total=8, propagate=False):
    Q, R, Qf, alpha, tol, sig_u = hyper
    np.random.seed(seed)
    mu_u = mu_scale * np.random.randn(T, 1)
    runs = []
    for c in (coef, None):
        model = noisy(model_name, c)
        g = I2cGraph(model, T, Q, R, Qf, alpha, tol, mu_u, sig_u, None, None, CubatureQuadrature(*quad))
        extra = dict(seed=seed)
        if propagate:  # as case_propagate_expert: expert controller, calibrate_alpha before the EM loop
            g._propagate = True
            extra.update(propagate=True, use_expert_controller=True, calibrate_first=True)
        out = G.problem_inputs(model_name, model, T, Q, R, Qf, alpha, tol, mu_u, sig_u, None, None, quad, process_noise=coef, **extra)
        if propagate:
            g.calibrate_alpha()
            out["alpha_calibrated"] = np.asarray(g.alpha, float)
        G.run_em(g, n_detail, n_total, out)
        assert all(np.all(np.isfinite(v)) for k, v in out.items() if k != "meta"), name
        runs.append(out)
    assert_moves(name, runs[0], runs[1])
    G.save(name, runs[0])


PENDULUM_HYPER = (np.diag([1, 100.0, 1]), np.diag([2.0]), np.diag([1, 100.0, 1]), 100.0, 0.0, 2.0 * np.eye(1))  # case_pendulum
CARTPOLE_HYPER = (np.diag([1.0, 1.0, 100.0, 10.0, 1.0]), np.diag([1.0]), np.diag([1.0, 1.0, 100.0, 10.0, 1.0]), 80.0, 0.0, np.eye(1))  # case_cartpole


def case_em_pendulum():
    em_case("em_pendulum_noise_T40", "PendulumKnown", PENDULUM_Q, 40, PENDULUM_HYPER, 3, 1e-2)


def case_em_pendulum_general():
    em_case("em_pendulum_noise_T40_general", "PendulumKnown", PENDULUM_Q, 40, PENDULUM_HYPER, 3, 1e-2, quad=(1.2, 0.44, 0.5))


def case_em_cartpole():
    em_case("em_cartpole_noise_T40", "CartpoleKnown", CARTPOLE_Q, 40, CARTPOLE_HYPER, 0, 1e-3)


def case_em_pendulum_propagate():
    Q, R, Qf, alpha, _, sig_u = PENDULUM_HYPER
    em_case("em_pendulum_noise_T40_propagate", "PendulumKnown", PENDULUM_Q, 40, (Q, R, Qf, alpha, 0.5, sig_u), 1, 1e-2, n_detail=3, n_total=5,
            propagate=True)


def case_mpc_pendulum():
    """as gen_golden.case_mpc_pendulum (feedback), H = 10, 15 steps, on the wrapped model: the planner AND the filter see Q"""
    from i2c.policy.mpc import PartiallyObservedMpcPolicy

    H, steps, n_iter, warm, seed = 10, 15, 2, 8, 5
    Q, R = np.diag([1, 100.0, 1]), np.diag([2.0])
    alpha0, sig_u = 10.0, 2.0 * np.eye(1)
    runs = []
    for c in (PENDULUM_Q, None):
        rng = np.random.default_rng(seed)
        model = noisy("PendulumKnown", c)
        model.sig_zeta = np.diag([1e-4, 1e-4, 1e-3])
        model.measure = lambda x, model=model: model.observe_terminal(x)
        model.dim_y = 3
        mu_u = 0.1 * rng.normal(size=(H, 1))
        z_traj = np.tile(np.asarray(model.zg, float).reshape(1, -1), (steps + H, 1))
        z_traj[:, 2] = 0.3 * np.sin(np.linspace(0, 3, steps + H))
        g = I2cGraph(model, H, Q, R, Q, alpha0, 1.0, mu_u, sig_u, None, None, CubatureQuadrature(1, 0, 0))
        g._propagate = True
        policy = PartiallyObservedMpcPolicy(g, n_iter, sig_u, np.copy(z_traj))
        policy.set_control(feedforward=False)
        out = G.problem_inputs("PendulumKnown", model, H, Q, R, Q, alpha0, 1.0, mu_u, sig_u, None, None, (1, 0, 0), feedforward=False,
                               steps=steps, n_iter=n_iter, warm=warm, process_noise=c)
        out["z_traj"], out["sig_zeta"] = z_traj, model.sig_zeta
        g.calibrate_alpha()
        out["alpha_cal1"] = np.array(g.alpha)
        policy.optimize(warm, model.x0, model.sig_x0)
        g.calibrate_alpha()
        out["alpha_cal2"] = np.array(g.alpha)
        G._mpc_loop(policy, model, steps, out, rng)
        assert all(np.all(np.isfinite(v)) for k, v in out.items() if k != "meta")
        runs.append(out)
    d = {k: rel(runs[0][k], runs[1][k]) for k in ("mu", "covar", "ctrl")}
    print("mpc_pendulum_noise_fb: against the constant-noise run: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert d["mu"] >= MARGIN * 1e-8 and d["covar"] >= MARGIN * 1e-8 and d["ctrl"] >= MARGIN * 1e-7, d
    G.save("mpc_pendulum_noise_fb", runs[0])


CASES = {"em_pendulum": case_em_pendulum, "em_pendulum_general": case_em_pendulum_general, "em_cartpole": case_em_cartpole,
         "em_pendulum_propagate": case_em_pendulum_propagate, "mpc_pendulum": case_mpc_pendulum}

if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
