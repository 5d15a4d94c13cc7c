"""TEST INFRASTRUCTURE ONLY -- golden vectors of the Riccati-form backward messages (I2cGraph._backward_ricatti_msgs, i2c.py:888-893
over I2cCell._backward_ricatti_msgs, :612-678) on well-conditioned problems, captured from the REAL reference (imported through
oracle/ref_shim.py, with the helpers of oracle/gen_golden.py). Runs only where the reference exists; no test imports it.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 python tools/gen_golden_riccati.py [case ...]

tests/golden/lin_lqr_compare.npz is the only other capture of these messages, and its noise of 1e-20 lets them be compared at 1e-4
only. Here: T = 12, B = 1, the arrays that case stores under riccati/*, after ONE forward/backward pass of Linearize() ("ric1/...",
feed-forward cells) and after THREE EM iterations ("ric3/...", feedback cells). The run goes on after the first capture, so the gain the
second iteration feeds back is the Riccati-form one the pass wrote into the cells, as in the reference:

    forward/backward, Riccati (ric1), M-step | one EM iteration | forward/backward, Riccati (ric3)

The *_cellalpha case scales the sig_xi (and lam_xi, sig_xi_terminal: the attributes update_xi sets, i2c.py:976-981) of every cell by
s_t = linspace(0.5, 2, T)[t] before the captured pass -- cells with temperatures of their own, which is what the engine's alpha_cell
holds; the terminal covariance takes the last cell's scale. One graph per capture there (the scaling is undone by the next M-step's
update_xi). The generator asserts that the scaled run differs from the unscaled one by at least 50x the tolerance the tests compare at.
Data only is written, under tests/golden/."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G  # noqa: E402  (installs the shim and imports the reference)

import numpy as np  # noqa: E402
from i2c.exp_types import Linearize  # noqa: E402  (the reference)
from i2c.i2c import I2cGraph  # noqa: E402
from i2c.model import make_env_model  # noqa: E402

T = 12
RICCATI_KEYS = ("K", "k", "sigK", "nu_x0_b", "lambda_x0_b")
SWEEP_KEYS = ("mu_xu0_m", "sig_xu0_m")
MARGIN = 50.0


def cell_scale():
    return np.linspace(0.5, 2.0, T)


def scale_cells(g, s):
    for c, s_t in zip(g.cells, s):
        c.sig_xi = s_t * np.copy(g.sig_xi)
        c.lam_xi = np.linalg.inv(c.sig_xi)
        if g.sig_xi_terminal is not None:
            c.sig_xi_terminal = s[-1] * np.copy(g.sig_xi_terminal)


def capture(g, out, n):
    """the posterior of the pass, then the Riccati messages and the controller they leave in the cells"""
    for k in SWEEP_KEYS:
        a = np.stack([np.asarray(getattr(c, k), float) for c in g.cells])
        out[f"ric{n}/{k}"] = a.reshape(a.shape[0], -1) if k.startswith("mu_") else a
    out[f"ric{n}/alpha"] = np.asarray(g.alpha, float)
    g._backward_ricatti_msgs()
    for k in RICCATI_KEYS:
        a = np.stack([np.asarray(getattr(c, k), float) for c in g.cells])
        out[f"ric{n}/{k}"] = a.reshape(a.shape[0], -1) if k in ("k", "nu_x0_b") else a


def pendulum():
    """hyper-parameters and action prior of gen_golden.case_lin_pendulum at T = 12"""
    np.random.seed(2)
    mu_u = 1e-1 * np.random.randn(T, 1)
    Q = np.diag([1, 100.0, 1])
    return "PendulumKnown", make_env_model("PendulumKnown", None), (Q, np.diag([1.0]), Q, 100.0, 0.99, mu_u, 0.2 * np.eye(1)), \
        dict(jacobian="complex-step stand-in for autograd.jacobian (oracle/ref_shim.py)")


def linear(noise=1e-4):
    """gen_golden.case_lin_linear at T = 12"""
    model = make_env_model("LinearKnown", None)
    model.sig_x0 = noise * np.eye(2)
    model.sig_eta = noise * np.eye(2)
    Q = np.diag([10.0, 10.0])
    return "LinearKnown", model, (Q, np.diag([1.0]), Q, 1e2, 0.0, np.zeros((T, 1)), 1e2 * np.eye(1)), dict(noise=noise)


def graph(problem):
    env, model, (Q, R, Qf, alpha, tol, mu_u, sig_u), extra = problem()
    g = I2cGraph(model, T, Q, R, Qf, alpha, tol, mu_u, sig_u, None, None, Linearize())
    out = G.problem_inputs(env, model, T, Q, R, Qf, alpha, tol, mu_u, sig_u, None, None, (1, 0, 0), inference="linearize", **extra)
    return g, out


def run_plain(problem):
    g, out = graph(problem)
    g.em_iter += 1
    g._forward_backward_msgs()
    capture(g, out, 1)
    g._maximize()
    g.learn_msgs()
    g.em_iter += 1
    g._forward_backward_msgs()
    capture(g, out, 3)
    return out


def run_scaled(problem, s):
    out = None
    for n in (1, 3):
        g, o = graph(problem)
        out = out or o
        for _ in range(n - 1):
            g.learn_msgs()
        g.em_iter += 1
        scale_cells(g, s)
        g._forward_backward_msgs()
        capture(g, out, n)
    return out


def finite(out):
    return all(np.all(np.isfinite(v)) for k, v in out.items() if k != "meta")


def case_pendulum():
    out = run_plain(pendulum)
    assert finite(out)
    G.save("lin_pendulum_riccati_T12", out)


def case_linear():
    out = run_plain(linear)
    assert finite(out)
    G.save("lin_linear_riccati_T12", out)


def case_pendulum_cellalpha():
    import json

    s = cell_scale()
    out, base = run_scaled(pendulum, s), run_scaled(pendulum, np.ones(T))
    assert finite(out)
    for n in (1, 3):
        d = {k: float(np.max(np.abs(out[f"ric{n}/{k}"] - base[f"ric{n}/{k}"])) / np.max(np.abs(base[f"ric{n}/{k}"]))) for k in RICCATI_KEYS if k != "sigK"}
        print(f"lin_pendulum_riccati_T12_cellalpha ric{n}: against the unscaled run: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert min(d.values()) >= MARGIN * 1e-7, d
    out["meta"] = np.array(json.dumps({**json.loads(str(out["meta"])), "cell_scale": [float(v) for v in s]}))
    G.save("lin_pendulum_riccati_T12_cellalpha", out)


CASES = {"pendulum": case_pendulum, "linear": case_linear, "pendulum_cellalpha": case_pendulum_cellalpha}

if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
