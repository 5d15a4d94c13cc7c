"""TEST INFRASTRUCTURE ONLY -- Gauss-Hermite goldens of the d >= 5 models, written from the unmodified reference through
oracle/gen_golden.py (its capture / save helpers; that file stays as it is). Run:

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 python tools/gen_gh_golden.py [cartpole] [dcp]

    tests/golden/gh3_cartpole_T30.npz  CartpoleKnown, GaussHermiteQuadrature(3): 3^5 = 243 points per joint transform, 81 for the
                                       terminal one; hyper-parameters of case_cartpole (cartpole_known_quad.py: Q = Qf =
                                       diag(1, 1, 100, 10, 1), R = 1, alpha 80, tol 0, mu_u = 1e-3 randn(seed 0), sig_u = 1);
                                       T = 30, 2 detailed of 4 iterations
    tests/golden/gh3_dcp_T12.npz       DoubleCartpoleKnown, GaussHermiteQuadrature(3): 3^7 = 2 187 points per joint transform, 729
                                       for the terminal one; hyper-parameters of case_double_cartpole (double_cartpole_known_cq.py:
                                       Q = Qf = 1e-3 diag(1, 1, 100, 1, 100, 10, 1, 1), R = 1e-4, alpha 0.05, tol 0.99,
                                       mu_u = 1e-2 randn(seed 0), sig_u = 1); T = 12, 2 detailed of 3 iterations

The reference ran both clean (no non-PD covariance under its own arithmetic) with exactly these parameters: nothing had to be
shortened or tempered. Data only: inputs and the reference's outputs, every array float64.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import I2cGraph, GaussHermiteQuadrature, make_env_model, problem_inputs, run_em, save  # noqa: E402
import numpy as np  # noqa: E402


def case_gh_cartpole(T=30, degree=3, n_detail=2, n_total=4):
    np.random.seed(0)
    mu_u = 1e-3 * np.random.randn(T, 1)
    Q = np.diag([1.0, 1.0, 100.0, 10.0, 1.0])
    R = np.diag([1.0])
    model = make_env_model("CartpoleKnown", None)
    g = I2cGraph(model, T, Q, R, Q, 80.0, 0.0, mu_u, np.eye(1), None, None, GaussHermiteQuadrature(degree))
    out = problem_inputs("CartpoleKnown", model, T, Q, R, Q, 80.0, 0.0, mu_u, np.eye(1), None, None, (1, 0, 0), seed=0,
                         inference="gauss_hermite", gh_degree=degree)
    run_em(g, n_detail, n_total, out)
    save(f"gh{degree}_cartpole_T{T}", out)


def case_gh_double_cartpole(T=12, degree=3, n_detail=2, n_total=3):
    np.random.seed(0)
    mu_u = 1e-2 * np.random.randn(T, 1)
    sf = 1e-3
    Q = sf * np.diag([1.0, 1.0, 100.0, 1.0, 100.0, 10.0, 1.0, 1.0])
    R = sf * np.diag([0.1])
    model = make_env_model("DoubleCartpoleKnown", None)
    g = I2cGraph(model, T, Q, R, Q, 0.05, 0.99, mu_u, np.eye(1), None, None, GaussHermiteQuadrature(degree))
    out = problem_inputs("DoubleCartpoleKnown", model, T, Q, R, Q, 0.05, 0.99, mu_u, np.eye(1), None, None, (1, 0, 0), seed=0,
                         inference="gauss_hermite", gh_degree=degree)
    run_em(g, n_detail, n_total, out)
    save(f"gh{degree}_dcp_T{T}", out)


CASES = {"cartpole": case_gh_cartpole, "dcp": case_gh_double_cartpole}

if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
