"""The stand-in for `autograd.jacobian` that produced the Linearize goldens (oracle/ref_shim._central_difference_jacobian:
autograd is not installed in the build container) pinned by something OTHER than itself (round-5 review, weak #1a / item 7):

* pendulum (reference i2c/env_autograd.py:5-19): the hand-derived closed-form Jacobian, inside and outside the action clip;
* double cartpole (reference i2c/env_autograd.py:60-167): an independent scheme -- central differences at two step sizes with
  Richardson extrapolation (error O(h^4)) -- which shares no code with the complex-step stand-in.

Both to <= 1e-9 of the Jacobian's largest entry. The functions differentiated are the REFERENCE's own -- replayed from their
recorded calls (tests/golden/reference_dynamics_calls.npz, oracle/gen_reference_dynamics_golden.py) and, where the reference checkout
is present, live as well (imported in a child process through the shim: this process has the build's package under the name
`i2c`) -- and the oracle's NumPy twins (oracle/models_numpy.py, pinned to the reference by tests/golden/models_vectors.npz)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import models_numpy, ref_shim  # noqa: E402

PEND_XU = np.array([[0.7, -0.3, 0.4], [np.pi, 0.0, -1.5], [-2.1, 3.0, 2.5], [0.05, -4.0, -2.000001]])  # (the last two: outside the clip)
DCP_XU = np.array([[0.1, 0.3, -0.2, 0.5, -0.4, 0.2, 1.5], [-0.5, np.pi, np.pi, 0.0, 0.0, 0.0, 0.0], [0.3, 2.0, -1.0, -1.0, 2.0, -3.0, -4.0]])


def pendulum_jacobian_closed_form(xu):
    """d [x_pos, x_dot] / d [th, thd, u] of env_autograd.py:5-19, by hand."""
    dt, m, l, d, g, u_mx = 0.05, 1.0, 1.0, 1e-2, 9.80665, 2.0
    out = np.zeros((xu.shape[0], 2, 3))
    for p, (th, _thd, u) in enumerate(xu):
        a_th = -3.0 * g / (2 * l) * np.cos(th + np.pi)
        a_thd = -d
        a_u = 3.0 / (m * l ** 2) * (1.0 if abs(u) < u_mx else 0.0)
        xd = np.array([dt * a_th, 1.0 + dt * a_thd, dt * a_u])  # x_dot = thd + a dt
        out[p, 1] = xd
        out[p, 0] = np.array([1.0, 0.0, 0.0]) + dt * xd  # x_pos = th + x_dot dt
    return out


def richardson_jacobian(f, xu, h=2e-3):
    """(4 D(h/2) - D(h)) / 3 with D the central difference: O(h^4), no complex arithmetic."""
    def central(step):
        out = np.zeros((xu.shape[0], f(xu).shape[1], xu.shape[1]))
        for j in range(xu.shape[1]):
            e = np.zeros(xu.shape[1])
            e[j] = step
            out[:, :, j] = (f(xu + e) - f(xu - e)) / (2 * step)
        return out

    return (4.0 * central(h / 2) - central(h)) / 3.0


def standin_rows(f, xu):
    """The stand-in differentiates a (P, d) -> (P, n) map into (P, n, P, d); the per-point blocks are its diagonal."""
    jac = ref_shim._central_difference_jacobian(f, 0)(xu)
    assert jac.shape == (xu.shape[0], f(xu).shape[1], xu.shape[0], xu.shape[1])
    off = jac.copy()
    for p in range(xu.shape[0]):
        off[p, :, p, :] = 0.0
    assert np.all(off == 0.0), "rows of a batched dynamics function are independent"
    return np.stack([jac[p, :, p, :] for p in range(xu.shape[0])])


def check(f_pend, f_dcp, what):
    jp = standin_rows(f_pend, PEND_XU)
    ref = pendulum_jacobian_closed_form(PEND_XU)
    assert np.max(np.abs(jp - ref)) <= 1e-12 * np.max(np.abs(ref)), f"{what}: pendulum vs closed form {np.max(np.abs(jp - ref)):.2e}"
    assert jp[2, 1, 2] == 0.0 and jp[3, 0, 2] == 0.0, "outside the clip the action has no effect (autograd's clip rule)"
    jd = standin_rows(f_dcp, DCP_XU)
    rd = richardson_jacobian(f_dcp, DCP_XU)
    err = np.max(np.abs(jd - rd)) / np.max(np.abs(rd))
    assert err <= 1e-9, f"{what}: double cartpole vs Richardson-extrapolated differences {err:.2e}"
    return err


def test_standin_on_the_oracle_twins():
    pend, dcp = models_numpy.make_model("PendulumKnown"), models_numpy.make_model("DoubleCartpoleKnown")
    check(pend.dynamics, dcp.dynamics, "oracle twins")


_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from oracle import ref_shim
ref_shim.install()
import numpy as np
import test_jacobian_standin as t
from i2c import env_autograd as ref  # the REFERENCE's module (ref_shim put /root/reference first on sys.path)
assert ref.__file__.startswith(ref_shim.REFERENCE_ROOT), ref.__file__
err = t.check(ref.pendulum_dynamics, ref.double_cartpole_dynamics, "reference")
# and what the reference itself calls at run time: the module-level Jacobians built from the stand-in at import
jp = ref.pendulum_dydxu(t.PEND_XU)
assert np.max(np.abs(np.stack([jp[p, :, p, :] for p in range(4)]) - t.pendulum_jacobian_closed_form(t.PEND_XU))) <= 1e-12 * 2
print(json.dumps({{"dcp_err": err}}))
"""


class Replay:
    """One of the reference's dynamics functions replayed from its recorded calls (input -> output, matched exactly on the input,
    complex-step inputs included). A miss raises -- and is counted, since the stand-in treats any exception of a complex call as
    "not complex-safe"."""

    def __init__(self, z, tag):
        self.calls = [(z[f"{tag}_x{i}"], z[f"{tag}_y{i}"]) for i in range(int(z[tag + "_n"]))]
        self.misses = 0

    def __call__(self, x):
        x = np.asarray(x)
        for xi, yi in self.calls:
            if xi.dtype == x.dtype and xi.shape == x.shape and np.array_equal(xi, x):
                return yi.copy()
        self.misses += 1
        raise KeyError("no recorded call of the reference with this input")


def test_standin_on_the_reference_dynamics():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_dynamics_calls.npz"))
    pend, dcp = Replay(z, "pendulum"), Replay(z, "double_cartpole")
    assert check(pend, dcp, "reference (recorded)") <= 1e-9
    assert pend.misses == 0 and dcp.misses == 0, "the stand-in asked the recorded reference for a call it never made"
    # what the reference itself calls at run time: the module-level Jacobians built from the stand-in at import
    jp = z["pendulum_dydxu"]
    assert np.max(np.abs(np.stack([jp[p, :, p, :] for p in range(4)]) - pendulum_jacobian_closed_form(PEND_XU))) <= 1e-12 * 2
    if not ref_shim.reference_available():
        return
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["dcp_err"] <= 1e-9
