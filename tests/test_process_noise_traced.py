"""A model written in Python with state-action-dependent process noise (TracedModel.process_noise_fn, tests/plugins/py_models_noise.py):
functor_codegen.py traces the function as a fifth one and emits the functor's optional `process_noise` member. The traced pendulum
against a hand-written header of the same math (tests/plugins/pendulum_input_noise_expanded.hpp) on one sweep pair, to 1e-12; what the
generator emits and refuses; and that a model WITHOUT the function emits the text it always did.
CPU: the host simulation; `-m gpu`: the hipcc build of build()."""
import os
import sys

import numpy as np
import pytest

import hostsim
import parity
from golden_util import assert_close
from noise_models import PendulumInputNoiseExpandedKnown, PendulumInputNoiseNumpy
from parity import np_
from test_process_noise import against_twin, engine, problem

pkg = parity.pkg
PLUGINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plugins")
if PLUGINS not in sys.path:
    sys.path.insert(0, PLUGINS)
import py_models  # noqa: E402
import py_models_noise  # noqa: E402


def _traced_equals_header(device, lanes):
    """1e-12 on everything a sweep pair computes, the gain included. The header is pendulum_input_noise_expanded.hpp: the same model
    written by hand in the order of operations the generator emits, so what is compared is trace -> emit -> build -> load -> solve
    against a hand-written functor of the same fp64 operations. Measured on the host simulation against headers in ANOTHER order of
    operations (lane / quad): pendulum_input_noise.hpp: messages and posterior 6e-14, K 8.0e-12 / 1.7e-11; the generator's dynamics
    with that header's hand-ordered process_noise: posterior 1.3e-14, K 5.7e-12 / 7.3e-12 -- cond(sig_xx) = 2.5e3 times the last bits
    of two roundings of the same Q; the traced and the in-tree pendulum WITHOUT the term: K 1.1e-11 / 2.4e-11. That the emitted member
    is the header's Q is held pointwise (test_emitted_member_and_host_side) and by both models against the twin (tests/test_process_noise.py)."""
    _, _, p = problem("pendulum", 5, 12)
    a, b = engine(py_models_noise.PyPendulumInputNoise(), p, device, group_lanes=lanes), engine(PendulumInputNoiseExpandedKnown(), p, device, group_lanes=lanes)
    assert a.model_id != b.model_id and a.has_process_noise and b.has_process_noise
    for e in (a, b):
        e.forward_backward()
    for k in parity.FWD:
        assert_close(np_(a.forward_messages()[k]), np_(b.forward_messages()[k]), 1e-12, f"traced vs header {k}")
    for x, y, what in zip(a.marginal_state_action() + a.local_linear_policy(), b.marginal_state_action() + b.local_linear_policy(),
                          ("mu_xu0_m", "sig_xu0_m", "K", "k", "sigK")):
        print(f"traced vs header {what}: {float(np.max(np.abs(np_(x) - np_(y))) / np.max(np.abs(np_(y)))):.2e}")
        assert_close(np_(x), np_(y), 1e-12, "traced vs header " + what)
    assert a.failures() == [] and b.failures() == []


@pytest.mark.parametrize("lanes", [0, pkg._native.LANES_QUAD], ids=["lane", "quad"])
def test_traced_equals_header_cpu(lanes):
    _traced_equals_header("cpu", lanes)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [0, pkg._native.LANES_QUAD], ids=["lane", "quad"])
def test_traced_equals_header_gpu(lanes):
    _traced_equals_header("cuda", lanes)


def test_expanded_header_against_twin_cpu():
    """the header the traced model is compared with is itself the model: against the NumPy twin, as the other two plugins are"""
    against_twin("cpu", "pendulum_expanded", 5, 12)


@pytest.mark.gpu
def test_expanded_header_against_twin_gpu():
    against_twin("cuda", "pendulum_expanded", 5, 12)


def test_emitted_member_and_host_side():
    m = py_models_noise.PyPendulumInputNoise()
    _, _, text, _ = m.header_text()
    assert text.count("I2C_FN void process_noise(const R* p, const R* x, const R* sn, const R* cs, R* q)") == 1
    assert all(f"q[{k}] =" in text for k in range(3)) and "q[3]" not in text  # sym(2) packed-lower entries from the full matrix
    assert "jacobian" in text and text.count("FN == 3") == 0                   # no Jacobian of it
    xu = np.random.default_rng(0).normal(size=(4, 7, 3))
    assert_close(m.process_noise(xu), PendulumInputNoiseNumpy().process_noise(xu), 1e-15, "host side of process_noise_fn")
    xn, cov = m.forward(xu.reshape(-1, 3))
    assert_close(cov, m.sig_eta + m.process_noise(xu.reshape(-1, 3)), 1e-15, "forward: one covariance per point")


def test_model_without_the_function_is_unchanged():
    m = py_models.PyPendulum()
    assert not m.has_process_noise and m.process_noise(np.zeros((3, 3))) is None
    assert "process_noise" not in m.header_text()[2]


def test_refusals_at_trace_time():
    class Branch(py_models_noise.PyPendulumInputNoise):
        def process_noise_fn(self, xu, p, m):
            return [1.0 if xu[2] > 0 else 0.0, 0.0, 1.0]

    class Count(py_models_noise.PyPendulumInputNoise):
        def process_noise_fn(self, xu, p, m):
            return [xu[2] * xu[2], 0.0]

    class Sqrt(py_models_noise.PyPendulumInputNoise):  # outside the basic operation set
        def process_noise_fn(self, xu, p, m):
            return [m.sqrt(xu[2] * xu[2] + 1.0), 0.0, 1.0]

    for cls in (Branch, Count, Sqrt):
        with pytest.raises((ValueError, AttributeError)):
            cls().header_text()
