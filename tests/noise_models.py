"""Models with STATE-ACTION-DEPENDENT process noise for the tests (tests/test_process_noise*.py): the NumPy twins of
tests/plugins/pendulum_input_noise.hpp and tests/plugins/cartpole_input_noise.hpp in the oracle's protocol, and the product-side plugin
objects (KnownModel with `process_noise` and the header of the device functor).

The covariance of one step from the point xu is  sig_eta + Q(xu):
  pendulum:  Q = sign (s2 u^2 b b^T + c om^2  e2 e2^T),  b = (0.05, 1),       s2 = 1e-2, c = 1e-3
  cartpole:  Q = sign (s2 u^2 b b^T + c thd^2 e3 e3^T),  b = (0, 0, 1, 0.5),  s2 = 1e-3, c = 1e-4
with the RAW action u (what the dynamics functor is handed). `sign` is the functor's one parameter: +1, or -1 on a trajectory whose
Q is to be indefinite (failure isolation)."""
import os

import numpy as np

from i2c.known_models import CartpoleKnown, PendulumKnown
from oracle.models_numpy import Cartpole, Pendulum

PLUGINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plugins")
PENDULUM_Q = dict(s2=1e-2, c=1e-3, b=(0.05, 1.0), k=1, iu=2)   # k: the state entry whose square scales e_k e_k^T; iu: the action's index
CARTPOLE_Q = dict(s2=1e-3, c=1e-4, b=(0.0, 0.0, 1.0, 0.5), k=3, iu=4)


def input_noise(xu, coef, sign=1.0):
    """Q(xu), (..., nx, nx), for xu (..., d); `sign` broadcasts against xu[..., 0]."""
    xu = np.asarray(xu, float)
    b = np.asarray(coef["b"], float)
    e = np.zeros(b.size)
    e[coef["k"]] = 1.0
    a = coef["s2"] * xu[..., coef["iu"]] ** 2
    v = coef["c"] * xu[..., coef["k"]] ** 2
    q = a[..., None, None] * np.outer(b, b) + v[..., None, None] * np.outer(e, e)
    return np.asarray(sign, float)[..., None, None] * q


class _NoiseTwin:
    """sign: a scalar, or (B,) for a batch of points (B, P, d) -- one value per trajectory"""

    sign = 1.0

    def process_noise(self, xu):
        s = np.asarray(self.sign, float)
        return input_noise(xu, self.COEF, s.reshape(s.shape + (1,) * (np.ndim(xu) - 1 - s.ndim)))


class PendulumInputNoiseNumpy(_NoiseTwin, Pendulum):
    name = "PendulumInputNoise"
    COEF = PENDULUM_Q


class CartpoleInputNoiseNumpy(_NoiseTwin, Cartpole):
    name = "CartpoleInputNoise"
    COEF = CARTPOLE_Q


class _NoisePlugin:
    model_id = None  # (not the in-tree model's: the functor comes from the header)

    def device_params(self):
        return [1.0]

    def process_noise(self, xu):
        return input_noise(xu, self.COEF)


class PendulumInputNoiseKnown(_NoisePlugin, PendulumKnown):
    name = "PendulumInputNoise"
    model_name = "PendulumInputNoiseKnown"
    hip_header = os.path.join(PLUGINS, "pendulum_input_noise.hpp")
    COEF = PENDULUM_Q


class PendulumInputNoiseExpandedKnown(PendulumInputNoiseKnown):
    """the same model with its dynamics written out in the code generator's arithmetic (the header says why)"""

    model_name = "PendulumInputNoiseExpandedKnown"
    hip_header = os.path.join(PLUGINS, "pendulum_input_noise_expanded.hpp")


class CartpoleInputNoiseKnown(_NoisePlugin, CartpoleKnown):
    name = "CartpoleInputNoise"
    model_name = "CartpoleInputNoiseKnown"
    hip_header = os.path.join(PLUGINS, "cartpole_input_noise.hpp")
    COEF = CARTPOLE_Q


MODELS = {"pendulum": (PendulumInputNoiseKnown, PendulumInputNoiseNumpy), "cartpole": (CartpoleInputNoiseKnown, CartpoleInputNoiseNumpy),
          "pendulum_expanded": (PendulumInputNoiseExpandedKnown, PendulumInputNoiseNumpy)}
