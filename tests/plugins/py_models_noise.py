"""A model written in Python (i2c.traced_model.TracedModel) with STATE-ACTION-DEPENDENT process noise, for
tests/test_process_noise_traced.py: the pendulum of tests/plugins/pendulum_input_noise.hpp stated once as functions of scalars --
the in-tree pendulum's three functions and `process_noise_fn`, which functor_codegen.py traces as a fifth function and emits as the
functor's optional `process_noise` member."""
import numpy as np

from i2c.traced_model import TracedModel

_INF = np.inf
S2, C, B0 = 1e-2, 1e-3, 0.05


class PyPendulumInputNoise(TracedModel):
    """Q(xu) = sign (s2 u^2 b b^T + c om^2 e2 e2^T), b = (0.05, 1); params = {sign}"""

    name = "PendulumInputNoise"
    dim_x, dim_u, dim_z, dim_z_term = 2, 1, 4, 3

    def __init__(self, **kw):
        super().__init__(**kw)
        self.x0 = np.array([[np.pi], [0.0]])
        self.xag = np.array([[0.0], [1.0], [0.0]])
        self.xag_term = np.array([[0.0], [1.0], [0.0]])
        self.sig_x0 = 1e-5 * np.eye(2)
        self.sig_eta = np.diag([1e-5, 1e-5])
        self.xu_lim = np.array([[-_INF, -_INF, -2.0], [_INF, _INF, 2.0]])

    def device_params(self):
        return [1.0]

    def dynamics_fn(self, xu, p, m):
        th, om = xu[0], xu[1]
        torque = m.clip(xu[2], -2.0, 2.0)
        acc = (-3.0 * 9.80665 / 2.0) * m.sin(th + m.pi) - 1e-2 * om + 3.0 * torque
        om2 = om + 0.05 * acc
        return [th + 0.05 * om2, om2]

    def observe_fn(self, xu, p, m):
        return [m.sin(xu[0]), m.cos(xu[0]), xu[1], xu[2]]

    def observe_terminal_fn(self, x, p, m):
        return [m.sin(x[0]), m.cos(x[0]), x[1]]

    def process_noise_fn(self, xu, p, m):  # the full matrix, as rows: its lower triangle is packed
        a = p[0] * S2 * xu[2] * xu[2]
        return [[a * (B0 * B0), a * B0], [a * B0, a + p[0] * C * xu[1] * xu[1]]]


BUILT = ((PyPendulumInputNoise, {}),)
