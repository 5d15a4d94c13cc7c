"""Models written in Python (i2c.traced_model.TracedModel) for tests/test_functor_codegen.py and tests/test_traced_model.py:
the math of three in-tree models and of the header plugin van_der_pol.hpp, stated once as functions of scalars."""
import numpy as np

from i2c.traced_model import TracedModel

_INF = np.inf


class PyPendulum(TracedModel):
    """PendulumKnown (i2c/known_models.py; struct Pendulum, csrc/i2c_models.hpp)."""

    name = "Pendulum"
    dim_x, dim_u, dim_z, dim_z_term = 2, 1, 4, 3

    def __init__(self, **kw):
        super().__init__(**kw)
        self.x0 = np.array([[np.pi], [0.0]])
        self.xag = np.array([[0.0], [1.0], [0.0]])
        self.xag_term = np.array([[0.0], [1.0], [0.0]])
        self.sig_x0 = 1e-5 * np.eye(2)
        self.sig_eta = np.diag([1e-5, 1e-5])
        self.xu_lim = np.array([[-_INF, -_INF, -2.0], [_INF, _INF, 2.0]])

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


MU, DT, U_MAX = 1.5, 0.05, 3.0


class PyVanDerPol(TracedModel):
    """tests/plugins/van_der_pol.hpp: params = {mu, dt, u_max}, one observation that is not a pass-through."""

    name = "VanDerPol"
    dim_x, dim_u, dim_z, dim_z_term = 2, 1, 4, 2

    def __init__(self, **kw):
        super().__init__(**kw)
        self.x0 = np.array([[1.0], [0.0]])
        self.xag = np.zeros((3, 1))
        self.xag_term = np.zeros((2, 1))
        self.sig_x0 = 1e-4 * np.eye(2)
        self.sig_eta = 1e-5 * np.eye(2)
        self.xu_lim = np.array([[-_INF, -_INF, -U_MAX], [_INF, _INF, U_MAX]])

    def device_params(self):
        return [MU, DT, U_MAX]

    def dynamics_fn(self, xu, p, m):
        mu, dt, u_max = p
        u = m.clip(xu[2], -u_max, u_max)
        v = xu[1] + dt * (mu * (1.0 - xu[0] ** 2) * xu[1] - xu[0] + u)
        return [xu[0] + dt * v, v]

    def observe_fn(self, xu, p, m):
        return [xu[0], xu[1], xu[1] / (1.0 + xu[1] ** 2), xu[2]]

    def observe_terminal_fn(self, x, p, m):
        return [x[0], x[1]]


class PyCartpole(TracedModel):
    """CartpoleKnown (struct Cartpole)."""

    name = "Cartpole"
    dim_x, dim_u, dim_z, dim_z_term = 4, 1, 6, 5
    g = 9.81  # (a class attribute a test changes to get "the same model with another constant")

    def __init__(self, **kw):
        super().__init__(**kw)
        self.x0 = np.array([[0.0], [np.pi], [0.0], [0.0]])
        self.xag = np.array([[0.0], [0.0], [1.0], [0.0], [0.0]])
        self.sig_x0 = 1e-5 * np.eye(4)
        self.sig_eta = 1e-8 * np.eye(4)
        self.xu_lim = np.array([[-_INF] * 4 + [-5.0], [_INF] * 4 + [5.0]])

    def dynamics_fn(self, xu, p, m):
        g, m_p, ln, dt = self.g, 0.127, 0.3365, 1.0 / 250.0
        m_t = 0.37 + m_p
        u = m.clip(xu[4], -5.0, 5.0)
        s, c, w2 = m.sin(xu[1]), m.cos(xu[1]), xu[3] ** 2
        th_acc = (-m_p * ln * s * c * w2 + m_t * g * s - u * c) / (ln * (4.0 / 3.0 * m_t - m_p * c ** 2))
        x_acc = (m_p * ln * s * w2 - m_p * ln * th_acc * c + u) / m_t
        return [xu[0] + dt * xu[2], xu[1] + dt * xu[3], xu[2] + dt * x_acc, xu[3] + dt * th_acc]

    def observe_fn(self, xu, p, m):
        return [xu[0], m.sin(xu[1]), m.cos(xu[1]), xu[2], xu[3], xu[4]]

    def observe_terminal_fn(self, x, p, m):
        return [x[0], m.sin(x[1]), m.cos(x[1]), x[2], x[3]]


class PyDoubleCartpole(TracedModel):
    """DoubleCartpoleKnown (struct DoubleCartpole): the 3 x 3 solve written out through the adjugate, sin / cos of the angle
    difference as such (the emitter expands them by angle addition)."""

    name = "Double Cartpole"
    dim_x, dim_u, dim_z, dim_z_term = 6, 1, 9, 8

    def __init__(self, **kw):
        super().__init__(**kw)
        self.x0 = np.array([[0.0], [np.pi], [np.pi], [0.0], [0.0], [0.0]])
        self.xag = np.array([[0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]]).T
        self.sig_x0 = 1e-6 * np.eye(6)
        self.sig_eta = 1e-6 * np.eye(6)
        self.xu_lim = np.array([[-_INF] * 6 + [-10.0], [_INF] * 6 + [10.0]])

    def dynamics_fn(self, xu, p, m):
        dt, g, m1, m2, L1 = 1 / 125, 9.81, 0.127, 0.127, 0.3365
        l1 = l2 = L1 / 2
        m_t = 0.37 + m1 + m2
        h1, h2, h3 = m1 * l1 + m2 * L1, m2 * l2, L1 * l2 * m2
        s1, c1, s2, c2 = m.sin(xu[1]), m.cos(xu[1]), m.sin(xu[2]), m.cos(xu[2])
        sd, cd = m.sin(xu[1] - xu[2]), m.cos(xu[1] - xu[2])
        M00, M01, M02 = m_t, h1 * c1, h2 * c2
        M11, M12 = l1 ** 2 * m1 + L1 ** 2 * m2 + m1 * L1 / 12, h3 * cd
        M22 = l2 ** 2 * m2 + m2 * L1 / 12
        w1, w2 = xu[4], xu[5]
        r0 = 3.0 * m.clip(xu[6], -10.0, 10.0) + h1 * w1 * w1 * s1 + h2 * w2 * w2 * s2
        r1 = -h3 * w2 * w2 * sd + h1 * g * s1
        r2 = h3 * w1 * w1 * sd + h2 * g * s2
        A00, A01, A02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
        A11, A12, A22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
        idet = m.rcp(M00 * A00 + M01 * A01 + M02 * A02)
        acc = [(A00 * r0 + A01 * r1 + A02 * r2) * idet, (A01 * r0 + A11 * r1 + A12 * r2) * idet,
               (A02 * r0 + A12 * r1 + A22 * r2) * idet]
        vel = [xu[3 + i] + dt * acc[i] for i in range(3)]
        return [xu[i] + dt * vel[i] for i in range(3)] + vel

    def observe_fn(self, xu, p, m):
        return [xu[0], m.sin(xu[1]), m.cos(xu[1]), m.sin(xu[2]), m.cos(xu[2]), xu[3], xu[4], xu[5], xu[6]]

    def observe_terminal_fn(self, x, p, m):
        return [x[0], m.sin(x[1]), m.cos(x[1]), m.sin(x[2]), m.cos(x[2]), x[3], x[4], x[5]]


# what __graft_entry__.build() compiles for gfx950, so that no GPU test compiles: the three models, and each once more without
# the emitted Jacobian (the A/B of Linearize() in tests/test_traced_model.py)
BUILT = tuple((cls, kw) for cls in (PyPendulum, PyVanDerPol, PyCartpole) for kw in ({}, {"jacobian": False}))
