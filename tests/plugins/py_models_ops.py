"""Models written in Python with `operations = "extended"` (i2c.traced_model.TracedModel) for tests/test_functor_codegen_ops.py
and tests/test_traced_model_ops.py: sqrt, tanh, log, the selects and a sine the functor takes itself. Both are CONTINUOUS across
every kink: a sigma point within rounding of one moves no result by more than rounding."""
import numpy as np

from i2c.traced_model import TracedModel

_INF = np.inf


class PyDragPendulum(TracedModel):
    """A pendulum on a slope with a saturating motor, air drag and smooth Coulomb friction; complex-analytic operations only
    (the Linearize oracle differentiates the host side by complex step). params = {slope, dt, u_max}."""

    name = "DragPendulum"
    operations = "extended"
    dim_x, dim_u, dim_z, dim_z_term = 2, 1, 4, 2
    SLOPE, DT, U_MAX = 0.15, 0.05, 2.0
    DRAG, EPS, MU, K = 0.05, 1e-2, 0.1, 4.0

    def __init__(self, **kw):
        super().__init__(**kw)
        self.x0 = np.array([[np.pi], [0.0]])
        self.xag = np.array([[0.0], [1.0], [0.0]])
        self.xag_term = np.zeros((2, 1))
        self.sig_x0 = 1e-5 * np.eye(2)
        self.sig_eta = np.diag([1e-5, 1e-5])
        self.xu_lim = np.array([[-_INF, -_INF, -3.0], [_INF, _INF, 3.0]])

    def device_params(self):
        return [self.SLOPE, self.DT, self.U_MAX]

    def dynamics_fn(self, xu, p, m):
        slope, dt, u_max = p
        th, om = xu[0], xu[1]
        torque = u_max * m.tanh(xu[2] / u_max)                          # smooth actuator saturation
        drag = -self.DRAG * om * m.sqrt(om * om + self.EPS ** 2)        # ~ -c |om| om
        friction = -self.MU * m.tanh(self.K * om)                       # smooth Coulomb friction
        gravity = (3.0 * 9.80665 / 2.0) * m.sin(th - slope)             # a general sine: the slope is a device parameter
        om2 = om + dt * (gravity + drag + friction + 3.0 * torque)
        return [th + dt * om2, om2]

    def observe_fn(self, xu, p, m):
        return [m.sin(xu[0]), m.cos(xu[0]), m.log(1.0 + xu[1] * xu[1]), xu[2]]  # (theta: an angle coordinate, handed in)

    def observe_terminal_fn(self, x, p, m):
        return [x[0], x[1]]


class PyHovercraft(TracedModel):
    """A planar hovercraft: quadratic drag -c |v| v, a thrust limit per axis, more drag forwards than backwards (continuous:
    both branches vanish at vx = 0) and a keel term in |vy| (continuous likewise). Identity observation of (x, u)."""

    name = "Hovercraft"
    operations = "extended"
    dim_x, dim_u, dim_z, dim_z_term = 4, 2, 6, 4
    DT, U_MAX, DRAG, EPS, FWD, BACK, KEEL = 0.05, 1.5, 0.3, 1e-2, 0.2, 0.5, 0.1

    def __init__(self, **kw):
        super().__init__(**kw)
        self.x0 = np.array([[1.0], [-0.5], [0.0], [0.0]])
        self.xag = np.zeros((4, 1))
        self.xag_term = np.zeros((4, 1))
        self.sig_x0 = 1e-4 * np.eye(4)
        self.sig_eta = 1e-5 * np.eye(4)
        self.xu_lim = np.array([[-_INF] * 4 + [-self.U_MAX] * 2, [_INF] * 4 + [self.U_MAX] * 2])

    def dynamics_fn(self, xu, p, m):
        px, py, vx, vy = xu[:4]
        dt, u_max = self.DT, self.U_MAX
        ux = m.minimum(m.maximum(xu[4], -u_max), u_max)
        uy = m.minimum(m.maximum(xu[5], -u_max), u_max)
        speed = m.sqrt(vx * vx + vy * vy + self.EPS ** 2)
        ax = ux - self.DRAG * speed * vx - m.where_gt(vx, 0.0, self.FWD * vx, self.BACK * vx)
        ay = uy - self.DRAG * speed * vy - self.KEEL * abs(vy) * vx
        vx2, vy2 = vx + dt * ax, vy + dt * ay
        return [px + dt * vx2, py + dt * vy2, vx2, vy2]

    def observe_fn(self, xu, p, m):
        return list(xu)

    def observe_terminal_fn(self, x, p, m):
        return list(x)


# what __graft_entry__.build() compiles for gfx950 next to py_models.BUILT: both models, each with and without the emitted Jacobian
BUILT = tuple((cls, kw) for cls in (PyDragPendulum, PyHovercraft) for kw in ({}, {"jacobian": False}))
