"""i2c model-predictive controllers with the reference's class names and call protocol
(reference i2c/policy/mpc.py:16-182), batched: one policy drives B closed loops at once.

Every step of the loop is device work: the cubature Kalman filter (`i2c_ckf_filter`), `n_iter`
forward/backward sweeps warm-started from the shifted posterior, and the receding-horizon shift
(the reference's `cells.pop(0); cells.append(deepcopy(cell_init))` list surgery becomes a roll of
the [T][E][B] buffers plus a fresh last row). With B == 1 shapes are the reference's
((n, 1) columns); with B > 1 arrays carry a leading batch axis.

The policies ask the engine (BatchedI2c); they do not write its tensors. What they keep of its results on the host is kept
together with the engine's revision it was read at.
"""
import numpy as np
import torch

from .. import core

unpack_sym = core.engine.unpack_sym


def _np(t):
    if isinstance(t, np.ndarray):
        return np.array(t, dtype=np.float64)
    return np.array(t.detach().to(torch.float64).cpu().numpy(), copy=True)  # never alias a device/host buffer


def unpack(e):
    return unpack_sym(e.sig_x0.T, e.nx)


def _action(mean, cov_packed, n, deterministic):
    """The action to apply, (B, nu): the mean, or one np.random.multivariate_normal draw per trajectory, in order. mean: (B, nu)
    tensor or array; cov_packed: (B, sym n) packed covariance of a vector whose LAST nu components are the action (n = nu: the
    action's own; n = nx + nu: cell 0's joint) -- touched only when sampling."""
    mean = _np(mean)
    if deterministic:
        return mean
    lo = n - mean.shape[1]
    cov = _np(unpack_sym(torch.as_tensor(cov_packed), n)[:, lo:, lo:])
    return np.stack([np.random.multivariate_normal(m, s) for m, s in zip(mean, cov)])


class _LazyList(list):
    """A history list whose entries may be zero-argument callables -- device-side snapshots taken inside the control loop -- that are
    replaced by their host value when first READ: the single closed loop (the reference's shape) keeps the reference's histories
    (mus, covars, xu_history, z_history: mpc.py:165-170, plots) without a device -> host copy per entry and step."""

    def _at(self, k):
        v = list.__getitem__(self, k)
        if callable(v):
            v = v()
            list.__setitem__(self, k, v)
        return v

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._at(k) for k in range(*i.indices(len(self)))]
        return self._at(i if i >= 0 else len(self) + i)

    def __iter__(self):
        return (self._at(k) for k in range(len(self)))


class MpcPolicy:
    """Fully observed MPC (reference mpc.py:16-111). NB the reference's own __call__ is broken
    (it passes unknown kwargs to compute_update_alpha); this one runs."""

    def plot_history(self, res_path, name=""):
        """Figures are presentation, not part of the solver (I2cGraph._no_plot): the planned trajectories stay in xu_history."""
        return None

    def __init__(self, i2c, n_iter, sig_u, z_traj=None):
        self.i2c = i2c
        self.engine = e = i2c.engine
        self.B = e.B
        self.dim_u, self.dim_x = e.nu, e.nx
        self.sig_u = sig_u
        self.model = i2c.sys
        self.n_iter = n_iter
        self.set_control(True)  # mpc.py:21-22
        e.enable_per_cell_alpha()  # cell_init is copied NOW (mpc.py:26): appended cells carry today's sig_xi ...
        e.renew_cell_init()  # ... and today's cells[0] (deepcopy(i2c.cells[0]), mpc.py:26), not the constructor's
        self.z_traj = None if z_traj is None else np.asarray(z_traj, dtype=float)
        if self.z_traj is not None:
            zt = self.z_traj if self.z_traj.ndim == 3 else self.z_traj[None]
            e.set_targets(zt[:, : e.H])
        self._initial = e.snapshot()
        self.record_history = self.B == 1
        self.xu_history, self.z_history = _LazyList(), _LazyList()

    def set_control(self, feedforward):
        """mpc.py:35-41: feed-forward keeps every cell's action prior independent of the state."""
        e = self.engine
        if feedforward:
            e.tau = 0
        else:
            e.tau = e.H

    def reset(self):
        """Back to the solver state at construction (BatchedI2c.restore): posterior, temperatures, feed-forward flags, belief,
        targets, the ring and cleared status words; the plan histories start afresh. NOT restored: the engine's `temp` and
        `cell_init` and its metric histories."""
        self.engine.restore(self._initial)
        self.xu_history, self.z_history = _LazyList(), _LazyList()

    def _squeeze(self, a, column=False):
        if self.B == 1:
            a = a[0]
            return a.reshape(-1, 1) if column else a
        return a

    def _next_target(self, i):
        """Target of the cell that enters the horizon at step i (mpc.py:73-77, 177-181)."""
        if self.z_traj is None:
            return None
        e = self.engine
        zt = self.z_traj if self.z_traj.ndim == 3 else self.z_traj[None]
        if i + e.H < zt.shape[1]:
            z = np.broadcast_to(zt[:, i + e.H], (self.B, e.nz))
            return torch.as_tensor(np.array(z.T, order="C"), dtype=e.dtype, device=e.device)
        return None  # keep the previous last cell's target

    def _sweeps(self, n_iter):
        e = self.engine
        for _ in range(n_iter):
            e.forward_backward()
            e.update_priors()

    def _plan(self, n_iter):
        self._sweeps(n_iter)
        if self.B == 1:
            self.engine.raise_on_failure()

    def _first_action(self, deterministic):
        """cells[0].mu_u0_m (and sig_u0_m when sampling): only cell 0 of the posterior buffer is read back."""
        e = self.engine
        d, cell0 = e.d, e.post[e.t0]  # row t0 of the ring is cell 0
        return _action(cell0[e.nx: d].T, cell0[d: d + d * (d + 1) // 2].T, d, deterministic)

    def _copy_plan(self):
        """This step's plan as the (xu_history, z_history) entries it will be (mpc.py:165-170): device-side copies now, host arrays
        when read (_LazyList). None when no history is kept."""
        if not self.record_history:
            return None
        e = self.engine
        mu = e._rows(e.post, 0, e.d).clone()  # (B, T, d) in cell order (a copy: the ring row of cell 0 is about to be reused)
        xu = lambda: (lambda m: m[0][:, :, None] if self.B == 1 else m)(_np(mu))  # noqa: E731
        if e.zpost is None:
            return xu, None
        mz = e._rows(e.zpost, 0, e.nz).clone()
        return xu, lambda: (lambda m: m[0] if self.B == 1 else m)(_np(mz))

    def _record(self, plan):
        """Append a step's _copy_plan() to xu_history / z_history: only once the step's status has been checked."""
        if plan is not None:
            self.xu_history.append(plan[0])
            self.z_history.append(plan[1])

    def optimize(self, n_iter, x):
        x = np.asarray(x, dtype=float)
        assert x.reshape(-1, self.dim_x).shape[0] in (1, self.B), f"{x.shape}, {(self.dim_x, 1)}"
        e = self.engine
        e.set_initial_state(x.reshape(-1, self.dim_x), _np(unpack(e)))
        if self.B == 1:
            self.i2c.sys.x0 = x.reshape(self.dim_x, 1)
            self.i2c._x0_seen = None
        self._plan(n_iter)

    def __call__(self, i, x, deterministic=True):
        if not self.record_history:  # batched closed loops: the whole control step is one library call
            x = np.asarray(x, dtype=float)
            e = self.engine
            e.set_initial_state(x.reshape(-1, self.dim_x), _np(unpack(e)))
            mu_u, sig_u = e.mpc_step(self.n_iter, z_new=self._next_target(i))
            return self._squeeze(_action(mu_u, sig_u, self.dim_u, deterministic), column=True)
        self.optimize(self.n_iter, x)
        self._record(self._copy_plan())
        u = self._first_action(deterministic)
        self.engine.shift_horizon(self._next_target(i))
        return self._squeeze(u, column=True)

    def update_models(self, sys):
        raise NotImplementedError("models are compiled device functors; construct a new I2cGraph")


class _Staging:
    """The per-step host <-> device traffic of the partially observed loop goes through page-locked buffers: the measurement and
    the applied action go up in ONE copy, the first planned action (batched loop) or cell 0 with the belief and the status words
    (single loop) come down into them. (A pageable numpy array costs a staging copy and a synchronisation per transfer: three of
    them were a sixth of a planar-quadrotor control step at B = 1024.)"""

    def __init__(self, e):
        B, d, nx, nu, self.ny = e.B, e.d, e.nx, e.nu, e.dims.ny
        host = lambda *shape, dtype=e.dtype: torch.empty(*shape, dtype=dtype, pin_memory=e.device.type == "cuda")  # noqa: E731
        self.yu_host = host(self.ny + nu, B)
        self.yu_np = self.yu_host.numpy()
        self.yu_dev = torch.empty(self.ny + nu, B, dtype=e.dtype, device=e.device)
        self.action = host(nu, B)
        self.mu, self.cov, self.cell0 = host(nx, B), host(nx * (nx + 1) // 2, B), host(d + d * (d + 1) // 2, B)
        self.status = host(B, dtype=torch.int32)

    def upload(self, y, u):
        """y (ny, 1) or (B, ny), u (nu, 1) or (B, nu) -> their [ny][B] / [nu][B] device rows."""
        ny, (n, B) = self.ny, self.yu_np.shape
        self.yu_np[:ny] = np.broadcast_to(np.asarray(y, dtype=float).reshape(-1, ny), (B, ny)).T
        self.yu_np[ny:] = np.broadcast_to(np.asarray(u, dtype=float).reshape(-1, n - ny), (B, n - ny)).T
        self.yu_dev.copy_(self.yu_host, non_blocking=True)  # (the staging buffer is reused only after this step's action has come back)
        return self.yu_dev[:ny], self.yu_dev[ny:]


class PartiallyObservedMpcPolicy(MpcPolicy):
    """MPC on a cubature-Kalman-filtered belief (reference mpc.py:113-182)."""

    def __init__(self, i2c, n_iter, sig_u, z_traj=None):
        super().__init__(i2c, n_iter, sig_u, z_traj)
        # the belief lives in the solver's x0 / sig_x0 tensors: filter() updates them in place and the
        # next forward sweep starts from them, with no host round trip
        self.mus, self.covars = _LazyList(), _LazyList()
        self._belief_host = None  # (engine.belief_revision, mu, covar): host arrays of the belief as it was at that revision
        self._pinned = _Staging(self.engine)

    # -- belief as reference-shaped arrays ----------------------------------------------------
    def _belief(self):
        e = self.engine
        if self._belief_host is None or self._belief_host[0] != e.belief_revision:
            self._belief_host = (e.belief_revision, self._squeeze(_np(e.x0.T), column=True), self._squeeze(_np(unpack(e))))
        return self._belief_host

    @property
    def mu(self):
        return np.array(self._belief()[1], copy=True)

    @property
    def covar(self):
        return np.array(self._belief()[2], copy=True)

    def _dev(self, a, n):
        e = self.engine
        a = np.broadcast_to(np.asarray(a, dtype=float).reshape(-1, n), (self.B, n))
        return torch.as_tensor(np.array(a.T, order="C"), dtype=e.dtype, device=e.device)

    def _write_back_belief(self):
        """The single closed loop keeps the facade's sys.x0 / sys.sig_x0 the engine's belief (mpc.py:149-150), and tells the facade
        that it has seen them: nothing is uploaded again."""
        if self.B == 1:
            g = self.i2c
            g.sys.x0, g.sys.sig_x0 = self.mu, self.covar
            g._x0_seen = g._x0_key()

    def _measurement_noise(self):
        sig_zeta = self.i2c.sys.sig_zeta
        if sig_zeta is None:
            raise ValueError("sys.sig_zeta (measurement noise) must be set before filtering")
        return sig_zeta

    def filter(self, y, u):
        """mpc.py:125-145. y: (dim_y, 1) or (B, dim_y); u: (dim_u, 1) or (B, dim_u)."""
        e = self.engine
        e.ckf_filter(self._dev(y, e.dims.ny), self._dev(u, e.nu), self._measurement_noise())
        if self.B == 1:
            e.raise_on_failure()
        return self.mu, self.covar

    def optimize(self, n_iter, mu=None, covar=None):
        """mpc.py:147-154. With no arguments the current (filtered) belief is used as is."""
        if mu is not None:
            mu = np.asarray(mu, dtype=float)
            assert mu.reshape(-1, self.dim_x).shape[0] in (1, self.B), f"{mu.shape}, {(self.dim_x, 1)}"
            self.engine.set_initial_state(mu.reshape(-1, self.dim_x), covar)
        self._write_back_belief()
        self._plan(n_iter)

    def __call__(self, i, y, u, deterministic=True):
        if self.record_history:
            return self._single_loop_step(i, y, u, deterministic)
        e = self.engine  # batched closed loops: filter + plan + first action + shift in one library call
        if i > 0:
            sig_zeta = self._measurement_noise()
            mu_u, sig_u = e.mpc_step(self.n_iter, *self._pinned.upload(y, u), sig_zeta, z_new=self._next_target(i))
        else:
            mu_u, sig_u = e.mpc_step(self.n_iter, z_new=self._next_target(i))
        if deterministic:  # the mean alone, through the page-locked buffer
            self._pinned.action.copy_(e._mpc_action[: e.nu])  # (contiguous rows; blocks until the step has run)
            mu_u = self._pinned.action.numpy().T
        return self._squeeze(_action(mu_u, sig_u, self.dim_u, deterministic), column=True)

    def _single_loop_step(self, i, y, u, deterministic):
        """One closed loop (B = 1, the reference's shape; mpc.py:156-182): filter, plan, first action, record, shift -- the same
        library calls as the separate methods, enqueued without a host round trip in between and settled by ONE synchronisation:
        the failure status (the reference raises inside the step), the first action and the filtered belief come back together
        through page-locked buffers; the histories keep device-side snapshots until they are read (_LazyList), and take this
        step's only once its status has been checked: a step that raises leaves the four of them the same length. (Round 6: the
        step used to make a dozen blocking device -> host copies -- 0.86 ms per step on MI355X, most of it waiting.)"""
        e, s = self.engine, self._pinned
        d, nx = e.d, e.nx
        if i > 0:
            sig_zeta = self._measurement_noise()
            e.ckf_filter(*s.upload(y, u), sig_zeta)
        belief_revision = e.belief_revision
        s.mu.copy_(e.x0, non_blocking=True)      # the belief the plan starts from (planning does not change it)
        s.cov.copy_(e.sig_x0, non_blocking=True)
        self._sweeps(self.n_iter)
        plan = self._copy_plan()  # (enqueued ahead of the synchronisation: the copies run while the host waits)
        s.cell0.copy_(e.post[e.t0, : d + d * (d + 1) // 2, :], non_blocking=True)  # cells[0]: mu_xu0_m, sig_xu0_m (row t0 of the ring)
        s.status.copy_(e.status, non_blocking=True)
        if e.device.type == "cuda":
            torch.cuda.current_stream(e.device).synchronize()
        if self.B == 1:
            e.raise_on_failure(s.status.numpy())
        self._record(plan)
        mu_b = self._squeeze(np.array(s.mu.numpy().T, dtype=float), column=True)
        cov_b = self._squeeze(unpack_sym(s.cov.T.clone(), nx).numpy().astype(float))
        self._belief_host = (belief_revision, mu_b, cov_b)
        self.mus.append(np.array(mu_b, copy=True))
        self.covars.append(np.array(cov_b, copy=True))
        self._write_back_belief()
        cell0 = s.cell0.numpy().T  # (B, d + sym d)
        ctrl = _action(cell0[:, nx:d], cell0[:, d:], d, deterministic)
        e.shift_horizon(self._next_target(i))
        return self._squeeze(ctrl, column=True)
