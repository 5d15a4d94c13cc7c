"""Batched i2c engine: device state as PyTorch tensors, sweeps as HIP kernels through the C ABI.

`BatchedI2c` is the batched counterpart of the reference's I2cGraph (i2c/i2c.py:732-1314): B
independent trajectories of one model and horizon, optimised by the same EM iteration
(learn_msgs, i2c.py:1238-1245). The EM loop lives here in Python; every sweep is one call into
``libi2c_hip.so``. PyTorch is plumbing only: it owns the HBM buffers and the stream.

Device layout (see include/i2c_hip.h): every per-cell buffer is logically ``[T][E][B]``, symmetric matrices packed
(lower, row-major). Physically the trajectory index is innermost -- except for the models with wave kernels, whose
posterior / prior and forward-message buffers are trajectory-major (``[T][B][E]``) behind permuted views.
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from ._native import F32, F64, F64_F32S, I2cProblem


def sym_size(n):
    return n * (n + 1) // 2


def tril_index(n):
    r, c = np.tril_indices(n)
    return r, c  # row-major order of the lower triangle == packed order


def pack_sym_np(mat):
    """(..., n, n) -> (..., n(n+1)/2) packed lower, row-major."""
    mat = np.asarray(mat, dtype=np.float64)
    r, c = tril_index(mat.shape[-1])
    return mat[..., r, c]


def unpack_sym(packed, n):
    """torch (..., n(n+1)/2) -> (..., n, n) full symmetric."""
    r, c = tril_index(n)
    r_t = torch.as_tensor(r, device=packed.device)
    c_t = torch.as_tensor(c, device=packed.device)
    out = packed.new_zeros(packed.shape[:-1] + (n, n))
    out[..., r_t, c_t] = packed
    out[..., c_t, r_t] = packed
    return out


def _addr(t):
    """Device address of an optional tensor for a pointer field of a ctypes structure (None: NULL)."""
    return None if t is None else t.data_ptr()


POLICY_CODES = {"linear": 0, "expert": 1, "expert_soft": 1, "expert_hard": 2}  # the `policy` of i2c_rollout / I2cRolloutEval


class I2cNumericalError(np.linalg.LinAlgError):
    """A covariance lost positive definiteness (the reference raises LinAlgError from
    np.linalg.cholesky / scipy, i2c/inference/quadrature.py:17-24)."""


class BatchedI2c:
    def __init__(self, model, horizon, Q, R, Qf, alpha, alpha_update_tol, mu_u, sig_u,
                 mu_x_terminal=None, sig_x_terminal=None, quad=(1.0, 0.0, 0.0), x0=None, sig_x0=None,
                 z_traj=None, batch=None, dtype=torch.float64, device=None, lib=None, dtemp=1.0,
                 keep_zpost=True, keep_prior=False, keep_xm=True, backward_mode="auto", inference="cubature",
                 gh_degree=None, group_lanes=0, storage_dtype=None, allow_inexact=False, keep_prior_joint=False, post_layout=None,
                 deterministic_family=False, overlap_propagation=True, model_params=None, horizons=None):
        self.lib = lib if lib is not None else _native.load_library()
        if device is None:
            device = "cpu" if self.lib.is_host_sim else "cuda"
        self.device = torch.device(device)
        self._dev_index = None
        # What a host-side view of the engine's results was made at (I2cGraph's cell views, the policies' belief): `revision` advances
        # with every library call that takes buffers (_call) and every method that changes solver state from the host,
        # `belief_revision` wherever x0 / sig_x0 are written. Plain ints: a view is fresh while the number it kept still holds.
        self.revision = self.belief_revision = 0
        if self.lib.is_host_sim != (self.device.type == "cpu"):
            raise RuntimeError(
                f"library '{self.lib.build_info}' cannot run on device {self.device}: the HIP build needs a "
                "GPU tensor device (there is no CPU fallback)"
            )
        # (the request is resolved in two halves, around the cost model, so that every check keeps its place in the order)
        backward_mode = self._resolve_kernels(model, horizon, dtype, storage_dtype, allow_inexact, inference, quad, group_lanes,
                                              deterministic_family, backward_mode, overlap_propagation)
        priors = self._set_cost_model(model, Q, R, Qf, alpha_update_tol, mu_u, sig_u, x0, sig_x0, batch)
        self._resolve_inference(model, inference, gh_degree, quad, horizons, mu_x_terminal, sig_x_terminal, dtemp)
        self._allocate(model, priors, alpha, z_traj, keep_zpost, keep_prior, keep_xm, keep_prior_joint, post_layout, backward_mode,
                       model_params)

    def _resolve_kernels(self, model, horizon, dtype, storage_dtype, allow_inexact, inference, quad, group_lanes,
                         deterministic_family, backward_mode, overlap_propagation):
        """Request, first half: precision, the model's dimensions, the kernel family asked for. Returns the backward mode to ask for."""
        # Precision. dtype = ARITHMETIC type: float64 is the reference's arithmetic and the only parity-grade one.
        #   storage_dtype=torch.float32 with dtype=torch.float64: the mixed mode I2C_F64_F32S -- fp64 arithmetic on fp32-STORED
        #     per-cell buffers (post, fwd, xm, zpost, prior_out); half the HBM bytes, deviation from fp64 bounded
        #     (tests/test_precision.py); cubature EM path of the one-lane kernels only.
        #   dtype=torch.float32: fp32 arithmetic. NOT parity-grade (the curvature terms of the sigma-point transform are
        #     below fp32 resolution: O(1) deviation after a few EM iterations with status 0), so it has to be asked for
        #     explicitly with allow_inexact=True (tolerance sweeps).
        assert dtype in (torch.float64, torch.float32)
        if dtype == torch.float32 and not allow_inexact:
            raise ValueError("dtype=torch.float32 runs the kernels in fp32 ARITHMETIC, which is not parity-grade (DESIGN.md section 4): "
                             "pass allow_inexact=True for a tolerance sweep, or storage_dtype=torch.float32 with dtype=torch.float64 "
                             "for fp32 storage with fp64 arithmetic")
        if storage_dtype not in (None, dtype, torch.float32):
            raise ValueError("storage_dtype must be None, the arithmetic dtype, or torch.float32")
        self.dtype = dtype
        self.store_dtype = dtype if storage_dtype is None else storage_dtype
        self.mixed = self.store_dtype != self.dtype
        self.sys = model
        self.model_id = int(model.resolve_model_id(self.lib)) if hasattr(model, "resolve_model_id") else int(model.model_id)
        dims = self.lib.query(self.model_id)
        self.dims = dims
        nx, nu, nz, nzt = dims.nx, dims.nu, dims.nz, dims.nzt
        assert (nx, nu, nz) == (model.dim_x, model.dim_u, model.dim_z), "model plugin / library dimension mismatch"
        self.nx, self.nu, self.nz, self.nzt, self.d = nx, nu, nz, nzt, nx + nu
        self.H = T = int(horizon)
        # group kernels (csrc/i2c_group.hpp): `group_lanes` lanes of a wavefront per trajectory. 0 = the model's default
        # (one lane per trajectory, except for models that only have group kernels; the d >= 7 lane models run their
        # FORWARD sweep on the group kernels at small batches); True = the model's group width; -1 = one lane per
        # trajectory for every sweep.
        if group_lanes is True:
            group_lanes = dims.group_lanes
        # deterministic_family=True: results that do NOT depend on the batch size or on how a batch is sharded over GPUs (round-4
        # review, weak #9). The defaults pick the fastest kernel family and backward schedule for the batch at hand -- the family
        # changes at measured batch windows, the chunk count of the chunked schedule with B -- and families / schedules round
        # differently in the last bits. The switch pins what `group_lanes=0` and `backward_mode="auto"` would otherwise resolve
        # per batch: one lane per trajectory with the sequential (fused) backward walk for the d <= 8 models, the wave kernels
        # with their fused walk for the d = 16 model. A trajectory's result is then a function of its own inputs only (tested).
        # It is the slow-but-reproducible path at small batches; the default stays the fast one.
        self.overlap_propagation = bool(overlap_propagation)  # learn(n) with closed-loop propagation: see _learn_with_propagation
        self.deterministic_family = bool(deterministic_family)
        if self.deterministic_family:
            if not group_lanes:
                group_lanes = 64 if dims.wave else -1
                if dims.wave and inference == "cubature" and tuple(float(v) for v in quad) != (1.0, 0.0, 0.0):
                    group_lanes = _native.LANES_QUAD  # (the wave kernels only have the unit rule: general weights are the quad kernels', round 6)
            if backward_mode == "auto":
                backward_mode = "fused"
        self.group_lanes = int(group_lanes or 0)
        # 64 = the wave kernels (csrc/i2c_wave.hpp: one wavefront per trajectory, blocks in the fp64 matrix-instruction layout),
        # for the models that have them (dims.wave): forward and backward sweeps; propagation and filter run the model's default
        # 64 with inference="gauss_hermite": the grid kernels (csrc/i2c_grid.hpp: one wavefront per trajectory, the tensor grid strided
        # over its lanes) of every model that has one-lane kernels; they read and write the one-lane kernels' buffers
        self.grid_requested = bool(self.group_lanes == 64 and inference == "gauss_hermite" and not dims.group_only)
        ok = self.group_lanes in (0, dims.group_lanes) or (self.group_lanes == -1 and not dims.group_only) or self.grid_requested or \
            (self.group_lanes == 64 and (dims.wave or dims.quad)) or (self.group_lanes == _native.LANES_QUAD and dims.quad)
        if not ok:
            raise ValueError(f"group_lanes={self.group_lanes}: this model's group kernels use {dims.group_lanes} lanes"
                             + (" and it has no one-lane kernels" if dims.group_only else " (or -1: one lane per trajectory)")
                             + (" (or 64: one wavefront per trajectory)" if dims.wave else "")
                             + (" (or 64: four trajectories per wavefront, forward sweep)" if dims.quad else ""))
        # 64 on a model with the quad kernel (csrc/i2c_quad.hpp: four trajectories per wavefront on the 4 x 4 x 4 fp64 matrix
        # instruction): the FORWARD sweep runs on it, every other sweep on the model's default kernels
        # (_native.LANES_QUAD asks for it on a model that also has wave kernels, where 64 means those)
        self.quad_requested = bool(((self.group_lanes == 64 and dims.quad and not dims.wave) or self.group_lanes == _native.LANES_QUAD)
                                   and not self.grid_requested)
        self.uses_group_kernels = bool((self.group_lanes > 0 and not self.quad_requested and not self.grid_requested)
                                       or dims.group_only)  # a multi-lane family (group or wave) serves the sweeps
        if self.mixed and inference != "cubature":
            raise ValueError("fp32 storage (storage_dtype) is available for the cubature path only")
        if self.mixed and self.uses_group_kernels and not (dims.wave and self.group_lanes in (0, 64, _native.LANES_QUAD)):
            raise ValueError("fp32 storage (storage_dtype) is available for the one-lane, the quad and the wave kernels only")
        return backward_mode

    def _set_cost_model(self, model, Q, R, Qf, alpha_update_tol, mu_u, sig_u, x0, sig_x0, batch):
        """The batch size, the priors broadcast to it (returned for _allocate: mu_u, x0, sig_x0, sig_u) and the cost model."""
        T, nx, nu, nz, nzt = self.H, self.nx, self.nu, self.nz, self.nzt
        mu_u = np.asarray(mu_u, dtype=np.float64)
        if mu_u.ndim == 2:
            mu_u = mu_u[None]
        assert mu_u.shape[1:] == (T, nu), f"mu_u must be (T, nu) or (B, T, nu), got {mu_u.shape}"
        B = mu_u.shape[0]
        if x0 is not None:
            x0 = np.asarray(x0, dtype=np.float64).reshape(-1, nx)
            B = max(B, x0.shape[0])
        if batch is not None:
            B = max(B, int(batch))
        self.B = B
        mu_u = np.broadcast_to(mu_u, (B, T, nu))
        x0 = np.broadcast_to(np.asarray(model.x0, np.float64).reshape(nx) if x0 is None else x0, (B, nx))
        sig_x0 = np.asarray(model.sig_x0 if sig_x0 is None else sig_x0, dtype=np.float64)
        sig_x0 = np.broadcast_to(sig_x0, (B, nx, nx))
        sig_u = np.atleast_2d(np.asarray(sig_u, dtype=np.float64))
        self.mu_u0_base, self.sig_u0_base = np.array(mu_u), np.array(sig_u)  # the initial action prior (I2cCell.mu_u0_base, i2c.py:128-129)

        # cost model (i2c.py:778-793)
        R = np.atleast_2d(np.asarray(R, dtype=np.float64))
        if Q is not None:
            Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
            assert Q.shape[0] == Q.shape[1] and R.shape[0] == R.shape[1] and Q.shape[0] + R.shape[0] == nz, (
                f"blkdiag(Q, R) must be ({nz},{nz}), got Q {Q.shape}, R {R.shape}")
            QR = np.zeros((nz, nz))
            QR[: Q.shape[0], : Q.shape[0]] = Q
            QR[Q.shape[0]:, Q.shape[0]:] = R
        else:
            QR = R
        assert QR.shape == (nz, nz), f"blkdiag(Q, R) must be ({nz},{nz}), got {QR.shape}"
        assert np.allclose(QR, QR.T), "Q and R must be symmetric"
        self.Q, self.R, self.QR = Q, R, QR
        self.sig_xi0 = np.linalg.inv(QR)
        assert np.linalg.det(self.sig_xi0) > 0.0  # i2c.py:803-804
        self.has_Qf = Qf is not None and nzt > 0
        if Qf is not None:
            self.Qf = np.atleast_2d(np.asarray(Qf, dtype=np.float64))
            self.sig_xi_terminal_base = np.linalg.inv(self.Qf)
        else:
            self.Qf = np.zeros((nx, nx))  # i2c.py:792
            self.sig_xi_terminal_base = None
        self.alpha_update_tol = float(alpha_update_tol)
        return mu_u, x0, sig_x0, sig_u

    def _resolve_inference(self, model, inference, gh_degree, quad, horizons, mu_x_terminal, sig_x_terminal, dtemp):
        """Request, second half: the inference rule and what hangs on it (process noise, horizons, quadrature, terminal prior)."""
        dims, dtype, nx, nu, nzt = self.dims, self.dtype, self.nx, self.nu, self.nzt
        # inference method of the E-step (I2cGraph's `inference`, i2c.py:103-127): "cubature" = sigma points with
        # CubatureQuadrature(*quad); "linearize" = Linearize(), whose plan cost and propagation use
        # CubatureQuadrature(1, 0, 0) (i2c.py:109-115, 841-844)
        # "gauss_hermite" = GaussHermiteQuadrature(gh_degree): tensor grid of gh_degree ** dim points (exp_types.py:52-68)
        if inference not in ("cubature", "linearize", "gauss_hermite"):
            raise ValueError(f"unknown inference method {inference!r}")
        self.inference = inference
        # A model with state-action-dependent process noise (KnownModel.process_noise; the functor's process_noise member) is served by
        # the one-lane kernels and the d <= 8 quad kernels under the sigma-point rule: the other forms of the term do not exist, and the library answers
        # I2C_ENOTSUP for them (Impl::resolve) -- refused here, before anything is allocated.
        # Whether the FUNCTOR has the member is the library's to say: asked here, of the resolver, before anything is allocated -- the
        # state estimator's filter step under Linearize() is served for every model without the member (whatever kernels it has) and
        # is I2C_ENOTSUP for every model with it. A Python object that overrides process_noise over a functor without the member
        # (an in-tree model_id kept, say) would be solved with constant noise, silently: refused. The reverse -- a header with the
        # member under a class without the override -- is a model with the term.
        probe = _native.I2cProblem()
        probe.abi_version, probe.model_id, probe.B, probe.T = _native.ABI_VERSION, self.model_id, 1, 1
        probe.inference, probe.quad_alpha = _native.INF_LINEARIZE, 1.0
        functor_has = self.lib.i2c_kernel_family(C.byref(probe), _native.SWEEP_FILTER) == -2  # I2C_ENOTSUP
        if bool(getattr(model, "has_process_noise", False)) and not functor_has:
            raise ValueError(f"{type(model).__name__} overrides process_noise, but its device functor (model id {self.model_id}) has no "
                             "process_noise member: the kernels would solve it with constant noise (INTEGRATION.md section 3)")
        self.has_process_noise = functor_has
        if self.has_process_noise:
            if dims.group_only:
                raise ValueError("a model with process_noise needs the one-lane kernels (nx + nu <= 8): this one has group kernels only")
            if inference != "cubature":
                raise ValueError(f"inference={inference!r}: a model with process_noise is solved with the sigma-point rule (\"cubature\") only")
            # (the d <= 8 quad kernels: the forward sweep sums the term over its lanes; fp64 arithmetic, as every quad kernel)
            quad_ok = bool(dims.quad) and nx + nu <= 8 and dtype == torch.float64
            if self.group_lanes not in (0, -1) + ((64, _native.LANES_QUAD) if quad_ok else ()):
                raise ValueError(f"group_lanes={self.group_lanes}: a model with process_noise runs on the one-lane kernels (0 or -1)"
                                 + (f" or the quad kernels (64 or {_native.LANES_QUAD})" if quad_ok else ""))
        # Per-trajectory horizons (I2cProblem.horizons): trajectory b consists of cells 0 .. horizons[b] - 1; `horizon` stays the
        # allocated number of rows T >= max(horizons). Served by the one-lane kernels in fp64 under the sigma-point rule with the fused
        # backward walk (include/i2c_hip.h); checked here, on the host, before anything is allocated.
        self._horizons = None
        self._horizons_np = None if horizons is None else self._check_horizons(horizons, inference)
        self.linearize = inference == "linearize"
        self.gauss_hermite = inference == "gauss_hermite"
        self.gh_degree = 0
        if self.gauss_hermite:
            self.gh_degree = int(gh_degree)
            if not 1 <= self.gh_degree <= _native.MAX_GH_DEGREE:
                raise ValueError(f"gh_degree must be in 1..{_native.MAX_GH_DEGREE}")
            if self.gh_degree ** (nx + nu) > 2 ** 31 - 1:
                raise ValueError("gh_degree ** (nx + nu) points do not fit the kernels' 32-bit point counter")
            quad = (1.0, 0.0, 0.0)
        if self.linearize:
            quad = (1.0, 0.0, 0.0)
            if nzt == 0:
                raise NotImplementedError("Linearize() needs a terminal observation: for this model the reference's "
                                          "observe_terminal_linearize returns None and i2c.py:500-501 fails")
        self.quad = tuple(float(q) for q in quad)
        self.mu_x_terminal = None if mu_x_terminal is None else np.asarray(mu_x_terminal, np.float64).reshape(nx)
        self.sig_x_terminal = None if sig_x_terminal is None else np.asarray(sig_x_terminal, np.float64)
        self.has_x_terminal = self.sig_x_terminal is not None
        if self.has_x_terminal and self.mu_x_terminal is None:
            raise TypeError("sig_x_terminal given without mu_x_terminal: the reference's cubature rule crashes on it (i2c.py:558) and the "
                            "mean its Linearize rule back-calculates (i2c.py:464-470) is not implemented here")
        self.dtemp = float(dtemp)

    def _allocate(self, model, priors, alpha, z_traj, keep_zpost, keep_prior, keep_xm, keep_prior_joint, post_layout, backward_mode,
                  model_params):
        """The device buffers, the descriptor, and the resolver's two answers (backward schedule, kernel families) that size them."""
        mu_u, x0, sig_x0, sig_u = priors
        dims, T, B, nx, nu, nz, nzt = self.dims, self.H, self.B, self.nx, self.nu, self.nz, self.nzt
        inference = self.inference
        dev, dt, st = self.device, self.dtype, self.store_dtype
        to = lambda a: torch.as_tensor(np.array(a, dtype=np.float64, order="C"), dtype=dt, device=dev)  # noqa: E731
        zeros = lambda *s: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        zeros_s = lambda *s: torch.zeros(*s, dtype=st, device=dev)  # noqa: E731  (per-cell buffers: storage type)
        d = self.d
        # initial "posterior" = cell constructor state (i2c.py:95-100, 135-136)
        post = np.zeros((T, dims.e_post, B))
        post[:, :nx, :] = x0.T[None]
        post[:, nx:d, :] = np.transpose(mu_u, (1, 2, 0))
        S0 = np.zeros((B, d, d))
        S0[:, :nx, :nx] = sig_x0
        S0[:, nx:, nx:] = sig_u
        post[:, d: d + sym_size(d), :] = pack_sym_np(S0).T[None]
        o_k = d + sym_size(d) + nu * nx
        post[:, o_k: o_k + nu, :] = np.transpose(mu_u, (1, 2, 0))  # k = mu_u (i2c.py:136)
        post[:, o_k + nu:, :] = pack_sym_np(sig_u)[None, :, None]
        # Layout of the posterior / prior buffers (I2cProblem.post_layout): logically always [T][e_post][B]; for the models with
        # wave kernels the STORAGE is trajectory-major, [T][B][e_post] (a cell of a trajectory is contiguous: a wavefront, which
        # works on one trajectory, reads it as a few cache lines), and self.post is a permuted view of it, so every index
        # expression in this file and its callers is layout-blind; only the library (data_ptr) sees the difference.
        # post_layout: an explicit constructor argument (it is part of the ABI, I2cProblem.post_layout: callers handing raw pointers
        # to the C API must know it); None = trajectory-major for the models with wave kernels, [T][e][B] for every other model
        if post_layout is None:
            post_layout = 1 if dims.wave else 0
        if post_layout not in (0, 1) or (post_layout == 1 and not dims.wave):
            raise ValueError(f"post_layout={post_layout!r}: 0 ([T][e][B]) or 1 (trajectory-major, models with wave kernels only)")
        self.post_layout = int(post_layout)
        self.post = to(post).to(st)
        if self.post_layout == 1:
            self.post = self.post.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        # The forward sweep reads `prior`, the backward sweep writes `post`. Normally they are ONE buffer (after
        # _update_priors the prior IS the posterior, i2c.py:1210-1221, so the copy is free). keep_prior_joint=True keeps
        # them apart until update_priors(): two forward/backward passes without _update_priors() in between then start
        # from the same prior, as the reference's cells do (the drop-in I2cGraph asks for this; costs a second buffer).
        self.keep_prior_joint = bool(keep_prior_joint)
        self.prior = self.post
        self._post_spare = torch.empty_like(self.post) if self.keep_prior_joint else None
        self.fwd = zeros_s(T, dims.e_fwd, B)
        self.zpost = zeros_s(T, dims.e_zpost, B) if keep_zpost else None
        self.prior_out = zeros_s(T, d + sym_size(d), B) if keep_prior else None
        self.e_term = 4 + nzt + sym_size(nzt)
        self.term_stats = zeros(self.e_term, B)
        self.stats_out = zeros(4, B)
        self.prop = self.prop_stats = None  # made on first use: _propagation_buffers()
        self._loop_yu = self._eval_work = self._health = None  # (scratch of run_closed_loop, evaluate, iteration_health)
        self._mpc_action = zeros(nu + sym_size(nu), B)  # where a control step leaves the first planned action's moments
        self._minus_one = torch.full((B,), -1.0, dtype=dt, device=dev)  # costs_pf of an iteration without propagation (i2c.py:1065)
        self.x0 = to(x0.T)
        self.sig_x0 = to(pack_sym_np(sig_x0).T)
        self.alpha = to(np.broadcast_to(np.asarray(alpha, np.float64), (B,)))
        self.temp = torch.ones(B, dtype=dt, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.feedforward = torch.ones(T, dtype=torch.uint8, device=dev)  # i2c.py:132
        if z_traj is not None:
            z = np.broadcast_to(np.asarray(z_traj, np.float64), (B, T, nz))
            self.z = to(np.transpose(z, (1, 2, 0)))
        else:
            self.z = None
        self.zg = np.asarray(model.zg, np.float64).reshape(nz)
        self.zg_term = None if model.zg_term is None else np.asarray(model.zg_term, np.float64).reshape(-1)

        # Ring offset of the persistent per-cell buffers (post / prior, z, alpha_cell, feedforward): cell t of the horizon
        # lives in row (t0 + t) mod T (I2cProblem.t0). Only the MPC shift moves it; cells() / the getters undo it.
        self.t0 = 0
        self.alpha_cell = None      # [T][B] per-cell temperature, only in the MPC loop (see enable_per_cell_alpha)
        self.alpha_init = None
        self.terminal_cell = T - 1  # cell whose forward pass applies the terminal cost update (i2c.py:82,822)
        self.cell_init = self.post[0].clone()  # a fresh cell (I2cCell.__init__), appended by shift_horizon(): one cell block in the layout of post
        self.tau = T - 1  # i2c.py:833
        self._propagate = False
        self.use_expert_controller = True
        self.expert_cells = None  # optional [T] uint8 ring: per-cell use_expert_controller (set_cell_expert)
        self.em_iter = 0
        # per-iteration metrics as device tensors (B,): no host sync inside the EM loop
        self.alphas = [self.alpha.clone()]
        self.alphas_desired = [self.alpha.clone()]
        self.alphas_pf = [self.alpha.clone()]
        self.costs_m, self.costs_m_var, self.costs_pf, self.costs_pf_var, self.kl_terms = [], [], [], [], []
        self.backward_mode = {"auto": _native.BWD_AUTO, "two_pass": _native.BWD_TWO_PASS, "fused": _native.BWD_FUSED,
                              "chunked": _native.BWD_CHUNKED}[backward_mode]
        # ONE resolver (round-4 review, weak #8): the library decides which kernel family serves each sweep of THIS problem
        # (i2c_kernel_family) and which backward schedule will run (i2c_backward_schedule: inference rule, family, precision,
        # batch size, the request); the workspaces and the layout of the forward messages follow from its answers. A problem
        # the library refuses is refused here, with the library's code.
        self.work = None
        # Per-trajectory model parameters (I2cProblem.model_params_b): None = model.device_params() for every trajectory;
        # a (B, NP) array = trajectory b's dynamics / observe / measure use row b. Kept on the device as [NP][B] (arithmetic dtype).
        self._params_b = None
        if model_params is not None:
            self._params_b = self._params_to_device(model_params)
        if self._horizons_np is not None:
            self._horizons = torch.as_tensor(self._horizons_np, dtype=torch.int32, device=dev)
        self._problem = self._make_problem()
        mode = self.lib.i2c_backward_schedule(C.byref(self._problem))
        if mode not in (_native.BWD_TWO_PASS, _native.BWD_FUSED, _native.BWD_CHUNKED):
            raise RuntimeError(f"i2c_backward_schedule() refused the problem with code {mode} (include/i2c_hip.h): model "
                               f"{type(model).__name__}, inference {inference!r}, group_lanes {self.group_lanes}, B {B}, T {T}")
        self.fused_backward = mode == _native.BWD_FUSED
        self.backward_schedule = {_native.BWD_TWO_PASS: "two_pass", _native.BWD_FUSED: "fused", _native.BWD_CHUNKED: "chunked"}[mode]
        # the two-pass backward needs xm / cell_stats as workspace; the fused and chunked ones only write xm on request
        two_pass = mode == _native.BWD_TWO_PASS
        self.xm = zeros_s(T, dims.e_xm, B) if (keep_xm or two_pass) else None
        self.cell_stats = zeros(T, 2, B) if two_pass else None
        if mode == _native.BWD_CHUNKED:
            nbytes = self.lib.i2c_workspace_bytes(self.model_id, F64 if dt == torch.float64 else F32, B, T)
            self.work = torch.empty(nbytes // (8 if dt == torch.float64 else 4), dtype=dt, device=dev)
        # The forward-message buffer is private to the kernel family that writes and reads it: the wave kernels and the d = 16 quad
        # backward sweep keep it trajectory-major, [T][B][e_fwd] (include/i2c_hip.h); forward_messages() reads it through a view
        # either way. The reader decides.
        fam_b, fam_f = self.kernel_family("backward"), self.kernel_family("forward")  # (raise with the library's code on a refusal)
        self.fwd_trajectory_major = fam_b == "wave" or (fam_b == "quad" and bool(dims.wave))
        if fam_f == "wave" and not self.fwd_trajectory_major:
            raise RuntimeError("the wave forward sweep needs the wave backward sweep (forward-message layout)")
        if self.fwd_trajectory_major:
            self.fwd = self.fwd.reshape(T, B, dims.e_fwd)
        self._problem = self._make_problem()  # (now with the workspace)

    # ------------------------------------------------------------------ C-ABI plumbing
    def _make_problem(self, plant_params_b=None):
        """A descriptor of the engine as it is now. plant_params_b: a [NP][B] tensor that stands in for the engine's per-trajectory
        model parameters (_plant_problem)."""
        p = I2cProblem()
        p.abi_version = _native.ABI_VERSION
        p.model_id = self.model_id
        p.dtype = F64_F32S if self.mixed else (F64 if self.dtype == torch.float64 else F32)
        p.B, p.T = self.B, self.H
        p.has_Qf = int(self.has_Qf)
        p.has_x_terminal = int(self.has_x_terminal)
        p.z_per_cell = int(self.z is not None)
        p.backward_mode = self.backward_mode
        p.terminal_cell = int(self.terminal_cell)
        p.inference = (_native.INF_LINEARIZE if self.linearize else
                       _native.INF_GAUSS_HERMITE if self.gauss_hermite else _native.INF_CUBATURE)
        p.gh_degree = self.gh_degree
        p.group_lanes = self.group_lanes
        p.t0 = int(self.t0)
        p.post_layout = int(self.post_layout)
        if self.gauss_hermite:
            gx, gw = np.polynomial.hermite.hermgauss(self.gh_degree)  # exp_types.py:57
            for i in range(self.gh_degree):
                p.gh_nodes[i], p.gh_weights[i] = float(gx[i]), float(gw[i])
        p.expert_controller = int(bool(self.use_expert_controller))
        p.quad_alpha, p.quad_beta, p.quad_kappa = self.quad
        p.dtemp = self.dtemp

        def put(dst, arr):
            arr = np.asarray(arr, np.float64).reshape(-1)
            for i, v in enumerate(arr):
                dst[i] = float(v)

        put(p.sig_eta, pack_sym_np(np.asarray(self.sys.sig_eta, np.float64)))
        put(p.sig_xi0, pack_sym_np(self.sig_xi0))
        put(p.QR, pack_sym_np(self.QR))
        if self.has_Qf:
            assert self.Qf.shape == (self.nzt, self.nzt)
            put(p.sig_xiT0, pack_sym_np(self.sig_xi_terminal_base))
            put(p.Qf, pack_sym_np(self.Qf))
            put(p.zg_term, self.zg_term)
        put(p.zg, self.zg)
        if self.has_x_terminal:
            put(p.mu_x_term, self.mu_x_terminal)
            put(p.sig_x_term, pack_sym_np(self.sig_x_terminal))
        params = list(self.sys.device_params()) if hasattr(self.sys, "device_params") else []
        assert len(params) == self.dims.n_params, "model plugin / library parameter-count mismatch"
        put(p.model_params, params)
        p.x0 = self.x0.data_ptr()
        p.sig_x0 = self.sig_x0.data_ptr()
        p.z = self.z.data_ptr() if self.z is not None else None
        p.alpha = self.alpha.data_ptr()
        p.alpha_cell = self.alpha_cell.data_ptr() if self.alpha_cell is not None else None
        p.temp = self.temp.data_ptr()
        p.work = self.work.data_ptr() if self.work is not None else None
        p.feedforward = self.feedforward.data_ptr()
        p.expert = self.expert_cells.data_ptr() if self.expert_cells is not None else None
        params_b = self._params_b if plant_params_b is None else plant_params_b
        p.model_params_b = params_b.data_ptr() if params_b is not None else None
        p.horizons = self._horizons.data_ptr() if self._horizons is not None else None
        return p

    def _check_horizons(self, horizons, inference=None):
        """A sequence of B ints in [1, T] -> int32 array; ValueError for a wrong length or value, and for every combination the
        kernels with per-trajectory horizons do not serve (the message names what to drop)."""
        h = horizons.detach().cpu().numpy() if torch.is_tensor(horizons) else np.asarray(horizons)
        if h.ndim != 1 or h.shape[0] != self.B:
            raise ValueError(f"horizons must be a sequence of B = {self.B} ints, got shape {h.shape}")
        if not np.issubdtype(h.dtype, np.integer):
            if not np.all(np.isfinite(h)) or np.any(h != np.round(h)):
                raise ValueError("horizons must be integers")
        h = h.astype(np.int64)
        if np.any(h < 1) or np.any(h > self.H):
            raise ValueError(f"horizons must lie in [1, horizon] = [1, {self.H}] (`horizon` is the allocated number of cells and "
                             f"must be at least max(horizons)), got min {int(h.min())}, max {int(h.max())}")
        inference = self.inference if inference is None else inference
        drop = []
        if self.dims.group_only:
            raise ValueError(f"horizons: {type(self.sys).__name__} has no one-lane kernels (nx + nu > 8); drop horizons and solve "
                             "each horizon in an engine of its own")
        if self.group_lanes not in (0, -1):
            drop.append(f"group_lanes={self.group_lanes} (per-trajectory horizons run on the one-lane kernels: 0 or -1)")
        if inference != "cubature":
            drop.append(f"inference={inference!r} (the sigma-point rule \"cubature\" only)")
        if self.dtype != torch.float64 or self.mixed:
            drop.append("dtype / storage_dtype float32 (fp64 arithmetic and storage only)")
        if self.has_process_noise:
            drop.append("the model's process_noise member (constant process noise only)")
        if getattr(self, "alpha_cell", None) is not None:
            drop.append("per-cell temperatures (enable_per_cell_alpha)")
        if getattr(self, "t0", 0) != 0 or getattr(self, "terminal_cell", self.H - 1) not in (self.H - 1, -1):
            drop.append("the moved horizon ring of the MPC loop (shift_horizon / mpc_step)")
        if drop:
            raise ValueError("horizons cannot be combined with " + "; ".join(drop) + ": drop that, or drop horizons")
        return h.astype(np.int32)

    @property
    def horizons(self):
        """Per-trajectory horizons as a (B,) int32 tensor, or None when every trajectory has the allocated horizon."""
        return None if self._horizons is None else self._horizons.clone()

    def set_horizons(self, h):
        """Replace the per-trajectory horizons (a sequence of B ints in [1, horizon]) in place; an engine built without them gets
        its buffer here and from then on runs the one-lane kernels with the fused backward walk. Rows beyond a trajectory's new
        horizon keep whatever they held."""
        v = torch.as_tensor(self._check_horizons(h), dtype=torch.int32, device=self.device)
        self._horizons_np = v.cpu().numpy()
        if self._install("_horizons", v):
            mode = self.lib.i2c_backward_schedule(C.byref(self._problem))
            self._check(0 if mode == _native.BWD_FUSED else (mode if mode < 0 else -1), "i2c_backward_schedule")
            self.fused_backward, self.backward_schedule = True, "fused"

    def valid_cells(self):
        """(B, T) bool mask of the cells that exist: cell t of trajectory b with t < horizons[b] (all of them without horizons)."""
        t = torch.arange(self.H, device=self.device)
        if self._horizons is None:
            return torch.ones(self.B, self.H, dtype=torch.bool, device=self.device)
        return t[None, :] < self._horizons[:, None].to(t.dtype)

    def _cells_per_trajectory(self):
        """T_b as a (B,) tensor in the arithmetic dtype, or the float T without horizons."""
        return float(self.H) if self._horizons is None else self._horizons.to(self.dtype)

    def _no_horizons(self, what):
        if self._horizons is not None:
            raise ValueError(f"{what} is not available with per-trajectory horizons: drop horizons")

    def _params_to_device(self, params):
        """(B, NP) array / tensor of per-trajectory model parameters -> a new [NP][B] device tensor in the arithmetic dtype."""
        n_params = int(self.dims.n_params)
        if n_params == 0:
            raise ValueError(f"{type(self.sys).__name__} has no model parameters: there is nothing to vary per trajectory")
        a = params.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(params) else np.asarray(params, np.float64)
        if a.shape != (self.B, n_params):
            raise ValueError(f"model_params must be (B, NP) = ({self.B}, {n_params}), got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError("model_params must be finite")
        return torch.as_tensor(np.array(a.T, order="C"), dtype=self.dtype, device=self.device)

    @property
    def model_params(self):
        """Per-trajectory model parameters as a (B, NP) tensor, or None when every trajectory uses model.device_params()."""
        return None if self._params_b is None else self._params_b.T.clone()

    def set_model_params(self, params):
        """Replace the per-trajectory model parameters, (B, NP), in place (the device pointer stays: a payload that changes
        between MPC steps needs nothing else). An engine built without model_params gets its buffer here."""
        self._install("_params_b", self._params_to_device(params))

    def kernel_family(self, sweep="forward"):
        """Which kernel family serves a sweep of THIS problem ("lane", "group", "wave", "quad" or "grid"): i2c_kernel_family(), the library's
        single resolver of group_lanes, model defaults and batch thresholds. The last bits of a result depend on it.
        "chunk_passes": the compose + stitch passes of the chunked backward schedule, "chunk_stitch": its stitch pass alone (refused
        when another schedule runs)."""
        code = {"forward": _native.SWEEP_FORWARD, "backward": _native.SWEEP_BACKWARD, "propagate": _native.SWEEP_PROPAGATE,
                "filter": _native.SWEEP_FILTER, "chunk_passes": _native.SWEEP_CHUNK_PASSES, "chunk_stitch": _native.SWEEP_CHUNK_STITCH}[sweep]
        rc = self.lib.i2c_kernel_family(C.byref(self._problem), code)
        self._check(0 if rc > 0 else (rc or -1), "i2c_kernel_family")
        return _native.FAMILY_NAMES[rc]

    @property
    def forward_family(self):
        return self.kernel_family("forward")

    @property
    def backward_family(self):
        return self.kernel_family("backward")

    def refresh_problem(self):
        """Rebuild the C problem descriptor after changing host-side constants / tensors (a new buffer, that is a new pointer)."""
        self._problem = self._make_problem()

    def _install(self, name, value):
        """A persistent buffer the descriptor points to takes `value`: copied in place where the buffer exists (the pointer stays),
        else it becomes the buffer and the descriptor is rebuilt. Returns whether it was new."""
        buf = getattr(self, name)
        self.revision += 1
        if buf is None:
            setattr(self, name, value)
            self.refresh_problem()
        else:
            buf.copy_(value)
        return buf is None

    def sync_problem(self):
        """The one writer of the descriptor's mutable fields: they follow the engine's attributes. Runs before every library call
        (_call) and in the methods that move the ring (for whoever reads `_problem` in between). Returns the descriptor."""
        p = self._problem
        p.expert_controller = int(bool(self.use_expert_controller))
        p.t0 = int(self.t0)
        p.terminal_cell = int(self.terminal_cell)
        p.expert = None if self.expert_cells is None else self.expert_cells.data_ptr()
        return p

    def _call(self, name, *args, problem=None):
        """Every library call that takes buffers: lib.<name>(&problem, *args, stream) with the descriptor up to date, tensors handed
        over as pointers (None: NULL), a non-zero return code raised. problem: another descriptor (_plant_problem)."""
        self.revision += 1
        p = self.sync_problem() if problem is None else problem
        rc = getattr(self.lib, name)(C.byref(p), *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], self._stream())
        if rc != 0:
            self._check(rc, name)

    def _plant_problem(self, plant_params):
        """(descriptor, tensor to hold until the call is enqueued) of a call that runs on the PLANT's parameters (B, NP): a copy of
        the descriptor with them as model_params_b. None: the engine's own."""
        if plant_params is None:
            return self.sync_problem(), None
        plant = self._params_to_device(plant_params)
        return self._make_problem(plant), plant

    def _stream(self):
        """The caller's current HIP stream on the engine's device (what torch.cuda.current_stream(device).cuda_stream returns, read
        through the raw accessor: three sweeps per EM iteration ask for it, and the Stream-object path costs ~9 us each -- a tenth of
        a single-trajectory iteration's host time)."""
        if self.device.type == "cuda":
            if self._dev_index is None:
                self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
            if raw is not None:
                return C.c_void_p(raw(self._dev_index))
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    @staticmethod
    def _ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with code {rc} (see include/i2c_hip.h)")

    # ------------------------------------------------------------------ sweeps
    def forward_sweep(self):
        """I2cGraph._forward_msgs (i2c.py:876-880)."""
        if self.prior_out is not None:  # (the graph facade: the temperature THIS sweep ran at, for the cells' sig_z0_f = S_z + alpha xi)
            self.alpha_fwd = self.alpha.clone()
        self._call("i2c_forward_sweep", self.prior, self.fwd, self.prior_out, self.status)

    def backward_sweep(self):
        """I2cGraph._backward_msgs (i2c.py:882-886) + per-cell M-step statistics."""
        self._split_posterior()  # do not overwrite the prior of this sweep
        self._call("i2c_backward_sweep", self.fwd, self.xm, self.post, self.zpost, self.cell_stats, self.term_stats, self.status)

    def _split_posterior(self):
        """keep_prior_joint, before a sweep writes the posterior: it goes to the spare buffer, the prior stays what the forward
        sweep read. The inverse of _fold_posterior()."""
        if self.keep_prior_joint and self.post is self.prior:
            self.post, self._post_spare = self._post_spare, None

    def _fold_posterior(self):
        """The posterior becomes the prior (one buffer again); the old prior buffer is the spare one."""
        if self.prior is not self.post:
            self._post_spare, self.prior = self.prior, self.post

    def forward_backward(self):
        """I2cGraph._forward_backward_msgs (i2c.py:1231-1236)."""
        self.forward_sweep()
        self.backward_sweep()

    def riccati_sweep(self):
        """I2cGraph._backward_ricatti_msgs (i2c.py:888-893): Riccati-form backward messages after a Linearize
        forward/backward pass. Overwrites K, k, sigK with the Riccati-form controller (as the reference does) and
        returns the backward state message in information form, (nu_x0_b (B, T, nx), lambda_x0_b (B, T, nx, nx))."""
        self._no_horizons("riccati_sweep()")
        if not self.linearize:
            raise RuntimeError("the Riccati messages belong to the Linearize() path (i2c.py:612-678)")
        if self.prior_out is None or self.xm is None:
            raise RuntimeError("riccati_sweep() needs keep_prior=True and keep_xm=True")
        nx = self.nx
        self.ric = torch.zeros(self.H, nx + nx * nx, self.B, dtype=self.dtype, device=self.device)
        self._call("i2c_riccati_sweep", self.prior_out, self.fwd, self.xm, self.post, self.ric, self.status)
        nu = self.ric[:, :nx].permute(2, 0, 1)
        lam = self.ric[:, nx:].permute(2, 0, 1).reshape(self.B, self.H, nx, nx)
        return nu, lam

    def propagate(self, _stats=None):
        """I2cGraph.propagate (i2c.py:1247-1251). (_stats: a [3][B] row that receives the statistics instead of self.prop_stats)"""
        self._propagation_buffers()
        self._call("i2c_propagate", self.post, self.prop, self.prop_stats if _stats is None else _stats,
                   int(self.use_expert_controller), self.status)

    def _propagation_buffers(self):
        """prop ([T][e_prop][B]) and prop_stats ([3][B]: cost mean, cost variance, terminal KL), made on first use."""
        if self.prop is None:
            self.prop = torch.zeros(self.H, self.dims.e_prop, self.B, dtype=self.dtype, device=self.device)
            self.prop_stats = torch.zeros(3, self.B, dtype=self.dtype, device=self.device)

    def set_cell_expert(self, t, value):
        """cells[t].use_expert_controller = value (i2c.py:143): a per-cell flag like the reference's, allocated on first use
        (until then every cell follows `use_expert_controller`)."""
        if self.expert_cells is None:
            self.expert_cells = torch.full((self.H,), int(bool(self.use_expert_controller)), dtype=torch.uint8, device=self.device)
            self.sync_problem()
        self.expert_cells[(int(t) + self.t0) % self.H] = int(bool(value))
        self.revision += 1

    def cell_expert(self, t):
        if self.expert_cells is None:
            return bool(self.use_expert_controller)
        return bool(self.expert_cells[(int(t) + self.t0) % self.H].item())

    def update_priors(self):
        """I2cGraph._update_priors (i2c.py:1210-1221). The data copy is free: the forward sweep reads
        the posterior buffer as its prior; only the feed-forward -> feedback flags change."""
        if self.tau > 0:
            n = min(self.tau + 1, self.H)
            if self.t0 == 0:
                self.feedforward[:n] = 0  # one fill, no index arithmetic on the device
            else:
                self.feedforward[self.ring_rows(n)] = 0
        self._fold_posterior()
        self.revision += 1

    def _alpha_from_propagation(self):
        """calculate_alpha(sum of propagated observation covariances) (i2c.py:901-904, 934-939)."""
        return self.prop_stats[0] / (self.nz * self._cells_per_trajectory())

    def _mstep(self, update_alpha):
        """i2c_mstep on the statistics the last backward sweep left on the device -> a fresh [4][B] row: alpha_hat, alpha after the
        clamp, cost mean, cost variance."""
        self._call("i2c_mstep", self.term_stats, self.alpha_update_tol, int(bool(update_alpha)), self.stats_out)
        return self.stats_out.clone()

    def _record(self, mstep, prop=None, alphas=True, costs=True, alpha_pf=None, kl=None):
        """The one writer of the per-iteration history: plain lists of (B,) device tensors. The entries are views of rows copied once
        per iteration, and every costs_pf entry without propagation is the ONE constant row `_minus_one`: an entry of a history
        list must never be mutated in place, only replaced (as calibrate_alpha() does with alphas[-1]).
        mstep: [4][B] alpha_hat, alpha, cost mean, cost variance; prop: [3][B] propagated cost mean, variance, terminal KL, or None
        without propagation. alphas / costs: which halves of the M-step row this caller records; alpha_pf, kl: the entries of
        alphas_pf and kl_terms, where the caller has them."""
        if costs:
            self.costs_m.append(mstep[2])
            self.costs_m_var.append(mstep[3])
            if prop is None:
                self.costs_pf.append(self._minus_one)
            else:
                self.costs_pf.append(prop[0])
                self.costs_pf_var.append(prop[1])
        if alpha_pf is not None:
            self.alphas_pf.append(alpha_pf)
        if alphas:
            self.alphas_desired.append(mstep[0])
            self.alphas.append(mstep[1])
        if kl is not None:
            self.kl_terms.append(kl)

    def alpha_mstep(self, update_alpha=True):
        """compute_update_alpha (i2c.py:921-963) alone: alpha_hat from the backward sweep's statistics, the clamp, and --
        with update_alpha -- the new temperature in every cell (update_xi). No cost bookkeeping, no prior update.
        Returns (alpha_hat, alpha after the clamp) as (B,) tensors and appends them to alphas_desired / alphas."""
        out = self._mstep(update_alpha)
        self._record(out, costs=False)
        if update_alpha:
            self._broadcast_alpha()
        return out[0], out[1]

    def record_costs(self):
        """I2cGraph.calc_cost (i2c.py:1045-1066) alone: the expected cost of the current posterior (and of the propagation) appended
        to the cost lists, from the statistics the last backward sweep / propagation left on the device. The temperature is not
        touched (the M-step kernel runs with update_alpha = 0)."""
        self._record(self._mstep(False), self.prop_stats.clone() if self._propagate else None, alphas=False)

    def maximize(self, update_alpha=True):
        """I2cGraph._maximize (i2c.py:1004-1019): cost, prior update, temperature M-step."""
        out = self._mstep(update_alpha)
        ps = self.prop_stats.clone() if self._propagate else None  # ONE copy per iteration: the recorded rows are views of it
        self.update_priors()
        if update_alpha:
            self._broadcast_alpha()
        # (the KL term is float64 here and of the engine's dtype from i2c_learn_propagate: only an fp32 engine can tell)
        kl = (self._terminal_kl() if ps is None else ps[2].to(torch.float64)) if self.has_x_terminal else None
        self._record(out, ps, alpha_pf=None if ps is None else ps[0] / (self.nz * self._cells_per_trajectory()), kl=kl)

    def learn_msgs(self):
        """One EM iteration (I2cGraph.learn_msgs, i2c.py:1238-1245)."""
        self.em_iter += 1
        self.forward_backward()
        if self._propagate:
            self.propagate()
        self.maximize()

    def _learn_path(self, n_iters):
        """How learn(n_iters) runs: "stepwise" (n x learn_msgs), "fused" (i2c_learn) or "propagate" (i2c_learn_propagate).
        The library's loops update only alpha[b]; with per-cell temperatures (MPC) every cell has to take the new alpha each
        iteration (update_xi, i2c.py:961-981), which the stepwise path does through _broadcast_alpha(). Separate prior / posterior
        buffers (keep_prior_joint) need the host-side swap of update_priors(), kept priors (keep_prior) their alpha_fwd."""
        if n_iters <= 0 or self.alpha_cell is not None or self.keep_prior_joint or self.prior_out is not None:
            return "stepwise"
        if not self._propagate:
            return "fused"
        # closed-loop propagation inside the loop: the one-lane kernels under the sigma-point rule with fp64 / fp32 storage = arithmetic
        if self.mixed or self.uses_group_kernels or self.linearize or self.gauss_hermite:
            return "stepwise"
        return "propagate"

    def learn(self, n_iters):
        """n_iters EM iterations enqueued from C++ by ONE library call with no host round trip, the statistics of every iteration
        written straight into history rows: i2c_learn, or with closed-loop propagation (covariance control, BASELINE config 5)
        i2c_learn_propagate. The same numbers as n_iters x learn_msgs(), which is what runs where _learn_path() says so."""
        n_iters = int(n_iters)
        path = self._learn_path(n_iters)
        if path == "stepwise":
            for _ in range(n_iters):
                self.learn_msgs()
            return
        hist = torch.empty(n_iters, 4, self.B, dtype=self.dtype, device=self.device)  # alpha_hat, alpha, cost mean, cost variance
        sweeps = (self.post, self.fwd, self.xm, self.zpost, self.cell_stats, self.term_stats)
        if path == "propagate":
            return self._learn_with_propagation(n_iters, hist, sweeps)
        self._call("i2c_learn", *sweeps, self.alpha_update_tol, int(self.tau), n_iters, hist, self.status)
        self.em_iter += n_iters
        kl = self._terminal_kl() if self.has_x_terminal else None  # (nothing it reads changes inside the loop: once per call)
        for it in range(n_iters):
            self._record(hist[it], kl=kl)
        self._broadcast_alpha()

    def _learn_with_propagation(self, n_iters, hist, sweeps):
        """learn() through i2c_learn_propagate: forward, backward, propagate, M-step per iteration. From the second iteration on the
        propagation of iteration k shares a launch with the forward sweep of iteration k + 1 (`overlap_propagation`; lane kernels of
        the d <= 5 models): the two chains of T dependent cells become one (pendulum T=100, B=8192: 0.27 -> 0.19 ms per iteration)."""
        self._propagation_buffers()
        histp = torch.empty(n_iters, 3, self.B, dtype=self.dtype, device=self.device)  # propagated cost mean, variance, terminal KL
        self._call("i2c_learn_propagate", *sweeps, self.prop, histp, self.alpha_update_tol, int(self.tau), n_iters, hist,
                   int(self.use_expert_controller), int(self.overlap_propagation), self.status)
        self.em_iter += n_iters
        self.stats_out.copy_(hist[-1])
        self.prop_stats.copy_(histp[-1])
        apf = histp[:, 0] / (self.nz * self._cells_per_trajectory())  # = _alpha_from_propagation() of every iteration
        for it in range(n_iters):
            self._record(hist[it], histp[it], alpha_pf=apf[it], kl=histp[it, 2] if self.has_x_terminal else None)
        self._broadcast_alpha()

    def calibrate_alpha(self, only_decrease=False):
        """I2cGraph.calibrate_alpha (i2c.py:895-911)."""
        assert self._propagate
        self.propagate()
        a = self._alpha_from_propagation()
        if only_decrease:
            a = torch.where(a < self.alpha, a, self.alpha)
        self.alpha.copy_(a)
        self._broadcast_alpha()
        self.alphas[-1] = self.alpha.clone()

    # ------------------------------------------------------------------ MPC building blocks
    def set_initial_state(self, mu, cov):
        """sys.x0 / sys.sig_x0 of every trajectory (mpc.py:149-150). mu (B, nx) or (nx,), cov (B, nx, nx) or (nx, nx)."""
        mu = np.broadcast_to(np.asarray(mu, np.float64).reshape(-1, self.nx), (self.B, self.nx))
        cov = np.broadcast_to(np.asarray(cov, np.float64), (self.B, self.nx, self.nx))
        self.x0.copy_(torch.as_tensor(np.array(mu.T, order="C"), dtype=self.dtype))
        self.sig_x0.copy_(torch.as_tensor(np.array(pack_sym_np(cov).T, order="C"), dtype=self.dtype))
        self.revision += 1
        self.belief_revision += 1

    def ckf_filter(self, y, u, sig_zeta, mu=None, cov=None):
        """One cubature Kalman filter step on the belief (mu [nx][B], cov [sym nx][B]; default: the
        solver's x0 / sig_x0 tensors, updated in place) -- PartiallyObservedMpcPolicy.filter, mpc.py:125-145.
        y: [ny][B] tensor, u: [nu][B] tensor, sig_zeta: (ny, ny) array."""
        mu = self.x0 if mu is None else mu
        cov = self.sig_x0 if cov is None else cov
        ny = self.dims.ny
        assert y.shape == (ny, self.B) and u.shape == (self.nu, self.B) and y.dtype == self.dtype
        y, u = y.contiguous(), u.contiguous()  # bound to locals: a temporary copy must outlive the launch
        self.belief_revision += mu is self.x0 or cov is self.sig_x0
        self._call("i2c_ckf_filter", self._sig_zeta(sig_zeta, True), y, u, mu, cov, self.status)
        return mu, cov

    def enable_per_cell_alpha(self):
        """The reference's MPC appends `deepcopy(cell_init)`: that cell keeps the sig_xi it was copied with
        (the temperature at policy construction), because update_xi (i2c.py:976-981) only reaches the cells
        in the list when alpha changes and alpha is frozen inside the loop. Reproduced with a [T][B]
        per-cell temperature that follows the cells through the shift."""
        self._no_horizons("enable_per_cell_alpha()")
        if self.alpha_cell is None:
            self.alpha_init = self.alpha.clone()
            self.alpha_cell = self.alpha.reshape(1, -1).repeat(self.H, 1).contiguous()
            self.refresh_problem()
            self.revision += 1

    def renew_cell_init(self):
        """cell_init = deepcopy(cells[0]) (mpc.py:26): the cell shift_horizon() appends is, from now on, today's cell 0."""
        self.cell_init = self.post[self.t0].clone()

    def set_cell_feedforward(self, t, value):
        """cells[t].state_action_independence = value (i2c.py:132)."""
        self.feedforward[(int(t) + self.t0) % self.H] = 1 if value else 0
        self.revision += 1

    def set_alpha(self, value):
        """graph.alpha = value: the temperature of every trajectory (a scalar or (B,)), and of every cell in the chain."""
        self.alpha.copy_(torch.as_tensor(np.broadcast_to(np.asarray(value, float), (self.B,)).copy(), dtype=self.dtype))
        self._broadcast_alpha()
        self.revision += 1

    def _broadcast_alpha(self):
        """update_xi (i2c.py:976-981): every cell currently in the chain takes the graph's alpha."""
        if self.alpha_cell is not None:
            self.alpha_cell.copy_(self.alpha.reshape(1, -1).expand(self.H, -1))

    def ring_rows(self, n=None):
        """Physical rows of cells 0..n-1 (default: the whole horizon) in the ring buffers, as an index tensor."""
        n = self.H if n is None else n
        return (torch.arange(n, device=self.device) + self.t0) % self.H

    def cells(self, buf):
        """A ring buffer ([T][...]) in cell order (a view when the ring has not moved)."""
        return buf if self.t0 == 0 else torch.roll(buf, -self.t0, 0)

    def _advance_ring(self):
        self.t0 = (self.t0 + 1) % self.H
        if self.terminal_cell >= 0:
            self.terminal_cell -= 1
        self.sync_problem()

    def shift_horizon(self, z_new=None, want_action=False):
        """Receding horizon (mpc.py:174-181): drop cell 0, append a fresh feed-forward cell whose target is z_new ([nz][B]
        tensor) or, if None, the previous last cell's. The per-cell buffers are a ring: the fresh cell is written over the
        row of the dropped one (i2c_shift_horizon) and the ring offset advances -- nothing else moves. The `terminal_cell`
        flag stays with the cell it was set on (i2c.py:822), so its index decreases. Returns the dropped cell's action
        moments (mu_u (B, nu), sig_u packed (B, sym nu)) if want_action."""
        self._no_horizons("shift_horizon()")
        assert self.prior is self.post, "shift_horizon() between a sweep and its update_priors()"
        if z_new is not None:
            z_new = z_new.contiguous()
        self._call("i2c_shift_horizon", self.post, self.cell_init, self.alpha_init, z_new, self._mpc_action if want_action else None)
        self._advance_ring()
        if want_action:
            return self._mpc_action[: self.nu].T, self._mpc_action[self.nu:].T

    def mpc_step(self, n_iter, y=None, u=None, sig_zeta=None, z_new=None):
        """One control step of the MPC loop in one library call (i2c_mpc_step): optional filter step on the belief, n_iter
        sweeps, first action, receding-horizon shift -- no host round trip, no torch ops, no copy of the horizon (the per-cell
        buffers are a ring). Returns (mu_u (B, nu), sig_u packed (B, sym nu)) device tensors: the first planned action BEFORE
        the shift (cells[0].mu_u0_m, sig_u0_m). Same numbers as ckf_filter + n_iter x (forward_backward, update_priors) +
        shift_horizon."""
        self._no_horizons("mpc_step()")
        assert self.prior is self.post, "mpc_step() between a sweep and its update_priors()"
        st = _native.I2cMpcStep()
        st.do_filter = int(y is not None)
        self.belief_revision += y is not None
        if y is not None:
            assert y.shape == (self.dims.ny, self.B) and u.shape == (self.nu, self.B) and y.dtype == self.dtype
            y, u = y.contiguous(), u.contiguous()
            st.y, st.u = y.data_ptr(), u.data_ptr()
        self._fill_mpc_step(st, n_iter, self._sig_zeta(sig_zeta, True) if y is not None else None)
        if z_new is not None:
            z_new = z_new.contiguous()
        st.z_new = _addr(z_new)
        self._call("i2c_mpc_step", C.byref(st))
        self._advance_ring()
        return self._mpc_action[: self.nu].T, self._mpc_action[self.nu:].T

    # ------------------------------------------------------------------ the closed loop on the device
    def _fill_mpc_step(self, st, n_iter, zeta=None):
        """The fields of I2cMpcStep every control step of this engine shares (buffers, tau, the action row), and the measurement
        noise of a step that filters (zeta: what _sig_zeta() returned)."""
        st.n_iter, st.tau = int(n_iter), int(self.tau)
        st.post, st.fwd = self.post.data_ptr(), self.fwd.data_ptr()
        st.xm, st.zpost, st.cell_stats, st.term_stats = _addr(self.xm), _addr(self.zpost), _addr(self.cell_stats), self.term_stats.data_ptr()
        st.cell_init, st.alpha_init = self.cell_init.data_ptr(), _addr(self.alpha_init)
        st.action, st.status = self._mpc_action.data_ptr(), self.status.data_ptr()
        if zeta is not None:
            st.sig_zeta[: len(zeta)] = zeta[:]

    def _sig_zeta(self, sig_zeta, needed):
        """The measurement noise (ny, ny): the argument, else sys.sig_zeta; packed into a ctypes array, or None (an error if needed)."""
        if sig_zeta is None:
            sig_zeta = getattr(self.sys, "sig_zeta", None)
        if sig_zeta is None:
            if needed:
                raise ValueError("sig_zeta (measurement noise) is needed: pass it or set sys.sig_zeta")
            return None
        ny = self.dims.ny
        sig_zeta = np.asarray(sig_zeta, np.float64)
        assert sig_zeta.shape == (ny, ny), f"sig_zeta must be ({ny}, {ny}), got {sig_zeta.shape}"
        return (C.c_double * sym_size(ny))(*pack_sym_np(sig_zeta).reshape(-1))

    def _state_rows(self, a, n):
        """(B, n) / (n,) array or tensor -> a new contiguous [n][B] device tensor."""
        if torch.is_tensor(a):
            a = a.detach().to(self.device, self.dtype).reshape(-1, n)
            return a.expand(self.B, n).T.contiguous()
        a = np.broadcast_to(np.asarray(a, np.float64).reshape(-1, n), (self.B, n))
        return torch.as_tensor(np.array(a.T, order="C"), dtype=self.dtype, device=self.device)

    def _noise(self, given, shape, draw=False, generator=None):
        """Standard-normal samples of a simulation: the given ones (any array, taken in the kernels' layout `shape`), else drawn
        here with torch.randn(generator=generator) if `draw`, else None (no noise of that kind)."""
        if given is not None:
            return torch.as_tensor(given, dtype=self.dtype, device=self.device).reshape(shape).contiguous()
        return torch.randn(*shape, dtype=self.dtype, device=self.device, generator=generator) if draw else None

    def plant_step(self, x, u, sig_zeta=None, eps_x=None, eps_y=None, y_out=None, observe_state=False, z_ref=None, cost=None,
                   plant_params=None):
        """One step of B noisy plants on the device (i2c_plant_step): the host code between two control steps of a closed loop
        (mpc_quad.py:643-660). x: [nx][B] tensor, the true states, UPDATED IN PLACE; u: [nu][B] tensor, the action (e.g. the
        transposed first result of mpc_step). eps_x [nx][B] / eps_y [ny][B]: standard-normal samples or None (no noise of that
        kind). cost: optional (B,) tensor the stage cost (z - z_ref)^T QR (z - z_ref) is ADDED to; z_ref [nz][B] or None (sys.zg);
        z = observe(x, u) of the action as given (the dynamics clip it themselves, the cost does not: clip u first for that).
        observe_state=True: the belief mean x0 takes the new state and nothing is measured (MpcPolicy.__call__(i, x)); otherwise
        returns the measurement y [ny][B] (written into y_out when given) for the next mpc_step(y=..., u=...).
        plant_params: (B, NP) parameters of the plants when they differ from the planner's model."""
        nx, nu, ny, B = self.nx, self.nu, self.dims.ny, self.B
        assert x.shape == (nx, B) and x.is_contiguous() and x.dtype == self.dtype and x.device.type == self.device.type
        assert u.shape == (nu, B) and u.dtype == self.dtype
        u = u.contiguous()
        chk = lambda t, n: None if t is None else t.to(self.dtype).reshape(n, B).contiguous()  # noqa: E731
        eps_x, eps_y, z_ref = chk(eps_x, nx), chk(eps_y, ny), chk(z_ref, self.nz)
        if observe_state:
            assert eps_y is None and y_out is None, "nothing is measured in the fully observed mode"
        elif y_out is None:
            y_out = torch.empty(ny, B, dtype=self.dtype, device=self.device)
        if y_out is not None:
            assert y_out.shape == (ny, B) and y_out.is_contiguous() and y_out.dtype == self.dtype
        if cost is not None:
            assert cost.shape == (B,) and cost.is_contiguous() and cost.dtype == self.dtype
        problem, plant = self._plant_problem(plant_params)
        self._call("i2c_plant_step", self._sig_zeta(sig_zeta, eps_y is not None), x, u, eps_x, eps_y, y_out,
                   self.x0 if observe_state else None, z_ref, cost, problem=problem)
        self.belief_revision += bool(observe_state)
        return y_out

    def run_closed_loop(self, n_steps, n_iter, sig_zeta=None, x_true=None, process_noise=True, measurement_noise=True,
                        generator=None, plant_params=None, z_traj=None, observe_state=False, keep=("x", "u"), eps_x=None, eps_y=None):
        """A closed-loop MPC episode of n_steps control steps in ONE library call (i2c_mpc_episode), no host round trip: per step
        mpc_step(n_iter) -- with the cubature Kalman filter on the last measurement and action from the second step on -- then
        the noisy plants (plant_step). The loop of scripts/mpc_state_est/mpc_quad.py:643-660 for B systems at once.
          x_true            (B, nx) / (nx,) true initial states; None: the belief mean x0
          process_noise / measurement_noise   draw eps_x (N, nx, B) / eps_y (N, ny, B) with torch.randn(generator=generator) on the
                            engine's device (a seed reproduces an episode); eps_x / eps_y: use these samples instead
          sig_zeta          (ny, ny) measurement noise of the filter and the plant; None: sys.sig_zeta
          plant_params      (B, NP): the plants' parameters where they differ from the planner's model
          z_traj            (n_z, nz) or (B, n_z, nz) reference from THIS step on: row min(k, n_z - 1) prices step k, row
                            min(k + T, n_z - 1) is the target of the cell appended at step k (mpc.py:177-181). An engine without
                            per-cell targets gets rows 0 .. T-1 as its horizon's first; one that has them keeps its own.
                            None: the cost reference is sys.zg and an appended cell repeats the last target
          observe_state     fully observed loop (MpcPolicy.__call__(i, x)): the belief mean is the plant's state, no filter
          keep              which histories to return, of "x", "u", "y", "mu"
        Returns a dict of device tensors: x (B, N, nx) states before each step, u (B, N, nu), y (B, N, ny) measurements after
        each step, mu (B, N, nx) belief means the plans started from (as kept); cost (B,) summed tracking cost; x_true (B, nx)
        final states; eps_x / eps_y as used. The ring (t0, terminal_cell) is advanced as n_steps calls of mpc_step would.
        u and the cost are of the action AS PLANNED: the models' dynamics clip it to the actuator limits themselves, observe(x, u)
        does not, where the reference's loop clips first and records / prices the clipped action (mpc_quad.py:645-647, 659). They
        agree whenever the plan respects the limits.
        A trajectory that fails numerically is flagged in status (failures()); its rows go non-finite, the others are untouched."""
        self._no_horizons("run_closed_loop()")
        assert self.prior is self.post, "run_closed_loop() between a sweep and its update_priors()"
        N, B, T, dev, dt = int(n_steps), self.B, self.H, self.device, self.dtype
        nx, nu, nz, ny = self.nx, self.nu, self.nz, self.dims.ny
        unknown = set(keep) - {"x", "u", "y", "mu"}
        if unknown or (observe_state and "y" in keep):
            raise ValueError(f"keep={keep!r}: any of 'x', 'u', 'y', 'mu' ('y' only when the state is not observed)")
        eps_x = self._noise(eps_x, (N, nx, B), process_noise, generator)
        eps_y = None if observe_state else self._noise(eps_y, (N, ny, B), measurement_noise, generator)
        x = self.x0.clone() if x_true is None else self._state_rows(x_true, nx)
        zt = None
        if z_traj is not None:
            z = np.asarray(z_traj, np.float64)
            z = np.broadcast_to(z if z.ndim == 3 else z[None], (B, z.shape[-2], nz))
            if self.z is None:
                self.set_targets(z[:, np.minimum(np.arange(T), z.shape[1] - 1)])
            zt = torch.as_tensor(np.array(np.transpose(z, (1, 2, 0)), order="C"), dtype=dt, device=dev)
        st = _native.I2cMpcStep()
        self._fill_mpc_step(st, n_iter, self._sig_zeta(sig_zeta, not observe_state))
        if self._loop_yu is None:
            self._loop_yu = torch.zeros(ny + nu, B, dtype=dt, device=dev)
        hist = {k: torch.empty(N, n, B, dtype=dt, device=dev) if k in keep else None
                for k, n in (("x", nx), ("u", nu), ("y", ny), ("mu", nx))}
        cost = torch.zeros(B, dtype=dt, device=dev)
        plant = None if plant_params is None else self._params_to_device(plant_params)
        ep = _native.I2cEpisode()
        ep.n_steps, ep.observe_state, ep.n_z = N, int(bool(observe_state)), 0 if zt is None else int(zt.shape[0])
        ep.x_true, ep.eps_x, ep.eps_y, ep.plant_params_b, ep.z_traj = x.data_ptr(), _addr(eps_x), _addr(eps_y), _addr(plant), _addr(zt)
        ep.y, ep.u = self._loop_yu[:ny].data_ptr(), self._loop_yu[ny:].data_ptr()
        ep.x_hist, ep.u_hist, ep.y_hist, ep.mu_hist = _addr(hist["x"]), _addr(hist["u"]), _addr(hist["y"]), _addr(hist["mu"])
        ep.cost = cost.data_ptr()
        ep.t0_out, ep.terminal_cell_out = int(self.t0), int(self.terminal_cell)
        try:
            self._call("i2c_mpc_episode", C.byref(st), C.byref(ep))
        finally:  # where the call reports the ring, also after an error part-way
            self.belief_revision += 1
            self.t0, self.terminal_cell = int(ep.t0_out), int(ep.terminal_cell_out)
            self.sync_problem()
        out = {k: v.permute(2, 0, 1) for k, v in hist.items() if v is not None}
        out.update(cost=cost, x_true=x.T, eps_x=eps_x, eps_y=eps_y)
        return out

    def set_targets(self, z_traj):
        """Per-cell targets (mpc.py:29-31): z_traj (T, nz) or (B, T, nz)."""
        z = np.broadcast_to(np.asarray(z_traj, np.float64), (self.B, self.H, self.nz))
        zt = torch.as_tensor(np.array(np.transpose(z, (1, 2, 0)), order="C"), dtype=self.dtype, device=self.device)
        if self.t0:
            zt = torch.roll(zt, self.t0, 0)  # cell order -> ring rows
        self._install("z", zt.contiguous())

    def set_cell_target(self, t, value):
        """cells[t].z = value (mpc.py:29-31): the target of ONE cell, (nz, 1) or (B, nz). An engine without per-cell targets gets
        them here, every other cell with the model's goal."""
        if self.z is None:
            self.set_targets(self.zg)
        v = torch.as_tensor(np.asarray(value, dtype=float).reshape(-1, self.nz).T, dtype=self.dtype, device=self.device)
        self.z[(int(t) + self.t0) % self.H] = v.expand(self.nz, self.B)
        self.revision += 1

    def rollout(self, n_rollouts=1, policy="linear", process_noise=True, action_noise=False, sample_x0=False,
                generator=None, want=("xu", "z", "x_final", "z_term"), eps_x0=None, eps_x=None, eps_u=None, model_params=None):
        """Simulate the current controllers through the noisy model (env.batch_eval, i2c/env.py:93-103):
        n_rollouts per trajectory, all B * n_rollouts in one launch. Returns a dict of (R, B, T, ...) tensors.
        The standard-normal disturbances are drawn here (torch.randn) unless given: eps_x0 [nx][N], eps_x [T][nx][N],
        eps_u [T][nu][N] with N = n_rollouts * B, rollout n = r * B + b.
        model_params: (B, NP) parameters of the PLANT for this rollout only (rollout n simulates row n % B), e.g. controllers
        planned on the nominal model evaluated on perturbed ones; None = the planning parameters."""
        N, T, dev, dt = int(n_rollouts) * self.B, self.H, self.device, self.dtype
        code = POLICY_CODES[policy]
        eps_x0 = self._noise(eps_x0, (self.nx, N), sample_x0, generator)
        eps_x = self._noise(eps_x, (T, self.nx, N), process_noise, generator)
        eps_u = self._noise(eps_u, (T, self.nu, N), action_noise, generator)
        shapes = {"xu": (T, self.d, N), "z": (T, self.nz, N), "x_final": (self.nx, N), "z_term": (self.nzt, N)}
        out = {k: torch.empty(*s, dtype=dt, device=dev) if (k in want and s[-2] > 0) else None for k, s in shapes.items()}
        problem, plant = self._plant_problem(model_params)
        self._call("i2c_rollout", self.post, int(n_rollouts), code, eps_x0, eps_x, eps_u, out["xu"], out["z"], out["x_final"],
                   out["z_term"], problem=problem)
        R_, B = int(n_rollouts), self.B
        res = {"eps_x0": eps_x0, "eps_x": eps_x, "eps_u": eps_u}
        for k, v in out.items():
            if v is None:
                res[k] = None
            elif v.dim() == 3:
                res[k] = v.reshape(T, v.shape[1], R_, B).permute(2, 3, 0, 1)  # (R, B, T, n)
            else:
                res[k] = v.reshape(v.shape[0], R_, B).permute(1, 2, 0)  # (R, B, n)
        return res

    def evaluate(self, n_rollouts, policy="linear", process_noise=True, action_noise=False, sample_x0=False, seed=0, moments=True,
                 parts=None, first_trajectory=0, model_params=None, eps_x0=None, eps_x=None, eps_u=None, percentiles=(10, 90)):
        """Monte-Carlo evaluation of the current controllers on the device (`i2c_rollout_eval`): n_rollouts simulations of every
        trajectory through the noisy plant with noise drawn in the kernel (Philox4x32-10 keyed by `seed`, counter = (first_trajectory
        + b, r, t, kind): include/i2c_hip.h), reduced there to
            cost (R, B), cost_mean / cost_var (unbiased) / cost_min / cost_max (B,), cost_percentiles (len(percentiles), B)
            (torch.quantile, linear interpolation as np.percentile), n_bad (B,) int32: rollouts with a non-finite cost (their
            trajectory's statistics are NaN), xu_mean (B, T, d) and xu_cov (B, T, d, d) of (x_t, u_t) over the rollouts (None with
            moments=False; rows beyond a trajectory's horizon are NaN: valid_cells()), parts: lanes per trajectory that summed them.
        The cost is the problem's quadratic cost over all T_b steps plus the Qf term (i2c.utils.quadratic_trajectory_cost), NOT the
        reference evaluator's convention. eps_x0 / eps_x / eps_u: GIVEN standard normals in i2c_rollout's layouts, each switching
        its kind on and replacing the generator for it. model_params: (B, NP) plants for this call only, as in rollout().
        A sharded caller passes first_trajectory = dist.shard_range(...)[0] and gets the draws of the unsharded batch."""
        R_, B, T, dev, dt = int(n_rollouts), self.B, self.H, self.device, self.dtype
        if policy not in POLICY_CODES:
            raise ValueError(f"policy must be linear, expert_soft or expert_hard, got {policy!r}")
        code = POLICY_CODES[policy]
        if R_ < 1 or R_ >= 2 ** 31:
            raise ValueError(f"n_rollouts must be in [1, 2^31), got {n_rollouts}")
        if self.mixed or dt != torch.float64:
            raise ValueError("evaluate() needs an fp64 engine: the sums are fp64")
        P = 0 if parts is None else int(parts)
        if parts is not None and not 1 <= P <= R_:
            raise ValueError(f"parts must be in [1, n_rollouts = {R_}], got {parts}")
        first = int(first_trajectory)
        if first < 0 or first + B > 2 ** 32:
            raise ValueError(f"first_trajectory + B must fit 32 bits, got {first_trajectory} + {B}")
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed must be in [0, 2^64), got {seed}")
        qs = [float(q) for q in percentiles]
        if any(not 0.0 <= q <= 100.0 for q in qs):
            raise ValueError(f"percentiles must be in [0, 100], got {percentiles}")
        N = R_ * B
        eps_x0, eps_x, eps_u = self._noise(eps_x0, (self.nx, N)), self._noise(eps_x, (T, self.nx, N)), self._noise(eps_u, (T, self.nu, N))
        problem, plant = self._plant_problem(model_params)
        ev = _native.I2cRolloutEval()
        ev.n_rollouts, ev.policy, ev.parts, ev.seed, ev.first_trajectory = R_, code, P, seed, first
        ev.noise = ((_native.NOISE_PROCESS if process_noise else 0) | (_native.NOISE_ACTION if action_noise else 0) |
                    (_native.NOISE_X0 if sample_x0 else 0))
        ev.eps_x0, ev.eps_x, ev.eps_u = _addr(eps_x0), _addr(eps_x), _addr(eps_u)
        got = C.c_int32(0)
        nbytes = self.lib.i2c_rollout_eval_workspace(C.byref(problem), C.byref(ev), C.byref(got))
        if nbytes == 0:
            raise ValueError("i2c_rollout_eval_workspace refused the request (see include/i2c_hip.h)")
        cost = torch.empty(R_, B, dtype=dt, device=dev)
        stats = torch.empty(4, B, dtype=dt, device=dev)
        n_bad = torch.empty(B, dtype=torch.int32, device=dev)
        xu_mean = xu_cov = None
        if moments:
            if self._eval_work is None or self._eval_work.numel() != nbytes // 8:  # kept between calls of one shape
                self._eval_work = torch.empty(nbytes // 8, dtype=dt, device=dev)
            new = torch.empty if self._horizons is None else (lambda *s, **k: torch.full(s, float("nan"), **k))
            xu_mean = new(T, self.d, B, dtype=dt, device=dev)
            xu_cov = new(T, sym_size(self.d), B, dtype=dt, device=dev)
            ev.work, ev.xu_mean, ev.xu_cov = self._eval_work.data_ptr(), xu_mean.data_ptr(), xu_cov.data_ptr()
        ev.cost, ev.cost_stats, ev.n_bad = cost.data_ptr(), stats.data_ptr(), n_bad.data_ptr()
        self._call("i2c_rollout_eval", self.post, C.byref(ev), problem=problem)
        q = torch.as_tensor(qs, dtype=dt, device=dev) / 100.0
        return {
            "cost": cost, "cost_mean": stats[0], "cost_var": stats[1], "cost_min": stats[2], "cost_max": stats[3],
            "cost_percentiles": self._cost_quantiles(cost, q),
            "n_bad": n_bad,
            "xu_mean": None if xu_mean is None else xu_mean.permute(2, 0, 1),
            "xu_cov": None if xu_cov is None else unpack_sym(xu_cov.permute(2, 0, 1), self.d),
            "parts": int(got.value),
        }

    @staticmethod
    def _cost_quantiles(cost, q):
        """Quantiles q (in [0, 1]) over the rollouts of cost (R, B), linear interpolation between order statistics."""
        if q.numel() == 0:
            return cost.new_empty(0, cost.shape[1])
        if cost.numel() <= 2 ** 24:  # (torch.quantile's input limit)
            return torch.quantile(cost, q, dim=0)
        s, pos = cost.sort(0).values, q * (cost.shape[0] - 1)
        lo = pos.floor().long()
        hi = (lo + 1).clamp(max=cost.shape[0] - 1)
        return s[lo] + (s[hi] - s[lo]) * (pos - lo.to(pos.dtype))[:, None]

    def _terminal_kl(self):
        """mvn_kl_divergence(x3_pf[T-1] || terminal prior) (i2c.py:1012-1019, 1223-1229)."""
        nx = self.nx
        if self.prop is not None and self._propagate:
            return self.prop_stats[2].to(torch.float64).clone()  # computed by k_propagate for the state it just propagated
        if self.prop is None:
            mu1 = self.x0.T.to(torch.float64)
            sig1 = unpack_sym(self.sig_x0.T.to(torch.float64), nx)
        else:
            o = self.d + sym_size(self.d)
            if self._horizons is None:
                last = self.prop[-1]
            else:  # each trajectory's own last cell
                last = self.prop[self._horizons.long() - 1, :, torch.arange(self.B, device=self.device)].T
            mu1 = last[o: o + nx, :].T.to(torch.float64)
            sig1 = unpack_sym(last[o + nx: o + nx + sym_size(nx), :].T.to(torch.float64), nx)
        mu2 = torch.as_tensor(self.mu_x_terminal, dtype=torch.float64, device=self.device)
        sig2 = torch.as_tensor(self.sig_x_terminal, dtype=torch.float64, device=self.device)
        diff = mu2 - mu1
        dist = (diff * torch.linalg.solve(sig2, diff.T).T).sum(-1)
        log_det_ratio = torch.log(torch.linalg.det(sig2) / torch.linalg.det(sig1))
        trace_ratio = torch.diagonal(torch.linalg.solve(sig2, sig1), dim1=-2, dim2=-1).sum(-1)
        return 0.5 * (log_det_ratio + trace_ratio + dist - nx)

    # ------------------------------------------------------------------ the engine's state: checkpoint and snapshot
    # THE list of what persists between calls. A new persistent buffer is added here and nowhere else.
    _STATE_TENSORS = ("post", "alpha", "temp", "feedforward", "status", "x0", "sig_x0", "cell_init")
    _STATE_OPTIONAL = ("z", "alpha_cell", "alpha_init", "expert_cells")  # None until their setter has allocated them
    _STATE_LISTS = ("alphas", "alphas_desired", "alphas_pf", "costs_m", "costs_m_var", "costs_pf", "costs_pf_var", "kl_terms")
    _SNAPSHOT = ("post", "alpha", "alpha_cell", "feedforward", "x0", "sig_x0", "z")  # what restore() puts back (of the two above)

    def state_dict(self):
        """Everything a resumed EM or MPC run needs, as host tensors and plain scalars: posterior / prior state, temperatures (per
        trajectory and per cell), the belief x0 / sig_x0, per-cell targets, mode flags, the ring (t0, terminal_cell), tau, and the
        metric histories. `prior` differs from `post` only when saved between a sweep and its update_priors()."""
        host = lambda t: t.detach().cpu().clone()  # noqa: E731
        sd = {k: host(getattr(self, k)) for k in self._STATE_TENSORS}
        sd["prior"] = host(self.prior)
        for k in self._STATE_OPTIONAL:
            v = getattr(self, k)
            sd[k] = None if v is None else host(v)
        for k in self._STATE_LISTS:
            sd[k] = [host(t) for t in getattr(self, k)]
        sd.update(em_iter=self.em_iter, tau=self.tau, terminal_cell=self.terminal_cell, t0=self.t0, propagate=bool(self._propagate),
                  use_expert_controller=bool(self.use_expert_controller), horizon=self.H, batch=self.B)
        return sd

    def load_state_dict(self, sd):
        """The inverse of state_dict(), on an engine of the same problem. Optional buffers the checkpoint has and this engine has
        not are allocated through their setters."""
        if (sd["horizon"], sd["batch"]) != (self.H, self.B):
            raise ValueError("checkpoint is for another problem (model / horizon / batch)")
        for k in self._STATE_TENSORS:
            getattr(self, k).copy_(sd[k])
        self._fold_posterior()
        if not torch.equal(sd["prior"], sd["post"]):  # saved between a sweep and its update_priors()
            self._split_posterior()
            self.post.copy_(sd["post"])
            self.prior.copy_(sd["prior"])
        if sd["alpha_cell"] is not None:
            self.enable_per_cell_alpha()
        if sd.get("expert_cells") is not None and self.expert_cells is None:
            self.set_cell_expert(0, self.use_expert_controller)
        if sd["z"] is not None and self.z is None:
            self.set_targets(np.transpose(sd["z"].double().numpy(), (2, 0, 1)))
        for k in self._STATE_OPTIONAL:
            if sd.get(k) is not None:
                getattr(self, k).copy_(sd[k])
        for k in self._STATE_LISTS:
            setattr(self, k, [t.to(self.device) for t in sd[k]])
        self.em_iter, self.tau, self.terminal_cell, self.t0 = int(sd["em_iter"]), int(sd["tau"]), int(sd["terminal_cell"]), int(sd["t0"])
        self._propagate, self.use_expert_controller = bool(sd["propagate"]), bool(sd["use_expert_controller"])
        self.refresh_problem()
        self.revision += 1
        self.belief_revision += 1

    def snapshot(self):
        """A device-side copy of the solver state an MPC episode changes (MpcPolicy takes one at construction): the buffers of
        _SNAPSHOT that exist, in physical row order, and the ring they are valid with."""
        snap = {k: getattr(self, k).clone() for k in self._SNAPSHOT if getattr(self, k) is not None}
        snap.update(t0=self.t0, terminal_cell=self.terminal_cell)
        return snap

    def restore(self, snap):
        """Back to snapshot(): the buffers it holds, the ring, prior and posterior one buffer again, the status words cleared. NOT
        restored: `temp`, `cell_init` and the metric histories (an episode does not change the first two and keeps the last)."""
        self._fold_posterior()
        for k in self._SNAPSHOT:
            if k in snap:
                getattr(self, k).copy_(snap[k])
        self.status.zero_()
        self.t0, self.terminal_cell = snap["t0"], snap["terminal_cell"]  # rows were cloned in physical order, at this offset of the ring
        self.sync_problem()
        self.revision += 1
        self.belief_revision += 1

    def clear_history(self, names=("costs_m", "costs_m_var", "costs_pf", "costs_pf_var", "kl_terms")):
        """Start the named history lists afresh (default: the cost lists and the KL terms, what I2cGraph.reset_metrics clears; the
        three temperature lists go on)."""
        for k in names:
            assert k in self._STATE_LISTS, k
            setattr(self, k, [])

    # ------------------------------------------------------------------ failure reporting
    def failures(self, status=None):
        """Per-trajectory status words (reason << 16 | cell + 1; 0 = fine) -> list of (b, reason, t) for failed trajectories.
        status: a host copy of the words someone already fetched (iteration_health); default: read them now."""
        status = self.status.cpu().numpy() if status is None else status
        return [(int(b), int(s) >> 16, (int(s) & 0xFFFF) - 1) for b, s in enumerate(status) if s != 0]

    def raise_on_failure(self, status=None):
        """With B == 1 behave like the reference: raise; batched callers read `failures()`."""
        f = self.failures(status)
        if f:
            b, reason, t = f[0]
            raise I2cNumericalError(f"trajectory {b}, cell {t}: {_native.FAIL_REASONS.get(reason, reason)}")

    def iteration_health(self):
        """(status (B,) int32, alpha_hat of the last M-step (B,) float64) on the host after ONE stream synchronisation: what a
        single-trajectory caller checks after every EM iteration (the reference raises inside the iteration: LinAlgError from a
        Cholesky, "Alpha is NaN" from update_alpha, i2c.py:948-951). Two asynchronous copies into page-locked host memory, which the
        next call reuses: the arrays returned are copies the caller owns."""
        a = self.alphas_desired[-1]
        if self.device.type != "cuda":
            return self.status.numpy().copy(), a.to(torch.float64).numpy().copy()
        if self._health is None:
            self._health = (torch.empty(self.B, dtype=torch.int32).pin_memory(), torch.empty(self.B, dtype=self.dtype).pin_memory())
        hs, ha = self._health
        hs.copy_(self.status, non_blocking=True)
        ha.copy_(a, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return hs.numpy().copy(), ha.numpy().astype(np.float64)  # (astype copies)

    # ------------------------------------------------------------------ getters: (B, T, ...) tensors
    def _rows(self, buf, lo, n):
        if buf is self.post or buf is self.prior:  # ring buffers: back to cell order
            buf = self.cells(buf)
        return buf[:, lo: lo + n, :].permute(2, 0, 1)  # (B, T, n)

    def _sym_rows(self, buf, lo, n):
        return unpack_sym(self._rows(buf, lo, sym_size(n)), n)

    def marginal_state_action(self):
        """(mu_xu0_m (B,T,d), sig_xu0_m (B,T,d,d)): i2c.py:1300-1304."""
        return self._rows(self.post, 0, self.d), self._sym_rows(self.post, self.d, self.d)

    def local_linear_policy(self):
        """(K (B,T,nu,nx), k (B,T,nu), sigK (B,T,nu,nu)): i2c.py:1253-1264."""
        o = self.d + sym_size(self.d)
        K = self._rows(self.post, o, self.nu * self.nx).reshape(self.B, self.H, self.nu, self.nx)
        k = self._rows(self.post, o + self.nu * self.nx, self.nu)
        sigK = self._sym_rows(self.post, o + self.nu * self.nx + self.nu, self.nu)
        return K, k, sigK

    def forward_messages(self):
        d, nx = self.d, self.nx
        o = d + sym_size(d)
        fwd = self.fwd.permute(0, 2, 1) if self.fwd_trajectory_major else self.fwd  # [T][e_fwd][B] either way
        return dict(
            mu_xu1_f=self._rows(fwd, 0, d),
            sig_xu1_f=self._sym_rows(fwd, d, d),
            mu_x3_f=self._rows(fwd, o, nx),
            sig_x3_f=self._sym_rows(fwd, o + nx, nx),
            J_dyn=self._rows(fwd, o + nx + sym_size(nx), d * nx).reshape(self.B, self.H, d, nx),
        )

    def smoothed_next_state(self):
        assert self.xm is not None, "constructed with keep_xm=False"
        return self._rows(self.xm, 0, self.nx), self._sym_rows(self.xm, self.nx, self.nx)

    def observed_marginal(self):
        """(mu_z0_m (B,T,nz), sig_z0_m (B,T,nz,nz)) (i2c.py:594-596, 1312-1314)."""
        assert self.zpost is not None, "constructed with keep_zpost=False"
        return self._rows(self.zpost, 0, self.nz), self._sym_rows(self.zpost, self.nz, self.nz)

    def terminal_observed_marginal(self):
        if not self.has_Qf:
            return None, None
        nzt = self.nzt
        return self.term_stats[3: 3 + nzt].T, unpack_sym(self.term_stats[3 + nzt: 3 + nzt + sym_size(nzt)].T, nzt)

    def prior_state_action(self):
        assert self.prior_out is not None, "constructed with keep_prior=False"
        return self._rows(self.prior_out, 0, self.d), self._sym_rows(self.prior_out, self.d, self.d)

    def propagated(self):
        d, nx = self.d, self.nx
        o = d + sym_size(d)
        return dict(
            mu_xu0_pf=self._rows(self.prop, 0, d),
            sig_xu0_pf=self._sym_rows(self.prop, d, d),
            mu_x3_pf=self._rows(self.prop, o, nx),
            sig_x3_pf=self._sym_rows(self.prop, o + nx, nx),
        )

    # ------------------------------------------------------------------ history helpers
    @staticmethod
    def history(lst):
        """list of (B,) device tensors -> (n, B) float64 numpy (one host sync)."""
        if not lst:
            return np.zeros((0, 0))
        return torch.stack([x.to(torch.float64) for x in lst]).cpu().numpy()
