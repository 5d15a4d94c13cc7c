"""Per-trajectory model parameters (BatchedI2c(model_params=...), I2cProblem.model_params_b): B trajectories of DIFFERENT plants in
one solve. Every trajectory must compute what a solve of its own model copy (shared parameters) computes, on every kernel family;
the host simulation checks the kernel math here, the `gpu` tests the same comparisons on the MI355X."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import assert_close

pkg = parity.pkg
from i2c.known_models import make_env_model  # noqa: E402

_native = pkg._native
OUTPUTS = ("mu", "sig", "K", "k", "alpha", "mu_x3_f", "sig_x3_f", "xm", "sig_xm")


@pytest.fixture(scope="module")
def lib():
    return hostsim.load()


# ---- models, their parameter rows and model copies ------------------------------------------------------------------------
def with_params(model, row):
    """A copy of `model` whose device parameters (and NumPy dynamics) are `row`."""
    m = copy.deepcopy(model)
    row = np.asarray(row, np.float64)
    name = type(model).__name__
    if name in ("LinearExact", "LinearMinimumEnergy"):
        m.A, m.B, m.a = row[:4].reshape(2, 2), row[4:6].reshape(2, 1), row[6:8].reshape(2, 1)
    elif name == "PlanarQuadrotor":
        m.mass, m.inertia, m.force_mx = row
    elif name == "Quadrotor12":
        m.mass, m.Ixx, m.Iyy, m.Izz, m.force_mx = row
    else:  # an out-of-tree model: only the device functor reads the parameters
        m.device_params = lambda r=tuple(row): list(r)
    assert np.array_equal(np.asarray(m.device_params(), np.float64), row)
    return m


def param_rows(model, n, seed):
    """n distinct parameter rows around the model's own."""
    rng = np.random.default_rng(seed)
    base = np.asarray(model.device_params(), np.float64)
    name = type(model).__name__
    if name in ("LinearExact", "LinearMinimumEnergy"):
        rows = base + 0.02 * rng.normal(size=(n, base.size))
    elif name == "PlanarQuadrotor":  # mass, inertia +/- 20 %, thrust limit
        rows = base * np.column_stack((rng.uniform(0.8, 1.2, n), rng.uniform(0.8, 1.2, n), rng.uniform(0.9, 1.1, n)))
    elif name == "Quadrotor12":
        rows = base * np.column_stack([rng.uniform(0.8, 1.2, n) for _ in range(4)] + [rng.uniform(0.9, 1.1, n)])
    else:  # Van der Pol: mu, dt, u_max
        rows = base * np.column_stack((rng.uniform(0.5, 1.5, n), rng.uniform(0.9, 1.1, n), rng.uniform(0.9, 1.1, n)))
    return rows


def problem(model, T):
    """Cost and priors of a small problem of each model (the same x0 and action prior for every trajectory: the trajectories
    differ by their parameters only)."""
    name = type(model).__name__
    nx, nu = model.dim_x, model.dim_u
    if name == "LinearExact":
        return dict(Q=10.0 * np.eye(2), R=np.eye(1), Qf=10.0 * np.eye(2), alpha=800.0, tol=0.0, mu_u=np.zeros((T, 1)),
                    sig_u=np.eye(1), x0=np.array([5.0, 5.0]))
    if name == "PlanarQuadrotor":
        return dict(Q=np.diag([10.0, 10.0, 1.0, 0.1, 0.1, 0.1]), R=1e-2 * np.eye(2), Qf=np.diag([10.0, 10.0, 1.0, 0.1, 0.1, 0.1]),
                    alpha=1.0, tol=0.5, mu_u=np.full((T, 2), 0.5 * type(model)().gravity), sig_u=1e-2 * np.eye(2),
                    x0=np.asarray(model.x0, float).reshape(-1))
    if name == "Quadrotor12":
        return dict(Q=np.diag([10.0] * 3 + [1.0] * 3 + [0.1] * 6), R=1e-2 * np.eye(4), Qf=np.diag([10.0] * 3 + [1.0] * 3 + [0.1] * 6),
                    alpha=1.0, tol=0.5, mu_u=np.full((T, 4), 0.25 * type(model)().gravity), sig_u=1e-2 * np.eye(4), x0=np.zeros(12))
    if name == "PendulumKnown":
        return dict(Q=np.diag([1.0, 100.0, 1.0]), R=np.diag([2.0]), Qf=np.diag([1.0, 100.0, 1.0]), alpha=100.0, tol=0.0,
                    mu_u=np.zeros((T, 1)), sig_u=2.0 * np.eye(1), x0=np.array([np.pi, 0.0]))
    return dict(Q=np.diag([10.0, 1.0, 5.0]), R=np.diag([0.5]), Qf=np.diag([20.0, 2.0]), alpha=2.0, tol=0.5,
                mu_u=np.zeros((T, nu)), sig_u=0.5 * np.eye(nu), x0=np.array([1.0, 0.0]))


def linear_model():
    """LinearKnown with the noise level of the golden EM case (tests/golden/em_linear_T60: 1e-4)."""
    m = make_env_model("LinearKnown")
    m.sig_x0, m.sig_eta = 1e-4 * np.eye(2), 1e-4 * np.eye(2)
    return m


def engine(model, B, T, lib, device, model_params=None, **kw):
    p = problem(model, T)
    x0 = np.tile(p["x0"], (B, 1))
    mu_u = np.broadcast_to(p["mu_u"], (B, T, model.dim_u))
    return pkg.BatchedI2c(model, T, p["Q"], p["R"], p["Qf"], p["alpha"], p["tol"], mu_u, p["sig_u"], x0=x0, device=device, lib=lib,
                          model_params=model_params, **kw)


def solve(eng, n_iters):
    for _ in range(n_iters):
        eng.learn_msgs()
    if eng.device.type == "cuda":
        torch.cuda.synchronize()
    assert eng.failures() == []
    return outputs(eng)


def outputs(eng):
    mu, sig = eng.marginal_state_action()
    K, k, _ = eng.local_linear_policy()
    f = eng.forward_messages()
    xm, sxm = eng.smoothed_next_state()
    return {n: parity.np_(v) for n, v in dict(mu=mu, sig=sig, K=K, k=k, alpha=eng.alpha, mu_x3_f=f["mu_x3_f"], sig_x3_f=f["sig_x3_f"],
                                              xm=xm, sig_xm=sxm).items()}


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def check_rows(out, ref, rows, tol, what):
    """out: outputs of the per-trajectory engine; ref[j]: outputs whose trajectory rows[b] == j ... see callers."""
    for n in OUTPUTS:
        for b, (r, rb) in enumerate(rows):
            assert rel(out[n][b], ref[r][n][rb]) <= tol, f"{what}: {n} of trajectory {b}: {rel(out[n][b], ref[r][n][rb]):.2e} > {tol:.0e}"


def compare_with_copies(model, B, T, n_iters, lib, device, tol, n_sets=None, seed=0, **kw):
    """A per-trajectory solve of B trajectories against solves of each distinct parameter row on its own (shared parameters, the
    same batch size and kernel options, so the same family): trajectory b of both must agree to `tol`.
    n_sets = None: B distinct rows, each reference a B = 1 solve; otherwise n_sets rows dealt over the batch, each reference a solve of
    the whole batch with that row. Returns the per-trajectory outputs and the parameter rows."""
    if n_sets is None:
        rows = param_rows(model, B, seed)
        params, which = rows, np.arange(B)
    else:
        rows = param_rows(model, n_sets, seed)
        which = np.random.default_rng(seed + 1).integers(0, n_sets, B)
        which[:n_sets] = np.arange(n_sets)
        params = rows[which]
    eng = engine(model, B, T, lib, device, model_params=params, **kw)
    out = solve(eng, n_iters)
    if n_sets is None:
        ref = [solve(engine(with_params(model, rows[j]), 1, T, lib, device, **kw), n_iters) for j in range(B)]
        check_rows(out, ref, [(b, 0) for b in range(B)], tol, f"{type(model).__name__} B={B}")
    else:
        ref = [solve(engine(with_params(model, rows[j]), B, T, lib, device, **kw), n_iters) for j in range(n_sets)]
        check_rows(out, ref, [(int(which[b]), b) for b in range(B)], tol, f"{type(model).__name__} B={B}")
    return eng, out, params


def assert_params_matter(out, params, tol):
    """Guard: the parameter rows change the solved controllers by far more than the comparison tolerance."""
    K = out["K"].reshape(out["K"].shape[0], -1)
    _, first = np.unique(params, axis=0, return_index=True)
    first = np.sort(first)
    for i in first:
        for j in first:
            if i < j:
                assert rel(K[i], K[j]) > 1e3 * tol, f"trajectories {i} and {j}: controllers differ by {rel(K[i], K[j]):.1e} only"


# ---- host simulation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inference,kw", [("cubature", {}), ("linearize", {}), ("gauss_hermite", {"gh_degree": 3})])
def test_linear_per_trajectory_vs_model_copies(lib, inference, kw):
    model = linear_model()
    eng, out, params = compare_with_copies(model, 6, 20, 3, lib, "cpu", 1e-12, inference=inference, **kw)
    assert eng.forward_family == "lane"
    assert_params_matter(out, params, 1e-12)


def test_linear_per_trajectory_vs_oracle(lib):
    from oracle.i2c_numpy import CubatureRule, I2cOracle
    from oracle.models_numpy import make_model

    model, T, B = linear_model(), 20, 6
    eng, out, params = compare_with_copies(model, B, T, 3, lib, "cpu", 1e-12)
    p = problem(model, T)
    for b in range(B):
        om = make_model("LinearKnown", noise=1e-4)
        om.A, om.B, om.a = params[b, :4].reshape(2, 2), params[b, 4:6].reshape(2, 1), params[b, 6:8].copy()
        ora = I2cOracle(om, T, p["Q"], p["R"], p["Qf"], p["alpha"], p["tol"], p["mu_u"][None], p["sig_u"], rule=CubatureRule(1, 0, 0),
                        x0=p["x0"][None])
        for _ in range(3):
            ora.learn_msgs()
        parity.close(out["mu"][b], ora.mu_xu0_m[0], 1e-8, "mu_xu0_m")
        parity.close(out["sig"][b], ora.sig_xu0_m[0], 1e-8, "sig_xu0_m")
        parity.close(out["K"][b], ora.K[0], 1e-8, "K")
        parity.close(out["k"][b], ora.k[0], 1e-8, "k")
        assert_close(out["alpha"][b], ora.alpha[0], 1e-8, "alpha")


QUAD_FORMS = [dict(deterministic_family=True), dict(group_lanes=64)]  # lane family (fused walk), quad forward + backward


@pytest.mark.parametrize("kw", QUAD_FORMS, ids=["lane", "quad"])
def test_planar_quadrotor_per_trajectory_vs_model_copies(lib, kw):
    model = make_env_model("PlanarQuadrotor")
    eng, out, params = compare_with_copies(model, 5, 12, 3, lib, "cpu", 1e-12, **kw)
    assert eng.forward_family == ("quad" if "group_lanes" in kw else "lane")
    assert_params_matter(out, params, 1e-12)


@pytest.mark.parametrize("kw", QUAD_FORMS, ids=["lane", "quad"])
def test_planar_quadrotor_ragged_batch_and_permutation(lib, kw):
    """B = 67 (a ragged tail of the four-trajectories-per-wavefront mapping), five parameter rows dealt over the batch; then the rows
    permuted: every output must be permuted the same way (catches a trajectory / lane index mix-up)."""
    model, B, T = make_env_model("PlanarQuadrotor"), 67, 8
    eng, out, params = compare_with_copies(model, B, T, 2, lib, "cpu", 1e-12, n_sets=5, **kw)
    perm = np.random.default_rng(7).permutation(B)
    outp = solve(engine(model, B, T, lib, "cpu", model_params=params[perm], **kw), 2)
    for n in OUTPUTS:
        assert rel(outp[n], out[n][perm]) <= 1e-12, f"{n}: permuted parameters do not permute the result"


def test_plugin_per_trajectory_vs_model_copies(lib):
    from test_model_plugin import VanDerPolKnown

    model = make_env_model(VanDerPolKnown())
    assert model.resolve_model_id(lib) >= _native.PLUGIN_BASE
    eng, out, params = compare_with_copies(model, 4, 15, 3, lib, "cpu", 1e-12)
    assert_params_matter(out, params, 1e-12)


def test_set_model_params_in_place(lib):
    model = make_env_model("PlanarQuadrotor")
    rows = param_rows(model, 3, 5)
    eng = engine(model, 3, 8, lib, "cpu", model_params=rows[[0, 0, 0]])
    ptr = eng._problem.model_params_b
    eng.set_model_params(rows)
    assert eng._problem.model_params_b == ptr and np.array_equal(parity.np_(eng.model_params), rows)
    out = solve(eng, 2)
    ref = solve(engine(model, 3, 8, lib, "cpu", model_params=rows), 2)
    for n in OUTPUTS:
        assert rel(out[n], ref[n]) <= 1e-12
    assert engine(model, 3, 8, lib, "cpu").model_params is None


def test_refusals(lib):
    pend = make_env_model("PendulumKnown")
    with pytest.raises(ValueError, match="no model parameters"):
        engine(pend, 2, 8, lib, "cpu", model_params=np.zeros((2, 0)))
    quad = make_env_model("PlanarQuadrotor")
    with pytest.raises(ValueError, match=r"\(B, NP\)"):
        engine(quad, 2, 8, lib, "cpu", model_params=np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"\(B, NP\)"):
        engine(quad, 2, 8, lib, "cpu", model_params=np.ones((3, 3)))
    with pytest.raises(ValueError, match="finite"):
        engine(quad, 2, 8, lib, "cpu", model_params=np.array([[1.0, 1.0, np.nan], [1.0, 1.0, 1.0]]))
    # ... and at the ABI: a pointer on a model without parameters is I2C_EINVAL
    eng = engine(pend, 2, 8, lib, "cpu")
    p = eng._make_problem()
    buf = torch.zeros(2)
    p.model_params_b = buf.data_ptr()
    assert lib.i2c_backward_schedule(C.byref(p)) == -1 and lib.i2c_kernel_family(C.byref(p), _native.SWEEP_FORWARD) == -1


@pytest.mark.parametrize("name", ["PlanarQuadrotor", "Quadrotor12"])
def test_family_and_schedule_do_not_depend_on_per_trajectory_params(lib, name):
    model = make_env_model(name)
    sweeps = (_native.SWEEP_FORWARD, _native.SWEEP_BACKWARD, _native.SWEEP_PROPAGATE, _native.SWEEP_FILTER,
              _native.SWEEP_CHUNK_PASSES, _native.SWEEP_CHUNK_STITCH)
    for B in (1, 256, 1024, 1025, 4096, 8193):
        eng = engine(model, 1, 4, lib, "cpu")
        for lanes in (0, -1, 64, _native.LANES_QUAD, eng.dims.group_lanes):
            for mode in (_native.BWD_AUTO, _native.BWD_CHUNKED, _native.BWD_FUSED):
                p = eng._make_problem()
                p.B, p.group_lanes, p.backward_mode = B, lanes, mode
                buf = torch.zeros(eng.dims.n_params * B, dtype=torch.float64)
                q = type(p).from_buffer_copy(p)
                q.model_params_b = buf.data_ptr()
                assert lib.i2c_backward_schedule(C.byref(p)) == lib.i2c_backward_schedule(C.byref(q))
                for s in sweeps:
                    assert lib.i2c_kernel_family(C.byref(p), s) == lib.i2c_kernel_family(C.byref(q), s), (B, lanes, mode, s)


def numpy_rollout(models, eng, res):
    """The linear-policy rollout through each trajectory's model copy with the same disturbances (rollout n = r * B + b)."""
    K, k, sigK = (parity.np_(t) for t in eng.local_linear_policy())
    B, T, nx = eng.B, eng.H, eng.nx
    eps_x = parity.np_(res["eps_x"])
    x = np.tile(parity.np_(eng.x0).T, (eps_x.shape[2] // B, 1))
    Le = np.linalg.cholesky(np.asarray(eng.sys.sig_eta, float))
    xs = []
    for t in range(T):
        u = np.einsum("nij,nj->ni", np.tile(K[:, t], (x.shape[0] // B, 1, 1)), x) + np.tile(k[:, t], (x.shape[0] // B, 1))
        xu = np.hstack((x, u))
        xs.append(xu)
        x = np.vstack([models[n % B].dynamics(xu[n: n + 1]) for n in range(x.shape[0])]) + eps_x[t].T @ Le.T
    return np.stack(xs), x


@pytest.mark.parametrize("override", [False, True], ids=["planning_params", "plant_override"])
def test_rollout_per_trajectory_plants(lib, override):
    model, B, T = make_env_model("PlanarQuadrotor"), 4, 8
    plan, plant = param_rows(model, B, 11), param_rows(model, B, 12)
    eng = engine(model, B, T, lib, "cpu", model_params=None if override else plan)
    solve(eng, 2)
    g = torch.Generator().manual_seed(0)
    res = eng.rollout(n_rollouts=2, generator=g, model_params=plant if override else None)
    rows = plant if override else plan
    xs, xf = numpy_rollout([with_params(model, r) for r in rows], eng, res)
    got = parity.np_(res["xu"]).reshape(2 * B, T, -1)  # (R, B, T, d) -> rollout n = r * B + b
    assert rel(got, np.transpose(xs, (1, 0, 2))) <= 1e-10
    assert rel(parity.np_(res["x_final"]).reshape(2 * B, -1), xf) <= 1e-10
    # the override is for that rollout only, and it changes the result
    if override:
        assert eng.model_params is None
        base = eng.rollout(n_rollouts=2, eps_x=res["eps_x"])
        assert rel(parity.np_(base["x_final"]), parity.np_(res["x_final"])) > 1e-6


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib():
    return pkg.load_library()


GPU_TOL = 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("inference,kw", [("cubature", {}), ("linearize", {}), ("gauss_hermite", {"gh_degree": 3})])
def test_gpu_linear_lane(gpu_lib, inference, kw):
    eng, out, params = compare_with_copies(linear_model(), 6, 20, 3, gpu_lib, "cuda", GPU_TOL, inference=inference,
                                           deterministic_family=True, **kw)
    assert eng.forward_family == "lane"


@pytest.mark.gpu
@pytest.mark.parametrize("B,kw,fam", [(67, dict(deterministic_family=True), "lane"), (67, dict(group_lanes=64), "quad"),
                                      (1, {}, None), (200, {}, None), (67, dict(group_lanes=8), "group")],
                         ids=["lane", "quad64", "default_B1", "default_B200", "group8"])
def test_gpu_planar_quadrotor_families(gpu_lib, B, kw, fam):
    model = make_env_model("PlanarQuadrotor")
    eng, out, params = compare_with_copies(model, B, 12, 3, gpu_lib, "cuda", GPU_TOL, n_sets=None if B == 1 else 5, **kw)
    if fam:
        assert eng.forward_family == eng.backward_family == fam
    if B > 1:
        assert_params_matter(out, params, GPU_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("B,lanes,fam", [(64, 64, "wave"), (1030, _native.LANES_QUAD, "quad"), (70, 16, "group")])
def test_gpu_quadrotor12_families(gpu_lib, B, lanes, fam):
    model = make_env_model("Quadrotor12")
    eng, out, params = compare_with_copies(model, B, 10, 3, gpu_lib, "cuda", GPU_TOL, n_sets=4, group_lanes=lanes)
    assert eng.forward_family == eng.backward_family == fam
    assert_params_matter(out, params, GPU_TOL)


@pytest.mark.gpu
def test_gpu_planar_quadrotor_rollout_override(gpu_lib):
    model, B, T = make_env_model("PlanarQuadrotor"), 64, 10
    plant = param_rows(model, B, 12)
    eng = engine(model, B, T, gpu_lib, "cuda")
    solve(eng, 2)
    res = eng.rollout(n_rollouts=1, model_params=plant)
    xs, xf = numpy_rollout([with_params(model, r) for r in plant], eng, res)
    assert rel(parity.np_(res["x_final"]).reshape(B, -1), xf) <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 1030])
def test_gpu_quadrotor12_mpc_ckf_fleet(gpu_lib, B):
    """MPC + CKF control steps (i2c_mpc_step) of a fleet with per-vehicle masses and inertias against the same steps run for each
    distinct vehicle on its own (a whole batch of it)."""
    model, T, steps = make_env_model("Quadrotor12"), 10, 3
    rows = param_rows(model, 3, 21)
    which = np.arange(B) % 3
    sig_zeta = 1e-4 * np.eye(model.dim_y)

    def run(m, params, plant_rows):
        eng = engine(m, B, T, gpu_lib, "cuda", model_params=params)
        eng.enable_per_cell_alpha()
        solve(eng, 2)
        plants = [with_params(model, r) for r in plant_rows]
        x = np.zeros((B, model.dim_x))
        u = np.tile(np.full(model.dim_u, 0.25 * model.gravity), (B, 1))
        acts = []
        for _ in range(steps):
            x = np.vstack([plants[b].dynamics(np.hstack((x[b], u[b]))[None]) for b in range(B)])
            y = np.vstack([plants[b].measure(x[b: b + 1]) for b in range(B)])
            mu_u, _ = eng.mpc_step(2, y=torch.as_tensor(y.T.copy(), device="cuda"), u=torch.as_tensor(u.T.copy(), device="cuda"),
                                   sig_zeta=sig_zeta)
            u = parity.np_(mu_u)
            acts.append(u)
        torch.cuda.synchronize()
        assert eng.failures() == []
        return np.stack(acts, 1), parity.np_(eng.x0).T

    acts, belief = run(model, rows[which], rows[which])
    for j in range(3):
        a_j, b_j = run(with_params(model, rows[j]), None, rows[[j] * B])
        sel = which == j
        assert rel(acts[sel], a_j[sel]) <= GPU_TOL and rel(belief[sel], b_j[sel]) <= GPU_TOL
    assert rel(acts[0], acts[1]) > 1e-6  # (vehicles 0 and 1 carry different parameter sets: the comparison means something)
