"""Monte-Carlo policy evaluation on the device (`i2c_rollout_eval`, BatchedI2c.evaluate): the per-rollout costs, their statistics and
the moments of (x_t, u_t) over the rollouts, against numpy reductions of what `i2c_rollout` simulates from the same noise; the
counter-based generator against a numpy twin of its published layout; reproducibility (bit for bit across calls, batch splits and
stale workspaces), horizons, per-call plants, failure containment, a linear-Gaussian known answer, and the interface's refusals.
Every numeric check runs on the host simulation and, marked gpu, on the device."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import Case, assert_close, load_case

pkg = parity.pkg
N = pkg._native
np_ = parity.np_
ENOTSUP, EINVAL = -2, -1
M32 = np.uint64(0xFFFFFFFF)


# ---- the numpy twin of csrc/i2c_random.hpp ------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of 32-bit words held in uint64: ctr 4 arrays, key 2 -> 4 arrays."""
    c = [np.asarray(w, np.uint64) & M32 for w in ctr]
    k = [np.uint64(key[0]) & M32, np.uint64(key[1]) & M32]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return c


def twin_normals(seed, traj, r, t, kind, n):
    """The first n normals of every (trajectory, rollout) pair at step t: (n, len(r), len(traj)), layout of include/i2c_hip.h."""
    tr, rr = np.meshgrid(np.asarray(traj, np.uint64), np.asarray(r, np.uint64))  # (R, B)
    out = np.empty((n,) + tr.shape)
    for j in range((n + 1) // 2):
        w = philox4x32_10((tr, rr, np.full_like(tr, t), np.full_like(tr, kind + 4 * j)), (seed & 0xFFFFFFFF, seed >> 32))
        a = (w[0] << np.uint64(21)) | (w[1] >> np.uint64(11))
        b = (w[2] << np.uint64(21)) | (w[3] >> np.uint64(11))
        u1, u2 = (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53
        rho = np.sqrt(-2.0 * np.log(u1))
        out[2 * j] = rho * np.cos(2.0 * np.pi * u2)
        if 2 * j + 1 < n:
            out[2 * j + 1] = rho * np.sin(2.0 * np.pi * u2)
    return out


def twin_noise(seed, first, B, R_, T, nx, nu):
    """(eps_x0 [nx][N], eps_x [T][nx][N], eps_u [T][nu][N]), N = R * B, n = r * B + b: what the kernel draws for this seed"""
    traj, r = first + np.arange(B), np.arange(R_)
    e0 = twin_normals(seed, traj, r, 0xFFFFFFFF, 0, nx).reshape(nx, R_ * B)
    ex = np.stack([twin_normals(seed, traj, r, t, 1, nx).reshape(nx, R_ * B) for t in range(T)])
    eu = np.stack([twin_normals(seed, traj, r, t, 2, nu).reshape(nu, R_ * B) for t in range(T)])
    return e0, ex, eu


def test_the_twin_is_philox():
    """the published known-answer vectors (counter | key -> output)"""
    vectors = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
               ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
               ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in vectors:
        assert tuple(int(w) for w in philox4x32_10(ctr, key)) == want


# ---- cases: goldens cut short, solved for three iterations, shared by the tests (evaluate() leaves an engine as it found it) ----------
def cut(name, T):
    g = load_case(name)
    return Case({**dict(g), "meta": np.array(json.dumps(dict(g.meta, T=T))), "mu_u": g["mu_u"][:T]})


def lib_of(device):
    if device == "cpu":
        return hostsim.load()
    lib = pkg.load_library()
    assert not lib.is_host_sim
    return lib


SPECS = {  # name -> (golden, T, B)
    "pendulum": ("em_pendulum_T200", 12, 70),   # one full wavefront plus six lanes
    "pendulum10": ("em_pendulum_T200", 12, 10),
    "pendulum6": ("em_pendulum_T200", 12, 6),
    "dcp": ("em_dcp_T60", 9, 3),                # d = 7: 35 moment rows
    "quadrotor": ("em_quadrotor_T20", 8, 3),
    "quad12": ("em_quad12_T20", 6, 3),          # trajectory-major post
    "linear": ("em_linear_T60", 10, 2),
}
_ENGINES = {}


def inputs(spec):
    name, T, B = SPECS[spec]
    case = cut(name, T)
    return (case,) + parity.batched_inputs(case, B)


def build(case, device, x0, mu_u, n_iter=3, targets=None, **kw):
    eng = parity.engine_from_case(case, lib_of(device), device, x0=x0, mu_u=mu_u, **kw)
    if targets is not None:
        eng.set_targets(targets)
    for _ in range(n_iter):
        eng.learn_msgs()
    assert eng.failures() == []
    return eng


def solved(spec, device):
    if (spec, device) not in _ENGINES:
        case, x0, mu_u = inputs(spec)
        _ENGINES[spec, device] = build(case, device, x0, mu_u)
    return _ENGINES[spec, device]


def solved_special(which, device):
    """pendulum with per-cell targets; PendulumKnownActReg (no Qf, no terminal observation)"""
    if (which, device) not in _ENGINES:
        if which == "targets":
            case, x0, mu_u = inputs("pendulum6")
            zg = np.asarray(parity.product_model(case).zg, float).reshape(-1)
            z = zg[None] + 0.05 * np.random.default_rng(5).normal(size=(12, zg.size))
            _ENGINES[which, device] = build(case, device, x0, mu_u, targets=z)
        else:
            from i2c.known_models import make_env_model
            T, B = 12, 5
            x0 = np.array([np.pi, 0.0]) + 1e-2 * np.random.default_rng(4).normal(size=(B, 2))
            eng = pkg.BatchedI2c(make_env_model("PendulumKnownActReg"), T, None, np.diag([1.0]), None, 300.0, 1.0, np.zeros((B, T, 1)),
                                 0.5 * np.eye(1), x0=x0, device=device, lib=lib_of(device))
            for _ in range(3):
                eng.learn_msgs()
            assert eng.failures() == [] and not eng.has_Qf
            _ENGINES[which, device] = eng
    return _ENGINES[which, device]


OUTPUTS = ("cost", "cost_mean", "cost_var", "cost_min", "cost_max", "cost_percentiles", "n_bad", "xu_mean", "xu_cov")


def numpy_reductions(eng, res):
    """What evaluate() returns, from the tensors of a rollout() of the same noise"""
    xu, z = np_(res["xu"]), np_(res["z"])  # (R, B, T, .)
    zg = np.broadcast_to(eng.zg, z.shape[1:]) if eng.z is None else np.transpose(np_(eng.z), (2, 0, 1))
    e = z - zg[None]
    cost = np.einsum("rbti,ij,rbtj->rb", e, eng.QR, e)
    if eng.has_Qf:
        et = np_(res["z_term"]) - eng.zg_term[None, None]
        cost = cost + np.einsum("rbi,ij,rbj->rb", et, eng.Qf, et)
    R_, B, T, d = xu.shape
    with np.errstate(all="ignore"):
        cov = np.array([[np.cov(xu[:, b, t].T, ddof=1) for t in range(T)] for b in range(B)]).reshape(B, T, d, d)
        var = cost.var(0, ddof=1)
    return dict(cost=cost, cost_mean=cost.mean(0), cost_var=var, cost_min=cost.min(0), cost_max=cost.max(0),
                cost_percentiles=np.percentile(cost, (10, 90), axis=0), xu_mean=xu.mean(0), xu_cov=cov)


def check_given(eng, R_, policy="linear", parts=None, model_params=None, tol=1e-11, **noise):
    """evaluate() on the noise a rollout() drew, against numpy reductions of that rollout"""
    gen = torch.Generator(device=eng.device).manual_seed(11)
    res = eng.rollout(R_, policy, generator=gen, model_params=model_params, **noise)
    ref = numpy_reductions(eng, res)
    out = eng.evaluate(R_, policy, process_noise=False, parts=parts, model_params=model_params, eps_x0=res["eps_x0"], eps_x=res["eps_x"],
                       eps_u=res["eps_u"])
    assert int(out["n_bad"].sum()) == 0 and (parts is None or out["parts"] == parts)
    for k in ("cost", "cost_percentiles", "xu_mean", "xu_cov"):
        assert_close(np_(out[k]), ref[k], tol, f"{policy} parts={parts} {k}")
    # The four statistics are ONE output, cost_stats [4][B], and are compared as one array in the max-norm. A variance row on its own
    # cannot meet 1e-11 against another evaluation of the costs: the two sides' costs agree to a few ulp of the cost C, and a variance
    # s^2 of costs that differ by s << C amplifies that by C / s (double cartpole, T = 9: C ~ 1e3, s ~ 2e-4, measured 2.7e-11 with
    # costs that agree to 1e-16) -- in ANY fp64 implementation, this one and numpy's alike. What the reduction itself adds is held
    # to 1e-11 row by row below, against numpy on the very costs it read.
    stats = ("cost_mean", "cost_var", "cost_min", "cost_max")
    assert_close(np.stack([np_(out[k]) for k in stats]), np.stack([ref[k] for k in stats]), tol, f"{policy} parts={parts} cost_stats")
    own = np_(out["cost"])
    for k, v in zip(stats, (own.mean(0), own.var(0, ddof=1), own.min(0), own.max(0))):
        assert_close(np_(out[k]), v, tol, f"{policy} parts={parts} {k} of the costs returned")
    return out, ref


GIVEN = [
    ("pendulum", "linear", 5, 1, dict(process_noise=True)),
    ("pendulum", "linear", 5, 2, dict(process_noise=True)),  # the uneven split 3 + 2
    ("pendulum", "linear", 5, 5, dict(process_noise=True)),
    ("pendulum", "expert_soft", 5, 2, dict(process_noise=True, action_noise=True)),
    ("dcp", "linear", 4, 3, dict(process_noise=True, sample_x0=True)),
    ("quadrotor", "linear", 3, None, dict(process_noise=True)),
    ("quad12", "linear", 3, None, dict(process_noise=True)),
    ("targets", "linear", 4, 2, dict(process_noise=True)),
    ("actreg", "linear", 4, 2, dict(process_noise=True)),
]


def _given(device, spec, policy, R_, parts, noise):
    eng = solved_special(spec, device) if spec in ("targets", "actreg") else solved(spec, device)
    check_given(eng, R_, policy, parts, **noise)


@pytest.mark.parametrize("spec,policy,R_,parts,noise", GIVEN)
def test_given_noise_against_rollout_cpu(spec, policy, R_, parts, noise):
    _given("cpu", spec, policy, R_, parts, noise)


@pytest.mark.gpu
@pytest.mark.parametrize("spec,policy,R_,parts,noise", GIVEN)
def test_given_noise_against_rollout_gpu(spec, policy, R_, parts, noise):
    _given("cuda", spec, policy, R_, parts, noise)


# ---- generated noise ------------------------------------------------------------------------------------------------------------------
def same(a, b, keys=OUTPUTS):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert torch.equal(a[k], b[k]) or (torch.equal(torch.isnan(a[k]), torch.isnan(b[k])) and
                                               torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k]))), k


def _generated(device, spec, R_, seed, first):
    eng = solved(spec, device)
    flags = dict(process_noise=True, action_noise=True, sample_x0=True)
    a = eng.evaluate(R_, seed=seed, first_trajectory=first, **flags)
    e0, ex, eu = twin_noise(seed, first, eng.B, R_, eng.H, eng.nx, eng.nu)
    b = eng.evaluate(R_, process_noise=False, eps_x0=e0, eps_x=ex, eps_u=eu)
    for k in OUTPUTS:
        if k != "n_bad":
            assert_close(np_(a[k]), np_(b[k]), 1e-9, f"{spec} generated vs twin: {k}")
    c = eng.evaluate(R_, seed=seed + 1, first_trajectory=first, **flags)
    assert not torch.equal(a["cost"], c["cost"])
    # one kind alone draws what it draws with the others on
    d = eng.evaluate(R_, seed=seed, first_trajectory=first, process_noise=True)
    e = eng.evaluate(R_, process_noise=False, eps_x=ex)
    assert_close(np_(d["cost"]), np_(e["cost"]), 1e-9, f"{spec} process noise alone")


GENERATED = [("pendulum", 5, 2024, 0), ("dcp", 4, (0xDEADBEEF << 32) | 17, 3)]


@pytest.mark.parametrize("spec,R_,seed,first", GENERATED)
def test_generated_noise_against_twin_cpu(spec, R_, seed, first):
    _generated("cpu", spec, R_, seed, first)


@pytest.mark.gpu
@pytest.mark.parametrize("spec,R_,seed,first", GENERATED)
def test_generated_noise_against_twin_gpu(spec, R_, seed, first):
    _generated("cuda", spec, R_, seed, first)


def sub_engine(spec, device, lo, hi):
    case, x0, mu_u = inputs(spec)
    return build(case, device, x0[lo:hi], mu_u[lo:hi])


def columns(out, lo, hi):
    return {k: (None if out[k] is None else out[k][lo:hi] if k in ("xu_mean", "xu_cov") else out[k][..., lo:hi]) for k in OUTPUTS}


def _first_trajectory(device):
    big = solved("pendulum10", device).evaluate(4, seed=9, action_noise=True, sample_x0=True, parts=2)
    small = sub_engine("pendulum10", device, 7, 10).evaluate(4, seed=9, action_noise=True, sample_x0=True, parts=2, first_trajectory=7)
    same(columns(big, 7, 10), small)


def test_first_trajectory_cpu():
    _first_trajectory("cpu")


@pytest.mark.gpu
def test_first_trajectory_gpu():
    _first_trajectory("cuda")


# ---- reproducibility ------------------------------------------------------------------------------------------------------------------
def _reproducible(device):
    eng = solved("pendulum6", device)
    kw = dict(seed=3, action_noise=True, sample_x0=True, parts=2)
    a = eng.evaluate(5, **kw)
    work = eng._eval_work
    work.fill_(-7e77)  # a stale workspace cannot leak in: the first rollout of a lane stores
    b = eng.evaluate(5, **kw)
    assert eng._eval_work is work  # kept between calls of one shape
    same(a, b)
    work.zero_()
    same(a, eng.evaluate(5, **kw))
    for lo in (0, 3):  # a batch of 6 against two engines of 3
        same(columns(a, lo, lo + 3), sub_engine("pendulum6", device, lo, lo + 3).evaluate(5, first_trajectory=lo, **kw))
    for parts in (1, 5, None):
        c = eng.evaluate(5, **dict(kw, parts=parts))
        assert c["parts"] == (parts or 5)
        assert torch.equal(a["cost"], c["cost"]) and torch.equal(a["cost_mean"], c["cost_mean"])
        for k in ("xu_mean", "xu_cov"):
            assert_close(np_(c[k]), np_(a[k]), 1e-11, f"parts={parts} {k}")
    d = eng.evaluate(5, moments=False, **kw)
    assert d["xu_mean"] is None and d["xu_cov"] is None
    same(a, d, ("cost", "cost_mean", "cost_var", "cost_min", "cost_max", "cost_percentiles", "n_bad"))
    one = eng.evaluate(1, seed=3)  # one sample has no unbiased variance
    assert torch.isnan(one["cost_var"]).all() and torch.isnan(one["xu_cov"]).all() and torch.isfinite(one["xu_mean"]).all()


def test_reproducible_cpu():
    _reproducible("cpu")


@pytest.mark.gpu
def test_reproducible_gpu():
    _reproducible("cuda")


# ---- horizons -------------------------------------------------------------------------------------------------------------------------
def raw_evaluate(eng, R_, seed, parts, fill):
    """i2c_rollout_eval on buffers of the test's own, pre-filled with `fill`: -> (xu_mean [T][d][B], xu_cov, work)"""
    ev = N.I2cRolloutEval()
    ev.n_rollouts, ev.policy, ev.noise, ev.parts, ev.seed = R_, 0, N.NOISE_PROCESS, parts, seed
    n = eng.lib.i2c_rollout_eval_workspace(ctypes.byref(eng._problem), ctypes.byref(ev), None)
    E = eng.d + eng.d * (eng.d + 1) // 2
    assert n == parts * eng.H * E * eng.B * 8
    new = lambda *s: torch.full(s, fill, dtype=eng.dtype, device=eng.device)  # noqa: E731
    cost, mean, cov, work = new(R_, eng.B), new(eng.H, eng.d, eng.B), new(eng.H, E - eng.d, eng.B), new(n // 8)
    ev.cost, ev.xu_mean, ev.xu_cov, ev.work = cost.data_ptr(), mean.data_ptr(), cov.data_ptr(), work.data_ptr()
    assert eng.lib.i2c_rollout_eval(ctypes.byref(eng._problem), eng._ptr(eng.post), ctypes.byref(ev), eng._stream()) == 0
    return mean, cov, work.reshape(parts, eng.H, E, eng.B)


def _horizons(device):
    case, x0, mu_u = inputs("pendulum6")
    hz = [1, 2, 7, 12, 12]
    eng = build(case, device, x0[:5], mu_u[:5], horizons=hz)
    out = eng.evaluate(4, seed=21, parts=2)
    assert int(out["n_bad"].sum()) == 0
    for b, Tb in enumerate(hz):  # each trajectory: a batch of one, solved and evaluated at its own horizon
        solo_case = cut("em_pendulum_T200", Tb)
        solo = build(solo_case, device, x0[b:b + 1], mu_u[b:b + 1, :Tb], horizons=[Tb])
        ref = solo.evaluate(4, seed=21, parts=2, first_trajectory=b)
        for k in ("cost", "cost_mean", "cost_var", "cost_min", "cost_max"):
            assert torch.equal(out[k][..., b], ref[k][..., 0]), (k, b)
        for k in ("xu_mean", "xu_cov"):
            assert_close(np_(out[k][b, :Tb]), np_(ref[k][0]), 1e-11, f"trajectory {b} {k}")
            assert torch.isnan(out[k][b, Tb:]).all()  # rows that do not exist
    mean, cov, work = raw_evaluate(eng, 4, 21, 2, -7e77)
    valid = eng.valid_cells().T  # (T, B)
    for t in (mean, cov, work[0], work[1]):
        gone = (~valid)[:, None, :].expand_as(t)
        assert (t[gone] == -7e77).all() and torch.isfinite(t[~gone]).all() and (t[~gone] != -7e77).all()
    assert torch.equal(mean.permute(2, 0, 1)[valid.T], out["xu_mean"][valid.T])


def test_horizons_cpu():
    _horizons("cpu")


@pytest.mark.gpu
def test_horizons_gpu():
    _horizons("cuda")


# ---- other plants for one call ----------------------------------------------------------------------------------------------------------
def _other_plants(device):
    eng = solved("linear", device)
    base = np.asarray(eng.sys.device_params(), np.float64)
    P = base[None] + 0.02 * np.random.default_rng(8).normal(size=(eng.B, base.size))
    before = eng.model_params
    noise = dict(process_noise=True, action_noise=True, sample_x0=True)
    with_p, _ = check_given(eng, 6, "linear", 3, model_params=P, **noise)
    nominal, _ = check_given(eng, 6, "linear", 3, **noise)
    assert (with_p["cost"] - nominal["cost"]).abs().min() > 0  # the rows of P change every rollout
    assert eng.model_params is before and eng._problem.model_params_b in (None, 0)
    a, b = eng.evaluate(6, seed=4, model_params=P), eng.evaluate(6, seed=4)
    assert not torch.equal(a["cost"], b["cost"])
    same(b, eng.evaluate(6, seed=4))


def test_other_plants_cpu():
    _other_plants("cpu")


@pytest.mark.gpu
def test_other_plants_gpu():
    _other_plants("cuda")


# ---- failure containment ----------------------------------------------------------------------------------------------------------------
def _containment(device):
    eng = solved("pendulum6", device)
    kw = dict(seed=12, action_noise=True, parts=2)
    clean = eng.evaluate(5, **kw)
    keep = eng.post.clone()
    try:
        eng.post[3, :, 2] = float("nan")  # cell 3 of trajectory 2: its controller is NaN from there on
        bad = eng.evaluate(5, **kw)
    finally:
        eng.post.copy_(keep)
    assert int(bad["n_bad"][2]) == 5 and torch.isnan(bad["cost"][:, 2]).all()
    for k in ("cost_mean", "cost_var", "cost_min", "cost_max"):
        assert torch.isnan(bad[k][2]), k
    assert torch.equal(bad["xu_mean"][2, :3], clean["xu_mean"][2, :3]) and torch.equal(bad["xu_cov"][2, :3], clean["xu_cov"][2, :3])
    assert torch.isnan(bad["xu_mean"][2, 3]).all()  # (later cells may be finite again: a model that clips its action absorbs a NaN)
    others = [0, 1, 3, 4, 5]
    for k in OUTPUTS:
        sel = (lambda t: t[others]) if k in ("xu_mean", "xu_cov") else (lambda t: t[..., others])
        assert torch.equal(sel(bad[k]), sel(clean[k])), k


def test_containment_cpu():
    _containment("cpu")


@pytest.mark.gpu
def test_containment_gpu():
    _containment("cuda")


# ---- the known answer of a linear-Gaussian loop -----------------------------------------------------------------------------------------
def _linear_gaussian(device):
    """For a linear plant the closed-loop distribution IS the propagation's (u = K x + k with covariance K S K^T + sigK from
    N(x0, sig_x0)): R = 4096 rollouts against it within six Gaussian standard errors, sqrt(S_ii / R) on the mean and
    sqrt((S_ii S_jj + S_ij^2) / (R - 1)) on the covariance."""
    eng = solved("linear", device)
    R_ = 4096
    keep = eng.use_expert_controller
    try:
        eng.use_expert_controller = False
        eng.propagate()
    finally:
        eng.use_expert_controller = keep
    prop = eng.propagated()
    mu, S = np_(prop["mu_xu0_pf"]), np_(prop["sig_xu0_pf"])
    out = eng.evaluate(R_, seed=1234, process_noise=True, action_noise=True, sample_x0=True)
    assert out["parts"] == R_ and int(out["n_bad"].sum()) == 0
    dg = np.einsum("btii->bti", S)
    err_m = np.abs(np_(out["xu_mean"]) - mu) / (6.0 * np.sqrt(dg / R_))
    err_c = np.abs(np_(out["xu_cov"]) - S) / (6.0 * np.sqrt((dg[..., :, None] * dg[..., None, :] + S ** 2) / (R_ - 1)))
    print(f"linear-Gaussian: mean {err_m.max():.3f}, covariance {err_c.max():.3f} of the six-sigma bound")
    assert err_m.max() <= 1.0 and err_c.max() <= 1.0


def test_linear_gaussian_known_answer_cpu():
    _linear_gaussian("cpu")


@pytest.mark.gpu
def test_linear_gaussian_known_answer_gpu():
    _linear_gaussian("cuda")


# ---- interface ------------------------------------------------------------------------------------------------------------------------
_FLAG = (ctypes.c_int64 * 4)(1, 1, 1, 1)  # the argument checks only test pointers against NULL


def flag_problem(model_id=0, B=4, T=20, dtype=0):
    p = N.I2cProblem()
    p.abi_version, p.model_id, p.B, p.T, p.dtype, p.terminal_cell, p.gh_degree = N.ABI_VERSION, model_id, B, T, dtype, T - 1, 3
    p.quad_alpha, p.quad_beta, p.quad_kappa = 1.0, 0.0, 0.0
    for name in ("x0", "sig_x0", "alpha", "feedforward"):
        setattr(p, name, ctypes.addressof(_FLAG))
    return p


def flag_eval(**fields):
    ev = N.I2cRolloutEval()
    ev.n_rollouts, ev.cost = 4, ctypes.addressof(_FLAG)
    for k, v in fields.items():
        setattr(ev, k, v)
    return ev


@pytest.mark.parametrize("which", ["hostsim", "hip"])
def test_refusals_through_the_c_api(which):
    lib = hostsim.load() if which == "hostsim" else pkg.load_library()
    buf = ctypes.c_void_p(ctypes.addressof(_FLAG))
    f = buf.value
    call = lambda p, ev, post=buf: lib.i2c_rollout_eval(ctypes.byref(p), post, ctypes.byref(ev), None)  # noqa: E731
    p = flag_problem()
    assert call(p, flag_eval(), None) == EINVAL                       # no post
    assert call(p, flag_eval(cost=None)) == EINVAL
    assert call(p, flag_eval(n_rollouts=0)) == EINVAL
    assert call(p, flag_eval(policy=3)) == EINVAL and call(p, flag_eval(policy=-1)) == EINVAL
    assert call(p, flag_eval(xu_cov=f, work=f)) == EINVAL             # a covariance without a mean
    assert call(p, flag_eval(xu_mean=f, xu_cov=f)) == EINVAL          # moments without a workspace
    assert call(p, flag_eval(parts=-1)) == EINVAL and call(p, flag_eval(parts=5)) == EINVAL
    assert call(p, flag_eval(first_trajectory=2 ** 32 - 3)) == EINVAL  # first_trajectory + B beyond 32 bits
    assert lib.i2c_rollout_eval(ctypes.byref(p), buf, None, None) == EINVAL
    for dtype in (N.F32, N.F64_F32S):
        assert call(flag_problem(dtype=dtype), flag_eval()) == ENOTSUP  # the sums are fp64
    assert lib.i2c_rollout_eval_workspace(ctypes.byref(flag_problem(dtype=N.F32)), ctypes.byref(flag_eval()), None) == 0
    assert lib.i2c_rollout_eval_workspace(ctypes.byref(p), ctypes.byref(flag_eval(parts=5)), None) == 0
    assert N.I2cProblem._fields_[-1][0] == "horizons" and lib.i2c_abi_version() == 9  # entry points only: the problem and the ABI stay


def test_workspace_and_the_parts_rule():
    lib = hostsim.load()
    got = ctypes.c_int32(0)
    for model_id, d in ((0, 3), (3, 7)):
        E = d + d * (d + 1) // 2
        for B in (1, 70, 65536, 70000):
            for R_ in (1, 5, 100000):
                P = min(R_, max(1, -(-65536 // B)))
                n = lib.i2c_rollout_eval_workspace(ctypes.byref(flag_problem(model_id, B=B, T=20)), ctypes.byref(flag_eval(n_rollouts=R_)),
                                                   ctypes.byref(got))
                assert (n, got.value) == (P * 20 * E * B * 8, P), (model_id, B, R_)
    n = lib.i2c_rollout_eval_workspace(ctypes.byref(flag_problem(0, B=70, T=20)), ctypes.byref(flag_eval(n_rollouts=9, parts=4)), ctypes.byref(got))
    assert (n, got.value) == (4 * 20 * 9 * 70 * 8, 4)


def test_engine_refuses_before_it_allocates(monkeypatch):
    eng = solved("pendulum6", "cpu")

    def no_alloc(*a, **k):
        raise AssertionError("evaluate() allocated before it validated")

    bad = [dict(n_rollouts=0), dict(n_rollouts=4, policy="greedy"), dict(n_rollouts=4, parts=0), dict(n_rollouts=4, parts=5),
           dict(n_rollouts=4, first_trajectory=-1), dict(n_rollouts=4, first_trajectory=2 ** 32 - 3), dict(n_rollouts=4, seed=-1),
           dict(n_rollouts=4, seed=2 ** 64), dict(n_rollouts=4, percentiles=(10, 101)), dict(n_rollouts=4, model_params=np.ones((6, 1)))]
    with monkeypatch.context() as m:
        for name in ("empty", "zeros", "full", "as_tensor"):
            m.setattr(torch, name, no_alloc)
        for kw in bad:
            with pytest.raises(ValueError):
                eng.evaluate(**kw)
    case, x0, mu_u = inputs("pendulum6")
    f32 = parity.engine_from_case(case, hostsim.load(), "cpu", dtype=torch.float32, x0=x0, mu_u=mu_u, allow_inexact=True)
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", no_alloc)
        with pytest.raises(ValueError):
            f32.evaluate(4)


def test_a_model_library_from_before_the_entry_is_refused():
    """A model library without the i2c_model_ops_size symbol (csrc/i2c_model_entry.hip compiled with -DI2C_NO_OPS_SIZE: what one built
    before ModelOps grew looks like) is registered with the entry absent: I2C_ENOTSUP, nothing is read past its table."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("i2c_amd_build", os.path.join(hostsim.ROOT, "input-inference-for-control_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = hostsim.load()
    # a model type of its own: the tables are static objects of a function template (make_ops) with vague linkage, which the
    # dynamic linker unifies across libraries of ONE model type -- this library would get the id and the size of the Van der Pol
    # library that tests/test_model_plugin.py loads into the same process
    header = os.path.join(os.path.dirname(lib.path), "van_der_pol_v9.hpp")
    text = '#include "%s"\nnamespace i2c {\nstruct VanDerPolV9 : VanDerPol {};\n}\n' % os.path.join(hostsim.ROOT, "tests", "plugins", "van_der_pol.hpp")
    if not os.path.exists(header) or open(header).read() != text:
        with open(header, "w") as f:
            f.write(text)
    old = mod.build_model(header, name="van_der_pol_v9", struct="VanDerPolV9", host_sim=True, out_dir=os.path.dirname(lib.path), verbose=False,
                          entry_defs=["-DI2C_NO_OPS_SIZE"])
    raw = ctypes.CDLL(old)
    assert hasattr(raw, "i2c_model_ops") and not hasattr(raw, "i2c_model_ops_size")
    mid, _ = lib.load_model(old)
    buf = ctypes.c_void_p(ctypes.addressof(_FLAG))
    assert lib.i2c_rollout_eval(ctypes.byref(flag_problem(mid)), buf, ctypes.byref(flag_eval()), None) == ENOTSUP
    assert lib.i2c_rollout_eval(ctypes.byref(flag_problem(mid)), buf, ctypes.byref(flag_eval(n_rollouts=0)), None) == EINVAL


def test_bench_tool_counts_bytes_from_shapes():
    """tools/bench_rollout_eval.py: the bytes each side allocates, from shapes -- the pendulum at T = 200, B = 4096 with 1 024 rollouts
    each (13 GB of noise in; 20 GB of states and actions and 27 GB of observations out), and evaluate()'s own buffers against what an
    engine allocates"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_rollout_eval", os.path.join(hostsim.ROOT, "tools", "bench_rollout_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    nin, nout = tool.bytes_rollout_way("PendulumKnown", 200, 4096, 1024, True)
    assert nin == 200 * 2 * 4096 * 1024 * 8 and round(nin / 1e9) == 13
    assert nout == (200 * 3 + 200 * 4 + 3) * 4096 * 1024 * 8 and round(nout / 1e9) == 20 + 27
    assert tool.parts_rule(1, 70000) == 65536 and tool.parts_rule(70, 5) == 5 and tool.parts_rule(70000, 5) == 1
    eng = solved("pendulum6", "cpu")
    out = eng.evaluate(5, seed=1, parts=2)
    held = [out["cost"], out["cost_mean"], out["n_bad"], eng._eval_work, out["xu_mean"]]
    n = sum(t.untyped_storage().nbytes() for t in held) + 12 * 6 * 6 * 8  # (xu_cov comes back unpacked: its packed rows)
    assert n == tool.bytes_evaluate("PendulumKnown", 12, 6, 5, True, parts=2)
