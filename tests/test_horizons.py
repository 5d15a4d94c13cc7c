"""Per-trajectory horizons (I2cProblem.horizons; BatchedI2c(horizons=...)): trajectory b of a batch consists of cells
0 .. horizons[b] - 1 and its result is what a solve of that trajectory alone with that horizon computes.

Every comparison covers every existing cell (t < horizons[b]) of every output -- the posterior mean and covariance, K, k, sigK, the
forward messages, xm, zpost, cell_stats, alpha and the M-step statistics -- and no other cell. The kernel cases run on the host
simulation (CPU) and, marked `gpu`, on the HIP library at the same shapes.

  1  against the CPU oracle, one trajectory at a time, each oracle solved at its own horizon
  2  against the real reference: trajectory 0 of a mixed batch reproduces a golden
  3  a lane depends on nothing but its own trajectory, bit for bit (a full wave of short lanes plus a partial wave; permutation)
  4  all horizons equal to T agrees with the same problem without horizons (different instantiations: 1e-8)
  5  nothing is written or read beyond a horizon (NaN canaries)
  6  learn(n) == n x learn_msgs() bitwise; a deterministic rollout of a mixed batch equals the solo rollouts bitwise
  7  the resolver's answers and every refusal, through the C API with scalar fields only, and the engine's ValueErrors
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import Case, load_case, oracle_from_case
from test_feature_matrix import make_case

pkg = parity.pkg
N = pkg._native
np_ = parity.np_

PENDULUM = ("em_pendulum_T200", 12, None, [1, 2, 7, 12, 12])          # d = 3: the prefetch and double-buffer paths
DCP = ("em_dcp_T60", 9, None, [1, 5, 9])                              # d = 7: a cell loads its rows at its own top
LINEAR_PRIOR = ("em_linear_T60", 10, "terminal_prior", [1, 4, 10])    # a terminal state prior next to the terminal cost
LINEAR_PRIOR_ONLY = ("em_linear_T60", 10, "terminal_prior_only", [1, 4, 10])
PENDULUM_PROP = ("em_pendulum_T200", 12, "propagate", [1, 2, 7, 12, 12])
# (detail, summary) tolerances on the GPU: what tests/test_hip_parity.py gives the same golden
GPU_TOL = {"em_pendulum_T200": (1e-8, 1e-7), "em_dcp_T60": (1e-6, 1e-5), "em_linear_T60": (1e-8, 1e-7),
           "em_cartpole_T100": (1e-6, 1e-5), "em_quadrotor_T20": (1e-6, 1e-5)}
FWD = parity.FWD
PROP = ["mu_xu0_pf", "sig_xu0_pf", "mu_x3_pf", "sig_x3_pf"]


@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


@pytest.fixture(scope="module")
def hip():
    lib = pkg.load_library()
    assert not lib.is_host_sim
    return lib


def cut_case(name, T, variant=None):
    """A golden cut to T cells, as tests/test_feature_matrix.py cuts them (its variants included)."""
    if variant is None:
        g = load_case(name)
        return Case({**dict(g), "meta": np.array(json.dumps(dict(g.meta, T=T))), "mu_u": g["mu_u"][:T]})
    case = make_case(name, T, variant)
    assert not isinstance(case, str), case
    return case


def make_engine(case, lib, device, x0, mu_u, horizon=None, keep_prior=True, **kw):
    """parity.engine_from_case with every optional output of the sweeps kept (xm, zpost, cell_stats)."""
    meta = case.meta
    eng = pkg.BatchedI2c(parity.product_model(case), meta["T"] if horizon is None else horizon, case.get("Q"), case["R"], case.get("Qf"),
                         meta["alpha"], meta["tol"], mu_u, case["sig_u"], case.get("mu_x_term"), case.get("sig_x_term"),
                         quad=tuple(meta["quad"]), x0=x0, device=device, lib=lib, keep_prior=keep_prior, keep_xm=True, keep_zpost=True, **kw)
    eng._propagate = bool(meta.get("propagate"))
    if "use_expert_controller" in meta:
        eng.use_expert_controller = bool(meta["use_expert_controller"])
    eng.cell_stats = torch.zeros(eng.H, 2, eng.B, dtype=eng.dtype, device=eng.device)  # (an optional output of the fused walk)
    return eng


def per_cell(eng):
    """name -> (B, T, ...) tensor of every per-cell output"""
    out = dict(eng.forward_messages())
    out["mu_xu0_m"], out["sig_xu0_m"] = eng.marginal_state_action()
    out["K"], out["k"], out["sigK"] = eng.local_linear_policy()
    out["mu_x3_m"], out["sig_x3_m"] = eng.smoothed_next_state()
    out["mu_z0_m"], out["sig_z0_m"] = eng.observed_marginal()
    out["cell_cost"] = eng.cell_stats.permute(2, 0, 1)
    if eng.prior_out is not None:
        out["mu_xu0_f"], out["sig_xu0_f"] = eng.prior_state_action()
    if eng.prop is not None:
        out.update(eng.propagated())
    return out


def per_trajectory(eng):
    """name -> (B, ...) tensor: the temperature, the M-step's statistics, the backward sweep's sums and terminal moments"""
    out = {"alpha": eng.alpha, "mstep": eng.stats_out.T, "term_stats": eng.term_stats[: eng.e_term - 1].T, "status": eng.status}
    if eng.prop_stats is not None:
        out["prop_stats"] = eng.prop_stats.T
    return out


def solo_oracle(case, x0, mu_u, b, Tb, z=None):
    """The oracle of trajectory b alone at its own horizon (z: (B, T, nz) per-cell targets of the batch, or None)."""
    meta = dict(case.meta, T=int(Tb))
    over = {} if z is None else {"z_traj": z[b:b + 1, :Tb]}
    return oracle_from_case(Case({**dict(case), "meta": np.array(json.dumps(meta)), "mu_u": mu_u[b, :Tb]}), x0=x0[b:b + 1], **over)


def masked_rel_err(a, ref, valid):
    """max-norm relative error over the existing cells (the feature matrix's norm on them)"""
    a, ref = np.asarray(a, float)[valid], np.asarray(ref, float)[valid]
    assert np.all(np.isfinite(a)), "non-finite value in an existing cell"
    return float(np.max(np.abs(a - ref)) / (np.max(np.abs(ref)) + 1e-300))


def run_vs_oracles(lib, device, spec, tol_d, tol_p, tol_s):
    name, T, variant, horizons = spec
    compare_with_oracles(lib, device, cut_case(name, T, variant), horizons, tol_d, tol_p, tol_s, what=f"{name}/{variant}")


def compare_with_oracles(lib, device, case, horizons, tol_d, tol_p, tol_s, z=None, calibrate=False, what=""):
    """Three EM iterations of a mixed batch against one oracle per trajectory, solved at that trajectory's horizon: every existing cell
    of every per-cell output, the temperature, the M-step's statistics and the costs. z: (B, T, nz) per-cell targets. calibrate (cases
    with propagation): calibrate_alpha() before the first iteration, the temperature against each oracle's calibrate_alpha()."""
    T, B = case.meta["T"], len(horizons)
    x0, mu_u = parity.batched_inputs(case, B)
    eng = make_engine(case, lib, device, x0, mu_u, horizons=horizons, z_traj=z)
    assert eng.forward_family == eng.backward_family == "lane" and eng.backward_schedule == "fused"
    oras = [solo_oracle(case, x0, mu_u, b, Tb, z) for b, Tb in enumerate(horizons)]
    valid = np_(eng.valid_cells()).astype(bool)
    assert valid.sum() == sum(horizons)
    prop = bool(case.meta.get("propagate"))

    def check_scalars(scalars, it):
        for k, a, get in scalars:
            ref = np.array([np.asarray(get(o)).reshape(-1)[0] for o in oras])
            e = masked_rel_err(np_(a), ref, np.ones(B, bool))
            print(f"{what} it{it} {k}: {e:.2e}")
            assert e <= tol_s, f"{what} it{it} {k}: {e:.2e} > {tol_s:.0e}"

    if calibrate:
        assert prop
        eng.calibrate_alpha()
        for o in oras:
            o.calibrate_alpha()
        check_scalars([("calibrated alpha", eng.alpha, lambda o: o.alpha)], 0)
    elif prop:
        eng.propagate()
        for o in oras:
            o.propagate()
    keys = FWD + ["mu_xu0_m", "sig_xu0_m", "K", "k", "sigK", "mu_x3_m", "sig_x3_m", "mu_z0_m", "sig_z0_m"] + (PROP if prop else [])
    for it in range(1, 4):
        eng.learn_msgs()
        for o in oras:
            o.learn_msgs()
        got = per_cell(eng)

        def padded(get):
            first = np.asarray(get(oras[0]))[0]
            ref = np.full((B, T) + first.shape[1:], np.nan)
            for b, o in enumerate(oras):
                ref[b, : horizons[b]] = np.asarray(get(o))[0]
            return ref

        for k in keys:
            e = masked_rel_err(np_(got[k]), padded(lambda o, k=k: getattr(o, k)), valid)
            tol = tol_p if k in ("K", "k", "sigK") else tol_d
            print(f"{what} it{it} {k}: {e:.2e}")
            assert e <= tol, f"{what} it{it} {k}: {e:.2e} > {tol:.0e}"
        cost = np.stack([padded(lambda o, i=i: o._gaussian_cost(o.mu_z0_m, o.sig_z0_m)[i]) for i in (0, 1)], axis=-1)
        e = masked_rel_err(np_(got["cell_cost"]), cost, valid)
        assert e <= tol_d, f"{what} it{it} cell_stats: {e:.2e}"
        scalars = [("alpha", eng.alpha, lambda o: o.alpha), ("alpha_hat", eng.stats_out[0], lambda o: o.alphas_desired[-1]),
                   ("alpha_new", eng.stats_out[1], lambda o: o.alphas[-1]), ("cost", eng.stats_out[2], lambda o: o.costs_m[-1]),
                   ("cost_var", eng.stats_out[3], lambda o: o.costs_m_var[-1])]
        if prop:
            scalars += [("cost_pf", eng.prop_stats[0], lambda o: o.costs_pf[-1]), ("cost_pf_var", eng.prop_stats[1], lambda o: o.costs_pf_var[-1]),
                        ("alpha_pf", eng.alphas_pf[-1], lambda o: o.alphas_pf[-1])]
        if eng.has_x_terminal:
            scalars += [("kl", eng.kl_terms[-1], lambda o: o.kl_terms[-1])]
        check_scalars(scalars, it)
    assert eng.failures() == []
    return eng


ORACLE_CASES = [PENDULUM, DCP, LINEAR_PRIOR, LINEAR_PRIOR_ONLY, PENDULUM_PROP]
IDS = ["pendulum", "double_cartpole", "linear_terminal_prior", "linear_terminal_prior_only", "pendulum_propagate"]


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ORACLE_CASES, ids=IDS)
def test_hostsim_each_trajectory_against_its_oracle(sim, spec):
    run_vs_oracles(sim, "cpu", spec, 1e-7, 1e-7, 1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", ORACLE_CASES, ids=IDS)
def test_gpu_each_trajectory_against_its_oracle(hip, spec):
    tol_d, tol_s = GPU_TOL[spec[0]]
    run_vs_oracles(hip, "cuda", spec, tol_d, 10 * tol_d, tol_s)


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
GOLDENS = [("em_pendulum_T30_tau7", [30, 11, 3], 1e-8, 1e-7), ("em_covctrl_qf_T40", [40, 11, 3], 1e-7, 1e-6)]


def run_golden(lib, device, name, horizons, tol_d, tol_s):
    g = load_case(name)
    assert g.meta["T"] == horizons[0]
    x0, mu_u = parity.batched_inputs(g, len(horizons))
    eng = parity.check_against_golden(name, lib, device, tol_d, tol_s, x0=x0, mu_u=mu_u, horizons=horizons)
    assert eng.horizons.tolist() == horizons and eng.backward_schedule == "fused"


@pytest.mark.parametrize("name,horizons,tol_d,tol_s", GOLDENS)
def test_hostsim_golden_in_a_mixed_batch(sim, name, horizons, tol_d, tol_s):
    run_golden(sim, "cpu", name, horizons, tol_d, tol_s)


@pytest.mark.gpu
@pytest.mark.parametrize("name,horizons,tol_d,tol_s", GOLDENS)
def test_gpu_golden_in_a_mixed_batch(hip, name, horizons, tol_d, tol_s):
    run_golden(hip, "cuda", name, horizons, tol_d, tol_s)


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
# one full wave of short lanes (horizons cycling over 1 .. 5) plus a partial wave
LANES = [("em_pendulum_T200", 12, 70, [12, 1, 12, 6, 2, 12], [0, 4, 63, 64, 65, 69]),
         ("em_dcp_T60", 9, 66, [9, 1], [0, 4, 63, 64, 65])]


def assert_same_bits(a, b, Tb, what):
    """trajectory 0 of the solo engine `b` against one trajectory of the batch, `a`: the existing cells, bit for bit"""
    for k, v in a.items():
        w = b[k]
        x, y = (v[:Tb], w[0, :Tb]) if v.dim() >= 1 and k in CELL_KEYS else (v, w[0])
        assert torch.equal(x, y), f"{what}: {k} differs in its bits"


CELL_KEYS = set(FWD + PROP + ["mu_xu0_m", "sig_xu0_m", "K", "k", "sigK", "mu_x3_m", "sig_x3_m", "mu_z0_m", "sig_z0_m", "cell_cost",
                              "mu_xu0_f", "sig_xu0_f"])


def solved(case, lib, device, x0, mu_u, horizons, horizon=None, n_iter=2, **kw):
    eng = make_engine(case, lib, device, x0, mu_u, horizon=horizon, horizons=horizons, **kw)
    for _ in range(n_iter):
        eng.learn_msgs()
    assert eng.failures() == []
    return eng


def run_lane_independence(lib, device, name, T, B, tail, picks, variant=None, z=None, params=None):
    """z: (B, T, nz) per-cell targets, params: (B, NP) per-trajectory model parameters -- each picked trajectory is solved alone with
    its own rows of both, and the permutation permutes them with the rest."""
    case = cut_case(name, T, variant)
    horizons = [i % 5 + 1 for i in range(64)] + tail
    assert len(horizons) == B
    x0, mu_u = parity.batched_inputs(case, B)
    rows = lambda idx, Tb=T: {**({} if z is None else {"z_traj": z[idx, :Tb]}),  # noqa: E731
                              **({} if params is None else {"model_params": params[idx]})}
    eng = solved(case, lib, device, x0, mu_u, horizons, **rows(slice(None)))
    cells, traj = per_cell(eng), per_trajectory(eng)
    for b in picks:
        Tb = horizons[b]
        solo = solved(case, lib, device, x0[b:b + 1], mu_u[b:b + 1, :Tb], [Tb], horizon=Tb, **rows(slice(b, b + 1), Tb))
        assert_same_bits({k: v[b] for k, v in cells.items()}, per_cell(solo), Tb, f"{name} b={b} T_b={Tb}")
        assert_same_bits({k: v[b] for k, v in traj.items()}, per_trajectory(solo), Tb, f"{name} b={b} T_b={Tb}")
    # permuting the batch permutes the results
    perm = np.random.default_rng(7).permutation(B)
    other = solved(case, lib, device, x0[perm], mu_u[perm], [horizons[i] for i in perm], **rows(perm))
    valid = other.valid_cells()
    p = torch.as_tensor(perm, device=eng.device)
    assert torch.equal(valid, eng.valid_cells()[p])
    for k, v in per_cell(other).items():
        assert torch.equal(v[valid], cells[k][p][valid]), f"{name}: {k} of the permuted batch differs in its bits"
    for k, v in per_trajectory(other).items():
        assert torch.equal(v, traj[k][p]), f"{name}: {k} of the permuted batch differs in its bits"


@pytest.mark.parametrize("name,T,B,tail,picks", LANES, ids=["pendulum", "double_cartpole"])
def test_hostsim_a_lane_depends_on_its_own_trajectory_only(sim, name, T, B, tail, picks):
    run_lane_independence(sim, "cpu", name, T, B, tail, picks)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B,tail,picks", LANES, ids=["pendulum", "double_cartpole"])
def test_gpu_a_lane_depends_on_its_own_trajectory_only(hip, name, T, B, tail, picks):
    run_lane_independence(hip, "cuda", name, T, B, tail, picks)


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
def run_full_horizons(lib, device, spec):
    name, T, variant, horizons = spec
    case = cut_case(name, T, variant)
    B = len(horizons)
    x0, mu_u = parity.batched_inputs(case, B)
    a = make_engine(case, lib, device, x0, mu_u, horizons=[T] * B)
    b = make_engine(case, lib, device, x0, mu_u, group_lanes=-1, backward_mode="fused")
    assert b.horizons is None and bool(b.valid_cells().all())
    for _ in range(3):
        a.learn_msgs()
        b.learn_msgs()
    ca, cb = per_cell(a), per_cell(b)
    for k in ca:
        parity.assert_close(np_(ca[k]), np_(cb[k]), 1e-8, f"{name}: {k}, all horizons = T against no horizons")
    for k, v in per_trajectory(a).items():
        parity.assert_close(np_(v), np_(per_trajectory(b)[k]), 1e-8, f"{name}: {k}, all horizons = T against no horizons")


@pytest.mark.parametrize("spec", [PENDULUM, DCP], ids=["pendulum", "double_cartpole"])
def test_hostsim_all_horizons_equal_to_T(sim, spec):
    run_full_horizons(sim, "cpu", spec)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [PENDULUM, DCP], ids=["pendulum", "double_cartpole"])
def test_gpu_all_horizons_equal_to_T(hip, spec):
    run_full_horizons(hip, "cuda", spec)


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
def run_canaries(lib, device, spec, z=None):
    """z: (B, T, nz) per-cell targets; None: the model's own target in every cell of every trajectory"""
    name, T, _, horizons = spec
    case = cut_case(name, T, "propagate")
    B = len(horizons)
    x0, mu_u = parity.batched_inputs(case, B)
    zg = np.asarray(parity.product_model(case).zg, float).reshape(-1)
    eng = make_engine(case, lib, device, x0, mu_u, horizons=horizons, z_traj=np.broadcast_to(zg, (B, T, zg.size)) if z is None else z)
    eng.prop = torch.zeros(T, eng.dims.e_prop, B, dtype=eng.dtype, device=eng.device)
    eng.prop_stats = torch.zeros(3, B, dtype=eng.dtype, device=eng.device)
    valid = eng.valid_cells()
    outputs = {"fwd": eng.fwd, "xm": eng.xm, "zpost": eng.zpost, "cell_stats": eng.cell_stats, "prior_out": eng.prior_out, "prop": eng.prop}
    inputs = {"post": eng.post, "z": eng.z}  # (persistent: initialised by the engine, read by the sweeps)
    for k, buf in {**outputs, **inputs}.items():
        assert buf.shape[0] == T and buf.shape[2] == B, k
        buf.permute(2, 0, 1)[~valid] = float("nan")
    for _ in range(2):
        eng.learn_msgs()
    for k, buf in {**outputs, **inputs}.items():
        v = buf.permute(2, 0, 1)
        assert bool(torch.isnan(v[~valid]).all()), f"{k}: a row beyond a horizon was written"
        assert bool(torch.isfinite(v[valid]).all()), f"{k}: an existing cell is not finite (a row beyond a horizon was read)"
    for k, v in per_trajectory(eng).items():
        assert bool(torch.isfinite(v.to(torch.float64)).all()), k
    assert eng.failures() == []


@pytest.mark.parametrize("spec", [PENDULUM, DCP], ids=["pendulum", "double_cartpole"])
def test_hostsim_nothing_beyond_a_horizon_is_touched(sim, spec):
    run_canaries(sim, "cpu", spec)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [PENDULUM, DCP], ids=["pendulum", "double_cartpole"])
def test_gpu_nothing_beyond_a_horizon_is_touched(hip, spec):
    run_canaries(hip, "cuda", spec)


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
def run_learn_and_rollout(lib, device, spec):
    name, T, _, horizons = spec
    case = cut_case(name, T)
    B = len(horizons)
    x0, mu_u = parity.batched_inputs(case, B)
    a = make_engine(case, lib, device, x0, mu_u, keep_prior=False, horizons=horizons)
    b = make_engine(case, lib, device, x0, mu_u, keep_prior=False, horizons=horizons)
    a.learn(3)
    for _ in range(3):
        b.learn_msgs()
    valid = a.valid_cells()
    cb = per_cell(b)
    for k, v in per_cell(a).items():
        assert torch.equal(v[valid], cb[k][valid]), f"{name}: learn(3) and 3 x learn_msgs() differ in {k}"
    for hist in ("alphas", "alphas_desired", "costs_m", "costs_m_var"):
        ha, hb = torch.stack(getattr(a, hist)), torch.stack(getattr(b, hist))
        assert torch.equal(ha, hb), f"{name}: learn(3) and 3 x learn_msgs() differ in {hist}"
    assert torch.equal(a.alpha, b.alpha) and a.failures() == [] and b.failures() == []
    # the controllers of the mixed batch rolled out without noise: each trajectory as its solo engine rolls it out
    ra = a.rollout(1, process_noise=False)
    for bi, Tb in enumerate(horizons):
        solo = make_engine(case, lib, device, x0[bi:bi + 1], mu_u[bi:bi + 1, :Tb], horizon=Tb, keep_prior=False, horizons=[Tb])
        solo.learn(3)
        rs = solo.rollout(1, process_noise=False)
        for k in ("x_final", "z_term"):
            if ra[k] is not None:
                assert torch.equal(ra[k][0, bi], rs[k][0, 0]), f"{name} b={bi}: rollout {k}"
        for k in ("xu", "z"):
            assert torch.equal(ra[k][0, bi, :Tb], rs[k][0, 0]), f"{name} b={bi}: rollout {k}"


@pytest.mark.parametrize("spec", [PENDULUM, DCP], ids=["pendulum", "double_cartpole"])
def test_hostsim_learn_and_rollout(sim, spec):
    run_learn_and_rollout(sim, "cpu", spec)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [PENDULUM, DCP], ids=["pendulum", "double_cartpole"])
def test_gpu_learn_and_rollout(hip, spec):
    run_learn_and_rollout(hip, "cuda", spec)


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
ENOTSUP, EINVAL = -2, -1
_FLAG = (ctypes.c_int32 * 4)(1, 1, 1, 1)  # the resolvers only test the pointer against NULL


def shape(model_id=0, B=4, T=20, mode=0, inference=0, dtype=0, group_lanes=0, horizons=True, **fields):
    """An I2cProblem with its scalar fields only, as tests/test_abi.py builds them, plus the horizons flag"""
    p = N.I2cProblem()
    p.abi_version, p.model_id, p.B, p.T, p.backward_mode, p.inference, p.dtype = N.ABI_VERSION, model_id, B, T, mode, inference, dtype
    p.group_lanes, p.gh_degree, p.terminal_cell = group_lanes, 3, T - 1
    p.quad_alpha, p.quad_beta, p.quad_kappa = 1.0, 0.0, 0.0
    if horizons:
        p.horizons = ctypes.addressof(_FLAG)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def test_abi_size_and_version():
    lib = pkg.load_library()
    assert lib.i2c_abi_version() == 9 == N.ABI_VERSION
    assert lib.i2c_problem_size() == ctypes.sizeof(N.I2cProblem)
    assert N.I2cProblem._fields_[-1][0] == "horizons"  # appended at the END
    assert not N.I2cProblem().horizons                 # a zeroed problem: no horizons


def test_resolver_with_horizons():
    lib = pkg.load_library()
    fam = lambda p, sweep: lib.i2c_kernel_family(ctypes.byref(p), sweep)  # noqa: E731
    sched = lambda p: lib.i2c_backward_schedule(ctypes.byref(p))  # noqa: E731
    for model_id in (0, 2, 3, 4, 6):  # pendulum, cartpole, double cartpole, linear, planar quadrotor
        for B in (1, 300, 4096, 40000):
            for lanes in (0, -1):
                for mode in (N.BWD_AUTO, N.BWD_CHUNKED, N.BWD_TWO_PASS, N.BWD_FUSED):
                    p = shape(model_id, B=B, T=40, mode=mode, group_lanes=lanes)
                    assert [fam(p, s) for s in (N.SWEEP_FORWARD, N.SWEEP_BACKWARD, N.SWEEP_PROPAGATE)] == [1, 1, 1], (model_id, B, lanes, mode)
                    assert sched(p) == N.BWD_FUSED
                    assert fam(p, N.SWEEP_CHUNK_PASSES) == ENOTSUP  # no chunked schedule runs
    # general cubature weights are served; terminal_cell = -1 (no terminal update) as well
    assert sched(shape(0, quad_alpha=1.2, quad_beta=0.44, quad_kappa=0.5)) == N.BWD_FUSED
    assert sched(shape(0, terminal_cell=-1)) == N.BWD_FUSED
    # ... on every served model, also the rule whose weights do not sum to one (tests/test_horizons_options.py solves with both)
    for model_id in (0, 2, 3, 4, 6):
        for qa, qb, qk in ((1.2, 0.44, 0.5), (1.05, 0.0, 0.3)):
            for lanes in (0, -1):
                p = shape(model_id, group_lanes=lanes, quad_alpha=qa, quad_beta=qb, quad_kappa=qk)
                assert [fam(p, s) for s in (N.SWEEP_FORWARD, N.SWEEP_BACKWARD, N.SWEEP_PROPAGATE)] == [1, 1, 1], (model_id, qa, lanes)
                assert sched(p) == N.BWD_FUSED, (model_id, qa, lanes)
    # without horizons nothing changes: the default schedule of a small batch is the chunked one
    assert sched(shape(0, B=4096, T=200, horizons=False)) == N.BWD_CHUNKED


def refusals(lib):
    from noise_models import PendulumInputNoiseKnown

    noise_id = PendulumInputNoiseKnown().resolve_model_id(lib)
    d3 = lib.query(3)
    return [
        ("group kernels", shape(3, group_lanes=d3.group_lanes), ENOTSUP),
        ("quad / wave request", shape(3, group_lanes=64), ENOTSUP),
        ("quad forward request", shape(3, group_lanes=N.LANES_QUAD), ENOTSUP),
        ("grid request", shape(0, group_lanes=64, inference=N.INF_GAUSS_HERMITE), ENOTSUP),
        ("group_only model", shape(7, post_layout=1), ENOTSUP),
        ("group_only model, one lane asked for", shape(7, group_lanes=-1), ENOTSUP),
        ("Linearize", shape(0, inference=N.INF_LINEARIZE), ENOTSUP),
        ("Gauss-Hermite", shape(0, inference=N.INF_GAUSS_HERMITE), ENOTSUP),
        ("fp32", shape(0, dtype=N.F32), ENOTSUP),
        ("fp32 storage", shape(0, dtype=N.F64_F32S), ENOTSUP),
        ("process_noise", shape(noise_id), ENOTSUP),
        ("t0 != 0", shape(0, t0=3), EINVAL),
        ("alpha_cell", shape(0, alpha_cell=ctypes.addressof(_FLAG)), EINVAL),
        ("terminal_cell mid-horizon", shape(0, terminal_cell=7), EINVAL),
    ]


def test_refusals_through_the_c_api():
    lib = pkg.load_library()
    for what, p, code in refusals(lib):
        assert lib.i2c_backward_schedule(ctypes.byref(p)) == code, what
        for sweep in (N.SWEEP_FORWARD, N.SWEEP_BACKWARD, N.SWEEP_PROPAGATE):
            assert lib.i2c_kernel_family(ctypes.byref(p), sweep) == code, what
    # the entry points of the MPC ring and the Riccati messages: refused before any launch (every buffer is a flag here)
    p = shape(0, inference=N.INF_LINEARIZE)
    buf = ctypes.c_void_p(ctypes.addressof(_FLAG))
    for name in ("x0", "sig_x0", "alpha", "feedforward"):
        setattr(p, name, buf.value)
    assert lib.i2c_riccati_sweep(ctypes.byref(p), buf, buf, buf, buf, buf, buf, None) == EINVAL
    p = shape(0)
    for name in ("x0", "sig_x0", "alpha", "feedforward"):
        setattr(p, name, buf.value)
    st = N.I2cMpcStep()
    st.post = st.fwd = st.term_stats = st.cell_init = st.status = st.action = buf.value
    assert lib.i2c_mpc_step(ctypes.byref(p), ctypes.byref(st), None) == EINVAL
    assert lib.i2c_shift_horizon(ctypes.byref(p), buf, buf, None, None, None, None) == EINVAL
    ep = N.I2cEpisode()
    ep.n_steps, ep.observe_state = 0, 1
    ep.x_true = ep.u = ep.cost = buf.value
    assert lib.i2c_mpc_episode(ctypes.byref(p), ctypes.byref(st), ctypes.byref(ep), None) == EINVAL
    # ... and the same calls without horizons pass their argument checks (n_steps = 0: nothing is launched)
    p.horizons = None
    assert lib.i2c_mpc_episode(ctypes.byref(p), ctypes.byref(st), ctypes.byref(ep), None) == 0


def test_engine_refuses_before_it_allocates(sim, monkeypatch):
    case = cut_case("em_pendulum_T200", 12)
    x0, mu_u = parity.batched_inputs(case, 3)

    def no_alloc(*a, **k):
        raise AssertionError("the engine allocated before it validated")

    def build(**kw):
        with monkeypatch.context() as m:
            m.setattr(torch, "zeros", no_alloc)
            m.setattr(torch, "as_tensor", no_alloc)
            return make_engine(case, sim, "cpu", x0, mu_u, **kw)

    for bad in ([1, 2], [1, 2, 3, 4], [0, 2, 3], [1, 2, 13], [1.5, 2, 3]):
        with pytest.raises(ValueError, match="horizons"):
            build(horizons=bad)
    for kw, drop in ((dict(group_lanes=True), "group_lanes"), (dict(group_lanes=64), "group_lanes"), (dict(inference="linearize"), "inference"),
                     (dict(inference="gauss_hermite", gh_degree=3), "inference"), (dict(storage_dtype=torch.float32), "float32"),
                     (dict(dtype=torch.float32, allow_inexact=True), "float32")):
        with pytest.raises(ValueError, match=drop):
            build(horizons=[1, 2, 12], **kw)
    # a model with process_noise, and one without one-lane kernels
    from i2c.known_models import make_env_model
    from noise_models import PendulumInputNoiseKnown

    with monkeypatch.context() as m:
        m.setattr(torch, "zeros", no_alloc)
        with pytest.raises(ValueError, match="process_noise"):
            pkg.BatchedI2c(PendulumInputNoiseKnown(), 12, case.get("Q"), case["R"], case.get("Qf"), 100.0, 0.0, mu_u, case["sig_u"], x0=x0,
                           device="cpu", lib=sim, horizons=[1, 2, 12])
        q = make_env_model("Quadrotor12")
        with pytest.raises(ValueError, match="one-lane"):
            pkg.BatchedI2c(q, 12, np.eye(12), np.eye(4), np.eye(12), 1.0, 0.5, np.zeros((3, 12, 4)), np.eye(4), device="cpu", lib=sim,
                           horizons=[1, 2, 12])
    # accepted: deterministic_family and every backward_mode resolve to the one-lane kernels and the fused walk
    for kw in (dict(deterministic_family=True), dict(backward_mode="chunked"), dict(backward_mode="two_pass"), dict(group_lanes=-1)):
        eng = make_engine(case, sim, "cpu", x0, mu_u, horizons=[1, 2, 12], **kw)
        assert (eng.forward_family, eng.backward_family, eng.kernel_family("propagate"), eng.backward_schedule) == ("lane", "lane", "lane", "fused")
        assert eng.work is None
    # the ring of the MPC loop and the per-cell temperatures stay with the single horizon
    eng = make_engine(case, sim, "cpu", x0, mu_u, horizons=[1, 2, 12])
    for call in (eng.enable_per_cell_alpha, eng.shift_horizon, lambda: eng.mpc_step(1), eng.riccati_sweep):
        with pytest.raises(ValueError, match="horizons"):
            call()
    # set_horizons: in place, validated like the constructor's
    eng.set_horizons([3, 3, 4])
    assert eng.horizons.tolist() == [3, 3, 4] and eng.valid_cells().sum().item() == 10
    with pytest.raises(ValueError, match="horizons"):
        eng.set_horizons([3, 3, 40])
    plain = make_engine(case, sim, "cpu", x0, mu_u)
    assert plain.horizons is None and plain.backward_schedule != "fused"
    plain.set_horizons([12, 5, 1])
    assert plain.backward_schedule == "fused" and plain.valid_cells().sum().item() == 18
    plain.learn_msgs()
    assert plain.failures() == []
