"""The grid family (csrc/i2c_grid.hpp, I2C_FAMILY_GRID): GaussHermiteQuadrature(n) with ONE WAVEFRONT per trajectory -- the 64 lanes
run the one-lane cell on the same trajectory, the n^d grid points of every transform are strided over them and the partial moments
summed across the wavefront. Asked for with group_lanes=64 under inference="gauss_hermite".

Every check runs on the host simulation of the kernels (CPU: the 64 lanes are 64 threads) and, marked `gpu`, on the HIP library:
  1. the reference's existing Gauss-Hermite goldens (27 points: 37 idle lanes; 64 points: exactly one pass; covariance control;
     the MPC ring) on the new family, at the tolerances of their one-lane tests;
  2. two new goldens from the reference, cartpole (243 points: 3 passes + 51) and double cartpole (2 187 points: 34 passes + 11),
     on the grid AND on the one-lane family (never pinned before for d >= 5), at the project's cartpole / double-cartpole tolerances;
  3. batches that are no multiple of the waves per workgroup, against the CPU oracle;
  4. grid against one-lane kernels on identical inputs, 1e-8 relative on every buffer (agreement between families);
  5. forward sweep of one family with the backward sweep of the other (same buffers);
  6. a trajectory that fails leaves its neighbours bit-identical;
  7. the resolver, including an out-of-tree model.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import load_case, rel_err

N = parity.pkg._native
FAMILY_TOL = 1e-8  # two kernel families on the same inputs


@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


@pytest.fixture(scope="module")
def hip():
    lib = parity.pkg.load_library()
    assert not lib.is_host_sim, "GPU tests must run the HIP build"
    return lib


def _is_grid(eng):
    assert (eng.forward_family, eng.backward_family, eng.kernel_family("propagate"), eng.backward_schedule) == ("grid", "grid", "grid", "fused")
    assert eng.work is None  # the fused walk: no chunk workspace


# ---- 1. the existing reference goldens on the new family -------------------------------------------------------------------------
OLD_GOLDEN = ["gh3_pendulum_T40", "gh4_linear_T30", "gh3_covctrl_T100"]


@pytest.mark.parametrize("name", OLD_GOLDEN)
def test_grid_vs_reference_golden_cpu(sim, name):
    _is_grid(parity.check_against_golden(name, sim, "cpu", 1e-7, 1e-6, group_lanes=64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", OLD_GOLDEN)
def test_grid_vs_reference_golden_gpu(hip, name):
    _is_grid(parity.check_against_golden(name, hip, "cuda", 1e-7, 1e-6, group_lanes=64))


def test_grid_mpc_replay_cpu(sim):
    from test_mpc import _replay

    pol = _replay("mpc_pendulum_fb_gh3", sim, "cpu", 1e-7, group_lanes=64)
    assert pol.engine.forward_family == pol.engine.backward_family == "grid"


@pytest.mark.gpu
def test_grid_mpc_replay_gpu():
    from test_mpc import _replay

    pol = _replay("mpc_pendulum_fb_gh3", None, "cuda", 1e-6, group_lanes=64)
    assert pol.engine.forward_family == pol.engine.backward_family == "grid"


# ---- 2. the new goldens (d = 5 and d = 7), grid and one-lane family --------------------------------------------------------------
NEW_GOLDEN = ["gh3_cartpole_T30", "gh3_dcp_T12"]


def _new_golden(name, lib, device, lanes):
    eng = parity.check_against_golden(name, lib, device, 1e-6, 1e-5, group_lanes=lanes)
    assert eng.forward_family == eng.backward_family == {64: "grid", -1: "lane"}[lanes]


@pytest.mark.parametrize("lanes", [64, -1], ids=["grid", "lane"])
@pytest.mark.parametrize("name", NEW_GOLDEN)
def test_gauss_hermite_d5_d7_vs_reference_golden_cpu(sim, name, lanes):
    _new_golden(name, sim, "cpu", lanes)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [64, -1], ids=["grid", "lane"])
@pytest.mark.parametrize("name", NEW_GOLDEN)
def test_gauss_hermite_d5_d7_vs_reference_golden_gpu(hip, name, lanes):
    _new_golden(name, hip, "cuda", lanes)


# ---- 3. batched and ragged -------------------------------------------------------------------------------------------------------
BATCHES = [("gh3_cartpole_T30", 5), ("gh3_pendulum_T40", 130)]  # neither B is a multiple of the four waves of a workgroup


@pytest.mark.parametrize("name,B", BATCHES)
def test_grid_batch_vs_oracle_cpu(sim, name, B):
    eng, _ = parity.check_batch_against_oracle(name, sim, "cpu", B=B, n_iters=2, tol=1e-6, group_lanes=64)
    _is_grid(eng)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", BATCHES)
def test_grid_batch_vs_oracle_gpu(hip, name, B):
    eng, _ = parity.check_batch_against_oracle(name, hip, "cuda", B=B, n_iters=2, tol=1e-6, group_lanes=64)
    _is_grid(eng)


# ---- 4. / 5. grid against lane on identical inputs, and the two mixed ------------------------------------------------------------
def _buffers(eng):
    out = {"post": eng.post, "fwd": eng.fwd, "term_stats": eng.term_stats, "alpha": eng.alpha, "xm": eng.xm, "zpost": eng.zpost,
           "prior_out": eng.prior_out, "cost": eng.costs_m[-1]}
    return {k: parity.np_(v) for k, v in out.items() if v is not None}


def _same_buffers(a, b, what):
    ba, bb = _buffers(a), _buffers(b)
    assert ba.keys() == bb.keys()
    for k in ba:
        assert np.all(np.isfinite(ba[k])), f"{what} {k}: non-finite"
        e = rel_err(ba[k], bb[k])
        assert e <= FAMILY_TOL, f"{what}: {k} differs by {e:.3e} relative (max-norm)"


def _engine_degree(case, degree):
    import json

    return type(case)({**dict(case), "meta": np.array(json.dumps({**case.meta, "gh_degree": degree}))})


def _grid_vs_lane_case(lib, device):
    """Cartpole, degree 4: 4^5 = 1 024 points, an exact multiple of 64 (no ragged pass); B = 3, T = 8, two iterations."""
    g = _engine_degree(parity.with_horizon(load_case("gh3_cartpole_T30"), 8), 4)
    x0, mu_u = parity.batched_inputs(g, 3)
    engs = [parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, group_lanes=lanes, keep_xm=True, keep_zpost=True) for lanes in (64, -1)]
    assert [e.forward_family for e in engs] == ["grid", "lane"] and engs[0].gh_degree == 4
    for it in range(2):
        for e in engs:
            e.learn_msgs()
        _same_buffers(engs[0], engs[1], f"cartpole degree 4, it{it + 1}")
    assert engs[0].failures() == engs[1].failures() == []


def test_grid_agrees_with_lane_cpu(sim):
    _grid_vs_lane_case(sim, "cpu")


@pytest.mark.gpu
def test_grid_agrees_with_lane_gpu(hip):
    _grid_vs_lane_case(hip, "cuda")


def _mixed_families(lib, device):
    """Forward sweep of one family, backward sweep of the other, through the C ABI on the buffers of ONE engine: the two families
    read and write the same [T][E][B] buffers (post_layout 0, forward messages as the one-lane kernels write them)."""
    g = load_case("gh3_cartpole_T30")
    ref = parity.engine_from_case(g, lib, device, group_lanes=-1, backward_mode="fused")  # (the walk the grid family does)
    ref.forward_sweep()
    ref.backward_sweep()
    for fwd_lanes, bwd_lanes in ((64, -1), (-1, 64)):
        eng = parity.engine_from_case(g, lib, device, group_lanes=-1, backward_mode="fused")
        p = eng._problem
        p.group_lanes = fwd_lanes
        assert lib.i2c_kernel_family(C.byref(p), N.SWEEP_FORWARD) == {64: N.FAMILY_GRID, -1: N.FAMILY_LANE}[fwd_lanes]
        eng._check(lib.i2c_forward_sweep(C.byref(p), eng._ptr(eng.prior), eng._ptr(eng.fwd), eng._ptr(eng.prior_out), eng._ptr(eng.status),
                                         eng._stream()), "i2c_forward_sweep")
        p.group_lanes, p.backward_mode = bwd_lanes, N.BWD_FUSED
        assert lib.i2c_kernel_family(C.byref(p), N.SWEEP_BACKWARD) == {64: N.FAMILY_GRID, -1: N.FAMILY_LANE}[bwd_lanes]
        eng._check(lib.i2c_backward_sweep(C.byref(p), eng._ptr(eng.fwd), eng._ptr(eng.xm), eng._ptr(eng.post), eng._ptr(eng.zpost),
                                          eng._ptr(eng.cell_stats), eng._ptr(eng.term_stats), eng._ptr(eng.status), eng._stream()),
                   "i2c_backward_sweep")
        assert eng.failures() == []
        for k in ("post", "fwd", "term_stats", "prior_out"):
            a, b = parity.np_(getattr(eng, k)), parity.np_(getattr(ref, k))
            assert np.all(np.isfinite(a))
            e = rel_err(a, b)
            assert e <= FAMILY_TOL, f"forward {fwd_lanes} + backward {bwd_lanes}: {k} differs by {e:.3e} relative"


def test_grid_and_lane_sweeps_mix_cpu(sim):
    _mixed_families(sim, "cpu")


@pytest.mark.gpu
def test_grid_and_lane_sweeps_mix_gpu(hip):
    _mixed_families(hip, "cuda")


# ---- 6. failure isolation --------------------------------------------------------------------------------------------------------
def _failure_isolation(lib, device):
    """B = 3 on the cartpole, trajectory 1 with an indefinite sig_x0: the same status word as the one-lane kernel gives, that
    trajectory NaN, trajectories 0 and 2 bit-identical to a clean run of those two alone."""
    g = parity.with_horizon(load_case("gh3_cartpole_T30"), 6)
    x0, mu_u = parity.batched_inputs(g, 3)
    bad = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, group_lanes=64)
    lane = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, group_lanes=-1)
    clean = parity.engine_from_case(g, lib, device, x0=x0[[0, 2]], mu_u=mu_u[[0, 2]], group_lanes=64)
    assert bad.forward_family == clean.forward_family == "grid" and lane.forward_family == "lane"
    for e in (bad, lane):
        e.sig_x0[0, 1] = -1.0  # sig_x0[0][0] of trajectory 1 (packed index 0): a negative variance
    for e in (bad, lane, clean):
        for _ in range(2):
            e.learn_msgs()
    f = bad.failures()
    assert [(b, reason) for b, reason, _ in f] == [(1, 1)], f  # I2C_FAIL_PRIOR_JOINT
    assert torch.equal(bad.status, lane.status), (bad.status, lane.status)
    assert clean.failures() == []
    for k in ("post", "fwd"):
        assert torch.equal(getattr(bad, k)[:, :, [0, 2]], getattr(clean, k)), k
    assert torch.equal(bad.alpha[[0, 2]], clean.alpha) and torch.equal(bad.term_stats[:, [0, 2]], clean.term_stats)
    assert not torch.isfinite(bad.post[:, :, 1]).all()


def test_grid_failure_isolation_cpu(sim):
    _failure_isolation(sim, "cpu")


@pytest.mark.gpu
def test_grid_failure_isolation_gpu(hip):
    _failure_isolation(hip, "cuda")


# ---- 7. the resolver -------------------------------------------------------------------------------------------------------------
def _resolver(lib, model_id):
    p = N.I2cProblem()
    p.abi_version, p.model_id, p.B, p.T, p.backward_mode, p.dtype = N.ABI_VERSION, model_id, 3, 20, N.BWD_AUTO, N.F64
    p.inference, p.gh_degree, p.group_lanes, p.post_layout, p.quad_alpha = N.INF_GAUSS_HERMITE, 3, 64, 0, 1.0
    fam = lambda sweep: lib.i2c_kernel_family(C.byref(p), sweep)  # noqa: E731
    assert fam(N.SWEEP_FORWARD) == fam(N.SWEEP_BACKWARD) == fam(N.SWEEP_PROPAGATE) == N.FAMILY_GRID == 5
    assert N.FAMILY_NAMES[N.FAMILY_GRID] == "grid"
    for mode in (N.BWD_AUTO, N.BWD_FUSED, N.BWD_CHUNKED, N.BWD_TWO_PASS):  # one schedule, whatever is asked for
        p.backward_mode = mode
        assert lib.i2c_backward_schedule(C.byref(p)) == N.BWD_FUSED
    p.backward_mode = N.BWD_AUTO
    # the filter step keeps the cubature rule and its family: the answer of the same problem without the request
    with_request = fam(N.SWEEP_FILTER)
    p.group_lanes = 0
    assert with_request == fam(N.SWEEP_FILTER) and with_request > 0 and with_request != N.FAMILY_GRID
    # group_lanes = 0 (and -1) under Gauss-Hermite: the one-lane kernels, as before
    assert fam(N.SWEEP_FORWARD) == fam(N.SWEEP_BACKWARD) == fam(N.SWEEP_PROPAGATE) == N.FAMILY_LANE
    p.group_lanes = -1
    assert fam(N.SWEEP_FORWARD) == fam(N.SWEEP_BACKWARD) == fam(N.SWEEP_PROPAGATE) == N.FAMILY_LANE
    # fp32-stored messages: not compiled
    p.group_lanes, p.dtype = 64, N.F64_F32S
    assert fam(N.SWEEP_FORWARD) == fam(N.SWEEP_BACKWARD) == -2 and lib.i2c_backward_schedule(C.byref(p)) == -2  # I2C_ENOTSUP
    # the cubature rule with the same request is not the grid family's
    p.dtype, p.inference = N.F64, N.INF_CUBATURE
    assert fam(N.SWEEP_FORWARD) != N.FAMILY_GRID


@pytest.mark.parametrize("model", ["PendulumKnown", "CartpoleKnown", "DoubleCartpoleKnown", "PlanarQuadrotor"])
def test_grid_resolver_cpu(sim, model):
    _resolver(sim, N.MODEL_IDS[model])


@pytest.mark.gpu
def test_grid_resolver_gpu(hip):
    _resolver(hip, N.MODEL_IDS["CartpoleKnown"])


def _plugin(lib, device):
    """The van-der-Pol model of tests/test_model_plugin.py, built from its header as that test builds it: the grid kernels are
    instantiated inside the library's kernel layer, so an out-of-tree model gets them without a change to the model ABI."""
    import test_model_plugin as tp

    p = tp.problem(B=3, T=12)
    eng = parity.pkg.BatchedI2c(tp.make_env_model(tp.VanDerPolKnown()), p["T"], p["Q"], p["R"], p["Qf"], p["alpha"], p["tol"], p["mu_u"],
                                p["sig_u"], x0=p["x0"], device=device, lib=lib, inference="gauss_hermite", gh_degree=3, group_lanes=64)
    assert eng.model_id >= N.PLUGIN_BASE
    _is_grid(eng)
    _resolver(lib, eng.model_id)
    eng.learn_msgs()
    assert eng.failures() == []
    assert all(torch.isfinite(t).all() for t in (eng.post, eng.fwd, eng.alpha, eng.costs_m[-1]))


def test_grid_plugin_model_cpu(sim):
    _plugin(sim, "cpu")


@pytest.mark.gpu
def test_grid_plugin_model_gpu(hip):
    _plugin(hip, "cuda")
