"""learn(3) by ONE i2c_learn call against three learn_msgs() calls on a twin engine, bit for bit: every tail of the backward sweep.

Inside i2c_learn the sweeps of an iteration are coupled (csrc/i2c_impl.hpp, Impl::launches): the M-step rides on the reduction
kernel of the two-pass and chunked schedules or runs as k_mstep behind a walk without one, behind self-stitching walkers the next
forward sweep finishes reduction and M-step, and that sweep's helper wave composes the chunks of the backward sweep behind it. The
stepwise calls run the same kernels' bodies uncoupled -- forward sweep, stand-alone backward sweep, k_mstep --, so every output and
every row of the statistics history is compared with torch.equal, one case per tail at the smallest shape that still has it: 9
cells (two chunks, 5 + 4) and five trajectories; the 12-state quadrotor 5 cells and three trajectories.

Shared bodies; test_hostsim_* run the host simulation of the kernel code on the CPU, test_hip_* the same bodies on the GPU."""
import re

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import load_case
from test_forward_helper import env

pkg = parity.pkg
QUAD = pkg._native.LANES_QUAD


def make_engine(lib, device, name, T, B, **kw):
    """The golden case `name` over T cells, B trajectories, under its own inference rule (make_engine of
    tests/test_chunk_self_stitch.py without that file's forced family and schedule): no joint-prior output, with which
    BatchedI2c.learn would step through learn_msgs instead of calling i2c_learn."""
    g = parity.with_horizon(load_case(name), T)
    meta = g.meta
    x0, mu_u = parity.batched_inputs(g, B)
    sig_x0 = np.broadcast_to(g["sig_x0"], (B,) + g["sig_x0"].shape).copy()
    eng = pkg.BatchedI2c(parity.product_model(g), T, g.get("Q"), g["R"], g.get("Qf"), meta["alpha"], meta["tol"], mu_u, g["sig_u"],
                         g.get("mu_x_term"), g.get("sig_x_term"), quad=tuple(meta["quad"]), x0=x0, sig_x0=sig_x0, device=device, lib=lib,
                         inference=meta.get("inference", "cubature"), gh_degree=meta.get("gh_degree"), **kw)
    if "tau" in meta:
        eng.tau = int(meta["tau"])
    return eng


BUFFERS = ("post", "alpha", "status", "feedforward", "term_stats")
HISTORY = ("alphas", "alphas_desired", "costs_m", "costs_m_var")
N = 3

CASES = [
    # (golden case, T, B, engine arguments, (backward family, schedule that runs)): the tail of the backward sweep the case pins
    pytest.param("em_pendulum_T200", 9, 5, dict(backward_mode="chunked"), ("lane", "chunked"), id="pendulum-chunked"),  # two launches, M-step deferred into the next sweep
    pytest.param("em_pendulum_T200", 9, 5, dict(backward_mode="fused"), ("lane", "fused"), id="pendulum-fused"),  # no reduction: k_mstep
    pytest.param("em_pendulum_T200", 9, 5, dict(backward_mode="two_pass"), ("lane", "two_pass"), id="pendulum-two_pass"),  # M-step on k_reduce over cells
    pytest.param("em_pendulum_T200", 9, 5, dict(backward_mode="chunked", storage_dtype=torch.float32), ("lane", "chunked"),
                 id="pendulum-chunked-fp32-stored"),  # the same with fp32-stored messages
    pytest.param("em_pendulum_T200", 9, 5, dict(group_lanes=True), ("group", "fused"), id="pendulum-group"),  # group walk: k_mstep
    pytest.param("em_covctrl_T100", 9, 5, dict(backward_mode="chunked"), ("lane", "chunked"), id="covctrl-chunked"),  # terminal state prior: four passes, M-step on k_reduce over chunks
    pytest.param("em_cartpole_T100", 9, 5, dict(backward_mode="chunked", group_lanes=-1), ("lane", "chunked"), id="cartpole-lane-chunked"),  # d = 5 two-launch form
    pytest.param("em_dcp_T60", 9, 5, dict(backward_mode="chunked"), ("lane", "chunked"), id="dcp-chunked"),  # quad forward, lane walker, quad compose + stitch (d = 7: four passes)
    pytest.param("em_dcp_T60", 9, 5, dict(backward_mode="chunked", group_lanes=-1), ("lane", "chunked"), id="dcp-lane-chunked"),  # lane four passes
    pytest.param("em_dcp_T60", 9, 5, dict(group_lanes=64), ("quad", "fused"), id="dcp-quad-walk"),  # fused quad walk: k_mstep
    pytest.param("lin_pendulum_T100", 9, 5, dict(backward_mode="chunked"), ("lane", "chunked"), id="linearize-chunked"),  # M-step on k_chunk_reduce_lin
    pytest.param("lin_pendulum_T100", 9, 5, dict(backward_mode="fused"), ("lane", "fused"), id="linearize-fused"),  # k_mstep
    pytest.param("gh3_pendulum_T40", 9, 5, dict(backward_mode="chunked"), ("lane", "chunked"), id="gauss_hermite-chunked"),  # Gauss-Hermite passes
    pytest.param("em_quad12_T20", 5, 3, dict(group_lanes=64, backward_mode="fused"), ("wave", "fused"), id="quad12-wave-fused"),  # wave walk: k_mstep
    pytest.param("em_quad12_T20", 5, 3, dict(group_lanes=64, backward_mode="two_pass"), ("wave", "two_pass"), id="quad12-wave-two_pass"),  # wave scan + cell + reduce
    pytest.param("em_quad12_T20", 5, 3, dict(group_lanes=QUAD), ("quad", "fused"), id="quad12-quad"),  # quad walk
]
HELPER = [CASES[i] for i in (0, 3, 6)]  # B = 5 is below the default gate: the knob is what asks for the helper wave


def _case(lib, device, name, T, B, kw, runs, capfd=None):
    """One engine by learn(N), its twin by N learn_msgs(); capfd: under I2C_FORWARD_HELPER=1, and the library's own account
    (I2C_TRACE_PLAN=1) of the learn engine's forward sweeps says that all N ran the helper wave."""
    one, step = (make_engine(lib, device, name, T, B, **kw) for _ in range(2))
    assert (one.backward_family, one.backward_schedule) == runs
    # what makes BatchedI2c.learn enqueue ONE i2c_learn call instead of stepping through learn_msgs (engine.py)
    assert not one._propagate and one.prior_out is None and one.alpha_cell is None and not one.keep_prior_joint
    if capfd is None:
        one.learn(N)
    else:
        capfd.readouterr()
        with env(I2C_FORWARD_HELPER="1", I2C_TRACE_PLAN="1"):
            one.learn(N)
        assert re.findall(r"i2c_forward_lane: sweep=(\w+)", capfd.readouterr().err) == ["helper"] * N
    for _ in range(N):
        step.learn_msgs()
    assert one.em_iter == step.em_iter == N and one.failures() == step.failures() == []
    for k in BUFFERS:
        assert torch.equal(getattr(one, k), getattr(step, k)), k
    for k in HISTORY:
        rows_one, rows_step = getattr(one, k), getattr(step, k)
        assert len(rows_one) == len(rows_step) >= N, k
        for i, (x, y) in enumerate(zip(rows_one, rows_step)):
            assert torch.equal(x, y), (k, i)


# ---- the host simulation -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


@pytest.mark.parametrize("name,T,B,kw,runs", CASES)
def test_hostsim_learn_equals_stepwise(sim, name, T, B, kw, runs):
    _case(sim, "cpu", name, T, B, kw, runs)


@pytest.mark.parametrize("name,T,B,kw,runs", HELPER)
def test_hostsim_learn_with_helper_equals_stepwise(sim, capfd, name, T, B, kw, runs):
    _case(sim, "cpu", name, T, B, kw, runs, capfd)


# ---- the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    lib = pkg.load_library()
    assert not lib.is_host_sim, "GPU tests must run the HIP build"
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B,kw,runs", CASES)
def test_hip_learn_equals_stepwise(hip, name, T, B, kw, runs):
    _case(hip, "cuda", name, T, B, kw, runs)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B,kw,runs", HELPER)
def test_hip_learn_with_helper_equals_stepwise(hip, capfd, name, T, B, kw, runs):
    _case(hip, "cuda", name, T, B, kw, runs, capfd)
