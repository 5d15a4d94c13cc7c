"""The forward sweep with a helper wave against the parent's launches, bit for bit.

Inside i2c_learn the lane forward sweep of a d <= 5 model runs in workgroups of two wavefronts (k_forward_helper, csrc/i2c_impl.hpp):
wave 0 is the sweep and releases every chunk of the chunked backward schedule at the workgroup barrier once its messages are stored,
wave 1 composes that chunk with chunk_compose_body -- the compose pass of the backward sweep, which then starts with its walk.
I2C_FORWARD_HELPER=0 (read on every i2c_learn call) brings back k_forward / k_forward_mstep and the k_chunk_compose launch: learn(3)
on both paths in the same process (the helper is the default from 4096 trajectories on and asked for with I2C_FORWARD_HELPER=1 below), every output, the composites and the statistics history compared with torch.equal.

The helper's composites and a compose launch's are the same bytes in the same place, so which of the two wrote them is read from
the library's own account at its two dispatch sites (I2C_TRACE_PLAN=1 on stderr: "i2c_forward_lane: sweep=<helper|plain>" where
the sweep is launched, "i2c_backward_chunked: compose=<skipped|launched>" where the compose pass is).

Shared bodies; test_hostsim_* run the host simulation of the kernel code on the CPU (a lane's sweep, then its chunks), test_hip_*
the same bodies on the GPU, where a run that ends is also what shows that the number of barriers does not depend on the data."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import load_case
from test_chunk_geometry import geometry
from test_chunk_self_stitch import LANE, LEAN, SENTINEL, assert_same, four_passes, make_covctrl, make_engine

pkg = parity.pkg


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def comp_block(eng):
    """The composite block of the chunk workspace (ChunkWork, csrc/i2c_impl.hpp) as [chunks * elements][B]: at its head."""
    n = geometry(eng.B, eng.H)[0]
    nx = eng.nx
    return eng.work[:n * eng.B * (nx + nx * nx + nx * (nx + 1) // 2)].view(-1, eng.B)


def traced_learn(eng, n, capfd, **knobs):
    """eng.learn(n) under the knobs; returns whether the call ran the helper wave, read where the library dispatches: every lane
    forward sweep says which kernel it launches, every chunked backward sweep whether it launches its compose pass or skips it.
    The two go together, n times: a helper sweep in front of a compose launch would lose the gain, a plain sweep in front of a
    skipped compose pass the composites."""
    capfd.readouterr()
    with env(I2C_TRACE_PLAN="1", **knobs):
        eng.learn(n)
    err = capfd.readouterr().err
    sweeps = re.findall(r"i2c_forward_lane: sweep=(\w+)", err)
    composes = re.findall(r"i2c_backward_chunked: compose=(\w+)", err)
    assert len(sweeps) == len(composes) == n, err  # one i2c_learn call of n iterations
    assert (set(sweeps), set(composes)) in (({"helper"}, {"skipped"}), ({"plain"}, {"launched"})), err
    return sweeps[0] == "helper"


MIN_B = 4096  # forward_helper_min_b (csrc/i2c_impl.hpp): the batch size from which the helper is the default


def run_pair(make, capfd, helper=True, keep=None, new_knobs=None, n_learn=3):
    """learn(3) by ONE i2c_learn call with the helper and under I2C_FORWARD_HELPER=0. From MIN_B trajectories on "with the helper"
    is the default path, nothing set; below, where the plan keeps the parent's kernels because short chunks do not pay,
    I2C_FORWARD_HELPER=1 asks for it. helper: that path is expected to run the helper wave; keep: the trajectories compared
    (status words: all of them)."""
    new, old = make(), make()
    if new_knobs is None:
        new_knobs = {} if new.B >= MIN_B else dict(I2C_FORWARD_HELPER="1")
    for e in (new, old):
        comp_block(e).fill_(SENTINEL)
    assert traced_learn(new, n_learn, capfd, **(new_knobs or {})) == helper
    assert not traced_learn(old, n_learn, capfd, I2C_FORWARD_HELPER="0")
    assert new.em_iter == old.em_iter == n_learn and len(new.costs_m) == n_learn
    assert_same(new, old, keep, "learn")
    a, b = comp_block(new), comp_block(old)
    assert not (b == SENTINEL).any() and not (a == SENTINEL).any()  # written on either path: by the compose launch / by the helper
    assert torch.equal(a if keep is None else a[:, keep], b if keep is None else b[:, keep])
    return new, old


HORIZONS = (8, 9, 13, 37, 41, 131)  # chunks of 4+4, 5+4, 5+5+3, 7x5+2, 8x5+1, 26x5+1
BATCHES = (1, 5, 67, 130)  # a partly filled wave; a second and a third workgroup
GEOMETRY = {8: (2, 4, 4), 9: (2, 5, 4), 13: (3, 5, 3), 37: (8, 5, 2), 41: (9, 5, 1), 131: (27, 5, 1), 128: (32, 4, 4), 200: (29, 7, 4)}
CASES = [pytest.param(T, B, id=f"pendulum-T{T}-B{B}") for T in HORIZONS for B in BATCHES]
CASES += [pytest.param(128, 5, id="pendulum-T128-B5"), pytest.param(200, 5, id="pendulum-T200-B5")]  # all 32 chunks; chunks of 7 cells
# the DEFAULT is the helper from 4096 trajectories on: two chunks of four cells on either side; the headline's own geometry (16
# chunks: 15 of 13 cells and one of 5) on the device only, where it takes no time
CASES += [pytest.param(8, 4096, id="pendulum-T8-B4096-default")]
HEADLINE = (200, 4096, (16, 13, 5))


def _pendulum(lib, device, capfd, T, B, geo=None):
    assert geometry(B, T) == (geo or GEOMETRY[T])
    new, _ = run_pair(lambda: make_engine(lib, device, "em_pendulum_T200", T, B, **LEAN), capfd)
    assert new.failures() == [] and (new.forward_family, new.backward_schedule) == ("lane", "chunked")


def _no_terminal_observation(lib, device, capfd):
    """PendulumKnownActReg without a terminal prior: no terminal observation and no terminal state prior."""
    from i2c.known_models import make_env_model

    T, B = 37, 67

    def make():
        x0 = np.array([np.pi, 0.0]) + 1e-2 * np.random.default_rng(4).normal(size=(B, 2))
        eng = pkg.BatchedI2c(make_env_model("PendulumKnownActReg"), T, None, np.diag([1.0]), None, 300.0, 1.0, np.zeros((B, T, 1)),
                             0.5 * np.eye(1), x0=x0, device=device, lib=lib, **dict(LANE, **LEAN))
        eng.use_expert_controller = False
        return eng

    new, _ = run_pair(make, capfd)
    assert not new.has_x_terminal and new.failures() == []


def _cartpole(lib, device, capfd, B):
    new, _ = run_pair(lambda: make_engine(lib, device, "em_cartpole_T100", 37, B, **LEAN), capfd)
    assert new.d == 5 and new.failures() == [] and new.forward_family == "lane"


def _fp32_storage(lib, device, capfd):
    new, _ = run_pair(lambda: make_engine(lib, device, "em_pendulum_T200", 37, 67, storage_dtype=torch.float32, **LEAN), capfd)
    assert new.mixed and new.failures() == []


def _terminal_state_prior(lib, device, capfd):
    new, _ = run_pair(lambda: make_covctrl(lib, device, 12, 5), capfd, helper=False)
    assert new.has_x_terminal and new.failures() == []


def _double_cartpole(lib, device, capfd):
    """d = 7: the lane forward sweep has no helper variant."""
    def make():
        g = parity.with_horizon(load_case("em_dcp_T60"), 12)
        x0, mu_u = parity.batched_inputs(g, 3)
        return pkg.BatchedI2c(parity.product_model(g), 12, g.get("Q"), g["R"], g.get("Qf"), g.meta["alpha"], g.meta["tol"], mu_u, g["sig_u"],
                              quad=tuple(g.meta["quad"]), x0=x0, device=device, lib=lib, **dict(LANE, **LEAN))

    new, _ = run_pair(make, capfd, helper=False)
    assert new.d == 7 and (new.forward_family, new.backward_schedule) == ("lane", "chunked")


def _below_min_b(lib, device, capfd):
    """Below forward_helper_min_b the default path is the parent's: nothing set, no helper wave, the compose pass launched."""
    run_pair(lambda: make_engine(lib, device, "em_pendulum_T200", 37, 67, **LEAN), capfd, helper=False, new_knobs={})


def _four_passes(lib, device, capfd):
    """I2C_CHUNK_PASSES=4 switches the helper off as well: the reference path of tests/test_chunk_self_stitch.py is the parent's."""
    run_pair(lambda: make_engine(lib, device, "em_pendulum_T200", 37, 67, **LEAN), capfd, helper=False, new_knobs=dict(I2C_CHUNK_PASSES="4"))
    with four_passes():  # (that file's own switch reaches the library the same way)
        assert not traced_learn(make_engine(lib, device, "em_pendulum_T200", 37, 67, **LEAN), 1, capfd)


def _failing_trajectory(lib, device, capfd):
    """Trajectory 2 fails through its inputs (an indefinite sig_x0): the same status word on both paths, every other trajectory
    bit for bit, and the call ends -- both waves meet at the barrier once per chunk whatever a trajectory computes."""
    B = 67
    keep = [b for b in range(B) if b != 2]
    new, old = run_pair(lambda: make_engine(lib, device, "em_pendulum_T200", 37, B, bad=2, **LEAN), capfd, keep=keep)
    assert [f[0] for f in new.failures()] == [2] and int(new.status[2]) == int(old.status[2]) != 0
    assert not torch.isfinite(new.post[..., 2]).all()


BODIES = dict(below_min_b_keeps_parent=_below_min_b, no_terminal_observation=_no_terminal_observation, fp32_storage=_fp32_storage,
              terminal_state_prior_keeps_parent=_terminal_state_prior, double_cartpole_keeps_parent=_double_cartpole,
              four_passes_keep_parent=_four_passes, failing_trajectory=_failing_trajectory)


# ---- the host simulation -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


@pytest.mark.parametrize("T,B", CASES)
def test_hostsim_helper_equals_parent(sim, capfd, T, B):
    _pendulum(sim, "cpu", capfd, T, B)


@pytest.mark.parametrize("B", (5, 67))
def test_hostsim_helper_cartpole(sim, capfd, B):
    _cartpole(sim, "cpu", capfd, B)


@pytest.mark.parametrize("body", sorted(BODIES))
def test_hostsim_helper(sim, capfd, body):
    BODIES[body](sim, "cpu", capfd)


# ---- the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    lib = pkg.load_library()
    assert not lib.is_host_sim, "GPU tests must run the HIP build"
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("T,B", CASES)
def test_hip_helper_equals_parent(hip, capfd, T, B):
    _pendulum(hip, "cuda", capfd, T, B)


@pytest.mark.gpu
def test_hip_helper_equals_parent_headline_geometry(hip, capfd):
    _pendulum(hip, "cuda", capfd, *HEADLINE)


@pytest.mark.gpu
@pytest.mark.parametrize("B", (5, 67))
def test_hip_helper_cartpole(hip, capfd, B):
    _cartpole(hip, "cuda", capfd, B)


@pytest.mark.gpu
@pytest.mark.parametrize("body", sorted(BODIES))
def test_hip_helper(hip, capfd, body):
    BODIES[body](hip, "cuda", capfd)
