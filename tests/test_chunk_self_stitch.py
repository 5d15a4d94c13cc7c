"""The two-launch form of the chunked backward sweep against its four passes, bit for bit.

Where the stitch pass and the walk both run on the lane kernels (sigma-point rule, d <= 5, no terminal state prior) the walker of a
chunk computes the smoothed state entering it itself -- the terminal filtered state pushed through the composites of the chunks behind
it, the expressions and order of the stitch pass (apply_composite, csrc/i2c_cell.hpp) --, and inside i2c_learn the forward sweep of the
next iteration adds the walkers' partial sums in k_reduce's order and runs the M-step (k_forward_mstep, csrc/i2c_impl.hpp). The
arithmetic and its order are those of compose -> stitch -> walk -> reduce, which I2C_CHUNK_PASSES=4 (read on every backward call)
brings back: every output is compared with torch.equal, in the same process.

That the default really is the other path is read off the workspace: its boundary-state block is written by the stitch pass alone.

Shared bodies; test_hostsim_* run the host simulation of the kernel code on the CPU, test_hip_* the same bodies on the GPU."""
import contextlib
import os

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import load_case
from test_chunk_geometry import geometry

pkg = parity.pkg
LANE = dict(group_lanes=-1, backward_mode="chunked")
SENTINEL = -7.0e77


@contextlib.contextmanager
def four_passes():
    os.environ["I2C_CHUNK_PASSES"] = "4"
    try:
        yield
    finally:
        del os.environ["I2C_CHUNK_PASSES"]


def make_engine(lib, device, name, T, B, bad=None, **kw):
    """The golden case `name` over T cells, B trajectories (parity.engine_from_case without the joint-prior output, with which
    BatchedI2c.learn would step through learn_msgs instead of calling i2c_learn). bad: a trajectory with an indefinite sig_x0."""
    g = parity.with_horizon(load_case(name), T)
    meta = g.meta
    x0, mu_u = parity.batched_inputs(g, B)
    sig_x0 = np.broadcast_to(g["sig_x0"], (B,) + g["sig_x0"].shape).copy()
    if bad is not None:
        sig_x0[bad] = -sig_x0[bad]
    eng = pkg.BatchedI2c(parity.product_model(g), T, g.get("Q"), g["R"], g.get("Qf"), meta["alpha"], meta["tol"], mu_u, g["sig_u"],
                         g.get("mu_x_term"), g.get("sig_x_term"), quad=tuple(meta["quad"]), x0=x0, sig_x0=sig_x0, device=device, lib=lib,
                         **dict(LANE, **kw))
    if "tau" in meta:
        eng.tau = int(meta["tau"])
    return eng


def make_covctrl(lib, device, T, B):
    """A terminal state prior (covariance control on PendulumKnownActReg, as tests/test_hip_full_configs.py builds it)."""
    from i2c.known_models import make_env_model

    x0 = np.array([np.pi, 0.0]) + 1e-2 * np.random.default_rng(4).normal(size=(B, 2))
    eng = pkg.BatchedI2c(make_env_model("PendulumKnownActReg"), T, None, np.diag([1.0]), None, 300.0, 1.0, np.zeros((B, T, 1)),
                         0.5 * np.eye(1), np.array([0.0, 0.0]), np.diag([1e-3, 1e-3]), x0=x0, device=device, lib=lib, keep_xm=False,
                         keep_zpost=False, **LANE)
    eng.use_expert_controller = False
    return eng


def bnd_block(eng):
    """The boundary-state block of the chunk workspace (ChunkWork, csrc/i2c_impl.hpp): behind the composites."""
    n = geometry(eng.B, eng.H)[0]
    nx = eng.nx
    s = nx * (nx + 1) // 2
    lo = n * eng.B * (nx + nx * nx + s)
    assert eng.work.numel() == n * eng.B * ((nx + nx * nx + s) + (nx + s) + 3)
    return eng.work[lo:lo + n * eng.B * (nx + s)]


BUFFERS = ("post", "term_stats", "alpha", "status", "temp", "fwd")
OPTIONAL = ("xm", "zpost", "cell_stats")
HISTORY = ("alphas", "alphas_desired", "costs_m", "costs_m_var")


def assert_same(a, b, keep=None, what=""):
    """Every output buffer and every history row of engine a equals engine b's, bit for bit; keep: the trajectories compared
    (the status words are compared for all of them)."""
    assert a.failures() == b.failures(), (what, a.failures()[:3], b.failures()[:3])
    assert torch.equal(a.status, b.status), what
    for k in BUFFERS + OPTIONAL:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert torch.equal(x if keep is None else x[..., keep], y if keep is None else y[..., keep]), (what, k)
    for k in HISTORY:
        la, lb = getattr(a, k), getattr(b, k)
        assert len(la) == len(lb), (what, k)
        for i, (x, y) in enumerate(zip(la, lb)):
            assert torch.equal(x if keep is None else x[keep], y if keep is None else y[keep]), (what, k, i)


def run_pair(make, n_learn=3, stepwise=True, self_stitch=True, keep=None):
    """One engine on the default path and one under I2C_CHUNK_PASSES=4, the same calls: a stand-alone backward sweep between a
    forward sweep and an M-step of their own (the sweep ends with k_reduce on either path), then n_learn iterations by ONE
    i2c_learn call (the M-steps of all but the last one deferred into the next forward sweep)."""
    new, old = make(), make()
    assert (new.backward_family, new.backward_schedule, new.kernel_family("chunk_passes"), new.kernel_family("chunk_stitch")) == \
        ("lane", "chunked", "lane", "lane")
    for e in (new, old):
        bnd_block(e).fill_(SENTINEL)
    if stepwise:
        new.learn_msgs()
        with four_passes():
            old.learn_msgs()
        assert_same(new, old, keep, "stepwise")
    new.learn(n_learn)
    with four_passes():
        old.learn(n_learn)
    assert new.em_iter == old.em_iter == n_learn + int(stepwise)
    assert len(new.costs_m) == new.em_iter  # (one history row per iteration: i2c_learn ran, not a loop of learn_msgs)
    assert_same(new, old, keep, f"learn({n_learn})")
    # the stitch pass is the only writer of the boundary-state block: it ran under the knob, and without it only where it has to
    assert not (bnd_block(old) == SENTINEL).any()
    assert bool((bnd_block(new) == SENTINEL).all()) == self_stitch
    return new, old


LEAN = dict(keep_xm=False, keep_zpost=False)
CASES = [
    # (golden case, T, B, engine arguments): chunks and what the case is here for
    pytest.param("em_pendulum_T200", 9, 1, LEAN, id="pendulum-T9-B1"),  # 2 chunks: an empty suffix and a single composite
    pytest.param("em_pendulum_T200", 33, 65, LEAN, id="pendulum-T33-B65"),  # 7 chunks, the last of 3 cells; one lane in the last wave
    pytest.param("em_pendulum_T200", 43, 8200, LEAN, id="pendulum-T43-B8200"),  # 8 chunks from 65536 / B; 8 lanes in the last wave
    pytest.param("em_cartpole_T100", 17, 3, LEAN, id="cartpole-T17-B3"),  # d = 5
    pytest.param("em_pendulum_T200", 33, 65, dict(LEAN, storage_dtype=torch.float32), id="pendulum-fp32-stored-T33-B65"),
    # more composites behind a chunk than one batch of loads holds (chunk_boundary_state: 8 for nx <= 2, 4 beyond)
    pytest.param("em_pendulum_T200", 131, 5, LEAN, id="pendulum-T131-B5"),  # 27 chunks, one cell in the last
    pytest.param("em_cartpole_T100", 41, 3, LEAN, id="cartpole-T41-B3"),  # 9 chunks
]
GEOMETRY = {(9, 1): (2, 5, 4), (33, 65): (7, 5, 3), (43, 8200): (8, 6, 1), (17, 3): (4, 5, 2), (131, 5): (27, 5, 1), (41, 3): (9, 5, 1)}


def _case(lib, device, name, T, B, kw):
    assert geometry(B, T) == GEOMETRY[(T, B)]
    # (the large batch: the i2c_learn call alone -- the host simulation walks 8200 x 43 cells per sweep)
    new, _ = run_pair(lambda: make_engine(lib, device, name, T, B, **kw), stepwise=device != "cpu" or B < 1000)
    assert new.failures() == [] and new.mixed == ("storage_dtype" in kw) and new.xm is None and new.zpost is None


def _full_walker(lib, device):
    """The walker that also writes the smoothed state, the observed marginal and the per-cell statistics (not LEANW)."""
    def make():
        eng = make_engine(lib, device, "em_pendulum_T200", 33, 65, keep_xm=True, keep_zpost=True)
        eng.cell_stats = torch.zeros(eng.H, 2, eng.B, dtype=eng.dtype, device=eng.device)
        return eng

    new, _ = run_pair(make)
    assert new.failures() == [] and new.xm is not None and new.zpost is not None and bool((new.cell_stats != 0).any())


def _failing_trajectory(lib, device):
    """Trajectory 2 fails through its inputs (an indefinite sig_x0, as tests/test_edge_cases.py): the same status word on both
    paths, every other trajectory bit for bit (trajectory 2 itself is NaN on both)."""
    new, old = run_pair(lambda: make_engine(lib, device, "em_pendulum_T200", 33, 5, bad=2, **LEAN), keep=[0, 1, 3, 4])
    assert [f[0] for f in new.failures()] == [2] and int(new.status[2]) == int(old.status[2]) != 0
    assert not torch.isfinite(new.post[..., 2]).all()


def _terminal_factorisation_failure(lib, device):
    """A terminal filtered covariance that is not positive definite (poked into the forward messages of trajectory 2, as
    tests/test_chunk_geometry.py pokes a cell): the four passes report it from the stitch pass, before any walker runs (reason 6).
    The self-stitching walker of the LAST chunk reports it while the other chunks walk from boundary states that carry the same
    covariance, so a cell of theirs (reason 7) may take the status word first -- as between two failing cells of different chunks.
    Either way trajectory 2 is reported, alone, and every other trajectory is bit for bit the four passes'."""
    T, B = 33, 5
    new, old = (make_engine(lib, device, "em_pendulum_T200", T, B, **LEAN) for _ in range(2))
    for e in (new, old):
        e.forward_sweep()
        e.fwd[T - 1, e.d + e.d * (e.d + 1) // 2 + e.nx, 2] = -1.0  # sig_x3_f[0][0] of the last cell, trajectory 2
    new.backward_sweep()
    with four_passes():
        old.backward_sweep()
    assert [(b, r) for b, r, _ in old.failures()] == [(2, 6)], old.failures()
    fails = new.failures()
    assert [b for b, _, _ in fails] == [2] and fails[0][1] in (6, 7), fails
    keep = [0, 1, 3, 4]
    for k in ("post", "term_stats"):
        assert torch.equal(getattr(new, k)[..., keep], getattr(old, k)[..., keep]), k


def _terminal_state_prior(lib, device):
    """A terminal state prior's end of the chain advances temp[b] -- once per trajectory and sweep, so not by several walkers: such
    a problem stays on the four passes (the stitch pass writes its boundary states with and without the knob)."""
    T, B = 12, 5
    assert geometry(B, T) == (3, 4, 4)
    made = []

    def make():
        made.append(make_covctrl(lib, device, T, B))
        return made[-1]

    temp0 = make_covctrl(lib, device, T, B).temp.clone()
    new, old = run_pair(make, self_stitch=False)
    assert new.has_x_terminal and new.failures() == []
    assert torch.equal(new.temp, temp0 + 4 * float(new._problem.dtemp)) and float(new._problem.dtemp) != 0.0  # four sweeps, once each


def _learn_one(lib, device):
    """A single iteration: nothing to defer into, the call ends with k_reduce."""
    run_pair(lambda: make_engine(lib, device, "em_pendulum_T200", 33, 65, **LEAN), n_learn=1, stepwise=False)


def _learn_then_stepwise(lib, device):
    """learn(3) and then one iteration through the stepwise calls equals learn(4): the deferred M-step leaves no state behind."""
    a, b = (make_engine(lib, device, "em_pendulum_T200", 33, 65, **LEAN) for _ in range(2))
    a.learn(4)
    b.learn(3)
    b.em_iter += 1
    b.forward_sweep()
    b.backward_sweep()
    b.maximize()
    assert a.failures() == [] and a.em_iter == b.em_iter == 4
    assert_same(a, b, what="learn(3) + stepwise")


# ---- the host simulation -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


@pytest.mark.parametrize("name,T,B,kw", CASES)
def test_hostsim_self_stitch_equals_four_passes(sim, name, T, B, kw):
    _case(sim, "cpu", name, T, B, kw)


def test_hostsim_self_stitch_full_walker(sim):
    _full_walker(sim, "cpu")


def test_hostsim_self_stitch_failing_trajectory(sim):
    _failing_trajectory(sim, "cpu")


def test_hostsim_terminal_factorisation_failure(sim):
    _terminal_factorisation_failure(sim, "cpu")


def test_hostsim_terminal_state_prior_keeps_four_passes(sim):
    _terminal_state_prior(sim, "cpu")


def test_hostsim_learn_one_iteration(sim):
    _learn_one(sim, "cpu")


def test_hostsim_learn_then_stepwise_equals_learn(sim):
    _learn_then_stepwise(sim, "cpu")


# ---- the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    lib = pkg.load_library()
    assert not lib.is_host_sim, "GPU tests must run the HIP build"
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B,kw", CASES)
def test_hip_self_stitch_equals_four_passes(hip, name, T, B, kw):
    _case(hip, "cuda", name, T, B, kw)


@pytest.mark.gpu
def test_hip_self_stitch_full_walker(hip):
    _full_walker(hip, "cuda")


@pytest.mark.gpu
def test_hip_self_stitch_failing_trajectory(hip):
    _failing_trajectory(hip, "cuda")


@pytest.mark.gpu
def test_hip_terminal_factorisation_failure(hip):
    _terminal_factorisation_failure(hip, "cuda")


@pytest.mark.gpu
def test_hip_terminal_state_prior_keeps_four_passes(hip):
    _terminal_state_prior(hip, "cuda")


@pytest.mark.gpu
def test_hip_learn_one_iteration(hip):
    _learn_one(hip, "cuda")


@pytest.mark.gpu
def test_hip_learn_then_stepwise_equals_learn(hip):
    _learn_then_stepwise(hip, "cuda")
