"""The helper wave that also solves the smoother gains against the helper that only composes, bit for bit.

With fp64-stored messages the forward sweep of i2c_learn hands the smoother gain over to its helper wave (k_forward_helper<GAINH>,
csrc/i2c_impl.hpp): wave 0 stores the differences dl_j[k] of the dynamics transform in the d nx slots of J and forms neither sig_xy
nor J; wave 1 re-forms chol(sig_xu1_f), sig_xy, chol(sig_x3_f) and the solves from the row (gain_from_handoff, csrc/i2c_cell.hpp),
stores J over the hand-off and composes with it. On the flagged cell J is solved with the factor of sig_x3 BEFORE the terminal
update, which the sweep copies aside for the helper. It is the default of the models with d <= 3 (forward_helper_gain: the cartpole's
sweep waits for a helper that re-factors a 5 x 5 matrix per cell) and asked for with I2C_FORWARD_HELPER_GAIN=1 beyond them.
I2C_FORWARD_HELPER_GAIN=0 (read on every i2c_learn call) brings back the helper that only composes, I2C_FORWARD_HELPER=0 the sweep
without a helper: learn(3) on the paths in the same process, every output buffer
(the forward messages with their J rows among them), the composites, the statistics history and the status words compared with
torch.equal. Which wave solved the gains is read from the library's own account (I2C_TRACE_PLAN=1: "i2c_forward_lane: sweep=<helper|
plain> lean=<0|1> gain=<helper|sweep>").

The J rows are also compared on their own: a row left holding a hand-off (a chunk the helper did not finish -- the last one is
composed after the sweep has ended) or solved with the wrong factor (the flagged cell) fails there by name.

Shared bodies; test_hostsim_* run the host simulation of the kernel code on the CPU, test_hip_* the same bodies on the GPU."""
import re

import numpy as np
import pytest
import torch

import hostsim
import parity
from test_chunk_geometry import geometry
from test_chunk_self_stitch import LANE, LEAN, SENTINEL, assert_same, make_engine
from test_forward_helper import GEOMETRY, HEADLINE, MIN_B, comp_block, env
from test_learn_general_variants import CASES as GENERAL, prepared

pkg = parity.pkg
N = 3


def traced_learn(eng, capfd, **knobs):
    """eng.learn(N) under the knobs; returns what every lane forward sweep of the call said: (sweep, lean, gain), the same N times."""
    capfd.readouterr()
    with env(I2C_TRACE_PLAN="1", **knobs):
        eng.learn(N)
    err = capfd.readouterr().err
    said = re.findall(r"i2c_forward_lane: sweep=(\w+) lean=(\d) gain=(\w+)", err)
    assert len(said) == N and len(set(said)) == 1, err
    return said[0]


def j_rows(eng):
    """The J rows of the forward buffer [T][E_FWD][B]: behind mu_xu1_f, sig_xu1_f, mu_x3_f and sig_x3_f."""
    d, nx = eng.d, eng.nx
    lo = d + d * (d + 1) // 2 + nx + nx * (nx + 1) // 2
    fwd = eng.fwd.view(eng.H, -1, eng.B)
    assert fwd.shape[1] == lo + d * nx
    return fwd[:, lo:, :]


def same(a, b, keep, what):
    assert_same(a, b, keep, what)
    x, y = comp_block(a), comp_block(b)
    assert not (x == SENTINEL).any() and not (y == SENTINEL).any(), what
    assert torch.equal(x if keep is None else x[:, keep], y if keep is None else y[:, keep]), (what, "composites")
    ja, jb = j_rows(a), j_rows(b)
    if keep is not None:
        ja, jb = ja[..., keep], jb[..., keep]
    tc = int(a.terminal_cell)
    assert torch.equal(ja[-1], jb[-1]), (what, "J of the last cell of the last chunk")
    if 0 <= tc < a.H:
        assert torch.equal(ja[tc], jb[tc]), (what, "J of the flagged cell", tc)
    assert torch.equal(ja, jb), (what, "J rows")


def run_paths(make, capfd, lean=True, gain=True, keep=None, without_helper=False):
    """learn(3) by ONE i2c_learn call with the gain on the helper (for d <= 3 the default wherever the helper runs: from MIN_B
    trajectories on by itself, below with I2C_FORWARD_HELPER=1; for d > 3 with I2C_FORWARD_HELPER_GAIN=1) and under
    I2C_FORWARD_HELPER_GAIN=0; without_helper: also under I2C_FORWARD_HELPER=0. gain: the first path is expected to solve the gains
    on the helper."""
    new, old = make(), make()
    knobs = {} if new.B >= MIN_B else dict(I2C_FORWARD_HELPER="1")
    new_knobs = dict(knobs, I2C_FORWARD_HELPER_GAIN="1") if new.d > DEFAULT_MAX_D else knobs
    engines = [new, old] + ([make()] if without_helper else [])
    for e in engines:
        comp_block(e).fill_(SENTINEL)
    assert traced_learn(new, capfd, **new_knobs) == ("helper", str(int(lean)), "helper" if gain else "sweep")
    assert traced_learn(old, capfd, I2C_FORWARD_HELPER_GAIN="0", **knobs) == ("helper", str(int(lean)), "sweep")
    assert new.em_iter == old.em_iter == N and len(new.costs_m) == N
    same(new, old, keep, "I2C_FORWARD_HELPER_GAIN=0")
    if without_helper:
        assert traced_learn(engines[2], capfd, I2C_FORWARD_HELPER="0") == ("plain", str(int(lean)), "sweep")
        same(new, engines[2], keep, "I2C_FORWARD_HELPER=0")
    return new, old


DEFAULT_MAX_D = 3  # forward_helper_gain (csrc/i2c_impl.hpp): the models whose helper solves the gains with nothing set
HORIZONS = (8, 9, 13, 37)  # chunks of 4+4, 5+4 (a trailing chunk shorter by one), 5+5+3, 7x5+2
BATCHES = (1, 5, 67, 130)  # a partly filled wave; a second and a third workgroup
CASES = [pytest.param(T, B, id=f"pendulum-T{T}-B{B}") for T in HORIZONS for B in BATCHES]
CASES += [pytest.param(128, 5, id="pendulum-T128-B5")]  # all 32 chunks
assert GEOMETRY[41] == (9, 5, 1)  # ... and a chunk of ONE trailing cell:
CASES += [pytest.param(41, 5, id="pendulum-T41-B5")]


def _pendulum(lib, device, capfd, T, B, geo=None):
    """With a terminal observation on the last cell (the golden case's Qf). The pair at T = 37, B = 67 is the model's comparison
    against the sweep without a helper."""
    assert geometry(B, T) == (geo or GEOMETRY[T])
    new, _ = run_paths(lambda: make_engine(lib, device, "em_pendulum_T200", T, B, **LEAN), capfd, without_helper=(T, B) == (37, 67))
    assert new.failures() == [] and (new.forward_family, new.backward_schedule) == ("lane", "chunked")
    assert new.terminal_cell == T - 1


def _cartpole(lib, device, capfd, B):
    new, _ = run_paths(lambda: make_engine(lib, device, "em_cartpole_T100", 37, B, **LEAN), capfd, without_helper=B == 5)
    assert new.d == 5 and new.failures() == [] and new.forward_family == "lane"


def _no_terminal_observation(lib, device, capfd):
    """PendulumKnownActReg without a terminal prior: no terminal observation, the row's sig_x3_f is the one the sweep factored."""
    from i2c.known_models import make_env_model

    T, B = 37, 67

    def make():
        x0 = np.array([np.pi, 0.0]) + 1e-2 * np.random.default_rng(4).normal(size=(B, 2))
        eng = pkg.BatchedI2c(make_env_model("PendulumKnownActReg"), T, None, np.diag([1.0]), None, 300.0, 1.0, np.zeros((B, T, 1)),
                             0.5 * np.eye(1), x0=x0, device=device, lib=lib, **dict(LANE, **LEAN))
        eng.use_expert_controller = False
        return eng

    new, _ = run_paths(make, capfd, without_helper=True)
    assert not new.has_x_terminal and new.failures() == []


def _flagged_cell_mid_horizon(lib, device, capfd):
    """The ring moved three cells (tests/test_learn_general_variants.py, "ring3-tau3"): the flagged cell is cell T - 4 of 13, inside
    the second chunk, and the sweep is the general variant (LEAN = false), which the trace must say."""
    case = GENERAL["ring3-tau3"]
    new, _ = run_paths(lambda: prepared(lib, device, case), capfd, lean=False, without_helper=True)
    assert new.failures() == [] and new.t0 == 3 and new.terminal_cell == case.T - 1 - 3 and geometry(case.B, case.T) == (3, 5, 3)


def _general_weights(lib, device, capfd):
    """Weights that do not sum to one (W = 0.8975): the general cell from the weights alone."""
    case = GENERAL["weights-nonunit"]
    new, _ = run_paths(lambda: prepared(lib, device, case), capfd, lean=False, without_helper=True)
    assert new.failures() == []


def _general_weights_targets_ring(lib, device, capfd):
    """... and every general axis at once: weights, per-cell targets, a moved ring, tau."""
    case = GENERAL["all-pendulum-nonunit"]
    new, _ = run_paths(lambda: prepared(lib, device, case), capfd, lean=False)
    assert new.failures() == [] and new.t0 == 3


def _fp32_storage(lib, device, capfd):
    """fp32-stored messages: a hand-off would be rounded before the solve, so the sweep keeps its gains."""
    new, _ = run_paths(lambda: make_engine(lib, device, "em_pendulum_T200", 37, 67, storage_dtype=torch.float32, **LEAN), capfd, gain=False,
                       without_helper=True)
    assert new.mixed and new.failures() == []


def _failing_trajectory(lib, device, capfd):
    """Trajectory 2 fails through its inputs (an indefinite sig_x0): the same status word on both paths, every other trajectory
    bit for bit, and the call ends."""
    B = 67
    keep = [b for b in range(B) if b != 2]
    new, old = run_paths(lambda: make_engine(lib, device, "em_pendulum_T200", 37, B, bad=2, **LEAN), capfd, keep=keep, without_helper=True)
    assert [f[0] for f in new.failures()] == [2] and int(new.status[2]) == int(old.status[2]) != 0
    assert not torch.isfinite(new.post[..., 2]).all()


def _default_from_min_b(lib, device, capfd):
    """From forward_helper_min_b trajectories on the gain is on the helper with nothing set."""
    _pendulum(lib, device, capfd, 8, MIN_B)


def _cartpole_default_keeps_parent(lib, device, capfd):
    """d = 5: with nothing set the helper composes only (measured slower with the gain, profiles/forward_gain_helper_ab.txt)."""
    eng = make_engine(lib, device, "em_cartpole_T100", 37, 5, **LEAN)
    assert eng.d == 5 and traced_learn(eng, capfd, I2C_FORWARD_HELPER="1") == ("helper", "1", "sweep")


def _without_helper_no_gain(lib, device, capfd):
    """Below forward_helper_min_b, nothing set: no helper wave, and the trace says who solves the gains."""
    eng = make_engine(lib, device, "em_pendulum_T200", 37, 67, **LEAN)
    assert traced_learn(eng, capfd) == ("plain", "1", "sweep")
    eng = make_engine(lib, device, "em_pendulum_T200", 37, 67, **LEAN)
    assert traced_learn(eng, capfd, I2C_FORWARD_HELPER="1", I2C_CHUNK_PASSES="4") == ("plain", "1", "sweep")


BODIES = dict(no_terminal_observation=_no_terminal_observation, flagged_cell_mid_horizon=_flagged_cell_mid_horizon,
              general_weights=_general_weights, general_weights_targets_ring=_general_weights_targets_ring, fp32_storage=_fp32_storage,
              failing_trajectory=_failing_trajectory, default_from_min_b=_default_from_min_b,
              cartpole_default_keeps_parent=_cartpole_default_keeps_parent, without_helper_no_gain=_without_helper_no_gain)


# ---- the host simulation -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


@pytest.mark.parametrize("T,B", CASES)
def test_hostsim_gain_helper_equals_parent(sim, capfd, T, B):
    _pendulum(sim, "cpu", capfd, T, B)


@pytest.mark.parametrize("B", (5, 67))
def test_hostsim_gain_helper_cartpole(sim, capfd, B):
    _cartpole(sim, "cpu", capfd, B)


@pytest.mark.parametrize("body", sorted(BODIES))
def test_hostsim_gain_helper(sim, capfd, body):
    BODIES[body](sim, "cpu", capfd)


# ---- the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    lib = pkg.load_library()
    assert not lib.is_host_sim, "GPU tests must run the HIP build"
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("T,B", CASES)
def test_hip_gain_helper_equals_parent(hip, capfd, T, B):
    _pendulum(hip, "cuda", capfd, T, B)


@pytest.mark.gpu
def test_hip_gain_helper_equals_parent_headline_geometry(hip, capfd):
    _pendulum(hip, "cuda", capfd, *HEADLINE)


@pytest.mark.gpu
@pytest.mark.parametrize("B", (5, 67))
def test_hip_gain_helper_cartpole(hip, capfd, B):
    _cartpole(hip, "cuda", capfd, B)


@pytest.mark.gpu
@pytest.mark.parametrize("body", sorted(BODIES))
def test_hip_gain_helper(hip, capfd, body):
    BODIES[body](hip, "cuda", capfd)
