"""The coupled kernels of one i2c_learn call in their GENERAL variants, bit for bit against the code's own sibling paths.

tests/test_chunk_self_stitch.py, tests/test_forward_helper.py and tests/test_learn_tails.py build LEAN problems only: unit cubature
weights, one shared target, alpha[b] alone, the ring at its origin, for which run_forward (csrc/i2c_impl.hpp) launches the LEAN
variant of the lane forward sweep. Impl::launches does not look at leanness, so learn(n) on a problem with general cubature weights,
per-cell targets or a moved ring runs k_forward_mstep / k_forward_helper / k_forward_mstep_helper<M, R, false, S> and
k_chunk_walk_self with per-cell target fetches (not LEANW) or with c.row(t) != t. Here every case builds four identically prepared
engines and compares, with torch.equal on every output, the composites of the workspace and every history row,
  learn(3) with the helper wave (I2C_FORWARD_HELPER=1 below 4096 trajectories, nothing set from 4096 on)   against
  learn(3) under I2C_FORWARD_HELPER=0,  learn(3) under I2C_CHUNK_PASSES=4  and  three learn_msgs() calls.
That the first engine ran the helper wave, the self-stitching walker and the variant the case is here for is read from the
library's own account (I2C_TRACE_PLAN=1: "i2c_forward_lane: sweep=helper lean=0", "i2c_backward_chunked: compose=skipped walk=self
lean=<0|1>"). It is also what showed that general weights alone need not leave the LEAN sweep: see WEIGHTS and NONUNIT below.

Two references that are not the code's own: every case without a ring shift is compared with the NumPy oracle on the same inputs
(weights, per-cell targets, tau) at the tolerances of parity.check_batch_against_oracle (1e-8, policy 1e-7); the case with fp32-STORED
messages cannot meet those (a stored value is rounded to 6e-8) and is held to the bounds tests/test_precision.py asserts for that
mode. Every ring case with per-cell targets is compared bit for bit with an unrolled twin, an engine at t0 == 0 that holds the
same cells in cell order (tests/test_mpc.py, _ring_equals_unrolled) -- both sides in the general variant; a general run is never
compared with a LEAN one bit for bit, nothing promises that.

Shared bodies; test_hostsim_* run the host simulation of the kernel code on the CPU, test_hip_* the same bodies on the GPU, where
the contraction of the general cell behind the M-step prologue and around the chunk release is what is at stake (the host
simulation is built with -ffp-contract=off) and a call that returns shows that both waves meet at the barrier once per chunk."""
import json
import re
from dataclasses import dataclass, field, replace

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import load_case, oracle_from_case, rel_err
from test_chunk_geometry import geometry
from test_chunk_self_stitch import LANE, LEAN, SENTINEL, assert_same, make_engine
from test_forward_helper import MIN_B, comp_block, traced_learn
from test_model_params_batch import engine as params_engine, linear_model, param_rows
from test_precision import MIXED_BOUNDS

pkg = parity.pkg
N = 3
# Two rules with other weights than the unit rule's. Under the first the weights still SUM to one (W = 2 - alpha^2 + beta = 1): the
# points and their weights change, the correction terms of a rule with W != 1 stay out, and the forward sweep stays LEAN unless
# another axis is set. Under the second (tests/test_chunk_geometry.py, GENERAL) W = 0.8975: sig_eta_w, the m m^T term, the general
# variant from the weights alone. (A rule with W > 1 leaves these problems' covariances indefinite in the first sweep.)
WEIGHTS = (1.2, 0.44, 0.5)
NONUNIT = (1.05, 0.0, 0.3)
FULL = dict(keep_xm=True, keep_zpost=True)


def unit_sum(quad):
    return quad is None or abs(1.0 - quad[0] ** 2 + quad[1]) < 1e-14  # (make_rule, csrc/i2c_impl.hpp)


@dataclass(frozen=True)
class Case:
    name: str = "em_pendulum_T200"
    T: int = 13
    B: int = 5
    quad: tuple = None       # general cubature weights
    targets: bool = False    # per-cell targets, per trajectory
    shifts: int = 0          # shift_horizon() calls before learn: the ring moved
    tau: int = None
    bad: int = None          # a trajectory with an indefinite sig_x0
    full: bool = False       # the walker writes xm, zpost and cell_stats
    kw: dict = field(default_factory=dict)

    @property
    def lean_forward(self):
        return unit_sum(self.quad) and not self.targets and self.shifts == 0

    @property
    def lean_walk(self):  # (Launches::walk_lean: a moved ring and general weights leave the walker LEANW)
        return not self.targets and not self.full


def targets_of(case, eng):
    """goal + 0.1 N(0, 1) for every cell of every trajectory"""
    return eng.zg + 0.1 * np.random.default_rng(17).normal(size=(case.B, case.T, eng.nz))


def prepared(lib, device, case, shifts=None):
    eng = make_engine(lib, device, case.name, case.T, case.B, bad=case.bad, **dict(FULL if case.full else LEAN, **case.kw))
    if case.quad is not None:
        eng.quad = tuple(float(q) for q in case.quad)
        eng.refresh_problem()
    if case.targets:
        eng.set_targets(targets_of(case, eng))
    for _ in range(case.shifts if shifts is None else shifts):
        eng.shift_horizon()
    if case.tau is not None:
        eng.tau = case.tau
    if case.full:
        eng.cell_stats = torch.zeros(eng.H, 2, eng.B, dtype=eng.dtype, device=eng.device)
    return eng


class Tee:
    """capfd for traced_learn that keeps what it read last: the trace of the call."""

    def __init__(self, capfd):
        self.capfd, self.err = capfd, ""

    def readouterr(self):
        r = self.capfd.readouterr()
        self.err = r.err
        return r


def traced(eng, capfd, lean_forward, walk, **knobs):
    """eng.learn(N) under the knobs; asserts the variants the library says it launched and returns whether the helper wave ran.
    walk: ("self" | "plain", walker lean)."""
    tee = Tee(capfd)
    helper = traced_learn(eng, N, tee, **knobs)
    assert re.findall(r"i2c_forward_lane: sweep=\w+ lean=(\d)", tee.err) == [str(int(lean_forward))] * N, tee.err
    assert re.findall(r"i2c_backward_chunked: compose=\w+ walk=(\w+) lean=(\d)", tee.err) == [(walk[0], str(int(walk[1])))] * N, tee.err
    return helper


def same(a, b, keep, what):
    assert_same(a, b, keep, what)
    assert torch.equal(a.feedforward, b.feedforward), what
    x, y = comp_block(a), comp_block(b)
    assert not (x == SENTINEL).any() and not (y == SENTINEL).any(), what
    assert torch.equal(x if keep is None else x[:, keep], y if keep is None else y[:, keep]), (what, "composites")


def four_paths(make, capfd, lean_forward, lean_walk, keep=None, stepwise=True):
    """The helper path against its three siblings; returns the engine of the helper path."""
    new, off, four = make(), make(), make()
    assert (new.forward_family, new.backward_family, new.backward_schedule, new.kernel_family("chunk_passes"), new.kernel_family("chunk_stitch")) == \
        ("lane", "lane", "chunked", "lane", "lane")
    # what makes BatchedI2c.learn enqueue ONE i2c_learn call instead of stepping through learn_msgs (engine.py)
    assert not new._propagate and new.prior_out is None and new.alpha_cell is None and not new.keep_prior_joint
    for e in (new, off, four):
        comp_block(e).fill_(SENTINEL)
    knobs = {} if new.B >= MIN_B else dict(I2C_FORWARD_HELPER="1")
    assert traced(new, capfd, lean_forward, ("self", lean_walk), **knobs)
    assert not traced(off, capfd, lean_forward, ("self", lean_walk), I2C_FORWARD_HELPER="0")
    assert not traced(four, capfd, lean_forward, ("plain", lean_walk), I2C_CHUNK_PASSES="4")
    assert new.em_iter == off.em_iter == four.em_iter == N and len(new.costs_m) == N
    same(new, off, keep, "I2C_FORWARD_HELPER=0")
    same(new, four, keep, "I2C_CHUNK_PASSES=4")
    if stepwise:
        step = make()
        comp_block(step).fill_(SENTINEL)
        for _ in range(N):
            step.learn_msgs()
        assert step.em_iter == N
        same(new, step, keep, "learn_msgs")
    return new


def oracle_for(case, eng):
    g = parity.with_horizon(load_case(case.name), case.T)
    x0, mu_u = parity.batched_inputs(g, case.B)
    meta = {**g.meta, "quad": list(case.quad or g.meta["quad"])}
    o = oracle_from_case(type(g)({**dict(g), "meta": np.array(json.dumps(meta)), "mu_u": mu_u}), x0=x0, sig_x0=g["sig_x0"],
                         z_traj=targets_of(case, eng) if case.targets else None)
    if case.tau is not None:
        o.tau = case.tau
    for _ in range(N):
        o.learn_msgs()
    return o


def pairs_with_oracle(eng, o):
    """(quantity, engine's, oracle's, tolerance class) after the same number of iterations: what check_batch_against_oracle compares"""
    f = eng.forward_messages()
    out = [(k, f[k], getattr(o, k), "msg") for k in parity.FWD]
    mu, sig = eng.marginal_state_action()
    K, k, sigK = eng.local_linear_policy()
    out += [("mu_xu0_m", mu, o.mu_xu0_m, "msg"), ("sig_xu0_m", sig, o.sig_xu0_m, "msg"), ("K", K, o.K, "policy"), ("k", k, o.k, "policy"),
            ("sigK", sigK, o.sigK, "policy"), ("alpha", eng.alpha, o.alpha, "msg"), ("cost", eng.costs_m[-1], o.costs_m[-1], "msg")]
    return [(n, parity.np_(a), np.asarray(b), c) for n, a, b, c in out]


def against_oracle(case, eng, label, keep=None, tol=1e-8, tol_policy=1e-7):
    o = oracle_for(case, eng)
    pairs = [(n, a if keep is None else a[keep], b if keep is None else b[keep], c) for n, a, b, c in pairs_with_oracle(eng, o)]
    errs = {n: rel_err(a, b) for n, a, b, _ in pairs}
    print("oracle-errors", *label, " ".join(f"{n}={e:.1e}" for n, e in errs.items()))  # (every figure, before anything is asserted)
    if eng.mixed:
        # fp32-STORED messages: every stored value carries a rounding of 6e-8, which the EM amplifies (tests/test_precision.py). The
        # bounds are that file's for this model: the median over the batch of the posterior-mean deviation and of the cost deviation
        b_med, _, b_cost = MIXED_BOUNDS[case.name]
        a, b = dict((n, a) for n, a, _, _ in pairs), dict((n, b) for n, _, b, _ in pairs)
        dm = np.abs(a["mu_xu0_m"] - b["mu_xu0_m"]).reshape(len(b["alpha"]), -1).max(1) / np.abs(b["mu_xu0_m"]).max()
        dc = np.abs(a["cost"] - b["cost"]) / np.abs(b["cost"])
        print("oracle-errors", *label, f"fp32-stored: mean median {np.median(dm):.1e} cost median {np.median(dc):.1e}")
        assert np.median(dm) <= b_med and np.median(dc) <= b_cost
        return
    for n, a, b, cls in pairs:
        parity.close(a, b, tol_policy if cls == "policy" else tol, f"{label} {n}")


def against_unrolled(case, a, capfd, knobs):
    """a: the shifted engine BEFORE its learn call. The twin holds a's cells in cell order with the ring at its origin; both run
    learn(N) on the helper path (the general variant on either side: targets are per cell)."""
    assert case.targets and a.t0 == case.shifts % case.T != 0
    b = prepared(a.lib, a.device.type, case, shifts=0)
    for key in ("post", "z", "feedforward"):
        getattr(b, key).copy_(a.cells(getattr(a, key)))
    for key in ("x0", "sig_x0", "alpha", "temp"):
        getattr(b, key).copy_(getattr(a, key))
    b.terminal_cell = a.terminal_cell  # (the flag stays with the cell it was set on: its index went down with every shift)
    b._problem.terminal_cell = int(a.terminal_cell)
    assert b.t0 == 0 and b.terminal_cell == case.T - 1 - case.shifts
    assert traced(b, capfd, False, ("self", case.lean_walk), **knobs)
    return b


GEOMETRY = {(13, 5): (3, 5, 3), (13, 3): (3, 5, 3), (13, 67): (3, 5, 3), (8, 4096): (2, 4, 4), (131, 5): (27, 5, 1)}


def _case(lib, device, capfd, case, cid):
    assert geometry(case.B, case.T) == GEOMETRY[(case.T, case.B)]
    keep = None if case.bad is None else [b for b in range(case.B) if b != case.bad]
    # the large batch: the i2c_learn calls alone on the host simulation, as tests/test_chunk_self_stitch.py
    new = four_paths(lambda: prepared(lib, device, case), capfd, case.lean_forward, case.lean_walk, keep,
                     stepwise=device != "cpu" or case.B < 1000)
    assert new.mixed == ("storage_dtype" in case.kw) and (new.xm is not None) == (new.zpost is not None) == case.full
    assert new.t0 == case.shifts % case.T and (new.z is not None) == case.targets
    if case.full:
        assert bool((new.cell_stats != 0).any())
    if case.bad is None:
        assert new.failures() == []
    else:
        assert [f[0] for f in new.failures()] == [case.bad] and int(new.status[case.bad]) != 0
        assert not torch.isfinite(new.post[..., case.bad]).all()
    if case.tau is not None:  # k_to_feedback: the first tau + 1 cells of the horizon, wherever the ring put them
        ff = new.cells(new.feedforward).cpu().numpy()
        assert ff[:case.tau + 1].sum() == 0 and ff[case.tau + 1:].all(), ff
    if case.shifts == 0:
        against_oracle(case, new, (cid, device), keep)
    return new


def _ring_with_targets(lib, device, capfd, case, cid):
    """... and the unrolled twin of a ring case with per-cell targets."""
    a = prepared(lib, device, case)
    knobs = dict(I2C_FORWARD_HELPER="1")
    b = against_unrolled(case, a, capfd, knobs)
    assert traced(a, capfd, False, ("self", case.lean_walk), **knobs)
    assert a.failures() == b.failures() == []
    assert torch.equal(a.cells(a.post), b.post), "posterior"
    assert torch.equal(a.cells(a.feedforward), b.feedforward), "feedforward"
    for key in ("fwd", "term_stats", "alpha") + (("xm", "zpost", "cell_stats") if case.full else ()):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    _case(lib, device, capfd, case, cid)


PEND, CART = Case(), Case(name="em_cartpole_T100", B=3)
WT = replace(PEND, quad=WEIGHTS, targets=True)
ALL = dict(quad=WEIGHTS, targets=True, shifts=3, tau=3)
CASES = {
    "weights": replace(PEND, quad=WEIGHTS),
    "weights-nonunit": replace(PEND, quad=NONUNIT),
    "targets": replace(PEND, targets=True),
    "ring3": replace(PEND, shifts=3),   # the wrap lands on a chunk boundary: cell 10 -> row 0
    "ring6": replace(PEND, shifts=6),   # ... inside chunk 1: cell 7 -> row 0
    "tau3": replace(PEND, tau=3),
    "ring3-tau3": replace(PEND, shifts=3, tau=3),
    "all-pendulum": replace(PEND, **ALL),
    "all-pendulum-nonunit": replace(PEND, **dict(ALL, quad=NONUNIT)),
    "all-cartpole": replace(CART, **ALL),
    "all-full-walker-ring6": replace(PEND, **dict(ALL, shifts=6), full=True),  # not LEANW for two reasons at once
    "weights-targets-fp32-stored": replace(WT, kw=dict(storage_dtype=torch.float32)),  # the S = float instantiations
    "weights-targets-B67": replace(WT, B=67),  # a second workgroup and a partly filled wave
    "weights-targets-B67-failing": replace(WT, B=67, bad=2),
    "weights-T8-B4096-default": replace(PEND, T=8, B=4096, quad=WEIGHTS),  # the default gate: nothing set
    "weights-nonunit-T8-B4096-default": replace(PEND, T=8, B=4096, quad=NONUNIT),
}
LONG = replace(WT, T=131)  # 27 chunks: more composites behind a chunk than one batch of loads of chunk_boundary_state; the device only
RING_WITH_TARGETS = [k for k, c in CASES.items() if c.shifts and c.targets]
PLAIN = [k for k in CASES if k not in RING_WITH_TARGETS]


def _linear_params(lib, device, capfd, quad):
    """LinearKnown with per-trajectory parameters (tests/test_model_params_batch.py holds their oracle): the coupled kernels read
    row b of the parameters on either variant."""
    model, B, T = linear_model(), 5, 13
    rows = param_rows(model, B, 0)
    kw = dict(LANE, **LEAN)
    if quad is not None:
        kw["quad"] = quad
    new = four_paths(lambda: params_engine(model, B, T, lib, device, model_params=rows, **kw), capfd, unit_sum(quad), True)
    assert new.failures() == [] and new.model_params is not None and geometry(B, T) == GEOMETRY[(T, B)]
    K = new.local_linear_policy()[0]
    assert not torch.equal(K[0], K[1])  # (the rows matter)


# ---- the host simulation -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


@pytest.mark.parametrize("cid", PLAIN)
def test_hostsim_general_learn_paths(sim, capfd, cid):
    _case(sim, "cpu", capfd, CASES[cid], cid)


@pytest.mark.parametrize("cid", RING_WITH_TARGETS)
def test_hostsim_general_learn_paths_ring_with_targets(sim, capfd, cid):
    _ring_with_targets(sim, "cpu", capfd, CASES[cid], cid)


@pytest.mark.parametrize("quad", (None, NONUNIT), ids=("unit", "weights-nonunit"))
def test_hostsim_general_learn_paths_linear_params(sim, capfd, quad):
    _linear_params(sim, "cpu", capfd, quad)


# ---- the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    lib = pkg.load_library()
    assert not lib.is_host_sim, "GPU tests must run the HIP build"
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("cid", PLAIN)
def test_hip_general_learn_paths(hip, capfd, cid):
    _case(hip, "cuda", capfd, CASES[cid], cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", RING_WITH_TARGETS)
def test_hip_general_learn_paths_ring_with_targets(hip, capfd, cid):
    _ring_with_targets(hip, "cuda", capfd, CASES[cid], cid)


@pytest.mark.gpu
@pytest.mark.parametrize("quad", (None, NONUNIT), ids=("unit", "weights-nonunit"))
def test_hip_general_learn_paths_linear_params(hip, capfd, quad):
    _linear_params(hip, "cuda", capfd, quad)


@pytest.mark.gpu
def test_hip_general_learn_paths_long_chain(hip, capfd):
    _case(hip, "cuda", capfd, LONG, "weights-targets-T131")
