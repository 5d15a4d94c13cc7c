"""The host layer (engine.py, i2c/graph.py, i2c/policy/mpc.py) asks the library for exactly what it asked before it was refactored.

tools/engine_call_trace.py drives BatchedI2c, the I2cGraph facade and the MPC policies through every path of the host layer behind a
recording proxy of the library: entry names, scalar arguments, which engine tensor each pointer is, the descriptor's scalar fields
and optional pointers at every call, and the lengths / dtypes of the history lists afterwards. tests/golden/engine_calls.json is
that trace written by the commit BEFORE a refactor (the engine scenarios by 04df0b4, the facade and policy scenarios by d33584d);
it is never regenerated from the code under test.

Also here: learn()'s path choice against the two conditionals it replaced, for every combination of the flags they read,
iteration_health() handing out arrays the caller owns, and what the engine's revision counters make true by construction: cell
views and the policy's belief follow the engine whoever changed it, a batched policy that records survives one failed trajectory,
and a single-loop step that raises leaves the four histories the same length."""
import importlib.util
import itertools
import json
import os
import types

import numpy as np
import pytest
import torch

import hostsim
import parity
from i2c.exp_types import CubatureQuadrature
from i2c.i2c import I2cGraph
from i2c.known_models import make_env_model
from i2c.policy.mpc import PartiallyObservedMpcPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = parity.pkg


def _tool():
    spec = importlib.util.spec_from_file_location("engine_call_trace", os.path.join(ROOT, "tools", "engine_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def traces():
    tool = _tool()
    with open(tool.GOLDEN) as f:
        return tool.build_trace(hostsim.load()), json.load(f)


def test_scenarios_are_the_golden_files(traces):
    now, golden = traces
    assert sorted(now) == sorted(golden) and len(golden) == 40


@pytest.mark.parametrize("scenario", sorted(_tool().SCENARIOS))
def test_library_calls_equal_parent(traces, scenario):
    now, golden = traces[0][scenario], traces[1][scenario]
    assert [c["entry"] for c in now["calls"]] == [c["entry"] for c in golden["calls"]], "the sequence of library calls"
    for i, (a, b) in enumerate(zip(now["calls"], golden["calls"])):
        assert a == b, f"call {i} ({b['entry']})"
    assert now["history"] == golden["history"], "lengths / dtypes / shapes of the history lists"


def _learn_path_before(e, n_iters):
    """learn()'s two conditionals as they stood before _learn_path() (commit 04df0b4), verbatim."""
    if (e._propagate and n_iters > 0 and e.alpha_cell is None and not e.keep_prior_joint and e.prior_out is None
            and not e.mixed and not e.uses_group_kernels and not e.linearize and not e.gauss_hermite):
        return "propagate"
    if e._propagate or e.prior_out is not None or n_iters <= 0 or e.alpha_cell is not None or e.keep_prior_joint:
        return "stepwise"
    return "fused"


def test_learn_path_equals_the_conditionals_it_replaced():
    flags = ("_propagate", "keep_prior_joint", "mixed", "uses_group_kernels", "linearize", "gauss_hermite")
    seen = set()
    for n_iters, alpha_cell, prior_out, *bits in itertools.product((-1, 0, 1, 3), (None, object()), (None, object()),
                                                                   *[(False, True)] * len(flags)):
        e = types.SimpleNamespace(alpha_cell=alpha_cell, prior_out=prior_out, **dict(zip(flags, bits)))
        path = pkg.BatchedI2c._learn_path(e, n_iters)
        assert path == _learn_path_before(e, n_iters), (n_iters, vars(e))
        seen.add(path)
    assert seen == {"stepwise", "fused", "propagate"}


def _health_is_owned(lib, device):
    """iteration_health() returns arrays the caller owns: a second call neither overwrites nor aliases the first one's."""
    T, B = 4, 2
    rng = np.random.default_rng(0)
    eng = pkg.BatchedI2c(make_env_model("PendulumKnown"), T, np.diag([1.0, 100.0, 1.0]), np.diag([2.0]), np.diag([1.0, 100.0, 1.0]),
                         100.0, 0.0, 1e-2 * rng.normal(size=(B, T, 1)), 2.0 * np.eye(1),
                         x0=np.array([np.pi, 0.0]) + 1e-2 * rng.normal(size=(B, 2)), lib=lib, device=device)
    eng.learn_msgs()
    status1, alpha1 = eng.iteration_health()
    kept = status1.copy(), alpha1.copy()
    assert np.array_equal(alpha1, eng.alphas_desired[-1].cpu().numpy()) and np.array_equal(status1, eng.status.cpu().numpy())
    eng.learn_msgs()
    status2, alpha2 = eng.iteration_health()
    assert not np.array_equal(alpha2, kept[1]), "the second iteration has another alpha_hat"
    assert np.array_equal(status1, kept[0]) and np.array_equal(alpha1, kept[1]), "the first pair still holds its first values"
    for first in (status1, alpha1):
        for second in (status2, alpha2):
            assert not np.shares_memory(first, second)
    assert status1.dtype == np.int32 and alpha1.dtype == np.float64 and status1.flags.owndata and alpha1.flags.owndata


def test_iteration_health_returns_owned_arrays_cpu():
    _health_is_owned(hostsim.load(), "cpu")


@pytest.mark.gpu
def test_iteration_health_returns_owned_arrays_gpu():
    _health_is_owned(None, "cuda")


# ------------------------------------------------------------------------------------- views follow the engine's revision counters
T = 6
BACKENDS = [pytest.param((hostsim.load, "cpu"), id="sim"), pytest.param((lambda: None, "cuda"), id="hip", marks=pytest.mark.gpu)]


def _graph(backend, B):
    load, device = backend
    rng = np.random.default_rng(0)
    model = make_env_model("PendulumKnown")
    model.sig_zeta = 1e-3 * np.eye(3)
    Q = np.diag([1.0, 100.0, 1.0])
    x0 = np.array([np.pi, 0.0]) + 1e-2 * rng.normal(size=(B, 2))
    return I2cGraph(model, T, Q, np.diag([2.0]), Q, 100.0, 0.0, 1e-2 * rng.normal(size=(T, 1)), 2.0 * np.eye(1), None, None,
                    CubatureQuadrature(1, 0, 0), lib=load(), device=device, batch=B, x0=x0)


def _y(g, seed=1):
    rng = np.random.default_rng(seed)
    return np.asarray(g.sys.measure(np.array([np.pi, 0.0]) + 1e-2 * rng.normal(size=(g.B, 2))), float)


def _host(t):
    return np.array(t.detach().to(torch.float64).cpu().numpy(), copy=True)  # (on the host simulation .numpy() is a view of the buffer)


@pytest.mark.parametrize("change", ["engine.learn(2)", "engine.forward_backward()", "_update_priors()"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("backend", BACKENDS)
def test_cell_views_follow_the_engine(backend, B, change):
    """A cell attribute read after the ENGINE was driven directly equals a fresh read of the engine, and differs from the read
    before exactly where the engine's buffers differ."""
    g = _graph(backend, B)
    e, t = g.engine, 2
    g.learn_msgs()
    if change == "_update_priors()":
        g._forward_backward_msgs()

    def engine_now():
        mu, sig = e.marginal_state_action()
        K = e.local_linear_policy()[0]
        pick = (lambda a: _host(a)[0, t]) if B == 1 else (lambda a: _host(a)[:, t])
        return pick(mu[..., : e.nx]).reshape((-1, 1) if B == 1 else (B, -1)), pick(sig[..., : e.nx, : e.nx]), pick(K)

    def cell_now():
        return g.cells[t].mu_x0_m, g.cells[t].sig_x0_m, g.cells[t].K

    before, engine_before = cell_now(), engine_now()
    {"engine.learn(2)": lambda: e.learn(2), "engine.forward_backward()": e.forward_backward, "_update_priors()": g._update_priors}[change]()
    after, engine_after = cell_now(), engine_now()
    for a, b, ea, eb in zip(before, after, engine_before, engine_after):
        assert np.array_equal(b, eb) and b.shape == eb.shape, "the view equals a fresh read of the engine"
        assert np.array_equal(a, b) == np.array_equal(ea, eb), "... and changed where the engine's buffers did"
    if change != "_update_priors()":  # (which moves no numbers: the posterior buffer becomes the prior)
        assert not any(np.array_equal(a, b) for a, b in zip(engine_before, engine_after)), "the sweeps did change the posterior"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("backend", BACKENDS)
def test_policy_belief_follows_the_engine(backend, B):
    """pol.mu / pol.covar equal the engine's belief after engine.set_initial_state(...) and after sys.x0 = ... followed by a sweep."""
    g = _graph(backend, B)
    e = g.engine
    pol = PartiallyObservedMpcPolicy(g, 1, 2.0 * np.eye(1))
    pol(0, _y(g), np.zeros((B, 1)))

    def engine_belief():
        mu, cov = _host(e.x0.T), _host(pkg.engine.unpack_sym(e.sig_x0.T, e.nx))
        return (mu[0].reshape(-1, 1), cov[0]) if B == 1 else (mu, cov)

    def check(what):
        for got, want in zip((pol.mu, pol.covar), engine_belief()):
            assert got.shape == want.shape and np.array_equal(got, want), what

    check("after a control step")
    mu = np.array([3.0, 0.1]) + 0.01 * np.arange(B)[:, None]
    cov = np.array([[2e-3, 1e-4], [1e-4, 3e-3]])
    e.set_initial_state(mu, cov)
    check("after engine.set_initial_state")
    assert np.array_equal(np.asarray(pol.mu).reshape(B, -1), mu) and np.array_equal(np.asarray(pol.covar).reshape(B, 2, 2)[-1], cov)
    g.sys.x0, g.sys.sig_x0 = np.array([[2.9], [-0.1]]), 2.0 * cov
    g._forward_msgs()
    check("after sys.x0 = ... and a sweep")
    if B == 1:  # (only a single-trajectory graph follows sys.x0: I2cGraph._sync_initial_state)
        assert np.array_equal(pol.mu, g.sys.x0) and np.array_equal(pol.covar, g.sys.sig_x0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_batched_recording_policy_survives_one_failed_trajectory(backend):
    """record_history = True on a BATCHED policy, one trajectory failing through its inputs (an indefinite sig_x0 row: a status
    word, as tests/test_edge_cases.py): actions for the others, the failure in engine.failures(), sys.x0 / sig_x0 left alone."""
    B, bad = 3, 1
    g = _graph(backend, B)
    e = g.engine
    pol = PartiallyObservedMpcPolicy(g, 1, 2.0 * np.eye(1))
    pol.record_history = True
    cov = np.broadcast_to(np.asarray(g.sys.sig_x0, float), (B, 2, 2)).copy()
    cov[bad] = -cov[bad]
    e.set_initial_state(_host(e.x0.T), cov)
    x0_before, sig_x0_before = np.array(g.sys.x0, copy=True), np.array(g.sys.sig_x0, copy=True)
    u = pol(0, _y(g), np.zeros((B, 1)))
    assert u.shape == (B, 1) and np.isfinite(u[[b for b in range(B) if b != bad]]).all()
    assert [f[0] for f in e.failures()] == [bad]
    assert np.array_equal(g.sys.x0, x0_before) and np.array_equal(g.sys.sig_x0, sig_x0_before)
    assert len(pol.mus) == len(pol.covars) == len(pol.xu_history) == len(pol.z_history) == 1 and pol.mus[0].shape == (B, 2)


@pytest.mark.parametrize("backend", BACKENDS)
def test_raising_single_loop_step_keeps_the_histories_aligned(backend):
    g = _graph(backend, 1)
    pol = PartiallyObservedMpcPolicy(g, 1, 2.0 * np.eye(1))
    u = pol(0, _y(g), np.zeros((1, 1)))
    g.engine.set_initial_state(pol.mu.reshape(-1), -np.asarray(pol.covar))  # a bad input: the filter / forward sweep flag it
    with pytest.raises(pkg.I2cNumericalError):
        pol(1, _y(g, 2), u)
    assert len(pol.mus) == len(pol.covars) == len(pol.xu_history) == len(pol.z_history) == 1
