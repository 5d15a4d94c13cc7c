"""The host layer (engine.py) asks the library for exactly what it asked before it was refactored.

tools/engine_call_trace.py drives BatchedI2c, the I2cGraph facade and the MPC policy through every path of the host layer behind a
recording proxy of the library: entry names, scalar arguments, which engine tensor each pointer is, the descriptor's scalar fields
and optional pointers at every call, and the lengths / dtypes of the history lists afterwards. tests/golden/engine_calls.json is
that trace written by the commit BEFORE the refactor (04df0b4); it is never regenerated from the code under test.

Also here: learn()'s path choice against the two conditionals it replaced, for every combination of the flags they read, and
iteration_health() handing out arrays the caller owns."""
import importlib.util
import itertools
import json
import os
import types

import numpy as np
import pytest

import hostsim
import parity
from i2c.known_models import make_env_model

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
    assert sorted(now) == sorted(golden) and len(golden) >= 20


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
