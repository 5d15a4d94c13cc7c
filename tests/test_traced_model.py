"""Models written in Python (i2c.traced_model.TracedModel, tests/plugins/py_models.py) through the solver: the generated functor
against the hand-written functor of the same math (1e-8, the project's figure for two evaluations of one computation that round
differently: DESIGN section 8) and against the NumPy oracle fed the model's own NumPy side (the tolerances of
tests/test_model_plugin.py), on every kernel family the model is eligible for; Linearize() with the emitted Jacobian and with
dual numbers; per-trajectory parameters; the I2cGraph facade; the MPC step with the filter; the header cache.
CPU: the host simulation (g++ builds of the generated headers, made on first use); `-m gpu`: the hipcc builds of build()."""
import copy
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import load_case
from parity import close, np_

pkg = parity.pkg
PLUGINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plugins")
if PLUGINS not in sys.path:
    sys.path.insert(0, PLUGINS)
import py_models  # noqa: E402
from i2c.known_models import make_env_model  # noqa: E402
from i2c.model import TracedModel  # noqa: E402,F401  (exported from i2c.model, as KnownModel is)

STARTED = time.time()
T, ITERS = 12, 3
TOL = 1e-8
SYSTEMS = ("pendulum", "cartpole", "van_der_pol")
CASES = {"pendulum": ("em_pendulum_T200", "lin_pendulum_T100"), "cartpole": ("em_cartpole_T100", "lin_cartpole_T100")}


@functools.lru_cache(None)
def traced(system, jacobian=True):
    cls = {"pendulum": py_models.PyPendulum, "cartpole": py_models.PyCartpole, "van_der_pol": py_models.PyVanDerPol}[system]
    return cls(jacobian=jacobian)


@functools.lru_cache(None)
def hand_written(system):
    if system == "van_der_pol":
        from test_model_plugin import VanDerPolKnown

        return VanDerPolKnown()
    return make_env_model({"pendulum": "PendulumKnown", "cartpole": "CartpoleKnown"}[system])


@functools.lru_cache(None)
def problem(system, B, inference="cubature"):
    """(constructor arguments after the model, keyword arguments) of one small problem: T = 12 cells of the golden case of the
    system (the Van der Pol problem of tests/test_model_plugin.py), B perturbed initial states and action priors."""
    if system == "van_der_pol":
        from test_model_plugin import problem as vdp

        p = vdp(B=B, T=T)
        return (T, p["Q"], p["R"], p["Qf"], p["alpha"], p["tol"], p["mu_u"], p["sig_u"]), dict(x0=p["x0"], inference=inference)
    g = parity.with_horizon(load_case(CASES[system][inference == "linearize"]), T)
    x0, mu_u = parity.batched_inputs(g, B)
    m = g.meta
    return (T, g.get("Q"), g["R"], g.get("Qf"), m["alpha"], m["tol"], mu_u, g["sig_u"]), dict(x0=x0, inference=inference)


def engine(model, system, B, lib, device, inference="cubature", **kw):
    args, kws = problem(system, B, inference)
    return pkg.BatchedI2c(model, *args, device=device, lib=lib, **kws, **kw)


class OracleView:
    """A TracedModel's NumPy side in the oracle's protocol (oracle/models_numpy.py): flat x0 / targets, the model's own functions."""

    has_terminal_obs = True

    def __init__(self, m):
        self.name, self.dim_x, self.dim_u, self.dim_z, self.dim_z_term = m.name, m.dim_x, m.dim_u, m.dim_z, m.dim_z_term
        self.dim_xu = m.dim_xu
        self.x0, self.sig_x0, self.sig_eta = np.reshape(m.x0, -1), m.sig_x0, m.sig_eta
        self.zg, self.zg_term = np.reshape(m.zg, -1), np.reshape(m.zg_term, -1)
        self.dynamics, self.observe, self.observe_terminal = m.dynamics, m.observe, m.observe_terminal


def snapshot(o):
    return {k: np.array(getattr(o, k)) for k in ("mu_xu0_m", "sig_xu0_m", "K", "k", "sigK", "alpha")} | {"cost": np.array(o.costs_m[-1])}


@functools.lru_cache(None)
def oracle_run(system, B, inference="cubature", n_iters=ITERS):
    """The NumPy oracle on the traced model's NumPy side, computed once per (system, B, rule): a snapshot after every iteration."""
    from oracle.i2c_linearize_numpy import I2cLinearizeOracle
    from oracle.i2c_numpy import CubatureRule, I2cOracle

    args, kws = problem(system, B, inference)
    cls = I2cLinearizeOracle if inference == "linearize" else I2cOracle
    o = cls(OracleView(traced(system)), *args, rule=CubatureRule(1, 0, 0), x0=kws["x0"])
    out = []
    for _ in range(n_iters):
        o.learn_msgs()
        out.append(snapshot(o))
    return out


def same(a, b, what, tol=TOL):
    """Every per-cell quantity of two engines: posterior, controller, observed marginal, smoothed state, temperature, status."""
    for name, fa, fb in (("mu_xu0_m sig_xu0_m", a.marginal_state_action(), b.marginal_state_action()),
                         ("K k sigK", a.local_linear_policy(), b.local_linear_policy()),
                         ("mu_z0_m sig_z0_m", a.observed_marginal(), b.observed_marginal()),
                         ("mu_x3_m sig_x3_m", a.smoothed_next_state(), b.smoothed_next_state())):
        for n, x, y in zip(name.split(), fa, fb):
            close(np_(x), np_(y), tol, f"{what} {n}")
    close(np_(a.alpha), np_(b.alpha), tol, f"{what} alpha")
    close(np_(a.costs_m[-1]), np_(b.costs_m[-1]), tol, f"{what} cost")
    assert torch.equal(a.status, b.status) and a.failures() == [], f"{what}: status {a.failures()} / {b.failures()}"


def against_oracle(eng, ref, what, tol_policy=1e-7):
    """Cubature cases: the tolerances of tests/test_model_plugin.py (controller 1e-7). Linearize(): 1e-8 throughout."""
    mu, sig = eng.marginal_state_action()
    close(np_(mu), ref["mu_xu0_m"], 1e-8, what + " mu_xu0_m")
    close(np_(sig), ref["sig_xu0_m"], 1e-8, what + " sig_xu0_m")
    for n, v in zip(("K", "k", "sigK"), eng.local_linear_policy()):
        close(np_(v), ref[n], tol_policy, f"{what} {n}")
    close(np_(eng.alpha), ref["alpha"], 1e-8, what + " alpha")
    close(np_(eng.costs_m[-1]), ref["cost"], 1e-8, what + " cost")


def lanes_of(eng_dims, family):
    return {"lane": -1, "quad": 64, "group": eng_dims.group_lanes}[family]


# ---- the checks, on whichever library --------------------------------------------------------------------------------------------
def check_same_math(lib, device, system, B, family):
    model, hand = traced(system), hand_written(system)
    dims = lib.query(model.resolve_model_id(lib))
    assert dims.quad == 1 and dims.group_lanes in (4, 8)  # (all three systems are eligible for every family)
    lanes = lanes_of(dims, family)
    a, b = engine(model, system, B, lib, device, group_lanes=lanes), engine(hand, system, B, lib, device, group_lanes=lanes)
    assert a.model_id >= pkg._native.PLUGIN_BASE and a.model_id != b.model_id
    ref = oracle_run(system, B)
    for it in range(ITERS):
        a.learn_msgs()
        b.learn_msgs()
        what = f"{system} B={B} {family} it{it + 1}"
        assert a.forward_family == b.forward_family == family, (a.forward_family, b.forward_family)
        same(a, b, what + " traced vs hand-written")
        against_oracle(a, ref[it], what + " traced vs oracle")


def check_linearize(lib, device, system, B):
    ref = oracle_run(system, B, "linearize", 2)
    engs = [engine(m, system, B, lib, device, "linearize", group_lanes=-1)
            for m in (traced(system), traced(system, jacobian=False), hand_written(system))]
    assert len({e.model_id for e in engs}) == 3
    for it in range(2):
        for e in engs:
            e.learn_msgs()
        what = f"{system} B={B} linearize it{it + 1}"
        same(engs[0], engs[1], what + " emitted Jacobian vs dual numbers")
        same(engs[0], engs[2], what + " traced vs hand-written")
        against_oracle(engs[0], ref[it], what + " traced vs oracle", tol_policy=1e-8)
        against_oracle(engs[1], ref[it], what + " traced, dual numbers, vs oracle", tol_policy=1e-8)


def check_gauss_hermite(lib, device, lanes, family):
    a = engine(traced("pendulum"), "pendulum", 5, lib, device, "gauss_hermite", gh_degree=3, group_lanes=lanes)
    b = engine(hand_written("pendulum"), "pendulum", 5, lib, device, "gauss_hermite", gh_degree=3, group_lanes=lanes)
    a.learn_msgs()
    b.learn_msgs()
    assert a.forward_family == b.forward_family == family
    same(a, b, f"pendulum GaussHermite(3) {family}")


def check_parameters(lib, device):
    """Row b of a solve with per-trajectory parameters equals the B = 1 solve of a model copy with those parameters, bit for bit
    (the lane family on both sides) -- the property tests/test_model_params_batch.py checks for header models."""
    from test_model_params_batch import OUTPUTS, outputs, param_rows, with_params

    model, B = traced("van_der_pol"), 5
    rows = param_rows(model, B, 3)
    args, kws = problem("van_der_pol", B)

    def solve(m, x0, mu_u, **kw):
        e = pkg.BatchedI2c(m, *args[:6], mu_u, args[7], x0=x0, device=device, lib=lib, group_lanes=-1, deterministic_family=True, **kw)
        for _ in range(ITERS):
            e.learn_msgs()
        assert e.failures() == []
        return outputs(e)

    out = solve(model, kws["x0"], args[6], model_params=rows)
    for b in range(B):
        one = solve(with_params(model, rows[b]), kws["x0"][b: b + 1], args[6][b: b + 1])
        for n in OUTPUTS:
            assert np.array_equal(out[n][b], one[n][0]), f"{n} of trajectory {b}"
    assert not np.array_equal(out["K"][0], out["K"][1])


def check_facade(lib, device):
    from i2c.exp_types import CubatureQuadrature
    from i2c.i2c import I2cGraph

    args, kws = problem("pendulum", 1)
    graphs = []
    for sys_ in (make_env_model(py_models.PyPendulum), hand_written("pendulum")):
        g = I2cGraph(sys_, *args[:6], args[6][0], args[7], None, None, CubatureQuadrature(1, 0, 0), lib=lib, device=device)
        for _ in range(2):
            g.learn_msgs()
        graphs.append(g)
    assert isinstance(graphs[0].sys, py_models.PyPendulum) and make_env_model(graphs[0].sys) is graphs[0].sys
    for n, x, y in zip(("K", "k", "sigK"), graphs[0].get_local_linear_policy(), graphs[1].get_local_linear_policy()):
        close(np.asarray(x), np.asarray(y), TOL, f"I2cGraph {n}")


def check_closed_loop(lib, device):
    """Three control steps (filter on the belief, two sweeps, first action, shift) on the same measurements."""
    B, H = 5, 10
    args, kws = problem("pendulum", B)
    plant = hand_written("pendulum")
    sig_zeta = 1e-4 * np.eye(3)
    runs = []
    for model in (hand_written("pendulum"), traced("pendulum")):
        e = pkg.BatchedI2c(model, H, *args[1:6], args[6][:, :H], args[7], x0=kws["x0"], device=device, lib=lib)
        e.learn_msgs()
        e.enable_per_cell_alpha()
        x, u = kws["x0"].copy(), args[6][:, 0, :].copy()
        acts = []
        for step in range(3):
            x = plant.dynamics(np.hstack((x, u)))
            y = torch.as_tensor(np.ascontiguousarray(plant.measure(x).T), dtype=torch.float64, device=device)
            mu_u, _ = e.mpc_step(2, y, torch.as_tensor(np.ascontiguousarray(u.T), dtype=torch.float64, device=device), sig_zeta)
            acts.append(np_(mu_u).copy())
            u = (acts[-1] if not runs else runs[0][0][step]).copy()  # (the second engine is fed the first one's actions and measurements)
        assert e.failures() == []
        runs.append((acts, np_(e.x0).copy(), np_(e.sig_x0).copy()))
    for step in range(3):
        close(runs[1][0][step], runs[0][0][step], TOL, f"mpc_step {step} action")
    close(runs[1][1], runs[0][1], TOL, "belief mean")
    close(runs[1][2], runs[0][2], TOL, "belief covariance")


# ---- CPU: the host simulation ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    """The host simulation with every model of this file registered: on a fresh checkout their g++ builds run side by side."""
    import concurrent.futures

    lib = hostsim.load()
    models = [traced(s, j) for s in SYSTEMS for j in (True, False)] + [hand_written("van_der_pol")]
    with concurrent.futures.ThreadPoolExecutor(3) as pool:
        assert all(i >= pkg._native.PLUGIN_BASE for i in pool.map(lambda m: m.resolve_model_id(lib), models))
    return lib


@pytest.fixture(scope="module")
def gpu_lib():
    return pkg.load_library()


GRID = [(s, B, f) for s in SYSTEMS for B in (5, 67) for f in ("lane", "quad", "group")]


@pytest.mark.parametrize("system,B,family", GRID)
def test_same_math_two_functors_hostsim(lib, system, B, family):
    check_same_math(lib, "cpu", system, B, family)


@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("B", [5, 67])
def test_linearize_hostsim(lib, system, B):
    check_linearize(lib, "cpu", system, B)


@pytest.mark.parametrize("lanes,family", [(-1, "lane"), (64, "grid")])
def test_gauss_hermite_hostsim(lib, lanes, family):
    check_gauss_hermite(lib, "cpu", lanes, family)


def test_parameters_hostsim(lib):
    check_parameters(lib, "cpu")


def test_facade_hostsim(lib):
    check_facade(lib, "cpu")


def test_closed_loop_hostsim(lib):
    check_closed_loop(lib, "cpu")


def test_header_cache(lib, monkeypatch):
    """Resolving a model twice builds once and gives one id; another constant is another header, another library and another id;
    neither touches the in-tree library. (Host logic: not repeated on the GPU, where it would only compile.)"""
    import importlib.util

    built = []
    real = importlib.util.spec_from_file_location

    def spy(name, path, *a, **k):  # KnownModel._build_plugin loads build.py on every build request
        if os.path.basename(str(path)) == "build.py":
            built.append(path)
        return real(name, path, *a, **k)

    solver, stamp = lib.path, os.stat(lib.path).st_mtime_ns
    first, again = py_models.PyCartpole(), py_models.PyCartpole()
    monkeypatch.setattr(importlib.util, "spec_from_file_location", spy)
    lib.__dict__.get("_plugin_ids", {}).pop((first.emit(), first.hip_struct, first.hip_name), None)
    i0, i1 = first.resolve_model_id(lib), again.resolve_model_id(lib)
    assert i0 == i1 >= pkg._native.PLUGIN_BASE and len(built) == 1 and first.hip_header == again.hip_header
    heavier = type("PyCartpole", (py_models.PyCartpole,), {"g": 9.82})()
    i2 = heavier.resolve_model_id(lib)
    assert i2 not in (i0, hand_written("cartpole").model_id) and len(built) == 2
    assert heavier.hip_header != first.hip_header and heavier.hip_name != first.hip_name and heavier.hip_struct != first.hip_struct
    assert os.path.dirname(heavier.hip_header) == os.path.dirname(first.hip_header)
    assert (os.stat(solver).st_mtime_ns, lib.path) == (stamp, solver)
    assert lib.query(i2).nx == 4 and copy.deepcopy(heavier).resolve_model_id(lib) == i2
    # a model changed AFTER its first use is traced again: the device follows what the functions and flags now say
    again.jacobian = False
    assert again.resolve_model_id(lib) == traced("cartpole", jacobian=False).resolve_model_id(lib) != i0 and len(built) == 2
    again.jacobian = True
    assert again.resolve_model_id(lib) == i0


# ---- MI355X ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_libraries_of_build_are_found_gpu(gpu_lib):
    """Every model this file solves on the GPU was traced, emitted and compiled by build(): tracing it again here names the same
    library, which exists and is not rebuilt by resolving the model (its file is older than this process)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("i2c_amd_build", os.path.join(os.path.dirname(PLUGINS), "..", "input-inference-for-control_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    for cls, kw in py_models.BUILT:
        m = cls(**kw)
        m.emit()
        path = build.model_lib_path(m.hip_name)
        assert os.path.exists(path), f"{cls.__name__}{kw}: build() left no {os.path.basename(path)}"
        assert m.resolve_model_id(gpu_lib) >= pkg._native.PLUGIN_BASE
        assert os.stat(path).st_mtime < STARTED, f"{os.path.basename(path)} was compiled by this test run"


@pytest.mark.gpu
@pytest.mark.parametrize("system,B,family", GRID)
def test_same_math_two_functors_gpu(gpu_lib, system, B, family):
    check_same_math(gpu_lib, "cuda", system, B, family)


@pytest.mark.gpu
@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("B", [5, 67])
def test_linearize_gpu(gpu_lib, system, B):
    check_linearize(gpu_lib, "cuda", system, B)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,family", [(-1, "lane"), (64, "grid")])
def test_gauss_hermite_gpu(gpu_lib, lanes, family):
    check_gauss_hermite(gpu_lib, "cuda", lanes, family)


@pytest.mark.gpu
def test_parameters_gpu(gpu_lib):
    check_parameters(gpu_lib, "cuda")


@pytest.mark.gpu
def test_facade_gpu(gpu_lib):
    check_facade(gpu_lib, "cuda")


@pytest.mark.gpu
def test_closed_loop_gpu(gpu_lib):
    check_closed_loop(gpu_lib, "cuda")
