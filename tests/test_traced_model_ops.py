"""Models of the wider operation set (`operations = "extended"`: tests/plugins/py_models_ops.py) through the solver, mirroring
tests/test_traced_model.py: T = 12 cells, 3 EM iterations, B = 5 and B = 67 (across a wavefront, with a ragged tail), every
kernel family the models are eligible for (lane, quad, group) against the NumPy oracle fed the model's own NumPy side (1e-8, the
controller 1e-7: the tolerances of that file); Linearize() with the emitted Jacobian against dual numbers (1e-8) and, for the
complex-analytic PyDragPendulum, against the Linearize oracle; the per-trajectory slope parameter, which the general sine reads,
bit for bit against B = 1 solves; and the functors' values pointwise through the public entry points (plant_step, rollout).
CPU: the host simulation (g++ builds of the generated headers, made on first use); `-m gpu`: the hipcc builds of build().

Pointwise bound: 4 eps n_ops of tests/test_functor_codegen_ops.py (derived there), widened x 4 on either library because the
hardware's seed instructions differ from the emulated ones: 16 eps n_ops, per column relative to the column's scale (8.2e-14 for
PyDragPendulum, 7.1e-14 for PyHovercraft)."""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

import hostsim
import parity
from parity import np_

pkg = parity.pkg
PLUGINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plugins")
if PLUGINS not in sys.path:
    sys.path.insert(0, PLUGINS)
import py_models_ops  # noqa: E402
from probe_util import EPS, deviation, extra_points, points  # noqa: E402
from test_functor_codegen_ops import kink_points, n_ops  # noqa: E402
from test_traced_model import OracleView, against_oracle, lanes_of, same, snapshot  # noqa: E402

STARTED = time.time()
T, ITERS = 12, 3
SYSTEMS = {"drag_pendulum": py_models_ops.PyDragPendulum, "hovercraft": py_models_ops.PyHovercraft}


@functools.lru_cache(None)
def traced(system, jacobian=True):
    return SYSTEMS[system](jacobian=jacobian)


@functools.lru_cache(None)
def problem(system, B):
    """(constructor arguments after the model, keyword arguments): B perturbed initial states and action priors. The hovercraft
    starts near rest, so its sigma points straddle the kinks at vx = 0 and vy = 0 from the first cell on."""
    rng = np.random.default_rng(5)
    m = traced(system)
    if system == "drag_pendulum":
        x0 = np.array([np.pi, 0.0]) + 1e-2 * rng.normal(size=(B, 2))
        Q, R, Qf, sig_u = np.diag([1.0, 100.0, 1.0]), np.diag([2.0]), np.diag([20.0, 2.0]), 2.0 * np.eye(1)
    else:
        x0 = np.array([1.0, -0.5, 0.0, 0.0]) + 1e-2 * rng.normal(size=(B, 4))
        Q, R, Qf, sig_u = np.diag([10.0, 10.0, 1.0, 1.0]), 0.5 * np.eye(2), np.diag([20.0, 20.0, 2.0, 2.0]), 0.5 * np.eye(2)
    mu_u = 1e-2 * rng.normal(size=(B, T, m.dim_u))
    return (T, Q, R, Qf, 2.0, 0.5, mu_u, sig_u), dict(x0=x0)


def engine(model, system, B, lib, device, **kw):
    args, kws = problem(system, B)
    return pkg.BatchedI2c(model, *args, device=device, lib=lib, **kws, **kw)


@functools.lru_cache(None)
def oracle_run(system, B, inference="cubature", n_iters=ITERS):
    """The NumPy oracle on the model's NumPy side, once per (system, B, rule): a snapshot after every iteration."""
    from oracle.i2c_linearize_numpy import I2cLinearizeOracle
    from oracle.i2c_numpy import CubatureRule, I2cOracle

    args, kws = problem(system, B)
    view = OracleView(traced(system))
    if inference == "linearize":
        o = I2cLinearizeOracle(view, *args, x0=kws["x0"])
    else:
        o = I2cOracle(view, *args, rule=CubatureRule(1, 0, 0), x0=kws["x0"])
    out = []
    for _ in range(n_iters):
        o.learn_msgs()
        out.append(snapshot(o))
    return out


# ---- the checks, on whichever library --------------------------------------------------------------------------------------------
def check_em(lib, device, system, B, family):
    model = traced(system)
    dims = lib.query(model.resolve_model_id(lib))
    assert dims.quad == 1 and dims.group_lanes == (4 if system == "drag_pendulum" else 8)
    eng = engine(model, system, B, lib, device, group_lanes=lanes_of(dims, family))
    assert eng.model_id >= pkg._native.PLUGIN_BASE
    ref = oracle_run(system, B)
    for it in range(ITERS):
        eng.learn_msgs()
        assert eng.forward_family == family, eng.forward_family
        assert eng.failures() == [] and not torch.any(eng.status != 0)
        against_oracle(eng, ref[it], f"{system} B={B} {family} it{it + 1} traced vs oracle")


def check_linearize(lib, device, system, B):
    engs = [engine(traced(system, j), system, B, lib, device, inference="linearize", group_lanes=-1) for j in (True, False)]
    assert engs[0].model_id != engs[1].model_id
    ref = oracle_run(system, B, "linearize", 2) if system == "drag_pendulum" else None  # (complex-step Jacobians: analytic functions)
    for it in range(2):
        for e in engs:
            e.learn_msgs()
        what = f"{system} B={B} linearize it{it + 1}"
        same(engs[0], engs[1], what + " emitted Jacobian vs dual numbers")
        if ref is not None:
            against_oracle(engs[0], ref[it], what + " traced vs oracle", tol_policy=1e-8)
            against_oracle(engs[1], ref[it], what + " traced, dual numbers, vs oracle", tol_policy=1e-8)


def check_slope_parameter(lib, device):
    """Row b of a solve with per-trajectory parameters (slope, dt, u_max) equals the B = 1 solve of a model copy with those
    parameters, bit for bit on the lane family (the property check_parameters of tests/test_traced_model.py checks): the general
    sine sin(theta - slope) reads column b of the parameters."""
    from test_model_params_batch import OUTPUTS, outputs, param_rows, with_params

    model, B = traced("drag_pendulum"), 5
    rows = param_rows(model, B, 3)
    args, kws = problem("drag_pendulum", B)

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
    same_slope = rows.copy()
    same_slope[:, 0] = rows[0, 0]
    other = solve(model, kws["x0"], args[6], model_params=same_slope)
    assert not np.array_equal(out["K"][1], other["K"][1])  # (the slope alone moves the controllers)


def check_pointwise(lib, device, system):
    """dynamics and measure through a noise-free plant_step at B = 67 chosen points (the 64 + 3 of probe_util; for the hovercraft
    the last 5 of the 64 replaced by the points ON its kinks), observe through a noise-free rollout."""
    model, B = traced(system), 67
    base = points(model)
    kinks = kink_points(model, base)
    pts = np.vstack((base[:len(base) - len(kinks)], kinks, extra_points(model, base)))
    assert pts.shape == (B, model.dim_xu)
    bound = 16.0 * EPS * n_ops(model)
    eng = engine(model, system, B, lib, device, group_lanes=-1)
    as_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a.T), dtype=torch.float64, device=device)  # noqa: E731
    x, u = as_dev(pts[:, :model.dim_x]), as_dev(pts[:, model.dim_x:])
    y = eng.plant_step(x, u)
    x_new = np_(x).T
    dev = {"dynamics": deviation(x_new, model.dynamics(pts)), "measure": deviation(np_(y).T, model.measure(x_new))}
    eng.learn_msgs()
    r = eng.rollout(1, process_noise=False, want=("xu", "z"))
    xu = np_(r["xu"]).reshape(-1, model.dim_xu)
    dev["observe"] = deviation(np_(r["z"]).reshape(-1, model.dim_z), model.observe(xu))
    print(f"{system} on {device}: pointwise deviations {dev}, bound {bound:.3e}")
    for fn, d in dev.items():
        assert d <= bound, f"{system} {fn}: {d:.3e} > {bound:.3e}"


# ---- CPU: the host simulation ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import concurrent.futures

    lib = hostsim.load()
    models = [traced(s, j) for s in SYSTEMS for j in (True, False)]
    with concurrent.futures.ThreadPoolExecutor(2) as pool:
        assert all(i >= pkg._native.PLUGIN_BASE for i in pool.map(lambda m: m.resolve_model_id(lib), models))
    return lib


@pytest.fixture(scope="module")
def gpu_lib():
    return pkg.load_library()


GRID = [(s, B, f) for s in SYSTEMS for B in (5, 67) for f in ("lane", "quad", "group")]


@pytest.mark.parametrize("system,B,family", GRID)
def test_em_against_the_oracle_hostsim(lib, system, B, family):
    check_em(lib, "cpu", system, B, family)


@pytest.mark.parametrize("system", list(SYSTEMS))
@pytest.mark.parametrize("B", [5, 67])
def test_linearize_hostsim(lib, system, B):
    check_linearize(lib, "cpu", system, B)


def test_slope_parameter_hostsim(lib):
    check_slope_parameter(lib, "cpu")


@pytest.mark.parametrize("system", list(SYSTEMS))
def test_pointwise_hostsim(lib, system):
    check_pointwise(lib, "cpu", system)


# ---- MI355X ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_libraries_of_build_are_found_gpu(gpu_lib):
    """Both models, with and without the emitted Jacobian, were traced, emitted and compiled by build(): tracing them again here
    names the same libraries, which exist and are not rebuilt by resolving the models (their files are older than this process)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("i2c_amd_build", os.path.join(os.path.dirname(PLUGINS), "..", "input-inference-for-control_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    for cls, kw in py_models_ops.BUILT:
        m = cls(**kw)
        m.emit()
        path = build.model_lib_path(m.hip_name)
        assert os.path.exists(path), f"{cls.__name__}{kw}: build() left no {os.path.basename(path)}"
        assert m.resolve_model_id(gpu_lib) >= pkg._native.PLUGIN_BASE
        assert os.stat(path).st_mtime < STARTED, f"{os.path.basename(path)} was compiled by this test run"


@pytest.mark.gpu
@pytest.mark.parametrize("system,B,family", GRID)
def test_em_against_the_oracle_gpu(gpu_lib, system, B, family):
    check_em(gpu_lib, "cuda", system, B, family)


@pytest.mark.gpu
@pytest.mark.parametrize("system", list(SYSTEMS))
@pytest.mark.parametrize("B", [5, 67])
def test_linearize_gpu(gpu_lib, system, B):
    check_linearize(gpu_lib, "cuda", system, B)


@pytest.mark.gpu
def test_slope_parameter_gpu(gpu_lib):
    check_slope_parameter(gpu_lib, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("system", list(SYSTEMS))
def test_pointwise_gpu(gpu_lib, system):
    check_pointwise(gpu_lib, "cuda", system)
