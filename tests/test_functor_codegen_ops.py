"""The wider operation set of models written in Python (`operations = "extended"`: functor_codegen.py, i2c/traced_model.py,
tests/plugins/py_models_ops.py), without the solver: what is traced as an angle coordinate and what as a general sine, the hints
and knobs, what is accepted only in extended mode and what in neither, that basic models emit the text they emitted before the
wider set existed, and the generated code evaluated pointwise in the stand-alone host program of tests/test_functor_codegen.py
(tests/plugins/functor_probe.cpp; g++ -DI2C_HOST_SIM with AddressSanitizer and UBSan linked in, its own main, no preload).

Pointwise bound, derived: every scalar routine is within 2 ulp (csrc/i2c_linalg.hpp; tests/test_device_math_ops.py), NumPy's
within 1, so one operation moves the two sides apart by at most 4 eps relative to the output's scale (eps = 2^-52, the deviation
being per column max |a - b| / max |b|), and the error accumulates linearly at worst: 4 eps n_ops, n_ops the operation count of
the model's longest output (sympy.count_ops of the traced expression: 23 for PyDragPendulum, 20 for PyHovercraft, so 2.0e-14 and
1.8e-14; measured: 1.5e-16 and 1.6e-16 on the values, 1.9e-16 and 2.2e-16 between the two Jacobians). The emitted Jacobian is held to the dual-number path under the same figure, kink points included, and to central
differences at the 1e-7 of tests/test_functor_codegen.py away from the kinks."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

pkg = importlib.import_module("input-inference-for-control_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGINS = os.path.join(ROOT, "tests", "plugins")
if PLUGINS not in sys.path:
    sys.path.insert(0, PLUGINS)
import py_models  # noqa: E402
import py_models_ops  # noqa: E402
from probe_util import EPS, N_POINTS, compile_probe, deviation, emit_pair, extra_points, points, run_probe  # noqa: E402
from i2c.known_models import KnownModel  # noqa: E402
from i2c.traced_model import NumpyMath, TracedModel  # noqa: E402

MODELS = {"drag_pendulum": py_models_ops.PyDragPendulum, "hovercraft": py_models_ops.PyHovercraft}
# struct names (hashes of the emitted text) of py_models.BUILT and of the double cartpole on the commit before the wider set
BASIC_STRUCTS = {("PyPendulum", True): "PyPendulum_f5853c6d9a71", ("PyPendulum", False): "PyPendulum_b0c0ab2d1138",
                 ("PyVanDerPol", True): "PyVanDerPol_434d4ba3619a", ("PyVanDerPol", False): "PyVanDerPol_439a103f2180",
                 ("PyCartpole", True): "PyCartpole_386e8b9fa784", ("PyCartpole", False): "PyCartpole_88a1e71340e5"}
DOUBLE_CARTPOLE_STRUCT = "PyDoubleCartpole_6e3bd67bc649"


def kink_points(model, pts):
    """PyHovercraft: points exactly ON each kink -- vx = 0 (where_gt), vy = 0 (abs), ux = -u_max (maximum), uy = u_max
    (minimum), and all of them at once. (Other models: none.)"""
    if not isinstance(model, py_models_ops.PyHovercraft):
        return pts[:0]
    out = pts[:5].copy()
    out[0, 2] = 0.0
    out[1, 3] = 0.0
    out[2, 4] = -model.U_MAX
    out[3, 5] = model.U_MAX
    out[4, 2:] = [0.0, 0.0, -model.U_MAX, model.U_MAX]
    return out


def n_ops(model):
    cg, spec = model.trace()
    import sympy

    return max(int(sympy.count_ops(e)) for fn in cg.FUNCTIONS for e in spec.exprs[fn])


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    """Both models emitted (with and without the jacobian member), compiled and run once on the 64 + 3 points of probe_util and
    the kink points: {name: {"model", "out": probe output over all points, "pts", "n_away": the points away from kinks}}."""
    import concurrent.futures

    out_dir = str(tmp_path_factory.mktemp("probe_ops"))
    res, jobs = {}, {}
    with concurrent.futures.ThreadPoolExecutor(2) as pool:
        for name, cls in MODELS.items():
            model, path, dual = emit_pair(cls, out_dir)
            res[name] = {"model": model, "header": path}
            jobs[name] = pool.submit(compile_probe, out_dir, name, model.hip_struct, path, dual)
        for name, job in jobs.items():
            r = res[name]
            base = points(r["model"])
            r["pts"] = np.vstack((base, extra_points(r["model"], base), kink_points(r["model"], base)))
            r["out"] = run_probe(job.result(), r["model"].device_params(), r["pts"])
    return res


# ---- tracing ---------------------------------------------------------------------------------------------------------------------
def test_angle_coordinate_and_general_sine():
    m = py_models_ops.PyDragPendulum()
    cg, spec = m.trace()
    assert spec.extended and spec.angles == [0] and len(spec.general_sines) == 1
    assert spec.general_sines[0].free_symbols == {spec.xs[0], spec.ps[0]}  # theta - slope (up to sign)
    text = m.header_text()[2]
    assert 'operations = "extended"' in text.splitlines()[0] and "NA = 1" in text
    code = re.sub(r"//.*", "", text)
    # one call per function body that uses the general sine: dynamics, and the dynamics branch of jacobian<>; sine, cosine and the
    # derivative share the pair
    assert code.count("r_sincos(") == 2 and "std::" not in code and "pow(" not in code and "/" not in code
    assert py_models_ops.PyDragPendulum(jacobian=False).header_text()[2].count("r_sincos(") == 1
    cg2, spec2 = py_models_ops.PyHovercraft().trace()
    assert spec2.angles == [] and spec2.general_sines == []
    code2 = re.sub(r"//.*", "", py_models_ops.PyHovercraft().header_text()[2])
    assert "std::" not in code2 and "pow(" not in code2 and "/" not in code2 and "r_sincos(" not in code2
    for fn in ("r_sqrt(", "r_min(", "r_max(", "r_where_gt(", "r_abs(", "r_sign(", "r_tangent(", "r_sqrt_grad("):
        assert fn in code2, fn


def test_sines_of_products_parameters_and_actions_share_one_call_each():
    class Sines(py_models.PyVanDerPol):
        operations = "extended"

        def dynamics_fn(self, xu, p, m):
            a = xu[0] * xu[1]
            return [m.sin(a) + m.cos(a) + m.sin(2 * xu[0] + 0.25), m.sin(xu[2]) * m.cos(p[0] * xu[1]) + m.sin(m.sin(a))]

    cg, spec = Sines().trace()
    assert spec.angles == [0] and len(spec.general_sines) == 4  # x0 x1, u, mu x1 and the nested sin(x0 x1)
    text = Sines(jacobian=False).header_text()[2]
    dyn = text[text.index("void dynamics("):text.index("void observe(")]
    assert dyn.count("r_sincos(") == 4
    x = np.random.default_rng(1).normal(size=(7, 3))
    a = x[:, 0] * x[:, 1]
    np.testing.assert_allclose(Sines().dynamics(x)[:, 0], np.sin(a) + np.cos(a) + np.sin(2 * x[:, 0] + 0.25), rtol=1e-15)


@pytest.mark.parametrize("name,group", [("drag_pendulum", 4), ("hovercraft", 8)])
def test_hints_and_knobs(probed, name, group):
    model, hint = probed[name]["model"], probed[name]["out"]["HINT"]
    cg, spec = model.trace()
    assert cg.resolve_knobs(spec) == {"GROUP": group, "QUAD": True} and cg.quad_eligible(spec)
    assert hint["knobs"] == [group, 1, 0, 0, 1]
    if name == "drag_pendulum":
        assert hint["sizes"] == [2, 1, 4, 2, 3, 1, 2] and hint["ang"] == [0]
        assert hint["obs_lin"] == [-1, -1, -1, 2] and hint["obs_dep"][:3] == [0, 0, 1] and hint["term_lin"] == [0, 1]
    else:
        assert hint["sizes"] == [4, 2, 6, 4, 0, 0, 4] and hint["obs_lin"] == list(range(6)) and hint["term_lin"] == list(range(4))


# ---- what each mode accepts --------------------------------------------------------------------------------------------------------
def variant(operations, **fns):
    return type("Variant", (py_models.PyVanDerPol,), dict(fns, operations=operations))()


def test_half_integer_powers_and_abs():
    fn = dict(dynamics_fn=lambda self, xu, p, m: [xu[0] ** 0.5 + abs(xu[1]), (1.0 + xu[1] ** 2) ** -1.5 + m.sqrt(xu[0]) ** 3])
    text = variant("extended", **fn).header_text()[2]
    code = re.sub(r"//.*", "", text)
    assert "r_sqrt(x[0])" in code and "r_abs(x[1])" in code and "r_rsqrt(" in code and "pow(" not in code and "std::" not in code
    x = np.abs(np.random.default_rng(2).normal(size=(5, 3))) + 0.1
    ref = np.stack((np.sqrt(x[:, 0]) + np.abs(x[:, 1]), (1.0 + x[:, 1] ** 2) ** -1.5 + x[:, 0] ** 1.5), axis=-1)
    np.testing.assert_allclose(variant("extended", **fn).dynamics(x), ref, rtol=1e-15)
    # ... and basic mode refuses both with the messages it always had (a trailing hint names the attribute)
    with pytest.raises(ValueError, match=r"dynamics_fn: output 0: .*non-integer exponent.*operations = \"extended\""):
        variant("basic", dynamics_fn=lambda self, xu, p, m: [xu[0] ** 0.5, xu[1]]).trace()
    with pytest.raises(ValueError, match=r"observe_terminal_fn: output 1: 'Abs'.*operations = \"extended\""):
        variant("basic", observe_terminal_fn=lambda self, x, p, m: [x[0], abs(x[1])]).trace()
    with pytest.raises(ValueError, match=r"dynamics_fn: m\.sqrt is outside the operation set.*operations = \"extended\""):
        variant("basic", dynamics_fn=lambda self, xu, p, m: [m.sqrt(xu[0]), xu[1]]).trace()
    assert TracedModel.operations == "basic"
    with pytest.raises(ValueError, match=r"operations = 'everything'"):
        variant("everything").trace()


@pytest.mark.parametrize("operations", ["basic", "extended"])
def test_still_refused(operations):
    with pytest.raises(ValueError, match=r"dynamics_fn: m\.atan2 is outside the operation set"):
        variant(operations, dynamics_fn=lambda self, xu, p, m: [m.atan2(xu[0], xu[1]), xu[1]]).trace()
    with pytest.raises(ValueError, match=r"observe_fn: .*branch, comparison"):
        variant(operations, observe_fn=lambda self, xu, p, m: [xu[0] if xu[0] > 0 else -xu[0], xu[1], xu[1], xu[2]]).trace()
    with pytest.raises(ValueError, match=r"dynamics_fn: output 1: .*non-integer exponent"):
        variant(operations, dynamics_fn=lambda self, xu, p, m: [xu[0], xu[1] ** 0.3]).trace()
    with pytest.raises(ValueError, match=r"dynamics_fn: output 0: 'atan'"):
        import sympy

        variant(operations, dynamics_fn=lambda self, xu, p, m: [sympy.atan(xu[0]), xu[1]]).trace()


def test_basic_models_emit_the_text_they_always_did():
    for cls, kw in py_models.BUILT:
        assert cls(**kw).header_text()[1] == BASIC_STRUCTS[(cls.__name__, kw.get("jacobian", True))], (cls.__name__, kw)
    assert py_models.PyDoubleCartpole().header_text()[1] == DOUBLE_CARTPOLE_STRUCT


def test_numpy_side_takes_complex_points():
    m = py_models_ops.PyDragPendulum()
    x = np.array([[0.3, -0.7, 0.4]])
    h = 1e-30
    for f, n in ((m.dynamics, 3), (m.observe, 3)):
        for j in range(n):
            step = np.zeros(3)
            step[j] = 1.0
            d = np.imag(f(x + 1j * h * step)) / h
            ref = (f(x + 1e-6 * step) - f(x - 1e-6 * step)) / 2e-6
            np.testing.assert_allclose(d, ref, atol=1e-8)
    assert NumpyMath.where_gt(np.array([1.0, -1.0]), 0.0, 2.0, 3.0).tolist() == [2.0, 3.0]


# ---- pointwise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_values_against_the_numpy_side(probed, name):
    r = probed[name]
    model, pts, out = r["model"], r["pts"], r["out"]
    bound = 4.0 * EPS * n_ops(model)
    dev = {"dynamics": deviation(out["DYN"], model.dynamics(pts)), "observe": deviation(out["OBS"], model.observe(pts)),
           "observe_terminal": deviation(out["TERM"], model.observe_terminal(pts[:, :model.dim_x]))}
    print(f"{name}: {len(pts)} points, n_ops {n_ops(model)}, bound {bound:.3e}, values {dev}")
    for fn, d in dev.items():
        assert d <= bound, f"{name} {fn}: {d:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", list(MODELS))
def test_emitted_jacobian_against_dual_numbers(probed, name):
    r = probed[name]
    bound = 4.0 * EPS * n_ops(r["model"])
    dev = {i: deviation(r["out"][f"JA{i}"], r["out"][f"JD{i}"]) for i in range(3)}
    print(f"{name}: emitted Jacobian vs dual numbers over {len(r['pts'])} points (kinks included) {dev}, bound {bound:.3e}")
    for i, d in dev.items():
        assert d <= bound, f"{name} function {i}: {d:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", list(MODELS))
def test_jacobian_against_central_differences(probed, name):
    r = probed[name]
    model, pts = r["model"], r["pts"][:N_POINTS]  # (inside the limits and off every kink)
    fns = [(model.dynamics, model.dim_xu), (model.observe, model.dim_xu), (model.observe_terminal, model.dim_x)]
    for i, (f, n_in) in enumerate(fns):
        ref = np.array([KnownModel._jacobian(f, x[:n_in]).reshape(-1) for x in pts])
        err = np.max(np.abs(r["out"][f"JA{i}"][:N_POINTS] - ref)) / np.max(np.abs(ref))
        assert err < 1e-7, f"{name} function {i}: {err:.2e}"


def test_hovercraft_kinks(probed):
    """ON the kinks the conventions decide, identically in the emitted Jacobian and by dual numbers: abs' = 0 at vy = 0;
    where_gt(vx, 0, ...) takes the `else` branch at vx = 0; maximum(u, -u_max) and minimum(., u_max) take their first argument at
    a tie, so the thrust's derivative is still 1 ON either limit (and 0 beyond: the second of the 3 extra points)."""
    r = probed["hovercraft"]
    m, out = r["model"], r["out"]
    k = N_POINTS + 3
    ja, jd, x = out["JA0"][k:].reshape(5, 4, 6), out["JD0"][k:].reshape(5, 4, 6), r["pts"][k:]
    assert np.array_equal(ja[:, :, 4:], jd[:, :, 4:])
    speed = np.sqrt(x[:, 2] ** 2 + x[:, 3] ** 2 + m.EPS ** 2)
    # vx = 0: d ax / d vx = -DRAG speed - BACK (the else branch), exactly representable up to the products' rounding
    for q in (0, 4):
        assert abs(ja[q, 2, 2] - (1.0 + m.DT * (-m.DRAG * speed[q] - m.BACK))) <= 8 * EPS and abs(jd[q, 2, 2] - ja[q, 2, 2]) <= 8 * EPS
    # vy = 0: the keel term -KEEL |vy| vx contributes nothing to d ay / d vy (sign(0) = 0)
    for q in (1, 4):
        assert abs(ja[q, 3, 3] - (1.0 - m.DT * m.DRAG * speed[q])) <= 8 * EPS and abs(jd[q, 3, 3] - ja[q, 3, 3]) <= 8 * EPS
    assert ja[2, 2, 4] == m.DT and ja[3, 3, 5] == m.DT and ja[4, 2, 4] == m.DT and ja[4, 3, 5] == m.DT  # ON a limit: still 1
    beyond = out["JA0"][N_POINTS + 1].reshape(4, 6)
    assert np.all(beyond[:, 5] == 0.0) and np.all(out["JD0"][N_POINTS + 1].reshape(4, 6)[:, 5] == 0.0)
