"""The scalar routines a model functor may call beyond + - * / (csrc/i2c_linalg.hpp: r_sqrt, r_tanh, r_abs, r_min, r_max,
r_where_gt) and their dual-number overloads (csrc/i2c_linearize.hpp), in a stand-alone host program
(tests/plugins/device_math_probe.cpp, g++ -DI2C_HOST_SIM with AddressSanitizer and UBSan linked in; its own main, no preload):
the host simulation runs the formulas of the device, only the seed instructions are emulated.

Truth: mpmath at 50 digits. Bounds, fixed before anything was measured:
  * r_sqrt: 2 ulp, the figure csrc/i2c_linalg.hpp states for its scalar routines;
  * r_tanh: the largest RELATIVE error of glibc's std::tanh on the same arguments, measured by the same program, plus one ulp
    (2^-52, the EPS of tests/plugins/probe_util.py) -- what a branch-free routine may trade.
Measured (printed by the tests): r_sqrt 0.50 ulp; r_tanh 2.73e-16 relative beside glibc's 2.29e-16, bound 4.51e-16."""
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGINS = os.path.join(ROOT, "tests", "plugins")
CSRC = os.path.join(ROOT, "input-inference-for-control_amd", "csrc")
EPS = 2.0 ** -52
TINY = 2.0 ** -1022  # the smallest normal double
INF, NAN = math.inf, math.nan

mpmath.mp.dps = 50


def sqrt_args():
    rng = np.random.default_rng(11)
    pts = [TINY, math.nextafter(TINY, 1.0), math.nextafter(math.nextafter(TINY, 1.0), 1.0)]  # next to the subnormals
    pts += [2.0 ** k for k in range(-1021, 1024)]
    pts += list(10.0 ** rng.uniform(-300.0, 300.0, 4096))
    return [float(p) for p in pts]


def tanh_args():
    rng = np.random.default_rng(12)
    pts = [s * 2.0 ** -k for k in range(0, 61) for s in (1.0, -1.0)]
    pts += list(rng.uniform(-25.0, 25.0, 4096))
    return [float(p) for p in pts]


TANH_EXTRA = [40.0, -40.0, 700.0, -700.0, 20.0, -20.0, 0.0, -0.0, 5e-324, -5e-324, INF, -INF]
SQRT_SPECIAL = [0.0, -0.0, INF, -1.0, -TINY, -INF, NAN, 5e-324, 1e-310, 2.0 ** -1030]
# (a v d), (M av ad bv bd), (W a b xv xd yv yd), (L v d), (C v d), (G g d): the kinks, at and beside them
KINKS = [("A", 0.0, 3.0), ("A", -0.0, 3.0), ("A", 5e-324, 3.0), ("A", -5e-324, 3.0), ("A", 2.5, 3.0), ("A", -2.5, 3.0),
         ("M", 1.0, 3.0, 1.0, 5.0), ("M", 1.0, 3.0, math.nextafter(1.0, 2.0), 5.0), ("M", 1.0, 3.0, math.nextafter(1.0, 0.0), 5.0),
         ("W", 0.0, 0.0, 2.0, 3.0, 4.0, 5.0), ("W", 5e-324, 0.0, 2.0, 3.0, 4.0, 5.0), ("W", -5e-324, 0.0, 2.0, 3.0, 4.0, 5.0),
         ("L", 2.0, 3.0), ("C", 0.5, 3.0), ("G", INF, 0.0), ("G", INF, 2.0), ("G", NAN, 0.0), ("G", 3.0, -2.0)]


def fmt(v):
    return "nan" if v != v else float(v).hex()


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    """The program compiled and run ONCE on every argument of this file: {tag: [rows of floats]} in request order."""
    out_dir = str(tmp_path_factory.mktemp("math_probe"))
    exe = os.path.join(out_dir, "device_math_probe")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DI2C_HOST_SIM", "-I", CSRC, os.path.join(PLUGINS, "device_math_probe.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    lines = [f"S {fmt(x)}" for x in sqrt_args() + SQRT_SPECIAL] + [f"T {fmt(x)}" for x in tanh_args() + TANH_EXTRA + [NAN]]
    lines += [" ".join([k[0]] + [fmt(v) for v in k[1:]]) for k in KINKS]
    with open(exe + ".in", "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, exe + ".in"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]  # (a sanitizer report goes to stderr)
    out = {}
    for line in r.stdout.splitlines():
        tok = line.split()
        out.setdefault(tok[0], []).append([float.fromhex(v) if "nan" not in v else NAN for v in tok[1:]])
    assert len(r.stdout.splitlines()) == len(lines)
    return out


def ulp_of(v):
    return math.ulp(abs(float(v)))


def test_sqrt_within_two_ulp(probed):
    args = sqrt_args()
    rows = probed["S"][:len(args)]
    worst = worst_d = 0.0
    for x, (s, d1, d0, dr0) in zip(args, rows):
        truth = mpmath.sqrt(mpmath.mpf(x))
        worst = max(worst, float(abs(mpmath.mpf(s) - truth) / ulp_of(truth)))
        assert s >= 0.0 and d0 == 0.0 and dr0 == 0.0
        dt = 1 / (2 * truth)
        if 1e-290 < x < 1e290:  # (the derivative's own range: rsqrt(x) / 2 stays a normal double throughout)
            worst_d = max(worst_d, float(abs(mpmath.mpf(d1) - dt) / ulp_of(dt)))
    print(f"r_sqrt: {worst:.3f} ulp at most over {len(args)} arguments; d r_sqrt: {worst_d:.3f} ulp")
    assert worst <= 2.0
    assert worst_d <= 2.0  # (rsqrt: one of the scalar routines of that figure; the halving is exact)


def test_sqrt_exact_cases(probed):
    rows = dict(zip([fmt(x) for x in SQRT_SPECIAL], probed["S"][len(sqrt_args()):]))
    zero, mzero = rows[fmt(0.0)], rows[fmt(-0.0)]
    assert zero[0] == 0.0 and math.copysign(1.0, zero[0]) == 1.0 and mzero[0] == 0.0 and math.copysign(1.0, mzero[0]) == -1.0
    assert rows[fmt(INF)][0] == INF
    for x in (-1.0, -TINY, -INF, NAN):
        assert rows[fmt(x)][0] != rows[fmt(x)][0], x
    # sqrt' at 0: a zero tangent stays exactly 0 (sqrt and rsqrt alike), a non-zero one is +inf
    assert zero[1] == INF and zero[2] == 0.0 and zero[3] == 0.0 and math.copysign(1.0, zero[2]) == 1.0
    # subnormal arguments: finite and non-negative, within the 2^-26 the routine's comment states
    for x in (5e-324, 1e-310, 2.0 ** -1030):
        s = rows[fmt(x)][0]
        assert 0.0 < s < INF and abs(s - math.sqrt(x)) <= 2.0 ** -26 * math.sqrt(x), (x, s)


def test_tanh_within_glibc_plus_one_ulp(probed):
    args = tanh_args()
    rows = probed["T"][:len(args)]
    mine = libm = worst_d = 0.0
    for x, (t, g, d) in zip(args, rows):
        truth = mpmath.tanh(mpmath.mpf(x))
        mine = max(mine, float(abs(mpmath.mpf(t) - truth) / abs(truth)))
        libm = max(libm, float(abs(mpmath.mpf(g) - truth) / abs(truth)))
        dt = 1 - truth * truth
        if abs(x) <= 4.0:  # (1 - t^2 cancels as t -> 1: beyond, the absolute error is what is small)
            worst_d = max(worst_d, float(abs(mpmath.mpf(d) - dt) / dt))
        assert abs(d - float(dt)) <= 8.0 * EPS
    bound = libm + EPS
    print(f"r_tanh: {mine:.3e} relative at most over {len(args)} arguments; glibc {libm:.3e}; bound {bound:.3e}; "
          f"d r_tanh {worst_d:.3e} relative on |x| <= 4")
    assert mine <= bound


def test_tanh_exact_cases(probed):
    args = tanh_args() + TANH_EXTRA
    rows = probed["T"]
    assert len(rows) == len(args) + 1 and rows[-1][0] != rows[-1][0] and rows[-1][2] != rows[-1][2]  # NaN in, NaN out
    got = {}
    for x, (t, _, d) in zip(args, rows):
        assert abs(t) <= 1.0 and math.copysign(1.0, t) == math.copysign(1.0, x), x
        got[fmt(x)] = t
        if abs(x) >= 20.0:
            assert abs(t) == 1.0 and d == 0.0, x
    for x in args:  # odd to the bit
        if fmt(-x) in got:
            assert got[fmt(-x)] == -got[fmt(x)] and math.copysign(1.0, got[fmt(-x)]) == -math.copysign(1.0, got[fmt(x)]), x
    assert got[fmt(5e-324)] == 5e-324 and got[fmt(0.0)] == 0.0 and got[fmt(2.0 ** -60)] == 2.0 ** -60


def test_derivative_conventions_at_the_kinks(probed):
    a = probed["A"]  # value, tangent, sign: 0 at +-0, +-3 beside it (the smallest subnormal included)
    assert [r[1] for r in a] == [0.0, 0.0, 3.0, -3.0, 3.0, -3.0] and [r[2] for r in a] == [0.0, 0.0, 1.0, -1.0, 1.0, -1.0]
    assert [r[0] for r in a] == [0.0, 0.0, 5e-324, 5e-324, 2.5, 2.5]
    up, down = math.nextafter(1.0, 2.0), math.nextafter(1.0, 0.0)
    m = probed["M"]  # max value, tangent, min value, tangent, plain max, plain min: a = (1, 3), b = (1 | 1+ | 1-, 5)
    assert m[0] == [1.0, 3.0, 1.0, 3.0, 1.0, 1.0]       # a tie: the first argument's derivative, in both
    assert m[1] == [up, 5.0, 1.0, 3.0, up, 1.0]
    assert m[2] == [1.0, 3.0, down, 5.0, 1.0, down]
    w = probed["W"]  # where_gt(a, 0, (2, 3), (4, 5)) at a = 0, +tiny, -tiny: the selected branch, nothing of a's or b's tangents
    assert w == [[4.0, 5.0, 4.0], [2.0, 3.0, 2.0], [4.0, 5.0, 4.0]]
    (lv, ld), = probed["L"]
    assert abs(lv - math.log(2.0)) <= 2 * math.ulp(lv) and abs(ld - 1.5) <= 2 * math.ulp(1.5)
    (sv, sd, cv, cd), = probed["C"]
    assert abs(sv - math.sin(0.5)) <= math.ulp(sv) and abs(cv - math.cos(0.5)) <= math.ulp(cv) and sd == 3.0 * cv and cd == -3.0 * sv
    g = [r[0] for r in probed["G"]]
    assert g[0] == 0.0 and g[1] == INF and g[2] == 0.0 and g[3] == -6.0
