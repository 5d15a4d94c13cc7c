"""The figures of profiles/traced_models.txt that need no GPU:
python tools/traced_models_report.py [pointwise] [resources]

pointwise  the measured bound of tests/test_functor_codegen.py for every system: delta_hand (the hand-written functor against its
           NumPy twin), the traced functor's deviation from its NumPy side, the emitted Jacobian against the dual-number path
resources  VGPRs, AGPRs and scratch per kernel of the fp64 translation unit of PyCartpole beside the in-tree Cartpole's, from
           hipcc -Rpass-analysis=kernel-resource-usage (through the I2C_HIPCC_EXTRA hook of build.py), and the kernels where the
           generated functor uses scratch and the hand-written one does not"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "input-inference-for-control_amd")
sys.path[:0] = [ROOT, PKG_DIR, os.path.join(ROOT, "tests", "plugins")]


def pointwise():
    import probe_util as t

    with tempfile.TemporaryDirectory() as d:
        res = t.probe_all(d)
    print(f"pointwise, 64 points inside xu_lim; deviation = largest over output columns of max |a - b| / max |b|; eps = {t.EPS:.3e}")
    for name, r in res.items():
        delta, traced, jac = t.figures(r)
        print(f"  {name:16s} delta_hand {delta:.3e}  bound 4 delta_hand + 4 eps {4 * delta + 4 * t.EPS:.3e}  traced values "
              + " ".join(f"{k} {v:.3e}" for k, v in traced.items()) + "  emitted Jacobian vs dual numbers "
              + " ".join(f"{k} {v:.3e}" for k, v in jac.items()) + f"  (trace + emit, twice: {r['seconds']:.2f} s)")


def resource_usage(build, struct, name, header=None):
    """{kernel name with the model's struct replaced by M: (VGPRs, AGPRs, scratch bytes per lane)} of the model's f64 unit."""
    obj, src, defs = build.model_tus(struct, name, [f'-DI2C_TU_HEADER="{header}"'] if header else [])[0]
    with tempfile.TemporaryDirectory() as d:
        cmd = [build.HIPCC] + build.FLAGS + defs + ["-c", os.path.join(build.CSRC, src), "-o", os.path.join(d, obj)]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
        for key, pat in (("v", r"\bVGPRs: (\d+)"), ("a", r"\bAGPRs: (\d+)"), ("s", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                out[cur][key] = int(m.group(1))
    names = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True).stdout.splitlines()
    res = {}
    for mangled, plain in zip(out, names):
        plain = re.sub(r"\bi2c::", "", plain.split("(")[0]).replace(struct, "M")
        res[plain] = (out[mangled].get("v", -1), out[mangled].get("a", -1), out[mangled].get("s", -1))
    return res


def resources():
    os.environ["I2C_HIPCC_EXTRA"] = (os.environ.get("I2C_HIPCC_EXTRA", "") + " -Rpass-analysis=kernel-resource-usage").strip()
    spec = importlib.util.spec_from_file_location("i2c_amd_build", os.path.join(PKG_DIR, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    import py_models

    m = py_models.PyCartpole()
    m.emit()
    hand = resource_usage(build, "Cartpole", "cartpole")
    traced = resource_usage(build, m.hip_struct, m.hip_name, m.hip_header)
    print(f"static resources, fp64 unit, gfx950: hand-written Cartpole | generated {m.hip_struct}   (VGPRs AGPRs scratch bytes/lane)")
    worse = []
    for k in sorted(set(hand) | set(traced)):
        h, t = hand.get(k), traced.get(k)
        print(f"  {k[:110]:110s} {str(h):18s} | {t}")
        if h and t and t[2] > 0 and h[2] == 0:
            worse.append(k)
    print(f"kernels where the generated functor uses scratch and the hand-written one does not: {worse or 'none'}")
    return worse


if __name__ == "__main__":
    what = sys.argv[1:] or ["pointwise", "resources"]
    if "pointwise" in what:
        pointwise()
    if "resources" in what:
        resources()
