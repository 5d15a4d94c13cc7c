"""The static figures of profiles/traced_models_ops.txt (no GPU needed):  python tools/traced_models_ops_report.py

For the two models of the extended operation set (tests/plugins/py_models_ops.py) beside PyPendulum and PyCartpole: VGPRs, AGPRs
and scratch of the lane forward sweep, the lane backward walk, the quad forward sweep and the propagation kernel of the fp64
translation unit (hipcc -Rpass-analysis=kernel-resource-usage on the emitted header, compiled as build.py --model does); every
kernel of an extended model that uses scratch; the opcode-class histogram of the lane forward time loop of PyDragPendulum beside
PyPendulum (tools/isa_histogram.py) with its branch count; the instruction counts of r_sqrt and r_tanh (a kernel of one call)."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "input-inference-for-control_amd")
sys.path[:0] = [ROOT, PKG_DIR, os.path.join(ROOT, "tests", "plugins"), os.path.join(ROOT, "tools")]
import isa_histogram  # noqa: E402

KERNELS = (("lane forward", r"^k_forward<M, double, true, false, double>"), ("lane backward walk", r"^k_chunk_walk<M, double"),
           ("quad forward", r"^k_quad_forward<M, double"), ("propagation", r"^k_propagate<M, double"))


def compile_unit(build, m, d):
    """-> (resource remarks {kernel: (VGPRs, AGPRs, scratch)}, assembly lines) of the model's fp64 translation unit."""
    obj, src, defs = build.model_tus(m.hip_struct, m.hip_name, [f'-DI2C_TU_HEADER="{m.hip_header}"'])[0]
    cmd = [build.HIPCC] + build.FLAGS + defs + ["-Rpass-analysis=kernel-resource-usage", "-save-temps=obj", "-c",
                                                os.path.join(build.CSRC, src), "-o", os.path.join(d, obj)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        f = re.search(r"Function Name: (\S+)", line)
        if f:
            cur = f.group(1)
            out[cur] = {}
        for key, pat in (("v", r"\bVGPRs: (\d+)"), ("a", r"\bAGPRs: (\d+)"), ("s", r"ScratchSize \[bytes/lane\]: (\d+)")):
            f = re.search(pat, line)
            if f and cur:
                out[cur][key] = int(f.group(1))
    names = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True).stdout.splitlines()
    res = {}
    for mangled, plain in zip(out, names):
        plain = re.sub(r"\bi2c::", "", re.sub(r"^void ", "", plain)).replace(m.hip_struct, "M")
        res[plain] = (mangled, out[mangled].get("v", -1), out[mangled].get("a", -1), out[mangled].get("s", -1))
    asm = next(f for f in os.listdir(d) if f.endswith("gfx950.s"))
    return res, open(os.path.join(d, asm)).read().split("\n")


def routine_counts():
    src = """#include "i2c_linalg.hpp"
extern "C" __global__ void one_sqrt(const double* x, double* y) { y[threadIdx.x] = i2c::r_sqrt(x[threadIdx.x]); }
extern "C" __global__ void one_tanh(const double* x, double* y) { y[threadIdx.x] = i2c::r_tanh(x[threadIdx.x]); }
extern "C" __global__ void one_copy(const double* x, double* y) { y[threadIdx.x] = x[threadIdx.x]; }
"""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "one.hip"), "w") as f:
            f.write(src)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(PKG_DIR, "csrc"), "-S",
                        "--cuda-device-only", "one.hip", "-o", "one.s"], check=True, capture_output=True, cwd=d)
        lines = open(os.path.join(d, "one.s")).read().split("\n")
    count = {}
    for k in ("one_sqrt", "one_tanh", "one_copy"):
        start = next(i for i, l in enumerate(lines) if l.startswith(f"{k}:"))
        body = [l.strip() for l in lines[start + 1: next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])]]
        body = [l for l in body if l and not l.startswith((";", ".")) and not l.endswith(":")]
        count[k] = (len(body), sum(1 for l in body if re.match(r"v_\w+_f64", l)), sum(1 for l in body if l.startswith(("s_cbranch", "s_branch"))),
                    sum(1 for l in body if re.match(r"v_(rsq|rcp)_f64", l)))
    base = count["one_copy"][0]
    for k, name in (("one_sqrt", "r_sqrt"), ("one_tanh", "r_tanh")):
        n, f64, br, seeds = count[k]
        print(f"  {name}: {n - base} instructions beyond the load / store shell ({f64} fp64 vector instructions, {seeds} seed "
              f"instruction(s) v_rsq_f64 / v_rcp_f64, {br} branches)")


def main():
    spec = importlib.util.spec_from_file_location("i2c_amd_build", os.path.join(PKG_DIR, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    import py_models
    import py_models_ops

    models = [py_models.PyPendulum(), py_models_ops.PyDragPendulum(), py_models.PyCartpole(), py_models_ops.PyHovercraft()]
    units = {}
    print("static resources, fp64 unit, gfx950 (VGPRs, AGPRs, scratch bytes per lane)")
    with tempfile.TemporaryDirectory() as top:
        for m in models:
            m.emit()
            d = os.path.join(top, m.hip_name)
            os.makedirs(d)
            units[type(m).__name__] = compile_unit(build, m, d)
    for label, pat in KERNELS:
        for name, (res, _) in units.items():
            hits = sorted(k for k in res if re.search(pat, k))
            for k in hits[:1]:
                print(f"  {label:20s} {name:16s} {str(res[k][1:]):16s} {k[:100]}")
    for name in ("PyDragPendulum", "PyHovercraft"):
        base = units["PyPendulum" if name == "PyDragPendulum" else "PyCartpole"][0]
        res = units[name][0]
        spills = sorted(k for k, v in res.items() if v[3] > 0)
        new = [k for k in spills if base.get(k, (0, 0, 0, 0))[3] == 0]
        print(f"  {name}: {len(res)} kernels, {len(spills)} with scratch; with scratch where "
              f"{'PyPendulum' if name == 'PyDragPendulum' else 'PyCartpole'} has none: " + ("none" if not new else ""))
        for k in new:
            print(f"    {res[k][1:]}  {k[:140]}")
    print("\nlane forward time loop, opcode classes (tools/isa_histogram.py)")
    for name in ("PyPendulum", "PyDragPendulum"):
        res, lines = units[name]
        k = sorted(k for k in res if re.search(KERNELS[0][1], k))[0]
        print(f"-- {name}")
        isa_histogram.histogram(lines, re.escape(res[k][0][2:]))
    print("\nthe routines alone")
    routine_counts()


if __name__ == "__main__":
    main()
