"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/reference_dynamics_calls.npz by importing the REAL reference (/root/reference)
through oracle/ref_shim.py:   PYTHONDONTWRITEBYTECODE=1 python oracle/gen_reference_dynamics_golden.py

tests/test_jacobian_standin.py::test_standin_on_the_reference_dynamics differentiates the reference's own pendulum and double cartpole
dynamics (i2c/env_autograd.py) with the Jacobian stand-in. This records every call its check makes of those two functions
(input -> output, the complex-step inputs included) and the module-level pendulum Jacobian at its points, so that the test replays
them where the reference is not present. The file holds data only (inputs + the reference's outputs)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import ref_shim  # noqa: E402

ref_shim.install()

import numpy as np  # noqa: E402
import test_jacobian_standin as t  # noqa: E402
from i2c import env_autograd as ref  # noqa: E402  (the reference)

OUT = os.path.join(ROOT, "tests", "golden", "reference_dynamics_calls.npz")


def recorder(fun, tag, store):
    calls = []

    def f(x):
        y = np.asarray(fun(x))
        calls.append((np.array(x, copy=True), np.array(y, copy=True)))
        return y

    store[tag] = calls
    return f


def main():
    assert ref.__file__.startswith(ref_shim.REFERENCE_ROOT), ref.__file__
    store = {}
    t.check(recorder(ref.pendulum_dynamics, "pendulum", store), recorder(ref.double_cartpole_dynamics, "double_cartpole", store),
            "reference")
    out = {"pendulum_dydxu": np.asarray(ref.pendulum_dydxu(t.PEND_XU))}
    for tag, calls in store.items():
        out[tag + "_n"] = np.array(len(calls))
        for i, (x, y) in enumerate(calls):
            out[f"{tag}_x{i}"], out[f"{tag}_y{i}"] = x, y
    np.savez_compressed(OUT, **out)
    print(OUT, {tag: len(calls) for tag, calls in store.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
