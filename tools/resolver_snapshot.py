"""The resolver as a whole, pinned: every answer of i2c_backward_schedule and i2c_kernel_family (the six I2C_SWEEP_* values) over a
grid of problems, asked through the C ABI with scalar fields only (as _shape() of tests/test_abi.py: no buffer exists; the three
pointers the resolver tests for null-ness get a dummy address) and kept as int8 tables in tests/golden/resolver_abi9.npz.
    python tools/resolver_snapshot.py                  compare the library's answers with the fixture (exit status 1 on a mismatch)
    python tools/resolver_snapshot.py --write          write the fixture
    python tools/resolver_snapshot.py --lib PATH       ask this library (default: the host simulation, tests/hostsim.py)
The tables (each [..., 7]: the schedule, then the family of sweep 0 .. 5):
    main     [model, dtype, inference, group_lanes, backward_mode, post_layout, rule, T, B]
    params   the same axes for the models with parameters, I2cProblem.model_params_b set
    edge     [model, dtype, inference, group_lanes, backward_mode, post_layout, rule, B]: T = 50, the two batch sizes either side of
             every 2 GiB bound of the model (elements per cell x B x 4 or 8 bytes, from I2cDims)
    window   [model, dtype, inference, group_lanes, backward_mode, post_layout, rule, flags, (B, T)]: per-cell targets / temperatures
             (z_per_cell with a non-null z, alpha_cell, both) inside and beyond the 4 GiB window of the multi-lane kernels
tests/test_resolver_snapshot.py compares them entry for entry, on the host simulation and on the device library."""
import ctypes
import importlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "input-inference-for-control_amd")]
pkg = importlib.import_module("input-inference-for-control_amd")
N = pkg._native

FIXTURE = os.path.join(ROOT, "tests", "golden", "resolver_abi9.npz")
MODELS = sorted(N.MODEL_IDS.values())
DTYPES = [N.F64, N.F32, N.F64_F32S]
INFERENCES = [N.INF_CUBATURE, N.INF_LINEARIZE, N.INF_GAUSS_HERMITE]
MODES = [N.BWD_AUTO, N.BWD_TWO_PASS, N.BWD_FUSED, N.BWD_CHUNKED]
LAYOUTS = [0, 1]
RULES = [(1.0, 0.0, 0.0), (1.2, 0.44, 0.5)]  # CubatureQuadrature(alpha, beta, kappa): the unit rule and general weights
HORIZONS = [5, 8, 50]
# both sides of every batch window of csrc/i2c_models.hpp and of I2C_BWD_FUSED_MIN_B
BATCHES = [1, 4, 63, 64, 65, 128, 129, 256, 257, 384, 385, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 12287, 12288, 20479, 20480,
           32768, 262144]
EDGE_T = 50
WINDOW_FLAGS = [(1, 0), (0, 1), (1, 1)]  # (z_per_cell with z, alpha_cell)
WINDOW_SHAPES = [(4096, 50), (262144, 8192)]  # (B, T): T B sizeof = 2^33 / 2^34 bytes at the second one
N_ANSWERS = 7
DUMMY = 64  # the address the null-tested pointers get: never dereferenced by the resolvers


def lanes_of(d):
    """The group_lanes requests asked of a model: default, one lane, its group width (4 where it has none), the wave / quad / grid
    request, I2C_LANES_QUAD, and a width nobody supports."""
    return [0, -1, d.group_lanes or 4, 64, N.LANES_QUAD, 3]


def edge_batches(d):
    """The batch sizes either side of every 2 GiB bound of the model: the largest B with E B s < 2^31 and the next one, for the
    per-cell element counts E the resolver bounds (forward / posterior / propagation cells and the chunk composites) and both sizes s."""
    sym = lambda n: n * (n + 1) // 2  # noqa: E731
    counts = {max(d.e_fwd, d.e_post, d.e_prop), max(d.e_fwd, d.e_post), max(d.e_post, d.e_prop), d.nx + d.nx * d.nx + sym(d.nx)}
    out = set()
    for e, s in itertools.product(counts, (4, 8)):
        b = ((1 << 31) - 1) // (e * s)
        out |= {b, b + 1}
    return sorted(out)


class Asker:
    """One I2cProblem reused for every question (the struct is mutated in place: 3.6 million calls stay a few seconds)."""

    def __init__(self, lib):
        self.p = N.I2cProblem()
        self.p.abi_version, self.p.gh_degree = N.ABI_VERSION, 3
        self.ref = ctypes.byref(self.p)
        self.schedule, self.family = lib.i2c_backward_schedule, lib.i2c_kernel_family

    def set(self, **fields):
        for k, v in fields.items():
            setattr(self.p, k, v)

    def answers(self, out):
        """Appends the seven answers to the flat list `out` (the tables are filled in the order of their axes)."""
        out.append(self.schedule(self.ref))
        family, ref = self.family, self.ref
        out.extend([family(ref, 0), family(ref, 1), family(ref, 2), family(ref, 3), family(ref, 4), family(ref, 5)])


def _outer(lib, models):
    """Askers with the slow axes set, in the order model x dtype x inference x group_lanes x backward_mode x post_layout x rule."""
    a = Asker(lib)
    for mid in models:
        for dt, inf, gl, mode, lay, rule in itertools.product(DTYPES, INFERENCES, lanes_of(lib.query(mid)), MODES, LAYOUTS, RULES):
            a.set(model_id=mid, dtype=dt, inference=inf, group_lanes=gl, backward_mode=mode, post_layout=lay, quad_alpha=rule[0],
                  quad_beta=rule[1], quad_kappa=rule[2])
            yield a


def _table(flat, n_models, *inner):
    return np.array(flat, np.int8).reshape((n_models, len(DTYPES), len(INFERENCES), 6, len(MODES), len(LAYOUTS), len(RULES)) + inner + (N_ANSWERS,))


def _grid(lib, models, params_b):
    flat = []
    for a in _outer(lib, models):
        a.set(model_params_b=DUMMY if params_b else None)
        for T in HORIZONS:
            a.p.T = T
            for B in BATCHES:
                a.p.B = B
                a.answers(flat)
    return _table(flat, len(models), len(HORIZONS), len(BATCHES))


def _edge(lib, batches):
    flat = []
    for a in _outer(lib, MODELS):
        a.p.T = EDGE_T
        for B in batches[MODELS.index(a.p.model_id)]:
            a.p.B = int(B)
            a.answers(flat)
    return _table(flat, len(MODELS), batches.shape[1])


def _window(lib):
    flat = []
    for a in _outer(lib, MODELS):
        for (zc, ac), (B, T) in itertools.product(WINDOW_FLAGS, WINDOW_SHAPES):
            a.set(B=B, T=T, z_per_cell=zc, z=DUMMY if zc else None, alpha_cell=DUMMY if ac else None)
            a.answers(flat)
    return _table(flat, len(MODELS), len(WINDOW_FLAGS), len(WINDOW_SHAPES))


def snapshot(lib):
    """{name: array}: the four tables and the values of their axes."""
    dims = [lib.query(m) for m in MODELS]
    with_params = [m for m, d in zip(MODELS, dims) if d.n_params > 0]
    edges = [edge_batches(d) for d in dims]
    assert len({len(e) for e in edges}) == 1, edges  # (distinct bounds per model: one row length)
    edge_b = np.array(edges, np.int64)
    return dict(
        main=_grid(lib, MODELS, False), params=_grid(lib, with_params, True), edge=_edge(lib, edge_b), window=_window(lib),
        models=np.array(MODELS), models_with_params=np.array(with_params), dtypes=np.array(DTYPES), inferences=np.array(INFERENCES),
        group_lanes=np.array([lanes_of(d) for d in dims]), backward_modes=np.array(MODES), post_layouts=np.array(LAYOUTS),
        rules=np.array(RULES), horizons=np.array(HORIZONS), batches=np.array(BATCHES), edge_batches=edge_b,
        window_flags=np.array(WINDOW_FLAGS), window_shapes=np.array(WINDOW_SHAPES))


ANSWER_NAMES = ["schedule", "forward", "backward", "propagate", "filter", "chunk_passes", "chunk_stitch"]


def describe(name, got, index):
    """The problem behind entry `index` of table `name`, field by field."""
    im, idt, ii, il, imo, ip, ir = index[:7]
    models = got["models_with_params"] if name == "params" else got["models"]
    f = dict(model_id=int(models[im]), dtype=int(got["dtypes"][idt]), inference=int(got["inferences"][ii]),
             group_lanes=int(got["group_lanes"][list(got["models"]).index(models[im])][il]), backward_mode=int(got["backward_modes"][imo]),
             post_layout=int(got["post_layouts"][ip]), rule=tuple(got["rules"][ir]))
    if name in ("main", "params"):
        f.update(T=int(got["horizons"][index[7]]), B=int(got["batches"][index[8]]), model_params_b=name == "params")
    elif name == "edge":
        f.update(T=EDGE_T, B=int(got["edge_batches"][im][index[7]]))
    else:
        zc, ac = got["window_flags"][index[7]]
        B, T = got["window_shapes"][index[8]]
        f.update(T=int(T), B=int(B), z_per_cell=int(zc), alpha_cell=bool(ac))
    return f"{ANSWER_NAMES[index[-1]]} of {f}"


def differences(want, got, limit=20):
    """[str]: the first `limit` differing entries (axes first: a grid that moved is reported as such)."""
    out = []
    for name in sorted(set(want) | set(got)):
        if name not in want or name not in got or want[name].shape != got[name].shape:
            out.append(f"{name}: table missing or of another shape")
        elif name not in ("main", "params", "edge", "window") and not np.array_equal(want[name], got[name]):
            out.append(f"{name}: axis values differ: fixture {want[name].tolist()} library {got[name].tolist()}")
    if out:
        return out
    for name in ("main", "params", "edge", "window"):
        bad = np.argwhere(want[name] != got[name])
        for index in bad[:max(0, limit - len(out))]:
            index = tuple(int(i) for i in index)
            out.append(f"{name}: {describe(name, got, index)}: fixture {int(want[name][index])}, library {int(got[name][index])}")
        if len(bad) > limit:
            out.append(f"{name}: ... {len(bad)} entries differ")
    return out


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def main(argv):
    if "--lib" in argv:
        lib = pkg.load_library(argv[argv.index("--lib") + 1])
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        lib = importlib.import_module("hostsim").load()
    got = snapshot(lib)
    n = sum(got[k].size for k in ("main", "params", "edge", "window"))
    if "--write" in argv:
        np.savez_compressed(FIXTURE, **got)
        print(f"{FIXTURE}: {n} answers of {lib.path} ({os.path.getsize(FIXTURE)} bytes)")
        return 0
    diff = differences(load_fixture(), got)
    print("\n".join(diff) if diff else f"{n} answers of {lib.path} equal {FIXTURE}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
