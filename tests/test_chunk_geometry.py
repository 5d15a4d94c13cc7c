"""The chunked backward schedule (compose + stitch + walk + reduce) at every edge of its chunk geometry.

chunk_geometry() (csrc/i2c_impl.hpp) cuts a horizon of T cells into n chunks of `len` cells, the last one shorter. The golden
horizons only ever give last chunks of three cells or more, fewer than the 32 chunks the rule allows, and a chunk count that T / 4
limits. Here: a last chunk of ONE and of TWO cells (the walker's row prefetch and the compose pass's look-ahead load clamp at t_lo on
their first step), all 32 chunks, a chunk count that the batch limits, batches ragged against the four trajectories of a quad
wavefront and the 64 lanes of a lane wavefront at once, a workspace that is poisoned before every call and guarded behind its end,
a numeric failure in the first and in the lone last cell of a chunk, and the I2C_CHUNKS knob with one cell per chunk.

Every form of the schedule runs them: lane compose / stitch / walk (lean and full walker, double- and single-buffered), the same
three in the quad form, the default mixes of the two, the Linearize and the Gauss-Hermite form, fp32-stored messages. The
reference is the NumPy fp64 oracle on identical inputs (parity.check_batch_against_oracle), never another kernel -- except where a
comparison is ABOUT two runs of the same kernels (bit-identity) and for fp32-stored messages, whose bound the project states
against the same storage's fused walk (test_precision.py).

Shared bodies; test_hostsim_* run the host simulation of the kernel code on the CPU, test_hip_* the same bodies on the GPU."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import hostsim
import parity
from golden_util import load_case

N = parity.pkg._native
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the geometry, restated -------------------------------------------------------------------------------------------------
def geometry(B, T, forced=0):
    """(number of chunks, cells per chunk, cells in the last chunk) of a batch of B trajectories over T cells: enough chunks for
    ~64K lanes, at most 32, at least four cells per chunk; I2C_CHUNKS = forced overrides the three caps."""
    nc = min(-(-65536 // B), 32, T // 4)
    if forced > 0:
        nc = min(forced, T)
    nc = max(nc, 1)
    ln = -(-T // nc)
    n = -(-T // ln)
    return n, ln, T - (n - 1) * ln


# the class every horizon below was chosen for: a retuned chunk_geometry() fails here instead of silently losing the edges
HORIZONS = {
    8: (2, 4, 4),     # the shortest horizon that is chunked at all
    9: (2, 5, 4),
    13: (3, 5, 3),
    37: (8, 5, 2),    # two cells in the last chunk; fewer chunks (8) than T / 4 asked for (9)
    41: (9, 5, 1),    # ONE cell in the last chunk
    128: (32, 4, 4),  # all 32 chunks
    131: (27, 5, 1),  # the cap of 32, then a one-cell tail
}
EDGES = (41, 128, 131)
BATCH_RULE = (8200, 43, (8, 6, 1))  # the chunk count comes from 65536 / B, not from T / 4 (10) or the cap; one-cell tail


def assert_geometry(B, T):
    assert geometry(B, T) == HORIZONS[T], (B, T, geometry(B, T))


def test_geometry_classes():
    for T, want in HORIZONS.items():
        for B in (1, 5, 6, 67, 100, 300):
            assert geometry(B, T) == want
    assert HORIZONS[37][0] < 37 // 4 and HORIZONS[131][0] < 32 == 131 // 4  # n < the count asked for
    B, T, want = BATCH_RULE
    assert geometry(B, T) == want and -(-65536 // B) == want[0] < min(32, T // 4)
    assert geometry(5, 12, forced=12) == (12, 1, 1) and geometry(5, 12, forced=1) == (1, 12, 12)


WORKSPACE_MODELS = ["em_pendulum_T200", "em_linear_T60", "em_cartpole_T100", "em_dcp_T60", "em_quadrotor_T20"]
WORKSPACE_GRID = [(B, T) for T in HORIZONS for B in (1, 5, 67, 300)] + [BATCH_RULE[:2], (12288, 200), (70000, 60), (3, 7), (1, 3)]


def _workspace_bytes(lib, device):
    """i2c_workspace_bytes() is exactly the three arrays of ChunkWork -- composites [n][NX + NX^2 + sym NX][B], boundary states
    [n][NX + sym NX][B], partial sums [n][3][B] -- in the arithmetic type, nothing on top, with n from the rule above."""
    for name in WORKSPACE_MODELS:
        eng = parity.engine_from_case(parity.with_horizon(load_case(name), 8), lib, device)
        nx = eng.nx
        sym = nx * (nx + 1) // 2
        per = (nx + nx * nx + sym) + (nx + sym) + 3
        for B, T in WORKSPACE_GRID:
            n = geometry(B, T)[0]
            for dtype, size in ((N.F64, 8), (N.F32, 4), (N.F64_F32S, 8)):
                assert lib.i2c_workspace_bytes(eng.model_id, dtype, B, T) == n * B * per * size, (name, B, T, dtype)


# ---- 2. the horizon sweep against the oracle -----------------------------------------------------------------------------------
LANE = dict(group_lanes=-1, backward_mode="chunked")
QUAD = dict(group_lanes=64, backward_mode="chunked")
FAMILIES = {  # (backward family, schedule, compose + stitch passes, stitch pass alone) of a request
    "lane": ("lane", "chunked", "lane", "lane"),
    "quad": ("quad", "chunked", "quad", "quad"),
    "walk_lane": ("lane", "chunked", "quad", "quad"),    # default mix: lane walker behind quad compose + stitch
    "stitch_quad": ("lane", "chunked", "lane", "quad"),  # default mix: the stitch pass alone in the quad form
}


def tolerance(name, device):
    """The project's own bounds (test_kernels_hostsim.py / test_hip_parity.py): for the pendulum class (pendulum, linear) 1e-9 on the
    host simulation and 1e-8 on the device, for the d >= 4 models and the other inference rules 1e-7 / 1e-6; policy x 10.
    (Known, and outside what the host simulation runs here: the linear model at B = 67, T = 131 -- a device case, bound 1e-8 --
    differs from the oracle by 1.12e-9 in sig_xu1_f on EVERY backward schedule, the fused and two-pass ones included.)"""
    if name in ("em_pendulum_T200", "em_linear_T60"):
        return 1e-9 if device == "cpu" else 1e-8
    return 1e-7 if device == "cpu" else 1e-6


def families_of(eng):
    return (eng.backward_family, eng.backward_schedule, eng.kernel_family("chunk_passes"), eng.kernel_family("chunk_stitch"))


def run_sweep_case(lib, device, name, form, B, T, **kw):
    assert_geometry(B, T)
    req = {"lane": LANE, "quad": QUAD}.get(form, {})
    eng, _ = parity.check_batch_against_oracle(name, lib, device, B, 2, tol=tolerance(name, device), T=T, **req, **kw)
    assert families_of(eng) == FAMILIES[form], (name, form, B, T, families_of(eng))
    assert eng.work is not None and eng.H == T and eng.B == B
    return eng


def _grid(name, form, pairs, **kw):
    return [pytest.param(name, form, B, T, kw, id=f"{name}-{form}{'-' + '-'.join(kw) if kw else ''}-B{B}-T{T}") for B, T in pairs]


def _sim_subset(params):
    """What the host simulation runs of a list: it steps the 64 lanes of every quad wavefront and chunk as threads, so B = 67 in the
    quad form takes it 4 - 14 s a case. It keeps one such case (the pendulum at T = 41); the device runs them all."""
    keep = lambda name, form, B, T: form != "quad" or B < 67 or (name, T) == ("em_pendulum_T200", 41)  # noqa: E731
    return [p for p in params if keep(*(p.values if hasattr(p, "values") else p)[:4])]


def _device_subset(params):
    """... and of the device: everything but the general-weights rule at T = 128 (see GENERAL)."""
    return [p for p in params if not (p.values[3] == 128 and "quad" in p.values[4])]


ALL_T_SMALL_B = [(B, T) for T in HORIZONS for B in (1, 5)]
EDGES_B5 = [(5, T) for T in EDGES]
RAGGED = [(67, 41), (67, 131)]  # 67 = 16 quad wavefronts + three of four slots = one lane wavefront + three lanes
# A variant of the quad form: one general-weights rule (W = 0.8975, the weights do not sum to one) on the double cartpole. Under it
# the gain is ill-conditioned (max |K| = 109 against 0.12 under the unit rule), and at most horizons EVERY schedule, the fused walks
# included, leaves parity.close()'s element-wise floor in some small entry while staying within 1.5e-7 in the max-norm. Measured
# on the host simulation, in units of the floor (quad chunked / quad fused / lane chunked / lane fused):
#   K after one iteration:  T = 13: 11 / 1.7 / 7.4 / 2.0    T = 9: 12 / 1.5 / 4.8 / 1.4    T = 37: 0.8 / 0.3 / 1.4 / 0.4
#   mu_xu1_f after two:     T = 131: 1.7 / 2.1 / 10 / 4.9   T = 128: 0.8 / 0.4 / 1.0 / 0.8  T = 41: 0.06 or less for all four
# That is the case's noise, not a chunk edge. So the rule runs the one-cell tail (T = 41) everywhere and all 32 chunks (T = 128) on
# the host simulation, whose arithmetic is fixed (no contraction); 0.8 of the floor is too close to ask of the device's other
# rounding. T = 131 is left to the unit rule on the same model.
GENERAL = dict(quad=(1.05, 0.0, 0.3))
SWEEP = (
    # every horizon on the lane and on the all-quad form (pendulum: the double-buffered lane walker, d <= 5)
    _grid("em_pendulum_T200", "lane", ALL_T_SMALL_B + RAGGED) + _grid("em_pendulum_T200", "quad", ALL_T_SMALL_B + RAGGED)
    # the single-buffered lane walker (d = 7)
    + _grid("em_dcp_T60", "lane", EDGES_B5 + [(1, 41)])
    # the lane schedule with the full (non-lean) walker: smoothed state, observed marginal, per-cell statistics, compared too
    + _grid("em_pendulum_T200", "lane", EDGES_B5 + [(5, 37)], optional_outputs=True) + _grid("em_dcp_T60", "lane", [(5, 41)], optional_outputs=True)
    + _grid("em_dcp_T60", "quad", [(5, 41)], optional_outputs=True)
    # the whole schedule in the quad form on every d <= 8 model, and one general-weights rule
    + _grid("em_linear_T60", "quad", EDGES_B5 + RAGGED) + _grid("em_cartpole_T100", "quad", EDGES_B5 + RAGGED)
    + _grid("em_dcp_T60", "quad", EDGES_B5 + [(1, 131), (5, 37)]) + _grid("em_quadrotor_T20", "quad", EDGES_B5)
    + _grid("em_dcp_T60", "quad", [(5, 41), (5, 128)], **GENERAL)
    # Linearize and Gauss-Hermite: their own compose / stitch / walk / reduce kernels
    + _grid("lin_pendulum_T100", "lane", EDGES_B5 + RAGGED + [(1, 41), (5, 37)]) + _grid("lin_dcp_T80", "lane", EDGES_B5)
    + _grid("gh3_pendulum_T40", "lane", EDGES_B5 + [(5, 37)])
)
# the default mixes, nothing asked for: the windows of the walker, the compose + stitch passes and the stitch pass alone
MIXES = (_grid("em_cartpole_T100", "walk_lane", [(100, T) for T in EDGES]) + _grid("em_dcp_T60", "stitch_quad", [(300, T) for T in EDGES])
         + _grid("em_dcp_T60", "quad", [(67, T) for T in EDGES]))
# The host simulation steps every quad wavefront as 64 threads: B = 67 ... 300 of these models take it minutes. Its twins run the SAME
# three mixes of kernels at B = 5, where a request reaches them: nothing asked for is the all-quad mix there; the schedule asked for by
# name keeps the lane walker behind quad compose + stitch passes; the library's window knobs (read once per process: a child) leave
# the stitch pass alone in the quad form.
MIXES_SIM = (_grid("em_dcp_T60", "quad", EDGES_B5) + _grid("em_dcp_T60", "walk_lane", EDGES_B5, backward_mode="chunked")
             + _grid("em_cartpole_T100", "walk_lane", [(5, 41)], backward_mode="chunked"))


def _sweep_form(lib, device, name, form, B, T, kw):
    if name.startswith(("lin_", "gh")):  # (these rules have one family; the request is the schedule alone)
        assert_geometry(B, T)
        eng, _ = parity.check_batch_against_oracle(name, lib, device, B, 2, tol=tolerance(name, device), T=T, backward_mode="chunked", **kw)
        assert (eng.backward_family, eng.backward_schedule) == ("lane", "chunked") and eng.work is not None  # (no quad passes to ask about)
        return
    run_sweep_case(lib, device, name, form, B, T, **kw)


def _default_mix(lib, device, name, form, B, T, **kw):
    assert_geometry(B, T)
    eng, _ = parity.check_batch_against_oracle(name, lib, device, B, 2, tol=tolerance(name, device), T=T, **kw)
    assert families_of(eng) == FAMILIES[form], (name, B, T, families_of(eng))


def stitch_mix_child(T):
    """(runs in the child, I2C_QUAD_PASSES_MAX_B = 0 and I2C_QUAD_STITCH_MAX_B = 1000) lane compose, QUAD stitch, lane walker."""
    _default_mix(hostsim.load(), "cpu", "em_dcp_T60", "stitch_quad", 5, T, backward_mode="chunked")
    print("mix ok")


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


def _fp32_storage(lib, device, name, form, B, T):
    """fp32-stored messages through the chunked schedule, against the SAME engine's fused walk under the same storage, at the bound
    test_precision.py holds that pair to (one iteration, posterior mean within 1e-5: storage rounding, composed in another order)."""
    assert_geometry(B, T)
    g = parity.with_horizon(load_case(name), T)
    x0, mu_u = parity.batched_inputs(g, B)
    req = {"lane": LANE, "quad": QUAD}[form]
    ch = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, storage_dtype=torch.float32, **req)
    fu = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, storage_dtype=torch.float32, **dict(req, backward_mode="fused"))
    assert families_of(ch) == FAMILIES[form] and fu.backward_schedule == "fused" and fu.backward_family == form
    assert ch.mixed and ch.fwd.dtype == torch.float32 and ch.post.dtype == torch.float32 and ch.work.dtype == torch.float64
    for e in (ch, fu):
        e.learn_msgs()
        assert e.failures() == []
    mu_c, mu_f = ch.marginal_state_action()[0].double(), fu.marginal_state_action()[0].double()
    assert torch.isfinite(ch.post.double()).all() and torch.isfinite(ch.alpha).all()
    assert _rel(mu_c, mu_f) < 1e-5, (name, form, B, T, _rel(mu_c, mu_f))


FP32 = [(name, form, B, T) for name in ("em_pendulum_T200", "em_dcp_T60") for form in ("lane", "quad") for B, T in EDGES_B5 + [(5, 37)]] + \
       [("em_pendulum_T200", form, B, T) for form in ("lane", "quad") for B, T in RAGGED]


# ---- 4. workspace hygiene -------------------------------------------------------------------------------------------------------
SENTINEL = -7.0e77
GUARD = 4096


def _workspace_hygiene(lib, device, name, form, T, B=67):
    """Every element of the workspace that a backward call reads was written by that call, and nothing is written behind
    i2c_workspace_bytes: the workspace is NaN before EACH call and has a sentinel-filled tail; two EM iterations give finite
    outputs, bit for bit those of the run on its own clean workspace, and leave the tail as it was."""
    assert_geometry(B, T)
    g = parity.with_horizon(load_case(name), T)
    x0, mu_u = parity.batched_inputs(g, B)
    req = {"lane": LANE, "quad": QUAD, "lin": dict(backward_mode="chunked")}[form]
    clean = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, **req)
    eng = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, **req)
    assert (eng.backward_family, eng.backward_schedule) == ("quad" if form == "quad" else "lane", "chunked")
    n = eng.work.numel()
    assert n * 8 == lib.i2c_workspace_bytes(eng.model_id, N.F64, B, T)
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=eng.device)
    eng.work = buf[:n]
    eng._problem.work = buf.data_ptr()
    for _ in range(2):
        clean.learn_msgs()
        eng.em_iter += 1
        eng.forward_sweep()
        buf[:n] = float("nan")
        eng.backward_sweep()
        eng.maximize()
    assert eng.failures() == [] and clean.failures() == []
    assert torch.equal(buf[n:], torch.full_like(buf[n:], SENTINEL)), "written behind the workspace"
    outs = lambda e: (e.post, e.alpha, e.term_stats, e.costs_m[-1], e.costs_m_var[-1], e.alphas_desired[-1])  # noqa: E731
    for a, b in zip(outs(eng), outs(clean)):
        assert torch.isfinite(a).all(), "an element of the workspace was read before this call wrote it"
        assert torch.equal(a, b)


HYGIENE = [(name, form, T) for name, form in (("em_pendulum_T200", "lane"), ("em_pendulum_T200", "quad"), ("em_dcp_T60", "lane"),
                                              ("em_dcp_T60", "quad"), ("lin_pendulum_T100", "lin")) for T in (41, 131)]


# ---- 5. failure isolation at the chunk edges ------------------------------------------------------------------------------------
def _failure_at_chunk_edge(lib, device, form, cell):
    """The numeric status path (reason 7: a smoothed joint that is not positive definite) in the lone cell of the last chunk and
    in the first cell of a chunk, T = 41 = eight chunks of five cells + one of one: trajectory 2 is reported, alone, and every other
    trajectory -- the three that share its quad wavefront included -- is bit for bit what the clean run gives."""
    T, B = 41, 6
    assert_geometry(B, T)
    assert cell % HORIZONS[T][1] == 0  # the first cell of its chunk (40: also its last)
    g = parity.with_horizon(load_case("em_dcp_T60"), T)
    x0, mu_u = parity.batched_inputs(g, B)
    req = {"lane": LANE, "quad": QUAD}[form]
    eng = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, **req)
    clean = parity.engine_from_case(g, lib, device, x0=x0, mu_u=mu_u, **req)
    assert families_of(eng) == FAMILIES[form]
    for e in (eng, clean):
        e.forward_sweep()
    eng.fwd[cell, eng.d, 2] = -1.0  # sig_xu1_f[0][0] of that cell, trajectory 2
    for e in (eng, clean):
        e.backward_sweep()
    assert clean.failures() == []
    assert [(b, r) for b, r, _ in eng.failures()] == [(2, 7)], eng.failures()  # (the chunks walk concurrently: any cell of trajectory 2)
    ok = [0, 1, 3, 4, 5]
    for a, b in zip(eng.marginal_state_action() + eng.local_linear_policy() + (eng.term_stats.T,),
                    clean.marginal_state_action() + clean.local_linear_policy() + (clean.term_stats.T,)):
        assert torch.equal(a[ok], b[ok])


# ---- 6. the I2C_CHUNKS knob (read once per process: a child process per value) --------------------------------------------------
def knob_child(device, forced):
    """(runs in the child) T = 12 with I2C_CHUNKS = 12: every chunk is one cell; = 1: the whole horizon is one chunk. Pendulum and
    double cartpole, lane and all-quad form, against the oracle, in sequence."""
    lib = hostsim.load() if device == "cpu" else parity.pkg.load_library()
    assert bool(lib.is_host_sim) == (device == "cpu")
    T = 12
    for name in ("em_pendulum_T200", "em_dcp_T60"):
        for form, B in (("lane", 5), ("quad", 5), ("quad", 1)):
            n = geometry(B, T, forced)[0]
            assert (n, geometry(B, T)[0]) == (forced, 3)
            eng, _ = parity.check_batch_against_oracle(name, lib, device, B, 2, tol=tolerance(name, device), T=T, **{"lane": LANE, "quad": QUAD}[form])
            assert families_of(eng) == FAMILIES[form]
            per = (eng.nx + eng.nx ** 2 + eng.nx * (eng.nx + 1) // 2) + (eng.nx + eng.nx * (eng.nx + 1) // 2) + 3
            assert eng.work.numel() == n * B * per, "the knob did not reach chunk_geometry()"
    print("knob ok")


def _child(call, env, ok, timeout):
    script = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "input-inference-for-control_amd")!r}, {os.path.join(ROOT, "tests")!r}]
        import test_chunk_geometry
        test_chunk_geometry.{call}
    """)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, **env), timeout=timeout)
    assert r.returncode == 0 and ok in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def _chunks_knob(device, forced, timeout):
    _child(f"knob_child({device!r}, {forced})", dict(I2C_CHUNKS=str(forced)), "knob ok", timeout)


# ---- the host simulation -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    return hostsim.load()


def test_hostsim_workspace_bytes(sim):
    _workspace_bytes(sim, "cpu")


@pytest.mark.parametrize("name,form,B,T,kw", _sim_subset(SWEEP))
def test_hostsim_chunk_geometry_vs_oracle(sim, name, form, B, T, kw):
    _sweep_form(sim, "cpu", name, form, B, T, kw)


@pytest.mark.parametrize("name,form,B,T,kw", MIXES_SIM)
def test_hostsim_chunk_geometry_mixes_vs_oracle(sim, name, form, B, T, kw):
    _default_mix(sim, "cpu", name, form, B, T, **kw)


@pytest.mark.parametrize("T", EDGES)
def test_hostsim_chunk_geometry_stitch_mix_vs_oracle(T):
    _child(f"stitch_mix_child({T})", dict(I2C_QUAD_PASSES_MAX_B="0", I2C_QUAD_STITCH_MAX_B="1000"), "mix ok", 300)


@pytest.mark.parametrize("name,form,B,T", _sim_subset(FP32))
def test_hostsim_chunk_geometry_fp32_storage(sim, name, form, B, T):
    _fp32_storage(sim, "cpu", name, form, B, T)


@pytest.mark.parametrize("name,form,T", HYGIENE)
def test_hostsim_chunk_workspace_hygiene(sim, name, form, T):
    """(B = 67 in the quad form takes the host simulation 10 - 90 s a case: it runs that form with B = 5, the device with 67)"""
    _workspace_hygiene(sim, "cpu", name, form, T, B=5 if form == "quad" else 67)


@pytest.mark.parametrize("cell", [40, 5])
@pytest.mark.parametrize("form", ["lane", "quad"])
def test_hostsim_chunk_edge_failure_is_per_trajectory(sim, form, cell):
    _failure_at_chunk_edge(sim, "cpu", form, cell)


@pytest.mark.parametrize("forced", [12, 1])
def test_hostsim_chunks_knob(forced):
    _chunks_knob("cpu", forced, 300)


# ---- the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    lib = parity.pkg.load_library()
    assert not lib.is_host_sim, "GPU tests must run the HIP build"
    return lib


@pytest.mark.gpu
def test_hip_workspace_bytes(hip):
    _workspace_bytes(hip, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,B,T,kw", _device_subset(SWEEP))
def test_hip_chunk_geometry_vs_oracle(hip, name, form, B, T, kw):
    _sweep_form(hip, "cuda", name, form, B, T, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,B,T,kw", MIXES)
def test_hip_chunk_geometry_default_mixes_vs_oracle(hip, name, form, B, T, kw):
    _default_mix(hip, "cuda", name, form, B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,B,T", FP32)
def test_hip_chunk_geometry_fp32_storage(hip, name, form, B, T):
    _fp32_storage(hip, "cuda", name, form, B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["auto", "chunked"])
def test_hip_chunk_count_from_the_batch_rule(hip, mode):
    """B = 8200, T = 43: eight chunks because 65536 / B says so, six cells each and ONE in the last; 8200 = 128 lane wavefronts +
    8 lanes = 2050 quad wavefronts. The default (lane walker and compose, quad stitch) and the lane schedule asked for by name,
    both against the ORACLE (two iterations of it on 8200 x 43 cells take a few seconds), at the pendulum's bound."""
    B, T, want = BATCH_RULE
    assert geometry(B, T) == want
    eng, _ = parity.check_batch_against_oracle("em_pendulum_T200", hip, "cuda", B, 2, tol=tolerance("em_pendulum_T200", "cuda"), T=T, backward_mode=mode)
    assert families_of(eng)[:2] == ("lane", "chunked")
    assert eng.work.numel() * 8 == hip.i2c_workspace_bytes(eng.model_id, N.F64, B, T) == want[0] * B * (2 + 4 + 3 + 2 + 3 + 3) * 8


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,T", HYGIENE)
def test_hip_chunk_workspace_hygiene(hip, name, form, T):
    _workspace_hygiene(hip, "cuda", name, form, T)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [40, 5])
@pytest.mark.parametrize("form", ["lane", "quad"])
def test_hip_chunk_edge_failure_is_per_trajectory(hip, form, cell):
    _failure_at_chunk_edge(hip, "cuda", form, cell)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [12, 1])
def test_hip_chunks_knob(forced):
    _chunks_knob("cuda", forced, 240)
