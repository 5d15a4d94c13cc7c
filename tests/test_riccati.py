"""The Riccati-form backward messages (k_riccati / riccati_body, csrc/i2c_linearize.hpp; BatchedI2c.riccati_sweep(), I2cGraph.
_backward_ricatti_msgs(), i2c_riccati_sweep): the reference's I2cCell._backward_ricatti_msgs (i2c.py:612-678) after a Linearize() pass.

  (a) batched oracle matrix: five models, horizons from 1 cell up, batches with a ragged last wavefront and three wavefronts,
      feed-forward and feedback cells, both backward schedules (all the kernel takes of them is xm[T-1]), every lane request;
  (b) the oracle, its per-cell twin (tests/riccati_twin.py) and the kernels against goldens captured from the real reference on
      well-conditioned problems (tools/gen_golden_riccati.py);
  (c) per-cell temperatures (I2cProblem.alpha_cell): the kernel took alpha[b] for every cell -- wrong by 0.3 to 0.6 on K, nu and lambda
      once the temperatures of the cells differ;
  (d) a moved ring and per-cell targets; (e) per-trajectory model parameters; (f) the failure code I2C_FAIL_RICCATI; (g) refusals.
Protocol of a case: n - 1 EM iterations, one forward/backward pass, then the Riccati messages, on the engine and on the oracle alike.
Bounds: 1e-8 max-norm relative on the host simulation (the per-iteration detail bound of tests/parity.py; two fp64 implementations,
LU in NumPy and Cholesky in the kernel: 2.6e-9 at worst), 1e-7 on the device (one decade above, as tests/test_chunk_geometry.py: the
device contracts multiply-adds; 1.5e-9 at worst). Measured figures, and which test catches which mutant: profiles/riccati_parity.txt.
CPU: the host simulation of the kernels; `-m gpu`: the library on the MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hostsim
import parity
from golden_util import assert_close, assert_close_per_cell, load_case, oracle_from_case, rel_err
from parity import close, np_
from riccati_twin import with_cell_alpha

pkg = parity.pkg
_native = pkg._native
sym = pkg.engine.sym_size
RIC = ("K", "k", "sigK", "nu_x0_b", "lambda_x0_b")
TOL = {"cpu": 1e-8, "cuda": 1e-7}
TOL_SWEEPS = {"cpu": 1e-9, "cuda": 1e-8}  # the twin against the ordinary sweeps, the device one decade above as in TOL (measured: 5.5e-11 / 3.5e-11)
EINVAL, ENOTSUP = -1, -2  # include/i2c_hip.h
FAIL_RICCATI = 10


def _lib(device):
    return hostsim.load() if device == "cpu" else pkg.load_library()


# ---- the protocol --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name, T):
    g = load_case(name)
    return g if T is None else parity.with_horizon(g, T)


def pair(name, T, B, device, **kw):
    """engine and oracle of golden case `name` over T cells on the batched inputs of tests/parity.py"""
    g = _case(name, T)
    x0, mu_u = parity.batched_inputs(g, B)
    eng = parity.engine_from_case(g, _lib(device), device, x0=x0, mu_u=mu_u, keep_xm=True, **kw)
    ora = oracle_from_case(type(g)({**dict(g), "mu_u": mu_u}), x0=x0)
    if g.meta.get("propagate"):
        eng.propagate()
        ora.propagate()
    return eng, ora


def sweeps(s, n):
    """n - 1 EM iterations and the forward/backward pass of the n-th (engine or oracle)"""
    for _ in range(n - 1):
        s.learn_msgs()
    s.em_iter += 1
    s.forward_backward()


def riccati(eng, expect_clean=True):
    """riccati_sweep() and what holds for every call: the posterior mean and covariance are not touched, sigK is the action block of
    the posterior covariance, and -- unless the case is about it -- nothing failed"""
    d, nx = eng.d, eng.nx
    before = eng.post.clone()
    nu, lam = eng.riccati_sweep()
    if eng.device.type == "cuda":
        torch.cuda.synchronize()
    K, k, sigK = eng.local_linear_policy()
    assert torch.equal(eng.post[:, : d + sym(d)], before[:, : d + sym(d)]), "the sweep wrote the posterior moments"
    if expect_clean:
        assert eng.failures() == [], eng.failures()
        assert torch.equal(sigK, eng.marginal_state_action()[1][:, :, nx:, nx:]), "sigK is not sig_u0_m"
    return dict(K=K.clone(), k=k.clone(), sigK=sigK.clone(), nu_x0_b=nu.clone(), lambda_x0_b=lam.clone())


def against(out, ref, tol, what, b=None):
    """the five outputs against ref (an oracle, or a mapping of arrays): max-norm relative at tol, and every (trajectory, cell) block
    on its own scale at the north star's 1e-4, so that a cell whose message is small cannot hide behind the large ones. Prints every
    figure for the record.
    (Not parity.close: its element-wise floor, tol / 100 = 1e-10 of the array maximum, is below the ORACLE's own rounding error in
    the end-of-chain cell, where lambda_x3_b = inv(sig_x3_m) - inv(sig_x3_f) cancels. Against 60-digit arithmetic on the inputs each
    side had (cartpole, T = 7, B = 5): oracle 5e-11 ... 4e-10, kernel 4e-11 ... 4.6e-10 of the maximum on nu_x0_b / lambda_x0_b, and
    the 1e-12 by which their inputs differ moves the exact answer by 1e-10 ... 3e-10.)"""
    for key in RIC:
        a = np_(out[key]) if b is None else np_(out[key])[b]
        r = np.asarray(getattr(ref, key) if not isinstance(ref, dict) else ref[key], float)
        print(f"riccati-parity | {what} | {key} | {rel_err(a, r):.3e}")
        assert_close(a, r, tol, f"{what} {key}")
        lead = 1 if b is not None else 2  # (T, ...) or (B, T, ...)
        assert_close_per_cell(a.reshape((-1,) + a.shape[lead:]), r.reshape((-1,) + r.shape[lead:]), 1e-4, f"{what} {key}")


def equal(a, b, what):
    for key in RIC:
        assert torch.equal(a[key], b[key]), f"{what}: {key} differs by {float((a[key] - b[key]).abs().max()):.3e}"


# ---- (a): the batched oracle matrix ----------------------------------------------------------------------------------------------
# (case, T, B, n, backward_mode): a sparse cross of horizons {1, 2, 3, 9, 13} (pendulum, linear), {7, 12} (cartpole), {8} (double
# cartpole), 12 (terminal state prior), batches {1, 5, 67, 130} = one lane, a ragged wavefront, a full and a ragged one, three
# wavefronts, n = 1 (feed-forward cells) and 3 (feedback cells), and at T = 9 every backward schedule
MATRIX = [
    ("lin_pendulum_T100", 1, 1, 1, "auto"), ("lin_pendulum_T100", 1, 67, 3, "auto"), ("lin_pendulum_T100", 2, 5, 3, "auto"),
    ("lin_pendulum_T100", 3, 130, 1, "auto"), ("lin_pendulum_T100", 9, 130, 3, "auto"), ("lin_pendulum_T100", 9, 5, 3, "fused"),
    ("lin_pendulum_T100", 9, 67, 3, "chunked"), ("lin_pendulum_T100", 13, 67, 1, "auto"), ("lin_pendulum_T100", 13, 5, 3, "auto"),
    ("lin_linear_T60", 1, 5, 3, "auto"), ("lin_linear_T60", 2, 130, 1, "auto"), ("lin_linear_T60", 3, 1, 3, "auto"),
    ("lin_linear_T60", 9, 67, 1, "chunked"), ("lin_linear_T60", 9, 1, 3, "fused"), ("lin_linear_T60", 13, 67, 3, "auto"),
    ("lin_cartpole_T100", 7, 5, 1, "auto"), ("lin_cartpole_T100", 7, 130, 3, "auto"), ("lin_cartpole_T100", 12, 67, 3, "auto"),
    ("lin_cartpole_T100", 12, 1, 1, "auto"),
    ("lin_dcp_T80", 8, 5, 3, "auto"), ("lin_dcp_T80", 8, 67, 1, "auto"), ("lin_dcp_T80", 8, 1, 3, "auto"),
    ("lin_covctrl_T50", 12, 5, 3, "auto"), ("lin_covctrl_T50", 12, 67, 1, "auto"),
]
MATRIX_IDS = [f"{c.split('_')[1]}-T{T}-B{B}-n{n}-{m}" for c, T, B, n, m in MATRIX]


def _matrix(device, name, T, B, n, mode):
    eng, ora = pair(name, T, B, device, backward_mode=mode)
    if mode != "auto":
        assert eng.backward_schedule == mode
    sweeps(eng, n)
    sweeps(ora, n)
    out = riccati(eng)
    ora.riccati_sweep()
    against(out, ora, TOL[device], f"{device} {name} T={T} B={B} n={n} {eng.backward_schedule}")


@pytest.mark.parametrize("name,T,B,n,mode", MATRIX, ids=MATRIX_IDS)
def test_oracle_matrix_cpu(name, T, B, n, mode):
    _matrix("cpu", name, T, B, n, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B,n,mode", MATRIX, ids=MATRIX_IDS)
def test_oracle_matrix_gpu(name, T, B, n, mode):
    _matrix("cuda", name, T, B, n, mode)


def _requests(device):
    """every request lane_request() lets through runs the one kernel there is: bit-identical results. (The request is put into the
    problem of the call: under Linearize() the planner of the ordinary sweeps has no quad kernels to give to 64.)"""
    outs = []
    for lanes in (0, -1, 64, _native.LANES_QUAD):
        eng, _ = pair("lin_cartpole_T100", 12, 5, device)
        sweeps(eng, 3)
        eng._problem.group_lanes = lanes
        outs.append(riccati(eng))
    for lanes, o in zip((-1, 64, _native.LANES_QUAD), outs[1:]):
        equal(o, outs[0], f"group_lanes={lanes} against 0")


def test_lane_requests_cpu():
    _requests("cpu")


@pytest.mark.gpu
def test_lane_requests_gpu():
    _requests("cuda")


# ---- (b): pinned to the reference -----------------------------------------------------------------------------------------------
PLAIN_GOLDENS = ["lin_pendulum_riccati_T12", "lin_linear_riccati_T12"]
CELL_GOLDEN = "lin_pendulum_riccati_T12_cellalpha"


def _golden(g, n):
    return {k: g[f"ric{n}/{k}"] for k in RIC + ("mu_xu0_m", "sig_xu0_m")}


def _replay_plain(s, do_riccati):
    """the generator's run: pass, Riccati (ric1), M-step | one EM iteration | pass, Riccati (ric3): the second iteration feeds back
    the gain the first Riccati pass left in the cells. Yields (n, result of do_riccati)."""
    s.em_iter += 1
    s.forward_backward()
    yield 1, do_riccati()
    s.maximize()
    s.learn_msgs()
    s.em_iter += 1
    s.forward_backward()
    yield 3, do_riccati()


def _oracle_outputs(o):
    o.riccati_sweep()
    return {k: getattr(o, k).copy() for k in RIC}


@pytest.mark.parametrize("name", PLAIN_GOLDENS)
def test_oracle_against_reference(name):
    g = load_case(name)
    o = oracle_from_case(g)
    for n, out in _replay_plain(o, lambda: _oracle_outputs(o)):
        for k in RIC:
            assert_close(out[k][0], g[f"ric{n}/{k}"], 1e-7, f"{name} ric{n} {k}")


def _scaled_oracle(g, n):
    o = oracle_from_case(g)
    for _ in range(n - 1):
        o.learn_msgs()
    o.em_iter += 1
    with_cell_alpha(o, o.alpha[:, None] * np.asarray(g.meta["cell_scale"])[None])
    o.forward_backward()
    return o


@pytest.mark.parametrize("n", [1, 3])
def test_twin_against_reference(n):
    g = load_case(CELL_GOLDEN)
    o = _scaled_oracle(g, n)
    assert_close(o.mu_xu0_m[0], g[f"ric{n}/mu_xu0_m"], 1e-7, f"ric{n} mu_xu0_m")
    assert_close(o.sig_xu0_m[0], g[f"ric{n}/sig_xu0_m"], 1e-7, f"ric{n} sig_xu0_m")
    out = _oracle_outputs(o)
    for k in RIC:
        assert_close(out[k][0], g[f"ric{n}/{k}"], 1e-7, f"{CELL_GOLDEN} ric{n} {k}")
    # (the unscaled oracle is nowhere near: the scaling is what the golden is about)
    assert rel_err(g[f"ric{n}/K"], load_case(PLAIN_GOLDENS[0])["ric1/K"]) > 1e-2


def _kernels_against_reference(device, name):
    g = load_case(name)
    eng = parity.engine_from_case(g, _lib(device), device, keep_xm=True)
    for n, out in _replay_plain(eng, lambda: riccati(eng)):
        against(out, _golden(g, n), TOL[device], f"{device} {name} ric{n}", b=0)


@pytest.mark.parametrize("name", PLAIN_GOLDENS)
def test_kernels_against_reference_cpu(name):
    _kernels_against_reference("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN_GOLDENS)
def test_kernels_against_reference_gpu(name):
    _kernels_against_reference("cuda", name)


def _kernels_against_reference_cellalpha(device, n):
    g = load_case(CELL_GOLDEN)
    eng = parity.engine_from_case(g, _lib(device), device, keep_xm=True)
    for _ in range(n - 1):
        eng.learn_msgs()
    eng.em_iter += 1
    eng.enable_per_cell_alpha()
    eng.alpha_cell *= torch.as_tensor(g.meta["cell_scale"], dtype=eng.dtype, device=eng.device)[:, None]
    eng.forward_backward()
    mu, sig = eng.marginal_state_action()
    close(np_(mu)[0], g[f"ric{n}/mu_xu0_m"], TOL[device], f"{device} {CELL_GOLDEN} ric{n} mu_xu0_m")
    close(np_(sig)[0], g[f"ric{n}/sig_xu0_m"], TOL[device], f"{device} {CELL_GOLDEN} ric{n} sig_xu0_m")
    against(riccati(eng), _golden(g, n), TOL[device], f"{device} {CELL_GOLDEN} ric{n}", b=0)


@pytest.mark.parametrize("n", [1, 3])
def test_kernels_against_reference_cellalpha_cpu(n):
    _kernels_against_reference_cellalpha("cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_kernels_against_reference_cellalpha_gpu(n):
    _kernels_against_reference_cellalpha("cuda", n)


# ---- (c): per-cell temperatures ---------------------------------------------------------------------------------------------------
def cell_scale(T, B):
    return np.outer(np.linspace(0.5, 2.0, T), np.linspace(1.0, 1.3, B))  # [T][B]


def _cell_alpha(device, name, n, T=12, B=5):
    eng, ora = pair(name, T, B, device)
    for s in (eng, ora):
        for _ in range(n - 1):
            s.learn_msgs()
        s.em_iter += 1
    scale = cell_scale(T, B)
    eng.enable_per_cell_alpha()
    eng.alpha_cell *= torch.as_tensor(scale, dtype=eng.dtype, device=eng.device)
    with_cell_alpha(ora, ora.alpha[:, None] * scale.T)
    eng.forward_backward()
    ora.forward_backward()
    # the twin is tied to kernels that are validated elsewhere: the ordinary sweeps honour alpha_cell
    what = f"{device} {name} cell alpha T={T} B={B} n={n}"
    mu, sig = eng.marginal_state_action()
    K, k, _ = eng.local_linear_policy()
    for key, a in (("mu_xu0_m", mu), ("sig_xu0_m", sig), ("K", K), ("k", k)):
        print(f"riccati-parity | {what} sweeps | {key} | {rel_err(np_(a), getattr(ora, key)):.3e}")
        close(np_(a), getattr(ora, key), TOL_SWEEPS[device], f"{what} sweeps {key}")
    out = riccati(eng)
    ora.riccati_sweep()
    against(out, ora, TOL[device], what)


CELL_ALPHA = [("lin_linear_T60", 3), ("lin_pendulum_T100", 1), ("lin_pendulum_T100", 3), ("lin_cartpole_T100", 3)]


@pytest.mark.parametrize("name,n", CELL_ALPHA)
def test_cell_alpha_cpu(name, n):
    _cell_alpha("cpu", name, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", CELL_ALPHA)
def test_cell_alpha_gpu(name, n):
    _cell_alpha("cuda", name, n)


def _cell_alpha_all_equal(device):
    """every row of alpha_cell equal to alpha: the run without alpha_cell, bit for bit"""
    outs = []
    for per_cell in (False, True):
        eng, _ = pair("lin_pendulum_T100", 12, 5, device)
        for _ in range(2):
            eng.learn_msgs()
        if per_cell:
            eng.enable_per_cell_alpha()
            assert torch.equal(eng.alpha_cell, eng.alpha.reshape(1, -1).expand(eng.H, -1))
        eng.em_iter += 1
        eng.forward_backward()
        outs.append(riccati(eng))
        outs[-1]["post"] = eng.post.clone()
    equal(outs[1], outs[0], "alpha_cell == alpha")
    assert torch.equal(outs[1]["post"], outs[0]["post"])


def test_cell_alpha_all_equal_cpu():
    _cell_alpha_all_equal("cpu")


@pytest.mark.gpu
def test_cell_alpha_all_equal_gpu():
    _cell_alpha_all_equal("cuda")


# ---- (d): a moved ring, per-cell targets ----------------------------------------------------------------------------------------
def _targets(eng, T, B, seed=7, extra=0):
    rng = np.random.default_rng(seed)
    return np.asarray(eng.zg).reshape(1, 1, -1) + 1e-2 * rng.normal(size=(B, T + extra, eng.nz))


def _ring(device, name, T, B, shifts=4):
    a, _ = pair(name, T, B, device)
    b, _ = pair(name, T, B, device)
    z = _targets(a, T, B, extra=shifts)
    for e in (a, b):
        e.set_targets(z[:, :T])
        e.enable_per_cell_alpha()
    a.alpha_cell *= torch.as_tensor(cell_scale(T, B), dtype=a.dtype, device=a.device)
    for s in range(shifts):
        a.forward_backward()
        a.update_priors()
        a.shift_horizon(torch.as_tensor(np.array(z[:, T + s].T, order="C"), dtype=a.dtype, device=a.device))
    assert a.t0 == shifts and b.t0 == 0
    # b := a in cell order, ring at the origin (the copy loop of tests/test_mpc.py::_ring_equals_unrolled)
    for key in ("post", "z", "alpha_cell", "feedforward"):
        getattr(b, key).copy_(a.cells(getattr(a, key)))
    for key in ("x0", "sig_x0", "alpha", "temp"):
        getattr(b, key).copy_(getattr(a, key))
    b.terminal_cell = a.terminal_cell
    b._problem.terminal_cell = int(a.terminal_cell)
    assert not torch.equal(a.z, b.z) and not torch.equal(a.alpha_cell, b.alpha_cell)  # (the ring HAS moved)
    outs = []
    for e in (a, b):
        e.forward_backward()
        outs.append(riccati(e))
    equal(outs[0], outs[1], f"{name}: ring at {shifts} against the unrolled horizon")
    assert torch.equal(a.cells(a.post), b.post)


RING = [("lin_pendulum_T100", 9, 5), ("lin_cartpole_T100", 9, 67)]


@pytest.mark.parametrize("name,T,B", RING)
def test_ring_equals_unrolled_cpu(name, T, B):
    _ring("cpu", name, T, B)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B", RING)
def test_ring_equals_unrolled_gpu(name, T, B):
    _ring("cuda", name, T, B)


def _per_cell_targets(device, T=9, B=5):
    eng, ora = pair("lin_pendulum_T100", T, B, device)
    z = _targets(eng, T, B)
    eng.set_targets(z)
    ora.z = z.copy()
    sweeps(eng, 3)
    sweeps(ora, 3)
    out = riccati(eng)
    ora.riccati_sweep()
    against(out, ora, TOL[device], f"{device} lin_pendulum_T100 per-cell targets T={T} B={B}")
    plain, _ = pair("lin_pendulum_T100", T, B, device)  # (... and the targets matter)
    sweeps(plain, 3)
    assert rel_err(np_(riccati(plain)["nu_x0_b"]), ora.nu_x0_b) > 1e-4


def test_per_cell_targets_cpu():
    _per_cell_targets("cpu")


@pytest.mark.gpu
def test_per_cell_targets_gpu():
    _per_cell_targets("cuda")


# ---- (e): per-trajectory model parameters ---------------------------------------------------------------------------------------
def _per_trajectory_params(device, T=8, n=2):
    import test_model_params_batch as mp

    model = mp.make_env_model("PlanarQuadrotor")  # d = 8: the widest model with one-lane kernels
    rows = mp.param_rows(model, 4, 3)
    lib = _lib(device)
    kw = dict(inference="linearize", keep_prior=True, keep_xm=True)

    def solve(m, B, params):
        eng = mp.engine(m, B, T, lib, device, model_params=params, **kw)
        sweeps(eng, n)
        return riccati(eng)

    out = solve(model, 4, rows)
    for j in range(4):
        one = solve(mp.with_params(model, rows[j]), 1, None)
        for key in RIC:
            assert torch.equal(out[key][j], one[key][0]), f"trajectory {j}: {key} differs from the solve of its own model copy"
    mp.assert_params_matter({"K": np_(out["K"])}, rows, 1e-5)  # (the gains of two rows differ by 2e-1)


def test_per_trajectory_params_cpu():
    _per_trajectory_params("cpu")


@pytest.mark.gpu
def test_per_trajectory_params_gpu():
    _per_trajectory_params("cuda")


# ---- (f): the failure code ------------------------------------------------------------------------------------------------------
def _improper_message(eng, b):
    """the smoothed state at the end of the chain := the forward message: lambda_x3_b = lambda_x3_m - lambda_x3_f is exactly zero"""
    T, d, nx = eng.H, eng.d, eng.nx
    o = d + sym(d)
    eng.xm[T - 1, :, b] = eng.fwd[T - 1, o: o + nx + sym(nx), b]


def _failure_isolation(device, B, bad, T=9):
    eng, _ = pair("lin_pendulum_T100", T, B, device)
    clean, _ = pair("lin_pendulum_T100", T, B, device)
    for e in (eng, clean):
        sweeps(e, 3)
    assert eng.xm.shape[1] == eng.nx + sym(eng.nx)
    _improper_message(eng, bad)
    out, ref = riccati(eng, expect_clean=False), riccati(clean)
    assert eng.failures() == [(bad, FAIL_RICCATI, 0)], eng.failures()
    assert int(eng.status[bad]) == (FAIL_RICCATI << 16) | 1
    keep = torch.as_tensor(np.delete(np.arange(B), bad), device=eng.device)
    for key in RIC:
        assert torch.equal(out[key][keep], ref[key][keep]), key
    assert torch.equal(eng.post[:, :, keep], clean.post[:, :, keep])
    # first-failure rule: a trajectory that has failed before keeps its word
    eng2, _ = pair("lin_pendulum_T100", T, B, device)
    sweeps(eng2, 3)
    _improper_message(eng2, bad)
    word = (3 << 16) | 5
    eng2.status[bad] = word
    riccati(eng2, expect_clean=False)
    assert int(eng2.status[bad]) == word and eng2.failures() == [(bad, 3, 4)]


FAILURES = [(5, 2), (67, 64)]  # (64: the first lane of the ragged second wavefront)


@pytest.mark.parametrize("B,bad", FAILURES)
def test_failure_isolation_cpu(B, bad):
    _failure_isolation("cpu", B, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("B,bad", FAILURES)
def test_failure_isolation_gpu(B, bad):
    _failure_isolation("cuda", B, bad)


def _no_terminal_cost(device, T=9, B=5):
    """without Qf the end of the chain passes the forward message on: every trajectory's backward message is improper; the call
    itself succeeds (I2C_OK), the status words say what happened"""
    g = _case("lin_linear_T60", T)
    g = type(g)({k: v for k, v in g.items() if k != "Qf"})
    x0, mu_u = parity.batched_inputs(g, B)
    eng = parity.engine_from_case(g, _lib(device), device, x0=x0, mu_u=mu_u, keep_xm=True)
    assert not eng.has_Qf
    sweeps(eng, 1)
    assert eng.failures() == []
    riccati(eng, expect_clean=False)  # (raises on any code but I2C_OK)
    assert eng.failures() == [(b, FAIL_RICCATI, 0) for b in range(B)]


def test_no_terminal_cost_cpu():
    _no_terminal_cost("cpu")


@pytest.mark.gpu
def test_no_terminal_cost_gpu():
    _no_terminal_cost("cuda")


# ---- (g): refusals --------------------------------------------------------------------------------------------------------------
def _refusals(device):
    lib = _lib(device)
    eng, _ = pair("lin_pendulum_T100", 3, 5, device)
    sweeps(eng, 1)
    eng.ric = torch.zeros(eng.H, eng.nx + eng.nx * eng.nx, eng.B, dtype=eng.dtype, device=eng.device)
    args = (eng._ptr(eng.prior_out), eng._ptr(eng.fwd), eng._ptr(eng.xm), eng._ptr(eng.post), eng._ptr(eng.ric), eng._ptr(eng.status), eng._stream())
    before = eng.post.clone()

    def call(**fields):
        p = eng._make_problem()
        for k, v in fields.items():
            setattr(p, k, v)
        return lib.i2c_riccati_sweep(C.byref(p), *args)

    assert call(inference=_native.INF_CUBATURE) == EINVAL                 # the messages belong to Linearize()
    assert call(dtype=_native.F64_F32S) == ENOTSUP                        # fp32-stored messages
    assert eng.dims.group_lanes > 0 and call(group_lanes=eng.dims.group_lanes) == ENOTSUP  # the model's group kernels have no such sweep
    assert torch.equal(eng.post, before) and eng.failures() == []         # (nothing ran)
    assert call() == 0
    # a model without one-lane kernels
    q, _ = pair("lin_quad12_T20", 3, 2, device)
    with pytest.raises(RuntimeError, match=f"i2c_riccati_sweep failed with code {ENOTSUP}"):
        q.riccati_sweep()
    # the engine: fp32 storage is refused for Linearize() before anything is built; the sweep needs the buffers it reads
    g = _case("lin_pendulum_T100", 3)
    with pytest.raises(ValueError, match="storage_dtype"):
        parity.engine_from_case(g, lib, device, storage_dtype=torch.float32)
    no_xm = parity.engine_from_case(g, lib, device, keep_xm=False, backward_mode="fused")
    sweeps(no_xm, 1)
    with pytest.raises(RuntimeError, match="keep_xm=True"):
        no_xm.riccati_sweep()
    cub = parity.engine_from_case(type(g)({**dict(g), "meta": np.array(str(g["meta"]).replace('"linearize"', '"cubature"'))}), lib, device, keep_xm=True)
    with pytest.raises(RuntimeError, match="Linearize"):
        cub.riccati_sweep()


def test_refusals_cpu():
    _refusals("cpu")


@pytest.mark.gpu
def test_refusals_gpu():
    _refusals("cuda")
