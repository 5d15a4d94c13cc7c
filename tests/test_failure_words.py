"""The failure word  status[b] = (reason << 16) | (cell + 1)  of every sweep, on every kernel family, against
tests/failure_twin.py -- a numpy answer to "where would the reference have raised" that decides positive definiteness by
eigenvalues, with a guard band that rounding cannot cross.

A MATRIX of kernel-family rows x injections, run on the host simulation and -- the same functions, marked gpu -- on the device.
Per case: exactly the poisoned trajectories carry a word; on the sequential sweeps (forward, the fused backward walk, propagate,
filter) the word equals the twin's (reason, cell); on the backward schedules that process cells concurrently (pass 2 of two_pass,
chunked) the reason equals the twin's and the cell is ONE of the cells whose smoothed joint is not positive definite; every
buffer the call writes is bit-identical to a clean engine's on the other trajectories; the failed trajectory is non-finite from
the failing cell on and -- forward sweeps -- bit-identical to the clean run before it (a word that points too late fails here).
A word already in status[b] survives every call; after status.zero_() the new failure is recorded.

Linearize rows: oracle/i2c_linearize_numpy.py goes through _sym_solve ONCE (the smoother gain, :138); every other factorisation
of its cells is np.linalg.inv / np.linalg.solve written in line, and it has no sigma points. One wrapped call out of a dozen is
no twin, so those rows are held to the invariants above and to the reasons include/i2c_hip.h documents (injections b, c, g and
the terminal update of the backward sweep). Not judged by the twin either: the KL factors of covariance control (reason 8 at
the last cell; I2cOracle.mvn_kl calls numpy in line, and no row here has a terminal state prior).

Every line `WORD ...` this module prints is one entry of profiles/failure_words.txt.
"""
import numpy as np
import pytest
import torch

import failure_twin
import hostsim
import parity
from golden_util import Case, load_case, oracle_from_case

pkg = parity.pkg
LANES_QUAD = pkg._native.LANES_QUAD
T = 8
SHAPES = [(6, (2,)), (70, (2, 67))]  # (B, poisoned): 67 sits in the second wavefront of the lane family, among live neighbours elsewhere
STALE = (10 << 16) | 3  # a word from an earlier call

# row -> (golden case, group_lanes, forward family, {backward schedule: backward family}, propagate family)
ROWS = {
    "lane-pendulum": ("em_pendulum_T40_quad_general", 0, "lane", {"fused": "lane", "two_pass": "lane", "chunked": "lane"}, "lane"),
    "group-pendulum": ("em_pendulum_T40_quad_general", True, "group", {"fused": "group"}, "group"),
    "quad-pendulum": ("em_pendulum_T40_quad_general", 64, "quad", {"fused": "quad", "two_pass": "lane", "chunked": "quad"}, "lane"),
    "quad-dcp": ("em_dcp_T60", 64, "quad", {"fused": "quad", "two_pass": "lane", "chunked": "quad"}, "lane"),
    "wave-quad12": ("em_quad12_T20", 0, "wave", {"fused": "wave", "two_pass": "wave"}, "quad"),
    "group-quad12": ("em_quad12_T20", 16, "group", {"fused": "group"}, "group"),
    "quad-quad12": ("em_quad12_T20", LANES_QUAD, "quad", {"fused": "quad", "two_pass": "wave"}, "quad"),
    "grid-pendulum": ("gh3_pendulum_T40", 64, "grid", {"fused": "grid"}, "grid"),
}
LANE_DCP = ("em_dcp_T60", -1, "lane", {"fused": "lane"}, "lane")  # (per-trajectory horizons run on the one-lane kernels only)

# Families that report a LATER stage than the twin's because the stage the twin names does not exist in their form of the cell.
# (family, model, twin's reason, injection) -> (reported reason, the code that justifies it). The cell always equals the twin's;
# an entry never stands for status 0. The injection is part of the key because WHICH later stage first sees the indefinite matrix
# depends on the entry that is negative: sig_z = S0 + alpha xi absorbs an action variance of -1 (alpha xi_uu = 100 for this
# model's R = 0.01 I) but not a state variance of -1 (alpha xi_xx = 0.1 ... 10), so the first is caught by chol(sig_xu1_f) and the
# second by the observation update.
_GROUP_ID_OBS = ("csrc/i2c_group.hpp, forward cell, stage 2: `if (OBS_ID && c.rule_xu.unit)` takes the moments of an identity observation "
                 "as blocks of the prior joint; g_chol<D>(.., L0, ..) -- flag_stage order 1, the only factorisation of sig_xu0_f -- is "
                 "in the else branch and is never executed for this model under the unit rule")
COARSER_BY_CONSTRUCTION = {
    ("group", "Quadrotor12", 1, "a:sig_x0"): (3, _GROUP_ID_OBS),
    ("group", "Quadrotor12", 1, "d:prior_uu[5]"): (4, _GROUP_ID_OBS),
}


def sym(n):
    return n * (n + 1) // 2


def _case(name, horizon=T):
    return parity.with_horizon(load_case(name), horizon)


def _engine(row, lib, device, B, horizon=T, keep_prior=True, case_over=None, **kw):
    name, lanes = row[:2]
    g = _case(name, horizon)
    if case_over:
        g = Case({**g, **case_over})
    meta = g.meta
    x0, mu_u = parity.batched_inputs(g, B)
    eng = pkg.BatchedI2c(parity.product_model(g), meta["T"], g.get("Q"), g["R"], g.get("Qf"), meta["alpha"], meta["tol"], mu_u, g["sig_u"],
                         quad=tuple(meta["quad"]), x0=x0, device=device, lib=lib, keep_prior=keep_prior,
                         inference=meta.get("inference", "cubature"), gh_degree=meta.get("gh_degree"), group_lanes=lanes, **kw)
    return eng


def _oracle(row, B, b, horizon=T, case_over=None):
    """The B = 1 oracle of trajectory b of the batch of B."""
    g = _case(row[0], horizon)
    if case_over:
        g = Case({**g, **case_over})
    x0, mu_u = parity.batched_inputs(g, B)
    return oracle_from_case(Case({**g, "mu_u": mu_u[b]}), x0=x0[b: b + 1])


def _word(eng, b):
    s = int(eng.status[b])
    return (s >> 16, (s & 0xFFFF) - 1) if s else None


def _buf(eng, name):
    """A buffer of the engine with the trajectory index LAST, whatever its storage layout."""
    t = getattr(eng, name)
    if name == "fwd" and eng.fwd_trajectory_major:
        t = t.permute(0, 2, 1)
    return t


def _keep(eng, bad):
    return torch.as_tensor(np.delete(np.arange(eng.B), list(bad)), device=eng.device)


def _neighbours_identical(eng, clean, bad, names):
    keep = _keep(eng, bad)
    for n in names:
        if getattr(eng, n) is None:
            continue
        a, c = _buf(eng, n), _buf(clean, n)
        assert torch.equal(a[..., keep], c[..., keep]), f"{n}: a neighbour of the failed trajectory differs from the clean run"


def _expected(family, model, twin, inj=None):
    """The word a family must report for the twin's answer: the twin's, or -- COARSER_BY_CONSTRUCTION -- a later stage of the same cell."""
    entry = COARSER_BY_CONSTRUCTION.get((family, model, twin[0], inj))
    return (entry[0], twin[1]) if entry else twin


def test_coarser_table_is_well_formed():
    order = {2: 0, 1: 1, 3: 2, 4: 3, 5: 4, 6: 5}  # execution order of the forward cell's stages by reason (flag_stage, i2c_cell.hpp)
    for (family, model, reason, inj), (reported, why) in COARSER_BY_CONSTRUCTION.items():
        assert reported != 0 and order[reported] > order[reason] and ".hpp" in why


_TWIN = {}


def _twin(key, make):
    if key not in _TWIN:
        _TWIN[key] = make()
    return _TWIN[key]


def _report(row_id, inj, device, b, twin, word):
    print(f"WORD {row_id:15s} {inj:22s} {device:4s} b={b:<3d} twin={twin} word={word}")


# ---- injections of the forward sweep ------------------------------------------------------------------------------------------------
# name -> (clean EM iterations first, poison the engine (eng, b), poison the B = 1 oracle (o))
def _e_sig_x0(eng, b):
    eng.sig_x0[0, b] = -1.0


def _o_sig_x0(o):
    o.sig_x0[0, 0, 0] = -1.0


def _e_alpha(eng, b):
    eng.alpha[b] = -eng.alpha[b]


def _o_alpha(o):
    o.alpha = -o.alpha


def _e_prior_xx(eng, b):
    eng.post[5, eng.d, b] = -1.0  # packed (0, 0) of the prior joint of cell 5


def _o_prior_xx(o):
    o.sig_xu0_f[0, 5, 0, 0] = o.sig_xu0_m[0, 5, 0, 0] = -1.0


def _e_prior_uu(eng, b):
    eng.post[5, eng.d + sym(eng.d) - 1, b] = -1.0  # the last packed entry: (d - 1, d - 1), an action variance


def _o_prior_uu(o):
    o.sig_xu0_f[0, 5, -1, -1] = o.sig_xu0_m[0, 5, -1, -1] = -1.0


FORWARD = {
    "a:sig_x0": (0, _e_sig_x0, _o_sig_x0),
    "b:alpha": (0, _e_alpha, _o_alpha),
    "c:prior_xx[5]": (1, _e_prior_xx, _o_prior_xx),
    "d:prior_uu[5]": (1, _e_prior_uu, _o_prior_uu),
}
LEARN_WRITES = ("fwd", "post", "xm", "zpost", "term_stats", "alpha", "prior_out", "cell_stats")


def _forward_twin(row_id, inj, B, b, call):
    n_clean, _, poison = FORWARD[inj]

    def make():
        o = _oracle(ROWS[row_id], B, b)
        for _ in range(n_clean):
            o.learn_msgs()
        poison(o)
        return failure_twin.first_failure(o, getattr(type(o), call))
    return _twin((row_id, inj, b, call), make)


def _failed_rows(eng, clean, b, cell, name="fwd"):
    """Trajectory b of a per-cell buffer: bit-identical to the clean run before `cell`, non-finite in every cell from it on."""
    a, c = _buf(eng, name)[..., b], _buf(clean, name)[..., b]
    assert torch.equal(a[:cell], c[:cell]), f"{name}: the failed trajectory differs from the clean run BEFORE cell {cell}"
    for t in range(cell, a.shape[0]):
        assert not torch.isfinite(a[t]).all(), f"{name}: the failed trajectory is finite in cell {t} >= {cell}"


def _forward_case(lib, device, row_id, inj, call, B, bad, sticky=False):
    """call: "forward_sweep", "learn_msgs" (sweep by sweep) or "learn" (the coupled i2c_learn kernels). sticky: first the same call
    on a third engine whose status already holds a word everywhere -- it survives (forward_sweep does not touch its inputs: after
    status.zero_() the same engine records the new failure and is the one that is checked)."""
    row = ROWS[row_id]
    n_clean, poison, _ = FORWARD[inj]
    coupled = call == "learn"
    clean, eng = (_engine(row, lib, device, B, keep_prior=not coupled) for _ in range(2))
    assert eng.forward_family == row[2] and eng.backward_family == row[3][eng.backward_schedule]
    for e in (clean, eng):
        for _ in range(n_clean):
            e.learn_msgs()
    assert eng.failures() == []
    for b in bad:
        poison(eng, b)
    if sticky:
        old = eng if call == "forward_sweep" else _engine(row, lib, device, B, keep_prior=not coupled)
        if old is not eng:
            for _ in range(n_clean):
                old.learn_msgs()
            for b in bad:
                poison(old, b)
        old.status.fill_(STALE)
        old.learn(1) if coupled else getattr(old, call)()
        assert (old.status == STALE).all(), (row_id, inj, call)
        old.status.zero_()
    for e in (clean, eng):
        e.learn(1) if coupled else getattr(e, call)()
    assert clean.failures() == []
    assert [f[0] for f in eng.failures()] == list(bad), eng.failures()
    model = type(eng.sys).__name__
    for b in bad:
        twin = _forward_twin(row_id, inj, B, b, "forward_sweep" if call == "forward_sweep" else "learn_msgs")
        _report(row_id, inj + "/" + call, device, b, twin, _word(eng, b))
        assert twin is not None
        assert _word(eng, b) == _expected(row[2], model, twin, inj), (row_id, inj, call, b, _word(eng, b), twin)
        _failed_rows(eng, clean, b, twin[1])
        if call != "forward_sweep":
            assert not torch.isfinite(eng.post[..., b]).all()
    _neighbours_identical(eng, clean, bad, ("fwd", "prior_out") if call == "forward_sweep" else LEARN_WRITES)
    return eng, clean


FWD_CASES = [(r, i, c) for r in ROWS for i in FORWARD for c in (("learn_msgs",) if i == "a:sig_x0" else ("forward_sweep",))] + \
            [(r, i, c) for r in ROWS for i in ("c:prior_xx[5]", "d:prior_uu[5]") for c in ("learn",)]


@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id,inj,call", FWD_CASES)
def test_forward_words_cpu(row_id, inj, call, B, bad):
    _forward_case(hostsim.load(), "cpu", row_id, inj, call, B, bad, sticky=B == 6)


@pytest.mark.gpu
@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id,inj,call", FWD_CASES)
def test_forward_words_gpu(row_id, inj, call, B, bad):
    _forward_case(None, "cuda", row_id, inj, call, B, bad, sticky=B == 6)


# ---- e / f: the prediction covariance and the terminal update, whole batch ----------------------------------------------------------
def _negated_noise(sig_eta):
    """-(sig_eta + I): the plain -sig_eta leaves the Gauss-Hermite row's sig3 at min eig = -9e-7 max|eig|, inside the twin's guard
    band (the spread of the dynamics' sigma points nearly cancels a process noise of 1e-6 ... 1e-4); this one is negative by 1."""
    sig_eta = np.asarray(sig_eta, float)
    return -(sig_eta + np.eye(sig_eta.shape[0]))


def _whole_batch_case(lib, device, row_id, what, B, horizon=T, horizons=None, row=None):
    """what = "e": sig_eta := -(sig_eta + I) (reason 5 at the first cell); "e-last": the same over ONE cell without a terminal cost, so
    that the only cell is the last one and its prediction is factored by the epilogue of the quad forward sweep; "f": Qf := -Qf
    (reason 6 at the trajectory's own last cell, also with per-trajectory horizons). Every trajectory fails: no neighbours."""
    row = row or ROWS[row_id]
    g = _case(row[0], horizon)
    over = {"Qf": -g["Qf"]} if what == "f" else {}
    kw = {} if horizons is None else {"horizons": horizons}
    if what == "e-last":
        eng, clean = (_engine(row, lib, device, B, horizon, case_over={"Qf": None}) for _ in range(2))
        assert not eng.has_Qf
    else:
        eng, clean = _engine(row, lib, device, B, horizon, case_over=over, **kw), _engine(row, lib, device, B, horizon, **kw)
    assert eng.forward_family == row[2]
    if what != "f":
        eng.sys.sig_eta = _negated_noise(eng.sys.sig_eta)
        eng.refresh_problem()
    eng.forward_sweep()
    clean.forward_sweep()
    assert clean.failures() == [] and [f[0] for f in eng.failures()] == list(range(B)), eng.failures()
    model = type(eng.sys).__name__
    for b in sorted({0, 2, B - 1} if horizons is None else set(range(B))):
        Tb = horizon if horizons is None else int(horizons[b])

        def make(b=b, Tb=Tb):
            o = _oracle(row, B, b, Tb, case_over={**over, **({"Qf": None} if what == "e-last" else {})})
            if what != "f":
                o.sig_eta = _negated_noise(o.sig_eta)
            return failure_twin.first_failure(o, type(o).forward_sweep)
        twin = _twin((row_id, what, b, Tb, horizon), make)
        _report(row_id, what + (f"/T_b={Tb}" if horizons is not None else ""), device, b, twin, _word(eng, b))
        assert twin == ((6, Tb - 1) if what == "f" else (5, 0))  # (what the injection is FOR: anything else is a wrong injection)
        assert _word(eng, b) == _expected(row[2], model, twin), (row_id, what, b, _word(eng, b), twin)
        a, c = _buf(eng, "fwd")[..., b][:Tb], _buf(clean, "fwd")[..., b][:Tb]  # (rows beyond a trajectory's own horizon are not written)
        assert torch.equal(a[:twin[1]], c[:twin[1]]) and all(not torch.isfinite(a[t]).all() for t in range(twin[1], Tb))


@pytest.mark.parametrize("what", ["e", "e-last", "f"])
@pytest.mark.parametrize("row_id", list(ROWS))
def test_whole_batch_words_cpu(row_id, what):
    _whole_batch_case(hostsim.load(), "cpu", row_id, what, 6, horizon=1 if what == "e-last" else T)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["e", "e-last", "f"])
@pytest.mark.parametrize("row_id", list(ROWS))
def test_whole_batch_words_gpu(row_id, what):
    _whole_batch_case(None, "cuda", row_id, what, 70, horizon=1 if what == "e-last" else T)


def _last_prediction_case(lib, device, row_id, B, bad):
    """Injection e in the LAST of eight cells, first seven clean: a NaN target of cell 7 in the poisoned trajectories. The
    covariances of that cell's update do not depend on the target, so its stages 0..3 pass; the updated MEAN is NaN, the dynamics'
    sigma points with it, and the prediction covariance is the first matrix that is not positive definite: (5, 7). No terminal cost,
    so that the quad forward sweep factors that prediction in its epilogue (the `T - 1` there, against the `t - 1` of the cells)."""
    row = ROWS[row_id]
    g = _case(row[0])
    nz = int(np.asarray(parity.product_model(g).zg).size)
    z = np.tile(np.asarray(parity.product_model(g).zg, float).reshape(1, 1, nz), (B, T, 1))
    zbad = z.copy()
    for b in bad:
        zbad[b, T - 1, 0] = np.nan
    clean, eng = (_engine(row, lib, device, B, case_over={"Qf": None}, z_traj=zz) for zz in (z, zbad))
    assert eng.forward_family == row[2] and not eng.has_Qf
    for e in (clean, eng):
        e.forward_sweep()
    assert clean.failures() == [] and [f[0] for f in eng.failures()] == list(bad), eng.failures()
    for b in bad:
        def make(b=b):
            gg = Case({**g, "Qf": None})
            x0, mu_u = parity.batched_inputs(gg, B)
            o = oracle_from_case(Case({**gg, "mu_u": mu_u[b]}), x0=x0[b: b + 1], z_traj=zbad[b: b + 1])
            return failure_twin.first_failure(o, type(o).forward_sweep)
        twin = _twin((row_id, "e-cell7", b), make)
        _report(row_id, "e:z[7]=nan/forward_sweep", device, b, twin, _word(eng, b))
        assert twin == (5, T - 1)
        assert _word(eng, b) == twin, (row_id, b, _word(eng, b), twin)
        _failed_rows(eng, clean, b, T - 1)
    _neighbours_identical(eng, clean, bad, ("fwd", "prior_out"))


@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id", list(ROWS))
def test_last_cell_prediction_words_cpu(row_id, B, bad):
    _last_prediction_case(hostsim.load(), "cpu", row_id, B, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id", list(ROWS))
def test_last_cell_prediction_words_gpu(row_id, B, bad):
    _last_prediction_case(None, "cuda", row_id, B, bad)


HORIZONS = [1, 2, 4, 8, 8, 3]


@pytest.mark.parametrize("row_id", ["lane-pendulum", "lane-dcp"])
def test_terminal_word_names_each_trajectorys_own_last_cell_cpu(row_id):
    _whole_batch_case(hostsim.load(), "cpu", row_id, "f", 6, horizons=HORIZONS, row=LANE_DCP if row_id == "lane-dcp" else None)


@pytest.mark.gpu
@pytest.mark.parametrize("row_id", ["lane-pendulum", "lane-dcp"])
def test_terminal_word_names_each_trajectorys_own_last_cell_gpu(row_id):
    _whole_batch_case(None, "cuda", row_id, "f", 6, horizons=HORIZONS, row=LANE_DCP if row_id == "lane-dcp" else None)


# ---- g: the backward sweep under every schedule --------------------------------------------------------------------------------------
def _poison_fwd(eng, b):
    _buf(eng, "fwd")[5, eng.d, b] = -1.0  # sig_xu1_f[0][0] of cell 5 (the view is layout-blind: fwd_trajectory_major on the wave rows)


BWD_WRITES = ("post", "xm", "zpost", "cell_stats", "term_stats")
BWD_CASES = [(r, s) for r in ROWS for s in ROWS[r][3]]


def _backward_twin(row_id, B, b):
    def make():
        o = _oracle(ROWS[row_id], B, b)
        o.forward_sweep()
        o.sig_xu1_f[0, 5, 0, 0] = -1.0
        return failure_twin.first_failure(o, type(o).backward_sweep), failure_twin.posterior_not_pd_cells(o)
    return _twin((row_id, "g", b), make)


def _backward_case(lib, device, row_id, schedule, B, bad, sticky=False):
    row = ROWS[row_id]
    clean, eng = (_engine(row, lib, device, B, backward_mode=schedule) for _ in range(2))
    assert eng.backward_schedule == schedule and eng.forward_family == row[2] and eng.backward_family == row[3][schedule]
    for e in (clean, eng):
        e.forward_sweep()
    for b in bad:
        _poison_fwd(eng, b)
    if sticky:
        eng.status.fill_(STALE)
        eng.backward_sweep()
        assert (eng.status == STALE).all()
        eng.status.zero_()
    eng.backward_sweep()
    clean.backward_sweep()
    assert clean.failures() == [] and [f[0] for f in eng.failures()] == list(bad), eng.failures()
    for b in bad:
        twin, cells = _backward_twin(row_id, B, b)
        _report(row_id, "g:fwd[5]/" + schedule, device, b, (twin, cells), _word(eng, b))
        assert twin == (7, 5) and 5 in cells
        word = _word(eng, b)
        if schedule == "fused":  # sequential: the first failing cell in sweep order (T - 1 down to 0)
            assert word == twin, (row_id, schedule, b, word, twin)
        else:  # cells processed concurrently: reason 7 and A failing cell of this trajectory
            assert word[0] == 7 and word[1] in cells, (row_id, schedule, b, word, cells)
        p, c = eng.post[..., b], clean.post[..., b]
        for t in cells:
            assert not torch.isfinite(p[t]).all(), f"post: the failed trajectory is finite in cell {t}"
        if schedule == "fused":
            assert torch.equal(p[6:], c[6:])  # before the failing cell in sweep order
            for t in range(0, 6):
                assert not torch.isfinite(p[t]).all(), f"post: the failed trajectory is finite in cell {t} <= 5"
    _neighbours_identical(eng, clean, bad, BWD_WRITES)


@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id,schedule", BWD_CASES)
def test_backward_words_cpu(row_id, schedule, B, bad):
    _backward_case(hostsim.load(), "cpu", row_id, schedule, B, bad, sticky=B == 6)


@pytest.mark.gpu
@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id,schedule", BWD_CASES)
def test_backward_words_gpu(row_id, schedule, B, bad):
    _backward_case(None, "cuda", row_id, schedule, B, bad, sticky=B == 6)


# ---- h: closed-loop propagation -------------------------------------------------------------------------------------------------------
def _propagate_twin(row_id, B, b):
    def make():
        o = _oracle(ROWS[row_id], B, b)
        o.learn_msgs()
        o.propagate()
        o.sig_xu0_m[0, 5, -1, -1] = -10.0
        return failure_twin.first_failure(o, type(o).propagate)
    return _twin((row_id, "h", b), make)


def _propagate_case(lib, device, row_id, B, bad, sticky=False):
    row = ROWS[row_id]
    clean, eng = (_engine(row, lib, device, B) for _ in range(2))
    assert (eng.forward_family, eng.backward_family, eng.kernel_family("propagate")) == (row[2], row[3][eng.backward_schedule], row[4])
    for e in (clean, eng):
        e.learn_msgs()
        e.propagate()
    assert eng.failures() == []
    for b in bad:
        eng.post[5, eng.d + sym(eng.d) - 1, b] = -10.0  # the posterior's last action variance of cell 5 (sigK is not read: i2c_cell.hpp, propagate_body)
    if sticky:
        eng.status.fill_(STALE)
        eng.propagate()
        assert (eng.status == STALE).all()
        eng.status.zero_()
    eng.propagate()
    assert [f[0] for f in eng.failures()] == list(bad), eng.failures()
    for b in bad:
        twin = _propagate_twin(row_id, B, b)
        _report(row_id, "h:post_uu[5]/" + eng.kernel_family("propagate"), device, b, twin, _word(eng, b))
        assert twin == (8, 5)
        assert _word(eng, b) == twin, (row_id, b, _word(eng, b), twin)
        _failed_rows(eng, clean, b, 5, "prop")
    _neighbours_identical(eng, clean, bad, ("prop", "prop_stats"))


@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id", list(ROWS))
def test_propagate_words_cpu(row_id, B, bad):
    _propagate_case(hostsim.load(), "cpu", row_id, B, bad, sticky=B == 6)


@pytest.mark.gpu
@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id", list(ROWS))
def test_propagate_words_gpu(row_id, B, bad):
    _propagate_case(None, "cuda", row_id, B, bad, sticky=B == 6)


# ---- i: the filter step ---------------------------------------------------------------------------------------------------------------
FILTER_ROWS = {"lane-pendulum": ("PendulumKnown", "mpc_pendulum_ff", 0, "lane"), "lane-planar": ("PlanarQuadrotor", "mpc_quadrotor_fb", 0, "lane"),
               "quad-quad12": ("Quadrotor12", "mpc_quad12_fb", 0, "quad"), "group-quad12": ("Quadrotor12", "mpc_quad12_fb", 16, "group")}


def _filter_case(lib, device, row_id, B, bad):
    from oracle.models_numpy import make_model
    from test_mpc import _policy

    model_name, golden, lanes, family = FILTER_ROWS[row_id]
    g = load_case(golden)
    om = make_model(model_name)
    nx, nu = om.dim_x, om.dim_u
    rng = np.random.default_rng(3)
    ny = om.measure(np.zeros((1, nx))).shape[-1]
    mu = np.asarray(om.x0) + 0.1 * rng.normal(size=(B, nx))
    A = rng.normal(size=(B, nx, nx))
    cov = 1e-3 * (A @ np.swapaxes(A, -1, -2)) + 1e-5 * np.eye(nx)
    u = rng.normal(size=(B, nu)) + (om.u_max / 4 if hasattr(om, "u_max") else 0.0)
    sig_zeta = np.diag(10.0 ** rng.uniform(-5, -2, size=ny))
    y = om.measure(mu) + 0.01 * rng.normal(size=(B, ny))
    bad_cov = cov.copy()
    for b in bad:
        bad_cov[b, 0, 0] = -1.0
    engines = []
    for c in (cov, bad_cov):
        _, i2c, _pol = _policy(g, lib, device, batch=B, group_lanes=lanes)
        e = i2c.engine
        assert e.kernel_family("filter") == family
        e.set_initial_state(mu, c)
        engines.append(e)
    clean, eng = engines
    to = lambda a: torch.as_tensor(np.array(a.T, order="C"), dtype=eng.dtype, device=eng.device)  # noqa: E731
    yt, ut = to(y), to(u)
    eng.status.fill_(STALE)
    eng.ckf_filter(yt, ut, sig_zeta)
    assert (eng.status == STALE).all()
    eng.status.zero_()
    eng.set_initial_state(mu, bad_cov)
    eng.ckf_filter(yt, ut, sig_zeta)
    clean.ckf_filter(yt, ut, sig_zeta)
    assert clean.failures() == [] and [f[0] for f in eng.failures()] == list(bad), eng.failures()
    for b in range(B):
        twin = failure_twin.ckf_first_failure(om, mu[b], bad_cov[b], u[b], sig_zeta)
        assert twin == ((9, 0) if b in bad else None)
        if b in bad:
            _report(row_id, "i:cov[0][0]/filter", device, b, twin, _word(eng, b))
            assert _word(eng, b) == twin
            assert not torch.isfinite(eng.sig_x0[:, b]).all()
    _neighbours_identical(eng, clean, bad, ("x0", "sig_x0"))


@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id", list(FILTER_ROWS))
def test_filter_words_cpu(row_id, B, bad):
    _filter_case(hostsim.load(), "cpu", row_id, B, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("row_id", list(FILTER_ROWS))
def test_filter_words_gpu(row_id, B, bad):
    _filter_case(None, "cuda", row_id, B, bad)


# ---- Linearize rows: no twin (module docstring); the invariants, and the reasons include/i2c_hip.h documents -------------------------
LIN_ROWS = {"lin-lane": ("lin_pendulum_T100", 0, "lane", {"fused": "lane"}, "lane"), "lin-wave": ("lin_quad12_T20", 0, "wave", {"fused": "wave"}, "quad")}
LIN_PINNED = {"b:alpha": (3, 0), "c:prior_xx[5]": (2, 5), "g:fwd[5]": (7, 5), "t:Qf": (6, T - 1)}


def _linearize_case(lib, device, row_id, what, B, bad):
    row = LIN_ROWS[row_id]
    over = {"Qf": -_case(row[0])["Qf"]} if what == "t:Qf" else None  # Linearize applies the terminal update in the BACKWARD sweep
    if over:
        bad = tuple(range(B))
    clean, eng = _engine(row, lib, device, B, backward_mode="fused"), _engine(row, lib, device, B, backward_mode="fused", case_over=over)
    assert (eng.forward_family, eng.backward_family, eng.backward_schedule) == (row[2], row[2], "fused")
    forward = what in FORWARD
    for e in (clean, eng):
        for _ in range(FORWARD[what][0] if forward else 0):
            e.learn_msgs()
        if not forward:
            e.forward_sweep()
    assert eng.failures() == []
    for b in bad:
        if forward:
            FORWARD[what][1](eng, b)
        elif what == "g:fwd[5]":
            _poison_fwd(eng, b)
    call = "forward_sweep" if forward else "backward_sweep"
    eng.status.fill_(STALE)
    getattr(eng, call)()
    assert (eng.status == STALE).all()
    eng.status.zero_()
    for e in (clean, eng):
        getattr(e, call)()
    assert clean.failures() == [] and [f[0] for f in eng.failures()] == list(bad), eng.failures()
    for b in bad[:3]:
        _report(row_id, what, device, b, "pinned " + str(LIN_PINNED[what]), _word(eng, b))
        assert _word(eng, b) == LIN_PINNED[what], (row_id, what, b, _word(eng, b))
        if forward:
            _failed_rows(eng, clean, b, LIN_PINNED[what][1])
        else:
            assert not torch.isfinite(eng.post[..., b]).all()
    _neighbours_identical(eng, clean, bad, ("fwd", "prior_out") if forward else BWD_WRITES)


@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("what", list(LIN_PINNED))
@pytest.mark.parametrize("row_id", list(LIN_ROWS))
def test_linearize_words_cpu(row_id, what, B, bad):
    _linearize_case(hostsim.load(), "cpu", row_id, what, B, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("B,bad", SHAPES)
@pytest.mark.parametrize("what", list(LIN_PINNED))
@pytest.mark.parametrize("row_id", list(LIN_ROWS))
def test_linearize_words_gpu(row_id, what, B, bad):
    _linearize_case(None, "cuda", row_id, what, B, bad)
