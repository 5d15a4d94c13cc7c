"""TEST INFRASTRUCTURE: where would the reference have raised?

A plain numpy answer to "which factorisation of which cell is the first whose matrix is not positive definite", for
tests/test_failure_words.py. Built on oracle.i2c_numpy.I2cOracle with B = 1 (one oracle per trajectory): the oracle's two
factorisation entry points -- SigmaPointTransform.points and _sym_solve -- are wrapped, and the POSITION of a call inside
_forward_cell / _backward_cell / _propagate_cell / _pdf_ratio gives the reason code of include/i2c_hip.h (the order is the one
oracle/i2c_numpy.py's cells execute, which is the documented order of csrc/i2c_cell.hpp's flag_stage):

    forward cell    pdf-ratio S (feedback cells)                      2
                    S0 (points of the prior joint)                    1
                    sig_z + sig_xi (_sym_solve)                       3
                    S1 (points of the updated joint)                  4
                    sig3 (_sym_solve)                                 5
                    terminal: points(sig3), sig_zt + sig_xi_terminal  6
    backward cell   end of chain: points(sig3m), tempered solves      6
                    sig_m (points, and the solve against its xx block) 7
    propagate cell  pdf-ratio S, the joint (points, twice)            8
    (the KL factors of covariance control, also reason 8, are NOT judged: I2cOracle.mvn_kl calls numpy in line)

Positive definiteness is decided independently of any Cholesky, by np.linalg.eigvalsh of the symmetrised matrix. The verdict
carries a CONDITION, not a tolerance: the failing matrix must have  min eig < -1e-6 max|eig|  (or be non-finite), and every
matrix factored before it  min eig > 1e-9 max|eig|;  a matrix in between raises Undecided -- the injection has to be chosen so
that rounding can flip neither verdict. The two pdf-ratio matrices of the forward cell do not pass through the wrapped entry
points (the oracle calls numpy directly): they are restated here from the same operands.
"""
import contextlib

import numpy as np

import oracle.i2c_numpy as onp

NEG, POS = -1e-6, 1e-9


class Undecided(AssertionError):
    """A matrix whose smallest eigenvalue is too close to zero for the verdict to survive rounding."""


class _Raised(Exception):
    def __init__(self, reason, cell):
        self.reason, self.cell = reason, cell


def is_pd(S, what=""):
    """True / False by the eigenvalues of the symmetrised matrix; Undecided inside the guard band. Non-finite: not PD."""
    S = np.asarray(S, float)
    S = S.reshape(S.shape[-2:]) if S.ndim > 2 else S
    if not np.all(np.isfinite(S)):
        return False
    ev = np.linalg.eigvalsh(0.5 * (S + S.T))
    top = float(np.max(np.abs(ev)))
    if top == 0.0:
        return False
    lo = float(ev[0]) / top
    if lo < NEG:
        return False
    if lo > POS:
        return True
    raise Undecided(f"{what}: min eig / max|eig| = {lo:.3e} lies in [{NEG:.0e}, {POS:.0e}]")


class FailureTwin:
    """Wraps ONE I2cOracle (B = 1). Inside `watching()` every factorisation of the oracle is judged by is_pd first."""

    def __init__(self, oracle):
        assert oracle.B == 1
        self.o = oracle
        self.sweep, self.cell, self.n_points, self.n_solve = None, -1, 0, 0

    # -- reasons by position ---------------------------------------------------------------------------------------------------
    def _reason(self, kind, tf=None):
        if self.sweep == "propagate":
            return 8
        if self.sweep == "backward":
            return 6 if (kind == "points" and tf is self.o.tf_x) else 7
        if kind == "points":
            if tf is self.o.tf_x:
                return 6
            r = (1, 4)[self.n_points]
            self.n_points += 1
            return r
        r = (3, 5, 6)[self.n_solve]
        self.n_solve += 1
        return r

    def _judge(self, S, reason, what):
        if not is_pd(S, f"{what} (reason {reason}, cell {self.cell})"):
            raise _Raised(reason, self.cell)

    @contextlib.contextmanager
    def watching(self):
        o, twin = self.o, self
        saved = dict(solve=onp._sym_solve, fc=o._forward_cell, bc=o._backward_cell, pc=o._propagate_cell, pr=o._pdf_ratio,
                     pxu=o.tf_xu.points, px=o.tf_x.points)

        def sym_solve(A, Bm):
            if twin.sweep is not None:
                twin._judge(A, twin._reason("solve"), "_sym_solve")
            return saved["solve"](A, Bm)

        def points_of(tf, orig):
            def points(m, S):
                twin._judge(S, twin._reason("points", tf), "points")
                return orig(m, S)
            return points

        def enter(sweep, t):
            twin.sweep, twin.cell, twin.n_points, twin.n_solve = sweep, t, 0, 0

        def forward_cell(t, mu_x, sig_x):
            enter("forward", t)
            if not o.feedforward[t]:  # the pdf ratio's S = sig_xx + sig_x (i2c_numpy.py:239-243; numpy called directly there)
                twin._judge(o.sig_xu0_f[:, t, :o.nx, :o.nx] + sig_x, 2, "pdf-ratio S")
            return saved["fc"](t, mu_x, sig_x)

        def backward_cell(t, mu_end, sig_end):
            enter("backward", t)
            if mu_end is None and o.sig_x_terminal is not None:  # covariance control: the tempered solves (i2c_numpy.py:296-303)
                sig_t = o.temp[:, None, None] * o.sig_x3_f[:, t]
                for S in (o.sig_x_terminal + sig_t, sig_t, o.sig_x_terminal):
                    twin._judge(S, 6, "end-of-chain solve")
            return saved["bc"](t, mu_end, sig_end)

        def propagate_cell(t, mu_x, sig_x):
            enter("propagate", t)
            return saved["pc"](t, mu_x, sig_x)

        def pdf_ratio(mean, cov, x):
            twin._judge(cov, 8, "pdf-ratio S")
            return saved["pr"](mean, cov, x)

        onp._sym_solve = sym_solve
        o._forward_cell, o._backward_cell, o._propagate_cell, o._pdf_ratio = forward_cell, backward_cell, propagate_cell, pdf_ratio
        o.tf_xu.points, o.tf_x.points = points_of(o.tf_xu, saved["pxu"]), points_of(o.tf_x, saved["px"])
        try:
            yield self
        finally:
            onp._sym_solve = saved["solve"]
            o._forward_cell, o._backward_cell, o._propagate_cell, o._pdf_ratio = saved["fc"], saved["bc"], saved["pc"], saved["pr"]
            o.tf_xu.points, o.tf_x.points = saved["pxu"], saved["px"]
            self.sweep = None

    def first_failure(self, call):
        """Runs call(oracle) -- a sweep, or several -- under watch: (reason, cell) of the first matrix that is not positive
        definite, or None when every factorisation would have gone through."""
        with self.watching():
            try:
                call(self.o)
            except _Raised as e:
                return e.reason, e.cell
        return None


def first_failure(oracle, call):
    return FailureTwin(oracle).first_failure(call)


def posterior_not_pd_cells(o):
    """The cells whose smoothed joint sig_m is not positive definite, from the forward messages the oracle holds: the backward
    recursion (i2c_numpy.py:314-328) restated WITHOUT any factorisation -- sig_m[t] needs only J, the forward messages and the xx
    block of sig_m[t + 1] -- so that it runs through cells whose matrix the reference would have refused. For a chain without
    covariance control (the smoothed state leaving the last cell is its forward message)."""
    assert o.B == 1 and o.sig_x_terminal is None
    bad, sig3m = [], None
    for t in reversed(range(o.H)):
        if sig3m is None:
            sig3m = o.sig_x3_f[:, t]
        J = o.J_dyn[:, t]
        sig_m = o.sig_xu1_f[:, t] + J @ (sig3m - o.sig_x3_f[:, t]) @ np.swapaxes(J, -1, -2)
        if not is_pd(sig_m, f"sig_m of cell {t}"):
            bad.append(t)
        sig3m = sig_m[:, :o.nx, :o.nx]
    return sorted(bad)


def ckf_first_failure(model, mu, cov, u, sig_zeta):
    """The eigenvalue-checked restatement of the filter step (tests/test_mpc.py's _ckf_oracle; mpc.py:125-145) for ONE belief:
    (9, 0) if the belief covariance, the predicted covariance or the innovation covariance is not positive definite, else None."""
    tf = onp.SigmaPointTransform(onp.CubatureRule(1, 0, 0), model.dim_x)
    mu, cov, u = np.asarray(mu, float).reshape(1, -1), np.asarray(cov, float).reshape(1, model.dim_x, model.dim_x), np.asarray(u, float).reshape(1, -1)
    if not is_pd(cov, "belief covariance"):
        return 9, 0
    X = tf.points(mu, cov)
    XU = np.concatenate((X, np.broadcast_to(u[:, None, :], X.shape[:2] + (u.shape[-1],))), axis=-1)
    Xf = model.dynamics(XU)
    w = tf.w
    mu_f = np.einsum("p,bpi->bi", w, Xf)
    sig_f = np.einsum("p,bpi,bpj->bij", w, Xf, Xf) - mu_f[:, :, None] * mu_f[:, None, :] + w.sum() * model.sig_eta
    if not is_pd(sig_f, "predicted covariance"):
        return 9, 0
    _, sig_y, _, _, _ = tf.forward(model.measure, mu_f, sig_f)
    if not is_pd(sig_y + sig_zeta, "innovation covariance"):
        return 9, 0
    return None
