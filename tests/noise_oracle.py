"""Test-side twin for models with state-action-dependent process noise: I2cOracle with the reference's contract
`sys.forward(x_pts) -> (means, one covariance PER POINT)` -- the noise of a dynamics transform is sum_p w_p (sig_eta + Q(x_p)) with the
rule's covariance weights (quadrature.py:46-58), where I2cOracle adds W sig_eta for its constant-noise models -- and the filter step of
the MPC state estimator with the same sum (mpc.py:131-137). The model is a NumPy twin with `process_noise(xu) -> (..., nx, nx)`
(tests/noise_models.py)."""
import numpy as np

from oracle.i2c_numpy import CubatureRule, I2cOracle, SigmaPointTransform, _T, _mv, _sym_solve


class NoiseOracle(I2cOracle):
    def _dynamics_with_noise(self, m, S):
        """the dynamics transform and sum_p w_p (sig_eta + Q(x_p)) over ITS points"""
        mu3, sig_y, sig_xy, X, _ = self.tf_xu.forward(self._forward_model, m, S)
        w = self.tf_xu.w
        return mu3, sig_y, sig_xy, w.sum() * self.sig_eta + np.einsum("p,...pij->...ij", w, self.sys.process_noise(X))

    # The two methods below restate I2cOracle._forward_cell (oracle/i2c_numpy.py:228-282) and I2cOracle._propagate_cell (:346-368)
    # whole, because oracle/ is not edited and each changes ONE line of its original: `sig_noise = self.tf_xu.w.sum() * self.sig_eta`
    # (:268) and `sig3 = sig_y + self.tf_xu.w.sum() * self.sig_eta` (:366) become the sum of _dynamics_with_noise. If the oracle
    # changes, they follow; tests/test_process_noise.py::test_twin_without_the_term_is_the_oracle (Q = 0: equal bit for bit) says when.
    def _forward_cell(self, t, mu_x, sig_x):
        """I2cOracle._forward_cell with the per-point noise sum in place of W sig_eta (the one line that differs)."""
        nx = self.nx
        if self.feedforward[t]:
            mu0 = np.concatenate((mu_x, self.mu_u0_f[:, t]), axis=-1)
            S0 = np.zeros((self.B, self.d, self.d))
            S0[:, :nx, :nx] = sig_x
            S0[:, nx:, nx:] = self.sig_u0_f[:, t]
        else:
            pj_mu, pj_sig = self.mu_xu0_f[:, t], self.sig_xu0_f[:, t]
            sig_xx, sig_ux = pj_sig[:, :nx, :nx], pj_sig[:, nx:, :nx]
            S = sig_xx + sig_x
            delta = mu_x - pj_mu[:, :nx]
            maha = np.einsum("bi,bi->b", delta, np.linalg.solve(S, delta[..., None])[..., 0])
            np.linalg.cholesky(S)
            K = self.K[:, t] * np.exp(-0.5 * maha)[:, None, None]
            mu_x0_m, mu_u0_m = self.mu_xu0_m[:, t, :nx], self.mu_xu0_m[:, t, nx:]
            sig_u0_m = self.sig_xu0_m[:, t, nx:, nx:]
            mu_u = mu_u0_m + _mv(K, mu_x - mu_x0_m)
            sig_u = sig_u0_m - K @ _T(sig_ux) + K @ sig_x @ _T(K)
            self.mu_u0_f[:, t], self.sig_u0_f[:, t] = mu_u, sig_u
            mu0 = np.concatenate((mu_x, mu_u), axis=-1)
            S0 = np.concatenate((np.concatenate((sig_x, sig_x @ _T(K)), axis=-1), np.concatenate((K @ sig_x, sig_u), axis=-1)), axis=-2)
        self.mu_xu0_f[:, t], self.sig_xu0_f[:, t] = mu0, S0

        mu_z, sig_z, sig_xz, _, _ = self.tf_xu.forward(self.sys.observe, mu0, S0)
        sig_z = sig_z + self.sig_xi
        G = _sym_solve(sig_z, sig_xz)
        mu1 = mu0 + _mv(G, self.z[:, t] - mu_z)
        S1 = S0 - G @ _T(sig_xz)
        self.mu_z0_f[:, t], self.sig_z0_f[:, t] = mu_z, sig_z
        self.mu_xu1_f[:, t], self.sig_xu1_f[:, t] = mu1, S1

        mu3, sig_y, sig_xy, sig_noise = self._dynamics_with_noise(mu1, S1)
        sig3 = sig_y + sig_noise
        sig3 = (sig3 + _T(sig3)) / 2
        J = _sym_solve(sig3, sig_xy)

        if t == self.H - 1 and self.sig_xi_terminal is not None:
            mu_zt, sig_zt, sig_xzt, _, _ = self.tf_x.forward(self.sys.observe_terminal, mu3, sig3)
            sig_zt = sig_zt + self.sig_xi_terminal
            Gt = _sym_solve(sig_zt, sig_xzt)
            mu3 = mu3 + _mv(Gt, self.z_term - mu_zt)
            sig3 = sig3 - Gt @ _T(sig_xzt)
        self.mu_x3_f[:, t], self.sig_x3_f[:, t], self.J_dyn[:, t] = mu3, sig3, J
        return mu3, sig3

    def _propagate_cell(self, t, mu_x, sig_x):
        """I2cOracle._propagate_cell with the per-point noise sum in place of W sig_eta."""
        nx = self.nx
        K = self.K[:, t].copy()
        mu_x0_m, mu_u0_m = self.mu_xu0_m[:, t, :nx], self.mu_xu0_m[:, t, nx:]
        sig_x0_m, sig_u0_m = self.sig_xu0_m[:, t, :nx, :nx], self.sig_xu0_m[:, t, nx:, nx:]
        if self.feedforward[t]:
            mu_u, sig_u = mu_u0_m, sig_u0_m
        else:
            if self.use_expert_controller:
                K = K * self._pdf_ratio(mu_x0_m, sig_x0_m + sig_x, mu_x)[:, None, None]
            mu_u = mu_u0_m + _mv(K, mu_x - mu_x0_m)
            sig_u = K @ sig_x @ _T(K) + sig_u0_m - K @ sig_x0_m @ _T(K)
        mu0 = np.concatenate((mu_x, mu_u), axis=-1)
        S0 = np.concatenate((np.concatenate((sig_x, sig_x @ _T(K)), axis=-1), np.concatenate((K @ sig_x, sig_u), axis=-1)), axis=-2)
        self.mu_xu0_pf[:, t], self.sig_xu0_pf[:, t] = mu0, S0
        self.mu_z0_pf[:, t], self.sig_z0_pf[:, t], _, _, _ = self.tf_xu.forward(self.sys.observe, mu0, S0)
        mu3, sig_y, _, sig_noise = self._dynamics_with_noise(mu0, S0)
        sig3 = sig_y + sig_noise
        self.mu_x3_pf[:, t], self.sig_x3_pf[:, t] = mu3, sig3
        return mu3, sig3


def ckf_filter(model, mu, cov, u, y, sig_zeta):
    """PartiallyObservedMpcPolicy.filter (mpc.py:125-145), batched, for such a model: the predicted covariance takes
    sum_p w_p (sig_eta + Q(x_p, u)) with the applied action fixed. The estimator's rule is CubatureQuadrature(1, 0, 0)."""
    tf = SigmaPointTransform(CubatureRule(1, 0, 0), model.dim_x)
    X = tf.points(mu, cov)
    XU = np.concatenate((X, np.broadcast_to(u[:, None, :], X.shape[:2] + (u.shape[-1],))), axis=-1)
    Xf = model.dynamics(XU)
    w = tf.w
    mu_f = np.einsum("p,bpi->bi", w, Xf)
    sig_f = np.einsum("p,bpi,bpj->bij", w, Xf, Xf) - mu_f[:, :, None] * mu_f[:, None, :] + w.sum() * model.sig_eta
    sig_f = sig_f + np.einsum("p,bpij->bij", w, model.process_noise(XU))
    mu_y, sig_y, sig_xy, _, _ = tf.forward(model.measure if hasattr(model, "measure") else model.observe_terminal, mu_f, sig_f)
    sig_y = sig_y + sig_zeta
    K = _sym_solve(sig_y, sig_xy)
    return mu_f + _mv(K, y - mu_y), sig_f - K @ sig_y @ _T(K)


def sample_step(model, x, u, eps):
    """x' = f(x, u) + chol(sig_eta + Q(x, u)) eps for a batch of states (N, nx), actions (N, nu) and standard normals (N, nx)."""
    xu = np.concatenate((x, u), axis=-1)
    L = np.linalg.cholesky(model.sig_eta + model.process_noise(xu))
    return model.dynamics(xu) + _mv(L, eps)
