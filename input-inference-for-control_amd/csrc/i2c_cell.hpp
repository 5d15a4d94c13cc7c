// Per-trajectory cell math of the Gaussian i2c cubature path, one trajectory per lane.
//
// Mathematically identical to the reference's I2cCell (i2c/i2c.py:350-447, 544-610, 150-199)
// and QuadratureInference (i2c/inference/quadrature.py:15-58), but arranged for registers:
//   * sigma points are generated column by column from the Cholesky factor and consumed
//     immediately (pairwise +/- differences), so only O(d * ny) accumulators are live;
//   * covariances are accumulated in the centred, shift-by-centre-point form (no
//     sum w y y^T - m m^T cancellation); the general-weight correction terms
//     reproduce the reference's formula exactly, including its use of w_sig for the mean;
//   * the Kalman-style update uses only forward substitutions with chol(sig_z):
//        V = C^{-1} sig_xz^T,  mu += V^T C^{-1} r,  sig -= V^T V   (symmetric by construction);
//   * the controller (K, k, sigK) falls out of the Cholesky factor of the posterior joint.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "../../include/i2c_hip.h"
#include "i2c_linalg.hpp"
#include "i2c_models.hpp"
#include "i2c_random.hpp"

namespace i2c {

// Sigma-point rule for one input dimension (i2c/exp_types.py:36-49), precomputed on the host.
template <typename R> struct Rule {
  R sf;   // sqrt(dim + lam)
  R w0;   // weights_sig[0]
  R wi;   // weights_sig[1:]
  R W;    // sum of weights_sig (= 1 unless 1 - alpha^2 + beta != 0)
  int unit;  // W == 1 exactly: skip the correction terms
  // Gauss-Hermite tensor grid (i2c/exp_types.py:52-68), used by the GRID variants only: gh_degree^dim points
  // m + sqrt(2) L xi, xi in gh_x^dim, weight = prod gh_w (the 1-D weights already divided by sqrt(pi))
  int gh_degree, gh_points;
  R gh_x[I2C_MAX_GH_DEGREE], gh_w[I2C_MAX_GH_DEGREE];
};

// Per-trajectory model parameters (I2cProblem.model_params_b) are a compile-time flag carried by the model type: every kernel
// instantiated on PerTraj<M> evaluates trajectory b's functors with column b of the [NP][B] device array c.params_b; the
// kernels of M itself keep reading the batch constants c.params from the kernel-argument segment. Only models with NP > 0
// get the PerTraj instantiations (make_ops, i2c_impl.hpp).
template <class M> struct PerTraj : M {};
template <class M> struct is_per_traj : std::false_type {};
template <class M> struct is_per_traj<PerTraj<M>> : std::true_type {};
// ... and the [NP][B] array itself, a member of Consts<PerTraj<M>, R> only (an empty base otherwise: the kernel arguments of the
// shared-parameter kernels are laid out as without the feature)
template <typename R, bool PER_TRAJ> struct ParamsB {};
template <typename R> struct ParamsB<R, true> {
  const R* params_b;
};
template <class M, typename R> struct Consts : ParamsB<R, is_per_traj<M>::value> {
  static constexpr int NX = M::NX, NU = M::NU, NZ = M::NZ, NZT = M::NZT, D = NX + NU;
  static constexpr int NZT1 = NZT > 0 ? NZT : 1, NP1 = M::NP > 0 ? M::NP : 1;
  static constexpr int E_PRI = D + sym(D) + NU * NX;                        // rows the forward reads
  static constexpr int E_POST = E_PRI + NU + sym(NU);
  static constexpr int E_FWD = D + sym(D) + NX + sym(NX) + D * NX;
  static constexpr int E_XM = NX + sym(NX);
  static constexpr int E_ZPOST = NZ + sym(NZ);
  static constexpr int E_PROP = D + sym(D) + NX + sym(NX);
  static constexpr int E_TERM = 4 + NZT + sym(NZT);  // last row: plan-cost sum of the Linearize path
  int B, T;
  // Ring offset of the PERSISTENT per-cell buffers (prior/post, z, alpha_cell, feedforward): cell t lives in row
  // (t0 + t) mod T. 0 outside the MPC loop; the receding-horizon shift (mpc.py:174-181) advances it by one instead of
  // moving every row. Scratch buffers of a sweep (fwd, xm, zpost, prior_out, prop, cell_stats) are indexed by t directly.
  int t0;
  I2C_HD inline int row(const int t) const {
    const int r = t + t0;
    return r >= T ? r - T : r;
  }
  int has_Qf, has_x_terminal, z_per_cell, use_expert, terminal_cell, inference;
  int qr_diag, qf_diag;  // cost weights are diagonal: cheap closed forms in gaussian_cost
  int post_tm;           // posterior / prior buffers are trajectory-major, [T][B][E_POST] (I2cProblem.post_layout; wave-capable models)
  int fwd_tm;            // quad forward kernel only: write the forward messages trajectory-major, [T][B][E_FWD] (the wave kernels read them)
  // element e of trajectory b inside one cell block of the posterior / prior buffer: stride of e and offset of b
  I2C_HD inline long post_es() const { return post_tm ? 1L : (long)B; }
  I2C_HD inline long post_bo(const int b) const { return post_tm ? (long)b * E_POST : (long)b; }
  Rule<R> rule_xu, rule_x;
  R dtemp, tol;
  R sig_eta_w[sym(NX)];  // W(d) * sig_eta, W = sum of the d-dimensional rule's weights
  R sig_eta[sym(NX)], sig_xi0[sym(NZ)], QR[sym(NZ)], sig_xiT0[sym(NZT1)], Qf[sym(NZT1)];
  R zg[NZ], zg_term[NZT1], mu_x_term[NX], sig_x_term[sym(NX)], params[NP1];
};

// column b of the [NP][B] array: parameter i at p[i * B]
template <typename R> struct ParamCol {
  const R* p;
  long B;
};
template <class M, typename R> using ParamSrc = std::conditional_t<is_per_traj<M>::value, ParamCol<R>, const R*>;
// where trajectory b's functors read their parameters (b in [0, B): the multi-lane kernels pass a clamped index for dead lanes)
template <class M, typename R> I2C_FN ParamSrc<M, R> params_of(const Consts<M, R>& c, const int b) {
  if constexpr (is_per_traj<M>::value) return ParamCol<R>{c.params_b + b, (long)c.B};
  else return c.params;
}
// ... gathered into the functor's `const R* p` at the point of use (L1 / L2 resident, so nothing has to stay live in registers
// across a sweep: the kernels that evaluate the functors are the register-heavy ones); the shared-parameter kernels pass c.params
// itself, in code that is the same as without the feature
template <int NP, typename R> I2C_FN const R* param_ptr(const ParamCol<R>& s, R* buf) {
#pragma unroll
  for (int i = 0; i < NP; ++i) buf[i] = s.p[i * s.B];
  return buf;
}

// The three model callbacks as functors: f(x, sin(angles of x), cos(angles of x), y), parameters from params_of().
template <class M, typename R> struct ObserveF {
  ParamSrc<M, R> p;
  I2C_HD inline void operator()(const R* x, const R* sn, const R* cs, R* y) const {
    if constexpr (is_per_traj<M>::value) {
      R pb[M::NP];
      M::observe(param_ptr<M::NP>(p, pb), x, sn, cs, y);
    } else {
      M::observe(p, x, sn, cs, y);
    }
  }
};
template <class M, typename R> struct DynamicsF {
  ParamSrc<M, R> p;
  I2C_HD inline void operator()(const R* x, const R* sn, const R* cs, R* y) const {
    if constexpr (is_per_traj<M>::value) {
      R pb[M::NP];
      M::dynamics(param_ptr<M::NP>(p, pb), x, sn, cs, y);
    } else {
      M::dynamics(p, x, sn, cs, y);
    }
  }
};
template <class M, typename R> struct MeasureF {
  ParamSrc<M, R> p;
  I2C_HD inline void operator()(const R* x, const R* sn, const R* cs, R* y) const {
    if constexpr (is_per_traj<M>::value) {
      R pb[M::NP];
      M::measure(param_ptr<M::NP>(p, pb), x, sn, cs, y);
    } else {
      M::measure(p, x, sn, cs, y);
    }
  }
};
// dynamics as a function of the state only, with a known action appended (CKF prediction, mpc.py:129-131)
template <class M, typename R> struct DynamicsFixedUF {
  ParamSrc<M, R> p;
  const R* u;
  I2C_HD inline void operator()(const R* x, const R* sn, const R* cs, R* y) const {
    R xu[M::NX + M::NU];
#pragma unroll
    for (int i = 0; i < M::NX; ++i) xu[i] = x[i];
#pragma unroll
    for (int i = 0; i < M::NU; ++i) xu[M::NX + i] = u[i];
    if constexpr (is_per_traj<M>::value) {
      R pb[M::NP];
      M::dynamics(param_ptr<M::NP>(p, pb), xu, sn, cs, y);
    } else {
      M::dynamics(p, xu, sn, cs, y);
    }
  }
};
// OPTIONAL member of a functor: the state-action-dependent part of the one-step covariance at the point xu (same arguments and
// operation set as dynamics), so that the covariance of a point is sig_eta + Q(xu) -- the reference's `sys.forward(x_pts) -> (means, one
// covariance PER POINT)`, summed with the rule's covariance weights by its consumers (quadrature.py:46-58, mpc.py:131-137):
//   template <typename R> I2C_FN void process_noise(const R* p, const R* xu, const R* sn, const R* cs, R* q);  // q[sym(NX)], packed lower
// Detected, never required: a model without it compiles to what it compiled to before the member existed.
template <class M, typename R, typename = void> struct has_process_noise : std::false_type {};
template <class M, typename R>
struct has_process_noise<M, R, std::void_t<decltype(M::template process_noise<R>((const R*)nullptr, (const R*)nullptr, (const R*)nullptr,
                                                                                 (const R*)nullptr, (R*)nullptr))>> : std::true_type {};
// Q at one point, parameters as the callbacks above take them
template <class M, typename R> I2C_FN void process_noise_at(const ParamSrc<M, R>& p, const R* xu, const R* sn, const R* cs, R* q) {
  if constexpr (is_per_traj<M>::value) {
    R pb[M::NP];
    M::process_noise(param_ptr<M::NP>(p, pb), xu, sn, cs, q);
  } else {
    M::process_noise(p, xu, sn, cs, q);
  }
}
// The dynamics of such a model inside a sigma-point transform: sp_transform evaluates noise() at every point it evaluates the
// callback at -- the point and its sines / cosines exist there -- and leaves sum_p w_p Q(x_p) in q[sym(NX)] (centre point with the
// weight w0, which general weights may make negative; then the pairs in column order, times wi).
template <class M, typename R> struct DynamicsNoiseF : DynamicsF<M, R> {
  static constexpr int NQ = sym(M::NX);
  R* q;
  I2C_HD inline void noise(const R* x, const R* sn, const R* cs, R* qp) const { process_noise_at<M, R>(this->p, x, sn, cs, qp); }
};
// ... and with a known action appended (CKF prediction): Q(x_p, u)
template <class M, typename R> struct DynamicsFixedUNoiseF : DynamicsFixedUF<M, R> {
  static constexpr int NQ = sym(M::NX);
  R* q;
  I2C_HD inline void noise(const R* x, const R* sn, const R* cs, R* qp) const {
    R xu[M::NX + M::NU];
#pragma unroll
    for (int i = 0; i < M::NX; ++i) xu[i] = x[i];
#pragma unroll
    for (int i = 0; i < M::NU; ++i) xu[M::NX + i] = this->u[i];
    process_noise_at<M, R>(this->p, xu, sn, cs, qp);
  }
};
template <class F, typename = void> struct carries_noise : std::false_type {};
template <class F> struct carries_noise<F, std::void_t<decltype(F::NQ)>> : std::true_type {};

template <class M, typename R> struct ObserveTermF {
  ParamSrc<M, R> p;
  I2C_HD inline void operator()(const R* x, const R* sn, const R* cs, R* y) const {
    if constexpr (is_per_traj<M>::value) {
      R pb[M::NP];
      M::observe_terminal(param_ptr<M::NP>(p, pb), x, sn, cs, y);
    } else {
      M::observe_terminal(p, x, sn, cs, y);
    }
  }
};

// Compile-time structure of a model callback, used to skip sigma-point work that is exactly
// known: output k is either a pass-through of input lin(k) (>= 0) or nonlinear (lin(k) < 0) and
// then depends on no input with index above dep(k). (Column j of the cubature points only moves
// inputs i >= j because the Cholesky factor is lower triangular.)
template <class M> struct ObsStruct {
  I2C_HD static constexpr int lin(int k) { return M::obs_lin(k); }
  I2C_HD static constexpr int dep(int k) { return M::obs_dep(k); }
};
template <class M> struct TermStruct {
  I2C_HD static constexpr int lin(int k) { return M::term_lin(k); }
  I2C_HD static constexpr int dep(int k) { return M::term_dep(k); }
};
template <class M> struct MeasStruct {
  I2C_HD static constexpr int lin(int k) { return M::meas_lin(k); }
  I2C_HD static constexpr int dep(int k) { return M::meas_dep(k); }
};
template <int DIN> struct DenseStruct {
  I2C_HD static constexpr int lin(int) { return -1; }
  I2C_HD static constexpr int dep(int) { return DIN - 1; }
};

// Gaussian push-through  N(m, Sin = L L^T) -> (my, Sy [, Sxy])   (quadrature.py:27-58).
//   L     packed lower Cholesky factor of the input covariance Sin (DIN)
//   my    [DOUT]   weighted mean (uses weights_sig, as the reference does)
//   Sy    [sym DOUT] covariance, equal to  sum_p w_p y_p y_p^T - my my^T
//   Sxy   [DIN * DOUT] row-major cross-covariance = sum_p w_p x_p y_p^T - m my^T  (only if CROSS)
//
// With pairwise sums a_j = (y_j+ - y0) + (y_j- - y0) and differences dl_j = y_j+ - y_j-:
//   my = W y0 + wi sum_j a_j,   Sy = wi/2 sum_j (a_j a_j^T + dl_j dl_j^T) - wi^2 A A^T (+ terms in 1-W),
//   Sxy = wi sf L [dl_0 .. dl_{d-1}]^T.
// For a pass-through output a_j = 0 and dl_j = 2 sf L[i][j] exactly, so its moments are rows of
// Sin (2 wi sf^2 = 1 for every alpha, beta, kappa) and cost nothing.
// Trig of the model's angle coordinates is computed once at the mean and once per (angle, column)
// offset d = sf L[i][j], then rotated: sin(m +/- d) = s0 cd +/- c0 sd, cos(m +/- d) = c0 cd -/+ s0 sd.
// HANDOFF (a dense callback with CROSS only: every output moves with every column): Sxy is not formed. It receives the differences
// themselves, Sxy[j * DOUT + k] = dl_j[k] -- DIN * DOUT values, the cross-covariance's own count -- and whoever takes them forms
// wi sf L [dl_0 .. dl_{d-1}]^T from them and the factor (gain_from_handoff: the forward sweep's helper wave).
template <class M, class ST, int DIN, int DOUT, bool CROSS, bool UNITW = false, bool HANDOFF = false, typename R, class F>
I2C_FN void sp_transform(const Rule<R>& rule, const R* m, const R* Sin, const R* L, const F& f, R* my, R* Sy,
                         R* Sxy, const PolyTab<R>* tab = nullptr) {
  static_assert(!HANDOFF || (CROSS && ST::lin(0) < 0 && ST::dep(0) == DIN - 1 && ST::lin(DOUT - 1) < 0 && ST::dep(DOUT - 1) == DIN - 1),
                "the hand-off of the differences is the dense callback's");
  constexpr int NA = M::NA, NA1 = NA > 0 ? NA : 1;
  R s0[NA1], c0[NA1];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    if (tab)
      r_sincos(m[M::ang(a)], *tab, &s0[a], &c0[a]);
    else
      r_sincos(m[M::ang(a)], &s0[a], &c0[a]);
  }
  R y0[DOUT];
  f(m, s0, c0, y0);
  // (a functor that carries a point-dependent noise term, DynamicsNoiseF: Q at the centre, then the sum over the pairs)
  constexpr bool NOISE = carries_noise<F>::value;
  static_assert(!NOISE || (!HANDOFF && ST::lin(0) < 0 && ST::dep(0) == DIN - 1), "a noise term rides on a dense callback, whose every column is evaluated");
  R q0[NOISE ? sym(DOUT) : 1], qs[NOISE ? sym(DOUT) : 1];
  if constexpr (NOISE) {
    f.noise(m, s0, c0, q0);
#pragma unroll
    for (int i = 0; i < sym(DOUT); ++i) qs[i] = R(0);
  }
  R A[DOUT];
#pragma unroll
  for (int k = 0; k < DOUT; ++k) A[k] = R(0);
#pragma unroll
  for (int k = 0; k < sym(DOUT); ++k) Sy[k] = R(0);
  if (CROSS && !HANDOFF) {
#pragma unroll
    for (int k = 0; k < DIN * DOUT; ++k) Sxy[k] = R(0);
  }
#pragma unroll
  for (int j = 0; j < DIN; ++j) {
    // does any nonlinear output move with this column?
    bool any = false;
#pragma unroll
    for (int k = 0; k < DOUT; ++k) any = any || (ST::lin(k) < 0 && ST::dep(k) >= j);
    R a[DOUT], dl[DOUT];
    if (any) {
      // points m +/- sf L[:, j]; rows above the diagonal of L are structurally zero
      R xp[DIN], xm[DIN];
#pragma unroll
      for (int i = 0; i < DIN; ++i) {
        if (i < j) {
          xp[i] = m[i];
          xm[i] = m[i];
        } else {
          const R d = rule.sf * L[tri(i, j)];
          xp[i] = m[i] + d;
          xm[i] = m[i] - d;
        }
      }
      R sp[NA1], cp[NA1], sm[NA1], cm[NA1];
#pragma unroll
      for (int q = 0; q < NA; ++q) {
        if (M::ang(q) < j) {  // this column does not move the angle
          sp[q] = sm[q] = s0[q];
          cp[q] = cm[q] = c0[q];
        } else {
          R sd, cd;
          if (tab)
            r_sincos(rule.sf * L[tri(M::ang(q), j)], *tab, &sd, &cd);
          else
            r_sincos_small(rule.sf * L[tri(M::ang(q), j)], &sd, &cd);
          sp[q] = s0[q] * cd + c0[q] * sd;
          cp[q] = c0[q] * cd - s0[q] * sd;
          sm[q] = s0[q] * cd - c0[q] * sd;
          cm[q] = c0[q] * cd + s0[q] * sd;
        }
      }
      R yp[DOUT], ym[DOUT];
      f(xp, sp, cp, yp);
      f(xm, sm, cm, ym);
      if constexpr (NOISE) {
        R qp[sym(DOUT)], qm[sym(DOUT)];
        f.noise(xp, sp, cp, qp);
        f.noise(xm, sm, cm, qm);
#pragma unroll
        for (int i = 0; i < sym(DOUT); ++i) qs[i] += qp[i] + qm[i];
      }
#pragma unroll
      for (int k = 0; k < DOUT; ++k) {
        a[k] = (yp[k] - y0[k]) + (ym[k] - y0[k]);
        dl[k] = yp[k] - ym[k];
      }
    }
    // per-output activity in this column (all compile-time after unrolling)
#pragma unroll
    for (int k = 0; k < DOUT; ++k) {
      const bool nl_k = ST::lin(k) < 0 && ST::dep(k) >= j;
      if (ST::lin(k) >= j) dl[k] = R(2) * rule.sf * L[tri(ST::lin(k) >= j ? ST::lin(k) : j, j)];
      if (nl_k) A[k] += a[k];
#pragma unroll
      for (int l = 0; l <= k; ++l) {
        const bool nl_l = ST::lin(l) < 0 && ST::dep(l) >= j;
        const bool d_k = nl_k || ST::lin(k) >= j, d_l = nl_l || ST::lin(l) >= j;
        const bool both_lin = ST::lin(k) >= 0 && ST::lin(l) >= 0;
        if (nl_k && nl_l) Sy[tri(k, l)] += a[k] * a[l];
        if (d_k && d_l && !both_lin) Sy[tri(k, l)] += dl[k] * dl[l];
      }
      if (CROSS && HANDOFF) Sxy[j * DOUT + k] = dl[k];
      if (CROSS && !HANDOFF && nl_k) {
#pragma unroll
        for (int i = j; i < DIN; ++i) Sxy[i * DOUT + k] += L[tri(i, j)] * dl[k];
      }
    }
    sched_fence<(DIN >= 6)>();
  }
  const R hw = R(0.5) * rule.wi, w2 = rule.wi * rule.wi, cs = rule.wi * rule.sf;
  if constexpr (NOISE) {
#pragma unroll
    for (int i = 0; i < sym(DOUT); ++i) f.q[i] = rule.w0 * q0[i] + rule.wi * qs[i];
  }
#pragma unroll
  for (int k = 0; k < DOUT; ++k) {
    const R Wk = UNITW ? R(1) : rule.W;
    my[k] = ST::lin(k) >= 0 ? Wk * m[ST::lin(k) >= 0 ? ST::lin(k) : 0] : Wk * y0[k] + rule.wi * A[k];
#pragma unroll
    for (int l = 0; l <= k; ++l) {
      if (ST::lin(k) >= 0 && ST::lin(l) >= 0)
        Sy[tri(k, l)] = Sin[tri_any(ST::lin(k) >= 0 ? ST::lin(k) : 0, ST::lin(l) >= 0 ? ST::lin(l) : 0)];
      else
        Sy[tri(k, l)] = hw * Sy[tri(k, l)] - w2 * A[k] * A[l];
    }
    if (CROSS && !HANDOFF) {
#pragma unroll
      for (int i = 0; i < DIN; ++i)
        Sxy[i * DOUT + k] = ST::lin(k) >= 0 ? Sin[tri_any(i, ST::lin(k) >= 0 ? ST::lin(k) : 0)] : cs * Sxy[i * DOUT + k];
    }
  }
  if (!UNITW && !rule.unit) {  // sum of weights != 1: the reference's m m^T term no longer cancels
    const R omw = R(1) - rule.W;
    R yc[DOUT];
#pragma unroll
    for (int k = 0; k < DOUT; ++k) yc[k] = ST::lin(k) >= 0 ? m[ST::lin(k) >= 0 ? ST::lin(k) : 0] : y0[k];
#pragma unroll
    for (int k = 0; k < DOUT; ++k)
#pragma unroll
      for (int l = 0; l <= k; ++l)
        Sy[tri(k, l)] += omw * (rule.W * yc[k] * yc[l] + rule.wi * (A[k] * yc[l] + yc[k] * A[l]));
  }
}

// Kalman-style update of N(mu, S) (dimension DX) on an observation with moments
// (mz, Sz + noise, Sxz) and target zt:  i2c.py:394-403 / 435-443.
// On entry Sz already includes the observation noise. Returns false if Sz is not PD.
template <int DX, int DZ, typename R>
I2C_FN bool kalman_update(R* mu, R* S, const R* mz, R* Sz, R* Sxz, const R* zt) {
  R rinv[DZ];
  const bool ok = chol<DZ>(Sz, rinv);
  R q[DZ];
#pragma unroll
  for (int k = 0; k < DZ; ++k) q[k] = zt[k] - mz[k];
  fsub<DZ>(Sz, rinv, q);
#pragma unroll
  for (int i = 0; i < DX; ++i) {
    fsub<DZ>(Sz, rinv, &Sxz[i * DZ]);  // row i of V^T
    R v = mu[i];
#pragma unroll
    for (int k = 0; k < DZ; ++k) v += Sxz[i * DZ + k] * q[k];
    mu[i] = v;
    sched_fence<(DZ >= 8)>();
  }
#pragma unroll
  for (int i = 0; i < DX; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      R v = S[tri(i, j)];
#pragma unroll
      for (int k = 0; k < DZ; ++k) v -= Sxz[i * DZ + k] * Sxz[j * DZ + k];
      S[tri(i, j)] = v;
    }
  return ok;
}

// exp(-1/2 delta^T S^{-1} delta): the ratio N(x; m, S) / N(m; m, S) of i2c.py:369-374, 162-165.
template <int N, typename R> I2C_FN R pdf_ratio(R* S, const R* delta, bool* ok, const PolyTab<R>* tab = nullptr) {
  R rinv[N], q[N];
  *ok = chol<N>(S, rinv);
#pragma unroll
  for (int i = 0; i < N; ++i) q[i] = delta[i];
  fsub<N>(S, rinv, q);
  R maha = R(0);
#pragma unroll
  for (int i = 0; i < N; ++i) maha += q[i] * q[i];
  (void)tab;
  return r_exp(R(-0.5) * maha);
}

// Joint prior over (x, u) from the incoming state message and the previous controller
// (feedback mode: i2c.py:361-387; propagation: i2c.py:158-179). Kt = scaled gain (nu x nx).
//   mu_u = qmu_u + Kt (mu_x - qmu_x);  cross = Kt sig_x;  sig_u given by the caller.
template <int NX, int NU, typename R>
I2C_FN void joint_from_gain(const R* mu_x, const R* sig_x, const R* Kt, const R* qmu_x, const R* qmu_u,
                            const R* sig_u, R* mu0, R* S0) {
  constexpr int D = NX + NU;
#pragma unroll
  for (int i = 0; i < NX; ++i) mu0[i] = mu_x[i];
#pragma unroll
  for (int a = 0; a < NU; ++a) {
    R v = qmu_u[a];
#pragma unroll
    for (int k = 0; k < NX; ++k) v += Kt[a * NX + k] * (mu_x[k] - qmu_x[k]);
    mu0[NX + a] = v;
  }
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) S0[tri(i, j)] = sig_x[tri(i, j)];
#pragma unroll
  for (int a = 0; a < NU; ++a) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R v = R(0);
#pragma unroll
      for (int k = 0; k < NX; ++k) v += Kt[a * NX + k] * sig_x[tri_any(k, j)];
      S0[tri(NX + a, j)] = v;
    }
#pragma unroll
    for (int c = 0; c <= a; ++c) S0[tri(NX + a, NX + c)] = sig_u[tri(a, c)];
  }
  (void)D;
}

// Kt sig Kt^T (packed sym NU) for packed sym sig (NX)
template <int NX, int NU, typename R> I2C_FN void gain_quad(const R* Kt, const R* sig, R* out) {
  R KS[NU * NX];
#pragma unroll
  for (int a = 0; a < NU; ++a)
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R v = R(0);
#pragma unroll
      for (int k = 0; k < NX; ++k) v += Kt[a * NX + k] * sig[tri_any(k, j)];
      KS[a * NX + j] = v;
    }
#pragma unroll
  for (int a = 0; a < NU; ++a)
#pragma unroll
    for (int c = 0; c <= a; ++c) {
      R v = R(0);
#pragma unroll
      for (int j = 0; j < NX; ++j) v += KS[a * NX + j] * Kt[c * NX + j];
      out[tri(a, c)] = v;
    }
}

// Branch-free bookkeeping of the first failure: keeps the sweep's cells free of control flow, so that
// each cell stays one large scheduling region.
I2C_FN int note_failure(int fail, bool ok, int reason, int t) {
  return (fail == 0 && !ok) ? ((reason << 16) | (t + 1)) : fail;
}
// Cheaper bookkeeping inside a forward cell: each stage only raises a small integer (inline constants, no `fail == 0`
// test), and the first-failure status word is formed once per cell. Stages in execution order 0..5 = pdf ratio, prior
// joint, observation, updated joint, prediction, terminal update (reasons 2, 1, 3, 4, 5, 6); the FIRST failed stage has
// the largest value, and later stages of a poisoned cell cannot override it.
I2C_FN int flag_stage(int cell_bad, bool ok, int order) {
  const int v = ok ? 0 : 7 - order;
  return cell_bad > v ? cell_bad : v;
}
I2C_FN int fold_cell_failure(int fail, int cell_bad, int t) {
  const int order = 7 - cell_bad;
  const int reason = order == 0 ? 2 : (order == 1 ? 1 : order + 1);
  return (fail == 0 && cell_bad != 0) ? ((reason << 16) | (t + 1)) : fail;
}
// A temperature alpha <= 0 (or NaN) makes sig_z + alpha xi indefinite: the reference's la.solve(assume_a='pos') raises (i2c.py:398).
// Update forms that only divide by alpha take it through this, so that their factorisation fails on the NaN (one compare and select).
template <typename R> I2C_FN R positive_or_nan(const R alpha) { return alpha > R(0) ? alpha : R(__builtin_nan("")); }
// "The failed trajectory goes NaN" made explicit in what the lane, grid and group forward sweeps and the propagation kernels STORE:
// a NaN that a failed pivot leaves in the ACTION part of a factor only (the last pivot of a joint) reaches the next cell through
// the model functor alone, and a functor may drop it (the device's r_clip is v_max / v_min, which return the other operand;
// r_min / r_max / r_where_gt drop one too). On the stored value, not the carried one: a select on the state mean sits on the
// cell-to-cell dependency chain of a lone wave (measured: 1.8 % of the flagship benchmark).
template <typename R> I2C_FN R nan_if(const bool bad, const R x) { return bad ? R(__builtin_nan("")) : x; }
I2C_FN void set_status(int32_t* status, int b, int reason, int t) {
  if (status[b] == 0) status[b] = (reason << 16) | (t + 1);
}

// ------------------------------------------------------------------------------------------
// Forward sweep: one lane walks one trajectory through all T cells (i2c.py:876-880, 350-447).
// ------------------------------------------------------------------------------------------
// Gaussian push-through with a tensor-grid rule (GaussHermiteQuadrature): the same moments as sp_transform,
//   my = sum_p w_p y_p,  Sy = sum_p w_p y_p y_p^T - my my^T,  Sxy = sum_p w_p x_p y_p^T - m my^T   (quadrature.py:34-44),
// accumulated about the centre value y0 = f(m):  my = y0 + s1,  Sy = S2 - s1 s1^T,  Sxy = sum_p w_p dx_p dy_p^T
// (the weights sum to 1 and the grid is symmetric, so the terms in (1 - W) and sum_p w_p dx_p vanish to rounding).
// The point index runs through a mixed-radix odometer in registers; gh_degree^DIN points, no structure is exploited.
template <class M, int DIN, int DOUT, bool CROSS, typename R, class F>
I2C_FN void grid_transform(const Rule<R>& rule, const R* m, const R* L, const F& f, R* my, R* Sy, R* Sxy) {
  constexpr int NA = M::NA, NA1 = NA > 0 ? NA : 1;
  R sn[NA1], cs[NA1], y0[DOUT], s1[DOUT];
#pragma unroll
  for (int a = 0; a < NA; ++a) r_sincos(m[M::ang(a)], &sn[a], &cs[a]);
  f(m, sn, cs, y0);
#pragma unroll
  for (int k = 0; k < DOUT; ++k) s1[k] = R(0);
#pragma unroll
  for (int k = 0; k < sym(DOUT); ++k) Sy[k] = R(0);
  if (CROSS) {
#pragma unroll
    for (int k = 0; k < DIN * DOUT; ++k) Sxy[k] = R(0);
  }
  int dig[DIN];
#pragma unroll
  for (int i = 0; i < DIN; ++i) dig[i] = 0;
  const int deg = rule.gh_degree;
  for (int p = 0; p < rule.gh_points; ++p) {
    R xi[DIN], w = R(1);
#pragma unroll
    for (int i = 0; i < DIN; ++i) {
      R xv = rule.gh_x[0], wv = rule.gh_w[0];
#pragma unroll
      for (int q = 1; q < I2C_MAX_GH_DEGREE; ++q) {
        xv = dig[i] == q ? rule.gh_x[q] : xv;
        wv = dig[i] == q ? rule.gh_w[q] : wv;
      }
      xi[i] = xv;
      w *= wv;
    }
    R dx[DIN], x[DIN], y[DOUT];
#pragma unroll
    for (int i = 0; i < DIN; ++i) {
      R v = R(0);
#pragma unroll
      for (int j = 0; j <= i; ++j) v += L[tri(i, j)] * xi[j];
      dx[i] = rule.sf * v;
      x[i] = m[i] + dx[i];
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) r_sincos(x[M::ang(a)], &sn[a], &cs[a]);
    f(x, sn, cs, y);
#pragma unroll
    for (int k = 0; k < DOUT; ++k) y[k] -= y0[k];
#pragma unroll
    for (int k = 0; k < DOUT; ++k) {
      const R wy = w * y[k];
      s1[k] += wy;
#pragma unroll
      for (int l = 0; l <= k; ++l) Sy[tri(k, l)] += wy * y[l];
      if (CROSS) {
#pragma unroll
        for (int i = 0; i < DIN; ++i) Sxy[i * DOUT + k] += dx[i] * wy;
      }
    }
    // odometer: dig[0] is the fastest digit
    bool carry = true;
#pragma unroll
    for (int i = 0; i < DIN; ++i) {
      const int nd = dig[i] + (carry ? 1 : 0);
      carry = nd >= deg;
      dig[i] = carry ? 0 : nd;
    }
  }
#pragma unroll
  for (int k = 0; k < DOUT; ++k) my[k] = y0[k] + s1[k];
#pragma unroll
  for (int k = 0; k < DOUT; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) Sy[tri(k, l)] -= s1[k] * s1[l];
}

// The same transform with the grid UNROLLED at compile time (degree DEG, DIN <= 3: 27 / 64 points for the pendulum-sized models),
// axis 0 outermost. What the run-time odometer above cannot exploit:
//   * L is lower triangular: axis j only moves the coordinates i >= j, so the offsets of a point are built level by level
//     (one multiply-add per coordinate and level instead of a triangular product per point);
//   * an angle coordinate with input index ia is fixed once the axes 0 .. ia are: its sine / cosine is evaluated at THAT level
//     and shared by every point below it (the pendulum's angle is coordinate 0: DEG evaluations instead of DEG^3);
//   * the weight of a point is the product of its levels' weights: one multiply per point;
//   * the cross-covariance rows of the coordinates that do not move inside the innermost axis take the innermost partial sums
//     sum_k w_k dy_k once per pass instead of once per point.
// Same moments, same order of the points within a level; the sums associate differently (last bits).
template <class M, int DEG, int DIN, int DOUT, bool CROSS, typename R, class F>
I2C_FN void grid_transform_ct(const Rule<R>& rule, const R* m, const R* L, const F& f, R* my, R* Sy, R* Sxy) {
  static_assert(DIN >= 1 && DIN <= 3, "unrolled grid: up to three input dimensions");
  constexpr int NA = M::NA, NA1 = NA > 0 ? NA : 1;
  R sn[NA1], cs[NA1], y0[DOUT], s1[DOUT];
#pragma unroll
  for (int a = 0; a < NA; ++a) r_sincos(m[M::ang(a)], &sn[a], &cs[a]);
  f(m, sn, cs, y0);
#pragma unroll
  for (int k = 0; k < DOUT; ++k) s1[k] = R(0);
#pragma unroll
  for (int k = 0; k < sym(DOUT); ++k) Sy[k] = R(0);
  if (CROSS) {
#pragma unroll
    for (int k = 0; k < DIN * DOUT; ++k) Sxy[k] = R(0);
  }
  R xs[DEG], ws[DEG];  // sf * node, weight
#pragma unroll
  for (int q = 0; q < DEG; ++q) xs[q] = rule.sf * rule.gh_x[q], ws[q] = rule.gh_w[q];
  constexpr int N1 = DIN > 1 ? DEG : 1, N2 = DIN > 2 ? DEG : 1;
#pragma unroll
  for (int i0 = 0; i0 < DEG; ++i0) {
    R d0[DIN];  // offsets after level 0
#pragma unroll
    for (int i = 0; i < DIN; ++i) d0[i] = L[tri(i, 0)] * xs[i0];
#pragma unroll
    for (int a = 0; a < NA; ++a)
      if (M::ang(a) == 0) r_sincos(m[0] + d0[0], &sn[a], &cs[a]);
#pragma unroll
    for (int i1 = 0; i1 < N1; ++i1) {
      R d1[DIN];
      R w1 = ws[i0];
#pragma unroll
      for (int i = 0; i < DIN; ++i) d1[i] = d0[i];
      if constexpr (DIN > 1) {
#pragma unroll
        for (int i = 1; i < DIN; ++i) d1[i] += L[tri(i, 1)] * xs[i1];
        w1 *= ws[i1];
#pragma unroll
        for (int a = 0; a < NA; ++a)
          if (M::ang(a) == 1) r_sincos(m[1] + d1[1], &sn[a], &cs[a]);
      }
      R part[DOUT];  // sum over the innermost axis of w dy (cross-covariance rows of the coordinates it does not move)
#pragma unroll
      for (int k = 0; k < DOUT; ++k) part[k] = R(0);
#pragma unroll
      for (int i2 = 0; i2 < N2; ++i2) {
        R dx[DIN], x[DIN], y[DOUT];
        R w = w1;
#pragma unroll
        for (int i = 0; i < DIN; ++i) dx[i] = d1[i];
        if constexpr (DIN > 2) {
          dx[2] += L[tri(2, 2)] * xs[i2];
          w *= ws[i2];
#pragma unroll
          for (int a = 0; a < NA; ++a)
            if (M::ang(a) == 2) r_sincos(m[2] + dx[2], &sn[a], &cs[a]);
        }
#pragma unroll
        for (int i = 0; i < DIN; ++i) x[i] = m[i] + dx[i];
        f(x, sn, cs, y);
#pragma unroll
        for (int k = 0; k < DOUT; ++k) {
          const R wy = w * (y[k] - y0[k]);
          y[k] -= y0[k];
          part[k] += wy;
#pragma unroll
          for (int l = 0; l <= k; ++l) Sy[tri(k, l)] += wy * y[l];
          if (CROSS) Sxy[(DIN - 1) * DOUT + k] += dx[DIN - 1] * wy;  // the coordinate the innermost axis moves
        }
      }
#pragma unroll
      for (int k = 0; k < DOUT; ++k) {
        s1[k] += part[k];
        if (CROSS) {
#pragma unroll
          for (int i = 0; i < DIN - 1; ++i) Sxy[i * DOUT + k] += d1[i] * part[k];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DOUT; ++k) my[k] = y0[k] + s1[k];
#pragma unroll
  for (int k = 0; k < DOUT; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) Sy[tri(k, l)] -= s1[k] * s1[l];
}

// GRID selects the rule of a cell body at compile time: 0 the sigma points, GRID_LANE the tensor grid walked by the body's own lane,
// GRID_WAVE the tensor grid strided over the 64 lanes of a wavefront that all run the body on ONE trajectory (the grid family,
// i2c_grid.hpp). In a GRID_WAVE body every lane holds the same bits in every value -- grid_allreduce guarantees it after a
// transform, everything else is computed redundantly from the same inputs -- so its control flow is wave-uniform; loads are
// same-address broadcasts and only lane 0 stores (grid_writer). The sigma-point and GRID_LANE kernels are unchanged by it.
constexpr int GRID_LANE = 1, GRID_WAVE = 2;
#ifdef I2C_HOST_SIM
// The simulated lane of a GRID_WAVE body (tests only): the 64 lanes of a trajectory are 64 cooperatively scheduled contexts of ONE
// thread (grid_sim_team, i2c_grid.hpp); what the device reads from its lane id and exchanges with cross-lane instructions comes
// from here. xch: 64 x GridXch<M>::N values.
struct GridLaneSim {
  int l;
  double* xch;
};
inline thread_local GridLaneSim grid_lane_sim{0, nullptr};
inline void grid_sim_sync();  // the team's barrier: every lane arrives before any lane goes on (i2c_grid.hpp)
#endif
I2C_FN int grid_lane() {
#ifdef I2C_HOST_SIM
  return grid_lane_sim.l;
#else
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#endif
}
// does this lane store the body's results? (a compile-time `true` in the one-lane kernels)
template <int GRID> I2C_FN bool grid_writer() {
  if constexpr (GRID == GRID_WAVE) return grid_lane() == 0;
  else return true;
}
// between a body's read of a location and its writer's update of the same one (the tempering state of covariance control): the
// device's lanes run in lockstep, the simulation's lanes wait for each other
template <int GRID> I2C_FN void grid_read_before_write() {
#ifdef I2C_HOST_SIM
  if constexpr (GRID == GRID_WAVE) grid_sim_sync();
#endif
}
template <class M, int DIN, int DOUT, bool CROSS, typename R, class F>
I2C_FN void grid_transform_wave(const Rule<R>& rule, const R* m, const R* L, const F& f, R* my, R* Sy, R* Sxy);  // i2c_grid.hpp

template <int GRID, class M, class ST, int DIN, int DOUT, bool CROSS, bool UNITW = false, bool HANDOFF = false, typename R, class F>
I2C_FN void transform(const Rule<R>& rule, const R* m, const R* Sin, const R* L, const F& f, R* my, R* Sy, R* Sxy,
                      const PolyTab<R>* tab = nullptr) {
  static_assert(!HANDOFF || GRID == 0, "the hand-off of the differences is the sigma-point rule's (sp_transform)");
  if constexpr (GRID == GRID_WAVE) {
    grid_transform_wave<M, DIN, DOUT, CROSS>(rule, m, L, f, my, Sy, Sxy);
  } else if constexpr (GRID != 0) {
    if constexpr (DIN <= 3) {  // degrees 2 .. 4 of the pendulum-sized models: the unrolled grid (wave-uniform choice)
      if (rule.gh_degree == 3) return grid_transform_ct<M, 3, DIN, DOUT, CROSS>(rule, m, L, f, my, Sy, Sxy);
      if (rule.gh_degree == 4) return grid_transform_ct<M, 4, DIN, DOUT, CROSS>(rule, m, L, f, my, Sy, Sxy);
      if (rule.gh_degree == 2) return grid_transform_ct<M, 2, DIN, DOUT, CROSS>(rule, m, L, f, my, Sy, Sxy);
    }
    grid_transform<M, DIN, DOUT, CROSS>(rule, m, L, f, my, Sy, Sxy);
  } else
    sp_transform<M, ST, DIN, DOUT, CROSS, UNITW, HANDOFF>(rule, m, Sin, L, f, my, Sy, Sxy, tab);
}


// S = element type of the PER-CELL buffers in HBM (prior/post, fwd, prior_out, xm, zpost): R normally, float with R =
// double in the mixed mode I2C_F64_F32S (fp64 arithmetic on fp32-stored messages). Per-trajectory data stays R.
template <typename R, typename S = R> struct FwdArgs {
  const S* prior;   // [T][E_POST][B]
  S* fwd;           // [T][E_FWD][B]
  S* prior_out;     // [T][D + sym(D)][B] or null
  const R* x0;      // [NX][B]
  const R* sig_x0;  // [sym NX][B]
  const R* z;       // [T][NZ][B] or null
  const R* alpha;   // [B]
  const R* alpha_cell;  // [T][B] or null
  const uint8_t* ff;  // [T]
  int32_t* status;  // [B]
  const uint8_t* expert;  // [T] ring or null: per-cell use_expert_controller (Linearize forward only, i2c.py:259-265)
};

// REL: what the sweep does when a chunk of the chunked backward schedule has all its forward messages in memory. NoRelease: nothing
// (every kernel but one). ChunkRelease (k_forward_helper, i2c_impl.hpp): the sweep shares its workgroup with a second wavefront that
// composes the finished chunks; release() makes this wave's stores visible to it and meets it at the workgroup barrier. The sweep
// calls release() once per chunk -- n_chunks times whatever happens to a trajectory (failures are branch-free) --, the helper waits
// at the barrier as many times: no wave ever waits on memory contents.
// Inside the cell the test `t == at` and the release are ONE statement without control flow the compiler can see: a branch there
// splits the cell's basic block, and a product and its sum on different sides of the split are no longer contracted into the same
// fused multiply-add -- the sweep would round differently from k_forward (measured: two fma fewer per cell, posterior off in the last
// bits). The wait for this wave's stores (vmcnt(0)) is the release; "memory" keeps the compiler's accesses on their side of it.
// That is enough where the waves of a workgroup share one CU and its vector L1 (the default; the kernel is NOT built for threadgroup-
// split mode, where the two waves could sit on different CUs and the release would have to write back / invalidate as well).
// The contraction is the compiler's choice: the device cases of tests/test_forward_helper.py (torch.equal against k_forward; the LEAN
// cell) and of tests/test_learn_general_variants.py (the general cell: weights that do not sum to one, per-cell targets, a moved
// ring) are what holds it across compiler versions.
// GAIN (ChunkReleaseGain: k_forward_helper<GAINH>, fp64-stored messages): the helper also finishes the smoother gain J = sig_xy
// sig_x3^-1 of every cell it composes -- J is only stored by the sweep, never read by it, so neither it nor sig_xy is on the carried
// chain. The sweep then hands over, in J's own d nx slots of the row, the differences dl_j[k] of the dynamics transform (sp_transform
// <HANDOFF>) and forms neither sig_xy nor J; the helper re-forms chol(sig_xu1_f), sig_xy, chol(sig_x3_f) and the solves from the row
// with the sweep's expressions in the sweep's order (gain_from_handoff) and stores J over the hand-off. On the flagged cell J is
// solved with the factor of sig_x3 BEFORE the terminal update while the row holds the one after it: there the sweep copies the earlier
// one to term_sig [sym NX][B] (rows of the chunk workspace that are dead while the sweep runs: forward_helper_lane, i2c_impl.hpp),
// inside the terminal block it has anyway.
struct NoRelease {
  static constexpr bool ON = false, GAIN = false;
  int chunk_len;
  I2C_HD inline void release() const {}
  I2C_HD inline void release_if(int, int) const {}
};
struct ChunkRelease {
  static constexpr bool ON = true, GAIN = false;
  int chunk_len;  // ChunkArgs::chunk_len, wave-uniform
  I2C_HD inline void release() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), whatever the target's memory model asks of a workgroup-scope fence
    __builtin_amdgcn_s_barrier();
#endif
  }
  I2C_HD inline void release_if(const int t, const int at) const {  // t, at: wave-uniform
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_cmp_lg_u32 %0, %1\n\ts_cbranch_scc1 .Lnot_released_%=\n\ts_waitcnt vmcnt(0)\n\ts_barrier\n.Lnot_released_%=:"
                 :
                 : "s"(t), "s"(at)
                 : "memory", "scc");
#else
    (void)t, (void)at;
#endif
  }
};
template <typename R> struct ChunkReleaseGain {
  static constexpr bool ON = true, GAIN = true;
  int chunk_len;
  R* term_sig;  // [sym NX][B]: sig_x3 of the flagged cell before its terminal update
  I2C_HD inline void release() const { ChunkRelease{chunk_len}.release(); }
  I2C_HD inline void release_if(const int t, const int at) const { ChunkRelease{chunk_len}.release_if(t, at); }
};

// LEAN = the common case fixed at compile time (weights sum to 1, shared target, trajectory-level alpha, no
// joint-prior output): the corresponding wave-uniform runtime branches disappear from the cell, which keeps
// it one scheduling region. The generic variant (LEAN = false) handles everything.
// HZ (per-trajectory horizons, I2cProblem.horizons; generic variant, t0 = 0, no alpha_cell): the lane's loop runs to ITS horizon Tb
// (clamp_horizon) and the terminal update fires in its cell Tb - 1. The time index stays ONE value for the lanes that are still
// running -- a lane that is done leaves the loop, the others go on with the same t --, so the wave-uniform row offsets (make_window,
// wld, uniform_u32) hold as they are. The one-cell-ahead fetches (prior rows, target, mode flag) name row t + 1, wave-uniform as
// well, and a lane in its last cell takes no part in them: no row t >= Tb is read. The flag is compile-time and defaults to off:
// every other instantiation compiles from the code it had.
I2C_HD inline int clamp_horizon(const int h, const int T) { return h < 1 ? 1 : (h > T ? T : h); }
template <class M, typename R, bool LEAN = false, int GRID = 0, typename ST_ = R, class REL = NoRelease, bool HZ = false>
I2C_HD inline void forward_sweep_body(const Consts<M, R>& c, const FwdArgs<R, ST_>& a, const int b, const REL rel = REL{0},
                                      [[maybe_unused]] const int Tb = 0) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NU = C::NU, NZ = C::NZ, NZT = C::NZT, D = C::D;
  constexpr unsigned W = sizeof(ST_);
  static_assert(!HZ || (!LEAN && GRID == 0 && !REL::ON), "per-trajectory horizons: the generic one-lane sweep on its own");
  const unsigned long B = c.B;
  const int T = HZ ? Tb : c.T;
  const unsigned bo = (unsigned)b * W;     // the lane's byte offset inside any row
  const unsigned rb0 = (unsigned)(B * W);  // bytes per row (wave-uniform)
  const R alpha_traj = a.alpha[b];
  const bool wr = grid_writer<GRID>();  // (GRID_WAVE: lane 0 of the trajectory's wavefront; `true` otherwise)
  int fail = 0;  // first failure of this trajectory, (reason << 16) | (t + 1); kept in a register, stored once

  R mu_x[NX], sig_x[sym(NX)];
#pragma unroll
  for (int i = 0; i < NX; ++i) mu_x[i] = a.x0[i * B + b];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) sig_x[i] = a.sig_x0[i * B + b];

  // Per-row byte offsets bo + e * rb as VGPR values (small models): a buffer access then needs no scalar multiply for its
  // row offset. The lone wave of the small-batch regime is instruction-issue-bound and a SALU instruction costs it the
  // same 4 clocks as a VALU one (profiles/r1_k_forward_sq_counters.json); VGPRs are plentiful here.
  constexpr bool VOFF = C::D <= 5;
  unsigned voff[VOFF ? C::E_FWD : 1];
  if (VOFF) {
#pragma unroll
    for (int e = 0; e < C::E_FWD; ++e) voff[e] = bo + (unsigned)e * rb0;
  }
  // software prefetch of the next cell's prior rows: the loads do not depend on the recursion.
  // Small models fetch the NEXT cell's prior rows right after a cell has consumed its own (below), straight into the same
  // registers: a whole cell ahead of their use, no copies. For d >= 6 those d + s(d) + nu nx doubles would sit on top of a
  // register peak that already fills the 512-VGPR file, so there EVERY cell (the first included: loaded here and skipped in
  // the loop, the rows become loop-carried values that stay live through every cell to the back edge) loads its rows at the
  // top of its own cell: one exposed HBM round trip (~1 us) per ~15 us cell rather than scratch traffic throughout.
  constexpr bool PREFETCH = C::D <= 5;
  R pri[C::E_PRI], zt[NZ];
  if (PREFETCH) {
    const unsigned rb = rb0;
    const Window w = make_window(a.prior + (unsigned long)(LEAN ? 0 : c.row(0)) * C::E_POST * B, (unsigned long)C::E_POST * rb);
#pragma unroll
    for (int e = 0; e < C::E_PRI; ++e) pri[e] = (R)wld<ST_>(w, VOFF ? 0u : (e) * rb, VOFF ? voff[e] : bo);
#pragma unroll
    for (int k = 0; k < NZ; ++k) zt[k] = (!LEAN && c.z_per_cell) ? a.z[((long)c.row(0) * NZ + k) * B + b] : c.zg[k];
  }

  // The feed-forward flag of a cell is a byte in global memory: loaded at the top of its own cell it is a dependent
  // vector load whose full latency (plus, vmcnt being shared, the acknowledgement of the previous cell's last stores)
  // is exposed EVERY cell. It is therefore fetched one cell ahead, together with the prior rows.
  unsigned ff_cur = a.ff[LEAN ? 0 : c.row(0)];
  // (a trajectory of ONE cell never leaves feed-forward mode, whatever the batch's shared flag of cell 0 says: a graph of horizon 1
  //  has tau = 0 and _update_priors switches nothing, i2c.py:833, 1212)
  if constexpr (HZ) ff_cur = T == 1 ? 1u : ff_cur;
  // Small models never factor the prior joint: its Cholesky factor is assembled from the factor Lx of the incoming
  // sig_x0_f (= chol(sig_x3_f) of the previous cell, already needed for the smoother gain) as
  //   L0 = [[Lx, 0], [K~ Lx, chol(sig_u|x)]],  sig_u|x = sig_u0_m - K~ sig_ux^T   (feed-forward: K~ = 0, sig_u|x = sig_u0_f),
  // which takes one nu x nu factorisation instead of a d x d one off the critical path. (For d >= 6 the carried
  // factor would cost nx(nx+1)/2 more live registers across the whole cell.)
  constexpr bool STRUCT_L0 = C::D <= 5;
  R Lx[STRUCT_L0 ? sym(NX) : 1];
  if (STRUCT_L0) {
    R rx[NX];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) Lx[i] = sig_x[i];
    fail = note_failure(fail, chol<NX>(Lx, rx), 1, 0);
  }

  // Settle the loads issued so far: the waitcnt pass joins the loop-entry state with the back-edge state, and pending
  // loads on the entry path would put an `s_waitcnt vmcnt(0)` at the loop top that executes every cell (see below).
  ff_cur = opaque(ff_cur);
  if (PREFETCH) {
#pragma unroll
    for (int e = 0; e < C::E_PRI; ++e) pri[e] = opaque(pri[e]);
#pragma unroll
    for (int k = 0; k < NZ; ++k) zt[k] = opaque(zt[k]);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) mu_x[i] = opaque(mu_x[i]);
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) sig_x[i] = opaque(sig_x[i]);
  const R alpha_settled = opaque(alpha_traj);
  R alpha_cur = opaque((!LEAN && a.alpha_cell) ? a.alpha_cell[(long)c.row(0) * B + b] : alpha_settled);  // per-cell temperature, fetched a cell ahead
  // Per-cell constants as VGPR values (small models): left as kernel arguments they sit in ~30 SGPRs for the whole
  // sweep, and the scalar file then spills (v_readlane) and re-materialises polynomial literals (s_mov) in every cell.
  // Only where the register file has room: the cartpole (21 + 10 doubles) already overflows into AGPRs and slows down.
  constexpr bool CONST_V = VOFF && (sym(NZ) + sym(NX) <= 16);
  PolyTab<R> ptab;  // sincos coefficients as VGPR values (see PolyTab), same condition
  if (CONST_V) poly_tab_init(ptab);
  const PolyTab<R>* const tab = CONST_V ? &ptab : nullptr;
  R xi0_v[CONST_V ? sym(NZ) : 1], eta_v[CONST_V ? sym(NX) : 1];
  if (CONST_V) {
#pragma unroll
    for (int i = 0; i < sym(NZ); ++i) xi0_v[i] = opaque(c.sig_xi0[i]);
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) eta_v[i] = opaque(LEAN ? c.sig_eta[i] : c.sig_eta_w[i]);
  }

  [[maybe_unused]] int next_release = rel.chunk_len;  // (REL) the first cell of the second chunk
  for (int t = 0; t < T; ++t) {
    // HZ: t + 1, the same for every running lane; `more` keeps a lane in its last cell out of the fetches (rows are plain: t0 = 0)
    const int tn = HZ ? t + 1 : (t + 1 < T ? t + 1 : t);
    [[maybe_unused]] const bool more = !HZ || t + 1 < T;
    const int tr = (LEAN || HZ) ? t : c.row(t), tnr = (LEAN || HZ) ? tn : c.row(tn);  // rows of the persistent buffers (ring, see Consts::t0)
    const unsigned rb = opaque_uniform(rb0);  // see opaque_uniform(): no hoisting of e * rb
    // Large models: an index the compiler cannot see through (always 0) makes the big constant tables of the kernel
    // argument (sig_xi0: 45 doubles for the double cartpole, sig_eta: 21) scalar LOADS next to their single use in each
    // cell; hoisted out of the time loop they occupy ~130 SGPRs and the scalar file spills through v_writelane /
    // v_readlane (540 of the 7 800 instructions of that kernel).
    const int kz = (C::D >= 6) ? (int)opaque_uniform(0u) : 0;
    if (!PREFETCH) {  // see PREFETCH above
      const Window w = make_window(a.prior + (unsigned long)tr * C::E_POST * B, (unsigned long)C::E_POST * rb);
#pragma unroll
      for (int e = 0; e < C::E_PRI; ++e) pri[e] = (R)wld<ST_>(w, VOFF ? 0u : (e) * rb, VOFF ? voff[e] : bo);
#pragma unroll
      for (int k = 0; k < NZ; ++k) zt[k] = (!LEAN && c.z_per_cell) ? a.z[((long)tr * NZ + k) * B + b] : c.zg[k];
    }

    // per-cell temperature only in the MPC loop (stale sig_xi of appended cells); else the trajectory's
    const R alpha = opaque(alpha_cur);
    const R* pmu = pri;               // prior joint mean  (== previous posterior, see i2c_hip.h)
    const R* psig = pri + D;          // prior joint covariance
    const R* Kprev = pri + D + sym(D);

    // ---- 1. joint prior over (x, u) ---------------------------------------------------
    int cell_bad = 0;  // 0, or 7 - (execution order of the first failed stage of this cell), see flag_stage()
    R mu0[D], S0[sym(D)];
    R L0[STRUCT_L0 ? sym(D) : 1], Luu[sym(NU)], ruu[NU];  // Luu: conditional action covariance, then its factor
    if (ff_cur != 0) {  // feed-forward: independent action prior (i2c.py:355-360)
#pragma unroll
      for (int i = 0; i < NX; ++i) mu0[i] = mu_x[i];
#pragma unroll
      for (int i = NX; i < D; ++i) mu0[i] = pmu[i];
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j)
          S0[tri(i, j)] = (i < NX) ? sig_x[tri(i, j)] : (j >= NX ? psig[tri(i, j)] : R(0));
      if (STRUCT_L0) {
#pragma unroll
        for (int p = 0; p < NU; ++p)
#pragma unroll
          for (int q = 0; q <= p; ++q) Luu[tri(p, q)] = psig[tri(NX + p, NX + q)];
#pragma unroll
        for (int p = 0; p < NU; ++p)
#pragma unroll
          for (int j = 0; j < NX; ++j) L0[tri(NX + p, j)] = R(0);
      }
    } else {  // feedback: condition the previous controller on the new state message (i2c.py:361-387)
      R S[sym(NX)], delta[NX];
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) S[i] = psig[i] + sig_x[i];  // xx block is the packed prefix
#pragma unroll
      for (int i = 0; i < NX; ++i) delta[i] = mu_x[i] - pmu[i];
      bool ok;
      const R rho = pdf_ratio<NX>(S, delta, &ok, tab);
      cell_bad = flag_stage(cell_bad, ok, 0);
      R Kt[NU * NX];
#pragma unroll
      for (int i = 0; i < NU * NX; ++i) Kt[i] = rho * Kprev[i];
      // sig_u0_f = sig_u0_m - Kt sig_ux^T + Kt sig_x0_f Kt^T
      R sig_u[sym(NU)];
      gain_quad<NX, NU>(Kt, sig_x, sig_u);
#pragma unroll
      for (int p = 0; p < NU; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) {
          R v = psig[tri(NX + p, NX + q)];
#pragma unroll
          for (int k = 0; k < NX; ++k) v -= Kt[p * NX + k] * psig[tri(NX + q, k)];
          Luu[tri(p, q)] = v;  // sig_u0_m - K~ sig_ux^T
          sig_u[tri(p, q)] += v;
        }
      joint_from_gain<NX, NU>(mu_x, sig_x, Kt, pmu, pmu + NX, sig_u, mu0, S0);
      if (STRUCT_L0) {
#pragma unroll
        for (int p = 0; p < NU; ++p)
#pragma unroll
          for (int j = 0; j < NX; ++j) {
            R v = R(0);
#pragma unroll
            for (int k = j; k < NX; ++k) v += Kt[p * NX + k] * Lx[tri(k, j)];
            L0[tri(NX + p, j)] = v;
          }
      }
    }
    if (STRUCT_L0) {
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) L0[i] = Lx[i];  // xx block = packed prefix
      cell_bad = flag_stage(cell_bad, chol<NU>(Luu, ruu), 1);
#pragma unroll
      for (int p = 0; p < NU; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) L0[tri(NX + p, NX + q)] = Luu[tri(p, q)];
    }
    if (!LEAN && a.prior_out && wr) {
      const Window w = make_window(a.prior_out + (unsigned long)t * (D + sym(D)) * B, (unsigned long)(D + sym(D)) * rb);
#pragma unroll
      for (int e = 0; e < D; ++e) wst(w, VOFF ? 0u : (e) * rb, VOFF ? voff[e] : bo, (ST_)mu0[e]);
#pragma unroll
      for (int e = 0; e < sym(D); ++e) wst(w, VOFF ? 0u : (D + e) * rb, VOFF ? voff[D + e] : bo, (ST_)S0[e]);
    }

    if constexpr (HZ) {
      if (more) {  // (no alpha_cell with horizons: refused by the resolver)
        ff_cur = a.ff[tnr];
        if (PREFETCH) {
          const Window w = make_window(a.prior + (unsigned long)tnr * C::E_POST * B, (unsigned long)C::E_POST * rb);
#pragma unroll
          for (int e = 0; e < C::E_PRI; ++e) pri[e] = (R)wld<ST_>(w, VOFF ? 0u : (e) * rb, VOFF ? voff[e] : bo);
        }
      }
    } else {
    ff_cur = a.ff[tnr];  // the next cell's flag, a whole cell ahead of its use
    if (!LEAN && a.alpha_cell) alpha_cur = a.alpha_cell[(long)tnr * B + b];
    if (PREFETCH) {  // pri is dead from here on: refill it with the next cell's rows
      const Window w = make_window(a.prior + (unsigned long)tnr * C::E_POST * B, (unsigned long)C::E_POST * rb);
#pragma unroll
      for (int e = 0; e < C::E_PRI; ++e) pri[e] = (R)wld<ST_>(w, VOFF ? 0u : (e) * rb, VOFF ? voff[e] : bo);
    }
    }

    // ---- 2. cost "observation": measurement update on z (i2c.py:390-407) --------------
    sched_fence<(D >= 6)>();
    {
      R Lf[STRUCT_L0 ? 1 : sym(D)], rinv[D];
      if (!STRUCT_L0) {
#pragma unroll
        for (int i = 0; i < sym(D); ++i) Lf[i] = S0[i];
        cell_bad = flag_stage(cell_bad, chol<D>(Lf, rinv), 1);
      }
      const R* L = STRUCT_L0 ? L0 : Lf;
      R mz[NZ], Sz[sym(NZ)], Sxz[D * NZ];
      transform<GRID, M, ObsStruct<M>, D, NZ, true, LEAN>(c.rule_xu, mu0, S0, L, ObserveF<M, R>{params_of(c, b)}, mz, Sz, Sxz, tab);
#pragma unroll
      for (int i = 0; i < sym(NZ); ++i) Sz[i] += alpha * (CONST_V ? xi0_v[i] : c.sig_xi0[i + kz]);
      cell_bad = flag_stage(cell_bad, kalman_update<D, NZ>(mu0, S0, mz, Sz, Sxz, zt), 2);
    }
    if (!LEAN && PREFETCH && c.z_per_cell && more) {  // the target is consumed: fetch the next cell's
#pragma unroll
      for (int k = 0; k < NZ; ++k) zt[k] = a.z[((long)tnr * NZ + k) * B + b];
    }
    // mu0 / S0 now hold mu_xu1_f / sig_xu1_f
    const Window out = make_window(a.fwd + (unsigned long)t * C::E_FWD * B, (unsigned long)C::E_FWD * rb);
    if (wr) {
#pragma unroll
      for (int e = 0; e < D; ++e) wst(out, VOFF ? 0u : (e) * rb, VOFF ? voff[e] : bo, (ST_)mu0[e]);
#pragma unroll
      for (int e = 0; e < sym(D); ++e) wst(out, VOFF ? 0u : (D + e) * rb, VOFF ? voff[D + e] : bo, (ST_)S0[e]);
    }

    // ---- 3. dynamics push-through (i2c.py:415-421) and smoother gain (i2c.py:423-425) --
    sched_fence<(D >= 6)>();
    R Sxy[D * NX];
    constexpr bool NOISE = GRID == 0 && has_process_noise<M, R>::value;
    static_assert(!NOISE || !REL::ON, "a model with process_noise runs the plain sweep (Impl::launches)");
    [[maybe_unused]] R qn[NOISE ? sym(NX) : 1];
    {
      R L[sym(D)], rinv[D];
#pragma unroll
      for (int i = 0; i < sym(D); ++i) L[i] = S0[i];
      cell_bad = flag_stage(cell_bad, chol<D>(L, rinv), 3);
      // (REL::GAIN: Sxy takes the hand-off dl_j[k] and stays it; the helper wave forms sig_xy and J)
      if constexpr (NOISE)
        transform<GRID, M, DenseStruct<D>, D, NX, true, LEAN>(c.rule_xu, mu0, S0, L, DynamicsNoiseF<M, R>{{params_of(c, b)}, qn}, mu_x, sig_x, Sxy, tab);
      else
        transform<GRID, M, DenseStruct<D>, D, NX, true, LEAN, REL::GAIN>(c.rule_xu, mu0, S0, L, DynamicsF<M, R>{params_of(c, b)}, mu_x, sig_x, Sxy, tab);
    }
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) sig_x[i] += CONST_V ? eta_v[i] : (LEAN ? c.sig_eta[i + kz] : c.sig_eta_w[i + kz]);  // sum_p w_p sig_eta (quadrature.py:57)
    if constexpr (NOISE) {  // ... + sum_p w_p Q(x_p): the model's point-dependent part (has_process_noise)
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) sig_x[i] += qn[i];
    }
    R L3[sym(NX)], rinv3[NX];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) L3[i] = sig_x[i];
    cell_bad = flag_stage(cell_bad, chol<NX>(L3, rinv3), 4);
    sched_fence<(D >= 6)>();
    if constexpr (!REL::GAIN) {
#pragma unroll
      for (int i = 0; i < D; ++i) {  // J = sig_xy sig_x3^{-1}, row by row
        fsub<NX>(L3, rinv3, &Sxy[i * NX]);
        bsub<NX>(L3, rinv3, &Sxy[i * NX]);
        sched_fence<(D >= 6)>();
      }
    }

    // gfx9 counts loads AND stores in one counter (vmcnt). A wait on the prefetched prior rows placed (by the compiler)
    // at the top of the next cell also waits for the L2 to acknowledge this cell's LAST stores, issued a few
    // instructions earlier. Touching the prefetched registers here, before the tail stores, puts the wait where
    // everything outstanding is old -- the loads were issued most of a cell ago -- and, together with settling the
    // pre-loop loads (above; the waitcnt pass joins the loop-entry state with the back-edge state), leaves the loop
    // top without any s_waitcnt: 372 -> 357 us. (Measured alternative: touching after the tail stores, 363 us.)
    ff_cur = opaque(ff_cur);
    if (!LEAN) {  // the per-cell temperature and targets of the MPC loop were fetched ahead as well
      alpha_cur = opaque(alpha_cur);
      if (PREFETCH) {
#pragma unroll
        for (int k = 0; k < NZ; ++k) zt[k] = opaque(zt[k]);
      }
    }
    if (PREFETCH) {
#pragma unroll
      for (int e = 0; e < C::E_PRI; ++e) pri[e] = opaque(pri[e]);
    }
    // The first cell of a chunk releases the PREVIOUS chunk (REL above): here every store of the previous cell is older than loads
    // that have returned, and this cell's own (mu0, S0) were issued a dynamics transform ago -- the wait inside release() finds
    // nothing outstanding. (At the end of the chunk's own last cell it would wait for that cell's store acknowledgements.)
    if constexpr (REL::ON) {
      rel.release_if(t, next_release);
      next_release += t == next_release ? rel.chunk_len : 0;
    }
    // J is written out BEFORE the terminal update so that its d*nx registers are dead there (with J
    // live the terminal block is the register peak of the large models and spills to scratch)
    if (wr) {
#pragma unroll
      for (int e = 0; e < D * NX; ++e) wst(out, VOFF ? 0u : (D + sym(D) + NX + sym(NX) + e) * rb, VOFF ? voff[D + sym(D) + NX + sym(NX) + e] : bo, (ST_)Sxy[e]);
    }
    sched_fence<(D >= 6)>();

    // ---- 4. terminal cost observation on the flagged cell, after J (i2c.py:430-443) ----
    if (NZT > 0 && (HZ ? (c.terminal_cell >= 0 && t == T - 1) : t == c.terminal_cell) && c.has_Qf) {
      constexpr int NT = C::NZT1;
      R mzt[NT], Szt[sym(NT)], Sxzt[NX * NT];
      if constexpr (REL::GAIN) {  // the helper solves this cell's J with the factor of sig_x3 as it is HERE (see ChunkReleaseGain)
        if (wr) {
#pragma unroll
          for (int i = 0; i < sym(NX); ++i) rel.term_sig[(unsigned long)i * B + b] = sig_x[i];
        }
      }
      transform<GRID, M, TermStruct<M>, NX, NT, true, LEAN>(c.rule_x, mu_x, sig_x, L3, ObserveTermF<M, R>{params_of(c, b)}, mzt, Szt, Sxzt);
#pragma unroll
      for (int i = 0; i < sym(NT); ++i) Szt[i] += alpha * c.sig_xiT0[i];
      cell_bad = flag_stage(cell_bad, kalman_update<NX, NT>(mu_x, sig_x, mzt, Szt, Sxzt, c.zg_term), 5);
      if (STRUCT_L0) {  // the next cell (MPC: the flagged cell can sit mid-horizon) needs the factor of the UPDATED sig_x
#pragma unroll
        for (int i = 0; i < sym(NX); ++i) L3[i] = sig_x[i];
        cell_bad = flag_stage(cell_bad, chol<NX>(L3, rinv3), 5);
      }
    }
    if (STRUCT_L0) {
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) Lx[i] = L3[i];
    }
    fail = fold_cell_failure(fail, cell_bad, t);
    if (wr) {
#pragma unroll
      for (int e = 0; e < NX; ++e)  // (e = 0: NaN in the rows of a failed trajectory from the failing cell on -- the STORED value only, see nan_if)
        wst(out, VOFF ? 0u : (D + sym(D) + e) * rb, VOFF ? voff[D + sym(D) + e] : bo, (ST_)(e == 0 ? nan_if(fail != 0, mu_x[e]) : mu_x[e]));
#pragma unroll
      for (int e = 0; e < sym(NX); ++e) wst(out, VOFF ? 0u : (D + sym(D) + NX + e) * rb, VOFF ? voff[D + sym(D) + NX + e] : bo, (ST_)sig_x[e]);
    }

  }
  if constexpr (REL::ON) rel.release();  // the last chunk
  if (wr && fail != 0 && a.status[b] == 0) a.status[b] = fail;
}

// ------------------------------------------------------------------------------------------
// Backward pass building blocks (i2c.py:544-610), all on registers of one lane.
// ------------------------------------------------------------------------------------------

// End of chain (i2c.py:546-564): the smoothed terminal state, either the filtered one or, for
// covariance control, its product with the tempered terminal prior (i2c.py:548-559).
template <class M, typename R, int GRID = 0>
I2C_FN void end_of_chain(const Consts<M, R>& c, R* temp, const int b, const R* m3f, const R* S3f, R* m3m, R* S3m,
                         int32_t* status, const int t_last = -1) {  // t_last: the trajectory's own last cell (horizons); -1: T - 1
  constexpr int NX = M::NX;
  const bool wr = grid_writer<GRID>();
  if (c.has_x_terminal) {
    const R tmp = temp[b];
    grid_read_before_write<GRID>();
    if (wr) temp[b] = tmp + c.dtemp;
    R St[sym(NX)], Ssum[sym(NX)], rinv[NX];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) {
      St[i] = tmp * S3f[i];
      Ssum[i] = c.sig_x_term[i] + St[i];
    }
    bool ok = chol<NX>(Ssum, rinv);
    // sig_x3_m = St - St (sig_T + St)^{-1} St  = St - W^T W,  W = chol(sum)^{-1} St
    R Wm[NX * NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R col[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = St[tri_any(i, j)];
      fsub<NX>(Ssum, rinv, col);
#pragma unroll
      for (int i = 0; i < NX; ++i) Wm[i * NX + j] = col[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        R v = St[tri(i, j)];
#pragma unroll
        for (int k = 0; k < NX; ++k) v -= Wm[k * NX + i] * Wm[k * NX + j];
        S3m[tri(i, j)] = v;
      }
    // mu_x3_m = sig_x3_m (St^{-1} mu_x3_f + sig_T^{-1} mu_T)
    R r1[NX], r2[NX], Lt[sym(NX)], LT[sym(NX)];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) {
      Lt[i] = St[i];
      LT[i] = c.sig_x_term[i];
    }
    ok = chol<NX>(Lt, rinv) && ok;
#pragma unroll
    for (int i = 0; i < NX; ++i) r1[i] = m3f[i];
    fsub<NX>(Lt, rinv, r1);
    bsub<NX>(Lt, rinv, r1);
    ok = chol<NX>(LT, rinv) && ok;
#pragma unroll
    for (int i = 0; i < NX; ++i) r2[i] = c.mu_x_term[i];
    fsub<NX>(LT, rinv, r2);
    bsub<NX>(LT, rinv, r2);
#pragma unroll
    for (int i = 0; i < NX; ++i) r1[i] += r2[i];
    symv<NX>(S3m, r1, m3m);
    if (!ok && wr) set_status(status, b, 6, t_last >= 0 ? t_last : c.T - 1);
  } else {
#pragma unroll
    for (int i = 0; i < NX; ++i) m3m[i] = m3f[i];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) S3m[i] = S3f[i];
  }
}

// Expected quadratic cost of N(mz, Sz) against target zt under weight W (packed sym):
//   m = err^T W err + tr(Sz W),  v = 2 tr((Sz W)^2) + 4 err^T W Sz W err   (i2c.py:1034-1043)
template <int N, typename R>
I2C_FN void gaussian_cost(const R* W, const bool w_diag, const R* mz, const R* Sz, const R* zt, R* m, R* v) {
  R err[N];
#pragma unroll
  for (int i = 0; i < N; ++i) err[i] = mz[i] - zt[i];
  if (w_diag) {  // W = diag(w): every shipped cost (Q, R, Qf diagonal). SW_ij = Sz_ij w_j
    R mm = R(0), tr2 = R(0), quad = R(0), we[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      we[i] = W[tri(i, i)] * err[i];
      mm += we[i] * err[i] + W[tri(i, i)] * Sz[tri(i, i)];
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const R sww = Sz[tri(i, j)] * (W[tri(i, i)] * W[tri(j, j)]);
        tr2 += (i == j ? R(1) : R(2)) * Sz[tri(i, j)] * sww;
        quad += (i == j ? R(1) : R(2)) * Sz[tri(i, j)] * (we[i] * we[j]);
      }
    *m = mm;
    *v = R(2) * tr2 + R(4) * quad;
    return;
  }
  R We[N];
  symv<N>(W, err, We);
  R SW[N * N];  // Sz W (not symmetric)
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      R s = R(0);
#pragma unroll
      for (int k = 0; k < N; ++k) s += Sz[tri_any(i, k)] * W[tri_any(k, j)];
      SW[i * N + j] = s;
    }
  R mm = R(0), tr2 = R(0), quad = R(0);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    mm += err[i] * We[i] + SW[i * N + i];
    R SWe = R(0);  // (Sz W err)_i = sum_j Sz[i][j] We[j]
#pragma unroll
    for (int j = 0; j < N; ++j) {
      tr2 += SW[i * N + j] * SW[j * N + i];
      SWe += Sz[tri_any(i, j)] * We[j];
    }
    quad += We[i] * SWe;
  }
  *m = mm;
  *v = R(2) * tr2 + R(4) * quad;
}

// Terminal observation statistics (i2c.py:567-570, 989-992): tr(Qf (errT errT^T + sig_z3_m)).
template <class M, typename R, int GRID = 0>
I2C_FN R terminal_obs_stats(const Consts<M, R>& c, const int b, const R* m3m, const R* S3m, R* term_stats,
                            int32_t* status, const int t_last = -1) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NZT = C::NZT;
  const long B = c.B;
  const bool wr = grid_writer<GRID>();
  R trT = R(0);
  if (NZT > 0 && c.has_Qf) {
    constexpr int NT = C::NZT1;
    R L3[sym(NX)], rinv3[NX], mzt[NT], Szt[sym(NT)];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) L3[i] = S3m[i];
    if (!chol<NX>(L3, rinv3) && wr) set_status(status, b, 6, t_last >= 0 ? t_last : c.T - 1);
    transform<GRID, M, TermStruct<M>, NX, NT, false>(c.rule_x, m3m, S3m, L3, ObserveTermF<M, R>{params_of(c, b)}, mzt, Szt,
                                                  (R*)nullptr);
    R tv;
    gaussian_cost<NT>(c.Qf, c.qf_diag != 0, mzt, Szt, c.zg_term, &trT, &tv);
    if (wr) {
#pragma unroll
      for (int k = 0; k < NT; ++k) term_stats[(long)(3 + k) * B + b] = mzt[k];
#pragma unroll
      for (int k = 0; k < sym(NT); ++k) term_stats[(long)(3 + NT + k) * B + b] = Szt[k];
    }
  }
  if (wr) term_stats[b] = trT;
  return trT;
}

// One backward cell given the smoothed next state: RTS update of the joint (i2c.py:580-583),
// posterior observation statistics (i2c.py:594-596) with their expected cost (i2c.py:1034-1043),
// and the controller (i2c.py:600-608) read off the Cholesky factor L of the posterior joint:
//   K L_xx = L_ux  ->  K^T = L_xx^{-T} L_ux^T ;  sigK = L_uu L_uu^T ;  k = mu_u - K mu_x.
// In: mu/S = mu_xu1_f / sig_xu1_f, J, dm = mu_x3_m - mu_x3_f, dS = sig_x3_m - sig_x3_f.
// Out: mu/S = mu_xu0_m / sig_xu0_m, ctl = [K | k | sigK], mz/Sz, cost mean / variance.
template <class M, typename R, int GRID = 0>
I2C_FN bool cell_posterior(const Consts<M, R>& c, const int b, const R* zt, R* mu, R* S, const R* J, const R* dm, const R* dS,
                           R* ctl, R* mz, R* Sz, R* cm, R* cv, const PolyTab<R>* tab = nullptr) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NU = C::NU, NZ = C::NZ, D = C::D;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    R v = mu[i];
#pragma unroll
    for (int k = 0; k < NX; ++k) v += J[i * NX + k] * dm[k];
    mu[i] = v;
  }
  add_JDJt<D, NX>(J, dS, S);
  R Lm[sym(D)], rinv[D];
#pragma unroll
  for (int e = 0; e < sym(D); ++e) Lm[e] = S[e];
  const bool ok = chol<D>(Lm, rinv);
  transform<GRID, M, ObsStruct<M>, D, NZ, false>(c.rule_xu, mu, S, Lm, ObserveF<M, R>{params_of(c, b)}, mz, Sz, (R*)nullptr, tab);
  gaussian_cost<NZ>(c.QR, c.qr_diag != 0, mz, Sz, zt, cm, cv);
#pragma unroll
  for (int p = 0; p < NU; ++p) {
#pragma unroll
    for (int k = 0; k < NX; ++k) ctl[p * NX + k] = Lm[tri(NX + p, k)];
    bsub<NX>(Lm, rinv, &ctl[p * NX]);  // leading NX x NX block of L is chol(sig_xx)
  }
#pragma unroll
  for (int p = 0; p < NU; ++p) {
    R v = mu[NX + p];
#pragma unroll
    for (int k = 0; k < NX; ++k) v -= ctl[p * NX + k] * mu[k];
    ctl[NU * NX + p] = v;
  }
#pragma unroll
  for (int p = 0; p < NU; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) {
      R v = R(0);
#pragma unroll
      for (int k = 0; k <= q; ++k) v += Lm[tri(NX + p, NX + k)] * Lm[tri(NX + q, NX + k)];
      ctl[NU * NX + NU + tri(p, q)] = v;
    }
  return ok;
}

// ------------------------------------------------------------------------------------------
// Backward sweep, TWO-PASS form (small batches): (1) a light sequential scan of the x-marginal
// recursion
//   mu_x0_m = mu_x1_f + Jx (mu_x3_m - mu_x3_f);  sig_x0_m = sig_x1_f + Jx (sig_x3_m - sig_x3_f) Jx^T,
// which is affine in (mu_x3_m, sig_x3_m), touches only nx x nx blocks and is the ONLY sequential
// part of the backward pass; (2) everything else, independent per cell, one lane per (t, b);
// (3) a deterministic reduction of the per-cell cost statistics over t.
// ------------------------------------------------------------------------------------------
template <typename R, typename S = R> struct ScanArgs {
  const S* fwd;  // [T][E_FWD][B]
  S* xm;         // [T][E_XM][B]
  R* temp;       // [B] or null
  int32_t* status;
};

template <int NX, typename R> struct ScanRow {  // the rows of one cell the recursion needs
  R mu1[NX], S1[sym(NX)], m3f[NX], S3f[sym(NX)], Jx[NX * NX];
};

template <class M, typename R, typename S = R>
I2C_HD inline void backward_scan_body(const Consts<M, R>& c, const ScanArgs<R, S>& a, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, O_J = O_S3 + sym(NX);
  // The recursion itself is ~40 FMAs per cell; what bounds this kernel is load latency with only
  // B/64 wavefronts in flight. Cells are therefore fetched U at a time, one chunk ahead.
  constexpr int U = NX <= 2 ? 4 : 1;
  const long B = c.B;
  const int T = c.T;
  using Row = ScanRow<NX, R>;

  auto load = [&](int t, Row& r) {
    const S* in = a.fwd + ((long)(t > 0 ? t : 0) * C::E_FWD) * B + b;
#pragma unroll
    for (int i = 0; i < NX; ++i) r.mu1[i] = in[(long)i * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) r.S1[i] = in[(long)(D + i) * B];
#pragma unroll
    for (int i = 0; i < NX; ++i) r.m3f[i] = in[(long)(O_MU3 + i) * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) r.S3f[i] = in[(long)(O_S3 + i) * B];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) r.Jx[i] = in[(long)(O_J + i) * B];
  };
  Row cur[U], nxt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) load(T - 1 - u, cur[u]);

  R m3m[NX], S3m[sym(NX)];
  end_of_chain<M, R>(c, a.temp, b, cur[0].m3f, cur[0].S3f, m3m, S3m, a.status);

  for (int t0 = T - 1; t0 >= 0; t0 -= U) {
#pragma unroll
    for (int u = 0; u < U; ++u) load(t0 - U - u, nxt[u]);  // next chunk (clamped at cell 0)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 - u;
      if (t < 0) break;
      const Row& r = cur[u];
      S* out = a.xm + ((long)t * C::E_XM) * B + b;
#pragma unroll
      for (int i = 0; i < NX; ++i) out[(long)i * B] = m3m[i];
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) out[(long)(NX + i) * B] = S3m[i];
      R dm[NX], dS[sym(NX)];
#pragma unroll
      for (int i = 0; i < NX; ++i) dm[i] = m3m[i] - r.m3f[i];
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) dS[i] = S3m[i] - r.S3f[i];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        R v = r.mu1[i];
#pragma unroll
        for (int k = 0; k < NX; ++k) v += r.Jx[i * NX + k] * dm[k];
        m3m[i] = v;
      }
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) S3m[i] = r.S1[i];
      add_JDJt<NX, NX>(r.Jx, dS, S3m);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = nxt[u];
  }
}

#ifndef I2C_WALK_VOFF
#define I2C_WALK_VOFF 1
#endif
template <typename R, typename S = R> struct CellArgs {
  const S* fwd;      // [T][E_FWD][B]
  const S* xm;       // [T][E_XM][B]   (two-pass: input; fused: optional output)
  const R* z;        // [T][NZ][B] or null
  S* post;           // [T][E_POST][B]
  S* zpost;          // [T][E_ZPOST][B] or null
  R* cell_stats;     // [T][2][B]      (two-pass: required workspace; fused: optional output)
  R* term_stats;     // [E_TERM][B]
  R* temp;           // [B] or null (fused only)
  int32_t* status;
  const R* alpha;    // [B] (Linearize backward only: terminal cost update at the end of the chain)
};

// voff (small models, see forward_sweep_body): the lane's byte offset of row e, bo + e * rb, as VGPR values -- the stores then go
// through one buffer window per cell and need no scalar address arithmetic (5 - 6 scalar instructions per row otherwise, and
// the lone wave of the small-batch regime pays 4 clocks for each of them).
template <class M, typename R, typename S_>
I2C_FN void store_cell(const Consts<M, R>& c, const CellArgs<R, S_>& a, const int t, const int b, const R* mu, const R* S,
                       const R* ctl, const R* mz, const R* Sz, const R cm, const R cv, const unsigned* voff = nullptr) {
  using C = Consts<M, R>;
  constexpr int NZ = C::NZ, D = C::D;
  const long B = c.B;
  if (voff) {
    const unsigned rb = (unsigned)(B * sizeof(S_));
    const Window wp = make_window(a.post + (unsigned long)c.row(t) * C::E_POST * B, (unsigned long)C::E_POST * rb);
#pragma unroll
    for (int e = 0; e < D; ++e) wst(wp, 0u, voff[e], (S_)mu[e]);
#pragma unroll
    for (int e = 0; e < sym(D); ++e) wst(wp, 0u, voff[D + e], (S_)S[e]);
#pragma unroll
    for (int e = 0; e < C::E_POST - D - sym(D); ++e) wst(wp, 0u, voff[D + sym(D) + e], (S_)ctl[e]);
    if (a.zpost) {
      const Window wz = make_window(a.zpost + (unsigned long)t * C::E_ZPOST * B, (unsigned long)C::E_ZPOST * rb);
#pragma unroll
      for (int k = 0; k < NZ; ++k) wst(wz, 0u, voff[k], (S_)mz[k]);
#pragma unroll
      for (int k = 0; k < sym(NZ); ++k) wst(wz, 0u, voff[NZ + k], (S_)Sz[k]);
    }
    if (a.cell_stats) {
      a.cell_stats[((long)t * 2 + 0) * B + b] = cm;
      a.cell_stats[((long)t * 2 + 1) * B + b] = cv;
    }
    return;
  }
  S_* out = a.post + ((long)c.row(t) * C::E_POST) * B + b;
#pragma unroll
  for (int e = 0; e < D; ++e) out[(long)e * B] = (S_)mu[e];
#pragma unroll
  for (int e = 0; e < sym(D); ++e) out[(long)(D + e) * B] = (S_)S[e];
#pragma unroll
  for (int e = 0; e < C::E_POST - D - sym(D); ++e) out[(long)(D + sym(D) + e) * B] = (S_)ctl[e];
  if (a.zpost) {
    S_* zo = a.zpost + ((long)t * C::E_ZPOST) * B + b;
#pragma unroll
    for (int k = 0; k < NZ; ++k) zo[(long)k * B] = (S_)mz[k];
#pragma unroll
    for (int k = 0; k < sym(NZ); ++k) zo[(long)(NZ + k) * B] = (S_)Sz[k];
  }
  if (a.cell_stats) {
    a.cell_stats[((long)t * 2 + 0) * B + b] = cm;
    a.cell_stats[((long)t * 2 + 1) * B + b] = cv;
  }
}

// pass (2): one lane per (t, b)
template <class M, typename R, typename S_ = R>
I2C_HD inline void backward_cell_body(const Consts<M, R>& c, const CellArgs<R, S_>& a, const int t, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NZ = C::NZ, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, O_J = O_S3 + sym(NX);
  const long B = c.B;
  const S_* in = a.fwd + ((long)t * C::E_FWD) * B + b;
  const S_* xin = a.xm + ((long)t * C::E_XM) * B + b;

  R mu[D], S[sym(D)], J[D * NX], dm[NX], dS[sym(NX)], m3m[NX], S3m[sym(NX)];
#pragma unroll
  for (int e = 0; e < D; ++e) mu[e] = in[(long)e * B];
#pragma unroll
  for (int e = 0; e < sym(D); ++e) S[e] = in[(long)(D + e) * B];
#pragma unroll
  for (int e = 0; e < NX; ++e) {
    m3m[e] = xin[(long)e * B];
    dm[e] = m3m[e] - in[(long)(O_MU3 + e) * B];
  }
#pragma unroll
  for (int e = 0; e < sym(NX); ++e) {
    S3m[e] = xin[(long)(NX + e) * B];
    dS[e] = S3m[e] - in[(long)(O_S3 + e) * B];
  }
#pragma unroll
  for (int e = 0; e < D * NX; ++e) J[e] = in[(long)(O_J + e) * B];
  R zt[NZ];
#pragma unroll
  for (int k = 0; k < NZ; ++k) zt[k] = c.z_per_cell ? a.z[((long)c.row(t) * NZ + k) * B + b] : c.zg[k];

  R ctl[C::E_POST - D - sym(D)], mz[NZ], Sz[sym(NZ)], cm, cv;
  if (!cell_posterior<M, R>(c, b, zt, mu, S, J, dm, dS, ctl, mz, Sz, &cm, &cv)) set_status(a.status, b, 7, t);
  store_cell<M, R, S_>(c, a, t, b, mu, S, ctl, mz, Sz, cm, cv);
  if (t == c.T - 1) terminal_obs_stats<M, R>(c, b, m3m, S3m, a.term_stats, a.status);
}

// pass (3): term_stats rows 1, 2 = sum_t m_t, sum_t v_t. `part`/`nparts` split t between the
// cooperating lanes of one trajectory; the caller adds the partial sums in a fixed order.
template <class M, typename R>
I2C_FN void reduce_partial(const Consts<M, R>& c, const R* cell_stats, const int b, const int part, const int nparts,
                           R* m, R* v) {
  const long B = c.B;
  R sm = R(0), sv = R(0);
#pragma unroll 4
  for (int t = part; t < c.T; t += nparts) {
    sm += cell_stats[((long)t * 2 + 0) * B + b];
    sv += cell_stats[((long)t * 2 + 1) * B + b];
  }
  *m = sm;
  *v = sv;
}

// ------------------------------------------------------------------------------------------
// Backward sweep, FUSED form (large batches): one lane walks one trajectory from T-1 to 0 doing
// the whole cell; each forward row is read once and the cost sums stay in registers, so the pass
// moves E_FWD + E_POST elements per cell instead of the two-pass form's ~2x that.
// ------------------------------------------------------------------------------------------
// LEANW: as in chunk_walk_body (no optional outputs, one shared target: a compile-time count of the memory operations of a cell).
// HZ (per-trajectory horizons, see forward_sweep_body): the walk stays aligned in t across the wave -- the row offsets are wave-uniform
// (make_window, wld, uniform_u32), which holds for a partly active wave but not for lanes that each start at their own Tb - 1. So the
// lane first loads ITS row Tb - 1 with plain per-lane addressing, once per trajectory, and runs the end of the chain and the terminal
// statistics on it; the time loop then comes down from T - 1 for the whole wave and the lane takes no part while t >= Tb. From its
// first live cell on it is the walk as it was: the double-buffered form (d <= 5) finds that cell's row in `row` and fetches cell
// t - 1, the d >= 6 form loads each cell at its top. Rows t >= Tb are neither read nor written.
template <class M, typename R, int GRID = 0, typename S_ = R, bool LEANW = false, bool HZ = false>
I2C_HD inline void backward_fused_body(const Consts<M, R>& c, const CellArgs<R, S_>& a_in, const int b, [[maybe_unused]] const int Tb = 0) {
  static_assert(!HZ || GRID == 0, "per-trajectory horizons: the one-lane walk");
  CellArgs<R, S_> a = a_in;
  if (LEANW) a.xm = nullptr, a.zpost = nullptr, a.cell_stats = nullptr;
  const bool z_per_cell = LEANW ? false : c.z_per_cell != 0;
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NZ = C::NZ, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, O_J = O_S3 + sym(NX);
  constexpr unsigned W = sizeof(S_);
  const unsigned long B = c.B;
  const int T = c.T;
  const unsigned bo = (unsigned)b * W, rb = (unsigned)(B * W);
  const bool wr = grid_writer<GRID>();  // (GRID_WAVE: lane 0 of the trajectory's wavefront; `true` otherwise)

  constexpr bool DOUBLE_BUFFER = C::D <= 5;  // see chunk_walk_body
  constexpr bool VOFF = LEANW && !GRID && C::D <= 5;  // row offsets in VGPRs, sincos table in registers (chunk_walk_body)
  constexpr int NOFF = C::E_FWD > C::E_POST ? C::E_FWD : C::E_POST;
  unsigned voff[VOFF ? NOFF : 1];
  if (VOFF) {
#pragma unroll
    for (int e = 0; e < NOFF; ++e) voff[e] = bo + (unsigned)e * rb;
  }
  PolyTab<R> ptab;
  if (VOFF) poly_tab_init(ptab);
  const PolyTab<R>* const tab = VOFF ? &ptab : nullptr;
  R row[C::E_FWD], nxt[DOUBLE_BUFFER ? C::E_FWD : 1];
  R m3m[NX], S3m[sym(NX)];
  if constexpr (HZ) {
    const S_* in = a.fwd + ((unsigned long)(Tb - 1) * C::E_FWD) * B + b;  // the lane's own last row: per-lane addresses
    if (DOUBLE_BUFFER) {
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e) row[e] = opaque((R)in[(unsigned long)e * B]);
      end_of_chain<M, R, GRID>(c, a.temp, b, row + O_MU3, row + O_S3, m3m, S3m, a.status, Tb - 1);
    } else {
      R m3f[NX], S3f[sym(NX)];
#pragma unroll
      for (int e = 0; e < NX; ++e) m3f[e] = (R)in[(unsigned long)(O_MU3 + e) * B];
#pragma unroll
      for (int e = 0; e < sym(NX); ++e) S3f[e] = (R)in[(unsigned long)(O_S3 + e) * B];
      end_of_chain<M, R, GRID>(c, a.temp, b, m3f, S3f, m3m, S3m, a.status, Tb - 1);
    }
    terminal_obs_stats<M, R, GRID>(c, b, m3m, S3m, a.term_stats, a.status, Tb - 1);
  } else {
  {
    const Window w = make_window(a.fwd + (unsigned long)(T - 1) * C::E_FWD * B, (unsigned long)C::E_FWD * rb);
    if (DOUBLE_BUFFER) {
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e) row[e] = (R)wld<S_>(w, VOFF ? 0u : e * rb, VOFF ? voff[e] : bo);
      if (LEANW) {  // settled before the loop (chunk_walk_body)
#pragma unroll
        for (int e = 0; e < C::E_FWD; ++e) row[e] = opaque(row[e]);
      }
      end_of_chain<M, R, GRID>(c, a.temp, b, row + O_MU3, row + O_S3, m3m, S3m, a.status);
    } else {
      // Only the filtered terminal state here: the loop below loads EVERY cell's row at the top of its own cell, the last
      // one included. Loaded here and skipped there, the row becomes a loop-carried value and all 100+ doubles of it stay
      // live through every cell to the back edge (that was the 452 B per lane of scratch of the d = 7 fused walk).
      R m3f[NX], S3f[sym(NX)];
#pragma unroll
      for (int e = 0; e < NX; ++e) m3f[e] = (R)wld<S_>(w, (O_MU3 + e) * rb, bo);
#pragma unroll
      for (int e = 0; e < sym(NX); ++e) S3f[e] = (R)wld<S_>(w, (O_S3 + e) * rb, bo);
      end_of_chain<M, R, GRID>(c, a.temp, b, m3f, S3f, m3m, S3m, a.status);
    }
  }
  terminal_obs_stats<M, R, GRID>(c, b, m3m, S3m, a.term_stats, a.status);
  }

  R sum_m = R(0), sum_v = R(0);
  for (int t = T - 1; t >= 0; --t) {
    if constexpr (HZ) {
      if (t >= Tb) continue;  // the lane's chain has not begun
    }
    if (DOUBLE_BUFFER) {
      const int tp = t > 0 ? t - 1 : 0;
      const Window w = make_window(a.fwd + (unsigned long)tp * C::E_FWD * B, (unsigned long)C::E_FWD * rb);
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e) nxt[DOUBLE_BUFFER ? e : 0] = (R)wld<S_>(w, VOFF ? 0u : e * rb, VOFF ? voff[e] : bo);
    } else {
      const Window w = make_window(a.fwd + (unsigned long)t * C::E_FWD * B, (unsigned long)C::E_FWD * rb);
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e) row[e] = (R)wld<S_>(w, e * rb, bo);
    }
    if (a.xm && wr) {
      S_* xo = const_cast<S_*>(a.xm) + ((long)t * C::E_XM) * B + b;
#pragma unroll
      for (int i = 0; i < NX; ++i) xo[(long)i * B] = (S_)m3m[i];
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) xo[(long)(NX + i) * B] = (S_)S3m[i];
    }
    R dm[NX], dS[sym(NX)], zt[NZ];
#pragma unroll
    for (int i = 0; i < NX; ++i) dm[i] = m3m[i] - row[O_MU3 + i];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) dS[i] = S3m[i] - row[O_S3 + i];
#pragma unroll
    for (int k = 0; k < NZ; ++k) zt[k] = z_per_cell ? a.z[((long)c.row(t) * NZ + k) * B + b] : c.zg[k];
    R* mu = row;
    R* S = row + D;
    R ctl[C::E_POST - D - sym(D)], mz[NZ], Sz[sym(NZ)], cm, cv;
    if (!cell_posterior<M, R, GRID>(c, b, zt, mu, S, row + O_J, dm, dS, ctl, mz, Sz, &cm, &cv, tab) && wr) set_status(a.status, b, 7, t);
    if (wr) store_cell<M, R, S_>(c, a, t, b, mu, S, ctl, mz, Sz, cm, cv, VOFF ? voff : nullptr);
    sum_m += cm;
    sum_v += cv;
#pragma unroll
    for (int i = 0; i < NX; ++i) m3m[i] = mu[i];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) S3m[i] = S[i];  // xx block = packed prefix
    if (DOUBLE_BUFFER) {
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e) row[e] = nxt[DOUBLE_BUFFER ? e : 0];
    }
  }
  if (wr) {
    a.term_stats[B + b] = sum_m;
    a.term_stats[2 * B + b] = sum_v;
  }
}

// ------------------------------------------------------------------------------------------
// Backward sweep, CHUNKED form (small batches): the x-marginal recursion is affine,
//   (m, S)_t = (a_t + Jx_t m_{t+1},  C_t + Jx_t S_{t+1} Jx_t^T),   a_t = mu_x1_f - Jx_t mu_x3_f,
//                                                                   C_t = sig_x1_f - Jx_t sig_x3_f Jx_t^T,
// so maps compose: T cells are cut into NC chunks, (1) every chunk's composite map (a, G, C) is built
// in parallel [one lane per (chunk, b)], (2) one lane per trajectory applies the NC composites to get
// the smoothed state entering every chunk, (3) every chunk is walked in parallel doing the complete
// cell work from its boundary value. The sequential depth drops from T to ~2 T / NC + NC.
// ------------------------------------------------------------------------------------------
template <typename R, typename S_ = R> struct ChunkArgs {
  CellArgs<R, S_> cell;  // fwd, xm (optional out), z, post, zpost, cell_stats (optional out), term_stats, temp, status
  R* comp;           // [NC][NX + NX*NX + sym(NX)][B]  composite maps
  R* bnd;            // [NC][NX + sym(NX)][B]          smoothed state entering each chunk
  R* part;           // [NC][2][B]                     per-chunk cost sums ([NC][3][B] in the Linearize form)
  int n_chunks, chunk_len;
};

template <class M, typename R, typename S_ = R>
I2C_HD inline void chunk_compose_body(const Consts<M, R>& c, const ChunkArgs<R, S_>& a, const int ch, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, O_J = O_S3 + sym(NX);
  const long B = c.B;
  const int t_lo = ch * a.chunk_len, t_hi = (t_lo + a.chunk_len < c.T) ? t_lo + a.chunk_len : c.T;
  R av[NX], G[NX * NX], Cc[sym(NX)];
#pragma unroll
  for (int i = 0; i < NX; ++i) av[i] = R(0);
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int j = 0; j < NX; ++j) G[i * NX + j] = i == j ? R(1) : R(0);
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) Cc[i] = R(0);
  using Row = ScanRow<NX, R>;
  auto load = [&](int t, Row& r) {
    const S_* in = a.cell.fwd + ((long)t * C::E_FWD) * B + b;
#pragma unroll
    for (int i = 0; i < NX; ++i) r.mu1[i] = in[(long)i * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) r.S1[i] = in[(long)(D + i) * B];
#pragma unroll
    for (int i = 0; i < NX; ++i) r.m3f[i] = in[(long)(O_MU3 + i) * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) r.S3f[i] = in[(long)(O_S3 + i) * B];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) r.Jx[i] = in[(long)(O_J + i) * B];
  };
  Row cur, nxt;
  load(t_hi - 1, cur);
  for (int t = t_hi - 1; t >= t_lo; --t) {
    load(t > t_lo ? t - 1 : t_lo, nxt);  // one cell ahead: the loads do not depend on the composition
    const R* mu1 = cur.mu1;
    const R* S1 = cur.S1;
    const R* m3f = cur.m3f;
    const R* Jx = cur.Jx;
    R S3n[sym(NX)];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) S3n[i] = Cc[i] - cur.S3f[i];  // C - sig_x3_f
    // a <- mu1 + Jx (a - m3f);  C <- S1 + Jx (C - S3f) Jx^T;  G <- Jx G
    R an[NX], Gn[NX * NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      R v = mu1[i];
#pragma unroll
      for (int k = 0; k < NX; ++k) v += Jx[i * NX + k] * (av[k] - m3f[k]);
      an[i] = v;
    }
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) Cc[i] = S1[i];
    add_JDJt<NX, NX>(Jx, S3n, Cc);
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        R v = R(0);
#pragma unroll
        for (int k = 0; k < NX; ++k) v += Jx[i * NX + k] * G[k * NX + j];
        Gn[i * NX + j] = v;
      }
#pragma unroll
    for (int i = 0; i < NX; ++i) av[i] = an[i];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) G[i] = Gn[i];
    cur = nxt;
  }
  constexpr int EC = NX + NX * NX + sym(NX);
  R* out = a.comp + ((long)ch * EC) * B + b;
#pragma unroll
  for (int i = 0; i < NX; ++i) out[(long)i * B] = av[i];
#pragma unroll
  for (int i = 0; i < NX * NX; ++i) out[(long)(NX + i) * B] = G[i];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) out[(long)(NX + NX * NX + i) * B] = Cc[i];
}

// The smoother gain of one cell from the forward sweep's hand-off (ChunkReleaseGain): J holds the differences dl_j[k] of the dynamics
// transform on entry, J = sig_xy sig_x3^-1 [D][NX] on return. S_xu1: sig_xu1_f of the row; S_x3: sig_x3 as the sweep factored it.
// The expressions are the sweep's own, in its order -- chol<D> of section 3, the accumulation and the scaling of sp_transform<CROSS>,
// chol<NX>, fsub and bsub per row --, so that the gain is the bits forward_sweep_body stores without the hand-off.
template <class M, typename R> I2C_FN void gain_from_handoff(const Rule<R>& rule, const R* S_xu1, const R* S_x3, R* J) {
  constexpr int NX = M::NX, D = M::NX + M::NU;
  R L[sym(D)], rinv[D], Sxy[D * NX];
#pragma unroll
  for (int i = 0; i < sym(D); ++i) L[i] = S_xu1[i];
  chol<D>(L, rinv);
#pragma unroll
  for (int k = 0; k < D * NX; ++k) Sxy[k] = R(0);
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int k = 0; k < NX; ++k)
#pragma unroll
      for (int i = j; i < D; ++i) Sxy[i * NX + k] += L[tri(i, j)] * J[j * NX + k];
  const R cs = rule.wi * rule.sf;
#pragma unroll
  for (int k = 0; k < NX; ++k)
#pragma unroll
    for (int i = 0; i < D; ++i) Sxy[i * NX + k] = cs * Sxy[i * NX + k];
  R L3[sym(NX)], rinv3[NX];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) L3[i] = S_x3[i];
  chol<NX>(L3, rinv3);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    fsub<NX>(L3, rinv3, &Sxy[i * NX]);
    bsub<NX>(L3, rinv3, &Sxy[i * NX]);
  }
#pragma unroll
  for (int k = 0; k < D * NX; ++k) J[k] = Sxy[k];
}

// chunk_compose_body behind a sweep that hands the gain over (ChunkReleaseGain; fp64-stored messages): every cell's J is finished from
// its row (gain_from_handoff), stored over the hand-off, and composed from registers -- the composition itself is chunk_compose_body's,
// expression for expression. The rows are fetched a cell ahead as there, so the solves sit under the load round trip of the next row.
// term_sig: the flagged cell's sig_x3 before its terminal update (any t: a receding horizon flags a cell mid-horizon); the source of
// a cell's sig_x3 is chosen by address, without a branch.
template <class M, typename R>
I2C_HD inline void chunk_compose_gain_body(const Consts<M, R>& c, const ChunkArgs<R, R>& a, const R* term_sig, const int ch, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, O_J = O_S3 + sym(NX);
  const long B = c.B;
  const int t_lo = ch * a.chunk_len, t_hi = (t_lo + a.chunk_len < c.T) ? t_lo + a.chunk_len : c.T;
  const int t_term = (C::NZT > 0 && c.has_Qf) ? c.terminal_cell : -1;
  R av[NX], G[NX * NX], Cc[sym(NX)];
#pragma unroll
  for (int i = 0; i < NX; ++i) av[i] = R(0);
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int j = 0; j < NX; ++j) G[i * NX + j] = i == j ? R(1) : R(0);
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) Cc[i] = R(0);
  struct Row {
    R mu1[NX], S1[sym(D)], m3f[NX], S3f[sym(NX)], S3g[sym(NX)], J[D * NX];
  };
  auto load = [&](int t, Row& r) {
    const R* in = a.cell.fwd + ((long)t * C::E_FWD) * B + b;
    const R* s3 = t == t_term ? term_sig + b : in + (long)O_S3 * B;
#pragma unroll
    for (int i = 0; i < NX; ++i) r.mu1[i] = in[(long)i * B];
#pragma unroll
    for (int i = 0; i < sym(D); ++i) r.S1[i] = in[(long)(D + i) * B];
#pragma unroll
    for (int i = 0; i < NX; ++i) r.m3f[i] = in[(long)(O_MU3 + i) * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) r.S3f[i] = in[(long)(O_S3 + i) * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) r.S3g[i] = s3[(long)i * B];
#pragma unroll
    for (int i = 0; i < D * NX; ++i) r.J[i] = in[(long)(O_J + i) * B];
  };
  Row cur, nxt;
  load(t_hi - 1, cur);
  for (int t = t_hi - 1; t >= t_lo; --t) {
    load(t > t_lo ? t - 1 : t_lo, nxt);  // one cell ahead, without a branch (the last one re-reads this row: unused)
    gain_from_handoff<M, R>(c.rule_xu, cur.S1, cur.S3g, cur.J);
    R* out = const_cast<R*>(a.cell.fwd) + ((long)t * C::E_FWD + O_J) * B + b;
#pragma unroll
    for (int i = 0; i < D * NX; ++i) out[(long)i * B] = cur.J[i];
    R Jx[NX * NX];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) Jx[i] = opaque(cur.J[i]);  // as loaded values: the composition contracts as chunk_compose_body's
    const R* mu1 = cur.mu1;
    const R* S1 = cur.S1;  // (the xx block is the packed prefix)
    const R* m3f = cur.m3f;
    R S3n[sym(NX)];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) S3n[i] = Cc[i] - cur.S3f[i];  // C - sig_x3_f
    // a <- mu1 + Jx (a - m3f);  C <- S1 + Jx (C - S3f) Jx^T;  G <- Jx G
    R an[NX], Gn[NX * NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      R v = mu1[i];
#pragma unroll
      for (int k = 0; k < NX; ++k) v += Jx[i * NX + k] * (av[k] - m3f[k]);
      an[i] = v;
    }
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) Cc[i] = S1[i];
    add_JDJt<NX, NX>(Jx, S3n, Cc);
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        R v = R(0);
#pragma unroll
        for (int k = 0; k < NX; ++k) v += Jx[i * NX + k] * G[k * NX + j];
        Gn[i * NX + j] = v;
      }
#pragma unroll
    for (int i = 0; i < NX; ++i) av[i] = an[i];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) G[i] = Gn[i];
    cur = nxt;
  }
  constexpr int EC = NX + NX * NX + sym(NX);
  R* comp = a.comp + ((long)ch * EC) * B + b;
#pragma unroll
  for (int i = 0; i < NX; ++i) comp[(long)i * B] = av[i];
#pragma unroll
  for (int i = 0; i < NX * NX; ++i) comp[(long)(NX + i) * B] = G[i];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) comp[(long)(NX + NX * NX + i) * B] = Cc[i];
}

// One step of the stitch recursion: the smoothed state (m, S) that enters a chunk pushed through that chunk's composite map,
//   m <- a + G m,  S <- C + G S G^T   (Cc is overwritten).
// Written once for the stitch pass and for the self-stitching walker (chunk_boundary_state): the same expressions in the same order
// from the same start, so the boundary states of the two are bit-identical.
template <int NX, typename R> I2C_FN void apply_composite(const R* av, const R* G, R* Cc, R* m, R* S) {
  R mn[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    R v = av[i];
#pragma unroll
    for (int k = 0; k < NX; ++k) v += G[i * NX + k] * m[k];
    mn[i] = v;
  }
  add_JDJt<NX, NX>(G, S, Cc);  // C + G S G^T
#pragma unroll
  for (int i = 0; i < NX; ++i) m[i] = mn[i];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) S[i] = Cc[i];
}

template <class M, typename R, typename S_ = R, int GRID = 0>
I2C_HD inline void chunk_stitch_body(const Consts<M, R>& c, const ChunkArgs<R, S_>& a, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, EC = NX + NX * NX + sym(NX);
  const long B = c.B;
  const S_* last = a.cell.fwd + ((long)(c.T - 1) * C::E_FWD) * B + b;
  R m3f[NX], S3f[sym(NX)], m[NX], S[sym(NX)];
#pragma unroll
  for (int i = 0; i < NX; ++i) m3f[i] = last[(long)(O_MU3 + i) * B];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) S3f[i] = last[(long)(O_S3 + i) * B];
  end_of_chain<M, R>(c, a.cell.temp, b, m3f, S3f, m, S, a.cell.status);
  terminal_obs_stats<M, R, GRID>(c, b, m, S, a.cell.term_stats, a.cell.status);
  R av[NX], G[NX * NX], Cc[sym(NX)], nav[NX], nG[NX * NX], nCc[sym(NX)];
  auto loadc = [&](int ch, R* la, R* lG, R* lC) {
    const R* cp = a.comp + ((long)(ch > 0 ? ch : 0) * EC) * B + b;
#pragma unroll
    for (int i = 0; i < NX; ++i) la[i] = cp[(long)i * B];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) lG[i] = cp[(long)(NX + i) * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) lC[i] = cp[(long)(NX + NX * NX + i) * B];
  };
  loadc(a.n_chunks - 1, av, G, Cc);
  for (int ch = a.n_chunks - 1; ch >= 0; --ch) {
    loadc(ch - 1, nav, nG, nCc);  // next composite, one step ahead
    R* bo = a.bnd + ((long)ch * C::E_XM) * B + b;
#pragma unroll
    for (int i = 0; i < NX; ++i) bo[(long)i * B] = m[i];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) bo[(long)(NX + i) * B] = S[i];
    apply_composite<NX, R>(av, G, Cc, m, S);
#pragma unroll
    for (int i = 0; i < NX; ++i) av[i] = nav[i];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) G[i] = nG[i];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) Cc[i] = nCc[i];
  }
}

// The self-stitching walker's boundary state: the smoothed state entering chunk `ch`, recomputed by that chunk's walker instead of
// read from `bnd` -- the terminal filtered state pushed through the composites of chunks NC-1 .. ch+1, which is what chunk_stitch_body
// stores into bnd[ch]. The stitch pass (a launch and a chain of NC dependent load round trips on B / 64 waves) then does not run.
// Only for problems WITHOUT a terminal state prior: there end_of_chain is the identity on the filtered state (with one it advances
// temp[b], once per trajectory -- several walkers per trajectory would race; Impl::backward_chunked keeps those on the stitch pass).
// The composites are fetched DEPTH at a time, all loads of a batch issued before its first application (one round trip per batch:
// NC <= 16 is one batch for nx = 2); a walker whose suffix is shorter re-reads the composite nearest to it instead (same cache line).
template <class M, typename R, typename S_>
I2C_FN void chunk_boundary_state(const Consts<M, R>& c, const ChunkArgs<R, S_>& a, const int ch, const int b, R* m, R* S) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, EC = NX + NX * NX + sym(NX);
  constexpr int DEPTH = NX <= 2 ? 8 : 4;
  const long B = c.B;
  const S_* last = a.cell.fwd + ((long)(c.T - 1) * C::E_FWD) * B + b;
#pragma unroll
  for (int i = 0; i < NX; ++i) m[i] = last[(long)(O_MU3 + i) * B];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) S[i] = last[(long)(O_S3 + i) * B];
  for (int hi = a.n_chunks - 1; hi > ch; hi -= DEPTH) {
    R comp[DEPTH][EC];
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) {
      const R* cp = a.comp + ((long)(hi - k > ch ? hi - k : ch + 1) * EC) * B + b;
#pragma unroll
      for (int i = 0; i < EC; ++i) comp[k][i] = cp[(long)i * B];
    }
#pragma unroll
    for (int k = 0; k < DEPTH; ++k)
      if (hi - k > ch) apply_composite<NX, R>(comp[k], comp[k] + NX, comp[k] + NX + NX * NX, m, S);
  }
}

// LEANW: the common case fixed at compile time (no smoothed-state / observed-marginal / per-cell-cost outputs, one shared target):
// with the optional stores behind run-time branches the compiler cannot count the memory operations between the row prefetch and
// its use, so its s_waitcnt at the top of a cell also waits for the PREVIOUS cell's stores to be acknowledged (vmcnt is one
// in-order counter) -- 41 % of the walk's cycles (profiles/r3_pendulum_B4096_chunked_sq_summary.txt).
// GRID: the Gauss-Hermite tensor-grid transform in the cell (GaussHermiteQuadrature: the chunked schedule of that rule)
// SELF: the self-stitching form (sigma-point rule, no terminal state prior, d <= 5): the walker computes its own boundary state
// (chunk_boundary_state) behind the prefetch of its first row, and the walker of the LAST chunk -- whose boundary state is the end of
// the chain -- writes the terminal observation statistics, once per trajectory, as the stitch pass does in the four-pass schedule.
template <class M, typename R, typename S_ = R, bool LEANW = false, int GRID = 0, bool SELF = false>
I2C_HD inline void chunk_walk_body(const Consts<M, R>& c, const ChunkArgs<R, S_>& a, const int ch, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NZ = C::NZ, D = C::D;
  constexpr int O_MU3 = D + sym(D), O_S3 = O_MU3 + NX, O_J = O_S3 + sym(NX);
  constexpr unsigned W = sizeof(S_);
  const unsigned long B = c.B;
  const unsigned bo = (unsigned)b * W, rb = (unsigned)(B * W);
  const int t_lo = ch * a.chunk_len, t_hi = (t_lo + a.chunk_len < c.T) ? t_lo + a.chunk_len : c.T;
  CellArgs<R, S_> ca = a.cell;
  if (LEANW) ca.xm = nullptr, ca.zpost = nullptr, ca.cell_stats = nullptr;
  const bool z_per_cell = LEANW ? false : c.z_per_cell != 0;
  R m3m[NX], S3m[sym(NX)];
  if (!SELF) {
    const R* bi = a.bnd + ((long)ch * C::E_XM) * B + b;
#pragma unroll
    for (int i = 0; i < NX; ++i) m3m[i] = bi[(long)i * B];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) S3m[i] = bi[(long)(NX + i) * B];
  }
  // The next cell's forward row is fetched while this cell computes -- but only where a second row fits: for d >= 6 a
  // row is 100+ doubles, two of them overflow the register file into scratch and the walk then waits on scratch traffic
  // 80 % of the time (SQ counters); there the row is loaded at the top of its own cell.
  constexpr bool DOUBLE_BUFFER = C::D <= 5;
  // per-row byte offsets as VGPR values (small models; see forward_sweep_body and store_cell)
  constexpr bool VOFF = I2C_WALK_VOFF && C::D <= 5;
  constexpr int NOFF = C::E_FWD > C::E_POST ? (C::E_FWD > C::E_ZPOST ? C::E_FWD : C::E_ZPOST) : (C::E_POST > C::E_ZPOST ? C::E_POST : C::E_ZPOST);
  unsigned voff[VOFF ? NOFF : 1];
  if (VOFF) {
#pragma unroll
    for (int e = 0; e < NOFF; ++e) voff[e] = bo + (unsigned)e * rb;
  }
  PolyTab<R> ptab;  // sincos coefficients as VGPR values (24 literal moves per cell otherwise), same condition
  if (VOFF) poly_tab_init(ptab);
  const PolyTab<R>* const tab = VOFF ? &ptab : nullptr;
  R row[C::E_FWD], nxt[DOUBLE_BUFFER ? C::E_FWD : 1];
  if (DOUBLE_BUFFER) {
    const Window w = make_window(ca.fwd + (unsigned long)(t_hi - 1) * C::E_FWD * B, (unsigned long)C::E_FWD * rb);
#pragma unroll
    for (int e = 0; e < C::E_FWD; ++e) row[e] = (R)wld<S_>(w, VOFF ? 0u : e * rb, VOFF ? voff[e] : bo);
    // settle them before the loop: the waitcnt pass joins the loop-entry state with the back-edge state, and loads still pending
    // on the entry path (youngest operations there, but older than a cell's stores on the back edge) make it wait for
    // vmcnt(0) -- the previous cell's stores -- at the top of EVERY cell (see forward_sweep_body)
    if (SELF) {  // (younger than the row's loads in the in-order counter: the settling below covers them as well)
      static_assert(!SELF || (GRID == 0 && DOUBLE_BUFFER), "the self-stitching walker: sigma-point rule, d <= 5");
      chunk_boundary_state<M, R, S_>(c, a, ch, b, m3m, S3m);
      if (ch == a.n_chunks - 1) terminal_obs_stats<M, R, GRID>(c, b, m3m, S3m, ca.term_stats, ca.status);
    }
    if (LEANW) {
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e) row[e] = opaque(row[e]);
    }
  }
  R sum_m = R(0), sum_v = R(0);
  for (int t = t_hi - 1; t >= t_lo; --t) {
    {
      const int tp = DOUBLE_BUFFER ? (t > t_lo ? t - 1 : t_lo) : t;
      const Window w = make_window(ca.fwd + (unsigned long)tp * C::E_FWD * B, (unsigned long)C::E_FWD * rb);
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e)
        (DOUBLE_BUFFER ? nxt[DOUBLE_BUFFER ? e : 0] : row[e]) = (R)wld<S_>(w, VOFF ? 0u : e * rb, VOFF ? voff[e] : bo);
    }
    if (ca.xm) {
      S_* xo = const_cast<S_*>(ca.xm) + ((long)t * C::E_XM) * B + b;
#pragma unroll
      for (int i = 0; i < NX; ++i) xo[(long)i * B] = (S_)m3m[i];
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) xo[(long)(NX + i) * B] = (S_)S3m[i];
    }
    R dm[NX], dS[sym(NX)], zt[NZ];
#pragma unroll
    for (int i = 0; i < NX; ++i) dm[i] = m3m[i] - row[O_MU3 + i];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) dS[i] = S3m[i] - row[O_S3 + i];
    if (VOFF && z_per_cell) {  // (NZ <= E_FWD: the row offsets cover it; R-typed rows: 8 / sizeof(S_) scales them)
      static_assert(NZ <= NOFF, "row offsets");
      const Window wz = make_window(ca.z + (unsigned long)c.row(t) * NZ * B, (unsigned long)NZ * B * sizeof(R));
#pragma unroll
      for (int k = 0; k < NZ; ++k) zt[k] = wld<R>(wz, 0u, voff[k] * (unsigned)(sizeof(R) / W));
    } else {
#pragma unroll
      for (int k = 0; k < NZ; ++k) zt[k] = z_per_cell ? ca.z[((long)c.row(t) * NZ + k) * B + b] : c.zg[k];
    }
    R* mu = row;
    R* S = row + D;
    R ctl[C::E_POST - D - sym(D)], mz[NZ], Sz[sym(NZ)], cm, cv;
    if (!cell_posterior<M, R, GRID>(c, b, zt, mu, S, row + O_J, dm, dS, ctl, mz, Sz, &cm, &cv, tab)) set_status(ca.status, b, 7, t);
    store_cell<M, R, S_>(c, ca, t, b, mu, S, ctl, mz, Sz, cm, cv, VOFF ? voff : nullptr);
    sum_m += cm;
    sum_v += cv;
#pragma unroll
    for (int i = 0; i < NX; ++i) m3m[i] = mu[i];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) S3m[i] = S[i];
    if (DOUBLE_BUFFER) {
#pragma unroll
      for (int e = 0; e < C::E_FWD; ++e) row[e] = nxt[DOUBLE_BUFFER ? e : 0];
    }
  }
  a.part[((long)ch * 2 + 0) * B + b] = sum_m;
  a.part[((long)ch * 2 + 1) * B + b] = sum_v;
}

// ------------------------------------------------------------------------------------------
// M-step on the temperature (i2c.py:913-963, 1045-1053). One lane per trajectory, O(1) work:
// the sums over t were produced by the backward sweep (term_stats rows 1, 2).
// ------------------------------------------------------------------------------------------
template <typename R> struct MstepArgs {
  const R* term_stats;  // [E_TERM][B]
  R* alpha;             // [B]
  R* stats_out;         // [4][B]
  int update;
};

// The M-step on values: `stat`, `v`, `m` = the alpha statistic, the cost variance and the plan cost (term_stats rows 1, 2 and, under
// Linearize, the last one), `trT` = the terminal statistic (row 0), `alpha` = the trajectory's temperature. mstep_body reads them
// from term_stats; the prologue of k_forward_mstep (i2c_impl.hpp) has them in registers.
template <class M, typename R>
I2C_FN void mstep_update(const Consts<M, R>& c, const MstepArgs<R>& a, const int b, const R trT, const R stat, const R v, const R m,
                         const R alpha, const int T_own = 0) {  // T_own: the trajectory's own horizon (I2cProblem.horizons); 0: c.T
  using C = Consts<M, R>;
  const long B = c.B;
  R tr = stat, sf = R(C::NZ) * R(T_own > 0 ? T_own : c.T);
  if (C::NZT > 0 && c.has_Qf) {
    tr += trT;
    sf += R(C::NZT);
  }
  const R alpha_hat = tr / sf;
  R alpha_new = alpha;
  if (a.update) {
    if (c.tol >= R(0)) {  // i2c.py:953-959
      const R ratio = alpha_hat / alpha;
      alpha_new = alpha_hat;
      if (ratio < c.tol) alpha_new = c.tol * alpha;
      if (ratio > R(2) - c.tol) alpha_new = (R(2) - c.tol) * alpha;
    }
    a.alpha[b] = alpha_new;
  }
  a.stats_out[b] = alpha_hat;
  a.stats_out[B + b] = alpha_new;
  a.stats_out[2 * B + b] = m;
  a.stats_out[3 * B + b] = v;
}
template <class M, typename R>
I2C_HD inline void mstep_body(const Consts<M, R>& c, const MstepArgs<R>& a, const int b, const int T_own = 0) {
  using C = Consts<M, R>;
  const long B = c.B;
  // row 1 is the alpha statistic sum_t tr(QR (err err^T + sig_z0_m)); in the sigma-point path it IS the plan cost,
  // the Linearize path reports the cost of the graph's cubature transform separately (last row)
  const R stat = a.term_stats[B + b], v = a.term_stats[2 * B + b];
  const R m = c.inference == I2C_INF_LINEARIZE ? a.term_stats[(long)(C::E_TERM - 1) * B + b] : stat;
  const R trT = (C::NZT > 0 && c.has_Qf) ? a.term_stats[b] : R(0);
  mstep_update<M, R>(c, a, b, trT, stat, v, m, a.alpha[b], T_own);
}

// ------------------------------------------------------------------------------------------
// Closed-loop propagation (i2c.py:150-199, 1247-1251): forward-only rollout of the controller
// distribution through the model. One lane per trajectory.
// ------------------------------------------------------------------------------------------
template <typename R> struct PropArgs {
  const R* post;   // [T][E_POST][B]
  R* prop;         // [T][E_PROP][B]
  R* prop_stats;   // [3][B]: sum_t of the propagated cost mean / variance, KL of the final state to the terminal prior
  const R* x0;
  const R* sig_x0;
  const R* z;
  const uint8_t* ff;
  int32_t* status;
  const uint8_t* expert;  // [T] ring or null: per-cell use_expert_controller (i2c.py:143,160); null: Consts::use_expert
};

// HZ (per-trajectory horizons, see forward_sweep_body): the lane's cells end at its horizon Tb; every row address here is the lane's
// own, so the one-cell-ahead fetches simply clamp to the lane's last cell, and the KL row is that of cell Tb - 1.
template <class M, typename R, int GRID = 0, bool HZ = false>
I2C_HD inline void propagate_body(const Consts<M, R>& c, const PropArgs<R>& a, const int b, [[maybe_unused]] const int Tb = 0) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NU = C::NU, NZ = C::NZ, D = C::D;
  const long B = c.B;
  const int T = HZ ? Tb : c.T;
  const bool wr = grid_writer<GRID>();  // (GRID_WAVE: lane 0 of the trajectory's wavefront; `true` otherwise)
  R mu_x[NX], sig_x[sym(NX)];
#pragma unroll
  for (int i = 0; i < NX; ++i) mu_x[i] = a.x0[i * B + b];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) sig_x[i] = a.sig_x0[i * B + b];
  // the posterior rows of the next cell are fetched a cell ahead where a second set fits (see forward_sweep_body)
  constexpr bool PREFETCH = C::D <= 5;
  R pri[C::E_PRI];
  if (PREFETCH) {
#pragma unroll
    for (int e = 0; e < C::E_PRI; ++e) pri[e] = a.post[((long)c.row(0) * C::E_POST + e) * B + b];
  }
  // The mode and expert flags of a cell are bytes in global memory: loaded at the top of their own cell they are dependent
  // loads whose full latency -- plus, vmcnt being one in-order counter, the acknowledgement of the previous cell's stores and
  // the arrival of the rows just requested -- is exposed EVERY cell (see forward_sweep_body). Fetched one cell ahead, and
  // everything settled before the loop (a load pending on the loop-entry path makes the waitcnt pass wait for vmcnt(0) at the top).
  unsigned ff_cur = a.ff[c.row(0)], ex_cur = a.expert ? (unsigned)a.expert[c.row(0)] : (unsigned)(c.use_expert != 0);
  if constexpr (HZ) ff_cur = T == 1 ? 1u : ff_cur;  // (a trajectory of one cell stays in feed-forward mode: forward_sweep_body)
  ff_cur = opaque(ff_cur);
  ex_cur = opaque(ex_cur);
  if (PREFETCH) {
#pragma unroll
    for (int e = 0; e < C::E_PRI; ++e) pri[e] = opaque(pri[e]);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) mu_x[i] = opaque(mu_x[i]);
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) sig_x[i] = opaque(sig_x[i]);
  // The per-cell target too: a load behind a run-time branch in the middle of the cell leaves an s_waitcnt vmcnt(0) at the join,
  // which every cell pays with the acknowledgement of the stores it has just issued. Small models: fetched a cell ahead and
  // WITHOUT a branch (when there are no per-cell targets the loads read the trajectory's x0 row and are discarded).
  constexpr bool ZPRE = PREFETCH && NZ <= NX * 4;
  R zt_cur[ZPRE ? NZ : 1];
  auto fetch_z = [&](const int row, R* zt) {
    const R* src = c.z_per_cell ? a.z + ((long)row * NZ) * B + b : a.x0 + b;
    const long st = c.z_per_cell ? B : 0;
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
      const R v = src[(long)k * st];
      zt[k] = c.z_per_cell ? v : c.zg[k];
    }
  };
  if (ZPRE) {
    fetch_z(c.row(0), zt_cur);
#pragma unroll
    for (int k = 0; k < NZ; ++k) zt_cur[k] = opaque(zt_cur[k]);
  }
  R sum_m = R(0), sum_v = R(0);
  bool dead = false;  // this trajectory has failed at this or an earlier cell (see nan_if)

  // (HZ: the loop itself stays wave-uniform and a lane that is done sits the rest out -- leaving the loop lane by lane would keep a
  //  copy of everything that is live behind it, the state and the sums, per exit: scratch for the d >= 6 models)
  for (int t = 0; t < (HZ ? c.T : T); ++t) {
    if constexpr (HZ) {
      if (t >= T) continue;
    }
    R nxt[PREFETCH ? C::E_PRI : 1];
    const int tn1 = t + 1 < T ? t + 1 : t;  // the next cell (flags), and where a second set of rows fits also its rows
    const int tn = PREFETCH ? tn1 : t;
#pragma unroll
    for (int e = 0; e < C::E_PRI; ++e)
      (PREFETCH ? nxt[PREFETCH ? e : 0] : pri[e]) = a.post[((long)c.row(tn) * C::E_POST + e) * B + b];
    const R* qmu = pri;
    const R* qsig = pri + D;
    const R* Kpost = pri + D + sym(D);

    R mu0[D], S0[sym(D)], Kt[NU * NX], sig_u[sym(NU)];
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) Kt[i] = Kpost[i];
    const unsigned ff_now = ff_cur, ex_now = ex_cur;
    R zt_nxt[ZPRE ? NZ : 1];
    if (ZPRE) fetch_z(c.row(tn1), zt_nxt);
    // (HZ: the flags are one [T] array for the whole batch: the next cell's index stays wave-uniform, clamped to the allocated T)
    if constexpr (HZ) {
      const int tnf = t + 1 < c.T ? t + 1 : t;
      ff_cur = a.ff[tnf];
      if (a.expert) ex_cur = a.expert[tnf];
    } else {
    ff_cur = a.ff[c.row(tn1)];  // the next cell's flags, a whole cell ahead of their use
    if (a.expert) ex_cur = a.expert[c.row(tn1)];
    }
    if (ff_now) {  // i2c.py:155-157: action marginal, but the joint still carries K sig_x (i2c.py:173-179)
#pragma unroll
      for (int p = 0; p < NU; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) sig_u[tri(p, q)] = qsig[tri(NX + p, NX + q)];
      joint_from_gain<NX, NU>(mu_x, sig_x, Kt, mu_x, qmu + NX, sig_u, mu0, S0);
    } else {
      if (ex_now != 0) {  // i2c.py:160-167
        R S[sym(NX)], delta[NX];
#pragma unroll
        for (int i = 0; i < sym(NX); ++i) S[i] = qsig[i] + sig_x[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) delta[i] = mu_x[i] - qmu[i];
        bool ok;
        const R rho = pdf_ratio<NX>(S, delta, &ok);
        if (ok) {  // the reference logs the exception and keeps K unscaled (i2c.py:166-167)
#pragma unroll
          for (int i = 0; i < NU * NX; ++i) Kt[i] *= rho;
        }
      }
      // sig_u0_pf = K sig_x0_pf K^T + sig_u0_m - K sig_x0_m K^T  (i2c.py:169-171)
      R q1[sym(NU)], q2[sym(NU)];
      gain_quad<NX, NU>(Kt, sig_x, q1);
      gain_quad<NX, NU>(Kt, qsig, q2);
#pragma unroll
      for (int p = 0; p < NU; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) sig_u[tri(p, q)] = q1[tri(p, q)] + qsig[tri(NX + p, NX + q)] - q2[tri(p, q)];
      joint_from_gain<NX, NU>(mu_x, sig_x, Kt, qmu, qmu + NX, sig_u, mu0, S0);
    }
    R* out = a.prop + ((long)t * C::E_PROP) * B + b;
    if (wr) {
#pragma unroll
      for (int e = 0; e < D; ++e) out[(long)e * B] = mu0[e];
#pragma unroll
      for (int e = 0; e < sym(D); ++e) out[(long)(D + e) * B] = S0[e];
    }

    R L0[sym(D)], rinv[D];
#pragma unroll
    for (int e = 0; e < sym(D); ++e) L0[e] = S0[e];
    const bool ok0 = chol<D>(L0, rinv);
    if (!ok0 && wr) set_status(a.status, b, 8, t);
    dead = dead || !ok0;
    R zt[NZ], mz[NZ], Sz[sym(NZ)];
#pragma unroll
    for (int k = 0; k < NZ; ++k) zt[k] = ZPRE ? zt_cur[ZPRE ? k : 0] : (c.z_per_cell ? a.z[((long)c.row(t) * NZ + k) * B + b] : c.zg[k]);
    transform<GRID, M, ObsStruct<M>, D, NZ, false>(c.rule_xu, mu0, S0, L0, ObserveF<M, R>{params_of(c, b)}, mz, Sz, (R*)nullptr);
    R cm, cv;
    gaussian_cost<NZ>(c.QR, c.qr_diag != 0, mz, Sz, zt, &cm, &cv);
    sum_m += cm;
    sum_v += cv;

    if constexpr (GRID == 0 && has_process_noise<M, R>::value) {  // sum_p w_p (sig_eta + Q(x_p))
      R qn[sym(NX)];
      transform<GRID, M, DenseStruct<D>, D, NX, false>(c.rule_xu, mu0, S0, L0, DynamicsNoiseF<M, R>{{params_of(c, b)}, qn}, mu_x, sig_x, (R*)nullptr);
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) sig_x[i] += c.sig_eta_w[i] + qn[i];
    } else {
      transform<GRID, M, DenseStruct<D>, D, NX, false>(c.rule_xu, mu0, S0, L0, DynamicsF<M, R>{params_of(c, b)}, mu_x, sig_x, (R*)nullptr);
#pragma unroll
      for (int i = 0; i < sym(NX); ++i) sig_x[i] += c.sig_eta_w[i];
    }
    if (wr) {
#pragma unroll
      for (int e = 0; e < NX; ++e) out[(long)(D + sym(D) + e) * B] = nan_if(dead, mu_x[e]);  // (rows of a failed trajectory: NaN from the failing cell on)
#pragma unroll
      for (int e = 0; e < sym(NX); ++e) out[(long)(D + sym(D) + NX + e) * B] = sig_x[e];
    }
    if (ZPRE) {
#pragma unroll
      for (int k = 0; k < NZ; ++k) zt_cur[k] = zt_nxt[ZPRE ? k : 0];
    }
    if (PREFETCH) {
#pragma unroll
      for (int e = 0; e < C::E_PRI; ++e) pri[e] = nxt[PREFETCH ? e : 0];
    }
  }
  if (wr) {
    a.prop_stats[b] = sum_m;
    a.prop_stats[B + b] = sum_v;
  }
  // KL(x3_pf[T-1] || terminal prior) of covariance control (I2cGraph._maximize, i2c.py:1012-1019, mvn_kl_divergence
  // :1223-1229) from the two Cholesky factors: log det ratio = 2 sum log(L2_ii / L1_ii), tr(S2^-1 S1) = ||L2^-1 L1||_F^2.
  R kl = R(0);
  if (c.has_x_terminal) {
    R L1[sym(NX)], r1[NX], L2[sym(NX)], r2[NX];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) {
      L1[i] = sig_x[i];
      L2[i] = c.sig_x_term[i];
    }
    const bool ok = chol<NX>(L1, r1) && chol<NX>(L2, r2);
    if (!ok && wr) set_status(a.status, b, 8, T - 1);
    R logdet = R(0), tr = R(0), dq[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      logdet += r_log(r1[i]) - r_log(r2[i]);  // log(L2_ii) - log(L1_ii) with r = 1 / L_ii
      dq[i] = c.mu_x_term[i] - mu_x[i];
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) {  // column j of L2^-1 L1
      R col[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = i >= j ? L1[tri(i, j)] : R(0);
      fsub<NX>(L2, r2, col);
#pragma unroll
      for (int i = 0; i < NX; ++i) tr += col[i] * col[i];
    }
    fsub<NX>(L2, r2, dq);
    R maha = R(0);
#pragma unroll
    for (int i = 0; i < NX; ++i) maha += dq[i] * dq[i];
    kl = R(0.5) * (R(2) * logdet + tr + maha - R(NX));
  }
  if (wr) a.prop_stats[2 * B + b] = kl;
}

// ------------------------------------------------------------------------------------------
// Cubature Kalman filter step of the MPC state estimator (PartiallyObservedMpcPolicy.filter,
// i2c/policy/mpc.py:125-145): predict the belief through the dynamics with the applied action,
// then innovate on the measurement y. One lane per trajectory.
// ------------------------------------------------------------------------------------------
template <typename R> struct CkfArgs {
  const R* y;       // [NY][B]
  const R* u;       // [NU][B]
  R* mu;            // [NX][B]      in/out
  R* cov;           // [sym NX][B]  in/out
  int32_t* status;  // [B]
};

template <class M, typename R>
I2C_HD inline void ckf_filter_body(const Consts<M, R>& c, const R* sig_zeta, const CkfArgs<R>& a, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NU = C::NU, NY = M::NY;
  const long B = c.B;
  R mu[NX], S[sym(NX)], L[sym(NX)], rinv[NX], u[NU], y[NY];
#pragma unroll
  for (int i = 0; i < NX; ++i) mu[i] = a.mu[(long)i * B + b];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) L[i] = S[i] = a.cov[(long)i * B + b];
#pragma unroll
  for (int i = 0; i < NU; ++i) u[i] = a.u[(long)i * B + b];
#pragma unroll
  for (int i = 0; i < NY; ++i) y[i] = a.y[(long)i * B + b];
  bool ok = chol<NX>(L, rinv);
  // prediction (mpc.py:129-137): x-only sigma points, the action is appended unchanged
  R mf[NX], Sf[sym(NX)];
  if constexpr (has_process_noise<M, R>::value) {  // sum_p w_p (sig_eta + Q(x_p, u)), the applied action fixed
    R qn[sym(NX)];
    sp_transform<M, DenseStruct<NX>, NX, NX, false>(c.rule_x, mu, S, L, DynamicsFixedUNoiseF<M, R>{{params_of(c, b), u}, qn}, mf, Sf,
                                                    (R*)nullptr);
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) L[i] = Sf[i] = Sf[i] + c.rule_x.W * c.sig_eta[i] + qn[i];
  } else {
    sp_transform<M, DenseStruct<NX>, NX, NX, false>(c.rule_x, mu, S, L, DynamicsFixedUF<M, R>{params_of(c, b), u}, mf, Sf,
                                                    (R*)nullptr);
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) L[i] = Sf[i] = Sf[i] + c.rule_x.W * c.sig_eta[i];
  }
  ok = chol<NX>(L, rinv) && ok;
  // innovation (mpc.py:139-145): K = sig_xy sig_y^{-1}; mu = mu_f + K (y - mu_y); cov = sig_f - K sig_y K^T
  R my[NY], Sy[sym(NY)], Sxy[NX * NY];
  sp_transform<M, MeasStruct<M>, NX, NY, true>(c.rule_x, mf, Sf, L, MeasureF<M, R>{params_of(c, b)}, my, Sy, Sxy);
#pragma unroll
  for (int i = 0; i < sym(NY); ++i) Sy[i] += sig_zeta[i];
  ok = kalman_update<NX, NY>(mf, Sf, my, Sy, Sxy, y) && ok;
#pragma unroll
  for (int i = 0; i < NX; ++i) a.mu[(long)i * B + b] = mf[i];
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) a.cov[(long)i * B + b] = Sf[i];
  if (!ok) set_status(a.status, b, 9, 0);
}

// ------------------------------------------------------------------------------------------
// Policy rollouts through the (noisy) known model: replaces BaseSim.run / batch_eval
// (i2c/env.py:40-103, BaseKnownSim.forward :180-187) driven by the time-indexed linear-Gaussian
// policies of i2c/policy/linear.py. One lane per rollout n = r * B + b (r-th rollout of trajectory
// b), T sequential steps; the disturbance samples are supplied by the caller as standard normals so
// that a rollout is a deterministic function of its inputs.
// ------------------------------------------------------------------------------------------
// Le = chol(sig_eta + Q(xu)) of a model with process_noise (the sampling kernels); false: not positive definite
template <class M, typename R> I2C_FN bool step_noise_factor(const R* sig_eta, const R* prm, const R* xu, const R* sn, const R* cs, R* Le) {
  constexpr int NX = M::NX;
  R q[sym(NX)], rinv[NX];
  M::process_noise(prm, xu, sn, cs, q);
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) Le[i] = sig_eta[i] + q[i];
  return chol<NX>(Le, rinv);
}

template <typename R> struct RolloutArgs {
  const R* post;     // [T][E_POST][B]  posterior + controller written by the backward sweep
  const R* x0;       // [NX][B]
  const R* sig_x0;   // [sym NX][B]
  const R* eps_x0;   // [NX][N] or null: x0 ~ N(x0, sig_x0) (BaseLinear.init_env, env.py:195-197)
  const R* eps_x;    // [T][NX][N] or null: process noise chol(sig_eta) eps (env.py:184-186)
  const R* eps_u;    // [T][NU][N] or null: action noise chol(sigK) eps (linear.py:36-41, 86-90)
  R* xu;             // [T][D][N]  or null: (x_t, u_t)                      (env.py:66-68)
  R* z;              // [T][NZ][N] or null: observe(x_t, u_t)               (env.py:70)
  R* x_final;        // [NX][N]    or null: state after the last step
  R* z_term;         // [NZT][N]   or null: observe_terminal(x_T)           (env.py:73)
  int n_rollouts;    // N = n_rollouts * B
  int policy;        // 0: u = K x + k (TimeIndexedLinearGaussianPolicy); 1: expert, soft weight;
                     // 2: expert, hard weight (ExpertTimeIndexedLinearGaussianPolicy, linear.py:46-90)
};

// Where a rollout's standard normals come from is a compile-time choice of the body: the caller's tensors (GivenNoise: i2c_rollout,
// a NULL pointer switches that kind off), or per kind the caller's tensor where it is given and else the counter-based generator
// of i2c_random.hpp (EvalNoise: i2c_rollout_eval). draw_*() readies the normals of one vector, x0() / x() / u() hand out element j.
template <int NX, int NU, typename R, typename IDX> struct GivenNoise {
  const R *e0, *ex, *eu;
  long N;
  IDX n;  // column of this rollout in the tensors
  I2C_HD inline bool x0_on() const { return e0 != nullptr; }
  I2C_HD inline bool x_on() const { return ex != nullptr; }
  I2C_HD inline bool u_on() const { return eu != nullptr; }
  I2C_HD inline void draw_x0() {}
  I2C_HD inline void draw_x(int) {}
  I2C_HD inline void draw_u(int) {}
  I2C_HD inline R x0(const int j) const { return e0[(long)j * N + n]; }
  I2C_HD inline R x(const int t, const int j) const { return ex[((long)t * NX + j) * N + n]; }
  I2C_HD inline R u(const int t, const int j) const { return eu[((long)t * NU + j) * N + n]; }
};
template <int NX, int NU, typename R> struct EvalNoise {
  GivenNoise<NX, NU, R, long> g;
  uint64_t seed;
  uint32_t traj, r;  // counter words 0 and 1: global trajectory, rollout
  int bits;          // I2cRolloutEval.noise
  R z0[NX], zx[NX], zu[NU];
  I2C_HD inline bool x0_on() const { return g.e0 != nullptr || (bits & 4); }
  I2C_HD inline bool x_on() const { return g.ex != nullptr || (bits & 1); }
  I2C_HD inline bool u_on() const { return g.eu != nullptr || (bits & 2); }
  I2C_HD inline void draw_x0() {
    if (g.e0) {
#pragma unroll
      for (int j = 0; j < NX; ++j) z0[j] = g.x0(j);
    } else {
      normals<NX>(seed, traj, r, RNG_T_X0, RNG_X0, z0);
    }
  }
  I2C_HD inline void draw_x(const int t) {
    if (g.ex) {
#pragma unroll
      for (int j = 0; j < NX; ++j) zx[j] = g.x(t, j);
    } else {
      normals<NX>(seed, traj, r, (uint32_t)t, RNG_PROCESS, zx);
    }
  }
  I2C_HD inline void draw_u(const int t) {
    if (g.eu) {
#pragma unroll
      for (int j = 0; j < NU; ++j) zu[j] = g.u(t, j);
    } else {
      normals<NU>(seed, traj, r, (uint32_t)t, RNG_ACTION, zu);
    }
  }
  I2C_HD inline R x0(const int j) const { return z0[j]; }
  I2C_HD inline R x(int, const int j) const { return zx[j]; }
  I2C_HD inline R u(int, const int j) const { return zu[j]; }
};

// What i2c_rollout_eval adds to a rollout (the ACCUMULATING sink of the body, against the row stores of i2c_rollout): the cost of
// the rollout in a register, and the partial moment sums of the lane's part.
template <typename R> struct EvalArgs {
  const R* z;    // [T][NZ][B] per-cell targets of the problem, or null (c.zg)
  R* cost;       // [n_rollouts][B]
  R* work;       // [parts][T][D + sym D][B] or null: S1 = sum delta, S2 = sum delta delta^T of each part, delta = (x, u) - planned mean
  uint64_t seed;
  uint32_t first_trajectory;
  int noise, parts;
};

// y^T W y, W packed lower
template <int N, typename R> I2C_FN R quad_form(const R* W, const R* y) {
  R q = R(0);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    R r = R(0);
#pragma unroll
    for (int j = 0; j < i; ++j) r += W[tri(i, j)] * y[j];
    q += y[i] * (W[tri(i, i)] * y[i] + R(2) * r);
  }
  return q;
}

// HZ (per-trajectory horizons): rollout n runs trajectory n % B's horizon Tb; x_final and z_term are the state behind cell Tb - 1
// EVAL (i2c_rollout_eval): the same steps with the noise of EvalNoise and the accumulating sink: `n` is the trajectory b, `r` the
// rollout, `q` the lane's part, `first` says that this is the first rollout the lane adds to its part's sums (it STORES them, later
// ones load, add and store: the workspace needs no clearing)
template <class M, typename R, bool HZ = false, bool EVAL = false>
I2C_HD inline void rollout_body(const Consts<M, R>& c, const RolloutArgs<R>& a, const int n, [[maybe_unused]] const int Tb = 0,
                                [[maybe_unused]] const EvalArgs<R>* ev = nullptr, [[maybe_unused]] const int r = 0,
                                [[maybe_unused]] const int q = 0, [[maybe_unused]] const bool first = true) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NU = C::NU, NZ = C::NZ, NZT = C::NZT, D = C::D, NA1 = M::NA > 0 ? M::NA : 1;
  const long B = c.B, N = (long)a.n_rollouts * B;
  const int b = EVAL ? n : n % c.B;
  const int T = HZ ? Tb : c.T;
  std::conditional_t<EVAL, EvalNoise<NX, NU, R>, GivenNoise<NX, NU, R, int>> nz;
  if constexpr (EVAL) nz = {{a.eps_x0, a.eps_x, a.eps_u, N, (long)r * B + b}, ev->seed, ev->first_trajectory + (uint32_t)b, (uint32_t)r, ev->noise, {}, {}, {}};
  else nz = {a.eps_x0, a.eps_x, a.eps_u, N, n};
  [[maybe_unused]] R cost = R(0);
  R pb[C::NP1];
  const R* prm = c.params;
  if constexpr (is_per_traj<M>::value) prm = param_ptr<M::NP>(params_of(c, b), pb);  // rollout n runs trajectory n % B's plant
  R x[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = a.x0[i * B + b];
  if (nz.x0_on()) {
    R L[sym(NX)], rinv[NX];
#pragma unroll
    for (int i = 0; i < sym(NX); ++i) L[i] = a.sig_x0[i * B + b];
    chol<NX>(L, rinv);
    nz.draw_x0();
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) x[i] += L[tri(i, j)] * nz.x0(j);
  }
  R Le[sym(NX)], rinv_e[NX];  // chol(sig_eta), constant (a model with process_noise: refactored at every step)
#pragma unroll
  for (int i = 0; i < sym(NX); ++i) Le[i] = c.sig_eta[i];
  if (nz.x_on()) chol<NX>(Le, rinv_e);

  for (int t = 0; t < T; ++t) {
    const long es = c.post_es();
    const R* row = a.post + ((long)c.row(t) * C::E_POST) * B + c.post_bo(b);
    R u[NU], Kc[NU * NX];
#pragma unroll
    for (int e = 0; e < NU * NX; ++e) Kc[e] = row[(long)(D + sym(D) + e) * es];
    if (a.policy == 0) {  // u = K x + k
#pragma unroll
      for (int p = 0; p < NU; ++p) {
        R v = row[(long)(C::E_PRI + p) * es];
#pragma unroll
        for (int k = 0; k < NX; ++k) v += Kc[p * NX + k] * x[k];
        u[p] = v;
      }
    } else {  // u = mu_u + w K (x - mu_x), w = exp(-maha/2) (soft) or [maha/2 < 3] (hard); lam = sig_x^{-1}
      R dlt[NX], q[NX], S[sym(NX)], rinv[NX];
#pragma unroll
      for (int k = 0; k < NX; ++k) q[k] = dlt[k] = x[k] - row[(long)k * es];
#pragma unroll
      for (int k = 0; k < sym(NX); ++k) S[k] = row[(long)(D + k) * es];
      chol<NX>(S, rinv);
      fsub<NX>(S, rinv, q);
      R half = R(0);
#pragma unroll
      for (int k = 0; k < NX; ++k) half += q[k] * q[k];
      half *= R(0.5);
      const R w = a.policy == 1 ? r_exp(-half) : (half < R(3) ? R(1) : R(0));
#pragma unroll
      for (int p = 0; p < NU; ++p) {
        R v = R(0);
#pragma unroll
        for (int k = 0; k < NX; ++k) v += Kc[p * NX + k] * dlt[k];
        u[p] = row[(long)(NX + p) * es] + w * v;
      }
    }
    if (nz.u_on()) {  // u += chol(sigK) eps
      R Lk[sym(NU)], rk[NU];
#pragma unroll
      for (int k = 0; k < sym(NU); ++k) Lk[k] = row[(long)(C::E_PRI + NU + k) * es];
      chol<NU>(Lk, rk);
      nz.draw_u(t);
#pragma unroll
      for (int p = 0; p < NU; ++p)
#pragma unroll
        for (int q2 = 0; q2 <= p; ++q2) u[p] += Lk[tri(p, q2)] * nz.u(t, q2);
    }
    R xu[D], sn[NA1], cs[NA1], zt[NZ], xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xu[i] = x[i];
#pragma unroll
    for (int i = 0; i < NU; ++i) xu[NX + i] = u[i];
#pragma unroll
    for (int q2 = 0; q2 < M::NA; ++q2) r_sincos(xu[M::ang(q2)], &sn[q2], &cs[q2]);
    M::observe(prm, xu, sn, cs, zt);
    M::dynamics(prm, xu, sn, cs, xn);
    if constexpr (EVAL) {  // the accumulating sink: this step's cost, and (x, u) - planned mean into the part's sums
#pragma unroll
      for (int k = 0; k < NZ; ++k) zt[k] -= ev->z ? ev->z[((long)c.row(t) * NZ + k) * B + b] : c.zg[k];
      cost += quad_form<NZ>(c.QR, zt);
      if (ev->work) {
        R* w = ev->work + (((long)q * c.T + t) * (D + sym(D))) * B + b;
        R dl[D];
#pragma unroll
        for (int i = 0; i < D; ++i) dl[i] = xu[i] - row[(long)i * es];
        if (first) {
#pragma unroll
          for (int i = 0; i < D; ++i) w[(long)i * B] = dl[i];
#pragma unroll
          for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) w[(long)(D + tri(i, j)) * B] = dl[i] * dl[j];
        } else {
#pragma unroll
          for (int i = 0; i < D; ++i) w[(long)i * B] += dl[i];
#pragma unroll
          for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) w[(long)(D + tri(i, j)) * B] += dl[i] * dl[j];
        }
      }
    } else {
      if (a.xu) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.xu[((long)t * D + i) * N + n] = xu[i];
      }
      if (a.z) {
#pragma unroll
        for (int i = 0; i < NZ; ++i) a.z[((long)t * NZ + i) * N + n] = zt[i];
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = xn[i];
    if (nz.x_on()) {
      nz.draw_x(t);
      if constexpr (has_process_noise<M, R>::value) {  // x' = f(x, u) + chol(sig_eta + Q(x, u)) eps, factored in the lane at every step
        const bool ok = step_noise_factor<M, R>(c.sig_eta, prm, xu, sn, cs, Le);
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) x[i] += Le[tri(i, j)] * nz.x(t, j);
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = ok ? x[i] : R(__builtin_nan(""));  // (not positive definite: this rollout's state is NaN from here on)
      } else {
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) x[i] += Le[tri(i, j)] * nz.x(t, j);
      }
    }
  }
  if constexpr (EVAL) {  // the terminal cost of a problem with Qf, then the one store
    if (NZT > 0 && c.has_Qf) {
      R sn[NA1], cs[NA1], zT[C::NZT1];
#pragma unroll
      for (int q2 = 0; q2 < M::NA; ++q2) r_sincos(x[M::ang(q2)], &sn[q2], &cs[q2]);
      M::observe_terminal(prm, x, sn, cs, zT);
#pragma unroll
      for (int i = 0; i < NZT; ++i) zT[i] -= c.zg_term[i];
      cost += quad_form<C::NZT1>(c.Qf, zT);
    }
    ev->cost[(long)r * B + b] = cost;
  } else {
    if (a.x_final) {
#pragma unroll
      for (int i = 0; i < NX; ++i) a.x_final[(long)i * N + n] = x[i];
    }
    if (NZT > 0 && a.z_term) {
      R sn[NA1], cs[NA1], zT[C::NZT1];
#pragma unroll
      for (int q2 = 0; q2 < M::NA; ++q2) r_sincos(x[M::ang(q2)], &sn[q2], &cs[q2]);
      M::observe_terminal(prm, x, sn, cs, zT);
#pragma unroll
      for (int i = 0; i < NZT; ++i) a.z_term[(long)i * N + n] = zT[i];
    }
  }
}

// The reduction of i2c_rollout_eval: lane (t, b) adds the parts' sums of cell t in ascending part order and writes mean and covariance
//   mean = mu + S1 / R,  cov = (S2 - S1 S1^T / R) / (R - 1)     (R = 1: NaN, as an unbiased estimate of one sample is);
// the t = 0 lanes also do the cost statistics of their trajectory, two passes over cost[r * B + b] with r ascending. A trajectory
// with a non-finite cost gets NaN statistics and the count of such rollouts in n_bad.
template <typename R> struct EvalReduceArgs {
  const R* post;
  const R* work;    // null: no moments
  const R* cost;    // [n_rollouts][B]
  R* cost_stats;    // [4][B] or null
  int32_t* n_bad;   // [B] or null
  R* xu_mean;       // [T][D][B] or null
  R* xu_cov;        // [T][sym D][B] or null
  int n_rollouts, parts;
};
template <class M, typename R>
I2C_HD inline void rollout_eval_reduce_body(const Consts<M, R>& c, const EvalReduceArgs<R>& a, const int t, const int b, const int Tb) {
  using C = Consts<M, R>;
  constexpr int D = C::D, E = D + sym(D);
  const long B = c.B;
  const int Rn = a.n_rollouts;
  // (both loops below: U loads in flight, then the additions in ascending order -- one lane walks a long column, so what a step costs
  // is the latency of its loads)
  constexpr int U = 16;
  if (t == 0 && (a.cost_stats || a.n_bad)) {
    R s = R(0), lo = a.cost[b], hi = a.cost[b];
    int bad = 0;
    for (int r0 = 0; r0 < Rn; r0 += U) {
      R v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = a.cost[(long)(r0 + k < Rn ? r0 + k : Rn - 1) * B + b];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (r0 + k < Rn) {
          s += v[k];
          lo = v[k] < lo ? v[k] : lo;
          hi = v[k] > hi ? v[k] : hi;
          bad += (v[k] - v[k] == R(0)) ? 0 : 1;
        }
      }
    }
    const R mean = s / R(Rn);
    R ss = R(0);
    for (int r0 = 0; r0 < Rn; r0 += U) {
      R v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = a.cost[(long)(r0 + k < Rn ? r0 + k : Rn - 1) * B + b];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const R dv = v[k] - mean;
        if (r0 + k < Rn) ss += dv * dv;
      }
    }
    const R nan = R(__builtin_nan(""));
    if (a.cost_stats) {
      a.cost_stats[b] = bad ? nan : mean;
      a.cost_stats[B + b] = bad ? nan : ss / R(Rn - 1);
      a.cost_stats[2 * B + b] = bad ? nan : lo;
      a.cost_stats[3 * B + b] = bad ? nan : hi;
    }
    if (a.n_bad) a.n_bad[b] = bad;
  }
  if (!a.work || !a.xu_mean || t >= Tb) return;
  R S[E];
#pragma unroll
  for (int e = 0; e < E; ++e) S[e] = a.work[((long)t * E + e) * B + b];
  constexpr int UP = E <= 9 ? 8 : (E <= 20 ? 4 : (E <= 35 ? 2 : 1));  // parts in flight: UP * E loads
  for (int q0 = 1; q0 < a.parts; q0 += UP) {
    R v[UP][E];
#pragma unroll
    for (int k = 0; k < UP; ++k) {
      const R* w = a.work + (((long)(q0 + k < a.parts ? q0 + k : a.parts - 1) * c.T + t) * E) * B + b;
#pragma unroll
      for (int e = 0; e < E; ++e) v[k][e] = w[(long)e * B];
    }
#pragma unroll
    for (int k = 0; k < UP; ++k) {
      if (q0 + k < a.parts) {
#pragma unroll
        for (int e = 0; e < E; ++e) S[e] += v[k][e];
      }
    }
  }
  const R* row = a.post + ((long)c.row(t) * C::E_POST) * B + c.post_bo(b);
  const long es = c.post_es();
  const R rn = R(Rn), rn1 = R(Rn - 1);
#pragma unroll
  for (int i = 0; i < D; ++i) a.xu_mean[((long)t * D + i) * B + b] = row[(long)i * es] + S[i] / rn;
  if (a.xu_cov) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) a.xu_cov[((long)t * sym(D) + tri(i, j)) * B + b] = (S[D + tri(i, j)] - S[i] * S[j] / rn) / rn1;
  }
}

// ------------------------------------------------------------------------------------------
// One step of the PLANT under the action a control step just planned: the part of the closed MPC loop between two calls of
// the policy (scripts/mpc_state_est/mpc_quad.py:643-660; env step :414-420, measurement :408-412), one lane per trajectory:
//   history rows; cost[b] += (z - z_ref)^T QR (z - z_ref), z = observe(x, u);  x' = dynamics(x, u) + Le eps_x;
//   y = measure(x') + Lz eps_y  (partially observed)   or   belief mean <- x'  (fully observed, mpc.py:95-111).
// Le = chol(sig_eta) and Lz = chol(sig_zeta) are constant: factored once per call on the host (PlantNoise, kernel arguments).
// The functors clip the action themselves, so the raw planned action is what is recorded and handed to the next filter step.
// The plant's parameters are those of the problem the launcher was given (shared, or column b of model_params_b: PerTraj<M>).
// ------------------------------------------------------------------------------------------
template <class M, typename R> struct PlantNoise {
  R Le[sym(M::NX)], Lz[sym(M::NY)];
};
template <typename R> struct PlantArgs {
  R* x;            // [NX][B]  true state, in/out
  const R* u;      // [NU][B]  the planned action (first NU rows of I2cMpcStep.action)
  const R* eps_x;  // [NX][B] or null: process noise, standard normal
  const R* eps_y;  // [NY][B] or null: measurement noise, standard normal
  R* y_out;        // [NY][B] or null: the measurement the next filter step reads
  R* u_out;        // [NU][B] or null: the applied action the next filter step reads
  R* x_obs;        // [NX][B] or null: fully observed mode, the belief mean (I2cProblem.x0) takes x'
  const R* mu;     // [NX][B] or null: the belief mean the plan started from, copied to mu_hist
  const R* z_ref;  // [NZ][B] or null (the batch target c.zg): reference of this step's cost
  R* cost;         // [B] or null: accumulated
  R* x_hist;       // [NX][B] or null: x before the step
  R* u_hist;       // [NU][B] or null
  R* y_hist;       // [NY][B] or null: y after the step
  R* mu_hist;      // [NX][B] or null
};

template <class M, typename R>
I2C_HD inline void plant_step_body(const Consts<M, R>& c, const PlantNoise<M, R>& nz, const PlantArgs<R>& a, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NU = C::NU, NZ = C::NZ, NY = M::NY, D = C::D, NA1 = M::NA > 0 ? M::NA : 1;
  const long B = c.B;
  R pb[C::NP1];
  const R* prm = c.params;
  if constexpr (is_per_traj<M>::value) prm = param_ptr<M::NP>(params_of(c, b), pb);
  R xu[D], sn[NA1], cs[NA1], zt[NZ], xn[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) xu[i] = a.x[(long)i * B + b];
#pragma unroll
  for (int i = 0; i < NU; ++i) xu[NX + i] = a.u[(long)i * B + b];
  if (a.x_hist) {
#pragma unroll
    for (int i = 0; i < NX; ++i) a.x_hist[(long)i * B + b] = xu[i];
  }
  if (a.u_hist) {
#pragma unroll
    for (int i = 0; i < NU; ++i) a.u_hist[(long)i * B + b] = xu[NX + i];
  }
  if (a.mu_hist) {
#pragma unroll
    for (int i = 0; i < NX; ++i) a.mu_hist[(long)i * B + b] = a.mu[(long)i * B + b];
  }
#pragma unroll
  for (int q = 0; q < M::NA; ++q) r_sincos(xu[M::ang(q)], &sn[q], &cs[q]);
  M::observe(prm, xu, sn, cs, zt);
  M::dynamics(prm, xu, sn, cs, xn);
  if (a.cost) {  // stage cost of (x, u) against this step's reference (mpc_quad.py:659-660)
#pragma unroll
    for (int k = 0; k < NZ; ++k) zt[k] -= a.z_ref ? a.z_ref[(long)k * B + b] : c.zg[k];
    R q = R(0);
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      R r = R(0);
#pragma unroll
      for (int j = 0; j < i; ++j) r += c.QR[tri(i, j)] * zt[j];
      q += zt[i] * (c.QR[tri(i, i)] * zt[i] + R(2) * r);
    }
    a.cost[b] += q;
  }
  if (a.eps_x) {
    R e[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) e[j] = a.eps_x[(long)j * B + b];
    if constexpr (has_process_noise<M, R>::value) {  // chol(sig_eta + Q(x, u)) of this step, factored in the lane
      R Le[sym(NX)];
      const bool ok = step_noise_factor<M, R>(c.sig_eta, prm, xu, sn, cs, Le);
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) xn[i] += Le[tri(i, j)] * e[j];
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = ok ? xn[i] : R(__builtin_nan(""));
    } else {
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) xn[i] += nz.Le[tri(i, j)] * e[j];
    }
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) a.x[(long)i * B + b] = xn[i];
  if (a.u_out) {
#pragma unroll
    for (int i = 0; i < NU; ++i) a.u_out[(long)i * B + b] = xu[NX + i];
  }
  if (a.x_obs) {
#pragma unroll
    for (int i = 0; i < NX; ++i) a.x_obs[(long)i * B + b] = xn[i];
  }
  if (a.y_out || a.y_hist) {
    R y[NY];
#pragma unroll
    for (int q = 0; q < M::NA; ++q) r_sincos(xn[M::ang(q)], &sn[q], &cs[q]);
    M::measure(prm, xn, sn, cs, y);
    if (a.eps_y) {
      R e[NY];
#pragma unroll
      for (int j = 0; j < NY; ++j) e[j] = a.eps_y[(long)j * B + b];
#pragma unroll
      for (int i = 0; i < NY; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) y[i] += nz.Lz[tri(i, j)] * e[j];
    }
    if (a.y_out) {
#pragma unroll
      for (int i = 0; i < NY; ++i) a.y_out[(long)i * B + b] = y[i];
    }
    if (a.y_hist) {
#pragma unroll
      for (int i = 0; i < NY; ++i) a.y_hist[(long)i * B + b] = y[i];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Receding-horizon shift of the MPC loop (PartiallyObservedMpcPolicy.__call__, i2c/policy/mpc.py:171-181):
//   u = cells[0].mu_u0_m;  cells.pop(0);  cells.append(deepcopy(cell_init)) with the next target.
// The persistent per-cell buffers are a RING (Consts::t0): popping cell 0 and appending a cell is "advance t0 by one"
// (done by the caller after this kernel) plus ONE fresh row, written here over the row cell 0 occupied -- one lane per
// trajectory, after the first action and its covariance were copied out of that row. The fresh cell keeps the temperature
// `alpha_init` it was copied with (see I2cProblem.alpha_cell) and is in feed-forward mode.
// ------------------------------------------------------------------------------------------
template <typename R> struct ShiftArgs {
  R* post;               // [T][E_POST][B]   ring
  const R* cell_init;    // [E_POST][B]
  R* alpha_cell;         // [T][B] ring, or null
  const R* alpha_init;   // [B] or null
  R* z;                  // [T][NZ][B] ring, or null
  const R* z_new;        // [NZ][B] or null: target of the appended cell (null: the previous last cell's)
  uint8_t* ff;           // [T] ring
  R* action;             // [NU + sym(NU)][B]: cells[0].mu_u0_m, sig_u0_m (packed) BEFORE the shift
};

template <class M, typename R>
I2C_HD inline void mpc_shift_body(const Consts<M, R>& c, const ShiftArgs<R>& a, const int b) {
  using C = Consts<M, R>;
  constexpr int NX = C::NX, NU = C::NU, NZ = C::NZ, D = C::D;
  const long B = c.B;
  const int r0 = c.row(0), rl = c.row(c.T - 1);  // rows of the first and of the last cell of the current horizon
  const long es = c.post_es();
  const R* p0 = a.post + ((long)r0 * C::E_POST) * B + c.post_bo(b);
  if (a.action) {
#pragma unroll
    for (int i = 0; i < NU; ++i) a.action[(long)i * B + b] = p0[(long)(NX + i) * es];
#pragma unroll
    for (int p = 0; p < NU; ++p)
#pragma unroll
      for (int q = 0; q <= p; ++q) a.action[(long)(NU + tri(p, q)) * B + b] = p0[(long)(D + tri(NX + p, NX + q)) * es];
  }
  // (the fresh cell itself -- cell_init, one cell block in the layout of `post` -- is a plain block copy: Impl::shift)
  if (a.alpha_cell) a.alpha_cell[(long)r0 * B + b] = a.alpha_init[b];
  if (a.z) {
#pragma unroll
    for (int k = 0; k < NZ; ++k)
      a.z[((long)r0 * NZ + k) * B + b] = a.z_new ? a.z_new[(long)k * B + b] : a.z[((long)rl * NZ + k) * B + b];
  }
  if (b == 0) a.ff[r0] = (uint8_t)1;
}

}  // namespace i2c
