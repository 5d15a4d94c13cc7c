// The pendulum with input noise of tests/plugins/pendulum_input_noise.hpp once more, for tests/test_process_noise_traced.py, written
// by hand in the ORDER OF OPERATIONS functor_codegen.py emits for the same math (the constants of the step and of Q folded, one clip):
//   Q = sign (s2 u^2 b b^T + c om^2 e2 e2^T), b = (0.05, 1), s2 = 1e-2, c = 1e-3;  params = {sign}.
// Against the traced model of tests/plugins/py_models_noise.py every member is then the same sequence of fp64 operations, and a
// sweep pair of the two agrees to 1e-12 in every quantity, the controller gain included. With the step or the member in
// pendulum_input_noise.hpp's order instead, the posteriors still agree to 1e-14, but the gain K = sig_ux sig_xx^-1 only to 6e-12 ..
// 2e-11: cond(sig_xx) = 2.5e3 on that problem amplifies the last-bit differences of two roundings of the same Q.
#pragma once

namespace i2c {

struct PendulumInputNoiseExpanded : ModelDefaults {
  static constexpr int NX = 2, NU = 1, NZ = 4, NZT = 3, NP = 1, NA = 1, NY = 3;
  static constexpr int GROUP = 4;
  static constexpr bool QUAD = true;
  I2C_HD static constexpr int ang(int) { return 0; }
  I2C_HD static constexpr int obs_lin(int k) { return k < 2 ? -1 : k - 1; }
  I2C_HD static constexpr int obs_dep(int k) { return k < 2 ? 0 : k - 1; }
  I2C_HD static constexpr int term_lin(int k) { return k < 2 ? -1 : 1; }
  I2C_HD static constexpr int term_dep(int k) { return k < 2 ? 0 : 1; }
  I2C_HD static constexpr int meas_lin(int k) { return k < 2 ? -1 : 1; }
  I2C_HD static constexpr int meas_dep(int k) { return k < 2 ? 0 : 1; }
  template <typename R> I2C_FN void dynamics(const R*, const R* x, const R* sn, const R*, R* y) {
    const R t0 = r_clip(x[2], R(-2.0), R(2.0));
    y[0] = x[0] + R(0.03677493750000001) * sn[0] + R(0.049975000000000006) * x[1] + R(0.0075000000000000015) * t0;
    y[1] = R(0.15000000000000002) * t0 + R(0.7354987500000001) * sn[0] + R(0.9995) * x[1];
  }
  template <typename R> I2C_FN void observe(const R*, const R* x, const R* sn, const R* cs, R* y) {
    y[0] = sn[0];
    y[1] = cs[0];
    y[2] = x[1];
    y[3] = x[2];
  }
  template <typename R> I2C_FN void observe_terminal(const R*, const R* x, const R* sn, const R* cs, R* y) {
    y[0] = sn[0];
    y[1] = cs[0];
    y[2] = x[1];
  }
  template <typename R> I2C_FN void measure(const R* p, const R* x, const R* sn, const R* cs, R* y) { observe_terminal(p, x, sn, cs, y); }
  template <typename R> I2C_FN void process_noise(const R* p, const R* x, const R*, const R*, R* q) {  // s2 b0^2, s2 b0, s2, c folded
    const R t0 = p[0] * x[2] * x[2];
    q[0] = R(2.5000000000000005e-05) * t0;
    q[1] = R(0.0005) * t0;
    q[2] = R(0.01) * t0 + R(0.001) * p[0] * x[1] * x[1];
  }
};

}  // namespace i2c
