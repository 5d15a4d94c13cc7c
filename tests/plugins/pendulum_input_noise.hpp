// An OUT-OF-TREE model with STATE-ACTION-DEPENDENT process noise (tests/test_process_noise*.py): the in-tree Pendulum functor plus
// the optional `process_noise` member (csrc/i2c_cell.hpp). The covariance of one step from the point
// xu = (th, om, u) is  sig_eta + Q(xu)  with
//   Q(xu) = sign * (s2 u^2 b b^T + c om^2 e2 e2^T),   b = (0.05, 1),  s2 = 1e-2,  c = 1e-3:
// actuator noise that grows with the torque asked for (the raw action, as the dynamics functor is handed it) and a velocity-dependent
// term. params = {sign}: +1 in every test but the failure-isolation one, where -1 on one trajectory makes its Q indefinite.
// The NumPy twin is PendulumInputNoiseNumpy (tests/noise_models.py).
#pragma once

namespace i2c {

struct PendulumInputNoise : Pendulum {
  static constexpr int ID = -1, NP = 1;
  template <typename R> I2C_FN void process_noise(const R* p, const R* xu, const R*, const R*, R* q) {  // q[sym(2)], packed lower
    const R s2 = R(1e-2), c = R(1e-3), b0 = R(0.05);
    const R a = p[0] * s2 * xu[2] * xu[2];
    q[0] = a * (b0 * b0);
    q[1] = a * b0;
    q[2] = a + p[0] * c * xu[1] * xu[1];
  }
};

}  // namespace i2c
