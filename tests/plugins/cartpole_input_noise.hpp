// An OUT-OF-TREE model with STATE-ACTION-DEPENDENT process noise, d = 5 (tests/test_process_noise*.py): the in-tree Cartpole functor
// plus the optional `process_noise` member. The covariance of one step from xu = (x, th, xd, thd, u) is  sig_eta + Q(xu)  with
//   Q(xu) = sign * (s2 u^2 b b^T + c thd^2 e3 e3^T),   b = (0, 0, 1, 0.5),  s2 = 1e-3,  c = 1e-4
// (two non-zero entries of b: the packed off-diagonal entry (3, 2) is exercised). params = {sign}.
// The NumPy twin is CartpoleInputNoiseNumpy (tests/noise_models.py).
#pragma once

namespace i2c {

struct CartpoleInputNoise : Cartpole {
  static constexpr int ID = -1, NP = 1;
  template <typename R> I2C_FN void process_noise(const R* p, const R* xu, const R*, const R*, R* q) {  // q[sym(4)], packed lower
    const R s2 = R(1e-3), c = R(1e-4), b3 = R(0.5);
    const R a = p[0] * s2 * xu[4] * xu[4];
#pragma unroll
    for (int i = 0; i < 10; ++i) q[i] = R(0);
    q[5] = a;                                    // (2, 2)
    q[8] = a * b3;                               // (3, 2)
    q[9] = a * (b3 * b3) + p[0] * c * xu[3] * xu[3];  // (3, 3)
  }
};

}  // namespace i2c
