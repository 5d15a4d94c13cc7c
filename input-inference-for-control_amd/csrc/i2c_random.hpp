// The counter-based generator of i2c_rollout_eval: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
// 1, 2, 3", SC'11) and the Box-Muller pair on top of it. Plain C++: the device and the host simulation compile this text.
//
// One call serves one PAIR of standard normals of one rollout step. The layout is part of the interface (include/i2c_hip.h):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (first_trajectory + b,  r,  t,  kind + 4 * j)      kind: 0 x0 (t = 0xffffffff), 1 process, 2 action
//   pair j -> normals 2j and 2j + 1 of that kind's vector; an odd last normal is dropped
//   a = (w0 << 21) | (w1 >> 11);  u1 = (a + 1) * 2^-53  in (0, 1]
//   b = (w2 << 21) | (w3 >> 11);  u2 = b * 2^-53        in [0, 1)
//   rho = sqrt(-2 log(u1));  z[2j] = rho cos(2 pi u2),  z[2j + 1] = rho sin(2 pi u2)
// so a draw depends on (seed, global trajectory, r, t, kind, j) and on nothing else: not on B, the part split or the launch shape.
#pragma once
#include <stdint.h>
#include "i2c_linalg.hpp"

namespace i2c {

constexpr int RNG_X0 = 0, RNG_PROCESS = 1, RNG_ACTION = 2;  // `kind`
constexpr uint32_t RNG_T_X0 = 0xffffffffu;                  // the time word of the x0 draw

struct Philox {
  uint32_t w[4];
};

I2C_FN Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

// normals 2j and 2j + 1 of one (trajectory, rollout, step, kind)
I2C_FN void normal_pair(const uint64_t seed, const uint32_t traj, const uint32_t r, const uint32_t t, const int kind, const int j,
                        double* z0, double* z1) {
  const Philox o = philox4x32_10(traj, r, t, (uint32_t)(kind + 4 * j), (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  const uint64_t a = ((uint64_t)o.w[0] << 21) | (o.w[1] >> 11), b = ((uint64_t)o.w[2] << 21) | (o.w[3] >> 11);
  const double u1 = (double)(a + 1) * 0x1p-53, u2 = (double)b * 0x1p-53;
  const double rho = r_sqrt(-2.0 * r_log(u1));
  double s, c;
  r_sincos(6.283185307179586476925286766559 * u2, &s, &c);
  *z0 = rho * c;
  *z1 = rho * s;
}

// the first n normals of one (trajectory, rollout, step, kind)
template <int n> I2C_FN void normals(const uint64_t seed, const uint32_t traj, const uint32_t r, const uint32_t t, const int kind, double* z) {
#pragma unroll
  for (int j = 0; j < (n + 1) / 2; ++j) {
    double z0, z1;
    normal_pair(seed, traj, r, t, kind, j, &z0, &z1);
    z[2 * j] = z0;
    if (2 * j + 1 < n) z[2 * j + 1] = z1;
  }
}

}  // namespace i2c
