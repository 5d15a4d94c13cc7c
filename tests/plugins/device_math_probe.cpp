// Stand-alone host program for tests/test_device_math_ops.py: the scalar routines a model functor may call beyond + - * / and
// their dual-number overloads, evaluated on the arguments of a text file. Compiled with g++ -DI2C_HOST_SIM -I <csrc>.
// argv[1]: one request per line, hex floats; the answer is one line of hex floats with the same tag:
//   S x             -> r_sqrt(x), d r_sqrt at tangent 1, d r_sqrt at tangent 0, d r_rsqrt at tangent 0
//   T x             -> r_tanh(x), std::tanh(x), d r_tanh at tangent 1
//   A v d           -> r_abs(Dual(v, d)): value, tangent, r_sign(v)
//   M av ad bv bd   -> r_max, r_min of the two duals: value, tangent each
//   W a b xv xd yv yd -> r_where_gt (a, b carry tangents 7 and 11): value, tangent; and the plain-double select
//   L v d           -> r_log(Dual): value, tangent
//   C v d           -> r_sincos(Dual): sine value, tangent, cosine value, tangent
//   G g d           -> r_tangent(g, d)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "i2c_linearize.hpp"

using namespace i2c;
using D = Dual<double>;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tag[8], tok[64];
  auto next = [&]() {
    if (std::fscanf(f, "%63s", tok) != 1) std::exit(3);
    return std::strcmp(tok, "nan") == 0 ? std::nan("") : std::strtod(tok, nullptr);
  };
  while (std::fscanf(f, "%7s", tag) == 1) {
    double v[6], out[6];
    int n_in = 0, n_out = 0;
    switch (tag[0]) {
      case 'S': n_in = 1; break;
      case 'T': n_in = 1; break;
      case 'A': case 'L': case 'C': case 'G': n_in = 2; break;
      case 'M': n_in = 4; break;
      case 'W': n_in = 6; break;
      default: return 4;
    }
    for (int i = 0; i < n_in; ++i) v[i] = next();
    if (tag[0] == 'S') {
      out[0] = r_sqrt(v[0]), out[1] = r_sqrt(D(v[0], 1.0)).d, out[2] = r_sqrt(D(v[0], 0.0)).d, out[3] = r_rsqrt(D(v[0], 0.0)).d;
      n_out = 4;
      if (r_sqrt(D(v[0], 1.0)).v != out[0] && out[0] == out[0]) return 5;
    } else if (tag[0] == 'T') {
      out[0] = r_tanh(v[0]), out[1] = std::tanh(v[0]), out[2] = r_tanh(D(v[0], 1.0)).d;
      n_out = 3;
    } else if (tag[0] == 'A') {
      const D a = r_abs(D(v[0], v[1]));
      out[0] = a.v, out[1] = a.d, out[2] = r_sign(v[0]);
      n_out = 3;
    } else if (tag[0] == 'M') {
      const D a(v[0], v[1]), b(v[2], v[3]), hi = r_max(a, b), lo = r_min(a, b);
      out[0] = hi.v, out[1] = hi.d, out[2] = lo.v, out[3] = lo.d, out[4] = r_max(v[0], v[2]), out[5] = r_min(v[0], v[2]);
      n_out = 6;
    } else if (tag[0] == 'W') {
      const D w = r_where_gt(D(v[0], 7.0), D(v[1], 11.0), D(v[2], v[3]), D(v[4], v[5]));
      out[0] = w.v, out[1] = w.d, out[2] = r_where_gt(v[0], v[1], v[2], v[4]);
      n_out = 3;
    } else if (tag[0] == 'L') {
      const D l = r_log(D(v[0], v[1]));
      out[0] = l.v, out[1] = l.d;
      n_out = 2;
    } else if (tag[0] == 'C') {
      D s, c;
      r_sincos(D(v[0], v[1]), &s, &c);
      out[0] = s.v, out[1] = s.d, out[2] = c.v, out[3] = c.d;
      n_out = 4;
    } else {
      out[0] = r_tangent(v[0], v[1]);
      n_out = 1;
    }
    std::printf("%s", tag);
    for (int i = 0; i < n_out; ++i) std::printf(" %a", out[i]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
