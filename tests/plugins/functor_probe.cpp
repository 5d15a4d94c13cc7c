// Stand-alone host program for tests/test_functor_codegen.py: one model functor -- in-tree, a header plugin or a generated header --
// printed as its compile-time structure and evaluated pointwise. Compiled with g++ -DI2C_HOST_SIM -I <csrc> and
//   -DPROBE_MODEL=<struct>          [-DPROBE_HEADER="<header that defines it>"]
//   [-DPROBE_DUAL_MODEL=<struct>     -DPROBE_DUAL_HEADER="..."]   the same model WITHOUT a jacobian member (default: PROBE_MODEL):
//                                                                  value_and_jacobian on it is the dual-number path
// argv[1]: a text file "n_params p...\n n_points\n x_0 ... x_{d-1}\n ..." (hex floats). Output: "HINT <name> v..." lines, then per
// point DYN / OBS / TERM (values), JDx (dual-number Jacobian of function x) and, where the functor has the member, JAx (jacobian<x>).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "i2c_linearize.hpp"
#ifdef PROBE_HEADER
#include PROBE_HEADER
#endif
#ifdef PROBE_DUAL_HEADER
#include PROBE_DUAL_HEADER
#endif
#ifndef PROBE_DUAL_MODEL
#define PROBE_DUAL_MODEL PROBE_MODEL
#endif

using namespace i2c;
using M = PROBE_MODEL;
using MD = PROBE_DUAL_MODEL;
constexpr int NX = M::NX, NU = M::NU, NZ = M::NZ, NZT = M::NZT, D = NX + NU, NA1 = M::NA > 0 ? M::NA : 1, NP1 = M::NP > 0 ? M::NP : 1;
static_assert(MD::NX == NX && MD::NU == NU && MD::NZ == NZ && MD::NZT == NZT && MD::NA == M::NA, "the two structs are one model");

static void row(const char* tag, const double* v, const int n) {
  std::printf("%s", tag);
  for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
  std::printf("\n");
}
template <class F> static void hint(const char* name, const int n, const F& f) {
  std::printf("HINT %s", name);
  for (int k = 0; k < n; ++k) std::printf(" %d", f(k));
  std::printf("\n");
}
template <class MM, int FN, int DIN, int DOUT> static void jac(const char* tag, const double* p, const double* x) {
  if constexpr (DOUT > 0) {
    double y[DOUT], J[DOUT * DIN];
    value_and_jacobian<MM, FN, DIN, DOUT, double>(p, x, y, J);
    row(tag, J, DOUT * DIN);
    float pf[NP1], xf[DIN], yf[DOUT], Jf[DOUT * DIN];  // (the functions instantiate on float and Dual<float> too)
    for (int i = 0; i < M::NP; ++i) pf[i] = (float)p[i];
    for (int i = 0; i < DIN; ++i) xf[i] = (float)x[i];
    value_and_jacobian<MM, FN, DIN, DOUT, float>(pf, xf, yf, Jf);
  }
}

int main(int argc, char** argv) {
  std::printf("HINT sizes %d %d %d %d %d %d %d\n", NX, NU, NZ, NZT, (int)M::NP, (int)M::NA, (int)M::NY);
  std::printf("HINT knobs %d %d %d %d %d\n", (int)M::GROUP, M::QUAD ? 1 : 0, (int)M::QUAD_FORWARD_MAX_B, (int)M::QUAD_FORWARD_MIN_B,
              has_jacobian<M, FN_DYNAMICS, double>::value ? 1 : 0);
  hint("ang", M::NA, [](int a) { return M::ang(a); });
  hint("obs_lin", NZ, [](int k) { return M::obs_lin(k); });
  hint("obs_dep", NZ, [](int k) { return M::obs_dep(k); });
  hint("term_lin", NZT, [](int k) { return M::term_lin(k); });
  hint("term_dep", NZT, [](int k) { return M::term_dep(k); });
  hint("meas_lin", M::NY, [](int k) { return M::meas_lin(k); });
  hint("meas_dep", M::NY, [](int k) { return M::meas_dep(k); });
  if (argc < 2) return 0;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tok[64];
  auto next = [&]() {
    if (std::fscanf(f, "%63s", tok) != 1) std::exit(3);
    return std::strtod(tok, nullptr);
  };
  const int np = (int)next();
  if (np != M::NP) return 4;
  double p[NP1] = {0};
  for (int i = 0; i < np; ++i) p[i] = next();
  const int n = (int)next();
  for (int q = 0; q < n; ++q) {
    double x[D], sn[NA1], cs[NA1], xn[NX], z[NZ], zt[NZT > 0 ? NZT : 1];
    for (int i = 0; i < D; ++i) x[i] = next();
    for (int a = 0; a < M::NA; ++a) r_sincos(x[M::ang(a)], &sn[a], &cs[a]);
    M::dynamics((const double*)p, (const double*)x, (const double*)sn, (const double*)cs, xn);
    row("DYN", xn, NX);
    M::observe((const double*)p, (const double*)x, (const double*)sn, (const double*)cs, z);
    row("OBS", z, NZ);
    if constexpr (NZT > 0) {
      M::observe_terminal((const double*)p, (const double*)x, (const double*)sn, (const double*)cs, zt);
      row("TERM", zt, NZT);
    }
    jac<MD, FN_DYNAMICS, D, NX>("JD0", p, x);
    jac<MD, FN_OBSERVE, D, NZ>("JD1", p, x);
    jac<MD, FN_OBSERVE_TERMINAL, NX, NZT>("JD2", p, x);
    if constexpr (has_jacobian<M, FN_DYNAMICS, double>::value) {
      jac<M, FN_DYNAMICS, D, NX>("JA0", p, x);
      jac<M, FN_OBSERVE, D, NZ>("JA1", p, x);
      jac<M, FN_OBSERVE_TERMINAL, NX, NZT>("JA2", p, x);
    }
  }
  std::fclose(f);
  return 0;
}
