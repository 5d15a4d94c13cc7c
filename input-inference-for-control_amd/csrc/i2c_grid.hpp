// Grid family: the Gauss-Hermite tensor-grid rule with ONE WAVEFRONT per trajectory.
//
// The one-lane kernels walk the gh_degree^d points of every transform serially (grid_transform, i2c_cell.hpp): 243 points for the
// cartpole at degree 3, 2 187 for the double cartpole, several transforms per cell, T cells in a chain -- on one lane of one
// wavefront at B = 1. The points of a transform are independent and everything else in the cell (Cholesky factors, the update,
// the RTS step) is small, so here
//   * the 64 lanes of a wavefront all run the SAME one-lane cell body on the SAME trajectory (forward_sweep_body,
//     backward_fused_body, propagate_body with GRID = GRID_WAVE): trajectory index = wavefront index;
//   * inside a transform lane l evaluates the points l, l + 64, l + 128, ... and the partial moments are summed across the
//     wavefront (grid_allreduce): 64 x the parallelism of the point loop for one reduction per transform;
//   * the rest of the cell runs redundantly, and bit-identically, in every lane; loads are same-address broadcasts and only
//     lane 0 stores (grid_writer, i2c_cell.hpp).
// Buffers are the common [T][E][B] ones as the one-lane kernels read and write them, so sweeps of the two families can be mixed.
// fp64 only. The host simulation (tests only) runs the 64 lanes of a trajectory as 64 contexts of one thread that hand over to each
// other where the device exchanges values (a wavefront of threads, as the group and wave simulations have, spends its time in the
// scheduler: every lane runs the WHOLE cell here, and there are two hand-overs per transform).
#pragma once
#include "i2c_cell.hpp"
#ifdef I2C_HOST_SIM
#include <ucontext.h>
#include <functional>
#include <memory>
#endif

namespace i2c {

// values one transform reduces: s1, the packed second moment and, with CROSS, the cross moment
template <int DIN, int DOUT, bool CROSS> constexpr int grid_nred() { return DOUT + sym(DOUT) + (CROSS ? DIN * DOUT : 0); }
// ... and the most any transform of a model's cells reduces (the exchange region of the host simulation, per lane)
template <class M> struct GridXch {
  static constexpr int D = M::NX + M::NU, NT = M::NZT > 0 ? M::NZT : 1;
  static constexpr int N0 = grid_nred<D, M::NZ, true>(), N1 = grid_nred<D, M::NX, true>(), N2 = grid_nred<M::NX, NT, true>();
  static constexpr int N = N0 > N1 ? (N0 > N2 ? N0 : N2) : (N1 > N2 ? N1 : N2);
};

#ifdef I2C_HOST_SIM
// One simulated wavefront: the lanes are ucontext fibres resumed round-robin by grid_sim_team(); a lane that reaches a barrier hands
// back, and is resumed only after every other lane has reached the same barrier (all lanes pass the same sequence of barriers: their
// control flow is uniform). The lane bodies keep everything in one inlined frame: 512 KiB of stack each.
struct GridFibres {
  static constexpr size_t STACK = 512 * 1024;
  ucontext_t main, lane[64];
  bool done[64];
  std::function<void()> body;
};
inline thread_local GridFibres* grid_fibres = nullptr;
inline void grid_sim_sync() {
  GridFibres* f = grid_fibres;
  swapcontext(&f->lane[grid_lane_sim.l], &f->main);
}
inline void grid_fibre_entry() {
  grid_fibres->body();
  grid_fibres->done[grid_lane_sim.l] = true;  // (returns to uc_link: the team's loop)
}
// runs body() once in each of the 64 lanes of a team; `stacks`: 64 x GridFibres::STACK bytes, `xch`: the team's exchange region
template <class Body> static void grid_sim_team(char* stacks, double* xch, const Body& body) {
  GridFibres f;
  f.body = body;
  grid_fibres = &f;
  for (int l = 0; l < 64; ++l) {
    getcontext(&f.lane[l]);
    f.lane[l].uc_stack.ss_sp = stacks + (size_t)l * GridFibres::STACK;
    f.lane[l].uc_stack.ss_size = GridFibres::STACK;
    f.lane[l].uc_link = &f.main;
    makecontext(&f.lane[l], grid_fibre_entry, 0);
    f.done[l] = false;
  }
  for (bool any = true; any;) {
    any = false;
    for (int l = 0; l < 64; ++l)
      if (!f.done[l]) {
        grid_lane_sim = GridLaneSim{l, xch};
        swapcontext(&f.main, &f.lane[l]);
        any = true;
      }
  }
  grid_fibres = nullptr;
}
#else
// the value of the lane a DPP control pairs this one with (all 64 lanes active)
template <int CTRL> I2C_FN double grid_dpp(const double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
#endif

#ifdef I2C_HOST_SIM
// what lane k holds after `s` steps of the butterfly below: its own value after s - 1 steps plus its partner's
inline double grid_sim_butterfly(const double* x, const int s, const int k) {
  if (s == 0) return x[k];
  const int partner[6] = {k ^ 1, k ^ 2, (k & ~7) | (7 - (k & 7)), (k & ~15) | (15 - (k & 15)), k ^ 32, k ^ 16};
  return grid_sim_butterfly(x, s - 1, k) + grid_sim_butterfly(x, s - 1, partner[s - 1]);
}
#endif
// Sum of v[i] over the 64 lanes of the wavefront, result in every lane: a butterfly of six steps. Each step pairs every lane with
// ONE partner and both add the same two numbers -- x + y in one lane, y + x in the other: floating-point addition commutes, so
// after a step the two hold the same bits, and after six EVERY LANE ENDS WITH THE SAME BITS. The Cholesky failure flags, `status`
// and all control flow after a transform rely on exactly that (a body that branched differently in two lanes would leave the
// cross-lane instructions of the next transform with inactive partners).
//   steps 1, 2: lanes l ^ 1, l ^ 2 (DPP quad_perm);  3: the mirror inside a half row, 7 - l (quads hold one value by then);
//   4: the mirror inside a row, 15 - l;  5, 6: the other half of the wavefront, the neighbouring row (v_permlane32_swap, v_permlane16_swap).
template <int N, typename R> I2C_FN void grid_allreduce(R* v) {
  static_assert(sizeof(R) == 8, "grid family: fp64 only");
#ifdef I2C_HOST_SIM
  const GridLaneSim& g = grid_lane_sim;
  const int l = g.l;
  // every lane publishes its values, then evaluates ITS OWN end of the butterfly -- the same pairs in the same order as the device:
  // two barriers per reduction instead of two per step (that all 64 ends carry the same bits is what the tests then observe)
  grid_sim_sync();  // (every lane has read the values of the previous reduction)
  for (int i = 0; i < N; ++i) g.xch[i * 64 + l] = v[i];
  grid_sim_sync();
  for (int i = 0; i < N; ++i) v[i] = grid_sim_butterfly(g.xch + i * 64, 6, l);
#else
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = v[i];
    x = x + grid_dpp<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x = x + grid_dpp<0x4E>(x);   // quad_perm [2, 3, 0, 1]
    x = x + grid_dpp<0x141>(x);  // row_half_mirror
    x = x + grid_dpp<0x140>(x);  // row_mirror
    int lo = __double2loint(x), hi = __double2hiint(x);
    const auto l32 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto h32 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    x = __hiloint2double(h32[0], l32[0]) + __hiloint2double(h32[1], l32[1]);  // lower half + upper half, in both halves
    lo = __double2loint(x), hi = __double2hiint(x);
    const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v[i] = __hiloint2double(h16[0], l16[0]) + __hiloint2double(h16[1], l16[1]);  // even row + odd row, in both rows
  }
#endif
}

// grid_transform (i2c_cell.hpp) with the points strided over the wavefront: the same moments, centred about y0 = f(m) the same way.
// Lane l takes the points p = l + 64 k, k < ceil(N / 64); the digits of p (digit 0 fastest, as in the one-lane odometer) are decoded
// once and then advanced by 64 in base gh_degree. A lane whose p >= N evaluates the centre with weight 0: finite, and nothing added.
// The trip count is wave-uniform and every lane reaches the reduction.
template <class M, int DIN, int DOUT, bool CROSS, typename R, class F>
I2C_FN void grid_transform_wave(const Rule<R>& rule, const R* m, const R* L, const F& f, R* my, R* Sy, R* Sxy) {
  constexpr int NA = M::NA, NA1 = NA > 0 ? NA : 1;
  constexpr int NRED = grid_nred<DIN, DOUT, CROSS>(), O_S2 = DOUT, O_SX = DOUT + sym(DOUT);
  R sn[NA1], cs[NA1], y0[DOUT], acc[NRED];  // acc = [s1 | S2 packed | Sxy]
#pragma unroll
  for (int a = 0; a < NA; ++a) r_sincos(m[M::ang(a)], &sn[a], &cs[a]);
  f(m, sn, cs, y0);
#pragma unroll
  for (int k = 0; k < NRED; ++k) acc[k] = R(0);
  const int deg = rule.gh_degree, npts = rule.gh_points, lane = grid_lane();
  int dig[DIN], step[DIN];  // digits of this lane's point, and of the stride 64
  {
    int q = lane, s = 64;
#pragma unroll
    for (int i = 0; i < DIN; ++i) {
      dig[i] = q % deg, q /= deg;
      step[i] = s % deg, s /= deg;
    }
  }
  for (int p0 = 0; p0 < npts; p0 += 64) {
    const bool live = p0 + lane < npts;
    R xi[DIN], w = live ? R(1) : R(0);
#pragma unroll
    for (int i = 0; i < DIN; ++i) {
      R xv = rule.gh_x[0], wv = rule.gh_w[0];
#pragma unroll
      for (int q = 1; q < I2C_MAX_GH_DEGREE; ++q) {
        xv = dig[i] == q ? rule.gh_x[q] : xv;
        wv = dig[i] == q ? rule.gh_w[q] : wv;
      }
      xi[i] = live ? xv : R(0);
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
      acc[k] += wy;
#pragma unroll
      for (int l = 0; l <= k; ++l) acc[O_S2 + tri(k, l)] += wy * y[l];
      if (CROSS) {
#pragma unroll
        for (int i = 0; i < DIN; ++i) acc[O_SX + i * DOUT + k] += dx[i] * wy;
      }
    }
    // the odometer advanced by 64: digit-wise addition with carry (every digit and every step digit is below gh_degree)
    int carry = 0;
#pragma unroll
    for (int i = 0; i < DIN; ++i) {
      const int nd = dig[i] + step[i] + carry;
      carry = nd >= deg ? 1 : 0;
      dig[i] = carry ? nd - deg : nd;
    }
  }
  grid_allreduce<NRED>(acc);
#pragma unroll
  for (int k = 0; k < DOUT; ++k) my[k] = y0[k] + acc[k];
#pragma unroll
  for (int k = 0; k < DOUT; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) Sy[tri(k, l)] = acc[O_S2 + tri(k, l)] - acc[k] * acc[l];
  if (CROSS) {
#pragma unroll
    for (int k = 0; k < DIN * DOUT; ++k) Sxy[k] = acc[O_SX + k];
  }
}

// ---- the three sweeps: the one-lane cell bodies, run by every lane of the trajectory's wavefront ---------------------------------
// (the generic forward body: per-cell targets and temperatures, the ring offset, prior_out -- all of it is in there)
enum { GRK_FORWARD = 0, GRK_BACKWARD = 1, GRK_PROPAGATE = 2 };
constexpr int GRID_WAVES_PER_BLOCK = 4;  // one per SIMD of a compute unit
template <int KIND, class M, typename R, class A> I2C_FN void grid_body(const Consts<M, R>& c, const A& a, const int b) {
  if constexpr (KIND == GRK_FORWARD) forward_sweep_body<M, R, false, GRID_WAVE, R>(c, a, b);
  if constexpr (KIND == GRK_BACKWARD) backward_fused_body<M, R, GRID_WAVE, R, false>(c, a, b);
  if constexpr (KIND == GRK_PROPAGATE) propagate_body<M, R, GRID_WAVE>(c, a, b);
}
#ifndef I2C_HOST_SIM
// trajectory of this wavefront; behind the batch's end the whole wave leaves (wave-uniform)
__device__ __forceinline__ long grid_traj() { return (long)blockIdx.x * GRID_WAVES_PER_BLOCK + (threadIdx.x >> 6); }
template <class M, typename R>
__global__ __launch_bounds__(64 * GRID_WAVES_PER_BLOCK) void k_grid_forward(const Consts<M, R> c, const FwdArgs<R, R> a) {
  const long b = grid_traj();
  if (b < c.B) grid_body<GRK_FORWARD, M, R>(c, a, (int)b);
}
template <class M, typename R>
__global__ __launch_bounds__(64 * GRID_WAVES_PER_BLOCK) void k_grid_backward(const Consts<M, R> c, const CellArgs<R, R> a) {
  const long b = grid_traj();
  if (b < c.B) grid_body<GRK_BACKWARD, M, R>(c, a, (int)b);
}
template <class M, typename R>
__global__ __launch_bounds__(64 * GRID_WAVES_PER_BLOCK) void k_grid_propagate(const Consts<M, R> c, const PropArgs<R> a) {
  const long b = grid_traj();
  if (b < c.B) grid_body<GRK_PROPAGATE, M, R>(c, a, (int)b);
}
#endif

}  // namespace i2c
