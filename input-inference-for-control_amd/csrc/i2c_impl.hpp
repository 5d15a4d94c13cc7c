// Kernels and their launchers for one (model, dtype) pair: Impl<M, R>, instantiated by i2c_model_tu.hip.
//
// Built two ways:
//   hipcc --offload-arch=gfx950            -> libi2c_hip.so      (THE product; the only library
//                                                                 the Python package ever loads)
//   g++ -x c++ -DI2C_HOST_SIM              -> libi2c_hostsim.so  (tests only: the same cell math
//                                                                 looped on the CPU so that kernel
//                                                                 numerics can be checked against the
//                                                                 oracle on a box without a GPU)
//
// Layout: the launch layer of the one-lane kernels (launch(), I2C_KERNEL) and those kernels; the launch layer of the multi-lane
// kernels (host simulation: sim_teams(); device: I2C_QUAD_SETUP / launch_quad(), the XCD placement) and the group, wave and quad
// kernels, each with its launcher, and the launcher of the grid kernels; the problem constants, the chunk workspace and the per-model
// batch sizes; Impl<M, R, S>: which family and schedule serve a problem (resolve -> Plan), what a call launches beyond that (launches ->
// Launches: the schedule that runs, the couplings of an i2c_learn iteration's sweeps), the sweeps' launchers and the entry points.
#pragma once
#include "i2c_entry.hpp"
#include "i2c_cell.hpp"
#include "i2c_group.hpp"
#include "i2c_wave.hpp"
#include "i2c_quad.hpp"
#include "i2c_grid.hpp"
#include "i2c_linearize.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace i2c {

// One wavefront per workgroup for the sequential sweeps: at B = 4096 that is 64 workgroups on
// 64 different CUs, each wave with a CU's issue ports, L1 and scalar cache to itself.
constexpr int SWEEP_BLOCK = 64;   // a wavefront: workgroup of the group kernels and of k_reduce
// Workgroup of the one-lane-per-trajectory kernels: ONE wavefront. (Round 5 measured four -- the hardware deals the waves of one
// workgroup onto the four SIMDs of its CU, while single-wave workgroups may double up on a SIMD, see quad_waves_per_block below --
// and kept one: these kernels move a 512-byte segment of a different row with every memory instruction, and four waves behind ONE
// CU's memory pipeline cost more than a doubled SIMD: pendulum B = 16384 backward 0.19 -> 0.28 ms, planar quadrotor B = 1024
// backward 0.071 -> 0.100, covariance-control iteration 0.18 -> 0.28; no shape got faster. -DI2C_LANE_BLOCK=256 rebuilds that.)
#ifndef I2C_LANE_BLOCK
#define I2C_LANE_BLOCK 64
#endif
constexpr int LANE_BLOCK = I2C_LANE_BLOCK;
constexpr int CELL_BLOCK = 256;

// ---- the ONE place that knows how a per-lane body runs ---------------------------------------------------------------
// (one lane per trajectory; the bodies that run as a TEAM of lanes -- group, wave and quad kernels -- have theirs further down:
// "the ONE place that knows how a multi-lane body runs")
// Device: a HIP kernel, lane index from the block / thread ids, started by launch() through hipLaunchKernelGGL.
// Host simulation (tests only): the same function with the lane indices as leading arguments, looped by launch().
// A kernel is written once:   template <...> I2C_KERNEL(BLOCK) k_name(I2C_LANE_PARAMS const C c, const A a) {
//                               const int b = I2C_LANE_X(BLOCK); ... I2C_LANE_Y ... }
#ifdef I2C_HOST_SIM
#define I2C_KERNEL(BLOCK) static void
#define I2C_LANE_PARAMS const long lane_x_, const int lane_y_,
#define I2C_LANE_X(BLOCK) ((void)lane_y_, lane_x_)
#define I2C_LANE_Y lane_y_
template <class K, class... A>
static int launch(K kernel, const long n, const int ny, const int /*block*/, void* /*stream*/, const A&... args) {
  for (int y = 0; y < ny; ++y)
    for (long x = 0; x < n; ++x) kernel(x, y, args...);
  return I2C_OK;
}
static int copy_bytes(void* dst, const void* src, size_t n, void*) {
  std::memcpy(dst, src, n);
  return I2C_OK;
}
static int sweep_lanes() { return LANE_BLOCK; }  // (the device form's experiment knob does not exist here)
#else
#define I2C_KERNEL(BLOCK) __global__ __launch_bounds__(BLOCK) void
#define I2C_LANE_PARAMS
#define I2C_LANE_X(BLOCK) ((long)blockIdx.x * (BLOCK) + threadIdx.x)
#define I2C_LANE_Y ((int)blockIdx.y)
// Experiment knob (not part of the ABI): I2C_SWEEP_LANES=<n<=64> launches the sequential sweeps with
// n active lanes per wavefront (more, emptier waves on more SIMDs).
static int sweep_lanes() {
  static int v = [] {
    const char* e = getenv("I2C_SWEEP_LANES");
    const int n = e ? atoi(e) : LANE_BLOCK;
    return (n >= 1 && n <= LANE_BLOCK) ? n : LANE_BLOCK;
  }();
  return v;
}
template <class K, class... A>
static int launch(K kernel, const long n, const int ny, const int block, void* stream, const A&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + block - 1) / block), ny), dim3(block), 0, (hipStream_t)stream, args...);
  return hipGetLastError() == hipSuccess ? I2C_OK : I2C_ELAUNCH;
}
static int copy_bytes(void* dst, const void* src, size_t n, void* stream) {
  return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? I2C_OK : I2C_ELAUNCH;
}
#endif

template <class M, typename R, bool LEAN, bool GRID = false, typename S = R>
I2C_KERNEL(LANE_BLOCK) k_forward(I2C_LANE_PARAMS const Consts<M, R> c, const FwdArgs<R, S> a, const int block) {
  const long b = I2C_LANE_X(block);  // `block` = active lanes per wave (I2C_SWEEP_LANES experiment), normally 64
  if (b < c.B) forward_sweep_body<M, R, LEAN, GRID, S>(c, a, (int)b);
}
template <class M, typename R> I2C_KERNEL(LANE_BLOCK) k_forward_lin(I2C_LANE_PARAMS const Consts<M, R> c, const FwdArgs<R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) forward_lin_body<M, R>(c, a, (int)b);
}
template <class M, typename R> I2C_KERNEL(LANE_BLOCK) k_bwd_lin(I2C_LANE_PARAMS const Consts<M, R> c, const CellArgs<R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) backward_lin_body<M, R>(c, a, (int)b);
}
template <class M, typename R> I2C_KERNEL(LANE_BLOCK) k_riccati(I2C_LANE_PARAMS const Consts<M, R> c, const RiccatiArgs<R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) riccati_body<M, R>(c, a, (int)b);
}
template <class M, typename R, typename S = R>
I2C_KERNEL(LANE_BLOCK) k_scan(I2C_LANE_PARAMS const Consts<M, R> c, const ScanArgs<R, S> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) backward_scan_body<M, R, S>(c, a, (int)b);
}
template <class M, typename R, typename S = R>
I2C_KERNEL(CELL_BLOCK) k_cell(I2C_LANE_PARAMS const Consts<M, R> c, const CellArgs<R, S> a) {
  const long b = I2C_LANE_X(CELL_BLOCK);
  if (b < c.B) backward_cell_body<M, R, S>(c, a, I2C_LANE_Y, (int)b);
}
template <class M, typename R, bool GRID = false, typename S = R, bool LEANW = false>
I2C_KERNEL(LANE_BLOCK) k_bwd_fused(I2C_LANE_PARAMS const Consts<M, R> c, const CellArgs<R, S> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) backward_fused_body<M, R, GRID, S, LEANW>(c, a, (int)b);
}
template <class M, typename R, typename S = R>
I2C_KERNEL(LANE_BLOCK) k_chunk_compose(I2C_LANE_PARAMS const Consts<M, R> c, const ChunkArgs<R, S> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) chunk_compose_body<M, R, S>(c, a, I2C_LANE_Y, (int)b);
}
template <class M, typename R, typename S = R, bool GRID = false>
I2C_KERNEL(LANE_BLOCK) k_chunk_stitch(I2C_LANE_PARAMS const Consts<M, R> c, const ChunkArgs<R, S> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) chunk_stitch_body<M, R, S, GRID>(c, a, (int)b);
}
#ifndef I2C_WALK_LEAN
#define I2C_WALK_LEAN 1
#endif
template <class M, typename R, typename S = R, bool LEANW = false, bool GRID = false>
I2C_KERNEL(LANE_BLOCK) k_chunk_walk(I2C_LANE_PARAMS const Consts<M, R> c, const ChunkArgs<R, S> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) chunk_walk_body<M, R, S, LEANW, GRID>(c, a, I2C_LANE_Y, (int)b);
}
// the self-stitching walker (chunk_walk_body<SELF>): the stitch pass's work in the prologue of the walk, d <= 5
template <class M, typename R, typename S = R, bool LEANW = false>
I2C_KERNEL(LANE_BLOCK) k_chunk_walk_self(I2C_LANE_PARAMS const Consts<M, R> c, const ChunkArgs<R, S> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) chunk_walk_body<M, R, S, LEANW, 0, true>(c, a, I2C_LANE_Y, (int)b);
}
template <class M, typename R> I2C_KERNEL(LANE_BLOCK) k_chunk_stitch_lin(I2C_LANE_PARAMS const Consts<M, R> c, const ChunkArgs<R, R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) chunk_stitch_lin_body<M, R>(c, a, (int)b);
}
template <class M, typename R> I2C_KERNEL(LANE_BLOCK) k_chunk_walk_lin(I2C_LANE_PARAMS const Consts<M, R> c, const ChunkArgs<R, R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) chunk_walk_lin_body<M, R>(c, a, I2C_LANE_Y, (int)b);
}
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_chunk_reduce_lin(I2C_LANE_PARAMS const Consts<M, R> c, const ChunkArgs<R, R> a, const MstepArgs<R> ms) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) chunk_reduce_lin_body<M, R>(c, a, ms, (int)b);
}
template <class M, typename R> I2C_KERNEL(LANE_BLOCK) k_mstep(I2C_LANE_PARAMS const Consts<M, R> c, const MstepArgs<R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) mstep_body<M, R>(c, a, (int)b);
}
template <class M, typename R, bool GRID = false>
I2C_KERNEL(LANE_BLOCK) k_propagate(I2C_LANE_PARAMS const Consts<M, R> c, const PropArgs<R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) propagate_body<M, R, GRID>(c, a, (int)b);
}
// The forward sweep of one EM iteration and the closed-loop propagation of the PREVIOUS one in ONE launch (grid row 0 / row 1).
// Both walk T dependent cells with one lane per trajectory, both only read the posterior buffer; at the batch sizes of covariance
// control (B = 8192: 128 wavefronts each) run one after the other they are two chains, in one dispatch the workgroup distributor
// deals the 256 workgroups onto 256 different CUs and they are one. (Two STREAMS do not do this: measured, the two kernels' waves
// land on the same SIMDs and the propagation takes 165 instead of 95 us -- profiles/r5_covctrl_overlap.txt.)
template <class M, typename R, bool LEAN>
I2C_KERNEL(LANE_BLOCK) k_forward_propagate(I2C_LANE_PARAMS const Consts<M, R> c, const FwdArgs<R, R> af, const PropArgs<R> ap) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b >= c.B) return;
  if (I2C_LANE_Y == 0) forward_sweep_body<M, R, LEAN, false, R>(c, af, (int)b);
  else propagate_body<M, R, false>(c, ap, (int)b);
}
template <class M, typename R> struct ZetaArg {
  R v[sym(M::NY)];
};
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_ckf(I2C_LANE_PARAMS const Consts<M, R> c, const ZetaArg<M, R> z, const CkfArgs<R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) ckf_filter_body<M, R>(c, z.v, a, (int)b);
}
template <class M, typename R> I2C_KERNEL(CELL_BLOCK) k_mpc_shift(I2C_LANE_PARAMS const Consts<M, R> c, const ShiftArgs<R> a) {
  const long b = I2C_LANE_X(CELL_BLOCK);
  if (b < c.B) mpc_shift_body<M, R>(c, a, (int)b);
}
// mode flags of cells 0 .. n-1 (ring rows t0 .. t0+n-1 mod T) to feedback: ONE launch (two hipMemsetAsync spans of odd length
// are split by the runtime into up to five fill kernels, 5 us each: a twentieth of a planar-quadrotor control step)
template <class M> I2C_KERNEL(CELL_BLOCK) k_to_feedback(I2C_LANE_PARAMS uint8_t* ff, const int t0, const int n, const int T) {
  const long i = I2C_LANE_X(CELL_BLOCK);
  if (i < n) ff[(t0 + (int)i) % T] = 0;
}
template <class M, typename R> I2C_KERNEL(LANE_BLOCK) k_rollout(I2C_LANE_PARAMS const Consts<M, R> c, const RolloutArgs<R> a) {
  const long n = I2C_LANE_X(LANE_BLOCK);
  if (n < (long)a.n_rollouts * c.B) rollout_body<M, R>(c, a, (int)n);
}
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_plant_step(I2C_LANE_PARAMS const Consts<M, R> c, const PlantNoise<M, R> nz, const PlantArgs<R> a) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) plant_step_body<M, R>(c, nz, a, (int)b);
}

// Per-trajectory horizons (I2cProblem.horizons, [B] int32): the HZ instantiations of the one-lane bodies (i2c_cell.hpp), fp64,
// sigma-point rule. Lane b reads its horizon once, clamped to [1, T], and hands it to the body; rollout n takes column n % B.
// One variant per sweep -- the generic forward cell, the walk with every optional output -- so a model adds five kernels.
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_forward_hz(I2C_LANE_PARAMS const Consts<M, R> c, const FwdArgs<R, R> a, const int32_t* const hz) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) forward_sweep_body<M, R, false, 0, R, NoRelease, true>(c, a, (int)b, NoRelease{0}, clamp_horizon(hz[b], c.T));
}
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_bwd_fused_hz(I2C_LANE_PARAMS const Consts<M, R> c, const CellArgs<R, R> a, const int32_t* const hz) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) backward_fused_body<M, R, 0, R, false, true>(c, a, (int)b, clamp_horizon(hz[b], c.T));
}
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_mstep_hz(I2C_LANE_PARAMS const Consts<M, R> c, const MstepArgs<R> a, const int32_t* const hz) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) mstep_body<M, R>(c, a, (int)b, clamp_horizon(hz[b], c.T));
}
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_propagate_hz(I2C_LANE_PARAMS const Consts<M, R> c, const PropArgs<R> a, const int32_t* const hz) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) propagate_body<M, R, 0, true>(c, a, (int)b, clamp_horizon(hz[b], c.T));
}
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_rollout_hz(I2C_LANE_PARAMS const Consts<M, R> c, const RolloutArgs<R> a, const int32_t* const hz) {
  const long n = I2C_LANE_X(LANE_BLOCK);
  if (n < (long)a.n_rollouts * c.B) rollout_body<M, R, true>(c, a, (int)n, clamp_horizon(hz[n % c.B], c.T));
}

// Monte-Carlo policy evaluation (i2c_rollout_eval): rollout_body with the generator's noise and the accumulating sink. A flat launch
// of parts * B lanes, lane x = part q * B + trajectory b: lane (q, b) runs rollouts q, q + parts, ... of trajectory b in turn. (Flat,
// not a part per grid row: a row of B = 1 would be a wavefront with one live lane -- measured, 65536 rollouts of one trajectory took
// 50 ms that way -- and the grid's second dimension stops at 65535.) The lanes of a wavefront are consecutive b of one part, or the tail
// of one part and the head of the next: every access of the [e][b] rows is one or two contiguous runs. Without moments parts =
// n_rollouts: one lane per rollout. `hz`: the horizons, or null.
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_rollout_eval(I2C_LANE_PARAMS const Consts<M, R> c, const RolloutArgs<R> a, const EvalArgs<R> ev,
                                      const int32_t* const hz) {
  const long x = I2C_LANE_X(LANE_BLOCK);
  const int q = (int)(x / c.B), b = (int)(x % c.B);
  if (q >= ev.parts) return;
  const int Tb = hz ? clamp_horizon(hz[b], c.T) : c.T;
  for (long r = q; r < a.n_rollouts; r += ev.parts) rollout_body<M, R, true, true>(c, a, b, Tb, &ev, (int)r, q, r == q);
}
// ... and its reduction: lane (t, b), t the grid's second dimension (one row of lanes when there are no moments)
template <class M, typename R>
I2C_KERNEL(LANE_BLOCK) k_rollout_eval_reduce(I2C_LANE_PARAMS const Consts<M, R> c, const EvalReduceArgs<R> a, const int32_t* const hz) {
  const long b = I2C_LANE_X(LANE_BLOCK);
  if (b < c.B) rollout_eval_reduce_body<M, R>(c, a, I2C_LANE_Y, (int)b, hz ? clamp_horizon(hz[b], c.T) : c.T);
}

// Sum of the per-cell cost statistics over t: REDUCE_PARTS lanes per trajectory, fixed summation order; with `ms.alpha`
// set (i2c_learn) the temperature M-step rides on it. The device form exchanges the partial sums through LDS; the host
// form walks the same partition in the same order.
constexpr int REDUCE_PARTS = 8;
template <class M, typename R, class CA>
I2C_FN void reduce_finish(const Consts<M, R>& c, const CA& a, const MstepArgs<R>& ms, const int T_mstep, const int b,
                          const R m, const R v) {
  a.term_stats[(long)c.B + b] = m;
  a.term_stats[2 * (long)c.B + b] = v;
  if (ms.alpha) {
    Consts<M, R> cm = c;
    cm.T = T_mstep;  // c.T is the number of summands here (cells or chunks), the M-step needs the horizon
    mstep_body<M, R>(cm, ms, b);
  }
}
#ifdef I2C_HOST_SIM
template <class M, typename R, class CA>
static int launch_reduce(const Consts<M, R>& c, const CA& a, const MstepArgs<R>& ms, const int T_mstep, void*) {
  for (int b = 0; b < c.B; ++b) {
    R m = R(0), v = R(0);
    for (int q = 0; q < REDUCE_PARTS; ++q) {
      R pm, pv;
      reduce_partial<M, R>(c, a.cell_stats, b, q, REDUCE_PARTS, &pm, &pv);
      m += pm;
      v += pv;
    }
    reduce_finish<M, R>(c, a, ms, T_mstep, b, m, v);
  }
  return I2C_OK;
}
#else
template <class M, typename R, class CA>
__global__ __launch_bounds__(SWEEP_BLOCK* REDUCE_PARTS) void k_reduce(const Consts<M, R> c, const CA a,
                                                                      const MstepArgs<R> ms, const int T_mstep) {
  __shared__ R sm[REDUCE_PARTS][SWEEP_BLOCK], sv[REDUCE_PARTS][SWEEP_BLOCK];
  const int b = blockIdx.x * SWEEP_BLOCK + threadIdx.x;
  R m = R(0), v = R(0);
  if (b < c.B) reduce_partial<M, R>(c, a.cell_stats, b, threadIdx.y, REDUCE_PARTS, &m, &v);
  sm[threadIdx.y][threadIdx.x] = m;
  sv[threadIdx.y][threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.y == 0 && b < c.B) {
    m = sm[0][threadIdx.x];
    v = sv[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < REDUCE_PARTS; ++q) {
      m += sm[q][threadIdx.x];
      v += sv[q][threadIdx.x];
    }
    reduce_finish<M, R>(c, a, ms, T_mstep, b, m, v);
  }
}
template <class M, typename R, class CA>
static int launch_reduce(const Consts<M, R>& c, const CA& a, const MstepArgs<R>& ms, const int T_mstep, void* stream) {
  hipLaunchKernelGGL((k_reduce<M, R, CA>), dim3((c.B + SWEEP_BLOCK - 1) / SWEEP_BLOCK), dim3(SWEEP_BLOCK, REDUCE_PARTS), 0,
                     (hipStream_t)stream, c, a, ms, T_mstep);
  return hipGetLastError() == hipSuccess ? I2C_OK : I2C_ELAUNCH;
}
#endif

// The reduction and M-step of one EM iteration finished by the NEXT iteration's forward sweep (i2c_learn behind a self-stitching
// chunked backward sweep; Impl::learn): lane b of k_forward_mstep adds the walkers' partial sums part[NC][2][B] of its trajectory in
// k_reduce's order, writes term_stats rows 1, 2 and runs the M-step (mstep_update) -- all before the sweep reads alpha[b], which that
// M-step updates. The kernel boundary behind the walk gives the visibility; the lane reads and writes only its own trajectory's
// elements, so nothing is exchanged between lanes. k_reduce -- a launch and a drain for O(NC) additions per trajectory -- then runs
// once per i2c_learn call, after the last iteration.
template <typename R> struct PendingMstep {
  const R* part;     // [NC][2][B]: the walkers' cost sums
  R* term_stats;     // [E_TERM][B]
  MstepArgs<R> ms;   // alpha, the iteration's row of the statistics history
  int n_chunks;
  R tol;             // the M-step's tolerance (the forward sweep's constants carry none)
};
// The order of the additions is k_reduce's: its lane q adds the chunks q, q + REDUCE_PARTS, ... in ascending order (reduce_partial) --
// accumulator q here --, then the partial sums are added in the order of q. At the head of a kernel every load is a round trip to
// memory, so the prologue makes ONE: the temperature, the terminal statistic and 2 x REDUCE_PARTS chunks' sums are requested before
// anything is stored (NC <= 16: all of them), and the M-step works on those registers instead of reading back what was just written.
// A round that reaches past the last chunk re-reads it and adds +0 instead, which changes no accumulator (none of them can hold -0:
// each starts from +0). Sigma-point rule only: the plan cost is the alpha statistic.
template <class M, typename R> I2C_FN void finish_pending_mstep(const Consts<M, R>& c, const PendingMstep<R>& pm, const int b) {
  using C = Consts<M, R>;
  constexpr int P = REDUCE_PARTS;
  const long B = c.B;
  const int nc = pm.n_chunks;
  const R alpha = pm.ms.alpha[b];
  const R trT = (C::NZT > 0 && c.has_Qf) ? pm.term_stats[b] : R(0);
  R sm[P], sv[P];
#pragma unroll
  for (int q = 0; q < P; ++q) sm[q] = sv[q] = R(0);
  for (int t0 = 0; t0 < nc; t0 += 2 * P) {
    R pm_t[2 * P], pv_t[2 * P];
#pragma unroll
    for (int i = 0; i < 2 * P; ++i) {
      const long t = t0 + i < nc ? t0 + i : nc - 1;
      pm_t[i] = pm.part[(t * 2 + 0) * B + b];
      pv_t[i] = pm.part[(t * 2 + 1) * B + b];
    }
#pragma unroll
    for (int i = 0; i < 2 * P; ++i) {
      const bool in = t0 + i < nc;
      sm[i % P] += in ? pm_t[i] : R(0);
      sv[i % P] += in ? pv_t[i] : R(0);
    }
  }
  R m = R(0), v = R(0);
#pragma unroll
  for (int q = 0; q < P; ++q) {
    m += sm[q];
    v += sv[q];
  }
  pm.term_stats[B + b] = m;  // (reduce_finish)
  pm.term_stats[2 * B + b] = v;
  Consts<M, R> cm = c;
  cm.tol = pm.tol;
  mstep_update<M, R>(cm, pm.ms, b, trT, m, v, m, alpha);
}
// (the time loop is forward_sweep_body's own: the prologue sits in front of it, outside)
template <class M, typename R, bool LEAN, typename S = R>
I2C_KERNEL(LANE_BLOCK) k_forward_mstep(I2C_LANE_PARAMS const Consts<M, R> c, const FwdArgs<R, S> a, const int block, const PendingMstep<R> pm) {
  const long b = I2C_LANE_X(block);
  if (b < c.B) {
    finish_pending_mstep<M, R>(c, pm, (int)b);
    forward_sweep_body<M, R, LEAN, 0, S>(c, a, (int)b);
  }
}

// The forward sweep of i2c_learn with a HELPER wavefront (Impl::launches): a workgroup of two waves over the same 64
// trajectories. Wave 0 is k_forward / k_forward_mstep and releases every chunk of the chunked backward schedule once its messages are
// stored (ChunkRelease, i2c_cell.hpp); wave 1 -- on another SIMD of the same CU, so it takes no issue slot from the chain -- waits at
// the workgroup barrier and then composes that chunk with chunk_compose_body, unchanged: the composites are k_chunk_compose's bit
// for bit, and the backward sweep that follows starts with its walk. Both waves take the chunk geometry from the same argument and
// meet at the barrier n_chunks times; nothing is exchanged through flags in memory. (Every wave has a live lane: the grid covers B.)
// Host simulation: a lane's sweep, then its chunks -- a valid schedule, compose reads only finished rows.
// GAINH (fp64-stored messages; Launches::helper_gain): wave 0 hands the smoother gain over as well (ChunkReleaseGain, i2c_cell.hpp) and
// wave 1 finishes it cell by cell inside its compose loop (chunk_compose_gain_body). The flagged cell's sig_x3 travels through the
// first sym(NX) rows of the per-chunk cost sums `part` [NC][3][B] of the chunk workspace, which are dead while a sweep of i2c_learn
// runs: the pending M-step has read them in this kernel's prologue, lane b its own column b as here, and the walk behind the sweep
// writes every one of them again before anything reads them (Impl::launches keeps the variant to 3 NC >= sym(NX)).
template <class M, typename R, bool LEAN, typename S, bool MSTEP, bool GAINH>
I2C_FN void forward_helper_lane(const Consts<M, R>& c, const FwdArgs<R, S>& a, const ChunkArgs<R, S>& ch, const PendingMstep<R>& pm,
                                const int role, const int b) {
  if constexpr (GAINH) {
    static_assert(sizeof(S) == sizeof(R), "the gain hand-off is not rounded to a narrower storage type");
    R* const term_sig = ch.part;
    if (role == 0) {
      if constexpr (MSTEP) finish_pending_mstep<M, R>(c, pm, b);
      forward_sweep_body<M, R, LEAN, 0, S, ChunkReleaseGain<R>>(c, a, b, ChunkReleaseGain<R>{ch.chunk_len, term_sig});
    } else {
      for (int k = 0; k < ch.n_chunks; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
        chunk_compose_gain_body<M, R>(c, ch, term_sig, k, b);
      }
    }
  } else if (role == 0) {
    if constexpr (MSTEP) finish_pending_mstep<M, R>(c, pm, b);
    forward_sweep_body<M, R, LEAN, 0, S, ChunkRelease>(c, a, b, ChunkRelease{ch.chunk_len});
  } else {
    for (int k = 0; k < ch.n_chunks; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
      chunk_compose_body<M, R, S>(c, ch, k, b);
    }
  }
}
#ifdef I2C_HOST_SIM
constexpr int HELPER_WAVES = 1;  // (lanes per trajectory that launch() loops over)
#define I2C_HELPER_LANES                                                                \
  const long b = I2C_LANE_X(LANE_BLOCK);                                                \
  for (int role = 0; role < 2; ++role)
#else
constexpr int HELPER_WAVES = 2;
#define I2C_HELPER_LANES                                                                \
  const long b = (long)blockIdx.x * LANE_BLOCK + (threadIdx.x & (LANE_BLOCK - 1));      \
  const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LANE_BLOCK));     \
  if (b < c.B)
#endif
template <class M, typename R, bool LEAN, typename S = R, bool GAINH = false>
I2C_KERNEL(2 * LANE_BLOCK) k_forward_helper(I2C_LANE_PARAMS const Consts<M, R> c, const FwdArgs<R, S> a, const ChunkArgs<R, S> ch) {
  I2C_HELPER_LANES forward_helper_lane<M, R, LEAN, S, false, GAINH>(c, a, ch, PendingMstep<R>{}, role, (int)b);
}
template <class M, typename R, bool LEAN, typename S = R, bool GAINH = false>
I2C_KERNEL(2 * LANE_BLOCK) k_forward_mstep_helper(I2C_LANE_PARAMS const Consts<M, R> c, const FwdArgs<R, S> a, const ChunkArgs<R, S> ch,
                                                  const PendingMstep<R> pm) {
  I2C_HELPER_LANES forward_helper_lane<M, R, LEAN, S, true, GAINH>(c, a, ch, pm, role, (int)b);
}
#undef I2C_HELPER_LANES

// ---- the ONE place that knows how a multi-lane body runs -----------------------------------------------------------------------
// The group, wave and quad kernels run a body as a TEAM of lanes (G, 64, 64) that share an LDS region and exchange values across lanes.
// Device: the set-up of a team lives in one place per family -- k_group, k_wave, and for the seven quad kernels I2C_QUAD_SETUP (constants
// into LDS, the lane's four-trajectory slot, the wave-uniform exit, the Quad<R>) with launch_quad() (grid formula, error tail).
// Host simulation (tests only): sim_teams() is the only function that starts threads; a launcher passes it the team size, the LDS size
// and its body, sim_quad() adds the decoding of a quad lane. Each launch_*() below is written once, with the two forms side by side.
// Shared by both: the unit-rule predicate and the GENERAL x LEANQ variant choice of the quad launchers.

// cubature weights with lam = 0: unit weights, no weight on the centre (every shipped config) -- of one rule, or of both rules of a problem
template <typename R> static bool unit_rule(const Rule<R>& r) { return r.unit && r.w0 == R(0); }
template <class M, typename R> static bool unit_rule(const Consts<M, R>& c) { return unit_rule(c.rule_xu) && unit_rule(c.rule_x); }

#ifdef I2C_HOST_SIM
// body(i, y, l, sh, &bar, xch) for every team i < n_teams, grid row y < n_rows and lane l < team: the lanes of a team are threads that share
// a barrier (waited on wherever the device code has its LDS fence or a cross-lane instruction), a zeroed LDS region of `lds` elements and
// the 128 exchange slots of the emulated cross-lane instructions. rows_on_team = false: every grid row is a team of its own (one CELL per
// row: the wave two-pass schedule). true: a team walks its rows one after the other on the same threads (one CHUNK per row: the simulated
// wavefront of a quad group walks its chunks in turn -- 64 threads per group, not 64 per group and chunk).
template <typename R, class Body>
static void sim_teams(const int team, const long n_teams, const int n_rows, const bool rows_on_team, const size_t lds, const Body& body) {
  for (int y0 = 0; y0 < (rows_on_team ? 1 : n_rows); ++y0)
    for (long i = 0; i < n_teams; ++i) {
      std::vector<R> sh(lds, R(0)), xch(128, R(0));
      HostBarrier bar(team);
      std::vector<std::thread> lanes;
      for (int l = 0; l < team; ++l)
        lanes.emplace_back([&, l] {
          for (int y = y0; y < (rows_on_team ? n_rows : y0 + 1); ++y) body(i, y, l, lds ? sh.data() : (R*)nullptr, &bar, xch.data());
        });
      for (auto& th : lanes) th.join();
    }
}
#else
// The batch constants are unpacked into LDS with per-lane indices, read straight from the kernel-argument segment: `c` is the first
// kernel parameter (offset 0), `zeta` -- where a kernel has it -- follows it at its natural alignment.
template <class M, typename R> __device__ __forceinline__ const Consts<M, R>* kernarg_consts() {
  return (const Consts<M, R>*)__builtin_amdgcn_kernarg_segment_ptr();
}
template <class M, typename R> __device__ __forceinline__ const R* kernarg_zeta() {
  constexpr size_t zoff = (sizeof(Consts<M, R>) + alignof(ZetaArg<M, R>) - 1) / alignof(ZetaArg<M, R>) * alignof(ZetaArg<M, R>);
  return ((const ZetaArg<M, R>*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + zoff))->v;
}
// XCD placement: first trajectory of workgroup i, and the grid that covers B trajectories with it (one wave of k_wave = one trajectory,
// four waves per workgroup; one single-wave workgroup of k_quad_forward = four trajectories).
// k_wave: a wave reads ONE 8-byte element of every [B]-contiguous row: the 16 trajectories that share a 128-byte line of each row
// are mapped onto four workgroups of the SAME XCD (workgroups are dealt round-robin over the 8 XCDs, so blocks i and i + 8
// share an L2): every line is then fetched from HBM once per XCD instead of once per wave.
// k_quad_forward with single-wave workgroups: a wave reads four consecutive trajectories (32 bytes) of every [B]-contiguous row: the
// four waves that share a 128-byte line of each row are mapped onto workgroups of the SAME XCD in the same way.
// Placement is a speed heuristic only -- any mapping computes the same result.
__device__ __forceinline__ long xcd_first_traj(const unsigned i) {
  const unsigned x = i & 7u, r = (i >> 3) & 3u, g = i >> 5;
  return 16L * (g * 8u + x) + 4 * r;
}
static unsigned xcd_blocks(const long B) { return (unsigned)((B + 127) / 128) * 32u; }
#endif

// ---- group kernels (i2c_group.hpp): G lanes per trajectory, 64 / G trajectories per wavefront ------------------------
// KIND selects the sweep; the bodies share their argument plumbing. Device: one wave per workgroup, the batch constants
// and every group's exchange region in LDS. Host simulation: the G lanes of a group are G threads.
enum { GK_FORWARD = 0, GK_BACKWARD = 1, GK_PROPAGATE = 2, GK_CKF = 3 };
// FULLW: non-diagonal cost weights (only the sweeps that price the cost, backward and propagate, have that variant)
template <int KIND, class M, typename R, int G, bool FULLW, class KC, class A>
I2C_FN void group_body(const Consts<M, R>& c, const KC& kc, const A& a, const int b, const Grp<R, G>& g) {
  if constexpr (KIND == GK_FORWARD) forward_group_body<M, R, G, FULLW>(c, kc, a, b, g);  // (FULLW: the lean variant here)
  if constexpr (KIND == GK_BACKWARD) backward_group_body<M, R, G, FULLW>(c, kc, a, b, g);
  if constexpr (KIND == GK_PROPAGATE) propagate_group_body<M, R, G, FULLW>(c, kc, a, b, g);
  if constexpr (KIND == GK_CKF) ckf_group_body<M, R, G>(c, kc, a, b, g);
}
#ifndef I2C_HOST_SIM
template <int KIND, class M, typename R, int G, bool FULLW, class A>
__global__ __launch_bounds__(SWEEP_BLOCK) void k_group(const Consts<M, R> c, const ZetaArg<M, R> zeta, const int has_zeta, const A a) {
  __shared__ GConst<M, R> kc;
  __shared__ R sh[(SWEEP_BLOCK / G) * Grp<R, G>::SIZE];
  gconst_fill<M, R>(kc, kernarg_consts<M, R>(), has_zeta ? kernarg_zeta<M, R>() : (const R*)nullptr, (int)threadIdx.x, SWEEP_BLOCK);
  __syncthreads();
  const long lane = (long)blockIdx.x * SWEEP_BLOCK + threadIdx.x;
  const long b = lane / G;
  if (b >= c.B) return;
  const Grp<R, G> g{(int)(threadIdx.x % G), (lds_ptr<R>)(sh + (threadIdx.x / G) * Grp<R, G>::SIZE)};
  group_body<KIND, M, R, G, FULLW>(c, kc, a, (int)b, g);
}
#endif
template <int KIND, class M, typename R, int G, bool FULLW, class A>
static int launch_group_w(const Consts<M, R>& c, const ZetaArg<M, R>* zeta, const A& a, void* stream) {
#ifdef I2C_HOST_SIM
  GConst<M, R> kc;
  gconst_fill<M, R>(kc, &c, zeta ? zeta->v : (const R*)nullptr, 0, 1);
  sim_teams<R>(G, c.B, 1, false, Grp<R, G>::SIZE, [&](const long b, int, const int r, R* sh, HostBarrier* bar, R*) {
    group_body<KIND, M, R, G, FULLW>(c, kc, a, (int)b, Grp<R, G>{r, sh, bar});
  });
  return I2C_OK;
#else
  ZetaArg<M, R> z{};
  if (zeta) z = *zeta;
  const long lanes = (long)c.B * G;
  hipLaunchKernelGGL((k_group<KIND, M, R, G, FULLW, A>), dim3((unsigned)((lanes + SWEEP_BLOCK - 1) / SWEEP_BLOCK)), dim3(SWEEP_BLOCK), 0,
                     (hipStream_t)stream, c, z, zeta ? 1 : 0, a);
  return hipGetLastError() == hipSuccess ? I2C_OK : I2C_ELAUNCH;
#endif
}

// ---- wave kernels (i2c_wave.hpp): one wavefront per trajectory, four per workgroup ----------------------------------------------
enum { WK_FORWARD = 0, WK_BACKWARD = 1, WK_SCAN = 2, WK_CELL = 3, WK_FORWARD_PL = 4 };  // _PL: pivot blocks through LDS
constexpr int WAVES_PER_BLOCK = 4;
template <int KIND, class M, typename R, typename S, bool LIN, class KC, class A>
I2C_FN void wave_body(const Consts<M, R>& c, const KC& kc, const A& a, const int t, const int b, const Wave<R>& w) {
  if constexpr (KIND == WK_FORWARD) forward_wave_body<M, R, S, LIN, false>(c, kc, a, b, w);
  if constexpr (KIND == WK_FORWARD_PL) forward_wave_body<M, R, S, LIN, true>(c, kc, a, b, w);
  if constexpr (KIND == WK_BACKWARD) backward_wave_body<M, R, S, LIN>(c, kc, a, b, w);
  if constexpr (KIND == WK_SCAN) backward_wave_scan_body<M, R, S>(c, kc, a, b, w);
  if constexpr (KIND == WK_CELL) backward_wave_cell_body<M, R, S>(c, kc, a, t, b, w);  // one wave per (t, b)
}
#ifndef I2C_HOST_SIM
template <int KIND, class M, typename R, typename S, bool LIN, class A>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, 2) void k_wave(const Consts<M, R> c, const A a) {
  __shared__ WConst<M, R> kc;
  __shared__ R sh[WAVES_PER_BLOCK * WaveLds::SIZE];
  wconst_fill<M, R>(kc, kernarg_consts<M, R>(), (int)threadIdx.x, 64 * WAVES_PER_BLOCK);
  __syncthreads();
  const long b = xcd_first_traj(blockIdx.x) + (threadIdx.x >> 6);
  if (b >= c.B) return;
  const int l = (int)(threadIdx.x & 63u);
  const Wave<R> w{l, l >> 4, l & 15, (lds_ptr<R>)(sh + (threadIdx.x >> 6) * WaveLds::SIZE)};
  wave_body<KIND, M, R, S, LIN>(c, kc, a, (int)blockIdx.y, (int)b, w);
}
#endif
template <int KIND, class M, typename R, typename S, bool LIN, class A>
static int launch_wave_v(const Consts<M, R>& c, const A& a, void* stream) {
  const int n_rows = KIND == WK_CELL ? c.T : 1;
#ifdef I2C_HOST_SIM
  WConst<M, R> kc;
  wconst_fill<M, R>(kc, &c, 0, 1);
  sim_teams<R>(64, c.B, n_rows, false, WaveLds::SIZE, [&](const long b, const int t, const int l, R* sh, HostBarrier* bar, R* xch) {
    wave_body<KIND, M, R, S, LIN>(c, kc, a, t, (int)b, Wave<R>{l, l >> 4, l & 15, sh, bar, xch});
  });
  return I2C_OK;
#else
  hipLaunchKernelGGL((k_wave<KIND, M, R, S, LIN, A>), dim3(xcd_blocks(c.B), (unsigned)n_rows), dim3(64 * WAVES_PER_BLOCK), 0, (hipStream_t)stream, c, a);
  return hipGetLastError() == hipSuccess ? I2C_OK : I2C_ELAUNCH;
#endif
}

// ---- quad kernels (i2c_quad.hpp): four trajectories per wavefront, four wavefronts per workgroup ------------------------------
// Workgroup of the quad kernels: FOUR wavefronts for every model (round 5; d <= 8 had one). With single-wave workgroups the
// dispatcher dealt 1024 waves as four per CU, but inside a CU a wave could land on a SIMD that already had one while another
// stayed empty (s_getreg HW_ID of every wave, profiles/r5_wave_placement.txt: 28 - 35 of 1024 SIMDs doubled) -- depending on the
// batch size and on what ran before, the SAME forward sweep took 1.27 or 1.87 ms (double cartpole B = 4096 / 4032; cartpole
// 1.39 / 2.02): the two-waves-per-SIMD issue rate for the whole launch, which is as slow as its slowest wave. The waves of ONE
// workgroup go to the four SIMDs of its CU: 1.26 ms at every batch size <= 4096. They also cover one whole 128-byte line of every
// [B]-contiguous row between them (four trajectories = 32 bytes per wave).
#ifndef I2C_QUAD_WPB
#define I2C_QUAD_WPB 4
#endif
template <class M> constexpr int quad_waves_per_block() { return QG<M>::WIDE ? 4 : I2C_QUAD_WPB; }
constexpr int QB_WAVES_PER_BLOCK = 4;  // ... and of the backward sweep and the chunk passes
// the batch constants of a quad kernel, by the type of its LDS copy (zeta: the filter step's alone; NoConst: the compose pass has none)
struct NoConst {};
template <class M, typename R> I2C_FN void quad_const_fill(NoConst&, const Consts<M, R>*, const R*, const int, const int) {}
template <class M, typename R> I2C_FN void quad_const_fill(QConst<M, R>& k, const Consts<M, R>* c, const R*, const int tid, const int n) { qconst_fill<M, R>(k, c, tid, n); }
template <class M, typename R> I2C_FN void quad_const_fill(QBConst<M, R>& k, const Consts<M, R>* c, const R*, const int tid, const int n) { qbconst_fill<M, R>(k, c, tid, n); }
template <class M, typename R> I2C_FN void quad_const_fill(QPConst<M, R>& k, const Consts<M, R>* c, const R*, const int tid, const int n) { qpconst_fill<M, R>(k, c, tid, n); }
template <class M, typename R> I2C_FN void quad_const_fill(QKConst<M, R>& k, const Consts<M, R>* c, const R* zeta, const int tid, const int n) { qkconst_fill<M, R>(k, c, zeta, tid, n); }
#ifdef I2C_HOST_SIM
// a simulated quad wavefront: lane l serves slot g = (l >> 2) & 3 of its four trajectories with `lsz` LDS elements each; the slots behind the
// batch's end run on its last trajectory with live = false. body(kc, b, live, q, chunk); n_chunks = 0: a kernel without a chunk row
template <class KC, class M, typename R, class Body>
static int sim_quad(const Consts<M, R>& c, const R* zeta, const int lsz, const int n_chunks, const Body& body) {
  KC kc;
  quad_const_fill<M, R>(kc, &c, zeta, 0, 1);
  sim_teams<R>(64, (c.B + 3) / 4, n_chunks ? n_chunks : 1, true, (size_t)4 * lsz, [&](const long i, const int ch, const int l, R* sh, HostBarrier* bar, R* xch) {
    const int g = (l >> 2) & 3, b = 4 * (int)i + g;
    const bool live = b < c.B;
    body(kc, live ? b : c.B - 1, live, Quad<R>{l, l >> 4, g, l & 3, sh ? sh + g * lsz : sh, bar, xch}, ch);
  });
  return I2C_OK;
}
#else
// THE set-up of a quad kernel, from the constants into LDS to the finished Quad<R>: a macro in the style of I2C_KERNEL -- the statements
// are the kernel's own, so `kc` and `sh` are its __shared__ objects and `l`, `wv`, `g`, `b`, `live`, `q` its constants. A kernel reads
//   { I2C_QUAD_SETUP(waves per workgroup, LDS elements per trajectory, FORWARD, type of the constants); its_body(c, kc, a, b, live, q); }
// `kc` is filled from the kernel-argument segment by the whole workgroup; lane l serves slot g = (l >> 2) & 3 of its wave's four
// trajectories; a wave without a trajectory leaves the kernel (wave-uniform); the slots behind the batch's end run on its last
// trajectory with live = false. FORWARD: k_quad_forward, which alone has the single-wave workgroup experiment (-DI2C_QUAD_WPB=1: XCD
// placement) and the two diagnostic builds. I2C_QUAD_LANE is the part without constants and LDS (the compose pass).
template <int WPB, bool FORWARD> __device__ __forceinline__ long quad_first_traj(const int wv) {
  if constexpr (FORWARD && WPB == 1) return xcd_first_traj(blockIdx.x);
  // the waves of a workgroup take consecutive groups of four trajectories: one 128-byte line of a [B]-contiguous row (the d = 16
  // backward sweep has trajectory-major buffers: nothing is shared between its waves)
  else return 4L * ((long)blockIdx.x * WPB + wv);
}
#ifdef I2C_QUAD_PLACEMENT  // (diagnostic build, never shipped: where the dispatcher put this wave -- tools/placement_summary.py)
#define I2C_QUAD_PLACEMENT_PRINT(FORWARD)                                                                                      \
  if (FORWARD && l == 0)                                                                                                       \
    printf("placement %u %d %u %u\n", blockIdx.x, b0 < c.B ? 1 : 0, (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4),       \
           (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20));
#else
#define I2C_QUAD_PLACEMENT_PRINT(FORWARD)
#endif
#ifdef I2C_QF_NOSTORE  // (experiment, never shipped: the sweep without its stores -- how much of it is the store path)
constexpr bool QF_NOSTORE = true;
#else
constexpr bool QF_NOSTORE = false;
#endif
#define I2C_QUAD_LANE(WPB_, LDS, FORWARD)                                                                  \
  const int l = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6), g = (l >> 2) & 3;                  \
  const long b0 = quad_first_traj<WPB_, FORWARD>(wv);                                                      \
  I2C_QUAD_PLACEMENT_PRINT(FORWARD)                                                                        \
  if (b0 >= c.B) return; /* (wave-uniform: no trajectory in this wave) */                                  \
  const bool live = (FORWARD && QF_NOSTORE) ? false : b0 + g < c.B;                                        \
  const int b = (int)(b0 + g < c.B ? b0 + g : c.B - 1);                                                    \
  const Quad<R> q{l, l >> 4, g, l & 3, LDS};
#define I2C_QUAD_SETUP(WPB_, LSZ_, FORWARD, ...)                                                           \
  constexpr int WPB = WPB_, LSZ = LSZ_;                                                                    \
  __shared__ __VA_ARGS__ kc;                                                                               \
  __shared__ R sh[WPB * 4 * LSZ];                                                                          \
  quad_const_fill<M, R>(kc, kernarg_consts<M, R>(),                                                        \
                        std::is_same<__VA_ARGS__, QKConst<M, R>>::value ? kernarg_zeta<M, R>() : (const R*)nullptr, /* (its 2nd parameter) */ \
                        (int)threadIdx.x, 64 * WPB);                                                       \
  __syncthreads();                                                                                         \
  I2C_QUAD_LANE(WPB, (lds_ptr<R>)(sh + (wv * 4 + g) * LSZ), FORWARD)
// ... and its launch: a wave per four trajectories, WPB of them per workgroup (XCD: the single-wave placement grid), `rows` grid rows
template <int WPB, bool XCD = false, class K, class... A>
static int launch_quad(K kernel, const int B, const unsigned rows, void* stream, const A&... args) {
  const unsigned blocks = XCD ? xcd_blocks(B) : (unsigned)(((long)B + 4 * WPB - 1) / (4 * WPB));
  hipLaunchKernelGGL(kernel, dim3(blocks, rows), dim3(64 * WPB), 0, (hipStream_t)stream, args...);
  return hipGetLastError() == hipSuccess ? I2C_OK : I2C_ELAUNCH;
}
#endif
// Which instantiation of a quad kernel serves a problem: f(GENERAL, LEANQ) with the two as std::bool_constant. GENERAL: cubature weights
// with lam != 0, for the models that have the variant (quad_general_exists; Impl::quad_supported has checked) -- I2C_ENOTSUP for the
// others; unit weights (lam = 0, every shipped config) run the plain one. LEANQ: no optional output asked for, in the kernels that
// have a lean variant (HAS_LEAN; the others are only ever instantiated with LEANQ = false).
template <class M, bool HAS_LEAN, class F> static int quad_variant(const bool unit, const bool lean, const F& f) {
  if (!unit) {
    if constexpr (quad_general_exists<M>()) {
      if constexpr (HAS_LEAN) {
        if (lean) return f(std::true_type{}, std::true_type{});
      }
      return f(std::true_type{}, std::false_type{});
    } else {
      return I2C_ENOTSUP;
    }
  }
  if constexpr (HAS_LEAN) {
    if (lean) return f(std::false_type{}, std::true_type{});
  }
  return f(std::false_type{}, std::false_type{});
}

// the quad forward sweep (forward_quad_body)
#ifndef I2C_HOST_SIM
#ifndef I2C_QF_ATTR  // (experiment knob: extra attributes of the quad forward kernel, e.g. __attribute__((amdgpu_waves_per_eu(1, 1))))
#define I2C_QF_ATTR
#endif
template <class M, typename R, typename S, class A, bool GENERAL = false>
__global__ __launch_bounds__(64 * quad_waves_per_block<M>(), 2) I2C_QF_ATTR void k_quad_forward(const Consts<M, R> c, const A a) {
  I2C_QUAD_SETUP(quad_waves_per_block<M>(), QG<M>::SIZE, true, QConst<M, R>)
  forward_quad_body<M, R, S, GENERAL>(c, kc, a, b, live, q);
}
#endif
template <class M, typename R, typename S, class A>
static int launch_quad_forward(const Consts<M, R>& c, const A& a, void* stream) {
  return quad_variant<M, false>(unit_rule(c), false, [&](auto general, auto) {
    constexpr bool GENERAL = decltype(general)::value;
#ifdef I2C_HOST_SIM
    return sim_quad<QConst<M, R>>(c, (const R*)nullptr, QG<M>::SIZE, 0, [&](const auto& kc, const int b, const bool live, const Quad<R>& q, int) {
      forward_quad_body<M, R, S, GENERAL>(c, kc, a, b, live, q);
    });
#else
    constexpr int WPB = quad_waves_per_block<M>();
    return launch_quad<WPB, WPB == 1>(k_quad_forward<M, R, S, A, GENERAL>, c.B, 1u, stream, c, a);
#endif
  });
}

// the quad backward sweep: d = 16 models with identity observations (backward_quad_body, trajectory-major buffers), and -- round 6 --
// every model of the d <= 8 geometry (backward_quad8_body: sigma-point observations, actions that share a block with states)
template <class M> constexpr bool quad_backward_exists() {
  if constexpr (!QG<M>::WIDE) return quad_backward8_exists<M>();
  else
    return M::NX % 4 == 0 && (M::NX + M::NU) % 4 == 0 && M::NU <= 4 && M::NZ == M::NX + M::NU && st_identity<ObsStruct<M>, M::NZ>() &&
           (M::NZT == 0 || (M::NZT == M::NX && st_identity<TermStruct<M>, M::NZT>()));
}
// LDS region of one trajectory: the staged cell block of the d = 16 form, the sigma-point geometry of the d <= 8 one
template <class M> constexpr int quad_backward_lds() { return QG<M>::WIDE ? QBG<M>::SIZE : QG<M>::SIZE; }
template <class M, typename R, typename S, bool GENERAL, bool LEANQ, class KC, class A>
I2C_FN void quad_backward_dispatch(const Consts<M, R>& c, const KC& kc, const A& a, const int b, const bool live, const Quad<R>& q) {
  if constexpr (QG<M>::WIDE) backward_quad_body<M, R, S, GENERAL>(c, kc, a, b, live, q);
  else backward_quad8_body<M, R, S, GENERAL, LEANQ>(c, kc, a, b, live, q);
}
#ifndef I2C_HOST_SIM
template <class M, typename R, typename S, class A, bool GENERAL = false, bool LEANQ = false>
__global__ __launch_bounds__(64 * QB_WAVES_PER_BLOCK, 2) void k_quad_backward(const Consts<M, R> c, const A a) {
  I2C_QUAD_SETUP(QB_WAVES_PER_BLOCK, quad_backward_lds<M>(), false, QBConst<M, R>)
  quad_backward_dispatch<M, R, S, GENERAL, LEANQ>(c, kc, a, b, live, q);
}
#endif
// d <= 8: the lean variant when no optional output is asked for
template <class M, typename R, typename S, class A>
static int launch_quad_backward(const Consts<M, R>& c, const A& a, void* stream) {
  return quad_variant<M, !QG<M>::WIDE>(unit_rule(c), !a.xm && !a.zpost && !a.cell_stats, [&](auto general, auto leanq) {
    constexpr bool GENERAL = decltype(general)::value, LEANQ = decltype(leanq)::value;
#ifdef I2C_HOST_SIM
    return sim_quad<QBConst<M, R>>(c, (const R*)nullptr, quad_backward_lds<M>(), 0, [&](const auto& kc, const int b, const bool live, const Quad<R>& q, int) {
      quad_backward_dispatch<M, R, S, GENERAL, LEANQ>(c, kc, a, b, live, q);
    });
#else
    return launch_quad<QB_WAVES_PER_BLOCK>(k_quad_backward<M, R, S, A, GENERAL, LEANQ>, c.B, 1u, stream, c, a);
#endif
  });
}

// the chunked schedule in the quad form (d <= 8): the WALKER (backward_quad8_body<QB8_CHUNK_WALK>: grid = groups of four trajectories x
// chunks), the COMPOSE and the STITCH pass (compose_quad8_body, backward_quad8_body<QB8_STITCH>)
template <class M, typename R, typename S> I2C_FN QChunk<R> quad_chunk_of(const Consts<M, R>& c, const ChunkArgs<R, S>& a, const int ch) {
  const int t_lo = ch * a.chunk_len, t_hi = (t_lo + a.chunk_len < c.T) ? t_lo + a.chunk_len : c.T;
  return QChunk<R>{a.bnd, a.part, ch, t_lo, t_hi, a.comp, a.n_chunks};
}
#ifndef I2C_HOST_SIM
template <class M, typename R, typename S>
__global__ __launch_bounds__(64 * QB_WAVES_PER_BLOCK, 2) void k_quad_chunk_compose(const Consts<M, R> c, const ChunkArgs<R, S> a) {
  I2C_QUAD_LANE(QB_WAVES_PER_BLOCK, (lds_ptr<R>)nullptr, false)
  const QChunk<R> qc = quad_chunk_of<M, R, S>(c, a, (int)blockIdx.y);
  compose_quad8_body<M, R, S>(c, a.cell.fwd, a.comp, qc.ch, qc.t_lo, qc.t_hi, b, live, q);
}
template <class M, typename R, typename S, bool GENERAL = false>
__global__ __launch_bounds__(64 * QB_WAVES_PER_BLOCK, 2) void k_quad_chunk_stitch(const Consts<M, R> c, const ChunkArgs<R, S> a) {
  I2C_QUAD_SETUP(QB_WAVES_PER_BLOCK, quad_backward_lds<M>(), false, QBConst<M, R>)
  backward_quad8_body<M, R, S, GENERAL, true, QB8_STITCH>(c, kc, a.cell, b, live, q, QChunk<R>{a.bnd, a.part, 0, 0, c.T, a.comp, a.n_chunks});
}
template <class M, typename R, typename S, bool GENERAL = false, bool LEANQ = false>
__global__ __launch_bounds__(64 * QB_WAVES_PER_BLOCK, 2) void k_quad_chunk_walk(const Consts<M, R> c, const ChunkArgs<R, S> a) {
  I2C_QUAD_SETUP(QB_WAVES_PER_BLOCK, quad_backward_lds<M>(), false, QBConst<M, R>)
  backward_quad8_body<M, R, S, GENERAL, LEANQ, QB8_CHUNK_WALK>(c, kc, a.cell, b, live, q, quad_chunk_of<M, R, S>(c, a, (int)blockIdx.y));
}
#endif
template <class M, typename R, typename S>
static int launch_quad_chunk_compose(const Consts<M, R>& c, const ChunkArgs<R, S>& a, void* stream) {
  if constexpr (!QG<M>::WIDE) {
#ifdef I2C_HOST_SIM
    return sim_quad<NoConst>(c, (const R*)nullptr, 0, a.n_chunks, [&](const NoConst&, const int b, const bool live, const Quad<R>& q, const int ch) {
      const QChunk<R> qc = quad_chunk_of<M, R, S>(c, a, ch);
      compose_quad8_body<M, R, S>(c, a.cell.fwd, a.comp, ch, qc.t_lo, qc.t_hi, b, live, q);
    });
#else
    return launch_quad<QB_WAVES_PER_BLOCK>(k_quad_chunk_compose<M, R, S>, c.B, (unsigned)a.n_chunks, stream, c, a);
#endif
  }
  return I2C_ENOTSUP;
}
template <class M, typename R, typename S>
static int launch_quad_chunk_stitch(const Consts<M, R>& c, const ChunkArgs<R, S>& a, void* stream) {
  if constexpr (!QG<M>::WIDE) {
    return quad_variant<M, false>(unit_rule(c), false, [&](auto general, auto) {
      constexpr bool GENERAL = decltype(general)::value;
#ifdef I2C_HOST_SIM
      return sim_quad<QBConst<M, R>>(c, (const R*)nullptr, quad_backward_lds<M>(), 0, [&](const auto& kc, const int b, const bool live, const Quad<R>& q, int) {
        backward_quad8_body<M, R, S, GENERAL, true, QB8_STITCH>(c, kc, a.cell, b, live, q, quad_chunk_of<M, R, S>(c, a, 0));
      });
#else
      return launch_quad<QB_WAVES_PER_BLOCK>(k_quad_chunk_stitch<M, R, S, GENERAL>, c.B, 1u, stream, c, a);
#endif
    });
  }
  return I2C_ENOTSUP;
}
template <class M, typename R, typename S>
static int launch_quad_chunk_walk(const Consts<M, R>& c, const ChunkArgs<R, S>& a, void* stream) {
  if constexpr (!QG<M>::WIDE) {
    return quad_variant<M, true>(unit_rule(c), !a.cell.xm && !a.cell.zpost && !a.cell.cell_stats, [&](auto general, auto leanq) {
      constexpr bool GENERAL = decltype(general)::value, LEANQ = decltype(leanq)::value;
#ifdef I2C_HOST_SIM
      return sim_quad<QBConst<M, R>>(c, (const R*)nullptr, quad_backward_lds<M>(), a.n_chunks, [&](const auto& kc, const int b, const bool live, const Quad<R>& q, const int ch) {
        backward_quad8_body<M, R, S, GENERAL, LEANQ, QB8_CHUNK_WALK>(c, kc, a.cell, b, live, q, quad_chunk_of<M, R, S>(c, a, ch));
      });
#else
      return launch_quad<QB_WAVES_PER_BLOCK>(k_quad_chunk_walk<M, R, S, GENERAL, LEANQ>, c.B, (unsigned)a.n_chunks, stream, c, a);
#endif
    });
  }
  return I2C_ENOTSUP;
}

// the quad propagation (propagate_quad_body): d = 16 models with identity observations
#ifndef I2C_HOST_SIM
template <class M, typename R, bool GENERAL = false>
__global__ __launch_bounds__(64 * quad_waves_per_block<M>(), 2) void k_quad_propagate(const Consts<M, R> c, const PropArgs<R> a) {
  I2C_QUAD_SETUP(quad_waves_per_block<M>(), QG<M>::SIZE, false, QPConst<M, R>)
  propagate_quad_body<M, R, GENERAL>(c, kc, a, b, live, q);
}
#endif
// unit weights, or (round 6) the GENERAL variant: any CubatureQuadrature(alpha, beta, kappa)
template <class M, typename R>
static int launch_quad_propagate(const Consts<M, R>& c, const PropArgs<R>& a, void* stream) {
  return quad_variant<M, false>(unit_rule(c.rule_xu), false, [&](auto general, auto) {
    constexpr bool GENERAL = decltype(general)::value;
#ifdef I2C_HOST_SIM
    return sim_quad<QPConst<M, R>>(c, (const R*)nullptr, QG<M>::SIZE, 0, [&](const auto& kc, const int b, const bool live, const Quad<R>& q, int) {
      propagate_quad_body<M, R, GENERAL>(c, kc, a, b, live, q);
    });
#else
    return launch_quad<quad_waves_per_block<M>()>(k_quad_propagate<M, R, GENERAL>, c.B, 1u, stream, c, a);
#endif
  });
}

// the quad filter step (ckf_quad_body): d = 16 models
#ifndef I2C_HOST_SIM
template <class M, typename R>
__global__ __launch_bounds__(64 * quad_waves_per_block<M>(), 2) void k_quad_ckf(const Consts<M, R> c, const ZetaArg<M, R> zeta, const CkfArgs<R> a) {
  I2C_QUAD_SETUP(quad_waves_per_block<M>(), QG<M>::SIZE, false, QKConst<M, R>)  // (kc: with `zeta`, the second parameter)
  ckf_quad_body<M, R>(c, kc, a, b, live, q);
}
#endif
template <class M, typename R>
static int launch_quad_ckf(const Consts<M, R>& c, const ZetaArg<M, R>& zeta, const CkfArgs<R>& a, void* stream) {
#ifdef I2C_HOST_SIM
  return sim_quad<QKConst<M, R>>(c, zeta.v, QG<M>::SIZE, 0, [&](const auto& kc, const int b, const bool live, const Quad<R>& q, int) {
    ckf_quad_body<M, R>(c, kc, a, b, live, q);
  });
#else
  return launch_quad<quad_waves_per_block<M>()>(k_quad_ckf<M, R>, c.B, 1u, stream, c, zeta, a);
#endif
}

// ---- grid kernels (i2c_grid.hpp): one wavefront per trajectory runs the one-lane body, the Gauss-Hermite grid strided over its lanes ----
// Device: GRID_WAVES_PER_BLOCK trajectories per workgroup. Host simulation: grid_sim_team() runs the 64 lanes of a trajectory (no
// threads: see i2c_grid.hpp), one trajectory after the other.
template <int KIND, class M, typename R, class A>
static int launch_grid(const Consts<M, R>& c, const A& a, void* stream) {
#ifdef I2C_HOST_SIM
  std::unique_ptr<char[]> stacks(new char[64 * GridFibres::STACK]);
  std::vector<double> xch((size_t)64 * GridXch<M>::N);
  for (int b = 0; b < c.B; ++b) grid_sim_team(stacks.get(), xch.data(), [&] { grid_body<KIND, M, R>(c, a, b); });
  return I2C_OK;
#else
  const dim3 grid((unsigned)(((long)c.B + GRID_WAVES_PER_BLOCK - 1) / GRID_WAVES_PER_BLOCK)), block(64 * GRID_WAVES_PER_BLOCK);
  if constexpr (KIND == GRK_FORWARD) hipLaunchKernelGGL((k_grid_forward<M, R>), grid, block, 0, (hipStream_t)stream, c, a);
  if constexpr (KIND == GRK_BACKWARD) hipLaunchKernelGGL((k_grid_backward<M, R>), grid, block, 0, (hipStream_t)stream, c, a);
  if constexpr (KIND == GRK_PROPAGATE) hipLaunchKernelGGL((k_grid_propagate<M, R>), grid, block, 0, (hipStream_t)stream, c, a);
  return hipGetLastError() == hipSuccess ? I2C_OK : I2C_ELAUNCH;
#endif
}

template <int KIND, class M, typename R, typename S, class A>
static int launch_wave(const Consts<M, R>& c, const A& a, void* stream) {
  if constexpr (KIND == WK_FORWARD) {  // batches whose waves share a SIMD: the variant with the pivot blocks through LDS
    if (c.B > 1024 && c.inference != I2C_INF_LINEARIZE) return launch_wave_v<WK_FORWARD_PL, M, R, S, false>(c, a, stream);
  }
  if constexpr (sizeof(S) == sizeof(R) && M::NZT > 0 && (KIND == WK_FORWARD || KIND == WK_BACKWARD)) {
    // the Linearize variant: fp64 storage, models with a terminal observation, one backward schedule
    if (c.inference == I2C_INF_LINEARIZE) return launch_wave_v<KIND, M, R, S, true>(c, a, stream);
  }
  return launch_wave_v<KIND, M, R, S, false>(c, a, stream);
}

template <int KIND, class M, typename R, int G, class A>
static int launch_group(const Consts<M, R>& c, const ZetaArg<M, R>* zeta, const A& a, void* stream) {
  if constexpr (KIND == GK_BACKWARD || KIND == GK_PROPAGATE) {
    const bool fullw = !c.qr_diag || (KIND == GK_BACKWARD && c.has_Qf && !c.qf_diag);
    if (fullw) return launch_group_w<KIND, M, R, G, true>(c, zeta, a, stream);
  }
  if constexpr (KIND == GK_FORWARD) {  // the compile-time lean variant (forward_group_body)
    if (!c.z_per_cell && !a.alpha_cell && !a.prior_out && c.t0 == 0) return launch_group_w<KIND, M, R, G, true>(c, zeta, a, stream);
  }
  return launch_group_w<KIND, M, R, G, false>(c, zeta, a, stream);
}

template <typename R> static Rule<R> make_rule(const I2cProblem* p, int dim) {
  // CubatureQuadrature.weights, i2c/exp_types.py:40-49
  const double a = p->quad_alpha, lam = a * a * (dim + p->quad_kappa) - dim;
  const double wi = 1.0 / (2.0 * (dim + lam));
  const double w0 = 2.0 * lam * wi + (1.0 - a * a + p->quad_beta);
  const double W = w0 + 2.0 * dim * wi;
  Rule<R> r;
  r.sf = (R)std::sqrt(dim + lam);
  r.w0 = (R)w0;
  r.wi = (R)wi;
  r.unit = std::fabs(W - 1.0) < 1e-14;
  r.W = r.unit ? (R)1 : (R)W;
  r.gh_degree = 0;
  r.gh_points = 0;
  for (int q = 0; q < I2C_MAX_GH_DEGREE; ++q) r.gh_x[q] = r.gh_w[q] = (R)0;
  if (p->inference == I2C_INF_GAUSS_HERMITE) {  // GaussHermiteQuadrature.weights, i2c/exp_types.py:63-68
    r.sf = (R)std::sqrt(2.0);
    r.w0 = r.wi = (R)0;
    r.W = (R)1;
    r.unit = 1;
    r.gh_degree = p->gh_degree;
    long n = 1;
    for (int i = 0; i < dim; ++i) n *= p->gh_degree;
    r.gh_points = (int)n;
    for (int q = 0; q < p->gh_degree; ++q) {
      r.gh_x[q] = (R)p->gh_nodes[q];
      r.gh_w[q] = (R)(p->gh_weights[q] / std::sqrt(3.14159265358979323846));
    }
  }
  return r;
}

template <class M, typename R> static Consts<M, R> make_consts(const I2cProblem* p, double tol, int use_expert) {
  using C = Consts<M, R>;
  C c;
  std::memset(&c, 0, sizeof(c));
  c.B = p->B;
  c.T = p->T;
  c.t0 = p->t0;
  c.has_Qf = p->has_Qf && M::NZT > 0;
  c.has_x_terminal = p->has_x_terminal;
  c.z_per_cell = p->z_per_cell && p->z != nullptr;
  c.use_expert = use_expert;
  c.terminal_cell = p->terminal_cell;
  c.inference = p->inference;
  c.post_tm = (p->post_layout == 1 && M::WAVE) ? 1 : 0;
  auto is_diag = [](const double* W, int n) {
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < i; ++j)
        if (W[i * (i + 1) / 2 + j] != 0.0) return 0;
    return 1;
  };
  c.qr_diag = is_diag(p->QR, C::NZ);
  c.qf_diag = is_diag(p->Qf, C::NZT);
  c.rule_xu = make_rule<R>(p, C::D);
  c.rule_x = make_rule<R>(p, C::NX);
  c.dtemp = (R)p->dtemp;
  c.tol = (R)tol;
  for (int i = 0; i < sym(C::NX); ++i) c.sig_eta[i] = (R)p->sig_eta[i];
  for (int i = 0; i < sym(C::NX); ++i) c.sig_eta_w[i] = c.rule_xu.W * c.sig_eta[i];
  for (int i = 0; i < sym(C::NZ); ++i) c.sig_xi0[i] = (R)p->sig_xi0[i];
  for (int i = 0; i < sym(C::NZ); ++i) c.QR[i] = (R)p->QR[i];
  for (int i = 0; i < sym(C::NZT); ++i) c.sig_xiT0[i] = (R)p->sig_xiT0[i];
  for (int i = 0; i < sym(C::NZT); ++i) c.Qf[i] = (R)p->Qf[i];
  for (int i = 0; i < C::NZ; ++i) c.zg[i] = (R)p->zg[i];
  for (int i = 0; i < C::NZT; ++i) c.zg_term[i] = (R)p->zg_term[i];
  for (int i = 0; i < C::NX; ++i) c.mu_x_term[i] = (R)p->mu_x_term[i];
  for (int i = 0; i < sym(C::NX); ++i) c.sig_x_term[i] = (R)p->sig_x_term[i];
  for (int i = 0; i < M::NP; ++i) c.params[i] = (R)p->model_params[i];
  if constexpr (is_per_traj<M>::value) c.params_b = (const R*)p->model_params_b;
  return c;
}

// Chunk geometry of the chunked backward sweep: enough chunks to put ~64K lanes in flight, at least 4
// cells per chunk, at most 32 chunks.
static void chunk_geometry(int B, int T, int* n_chunks, int* chunk_len) {
  static const int forced = [] {  // experiment knob (not part of the ABI)
    const char* e = getenv("I2C_CHUNKS");
    return e ? atoi(e) : 0;
  }();
  int nc = (65536 + B - 1) / B;
  if (nc > 32) nc = 32;
  if (nc > T / 4) nc = T / 4;
  if (forced > 0) nc = forced < T ? forced : T;  // (the knob overrides the caps: tools/r6_chunk_sweep.sh)
  if (nc < 1) nc = 1;
  const int len = (T + nc - 1) / nc;
  *chunk_len = len;
  *n_chunks = (T + len - 1) / len;
}
// Experiment knob (not part of the ABI), read once on EVERY library call (Impl::launches): I2C_CHUNK_PASSES=4 runs the chunked schedule
// as its four passes compose -> stitch -> walk -> reduce wherever the two-launch form (self-stitching walker, deferred reduction)
// would run: the reference of that form's tests and of its A/B timing.
static bool chunk_four_passes() {
  const char* e = getenv("I2C_CHUNK_PASSES");
  return e && atoi(e) == 4;
}
// Diagnostic knob (not part of the ABI), read where it reports: I2C_TRACE_PLAN=1 writes to stderr what a call dispatches beyond what
// the plan's exports report -- at the launch of a lane forward sweep "i2c_forward_lane: sweep=<helper|plain> lean=<0|1>
// gain=<helper|sweep>" (the compile-time variant of the sweep, and which wave solves the smoother gains), in the chunked schedule
// "i2c_backward_chunked: compose=<skipped|launched> walk=<self|plain> lean=<0|1>" (the walker and its variant).
// tests/test_forward_helper.py reads them -- the helper wave's composites and a compose launch's are the same bytes in the same
// place --, tests/test_learn_general_variants.py that the general variants ran, tests/test_forward_gain_helper.py who solved the gains.
static bool plan_trace() {
  const char* e = getenv("I2C_TRACE_PLAN");
  return e && atoi(e) == 1;
}
// The workspace of the chunked schedules (I2cProblem.work), as element offsets: the composite maps [NC][NX + NX*NX + sym(NX)][B] at 0,
// behind them the smoothed states entering the chunks [NC][NX + sym(NX)][B] and the per-chunk cost sums [NC][3][B]
template <class M> struct ChunkWork {
  size_t bnd, part, total;
  ChunkWork(const int B, const int n_chunks) {
    constexpr int NX = M::NX;
    const size_t n = (size_t)n_chunks * (size_t)B;
    bnd = n * (NX + NX * NX + sym(NX));
    part = bnd + n * (NX + sym(NX));
    total = part + n * 3;  // (3: the Linearize form's partial sums)
  }
};
template <class M> static size_t workspace_elems(int B, int T) {
  int nc, len;
  chunk_geometry(B, T, &nc, &len);
  return ChunkWork<M>(B, nc).total;
}
// the arguments of a chunked schedule's passes: the geometry of this batch and its workspace carved
template <class M, typename R, typename S> static ChunkArgs<R, S> chunk_args(const I2cProblem* p, const CellArgs<R, S>& a) {
  ChunkArgs<R, S> ch{a, (R*)p->work, nullptr, nullptr, 0, 0};
  chunk_geometry(p->B, p->T, &ch.n_chunks, &ch.chunk_len);
  const ChunkWork<M> w(p->B, ch.n_chunks);
  ch.bnd = ch.comp + w.bnd;
  ch.part = ch.comp + w.part;
  return ch;
}

// ONE detection helper for the batch sizes a model may set for itself (measured per model, i2c_models.hpp): name<M>::value is M::MEMBER
// where the model declares it, DEFAULT otherwise
#define I2C_MODEL_CONST(name, MEMBER, DEFAULT)                                                                      \
  template <class M, class = void> struct name : std::integral_constant<int, (DEFAULT)> {};                         \
  template <class M> struct name<M, std::void_t<decltype(M::MEMBER)>> : std::integral_constant<int, M::MEMBER> {};
// batch size from which I2C_BWD_AUTO runs the fused walk: the model's own measured crossover, or the library-wide default
I2C_MODEL_CONST(bwd_fused_min_b, BWD_FUSED_MIN_B, I2C_BWD_FUSED_MIN_B)
// batch size from which the forward sweep of i2c_learn composes the chunks on a helper wave (Impl::launches); see
// ModelDefaults (i2c_models.hpp) for the measurement behind the default
I2C_MODEL_CONST(forward_helper_min_b, FORWARD_HELPER_MIN_B, 4096)
// does that helper wave also solve the smoother gains by default (Launches::helper_gain)? Measured (profiles/forward_gain_helper_ab.txt):
// the pendulum (d = 3) gains 10 us per iteration at B = 4096, the cartpole (d = 5: the helper re-factors a 5 x 5 matrix per cell
// and the sweep waits for it) loses 14 us there and 57 us at B = 8192; d = 4 is not measured and stays off
I2C_MODEL_CONST(forward_helper_gain, FORWARD_HELPER_GAIN, M::NX + M::NU <= 3)
// batch window in which the d <= 8 quad backward sweep is the model's DEFAULT; models without the pair: on request only
I2C_MODEL_CONST(quad_backward_min_b, QUAD_BACKWARD8_MIN_B, 0)
I2C_MODEL_CONST(quad_backward_max_b, QUAD_BACKWARD8_MAX_B, -1)
// batch window in which the chunked schedule's WALK pass runs on the quad walker by default (backward_quad8_body<CHUNK>); models
// without the pair: on request only (group_lanes = 64 + "chunked")
I2C_MODEL_CONST(quad_chunk_walk_min_b, QUAD_CHUNK_WALK_MIN_B, 0)
I2C_MODEL_CONST(quad_chunk_walk_max_b, QUAD_CHUNK_WALK_MAX_B, -1)
// batch window in which the COMPOSE and STITCH passes of the chunked schedule run in the quad form by default (compose_quad8_body,
// backward_quad8_body<QB8_STITCH>); whatever walker follows
I2C_MODEL_CONST(quad_chunk_passes_min_b, QUAD_CHUNK_PASSES_MIN_B, 0)
I2C_MODEL_CONST(quad_chunk_passes_max_b, QUAD_CHUNK_PASSES_MAX_B, -1)
// ... and the batch size up to which the STITCH pass alone stays in the quad form
I2C_MODEL_CONST(quad_chunk_stitch_max_b, QUAD_CHUNK_STITCH_MAX_B, -1)
#undef I2C_MODEL_CONST

// ---- per-(model, dtype) entry points ------------------------------------------------------
// Which kernels a model has (i2c_models.hpp):
//   M::GROUP      lanes per trajectory of the model's group kernels (0: none compiled); fp64 only
//   M::WAVE       the wave kernels (i2c_wave.hpp: one wavefront per trajectory, d = 16) exist for this model
//   M::QUAD       the quad kernels (i2c_quad.hpp: four trajectories per wavefront) exist for this model
//   M::GROUP_ONLY the one-lane-per-trajectory kernels are NOT compiled for this model (d = nx + nu > 8 does not fit one
//                 lane's registers): every call runs the wave, quad or group kernels
//   S             storage type of the per-cell buffers: R, or float with R = double (I2C_F64_F32S: the cubature EM path of the
//                 one-lane, the quad and the wave kernels -- forward, backward, M-step, i2c_learn; everything else is I2C_ENOTSUP)
// Which of them serve a problem is decided ONCE per library call: Impl::resolve(problem) -> Plan. It reads I2cProblem.group_lanes
// (0: the model's default; -1: one lane per trajectory; G = M::GROUP: the group kernels; 64: the wave kernels, the quad kernels of a
// model without them, the grid kernels under I2C_INF_GAUSS_HERMITE; I2C_LANES_QUAD; anything else: I2C_ENOTSUP) as a Request, then
// walks one ordered rule list per sweep (forward_family, backward_family, propagate_family, filter_family), then the backward schedule
// and the passes of the chunked one. The two exports report from the plan (family_of, plan); the launchers (run_forward, run_backward,
// backward_chunked, run_propagate, run_ckf) read the plan and the call's Launches, never the request fields or a knob.

// What a problem resolves to: families are I2C_FAMILY_* or the negative error code the sweep returns
struct Plan {
  int forward, backward, propagate, filter;
  int schedule;   // I2C_BWD_* as i2c_backward_schedule reports it: the workspace of a chunked answer is assumed (Impl::schedule_with)
  int walker;     // schedule == I2C_BWD_CHUNKED: the family of the walk pass (lane or quad)
  int compose, stitch;  // ... and of the compose and stitch passes, as I2C_SWEEP_CHUNK_PASSES / _STITCH report them (sigma-point rule only)
  int rule;       // the rule variant of the lane bodies: I2C_INF_CUBATURE, _LINEARIZE or _GAUSS_HERMITE
  bool fwd_tm;    // the quad forward sweep writes its messages where a wave / quad backward sweep reads them (Consts::fwd_tm)
  bool fusable;   // i2c_learn_propagate: a forward sweep and the previous propagation may share a launch (k_forward_propagate)
};
// What a forward + backward pair of ONE library call launches beyond what the plan says: Impl::launches, at the top of every entry
// point that runs one, from the plan, the constants, the optional buffers that are present and the knobs. The launchers read it.
struct Launches {
  const int schedule;      // the backward schedule that RUNS: the plan's, or its fall-back without a workspace (Impl::schedule_with)
  const bool self_stitch;  // chunked: the walkers compute their boundary states themselves -- two launches, no stitch pass
  const bool helper;       // i2c_learn: the lane forward sweep composes the chunks on a helper wave, the chunked schedule starts with its walk
  const bool helper_gain;  // ... and the helper wave finishes the smoother gains, which the sweep only hands over (fp64-stored messages)
  const bool defer;        // i2c_learn: the next forward sweep finishes the reduction and the M-step of every iteration but the call's last
  const bool reduces;      // the backward sweep ends in a reduction kernel (or defers it): the M-step of an iteration rides on that
  const bool walk_lean;    // the lane walkers, fused and chunked, write no optional output (see chunk_walk_body)
};

template <class M, typename R, typename S = R> struct Impl {
  using C = Consts<M, R>;
  static constexpr bool MIXED = sizeof(S) != sizeof(R);
  static constexpr int G = M::GROUP;
  // A model with the optional process_noise member (state-action-dependent process noise, i2c_cell.hpp) is served by the one-lane
  // kernels under the sigma-point rule and, for its forward sweep, by the d <= 8 quad kernels (whose backward passes read what the
  // forward sweep stored and need nothing): no other multi-lane family is instantiated for it, none is its default, and a request
  // for one, for Linearize() / Gauss-Hermite or for the Riccati messages is I2C_ENOTSUP (those forms of the term do not exist).
  static constexpr bool NOISE = has_process_noise<M, R>::value;
  static constexpr bool HAS_GROUP = G > 0 && sizeof(R) == 8 && !MIXED && !NOISE;
  static constexpr bool LANE = !M::GROUP_ONLY;  // one-lane-per-trajectory kernels exist
  static constexpr bool HAS_WAVE = M::WAVE && sizeof(R) == 8 && !NOISE;  // fp64 matrix instruction; the storage type S may be float
  static constexpr bool HAS_QUAD = M::QUAD && sizeof(R) == 8 && !(NOISE && QG<M>::WIDE);  // fp64 matrix instruction (i2c_quad.hpp): forward sweep; the storage type S may be float
  static constexpr bool WIDE = QG<M>::WIDE;                    // the d = 16 form of the quad kernels
  static constexpr bool HAS_QUAD_BACKWARD = HAS_QUAD && quad_backward_exists<M>();  // ... and the backward sweep
  static constexpr bool QUAD8 = HAS_QUAD_BACKWARD && !WIDE && LANE;  // d <= 8: the fused quad walk, and the quad passes of the chunked schedule
  static constexpr bool HAS_QUAD_CKF = HAS_QUAD && !MIXED && quad_ckf_exists<M>();  // the filter step of the d = 16 form
  static constexpr bool HAS_QUAD_PROP = HAS_QUAD && !MIXED && quad_propagate_exists<M>();  // the closed-loop propagation of the d = 16 form
  static constexpr bool HAS_GRID = LANE && sizeof(R) == 8 && !MIXED && !NOISE;  // the grid kernels run the one-lane bodies: wherever those exist, fp64

  // ---- the resolver -------------------------------------------------------------------------------------------------------------
  // I2cProblem.group_lanes, normalised once against what the model has; nothing below reads the field again
  enum Request {
    REQ_DEFAULT,       // 0 (and 64 / I2C_LANES_QUAD where the kernels they name need fp64 arithmetic and R is float)
    REQ_ONE_LANE,      // -1: one lane per trajectory, no hybrid forward
    REQ_GROUP,         // G
    REQ_WAVE,          // 64 on a model with wave kernels (M::WAVE implies d = 16: i2c_wave.hpp)
    REQ_QUAD,          // 64 on a model with quad kernels only, I2C_LANES_QUAD on a d = 16 model: every sweep the quad form has
    REQ_QUAD_FORWARD,  // I2C_LANES_QUAD on a d <= 8 model: the quad forward sweep; the other sweeps resolve as the default does
    REQ_GRID,          // 64 under I2C_INF_GAUSS_HERMITE: forward, backward, propagation on the grid kernels
    REQ_NOT_OURS       // a width this model does not have
  };
  static Request request(const int lanes, const int inference) {
    if (lanes == 0) return REQ_DEFAULT;
    if (lanes == -1) return REQ_ONE_LANE;
    if constexpr (NOISE) {  // the quad kernels by either name, nothing else
      if (HAS_QUAD && (lanes == 64 || lanes == I2C_LANES_QUAD)) return lanes == 64 ? REQ_QUAD : REQ_QUAD_FORWARD;
      return REQ_NOT_OURS;
    }
    if (lanes == 64 && HAS_GRID && inference == I2C_INF_GAUSS_HERMITE) return REQ_GRID;
    if (lanes == 64 && (M::WAVE || M::QUAD)) return HAS_WAVE ? REQ_WAVE : (HAS_QUAD ? REQ_QUAD : REQ_DEFAULT);
    if (lanes == I2C_LANES_QUAD) return HAS_QUAD ? (WIDE ? REQ_QUAD : REQ_QUAD_FORWARD) : REQ_DEFAULT;
    return (HAS_GROUP && lanes == G) ? REQ_GROUP : REQ_NOT_OURS;
  }
  // the requests under which the sweeps that only have a one-lane form run (the Riccati messages): everything but a width the model
  // has group kernels for or does not have at all (I2C_LANES_QUAD names nothing on a model without quad kernels)
  static bool lane_request(const int lanes) {
    return lanes == 0 || lanes == -1 || (lanes == 64 && (M::WAVE || M::QUAD)) || (lanes == I2C_LANES_QUAD && M::QUAD);
  }
  // requests that leave the family open: a sweep the named kernels do not have runs what the model runs by default
  static bool family_open(const Request r) { return r == REQ_DEFAULT || r == REQ_WAVE || r == REQ_QUAD || r == REQ_QUAD_FORWARD; }
  static bool by_default(const Request r) { return r == REQ_DEFAULT || r == REQ_QUAD_FORWARD; }  // (of the sweeps behind the forward one)

  // per-cell targets [T][NZ][B] and temperatures [T][B] are addressed through 32-bit byte offsets of one buffer window by the
  // group, wave and quad kernels: beyond 4 GiB the offset would wrap and read the wrong cell (round-3 advice)
  static int window_32bit_ok(const I2cProblem* p) {
    if (p->z_per_cell && p->z && (long)p->T * C::NZ * (long)p->B * (long)sizeof(R) >= (1L << 32)) return I2C_EINVAL;
    if (p->alpha_cell && (long)p->T * (long)p->B * (long)sizeof(R) >= (1L << 32)) return I2C_EINVAL;
    return I2C_OK;
  }
  // a per-cell block of `elems` elements of `size` bytes stays inside the 2 GiB the predicated stores park their masked-off lanes behind
  static bool below_2gib(const long elems, const I2cProblem* p, const size_t size) { return elems * (long)p->B * (long)size < (1L << 31); }
  static constexpr long E_SWEEPS = C::E_FWD > C::E_POST ? C::E_FWD : C::E_POST;                   // forward messages, posterior
  static constexpr long E_CLOSED = C::E_POST > C::E_PROP ? C::E_POST : C::E_PROP;                 // posterior, propagation
  static constexpr long E_COMPOSITE = M::NX + M::NX * M::NX + sym(M::NX);                         // a chunk's composite map
  // what the group form does not cover: other inference rules (the state estimator's is the unit cubature rule whatever the graph
  // infers with; closed-loop propagation under Linearize() IS that rule: i2c.py:109-115); cells beyond 2 GiB (GIO::st_if)
  static int group_supported(const I2cProblem* p, const int sweep) {
    if (sweep != I2C_SWEEP_FILTER && p->inference != I2C_INF_CUBATURE && !(p->inference == I2C_INF_LINEARIZE && sweep == I2C_SWEEP_PROPAGATE))
      return I2C_ENOTSUP;
    if (!below_2gib(E_SWEEPS > C::E_PROP ? E_SWEEPS : C::E_PROP, p, sizeof(R))) return I2C_EINVAL;
    return window_32bit_ok(p);
  }
  // what the wave form covers: the cubature rule with lam = 0 (every shipped config: unit weights, no weight on the centre;
  // the centring of the pairwise sums relies on 2 d wi = 1), windows below 2 GiB (WIO::st_if)
  static int wave_supported(const I2cProblem* p, const bool unit) {
    if (p->inference == I2C_INF_LINEARIZE) {  // Linearize(): fp64 storage; needs a terminal observation like the lane form
      if (MIXED) return I2C_ENOTSUP;
      if (M::NZT == 0) return I2C_EINVAL;
    } else if (p->inference != I2C_INF_CUBATURE) {
      return I2C_ENOTSUP;
    }  // (a terminal state prior -- covariance control -- is the backward sweep's end of the chain: w_end_of_chain, round 4)
    if (!unit) return I2C_ENOTSUP;
    if (!below_2gib(E_SWEEPS, p, sizeof(S))) return I2C_EINVAL;
    return window_32bit_ok(p);
  }
  // what the quad form covers: the cubature rule with lam = 0 for every model (the d = 8 models evaluate no centre point at all); any
  // CubatureQuadrature(alpha, beta, kappa) for the models with the GENERAL variant (quad_general_exists, round 5); windows below 2 GiB
  static int quad_supported(const I2cProblem* p, const bool unit) {
    if (p->inference != I2C_INF_CUBATURE) return I2C_ENOTSUP;
    if (!quad_general_exists<M>() && !unit) return I2C_ENOTSUP;
    // the d = 16 form addresses trajectory-major buffers only: the posterior / prior in that layout (the engine's default for the
    // wave-capable models) and forward messages that the wave backward sweep reads
    if (WIDE && (p->post_layout != 1 || !HAS_WAVE)) return I2C_ENOTSUP;
    if (!below_2gib(E_SWEEPS, p, sizeof(S))) return I2C_EINVAL;
    return window_32bit_ok(p);
  }
  // the compose / stitch passes in the quad form: what the forward form covers, and composites (arithmetic-typed rows, which
  // quad_supported's storage-typed bound does not cover under fp32 storage) inside the 2 GiB window of a chunk
  static bool quad_passes_supported(const I2cProblem* p, const bool unit) {
    return QUAD8 && quad_supported(p, unit) == I2C_OK && below_2gib(E_COMPOSITE, p, sizeof(R));
  }
  // experiment knobs (not part of the ABI), read once per process: a batch size that overrides the model's window of the quad compose +
  // stitch passes / of the quad stitch pass alone; -2: not set
  static int env_knob(const char* name) {
    const char* e = getenv(name);
    return e ? atoi(e) : -2;
  }
  static int quad_passes_max_b_knob() {
    static const int v = env_knob("I2C_QUAD_PASSES_MAX_B");
    return v;
  }
  static int quad_stitch_max_b_knob() {
    static const int v = env_knob("I2C_QUAD_STITCH_MAX_B");
    return v;
  }

  // The batch rule of the lane kernels. Small batches: the sequential depth decides -> chunked. Large ones: HBM traffic decides ->
  // fused (the chunked form moves compose + stitch + walk = 1.44x the walk's bytes, PMC: pendulum 381 against 264.5 B per cell, double
  // cartpole 1 914 against 1 177). The crossover is PER MODEL (M::BWD_FUSED_MIN_B, i2c_models.hpp), re-derived in round 5 from time AND
  // traffic at B = 8192 .. 32768, beyond the 256 MB Infinity Cache (profiles/r5_backward_crossover.txt): pendulum 8192: chunked 0.111 /
  // fused 0.175 ms, 16384: 0.237 / 0.193 (cartpole 0.72 / 0.99, 1.38 / 1.01; planar quadrotor 0.21 / 0.27, 0.38 / 0.30); double
  // cartpole 16384: 1.67 / 1.86, 24576: 3.44 / 2.20. Models that only have group kernels run the fused walk.
  static int lane_schedule(const int B, const int T, const int requested) {
    // wave kernels: the fused walk, or on request the two-pass schedule (scan + one wave per (t, b) cell). Measured on MI355X
    // (12-state quadrotor, T = 50): the two-pass form is SLOWER at every batch -- B = 256: 0.179 against 0.162 ms, B = 1024:
    // 0.347 against 0.184 ms -- because with T times as many waves in flight the sweep is bound by the vector-memory
    // pipeline: a wave's load touches one 8-byte element in each of 64 different [B]-contiguous rows (64 cache lines per
    // instruction), which a lone wave per SIMD hides behind its dependent arithmetic and 50 waves per SIMD do not.
    if (M::WAVE && M::GROUP_ONLY) return requested == I2C_BWD_TWO_PASS ? I2C_BWD_TWO_PASS : I2C_BWD_FUSED;
    if (M::GROUP_ONLY) return I2C_BWD_FUSED;
    int mode = requested;
    if (mode == I2C_BWD_AUTO) mode = B < bwd_fused_min_b<M>::value ? I2C_BWD_CHUNKED : I2C_BWD_FUSED;
    if (mode == I2C_BWD_CHUNKED && T < 8) mode = I2C_BWD_TWO_PASS;  // too short to chunk
    return mode;
  }
  // d <= 8: is the quad walker the DEFAULT walk pass of this problem? (no backward request, the chunked schedule is the batch's default
  // and long enough to chunk, the batch inside the model's measured window)
  static bool quad_walker_default(const I2cProblem* p, const Request req) {
    return QUAD8 && by_default(req) && p->backward_mode == I2C_BWD_AUTO && p->inference == I2C_INF_CUBATURE &&
           p->B >= quad_chunk_walk_min_b<M>::value && p->B <= quad_chunk_walk_max_b<M>::value &&
           lane_schedule(p->B, p->T, I2C_BWD_AUTO) == I2C_BWD_CHUNKED;
  }

  // The tail of every sweep's list: the one-lane kernels, or the group kernels -- asked for, the only ones the model has, or (forward
  // sweep, nothing asked for) the hybrid default of the d >= 7 lane models while the batch leaves every group wave a SIMD of its own
  // (measured, planar quadrotor d = 8 at B = 4096: forward 0.51 -> 0.40 ms, while its chunked lane backward stays the faster one; the
  // buffers of the families are the same, so the backward schedules are unaffected).
  static int lane_or_group(const I2cProblem* p, const Request req, const int sweep) {
    if (req == REQ_NOT_OURS || (req == REQ_ONE_LANE && !LANE)) return I2C_ENOTSUP;
    if constexpr (MIXED) {  // fp64 arithmetic on fp32-stored messages: the cubature EM path
      const bool em = sweep == I2C_SWEEP_FORWARD || sweep == I2C_SWEEP_BACKWARD;
      return (LANE && em && p->inference == I2C_INF_CUBATURE) ? I2C_FAMILY_LANE : I2C_ENOTSUP;
    }
    bool group = req == REQ_GROUP || (family_open(req) && !LANE);
    if constexpr (HAS_GROUP && M::GROUP_FORWARD_AUTO) {
      if (!group && sweep == I2C_SWEEP_FORWARD && req == REQ_DEFAULT && (long)p->B * G <= I2C_GROUP_FORWARD_MAX_LANES &&
          group_supported(p, sweep) == I2C_OK)
        group = true;
    }
    if (group) {
      if constexpr (HAS_GROUP) {
        const int rc = group_supported(p, sweep);
        return rc != I2C_OK ? rc : I2C_FAMILY_GROUP;
      }
      return I2C_ENOTSUP;
    }
    return I2C_FAMILY_LANE;
  }
  // ... before it, for the forward and backward sweeps: the wave kernels, asked for or the model's default wherever they apply
  static int wave_lane_or_group(const I2cProblem* p, const Request req, const bool unit, const int sweep) {
    if constexpr (HAS_WAVE) {
      if (family_open(req)) {
        const int rc = wave_supported(p, unit);
        if (rc == I2C_OK) return I2C_FAMILY_WAVE;
        if (req == REQ_WAVE || MIXED) return rc;
      }
    }
    return lane_or_group(p, req, sweep);
  }
  // The quad forward sweep: asked for, or the model's default inside its batch window -- and for d = 16 with general cubature weights
  // at every batch size, since the wave kernels only have the unit rule. Asked for, its refusal is the answer.
  static int forward_family(const I2cProblem* p, const Request req, const bool unit) {
    if (req == REQ_GRID) return I2C_FAMILY_GRID;
    if constexpr (HAS_QUAD) {
      const bool asked = req == REQ_QUAD || req == REQ_QUAD_FORWARD;
      const bool general_wide = WIDE && quad_general_exists<M>() && !unit;
      if (asked || (req == REQ_DEFAULT && ((p->B >= M::QUAD_FORWARD_MIN_B && p->B <= M::QUAD_FORWARD_MAX_B) || general_wide))) {
        const int rc = quad_supported(p, unit);
        if (rc == I2C_OK) return I2C_FAMILY_QUAD;
        if (asked) return rc;
      }
    }
    return wave_lane_or_group(p, req, unit, I2C_SWEEP_FORWARD);
  }
  // The quad backward sweep. d = 16: the fused walk, with the forward sweep (from the larger of the two MIN_B on) -- an explicit two-pass
  // request keeps the wave form. d <= 8 (round 6), two forms of backward_quad8_body: (i) the fused walk of four trajectories per
  // wavefront, ONE pass over the forward messages: asked for (with the schedule left open or "fused"), or inside quad_backward_min_b ..
  // _max_b (no in-tree model has one); (ii) the WALKER of the chunked schedule: asked for (with "chunked"), or the default inside the
  // model's quad_chunk_walk_min_b .. _max_b where the chunked schedule is the batch's default (quad_walker_default). An explicit
  // "two_pass" is the lane kernels'.
  static int backward_family(const I2cProblem* p, const Request req, const bool unit) {
    if (req == REQ_GRID) return I2C_FAMILY_GRID;
    if constexpr (HAS_QUAD_BACKWARD) {
      const bool asked = req == REQ_QUAD;
      const bool general_wide = WIDE && quad_general_exists<M>() && !unit;
      bool mode_ok, in_window;
      if constexpr (WIDE) {
        mode_ok = p->backward_mode != I2C_BWD_TWO_PASS;
        in_window = p->B >= (M::QUAD_BACKWARD_MIN_B > M::QUAD_FORWARD_MIN_B ? M::QUAD_BACKWARD_MIN_B : M::QUAD_FORWARD_MIN_B) && p->B <= M::QUAD_FORWARD_MAX_B;
      } else {
        mode_ok = asked ? p->backward_mode != I2C_BWD_TWO_PASS : p->backward_mode == I2C_BWD_AUTO;
        in_window = (p->B >= quad_backward_min_b<M>::value && p->B <= quad_backward_max_b<M>::value) || quad_walker_default(p, req);
      }
      if (mode_ok && (asked || (by_default(req) && (in_window || general_wide)))) {
        const int rc = quad_supported(p, unit);
        if (rc == I2C_OK) return I2C_FAMILY_QUAD;
        if (asked) return rc;
      }
    }
    return wave_lane_or_group(p, req, unit, I2C_SWEEP_BACKWARD);
  }
  // The closed-loop propagation of a matrix-instruction graph: the quad form where it applies (unit cubature rule -- `unit_xu`: a
  // Linearize() graph propagates with it whatever the quad fields say --, trajectory-major posterior). The posterior / propagation
  // cells are addressed through 32-bit offsets of one window per cell, masked stores parked at 2 GiB: beyond it, refused.
  static int propagate_family(const I2cProblem* p, const Request req, const bool unit_xu) {
    if (req == REQ_GRID) return I2C_FAMILY_GRID;
    if constexpr (HAS_QUAD_PROP) {
      if (family_open(req) && p->inference != I2C_INF_GAUSS_HERMITE && p->post_layout == 1 && (unit_xu || quad_general_exists<M>()) &&
          window_32bit_ok(p) == I2C_OK)
        return below_2gib(E_CLOSED, p, sizeof(R)) ? I2C_FAMILY_QUAD : I2C_EINVAL;
    }
    return lane_or_group(p, req, I2C_SWEEP_PROPAGATE);
  }
  // The state estimator: the quad filter step of a matrix-instruction graph. `req`: the request read under the estimator's own rule
  static int filter_family(const I2cProblem* p, const Request req) {
    if (HAS_QUAD_CKF && family_open(req)) return I2C_FAMILY_QUAD;
    return lane_or_group(p, req, I2C_SWEEP_FILTER);
  }
  // The schedule of the backward sweep: the family that serves it, the inference rule, the storage type, then the batch rule of the
  // lane kernels
  static int backward_schedule(const I2cProblem* p, const Request req, const int fam) {
    if (fam < 0) return fam;
    const int lane_rule = lane_schedule(p->B, p->T, p->backward_mode);
    if (fam == I2C_FAMILY_WAVE)  // the fused walk; the two-pass form on request (cubature rule)
      return (lane_rule == I2C_BWD_TWO_PASS && p->inference == I2C_INF_CUBATURE) ? I2C_BWD_TWO_PASS : I2C_BWD_FUSED;
    // d <= 8 quad: the chunked schedule with the quad walker when asked for by name, or as the model's default
    if (QUAD8 && fam == I2C_FAMILY_QUAD && p->T >= 8 && (p->backward_mode == I2C_BWD_CHUNKED || quad_walker_default(p, req))) return I2C_BWD_CHUNKED;
    if (fam != I2C_FAMILY_LANE) return I2C_BWD_FUSED;  // four trajectories / a group of lanes / a wavefront walk T-1..0
    if (p->inference == I2C_INF_LINEARIZE && M::NZT == 0) return I2C_EINVAL;  // no terminal observation: the reference fails at i2c.py:500-501
    if (p->inference != I2C_INF_CUBATURE) return (!MIXED && lane_rule == I2C_BWD_CHUNKED) ? I2C_BWD_CHUNKED : I2C_BWD_FUSED;  // no two-pass form
    return lane_rule;
  }
  // The compose pass of the chunked sigma-point schedule in the quad form: with the quad walker asked for by name (group_lanes = 64 and
  // "chunked": the whole schedule on matrix instructions) or, by default, inside the model's quad_chunk_passes_min_b .. _max_b
  static bool quad_compose(const I2cProblem* p, const Request req, const bool unit) {
    if (!quad_passes_supported(p, unit)) return false;
    if (req == REQ_QUAD && p->backward_mode == I2C_BWD_CHUNKED) return true;
    const int knob = quad_passes_max_b_knob();
    const int min_b = knob > -2 ? 1 : quad_chunk_passes_min_b<M>::value, max_b = knob > -2 ? knob : quad_chunk_passes_max_b<M>::value;
    return by_default(req) && p->B >= min_b && p->B <= max_b;
  }
  // ... and the STITCH pass alone, beyond that window: a chain of NC dependent steps on B / 64 lane wavefronts whatever the batch --
  // 0.85 us per quad step against 1.6 - 2.5 us per lane step
  static bool quad_stitch_alone(const I2cProblem* p, const Request req, const bool unit) {
    const int knob = quad_stitch_max_b_knob();
    return by_default(req) && p->B <= (knob > -2 ? knob : quad_chunk_stitch_max_b<M>::value) && quad_passes_supported(p, unit);
  }

  // Per-trajectory horizons (I2cProblem.horizons): the HZ kernels exist for the one-lane bodies in fp64 under the sigma-point rule, for
  // models without process_noise; the forward, backward and propagate sweeps then resolve to I2C_FAMILY_LANE (group_lanes 0 and -1
  // alike: no default hands a sweep to another family) and the backward sweep to the fused walk, whatever schedule is asked for. What
  // those kernels do not cover is refused here, before any launch: I2C_ENOTSUP for what is not compiled, I2C_EINVAL for a problem whose
  // fields contradict a horizon per trajectory (a moved ring, per-cell temperatures -- both belong to the MPC loop --, a terminal cell
  // that is not "each trajectory's last one", T - 1, or none).
  static constexpr bool HAS_HORIZONS = LANE && sizeof(R) == 8 && !MIXED && !NOISE;
  static int horizons_supported(const I2cProblem* p) {
    if (!HAS_HORIZONS) return I2C_ENOTSUP;
    if (p->group_lanes != 0 && p->group_lanes != -1) return I2C_ENOTSUP;
    if (p->inference != I2C_INF_CUBATURE) return I2C_ENOTSUP;
    if (p->t0 != 0 || p->alpha_cell) return I2C_EINVAL;
    if (p->terminal_cell != p->T - 1 && p->terminal_cell != -1) return I2C_EINVAL;
    return I2C_OK;
  }

  // THE place that decides which kernel family and which backward schedule serve a problem (i2c_kernel_family() and
  // i2c_backward_schedule() report it; every entry point below dispatches from it)
  static Plan resolve(const I2cProblem* p) {
    const Rule<R> rule_xu = make_rule<R>(p, C::D), rule_x = make_rule<R>(p, C::NX);
    const bool unit_xu = unit_rule(rule_xu), unit = unit_xu && unit_rule(rule_x);
    const Request req = request(p->group_lanes, p->inference);
    Plan pl;
    pl.rule = p->inference;
    if (p->horizons) {  // per-trajectory horizons: the one-lane kernels and the fused walk, or the refusal (horizons_supported)
      const int rc = horizons_supported(p);
      pl.forward = pl.backward = pl.propagate = rc == I2C_OK ? I2C_FAMILY_LANE : rc;
      pl.filter = filter_family(p, req == REQ_GRID ? request(p->group_lanes, I2C_INF_CUBATURE) : req);  // (reads no horizon)
      pl.schedule = rc == I2C_OK ? I2C_BWD_FUSED : rc;
      pl.walker = I2C_ENOTSUP;
      pl.compose = pl.stitch = rc == I2C_OK ? I2C_ENOTSUP : rc;
      pl.fwd_tm = pl.fusable = false;
      return pl;
    }
    if constexpr (NOISE) {
      if (p->inference != I2C_INF_CUBATURE) {
        pl.forward = pl.backward = pl.propagate = pl.filter = pl.schedule = pl.walker = pl.compose = pl.stitch = I2C_ENOTSUP;
        pl.fwd_tm = pl.fusable = false;
        return pl;
      }
    }
    pl.forward = forward_family(p, req, unit);
    pl.backward = backward_family(p, req, unit);
    pl.propagate = propagate_family(p, req, unit_xu || p->inference == I2C_INF_LINEARIZE);
    // (the state estimator's rule is fixed, whatever the graph infers with -- CubatureQuadrature(1, 0, 0), mpc.py:121-123 --, so the
    //  filter step is no grid sweep: under a grid request it sees what 64 names under the cubature rule)
    pl.filter = filter_family(p, req == REQ_GRID ? request(p->group_lanes, I2C_INF_CUBATURE) : req);
    pl.schedule = backward_schedule(p, req, pl.backward);
    const bool chunked = pl.schedule == I2C_BWD_CHUNKED;
    pl.walker = chunked ? pl.backward : I2C_ENOTSUP;
    pl.compose = pl.stitch = pl.schedule < 0 ? pl.schedule : I2C_ENOTSUP;
    if (chunked && p->inference == I2C_INF_CUBATURE) {
      pl.compose = quad_compose(p, req, unit) ? I2C_FAMILY_QUAD : I2C_FAMILY_LANE;
      pl.stitch = (pl.compose == I2C_FAMILY_QUAD || quad_stitch_alone(p, req, unit)) ? I2C_FAMILY_QUAD : I2C_FAMILY_LANE;
    }
    // (the fp32-storage path has never set the flag)
    pl.fwd_tm = !MIXED && pl.forward == I2C_FAMILY_QUAD && ((M::WAVE && pl.backward == I2C_FAMILY_WAVE) || (HAS_QUAD_BACKWARD && pl.backward == I2C_FAMILY_QUAD));
    pl.fusable = !NOISE && LANE && C::D <= 5 && p->inference == I2C_INF_CUBATURE && pl.forward == I2C_FAMILY_LANE && pl.propagate == I2C_FAMILY_LANE &&
                 rule_xu.unit && rule_x.unit && !(p->z_per_cell && p->z) && !p->alpha_cell && p->t0 == 0;
    return pl;
  }
  static int plan(const I2cProblem* p) { return resolve(p).schedule; }
  static int family_of(const I2cProblem* p, const int sweep) {
    const Plan pl = resolve(p);
    const int of_sweep[] = {pl.forward, pl.backward, pl.propagate, pl.filter, pl.compose, pl.stitch};  // I2C_SWEEP_FORWARD .. _CHUNK_STITCH
    return of_sweep[sweep];
  }
  // the schedule that runs: a chunked answer without its workspace (I2cProblem.work) falls back to the two-pass form, or -- the quad
  // walker and the rules without a two-pass form -- to the fused walk
  static int schedule_with(const Plan& pl, const bool workspace) {
    if (pl.schedule != I2C_BWD_CHUNKED || workspace) return pl.schedule;
    return (pl.rule == I2C_INF_CUBATURE && pl.walker != I2C_FAMILY_QUAD) ? I2C_BWD_TWO_PASS : I2C_BWD_FUSED;
  }

  // ---- the constants of a call ---------------------------------------------------------------------------------------------------
  static I2cProblem with_unit_rule(const I2cProblem* p) {
    I2cProblem q = *p;
    q.quad_alpha = 1.0, q.quad_beta = 0.0, q.quad_kappa = 0.0;
    return q;
  }
  static C forward_consts(const I2cProblem* p) { return make_consts<M, R>(p, 0.0, p->inference == I2C_INF_LINEARIZE ? p->expert_controller : 0); }
  // under Linearize() the closed-loop propagation IS CubatureQuadrature(1, 0, 0) whatever the caller left in the quad fields (i2c.py:109-115)
  static C propagate_consts(const I2cProblem* p, const int use_expert) {
    if (p->inference != I2C_INF_LINEARIZE) return make_consts<M, R>(p, 0.0, use_expert);
    const I2cProblem q = with_unit_rule(p);
    return make_consts<M, R>(&q, 0.0, use_expert);
  }
  // ... and so is the state estimator's rule, whatever the graph infers with
  static C filter_consts(const I2cProblem* p) {
    I2cProblem q = with_unit_rule(p);
    q.inference = I2C_INF_CUBATURE;
    return make_consts<M, R>(&q, 0.0, 0);
  }

  // ---- what a call launches beyond its plan ---------------------------------------------------------------------------------------
  // The two-launch form of the chunked schedule (compose, self-stitching walk) and the forward sweep's helper wave exist for the d <= 5
  // lane models ...
  static constexpr bool SELF_STITCH = LANE && C::D <= 5;
  // ... and run where the chunked schedule runs under the sigma-point rule, for problems without a terminal state prior (whose end of
  // the chain advances temp[b]: once per trajectory, so not by several walkers). The walkers stitch themselves where the stitch and
  // walk passes are the lane kernels'. `in_learn` (i2c_learn alone: every forward sweep is followed by this plan's backward sweep): the
  // lane forward sweep composes the chunks on a second wave (k_forward_helper) where the compose pass is the lane kernels', 64 lanes to
  // a wave, from the batch size at which it pays (forward_helper_min_b: short chunks leave the helper no more time to compose a chunk
  // than the sweep takes to produce the next), and its M-step prologue (k_forward_mstep) takes the reduction behind such walkers.
  // Knobs (not part of the ABI), read HERE, once per library call -- the tests flip them inside one process: I2C_CHUNK_PASSES=4
  // (chunk_four_passes) brings back the four passes and the sweep without the helper; I2C_FORWARD_HELPER=0 that sweep and the compose
  // launch (the reference of tests/test_forward_helper.py and of the A/B timing), any other value the helper below forward_helper_min_b.
  static Launches launches(const I2cProblem* p, const Plan& pl, const C& c, const void* xm, const void* zpost, const void* cell_stats,
                           const bool in_learn) {
    const int mode = schedule_with(pl, p->work != nullptr);
    const bool chunked = mode == I2C_BWD_CHUNKED;  // (the plan answers it for the lane family and the d <= 8 quad walker: backward_chunked)
    const bool two_launch = SELF_STITCH && chunked && pl.rule == I2C_INF_CUBATURE && !c.has_x_terminal && !chunk_four_passes();
    const bool self = two_launch && pl.stitch == I2C_FAMILY_LANE && pl.walker == I2C_FAMILY_LANE;
    const bool lane_forward = in_learn && two_launch && pl.forward == I2C_FAMILY_LANE;
    bool helper = !NOISE && lane_forward && pl.compose == I2C_FAMILY_LANE && LANE_BLOCK == 64 && sweep_lanes() == LANE_BLOCK;
    if (helper) {
      const char* e = getenv("I2C_FORWARD_HELPER");
      helper = e ? strcmp(e, "0") != 0 : p->B >= forward_helper_min_b<M>::value;
    }
    // a reduction: the chunked and the two-pass schedule's (lane: neither chunked nor fused; wave: given its workspaces), no walk's
    const bool reduces = pl.backward == I2C_FAMILY_WAVE   ? mode == I2C_BWD_TWO_PASS && xm && cell_stats
                         : pl.backward == I2C_FAMILY_LANE ? mode != I2C_BWD_FUSED
                                                          : chunked;
    // I2C_FORWARD_HELPER_GAIN=0: the helper composes only and the sweep solves its gains itself (the reference of
    // tests/test_forward_gain_helper.py and of the A/B timing); any other value: the helper solves them also for a model whose default
    // is the sweep (forward_helper_gain)
    const char* const eg = getenv("I2C_FORWARD_HELPER_GAIN");
    int n_chunks, chunk_len;
    chunk_geometry(p->B, p->T, &n_chunks, &chunk_len);
    const bool helper_gain = helper && !MIXED && 3 * n_chunks >= sym(C::NX) && (eg ? strcmp(eg, "0") != 0 : forward_helper_gain<M>::value != 0);
    return Launches{mode, self, helper, helper_gain, !NOISE && lane_forward && self, reduces, I2C_WALK_LEAN && !xm && !zpost && !cell_stats && !c.z_per_cell};
  }

  // ---- the sweeps: each written once for either storage type, dispatched from the plan and the call's Launches ---------------------
  // The lane forward sweep under the sigma-point rule: k_forward, with the prologue of a pending M-step, with the helper wave (two
  // waves per workgroup: the sweep, and the compose pass of the backward sweep behind it) or with both
  template <bool LEAN>
  static int launch_forward_lane(const I2cProblem* p, const Launches& L, const C& c, const FwdArgs<R, S>& a, const PendingMstep<R>& pend, void* stream) {
    const int lanes = sweep_lanes();
    if constexpr (SELF_STITCH && !NOISE) {  // (process_noise: neither the helper wave nor the deferred M-step, Impl::launches)
      if (L.helper) {
        constexpr int W = HELPER_WAVES;
        const ChunkArgs<R, S> ch = chunk_args<M>(p, CellArgs<R, S>{a.fwd});  // (the compose pass reads the forward messages only)
        if constexpr (!MIXED) {
          if (L.helper_gain)
            return pend.part ? launch(k_forward_mstep_helper<M, R, LEAN, S, true>, W * (long)p->B, 1, W * LANE_BLOCK, stream, c, a, ch, pend)
                             : launch(k_forward_helper<M, R, LEAN, S, true>, W * (long)p->B, 1, W * LANE_BLOCK, stream, c, a, ch);
        }
        return pend.part ? launch(k_forward_mstep_helper<M, R, LEAN, S>, W * (long)p->B, 1, W * LANE_BLOCK, stream, c, a, ch, pend)
                         : launch(k_forward_helper<M, R, LEAN, S>, W * (long)p->B, 1, W * LANE_BLOCK, stream, c, a, ch);
      }
      if (pend.part) return launch(k_forward_mstep<M, R, LEAN, S>, p->B, 1, lanes, stream, c, a, lanes, pend);
    }
    return launch(k_forward<M, R, LEAN, false, S>, p->B, 1, lanes, stream, c, a, lanes);
  }
  // `pend` (i2c_learn only, Launches::defer; .part set): the previous iteration's reduction and M-step, finished in this sweep's prologue
  static int run_forward(const I2cProblem* p, const Plan& pl, const Launches& L, const C& c, const void* prior, void* fwd, void* prior_out,
                         int32_t* status, void* stream, const PendingMstep<R>& pend = {}) {
    if (pl.forward < 0) return pl.forward;
    const FwdArgs<R, S> a{(const S*)prior, (S*)fwd, (S*)prior_out, (const R*)p->x0, (const R*)p->sig_x0,
                          (const R*)p->z,  (const R*)p->alpha, (const R*)p->alpha_cell, p->feedforward, status, p->expert};
    if (p->horizons) {  // (resolved to the one-lane kernels: horizons_supported)
      if constexpr (HAS_HORIZONS) return launch(k_forward_hz<M, R>, p->B, 1, LANE_BLOCK, stream, c, a, p->horizons);
      return I2C_ENOTSUP;
    }
    if (pl.forward == I2C_FAMILY_WAVE) {
      if constexpr (HAS_WAVE) return launch_wave<WK_FORWARD, M, R, S>(c, a, stream);
    }
    if (pl.forward == I2C_FAMILY_QUAD) {
      if constexpr (HAS_QUAD) {
        C cq = c;
        cq.fwd_tm = pl.fwd_tm;
        return launch_quad_forward<M, R, S>(cq, a, stream);
      }
    }
    if (pl.forward == I2C_FAMILY_GROUP) {
      if constexpr (HAS_GROUP) return launch_group<GK_FORWARD, M, R, G>(c, nullptr, a, stream);
    }
    if (pl.forward == I2C_FAMILY_GRID) {
      if constexpr (HAS_GRID) return launch_grid<GRK_FORWARD, M, R>(c, a, stream);
    }
    if constexpr (LANE) {
      if constexpr (!MIXED) {  // (these two rules: fp64 storage)
        if (pl.rule == I2C_INF_LINEARIZE) return launch(k_forward_lin<M, R>, p->B, 1, LANE_BLOCK, stream, c, a);
        if (pl.rule == I2C_INF_GAUSS_HERMITE) return launch(k_forward<M, R, false, true>, p->B, 1, LANE_BLOCK, stream, c, a, LANE_BLOCK);
      }
      const bool lean = c.rule_xu.unit && c.rule_x.unit && !c.z_per_cell && !a.alpha_cell && !a.prior_out && c.t0 == 0;
      if (plan_trace())
        fprintf(stderr, "i2c_forward_lane: sweep=%s lean=%d gain=%s\n", L.helper ? "helper" : "plain", (int)lean, L.helper_gain ? "helper" : "sweep");
      return lean ? launch_forward_lane<true>(p, L, c, a, pend, stream) : launch_forward_lane<false>(p, L, c, a, pend, stream);
    }
    return I2C_ENOTSUP;
  }
  static int forward(const I2cProblem* p, const void* prior, void* fwd, void* prior_out, int32_t* status, void* stream) {
    const Plan pl = resolve(p);
    const C c = forward_consts(p);
    return run_forward(p, pl, launches(p, pl, c, nullptr, nullptr, nullptr, false), c, prior, fwd, prior_out, status, stream);
  }

  // Linearize() applies the terminal cost at the END of the chain, with the temperature of the cell that sits there
  // (i2c.py:475-491: the cell's own sig_xi_terminal). A receding-horizon loop appends cells that keep the temperature they were
  // copied with (I2cProblem.alpha_cell), so after the first shift that is not the graph's alpha.
  static const R* terminal_alpha(const I2cProblem* p, const C& c) {
    return p->alpha_cell ? (const R*)p->alpha_cell + (long)c.row(p->T - 1) * (long)p->B : (const R*)p->alpha;
  }
  // the M-step an iteration of i2c_learn ends with (run_mstep, or riding on a reduction: Launches::reduces), and a stand-alone sweep's none
  static MstepArgs<R> mstep_args(const I2cProblem* p, const void* term_stats, void* stats_out, const int update = 1) {
    return MstepArgs<R>{(const R*)term_stats, (R*)p->alpha, (R*)stats_out, update};
  }
  static MstepArgs<R> no_mstep(const void* term_stats) { return MstepArgs<R>{(const R*)term_stats, nullptr, nullptr, 0}; }
  // `c`: the constants of the call, with the M-step's tolerance where `ms` is one; `last`: the call's last iteration (Launches::defer)
  static int run_backward(const I2cProblem* p, const Plan& pl, const Launches& L, const C& c, const void* fwd, void* xm, void* post, void* zpost,
                          void* cell_stats, void* term_stats, int32_t* status, void* stream, const MstepArgs<R>& ms, const bool last = true) {
    if (pl.backward < 0) return pl.backward;
    if (pl.schedule < 0) return pl.schedule;
    const CellArgs<R, S> a{(const S*)fwd,  (const S*)xm,   (const R*)p->z, (S*)post, (S*)zpost,
                           (R*)cell_stats, (R*)term_stats, (R*)p->temp,    status,   terminal_alpha(p, c)};
    const int mode = L.schedule;
    int rc = I2C_ENOTSUP;
    if (p->horizons) {  // one schedule: the fused walk, each lane from its own last cell
      if constexpr (HAS_HORIZONS) return launch(k_bwd_fused_hz<M, R>, p->B, 1, LANE_BLOCK, stream, c, a, p->horizons);
      return I2C_ENOTSUP;
    }
    if (pl.backward == I2C_FAMILY_WAVE) {
      // the fused walk; two-pass (scan, one wave per cell, reduction -- with the M-step riding on it in i2c_learn) when that schedule
      // is asked for and its workspaces exist
      if constexpr (HAS_WAVE) {
        if (mode != I2C_BWD_TWO_PASS || !a.xm || !a.cell_stats) return launch_wave<WK_BACKWARD, M, R, S>(c, a, stream);
        rc = launch_wave<WK_SCAN, M, R, S>(c, a, stream);
        if (rc == I2C_OK) rc = launch_wave<WK_CELL, M, R, S>(c, a, stream);
        if (rc == I2C_OK) rc = launch_reduce<M, R>(c, a, ms, p->T, stream);
      }
      return rc;
    }
    if (pl.backward == I2C_FAMILY_QUAD) {
      if constexpr (HAS_QUAD_BACKWARD) {
        if constexpr (QUAD8) {
          if (mode == I2C_BWD_CHUNKED) return backward_chunked(p, pl, L, c, a, ms, last, stream);
        }
        return launch_quad_backward<M, R, S>(c, a, stream);
      }
    }
    if (pl.backward == I2C_FAMILY_GROUP) {  // one schedule: the group walks T-1..0 (the fused form)
      if constexpr (HAS_GROUP) return launch_group<GK_BACKWARD, M, R, G>(c, nullptr, a, stream);
    }
    if (pl.backward == I2C_FAMILY_GRID) {  // one schedule as well: the fused walk, no workspace
      if constexpr (HAS_GRID) return launch_grid<GRK_BACKWARD, M, R>(c, a, stream);
    }
    if constexpr (LANE) {
      if (mode == I2C_BWD_CHUNKED) return backward_chunked(p, pl, L, c, a, ms, last, stream);
      if (mode == I2C_BWD_FUSED) {  // a lane per trajectory walks T-1..0
        if constexpr (!MIXED) {
          if (pl.rule == I2C_INF_LINEARIZE) return launch(k_bwd_lin<M, R>, p->B, 1, LANE_BLOCK, stream, c, a);
          if (pl.rule == I2C_INF_GAUSS_HERMITE) return launch(k_bwd_fused<M, R, true>, p->B, 1, LANE_BLOCK, stream, c, a);
        }
        return L.walk_lean ? launch(k_bwd_fused<M, R, false, S, true>, p->B, 1, LANE_BLOCK, stream, c, a)
                           : launch(k_bwd_fused<M, R, false, S>, p->B, 1, LANE_BLOCK, stream, c, a);
      }
      if (!a.xm || !a.cell_stats) return I2C_EINVAL;  // two-pass needs both as workspace
      const ScanArgs<R, S> sc{a.fwd, const_cast<S*>(a.xm), (R*)p->temp, a.status};
      rc = launch(k_scan<M, R, S>, p->B, 1, LANE_BLOCK, stream, c, sc);
      if (rc == I2C_OK) rc = launch(k_cell<M, R, S>, p->B, p->T, CELL_BLOCK, stream, c, a);
      if (rc == I2C_OK) rc = launch_reduce<M, R>(c, a, ms, p->T, stream);
    }
    return rc;
  }
  // The chunked schedule for every rule: compose (one lane per trajectory and chunk) -> stitch -> walk -> reduce; in the two-launch form
  // (Launches::self_stitch) compose -> self-stitching walk, then the reduction, unless i2c_learn's next forward sweep takes it
  // (Launches::defer, every iteration but the `last`); behind a forward sweep with the helper wave (Launches::helper) the composites
  // are written and the schedule starts behind its compose pass. Sigma-point rule: each of the first three passes on the lane kernels
  // or in the quad form (four trajectories per wavefront), as the plan says. Linearize and Gauss-Hermite (fp64 storage): the lane
  // kernels, with their own stitch and walk -- the composition of the x-marginal recursion has no transform in it --, and Linearize
  // its own reduction over the chunks' partial sums.
  static int backward_chunked(const I2cProblem* p, const Plan& pl, const Launches& L, const C& c, const CellArgs<R, S>& a, const MstepArgs<R>& ms,
                              const bool last, void* stream) {
    int rc = I2C_ENOTSUP;
    if constexpr (LANE) {
      const ChunkArgs<R, S> ch = chunk_args<M>(p, a);
      const long B = p->B;
      const int nc = ch.n_chunks;
      const bool lin = !MIXED && pl.rule == I2C_INF_LINEARIZE, gh = !MIXED && pl.rule == I2C_INF_GAUSS_HERMITE;
      const bool self = L.self_stitch;
      // compose
      if (plan_trace())
        fprintf(stderr, "i2c_backward_chunked: compose=%s walk=%s lean=%d\n", L.helper ? "skipped" : "launched", self ? "self" : "plain",
                (int)L.walk_lean);
      if (L.helper) {
        rc = I2C_OK;
      } else if (pl.compose == I2C_FAMILY_QUAD) {
        if constexpr (QUAD8) rc = launch_quad_chunk_compose<M, R, S>(c, ch, stream);
      } else {
        rc = launch(k_chunk_compose<M, R, S>, B, nc, LANE_BLOCK, stream, c, ch);
      }
      if (rc != I2C_OK) return rc;
      // stitch
      rc = I2C_ENOTSUP;
      if (pl.stitch == I2C_FAMILY_QUAD) {
        if constexpr (QUAD8) rc = launch_quad_chunk_stitch<M, R, S>(c, ch, stream);
      } else if (lin || gh) {
        if constexpr (!MIXED)
          rc = lin ? launch(k_chunk_stitch_lin<M, R>, B, 1, LANE_BLOCK, stream, c, ch) : launch(k_chunk_stitch<M, R, R, true>, B, 1, LANE_BLOCK, stream, c, ch);
      } else if (!self) {
        rc = launch(k_chunk_stitch<M, R, S>, B, 1, LANE_BLOCK, stream, c, ch);
      } else {
        rc = I2C_OK;  // (the walkers compute their boundary states themselves; `bnd` stays unused)
      }
      if (rc != I2C_OK) return rc;
      // walk
      rc = I2C_ENOTSUP;
      if (pl.walker == I2C_FAMILY_QUAD) {
        if constexpr (QUAD8) rc = launch_quad_chunk_walk<M, R, S>(c, ch, stream);
      } else if (lin || gh) {
        if constexpr (!MIXED)
          rc = lin ? launch(k_chunk_walk_lin<M, R>, B, nc, LANE_BLOCK, stream, c, ch) : launch(k_chunk_walk<M, R, R, false, true>, B, nc, LANE_BLOCK, stream, c, ch);
      } else {
        const bool lean = L.walk_lean;
        if constexpr (SELF_STITCH) {
          if (self)
            rc = lean ? launch(k_chunk_walk_self<M, R, S, true>, B, nc, LANE_BLOCK, stream, c, ch)
                      : launch(k_chunk_walk_self<M, R, S>, B, nc, LANE_BLOCK, stream, c, ch);
        }
        if (!self) rc = lean ? launch(k_chunk_walk<M, R, S, true>, B, nc, LANE_BLOCK, stream, c, ch) : launch(k_chunk_walk<M, R, S>, B, nc, LANE_BLOCK, stream, c, ch);
      }
      if (rc != I2C_OK) return rc;
      // reduce
      if (lin) {
        if constexpr (!MIXED) rc = launch(k_chunk_reduce_lin<M, R>, B, 1, LANE_BLOCK, stream, c, ch, ms);
      } else if (!L.defer || last) {  // (deferred: finish_pending_mstep in the prologue of the caller's next forward sweep, pending_mstep)
        C cr = c;  // reduction over chunks instead of cells: same kernel, T := number of chunks
        cr.T = nc;
        CellArgs<R, S> ared = a;
        ared.cell_stats = ch.part;
        rc = launch_reduce<M, R>(cr, ared, ms, p->T, stream);
      }
    }
    return rc;
  }
  static int backward(const I2cProblem* p, const void* fwd, void* xm, void* post, void* zpost, void* cell_stats,
                      void* term_stats, int32_t* status, void* stream) {
    const Plan pl = resolve(p);
    const C c = make_consts<M, R>(p, 0.0, 0);
    return run_backward(p, pl, launches(p, pl, c, xm, zpost, cell_stats, false), c, fwd, xm, post, zpost, cell_stats, term_stats, status, stream,
                        no_mstep(term_stats));
  }

  static int riccati(const I2cProblem* p, const void* prior_out, const void* fwd, const void* xm, void* post, void* ric,
                     int32_t* status, void* stream) {
    if constexpr (MIXED || NOISE) return I2C_ENOTSUP;  // (NOISE: the Riccati messages read the constant sig_eta alone)
    if (p->horizons) return I2C_EINVAL;  // (a Linearize pass: no per-trajectory horizons)
    if constexpr (LANE) {
      if (!lane_request(p->group_lanes)) return I2C_ENOTSUP;
      const C c = make_consts<M, R>(p, 0.0, 0);
      RiccatiArgs<R> a{(const R*)prior_out, (const R*)fwd, (const R*)xm, (const R*)p->z, (const R*)p->alpha,
                       (const R*)p->alpha_cell, (R*)post, (R*)ric, status};
      return launch(k_riccati<M, R>, p->B, 1, LANE_BLOCK, stream, c, a);
    }
    return I2C_ENOTSUP;
  }

  // `c`: the constants of the call with the M-step's tolerance
  static int run_mstep(const I2cProblem* p, const C& c, const MstepArgs<R>& a, void* stream) {
    if (p->horizons) {  // sf = nz T_b (+ nzt)
      if constexpr (HAS_HORIZONS) return horizons_supported(p) != I2C_OK ? horizons_supported(p) : launch(k_mstep_hz<M, R>, p->B, 1, LANE_BLOCK, stream, c, a, p->horizons);
      return I2C_ENOTSUP;
    }
    return launch(k_mstep<M, R>, p->B, 1, LANE_BLOCK, stream, c, a);
  }
  static int mstep(const I2cProblem* p, const void* term_stats, double tol, int update, void* stats_out, void* stream) {
    return run_mstep(p, make_consts<M, R>(p, tol, 0), mstep_args(p, term_stats, stats_out, update), stream);
  }

  // _update_priors (i2c.py:1210-1213): cells with index <= tau switch to feedback mode
  static int to_feedback(const I2cProblem* p, int tau, void* stream) {
    const int n = tau + 1 < p->T ? tau + 1 : p->T;  // cells 0 .. n-1 = ring rows t0 .. t0+n-1 (mod T): at most two spans
    return launch(k_to_feedback<M>, n, 1, CELL_BLOCK, stream, const_cast<uint8_t*>(p->feedforward), p->t0, n, p->T);
  }

  static int learn(const I2cProblem* p, void* post, void* fwd, void* xm, void* zpost, void* cell_stats,
                   void* term_stats, double tol, int tau, int n_iters, void* stats_hist, int32_t* status,
                   void* stream) {
    const Plan pl = resolve(p);
    const C cf = forward_consts(p), cb = make_consts<M, R>(p, tol, 0);
    const Launches L = launches(p, pl, cb, xm, zpost, cell_stats, true);
    // Behind a self-stitching chunked backward sweep the reduction and the M-step of iteration `it` run in the prologue of iteration
    // it + 1's forward sweep (k_forward_mstep); the last iteration of the call ends with k_reduce as a backward sweep on its own does.
    PendingMstep<R> pend{};  // (.part == nullptr: none)
    for (int it = 0; it < n_iters; ++it) {
      const bool last = it + 1 == n_iters;
      const MstepArgs<R> ms = mstep_args(p, term_stats, (R*)stats_hist + (size_t)it * 4 * p->B);
      int rc = run_forward(p, pl, L, cf, post, fwd, nullptr, status, stream, pend);
      if (rc == I2C_OK) rc = run_backward(p, pl, L, cb, fwd, xm, post, zpost, cell_stats, term_stats, status, stream, ms, last);
      pend = (L.defer && !last) ? pending_mstep(p, cb, term_stats, ms) : PendingMstep<R>{};
      if (rc == I2C_OK) rc = finish_iteration(p, L, cb, ms, tau, it, stream);
      if (rc != I2C_OK) return rc;
    }
    return I2C_OK;
  }
  // what the forward sweep behind a deferring backward sweep finishes: the walkers' partial sums in the chunk workspace, and this M-step
  static PendingMstep<R> pending_mstep(const I2cProblem* p, const C& c, void* term_stats, const MstepArgs<R>& ms) {
    const ChunkArgs<R, S> ch = chunk_args<M>(p, CellArgs<R, S>{});
    return PendingMstep<R>{ch.part, (R*)term_stats, ms, ch.n_chunks, c.tol};
  }
  // the tail of an EM iteration: the M-step in a kernel of its own where no reduction carried it, and after the first one the mode flags
  static int finish_iteration(const I2cProblem* p, const Launches& L, const C& c, const MstepArgs<R>& ms, const int tau, const int it, void* stream) {
    int rc = L.reduces ? I2C_OK : run_mstep(p, c, ms, stream);  // fused / group / Linearize / Gauss-Hermite walks have no reduction kernel
    if (rc == I2C_OK && tau > 0 && it == 0) rc = to_feedback(p, tau, stream);  // idempotent: once per call
    return rc;
  }

  // n_iters EM iterations WITH closed-loop propagation (covariance control: learn_msgs with _propagate, i2c.py:1238-1251) enqueued by
  // one call: forward, backward, propagate, M-step per iteration. From the second iteration on the propagation of iteration k
  // shares a launch with the forward sweep of iteration k + 1 (k_forward_propagate) where both run on the lane kernels (Plan::fusable);
  // the first one runs in order -- its M-step is followed by the mode-flag switch the propagation reads. Same kernels' bodies, same
  // inputs as the one-by-one calls: identical results (a trajectory that fails in BOTH overlapped sweeps records either code).
  static int learn_propagate(const I2cProblem* p, void* post, void* fwd, void* xm, void* zpost, void* cell_stats, void* term_stats,
                             void* prop, void* prop_hist, double tol, int tau, int n_iters, void* stats_hist, int use_expert,
                             int overlap, int32_t* status, void* stream) {
    if constexpr (MIXED) return I2C_ENOTSUP;
    const Plan pl = resolve(p);
    const C cf = forward_consts(p), cb = make_consts<M, R>(p, tol, 0), cp = propagate_consts(p, use_expert);
    const Launches L = launches(p, pl, cb, xm, zpost, cell_stats, false);
    auto prop_row = [&](int it) { return (void*)((R*)prop_hist + (size_t)it * 3 * p->B); };
    int pending = -1;  // iteration whose propagation has not run yet
    for (int it = 0; it < n_iters; ++it) {
      int rc = I2C_OK;
      bool fused = false;
      if constexpr (LANE && C::D <= 5 && !NOISE) {
        if (overlap && pl.fusable && pending >= 0) {  // (fusable: the sigma-point rule as given, so cp is the forward sweep's constants with use_expert)
          FwdArgs<R> af{(const R*)post, (R*)fwd, nullptr, (const R*)p->x0, (const R*)p->sig_x0, (const R*)p->z, (const R*)p->alpha,
                        (const R*)p->alpha_cell, p->feedforward, status, p->expert};
          PropArgs<R> ap{(const R*)post, (R*)prop, (R*)prop_row(pending), (const R*)p->x0, (const R*)p->sig_x0,
                         (const R*)p->z, p->feedforward, status, p->expert};
          rc = launch(k_forward_propagate<M, R, true>, p->B, 2, LANE_BLOCK, stream, cp, af, ap);
          fused = true;
          pending = -1;
        }
      }
      if (!fused) {
        if (pending >= 0) {
          rc = run_propagate(p, pl, cp, post, prop, prop_row(pending), status, stream);
          pending = -1;
          if (rc != I2C_OK) return rc;
        }
        rc = run_forward(p, pl, L, cf, post, fwd, nullptr, status, stream);
      }
      if (rc != I2C_OK) return rc;
      const MstepArgs<R> ms = mstep_args(p, term_stats, (R*)stats_hist + (size_t)it * 4 * p->B);
      rc = run_backward(p, pl, L, cb, fwd, xm, post, zpost, cell_stats, term_stats, status, stream, ms);
      if (rc != I2C_OK) return rc;
      if (it == 0) {  // in order: the mode flags change right after this M-step
        rc = run_propagate(p, pl, cp, post, prop, prop_row(0), status, stream);
        if (rc != I2C_OK) return rc;
      } else {
        pending = it;
      }
      rc = finish_iteration(p, L, cb, ms, tau, it, stream);
      if (rc != I2C_OK) return rc;
    }
    if (pending >= 0) return run_propagate(p, pl, cp, post, prop, prop_row(pending), status, stream);
    return I2C_OK;
  }

  static int run_ckf(const I2cProblem* p, const Plan& pl, const double* sig_zeta, const void* y, const void* u, void* mu, void* cov,
                     int32_t* status, void* stream) {
    if (pl.filter < 0) return pl.filter;
    const C c = filter_consts(p);
    ZetaArg<M, R> z;
    for (int i = 0; i < sym(M::NY); ++i) z.v[i] = (R)sig_zeta[i];
    CkfArgs<R> a{(const R*)y, (const R*)u, (R*)mu, (R*)cov, status};
    if (pl.filter == I2C_FAMILY_QUAD) {
      if constexpr (HAS_QUAD_CKF) return launch_quad_ckf<M, R>(c, z, a, stream);
    }
    if (pl.filter == I2C_FAMILY_GROUP) {
      if constexpr (HAS_GROUP) return launch_group<GK_CKF, M, R, G>(c, &z, a, stream);
    }
    if constexpr (LANE) return launch(k_ckf<M, R>, p->B, 1, LANE_BLOCK, stream, c, z, a);
    return I2C_ENOTSUP;
  }
  static int ckf(const I2cProblem* p, const double* sig_zeta, const void* y, const void* u, void* mu, void* cov,
                 int32_t* status, void* stream) {
    if constexpr (MIXED) return I2C_ENOTSUP;
    return run_ckf(p, resolve(p), sig_zeta, y, u, mu, cov, status, stream);
  }

  // One control step of the MPC loop enqueued by one call (i2c/policy/mpc.py:156-182): filter, n_iter x (forward,
  // backward, _update_priors), first action, and the horizon shift: one fresh row written into the ring of per-cell buffers
  // (the caller then advances I2cProblem.t0 by one and moves terminal_cell).
  static int mpc_step(const I2cProblem* p, const I2cMpcStep* m, void* stream) {
    if constexpr (MIXED) return I2C_ENOTSUP;
    if (p->horizons) return I2C_EINVAL;  // the ring of the MPC loop has one horizon
    const Plan pl = resolve(p);
    const C cf = forward_consts(p), cb = make_consts<M, R>(p, 0.0, 0);
    const Launches L = launches(p, pl, cb, m->xm, m->zpost, m->cell_stats, false);
    int rc = I2C_OK;
    if (m->do_filter) rc = run_ckf(p, pl, m->sig_zeta, m->y, m->u, const_cast<void*>(p->x0), const_cast<void*>(p->sig_x0), m->status, stream);
    for (int it = 0; it < m->n_iter && rc == I2C_OK; ++it) {
      rc = run_forward(p, pl, L, cf, m->post, m->fwd, nullptr, m->status, stream);
      if (rc == I2C_OK) rc = run_backward(p, pl, L, cb, m->fwd, m->xm, m->post, m->zpost, m->cell_stats, m->term_stats, m->status, stream, no_mstep(m->term_stats));
      if (rc == I2C_OK && m->tau > 0 && it == 0) rc = to_feedback(p, m->tau, stream);  // (idempotent within a step: _update_priors)
    }
    if (rc != I2C_OK) return rc;
    return run_shift(p, cb, m->post, m->cell_init, m->alpha_init, m->z_new, m->action, stream);
  }
  // the receding-horizon shift alone (BatchedI2c.shift_horizon, the step-by-step path of the policies)
  static int shift(const I2cProblem* p, void* post, const void* cell_init, const void* alpha_init, const void* z_new, void* action,
                   void* stream) {
    if constexpr (MIXED) return I2C_ENOTSUP;
    if (p->horizons) return I2C_EINVAL;
    return run_shift(p, make_consts<M, R>(p, 0.0, 0), post, cell_init, alpha_init, z_new, action, stream);
  }
  static int run_shift(const I2cProblem* p, const C& c, void* post, const void* cell_init, const void* alpha_init, const void* z_new,
                       void* action, void* stream) {
    ShiftArgs<R> a{(R*)post, (const R*)cell_init, (R*)const_cast<void*>(p->alpha_cell), (const R*)alpha_init,
                   (R*)const_cast<void*>(p->z_per_cell ? p->z : nullptr), (const R*)z_new, const_cast<uint8_t*>(p->feedforward),
                   (R*)action};
    // the per-trajectory part (first action out, temperature, target, mode flag of the fresh cell), then the fresh cell: one
    // contiguous block copy (a lane-per-trajectory loop over the e_post elements took 111 us at B = 1024 for the 12-state
    // quadrotor: 230 dependent partial-line stores per lane -- a tenth of the control step)
    int rc = launch(k_mpc_shift<M, R>, p->B, 1, CELL_BLOCK, stream, c, a);
    if (rc == I2C_OK)
      rc = copy_bytes((R*)post + (size_t)c.row(0) * C::E_POST * p->B, cell_init, (size_t)C::E_POST * p->B * sizeof(R), stream);
    return rc;
  }

  static int rollout(const I2cProblem* p, const void* post, int n_rollouts, int policy, const void* eps_x0,
                     const void* eps_x, const void* eps_u, void* xu, void* z, void* x_final, void* z_term,
                     void* stream) {
    if constexpr (MIXED) return I2C_ENOTSUP;
    const C c = make_consts<M, R>(p, 0.0, 0);
    if (p->horizons && horizons_supported(p) != I2C_OK) return horizons_supported(p);
    RolloutArgs<R> a{(const R*)post, (const R*)p->x0, (const R*)p->sig_x0, (const R*)eps_x0, (const R*)eps_x,
                     (const R*)eps_u, (R*)xu, (R*)z, (R*)x_final, (R*)z_term, n_rollouts, policy};
    if (p->horizons) {  // rollout n ends behind cell T_b - 1 of trajectory b = n % B
      if constexpr (HAS_HORIZONS) return launch(k_rollout_hz<M, R>, (long)n_rollouts * p->B, 1, LANE_BLOCK, stream, c, a, p->horizons);
      return I2C_ENOTSUP;
    }
    return launch(k_rollout<M, R>, (long)n_rollouts * p->B, 1, LANE_BLOCK, stream, c, a);
  }

  // i2c_rollout_eval: `parts` as i2c_capi.hip resolved it (1 .. n_rollouts); the arguments are checked there
  static int rollout_eval(const I2cProblem* p, const void* post, const I2cRolloutEval* e, int parts, void* stream) {
    if constexpr (MIXED || sizeof(R) != 8) {
      return I2C_ENOTSUP;  // the sums are fp64
    } else {
      const C c = make_consts<M, R>(p, 0.0, 0);
      if (p->horizons && horizons_supported(p) != I2C_OK) return horizons_supported(p);
      RolloutArgs<R> a{(const R*)post, (const R*)p->x0, (const R*)p->sig_x0, (const R*)e->eps_x0, (const R*)e->eps_x,
                       (const R*)e->eps_u, nullptr, nullptr, nullptr, nullptr, e->n_rollouts, e->policy};
      const bool moments = e->xu_mean != nullptr;
      EvalArgs<R> ev{(const R*)(c.z_per_cell ? p->z : nullptr), (R*)e->cost, moments ? (R*)e->work : nullptr, e->seed, e->first_trajectory,
                     e->noise, moments ? parts : e->n_rollouts};
      int rc = launch(k_rollout_eval<M, R>, (long)ev.parts * p->B, 1, LANE_BLOCK, stream, c, a, ev, p->horizons);
      if (rc != I2C_OK || (!moments && !e->cost_stats && !e->n_bad)) return rc;
      EvalReduceArgs<R> ra{(const R*)post, ev.work, (const R*)e->cost, (R*)e->cost_stats, e->n_bad, (R*)e->xu_mean, (R*)e->xu_cov,
                           e->n_rollouts, ev.parts};
      return launch(k_rollout_eval_reduce<M, R>, p->B, moments ? p->T : 1, LANE_BLOCK, stream, c, ra, p->horizons);
    }
  }

  // One plant step of the closed MPC loop (i2c_plant_step, and every step of i2c_mpc_episode): plant_step_body, one lane per
  // trajectory for every model -- it is one dynamics, one observe and one measure evaluation, with nothing to share between lanes.
  static int plant_step(const I2cProblem* p, const PlantCall* k, void* stream) {
    if constexpr (MIXED) return I2C_ENOTSUP;
    const C c = make_consts<M, R>(p, 0.0, 0);
    PlantNoise<M, R> nz{};
    for (int i = 0; i < sym(M::NX); ++i) nz.Le[i] = k->Le ? (R)k->Le[i] : R(0);
    for (int i = 0; i < sym(M::NY); ++i) nz.Lz[i] = k->Lz ? (R)k->Lz[i] : R(0);
    PlantArgs<R> a{(R*)k->x,           (const R*)k->u,     (const R*)k->eps_x, (const R*)k->eps_y, (R*)k->y_out,
                   (R*)k->u_out,       (R*)k->x_obs,       (const R*)k->mu,    (const R*)k->z_ref, (R*)k->cost,
                   (R*)k->x_hist,      (R*)k->u_hist,      (R*)k->y_hist,      (R*)k->mu_hist};
    return launch(k_plant_step<M, R>, p->B, 1, LANE_BLOCK, stream, c, nz, a);
  }

  // `c`: propagate_consts
  static int run_propagate(const I2cProblem* p, const Plan& pl, const C& c, const void* post, void* prop, void* prop_stats, int32_t* status,
                           void* stream) {
    if (pl.propagate < 0) return pl.propagate;
    PropArgs<R> a{(const R*)post, (R*)prop, (R*)prop_stats, (const R*)p->x0, (const R*)p->sig_x0,
                  (const R*)p->z, p->feedforward, status, p->expert};
    if (p->horizons) {
      if constexpr (HAS_HORIZONS) return launch(k_propagate_hz<M, R>, p->B, 1, LANE_BLOCK, stream, c, a, p->horizons);
      return I2C_ENOTSUP;
    }
    if (pl.propagate == I2C_FAMILY_QUAD) {
      if constexpr (HAS_QUAD_PROP) return launch_quad_propagate<M, R>(c, a, stream);
    }
    if (pl.propagate == I2C_FAMILY_GROUP) {
      if constexpr (HAS_GROUP) return launch_group<GK_PROPAGATE, M, R, G>(c, nullptr, a, stream);
    }
    if (pl.propagate == I2C_FAMILY_GRID) {
      if constexpr (HAS_GRID) return launch_grid<GRK_PROPAGATE, M, R>(c, a, stream);
    }
    if constexpr (LANE) {
      if (pl.rule == I2C_INF_GAUSS_HERMITE) return launch(k_propagate<M, R, true>, p->B, 1, LANE_BLOCK, stream, c, a);
      return launch(k_propagate<M, R>, p->B, 1, LANE_BLOCK, stream, c, a);
    }
    return I2C_ENOTSUP;
  }
  static int propagate(const I2cProblem* p, const void* post, void* prop, void* prop_stats, int use_expert,
                       int32_t* status, void* stream) {
    if constexpr (MIXED) return I2C_ENOTSUP;
    return run_propagate(p, resolve(p), propagate_consts(p, use_expert), post, prop, prop_stats, status, stream);
  }
};

template <class M> static void fill_dims(I2cDims* d) {
  using C = Consts<M, double>;
  d->nx = M::NX;
  d->nu = M::NU;
  d->nz = M::NZ;
  d->nzt = M::NZT;
  d->e_post = C::E_POST;
  d->e_fwd = C::E_FWD;
  d->e_xm = C::E_XM;
  d->e_zpost = C::E_ZPOST;
  d->e_prop = C::E_PROP;
  d->n_params = M::NP;
  d->ny = M::NY;
  d->group_lanes = M::GROUP;
  d->group_only = M::GROUP_ONLY ? 1 : 0;
  d->wave = M::WAVE ? 1 : 0;
  d->quad = M::QUAD ? 1 : 0;
}

// per_traj: the table of Impl<PerTraj<M>, R, S> (per-trajectory parameters, I2cProblem.model_params_b; i2c_capi.hip switches to it when the
// pointer is set), built in a translation unit of its own (i2c_model_tu.hip); nullptr for a model without parameters and in that table
template <class M, typename R, typename S = R> const ModelOps* make_ops(const ModelOps* per_traj) {
  using I = Impl<M, R, S>;
  static const ModelOps ops = {&I::forward, &I::backward,  &I::mstep,        &I::learn,           &I::ckf,
                               &I::rollout, &I::propagate, &I::riccati,   &I::mpc_step,        &fill_dims<M>,
                               &workspace_elems<M>, &I::plan, &I::shift, &I::family_of, &I::learn_propagate, per_traj,
                               &I::plant_step, &I::rollout_eval};
  return &ops;
}
// ... the per-trajectory table itself: only models with parameters have one
template <class M, typename R, typename S = R> const ModelOps* make_per_traj_ops() {
  if constexpr (M::NP > 0) return make_ops<PerTraj<M>, R, S>(nullptr);
  else return nullptr;
}

}  // namespace i2c
