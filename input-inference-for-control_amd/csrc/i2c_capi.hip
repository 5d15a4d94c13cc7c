// C ABI (include/i2c_hip.h): argument checks and dispatch over (model_id, dtype) to the per-pair translation units
// (i2c_model_tu.hip -> i2c_impl.hpp). No kernel code is compiled here.
#include <dlfcn.h>

#include <cmath>
#include <cstddef>
#include <mutex>

#include "i2c_entry.hpp"

namespace {

// Out-of-tree models (i2c_register_model / i2c_load_model): an append-only table of per-dtype ops tables. The only mutable
// state of the library: entries are written once under the mutex and never change or move afterwards, so readers of a
// published id need no lock.
struct PluginEntry {
  const i2c::ModelOps* ops[3];  // I2C_F64, I2C_F32, I2C_F64_F32S (nullptr: that precision was not built)
  size_t ops_bytes;             // how much of a table exists: sizeof(ModelOps) as the LIBRARY was compiled (i2c_model_ops_size)
};  // (a library opened by i2c_load_model stays loaded for the life of the process: its handle is never closed once registered)
PluginEntry g_plugins[I2C_MAX_PLUGIN_MODELS];
int g_n_plugins = 0;
std::mutex g_plugin_mutex;

const i2c::ModelOps* find_ops(int model_id, int dtype) {
  if (dtype != I2C_F64 && dtype != I2C_F32 && dtype != I2C_F64_F32S) return nullptr;
  if (model_id >= I2C_MODEL_PLUGIN_BASE) {
    const int k = model_id - I2C_MODEL_PLUGIN_BASE;
    int n;
    {
      std::lock_guard<std::mutex> lock(g_plugin_mutex);
      n = g_n_plugins;
    }
    return k < n ? g_plugins[k].ops[dtype] : nullptr;
  }
  switch (model_id) {
#define I2C_CASE(ID, MODEL, name) \
  case ID: return dtype == I2C_F64 ? i2c::ops_##name##_f64() : (dtype == I2C_F32 ? i2c::ops_##name##_f32() : i2c::ops_##name##_f64s());
    I2C_FOR_EACH_MODEL(I2C_CASE)
#undef I2C_CASE
    default: return nullptr;
  }
}

// the scalar fields alone (what the resolvers i2c_kernel_family / i2c_backward_schedule read: no buffer needs to exist yet)
int check_problem_shape(const I2cProblem* p);
int check_problem(const I2cProblem* p) {
  const int rc = check_problem_shape(p);
  if (rc != I2C_OK) return rc;
  if (!p->x0 || !p->sig_x0 || !p->alpha || !p->feedforward) return I2C_EINVAL;
  if (p->has_x_terminal && !p->temp) return I2C_EINVAL;
  return I2C_OK;
}
int check_problem_shape(const I2cProblem* p) {
  if (!p || p->abi_version != I2C_ABI_VERSION) return I2C_EINVAL;
  if (p->B < 1 || p->T < 1 || p->T > 65535) return I2C_EINVAL;  // status words keep t + 1 in 16 bits
  if (p->inference < I2C_INF_CUBATURE || p->inference > I2C_INF_GAUSS_HERMITE) return I2C_EINVAL;
  if (p->inference == I2C_INF_GAUSS_HERMITE && (p->gh_degree < 1 || p->gh_degree > I2C_MAX_GH_DEGREE)) return I2C_EINVAL;
  if (p->t0 < 0 || p->t0 >= p->T) return I2C_EINVAL;
  if (p->post_layout != 0 && p->post_layout != 1) return I2C_EINVAL;
  if (p->post_layout == 1) {  // trajectory-major posterior: only the models whose every kernel knows it
    I2cDims d;
    const i2c::ModelOps* ops = find_ops(p->model_id, I2C_F64);
    if (!ops) return I2C_EINVAL;
    ops->dims(&d);
    if (!d.wave) return I2C_ENOTSUP;
  }
  if (p->model_params_b) {  // per-trajectory parameters: nothing to vary on a model without parameters
    I2cDims d;
    const i2c::ModelOps* ops = find_ops(p->model_id, I2C_F64);
    if (!ops) return I2C_EINVAL;
    ops->dims(&d);
    if (d.n_params == 0) return I2C_EINVAL;
  }
  return I2C_OK;
}

}  // namespace

// Check the problem, find the (model, dtype) table, call one of its entries.
#define I2C_DISPATCH(p, CALL)                                             \
  do {                                                                    \
    const int rc_ = check_problem(p);                                     \
    if (rc_ != I2C_OK) return rc_;                                        \
    const i2c::ModelOps* ops_ = find_ops((p)->model_id, (p)->dtype);      \
    if (ops_ && (p)->model_params_b) ops_ = ops_->per_traj;               \
    if (!ops_) return I2C_EINVAL;                                         \
    return ops_->CALL;                                                    \
  } while (0)

extern "C" {

int i2c_abi_version(void) { return I2C_ABI_VERSION; }

size_t i2c_problem_size(void) { return sizeof(I2cProblem); }

const char* i2c_build_info(void) {
#ifdef I2C_HOST_SIM
  return "i2c host-simulation build (CPU, tests only)";
#else
  return "i2c hip build: gfx950 (MI355X), wave64; lane kernels (one trajectory per lane) + group kernels (4/8/16 lanes per trajectory, LDS exchange) + wave kernels (one wavefront per trajectory, v_mfma_f64_16x16x4_f64) + quad kernels (four trajectories per wavefront, v_mfma_f64_4x4x4_4b_f64) + grid kernels (Gauss-Hermite grid over one wavefront per trajectory)";
#endif
}

// the two resolvers read scalar fields only: they answer before any buffer of the problem exists
#define I2C_DISPATCH_SHAPE(p, CALL)                                       \
  do {                                                                    \
    const int rc_ = check_problem_shape(p);                               \
    if (rc_ != I2C_OK) return rc_;                                        \
    const i2c::ModelOps* ops_ = find_ops((p)->model_id, (p)->dtype);      \
    if (!ops_) return I2C_EINVAL;                                         \
    return ops_->CALL;                                                    \
  } while (0)

int i2c_backward_schedule(const I2cProblem* p) {
  if (p && (p->backward_mode < I2C_BWD_AUTO || p->backward_mode > I2C_BWD_CHUNKED)) return I2C_EINVAL;
  I2C_DISPATCH_SHAPE(p, plan(p));
}

int i2c_kernel_family(const I2cProblem* p, int sweep) {
  if (sweep < I2C_SWEEP_FORWARD || sweep > I2C_SWEEP_CHUNK_STITCH) return I2C_EINVAL;
  I2C_DISPATCH_SHAPE(p, family(p, sweep));
}

size_t i2c_workspace_bytes(int model_id, int dtype, int B, int T) {
  if (B < 1 || T < 1) return 0;
  const i2c::ModelOps* ops = find_ops(model_id, I2C_F64);
  return ops ? (dtype == I2C_F32 ? 4 : 8) * ops->workspace_elems(B, T) : 0;  // the workspace is arithmetic-typed (fp64 in I2C_F64_F32S)
}

// Entries appended to ModelOps after ABI v9 froze (rollout_eval): a table whose library does not state its size ends before them
constexpr size_t OPS_BYTES_V9 = offsetof(i2c::ModelOps, rollout_eval);

static int register_model(int abi_version, const I2cModelOps* ops_f64, const I2cModelOps* ops_f32, const I2cModelOps* ops_f64s,
                          I2cDims* dims_out, size_t ops_bytes) {
  if (abi_version != I2C_ABI_VERSION || !ops_f64) return I2C_EINVAL;
  const i2c::ModelOps* t[3] = {reinterpret_cast<const i2c::ModelOps*>(ops_f64), reinterpret_cast<const i2c::ModelOps*>(ops_f32),
                               reinterpret_cast<const i2c::ModelOps*>(ops_f64s)};
  I2cDims d;
  t[0]->dims(&d);
  if (d.nx < 1 || d.nx > I2C_MAX_NX || d.nu < 1 || d.nu > I2C_MAX_NU || d.nz < 1 || d.nz > I2C_MAX_NZ || d.nzt < 0 || d.nzt > I2C_MAX_NZ ||
      d.n_params < 0 || d.n_params > I2C_MAX_PARAMS || d.ny < 0 || d.ny > I2C_MAX_NZ)
    return I2C_EINVAL;  // the host constants of I2cProblem have fixed capacities
  std::lock_guard<std::mutex> lock(g_plugin_mutex);
  for (int k = 0; k < g_n_plugins; ++k)  // registering the same tables again returns the id they already have
    if (g_plugins[k].ops[0] == t[0]) {
      if (dims_out) *dims_out = d;
      return I2C_MODEL_PLUGIN_BASE + k;
    }
  if (g_n_plugins >= I2C_MAX_PLUGIN_MODELS) return I2C_ENOTSUP;
  g_plugins[g_n_plugins] = PluginEntry{{t[0], t[1], t[2]}, ops_bytes};
  if (dims_out) *dims_out = d;
  return I2C_MODEL_PLUGIN_BASE + g_n_plugins++;
}

int i2c_register_model(int abi_version, const I2cModelOps* ops_f64, const I2cModelOps* ops_f32, const I2cModelOps* ops_f64s,
                       I2cDims* dims_out) {
  return register_model(abi_version, ops_f64, ops_f32, ops_f64s, dims_out, OPS_BYTES_V9);
}

int i2c_load_model(const char* path, I2cDims* dims_out) {
  if (!path) return I2C_EINVAL;
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) return I2C_EINVAL;
  typedef int (*abi_fn)(void);
  typedef const I2cModelOps* (*ops_fn)(int);
  abi_fn abi = (abi_fn)dlsym(h, "i2c_model_abi_version");
  ops_fn ops = (ops_fn)dlsym(h, "i2c_model_ops");
  if (!abi || !ops) {
    dlclose(h);
    return I2C_EINVAL;
  }
  typedef size_t (*size_fn)(void);
  size_fn size = (size_fn)dlsym(h, "i2c_model_ops_size");  // optional: a library built before the table grew has none
  const int id = register_model(abi(), ops(I2C_F64), ops(I2C_F32), ops(I2C_F64_F32S), dims_out, size ? size() : OPS_BYTES_V9);
  if (id < 0) dlclose(h);  // (a library registered twice keeps its first handle: dlopen reference-counts)
  return id;
}

int i2c_query(int model_id, I2cDims* out) {
  const i2c::ModelOps* ops = find_ops(model_id, I2C_F64);
  if (!out || !ops) return I2C_EINVAL;
  ops->dims(out);
  return I2C_OK;
}

int i2c_forward_sweep(const I2cProblem* p, const void* prior, void* fwd, void* prior_out, int32_t* status,
                      void* stream) {
  if (!prior || !fwd || !status) return I2C_EINVAL;
  I2C_DISPATCH(p, forward(p, prior, fwd, prior_out, status, stream));
}

int i2c_backward_sweep(const I2cProblem* p, const void* fwd, void* xm, void* post, void* zpost, void* cell_stats,
                       void* term_stats, int32_t* status, void* stream) {
  if (!fwd || !post || !term_stats || !status) return I2C_EINVAL;
  I2C_DISPATCH(p, backward(p, fwd, xm, post, zpost, cell_stats, term_stats, status, stream));
}

int i2c_mstep(const I2cProblem* p, const void* term_stats, double alpha_update_tol, int update, void* stats_out,
              void* stream) {
  if (!term_stats || !stats_out) return I2C_EINVAL;
  I2C_DISPATCH(p, mstep(p, term_stats, alpha_update_tol, update, stats_out, stream));
}

int i2c_propagate(const I2cProblem* p, const void* post, void* prop, void* prop_stats, int use_expert_controller,
                  int32_t* status, void* stream) {
  if (!post || !prop || !prop_stats || !status) return I2C_EINVAL;
  I2C_DISPATCH(p, propagate(p, post, prop, prop_stats, use_expert_controller, status, stream));
}

int i2c_learn(const I2cProblem* p, void* post, void* fwd, void* xm, void* zpost, void* cell_stats, void* term_stats,
              double alpha_update_tol, int tau, int n_iters, void* stats_hist, int32_t* status, void* stream) {
  if (!post || !fwd || !term_stats || !stats_hist || !status || n_iters < 0) return I2C_EINVAL;
  I2C_DISPATCH(p, learn(p, post, fwd, xm, zpost, cell_stats, term_stats, alpha_update_tol, tau, n_iters, stats_hist,
                        status, stream));
}

int i2c_learn_propagate(const I2cProblem* p, void* post, void* fwd, void* xm, void* zpost, void* cell_stats, void* term_stats, void* prop,
                        void* prop_hist, double alpha_update_tol, int tau, int n_iters, void* stats_hist, int use_expert_controller,
                        int overlap, int32_t* status, void* stream) {
  if (!post || !fwd || !term_stats || !prop || !prop_hist || !stats_hist || !status || n_iters < 0) return I2C_EINVAL;
  I2C_DISPATCH(p, learn_propagate(p, post, fwd, xm, zpost, cell_stats, term_stats, prop, prop_hist, alpha_update_tol, tau, n_iters,
                                  stats_hist, use_expert_controller, overlap, status, stream));
}

int i2c_rollout(const I2cProblem* p, const void* post, int n_rollouts, int policy, const void* eps_x0,
                const void* eps_x, const void* eps_u, void* xu, void* z, void* x_final, void* z_term, void* stream) {
  if (!post || n_rollouts < 1 || policy < 0 || policy > 2) return I2C_EINVAL;
  I2C_DISPATCH(p, rollout(p, post, n_rollouts, policy, eps_x0, eps_x, eps_u, xu, z, x_final, z_term, stream));
}

// parts = 0: the lane budget chunk_geometry uses, 65536 lanes over the batch
static int eval_parts(const I2cProblem* p, const I2cRolloutEval* e) {
  if (e->parts != 0) return e->parts;
  const long want = (65536L + p->B - 1) / p->B;
  return (int)(want < e->n_rollouts ? want : e->n_rollouts);
}
// what both calls refuse from the scalar fields
static int check_eval(const I2cProblem* p, const I2cRolloutEval* e) {
  if (!e || e->n_rollouts < 1 || e->policy < 0 || e->policy > 2) return I2C_EINVAL;
  if (e->parts < 0 || e->parts > e->n_rollouts) return I2C_EINVAL;
  const int rc = check_problem_shape(p);
  if (rc != I2C_OK) return rc;
  if ((uint64_t)e->first_trajectory + (uint64_t)p->B > 0x100000000ull) return I2C_EINVAL;
  if (p->dtype != I2C_F64) return I2C_ENOTSUP;  // the sums are fp64
  return I2C_OK;
}

size_t i2c_rollout_eval_workspace(const I2cProblem* p, const I2cRolloutEval* ev, int32_t* parts_out) {
  if (check_eval(p, ev) != I2C_OK) return 0;
  I2cDims d;
  const i2c::ModelOps* ops = find_ops(p->model_id, I2C_F64);
  if (!ops) return 0;
  ops->dims(&d);
  const int parts = eval_parts(p, ev), dd = d.nx + d.nu;
  if (parts_out) *parts_out = parts;
  return (size_t)parts * (size_t)p->T * (size_t)(dd + I2C_SYM(dd)) * (size_t)p->B * 8;
}

int i2c_rollout_eval(const I2cProblem* p, const void* post, const I2cRolloutEval* ev, void* stream) {
  if (!post || !ev || !ev->cost) return I2C_EINVAL;
  if ((ev->xu_cov && !ev->xu_mean) || (ev->xu_mean && !ev->work)) return I2C_EINVAL;
  int rc = check_eval(p, ev);
  if (rc != I2C_OK) return rc;
  rc = check_problem(p);
  if (rc != I2C_OK) return rc;
  if (p->model_id >= I2C_MODEL_PLUGIN_BASE) {  // a model library from before the entry existed: its tables end above it
    const int k = p->model_id - I2C_MODEL_PLUGIN_BASE;
    std::lock_guard<std::mutex> lock(g_plugin_mutex);
    if (k >= g_n_plugins) return I2C_EINVAL;
    if (g_plugins[k].ops_bytes < offsetof(i2c::ModelOps, rollout_eval) + sizeof(void*)) return I2C_ENOTSUP;
  }
  const i2c::ModelOps* ops = find_ops(p->model_id, p->dtype);
  if (ops && p->model_params_b) ops = ops->per_traj;
  if (!ops) return I2C_EINVAL;
  return ops->rollout_eval(p, post, ev, eval_parts(p, ev), stream);
}

int i2c_riccati_sweep(const I2cProblem* p, const void* prior_out, const void* fwd, const void* xm, void* post, void* ric,
                      int32_t* status, void* stream) {
  if (!prior_out || !fwd || !xm || !post || !ric || !status) return I2C_EINVAL;
  if (p && p->inference != I2C_INF_LINEARIZE) return I2C_EINVAL;
  if (p && p->horizons) return I2C_EINVAL;  // per-trajectory horizons: the sigma-point EM path only
  I2C_DISPATCH(p, riccati(p, prior_out, fwd, xm, post, ric, status, stream));
}

int i2c_mpc_step(const I2cProblem* p, const I2cMpcStep* m, void* stream) {
  if (!m || !m->post || !m->fwd || !m->term_stats || !m->cell_init || !m->status || m->n_iter < 0) return I2C_EINVAL;
  if (m->do_filter && (!m->y || !m->u)) return I2C_EINVAL;
  if (p && p->alpha_cell && !m->alpha_init) return I2C_EINVAL;
  if (p && p->horizons) return I2C_EINVAL;  // the ring of the MPC loop has one horizon
  I2C_DISPATCH(p, mpc_step(p, m, stream));
}

int i2c_shift_horizon(const I2cProblem* p, void* post, const void* cell_init, const void* alpha_init, const void* z_new,
                      void* action, void* stream) {
  if (!post || !cell_init) return I2C_EINVAL;
  if (p && p->alpha_cell && !alpha_init) return I2C_EINVAL;
  if (p && p->horizons) return I2C_EINVAL;
  I2C_DISPATCH(p, shift(p, post, cell_init, alpha_init, z_new, action, stream));
}

int i2c_ckf_filter(const I2cProblem* p, const double* sig_zeta, const void* y, const void* u, void* mu, void* cov,
                   int32_t* status, void* stream) {
  if (!sig_zeta || !y || !u || !mu || !cov || !status) return I2C_EINVAL;
  I2C_DISPATCH(p, ckf(p, sig_zeta, y, u, mu, cov, status, stream));
}

}  // extern "C"

namespace {

// packed lower Cholesky factor of a packed symmetric n x n matrix, on the host: the plant's noise covariances are constants of a
// call, so they are factored here once and travel to the kernel as arguments. false: not positive definite.
bool chol_packed_host(const double* S, int n, double* L) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double v = S[i * (i + 1) / 2 + j];
      for (int k = 0; k < j; ++k) v -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      if (i == j) {
        if (!(v > 0.0)) return false;
        L[i * (i + 1) / 2 + i] = std::sqrt(v);
      } else {
        L[i * (i + 1) / 2 + j] = v / L[j * (j + 1) / 2 + j];
      }
    }
  return true;
}

// the table that simulates the plant of problem p, and the two noise factors (NULL in `call` where a noise is off)
struct PlantSetup {
  const i2c::ModelOps* ops;
  I2cDims d;
  double Le[I2C_SYM(I2C_MAX_NX)], Lz[I2C_SYM(I2C_MAX_NZ)];
};
// (buffers: also require the problem's device buffers -- the episode runs sweeps on them; the plant step alone reads none)
int plant_setup(const I2cProblem* p, const double* sig_zeta, bool noise_x, bool noise_y, bool buffers, PlantSetup* s) {
  const int rc = buffers ? check_problem(p) : check_problem_shape(p);
  if (rc != I2C_OK) return rc;
  s->ops = find_ops(p->model_id, p->dtype);
  if (s->ops && p->model_params_b) s->ops = s->ops->per_traj;
  if (!s->ops) return I2C_EINVAL;
  s->ops->dims(&s->d);
  if (noise_x && !chol_packed_host(p->sig_eta, s->d.nx, s->Le)) return I2C_EINVAL;
  if (noise_y && (!sig_zeta || !chol_packed_host(sig_zeta, s->d.ny, s->Lz))) return I2C_EINVAL;
  return I2C_OK;
}

}  // namespace

extern "C" {

int i2c_plant_step(const I2cProblem* p, const double* sig_zeta, void* x, const void* u, const void* eps_x, const void* eps_y,
                   void* y_out, void* x_obs, const void* z_ref, void* cost, void* stream) {
  if (!x || !u || (eps_y && !y_out)) return I2C_EINVAL;
  PlantSetup s;
  const int rc = plant_setup(p, sig_zeta, eps_x != nullptr, eps_y != nullptr, false, &s);
  if (rc != I2C_OK) return rc;
  const i2c::PlantCall k{x,       u,     eps_x,   eps_y,   y_out,   nullptr, x_obs, nullptr, z_ref,
                         cost,    nullptr, nullptr, nullptr, nullptr, eps_x ? s.Le : nullptr, eps_y ? s.Lz : nullptr};
  return s.ops->plant_step(p, &k, stream);
}

int i2c_mpc_episode(const I2cProblem* p, const I2cMpcStep* m, I2cEpisode* ep, void* stream) {
  if (!m || !m->post || !m->fwd || !m->term_stats || !m->cell_init || !m->status || !m->action || m->n_iter < 0) return I2C_EINVAL;
  if (!ep || ep->n_steps < 0 || !ep->x_true || !ep->u || !ep->cost) return I2C_EINVAL;
  if (ep->observe_state != 0 && ep->observe_state != 1) return I2C_EINVAL;
  if (!ep->observe_state && !ep->y) return I2C_EINVAL;
  if (ep->observe_state && (ep->eps_y || ep->y_hist)) return I2C_EINVAL;  // nothing is measured in that mode
  if (p && p->alpha_cell && !m->alpha_init) return I2C_EINVAL;
  if (ep->z_traj && (ep->n_z < 1 || !p || !p->z_per_cell || !p->z)) return I2C_EINVAL;
  if (p && p->horizons) return I2C_EINVAL;
  int rc = check_problem(p);
  if (rc != I2C_OK) return rc;
  const i2c::ModelOps* planner = find_ops(p->model_id, p->dtype);
  if (planner && p->model_params_b) planner = planner->per_traj;
  if (!planner) return I2C_EINVAL;
  // the plant: the planner's problem with the plants' own parameters where they are given (check_problem refuses them on a model
  // without parameters); only its model, noise, cost weights and parameters are read
  I2cProblem plant = *p;
  if (ep->plant_params_b) plant.model_params_b = ep->plant_params_b;
  PlantSetup s;
  rc = plant_setup(&plant, m->sig_zeta, ep->eps_x != nullptr, ep->eps_y != nullptr, true, &s);
  if (rc != I2C_OK) return rc;
  const size_t es = p->dtype == I2C_F32 ? 4 : 8, B = (size_t)p->B;
  auto row = [&](const void* base, long k, int n) -> const char* {
    return base ? (const char*)base + (size_t)k * (size_t)n * B * es : nullptr;
  };
  auto rowm = [&](void* base, long k, int n) -> void* { return const_cast<char*>(row(base, k, n)); };
  const int nx = s.d.nx, nu = s.d.nu, nz = s.d.nz, ny = s.d.ny;
  I2cProblem q = *p;  // the ring moves on this copy
  I2cMpcStep st = *m;
  st.y = ep->y;
  st.u = ep->u;
  ep->t0_out = q.t0;
  ep->terminal_cell_out = q.terminal_cell;
  for (int k = 0; k < ep->n_steps; ++k) {
    st.do_filter = (!ep->observe_state && k >= 1) ? 1 : 0;
    st.z_new = ep->z_traj ? row(ep->z_traj, (long)k + p->T < ep->n_z ? (long)k + p->T : ep->n_z - 1, nz) : nullptr;
    rc = planner->mpc_step(&q, &st, stream);
    if (rc != I2C_OK) return rc;
    const i2c::PlantCall c{ep->x_true,
                           m->action,
                           row(ep->eps_x, k, nx),
                           row(ep->eps_y, k, ny),
                           ep->observe_state ? nullptr : ep->y,
                           ep->u,
                           ep->observe_state ? const_cast<void*>(p->x0) : nullptr,
                           p->x0,
                           ep->z_traj ? row(ep->z_traj, k < ep->n_z ? k : ep->n_z - 1, nz) : nullptr,
                           ep->cost,
                           rowm(ep->x_hist, k, nx),
                           rowm(ep->u_hist, k, nu),
                           rowm(ep->y_hist, k, ny),
                           rowm(ep->mu_hist, k, nx),
                           ep->eps_x ? s.Le : nullptr,
                           ep->eps_y ? s.Lz : nullptr};
    rc = s.ops->plant_step(&plant, &c, stream);
    if (rc != I2C_OK) return rc;
    q.t0 = (q.t0 + 1) % q.T;
    if (q.terminal_cell >= 0) q.terminal_cell -= 1;
    ep->t0_out = q.t0;  // (kept current step by step: after a launch error the caller still knows where the ring stands)
    ep->terminal_cell_out = q.terminal_cell;
  }
  return I2C_OK;
}

}  // extern "C"
