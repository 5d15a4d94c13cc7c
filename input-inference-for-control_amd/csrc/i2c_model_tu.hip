// One translation unit per (model, dtype): compiled with
//   -DI2C_TU_MODEL=<struct in i2c_models.hpp> -DI2C_TU_REAL=<double|float> -DI2C_TU_OPS=<ops_<name>_<f64|f32|f64s>>
//   [-DI2C_TU_STORE=float]   storage type of the per-cell buffers (default: I2C_TU_REAL); f64s = double arithmetic, float storage
//   -DI2C_TU_OPS_PT=<ops_<name>_<tag>_pt> [-DI2C_TU_PER_TRAJ]   the per-trajectory-parameter table: compiled a second time with
//                               -DI2C_TU_PER_TRAJ, which builds that table instead of the shared-parameter one
// (see build.py). All kernels of the pair are instantiated here and nowhere else.
//   [-DI2C_TU_HEADER="<path>"]  an OUT-OF-TREE model: the header that defines struct I2C_TU_MODEL in namespace i2c (derived from
//                               ModelDefaults, i2c_models.hpp); `python build.py --model <path>`
#include "i2c_impl.hpp"
#ifdef I2C_TU_HEADER
#include I2C_TU_HEADER
#endif

#if !defined(I2C_TU_MODEL) || !defined(I2C_TU_REAL) || !defined(I2C_TU_OPS) || !defined(I2C_TU_OPS_PT)
#error "compile with -DI2C_TU_MODEL=... -DI2C_TU_REAL=... -DI2C_TU_OPS=... -DI2C_TU_OPS_PT=..."
#endif

namespace i2c {
#ifndef I2C_TU_STORE
#define I2C_TU_STORE I2C_TU_REAL
#endif
const ModelOps* I2C_TU_OPS_PT();
#ifdef I2C_TU_PER_TRAJ
// The per-trajectory-parameter table of the pair (Impl<PerTraj<model>>, I2cProblem.model_params_b) lives in a translation unit of its
// own: the shared-parameter kernels of the other one then compile exactly as without it (device helpers that both kernel sets call
// would otherwise be inlined differently). nullptr for a model without parameters.
const ModelOps* I2C_TU_OPS_PT() { return make_per_traj_ops<I2C_TU_MODEL, I2C_TU_REAL, I2C_TU_STORE>(); }
#else
const ModelOps* I2C_TU_OPS() { return make_ops<I2C_TU_MODEL, I2C_TU_REAL, I2C_TU_STORE>(I2C_TU_OPS_PT()); }
#endif
}  // namespace i2c
