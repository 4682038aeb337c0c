// rvo3d_capi.hip -- the C-ABI of include/rvo3d.h over the gfx950 kernels.
// Host side: handle + device buffers + launches.  No torch types, no
// exceptions across the boundary, no allocation in step/observe.
#include "../../include/rvo3d.h"
#include "rvo3d_device.hpp"
#include "rvo3d_host_setup.hpp"

#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

using rvo3d::Params;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                            \
  do {                                                                           \
    hipError_t _e = (expr);                                                      \
    if (_e != hipSuccess)                                                        \
      return fail(RVO3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// "Nothing throws" (include/rvo3d.h): every entry point that returns a status runs between these two.
// A host allocation that fails (std::vector staging in rvo3d_load_world, the error string itself) or
// any other C++ exception becomes RVO3D_ERR_INVALID instead of crossing the extern "C" boundary.
int api_caught(const char* what) noexcept {
  try {
    g_err = std::string("C++ exception: ") + what;
  } catch (...) {
    try { g_err.clear(); } catch (...) { }
  }
  return RVO3D_ERR_INVALID;
}
#define RVO3D_API_BEGIN try {
#define RVO3D_API_END                                              \
  }                                                                \
  catch (const std::exception& e) { return api_caught(e.what()); } \
  catch (...) { return api_caught("unknown"); }

using rvo3d::align_up;
using rvo3d::Pick;
using rvo3d::pick_kernel;
}  // namespace

struct rvo3d_env {
  rvo3d_config cfg;
  Params P;             // pointers into `arena`
  rvo3d::Cold cold;     // host copy of the rarely used parameters (device copy: P.cold_)
  void* arena = nullptr;
  size_t arena_bytes = 0;
  bool world_loaded = false;
  bool dv_valid = false;  // dvk_a/dvk_b describe the current state (see Params::dv_cached)
  bool g_valid = false;   // gcache describes the current state (see Params::g_cached)
  rvo3d::Geometry geo{};  // threads, blocks, LDS bytes of the step's launch
  // per-env building sets (rvo3d_set_env_buildings): one device allocation of records + cells while attached.  `cold`
  // stays the shared list's description; the device copy of Cold is whichever of the two is in force.
  void* env_bld = nullptr;
  double rmax = 0.0;  // largest drone radius of the loaded world: the reach of the building lists
  rvo3d::Cold live;   // host mirror of the device copy of Cold (the shared list's or the per-env sets', with the counts)
  // per-env drone counts (rvo3d_set_drone_counts): attached while `counted`; the device array is allocated by the first
  // attaching call and kept until rvo3d_destroy
  bool counted = false;
  int32_t* counts_dev = nullptr;
  std::vector<int32_t> counts;  // host copy of the counts in force
  rvo3d::Geometry cgeo{};       // launch geometry of the counted step
  bool ctwo_phase = false;      // Cold::cnt_two_phase while attached
  int lds_pad = 0;              // diagnostics build only: the extra LDS bytes of every step launch (0 in the product)
  // rvo3d_eval_account_safety: the scan's per-env step values, [E] doubles x 3 then [E] int32; allocated by the first
  // rvo3d_load_world and kept until rvo3d_destroy
  double* safety_scratch = nullptr;
  // rvo3d_orca_vel: the lanes' planes, [slot][6][E * N] doubles; allocated by the first call, grown by a call that needs
  // more slots (max_neighbors + max_buildings) and kept until rvo3d_destroy
  double* orca_ws = nullptr;
  size_t orca_ws_bytes = 0;
};

namespace {

// One device allocation, carved into 256-B aligned struct-of-arrays fields.
int carve(rvo3d_env* h) {
  const rvo3d_config& c = h->cfg;
  const size_t EN = (size_t)c.num_envs * c.num_drones;
  const size_t S = align_up(EN, 64);  // common element stride of every per-drone array
  Params& P = h->P;
  rvo3d::Cold& C = h->cold;
  P.S = (uint32_t)S;
  const size_t nf = Params::f64_arrays(c.max_points, c.neighbors_num);
  const size_t ni = Params::i32_arrays(c.neighbors_num, P.nw);
  struct Field { void** slot; size_t bytes; };
  std::vector<Field> f = {
      {(void**)&P.f64, nf * S * 8},
      {(void**)&P.i32, ni * S * 4},
      {(void**)&P.u8, 2 * S},
      {(void**)&C.bld, (size_t)(c.num_buildings > 0 ? c.num_buildings : 1) * 4 * 8},
      {(void**)&C.pow95, (size_t)c.max_points * 8},
      {(void**)&C.bgrid, (size_t)(C.bgx > 0 ? C.bgx * C.bgy : 1) * (rvo3d::kBgridK + 1) * 2},
      {(void**)&P.err, 256},
      {(void**)&P.cold_, sizeof(rvo3d::Cold)},
  };
  size_t total = 0;
  for (auto& x : f) total += align_up(x.bytes, 256);
  HIP_TRY(hipMalloc(&h->arena, total));
  HIP_TRY(hipMemset(h->arena, 0, total));
  h->arena_bytes = total;
  size_t off = 0;
  for (auto& x : f) {
    *x.slot = static_cast<char*>(h->arena) + off;
    off += align_up(x.bytes, 256);
  }
  HIP_TRY(hipMemcpy((void*)P.cold_, &C, sizeof C, hipMemcpyHostToDevice));  // complete by now
  h->live = C;
  return RVO3D_OK;
}

// Makes the handle's device current for the duration of one API call and puts the caller's
// device back afterwards (a single-process multi-GPU program keeps its own current device).
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  int enter(int dev) {
    hipError_t e = hipGetDevice(&prev);
    if (e == hipSuccess && prev != dev) {
      e = hipSetDevice(dev);
      changed = e == hipSuccess;
    }
    if (e != hipSuccess) return fail(RVO3D_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return RVO3D_OK;
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

int check(rvo3d_env* h, bool need_world, DeviceGuard& g) {
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (need_world && !h->world_loaded)
    return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  return g.enter(h->cfg.device);
}

template <int MODE, int NW, int NFIX, bool TRAIN, bool PAD>
void launch_inst(rvo3d_env* h, const Params& P, hipStream_t s) {
  hipLaunchKernelGGL((rvo3d::env_kernel<MODE, NW, NFIX, TRAIN, PAD>), dim3(h->geo.blocks), dim3(h->geo.threads), h->geo.lds, s, P);
}
template <int MODE, int NW, int NFIX, bool PAD>
void launch_train(rvo3d_env* h, const Params& P, hipStream_t s) {
  // both env_train modes have their instantiations (the evaluator of train/policy_test.py:46 runs env_train = False)
  if (P.env_train) launch_inst<MODE, NW, NFIX, true, PAD>(h, P, s);
  else launch_inst<MODE, NW, NFIX, false, PAD>(h, P, s);
}

// a handle with drone counts: the counted twin of the padded compile-time ring pick_counted_kernel names
template <int MODE, int NW, int NFIX>
void launch_counted(rvo3d_env* h, const Params& P, hipStream_t s) {
  const dim3 grid(h->cgeo.blocks), block(h->cgeo.threads);
  if (P.env_train) hipLaunchKernelGGL((rvo3d::env_kernel_counted<MODE, NW, NFIX, true>), grid, block, h->cgeo.lds, s, P);
  else hipLaunchKernelGGL((rvo3d::env_kernel_counted<MODE, NW, NFIX, false>), grid, block, h->cgeo.lds, s, P);
}

template <int MODE, int NW>
int launch_nw(rvo3d_env* h, const Params& P, hipStream_t s) {
  if (h->counted) {
    if constexpr (NW == 1) {
      if (rvo3d::pick_counted_kernel(P).nfix == 32) launch_counted<MODE, 1, 32>(h, P, s);
      else launch_counted<MODE, 1, 64>(h, P, s);
    } else if constexpr (NW == 2 || NW == 3 || NW == 4) {
      launch_counted<MODE, NW, 64 * NW>(h, P, s);
    } else {
      return fail(RVO3D_ERR_INVALID, "drone counts need num_drones <= 256");
    }
    HIP_TRY(hipGetLastError());
    return RVO3D_OK;
  }
  const Pick k = pick_kernel(P);
  if constexpr (NW == 1) {
    if (k.nfix == 64) { if (k.pad) launch_train<MODE, 1, 64, true>(h, P, s); else launch_train<MODE, 1, 64, false>(h, P, s); }
    else if (k.nfix == 32) { if (k.pad) launch_train<MODE, 1, 32, true>(h, P, s); else launch_train<MODE, 1, 32, false>(h, P, s); }
    else if (k.nfix == 16) launch_train<MODE, 1, 16, false>(h, P, s);
    else launch_train<MODE, 1, 0, false>(h, P, s);
  } else if constexpr (NW == 2 || NW == 3 || NW == 4) {
    launch_train<MODE, NW, 64 * NW, true>(h, P, s);
  } else {
    launch_train<MODE, NW, 0, false>(h, P, s);
  }
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
}

template <int MODE>
int launch(rvo3d_env* h, const Params& P, hipStream_t s) {
  switch (P.nw) {
    case 1: return launch_nw<MODE, 1>(h, P, s);
    case 2: return launch_nw<MODE, 2>(h, P, s);
    case 3: return launch_nw<MODE, 3>(h, P, s);
    case 4: return launch_nw<MODE, 4>(h, P, s);
    default: return launch_nw<MODE, 8>(h, P, s);
  }
}

// (only the generic kernels can need more than 64 KiB: the compile-time ones stop at 256 drones = 40 KiB)
template <int MODE, int NW>
hipError_t allow_lds(int bytes) {
  hipError_t e = hipFuncSetAttribute((const void*)rvo3d::env_kernel<MODE, NW, 0, true, false>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)rvo3d::env_kernel<MODE, NW, 0, false, false>,
                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
template <int NW>
bool allow_lds_all(int bytes) {
  return allow_lds<rvo3d::kObserve, NW>(bytes) == hipSuccess &&
         allow_lds<rvo3d::kStep, NW>(bytes) == hipSuccess &&
         allow_lds<rvo3d::kStepAutoReset, NW>(bytes) == hipSuccess;
}

}  // namespace

#ifndef RVO3D_MLP_WAVES
#define RVO3D_MLP_WAVES 8
#endif
namespace {
constexpr int kMlpWaves = RVO3D_MLP_WAVES;  // waves per workgroup of policy_mlp_kernel / policy_mlp_x3_kernel
// More than 64 KB of dynamic LDS needs the attribute, once per device (the function object is per device) and
// instantiation; a lost race between two threads sets it twice, which is harmless
template <auto Kernel>
int allow_dynamic_lds(int bytes) {
  static uint64_t attr_set = 0;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !((attr_set >> dev) & 1)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (dev >= 0 && dev < 64) attr_set |= (uint64_t)1 << dev;
  }
  return RVO3D_OK;
}
// X3: the split-bf16 (float32-class) kernel of csrc/rvo3d_policy_mlp_x3.hpp, else the bf16 one
template <bool X3, int KS1>
int launch_policy_mlp(const rvo3d::PolicyMlpArgs& A, unsigned grid, hipStream_t s) {
  constexpr auto kernel = X3 ? rvo3d::policy_mlp_x3_kernel<KS1, kMlpWaves> : rvo3d::policy_mlp_kernel<KS1, kMlpWaves>;
  constexpr int lds = X3 ? rvo3d::kX3LdsBytes : rvo3d::mlp_lds_bytes(KS1);
  if (int rc = allow_dynamic_lds<kernel>(lds)) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kMlpWaves), lds, s, A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
}
template <int H, int ND, bool X3>
int launch_policy_rnn_tiles(const rvo3d::RnnTilesArgs& A, unsigned grid, hipStream_t s) {
  // the running hidden state, 128 H bytes per wave (X3: afterwards the features' split fragments, the same size)
  constexpr int lds = rvo3d::kRnnTilesWaves * H * 128;
  if (int rc = allow_dynamic_lds<rvo3d::policy_rnn_tiles_kernel<H, ND, X3>>(lds)) return rc;
  hipLaunchKernelGGL((rvo3d::policy_rnn_tiles_kernel<H, ND, X3>), dim3(grid), dim3(64 * rvo3d::kRnnTilesWaves), lds, s, A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
}
bool rnn_tiles_shape_ok(int32_t hidden, int32_t in_dim, int32_t state_dim) {
  return (hidden == 64 || hidden == 256) && in_dim == 9 && state_dim >= 1 && state_dim <= 16;
}

// optional noise counter in device memory (rvo3d_rollout_set_step_counter): added to the `step` of every sampling launch,
// advanced by rvo3d_rollout_account - lets a caller replay a captured launch sequence (a HIP graph) with fresh noise
std::atomic<uint64_t*> g_step_dev{nullptr};

// The sampling tail's arguments as every policy-step entry point takes them, with the registered noise counter
rvo3d::PolicySampleArgs sample_args(int32_t tanh_out, const float* log_std, float std_factor, uint64_t seed, uint64_t step,
                                    int64_t rows, float* act, float* logp, float* val, float* dbg_mu, float* dbg_raw) {
  rvo3d::PolicySampleArgs S{};
  S.tanh_out = tanh_out; S.log_std = log_std; S.std_factor = std_factor; S.seed = seed; S.step = step;
  S.step_dev = g_step_dev.load();
  S.rows = rows; S.act = act; S.logp = logp; S.val = val; S.dbg_mu = dbg_mu; S.dbg_raw = dbg_raw;
  return S;
}

// The weights of an rvo3d_rnn_policy into a launch's arguments, in two parts so that each caller keeps the order of its
// checks: the reader (forward direction and LayerNorm required, the reverse direction all or nothing), then the actor's
// and the critic's stacks ([0] / [1]; also the weights of the mlp packs).
template <class Args>
int copy_reader(Args& A, const rvo3d_rnn_policy& net) {
  if (!net.w_ih_f || !net.w_hh_f || !net.b_ih_f || !net.b_hh_f || !net.ln_w || !net.ln_b)
    return fail(RVO3D_ERR_INVALID, "null reader weight");
  const bool bi = net.w_ih_r != nullptr;
  if (bi != (net.w_hh_r != nullptr) || bi != (net.b_ih_r != nullptr) || bi != (net.b_hh_r != nullptr))
    return fail(RVO3D_ERR_INVALID, "the reverse direction needs all four of w_ih_r / w_hh_r / b_ih_r / b_hh_r");
  A.w_ih[0] = net.w_ih_f; A.w_hh[0] = net.w_hh_f; A.b_ih[0] = net.b_ih_f; A.b_hh[0] = net.b_hh_f;
  A.w_ih[1] = net.w_ih_r; A.w_hh[1] = net.w_hh_r; A.b_ih[1] = net.b_ih_r; A.b_hh[1] = net.b_hh_r;
  A.ln_w = net.ln_w; A.ln_b = net.ln_b; A.eps = net.ln_eps;
  return RVO3D_OK;
}
template <class Args>
int copy_heads(Args& A, const rvo3d_mlp_weights& pi, const rvo3d_mlp_weights& v, const char* missing) {
  const rvo3d_mlp_weights* n[2] = {&pi, &v};
  for (int i = 0; i < 2; ++i) {
    if (!n[i]->w1 || !n[i]->b1 || !n[i]->w2 || !n[i]->b2 || !n[i]->w3 || !n[i]->b3)
      return fail(RVO3D_ERR_INVALID, missing);
    A.w1[i] = n[i]->w1; A.b1[i] = n[i]->b1; A.w2[i] = n[i]->w2; A.b2[i] = n[i]->b2; A.w3[i] = n[i]->w3; A.b3[i] = n[i]->b3;
  }
  return RVO3D_OK;
}

// rvo3d_policy_mlp_* (X3 = false) and rvo3d_policy_mlp_x3_* (X3 = true): the same arguments, checks and launch geometry;
// the precision picks the kernels and the blob layout.  (Called between the entry points' RVO3D_API_BEGIN / END.)
template <bool X3>
int64_t mlp_net_bytes(int ks1) { return X3 ? rvo3d::mlp_x3_net_bytes(ks1) : rvo3d::mlp_net_bytes(ks1); }

template <bool X3>
int64_t policy_mlp_blob_bytes(int32_t obs_width) {
  if (obs_width < 1 || obs_width > 126) return -1;
  return 2 * mlp_net_bytes<X3>(rvo3d::mlp_ks1(obs_width));
}

template <bool X3>
int policy_mlp_pack(const rvo3d_mlp_weights* pi, const rvo3d_mlp_weights* v, int32_t obs_width, void* blob, void* stream) {
  if (!pi || !v || !blob) return fail(RVO3D_ERR_INVALID, "null pointer");
  if (obs_width < 1 || obs_width > 126) return fail(RVO3D_ERR_INVALID, "obs_width must be 1..126");
  if (reinterpret_cast<uintptr_t>(blob) & 15) return fail(RVO3D_ERR_INVALID, "blob must be 16-byte aligned");
  rvo3d::MlpPackArgs A;
  A.k_in = obs_width; A.ks1 = rvo3d::mlp_ks1(obs_width);
  if (int rc = copy_heads(A, *pi, *v, "null weight pointer")) return rc;
  A.blob = static_cast<unsigned char*>(blob);
  hipLaunchKernelGGL(X3 ? rvo3d::mlp_x3_pack_kernel : rvo3d::mlp_pack_kernel, dim3(64, 2), dim3(256), 0,
                     static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
}

template <bool X3>
int policy_mlp_sample(const void* blob, int32_t obs_width, const float* obs, int64_t obs_ld, int64_t rows,
                      const int32_t* vo_count, int32_t state_dim, int32_t row_dim, int32_t tanh_out, const float* log_std,
                      float std_factor, uint64_t seed, uint64_t step, float* act, float* logp, float* val, float* dbg_mu,
                      float* dbg_raw, void* stream) {
  if (!blob || !obs || !log_std || !act || !logp || !val) return fail(RVO3D_ERR_INVALID, "null pointer");
  if (obs_width < 1 || obs_width > 126) return fail(RVO3D_ERR_INVALID, "obs_width must be 1..126");
  if (rows < 0 || obs_ld < obs_width) return fail(RVO3D_ERR_INVALID, "rows < 0 or obs_ld < obs_width");
  if (rows > 0 && ((rows - 1) * obs_ld + obs_width) * 4 > (int64_t)0x7fffffff)
    return fail(RVO3D_ERR_INVALID, "the observation array must stay below 2 GiB per call (32-bit buffer offsets): split the rows");
  if (reinterpret_cast<uintptr_t>(obs) & 3) return fail(RVO3D_ERR_INVALID, "obs must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(blob) & 15) return fail(RVO3D_ERR_INVALID, "blob must be 16-byte aligned");
  if (rows == 0) return RVO3D_OK;
  int dev = 0, cus = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int ks1 = rvo3d::mlp_ks1(obs_width);
  rvo3d::PolicyMlpArgs A;
  A.blob = static_cast<const unsigned char*>(blob); A.net_bytes = mlp_net_bytes<X3>(ks1);
  A.obs = obs; A.ld_obs = obs_ld; A.k_in = obs_width;
  A.cnt = vo_count; A.state_dim = state_dim; A.row_dim = row_dim;
  if (vo_count && (state_dim < 0 || row_dim < 1 || state_dim > obs_width))
    return fail(RVO3D_ERR_INVALID, "vo_count needs 0 <= state_dim <= obs_width and row_dim >= 1");
  A.S = sample_args(tanh_out, log_std, std_factor, seed, step, rows, act, logp, val, dbg_mu, dbg_raw);
  // one workgroup per CU, half of them per network; every wave takes 64 rows per trip
  const int64_t nchunks = (rows + 63) / 64;
  int64_t G = (nchunks + kMlpWaves - 1) / kMlpWaves;
  const int64_t Gmax = cus >= 2 ? cus / 2 : 1;
  if (G > Gmax) G = Gmax;
  const unsigned grid = (unsigned)(2 * G);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (ks1) {
    case 1: return launch_policy_mlp<X3, 1>(A, grid, s);
    case 2: return launch_policy_mlp<X3, 2>(A, grid, s);
    case 3: return launch_policy_mlp<X3, 3>(A, grid, s);
    case 4: return launch_policy_mlp<X3, 4>(A, grid, s);
    case 5: return launch_policy_mlp<X3, 5>(A, grid, s);
    case 6: return launch_policy_mlp<X3, 6>(A, grid, s);
    case 7: return launch_policy_mlp<X3, 7>(A, grid, s);
    default: return launch_policy_mlp<X3, 8>(A, grid, s);
  }
}

// The scalar per-drone fields of rvo3d_get_state / rvo3d_set_state in the order both copy them:
// the caller's array (null: skipped), the arena's, bytes.
struct ScalarField { const void* caller; void* arena; size_t bytes; };
std::array<ScalarField, 8> scalar_fields(const Params& P, const double* yaw, const double* pitch, const double* real_len,
                                         const double* max_dev, const double* extra_len, const int32_t* wp_idx,
                                         const uint8_t* arrive, const uint8_t* dest) {
  const size_t EN = (size_t)(P.E * P.N);
  return {{{yaw, P.yaw(), EN * 8}, {pitch, P.pitch(), EN * 8}, {real_len, P.real_len(), EN * 8},
           {max_dev, P.max_dev(), EN * 8}, {extra_len, P.extra_len(), EN * 8}, {wp_idx, P.wp_idx(), EN * 4},
           {arrive, P.arrive(), EN}, {dest, P.dest(), EN}}};
}
// rvo3d_policy_rnn_tiles* (X3 = false) and rvo3d_policy_rnn_tiles_x3* (X3 = true): the same arguments, checks (all of
// them before the first HIP call), error texts and launch geometry; the precision picks the instantiations and the blob
// layout.  (Called between the entry points' RVO3D_API_BEGIN / END.)
template <bool X3>
int64_t policy_rnn_tiles_blob_bytes(int32_t hidden, int32_t in_dim, int32_t state_dim, int32_t bidir) {
  if (!rnn_tiles_shape_ok(hidden, in_dim, state_dim)) return -1;
  return rvo3d::rnn_tiles_layout(hidden, bidir ? 2 : 1, X3).total;
}

template <bool X3>
int policy_rnn_tiles_pack(const rvo3d_rnn_policy* net, void* blob, int64_t blob_bytes, void* stream) {
  if (!net || !blob) return fail(RVO3D_ERR_INVALID, "null pointer");
  rvo3d::RnnTilesPackArgs A;
  if (int rc = copy_reader(A, *net)) return rc;
  const bool bi = net->w_ih_r != nullptr;
  if (!rnn_tiles_shape_ok(net->hidden, net->in_dim, net->state_dim))
    return fail(RVO3D_ERR_INVALID, "rnn tiles: hidden must be 64 or 256, in_dim 9, state_dim 1..16");
  if (reinterpret_cast<uintptr_t>(blob) & 15) return fail(RVO3D_ERR_INVALID, "blob must be 16-byte aligned");
  if (blob_bytes != policy_rnn_tiles_blob_bytes<X3>(net->hidden, net->in_dim, net->state_dim, bi))
    return fail(RVO3D_ERR_INVALID, "blob_bytes does not match rvo3d_policy_rnn_tiles_blob_bytes for this shape");
  if (int rc = copy_heads(A, net->pi, net->v, "null head weight")) return rc;
  A.H = net->hidden; A.ND = bi ? 2 : 1; A.SD = net->state_dim; A.IN = net->in_dim;
  A.blob = static_cast<unsigned char*>(blob);
  hipLaunchKernelGGL(rvo3d::rnn_tiles_pack_kernel<X3>, dim3(128), dim3(256), 0, static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
}

template <bool X3>
int policy_rnn_tiles(const void* blob, int64_t blob_bytes, int32_t hidden, int32_t in_dim, int32_t state_dim,
                     int32_t bidir, const float* obs, int64_t obs_ld, const int32_t* vo_count, const int32_t* list,
                     int32_t* count, int32_t* done_blocks, int32_t* work, int64_t max_rows, int32_t slots,
                     int32_t tanh_out, const float* log_std, float std_factor, uint64_t seed, uint64_t step,
                     float* act, float* logp, float* val, float* dbg_mu, void* stream) {
  if (!blob || !obs || !vo_count || !list || !count || !done_blocks || !work || !log_std || !act || !logp || !val)
    return fail(RVO3D_ERR_INVALID, "null pointer");
  if (!rnn_tiles_shape_ok(hidden, in_dim, state_dim))
    return fail(RVO3D_ERR_INVALID, "rnn tiles: hidden must be 64 or 256, in_dim 9, state_dim 1..16");
  if (slots < 1 || slots > rvo3d::kRnnTilesMaxSlots) return fail(RVO3D_ERR_INVALID, "slots must be 1..12");
  // (the two precisions' blobs differ in size for every shape: a blob of the other one is refused here)
  if (blob_bytes != policy_rnn_tiles_blob_bytes<X3>(hidden, in_dim, state_dim, bidir))
    return fail(RVO3D_ERR_INVALID, "blob_bytes does not match this shape: the blob was packed for another one");
  if (reinterpret_cast<uintptr_t>(blob) & 15) return fail(RVO3D_ERR_INVALID, "blob must be 16-byte aligned");
  if (max_rows < 1 || max_rows > 0x7fffffff) return fail(RVO3D_ERR_INVALID, "max_rows must be 1..2^31-1");
  if (obs_ld < state_dim + slots * in_dim) return fail(RVO3D_ERR_INVALID, "obs_ld < state_dim + slots * in_dim");
  int dev = 0, cus = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  rvo3d::RnnTilesArgs A;
  A.blob = static_cast<const unsigned char*>(blob);
  A.obs = obs; A.obs_ld = obs_ld; A.cnt = vo_count; A.list = list; A.count = count; A.done_blocks = done_blocks;
  A.work = work; A.max_rows = max_rows; A.SD = state_dim; A.slots = slots;
  A.S = sample_args(tanh_out, log_std, std_factor, seed, step, 0, act, logp, val, dbg_mu, nullptr);
  A.S.step_dev = nullptr;  // (never graph-replayed: the noise counter is `step` alone)
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rvo3d::rnn_tiles_bucket_kernel, dim3(256), dim3(256), 0, s, A);
  HIP_TRY(hipGetLastError());
  const unsigned grid = (unsigned)(cus > 0 ? cus : 1);  // one workgroup (four independent waves) per CU, persistent
  if (hidden == 64)
    return bidir ? launch_policy_rnn_tiles<64, 2, X3>(A, grid, s) : launch_policy_rnn_tiles<64, 1, X3>(A, grid, s);
  return bidir ? launch_policy_rnn_tiles<256, 2, X3>(A, grid, s) : launch_policy_rnn_tiles<256, 1, X3>(A, grid, s);
}
}  // namespace

extern "C" {

int rvo3d_version(void) { return RVO3D_VERSION; }
const char* rvo3d_last_error(void) { return g_err.c_str(); }

int rvo3d_create(const rvo3d_config* cfg, rvo3d_env** out) {
  RVO3D_API_BEGIN
  if (!cfg || !out) return fail(RVO3D_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->num_envs < 1 || cfg->num_drones < 1 || cfg->num_drones > rvo3d::kMaxThreads)
    return fail(RVO3D_ERR_INVALID, "need num_envs >= 1 and 1 <= num_drones <= 512");
  if (cfg->max_points < 2 || cfg->num_buildings < 0 || cfg->neighbors_num < 0)
    return fail(RVO3D_ERR_INVALID, "need max_points >= 2, num_buildings >= 0, neighbors_num >= 0");
  if ((long long)cfg->num_envs * cfg->num_drones > (1ll << 30))
    return fail(RVO3D_ERR_INVALID, "num_envs * num_drones too large");
  if (cfg->action_decimals > 9) return fail(RVO3D_ERR_INVALID, "action_decimals must be <= 9");
  DeviceGuard dg;
  if (int rc0 = dg.enter(cfg->device)) return rc0;

  rvo3d_env* h = new (std::nothrow) rvo3d_env();
  if (!h) return fail(RVO3D_ERR_INVALID, "out of host memory");
  // owns h until the very end: every early return - and an exception - frees the handle and its arena
  struct Owner {
    rvo3d_env* p;
    ~Owner() {
      if (!p) return;
      if (p->arena) (void)hipFree(p->arena);
      delete p;
    }
  } owner{h};
  h->cfg = *cfg;
  Params& P = h->P;
  int lds_pad = 0;
#ifdef RVO3D_DIAG
  if (const char* pad = std::getenv("RVO3D_LDS_PAD")) lds_pad = std::atoi(pad);  // diagnostics build only: cap occupancy
#endif
  std::string err;
  h->lds_pad = lds_pad;
  if (int rc = rvo3d::plan_env(cfg, lds_pad, P, h->cold, h->geo, err)) return fail(rc, err);
#ifdef RVO3D_DIAG
  if (const char* ab = std::getenv("RVO3D_ABLATE")) P.ablate = std::atoi(ab);  // diagnostics build only
#endif
  if (h->geo.lds > 64 * 1024) {
    const bool ok = P.nw == 1 ? allow_lds_all<1>(h->geo.lds) : (P.nw == 8 && allow_lds_all<8>(h->geo.lds));
    if (!ok) {
      return fail(RVO3D_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    }
  }
  int rc = carve(h);
  if (rc != RVO3D_OK) return rc;
  owner.p = nullptr;
  *out = h;
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_destroy(rvo3d_env* h) {
  RVO3D_API_BEGIN
  if (!h) return RVO3D_OK;
  DeviceGuard dg;
  (void)dg.enter(h->cfg.device);
  (void)hipDeviceSynchronize();
  if (h->env_bld) (void)hipFree(h->env_bld);
  if (h->counts_dev) (void)hipFree(h->counts_dev);
  if (h->safety_scratch) (void)hipFree(h->safety_scratch);
  if (h->orca_ws) (void)hipFree(h->orca_ws);
  if (h->arena) (void)hipFree(h->arena);
  delete h;
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_load_world(rvo3d_env* h, const double* waypoints, const int32_t* n_points,
                     const double* buildings, const double* radius, const double* priority,
                     void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, false, dg);
  if (rc) return rc;
  if (!waypoints || !n_points) return fail(RVO3D_ERR_INVALID, "waypoints / n_points are required");
  const Params& P = h->P;
  const rvo3d::Cold& C = h->cold;
  if (C.nb > 0 && !buildings) return fail(RVO3D_ERR_INVALID, "buildings required when num_buildings > 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t EN = (size_t)P.E * P.N;
  rvo3d::StagedWorld w;
  std::string err;
  if (int rc2 = rvo3d::stage_world(h->P, waypoints, n_points, radius, priority, w, err)) return fail(rc2, err);
  if (!h->safety_scratch) HIP_TRY(hipMalloc((void**)&h->safety_scratch, align_up((size_t)P.E * (3 * 8 + 4), 256)));
  // a new world drops per-env building sets and drone counts: the shared list and full envs are in force again (the
  // sets' allocation goes at the end)
  if (h->env_bld || h->counted) HIP_TRY(hipMemcpyAsync((void*)P.cold_, &C, sizeof C, hipMemcpyHostToDevice, s));
  // [P][3] rows of EN doubles into arrays of stride S
  HIP_TRY(hipMemcpy2DAsync((void*)P.wp(0, 0), (size_t)P.S * 8, w.wp.data(), EN * 8, EN * 8,
                           (size_t)P.P * 3, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync((void*)P.n_points(), n_points, EN * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync((void*)P.route_len(), w.rl.data(), EN * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync((void*)P.radius(), w.rad.data(), EN * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync((void*)P.prio(), w.pri.data(), EN * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync((void*)C.pow95, w.p95.data(), (size_t)P.P * 8, hipMemcpyHostToDevice, s));
  std::vector<uint16_t> grid;
  if (C.nb > 0) {
    HIP_TRY(hipMemcpyAsync((void*)C.bld, buildings, (size_t)C.nb * 32, hipMemcpyHostToDevice, s));
    if (C.bgx > 0) {
      grid = rvo3d::build_building_grid(C, buildings, w.rad);
      HIP_TRY(hipMemcpyAsync((void*)C.bgrid, grid.data(), grid.size() * 2, hipMemcpyHostToDevice, s));
    }
  }
  HIP_TRY(hipMemsetAsync(P.extra_len(), 0, EN * 8, s));
  const int tb = 256;
  hipLaunchKernelGGL(rvo3d::dv0_kernel, dim3((unsigned)((EN + tb - 1) / tb)), dim3(tb), 0, s, P);
  hipLaunchKernelGGL(rvo3d::reset_kernel, dim3((unsigned)((EN + tb - 1) / tb)), dim3(tb), 0, s, P,
                     (const uint8_t*)nullptr, (const uint8_t*)nullptr);
  hipLaunchKernelGGL(rvo3d::wpcache_kernel, dim3((unsigned)((EN + tb - 1) / tb)), dim3(tb), 0, s, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));  // the host staging vectors die here
  if (h->env_bld) {
    (void)hipFree(h->env_bld);
    h->env_bld = nullptr;
  }
  h->live = C;
  h->counted = false;
  h->counts.clear();
  h->rmax = rvo3d::largest_radius(w.rad);
  h->world_loaded = true;
  h->dv_valid = true;  // reset_kernel filed the des_vel of every start state
  h->g_valid = false;
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_set_env_buildings(rvo3d_env* h, const double* buildings, const int32_t* counts, int32_t nb_max, void* stream) {
  RVO3D_API_BEGIN
  // every argument check, and all of the host's work, before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  const Params& P = h->P;
  bool detach = false;
  std::string err;
  if (int rc = rvo3d::check_env_buildings(P.E, buildings, counts, nb_max, detach, err)) return fail(rc, err);
  rvo3d::Cold C = h->cold;  // the shared list's; attached: nb_max records and a grid of its own per env
  rvo3d::StagedEnvBuildings w;
  size_t bld_bytes = 0, grid_bytes = 0;
  if (!detach) {
    rvo3d::env_grid_dims(&h->cfg, P.E, rvo3d::kEnvGridBudget, C);
    C.nb = nb_max;
    rvo3d::stage_env_buildings(C, P.E, buildings, counts, nb_max, h->rmax, w);
    bld_bytes = align_up(w.bld.size() * 8, 256);
    grid_bytes = w.grid.size() * 2;
    C.bld_stride = (uint32_t)nb_max * 4u;
    C.bgrid_stride = (uint32_t)((size_t)C.bgx * C.bgy * (rvo3d::kBgridK + 1));
  }
  C.counts = h->live.counts; C.cnt_two_phase = h->live.cnt_two_phase;  // drone counts stay as they are
  DeviceGuard dg;
  if (int rc = dg.enter(h->cfg.device)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  void* buf = nullptr;
  if (!detach) {
    HIP_TRY(hipMalloc(&buf, bld_bytes + (grid_bytes ? grid_bytes : 256)));
    C.bld = static_cast<const double*>(buf);
    C.bgrid = reinterpret_cast<const uint16_t*>(static_cast<char*>(buf) + bld_bytes);
  }
  // in stream order behind the steps already enqueued; the old sets are freed once nothing reads them
  hipError_t e = hipSuccess;
  if (!detach) e = hipMemcpyAsync(buf, w.bld.data(), w.bld.size() * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && grid_bytes)
    e = hipMemcpyAsync(static_cast<char*>(buf) + bld_bytes, w.grid.data(), grid_bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync((void*)P.cold_, &C, sizeof C, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host staging dies here
  if (e != hipSuccess) {
    if (buf) (void)hipFree(buf);
    return fail(RVO3D_ERR_HIP, std::string("rvo3d_set_env_buildings: ") + hipGetErrorString(e));
  }
  if (h->env_bld) (void)hipFree(h->env_bld);
  h->env_bld = buf;
  h->live = C;
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_move_env_buildings(rvo3d_env* h, const rvo3d_building_motion* m, double dt, const uint8_t* env_mask,
                             double* buildings_out, void* stream) {
  RVO3D_API_BEGIN
  // every argument check before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  std::string err;
  if (int rc = rvo3d::check_move_env_buildings(h->world_loaded, h->env_bld != nullptr, m, dt, err)) return fail(rc, err);
  DeviceGuard dg;
  if (int rc = dg.enter(h->cfg.device)) return rc;
  const rvo3d::Cold& C = h->live;  // the sets': records and cells inside the handle's env_bld allocation
  if (C.nb == 0) return RVO3D_OK;
  const rvo3d::MotionArgs A{const_cast<double*>(C.bld), const_cast<uint16_t*>(C.bgrid), C.bld_stride, C.bgrid_stride,
                            C.nb, C.bgx, C.bgy, C.bg_inv, h->rmax, dt, m->ends, m->speed, m->leg, env_mask, buildings_out};
  hipLaunchKernelGGL(rvo3d::move_buildings_kernel, dim3((unsigned)h->P.E), dim3(rvo3d::kMotionThreads), 0,
                     static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_set_drone_counts(rvo3d_env* h, const int32_t* counts, void* stream) {
  RVO3D_API_BEGIN
  // every argument check, and all of the host's work, before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  const Params& P = h->P;
  bool detach = false;
  std::string err;
  if (int rc = rvo3d::check_drone_counts(P.E, P.N, counts, detach, err)) return fail(rc, err);
  if (detach && !h->counted) return RVO3D_OK;  // full envs already
  rvo3d::Geometry cgeo{};
  bool two_phase = false;
  if (!detach)
    if (int rc = rvo3d::counted_geometry(h->lds_pad, P, h->geo, cgeo, two_phase, err)) return fail(rc, err);
  // the envs whose count changes (no counts: every env has N drones)
  std::vector<int32_t> now(counts ? counts : nullptr, counts ? counts + P.E : nullptr);
  std::vector<uint8_t> changed((size_t)P.E, 0);
  bool any = false;
  for (int e = 0; e < P.E; ++e) {
    const int32_t was = h->counted ? h->counts[(size_t)e] : P.N, is = detach ? P.N : counts[e];
    changed[(size_t)e] = was != is;
    any = any || was != is;
  }
  rvo3d::Cold C = h->live;
  DeviceGuard dg;
  if (int rc = dg.enter(h->cfg.device)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t* cdev = h->counts_dev;
  if (!detach && !cdev) HIP_TRY(hipMalloc((void**)&cdev, align_up((size_t)P.E * 4, 256)));
  uint8_t* mask = nullptr;
  if (any && hipMalloc((void**)&mask, (size_t)P.E) != hipSuccess) {
    if (cdev != h->counts_dev) (void)hipFree(cdev);
    return fail(RVO3D_ERR_HIP, "rvo3d_set_drone_counts: hipMalloc failed");
  }
  C.counts = detach ? nullptr : cdev;
  C.cnt_two_phase = (!detach && two_phase) ? 1 : 0;
  // in stream order behind the steps already enqueued: the counts, the parameters, then the reset of the changed envs
  hipError_t e = hipSuccess;
  if (!detach) e = hipMemcpyAsync(cdev, counts, (size_t)P.E * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync((void*)P.cold_, &C, sizeof C, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && any) e = hipMemcpyAsync(mask, changed.data(), (size_t)P.E, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && any) {
    const size_t EN = (size_t)P.E * P.N;
    hipLaunchKernelGGL(rvo3d::reset_fresh_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, s, P,
                       (const uint8_t*)mask);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the host staging and the mask die here
  if (mask) (void)hipFree(mask);
  h->counts_dev = cdev;  // (kept for the next attaching call, whatever became of this one)
  if (e != hipSuccess) {
    // the device copy of Cold may be the new one already: put back what the handle goes on describing (and the old
    // counts, which share the array), so that host and device agree again - as far as a failing device lets us
    if (h->counted) (void)hipMemcpy(cdev, h->counts.data(), (size_t)P.E * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy((void*)P.cold_, &h->live, sizeof h->live, hipMemcpyHostToDevice);
    h->g_valid = h->dv_valid = false;  // some envs may have been reset
    return fail(RVO3D_ERR_HIP, std::string("rvo3d_set_drone_counts: ") + hipGetErrorString(e));
  }
  h->live = C;
  h->counted = !detach;
  h->counts.swap(now);
  h->cgeo = cgeo;
  h->ctwo_phase = two_phase;
  // the stage-G words on file belong to the ring that wrote them, and to the positions before the resets; the des_vel
  // words of a reset env are its reset state's (reset_drone)
  h->g_valid = false;
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_drone_counts(rvo3d_env* h, const int32_t** device_counts) {
  RVO3D_API_BEGIN
  if (!h || !device_counts) return fail(RVO3D_ERR_INVALID, "null argument");
  *device_counts = h->counted ? h->counts_dev : nullptr;
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_set_routes(rvo3d_env* h, const uint8_t* env_mask, const double* waypoints, const int32_t* n_points,
                     void* stream) {
  RVO3D_API_BEGIN
  // every argument check before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!waypoints) return fail(RVO3D_ERR_INVALID, "waypoints is required");
  if (!n_points) return fail(RVO3D_ERR_INVALID, "n_points is required");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  DeviceGuard dg;
  if (int rc = dg.enter(h->cfg.device)) return rc;
  const Params& P = h->P;
  // one workgroup per env: it votes on the env's n_points before its first store
  hipLaunchKernelGGL(h->counted ? rvo3d::set_routes_counted_kernel : rvo3d::set_routes_kernel, dim3((unsigned)P.E),
                     dim3((unsigned)align_up((size_t)P.N, 64)), 0, static_cast<hipStream_t>(stream), P, env_mask, waypoints,
                     n_points);
  HIP_TRY(hipGetLastError());
  h->g_valid = false;  // positions change: the stage-G words on file are stale (the des_vel on file is the reset state's)
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_get_routes(rvo3d_env* h, double* waypoints, int32_t* n_points, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const Params& P = h->P;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t EN = (size_t)P.E * P.N;
  if (waypoints) {
    hipLaunchKernelGGL(rvo3d::get_routes_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, s, P, waypoints);
    HIP_TRY(hipGetLastError());
  }
  if (n_points) HIP_TRY(hipMemcpyAsync(n_points, P.n_points(), EN * 4, hipMemcpyDeviceToDevice, s));
  return RVO3D_OK;
  RVO3D_API_END
}

}  // extern "C"

namespace {

// the argument checks of the two samplers and of the planner that do not concern a config struct
int check_route_shape(const double* waypoints, const int32_t* n_points, int32_t num_envs, int32_t num_drones,
                      int32_t max_points) {
  if (!waypoints) return fail(RVO3D_ERR_INVALID, "waypoints is required");
  if (!n_points) return fail(RVO3D_ERR_INVALID, "n_points is required");
  if (num_envs < 1 || num_drones < 1 || num_drones > rvo3d::kMaxThreads)
    return fail(RVO3D_ERR_INVALID, "need num_envs >= 1 and 1 <= num_drones <= 512");
  if (max_points < 2) return fail(RVO3D_ERR_INVALID, "need max_points >= 2");
  return RVO3D_OK;
}

rvo3d::CityArgs city_args(const rvo3d_city& c) {
  rvo3d::CityArgs a;
  a.bld = c.nb_max > 0 ? c.buildings : nullptr;
  a.counts = c.counts; a.stride = c.env_stride; a.nb_max = c.nb_max;
  a.clear_xy = c.clear_xy; a.clear_z = c.clear_z; a.pad = c.pad;
  return a;
}

// LDS bytes of an env's staged building records
size_t city_lds_bytes(const rvo3d_city& c) {
  return (size_t)(c.nb_max < rvo3d::kCityLdsCap ? c.nb_max : rvo3d::kCityLdsCap) * 4 * sizeof(double);
}

// rvo3d_sample_routes and rvo3d_sample_routes_city (with_city): one set of checks, one launch
int sample_routes(const rvo3d_route_sampler* cfg, bool with_city, const rvo3d_city* city, int32_t num_envs,
                  int32_t num_drones, int32_t max_points, uint32_t draw, const uint8_t* env_mask, double* waypoints,
                  int32_t* n_points, int32_t* unplaced, void* stream) {
  // every argument check before the first HIP call
  if (!cfg) return fail(RVO3D_ERR_INVALID, "cfg is required");
  if (int rc = check_route_shape(waypoints, n_points, num_envs, num_drones, max_points)) return rc;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(cfg->lo[k]) || !std::isfinite(cfg->hi[k]) || !(cfg->lo[k] < cfg->hi[k]))
      return fail(RVO3D_ERR_INVALID, "lo / hi must be finite with lo < hi on every axis");
  if (!(cfg->min_sep >= 0.0) || !(cfg->min_len >= 0.0)) return fail(RVO3D_ERR_INVALID, "min_sep and min_len must be >= 0");
  if (cfg->max_tries < 1 || cfg->max_tries > 1024) return fail(RVO3D_ERR_INVALID, "max_tries must be 1..1024");
  if (with_city) {
    std::string err;
    if (int rc = rvo3d::check_city(city, err)) return fail(rc, err);
  }
  rvo3d::SampleRoutesArgs A;
  for (int k = 0; k < 3; ++k) {
    A.lo[k] = cfg->lo[k];
    A.span[k] = cfg->hi[k] - cfg->lo[k];
  }
  A.sep2 = cfg->min_sep * cfg->min_sep; A.len2 = cfg->min_len * cfg->min_len;
  A.max_tries = cfg->max_tries; A.N = num_drones; A.P = max_points;
  A.draw = draw; A.k0 = (uint32_t)cfg->seed; A.k1 = (uint32_t)(cfg->seed >> 32);
  A.env_offset = cfg->env_offset;
  A.env_mask = env_mask; A.wp = waypoints; A.n_points = n_points; A.unplaced = unplaced;
  // one workgroup per env, one lane per drone; LDS: one point per lane and the round's unplaced flags
  const size_t T = align_up((size_t)num_drones, 64);
  const size_t lds = T * (3 * sizeof(double) + 1);
  if (with_city)  // ... and the env's building records between the two
    hipLaunchKernelGGL(rvo3d::sample_routes_city_kernel, dim3((unsigned)num_envs), dim3((unsigned)T),
                       lds + city_lds_bytes(*city), static_cast<hipStream_t>(stream), A, city_args(*city));
  else
    hipLaunchKernelGGL(rvo3d::sample_routes_kernel, dim3((unsigned)num_envs), dim3((unsigned)T), lds,
                       static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
}

}  // namespace

extern "C" {

int rvo3d_sample_routes(const rvo3d_route_sampler* cfg, int32_t num_envs, int32_t num_drones, int32_t max_points,
                        uint32_t draw, const uint8_t* env_mask, double* waypoints, int32_t* n_points, int32_t* unplaced,
                        void* stream) {
  RVO3D_API_BEGIN
  return sample_routes(cfg, false, nullptr, num_envs, num_drones, max_points, draw, env_mask, waypoints, n_points,
                       unplaced, stream);
  RVO3D_API_END
}

int rvo3d_sample_routes_city(const rvo3d_route_sampler* cfg, const rvo3d_city* city, int32_t num_envs, int32_t num_drones,
                             int32_t max_points, uint32_t draw, const uint8_t* env_mask, double* waypoints,
                             int32_t* n_points, int32_t* unplaced, void* stream) {
  RVO3D_API_BEGIN
  return sample_routes(cfg, true, city, num_envs, num_drones, max_points, draw, env_mask, waypoints, n_points, unplaced,
                       stream);
  RVO3D_API_END
}

int rvo3d_plan_routes(const rvo3d_city* city, int32_t num_envs, int32_t num_drones, int32_t max_points,
                      const uint8_t* env_mask, double* waypoints, int32_t* n_points, int32_t* blocked,
                      uint8_t* blocked_mask, void* stream) {
  RVO3D_API_BEGIN
  // every argument check before the first HIP call
  std::string err;
  if (int rc = rvo3d::check_city(city, err)) return fail(rc, err);
  if (int rc = check_route_shape(waypoints, n_points, num_envs, num_drones, max_points)) return rc;
  rvo3d::PlanRoutesArgs A;
  A.city = city_args(*city);
  A.N = num_drones; A.P = max_points;
  A.env_mask = env_mask; A.wp = waypoints; A.n_points = n_points; A.blocked = blocked; A.blocked_mask = blocked_mask;
  // one workgroup per env, one lane per drone; LDS: the env's building records
  const dim3 grid((unsigned)num_envs), block((unsigned)align_up((size_t)num_drones, 64));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (max_points <= rvo3d::kPlanPrivatePoints)
    hipLaunchKernelGGL(rvo3d::plan_routes_kernel<true>, grid, block, city_lds_bytes(*city), s, A);
  else
    hipLaunchKernelGGL(rvo3d::plan_routes_kernel<false>, grid, block, city_lds_bytes(*city), s, A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_reset(rvo3d_env* h, const uint8_t* env_mask, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const size_t EN = (size_t)h->P.E * h->P.N;
  h->g_valid = false;  // positions change: the stage-G words on file are stale
  hipLaunchKernelGGL(rvo3d::reset_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h->P, env_mask, (const uint8_t*)nullptr);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_reset_drones(rvo3d_env* h, const uint8_t* drone_mask, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  if (!drone_mask) return fail(RVO3D_ERR_INVALID, "drone_mask is required");
  const size_t EN = (size_t)h->P.E * h->P.N;
  h->g_valid = false;
  hipLaunchKernelGGL(rvo3d::reset_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h->P, (const uint8_t*)nullptr, drone_mask);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

// The observation launch of rvo3d_observe and rvo3d_observe_envs (the device is current, the pointers are checked).
static int observe_launch(rvo3d_env* h, float* obs, int32_t* vo_count, void* stream) {
  Params P = h->P;
  P.obs = obs; P.vo_count = vo_count;
  P.zf16 = (h->cold.zf_q != 0 && (reinterpret_cast<uintptr_t>(obs) & 15) == 0 && P.nm > 0) ? 1 : 0;
  const int rc = launch<rvo3d::kObserve>(h, P, static_cast<hipStream_t>(stream));
  if (rc == RVO3D_OK) h->dv_valid = h->g_valid = true;  // observe files des_vel and the stage-G words
  return rc;
}

int rvo3d_observe(rvo3d_env* h, float* obs, int32_t* vo_count, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  if (!obs || !vo_count) return fail(RVO3D_ERR_INVALID, "obs / vo_count are required");
  return observe_launch(h, obs, vo_count, stream);
  RVO3D_API_END
}

int rvo3d_observe_envs(rvo3d_env* h, const uint8_t* env_mask, float* obs, int32_t* vo_count, float* scratch_obs,
                       int32_t* scratch_cnt, void* stream) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!env_mask || !obs || !vo_count || !scratch_obs || !scratch_cnt)
    return fail(RVO3D_ERR_INVALID, "env_mask / obs / vo_count / scratch_obs / scratch_cnt are required");
  if (scratch_obs == obs || scratch_cnt == vo_count)
    return fail(RVO3D_ERR_INVALID, "the scratch pair must be storage of its own");
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  rc = observe_launch(h, scratch_obs, scratch_cnt, stream);
  if (rc) return rc;
  const Params& P = h->P;
  const unsigned threads = (int64_t)P.N * P.W <= 256 ? 64u : 256u;
  hipLaunchKernelGGL(rvo3d::observe_select_kernel, dim3((unsigned)P.E), dim3(threads), 0, static_cast<hipStream_t>(stream),
                     P.N, P.W, env_mask, reinterpret_cast<const uint32_t*>(scratch_obs), scratch_cnt,
                     reinterpret_cast<uint32_t*>(obs), vo_count);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

// The one implementation behind the four step entry points (called between their RVO3D_API_BEGIN / END).  Policy
// mode lives in the per-call Params copy alone: of h it writes nothing but the two cache flags.
static int step_impl(rvo3d_env* h, const rvo3d_step_args& a, void* stream) {
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  if (!a.actions || !a.obs || !a.vo_count || !a.reward || !a.done || !a.info || !a.finish)
    return fail(RVO3D_ERR_INVALID, "null I/O pointer");
  const int32_t action_dtype = a.policy ? RVO3D_F32 : a.action_dtype;
  if (action_dtype != RVO3D_F32 && action_dtype != RVO3D_F64)
    return fail(RVO3D_ERR_INVALID, "action_dtype must be RVO3D_F32 or RVO3D_F64");
  Params P = h->P;
  P.action_mode = a.policy ? 1 : 0;
  P.acceler = a.acceler;
  P.actions = a.actions; P.action_f64 = action_dtype == RVO3D_F64;
  P.obs = a.obs; P.vo_count = a.vo_count; P.reward = a.reward;
  P.zf16 = (h->cold.zf_q != 0 && (reinterpret_cast<uintptr_t>(a.obs) & 15) == 0 && P.nm > 0) ? 1 : 0;
  P.done = a.done; P.info = a.info; P.finish = a.finish;
  // the absolute step hands out a reset mask only with auto-reset; the policy step takes it as given
  P.reset_mask = (a.policy || a.autoreset) ? a.reset_mask : nullptr;
  P.prev_cnt = a.prev_vo_count;  // (h->P's is always null: nothing of it outlives the call)
  P.dv_cached = h->dv_valid ? 1 : 0;
  P.g_cached = h->g_valid ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = a.autoreset ? launch<rvo3d::kStepAutoReset>(h, P, s) : launch<rvo3d::kStep>(h, P, s);
  if (rc == RVO3D_OK) h->dv_valid = h->g_valid = true;  // every step files both for the state it ends in
  return rc;
}

int rvo3d_step(rvo3d_env* h, const void* actions, int32_t action_dtype, float* obs,
               int32_t* vo_count, float* reward, uint8_t* done, uint8_t* info, uint8_t* finish,
               void* stream) {
  RVO3D_API_BEGIN
  rvo3d_step_args a{};
  a.actions = actions; a.action_dtype = action_dtype;
  a.obs = obs; a.vo_count = vo_count; a.reward = reward; a.done = done; a.info = info; a.finish = finish;
  return step_impl(h, a, stream);
  RVO3D_API_END
}

int rvo3d_step_policy(rvo3d_env* h, const float* a_inc, float acceler, float* obs,
                      int32_t* vo_count, float* reward, uint8_t* done, uint8_t* info,
                      uint8_t* finish, uint8_t* reset_mask, int32_t autoreset, void* stream) {
  RVO3D_API_BEGIN
  rvo3d_step_args a{};
  a.actions = a_inc; a.policy = 1; a.acceler = acceler; a.autoreset = autoreset;
  a.obs = obs; a.vo_count = vo_count; a.reward = reward; a.done = done; a.info = info; a.finish = finish;
  a.reset_mask = reset_mask;
  return step_impl(h, a, stream);
  RVO3D_API_END
}

int rvo3d_step_autoreset(rvo3d_env* h, const void* actions, int32_t action_dtype, float* obs,
                         int32_t* vo_count, float* reward, uint8_t* done, uint8_t* info,
                         uint8_t* finish, uint8_t* reset_mask, void* stream) {
  RVO3D_API_BEGIN
  rvo3d_step_args a{};
  a.actions = actions; a.action_dtype = action_dtype; a.autoreset = 1;
  a.obs = obs; a.vo_count = vo_count; a.reward = reward; a.done = done; a.info = info; a.finish = finish;
  a.reset_mask = reset_mask;
  return step_impl(h, a, stream);
  RVO3D_API_END
}

int rvo3d_step_ex(rvo3d_env* h, const rvo3d_step_args* a, void* stream) {
  RVO3D_API_BEGIN
  if (!a) return fail(RVO3D_ERR_INVALID, "null argument");
  return step_impl(h, *a, stream);
  RVO3D_API_END
}

int rvo3d_policy_sample(const rvo3d_policy_heads* hd, int64_t rows, float std_factor, uint64_t seed,
                        uint64_t step, float* act, float* logp, float* val, float* dbg_mu, float* dbg_raw,
                        void* stream) {
  RVO3D_API_BEGIN
  if (!hd || !hd->h_pi || !hd->h_v || !hd->log_std || !act || !logp || !val)
    return fail(RVO3D_ERR_INVALID, "null pointer");
  if (rows < 0) return fail(RVO3D_ERR_INVALID, "rows < 0");
  if (rows == 0) return RVO3D_OK;
  rvo3d::PolicySampleArgs A = sample_args(hd->hidden == 0 ? 0 : hd->tanh_out,  // (mu given: already activated)
                                          hd->log_std, std_factor, seed, step, rows, act, logp, val, dbg_mu, dbg_raw);
  A.h_pi = hd->h_pi; A.h_v = hd->h_v; A.ld_pi = hd->ld_pi; A.ld_v = hd->ld_v; A.hidden = hd->hidden;
  A.w_pi = hd->w_pi; A.b_pi = hd->b_pi; A.w_v = hd->w_v; A.b_v = hd->b_v;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hd->hidden == 0) {
    if (hd->ld_pi < 3 || hd->ld_v < 1) return fail(RVO3D_ERR_INVALID, "hidden == 0 needs ld_pi >= 3 and ld_v >= 1");
    hipLaunchKernelGGL(rvo3d::policy_sample_direct_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, A);
  } else {
    if (!hd->w_pi || !hd->b_pi || !hd->w_v || !hd->b_v) return fail(RVO3D_ERR_INVALID, "head weights are required");
    const bool bf = hd->dtype == RVO3D_BF16;
    if (!bf && hd->dtype != RVO3D_F32) return fail(RVO3D_ERR_INVALID, "dtype must be RVO3D_F32 or RVO3D_BF16");
    const int per_chunk = bf ? 256 : 128;  // 32 lanes x 16 bytes
    const int nch = hd->hidden / per_chunk;
    if (hd->hidden % per_chunk != 0 || (nch != 1 && nch != 2 && nch != 4 && nch != 8) || hd->hidden > 1024)
      return fail(RVO3D_ERR_INVALID, "hidden must be 128 / 256 / 512 / 1024 (float32) or 256 / 512 / 1024 (bfloat16)");
    const size_t es = bf ? 2 : 4;
    if (hd->ld_pi < hd->hidden || hd->ld_v < hd->hidden || (hd->ld_pi * es) % 16 || (hd->ld_v * es) % 16 ||
        (reinterpret_cast<uintptr_t>(hd->h_pi) & 15) || (reinterpret_cast<uintptr_t>(hd->h_v) & 15))
      return fail(RVO3D_ERR_INVALID, "hidden activations must be 16-byte aligned rows of at least `hidden` elements");
    const dim3 grid((unsigned)((rows + 127) / 128)), blk(256);  // 4 waves x 32 rows
#define RVO3D_PS(T, N) hipLaunchKernelGGL((rvo3d::policy_sample_kernel<T, N>), grid, blk, 0, s, A)
    if (bf) {
      if (nch == 1) RVO3D_PS(rvo3d::bf16_t, 1); else if (nch == 2) RVO3D_PS(rvo3d::bf16_t, 2); else RVO3D_PS(rvo3d::bf16_t, 4);
    } else {
      if (nch == 1) RVO3D_PS(float, 1); else if (nch == 2) RVO3D_PS(float, 2); else if (nch == 4) RVO3D_PS(float, 4); else RVO3D_PS(float, 8);
    }
#undef RVO3D_PS
  }
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int64_t rvo3d_policy_mlp_blob_bytes(int32_t obs_width) { return policy_mlp_blob_bytes<false>(obs_width); }

int rvo3d_policy_mlp_pack(const rvo3d_mlp_weights* pi, const rvo3d_mlp_weights* v, int32_t obs_width, void* blob,
                          void* stream) {
  RVO3D_API_BEGIN
  return policy_mlp_pack<false>(pi, v, obs_width, blob, stream);
  RVO3D_API_END
}

int rvo3d_policy_mlp_sample(const void* blob, int32_t obs_width, const float* obs, int64_t obs_ld, int64_t rows,
                            const int32_t* vo_count, int32_t state_dim, int32_t row_dim, int32_t tanh_out, const float* log_std, float std_factor, uint64_t seed, uint64_t step,
                            float* act, float* logp, float* val, float* dbg_mu, float* dbg_raw, void* stream) {
  RVO3D_API_BEGIN
  return policy_mlp_sample<false>(blob, obs_width, obs, obs_ld, rows, vo_count, state_dim, row_dim, tanh_out, log_std,
                                  std_factor, seed, step, act, logp, val, dbg_mu, dbg_raw, stream);
  RVO3D_API_END
}

// The float32-class twin of the trio above (train/policy/policy_rnn_ac.py:57-69, :197-257, float32): every product of
// the three layers is a_hi b_hi + a_lo b_hi + a_hi b_lo of bf16 halves (hi = bf16_rne(x), lo = bf16_rne(x - hi)) with
// float32 accumulation; the first layer's bias as hi and lo against an exact 1, b2 and the head biases in float32, ReLU
// on the float32 sums before the split; the per-row tail, the noise, vo_count and the range-checked observation reads
// are those of rvo3d_policy_mlp_sample.  Same arguments and checks.
int64_t rvo3d_policy_mlp_x3_blob_bytes(int32_t obs_width) { return policy_mlp_blob_bytes<true>(obs_width); }

int rvo3d_policy_mlp_x3_pack(const rvo3d_mlp_weights* pi, const rvo3d_mlp_weights* v, int32_t obs_width, void* blob,
                             void* stream) {
  RVO3D_API_BEGIN
  return policy_mlp_pack<true>(pi, v, obs_width, blob, stream);
  RVO3D_API_END
}

int rvo3d_policy_mlp_x3_sample(const void* blob, int32_t obs_width, const float* obs, int64_t obs_ld, int64_t rows,
                               const int32_t* vo_count, int32_t state_dim, int32_t row_dim, int32_t tanh_out, const float* log_std, float std_factor, uint64_t seed, uint64_t step,
                               float* act, float* logp, float* val, float* dbg_mu, float* dbg_raw, void* stream) {
  RVO3D_API_BEGIN
  return policy_mlp_sample<true>(blob, obs_width, obs, obs_ld, rows, vo_count, state_dim, row_dim, tanh_out, log_std,
                                 std_factor, seed, step, act, logp, val, dbg_mu, dbg_raw, stream);
  RVO3D_API_END
}

int rvo3d_reader_zero_features(const float* obs, int64_t obs_ld, int64_t rows, int32_t state_dim, int32_t feat_dim,
                               const float* ln_w, const float* ln_b, float sum_h0, float sumsq_h0, float ln_eps,
                               float* out, int64_t out_ld, const int32_t* vo_count, int32_t* list, int32_t* count,
                               void* stream) {
  RVO3D_API_BEGIN
  if (!obs || !ln_w || !ln_b || !out) return fail(RVO3D_ERR_INVALID, "null pointer");
  if ((vo_count != nullptr) != (list != nullptr) || (vo_count != nullptr) != (count != nullptr))
    return fail(RVO3D_ERR_INVALID, "vo_count, list and count go together");
  if (state_dim < 1 || state_dim > rvo3d::kReaderMaxSd || feat_dim <= state_dim)
    return fail(RVO3D_ERR_INVALID, "need 1 <= state_dim <= 32 and feat_dim > state_dim");
  // (the kernel reads the state in 16-byte pieces: the last one may take up to three floats beyond state_dim, still inside the row)
  if (rows < 0 || obs_ld < (state_dim + 3) / 4 * 4 || out_ld < state_dim + 8)
    return fail(RVO3D_ERR_INVALID, "rows / row strides too small");
  if (rows == 0) return RVO3D_OK;
  rvo3d::ZeroFeatArgs A{obs, obs_ld, rows, state_dim, feat_dim, ln_w, ln_b, sum_h0, sumsq_h0, ln_eps, out, out_ld,
                        vo_count, list, count};
  hipLaunchKernelGGL(rvo3d::reader_zero_features_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_policy_rows(const rvo3d_rnn_policy* net, const float* obs, int64_t obs_ld, const int32_t* vo_count,
                      const int32_t* list, int32_t* count, int32_t* done_blocks, int32_t tanh_out, const float* log_std,
                      float std_factor, uint64_t seed, uint64_t step, float* act, float* logp, float* val, void* stream) {
  RVO3D_API_BEGIN
  if (!net || !obs || !vo_count || !list || !count || !done_blocks || !log_std || !act || !logp || !val)
    return fail(RVO3D_ERR_INVALID, "null pointer");
  rvo3d::PolicyRowsArgs A;
  if (int rc = copy_reader(A, *net)) return rc;
  if (net->hidden < 1 || net->hidden > 256 || net->in_dim < 1 || net->in_dim > rvo3d::kReaderMaxIn || net->state_dim < 1 ||
      net->state_dim > rvo3d::kReaderMaxSd || net->slots < 1 || net->slots > 16)
    return fail(RVO3D_ERR_INVALID, "hidden <= 256, in_dim <= 16, state_dim <= 32, slots <= 16");
  if (obs_ld < net->state_dim + net->slots * net->in_dim) return fail(RVO3D_ERR_INVALID, "obs_ld too small");
  if (int rc = copy_heads(A, net->pi, net->v, "null head weight")) return rc;
  A.obs = obs; A.obs_ld = obs_ld; A.cnt = vo_count; A.list = list; A.count = count; A.done_blocks = done_blocks;
  A.state_dim = net->state_dim; A.in_dim = net->in_dim; A.H = net->hidden; A.slots = net->slots;
  A.S = sample_args(tanh_out, log_std, std_factor, seed, step, 0, act, logp, val, nullptr, nullptr);
  hipLaunchKernelGGL(rvo3d::policy_rows_kernel, dim3(256), dim3(256), 0, static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

// The biGRU policy step of the listed rows in 32-row MFMA tiles (csrc/rvo3d_policy_rnn_tiles.hpp): a bucket launch sorts
// the list into per-count sub-lists, a persistent launch runs the tiles.
int64_t rvo3d_policy_rnn_tiles_blob_bytes(int32_t hidden, int32_t in_dim, int32_t state_dim, int32_t bidir) {
  return policy_rnn_tiles_blob_bytes<false>(hidden, in_dim, state_dim, bidir);
}

int64_t rvo3d_policy_rnn_tiles_work_bytes(int64_t max_rows, int32_t slots) {
  if (max_rows < 1 || slots < 1 || slots > rvo3d::kRnnTilesMaxSlots) return -1;
  return 4 * (rvo3d::kRnnTilesWorkHeader + (int64_t)slots * max_rows);
}

int rvo3d_policy_rnn_tiles_pack(const rvo3d_rnn_policy* net, void* blob, int64_t blob_bytes, void* stream) {
  RVO3D_API_BEGIN
  return policy_rnn_tiles_pack<false>(net, blob, blob_bytes, stream);
  RVO3D_API_END
}

int rvo3d_policy_rnn_tiles(const void* blob, int64_t blob_bytes, int32_t hidden, int32_t in_dim, int32_t state_dim,
                           int32_t bidir, const float* obs, int64_t obs_ld, const int32_t* vo_count, const int32_t* list,
                           int32_t* count, int32_t* done_blocks, int32_t* work, int64_t max_rows, int32_t slots,
                           int32_t tanh_out, const float* log_std, float std_factor, uint64_t seed, uint64_t step,
                           float* act, float* logp, float* val, float* dbg_mu, void* stream) {
  RVO3D_API_BEGIN
  return policy_rnn_tiles<false>(blob, blob_bytes, hidden, in_dim, state_dim, bidir, obs, obs_ld, vo_count, list, count,
                                 done_blocks, work, max_rows, slots, tanh_out, log_std, std_factor, seed, step, act, logp,
                                 val, dbg_mu, stream);
  RVO3D_API_END
}

// The float32-class twin of the trio above: the stacks behind the LayerNorm in split bf16 as the GRU's products already
// are (see csrc/rvo3d_policy_rnn_tiles.hpp), on a blob of its own layout and size; same work area, list, counters,
// noise and per-row tail.
int64_t rvo3d_policy_rnn_tiles_x3_blob_bytes(int32_t hidden, int32_t in_dim, int32_t state_dim, int32_t bidir) {
  return policy_rnn_tiles_blob_bytes<true>(hidden, in_dim, state_dim, bidir);
}

int rvo3d_policy_rnn_tiles_x3_pack(const rvo3d_rnn_policy* net, void* blob, int64_t blob_bytes, void* stream) {
  RVO3D_API_BEGIN
  return policy_rnn_tiles_pack<true>(net, blob, blob_bytes, stream);
  RVO3D_API_END
}

int rvo3d_policy_rnn_tiles_x3(const void* blob, int64_t blob_bytes, int32_t hidden, int32_t in_dim, int32_t state_dim,
                              int32_t bidir, const float* obs, int64_t obs_ld, const int32_t* vo_count,
                              const int32_t* list, int32_t* count, int32_t* done_blocks, int32_t* work, int64_t max_rows,
                              int32_t slots, int32_t tanh_out, const float* log_std, float std_factor, uint64_t seed,
                              uint64_t step, float* act, float* logp, float* val, float* dbg_mu, void* stream) {
  RVO3D_API_BEGIN
  return policy_rnn_tiles<true>(blob, blob_bytes, hidden, in_dim, state_dim, bidir, obs, obs_ld, vo_count, list, count,
                                done_blocks, work, max_rows, slots, tanh_out, log_std, std_factor, seed, step, act, logp,
                                val, dbg_mu, stream);
  RVO3D_API_END
}

int rvo3d_reader_first_step(const rvo3d_gru_reader* rd, const float* obs, int64_t obs_ld, int64_t rows, void* feat,
                            int32_t feat_dtype, int64_t feat_ld, void* stream) {
  RVO3D_API_BEGIN
  if (!rd || !obs || !feat || !rd->w_ih_f || !rd->b_ih_f || !rd->b_hh_f || !rd->ln_w || !rd->ln_b)
    return fail(RVO3D_ERR_INVALID, "null pointer");
  if ((rd->w_ih_r != nullptr) != (rd->b_ih_r != nullptr) || (rd->w_ih_r != nullptr) != (rd->b_hh_r != nullptr))
    return fail(RVO3D_ERR_INVALID, "the reverse direction needs all three of w_ih_r / b_ih_r / b_hh_r");
  if (rd->hidden < 64 || rd->hidden > 256 || rd->hidden % 64 != 0 || rd->in_dim != 9 || rd->state_dim < 0 ||
      rd->state_dim > rvo3d::kReaderMaxSd)
    return fail(RVO3D_ERR_INVALID, "hidden must be 64 / 128 / 192 / 256, in_dim 9, state_dim <= 32");
  if (feat_dtype != RVO3D_F32 && feat_dtype != RVO3D_BF16) return fail(RVO3D_ERR_INVALID, "feat_dtype must be RVO3D_F32 or RVO3D_BF16");
  if (rows < 0 || obs_ld < rd->state_dim + rd->in_dim || feat_ld < rd->state_dim + rd->hidden)
    return fail(RVO3D_ERR_INVALID, "rows / row strides too small");
  if (feat_dtype == RVO3D_BF16 && ((reinterpret_cast<uintptr_t>(feat) & 7) || (feat_ld & 3)))
    return fail(RVO3D_ERR_INVALID, "bf16 features: feat 8-byte aligned, feat_ld a multiple of 4");
  if (rows == 0) return RVO3D_OK;
  rvo3d::ReaderArgs A;
  A.w_ih_f = rd->w_ih_f; A.b_ih_f = rd->b_ih_f; A.b_hh_f = rd->b_hh_f;
  A.w_ih_r = rd->w_ih_r; A.b_ih_r = rd->b_ih_r; A.b_hh_r = rd->b_hh_r;
  A.ln_w = rd->ln_w; A.ln_b = rd->ln_b; A.H = rd->hidden; A.IN = rd->in_dim; A.SD = rd->state_dim; A.eps = rd->ln_eps;
  A.obs = obs; A.obs_ld = obs_ld; A.rows = rows; A.feat = feat; A.feat_bf16 = feat_dtype == RVO3D_BF16; A.feat_ld = feat_ld;
  const int64_t groups = (rows + rvo3d::kReaderRows - 1) / rvo3d::kReaderRows;
  // a few workgroups per CU, each looping over row groups: the unit's weights are loaded once per workgroup
  const unsigned grid = (unsigned)(groups < 256 * 8 ? groups : 256 * 8);
  hipLaunchKernelGGL((rvo3d::reader_first_step_kernel<9>), dim3(grid), dim3((unsigned)rd->hidden), 0,
                     static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_rollout_set_step_counter(uint64_t* device_counter) {
  RVO3D_API_BEGIN
  g_step_dev.store(device_counter);
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_rollout_account(int32_t E, int32_t N, const float* reward, const uint8_t* done, const uint8_t* finish,
                          int32_t sanitize, int32_t max_ep_len, int32_t epoch_end, float* rew_slot, float* ep_ret,
                          int32_t* ep_len, uint8_t* cut_slot, uint8_t* extra_mask, double* sums, int32_t* any_extra,
                          void* stream) {
  RVO3D_API_BEGIN
  return rvo3d_rollout_account_n(E, N, nullptr, reward, done, finish, sanitize, max_ep_len, epoch_end, rew_slot, ep_ret,
                                 ep_len, cut_slot, extra_mask, sums, any_extra, stream);
  RVO3D_API_END
}

int rvo3d_rollout_account_n(int32_t E, int32_t N, const int32_t* drone_counts, const float* reward, const uint8_t* done,
                            const uint8_t* finish, int32_t sanitize, int32_t max_ep_len, int32_t epoch_end, float* rew_slot,
                            float* ep_ret, int32_t* ep_len, uint8_t* cut_slot, uint8_t* extra_mask, double* sums,
                            int32_t* any_extra, void* stream) {
  RVO3D_API_BEGIN
  if (E < 1 || N < 1 || N > rvo3d::kMaxThreads) return fail(RVO3D_ERR_INVALID, "need num_envs >= 1 and 1 <= num_drones <= 512");
  if (!reward || !done || !finish || !rew_slot || !ep_ret || !ep_len || !cut_slot || !extra_mask || !sums || !any_extra)
    return fail(RVO3D_ERR_INVALID, "null pointer");
  rvo3d::AccountArgs A{E, N, reward, done, finish, sanitize, max_ep_len, epoch_end, rew_slot, ep_ret, ep_len,
                       cut_slot, extra_mask, sums, any_extra, g_step_dev.load()};
  const dim3 grid((unsigned)E), block((unsigned)align_up((size_t)N, 64));
  if (drone_counts)
    hipLaunchKernelGGL(rvo3d::rollout_account_counted_kernel, grid, block, 0, static_cast<hipStream_t>(stream), A, drone_counts);
  else
    hipLaunchKernelGGL(rvo3d::rollout_account_kernel, grid, block, 0, static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_gae(const float* rew, const float* val, const uint8_t* cut, int64_t steps, int64_t envs, int64_t drones,
              double gamma, double lam, float* adv, float* ret, void* stream) {
  RVO3D_API_BEGIN
  // (every check precedes the first HIP call: the argument checks run on a machine without a GPU)
  if (!rew || !val || !cut || !adv || !ret) return fail(RVO3D_ERR_INVALID, "null pointer");
  if (steps < 1 || envs < 1 || drones < 1) return fail(RVO3D_ERR_INVALID, "need steps >= 1, envs >= 1 and drones >= 1");
  if (!std::isfinite(gamma) || !std::isfinite(lam)) return fail(RVO3D_ERR_INVALID, "gamma and lam must be finite");
  // one lane per column in 256-lane workgroups on a 1-D grid; the byte ranges below stay far inside 64 bits
  const int64_t kMaxColumns = (int64_t)0x7fffffff * 256, kMaxElems = (int64_t)1 << 58;
  if (envs > kMaxColumns / drones || steps > kMaxElems / (envs * drones))
    return fail(RVO3D_ERR_INVALID, "steps * envs * drones too large");
  const uint64_t n4 = (uint64_t)steps * (uint64_t)envs * (uint64_t)drones * 4, n1 = (uint64_t)steps * (uint64_t)envs;
  auto overlap = [](const void* a, uint64_t an, const void* b, uint64_t bn) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bn && y < x + an;
  };
  if (overlap(adv, n4, rew, n4) || overlap(adv, n4, val, n4) || overlap(adv, n4, cut, n1) ||
      overlap(ret, n4, rew, n4) || overlap(ret, n4, val, n4) || overlap(ret, n4, cut, n1) || overlap(adv, n4, ret, n4))
    return fail(RVO3D_ERR_INVALID, "adv / ret overlap an input or each other: the outputs need storage of their own");
  const int64_t columns = envs * drones;
  rvo3d::GaeArgs A{rew, val, cut, steps, envs, drones, gamma, gamma * lam, adv, ret};
  hipLaunchKernelGGL(rvo3d::gae_kernel, dim3((unsigned)((columns + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_eval_action(rvo3d_env* h, const float* a, float acceler_vel, double* action64, void* stream) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!a || !action64) return fail(RVO3D_ERR_INVALID, "a / action64 are required");
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const size_t EN = (size_t)h->P.E * h->P.N;
  hipLaunchKernelGGL(h->counted ? rvo3d::eval_action_counted_kernel : rvo3d::eval_action_kernel,
                     dim3((unsigned)((EN + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h->P, a, acceler_vel, action64);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

}  // extern "C"

namespace {
// rvo3d_eval_account and rvo3d_eval_account_safety: the same checks (before the first HIP call), arguments and grid
int check_eval_account_args(const float* reward, const uint8_t* done, const uint8_t* info, const uint8_t* finish,
                            int32_t max_ep_len, int32_t quota, const rvo3d_eval_bufs* b) {
  if (!reward || !done || !info || !finish || !b) return fail(RVO3D_ERR_INVALID, "null pointer");
  if (!b->ep_len || !b->ep_ret || !b->speed_sum || !b->counted || !b->rec_len || !b->rec_ret || !b->rec_speed ||
      !b->rec_step || !b->rec_flags || !b->remaining || !b->ended)
    return fail(RVO3D_ERR_INVALID, "null pointer in rvo3d_eval_bufs");
  if (max_ep_len < 1 || quota < 1) return fail(RVO3D_ERR_INVALID, "need max_ep_len >= 1 and quota >= 1");
  return RVO3D_OK;
}
rvo3d::EvalAccountArgs eval_account_args(const float* reward, const uint8_t* done, const uint8_t* info,
                                         const uint8_t* finish, int32_t max_ep_len, int32_t quota, int64_t step,
                                         const rvo3d_eval_bufs* b) {
  return {reward, done, info, finish, max_ep_len, quota, step, b->ep_len, b->ep_ret, b->speed_sum,
          b->counted, b->rec_len, b->rec_ret, b->rec_speed, b->rec_step, b->rec_flags, b->remaining, b->ended};
}
// eval_lanes_per_env(N) lanes per env: up to 256 envs per workgroup for N = 1, one wave per env from 33 drones on
dim3 eval_account_grid(const rvo3d_env* h) {
  const size_t lanes = (size_t)h->P.E * (size_t)rvo3d::eval_lanes_per_env(h->P.N);
  return dim3((unsigned)((lanes + rvo3d::kEvalAccountThreads - 1) / rvo3d::kEvalAccountThreads));
}
}  // namespace

extern "C" {

int rvo3d_eval_account(rvo3d_env* h, const float* reward, const uint8_t* done, const uint8_t* info, const uint8_t* finish,
                       int32_t max_ep_len, int32_t quota, int64_t step, const rvo3d_eval_bufs* b, void* stream) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (int rc = check_eval_account_args(reward, done, info, finish, max_ep_len, quota, b)) return rc;
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  hipLaunchKernelGGL(h->counted ? rvo3d::eval_account_counted_kernel : rvo3d::eval_account_kernel, eval_account_grid(h),
                     dim3(rvo3d::kEvalAccountThreads), 0, static_cast<hipStream_t>(stream), h->P,
                     eval_account_args(reward, done, info, finish, max_ep_len, quota, step, b));
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

}  // extern "C"

namespace {
// the launch geometry of the kernels with one lane per drone and whole envs per block (safety_scan_body's)
struct EnvLanes {
  dim3 grid, block;
};
EnvLanes env_lanes(const rvo3d_env* h) {
  const int N = h->P.N, T = rvo3d::safety_threads(N);
  const size_t epb = (size_t)(T / rvo3d::safety_lanes_per_env(N));
  return EnvLanes{dim3((unsigned)(((size_t)h->P.E + epb - 1) / epb)), dim3((unsigned)T)};
}
// the scan's launch for both entry points below (arguments checked, device entered)
int launch_safety_scan(rvo3d_env* h, const rvo3d::SafetyArgs& A, hipStream_t s) {
  const EnvLanes g = env_lanes(h);
  hipLaunchKernelGGL(h->counted ? rvo3d::safety_scan_counted_kernel : rvo3d::safety_scan_kernel, g.grid, g.block,
                     rvo3d::safety_lds_bytes(h->P.N), s, h->P, A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
}
bool near_margin_ok(double m) { return std::isfinite(m) && m >= 0.0; }
// the building velocities' arguments: no motion, no velocity
rvo3d::BuildingVelArgs building_vel_args(const rvo3d_building_motion* m, double dt) {
  return rvo3d::BuildingVelArgs{m ? m->ends : nullptr, m ? m->speed : nullptr, m ? m->leg : nullptr, dt};
}
// the classical RVO velocity's arguments; false: acceler is refused (rvo3d::kRvoAccelerWhy)
bool rvo_vel_args(const double* vmax, double acceler, rvo3d::RvoVelArgs* A) {
  if (!rvo3d::rvo_acceler_ok(acceler)) return false;
  for (int k = 0; k < 3; ++k) A->vmax[k] = vmax[k];
  A->acceler = acceler;
  return true;
}
}  // namespace

extern "C" {

int rvo3d_safety_scan(rvo3d_env* h, double near_margin, double* sep, double* bclear, double* wall, int32_t* near_pairs,
                      void* stream) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!near_margin_ok(near_margin)) return fail(RVO3D_ERR_INVALID, "near_margin must be finite and >= 0");
  if (!sep && !bclear && !wall && !near_pairs) return fail(RVO3D_ERR_INVALID, "at least one output is required");
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const rvo3d::SafetyArgs A{near_margin, sep, bclear, wall, near_pairs, nullptr, nullptr, nullptr};
  return launch_safety_scan(h, A, static_cast<hipStream_t>(stream));
  RVO3D_API_END
}

int rvo3d_eval_account_safety(rvo3d_env* h, const float* reward, const uint8_t* done, const uint8_t* info,
                              const uint8_t* finish, int32_t max_ep_len, int32_t quota, int64_t step,
                              const rvo3d_eval_bufs* b, double near_margin, const rvo3d_eval_safety_bufs* sb,
                              void* stream) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (int rc = check_eval_account_args(reward, done, info, finish, max_ep_len, quota, b)) return rc;
  if (!near_margin_ok(near_margin)) return fail(RVO3D_ERR_INVALID, "near_margin must be finite and >= 0");
  if (!sb) return fail(RVO3D_ERR_INVALID, "null pointer");
  if (!sb->ep_min_sep || !sb->ep_min_bclear || !sb->ep_min_wall || !sb->ep_near || !sb->rec_min_sep ||
      !sb->rec_min_bclear || !sb->rec_min_wall || !sb->rec_near)
    return fail(RVO3D_ERR_INVALID, "null pointer in rvo3d_eval_safety_bufs");
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t E = (size_t)h->P.E;
  double* st = h->safety_scratch;  // (rvo3d_load_world allocated it)
  int32_t* st_near = reinterpret_cast<int32_t*>(st + 3 * E);
  const rvo3d::SafetyArgs A{near_margin, nullptr, nullptr, nullptr, st_near, st, st + E, st + 2 * E};
  if (int rc2 = launch_safety_scan(h, A, s)) return rc2;
  const rvo3d::EvalSafetyArgs S{st, st + E, st + 2 * E, st_near, sb->ep_min_sep, sb->ep_min_bclear, sb->ep_min_wall,
                                sb->ep_near, sb->rec_min_sep, sb->rec_min_bclear, sb->rec_min_wall, sb->rec_near, quota};
  hipLaunchKernelGGL(h->counted ? rvo3d::eval_account_safety_counted_kernel : rvo3d::eval_account_safety_kernel,
                     eval_account_grid(h), dim3(rvo3d::kEvalAccountThreads), 0, s, h->P,
                     eval_account_args(reward, done, info, finish, max_ep_len, quota, step, b), S);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_building_rows(rvo3d_env* h, const rvo3d_building_rows_args* a, void* stream) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  const char* why = "";
  if (int rc = rvo3d::building_rows_check(a, h->P.W, (int64_t)h->P.E * h->P.N, &why)) return fail(rc, why);
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const EnvLanes g = env_lanes(h);
  const rvo3d::BuildingRowsArgs A{a->k, a->reach, a->below, a->rows, a->row_ld, a->col0, a->b_count, a->obs};
  hipLaunchKernelGGL(h->counted ? rvo3d::building_rows_counted_kernel : rvo3d::building_rows_kernel, g.grid, g.block,
                     rvo3d::building_lds_bytes(h->P.N, a->k), static_cast<hipStream_t>(stream), h->P, A);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_building_rows_moving(rvo3d_env* h, const rvo3d_building_rows_args* a, const rvo3d_building_motion* m, double dt,
                               void* stream) {
  RVO3D_API_BEGIN
  // every argument check before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  const char* why = "";
  if (int rc = rvo3d::building_rows_moving_check(a, h->P.W, (int64_t)h->P.E * h->P.N, h->env_bld != nullptr, m, dt, &why))
    return fail(rc, why);
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const EnvLanes g = env_lanes(h);
  const rvo3d::BuildingRowsArgs A{a->k, a->reach, a->below, a->rows, a->row_ld, a->col0, a->b_count, a->obs};
  hipLaunchKernelGGL(h->counted ? rvo3d::building_rows_moving_counted_kernel : rvo3d::building_rows_moving_kernel, g.grid,
                     g.block, rvo3d::building_lds_bytes(h->P.N, a->k, rvo3d::kBldRowFloatsMoving),
                     static_cast<hipStream_t>(stream), h->P, A, building_vel_args(m, dt));
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_set_reward_f64(rvo3d_env* h, double* reward64) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  h->P.reward64 = reward64;
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_des_vel(rvo3d_env* h, double* des_vel, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  if (!des_vel) return fail(RVO3D_ERR_INVALID, "des_vel is required");
  const size_t EN = (size_t)h->P.E * h->P.N;
  hipLaunchKernelGGL(h->counted ? rvo3d::des_vel_counted_kernel : rvo3d::des_vel_kernel,
                     dim3((unsigned)((EN + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h->P, des_vel);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_rvo_vel(rvo3d_env* h, const double* vmax, double acceler, double* out_vel, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  if (!vmax || !out_vel) return fail(RVO3D_ERR_INVALID, "vmax / out_vel are required");
  rvo3d::RvoVelArgs A;
  if (!rvo_vel_args(vmax, acceler, &A)) return fail(RVO3D_ERR_INVALID, rvo3d::kRvoAccelerWhy);
  const int T = (int)align_up((size_t)h->P.N, 64);
  hipLaunchKernelGGL(h->counted ? rvo3d::rvo_vel_counted_kernel : rvo3d::rvo_vel_kernel, dim3((unsigned)h->P.E),
                     dim3((unsigned)T),
                     (size_t)T * 8 * sizeof(double), static_cast<hipStream_t>(stream), h->P, A, out_vel);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_rvo_vel_city(rvo3d_env* h, const rvo3d_rvo_city_args* a, const rvo3d_building_motion* m, double dt,
                       void* stream) {
  RVO3D_API_BEGIN
  // every argument check before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  const char* why = "";
  if (int rc = rvo3d::rvo_city_check(a, h->env_bld != nullptr, m, dt, &why)) return fail(rc, why);
  rvo3d::RvoVelArgs A;
  if (!rvo_vel_args(a->vmax, a->acceler, &A)) return fail(RVO3D_ERR_INVALID, rvo3d::kRvoAccelerWhy);
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const rvo3d::RvoCityArgs Y{a->reach, a->below, a->horizon, a->clear_xy, a->clear_z, a->out_vel,
                             reinterpret_cast<unsigned long long*>(a->live_mask),
                             reinterpret_cast<unsigned long long*>(a->cone_mask),
                             reinterpret_cast<unsigned long long*>(a->blocked_mask), a->tc_min, a->n_gated, a->tier};
  const int T = (int)align_up((size_t)h->P.N, 64);
  hipLaunchKernelGGL(h->counted ? rvo3d::rvo_city_counted_kernel : rvo3d::rvo_city_kernel, dim3((unsigned)h->P.E),
                     dim3((unsigned)T), (size_t)T * 8 * sizeof(double), static_cast<hipStream_t>(stream), h->P, A, Y,
                     building_vel_args(m, dt));
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_orca_vel(rvo3d_env* h, const rvo3d_orca_args* a, const rvo3d_building_motion* m, double dt, void* stream) {
  RVO3D_API_BEGIN
  // every argument check before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  const char* why = "";
  if (int rc = rvo3d::orca_check(a, h->env_bld != nullptr, m, dt, &why)) return fail(rc, why);
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const size_t EN = (size_t)h->P.E * h->P.N;
  const size_t need = (size_t)rvo3d::orca_ws_slots(a->max_neighbors, a->max_buildings) * 6 * EN * sizeof(double);
  if (need > h->orca_ws_bytes) {  // (hipFree waits for the launches that still read the old one)
    if (h->orca_ws) (void)hipFree(h->orca_ws);
    h->orca_ws = nullptr;
    h->orca_ws_bytes = 0;
    HIP_TRY(hipMalloc((void**)&h->orca_ws, need));
    h->orca_ws_bytes = need;
  }
  const rvo3d::OrcaArgs Y{a->time_horizon, a->time_step, a->max_speed, a->pref_speed, a->neighbor_dist * a->neighbor_dist,
                          a->reach, a->below, a->clear_xy, a->max_neighbors, a->max_buildings, a->out_vel,
                          a->n_neighbors, a->n_buildings, a->status, a->slack, h->orca_ws, EN};
  const int T = (int)align_up((size_t)h->P.N, 64);
  hipLaunchKernelGGL(h->counted ? rvo3d::orca_counted_kernel : rvo3d::orca_kernel, dim3((unsigned)h->P.E),
                     dim3((unsigned)T), rvo3d::orca_lds_bytes(T), static_cast<hipStream_t>(stream), h->P, Y,
                     building_vel_args(m, dt));
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_shield_action(rvo3d_env* h, const rvo3d_shield_args* a, const rvo3d_building_motion* m, double dt, void* stream) {
  RVO3D_API_BEGIN
  // every argument check before the first HIP call
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  const char* why = "";
  if (int rc = rvo3d::shield_check(a, h->env_bld != nullptr, m, dt, &why)) return fail(rc, why);
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const size_t EN = (size_t)h->P.E * h->P.N;
  const size_t need = (size_t)rvo3d::orca_ws_slots(a->max_neighbors, a->max_buildings) * 6 * EN * sizeof(double);
  if (need > h->orca_ws_bytes) {  // rvo3d_orca_vel's workspace, grown as it grows it
    if (h->orca_ws) (void)hipFree(h->orca_ws);
    h->orca_ws = nullptr;
    h->orca_ws_bytes = 0;
    HIP_TRY(hipMalloc((void**)&h->orca_ws, need));
    h->orca_ws_bytes = need;
  }
  const rvo3d::ShieldArgs Y{a->time_horizon, a->time_step, a->max_speed, a->neighbor_dist * a->neighbor_dist, a->reach,
                            a->below, a->clear_xy, a->max_neighbors, a->max_buildings, a->action, a->out_action,
                            a->pref_vel, a->out_vel, a->status, a->flags, a->slack,
                            reinterpret_cast<long long*>(a->totals), h->orca_ws, EN};
  const int T = (int)align_up((size_t)h->P.N, 64);
  hipLaunchKernelGGL(h->counted ? rvo3d::shield_counted_kernel : rvo3d::shield_kernel, dim3((unsigned)h->P.E),
                     dim3((unsigned)T), rvo3d::shield_lds_bytes(T), static_cast<hipStream_t>(stream), h->P, Y,
                     building_vel_args(m, dt));
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_vel_command(rvo3d_env* h, const double* vel, double* action, uint8_t* clipped, void* stream) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  if (!h->world_loaded) return fail(RVO3D_ERR_STATE, "rvo3d_load_world has not been called");
  if (!vel || !action) return fail(RVO3D_ERR_INVALID, "vel / action are required");
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const size_t EN = (size_t)h->P.E * h->P.N;
  hipLaunchKernelGGL(h->counted ? rvo3d::vel_command_counted_kernel : rvo3d::vel_command_kernel,
                     dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), h->P, vel, action,
                     clipped);
  HIP_TRY(hipGetLastError());
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_state_ptrs(rvo3d_env* h, rvo3d_state_view* out) {
  RVO3D_API_BEGIN
  if (!h || !out) return fail(RVO3D_ERR_INVALID, "null argument");
  const Params& P = h->P;
  out->px = P.px(); out->py = P.py(); out->pz = P.pz(); out->vx = P.vx(); out->vy = P.vy(); out->vz = P.vz();
  out->yaw = P.yaw(); out->pitch = P.pitch(); out->real_len = P.real_len(); out->max_dev = P.max_dev();
  out->extra_len = P.extra_len(); out->wp_idx = P.wp_idx(); out->arrive = P.arrive(); out->dest = P.dest();
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_get_state(rvo3d_env* h, double* pos, double* vel, double* yaw, double* pitch,
                    double* real_len, double* max_dev, double* extra_len, int32_t* wp_idx,
                    uint8_t* arrive, uint8_t* dest, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  const Params& P = h->P;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int EN = P.E * P.N;
  const dim3 grid((EN + 255) / 256), blk(256);
  if (pos) hipLaunchKernelGGL(rvo3d::soa_to_aos3, grid, blk, 0, s, P.px(), P.py(), P.pz(), pos, EN);
  if (vel) hipLaunchKernelGGL(rvo3d::soa_to_aos3, grid, blk, 0, s, P.vx(), P.vy(), P.vz(), vel, EN);
  HIP_TRY(hipGetLastError());
  const hipMemcpyKind k = hipMemcpyDeviceToDevice;
  for (const ScalarField& f : scalar_fields(P, yaw, pitch, real_len, max_dev, extra_len, wp_idx, arrive, dest))
    if (f.caller) HIP_TRY(hipMemcpyAsync(const_cast<void*>(f.caller), f.arena, f.bytes, k, s));
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_set_state(rvo3d_env* h, const double* pos, const double* vel, const double* yaw,
                    const double* pitch, const double* real_len, const double* max_dev,
                    const double* extra_len, const int32_t* wp_idx, const uint8_t* arrive,
                    const uint8_t* dest, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, true, dg);
  if (rc) return rc;
  h->dv_valid = h->g_valid = false;  // the next step recomputes the pre-move dronestate and stage G
  const Params& P = h->P;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int EN = P.E * P.N;
  const dim3 grid((EN + 255) / 256), blk(256);
  if (pos) hipLaunchKernelGGL(rvo3d::aos3_to_soa, grid, blk, 0, s, pos, P.px(), P.py(), P.pz(), EN);
  if (vel) hipLaunchKernelGGL(rvo3d::aos3_to_soa, grid, blk, 0, s, vel, P.vx(), P.vy(), P.vz(), EN);
  HIP_TRY(hipGetLastError());
  const hipMemcpyKind k = hipMemcpyDeviceToDevice;
  for (const ScalarField& f : scalar_fields(P, yaw, pitch, real_len, max_dev, extra_len, wp_idx, arrive, dest)) {
    if (!f.caller) continue;
    HIP_TRY(hipMemcpyAsync(f.arena, f.caller, f.bytes, k, s));
    // current / previous waypoint follow the index
    if (f.arena == P.wp_idx()) hipLaunchKernelGGL(rvo3d::wpcache_kernel, grid, blk, 0, s, P);
  }
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_error_flags(rvo3d_env* h, uint32_t* flags, void* stream) {
  RVO3D_API_BEGIN
  DeviceGuard dg;
  int rc = check(h, false, dg);
  if (rc) return rc;
  if (!flags) return fail(RVO3D_ERR_INVALID, "flags is required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(flags, h->P.err, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemsetAsync(h->P.err, 0, 4, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RVO3D_OK;
  RVO3D_API_END
}

#ifdef RVO3D_DIAG
// diagnostics build only (librvo3d_hip_diag.so, tools/): attach a device buffer
// [blocks][16] of s_memtime stamps, or NULL to detach
int rvo3d_debug_stamps(rvo3d_env* h, unsigned long long* stamps) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  h->P.dbg = stamps;
  return RVO3D_OK;
  RVO3D_API_END
}
#endif

int rvo3d_kernel_name(rvo3d_env* h, int32_t mode, char* buf, int32_t cap) {
  RVO3D_API_BEGIN
  if (!h || !buf || cap < 1) return fail(RVO3D_ERR_INVALID, "null handle / buffer");
  if (mode < 0 || mode > 2) return fail(RVO3D_ERR_INVALID, "mode: 0 observe, 1 step, 2 step + auto-reset");
  if (h->counted) {
    std::snprintf(buf, (size_t)cap, "rvo3d::env_kernel_counted<%d, %d, %d, %s>", (int)mode, h->P.nw,
                  rvo3d::pick_counted_kernel(h->P).nfix, h->P.env_train ? "true" : "false");
    return RVO3D_OK;
  }
  const Pick k = pick_kernel(h->P);
  std::snprintf(buf, (size_t)cap, "rvo3d::env_kernel<%d, %d, %d, %s, %s>", (int)mode, h->P.nw, k.nfix,
                h->P.env_train ? "true" : "false", k.pad ? "true" : "false");
  return RVO3D_OK;
  RVO3D_API_END
}

int rvo3d_launch_info(rvo3d_env* h, int32_t* threads, int32_t* envs_per_block, int32_t* blocks,
                      int32_t* lds_bytes) {
  RVO3D_API_BEGIN
  if (!h) return fail(RVO3D_ERR_INVALID, "null handle");
  const rvo3d::Geometry& G = h->counted ? h->cgeo : h->geo;
  if (threads) *threads = G.threads;
  if (envs_per_block) *envs_per_block = h->counted ? (G.threads == 64 ? 64 / rvo3d::pick_counted_kernel(h->P).nfix : 1) : h->P.epb;
  if (blocks) *blocks = G.blocks;
  if (lds_bytes) *lds_bytes = G.lds;
  return RVO3D_OK;
  RVO3D_API_END
}

}  // extern "C"
