// rvo3d_eval_kernels.hpp -- the evaluator's per-step glue around the env step (train/policy/post_train.py:38-128) on the
// device: the action glue (eval_action_kernel), the episode bookkeeping of every env with its records
// (eval_account_kernel, around the pure per-env decision eval_account_env) and the row select behind
// rvo3d_observe_envs (observe_select_kernel).  Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
// The per-env decision is plain C++ (__host__ __device__): tests/host/eval_account_check.hip calls it on the CPU.
#pragma once

#include "rvo3d_params.hpp"

namespace rvo3d {

// ---- action glue (post_train.py:63-74), one lane per drone ----
//   a = np.round(model.act(o), 2)          float32: rint(a * 100f) / 100f, a true division
//   action = acceler_vel * a + drone.vel   float32 product, widened, + float64 - and NOT rounded again (the trainer's
//                                          glue, rvo3d_step.hpp action_mode 1, rounds the sum as well)
// (-ffp-contract=off keeps the product and the sum apart.)
// CNT (the *_counted kernels): a handle with drone counts (rvo3d_set_drone_counts) - a ghost's action row is zero,
// whatever its input row holds.
template <bool CNT>
__device__ __forceinline__ void eval_action_body(const Params& P, const float* a, float acceler_vel, double* action64) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)P.E * P.N) return;
  if (CNT) {
    const int64_t e = g / P.N;
    if (g - e * P.N >= P.cold().counts[e]) {
      action64[g * 3] = 0.0; action64[g * 3 + 1] = 0.0; action64[g * 3 + 2] = 0.0;
      return;
    }
  }
  const float* A = a + g * 3;
  const double vv[3] = {P.vx()[g], P.vy()[g], P.vz()[g]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float r = __builtin_rintf(A[k] * 100.0f) / 100.0f;
    action64[g * 3 + k] = (double)(acceler_vel * r) + vv[k];
  }
}
__global__ void __launch_bounds__(256) eval_action_kernel(const Params P, const float* a, float acceler_vel,
                                                          double* action64) {
  eval_action_body<false>(P, a, acceler_vel, action64);
}
__global__ void __launch_bounds__(256) eval_action_counted_kernel(const Params P, const float* a, float acceler_vel,
                                                                  double* action64) {
  eval_action_body<true>(P, a, acceler_vel, action64);
}

// ---- episode bookkeeping of one evaluation step (post_train.py:78-105) ----
enum { kEvalArrived = 1, kEvalFinished = 2, kEvalCollided = 4, kEvalTimeout = 8 };  // bits of a record's flag byte

struct EvalEnvIn {
  int32_t ep_len;        // running values before this step
  double ep_ret, speed_sum;
  int32_t counted;       // episodes of this env recorded so far
  double norm_sum;       // sum over the env's drones of ||vel|| after the step
  int32_t n;             // drones of the env
  float reward0;         // r[0] (post_train.py:82)
  bool any_done, all_finish, all_info;
  int32_t max_ep_len, quota;
};
struct EvalEnvOut {
  int32_t ep_len;        // running values after this step (zero when the episode ended)
  double ep_ret, speed_sum;
  int32_t counted;
  bool ended;            // the env is reset behind this step
  bool record;           // ended with counted < quota: the rec_* values go to slot [counted before this step]
  int32_t rec_len;
  double rec_ret, rec_speed;
  uint8_t rec_flags;
};

// What one env's step does to its episode: mean speed added, return added, length + 1; the episode ends when a drone
// collided, at len == max_ep_len (the evaluator's `==`, post_train.py:86 - the trainer's timeout is `>`), or when every
// drone finished; an ended episode is recorded while the env's quota lasts, and ends the running values either way.
__host__ __device__ inline EvalEnvOut eval_account_env(const EvalEnvIn& in) {
  EvalEnvOut o;
  const double speed = in.norm_sum / (double)in.n;
  const double ssum = in.speed_sum + speed;
  const double ret = in.ep_ret + (double)in.reward0;
  const int32_t len = in.ep_len + 1;
  const bool timeout = len == in.max_ep_len;
  o.ended = in.any_done || timeout || in.all_finish;
  o.record = o.ended && in.counted < in.quota;
  o.rec_len = len;
  o.rec_ret = ret;
  o.rec_speed = ssum / (double)len;
  o.rec_flags = (uint8_t)((in.all_info ? kEvalArrived : 0) | (in.all_finish ? kEvalFinished : 0) |
                          (in.any_done ? kEvalCollided : 0) | (timeout ? kEvalTimeout : 0));
  o.counted = in.counted + (o.record ? 1 : 0);
  o.ep_len = o.ended ? 0 : len;
  o.ep_ret = o.ended ? 0.0 : ret;
  o.speed_sum = o.ended ? 0.0 : ssum;
  return o;
}

// Lanes that share one env: the smallest power of two >= n, at most a wave.  (Also what the host sizes the grid with.)
__host__ __device__ inline int eval_lanes_per_env(int n) {
  int l = 1;
  while (l < n && l < 64) l <<= 1;
  return l;
}
constexpr int kEvalAccountThreads = 256;

struct EvalAccountArgs {
  const float* reward;     // [E][N]
  const uint8_t *done, *info, *finish;  // [E][N]
  int32_t max_ep_len, quota;
  int64_t step;            // the caller's step number, stored with a record
  int32_t* ep_len;         // [E] running values
  double* ep_ret;
  double* speed_sum;
  int32_t* counted;
  int32_t* rec_len;        // [E][quota] records
  double* rec_ret;
  double* rec_speed;
  int64_t* rec_step;
  uint8_t* rec_flags;
  int32_t* remaining;      // [1]
  uint8_t* ended;          // [E]
};

// L = eval_lanes_per_env(N) consecutive lanes hold one env (64 / L envs per wave, four waves per workgroup); a lane takes
// the drones l, l + L, ... in order, then the L partial sums meet in a butterfly - an order that depends on N alone, so the
// float64 speed sum is the same bits in every run.  Lanes beyond E and beyond N stay in the butterfly with neutral values.
// CNT: the env's drones are its first counts[e]: they alone enter the sums and the flags, and they are summed in the
// order a handle of counts[e] drones sums them - by its eval_lanes_per_env(counts[e]) lanes, which are the first of this
// env's lanes; the butterfly's wider steps then only add the other lanes' zeros (x + 0.0 == x for the sums, all >= +0).
// `extra(e, counted before this step, decision)` runs on the env's deciding lane behind the decision: nothing here,
// the safety fold of rvo3d_safety_kernels.hpp for rvo3d_eval_account_safety.
struct EvalNoExtra {
  __device__ __forceinline__ void operator()(int64_t, int32_t, const EvalEnvOut&) const {}
};
template <bool CNT, class Extra>
__device__ __forceinline__ void eval_account_body(const Params P, const EvalAccountArgs A, const Extra extra) {
  const int N = P.N;
  const int L = eval_lanes_per_env(N);
  const int64_t slot = ((int64_t)blockIdx.x * kEvalAccountThreads + threadIdx.x) >> __builtin_ctz(L);  // env of this lane group
  const int l = (int)(threadIdx.x & (unsigned)(L - 1));
  const bool live = slot < (int64_t)P.E;
  const int64_t e = live ? slot : 0;
  double norm_sum = 0.0;
  int bits = 0;  // 1: a drone collided, 2: a drone has not finished, 4: a drone has not arrived
  const int Nl = (CNT && live) ? P.cold().counts[e] : N;  // the drones the env has
  const int Ll = CNT ? eval_lanes_per_env(Nl) : L;
  if (live && l < Ll) {
    for (int d = l; d < Nl; d += Ll) {
      const int64_t g = e * N + d;
      const double x = P.vx()[g], y = P.vy()[g], z = P.vz()[g];
      norm_sum += __builtin_sqrt(x * x + y * y + z * z);
      bits |= (A.done[g] != 0 ? 1 : 0) | (A.finish[g] == 0 ? 2 : 0) | (A.info[g] == 0 ? 4 : 0);
    }
  }
  for (int m = L >> 1; m >= 1; m >>= 1) {
    norm_sum += __shfl_xor(norm_sum, m, 64);
    bits |= __shfl_xor(bits, m, 64);
  }
  if (!live || l != 0) return;
  EvalEnvIn in;
  in.ep_len = A.ep_len[e]; in.ep_ret = A.ep_ret[e]; in.speed_sum = A.speed_sum[e]; in.counted = A.counted[e];
  in.norm_sum = norm_sum; in.n = Nl; in.reward0 = A.reward[e * N];
  in.any_done = (bits & 1) != 0; in.all_finish = (bits & 2) == 0; in.all_info = (bits & 4) == 0;
  in.max_ep_len = A.max_ep_len; in.quota = A.quota;
  const EvalEnvOut o = eval_account_env(in);
  if (o.record) {  // (counted < quota, and counted is never negative: the caller starts it at zero)
    const int64_t r = e * A.quota + in.counted;
    A.rec_len[r] = o.rec_len; A.rec_ret[r] = o.rec_ret; A.rec_speed[r] = o.rec_speed;
    A.rec_step[r] = A.step; A.rec_flags[r] = o.rec_flags;
    atomicSub(A.remaining, 1);
  }
  A.ep_len[e] = o.ep_len; A.ep_ret[e] = o.ep_ret; A.speed_sum[e] = o.speed_sum; A.counted[e] = o.counted;
  A.ended[e] = o.ended ? 1 : 0;
  extra(e, in.counted, o);
}
__global__ void __launch_bounds__(kEvalAccountThreads) eval_account_kernel(const Params P, const EvalAccountArgs A) {
  eval_account_body<false>(P, A, EvalNoExtra{});
}
__global__ void __launch_bounds__(kEvalAccountThreads) eval_account_counted_kernel(const Params P, const EvalAccountArgs A) {
  eval_account_body<true>(P, A, EvalNoExtra{});
}

// ---- row select of rvo3d_observe_envs: one workgroup per env; the envs whose mask byte is zero leave at once, the others
//      copy their N rows of W floats and their N counts from the scratch pair, word by word (bit for bit) ----
__global__ void __launch_bounds__(256) observe_select_kernel(int N, int W, const uint8_t* env_mask, const uint32_t* src_obs,
                                                             const int32_t* src_cnt, uint32_t* obs, int32_t* vo_count) {
  const int64_t e = blockIdx.x;
  if (env_mask[e] == 0) return;
  const int64_t words = (int64_t)N * W, base = e * words;
  for (int64_t i = threadIdx.x; i < words; i += blockDim.x) obs[base + i] = src_obs[base + i];
  for (int i = threadIdx.x; i < N; i += blockDim.x) vo_count[e * N + i] = src_cnt[e * N + i];
}

}  // namespace rvo3d
