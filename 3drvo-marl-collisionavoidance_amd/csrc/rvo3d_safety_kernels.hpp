// rvo3d_safety_kernels.hpp -- safety metrics of the handle's current state (include/rvo3d.h: rvo3d_safety_scan): per
// drone the separation to the nearest other drone, the clearance to the buildings its env collides with and to the map
// faces, per env the number of near pairs (safety_scan_kernel); and their fold into the evaluator's episode records
// (eval_account_safety_kernel: eval_account_body of rvo3d_eval_kernels.hpp with the fold hooked in behind the per-env
// decision).  Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
// The fold is plain C++ (__host__ __device__): tests/host/safety_account_check.hip calls it on the CPU.
#pragma once

#include "rvo3d_params.hpp"
#include "rvo3d_eval_kernels.hpp"

namespace rvo3d {

// The minimum rule of every safety value: from +inf, x < m ? x : m.  No value is ever -0.0 (rvo3d.h) or NaN for finite
// positions, so the result does not depend on the order in which the candidates meet.
__host__ __device__ inline double safety_min(double x, double m) { return x < m ? x : m; }
__host__ __device__ inline double safety_inf() { return __builtin_inf(); }

// ---- the episode fold (rvo3d_eval_account_safety) ----
struct EvalSafetyRun {
  double sep, bclear, wall;  // minima over the episode so far (+inf at its start)
  int64_t near;              // near pair-steps of the episode so far
};
// the running values with one more step in them: what a record stores when the episode ends behind this step
__host__ __device__ inline EvalSafetyRun eval_safety_fold(const EvalSafetyRun& run, const EvalSafetyRun& step) {
  return {safety_min(step.sep, run.sep), safety_min(step.bclear, run.bclear), safety_min(step.wall, run.wall),
          run.near + step.near};
}
// ... and what the env goes on with
__host__ __device__ inline EvalSafetyRun eval_safety_keep(const EvalSafetyRun& folded, bool ended) {
  return ended ? EvalSafetyRun{safety_inf(), safety_inf(), safety_inf(), 0} : folded;
}

// ---- the scan ----
struct SafetyArgs {
  double near_margin;
  double *sep, *bclear, *wall;              // [E][N], each nullable
  int32_t* near_pairs;                      // [E], nullable
  double *env_sep, *env_bclear, *env_wall;  // [E], each nullable: the minimum over the env's live drones
};

constexpr int kSafetyPackedThreads = 256;  // workgroup of the packed geometry (fleets of up to 64 drones)
// threads per workgroup, lanes per env, LDS bytes: what the host launches with and the kernel derives again
__host__ __device__ inline int safety_lanes_per_env(int n) { return n <= 64 ? eval_lanes_per_env(n) : (n + 63) / 64 * 64; }
__host__ __device__ inline int safety_threads(int n) { return n <= 64 ? kSafetyPackedThreads : (n + 63) / 64 * 64; }
constexpr int kSafetyMaxWaves = kMaxThreads / 64;
__host__ __device__ inline size_t safety_lds_bytes(int n) {
  return (size_t)safety_threads(n) * 8 * sizeof(double) + (size_t)kSafetyMaxWaves * (3 * sizeof(double) + sizeof(int32_t));
}

// One lane per drone.  Fleets of up to 64 drones: L = eval_lanes_per_env(N) consecutive lanes hold one env, 256 / L envs
// per workgroup (an env never straddles a wave); larger fleets: one env per workgroup of ceil(N / 64) waves.  Every live
// lane stages px, py, pz, r of its drone in LDS (struct-of-arrays: the lanes of one env read one address, a broadcast, and
// packed envs read addresses L * 8 B apart, which fall into different banks), then walks j over its env's slots.  The
// building records go through LDS in tiles of L per env: each lane of the env loads one record per tile.  An env's
// unused records (per-env sets: counts[e] .. nb_max - 1) hold h = -inf and fail p_z <= h like any building below the drone.
// The minima and the count are order-independent (safety_min; integer sum), so the geometry cannot show in the result.
// CNT: the env's live drones are its first counts[e]; ghost rows are written as +inf and their state is not read.
template <bool CNT>
__device__ __forceinline__ void safety_scan_body(const Params& P, const SafetyArgs& A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char safety_lds[];
  const int N = P.N, T = (int)blockDim.x, tid = (int)threadIdx.x;
  const int L = safety_lanes_per_env(N);  // == T for N > 64
  const int epb = T / L;
  const int sub = N <= 64 ? (tid >> __builtin_ctz(L)) : 0;
  const int l = tid - sub * L;
  const int64_t slot = (int64_t)blockIdx.x * epb + sub;
  const bool has_env = slot < (int64_t)P.E;
  const int64_t e = has_env ? slot : 0;
  const int n = has_env ? (CNT ? P.cold().counts[e] : N) : 0;  // the env's live drones
  const bool live = l < n;
  const int base = tid - l;  // the env's first slot

  double* s_px = reinterpret_cast<double*>(safety_lds);
  double *s_py = s_px + T, *s_pz = s_py + T, *s_r = s_pz + T;
  double *s_bx = s_r + T, *s_by = s_bx + T, *s_bh = s_by + T, *s_br = s_bh + T;
  double* s_red = s_br + T;                                                   // [3][kSafetyMaxWaves]
  int32_t* s_cnt = reinterpret_cast<int32_t*>(s_red + 3 * kSafetyMaxWaves);  // [kSafetyMaxWaves]

  const double inf = safety_inf();
  double px = 0.0, py = 0.0, pz = 0.0, r = 0.0;
  if (live) {
    const int64_t g = e * N + l;
    px = P.px()[g]; py = P.py()[g]; pz = P.pz()[g]; r = P.radius()[g];
    s_px[tid] = px; s_py[tid] = py; s_pz[tid] = pz; s_r[tid] = r;
  }
  __syncthreads();

  const bool want_pairs = A.sep || A.env_sep || A.near_pairs;
  const bool want_bld = A.bclear || A.env_bclear;
  double sep = inf, bclear = inf, wall = inf;
  int32_t near = 0;
  if (want_pairs && live) {
    for (int j = 0; j < n; ++j) {
      if (j == l) continue;
      const double rx = s_px[base + j] - px, ry = s_py[base + j] - py, rz = s_pz[base + j] - pz;
      const double d = __builtin_sqrt((ry * ry + rx * rx) + rz * rz) - (r + s_r[base + j]);
      sep = safety_min(d, sep);
      near += (j > l && d <= A.near_margin) ? 1 : 0;
    }
  }
  if (live) {
    const ColdC& C = P.cold();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double p = k == 0 ? px : (k == 1 ? py : pz);
      wall = safety_min(p, wall);
      wall = safety_min(C.map[k] - p, wall);
    }
    wall = wall + 0.0;  // -0.0 (a coordinate that is -0.0) becomes +0.0
  }
  if (want_bld) {
    const ColdC& C = P.cold();
    const int nb = C.nb;  // the same for every env: the barriers below are uniform
    const double* rec = C.bld + (size_t)e * C.bld_stride;
    for (int t0 = 0; t0 < nb; t0 += L) {
      __syncthreads();  // the tile before this one has been read
      if (has_env && t0 + l < nb) {
        const double* b = rec + (size_t)(t0 + l) * 4;
        s_bx[tid] = b[0]; s_by[tid] = b[1]; s_bh[tid] = b[2]; s_br[tid] = b[3];
      }
      __syncthreads();
      if (live) {
        const int m = nb - t0 < L ? nb - t0 : L;
        for (int k = 0; k < m; ++k) {
          if (pz <= s_bh[base + k]) {
            const double ex = px - s_bx[base + k], ey = py - s_by[base + k];
            bclear = safety_min(__builtin_sqrt(ex * ex + ey * ey) - (r + s_br[base + k]), bclear);
          }
        }
      }
    }
  }

  if (has_env && l < N) {  // ghost rows (live is false: the values are still +inf) included
    const int64_t g = e * N + l;
    if (A.sep) A.sep[g] = sep;
    if (A.bclear) A.bclear[g] = bclear;
    if (A.wall) A.wall[g] = wall;
  }
  if (!A.near_pairs && !A.env_sep && !A.env_bclear && !A.env_wall) return;

  // per env: the butterfly over the env's lanes (at most a wave; dead lanes hold +inf and 0), then one LDS step for an
  // env of several waves
  const int span = L < 64 ? L : 64;
  for (int m = span >> 1; m >= 1; m >>= 1) {
    sep = safety_min(__shfl_xor(sep, m, 64), sep);
    bclear = safety_min(__shfl_xor(bclear, m, 64), bclear);
    wall = safety_min(__shfl_xor(wall, m, 64), wall);
    near += __shfl_xor(near, m, 64);
  }
  if (L > 64) {
    const int w = tid >> 6, nwaves = T >> 6;
    if ((tid & 63) == 0) {
      s_red[w] = sep; s_red[kSafetyMaxWaves + w] = bclear; s_red[2 * kSafetyMaxWaves + w] = wall; s_cnt[w] = near;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < nwaves; ++k) {
        sep = safety_min(s_red[k], sep);
        bclear = safety_min(s_red[kSafetyMaxWaves + k], bclear);
        wall = safety_min(s_red[2 * kSafetyMaxWaves + k], wall);
        near += s_cnt[k];
      }
    }
  }
  if (has_env && l == 0) {
    if (A.near_pairs) A.near_pairs[e] = near;
    if (A.env_sep) A.env_sep[e] = sep;
    if (A.env_bclear) A.env_bclear[e] = bclear;
    if (A.env_wall) A.env_wall[e] = wall;
  }
}
__global__ void __launch_bounds__(kMaxThreads) safety_scan_kernel(const Params P, const SafetyArgs A) {
  safety_scan_body<false>(P, A);
}
__global__ void __launch_bounds__(kMaxThreads) safety_scan_counted_kernel(const Params P, const SafetyArgs A) {
  safety_scan_body<true>(P, A);
}

// ---- rvo3d_eval_account_safety: eval_account_body with this hook behind the per-env decision ----
struct EvalSafetyArgs {
  const double *step_sep, *step_bclear, *step_wall;  // [E]: this step's per-env values (the scan's env_* outputs)
  const int32_t* step_near;
  double *ep_min_sep, *ep_min_bclear, *ep_min_wall;  // [E] running
  int64_t* ep_near;
  double *rec_min_sep, *rec_min_bclear, *rec_min_wall;  // [E][quota] records
  int64_t* rec_near;
  int32_t quota;
};
struct EvalSafetyFold {
  EvalSafetyArgs S;
  // slot_before: counted[e] before this step, the record's slot when o.record
  __device__ __forceinline__ void operator()(int64_t e, int32_t slot_before, const EvalEnvOut& o) const {
    const EvalSafetyRun run{S.ep_min_sep[e], S.ep_min_bclear[e], S.ep_min_wall[e], S.ep_near[e]};
    const EvalSafetyRun step{S.step_sep[e], S.step_bclear[e], S.step_wall[e], (int64_t)S.step_near[e]};
    const EvalSafetyRun f = eval_safety_fold(run, step);
    if (o.record) {
      const int64_t r = e * S.quota + slot_before;
      S.rec_min_sep[r] = f.sep; S.rec_min_bclear[r] = f.bclear; S.rec_min_wall[r] = f.wall; S.rec_near[r] = f.near;
    }
    const EvalSafetyRun k = eval_safety_keep(f, o.ended);
    S.ep_min_sep[e] = k.sep; S.ep_min_bclear[e] = k.bclear; S.ep_min_wall[e] = k.wall; S.ep_near[e] = k.near;
  }
};
__global__ void __launch_bounds__(kEvalAccountThreads) eval_account_safety_kernel(const Params P, const EvalAccountArgs A,
                                                                                  const EvalSafetyArgs S) {
  eval_account_body<false>(P, A, EvalSafetyFold{S});
}
__global__ void __launch_bounds__(kEvalAccountThreads) eval_account_safety_counted_kernel(const Params P,
                                                                                          const EvalAccountArgs A,
                                                                                          const EvalSafetyArgs S) {
  eval_account_body<true>(P, A, EvalSafetyFold{S});
}

}  // namespace rvo3d
