// rvo3d_route_kernels.hpp -- Routes re-drawn on the device: the handle's routes replaced per env from device memory
// (set_routes_kernel), read back in the layout rvo3d_load_world takes (get_routes_kernel), and separated start / goal
// pairs per env from a counter-based generator (sample_routes_kernel; the batched counterpart of
// uaisa_env/world/random_start_end.py: random pairs with a minimum separation).  Off the hot path.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
#pragma once

#include "rvo3d_aux_kernels.hpp"
#include "rvo3d_rollout_kernels.hpp"

namespace rvo3d {

// ---- rvo3d_set_routes ------------------------------------------------------------------------------
// One workgroup per env, one lane per drone (64 * ceil(N / 64) lanes).  A masked env ends up as rvo3d_load_world leaves
// an env with these routes: the waypoint rows padded with the destination, n_points, the route length
// (drone.calculate_total_length, drone.py:409-429, legs in order as stage_world adds them), extra_len = 0, the reset
// state's des_vel and deviation (dv0_drone) and the reset state itself (reset_drone).  The workgroup votes on its env's
// n_points before the first store: one entry outside 2..P leaves the env as it was and raises RVO3D_FLAG_BAD_ROUTE.
constexpr uint32_t kFlagBadRoute = 4u;  // RVO3D_FLAG_BAD_ROUTE (include/rvo3d.h)

__global__ void __launch_bounds__(kMaxThreads) set_routes_kernel(const Params P, const uint8_t* env_mask,
                                                                 const double* wp_in, const int32_t* np_in) {
  const int e = blockIdx.x, d = threadIdx.x;
  if (env_mask && !env_mask[e]) return;  // the whole workgroup: no barrier is left behind
  const bool active = d < P.N;
  const int g = e * P.N + (active ? d : 0);
  const int np = np_in[g];
  if (__syncthreads_or(np < 2 || np > P.P)) {
    if (d == 0) atomicOr(P.err, kFlagBadRoute);
    return;
  }
  if (!active) return;
  const double* src = wp_in + (size_t)g * P.P * 3;
  double total = 0.0;
  for (int k = 0; k < P.P; ++k) {
    const int kk = k < np ? k : np - 1;  // pad with the destination
    const double x = src[kk * 3], y = src[kk * 3 + 1], z = src[kk * 3 + 2];
    P.wp(k, 0)[g] = x; P.wp(k, 1)[g] = y; P.wp(k, 2)[g] = z;
    if (k + 1 < np) {
      const double dx = src[(k + 1) * 3] - x, dy = src[(k + 1) * 3 + 1] - y, dz = src[(k + 1) * 3 + 2] - z;
      total += __builtin_sqrt(sq(dx) + sq(dy) + sq(dz));
    }
  }
  P.n_points()[g] = np;
  P.route_len()[g] = total;
  P.extra_len()[g] = 0.0;
  dv0_drone(P, g);    // reads the rows this lane has just stored
  reset_drone(P, g);
}

// rvo3d_get_routes: the waypoint rows as stored (padding included), [E][N][P][3]
__global__ void get_routes_kernel(const Params P, double* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.E * P.N) return;
  double* dst = out + (size_t)g * P.P * 3;
  for (int k = 0; k < P.P; ++k) {
    double v[3];
    load_wp(P, g, k, v);
    dst[3 * k] = v[0]; dst[3 * k + 1] = v[1]; dst[3 * k + 2] = v[2];
  }
}

// ---- rvo3d_sample_routes ---------------------------------------------------------------------------
// The rules (include/rvo3d.h has them in full; rvo3d_amd/routes.py restates them in numpy, bit for bit):
//   Candidate(kind, e, d, t) = the Philox4x32-10 block of counter (low word of env_offset + e, d, t + kind * 2^31, draw),
//   key = seed; coord_k = rint((lo_k + u_k * (hi_k - lo_k)) * 100) / 100 with u_k = (x_k + 0.5) * 2^-32, every operation
//   rounded on its own (the library is built with -ffp-contract=off).  In round t every unplaced drone d takes its
//   candidate c_d and is accepted iff c_d is min_sep away from every point placed in an earlier round and from the
//   candidate of every j < d unplaced at the start of the round, and - ends - min_len away from its own start.
// One workgroup per env, one lane per drone.  LDS holds ONE point per drone - its candidate of this round while it is
// unplaced, its place afterwards (the candidate it was accepted with: nothing is copied) - and the round's unplaced
// flags; every unplaced lane walks the others.  The rounds end when a workgroup-wide vote finds nobody unplaced; no round
// after that could change anything, so the result does not depend on the exit.  No atomics, no global scratch.
struct SampleRoutesArgs {
  double lo[3], span[3];  // span = hi - lo
  double sep2, len2;      // min_sep^2, min_len^2
  int32_t max_tries, N, P;
  uint32_t draw, k0, k1;  // key = seed
  int64_t env_offset;
  const uint8_t* env_mask;
  double* wp;             // [E][N][P][3]
  int32_t* n_points;      // [E][N]
  int32_t* unplaced;      // [E], nullable
};

__device__ __forceinline__ double dist2(const double a[3], double bx, double by, double bz) {
  const double dx = a[0] - bx, dy = a[1] - by, dz = a[2] - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(kMaxThreads) sample_routes_kernel(const SampleRoutesArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int e = blockIdx.x, d = threadIdx.x, T = blockDim.x, N = A.N;
  if (A.env_mask && !A.env_mask[e]) return;  // the whole workgroup
  double* const px = reinterpret_cast<double*>(smem);  // x y z, [T] each
  double* const py = px + T;
  double* const pz = py + T;
  uint8_t* const unf = reinterpret_cast<uint8_t*>(pz + T);  // [T] unplaced at the start of the round
  const bool active = d < N;
  const uint32_t c0 = (uint32_t)(uint64_t)(A.env_offset + e);
  double pt[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // this drone's start and end
  int left = 0;
  for (int kind = 0; kind < 2; ++kind) {
    bool un = active;
    double c[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < A.max_tries; ++t) {
      if (un) {
        uint32_t x[4];
        philox4x32_10(c0, (uint32_t)d, (uint32_t)t + ((uint32_t)kind << 31), A.draw, A.k0, A.k1, x);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double u = ((double)x[k] + 0.5) * 2.3283064365386963e-10;  // 2^-32
          c[k] = __builtin_rint((A.lo[k] + u * A.span[k]) * 100.0) / 100.0;
        }
        px[d] = c[0]; py[d] = c[1]; pz[d] = c[2];
      }
      unf[d] = un ? 1 : 0;
      __syncthreads();
      bool ok = true;
      if (un) {
        for (int j = 0; j < N; ++j) {
          if (j == d || (unf[j] && j > d)) continue;  // a later drone's candidate does not count
          if (dist2(c, px[j], py[j], pz[j]) < A.sep2) ok = false;
        }
        if (kind == 1 && !(dist2(c, pt[0][0], pt[0][1], pt[0][2]) >= A.len2)) ok = false;
      }
      const int more = __syncthreads_or(un && !ok);  // also: every read of this round precedes the next round's stores
      if (un && ok) un = false;
      if (!more) break;
    }
    pt[kind][0] = c[0]; pt[kind][1] = c[1]; pt[kind][2] = c[2];  // placed, or the last round's candidate
    left += __syncthreads_count(un);
  }
  if (A.unplaced && d == 0) A.unplaced[e] = left;
  if (!active) return;
  const size_t g = (size_t)e * N + d;
  double* dst = A.wp + g * A.P * 3;
  for (int k = 0; k < A.P; ++k) {
    const int q = k == 0 ? 0 : 1;
    dst[3 * k] = pt[q][0]; dst[3 * k + 1] = pt[q][1]; dst[3 * k + 2] = pt[q][2];
  }
  A.n_points[g] = 2;
}

}  // namespace rvo3d
