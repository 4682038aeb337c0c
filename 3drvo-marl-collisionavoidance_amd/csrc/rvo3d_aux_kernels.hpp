// rvo3d_aux_kernels.hpp -- Small kernels off the hot path: resets, waypoint / des_vel tables, des_vel, the classical
// RVO velocity selection, AoS <-> SoA copies.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
#pragma once

#include "rvo3d_step.hpp"
#include "rvo3d_rvo_rules.hpp"

namespace rvo3d {

// ---- small state kernels -------------------------------------------------------
// drone.reset (drone.py:270-291) of drone g: every field a reset writes (shared with set_routes_kernel).
__device__ __forceinline__ void reset_drone(const Params& P, int g) {
  double s[3];
  load_wp(P, g, 0, s);
  P.px()[g] = s[0]; P.py()[g] = s[1]; P.pz()[g] = s[2];
  P.vx()[g] = 0.0; P.vy()[g] = 0.0; P.vz()[g] = 0.0;
  P.wp_idx()[g] = 1; P.arrive()[g] = 0; P.dest()[g] = 0;
  P.real_len()[g] = 0.0; P.max_dev()[g] = 0.0; P.yaw()[g] = 0.0; P.pitch()[g] = 0.0;
  double c1[3];
  load_wp(P, g, 1, c1);
  store3(P.cur(0), P.cur(1), P.cur(2), g, c1);
  store3(P.prev(0), P.prev(1), P.prev(2), g, s);
  // des_vel of the start state is on file; a start state with a non-zero deviation (only
  // with non-finite waypoints) is left to the step's own dronestate
  const bool plain = P.dev0()[g] == 0.0;
  P.dvk_a()[g] = plain ? P.dv0_a()[g] : kDvInvalid;
  P.dvk_b()[g] = P.dv0_b()[g];
}
// ... for masked envs / drones.
__global__ void reset_kernel(const Params P, const uint8_t* env_mask, const uint8_t* drone_mask) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.E * P.N) return;
  if (env_mask && !env_mask[g / P.N]) return;
  if (drone_mask && !drone_mask[g]) return;
  reset_drone(P, g);
}

// ... for the envs whose drone count changes (rvo3d_set_drone_counts): as a freshly loaded handle's, extra_len included.
__global__ void reset_fresh_kernel(const Params P, const uint8_t* env_mask) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.E * P.N) return;
  if (!env_mask[g / P.N]) return;
  reset_drone(P, g);
  P.extra_len()[g] = 0.0;
}

// cur / prev from the waypoint index (rvo3d_load_world; rvo3d_set_state with wp_idx)
__global__ void wpcache_kernel(const Params P) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.E * P.N) return;
  const int np = P.n_points()[g];
  int i = P.wp_idx()[g];
  i = i < 1 ? 1 : (i > np - 1 ? np - 1 : i);  // the clamp only guards the table lookup
  double v[3];
  load_wp(P, g, i, v);
  store3(P.cur(0), P.cur(1), P.cur(2), g, v);
  load_wp(P, g, i - 1, v);
  store3(P.prev(0), P.prev(1), P.prev(2), g, v);
}

// rvo3d_load_world / rvo3d_set_routes: dronestate of a drone's reset state (drone.py:254-263 after
// drone.reset, :270-291): des_vel towards waypoint 1 and the deviation from the first leg.
__device__ __forceinline__ void dv0_drone(const Params& P, int g) {
  double p[3], cur[3], dv[3];
  load_wp(P, g, 0, p);
  load_wp(P, g, 1, cur);
  des_vel(P, p, cur, dv);
  uint32_t a, b;
  dv_encode(dv, a, b);
  P.dv0_a()[g] = a; P.dv0_b()[g] = b;
  P.dev0()[g] = deviation(p, cur, p);
}
__global__ void dv0_kernel(const Params P) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.E * P.N) return;
  dv0_drone(P, g);
}

// The live drones of env e of a handle with drone counts (rvo3d_set_drone_counts): what the *_counted kernels read.
__device__ __forceinline__ int live_drones(const Params& P, int e) { return P.cold().counts[e]; }

template <bool CNT>
__device__ __forceinline__ void des_vel_body(const Params P, double* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.E * P.N) return;
  if (CNT) {  // a ghost's row is zero
    const int e = g / P.N;
    if (g - e * P.N >= live_drones(P, e)) {
      out[3 * (size_t)g] = 0.0; out[3 * (size_t)g + 1] = 0.0; out[3 * (size_t)g + 2] = 0.0;
      return;
    }
  }
  double p[3] = {P.px()[g], P.py()[g], P.pz()[g]}, cur[3], dv[3];
  load3(P.cur(0), P.cur(1), P.cur(2), g, cur);
  des_vel(P, p, cur, dv);
  out[3 * (size_t)g] = dv[0]; out[3 * (size_t)g + 1] = dv[1]; out[3 * (size_t)g + 2] = dv[2];
}
__global__ void des_vel_kernel(const Params P, double* out) { des_vel_body<false>(P, out); }
__global__ void des_vel_counted_kernel(const Params P, double* out) { des_vel_body<true>(P, out); }

// ---- classical RVO velocity selection -----------------------------------
// uaisa_env/vel_obs/reciprocal_vel_obs.py:19-166 as intended (the class cannot run: list
// attribute assignment :109, slices :63-69/:105, missing return :119-124), built from the
// helpers it calls: get_alpha / get_PAA / get_rvo_array / get_beta / cal_exp_tim
// (vel_obs3D.py:8-66, 104-143).  PARITY UNPINNED for the driver loop; the helpers' arithmetic
// is pinned through the CPU restatement by tests/golden/rvo_vel.npz (tests/test_rvo_vel.py).
// One workgroup per env, one thread per drone; the env's records
// are staged in LDS; candidates (<= 64: acceler <= 1) are tested against every neighbour's
// velocity obstacle with one bit per candidate.
struct RvoVelArgs { double vmax[3]; double acceler; };

__device__ __forceinline__ int arange_len(double lo, double hi) {  // len(np.arange(lo, hi, 0.5))
  const double n = __builtin_ceil((hi - lo) / 0.5);
  return n > 0 ? (int)n : 0;
}
__device__ __forceinline__ double arange_at(double lo, int k) {  // numpy fills start + k * delta
  const double next = lo + 0.5;
  return k == 0 ? lo : (k == 1 ? next : lo + k * (next - lo));
}

// rvo_vel_body's drone side in three pieces: the candidate grid, the neighbour scan and the selection
// (rvo3d_rvo_rules.hpp: rvo_select).  rvo_city_body (rvo3d_rvo_city_kernels.hpp) shares the selection and restates the
// other two, for the speed of its kernel; its header comment has the figures.  A change here is a change there.

// The candidates of a drone flying at v0: per axis np.arange(lo, hi, 0.5) over the clipped [v0 - acceler, v0 + acceler],
// at most 4 values (the host checks acceler <= 1); candidate c = (ix * cnt1 + iy) * cnt2 + iz - nested loops, no
// division by the runtime counts - is live unless slower than 0.3 m/s.  Fills lo[3] and cnt[3], returns the live mask.
__device__ __forceinline__ unsigned long long rvo_grid(const RvoVelArgs& A, const double* v0, double* lo, int* cnt) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = clampd(v0[k] - A.acceler, -A.vmax[k], A.vmax[k]);  // np.clip
    const double hi = clampd(v0[k] + A.acceler, -A.vmax[k], A.vmax[k]);
    cnt[k] = arange_len(lo[k], hi);
    if (cnt[k] > 4) cnt[k] = 4;
  }
  unsigned long long live = 0ull;
  int c = 0;
  for (int ix = 0; ix < cnt[0]; ++ix)
    for (int iy = 0; iy < cnt[1]; ++iy)
      for (int iz = 0; iz < cnt[2]; ++iz, ++c)
        if (!(__builtin_sqrt(sq(arange_at(lo[0], ix)) + sq(arange_at(lo[1], iy)) + sq(arange_at(lo[2], iz))) < 0.3))
          live |= 1ull << c;
  return live;
}

// Drone d (record S) against the N - 1 others of its env, their records in LDS (lx: x y z vx vy vz r prio, [T] each),
// those within 10 m (T10: the squared gate): the least expected collision time and, one bit per live candidate, whether
// it lies inside some neighbour's velocity obstacle.
struct RvoCones {
  double tc_min;
  unsigned long long inside;
};
__device__ __forceinline__ RvoCones rvo_neighbours(const Drone S, const double* lx, int T, int N, int d, double T10,
                                                   const double* lo, const int* cnt, unsigned long long live) {
  double tc_min = __builtin_inf();
  unsigned long long inside = 0ull;
  for (int j = 0; j < N; ++j) {
    if (j == d) continue;
    const double bx = lx[j], by = lx[T + j], bz = lx[2 * T + j];
    const double fx = S.x - bx, fy = S.y - by, fz = S.z - bz;  // agent - drone (:40-43)
    if (!(dot3b(fx, fy, fz, fx, fy, fz) <= T10)) continue;     // norm <= 10
    const double bvx = lx[3 * T + j], bvy = lx[4 * T + j], bvz = lx[5 * T + j];
    const double br = lx[6 * T + j], bprio = lx[7 * T + j];
    // cal_exp_tim (vel_obs3D.py:104-143)
    {
      const double wx = S.vx - bvx, wy = S.vy - bvy, wz = S.vz - bvz, r = S.r + br;
      const double qa = sq(wx) + sq(wy) + sq(wz);
      const double qb = 2 * fx * wx + 2 * fy * wy + 2 * fz * wz;
      const double qc = sq(fx) + sq(fy) + sq(fz) - sq(r);
      double tc;
      if (qc <= 0) tc = 0.0;
      else {
        const double temp = sq(qb) - 4 * qa * qc;
        if (temp <= 0) tc = __builtin_inf();
        else {
          const double sr = __builtin_sqrt(temp);
          const double t1 = (-qb + sr) / (2 * qa), t2 = (-qb - sr) / (2 * qa);
          const double t3 = t1 >= 0 ? t1 : __builtin_inf(), t4 = t2 >= 0 ? t2 : __builtin_inf();
          tc = t3 < t4 ? t3 : t4;
        }
      }
      if (tc < tc_min) tc_min = tc;
    }
    const double ax = bx - S.x, ay = by - S.y, az = bz - S.z;  // get_rvo_array
    const double nab = norm3b(ax, ay, az);
    const double q = (S.r + br) / nab;
    const double alpha_c = (q <= 1.0) ? py_round2_c(asin(q)) : 157.0;       // get_alpha, alpha = alpha_c / 100
    const double alpha = alpha_c / 100.0;
    const double pr = S.prio / (S.prio + bprio);                            // get_PAA
    const double pax = pr * (2 * S.x + (S.vx + bvx) * 1), pay = pr * (2 * S.y + (S.vy + bvy) * 1),
                 paz = pr * (2 * S.z + (S.vz + bvz) * 1);
    // alpha > beta with beta = rint(acos(cs) * 100) / 100 holds iff rint(acos(cs) * 100) <= alpha_c - 1,
    // i.e. - away from the rounding tie - iff acos(cs) * 100 < alpha_c - 0.5, iff cs > cos((alpha_c - 0.5) / 100)
    // =: thr (> 0 for every alpha_c <= 157).  One cos per neighbour decides the candidates whose
    // cs^2 = dot |dot| / (|a|^2 |w|^2) is further than 1e-9 (relative) from thr^2 and from 1 (cs = 1 + ulp makes
    // arccos NaN: outside); the rest take the reference's own sequence.  alpha_c < 1: never inside.
    const double thr = cos((alpha_c - 0.5) / 100.0);
    const double thr2n = thr * thr * dot3b(ax, ay, az, ax, ay, az);
    const double nab2 = dot3b(ax, ay, az, ax, ay, az);
    if (alpha_c >= 1.0) {  // vo_out2 (:103-117)
      int c = 0;
      for (int ix = 0; ix < cnt[0]; ++ix) {
        const double wx = (S.x + arange_at(lo[0], ix) * 1) - pax;
        for (int iy = 0; iy < cnt[1]; ++iy) {
          const double wy = (S.y + arange_at(lo[1], iy) * 1) - pay;
          for (int iz = 0; iz < cnt[2]; ++iz, ++c) {
            if (!((live >> c) & 1ull)) continue;
            const double wz = (S.z + arange_at(lo[2], iz) * 1) - paz;
            const double dotp = dot3b(ax, ay, az, wx, wy, wz), w2 = dot3b(wx, wy, wz, wx, wy, wz);
            const double lhs = dotp * __builtin_fabs(dotp), rhs = thr2n * w2, one = nab2 * w2;
            bool in;
            if (lhs < rhs * (1.0 - 1e-9)) in = false;                          // surely cs < thr (or dot <= 0)
            else if (lhs > rhs * (1.0 + 1e-9) && lhs < one * (1.0 - 1e-9)) in = true;  // surely thr < cs < 1
            else {
              const double AB = nab * norm3b(wx, wy, wz);
              const double cs = (AB != 0) ? dotp / AB : 0.0;  // get_beta
              const double beta = __builtin_rint(acos(cs) * 100.0) / 100.0;
              in = alpha > beta;
            }
            if (in) inside |= 1ull << c;
          }
        }
      }
    }
  }
  return RvoCones{tc_min, inside};
}

// CNT (rvo_vel_counted_kernel): the env's drones are the first live_drones(P, e) of its P.N rows; the ghosts are invisible
// to them and their own rows are zero.
template <bool CNT>
__device__ __forceinline__ void rvo_vel_body(const Params P, const RvoVelArgs A, double* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = threadIdx.x, e = blockIdx.x;
  const int N = CNT ? live_drones(P, e) : P.N;  // the drones the env has
  const int T = blockDim.x;
  double* const lx = reinterpret_cast<double*>(smem);  // x y z vx vy vz r prio, [T] each
  const bool active = d < N;
  const int g = active ? e * P.N + d : e * P.N;
  if (CNT && !active && d < P.N) {
    double* o = out + 3 * ((size_t)e * P.N + d);
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
  }
  Drone S;
  S.x = P.px()[g]; S.y = P.py()[g]; S.z = P.pz()[g];
  S.vx = P.vx()[g]; S.vy = P.vy()[g]; S.vz = P.vz()[g];
  S.r = P.radius()[g]; S.prio = P.prio()[g];
  lx[d] = S.x; lx[T + d] = S.y; lx[2 * T + d] = S.z;
  lx[3 * T + d] = S.vx; lx[4 * T + d] = S.vy; lx[5 * T + d] = S.vz;
  lx[6 * T + d] = S.r; lx[7 * T + d] = S.prio;
  __syncthreads();
  if (!active) return;
  double cur[3], des[3];
  load3(P.cur(0), P.cur(1), P.cur(2), g, cur);
  const double p[3] = {S.x, S.y, S.z}, v0[3] = {S.vx, S.vy, S.vz};
  des_vel(P, p, cur, des);
  double lo[3];
  int cnt[3];
  const unsigned long long live = rvo_grid(A, v0, lo, cnt);
  const RvoCones nb = rvo_neighbours(S, lx, T, N, d, P.T10, lo, cnt, live);
  double* o = out + 3 * (size_t)g;
  if (!rvo_select(cnt, [&](int k, int i) { return arange_at(lo[k], i); }, des, nb.tc_min, live, nb.inside, 0ull, o)) {
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
  }
}
__global__ void __launch_bounds__(512) rvo_vel_kernel(const Params P, const RvoVelArgs A, double* out) {
  rvo_vel_body<false>(P, A, out);
}
__global__ void __launch_bounds__(512) rvo_vel_counted_kernel(const Params P, const RvoVelArgs A, double* out) {
  rvo_vel_body<true>(P, A, out);
}

// AoS <-> SoA copies for get_state / set_state
__global__ void aos3_to_soa(const double* src, double* x, double* y, double* z, int n) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  x[g] = src[3 * (size_t)g]; y[g] = src[3 * (size_t)g + 1]; z[g] = src[3 * (size_t)g + 2];
}
__global__ void soa_to_aos3(const double* x, const double* y, const double* z, double* dst, int n) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  dst[3 * (size_t)g] = x[g]; dst[3 * (size_t)g + 1] = y[g]; dst[3 * (size_t)g + 2] = z[g];
}

}  // namespace rvo3d
