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

// CNT (set_routes_counted_kernel, a handle with drone counts): the env's live drones alone vote and take their new
// routes; the ghosts' input rows are not read and their routes stay.
template <bool CNT>
__device__ __forceinline__ void set_routes_body(const Params P, const uint8_t* env_mask, const double* wp_in,
                                                const int32_t* np_in) {
  const int e = blockIdx.x, d = threadIdx.x;
  if (env_mask && !env_mask[e]) return;  // the whole workgroup: no barrier is left behind
  const bool active = d < (CNT ? live_drones(P, e) : P.N);
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
__global__ void __launch_bounds__(kMaxThreads) set_routes_kernel(const Params P, const uint8_t* env_mask,
                                                                 const double* wp_in, const int32_t* np_in) {
  set_routes_body<false>(P, env_mask, wp_in, np_in);
}
__global__ void __launch_bounds__(kMaxThreads) set_routes_counted_kernel(const Params P, const uint8_t* env_mask,
                                                                         const double* wp_in, const int32_t* np_in) {
  set_routes_body<true>(P, env_mask, wp_in, np_in);
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

// ---- the city of rvo3d_sample_routes_city / rvo3d_plan_routes ------------------------------------------
// rvo3d_city (include/rvo3d.h) as the kernels take it.  Env e sees records 0 .. count(e)-1 of bld + e * stride; a record
// (x, y, h, r) is used as (x, y, top = h + clear_z, R = r + clear_xy): two additions, each rounded once, whoever does
// them.  An env with at most kCityLdsCap records has them staged in LDS in that derived form, once, before the per-lane
// work; a longer list is read from global memory record by record (every lane reads the same record: one broadcast
// line).  The cap: 256 records = 8 KiB, five times the 50 buildings of the measured city and a sixth of what would
// start to cost the sampler's workgroups residency.
constexpr int kCityLdsCap = 256;

struct CityArgs {
  const double* bld;      // [E or 1][nb_max][4]; NULL: no buildings
  const int32_t* counts;  // [E], nullable
  int64_t stride;         // doubles per env: 0 or nb_max * 4
  int32_t nb_max;
  double clear_xy, clear_z, pad;
};

// what a workgroup knows of its env's city
struct CityView {
  const double* g;  // the env's records in global memory
  int nb;
  bool staged;      // the derived records are in LDS
  double clear_xy, clear_z;
};

// counts[e] comes from device memory the host cannot check: clamped to 0 .. nb_max, so no read leaves the list
__device__ __forceinline__ CityView city_of_env(const CityArgs& C, int e) {
  CityView V;
  int nb = C.bld ? C.nb_max : 0;
  if (nb > 0 && C.counts) {
    const int c = C.counts[e];
    nb = c < 0 ? 0 : (c < nb ? c : nb);
  }
  V.nb = nb;
  V.g = nb > 0 ? C.bld + (int64_t)e * C.stride : nullptr;
  V.staged = nb <= kCityLdsCap;
  V.clear_xy = C.clear_xy; V.clear_z = C.clear_z;
  return V;
}

// every lane of the workgroup calls this (it holds a barrier); lds: room for min(nb_max, kCityLdsCap) records
__device__ __forceinline__ void stage_city(const CityView& V, double* lds) {
  if (V.staged)
    for (int i = threadIdx.x; i < V.nb; i += blockDim.x) {
      const double* r = V.g + 4 * i;
      lds[4 * i] = r[0]; lds[4 * i + 1] = r[1]; lds[4 * i + 2] = r[2] + V.clear_z; lds[4 * i + 3] = r[3] + V.clear_xy;
    }
  __syncthreads();
}

__device__ __forceinline__ void city_building(const CityView& V, const double* lds, int i, double& x, double& y,
                                              double& top, double& R) {
  if (V.staged) {
    x = lds[4 * i]; y = lds[4 * i + 1]; top = lds[4 * i + 2]; R = lds[4 * i + 3];
  } else {
    const double* r = V.g + 4 * i;
    x = r[0]; y = r[1]; top = r[2] + V.clear_z; R = r[3] + V.clear_xy;
  }
}

// inside(p, b) for any building b of the env
__device__ __forceinline__ bool inside_any(const CityView& V, const double* lds, const double p[3]) {
  bool in = false;
  for (int i = 0; i < V.nb; ++i) {
    double x, y, top, R;
    city_building(V, lds, i, x, y, top, R);
    const double fx = p[0] - x, fy = p[1] - y;
    if ((fx * fx + fy * fy) < R * R && p[2] <= top) in = true;
  }
  return in;
}

// kCity: rule 3 (d) of rvo3d_sample_routes_city - a candidate inside a building of its env is refused (it still counts
// as c_j for the drones behind it: the vote below does not look at why a candidate fell).  The building records sit
// between the points and the flags in LDS; without kCity there are none and this is rvo3d_sample_routes' kernel.
template <bool kCity>
__device__ __forceinline__ void sample_routes_body(const SampleRoutesArgs& A, const CityArgs& city) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int e = blockIdx.x, d = threadIdx.x, T = blockDim.x, N = A.N;
  if (A.env_mask && !A.env_mask[e]) return;  // the whole workgroup
  double* const px = reinterpret_cast<double*>(smem);  // x y z, [T] each
  double* const py = px + T;
  double* const pz = py + T;
  double* const bl = pz + T;  // kCity: [min(nb_max, kCityLdsCap)][4]
  const int nbl = kCity ? (city.nb_max < kCityLdsCap ? city.nb_max : kCityLdsCap) : 0;
  uint8_t* const unf = reinterpret_cast<uint8_t*>(bl + 4 * nbl);  // [T] unplaced at the start of the round
  CityView V{};
  if (kCity) {
    V = city_of_env(city, e);
    stage_city(V, bl);
  }
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
        if (kCity && inside_any(V, bl, c)) ok = false;
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

__global__ void __launch_bounds__(kMaxThreads) sample_routes_kernel(const SampleRoutesArgs A) {
  sample_routes_body<false>(A, CityArgs{});
}

__global__ void __launch_bounds__(kMaxThreads) sample_routes_city_kernel(const SampleRoutesArgs A, const CityArgs city) {
  sample_routes_body<true>(A, city);
}

// ---- rvo3d_plan_routes -----------------------------------------------------------------------------
// The detour planner (include/rvo3d.h has the rules in full; CityRoutePlanner.plan_numpy restates them, bit for bit):
// a leg that crosses a building's clearance cylinder gets a waypoint beside the first such building, at the height the
// leg has where it is nearest to the axis, and the shortened leg is tested again - until the route is clear, the rows
// are used up or a rule gives up (the drone is then counted in `blocked`).  The batched counterpart of the reference's
// offline Theta* run (uaisa_env/world/theta_star_3D.py), not a port of it.
// One workgroup per env, one lane per drone.  The env's building records are staged in LDS once (city_of_env /
// stage_city above); the lanes then walk their own routes and are at different legs, so no barrier sits inside the
// loop: the one behind it counts the failed drones.  A lane's points live in private memory while max_points <=
// kPlanPrivatePoints, in its own rows of `waypoints` otherwise - the same code over RoutePts::at().
constexpr int kPlanPrivatePoints = 16;

struct PlanRoutesArgs {
  CityArgs city;
  int32_t N, P;
  const uint8_t* env_mask;
  double* wp;             // [E][N][P][3], in place
  int32_t* n_points;      // [E][N]
  int32_t* blocked;       // [E], nullable
  uint8_t* blocked_mask;  // [E][N], nullable
};

template <bool kPrivate> struct RoutePts;
template <> struct RoutePts<true> {
  double v[kPlanPrivatePoints * 3];
  __device__ __forceinline__ explicit RoutePts(double*) {}
  __device__ __forceinline__ double* at(int k) { return v + 3 * k; }
};
template <> struct RoutePts<false> {
  double* rows;
  __device__ __forceinline__ explicit RoutePts(double* r) : rows(r) {}
  __device__ __forceinline__ double* at(int k) { return rows + 3 * k; }
};

// the header's max(x, y) and min(x, y)
__device__ __forceinline__ double pick_max(double x, double y) { return x > y ? x : y; }
__device__ __forceinline__ double pick_min(double x, double y) { return x < y ? x : y; }
__device__ __forceinline__ double round2(double v) { return __builtin_rint(v * 100.0) / 100.0; }

template <bool kPrivate>
__global__ void __launch_bounds__(kMaxThreads) plan_routes_kernel(const PlanRoutesArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int e = blockIdx.x, d = threadIdx.x, P = A.P;
  if (A.env_mask && !A.env_mask[e]) return;  // the whole workgroup
  double* const bl = reinterpret_cast<double*>(smem);  // [min(nb_max, kCityLdsCap)][4]
  const CityView V = city_of_env(A.city, e);
  stage_city(V, bl);
  bool failed = false;
  if (d < A.N) {
    const size_t g = (size_t)e * A.N + d;
    double* const rows = A.wp + g * P * 3;
    RoutePts<kPrivate> pts(rows);
    if (kPrivate)
      for (int k = 0; k < 6; ++k) pts.at(0)[k] = rows[k];
    int len = 2, i = 0;
    while (i < len - 1) {
      const double ax = pts.at(i)[0], ay = pts.at(i)[1], az = pts.at(i)[2];
      const double bx = pts.at(i + 1)[0], by = pts.at(i + 1)[1], bz = pts.at(i + 1)[2];
      const double dx = bx - ax, dy = by - ay, dz = bz - az;
      const double a = dx * dx + dy * dy;
      // FirstBlocker: index order, strict <
      int first = -1;
      double ft0 = 0.0, ftc = 0.0;
      for (int b = 0; b < V.nb; ++b) {
        double x, y, top, R;
        city_building(V, bl, b, x, y, top, R);
        const double fx = ax - x, fy = ay - y;
        const double c = (fx * fx + fy * fy) - R * R;
        double t0 = 0.0, tc = 0.0;
        bool blk;
        if (a == 0.0) {
          blk = c < 0.0 && pick_min(az, bz) <= top;
        } else {
          const double bq = fx * dx + fy * dy;
          const double disc = bq * bq - a * c;
          if (!(disc > 0.0)) continue;
          const double s = __builtin_sqrt(disc);
          t0 = (-bq - s) / a;
          double t1 = (-bq + s) / a;
          if (t1 <= 0.0 || t0 >= 1.0) continue;
          t0 = pick_max(t0, 0.0);
          t1 = pick_min(t1, 1.0);
          const double z0 = az + t0 * dz, z1 = az + t1 * dz;
          blk = pick_min(z0, z1) <= top;
          tc = pick_min(pick_max(-bq / a, 0.0), 1.0);
        }
        if (blk && (first < 0 || t0 < ft0)) {
          first = b; ft0 = t0; ftc = tc;
        }
      }
      if (first < 0) {
        ++i;
        continue;
      }
      if (len == P || a == 0.0) {
        failed = true;
        break;
      }
      double x, y, top, R;
      city_building(V, bl, first, x, y, top, R);
      const double l2 = __builtin_sqrt(a);
      const double qx = ax + ftc * dx, qy = ay + ftc * dy;
      double nx = qx - x, ny = qy - y;
      double nl = __builtin_sqrt(nx * nx + ny * ny);
      if (nl < 1e-6) {  // the leg runs through the axis: its left normal
        nx = -dy; ny = dx; nl = l2;
      }
      const double D = R + A.city.pad;
      const double wx = round2(x + (nx / nl) * D), wy = round2(y + (ny / nl) * D), wz = round2(az + ftc * dz);
      if ((wx == ax && wy == ay && wz == az) || (wx == bx && wy == by && wz == bz)) {
        failed = true;
        break;
      }
      for (int k = len; k > i + 1; --k) {  // insert behind pts[i]; len < P: row `len` exists
        double* to = pts.at(k);
        const double* from = pts.at(k - 1);
        to[0] = from[0]; to[1] = from[1]; to[2] = from[2];
      }
      pts.at(i + 1)[0] = wx; pts.at(i + 1)[1] = wy; pts.at(i + 1)[2] = wz;
      ++len;
    }
    for (int k = 0; k < P; ++k) {  // the points, then the goal in every row behind them
      const double* from = pts.at(k < len ? k : len - 1);
      const double px = from[0], py = from[1], pz = from[2];
      rows[3 * k] = px; rows[3 * k + 1] = py; rows[3 * k + 2] = pz;
    }
    A.n_points[g] = len;
    if (A.blocked_mask) A.blocked_mask[g] = failed ? 1 : 0;
  }
  const int nfail = __syncthreads_count(failed);
  if (A.blocked && d == 0) A.blocked[e] = nfail;
}

}  // namespace rvo3d
