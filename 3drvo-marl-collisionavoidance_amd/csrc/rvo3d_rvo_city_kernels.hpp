// rvo3d_rvo_city_kernels.hpp -- the classical RVO velocity that also keeps clear of the buildings (include/rvo3d.h:
// rvo3d_rvo_vel_city): rvo_vel_kernel's candidates, cones and tc_min, then every candidate swept against the cylinders
// of the env's buildings - standing or moving (rvo3d_move_env_buildings) - over a look-ahead horizon, and a selection in
// four tiers.  What reciprocal_vel_obs.preprocess collects as obs_list and then drops.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
// The building arithmetic (rules 1-3), the selection (rvo3d_rvo_rules.hpp: rvo_select, shared with rvo_vel_body) and the
// argument checks are plain C++ (__host__ __device__ / host):
// tests/host/rvo_city_check.hip calls them on the CPU (it defines RVO3D_RVO_CITY_RULES_ONLY: the kernels below need the
// whole device code in front of them).
#pragma once

#include "../../include/rvo3d.h"
#include "rvo3d_building_kernels.hpp"
#include "rvo3d_rvo_rules.hpp"

namespace rvo3d {

// ---- rule 2, one (building, planar candidate velocity): every operation a float64 one, rounded on its own ----
// the clearance disk of a building that passed the gate (building_pair: ex, ey = p - b)
struct CityDisk {
  double ex2, ey2;  // 2.0 * ex, 2.0 * ey
  double cq;        // (ex*ex + ey*ey) - R*R, R = (r + r_b) + clear_xy: <= 0 inside the disk now
  double H;         // h_b + clear_z
};
__host__ __device__ inline CityDisk city_disk(double ex, double ey, double r, double br, double bh, double clear_xy,
                                              double clear_z) {
  const double R = (r + br) + clear_xy;
  return CityDisk{2.0 * ex, 2.0 * ey, (ex * ex + ey * ey) - R * R, bh + clear_z};
}
// the times at which the drone's centre, moving at (wx, wy) relative to the building, is inside the disk: [t_in, t_out];
// hit false: never, or only in the past.  No NaN leaves it for finite inputs whose squares do not overflow: inside the
// disk -(4a)*cq >= 0, so the root's argument is a sum of two non-negative numbers; outside a root is taken of disc > 0
// only, and a quotient 0/0 (a == 0 by underflow) fails t_in >= 0.
struct CityRoots {
  bool hit;
  double t_in, t_out;
};
__host__ __device__ inline CityRoots city_roots(const CityDisk& k, double wx, double wy) {
  const double a = wx * wx + wy * wy;
  const double bq = k.ex2 * wx + k.ey2 * wy;
  if (k.cq <= 0.0) {
    if (a == 0.0) return CityRoots{true, 0.0, safety_inf()};
    return CityRoots{true, 0.0, (-bq + __builtin_sqrt(bq * bq - (4.0 * a) * k.cq)) / (2.0 * a)};
  }
  const double disc = bq * bq - (4.0 * a) * k.cq;
  if (disc <= 0.0) return CityRoots{false, 0.0, 0.0};
  const double s = __builtin_sqrt(disc);
  const double t_in = (-bq - s) / (2.0 * a), t_out = (-bq + s) / (2.0 * a);
  if (!(t_in >= 0.0)) return CityRoots{false, 0.0, 0.0};  // moving away
  return CityRoots{true, t_in, t_out};
}
// ... and the height: the lowest the drone is while over the disk within the horizon, against the roof
__host__ __device__ inline bool city_blocks(const CityRoots& q, double pz, double cz, double H, double horizon) {
  if (!(q.t_in <= horizon)) return false;
  const double te = q.t_out < horizon ? q.t_out : horizon;
  const double z_in = pz + cz * q.t_in, z_e = pz + cz * te;
  const double zmin = z_e < z_in ? z_e : z_in;
  return zmin <= H;
}

// ---- rule 3 ----
// Tiers 1 and 2 are rvo_vel_body's selection (rvo3d_rvo_rules.hpp: rvo_select) over live & ~blocked; its 0 is tier 3
// (every live candidate is blocked) or tier 4 (none is live), o is not written.  The rule's name, as
// tests/host/rvo_city_check.hip calls it:
template <class Val>
__host__ __device__ inline int city_select(const int* cnt, Val val, const double* des, double tc_min,
                                           unsigned long long live, unsigned long long cone, unsigned long long blocked,
                                           double* o) {
  return rvo_select(cnt, val, des, tc_min, live, cone, blocked, o);
}
// Tier 3, candidates offered in ascending c: the largest tb, then the least dd, then the first
struct CityLast {
  bool have;
  double tb, dd, v[3];
};
__host__ __device__ inline void city_last_offer(CityLast& s, double tb, double vx, double vy, double vz, const double* des) {
  const double ax = des[0] - vx, ay = des[1] - vy, az = des[2] - vz;
  const double dd = __builtin_sqrt(ax * ax + ay * ay + az * az);
  if (!s.have || tb > s.tb || (tb == s.tb && dd < s.dd)) {
    s.have = true; s.tb = tb; s.dd = dd; s.v[0] = vx; s.v[1] = vy; s.v[2] = vz;
  }
}

// ---- the argument checks of rvo3d_rvo_vel_city, before the first HIP call.  RVO3D_OK, RVO3D_ERR_INVALID or
// RVO3D_ERR_STATE with the reason in *why.  sets_attached: rvo3d_set_env_buildings is in force on the handle.
inline int rvo_city_check(const rvo3d_rvo_city_args* a, bool sets_attached, const rvo3d_building_motion* m, double dt,
                          const char** why) {
  *why = "";
  if (!a) { *why = "null rvo3d_rvo_city_args"; return RVO3D_ERR_INVALID; }
  if (!a->out_vel) { *why = "out_vel is required"; return RVO3D_ERR_INVALID; }
  if (!rvo_acceler_ok(a->acceler)) { *why = kRvoAccelerWhy; return RVO3D_ERR_INVALID; }
  if (!building_finite(a->reach) || !(a->reach > 0.0)) { *why = "reach must be finite and > 0"; return RVO3D_ERR_INVALID; }
  if (!building_finite(a->below) || !(a->below >= 0.0)) { *why = "below must be finite and >= 0"; return RVO3D_ERR_INVALID; }
  if (!building_finite(a->horizon) || !(a->horizon > 0.0)) { *why = "horizon must be finite and > 0"; return RVO3D_ERR_INVALID; }
  if (!building_finite(a->clear_xy) || !(a->clear_xy >= 0.0)) { *why = "clear_xy must be finite and >= 0"; return RVO3D_ERR_INVALID; }
  if (!building_finite(a->clear_z) || !(a->clear_z >= 0.0)) { *why = "clear_z must be finite and >= 0"; return RVO3D_ERR_INVALID; }
  if (m && !sets_attached) { *why = "a motion needs attached per-env building sets (rvo3d_set_env_buildings)"; return RVO3D_ERR_STATE; }
  if (m && (!m->ends || !m->speed || !m->leg)) { *why = "ends, speed and leg are required"; return RVO3D_ERR_INVALID; }
  if (!building_finite(dt) || !(dt >= 0.0)) { *why = "dt must be finite and >= 0"; return RVO3D_ERR_INVALID; }
  return RVO3D_OK;
}

#ifndef RVO3D_RVO_CITY_RULES_ONLY
// ---- the kernel ----
struct RvoCityArgs {
  double reach, below, horizon, clear_xy, clear_z;
  double* out;
  unsigned long long *live_mask, *cone_mask, *blocked_mask;
  double* tc_min;
  int32_t *n_gated, *tier;
};

// rvo_vel_body's geometry: one workgroup per env, one lane per drone, T = align_up(N, 64) threads, the env's drone
// records in LDS (8 T doubles).  The selection is shared with rvo_vel_body (rvo3d_rvo_rules.hpp: rvo_select).  The grid
// and the neighbour scan below still restate rvo_grid and rvo_neighbours (rvo3d_aux_kernels.hpp), which rvo_vel_body
// calls: called from here they kept 166 VGPRs, 3 waves, no scratch and a neighbour loop with the same instructions, but
// other registers in it, and on the MI355X that kernel was 3 % (acceler 0.5) to 6 % (acceler 1) slower than this text
// (profiles/rvo_side_shared/measurements.txt).  Rule 5 - nothing in reach: the row is rvo_vel's - needs the two to stay
// the same arithmetic; tests/test_rvo_vel.py holds this kernel to rvo_vel's bits on the states the oracle pins.  Behind
// the drone side the same LDS takes the building
// records in tiles of T - x y h r and the velocity the loading lane computed, 6 T doubles - which every lane reads as a
// broadcast.  The fast path keeps three 64-bit masks per lane.  Tier 3 needs tb(c) per candidate: a second trip over the
// tiles per planar candidate (ix, iy) some lane of the workgroup needs (a workgroup-wide vote through LDS: the barriers
// stay uniform), four minima in registers at a time; the planar roots are still taken once per building and (ix, iy).
template <bool CNT>
__device__ __forceinline__ void rvo_city_body(const Params& P, const RvoVelArgs& A, const RvoCityArgs& Y, const BuildingVelArgs& V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = threadIdx.x, e = blockIdx.x;
  const int N = CNT ? live_drones(P, e) : P.N;  // the drones the env has
  const int T = blockDim.x;
  double* const lx = reinterpret_cast<double*>(smem);  // x y z vx vy vz r prio, [T] each
  const bool active = d < N;
  const int g = active ? e * P.N + d : e * P.N;
  const int row = d < P.N ? e * P.N + d : -1;  // the lane's output row (kept in a register: P.N need not be)
  Drone S;
  S.x = P.px()[g]; S.y = P.py()[g]; S.z = P.pz()[g];
  S.vx = P.vx()[g]; S.vy = P.vy()[g]; S.vz = P.vz()[g];
  S.r = P.radius()[g]; S.prio = P.prio()[g];
  lx[d] = S.x; lx[T + d] = S.y; lx[2 * T + d] = S.z;
  lx[3 * T + d] = S.vx; lx[4 * T + d] = S.vy; lx[5 * T + d] = S.vz;
  lx[6 * T + d] = S.r; lx[7 * T + d] = S.prio;
  __syncthreads();
  double des[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
  int cnt[3] = {0, 0, 0};
  unsigned long long live = 0ull, inside = 0ull;
  double tc_min = __builtin_inf();
  if (active) {  // ---- the drone side: rvo_grid and rvo_neighbours, restated (see above) ----
    double cur[3];
    load3(P.cur(0), P.cur(1), P.cur(2), g, cur);
    const double p[3] = {S.x, S.y, S.z}, v0[3] = {S.vx, S.vy, S.vz};
    des_vel(P, p, cur, des);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = clampd(v0[k] - A.acceler, -A.vmax[k], A.vmax[k]);  // np.clip
      const double hi = clampd(v0[k] + A.acceler, -A.vmax[k], A.vmax[k]);
      cnt[k] = arange_len(lo[k], hi);
      if (cnt[k] > 4) cnt[k] = 4;  // host checks acceler <= 1
    }
    {
      int c = 0;
      for (int ix = 0; ix < cnt[0]; ++ix)
        for (int iy = 0; iy < cnt[1]; ++iy)
          for (int iz = 0; iz < cnt[2]; ++iz, ++c)
            if (!(__builtin_sqrt(sq(arange_at(lo[0], ix)) + sq(arange_at(lo[1], iy)) + sq(arange_at(lo[2], iz))) < 0.3))
              live |= 1ull << c;
    }
    for (int j = 0; j < N; ++j) {
      if (j == d) continue;
      const double bx = lx[j], by = lx[T + j], bz = lx[2 * T + j];
      const double fx = S.x - bx, fy = S.y - by, fz = S.z - bz;  // agent - drone (:40-43)
      if (!(dot3b(fx, fy, fz, fx, fy, fz) <= P.T10)) continue;   // norm <= 10
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
      // the shortcut of rvo_neighbours (its comment has the proof): one cos per neighbour decides the candidates away
      // from the rounding tie, the rest take the reference's own sequence
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
  }
  __syncthreads();  // the drone records have been read: their LDS takes the building tiles from here on

  // ---- the buildings ----
  const ColdC& C = P.cold();
  const int nb = C.nb;  // the same for every env: the barriers below are uniform
  const double* const rec = C.bld + (size_t)e * C.bld_stride;
  double *const s_bx = lx, *const s_by = lx + T, *const s_bh = lx + 2 * T, *const s_br = lx + 3 * T,
         *const s_wx = lx + 4 * T, *const s_wy = lx + 5 * T;
  unsigned* const s_vote = reinterpret_cast<unsigned*>(lx + 6 * T);  // one word per wave (the tiles leave it alone)
  auto load_tile = [&](int t0) {
    __syncthreads();  // the tile before this one has been read
    if (t0 + d < nb) {
      const double* b = rec + (size_t)(t0 + d) * 4;
      const double bx = b[0], by = b[1], bh = b[2];
      MotionVel vb{0.0, 0.0};
      if (V.speed && motion_live(bh)) {  // (a motion: per-env sets are attached, nb is their nb_max)
        const size_t m = (size_t)e * (size_t)nb + (size_t)(t0 + d);
        vb = motion_velocity(bx, by, V.leg[m], V.ends + m * 4, V.speed[m], V.dt);
      }
      s_bx[d] = bx; s_by[d] = by; s_bh[d] = bh; s_br[d] = b[3]; s_wx[d] = vb.x; s_wy[d] = vb.y;
    }
    __syncthreads();
  };

  unsigned long long blocked = 0ull;
  int n_gated = 0;
  for (int t0 = 0; t0 < nb; t0 += T) {
    load_tile(t0);
    if (!active) continue;
    const int m = nb - t0 < T ? nb - t0 : T;
    for (int j = 0; j < m; ++j) {
      const double bh = s_bh[j];
      const BuildingPair q = building_pair(S.x, S.y, S.z, S.r, s_bx[j], s_by[j], bh, s_br[j], Y.reach, Y.below);
      if (!q.pass) continue;
      ++n_gated;
      const CityDisk k = city_disk(q.ex, q.ey, S.r, s_br[j], bh, Y.clear_xy, Y.clear_z);
      const double vbx = s_wx[j], vby = s_wy[j];
      int c = 0;
      for (int ix = 0; ix < cnt[0]; ++ix) {
        const double wx = arange_at(lo[0], ix) - vbx;
        for (int iy = 0; iy < cnt[1]; ++iy, c += cnt[2]) {
          const unsigned long long lv = (live >> c) & ((1ull << cnt[2]) - 1ull);
          if (!lv) continue;
          const CityRoots r = city_roots(k, wx, arange_at(lo[1], iy) - vby);  // once per (ix, iy)
          if (!r.hit || !(r.t_in <= Y.horizon)) continue;
          for (int iz = 0; iz < cnt[2]; ++iz)
            if (((lv >> iz) & 1ull) && city_blocks(r, S.z, arange_at(lo[2], iz), k.H, Y.horizon)) blocked |= 1ull << (c + iz);
        }
      }
    }
  }

  // ---- selection: tiers 1, 2 and 4 here ----
  int tier = 0;
  double o[3] = {0.0, 0.0, 0.0};
  unsigned need = 0u;  // bit ix * 4 + iy: this lane wants tb of the candidates (ix, iy, .)
  if (active) {
    tier = city_select(cnt, [&](int k, int i) { return arange_at(lo[k], i); }, des, tc_min, live, inside, blocked, o);
    if (tier == 0) {
      tier = live ? 3 : 4;
      if (live)
        for (int ix = 0; ix < cnt[0]; ++ix)
          for (int iy = 0; iy < cnt[1]; ++iy) need |= 1u << (ix * 4 + iy);
    }
  }
  // the vote: every wave's OR through LDS (no atomics), then the same word in every lane
  {
    unsigned w = 0u;
#pragma unroll
    for (int p = 0; p < 16; ++p) w |= __ballot((need >> p) & 1u) ? 1u << p : 0u;
    if ((d & 63) == 0) s_vote[d >> 6] = w;
    __syncthreads();
    unsigned all = 0u;
    for (int i = 0; i < (T >> 6); ++i) all |= s_vote[i];
    all = __builtin_amdgcn_readfirstlane(all);

    // ---- tier 3 (rare): the candidate that hits last ----
    CityLast best{false, 0.0, 0.0, {0.0, 0.0, 0.0}};
    for (int p = 0; p < 16; ++p) {
      if (!((all >> p) & 1u)) continue;  // (uniform)
      const int ix = p >> 2, iy = p & 3;
      const bool mine = (need >> p) & 1u;
      const int c0 = (ix * cnt[1] + iy) * cnt[2];
      const double cx = arange_at(lo[0], ix), cy = arange_at(lo[1], iy);
      double tb[4] = {__builtin_inf(), __builtin_inf(), __builtin_inf(), __builtin_inf()};
      for (int t0 = 0; t0 < nb; t0 += T) {
        load_tile(t0);
        if (!mine) continue;
        const int m = nb - t0 < T ? nb - t0 : T;
        for (int j = 0; j < m; ++j) {
          const double bh = s_bh[j];
          const BuildingPair q = building_pair(S.x, S.y, S.z, S.r, s_bx[j], s_by[j], bh, s_br[j], Y.reach, Y.below);
          if (!q.pass) continue;
          const CityDisk k = city_disk(q.ex, q.ey, S.r, s_br[j], bh, Y.clear_xy, Y.clear_z);
          const CityRoots r = city_roots(k, cx - s_wx[j], cy - s_wy[j]);
          if (!r.hit || !(r.t_in <= Y.horizon)) continue;
#pragma unroll
          for (int iz = 0; iz < 4; ++iz)
            if (iz < cnt[2] && ((live >> (c0 + iz)) & 1ull) && city_blocks(r, S.z, arange_at(lo[2], iz), k.H, Y.horizon))
              tb[iz] = r.t_in < tb[iz] ? r.t_in : tb[iz];
        }
      }
      if (mine) {
#pragma unroll
        for (int iz = 0; iz < 4; ++iz)
          if (iz < cnt[2] && ((live >> (c0 + iz)) & 1ull)) city_last_offer(best, tb[iz], cx, cy, arange_at(lo[2], iz), des);
      }
    }
    if (tier == 3) { o[0] = best.v[0]; o[1] = best.v[1]; o[2] = best.v[2]; }
  }

  if (tier == 0) {  // not a live drone (tested on the lane's own tier: the mask of `active` need not be kept until here)
    if (!CNT || row < 0) return;  // a ghost's row:
    const size_t q = (size_t)row;
    double* o = Y.out + 3 * q;
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
    if (Y.live_mask) Y.live_mask[q] = 0ull;
    if (Y.cone_mask) Y.cone_mask[q] = 0ull;
    if (Y.blocked_mask) Y.blocked_mask[q] = 0ull;
    if (Y.tc_min) Y.tc_min[q] = 0.0;
    if (Y.n_gated) Y.n_gated[q] = 0;
    if (Y.tier) Y.tier[q] = 0;
    return;
  }
  {
    double* w = Y.out + 3 * (size_t)g;
    w[0] = o[0]; w[1] = o[1]; w[2] = o[2];
    if (Y.live_mask) Y.live_mask[g] = live;
    if (Y.cone_mask) Y.cone_mask[g] = inside;
    if (Y.blocked_mask) Y.blocked_mask[g] = blocked;
    if (Y.tc_min) Y.tc_min[g] = tc_min;
    if (Y.n_gated) Y.n_gated[g] = n_gated;
    if (Y.tier) Y.tier[g] = tier;
  }
}
// Three waves per SIMD, rvo_vel_kernel's occupancy, are asked for: left to itself the compiler takes 170 VGPRs, two over
// the 168 that allow them.  With the attribute: 166, no scratch, no spills (profiles/rvo_city/measurements.txt).
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(3)))
rvo_city_kernel(const Params P, const RvoVelArgs A, const RvoCityArgs Y, const BuildingVelArgs V) {
  rvo_city_body<false>(P, A, Y, V);
}
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(3)))
rvo_city_counted_kernel(const Params P, const RvoVelArgs A, const RvoCityArgs Y, const BuildingVelArgs V) {
  rvo_city_body<true>(P, A, Y, V);
}
#endif  // RVO3D_RVO_CITY_RULES_ONLY

}  // namespace rvo3d
