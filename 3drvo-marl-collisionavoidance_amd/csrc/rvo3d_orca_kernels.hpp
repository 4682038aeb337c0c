// rvo3d_orca_kernels.hpp -- the ORCA velocity of every drone (include/rvo3d.h: rvo3d_orca_vel) and the converter from a
// wanted velocity to the step's action (rvo3d_vel_command).  The rules - the plane of a pair, the four linear programs,
// the selection slots, the converter, the argument checks - are plain C++ in rvo3d_orca_rules.hpp; this file is the
// launch geometry around them.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
#pragma once

#include "../../include/rvo3d.h"
#include "rvo3d_building_kernels.hpp"
#include "rvo3d_orca_rules.hpp"

namespace rvo3d {

struct OrcaArgs {
  double tau, time_step, max_speed, pref_speed, nd2;  // nd2 = neighbor_dist * neighbor_dist
  double reach, below, clear_xy;
  int32_t max_neighbors, max_buildings;
  double* out;
  int32_t *n_neighbors, *n_buildings, *status;
  double* slack;
  double* ws;      // the handle's plane workspace, [slot][6][ws_ld] doubles
  size_t ws_ld;    // E * N
};

// A lane's planes in the workspace: component c of slot s at base[(s * 6 + c) * ld], base = ws + the lane's row - the
// lanes of a wave that walk the planes together read consecutive doubles.
struct OrcaWsStore {
  double* base;
  size_t ld;
  __device__ __forceinline__ OrcaPlane get(int s) const {
    const double* p = base + (size_t)s * 6 * ld;
    return OrcaPlane{{p[0], p[ld], p[2 * ld]}, {p[3 * ld], p[4 * ld], p[5 * ld]}};
  }
  __device__ __forceinline__ void put(int s, const OrcaPlane& q) const {
    double* p = base + (size_t)s * 6 * ld;
    p[0] = q.point.x; p[ld] = q.point.y; p[2 * ld] = q.point.z;
    p[3 * ld] = q.normal.x; p[4 * ld] = q.normal.y; p[5 * ld] = q.normal.z;
  }
};
// slots a call needs: its planes, then the fallback's projected planes (one fewer)
__host__ __device__ inline int orca_ws_slots(int max_neighbors, int max_buildings) {
  return 2 * (max_neighbors + max_buildings) - 1;
}
__host__ __device__ inline size_t orca_lds_bytes(int T) { return (size_t)T * 11 * sizeof(double); }

// ---- what orca_body and shield_body (rvo3d_shield_kernels.hpp) share: the neighbour scan, the building gate and the
// plane construction, on the env's drone records in LDS (x y z vx vy vz r, [T] each).  `work`: the lane wants planes.

// Rule 2: the nearest neighbours among the env's N drones.
__device__ __forceinline__ void orca_scan_neighbors(const double* lx, int T, int N, int d, bool work, const Drone& S,
                                                    double nd2, OrcaSlots<kOrcaMaxNeighbors>& nbr) {
  orca_slots_clear(nbr);
  if (work) {
    for (int j = 0; j < N; ++j) {
      if (j == d) continue;
      const double rx = lx[j] - S.x, ry = lx[T + j] - S.y, rz = lx[2 * T + j] - S.z;
      const double d2 = (rx * rx + ry * ry) + rz * rz;
      if (d2 < nd2) orca_slots_insert(nbr, d2, j);
    }
  }
}

// Rule 3: the nearest buildings that pass the gate, the env's nb records staged in tiles of T.  Every lane of the
// workgroup calls it: it holds barriers (nb is the same for every env).
__device__ __forceinline__ void orca_gate_buildings(const double* rec, int nb, int T, int d, bool work, const Drone& S,
                                                    double reach, double below, double* s_bx, double* s_by, double* s_bh,
                                                    double* s_br, OrcaSlots<kOrcaMaxBuildings>& bs) {
  orca_slots_clear(bs);
  for (int t0 = 0; t0 < nb; t0 += T) {
    __syncthreads();  // the tile before this one has been read
    if (t0 + d < nb) {
      const double* b = rec + (size_t)(t0 + d) * 4;
      s_bx[d] = b[0]; s_by[d] = b[1]; s_bh[d] = b[2]; s_br[d] = b[3];
    }
    __syncthreads();
    if (!work) continue;
    const int m = nb - t0 < T ? nb - t0 : T;
    for (int j = 0; j < m; ++j) {
      const BuildingPair q = building_pair(S.x, S.y, S.z, S.r, s_bx[j], s_by[j], s_bh[j], s_br[j], reach, below);
      if (q.pass) orca_slots_insert(bs, q.gap, t0 + j);
    }
  }
}

// Rules 4 and 5: the planes, buildings first.  share(j): what the lane takes of the avoidance of neighbour j.
template <class Share>
__device__ __forceinline__ void orca_put_planes(const OrcaWsStore& planes, const double* lx, int T, int e, const Drone& S,
                                                const OrcaSlots<kOrcaMaxNeighbors>& nbr, int kn,
                                                const OrcaSlots<kOrcaMaxBuildings>& bs, int kb, const double* rec, int nb,
                                                const BuildingVelArgs& V, double tau, double time_step, double clear_xy,
                                                Share share) {
  const OrcaV3 vi = orca_v3(S.vx, S.vy, S.vz);
  int branch;
#pragma unroll 1
  for (int i = 0; i < kb; ++i) {
    const int32_t idx = orca_slots_index(bs, i);  // (a kept index is a live record of env e: below nb, never a filler)
    const double* b = rec + (size_t)idx * 4;
    const double bx = b[0], by = b[1];
    MotionVel vb{0.0, 0.0};
    if (V.speed) {
      const size_t m = (size_t)e * (size_t)nb + (size_t)idx;
      vb = motion_velocity(bx, by, V.leg[m], V.ends + m * 4, V.speed[m], V.dt);
    }
    planes.put(i, orca_plane(orca_v3(bx - S.x, by - S.y, 0.0), orca_v3(S.vx - vb.x, S.vy - vb.y, 0.0),
                             (S.r + b[3]) + clear_xy, tau, time_step, 1.0, vi, &branch));
  }
#pragma unroll 1
  for (int i = 0; i < kn; ++i) {
    const int32_t j = orca_slots_index(nbr, i);
    planes.put(kb + i, orca_plane(orca_v3(lx[j] - S.x, lx[T + j] - S.y, lx[2 * T + j] - S.z),
                                  orca_v3(S.vx - lx[3 * T + j], S.vy - lx[4 * T + j], S.vz - lx[5 * T + j]),
                                  S.r + lx[6 * T + j], tau, time_step, share(j), vi, &branch));
  }
}

// rvo_city_body's geometry: one workgroup per env, one lane per drone, T = align_up(N, 64) threads.  LDS: the env's drone
// records (x y z vx vy vz r, 7 T doubles), which the neighbour scan and then the drone planes read, and behind them the
// building records in tiles of T (x y h r, 4 T doubles) for the gate.  The sorted slots (16 neighbours, 8 buildings)
// stay in registers; the velocity of a building is computed for the at most max_buildings a lane keeps
// (building_rows_body's way), not for every record of a tile: the planes cannot be made before the selection is final.
// A lane's planes - at most 24, and 23 projected ones in the fallback - are indexed by run-time values in all four
// programs: they live in the handle's global workspace (OrcaWsStore), which serves every T; as a private array they
// would be scratch, and in LDS they fit up to T = 128 only (profiles/orca/measurements.txt).
template <bool CNT>
__device__ __forceinline__ void orca_body(const Params& P, const OrcaArgs& Y, const BuildingVelArgs& V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = threadIdx.x, e = blockIdx.x;
  const int N = CNT ? live_drones(P, e) : P.N;  // the drones the env has
  const int T = blockDim.x;
  double* const lx = reinterpret_cast<double*>(smem);  // x y z vx vy vz r, [T] each
  double *const s_bx = lx + 7 * T, *const s_by = lx + 8 * T, *const s_bh = lx + 9 * T, *const s_br = lx + 10 * T;
  const bool active = d < N;
  const int g = active ? e * P.N + d : e * P.N;
  const int row = d < P.N ? e * P.N + d : -1;  // the lane's output row
  Drone S;
  S.x = P.px()[g]; S.y = P.py()[g]; S.z = P.pz()[g];
  S.vx = P.vx()[g]; S.vy = P.vy()[g]; S.vz = P.vz()[g];
  S.r = P.radius()[g];
  lx[d] = S.x; lx[T + d] = S.y; lx[2 * T + d] = S.z;
  lx[3 * T + d] = S.vx; lx[4 * T + d] = S.vy; lx[5 * T + d] = S.vz;
  lx[6 * T + d] = S.r;
  __syncthreads();

  // ---- rule 2: the nearest neighbours ----
  OrcaSlots<kOrcaMaxNeighbors> nbr;
  orca_scan_neighbors(lx, T, N, d, active, S, Y.nd2, nbr);

  // ---- rule 3: the nearest buildings that pass the gate ----
  const ColdC& C = P.cold();
  const int nb = C.nb;  // the same for every env: the barriers of the gate are uniform
  const double* const rec = C.bld + (size_t)e * C.bld_stride;
  OrcaSlots<kOrcaMaxBuildings> bs;
  orca_gate_buildings(rec, nb, T, d, active, S, Y.reach, Y.below, s_bx, s_by, s_bh, s_br, bs);
  // (no barrier from here on)

  if (!active) {  // a ghost's row, or a lane past the env's rows
    if (!CNT || row < 0) return;
    const size_t q = (size_t)row;
    double* o = Y.out + 3 * q;
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
    if (Y.n_neighbors) Y.n_neighbors[q] = 0;
    if (Y.n_buildings) Y.n_buildings[q] = 0;
    if (Y.status) Y.status[q] = 0;
    if (Y.slack) Y.slack[q] = 0.0;
    return;
  }

  // ---- rules 4 and 5: the planes, buildings first ----
  const int kb = bs.seen < Y.max_buildings ? bs.seen : Y.max_buildings;
  const int kn = nbr.seen < Y.max_neighbors ? nbr.seen : Y.max_neighbors;
  const OrcaWsStore planes{Y.ws + (size_t)g, Y.ws_ld};
  const OrcaWsStore proj{Y.ws + (size_t)g + (size_t)(Y.max_neighbors + Y.max_buildings) * 6 * Y.ws_ld, Y.ws_ld};
  orca_put_planes(planes, lx, T, e, S, nbr, kn, bs, kb, rec, nb, V, Y.tau, Y.time_step, Y.clear_xy,
                  [](int) { return 0.5; });  // every drone takes half

  // ---- rules 1 and 6 ----
  double cur[3], des[3];
  load3(P.cur(0), P.cur(1), P.cur(2), g, cur);
  const double p[3] = {S.x, S.y, S.z};
  des_vel(P, p, cur, des);
  const OrcaV3 pref = orca_v3(Y.pref_speed * des[0], Y.pref_speed * des[1], Y.pref_speed * des[2]);
  const OrcaResult r = orca_solve(planes, proj, kb + kn, kb, Y.max_speed, pref);
  double* w = Y.out + 3 * (size_t)g;
  w[0] = r.v.x; w[1] = r.v.y; w[2] = r.v.z;
  if (Y.n_neighbors) Y.n_neighbors[g] = kn;
  if (Y.n_buildings) Y.n_buildings[g] = kb;
  if (Y.status) Y.status[g] = r.status;
  if (Y.slack) Y.slack[g] = r.slack;
}
__global__ void __launch_bounds__(512) orca_kernel(const Params P, const OrcaArgs Y, const BuildingVelArgs V) {
  orca_body<false>(P, Y, V);
}
__global__ void __launch_bounds__(512) orca_counted_kernel(const Params P, const OrcaArgs Y, const BuildingVelArgs V) {
  orca_body<true>(P, Y, V);
}

// ---- rvo3d_vel_command: one lane per drone row ----
template <bool CNT>
__device__ __forceinline__ void vel_command_body(const Params& P, const double* want, double* action, uint8_t* clipped) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.E * P.N) return;
  double a[3] = {0.0, 0.0, 0.0};
  unsigned bits = 0u;
  bool ghost = false;
  if (CNT) {
    const int e = g / P.N;
    ghost = g - e * P.N >= live_drones(P, e);
  }
  if (!ghost) {
    const double* w = want + 3 * (size_t)g;
    bits = vel_command(P.vx()[g], P.vy()[g], P.vz()[g], P.yaw()[g], P.pitch()[g], w[0], w[1], w[2], a);
  }
  double* o = action + 3 * (size_t)g;
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
  if (clipped) clipped[g] = (uint8_t)bits;
}
__global__ void vel_command_kernel(const Params P, const double* want, double* action, uint8_t* clipped) {
  vel_command_body<false>(P, want, action, clipped);
}
__global__ void vel_command_counted_kernel(const Params P, const double* want, double* action, uint8_t* clipped) {
  vel_command_body<true>(P, want, action, clipped);
}

}  // namespace rvo3d
