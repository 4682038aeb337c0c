// rvo3d_shield_kernels.hpp -- the action shield (include/rvo3d.h: rvo3d_shield_action): the velocity the step would give
// every drone for its action, ORCA's planes on the current state, the program for the permitted velocity nearest to it,
// and the action handed back untouched where the two agree, replaced by the command for the permitted velocity where
// they do not.  The shield's own rules are plain C++ in rvo3d_shield_rules.hpp, the planes and programs are
// rvo3d_orca_rules.hpp's, the neighbour scan, the building gate and the plane construction are orca_body's
// (rvo3d_orca_kernels.hpp); this file is the launch geometry around them.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
#pragma once

#include "rvo3d_orca_kernels.hpp"
#include "rvo3d_shield_rules.hpp"

namespace rvo3d {

struct ShieldArgs {
  double tau, time_step, max_speed, nd2;  // nd2 = neighbor_dist * neighbor_dist
  double reach, below, clear_xy;
  int32_t max_neighbors, max_buildings;
  const double* action;
  double* out_action;
  double *pref_vel, *out_vel;
  int32_t* status;
  uint8_t* flags;
  double* slack;
  long long* totals;  // [E][4]
  double* ws;         // the handle's plane workspace, as OrcaArgs::ws
  size_t ws_ld;       // E * N
};
// orca_body's records and, behind the building tiles, the dest byte of every drone
__host__ __device__ inline size_t shield_lds_bytes(int T) { return orca_lds_bytes(T) + (size_t)T; }

// orca_body's geometry: one workgroup per env, one lane per drone, T = align_up(N, 64) threads; the env's drone records
// in LDS (7 T doubles) with the building tiles behind them (4 T doubles) and one byte per drone for its dest flag, which
// the plane construction reads for the share (S2); the selection slots in registers, the planes in the handle's
// workspace.  A lane that is not judged (S5) takes part in the barriers only.  The totals are four __syncthreads_count
// over the workgroup, added by lane 0: the workgroup owns its env's four counters.
template <bool CNT>
__device__ __forceinline__ void shield_body(const Params& P, const ShieldArgs& Y, const BuildingVelArgs& V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = threadIdx.x, e = blockIdx.x;
  const int N = CNT ? live_drones(P, e) : P.N;  // the drones the env has
  const int T = blockDim.x;
  double* const lx = reinterpret_cast<double*>(smem);  // x y z vx vy vz r, [T] each
  double *const s_bx = lx + 7 * T, *const s_by = lx + 8 * T, *const s_bh = lx + 9 * T, *const s_br = lx + 10 * T;
  uint8_t* const s_dest = reinterpret_cast<uint8_t*>(lx + 11 * T);
  const bool active = d < N;
  const int g = active ? e * P.N + d : e * P.N;
  const int row = d < P.N ? e * P.N + d : -1;  // the lane's output row
  Drone S;
  S.x = P.px()[g]; S.y = P.py()[g]; S.z = P.pz()[g];
  S.vx = P.vx()[g]; S.vy = P.vy()[g]; S.vz = P.vz()[g];
  S.r = P.radius()[g];
  const bool dest = P.dest()[g] != 0;
  lx[d] = S.x; lx[T + d] = S.y; lx[2 * T + d] = S.z;
  lx[3 * T + d] = S.vx; lx[4 * T + d] = S.vy; lx[5 * T + d] = S.vz;
  lx[6 * T + d] = S.r;
  s_dest[d] = dest ? 1 : 0;
  double a[3] = {0.0, 0.0, 0.0};
  if (row >= 0) {  // (a ghost's action is read and not used: its row is written with zeros)
    const double* A = Y.action + 3 * (size_t)row;
    a[0] = A[0]; a[1] = A[1]; a[2] = A[2];
  }
  const bool judged = shield_judged(active, dest, a);
  __syncthreads();

  // ---- S2: the planes on the current state ----
  OrcaSlots<kOrcaMaxNeighbors> nbr;
  orca_scan_neighbors(lx, T, N, d, judged, S, Y.nd2, nbr);
  const ColdC& C = P.cold();
  const int nb = C.nb;  // the same for every env: the barriers of the gate are uniform
  const double* const rec = C.bld + (size_t)e * C.bld_stride;
  OrcaSlots<kOrcaMaxBuildings> bs;
  orca_gate_buildings(rec, nb, T, d, judged, S, Y.reach, Y.below, s_bx, s_by, s_bh, s_br, bs);

  bool intervened = false, fallback = false, clipped = false;
  if (judged) {
    const int kb = bs.seen < Y.max_buildings ? bs.seen : Y.max_buildings;
    const int kn = nbr.seen < Y.max_neighbors ? nbr.seen : Y.max_neighbors;
    const OrcaWsStore planes{Y.ws + (size_t)g, Y.ws_ld};
    const OrcaWsStore proj{Y.ws + (size_t)g + (size_t)(Y.max_neighbors + Y.max_buildings) * 6 * Y.ws_ld, Y.ws_ld};
    orca_put_planes(planes, lx, T, e, S, nbr, kn, bs, kb, rec, nb, V, Y.tau, Y.time_step, Y.clear_xy,
                    [s_dest](int j) { return s_dest[j] ? 1.0 : 0.5; });  // a parked neighbour takes no share

    // ---- S1, S3, S4 ----
    const double yaw = P.yaw()[g], pitch = P.pitch()[g];
    const OrcaV3 pref = shield_pref(S.vx, S.vy, S.vz, yaw, pitch, a);
    const OrcaResult r = orca_solve(planes, proj, kb + kn, kb, Y.max_speed, pref);
    double o[3];
    const unsigned bits = shield_finish(S.vx, S.vy, S.vz, yaw, pitch, a, pref, r.v, o);
    intervened = (bits & kShieldIntervened) != 0u;
    fallback = r.status == 3;
    clipped = intervened && (bits & 7u) != 0u;
    double* w = Y.out_action + 3 * (size_t)g;
    w[0] = o[0]; w[1] = o[1]; w[2] = o[2];
    if (Y.pref_vel) { double* q = Y.pref_vel + 3 * (size_t)g; q[0] = pref.x; q[1] = pref.y; q[2] = pref.z; }
    if (Y.out_vel) { double* q = Y.out_vel + 3 * (size_t)g; q[0] = r.v.x; q[1] = r.v.y; q[2] = r.v.z; }
    if (Y.status) Y.status[g] = r.status;
    if (Y.flags) Y.flags[g] = (uint8_t)bits;
    if (Y.slack) Y.slack[g] = r.slack;
  } else if (row >= 0) {  // S5: the action passes (a ghost's row: zeros), every diagnostic 0
    const size_t q = (size_t)row;
    const bool ghost = !active;
    double* w = Y.out_action + 3 * q;
    w[0] = ghost ? 0.0 : a[0]; w[1] = ghost ? 0.0 : a[1]; w[2] = ghost ? 0.0 : a[2];
    if (Y.pref_vel) { double* o = Y.pref_vel + 3 * q; o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; }
    if (Y.out_vel) { double* o = Y.out_vel + 3 * q; o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; }
    if (Y.status) Y.status[q] = 0;
    if (Y.flags) Y.flags[q] = 0;
    if (Y.slack) Y.slack[q] = 0.0;
  }

  // ---- S6 ----
  if (Y.totals) {  // (uniform)
    const int n_judged = __syncthreads_count(judged), n_int = __syncthreads_count(intervened);
    const int n_fall = __syncthreads_count(fallback), n_clip = __syncthreads_count(clipped);
    if (d == 0) {
      long long* t = Y.totals + 4 * (size_t)e;
      t[kShieldJudged] += n_judged; t[kShieldTotIntervened] += n_int;
      t[kShieldTotFallback] += n_fall; t[kShieldTotClipped] += n_clip;
    }
  }
}
__global__ void __launch_bounds__(512) shield_kernel(const Params P, const ShieldArgs Y, const BuildingVelArgs V) {
  shield_body<false>(P, Y, V);
}
__global__ void __launch_bounds__(512) shield_counted_kernel(const Params P, const ShieldArgs Y, const BuildingVelArgs V) {
  shield_body<true>(P, Y, V);
}

}  // namespace rvo3d
