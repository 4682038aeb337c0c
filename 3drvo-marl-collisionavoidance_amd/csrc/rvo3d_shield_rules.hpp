// rvo3d_shield_rules.hpp -- the rules of rvo3d_shield_action (include/rvo3d.h) that are the shield's own, in plain C++:
// S1, the velocity the step would give a drone for an action (drone.kinematicstep in the step's arithmetic); S4, the
// identity where that velocity is safe and the command where it is not; S5, the rows that are not judged; and the
// argument checks.  S2 and S3 - the planes and the program - are rvo3d_orca_rules.hpp's.  __host__ __device__ and
// nothing of the device code is needed: tests/host/shield_check.hip calls every function on the CPU, tests/shield_ref.py
// restates them.
#pragma once

#include <cmath>

#include "rvo3d_orca_rules.hpp"

namespace rvo3d {

constexpr double kShieldDeg2Rad = 0.017453292519943295;  // the step's kDeg2Rad
// rvo3d_shield_args::flags: bits 0..2 are vel_command's clipped bits of the command
constexpr unsigned kShieldIntervened = 8u;
// rvo3d_shield_args::totals, per env
constexpr int kShieldJudged = 0, kShieldTotIntervened = 1, kShieldTotFallback = 2, kShieldTotClipped = 3;

// ---- S1: the step's own pieces (rvo3d_math.hpp: norm3b, clampd, np_mod), restated for host and device ----
__host__ __device__ inline double shield_norm3(double x, double y, double z) {
  return __builtin_sqrt(__builtin_fma(z, z, __builtin_fma(y, y, x * x)));  // the OpenBLAS ddot chain of the step
}
__host__ __device__ inline double shield_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
__host__ __device__ inline double shield_mod(double a, double b) {  // npy_divmod's remainder
  double m;
  if (b > 0.0 && a > -b && a < 2.0 * b) m = a >= b ? a - b : a;  // (exact: the step's shortcut)
  else m = fmod(a, b);
  if (m != 0.0) {
    if ((b < 0.0) != (m < 0.0)) m += b;
  } else {
    m = __builtin_copysign(0.0, b);
  }
  return m;
}
// The velocity behind the step of a drone with velocity v and heading (yaw, pitch), degrees, for the action a - of a
// drone the step does not park.  The products are (speed * cos pitch') * cos yaw', as the step writes them.
__host__ __device__ inline OrcaV3 shield_pref(double vx, double vy, double vz, double yaw, double pitch, const double* a) {
  double speed = shield_norm3(vx, vy, vz);
  const double acc = shield_clamp(a[0] * 1.0, -1.0, 1.0);
  const double dyaw = shield_clamp(a[1] * 90.0, -90.0, 90.0);
  const double dpit = shield_clamp(a[2] * 90.0, -90.0, 90.0);
  const double nv = speed + acc;
  speed = (0.0 > nv) ? 0.0 : nv;
  yaw = shield_mod(yaw + dyaw, 360.0);
  pitch = shield_clamp(pitch + dpit, -90.0, 90.0);
  double sy, cy, sp, cp;
  sincos(yaw * kShieldDeg2Rad, &sy, &cy);
  sincos(pitch * kShieldDeg2Rad, &sp, &cp);
  return OrcaV3{speed * cp * cy, speed * cp * sy, speed * sp};
}

// ---- S5: is the row judged?  live: not a ghost row; dest: the drone's dest flag ----
__host__ __device__ inline bool shield_judged(bool live, bool dest, const double* a) {
  return live && !dest && orca_finite(a[0]) && orca_finite(a[1]) && orca_finite(a[2]);
}

// ---- S4: the action that leaves.  Not intervened (v == pref in every component): the action's own three doubles and
// flags 0; intervened: the command for v and kShieldIntervened | the command's clipped bits.
__host__ __device__ inline unsigned shield_finish(double vx, double vy, double vz, double yaw, double pitch, const double* a,
                                                  const OrcaV3& pref, const OrcaV3& v, double* out) {
  if (v.x != pref.x || v.y != pref.y || v.z != pref.z) return kShieldIntervened | vel_command(vx, vy, vz, yaw, pitch, v.x, v.y, v.z, out);
  out[0] = a[0]; out[1] = a[1]; out[2] = a[2];
  return 0u;
}

// ---- the argument checks of rvo3d_shield_action, before the first HIP call: orca_check's, on the shield's arguments ----
inline int shield_check(const rvo3d_shield_args* a, bool sets_attached, const rvo3d_building_motion* m, double dt,
                        const char** why) {
  *why = "";
  if (!a) { *why = "null rvo3d_shield_args"; return RVO3D_ERR_INVALID; }
  if (!a->action || !a->out_action) { *why = "action / out_action are required"; return RVO3D_ERR_INVALID; }
  rvo3d_orca_args o{};
  o.time_horizon = a->time_horizon; o.time_step = a->time_step; o.max_speed = a->max_speed; o.pref_speed = 0.0;
  o.neighbor_dist = a->neighbor_dist; o.max_neighbors = a->max_neighbors; o.max_buildings = a->max_buildings;
  o.reach = a->reach; o.below = a->below; o.clear_xy = a->clear_xy; o.out_vel = a->out_action;
  return orca_check(&o, sets_attached, m, dt, why);
}

}  // namespace rvo3d
