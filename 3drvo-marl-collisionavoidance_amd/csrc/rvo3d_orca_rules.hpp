// rvo3d_orca_rules.hpp -- the rules of rvo3d_orca_vel and rvo3d_vel_command (include/rvo3d.h) in plain C++: the ORCA
// plane of a pair, the four incremental linear programs of van den Berg, Guy, Lin, Manocha ("Reciprocal n-body collision
// avoidance") in three dimensions, the sorted selection slots, the converter from a wanted velocity to the step's action
// and the argument checks.  __host__ __device__ throughout and nothing of the device code is needed:
// tests/host/orca_check.hip calls every function on the CPU, tests/orca_ref.py restates them operation for operation.
// Every value is a float64 and every operation is rounded on its own (the library is built with -ffp-contract=off); a
// sum of three products is (a*b + c*d) + e*f.
#pragma once

#include <cmath>

#include "../../include/rvo3d.h"

namespace rvo3d {

constexpr int kOrcaMaxNeighbors = 16;  // rvo3d_orca_args::max_neighbors at most
constexpr int kOrcaMaxBuildings = 8;   // rvo3d_orca_args::max_buildings at most
constexpr int kOrcaMaxPlanes = kOrcaMaxNeighbors + kOrcaMaxBuildings;
constexpr int kOrcaStoreSlots = 2 * kOrcaMaxPlanes - 1;  // the planes, then the fallback's projected planes
constexpr double kOrcaEps = 1e-5;      // the authors' RVO_EPSILON

struct OrcaV3 { double x, y, z; };
__host__ __device__ inline OrcaV3 orca_v3(double x, double y, double z) { return OrcaV3{x, y, z}; }
__host__ __device__ inline OrcaV3 orca_add(const OrcaV3& a, const OrcaV3& b) { return OrcaV3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__host__ __device__ inline OrcaV3 orca_sub(const OrcaV3& a, const OrcaV3& b) { return OrcaV3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ inline OrcaV3 orca_mul(double s, const OrcaV3& a) { return OrcaV3{s * a.x, s * a.y, s * a.z}; }
__host__ __device__ inline OrcaV3 orca_div(const OrcaV3& a, double s) { return OrcaV3{a.x / s, a.y / s, a.z / s}; }
__host__ __device__ inline double orca_dot(const OrcaV3& a, const OrcaV3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ inline OrcaV3 orca_cross(const OrcaV3& a, const OrcaV3& b) {
  return OrcaV3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// a / |a|, and (1, 0, 0) for a zero-length a (a guard of the rules: rule 4)
__host__ __device__ inline OrcaV3 orca_unit(const OrcaV3& a, double len) {
  if (!(len > 0.0)) return OrcaV3{1.0, 0.0, 0.0};
  return orca_div(a, len);
}
__host__ __device__ inline bool orca_finite(double x) { return x - x == 0.0; }

struct OrcaPlane { OrcaV3 point, normal; };  // the half-space normal . (v - point) >= 0

// ---- rule 4: the plane drone i takes for agent j.  rel = p_j - p_i, w_rel = v_i - v_j, R the combined radius, share 0.5
// (a drone) or 1 (a building).  *branch: 0 cut-off circle, 1 leg, 2 already overlapping (diagnostics of the tests).
// Guards beyond the published construction: the root's argument is max(b*b - a*c, 0) (also for a NaN); a zero-length w
// takes the normal (1, 0, 0); a zero-length ww - w_rel on the cone's axis - takes a normal of the cone (below).
__host__ __device__ inline OrcaPlane orca_plane(const OrcaV3& rel, const OrcaV3& w_rel, double R, double tau,
                                                double time_step, double share, const OrcaV3& v_i, int* branch) {
  const double d2 = orca_dot(rel, rel), R2 = R * R;
  OrcaV3 n, u;
  if (d2 > R2) {
    const OrcaV3 w = orca_sub(w_rel, orca_div(rel, tau));
    const double wl2 = orca_dot(w, w), dp = orca_dot(w, rel);
    if (dp < 0.0 && dp * dp > R2 * wl2) {
      const double wl = __builtin_sqrt(wl2);
      n = orca_unit(w, wl);
      u = orca_mul(R / tau - wl, n);
      *branch = 0;
    } else {
      const double a = d2, b = orca_dot(rel, w_rel);
      const OrcaV3 cr = orca_cross(rel, w_rel);
      const double c = orca_dot(w_rel, w_rel) - orca_dot(cr, cr) / (d2 - R2);
      double disc = b * b - a * c;
      if (!(disc > 0.0)) disc = 0.0;
      const double t = (b + __builtin_sqrt(disc)) / a;
      const OrcaV3 ww = orca_sub(w_rel, orca_mul(t, rel));
      const double wwl = __builtin_sqrt(orca_dot(ww, ww));
      if (wwl > 0.0) n = orca_div(ww, wwl);
      else {
        // w_rel on the cone's axis (an exact head-on): every normal of the cone round the axis is as near.  The one
        // towards e x rel is taken, e = z (x for a vertical rel): the other drone, with -rel, takes the opposite one, as
        // reciprocity needs, and a planar pair stays planar.  The limit of ww / |ww|: cos(alpha) perp - sin(alpha) axis.
        const OrcaV3 e = (rel.x == 0.0 && rel.y == 0.0) ? OrcaV3{1.0, 0.0, 0.0} : OrcaV3{0.0, 0.0, 1.0};
        const OrcaV3 perp = orca_cross(e, rel);
        const double pl = __builtin_sqrt(orca_dot(perp, perp)), d = __builtin_sqrt(d2);
        n = orca_sub(orca_mul(__builtin_sqrt(d2 - R2) / d, orca_div(perp, pl)), orca_mul(R / d, orca_div(rel, d)));
      }
      u = orca_mul(R * t - wwl, n);
      *branch = 1;
    }
  } else {
    const OrcaV3 w = orca_sub(w_rel, orca_div(rel, time_step));
    const double wl = __builtin_sqrt(orca_dot(w, w));
    n = orca_unit(w, wl);
    u = orca_mul(R / time_step - wl, n);
    *branch = 2;
  }
  return OrcaPlane{orca_add(v_i, orca_mul(share, u)), n};
}

// ---- rules 2 and 3: K slots sorted by (key, index), touched through compile-time indices only so that they stay in
// registers (building_slots_insert's scheme).  Candidates arrive in index order and move in front of a slot only when
// strictly smaller: equal keys keep the lower index first.  The first k slots of the best K are the best k.
template <int K>
struct OrcaSlots {
  double key[K];
  int32_t idx[K];  // -1: empty (key +inf)
  int32_t seen;
};
template <int K>
__host__ __device__ inline void orca_slots_clear(OrcaSlots<K>& s) {
#pragma unroll
  for (int i = 0; i < K; ++i) { s.key[i] = __builtin_inf(); s.idx[i] = -1; }
  s.seen = 0;
}
template <int K>
__host__ __device__ inline void orca_slots_insert(OrcaSlots<K>& s, double key, int32_t index) {
  ++s.seen;
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    const bool here = key < s.key[i];
    const bool before = i > 0 && key < s.key[i > 0 ? i - 1 : 0];  // (slot i - 1 is still what it was)
    s.idx[i] = before ? s.idx[i > 0 ? i - 1 : 0] : (here ? index : s.idx[i]);
    s.key[i] = before ? s.key[i > 0 ? i - 1 : 0] : (here ? key : s.key[i]);
  }
}
template <int K>
__host__ __device__ inline int32_t orca_slots_index(const OrcaSlots<K>& s, int i) {  // slot i by a select chain
  int32_t idx = -1;
#pragma unroll
  for (int j = 0; j < K; ++j) idx = j == i ? s.idx[j] : idx;
  return idx;
}

// ---- rule 6: the programs.  A Store holds planes by slot: get(slot) -> OrcaPlane, put(slot, plane).  The kernel's lives
// in the handle's workspace, the host program's is an array.
// On the line point + t * dir inside the sphere of `radius`, under planes [0, count).
template <class Store>
__host__ __device__ inline bool orca_lp1(const Store& planes, int count, const OrcaV3& dir, const OrcaV3& point, double radius,
                                         const OrcaV3& opt, bool direction_opt, OrcaV3& result) {
  const double dp = orca_dot(point, dir);
  const double disc = (dp * dp + radius * radius) - orca_dot(point, point);
  if (!(disc >= 0.0)) return false;
  const double sd = __builtin_sqrt(disc);
  double t_left = -dp - sd, t_right = -dp + sd;
  for (int i = 0; i < count; ++i) {
    const OrcaPlane p = planes.get(i);
    const double num = orca_dot(orca_sub(p.point, point), p.normal);
    const double den = orca_dot(dir, p.normal);
    if (den * den <= kOrcaEps) {  // the line is (almost) parallel to plane i
      if (num > 0.0) return false;
      continue;
    }
    const double t = num / den;
    if (den >= 0.0) t_left = t > t_left ? t : t_left;
    else t_right = t < t_right ? t : t_right;
    if (t_left > t_right) return false;
  }
  double t;
  if (direction_opt) t = orca_dot(opt, dir) > 0.0 ? t_right : t_left;
  else {
    t = orca_dot(dir, orca_sub(opt, point));
    t = t < t_left ? t_left : (t > t_right ? t_right : t);
  }
  result = orca_add(point, orca_mul(t, dir));
  return true;
}

// On plane `no` inside the sphere, under planes [0, no).  Guard beyond the published program: a projected point that
// coincides with the circle's centre stays there (the published quotient would be x / 0).
template <class Store>
__host__ __device__ inline bool orca_lp2(const Store& planes, int no, double radius, const OrcaV3& opt, bool direction_opt,
                                         OrcaV3& result) {
  const OrcaPlane q = planes.get(no);
  const double dist = orca_dot(q.point, q.normal);
  const double dist2 = dist * dist, r2 = radius * radius;
  if (dist2 > r2) return false;
  const double pr2 = r2 - dist2;
  const OrcaV3 centre = orca_mul(dist, q.normal);
  if (direction_opt) {
    const OrcaV3 po = orca_sub(opt, orca_mul(orca_dot(opt, q.normal), q.normal));
    const double l2 = orca_dot(po, po);
    if (l2 <= kOrcaEps) result = centre;
    else result = orca_add(centre, orca_mul(__builtin_sqrt(pr2 / l2), po));
  } else {
    result = orca_add(opt, orca_mul(orca_dot(orca_sub(q.point, opt), q.normal), q.normal));
    if (orca_dot(result, result) > r2) {
      const OrcaV3 pres = orca_sub(result, centre);
      const double l2 = orca_dot(pres, pres);
      if (!(l2 > 0.0)) result = centre;
      else result = orca_add(centre, orca_mul(__builtin_sqrt(pr2 / l2), pres));
    }
  }
  for (int i = 0; i < no; ++i) {
    const OrcaPlane p = planes.get(i);
    if (orca_dot(p.normal, orca_sub(p.point, result)) > 0.0) {
      const OrcaV3 cr = orca_cross(p.normal, q.normal);
      const double cl2 = orca_dot(cr, cr);
      if (cl2 <= kOrcaEps) return false;  // (almost) parallel: plane i invalidates plane `no`
      const OrcaV3 dir = orca_div(cr, __builtin_sqrt(cl2));
      const OrcaV3 ln = orca_cross(dir, q.normal);
      const double s = orca_dot(orca_sub(p.point, q.point), p.normal) / orca_dot(ln, p.normal);
      const OrcaV3 lp = orca_add(q.point, orca_mul(s, ln));
      if (!orca_lp1(planes, i, dir, lp, radius, opt, direction_opt, result)) return false;
    }
  }
  return true;
}

// In space under planes [0, count): the point of the sphere nearest opt (direction_opt: furthest along the unit opt).
// Returns count, or the plane it failed at with result as it was before that plane.  *moved: some plane was violated by
// the running result (false: the result is the start - opt clipped to the sphere).
template <class Store>
__host__ __device__ inline int orca_lp3(const Store& planes, int count, double radius, const OrcaV3& opt, bool direction_opt,
                                        OrcaV3& result, bool* moved) {
  *moved = false;
  if (direction_opt) result = orca_mul(radius, opt);
  else {
    const double l2 = orca_dot(opt, opt);
    if (l2 > radius * radius) result = orca_mul(radius, orca_div(opt, __builtin_sqrt(l2)));
    else result = opt;
  }
  for (int i = 0; i < count; ++i) {
    const OrcaPlane p = planes.get(i);
    if (orca_dot(p.normal, orca_sub(p.point, result)) > 0.0) {
      *moved = true;
      const OrcaV3 keep = result;
      if (!orca_lp2(planes, i, radius, opt, direction_opt, result)) {
        result = keep;
        return i;
      }
    }
  }
  return count;
}

// The fallback from plane `begin` on: minimise the largest penetration.  Planes [0, hard) are the buildings': as the
// authors' 2-D library treats obstacle lines, they enter every projected problem unchanged; only planes from `hard` on
// are projected (relaxed).  A building plane the program itself failed at (begin < hard) is visited like any other: the
// building planes before it stay hard.  proj: count - 1 slots.
template <class Store, class Proj>
__host__ __device__ inline void orca_lp4(const Store& planes, Proj& proj, int count, int hard, int begin, double radius,
                                         OrcaV3& result) {
  double distance = 0.0;
  for (int i = begin; i < count; ++i) {
    const OrcaPlane pi = planes.get(i);
    if (!(orca_dot(pi.normal, orca_sub(pi.point, result)) > distance)) continue;
    int m = 0;
    for (int j = 0; j < i; ++j) {
      const OrcaPlane pj = planes.get(j);
      if (j < hard) { proj.put(m++, pj); continue; }
      OrcaPlane o;
      const OrcaV3 cr = orca_cross(pj.normal, pi.normal);
      if (orca_dot(cr, cr) <= kOrcaEps) {  // (almost) parallel
        if (orca_dot(pi.normal, pj.normal) > 0.0) continue;  // the same direction
        o.point = orca_mul(0.5, orca_add(pi.point, pj.point));
      } else {
        const OrcaV3 ln = orca_cross(cr, pi.normal);
        const double s = orca_dot(orca_sub(pj.point, pi.point), pj.normal) / orca_dot(ln, pj.normal);
        o.point = orca_add(pi.point, orca_mul(s, ln));
      }
      const OrcaV3 dn = orca_sub(pj.normal, pi.normal);
      o.normal = orca_unit(dn, __builtin_sqrt(orca_dot(dn, dn)));
      proj.put(m++, o);
    }
    const OrcaV3 keep = result;
    bool moved;
    if (orca_lp3(proj, m, radius, pi.normal, true, result, &moved) < m) result = keep;  // (rounding only: keep)
    distance = orca_dot(pi.normal, orca_sub(pi.point, result));
  }
}

// Rule 6 as a whole.  Planes [0, hard) the buildings', [hard, count) the drones'.  status 1: pref (clipped to the sphere)
// is feasible, 2: solved by the program, 3: no common point, the fallback ran.  *slack: the largest penetration of a
// drone plane at the result, 0 for status 1 and 2.
struct OrcaResult { OrcaV3 v; int status; double slack; };
template <class Store, class Proj>
__host__ __device__ inline OrcaResult orca_solve(const Store& planes, Proj& proj, int count, int hard, double max_speed,
                                                 const OrcaV3& pref) {
  OrcaResult r;
  bool moved;
  const int fail = orca_lp3(planes, count, max_speed, pref, false, r.v, &moved);
  r.slack = 0.0;
  if (fail == count) { r.status = moved ? 2 : 1; return r; }
  orca_lp4(planes, proj, count, hard, fail, max_speed, r.v);
  r.status = 3;
  for (int i = hard; i < count; ++i) {
    const OrcaPlane p = planes.get(i);
    const double pen = orca_dot(p.normal, orca_sub(p.point, r.v));
    r.slack = pen > r.slack ? pen : r.slack;
  }
  return r;
}

// ---- rvo3d_vel_command: the action whose kinematic step (drone.kinematicstep, rvo3d_step_body.hpp) turns the velocity v
// at heading (yaw, pitch), degrees, into w.  a[3]: clipped to [-1, 1]; returns the bits of the components that needed it.
constexpr double kOrcaRad2Deg = 57.29577951308232;  // 180 / pi
__host__ __device__ inline unsigned vel_command(double vx, double vy, double vz, double yaw, double pitch, double wx,
                                                double wy, double wz, double* a) {
  const double wn = __builtin_sqrt((wx * wx + wy * wy) + wz * wz);
  const double vn = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
  double r[3] = {wn - vn, 0.0, 0.0};
  if (wn > 0.0) {  // (|w| = 0 keeps both angles)
    const double turn = atan2(wy, wx) * kOrcaRad2Deg - yaw;
    r[1] = (turn - 360.0 * __builtin_floor((turn + 180.0) / 360.0)) / 90.0;  // wrapped into [-180, 180)
    double s = wz / wn;
    s = s < -1.0 ? -1.0 : (s > 1.0 ? 1.0 : s);
    r[2] = (asin(s) * kOrcaRad2Deg - pitch) / 90.0;
  }
  unsigned bits = 0u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (r[k] > 1.0) { r[k] = 1.0; bits |= 1u << k; }
    else if (r[k] < -1.0) { r[k] = -1.0; bits |= 1u << k; }
    a[k] = r[k];
  }
  return bits;
}

// ---- the argument checks of rvo3d_orca_vel, before the first HIP call.  RVO3D_OK, RVO3D_ERR_INVALID or RVO3D_ERR_STATE
// with the reason in *why.  sets_attached: rvo3d_set_env_buildings is in force on the handle.
inline int orca_check(const rvo3d_orca_args* a, bool sets_attached, const rvo3d_building_motion* m, double dt,
                      const char** why) {
  *why = "";
  const auto bad = [&](const char* w) { *why = w; return RVO3D_ERR_INVALID; };
  if (!a) return bad("null rvo3d_orca_args");
  if (!a->out_vel) return bad("out_vel is required");
  if (!orca_finite(a->time_horizon) || !(a->time_horizon > 0.0)) return bad("time_horizon must be finite and > 0");
  if (!orca_finite(a->time_step) || !(a->time_step > 0.0)) return bad("time_step must be finite and > 0");
  if (!orca_finite(a->max_speed) || !(a->max_speed >= 0.0)) return bad("max_speed must be finite and >= 0");
  if (!orca_finite(a->pref_speed) || !(a->pref_speed >= 0.0)) return bad("pref_speed must be finite and >= 0");
  if (!orca_finite(a->neighbor_dist) || !(a->neighbor_dist > 0.0)) return bad("neighbor_dist must be finite and > 0");
  if (a->max_neighbors < 1 || a->max_neighbors > kOrcaMaxNeighbors) return bad("max_neighbors must be 1..16");
  if (a->max_buildings < 0 || a->max_buildings > kOrcaMaxBuildings) return bad("max_buildings must be 0..8");
  if (!orca_finite(a->reach) || !(a->reach > 0.0)) return bad("reach must be finite and > 0");
  if (!orca_finite(a->below) || !(a->below >= 0.0)) return bad("below must be finite and >= 0");
  if (!orca_finite(a->clear_xy) || !(a->clear_xy >= 0.0)) return bad("clear_xy must be finite and >= 0");
  if (m && !sets_attached) { *why = "a motion needs attached per-env building sets (rvo3d_set_env_buildings)"; return RVO3D_ERR_STATE; }
  if (m && (!m->ends || !m->speed || !m->leg)) return bad("ends, speed and leg are required");
  if (!orca_finite(dt) || !(dt >= 0.0)) return bad("dt must be finite and >= 0");
  return RVO3D_OK;
}

}  // namespace rvo3d
