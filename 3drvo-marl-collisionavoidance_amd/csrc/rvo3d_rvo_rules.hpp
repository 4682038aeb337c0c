// rvo3d_rvo_rules.hpp -- what the classical RVO velocity (rvo3d_aux_kernels.hpp: rvo_vel_body) and its building-aware
// form (rvo3d_rvo_city_kernels.hpp: rvo_city_body) decide in plain C++: the acceler check and the selection among the
// candidates.  Needs nothing of the device code: tests/host/rvo_city_check.hip calls rvo_select on the CPU
// (as city_select, rvo3d_rvo_city_kernels.hpp).
#pragma once

namespace rvo3d {

// acceler <= 1 keeps the candidates at 4 per axis, 64 in all: one bit each.  The refusal's text, for every entry point.
inline bool rvo_acceler_ok(double acceler) { return acceler >= 0.0 && acceler <= 1.0; }
inline constexpr const char* kRvoAccelerWhy = "acceler must be in [0, 1] (at most 4 candidates per axis)";

// vel_select (reciprocal_vel_obs.py:119-124) over the candidates c = (ix * cnt[1] + iy) * cnt[2] + iz with the values
// val(axis, i), those of live & ~blocked.  1: outside every cone, closest to des; 2: none such - the least
// 1 * tc_inv + dd; Python's min keeps the first minimum.  0: every live candidate is blocked or none is live, o is not
// written.  rvo_vel_body has nothing blocked and answers 0 with zeros; rvo_city_body goes on to its tiers 3 and 4.
template <class Val>
__host__ __device__ inline int rvo_select(const int* cnt, Val val, const double* des, double tc_min,
                                          unsigned long long live, unsigned long long cone, unsigned long long blocked,
                                          double* o) {
  const unsigned long long free_ = live & ~blocked;
  const double tc_inv = (tc_min == 0) ? __builtin_inf() : 1.0 / tc_min;
  bool have_out = false, have_in = false;
  double best_out = 0, best_in = 0, so[3] = {0, 0, 0}, si[3] = {0, 0, 0};
  int c = 0;
  for (int ix = 0; ix < cnt[0]; ++ix)
    for (int iy = 0; iy < cnt[1]; ++iy)
      for (int iz = 0; iz < cnt[2]; ++iz, ++c) {
        if (!((free_ >> c) & 1ull)) continue;
        const double vx = val(0, ix), vy = val(1, iy), vz = val(2, iz);
        const double ax = des[0] - vx, ay = des[1] - vy, az = des[2] - vz;
        const double dd = __builtin_sqrt(ax * ax + ay * ay + az * az);
        if (!((cone >> c) & 1ull)) {
          if (!have_out || dd < best_out) { best_out = dd; so[0] = vx; so[1] = vy; so[2] = vz; have_out = true; }
        } else {
          const double pen = 1 * tc_inv + dd;
          if (!have_in || pen < best_in) { best_in = pen; si[0] = vx; si[1] = vy; si[2] = vz; have_in = true; }
        }
      }
  if (have_out) { o[0] = so[0]; o[1] = so[1]; o[2] = so[2]; return 1; }
  if (have_in) { o[0] = si[0]; o[1] = si[1]; o[2] = si[2]; return 2; }
  return 0;
}

}  // namespace rvo3d
