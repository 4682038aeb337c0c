// rvo3d_motion_kernels.hpp -- moving buildings (include/rvo3d.h: rvo3d_move_env_buildings): the records of the per-env
// building sets patrol between two endpoints, and the per-cell lists the step reads are rebuilt where they are - one
// launch, one workgroup per env, nothing allocated, nothing synchronised, no atomics.  The step, the safety scan and the
// building rows read the records and the lists from device memory on every call (Cold::bld / Cold::bgrid with a stride
// per env), so they see the moved cylinders without a change.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
// The move rule and the cell rule are plain C++ (__host__ __device__): tests/host/building_motion_check.hip runs the very
// same text on the CPU, the cell rule against build_building_grid (rvo3d_host_setup.hpp).
#pragma once

#include "../../include/rvo3d.h"
#include "rvo3d_params.hpp"

namespace rvo3d {

// ---- the move rule: every operation a float64 one, rounded on its own ----
// the filler stage_env_buildings writes behind counts[e]: never moved, never listed, nothing but its h is read
__host__ __device__ inline bool motion_live(double h) { return !(h == -__builtin_inf()); }

struct MotionStep {
  double x, y;
  uint8_t leg;
  bool moved;  // false: a static building (speed 0 or NaN, dt 0) - the record and leg keep their bits, ends is not read
};
// ends: the record's [2][2] endpoints (0 and 1, x then y); obs_circle's model (cal_des_vel_omni + move_forward) with
// cos = dx / d, sin = dy / d, and a patrol where the reference's obstacle stops
__host__ __device__ inline MotionStep motion_move(double x, double y, uint8_t leg, const double* ends, double speed,
                                                  double dt) {
  MotionStep m{x, y, leg, false};
  const double step = speed * dt;
  if (!(step > 0.0)) return m;
  m.moved = true;
  const int k = leg & 1;
  const double tx = ends[2 * k], ty = ends[2 * k + 1];
  const double dx = tx - x, dy = ty - y;
  const double d = __builtin_sqrt(dx * dx + dy * dy);
  if (d <= step) {  // arrived: exactly the endpoint, the rest of the step is not spent
    m.x = tx; m.y = ty;
    m.leg = (uint8_t)(leg ^ 1);
  } else {
    m.x = x + (dx / d) * step;
    m.y = y + (dy / d) * step;
  }
  return m;
}
// The velocity the record's next motion_move will have shown, where the record stands now (include/rvo3d.h:
// rvo3d_building_rows_moving, rule 2): the same step, d and branch; on arrival the move lands on T exactly, so the
// velocity is the rest of the way over dt.  A static building: (0, 0), ends is not read.
struct MotionVel { double x, y; };
__host__ __device__ inline MotionVel motion_velocity(double x, double y, uint8_t leg, const double* ends, double speed,
                                                     double dt) {
  MotionVel v{0.0, 0.0};
  const double step = speed * dt;
  if (!(step > 0.0)) return v;
  const int k = leg & 1;
  const double dx = ends[2 * k] - x, dy = ends[2 * k + 1] - y;
  const double d = __builtin_sqrt(dx * dx + dy * dy);
  if (d <= step) {
    v.x = dx / dt; v.y = dy / dt;
  } else {
    v.x = (dx / d) * speed; v.y = (dy / d) * speed;
  }
  return v;
}

// ---- the cell rule: what build_building_grid computes for one cell, u16 for u16 ----
// a building's reach in the lists: min(largest drone radius + r_b, the 5 m gate) + 1e-3 (never NaN)
__host__ __device__ inline double motion_reach(double rmax, double br) {
  double reach = rmax + br;
  if (!(reach < 5.0)) reach = 5.0;  // the gate (also a NaN radius)
  return reach + 1e-3;
}

// One cell as it lies in memory: kBgridK + 1 u16 = eight little-endian words, word 0's low half the count.  Touched
// through compile-time indices only, so that it stays in registers.
static_assert(kBgridK + 1 == 16, "a cell is 32 bytes: two 16-byte stores");
struct MotionCell { uint32_t w[8]; };
__host__ __device__ inline void motion_cell_put(MotionCell& c, int pos, uint32_t v) {
  const uint32_t sh = v << ((pos & 1) * 16);
#pragma unroll
  for (int j = 0; j < 8; ++j) c.w[j] |= (pos >> 1) == j ? sh : 0u;
}
// rec(b, x, y, reach) -> false for a filler, else the record's centre and motion_reach.  Cell (ix, iy) =
// [ix*cs, (ix+1)*cs] x [iy*cs, (iy+1)*cs], unbounded at the map's edge; the live records in index order; count 0xffff
// once more than kBgridK are listed (the first kBgridK stay listed, as on the host).
template <class Rec>
__host__ __device__ inline MotionCell motion_cell(int ix, int iy, int bgx, int bgy, double bg_inv, int nb, Rec rec) {
  MotionCell c{};
  const double inf = __builtin_inf();
  const double cs = 1.0 / bg_inv;
  const double x0 = ix == 0 ? -inf : ix * cs, x1 = ix == bgx - 1 ? inf : (ix + 1) * cs;
  const double y0 = iy == 0 ? -inf : iy * cs, y1 = iy == bgy - 1 ? inf : (iy + 1) * cs;
  int n = 0;
  bool overflow = false;
  for (int b = 0; b < nb && !overflow; ++b) {
    double bx, by, reach;
    if (!rec(b, bx, by, reach)) continue;
    const double dx = bx < x0 ? x0 - bx : (bx > x1 ? bx - x1 : 0.0);
    const double dy = by < y0 ? y0 - by : (by > y1 ? by - y1 : 0.0);
    if (!(dx * dx + dy * dy > reach * reach)) {  // also keeps NaN centres
      if (n == kBgridK) overflow = true;
      else motion_cell_put(c, 1 + n++, (uint32_t)b);
    }
  }
  c.w[0] |= overflow ? 0xffffu : (uint32_t)n;
  return c;
}

// ---- the kernel ----
struct MotionArgs {
  double* bld;          // the handle's records [E][nb][4] and cells [E][bgx * bgy][kBgridK + 1]
  uint16_t* bgrid;
  uint32_t bld_stride, bgrid_stride;
  int32_t nb, bgx, bgy;
  double bg_inv, rmax, dt;
  const double* ends;   // the caller's: [E][nb][2][2], [E][nb], [E][nb]
  const double* speed;
  uint8_t* leg;
  const uint8_t* mask;  // [E], nullable
  double* out;          // [E][nb][4], nullable
};

constexpr int kMotionThreads = 256;
// The records whose (x, y, reach) phase 2 finds in LDS: 3 x 8 B x 512 = 12 KiB per workgroup (eight four-wave workgroups
// fill a CU's wave slots before LDS does).  Records from this index on are read back from the handle's records, which the
// workgroup has written before the barrier.
constexpr int kMotionLdsRecords = 512;

__global__ void __launch_bounds__(kMotionThreads) move_buildings_kernel(const MotionArgs A) {
  __shared__ double s_x[kMotionLdsRecords], s_y[kMotionLdsRecords], s_reach[kMotionLdsRecords];
  const int e = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (A.mask && !A.mask[e]) return;  // (the whole workgroup: nothing of the env is read or written)
  const int nb = A.nb;
  double* const rec = A.bld + (size_t)e * A.bld_stride;
  const size_t row = (size_t)e * (size_t)nb;
  const double nan = __builtin_nan("");

  // phase 1: move
  for (int b = tid; b < nb; b += kMotionThreads) {
    double* const q = rec + (size_t)b * 4;
    double x = 0.0, y = 0.0, reach = nan;  // reach NaN: a filler
    // one round trip for h, the speed and leg (the caller's arrays have an entry for a filler too), a second one for
    // the rest of a live record and its endpoint
    const double bh = q[2];
    const double speed = A.speed[row + b];
    const uint8_t leg = A.leg[row + b];
    if (motion_live(bh)) {
      const double2 xy = *reinterpret_cast<const double2*>(q);
      const double br = q[3];
      const MotionStep m = motion_move(xy.x, xy.y, leg, A.ends + (row + b) * 4, speed, A.dt);
      if (m.moved) {
        *reinterpret_cast<double2*>(q) = make_double2(m.x, m.y);
        if (m.leg != leg) A.leg[row + b] = m.leg;
      }
      x = m.x; y = m.y;
      if (A.out) {
        double* const o = A.out + (row + b) * 4;
        o[0] = x; o[1] = y; o[2] = bh; o[3] = br;
      }
      reach = motion_reach(A.rmax, br);
    }
    if (b < kMotionLdsRecords) { s_x[b] = x; s_y[b] = y; s_reach[b] = reach; }
  }
  if (A.bgx == 0) return;
  __syncthreads();

  // phase 2: lists
  const int cells = A.bgx * A.bgy;
  uint16_t* const grid = A.bgrid + (size_t)e * A.bgrid_stride;
  const double rmax = A.rmax;
  for (int c = tid; c < cells; c += kMotionThreads) {
    const int ix = c / A.bgy, iy = c - ix * A.bgy;
    const MotionCell m = motion_cell(ix, iy, A.bgx, A.bgy, A.bg_inv, nb, [&](int b, double& bx, double& by, double& reach) {
      if (b < kMotionLdsRecords) {
        reach = s_reach[b];
        if (reach != reach) return false;
        bx = s_x[b]; by = s_y[b];
        return true;
      }
      const double* const q = rec + (size_t)b * 4;
      if (!motion_live(q[2])) return false;
      bx = q[0]; by = q[1];
      reach = motion_reach(rmax, q[3]);
      return true;
    });
    uint4* const dst = reinterpret_cast<uint4*>(grid + (size_t)c * (kBgridK + 1));
    dst[0] = make_uint4(m.w[0], m.w[1], m.w[2], m.w[3]);
    dst[1] = make_uint4(m.w[4], m.w[5], m.w[6], m.w[7]);
  }
}

}  // namespace rvo3d
