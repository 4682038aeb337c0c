// rvo3d_building_kernels.hpp -- nearest-building rows of the handle's current state (include/rvo3d.h:
// rvo3d_building_rows): per drone the k buildings with the smallest gap among those that pass the reference's gate
// (rvo_inter.preprocess, rvo_inter.py:99-105), as rows of six floats, alone or spliced into the dense observation row;
// and rvo3d_building_rows_moving: rows of eight floats, the urgency taken at the velocity relative to the building's and
// the building's velocity behind it.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
// The per-building arithmetic, the k-slot insertion and the argument checks are plain C++ (__host__ __device__ / host):
// tests/host/building_rows_check.hip and tests/host/building_rows_moving_check.hip call them on the CPU.
#pragma once

#include "../../include/rvo3d.h"
#include "rvo3d_params.hpp"
#include "rvo3d_safety_kernels.hpp"
#include "rvo3d_motion_kernels.hpp"

namespace rvo3d {

constexpr int kBldSlots = 8;      // rows per drone at most (rvo3d_building_rows_args::k)
constexpr int kBldRowFloats = 6;  // floats per building row
constexpr int kBldRowFloatsMoving = 8;  // ... of rvo3d_building_rows_moving: urg at the relative velocity, then vb_x, vb_y

// ---- one (drone, building) pair: every operation a float64 one, rounded on its own ----
// np.round(v, 2) of the observation, with + 0.0 behind it: no output is -0.0
__host__ __device__ inline double building_r2(double v) { return __builtin_rint(v * 100.0) / 100.0 + 0.0; }
// float32 of building_r2(v) without the division: float(k * 0.01) == float(k / 100.0) for every integer |k| < 2^24
// (round2_f32 of rvo3d_math.hpp, tests/test_numeric_shortcuts.py); larger magnitudes take the division
__host__ __device__ inline float building_r2f(double v) {
  const double k = __builtin_rint(v * 100.0);
  return __builtin_fabs(k) < 16777216.0 ? (float)(k * 0.01 + 0.0) : (float)(k / 100.0 + 0.0);
}

struct BuildingPair {
  bool pass;       // the gate: h_b > p_z - below and d <= reach
  double ex, ey;   // p - b
  double d, gap;   // centre distance; d - (r + r_b): the selection key, rvo3d_safety_scan's bclear term
};
__host__ __device__ inline BuildingPair building_pair(double px, double py, double pz, double r, double bx, double by,
                                                      double bh, double br, double reach, double below) {
  BuildingPair q;
  q.ex = px - bx; q.ey = py - by;
  q.d = __builtin_sqrt(q.ex * q.ex + q.ey * q.ey);
  q.gap = q.d - (r + br);
  q.pass = bh > pz - below && q.d <= reach;
  return q;
}
// cal_exp_tim_with_building (rvo_inter.py:249-275): the time until the drone's disc, moving at (vx, vy), touches the
// building's, in the plane; 0 inside, +inf when it never does
__host__ __device__ inline double building_time(double ex, double ey, double vx, double vy, double R) {
  const double a = vx * vx + vy * vy;
  const double bq = (2.0 * ex) * vx + (2.0 * ey) * vy;
  const double c = (ex * ex + ey * ey) - R * R;
  if (c <= 0.0) return 0.0;
  const double disc = bq * bq - (4.0 * a) * c;
  if (disc <= 0.0) return safety_inf();
  const double s = __builtin_sqrt(disc);
  const double t1 = (-bq + s) / (2.0 * a), t2 = (-bq - s) / (2.0 * a);
  const double t3 = t1 >= 0.0 ? t1 : safety_inf(), t4 = t2 >= 0.0 ? t2 : safety_inf();
  return t4 < t3 ? t4 : t3;
}
// the six floats of a kept building
__host__ __device__ inline void building_row(double px, double py, double pz, double vx, double vy, double r, double bx,
                                             double by, double bh, double br, float* out) {
  const BuildingPair q = building_pair(px, py, pz, r, bx, by, bh, br, 0.0, 0.0);  // (the gate's outcome is not used)
  const double t = building_time(q.ex, q.ey, vx, vy, r + br);
  const double urg = 1.0 / (t + kExpRadius);  // the VO rows' input_exp_time (rvo_inter.py:189)
  out[0] = building_r2f(bx - px); out[1] = building_r2f(by - py); out[2] = building_r2f(bh - pz);
  out[3] = building_r2f(br); out[4] = building_r2f(q.gap); out[5] = building_r2f(urg);
}
// the eight floats of a kept building that moves at (vbx, vby): the first five as above
__host__ __device__ inline void building_row_moving(double px, double py, double pz, double vx, double vy, double r,
                                                    double bx, double by, double bh, double br, double vbx, double vby,
                                                    float* out) {
  const BuildingPair q = building_pair(px, py, pz, r, bx, by, bh, br, 0.0, 0.0);
  const double t = building_time(q.ex, q.ey, vx - vbx, vy - vby, r + br);
  const double urg = 1.0 / (t + kExpRadius);
  out[0] = building_r2f(bx - px); out[1] = building_r2f(by - py); out[2] = building_r2f(bh - pz);
  out[3] = building_r2f(br); out[4] = building_r2f(q.gap); out[5] = building_r2f(urg);
  out[6] = building_r2f(vbx); out[7] = building_r2f(vby);
}

// ---- the k nearest: kBldSlots slots sorted by (gap, index), touched through compile-time indices only, so that they
// stay in registers.  Candidates arrive in index order and move in front of a slot only when strictly smaller: equal
// gaps keep the lower index first.  The first k slots of the best eight are the best k.
struct BuildingSlots {
  double gap[kBldSlots];
  int32_t idx[kBldSlots];  // -1: empty (gap +inf)
  int32_t passing;
};
__host__ __device__ inline void building_slots_clear(BuildingSlots& s) {
#pragma unroll
  for (int i = 0; i < kBldSlots; ++i) { s.gap[i] = safety_inf(); s.idx[i] = -1; }
  s.passing = 0;
}
__host__ __device__ inline void building_slots_insert(BuildingSlots& s, double gap, int32_t index) {
  ++s.passing;
#pragma unroll
  for (int i = kBldSlots - 1; i >= 0; --i) {
    const bool here = gap < s.gap[i];
    const bool before = i > 0 && gap < s.gap[i > 0 ? i - 1 : 0];  // (slot i - 1 is still what it was)
    s.idx[i] = before ? s.idx[i > 0 ? i - 1 : 0] : (here ? index : s.idx[i]);
    s.gap[i] = before ? s.gap[i > 0 ? i - 1 : 0] : (here ? gap : s.gap[i]);
  }
}

// ---- the argument checks of rvo3d_building_rows, before the first HIP call.  W: the dense width 12 + 9 * nm, rows_n:
// E * N, rf: floats per building row (6, or 8 for rvo3d_building_rows_moving).  RVO3D_OK or RVO3D_ERR_INVALID with the
// reason in *why.
inline bool building_finite(double x) { return x - x == 0.0; }
inline int building_rows_check(const rvo3d_building_rows_args* a, int W, int64_t rows_n, const char** why,
                               int rf = kBldRowFloats) {
  *why = "";
  if (!a) { *why = "null rvo3d_building_rows_args"; return RVO3D_ERR_INVALID; }
  if (a->k < 1 || a->k > kBldSlots) { *why = "k must be 1..8"; return RVO3D_ERR_INVALID; }
  if (!building_finite(a->reach) || !(a->reach > 0.0)) { *why = "reach must be finite and > 0"; return RVO3D_ERR_INVALID; }
  if (!building_finite(a->below) || !(a->below >= 0.0)) { *why = "below must be finite and >= 0"; return RVO3D_ERR_INVALID; }
  if (!a->rows) { *why = "rows is required"; return RVO3D_ERR_INVALID; }
  const bool six = rf == kBldRowFloats;
  const int64_t bf = (int64_t)rf * a->k;
  if (a->col0 < 0) { *why = "col0 must be >= 0"; return RVO3D_ERR_INVALID; }
  if (!a->obs) {
    if (a->row_ld < (int64_t)a->col0 + bf) { *why = six ? "row_ld must be >= col0 + 6 * k" : "row_ld must be >= col0 + 8 * k"; return RVO3D_ERR_INVALID; }
    return RVO3D_OK;
  }
  if (a->col0 != 12) { *why = "widen mode (obs given) needs col0 == 12"; return RVO3D_ERR_INVALID; }
  if (a->row_ld < (int64_t)W + bf) {
    *why = six ? "widen mode needs row_ld >= 12 + 9 * neighbors_num + 6 * k" : "widen mode needs row_ld >= 12 + 9 * neighbors_num + 8 * k";
    return RVO3D_ERR_INVALID;
  }
  if (rows_n > 0) {  // the floats either side touches: [obs, obs + rows_n * W) and [rows, rows + (rows_n - 1) * row_ld + W + 6k)
    const uintptr_t o0 = (uintptr_t)a->obs, o1 = o0 + (uintptr_t)rows_n * (uintptr_t)W * 4u;
    const uintptr_t r0 = (uintptr_t)a->rows, r1 = r0 + ((uintptr_t)(rows_n - 1) * (uintptr_t)a->row_ld + (uintptr_t)(W + bf)) * 4u;
    if (o0 < r1 && r0 < o1) { *why = "obs and rows overlap"; return RVO3D_ERR_INVALID; }
  }
  return RVO3D_OK;
}
// ... and of rvo3d_building_rows_moving: the above with rows of eight floats, then the motion (its device pointers: what
// they point at is the kernel's to read) and dt.  sets_attached: rvo3d_set_env_buildings is in force on the handle.
inline int building_rows_moving_check(const rvo3d_building_rows_args* a, int W, int64_t rows_n, bool sets_attached,
                                      const rvo3d_building_motion* m, double dt, const char** why) {
  if (int rc = building_rows_check(a, W, rows_n, why, kBldRowFloatsMoving)) return rc;
  if (m && !sets_attached) { *why = "a motion needs attached per-env building sets (rvo3d_set_env_buildings)"; return RVO3D_ERR_STATE; }
  if (m && (!m->ends || !m->speed || !m->leg)) { *why = "ends, speed and leg are required"; return RVO3D_ERR_INVALID; }
  if (!building_finite(dt) || !(dt >= 0.0)) { *why = "dt must be finite and >= 0"; return RVO3D_ERR_INVALID; }
  return RVO3D_OK;
}

// ---- the kernel ----
struct BuildingRowsArgs {
  int32_t k;
  double reach, below;
  float* rows;
  int64_t row_ld;
  int32_t col0;
  int32_t* b_count;
  const float* obs;
};
// the motion of rvo3d_building_rows_moving: [E][nb][2][2], [E][nb], [E][nb] with nb the attached sets' nb_max; speed
// nullptr: no motion, every building stands
struct BuildingVelArgs {
  const double* ends;
  const double* speed;
  const uint8_t* leg;
  double dt;
};

// safety_scan_body's geometry (safety_lanes_per_env / safety_threads): one lane per drone, fleets of up to 64 drones
// packed several envs per 256-thread workgroup, larger ones one workgroup per env; the building records go through LDS
// in tiles of L per env.  Behind the scan the rows leave through LDS as well, kBldStage lanes at a time: each lane of the
// batch stages its 6k (8k) floats (stride 6k + 1 / 8k + 1 dwords: odd, no bank conflicts), then every wave writes whole output rows,
// consecutive lanes consecutive dwords - in widen mode the 12 proprio floats, the building floats and the VO floats of
// the wide row in one sweep.
// LDS at T = 512, k = 8: 16 KiB of records + 24.5 KiB of stage for rows of six floats, 16 KiB + 32.5 KiB for rows of eight.
constexpr int kBldStage = 128;
__host__ __device__ inline int building_stage_stride(int k, int rf = kBldRowFloats) { return rf * k + 1; }
__host__ __device__ inline size_t building_lds_bytes(int n, int k, int rf = kBldRowFloats) {
  return (size_t)safety_threads(n) * 4 * sizeof(double) + (size_t)kBldStage * building_stage_stride(k, rf) * sizeof(float);
}

// RF: floats per building row.  kBldRowFloats: rvo3d_building_rows, V is not read.  kBldRowFloatsMoving: the row writer
// also reads the kept records' speed, leg and one endpoint (V.speed != nullptr) and writes building_row_moving's floats.
template <bool CNT, int RF>
__device__ __forceinline__ void building_rows_body(const Params& P, const BuildingRowsArgs& A, const BuildingVelArgs& V) {
  static_assert(RF == kBldRowFloats || RF == kBldRowFloatsMoving, "rows of six or eight floats");
  extern __shared__ __attribute__((aligned(16))) unsigned char building_lds[];
  const int N = P.N, T = (int)blockDim.x, tid = (int)threadIdx.x;
  const int L = safety_lanes_per_env(N);  // == T for N > 64
  const int epb = T / L;
  const int lshift = N <= 64 ? __builtin_ctz(L) : 0;
  const int sub = N <= 64 ? (tid >> lshift) : 0;
  const int l = tid - sub * L;
  const int64_t slot = (int64_t)blockIdx.x * epb + sub;
  const bool has_env = slot < (int64_t)P.E;
  const int64_t e = has_env ? slot : 0;
  const ColdC& C = P.cold();
  const int n = has_env ? (CNT ? C.counts[e] : N) : 0;  // the env's live drones
  const bool live = l < n;
  const int base = tid - l;  // the env's first slot

  double* s_bx = reinterpret_cast<double*>(building_lds);
  double *s_by = s_bx + T, *s_bh = s_by + T, *s_br = s_bh + T;
  float* s_out = reinterpret_cast<float*>(building_lds + (size_t)T * 4 * sizeof(double));  // [kBldStage][RF * k + 1]

  double px = 0.0, py = 0.0, pz = 0.0, vx = 0.0, vy = 0.0, r = 0.0;
  if (live) {
    const int64_t g = e * N + l;
    px = P.px()[g]; py = P.py()[g]; pz = P.pz()[g]; vx = P.vx()[g]; vy = P.vy()[g]; r = P.radius()[g];
  }

  BuildingSlots S;
  building_slots_clear(S);
  const int nb = C.nb;  // the same for every env: the barriers below are uniform
  const double* rec = C.bld + (size_t)e * C.bld_stride;
  for (int t0 = 0; t0 < nb; t0 += L) {
    __syncthreads();  // the tile before this one has been read
    if (has_env && t0 + l < nb) {
      const double* b = rec + (size_t)(t0 + l) * 4;
      s_bx[tid] = b[0]; s_by[tid] = b[1]; s_bh[tid] = b[2]; s_br[tid] = b[3];
    }
    __syncthreads();
    if (live) {
      const int m = nb - t0 < L ? nb - t0 : L;
      for (int j = 0; j < m; ++j) {
        const BuildingPair q = building_pair(px, py, pz, r, s_bx[base + j], s_by[base + j], s_bh[base + j],
                                             s_br[base + j], A.reach, A.below);
        if (q.pass) building_slots_insert(S, q.gap, t0 + j);
      }
    }
  }

  const int k = A.k, bf = RF * k, sk = building_stage_stride(k, RF);
  if (A.b_count && has_env && l < N) A.b_count[e * N + l] = S.passing < k ? S.passing : k;  // ghosts: 0

  const int W = P.W;
  const int width = A.obs ? W + bf : bf;  // floats written per output row, from column out0 on
  const int out0 = A.obs ? 0 : A.col0;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nwaves = T >> 6;  // (wave: in a scalar register)
  for (int c0 = 0; c0 < T; c0 += kBldStage) {
    if (tid >= c0 && tid < c0 + kBldStage) {
      float* o = s_out + (size_t)(tid - c0) * sk;
      if constexpr (RF == kBldRowFloats) {
#pragma unroll
        for (int i = 0; i < kBldSlots; ++i) {
          if (i < k) {
            float f[RF] = {};
            if (S.idx[i] >= 0) {
              const double* b = rec + (size_t)S.idx[i] * 4;
              building_row(px, py, pz, vx, vy, r, b[0], b[1], b[2], b[3], f);
            }
#pragma unroll
            for (int c = 0; c < RF; ++c) o[i * RF + c] = f[c];
          }
        }
      } else {
        // one copy of the row's arithmetic, the slot picked by a select chain (compile-time indices: registers): 74 VGPRs,
        // where eight unrolled copies of the velocity rule and the time took 124 and two of six waves per SIMD
#pragma unroll 1
        for (int i = 0; i < k; ++i) {
          int32_t idx = -1;
#pragma unroll
          for (int j = 0; j < kBldSlots; ++j) idx = j == i ? S.idx[j] : idx;
          float f[RF] = {};
          if (idx >= 0) {
            const double* b = rec + (size_t)idx * 4;
            const double bx = b[0], by = b[1];
            MotionVel vb{0.0, 0.0};
            if (V.speed) {  // (a kept index is a live record of env e: below nb, never a filler)
              const size_t m = (size_t)e * (size_t)nb + (size_t)idx;
              vb = motion_velocity(bx, by, V.leg[m], V.ends + m * 4, V.speed[m], V.dt);
            }
            building_row_moving(px, py, pz, vx, vy, r, bx, by, b[2], b[3], vb.x, vb.y, f);
          }
#pragma unroll
          for (int c = 0; c < RF; ++c) o[i * RF + c] = f[c];
        }
      }
    }
    __syncthreads();
    const int cn = T - c0 < kBldStage ? T - c0 : kBldStage;
    for (int q = wave; q < cn; q += nwaves) {  // one output row per wave and trip
      const int t = c0 + q;
      const int qsub = N <= 64 ? (t >> lshift) : 0;
      const int ql = t - qsub * L;
      const int64_t qe = (int64_t)blockIdx.x * epb + qsub;
      if (qe >= (int64_t)P.E || ql >= N) continue;
      const bool ghost = CNT && ql >= C.counts[qe];
      const int64_t g = qe * N + ql;
      float* dst = A.rows + g * A.row_ld + out0;
      const float* src = A.obs ? A.obs + g * (int64_t)W : nullptr;
      const float* st = s_out + (size_t)q * sk;
      for (int c = lane; c < width; c += 64) {
        float v;
        if (!A.obs) v = st[c];  // (a ghost staged zeros: its slots are empty)
        else if (ghost) v = 0.f;
        else if (c < 12) v = src[c];
        else if (c < 12 + bf) v = st[c - 12];
        else v = src[c - bf];
        dst[c] = v;
      }
    }
    __syncthreads();  // the batch has left before the next one is staged
  }
}
__global__ void __launch_bounds__(kMaxThreads) building_rows_kernel(const Params P, const BuildingRowsArgs A) {
  building_rows_body<false, kBldRowFloats>(P, A, BuildingVelArgs{});
}
__global__ void __launch_bounds__(kMaxThreads) building_rows_counted_kernel(const Params P, const BuildingRowsArgs A) {
  building_rows_body<true, kBldRowFloats>(P, A, BuildingVelArgs{});
}
__global__ void __launch_bounds__(kMaxThreads) building_rows_moving_kernel(const Params P, const BuildingRowsArgs A,
                                                                           const BuildingVelArgs V) {
  building_rows_body<false, kBldRowFloatsMoving>(P, A, V);
}
__global__ void __launch_bounds__(kMaxThreads) building_rows_moving_counted_kernel(const Params P, const BuildingRowsArgs A,
                                                                                   const BuildingVelArgs V) {
  building_rows_body<true, kBldRowFloatsMoving>(P, A, V);
}

}  // namespace rvo3d
