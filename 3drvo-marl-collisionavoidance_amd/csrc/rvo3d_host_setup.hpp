// rvo3d_host_setup.hpp -- what the host computes for an env handle before anything is allocated: thresholds,
// the float32 error bands, launch geometry, the zero-fill tables, the building grid, the staged world.
// Host only: no function here calls HIP or reads the environment, so tests/host/host_setup_check.hip runs
// all of it on a machine without a GPU.  Failures come back as a status of include/rvo3d.h plus a message.
#pragma once

#include "../../include/rvo3d.h"
#include "rvo3d_params.hpp"
#include "rvo3d_lds.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace rvo3d {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// x ** 2 as the reference computes it: glibc pow (the volatile exponent keeps
// the compiler from folding the call into x * x).
inline volatile double kTwo = 2.0;
inline double py_sq(double x) { return std::pow(x, kTwo); }

// max{x : sqrt(x) <= tau} for the host's correctly rounded sqrt: `norm <= tau`
// in the reference is exactly `norm^2 <= sq_threshold(tau)` on the device.
inline double sq_threshold(double tau) {
  volatile double x = tau * tau;
  while (std::sqrt(std::nextafter((double)x, INFINITY)) <= tau) x = std::nextafter((double)x, INFINITY);
  while (std::sqrt((double)x) > tau) x = std::nextafter((double)x, -INFINITY);
  return x;
}

// Which instantiation a handle's shape runs on: the compile-time ring size NFIX (0 = the generic kernel of
// its NW) and whether N is smaller than it (padded: ghost lanes).  One place decides; launch_nw() launches
// it and rvo3d_kernel_name() reports it.
struct Pick { int nfix; bool pad; };
inline Pick pick_kernel(const Params& P) {
  if (P.nw == 1) {
    // a one-wave workgroup of epb envs: segments of 64 / epb lanes
    const int seg = (P.epb == 1 || P.epb == 2 || P.epb == 4) ? 64 / P.epb : 0;
    if (seg && P.N == seg) return {seg, false};
    if (seg >= 32 && P.N < seg) return {seg, true};  // 33..63 drones on the 64 kernel, 22..31 on the 32 one
    return {0, false};
  }
  // multi-wave workgroups: the compile-time kernels take any N up to their size
  if (P.nw == 2) return {128, true};
  if (P.nw == 3) return {192, true};
  if (P.nw == 4) return {256, true};
  return {0, false};
}

// xy grid for the building gate: ~8 m cells, at most 64 x 64 (bgx == 0: no grid)
inline void building_grid_dims(const rvo3d_config* cfg, Cold& C) {
  C.bgx = C.bgy = 0; C.bg_inv = 0.0;
  if (cfg->num_buildings > 0 && cfg->map_size[0] > 0 && cfg->map_size[1] > 0 &&
      std::isfinite(cfg->map_size[0]) && std::isfinite(cfg->map_size[1])) {
    const double cs = std::fmax(8.0, std::fmax(cfg->map_size[0], cfg->map_size[1]) / 64.0);
    C.bgx = (int)std::ceil(cfg->map_size[0] / cs); C.bgy = (int)std::ceil(cfg->map_size[1] / cs);
    if (C.bgx < 1) C.bgx = 1;
    if (C.bgy < 1) C.bgy = 1;
    C.bg_inv = 1.0 / cs;
  }
}

// The float32 error bands of stage G and stage X1, from C.map and P.T10.
inline void filter_bands(Params& P, Cold& C) {
  // fp32 candidate filter (stage G).  Coordinates are centred on the map and
  // assumed within cmax of it (envs with a drone further out bypass the filter).
  // u = 2^-24.  A centred coordinate carries <= u*cmax of rounding, a difference
  // of two <= eD = u*(2*cmax + 2*10.5); a squared distance at |d| <= 10.5 is off by
  // <= 2*sqrt(3)*10.5*eD + 3*eD^2 + 8u*10.5^2; v.rel by <= |v|_1*(eD + 4u*10.5).
  // Every band below is twice its bound.
  double mx = std::fmax(C.map[0], std::fmax(C.map[1], C.map[2]));
  if (!(mx > 0)) mx = 1.0;
  for (int k = 0; k < 3; ++k) C.cen[k] = 0.5 * C.map[k];
  const double cmax = 0.75 * mx + 16.0;
  const double u = std::ldexp(1.0, -24);
  const double eD = u * (2.0 * cmax + 21.0);
  const double band = 2.0 * (2.0 * 1.7320508 * 10.5 * eD + 3.0 * eD * eD + 8.0 * u * 110.25);
  C.cmax = (float)cmax;
  P.band = std::nextafter((float)band, INFINITY);
  // stage G tests the sign of dx^2 + dy^2 + dz^2 - t' (one fma chain): the chain's own rounding
  // (<= 3 ulp of ~110) is inside the band, which is twice the bound as it is
  const float t10f = std::nextafter((float)(P.T10 + band), INFINITY);
  P.t10n = -std::nextafter(t10f, INFINITY);
  P.bandn = P.band + P.t10n;
  C.kdot = std::nextafter((float)(2.0 * (eD + 4.0 * u * 10.5) * 1.001), INFINITY);
  // stage X1 (wave mode).  With gap = d^2 - R^2 >= x1_gap = 512*band the relative
  // error of gap is <= 1/1024 and |rel| >= sqrt(gap); a direction cosine then
  // carries <= cs = 4*(sqrt(3)*eD/sqrt(gap) + 8u) of error.  K^2 is compared with
  // slack 1 - (4e-3 + 4*cs): 2e-3 for gap's error, the rest for dp, w2 and K.
  const double gap = 512.0 * band;
  const double cs = 4.0 * (1.7320508 * eD / std::sqrt(gap) + 8.0 * u);
  P.x1_gap = (float)gap;
  P.x1_k2 = (float)(1.0 - (4e-3 + 4.0 * cs));
  const double cs_out = cs > 1e-3 ? cs : 1e-3;
  P.x1_cs2 = (float)(cs_out * cs_out);
}

struct Geometry { int threads, blocks, lds; };

// Launch geometry: whole envs per workgroup.  N <= 64: a workgroup is ONE wave holding
// floor(64 / N) envs (its barriers are free, every wave is scheduled independently);
// larger envs get one workgroup of ceil(N / 64) waves each.
// (lds_pad: the diagnostics build's extra LDS bytes, which cap occupancy; 0 in the product)
inline int launch_geometry(int lds_pad, Params& P, Geometry& G, std::string& err) {
  const int N = P.N;
  int nw = (N + 63) / 64;
  P.nw = nw <= 4 ? nw : 8;  // 1..4 waves: the compile-time kernels for 64 / 128 / 192 / 256 drones; beyond: generic
  int epb = P.nw == 1 ? 64 / N : 1;
  if (epb > P.E) epb = P.E;
  // nw = 2 / 3 / 4: the compile-time kernels for 128 / 192 / 256 drones, any N up to that (ghost lanes)
  const int ring = (P.nw >= 2 && P.nw <= 4) ? 64 * P.nw : N;
  const int threads = P.nw == 1 ? 64 : (int)align_up((size_t)ring, 64);
  size_t lds = lds_bytes(threads, P.nm, epb, ring, P.nw);
  lds += (size_t)lds_pad;
  if (lds > 160 * 1024) {
    err = "neighbors_num * num_drones needs more than 160 KiB of LDS";
    return RVO3D_ERR_INVALID;
  }
  P.epb = epb;
  G.threads = threads;
  G.blocks = (P.E + epb - 1) / epb;
  G.lds = (int)lds;
  return RVO3D_OK;
}

// ---- per-env drone counts (rvo3d_set_drone_counts) ----

constexpr int kMaxCountedDrones = 256;  // the largest compile-time ring

// The argument checks of rvo3d_set_drone_counts (N: the handle's num_drones).  detach: the call asks for full envs again.
inline int check_drone_counts(int E, int N, const int32_t* counts, bool& detach, std::string& err) {
  detach = counts == nullptr;
  if (N > kMaxCountedDrones) {
    err = "drone counts need num_drones <= 256 (the compile-time rings)";
    return RVO3D_ERR_INVALID;
  }
  if (detach) return RVO3D_OK;
  for (int e = 0; e < E; ++e)
    if (counts[e] < 1 || counts[e] > N) {
      err = "counts entries must be in [1, num_drones]";
      return RVO3D_ERR_INVALID;
    }
  return RVO3D_OK;
}

// Which instantiation a handle with drone counts runs on: always a padded compile-time ring, the smallest that holds
// the layout's N rows - 32 lanes up to 32 drones (two envs per wave, also where a plain handle packs up to 32 envs of
// two drones into one: the price of the counts for small N), 64 up to 64, then pick_kernel's 128 / 192 / 256.
inline Pick pick_counted_kernel(const Params& P) {
  if (P.N <= 32) return {32, true};
  if (P.N <= 64) return {64, true};
  if (P.N <= 128) return {128, true};
  if (P.N <= 192) return {192, true};
  if (P.N <= kMaxCountedDrones) return {256, true};
  return {0, false};
}

// Its launch geometry (P: the handle's, with nw = ceil(N / 64) - the ring's as well) and whether the handle's
// two-phase table (zero_fill_tables: a full workgroup of G's shape) describes its workgroups too.
inline int counted_geometry(int lds_pad, const Params& P, const Geometry& G, Geometry& out, bool& two_phase,
                            std::string& err) {
  const Pick k = pick_counted_kernel(P);
  if (k.nfix == 0) {
    err = "drone counts need num_drones <= 256 (the compile-time rings)";
    return RVO3D_ERR_INVALID;
  }
  const int epb = k.nfix <= 64 ? 64 / k.nfix : 1;
  out.threads = k.nfix <= 64 ? 64 : k.nfix;
  out.blocks = (P.E + epb - 1) / epb;
  const size_t lds = lds_bytes(out.threads, P.nm, epb, k.nfix, P.nw) + (size_t)lds_pad;
  if (lds > 64 * 1024) {
    err = "neighbors_num * num_drones needs more than 64 KiB of LDS on the counted kernels";
    return RVO3D_ERR_INVALID;
  }
  out.lds = (int)lds;
  two_phase = epb == P.epb && out.threads == G.threads;
  return RVO3D_OK;
}

// The zero-fill index divisor with its magic multiplier, and the two-phase row writer's table.
inline int zero_fill_tables(const Params& P, int threads, Cold& C, std::string& err) {
  const int N = P.N, epb = P.epb;
  // zero-fill geometry: units per row of the VO region (float2 if rows are 8-B aligned)
  C.zf_div = (uint32_t)((P.W & 1) == 0 ? (P.W - 12) / 2 : (P.W - 12));
  C.zf_magic = 0;
  if (C.zf_div > 0) {
    const uint32_t m = (uint32_t)(((1ull << 32) + C.zf_div - 1) / C.zf_div);
    bool ok = true;
    const uint64_t qmax = (uint64_t)threads * C.zf_div;
    for (uint64_t q = 0; q < qmax && ok; ++q) ok = ((q * m) >> 32) == q / C.zf_div;
    if (!ok) {
      err = "neighbors_num too large for the zero-fill index trick";
      return RVO3D_ERR_INVALID;
    }
    C.zf_magic = m;
  }
  C.zf_q = (P.W & 1) == 0 ? (uint32_t)(P.W / 2) : 0u;  // row bytes / 8: the 16-B row writer applies
  // early_zero_blocks: which of its trips a thread quad stores in depends on W and the quad only
  C.zf_iters = 0;
  static_assert(kMaxThreads / 4 <= sizeof(C.zmask) / sizeof(C.zmask[0]),
                "Cold::zmask has one word per thread quad of the largest workgroup");
  std::memset(C.zmask, 0, sizeof C.zmask);
  {
    const uint32_t rb = 4u * (uint32_t)P.W;
    const uint32_t rows_full = (uint32_t)epb * (uint32_t)N, nwv = (uint32_t)threads / 64u;
    const uint32_t nblk = rows_full * rb >> 6;
    const uint32_t iters = (nblk + 16u * nwv - 1u) / (16u * nwv);
    if (C.zf_q != 0 && P.W >= 48 && (rows_full & 7u) == 0 && iters <= 32u) {
      for (uint32_t tq = 0; tq < (uint32_t)threads / 4u; ++tq) {
        uint32_t m = 0;
        for (uint32_t i = 0; i < iters; ++i) {
          const uint32_t blk = tq + 16u * nwv * i;  // tq = wave * 16 + (lane / 4)
          if (blk >= nblk) break;
          const uint32_t o = (blk * 64u) % rb;
          if (o >= 48u && o + 64u <= rb) m |= 1u << i;
        }
        C.zmask[tq] = m;
      }
      C.zf_iters = (int)iters;
    }
  }
  return RVO3D_OK;
}

// Everything rvo3d_create derives from a checked config, in one go: Params and Cold without their
// pointers, and the launch geometry.
inline int plan_env(const rvo3d_config* cfg, int lds_pad, Params& P, Cold& C, Geometry& G, std::string& err) {
  std::memset(&P, 0, sizeof P);
  std::memset(&C, 0, sizeof C);
  P.E = cfg->num_envs; P.N = cfg->num_drones; P.P = cfg->max_points;
  C.nb = cfg->num_buildings; P.nm = cfg->neighbors_num; P.env_train = cfg->env_train ? 1 : 0;
  P.W = 12 + 9 * P.nm;
  C.act_scale = cfg->action_decimals >= 0 ? std::pow(10.0, cfg->action_decimals) : 0.0;
  for (int k = 0; k < 3; ++k) C.map[k] = cfg->map_size[k];
  P.T10 = sq_threshold(10.0);  // rvo_inter.py:96
  C.T5 = sq_threshold(5.0);    // rvo_inter.py:104
  building_grid_dims(cfg, C);
  C.T04 = sq_threshold(0.4);   // drone.py:15 goal_threshold
  filter_bands(P, C);
  if (int rc = launch_geometry(lds_pad, P, G, err)) return rc;
  return zero_fill_tables(P, G.threads, C, err);
}

// The world as rvo3d_load_world copies it to the device: [P][3] rows of EN waypoint coordinates (padded with
// the destination), route lengths, radius / priority with the reference's defaults, 0.95 ** k.
struct StagedWorld { std::vector<double> wp, rl, rad, pri, p95; };
inline int stage_world(Params& P, const double* waypoints, const int32_t* n_points, const double* radius,
                       const double* priority, StagedWorld& w, std::string& err) {
  const size_t EN = (size_t)P.E * P.N;
  std::vector<double> wp((size_t)P.P * 3 * EN), rl(EN), rad(EN), pri(EN), p95(P.P);
  for (size_t g = 0; g < EN; ++g) {
    const int np = n_points[g];
    if (np < 2 || np > P.P) {
      err = "n_points entries must be in [2, max_points]";
      return RVO3D_ERR_INVALID;
    }
    const double* src = waypoints + g * P.P * 3;
    double total = 0.0;  // drone.calculate_total_length (drone.py:409-429)
    for (int k = 0; k < P.P; ++k) {
      const int kk = k < np ? k : np - 1;  // pad with the destination
      for (int c = 0; c < 3; ++c) wp[((size_t)k * 3 + c) * EN + g] = src[kk * 3 + c];
      if (k + 1 < np) {
        const double dx = src[(k + 1) * 3] - src[k * 3], dy = src[(k + 1) * 3 + 1] - src[k * 3 + 1],
                     dz = src[(k + 1) * 3 + 2] - src[k * 3 + 2];
        total += std::sqrt(py_sq(dx) + py_sq(dy) + py_sq(dz));
      }
    }
    rl[g] = total;
    rad[g] = radius ? radius[g] : 0.2;
    pri[g] = priority ? priority[g] : 5.0;
  }
  {
    // one radius and one priority for every drone (bit-identical doubles): the step takes them from
    // its argument block instead of reading 16 B per drone-step
    bool uni = true;
    for (size_t g = 1; g < EN && uni; ++g)
      uni = std::memcmp(&rad[g], &rad[0], 8) == 0 && std::memcmp(&pri[g], &pri[0], 8) == 0;
    P.uniform_rp = uni ? 1 : 0;
    P.r0 = rad[0];
    P.prio0 = pri[0];
  }
  for (int k = 0; k < P.P; ++k) p95[k] = std::pow(0.95, (double)k);  // ir_gym.py:283
  w.wp.swap(wp); w.rl.swap(rl); w.rad.swap(rad); w.pri.swap(pri); w.p95.swap(p95);
  return RVO3D_OK;
}

// The largest drone radius of a handle, as the building lists' reach uses it.
inline double largest_radius(const std::vector<double>& rad) {
  double rmax = 0.0;
  for (size_t g = 0; g < rad.size(); ++g) {
    if (rad[g] != rad[g]) rmax = INFINITY;  // a NaN radius: no pruning beyond the gate
    else if (rad[g] > rmax) rmax = rad[g];
  }
  return rmax;
}

// The per-cell building lists (C.bgx > 0), kBgridK + 1 u16 per cell.
inline std::vector<uint16_t> build_building_grid(const Cold& C, const double* buildings, const std::vector<double>& rad) {
  // cell (ix, iy) = [ix*cs, (ix+1)*cs] x [iy*cs, (iy+1)*cs], widened by 1e-3 m (the device
  // finds the cell with floor(x / cs) in floating point) and unbounded at the map's edge
  // (clamped lookups); a building is listed where a drone inside the cell could hit it:
  // within the 5 m gate AND within (largest drone radius + building radius) of its axis
  // (rvo_inter.py:104, :207) - with 0.2 m drones that is 2 cells per building instead of 5
  std::vector<uint16_t> grid;
  const int K = kBgridK;
  const double cs = 1.0 / C.bg_inv;
  const double rmax = largest_radius(rad);
  grid.assign((size_t)C.bgx * C.bgy * (K + 1), 0);
  for (int ix = 0; ix < C.bgx; ++ix)
    for (int iy = 0; iy < C.bgy; ++iy) {
      uint16_t* cell = &grid[((size_t)ix * C.bgy + iy) * (K + 1)];
      const double x0 = ix == 0 ? -INFINITY : ix * cs, x1 = ix == C.bgx - 1 ? INFINITY : (ix + 1) * cs;
      const double y0 = iy == 0 ? -INFINITY : iy * cs, y1 = iy == C.bgy - 1 ? INFINITY : (iy + 1) * cs;
      int n = 0;
      bool overflow = false;
      for (int b = 0; b < C.nb && !overflow; ++b) {
        const double bx = buildings[4 * b], by = buildings[4 * b + 1];
        double reach = rmax + buildings[4 * b + 3];
        if (!(reach < 5.0)) reach = 5.0;  // the gate (also a NaN radius)
        reach += 1e-3;
        const double dx = bx < x0 ? x0 - bx : (bx > x1 ? bx - x1 : 0.0);
        const double dy = by < y0 ? y0 - by : (by > y1 ? by - y1 : 0.0);
        if (!(dx * dx + dy * dy > reach * reach)) {  // also keeps NaN centres
          if (n == K || b > 0xfffe) overflow = true;
          else cell[1 + n++] = (uint16_t)b;
        }
      }
      cell[0] = overflow ? 0xffff : (uint16_t)n;
    }
  return grid;
}

// ---- per-env building sets (rvo3d_set_env_buildings) ----

constexpr int kMaxBuildings = 0xfffe;                   // u16 list entries; 0xffff is the "test all" count
constexpr size_t kBgridCellBytes = (kBgridK + 1) * 2;  // one cell: count + kBgridK indices
constexpr size_t kEnvGridBudget = (size_t)64 << 20;    // the cells of all envs together

// The argument checks of rvo3d_set_env_buildings.  detach: the call asks for the shared list again.
inline int check_env_buildings(int E, const double* buildings, const int32_t* counts, int32_t nb_max, bool& detach,
                               std::string& err) {
  detach = false;
  if (nb_max < 0) {
    err = "nb_max must be >= 0";
    return RVO3D_ERR_INVALID;
  }
  if (nb_max > kMaxBuildings) {
    err = "nb_max must stay below 65535 (16-bit building indices)";
    return RVO3D_ERR_INVALID;
  }
  if (!buildings || nb_max == 0) {
    if (buildings == nullptr && nb_max > 0 && counts) {
      err = "counts without buildings";
      return RVO3D_ERR_INVALID;
    }
    detach = true;
    return RVO3D_OK;
  }
  if (counts)
    for (int e = 0; e < E; ++e)
      if (counts[e] < 0 || counts[e] > nb_max) {
        err = "counts entries must be in [0, nb_max]";
        return RVO3D_ERR_INVALID;
      }
  return RVO3D_OK;
}

// The argument checks of rvo3d_move_env_buildings (its rvo3d_building_motion holds device pointers: what they point at
// is the kernel's to read).  sets_attached: rvo3d_set_env_buildings is in force on the handle.
inline int check_move_env_buildings(bool world_loaded, bool sets_attached, const rvo3d_building_motion* m, double dt,
                                    std::string& err) {
  if (!world_loaded) {
    err = "rvo3d_load_world has not been called";
    return RVO3D_ERR_STATE;
  }
  if (!sets_attached) {
    err = "no per-env building sets are attached (rvo3d_set_env_buildings)";
    return RVO3D_ERR_STATE;
  }
  if (!m) {
    err = "null rvo3d_building_motion";
    return RVO3D_ERR_INVALID;
  }
  if (!m->ends || !m->speed || !m->leg) {
    err = "ends, speed and leg are required";
    return RVO3D_ERR_INVALID;
  }
  if (!std::isfinite(dt) || !(dt >= 0.0)) {
    err = "dt must be finite and >= 0";
    return RVO3D_ERR_INVALID;
  }
  return RVO3D_OK;
}

// The checks rvo3d_sample_routes_city and rvo3d_plan_routes make of their rvo3d_city (its pointers are device
// pointers: what they point at is the kernels' to bound).
inline int check_city(const rvo3d_city* c, std::string& err) {
  if (!c) {
    err = "city is required";
    return RVO3D_ERR_INVALID;
  }
  if (!std::isfinite(c->clear_xy) || !std::isfinite(c->clear_z) || !(c->clear_xy >= 0.0) || !(c->clear_z >= 0.0)) {
    err = "clear_xy and clear_z must be finite and >= 0";
    return RVO3D_ERR_INVALID;
  }
  if (!std::isfinite(c->pad) || !(c->pad > 0.0)) {
    err = "pad must be finite and > 0";
    return RVO3D_ERR_INVALID;
  }
  if (c->nb_max < 0 || c->nb_max > kMaxBuildings) {
    err = "nb_max must be in [0, 65535)";
    return RVO3D_ERR_INVALID;
  }
  if (c->env_stride != 0 && c->env_stride != (int64_t)c->nb_max * 4) {
    err = "env_stride must be 0 (one shared list) or nb_max * 4 (a set per env)";
    return RVO3D_ERR_INVALID;
  }
  if (c->nb_max > 0 && !c->buildings) {
    err = "buildings is required when nb_max > 0";
    return RVO3D_ERR_INVALID;
  }
  return RVO3D_OK;
}

// Grid dimensions of the per-env lists: the shared path's (building_grid_dims) when E grids of them fit the
// budget, else the cell size grows until they do - down to one cell per env, which is the floor (beyond
// budget / 32 envs even that exceeds the budget).  Results do not depend on the dimensions: the lists are
// conservative and an overflowing cell tests every building.
inline void env_grid_dims(const rvo3d_config* cfg, int E, size_t budget, Cold& C) {
  rvo3d_config c = *cfg;
  c.num_buildings = 1;
  building_grid_dims(&c, C);
  if (C.bgx == 0) return;
  const size_t cells_max = budget / (kBgridCellBytes * (size_t)E);
  double cs = 1.0 / C.bg_inv;
  while ((size_t)C.bgx * C.bgy > cells_max && (C.bgx > 1 || C.bgy > 1)) {
    cs *= 1.125;
    C.bgx = (int)std::ceil(cfg->map_size[0] / cs); C.bgy = (int)std::ceil(cfg->map_size[1] / cs);
    if (C.bgx < 1) C.bgx = 1;
    if (C.bgy < 1) C.bgy = 1;
    C.bg_inv = 1.0 / cs;
  }
}

// What rvo3d_set_env_buildings copies to the device: [E][nb_max][4] records - env e's unused records
// counts[e] .. nb_max - 1 hold a building no drone can hit (h = -inf: `bh > z - 2` and `z <= bh` are false for
// every z, NaN included) - and [E][bgx * bgy] cells, env e's being build_building_grid of its own list.
// C: the handle's Cold with the dimensions of env_grid_dims; rmax: largest_radius of the loaded world.
struct StagedEnvBuildings { std::vector<double> bld; std::vector<uint16_t> grid; };
inline void stage_env_buildings(const Cold& C, int E, const double* buildings, const int32_t* counts, int32_t nb_max,
                                double rmax, StagedEnvBuildings& out) {
  const size_t rec = (size_t)nb_max * 4, cells = (size_t)C.bgx * C.bgy * (kBgridK + 1);
  out.bld.assign((size_t)E * rec, 0.0);
  out.grid.clear();
  out.grid.reserve((size_t)E * cells);
  const std::vector<double> rad(1, rmax);
  Cold Ce = C;
  for (int e = 0; e < E; ++e) {
    const int n = counts ? counts[e] : nb_max;
    double* dst = &out.bld[(size_t)e * rec];
    std::memcpy(dst, buildings + (size_t)e * rec, (size_t)n * 32);
    for (int b = n; b < nb_max; ++b) dst[4 * b + 2] = -INFINITY;
    if (C.bgx > 0) {
      Ce.nb = n;
      const std::vector<uint16_t> g = build_building_grid(Ce, dst, rad);
      out.grid.insert(out.grid.end(), g.begin(), g.end());
    }
  }
}

}  // namespace rvo3d
