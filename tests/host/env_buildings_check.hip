// env_buildings_check.hip -- stand-alone check of the per-env building sets' host set-up (csrc/rvo3d_host_setup.hpp:
// check_env_buildings, env_grid_dims, stage_env_buildings).  Calls no HIP function and needs no GPU;
// tests/test_env_buildings_host.py builds it with the host sanitizers and runs it.  Exit status 0 = every check held.
#include "rvo3d_params.hpp"
#include "rvo3d_lds.hpp"
#include "rvo3d_host_setup.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace rvo3d;

static long g_checks = 0;
#define REQUIRE(cond, ...)                                       \
  do {                                                           \
    ++g_checks;                                                  \
    if (!(cond)) {                                               \
      std::fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                         \
      std::fprintf(stderr, "\n");                                \
      std::exit(1);                                              \
    }                                                            \
  } while (0)

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t seed) : g(seed) {}
  double uni(double lo, double hi) { return lo + (hi - lo) * (double)(g() >> 11) * (1.0 / 9007199254740992.0); }
  uint64_t below(uint64_t n) { return g() % n; }
};

static rvo3d_config config(int E, const double* map) {
  rvo3d_config c{};
  c.num_envs = E; c.num_drones = 4; c.max_points = 2; c.num_buildings = 0; c.neighbors_num = 3;
  c.env_train = 1; c.device = 0; c.action_decimals = -1;
  for (int k = 0; k < 3; ++k) c.map_size[k] = map[k];
  return c;
}

// a. the validator
static void check_validator() {
  const double b[8 * 4] = {};
  bool detach = true;
  std::string err;
  const int32_t ok[3] = {0, 2, 1}, neg[3] = {0, -1, 1}, big[3] = {0, 3, 1};
  REQUIRE(check_env_buildings(3, b, ok, 2, detach, err) == RVO3D_OK && !detach, "counts in range");
  REQUIRE(check_env_buildings(3, b, nullptr, 2, detach, err) == RVO3D_OK && !detach, "NULL counts = nb_max everywhere");
  REQUIRE(check_env_buildings(3, b, neg, 2, detach, err) == RVO3D_ERR_INVALID && !err.empty(), "counts[e] < 0");
  REQUIRE(check_env_buildings(3, b, big, 2, detach, err) == RVO3D_ERR_INVALID, "counts[e] > nb_max");
  REQUIRE(check_env_buildings(3, b, nullptr, -1, detach, err) == RVO3D_ERR_INVALID, "nb_max < 0");
  // the index bound: 0xffff is the "test all" count, so 0xfffe buildings (indices 0 .. 0xfffd) are the most
  REQUIRE(kMaxBuildings == 0xfffe, "bound");
  REQUIRE(check_env_buildings(3, b, nullptr, 0xffff, detach, err) == RVO3D_ERR_INVALID, "nb_max at the bound");
  REQUIRE(check_env_buildings(3, b, nullptr, 0x10000, detach, err) == RVO3D_ERR_INVALID, "nb_max over the bound");
  REQUIRE(check_env_buildings(3, b, nullptr, 0x7fffffff, detach, err) == RVO3D_ERR_INVALID, "nb_max far over the bound");
  // (the validator reads counts only: a list of the largest accepted size needs no storage here)
  REQUIRE(check_env_buildings(3, b, nullptr, 0xfffe, detach, err) == RVO3D_OK && !detach, "the largest nb_max");
  REQUIRE(check_env_buildings(3, nullptr, nullptr, 0, detach, err) == RVO3D_OK && detach, "detach");
  REQUIRE(check_env_buildings(3, nullptr, nullptr, 5, detach, err) == RVO3D_OK && detach, "detach: no buildings");
  REQUIRE(check_env_buildings(3, b, ok, 0, detach, err) == RVO3D_OK && detach, "detach: nb_max == 0");
  REQUIRE(check_env_buildings(3, nullptr, ok, 2, detach, err) == RVO3D_ERR_INVALID, "counts without buildings");
}

// b. the budget rule
static void check_budget() {
  const double maps[5][3] = {{10, 10, 5}, {100, 100, 10}, {100, 80, 10}, {500, 500, 10}, {2000, 300, 50}};
  const int envs[] = {1, 3, 1024, 4096, 32768, 100000, 1 << 20, 1 << 21};
  const size_t budgets[] = {kEnvGridBudget, (size_t)1 << 20, 4096, 32};
  REQUIRE(kEnvGridBudget == ((size_t)64 << 20) && kBgridCellBytes == 32, "64 MiB, 32 B per cell");
  for (auto& map : maps)
    for (int E : envs)
      for (size_t budget : budgets) {
        rvo3d_config c = config(E, map);
        Cold S{}, C{};
        c.num_buildings = 7;
        building_grid_dims(&c, S);  // the shared path's
        c.num_buildings = 0;        // as the handle of a per-env world is created
        env_grid_dims(&c, E, budget, C);
        REQUIRE(C.bgx >= 1 && C.bgy >= 1 && C.bg_inv > 0, "at least 1 x 1 (%d x %d)", C.bgx, C.bgy);
        const size_t bytes = (size_t)E * C.bgx * C.bgy * kBgridCellBytes;
        if ((size_t)E * kBgridCellBytes <= budget) REQUIRE(bytes <= budget, "E %d: %zu bytes over %zu", E, bytes, budget);
        else REQUIRE(C.bgx == 1 && C.bgy == 1, "one cell per env is the floor");
        if ((size_t)E * S.bgx * S.bgy * kBgridCellBytes <= budget)
          REQUIRE(C.bgx == S.bgx && C.bgy == S.bgy && C.bg_inv == S.bg_inv, "the shared path's dimensions fit: kept");
        else if (S.bgx * S.bgy > 1) REQUIRE(C.bg_inv < S.bg_inv && C.bgx * C.bgy < S.bgx * S.bgy, "cells grew");
      }
  {  // no finite map: no grid, as on the shared path
    const double nomap[3] = {0, 10, 5};
    rvo3d_config c = config(4, nomap);
    Cold C{};
    env_grid_dims(&c, 4, kEnvGridBudget, C);
    REQUIRE(C.bgx == 0 && C.bgy == 0, "no grid");
  }
}

// c. env e's records and cells
static void check_staging(uint64_t seed, const double* map, int E, int nb_max, size_t budget, bool with_counts, bool nan_radius) {
  Rng r(seed);
  const int N = 4;
  rvo3d_config c = config(E, map);
  Cold C{};
  env_grid_dims(&c, E, budget, C);
  C.nb = nb_max;
  // per-drone radii; building radii beyond the 5 m gate
  std::vector<double> rad((size_t)E * N);
  for (auto& x : rad) x = r.uni(0.1, 0.9);
  if (nan_radius) rad[r.below(rad.size())] = NAN;
  const double rmax = largest_radius(rad);
  REQUIRE(nan_radius ? std::isinf(rmax) : (rmax >= 0.1 && rmax <= 0.9), "rmax %g", rmax);
  std::vector<double> bld((size_t)E * nb_max * 4);
  std::vector<int32_t> counts(E);
  for (int e = 0; e < E; ++e) {
    counts[e] = with_counts ? (int32_t)r.below((uint64_t)nb_max + 1) : nb_max;
    const bool cluster = r.below(2) != 0;  // half of the envs crowd one spot: overflowing cells
    const double cx = r.uni(0, map[0]), cy = r.uni(0, map[1]);
    for (int b = 0; b < nb_max; ++b) {
      double* q = &bld[((size_t)e * nb_max + b) * 4];
      q[0] = cluster && b % 2 ? cx + r.uni(-3, 3) : r.uni(-2.0, map[0] + 2.0);
      q[1] = cluster && b % 2 ? cy + r.uni(-3, 3) : r.uni(-2.0, map[1] + 2.0);
      q[2] = r.uni(0.5, map[2]);
      q[3] = r.below(4) == 0 ? r.uni(4.0, 7.0) : r.uni(0.05, 1.5);
    }
  }
  StagedEnvBuildings w;
  stage_env_buildings(C, E, bld.data(), with_counts ? counts.data() : nullptr, nb_max, rmax, w);
  const size_t rec = (size_t)nb_max * 4, cells = (size_t)C.bgx * C.bgy, K1 = kBgridK + 1;
  REQUIRE(w.bld.size() == (size_t)E * rec && w.grid.size() == (size_t)E * cells * K1, "sizes");
  long listed = 0, overflowing = 0, sampled_hits = 0;
  for (int e = 0; e < E; ++e) {
    const int n = counts[e];
    // records: the env's own, bit for bit, then buildings nobody can hit
    REQUIRE(n == 0 || std::memcmp(&w.bld[e * rec], &bld[e * rec], (size_t)n * 32) == 0, "env %d records", e);
    for (int b = n; b < nb_max; ++b) {
      const double bh = w.bld[e * rec + 4 * b + 2];
      REQUIRE(bh == -INFINITY, "env %d padding record %d", e, b);
      for (double z : {(double)-INFINITY, -1e300, 0.0, 5.0, 1e300, (double)INFINITY, (double)NAN})
        REQUIRE(!(bh > z - 2), "a padding record fails the gate's height test at z = %g", z);  // (so the gate fails)
    }
    // cells: u16 for u16 what build_building_grid gives for env e's list alone, with every drone's radius
    Cold Ce = C;
    Ce.nb = n;
    const std::vector<uint16_t> alone = build_building_grid(Ce, &bld[e * rec], rad);
    REQUIRE(alone.size() == cells * K1, "env %d grid size", e);
    REQUIRE(std::memcmp(alone.data(), &w.grid[e * cells * K1], alone.size() * 2) == 0, "env %d cells", e);
    // coverage, by brute force over sample points: whatever a drone of radius rmax at p could touch within the
    // 5 m gate is in the list of p's cell (found as the device finds it: floor, clamped), or the cell overflows
    for (int it = 0; it < 400; ++it) {
      double px = r.uni(-3.0, map[0] + 3.0), py = r.uni(-3.0, map[1] + 3.0);
      if (n > 0 && (it & 1)) {  // every other point next to one of the env's buildings
        const double* q = &bld[e * rec + 4 * r.below((uint64_t)n)];
        px = q[0] + r.uni(-4.0, 4.0); py = q[1] + r.uni(-4.0, 4.0);
      }
      int ix = (int)std::floor(px * C.bg_inv), iy = (int)std::floor(py * C.bg_inv);
      ix = ix < 0 ? 0 : (ix > C.bgx - 1 ? C.bgx - 1 : ix);
      iy = iy < 0 ? 0 : (iy > C.bgy - 1 ? C.bgy - 1 : iy);
      const uint16_t* cell = &w.grid[(e * cells + (size_t)ix * C.bgy + iy) * K1];
      const int cnt = cell[0];
      REQUIRE(cnt == 0xffff || cnt <= kBgridK, "count %d", cnt);
      if (cnt == 0xffff) { ++overflowing; continue; }
      for (int k = 1; k <= cnt; ++k) REQUIRE(cell[k] < n, "env %d lists building %d of %d", e, (int)cell[k], n);
      listed += cnt;
      for (int b = 0; b < n; ++b) {
        const double* q = &bld[e * rec + 4 * b];
        const double dis = std::sqrt((px - q[0]) * (px - q[0]) + (py - q[1]) * (py - q[1]));
        if (dis <= 5.0 && dis <= rmax + q[3]) {
          ++sampled_hits;
          bool found = false;
          for (int k = 1; k <= cnt; ++k) found |= cell[k] == b;
          REQUIRE(found, "env %d: building %d within reach of (%g, %g) is not listed in cell (%d, %d)", e, b, px, py, ix, iy);
        }
      }
    }
  }
  std::printf("staging seed %llu: E %d nb_max %d grid %d x %d: %ld entries seen, %ld overflowing lookups, %ld reachable pairs\n",
              (unsigned long long)seed, E, nb_max, C.bgx, C.bgy, listed, overflowing, sampled_hits);
  REQUIRE(nb_max == 0 || sampled_hits > 0, "the brute-force check saw no building within reach");
}

int main() {
  check_validator();
  check_budget();
  const double m1[3] = {24, 24, 8}, m2[3] = {100, 80, 10}, m3[3] = {300, 500, 10};
  check_staging(1, m1, 7, 40, kEnvGridBudget, true, false);
  check_staging(2, m2, 5, 50, kEnvGridBudget, false, false);
  check_staging(3, m2, 9, 64, 9 * 20 * 32, true, false);  // a budget that forces larger cells
  check_staging(4, m3, 6, 30, 6 * 32, true, false);       // one cell per env
  check_staging(5, m3, 4, 120, kEnvGridBudget, true, true);  // a NaN radius: the reach is the gate
  check_staging(6, m1, 3, 1, kEnvGridBudget, true, false);
  std::printf("env buildings ok: %ld checks\n", g_checks);
  return 0;
}
