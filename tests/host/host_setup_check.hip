// host_setup_check.hip -- stand-alone check of csrc/rvo3d_host_setup.hpp: what the host derives for an env handle,
// tested against properties stated from first principles.  Calls no HIP function and needs no GPU;
// tests/test_host_setup.py builds it with the host sanitizers and runs it.  Exit status 0 = every check held.
#include "rvo3d_params.hpp"
#include "rvo3d_lds.hpp"
#include "rvo3d_host_setup.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static const int kN[] = {1, 5, 8, 16, 22, 32, 40, 63, 64, 65, 100, 128, 129, 192, 200, 256, 257, 300, 512};
static const int kNm[] = {0, 1, 3, 5, 10, 12};
static const int kE[] = {1, 3, 4096};
static const double kMaps[][3] = {{10, 10, 5}, {100, 80, 10}, {500, 500, 10}, {2000, 2000, 50}, {6000, 300, 30},
                                  {8000, 8000, 50}};
static const int kNumMaps = (int)(sizeof(kMaps) / sizeof(kMaps[0]));
static const char* const kLdsMsg = "neighbors_num * num_drones needs more than 160 KiB of LDS";

static rvo3d_config config(int E, int N, int nm, const double* map, int nb = 0, int max_points = 4) {
  rvo3d_config c{};
  c.num_envs = E; c.num_drones = N; c.max_points = max_points; c.num_buildings = nb; c.neighbors_num = nm;
  c.env_train = 1; c.device = 0; c.action_decimals = -1;
  for (int k = 0; k < 3; ++k) c.map_size[k] = map[k];
  return c;
}

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t seed) : g(seed) {}
  double uni(double lo, double hi) { return lo + (hi - lo) * (double)(g() >> 11) * (1.0 / 9007199254740992.0); }
  uint64_t below(uint64_t n) { return g() % n; }
};

// a. max{x : sqrt(x) <= tau}
static void check_thresholds() {
  for (double tau : {10.0, 5.0, 0.4}) {
    const double T = sq_threshold(tau);
    REQUIRE(std::sqrt(T) <= tau, "tau %g", tau);
    REQUIRE(std::sqrt(std::nextafter(T, INFINITY)) > tau, "tau %g", tau);
  }
}

// b. the float32 squared distance of a pair at most 10.5 m apart, both within cmax of the centre, is within band / 2,
//    and its float32 v . rel (the fma chain of x1_pairs, v cast to float as stage_f32 casts it) within half of the
//    drone's kd = kdot |v|_1
static void check_bands(const double* map, const Params& P, const Cold& C) {
  REQUIRE(P.T10 == sq_threshold(10.0) && C.T5 == sq_threshold(5.0) && C.T04 == sq_threshold(0.4), "thresholds");
  REQUIRE(P.t10n < -(float)P.T10, "t10n %a", P.t10n);
  REQUIRE(P.bandn == P.band + P.t10n, "bandn %a", P.bandn);
  REQUIRE(P.x1_k2 > 0.0f && P.x1_k2 < 1.0f, "x1_k2 %a", P.x1_k2);
  // (P.band is the double band rounded to float, then one float up; 512 x is exact in either format)
  REQUIRE(P.x1_gap == 512.0f * std::nextafter(P.band, 0.0f), "x1_gap %a band %a", P.x1_gap, P.band);
  REQUIRE(P.band > 0.0f && C.kdot > 0.0f && P.x1_cs2 > 0.0f, "positive bands");
  for (int k = 0; k < 3; ++k) REQUIRE(C.cen[k] == 0.5 * map[k], "cen");
  Rng r(0x5eed0000u + (uint64_t)map[0] + (uint64_t)map[1]);
  const double cm = (double)C.cmax * 0.999999;
  double worst = 0.0, worst_dot = 0.0;
  for (int it = 0; it < 2000000; ++it) {
    double a[3], b[3], off[3], v[3], n2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double mag = (it & 1) ? r.uni(0.5 * cm, cm) : r.uni(0.0, cm);  // half of them far out: the largest rounding
      a[k] = r.below(2) ? mag : -mag;
      off[k] = r.uni(-1.0, 1.0);
      n2 += off[k] * off[k];
    }
    const double len = (it & 2) ? r.uni(10.0, 10.499) : r.uni(0.0, 10.499);
    const double sc = n2 > 0.0 ? len / std::sqrt(n2) : 0.0;
    float d[3], fv[3];
    double d2 = 0.0, dotp = 0.0;
    const double vscale = (it & 4) ? 10.0 : 1.0;  // |v|_1 of order 1 and of order 10
    for (int k = 0; k < 3; ++k) {
      v[k] = vscale * r.uni(-1.0, 1.0);
      fv[k] = (float)v[k];
      b[k] = a[k] + off[k] * sc;
      if (std::fabs(b[k]) > cm) b[k] = a[k] - off[k] * sc;  // (cmax >= 16 > 10.5: this one is inside)
      const double xa = C.cen[k] + a[k], xb = C.cen[k] + b[k];  // the coordinates as the state holds them
      const double ca = xa - C.cen[k], cb = xb - C.cen[k];      // centred in double, cast to float
      REQUIRE(std::fabs(ca) <= (double)C.cmax && std::fabs(cb) <= (double)C.cmax, "sample outside cmax");
      d[k] = (float)ca - (float)cb;
      d2 += (xa - xb) * (xa - xb);
      dotp += v[k] * (xa - xb);
    }
    REQUIRE(d2 <= 10.5 * 10.5, "sample too far apart: %g", d2);
    const float d2f = std::fma(d[2], d[2], std::fma(d[1], d[1], d[0] * d[0]));
    const double e = std::fabs((double)d2f - d2);
    if (e > worst) worst = e;
    REQUIRE(e <= 0.5 * (double)P.band, "map %g: fp32 d2 off by %g, band %g", map[0], e, (double)P.band);
    const float dotf = std::fma(fv[2], d[2], std::fma(fv[1], d[1], fv[0] * d[0]));
    const double kd = (double)C.kdot * ((double)std::fabs(fv[0]) + (double)std::fabs(fv[1]) + (double)std::fabs(fv[2]));
    const double ed = std::fabs((double)dotf - dotp);
    if (kd > 0.0 && ed / kd > worst_dot) worst_dot = ed / kd;
    REQUIRE(ed <= 0.5 * kd, "map %g: fp32 v.rel off by %g, kd %g", map[0], ed, kd);
  }
  std::printf("kdot: map %g x %g x %g  worst |v.rel f32 - v.rel| = %.3f x kd\n", map[0], map[1], map[2], worst_dot);
  std::printf("band: map %g x %g x %g  worst |d2f - d2| = %.3f x band\n", map[0], map[1], map[2], worst / (double)P.band);
}

// c. / d.  the two-phase row writer's table and the magic divisor
static void check_zero_fill(const Params& P, const Cold& C, const Geometry& G) {
  const uint32_t threads = (uint32_t)G.threads, rb = 4u * (uint32_t)P.W, nwv = threads / 64u;
  const uint32_t rows = (uint32_t)(P.epb * P.N);  // the rows of a full workgroup
  const uint32_t nblk = rows * rb / 64u, trips = (nblk + 16u * nwv - 1u) / (16u * nwv);
  const bool table = (P.W % 2) == 0 && P.W >= 48 && rows % 8u == 0 && trips <= 32u;
  REQUIRE(C.zf_iters == (table ? (int)trips : 0), "zf_iters %d for N %d nm %d epb %d", C.zf_iters, P.N, P.nm, P.epb);
  for (uint32_t tq = 0; tq < sizeof(C.zmask) / sizeof(C.zmask[0]); ++tq)
    for (uint32_t i = 0; i < 32u; ++i) {
      bool want = false;
      const uint32_t blk = tq + 16u * nwv * i;
      if (table && tq < threads / 4u && i < trips && blk < nblk) {
        want = true;
        for (uint32_t b = blk * 64u; b < blk * 64u + 64u; ++b) want = want && b % rb >= 48u;
      }
      REQUIRE(((C.zmask[tq] >> i) & 1u) == (want ? 1u : 0u), "zmask[%u] bit %u for N %d nm %d epb %d", tq, i, P.N,
              P.nm, P.epb);
    }
  REQUIRE(C.zf_div == (uint32_t)(P.W % 2 == 0 ? (P.W - 12) / 2 : P.W - 12), "zf_div");
  REQUIRE(C.zf_q == (P.W % 2 == 0 ? (uint32_t)P.W / 2u : 0u), "zf_q");
  if (C.zf_div > 0) {
    const uint64_t m = C.zf_magic;
    bool ok = true;
    for (uint64_t q = 0; q < (uint64_t)threads * C.zf_div; ++q) ok = ok && ((q * m) >> 32) == q / C.zf_div;
    REQUIRE(ok, "zf_magic %u for zf_div %u, %u threads", C.zf_magic, C.zf_div, threads);
  } else {
    REQUIRE(C.zf_magic == 0, "zf_magic without a divisor");
  }
}

// e. launch geometry and the kernel it selects
static void check_geometry(const rvo3d_config& c, const Params& P, const Geometry& G) {
  const int N = c.num_drones, E = c.num_envs;
  REQUIRE(P.nw == (N <= 256 ? (N + 63) / 64 : 8), "nw %d for N %d", P.nw, N);
  REQUIRE(P.epb >= 1 && P.epb <= E, "epb %d", P.epb);
  if (P.nw == 1) REQUIRE(P.epb * N <= 64, "epb %d N %d", P.epb, N);
  else REQUIRE(P.epb == 1, "epb %d N %d", P.epb, N);
  if (P.nw <= 4) REQUIRE(G.threads == 64 * P.nw, "threads %d nw %d", G.threads, P.nw);
  REQUIRE(G.threads >= P.epb * N && G.threads % 64 == 0 && G.threads <= kMaxThreads, "threads %d", G.threads);
  REQUIRE((long long)G.blocks * P.epb >= E && (long long)(G.blocks - 1) * P.epb < E, "blocks %d", G.blocks);
  REQUIRE(G.lds > 0 && G.lds <= 160 * 1024, "lds %d", G.lds);
  const Pick k = pick_kernel(P);
  REQUIRE(k.nfix == 0 || N <= k.nfix, "nfix %d N %d", k.nfix, N);
  if (!k.pad) REQUIRE(k.nfix == 0 || N == k.nfix, "nfix %d N %d unpadded", k.nfix, N);
  if (k.nfix != 0 && P.nw == 1) REQUIRE(P.epb * k.nfix == 64, "nfix %d epb %d", k.nfix, P.epb);
  if (P.nw >= 2 && P.nw <= 4) REQUIRE(k.nfix == 64 * P.nw, "nfix %d nw %d", k.nfix, P.nw);
}

static void check_matrix() {
  int shapes = 0;
  for (int mi = 0; mi < kNumMaps; ++mi) {
    bool bands_done = false;
    for (int N : kN) for (int nm : kNm) for (int E : kE) {
      const rvo3d_config c = config(E, N, nm, kMaps[mi]);
      Params P; Cold C; Geometry G{}; std::string err;
      const int rc = plan_env(&c, 0, P, C, G, err);
      REQUIRE(rc == RVO3D_OK && err.empty(), "plan_env(%d x %d, nm %d): %s", E, N, nm, err.c_str());
      REQUIRE(P.E == E && P.N == N && P.nm == nm && P.W == 12 + 9 * nm && P.P == c.max_points, "shape fields");
      check_geometry(c, P, G);
      check_zero_fill(P, C, G);
      if (!bands_done) check_bands(kMaps[mi], P, C);
      bands_done = true;
      // more LDS than a CU has: today's message, and nothing else changes the verdict
      const int over = 160 * 1024 - G.lds + 1;
      Params P2; Cold C2; Geometry G2{}; std::string e2;
      REQUIRE(plan_env(&c, over - 1, P2, C2, G2, e2) == RVO3D_OK && G2.lds == 160 * 1024, "lds pad to the limit");
      REQUIRE(plan_env(&c, over, P2, C2, G2, e2) == RVO3D_ERR_INVALID && e2 == kLdsMsg, "lds over: %s", e2.c_str());
      ++shapes;
    }
  }
  std::printf("matrix: %d shapes\n", shapes);
}

// f. every building a drone at a point could hit is in the list of the point's cell
static void check_building_grid() {
  long pairs = 0, overflowing = 0;
  for (int trial = 0; trial < 40; ++trial) {
    Rng r(0xb1d0000u + (uint64_t)trial);
    const bool dense = trial % 5 == 4;  // a small map full of buildings: cells with more than kBgridK
    const double hi = dense ? 40.0 : 620.0;
    const double map[3] = {r.uni(20.0, hi), r.uni(20.0, hi), 10.0};
    const int nb = dense ? 150 + (int)r.below(151) : 1 + (int)r.below(300);
    const bool nan_radius = trial == 38, nan_centre = trial == 39;
    std::vector<double> bld((size_t)nb * 4), rad(5);
    for (int b = 0; b < nb; ++b) {
      bld[4 * b] = r.uni(-3.0, map[0] + 3.0); bld[4 * b + 1] = r.uni(-3.0, map[1] + 3.0);
      bld[4 * b + 2] = r.uni(1.0, 10.0); bld[4 * b + 3] = r.uni(0.1, 4.0);
    }
    double rmax = trial % 3 == 0 ? 0.2 : r.uni(0.2, 3.1);
    for (size_t g = 0; g < rad.size(); ++g) rad[g] = g == 2 ? rmax : 0.2;
    if (nan_radius) { rad[4] = NAN; rmax = INFINITY; }
    if (nan_centre) bld[4 * (nb / 2)] = bld[4 * (nb / 2) + 1] = NAN;  // passes no distance test: kept everywhere
    const rvo3d_config c = config(1, 5, 0, map, nb);
    Cold C{};
    C.nb = nb;
    building_grid_dims(&c, C);
    REQUIRE(C.bgx >= 1 && C.bgx <= 64 && C.bgy >= 1 && C.bgy <= 64, "grid %d x %d", C.bgx, C.bgy);
    const double cs = 1.0 / C.bg_inv;
    REQUIRE(cs >= 8.0 && C.bgx * cs >= map[0] && C.bgy * cs >= map[1], "cells of %g m do not cover the map", cs);
    const std::vector<uint16_t> grid = build_building_grid(C, bld.data(), rad);
    REQUIRE(grid.size() == (size_t)C.bgx * C.bgy * (kBgridK + 1), "grid size");
    for (int cell = 0; cell < C.bgx * C.bgy; ++cell) {
      const uint16_t n = grid[(size_t)cell * (kBgridK + 1)];
      REQUIRE(n == 0xffff || n <= kBgridK, "count %u", n);
      if (n == 0xffff) { ++overflowing; continue; }
      for (int i = 0; i < n; ++i) REQUIRE(grid[(size_t)cell * (kBgridK + 1) + 1 + i] < nb, "index out of range");
    }
    for (int it = 0; it < 20000; ++it) {
      const double x = r.uni(-3.0, map[0] + 3.0), y = r.uni(-3.0, map[1] + 3.0);
      int ix = (int)std::floor(x * C.bg_inv), iy = (int)std::floor(y * C.bg_inv);  // building_hit's clamped lookup
      ix = ix < 0 ? 0 : (ix > C.bgx - 1 ? C.bgx - 1 : ix);
      iy = iy < 0 ? 0 : (iy > C.bgy - 1 ? C.bgy - 1 : iy);
      const uint16_t* cell = &grid[(size_t)(ix * C.bgy + iy) * (kBgridK + 1)];
      if (cell[0] == 0xffff) continue;
      for (int b = 0; b < nb; ++b) {
        const double dx = x - bld[4 * b], dy = y - bld[4 * b + 1], reach = std::fmin(5.0, rmax + bld[4 * b + 3]);
        const bool nan_b = bld[4 * b] != bld[4 * b];
        if (!nan_b && !(dx * dx + dy * dy <= reach * reach)) continue;
        bool listed = false;
        for (int i = 0; i < cell[0]; ++i) listed = listed || cell[1 + i] == b;
        ++pairs;
        REQUIRE(listed, "trial %d: building %d (%g, %g, r %g) missing at (%g, %g), rmax %g", trial, b, bld[4 * b],
                bld[4 * b + 1], bld[4 * b + 3], x, y, rmax);
      }
    }
  }
  REQUIRE(pairs > 10000 && overflowing > 0, "the trials exercise neither lists nor overflow: %ld, %ld", pairs, overflowing);
  std::printf("building grid: %ld qualifying (point, building) pairs, 0 missed, %ld overflowing cells\n", pairs, overflowing);
  // no buildings, or a map without extent: no grid
  const double flat[3] = {0.0, 50.0, 10.0};
  Cold C{};
  rvo3d_config c = config(1, 5, 0, kMaps[1], 0);
  building_grid_dims(&c, C);
  REQUIRE(C.bgx == 0 && C.bgy == 0 && C.bg_inv == 0.0, "grid without buildings");
  c = config(1, 5, 0, flat, 3);
  building_grid_dims(&c, C);
  REQUIRE(C.bgx == 0 && C.bgy == 0, "grid on a map without extent");
}

// g. the staged world
static void check_stage_world() {
  const int E = 2, N = 3, MP = 5, EN = E * N;
  Params P{};
  P.E = E; P.N = N; P.P = MP;
  Rng r(0x57a9e);
  std::vector<double> wpts((size_t)EN * MP * 3);
  for (double& x : wpts) x = r.uni(0.0, 50.0);
  std::vector<int32_t> np = {2, 5, 3, 2, 4, 5};
  StagedWorld w;
  std::string err;
  REQUIRE(stage_world(P, wpts.data(), np.data(), nullptr, nullptr, w, err) == RVO3D_OK, "%s", err.c_str());
  REQUIRE(w.wp.size() == (size_t)MP * 3 * EN && w.rl.size() == (size_t)EN && w.rad.size() == (size_t)EN &&
          w.pri.size() == (size_t)EN && w.p95.size() == (size_t)MP, "sizes");
  for (int g = 0; g < EN; ++g) {
    for (int k = 0; k < MP; ++k)
      for (int c = 0; c < 3; ++c) {
        const int kk = k < np[g] ? k : np[g] - 1;  // rows beyond n_points repeat the destination
        REQUIRE(w.wp[((size_t)k * 3 + c) * EN + g] == wpts[((size_t)g * MP + kk) * 3 + c], "wp[%d][%d] of drone %d", k, c, g);
      }
    REQUIRE(w.rad[g] == 0.2 && w.pri[g] == 5.0, "defaults");
    if (np[g] == 2) {
      const double* s = &wpts[(size_t)g * MP * 3];
      const double want = std::sqrt(std::pow(s[3] - s[0], 2.0) + std::pow(s[4] - s[1], 2.0) + std::pow(s[5] - s[2], 2.0));
      REQUIRE(w.rl[g] == want, "route length of drone %d: %a vs %a", g, w.rl[g], want);
    }
    double poly = 0.0;
    for (int k = 0; k + 1 < np[g]; ++k) {
      const double* s = &wpts[((size_t)g * MP + k) * 3];
      poly += std::hypot(std::hypot(s[3] - s[0], s[4] - s[1]), s[5] - s[2]);
    }
    REQUIRE(std::fabs(w.rl[g] - poly) <= 1e-12 * poly, "route length of drone %d", g);
  }
  for (int k = 0; k < MP; ++k) REQUIRE(std::fabs(w.p95[k] - std::exp(k * std::log(0.95))) < 1e-15, "0.95 ** %d", k);
  REQUIRE(P.uniform_rp == 1 && P.r0 == 0.2 && P.prio0 == 5.0, "uniform_rp for null arrays");
  std::vector<double> rad(EN, 0.3), pri(EN, 2.0);
  REQUIRE(stage_world(P, wpts.data(), np.data(), rad.data(), pri.data(), w, err) == RVO3D_OK, "%s", err.c_str());
  REQUIRE(P.uniform_rp == 1 && P.r0 == 0.3 && P.prio0 == 2.0, "uniform_rp for equal arrays");
  rad[4] = std::nextafter(0.3, 1.0);
  REQUIRE(stage_world(P, wpts.data(), np.data(), rad.data(), pri.data(), w, err) == RVO3D_OK, "%s", err.c_str());
  REQUIRE(P.uniform_rp == 0 && w.rad[4] == rad[4], "a radius that differs in the last bit");
  rad[4] = 0.3; pri[EN - 1] = std::nextafter(2.0, 3.0);
  REQUIRE(stage_world(P, wpts.data(), np.data(), rad.data(), pri.data(), w, err) == RVO3D_OK, "%s", err.c_str());
  REQUIRE(P.uniform_rp == 0, "a priority that differs in the last bit");
  for (int bad : {1, MP + 1}) {
    std::vector<int32_t> np2 = np;
    np2[3] = bad;
    err.clear();
    REQUIRE(stage_world(P, wpts.data(), np2.data(), nullptr, nullptr, w, err) == RVO3D_ERR_INVALID, "n_points %d accepted", bad);
    REQUIRE(err == "n_points entries must be in [2, max_points]", "message: %s", err.c_str());
  }
}

int main() {
  check_thresholds();
  check_matrix();
  check_building_grid();
  check_stage_world();
  std::printf("host set-up ok: %ld checks\n", g_checks);
  return 0;
}
