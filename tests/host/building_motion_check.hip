// building_motion_check.hip -- stand-alone check of the moving buildings' shared rules (csrc/rvo3d_motion_kernels.hpp:
// motion_move, motion_cell - the text move_buildings_kernel runs) and of the argument checks
// (csrc/rvo3d_host_setup.hpp: check_move_env_buildings).  Calls no HIP function and needs no GPU;
// tests/test_building_motion_host.py builds it with the host sanitizers, runs it and compares the trajectory it prints
// with tests/building_motion_ref.py.  Exit status 0 = every check held.
#include "rvo3d_params.hpp"
#include "rvo3d_lds.hpp"
#include "rvo3d_host_setup.hpp"
#include "rvo3d_motion_kernels.hpp"

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

static uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return u;
}

// One env as move_buildings_kernel walks it: phase 1 over the records, phase 2 over the cells (every record read back
// from the records just written, as the kernel does beyond its LDS cap).
static void advance_env(const Cold& C, double rmax, double dt, double* rec, int nb, const double* ends, const double* speed,
                        uint8_t* leg, uint16_t* grid) {
  for (int b = 0; b < nb; ++b) {
    double* q = rec + 4 * b;
    if (!motion_live(q[2])) continue;
    const MotionStep m = motion_move(q[0], q[1], leg[b], ends + 4 * b, speed[b], dt);
    if (m.moved) { q[0] = m.x; q[1] = m.y; leg[b] = m.leg; }
  }
  for (int c = 0; c < C.bgx * C.bgy; ++c) {
    const int ix = c / C.bgy, iy = c - ix * C.bgy;
    const MotionCell m = motion_cell(ix, iy, C.bgx, C.bgy, C.bg_inv, nb, [&](int b, double& bx, double& by, double& reach) {
      const double* q = rec + 4 * b;
      if (!motion_live(q[2])) return false;
      bx = q[0]; by = q[1];
      reach = motion_reach(rmax, q[3]);
      return true;
    });
    std::memcpy(grid + (size_t)c * (kBgridK + 1), m.w, sizeof m.w);
  }
}

// build_building_grid of the env's live records.  The host path only ever has fillers behind counts[e]; for fillers
// among the live records the list of the live records alone is built and its entries are renamed to the records' own
// indices (the order, by index, and the counts are the same).
static std::vector<uint16_t> host_grid(const Cold& C, const std::vector<double>& rec, int nb, double rmax) {
  std::vector<double> r;
  std::vector<uint16_t> index;
  for (int b = 0; b < nb; ++b)
    if (motion_live(rec[4 * b + 2])) {
      r.insert(r.end(), rec.begin() + 4 * b, rec.begin() + 4 * b + 4);
      index.push_back((uint16_t)b);
    }
  Cold Ce = C;
  Ce.nb = (int)index.size();
  std::vector<uint16_t> g = build_building_grid(Ce, r.data(), std::vector<double>(1, rmax));
  const size_t K1 = kBgridK + 1;
  for (size_t c = 0; c < g.size() / K1; ++c) {
    const int n = g[c * K1] == 0xffff ? kBgridK : g[c * K1];
    for (int k = 1; k <= n; ++k) g[c * K1 + k] = index[g[c * K1 + k]];
  }
  return g;
}

// a. after random moves the lists equal build_building_grid's, u16 for u16
static void check_lists(uint64_t seed, const double* map, int want_gx, int want_gy, bool fillers_between) {
  Rng r(seed);
  rvo3d_config c{};
  c.num_envs = 1; c.num_drones = 4; c.max_points = 2; c.neighbors_num = 3; c.env_train = 1; c.action_decimals = -1;
  for (int k = 0; k < 3; ++k) c.map_size[k] = map[k];
  Cold C{};
  env_grid_dims(&c, 1, kEnvGridBudget, C);
  REQUIRE(C.bgx == want_gx && C.bgy == want_gy, "grid %d x %d", C.bgx, C.bgy);
  const int nb = 40, n_live = 34;
  const double rmax = 0.6, dt = 1.0;
  std::vector<double> bld((size_t)nb * 4), ends((size_t)nb * 4), speed(nb);
  std::vector<uint8_t> leg(nb, 1);
  const double cx = 0.5 * map[0], cy = 0.5 * map[1];
  for (int b = 0; b < nb; ++b) {
    double* q = &bld[4 * b];
    const bool cluster = b < 20;  // 20 records start inside one cell: it overflows, and stops once they have left
    q[0] = cluster ? cx + r.uni(-1.5, 1.5) : r.uni(-1.0, map[0] + 1.0);
    q[1] = cluster ? cy + r.uni(-1.5, 1.5) : r.uni(-1.0, map[1] + 1.0);
    q[2] = r.uni(0.5, map[2]);
    q[3] = r.below(5) == 0 ? r.uni(4.0, 7.0) : r.uni(0.05, 1.5);
    ends[4 * b] = q[0]; ends[4 * b + 1] = q[1];
    ends[4 * b + 2] = r.uni(-3.0, map[0] + 3.0); ends[4 * b + 3] = r.uni(-3.0, map[1] + 3.0);  // (a building may leave the map)
    speed[b] = b % 7 == 6 ? 0.0 : r.uni(0.3, 1.5);
  }
  // fillers: behind n_live as stage_env_buildings leaves them, or - fillers_between - scattered among the live records
  for (int b = 0; b < nb; ++b)
    if (fillers_between ? (b % 6 == 3) : (b >= n_live)) { bld[4 * b] = bld[4 * b + 1] = bld[4 * b + 3] = 0.0; bld[4 * b + 2] = -INFINITY; }
  if (!fillers_between) {  // the start is what the host call stages
    std::vector<int32_t> cnt(1, n_live);
    StagedEnvBuildings w;
    Cold Cn = C;
    Cn.nb = nb;
    stage_env_buildings(Cn, 1, bld.data(), cnt.data(), nb, rmax, w);
    REQUIRE(std::memcmp(w.bld.data(), bld.data(), bld.size() * 8) == 0, "the staged records");
    REQUIRE(w.grid == host_grid(C, bld, nb, rmax), "host_grid is the staged grid");
  }
  const size_t cells = (size_t)C.bgx * C.bgy, K1 = kBgridK + 1;
  std::vector<uint16_t> grid(cells * K1, 0xabcd);
  const std::vector<double> start = bld;
  std::vector<int> was_over(cells, 0);
  long over = 0, stopped = 0, began = 0, flips = 0, listed = 0;
  for (int t = 0; t < 40; ++t) {
    const std::vector<uint8_t> leg0 = leg;
    advance_env(C, rmax, dt, bld.data(), nb, ends.data(), speed.data(), leg.data(), grid.data());
    const std::vector<uint16_t> want = host_grid(C, bld, nb, rmax);
    REQUIRE(want.size() == grid.size(), "sizes");
    for (size_t i = 0; i < want.size(); ++i)
      REQUIRE(want[i] == grid[i], "seed %llu step %d: cell %zu entry %zu: %u, build_building_grid has %u",
              (unsigned long long)seed, t, i / K1, i % K1, (unsigned)grid[i], (unsigned)want[i]);
    for (size_t cidx = 0; cidx < cells; ++cidx) {
      const int cnt = grid[cidx * K1];
      const int now = cnt == 0xffff;
      over += now; stopped += was_over[cidx] && !now; began += !was_over[cidx] && now && t > 0;
      if (!now) listed += cnt;
      was_over[cidx] = now;
    }
    for (int b = 0; b < nb; ++b) {
      flips += leg[b] != leg0[b];
      const double* q = &bld[4 * b];
      REQUIRE(bits(q[2]) == bits(start[4 * b + 2]) && bits(q[3]) == bits(start[4 * b + 3]), "h and r never change");
      if (!motion_live(q[2]) || speed[b] == 0.0)
        REQUIRE(bits(q[0]) == bits(start[4 * b]) && bits(q[1]) == bits(start[4 * b + 1]) && leg[b] == 1, "record %d stays", b);
    }
  }
  std::printf("lists seed %llu grid %d x %d fillers %s: %ld overflowing cell-steps, %ld stopped, %ld began, %ld flips, %ld entries\n",
              (unsigned long long)seed, C.bgx, C.bgy, fillers_between ? "between" : "behind", over, stopped, began, flips, listed);
  REQUIRE(over > 0, "no cell overflowed");
  REQUIRE(flips > 0, "no building reached an endpoint");
  if (cells > 1) REQUIRE(stopped > 0 && listed > 0, "no cell stopped overflowing");
}

// b. arrival: exactly the endpoint, leg flips, the rest of the step is not spent
static void check_arrival() {
  const double ends[4] = {0.0, 0.0, 3.0, 4.0};
  MotionStep m = motion_move(0.0, 0.0, 1, ends, 3.0, 1.0);
  REQUIRE(m.moved && m.leg == 1 && m.x == 0.0 + (3.0 / 5.0) * 3.0 && m.y == 0.0 + (4.0 / 5.0) * 3.0, "first step (%a, %a)", m.x, m.y);
  m = motion_move(m.x, m.y, m.leg, ends, 3.0, 1.0);  // 2 m to go, 3 m of step
  REQUIRE(m.moved && bits(m.x) == bits(3.0) && bits(m.y) == bits(4.0) && m.leg == 0, "arrival (%a, %a) leg %d", m.x, m.y, m.leg);
  m = motion_move(m.x, m.y, m.leg, ends, 3.0, 1.0);  // back towards endpoint 0
  REQUIRE(m.moved && m.leg == 0 && m.x < 3.0 && m.y < 4.0, "the way back");
  m = motion_move(m.x, m.y, m.leg, ends, 3.0, 1.0);
  REQUIRE(bits(m.x) == bits(0.0) && bits(m.y) == bits(0.0) && m.leg == 1, "endpoint 0 (%a, %a)", m.x, m.y);
  // d == step arrives; on the endpoint already (d == 0): stays there, flips
  m = motion_move(0.0, 0.0, 1, ends, 5.0, 1.0);
  REQUIRE(bits(m.x) == bits(3.0) && bits(m.y) == bits(4.0) && m.leg == 0, "d == step");
  m = motion_move(3.0, 4.0, 1, ends, 0.5, 1.0);
  REQUIRE(m.moved && bits(m.x) == bits(3.0) && bits(m.y) == bits(4.0) && m.leg == 0, "d == 0");
  // other values of leg count as their low bit
  m = motion_move(0.0, 0.0, 3, ends, 5.0, 1.0);
  REQUIRE(bits(m.x) == bits(3.0) && m.leg == 2, "leg 3 is endpoint 1");
  m = motion_move(1.0, 0.0, 2, ends, 5.0, 1.0);
  REQUIRE(bits(m.x) == bits(0.0) && m.leg == 3, "leg 2 is endpoint 0");
}

// c. a static building keeps its bits
static void check_static() {
  const double ends[4] = {NAN, NAN, NAN, NAN};  // not read
  uint64_t payload = 0x7ff8000000abcdefull;
  double odd;
  std::memcpy(&odd, &payload, 8);
  const double xs[4] = {-0.0, 1.0 / 3.0, odd, 1e-310};
  const double speeds[5] = {0.0, -0.0, NAN, -1.0, 2.0};
  for (double x : xs)
    for (int i = 0; i < 5; ++i) {
      const double dt = i == 4 ? 0.0 : 1.0;  // (a positive speed with dt 0 stays as well)
      for (uint8_t leg : {(uint8_t)0, (uint8_t)1, (uint8_t)7}) {
        const MotionStep m = motion_move(x, -x, leg, ends, speeds[i], dt);
        REQUIRE(!m.moved && bits(m.x) == bits(x) && bits(m.y) == bits(-x) && m.leg == leg, "static: speed %g dt %g", speeds[i], dt);
      }
    }
  REQUIRE(!motion_live(-INFINITY) && motion_live(0.0) && motion_live(INFINITY) && motion_live(NAN) && motion_live(-1e308), "fillers");
  REQUIRE(motion_reach(0.2, NAN) == 5.0 + 1e-3 && motion_reach(INFINITY, 1.0) == 5.0 + 1e-3 && motion_reach(0.2, 1.0) == (0.2 + 1.0) + 1e-3,
          "reach");
}

// d. the argument checks
static void check_arguments() {
  double d = 0;
  uint8_t u = 0;
  const rvo3d_building_motion ok{&d, &d, &u};
  std::string err;
  REQUIRE(check_move_env_buildings(true, true, &ok, 1.0, err) == RVO3D_OK, "accepted");
  REQUIRE(check_move_env_buildings(true, true, &ok, 0.0, err) == RVO3D_OK, "dt 0");
  REQUIRE(check_move_env_buildings(false, false, &ok, 1.0, err) == RVO3D_ERR_STATE && err.find("rvo3d_load_world") != std::string::npos,
          "no world: %s", err.c_str());
  REQUIRE(check_move_env_buildings(true, false, &ok, 1.0, err) == RVO3D_ERR_STATE && err.find("rvo3d_set_env_buildings") != std::string::npos,
          "no sets: %s", err.c_str());
  REQUIRE(check_move_env_buildings(true, true, nullptr, 1.0, err) == RVO3D_ERR_INVALID && err.find("rvo3d_building_motion") != std::string::npos,
          "null struct: %s", err.c_str());
  const rvo3d_building_motion bad[3] = {{nullptr, &d, &u}, {&d, nullptr, &u}, {&d, &d, nullptr}};
  for (const auto& b : bad)
    REQUIRE(check_move_env_buildings(true, true, &b, 1.0, err) == RVO3D_ERR_INVALID && err.find("required") != std::string::npos,
            "null member: %s", err.c_str());
  for (double dt : {-1.0, -1e-300, (double)NAN, (double)INFINITY, (double)-INFINITY})
    REQUIRE(check_move_env_buildings(true, true, &ok, dt, err) == RVO3D_ERR_INVALID && err.find("dt") != std::string::npos,
            "dt %g: %s", dt, err.c_str());
  // the state comes first: a handle without sets reports that, whatever else is wrong
  REQUIRE(check_move_env_buildings(true, false, nullptr, NAN, err) == RVO3D_ERR_STATE, "state before arguments");
}

// e. a small trajectory for tests/building_motion_ref.py: the inputs and every step's records, as bit patterns
static void print_trajectory() {
  Rng r(2024);
  const int nb = 12, T = 30;
  std::vector<double> bld((size_t)nb * 4), ends((size_t)nb * 4), speed(nb);
  std::vector<uint8_t> leg(nb);
  for (int b = 0; b < nb; ++b) {
    bld[4 * b] = r.uni(0, 24); bld[4 * b + 1] = r.uni(0, 24); bld[4 * b + 2] = b == 5 ? -INFINITY : r.uni(1, 8); bld[4 * b + 3] = r.uni(0.1, 1.5);
    ends[4 * b] = bld[4 * b]; ends[4 * b + 1] = bld[4 * b + 1];
    ends[4 * b + 2] = bld[4 * b] + r.uni(-6, 6); ends[4 * b + 3] = bld[4 * b + 1] + r.uni(-6, 6);
    speed[b] = b == 2 ? 0.0 : (b == 7 ? NAN : r.uni(0.3, 1.5));
    leg[b] = (uint8_t)(b == 9 ? 0 : 1);
  }
  const double dt = 0.7;
  std::printf("traj_dt %016llx\n", (unsigned long long)bits(dt));
  for (int b = 0; b < nb; ++b) {
    std::printf("traj_in %d %d", b, (int)leg[b]);
    for (int k = 0; k < 4; ++k) std::printf(" %016llx", (unsigned long long)bits(bld[4 * b + k]));
    for (int k = 0; k < 4; ++k) std::printf(" %016llx", (unsigned long long)bits(ends[4 * b + k]));
    std::printf(" %016llx\n", (unsigned long long)bits(speed[b]));
  }
  for (int t = 0; t < T; ++t)
    for (int b = 0; b < nb; ++b) {
      double* q = &bld[4 * b];
      if (motion_live(q[2])) {
        const MotionStep m = motion_move(q[0], q[1], leg[b], &ends[4 * b], speed[b], dt);
        if (m.moved) { q[0] = m.x; q[1] = m.y; leg[b] = m.leg; }
      }
      std::printf("traj %d %d %d %016llx %016llx\n", t, b, (int)leg[b], (unsigned long long)bits(q[0]), (unsigned long long)bits(q[1]));
    }
}

int main() {
  const double m3[3] = {24, 24, 8}, m1[3] = {6, 7, 8};
  check_lists(1, m3, 3, 3, false);
  check_lists(2, m3, 3, 3, true);
  check_lists(3, m1, 1, 1, false);
  check_lists(4, m1, 1, 1, true);
  check_arrival();
  check_static();
  check_arguments();
  print_trajectory();
  std::printf("building motion ok: %ld checks\n", g_checks);
  return 0;
}
