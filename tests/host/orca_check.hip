// orca_check.hip -- stand-alone CPU program over the rules of rvo3d_orca_vel and rvo3d_vel_command
// (csrc/rvo3d_orca_rules.hpp: orca_plane, orca_slots_*, orca_lp1..4, orca_solve, vel_command, orca_check;
// csrc/rvo3d_building_kernels.hpp: building_pair; csrc/rvo3d_motion_kernels.hpp: motion_velocity).  Calls no HIP function
// and needs no GPU.
//   orca_check IN OUT
// IN:  int32 n, nb, has_motion, max_neighbors, max_buildings; double time_horizon, time_step, max_speed, pref_speed,
//      neighbor_dist, reach, below, clear_xy, dt; n x 10 doubles (px py pz vx vy vz r des[3]); nb x (x y h r) doubles; with
//      has_motion: nb x (e0x e0y e1x e1y) doubles, nb speeds (double), nb legs (bytes).
// OUT: n x 3 int32 (n_neighbors, n_buildings, status); n x 4 doubles (slack, v[3]); n x 24 x 6 doubles (the planes in rule
//      5's order: point, normal; zeros behind the last) - what tests/test_orca_host.py compares with tests/orca_ref.py, bit
//      for bit.
// Without arguments it runs its own table of the argument checks and hand-computed cases.  Exit status 0 = all held.
#include "rvo3d_building_kernels.hpp"
#include "rvo3d_orca_rules.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

struct ArrayStore {
  OrcaPlane* p;
  OrcaPlane get(int s) const { return p[s]; }
  void put(int s, const OrcaPlane& q) const { p[s] = q; }
};

static double g_ends[4], g_speed[1], g_out[3];
static uint8_t g_leg[1];
static const rvo3d_building_motion g_motion{g_ends, g_speed, g_leg};

static int rc_of(const rvo3d_orca_args& a, const rvo3d_building_motion* m = &g_motion, double dt = 1.0, bool attached = true) {
  const char* why = nullptr;
  const int rc = orca_check(&a, attached, m, dt, &why);
  REQUIRE(why != nullptr && ((rc == RVO3D_OK) == (why[0] == 0)), "status %d with reason '%s'", rc, why ? why : "(null)");
  return rc;
}

static int self_test() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // ---- the argument checks ----
  rvo3d_orca_args ok{};
  ok.time_horizon = 5.0; ok.time_step = 1.0; ok.max_speed = 2.0; ok.pref_speed = 1.0; ok.neighbor_dist = 10.0;
  ok.max_neighbors = 10; ok.max_buildings = 4; ok.reach = 10.0; ok.below = 1.0; ok.clear_xy = 0.0; ok.out_vel = g_out;
  REQUIRE(rc_of(ok) == RVO3D_OK, "the plain call");
  const char* why = nullptr;
  REQUIRE(orca_check(nullptr, true, &g_motion, 1.0, &why) == RVO3D_ERR_INVALID, "null args");
  { auto a = ok; a.out_vel = nullptr; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "null out_vel"); }
  for (double v : {0.0, -1.0, nan, inf, -inf}) {
    { auto a = ok; a.time_horizon = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "time_horizon %g", v); }
    { auto a = ok; a.time_step = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "time_step %g", v); }
    { auto a = ok; a.neighbor_dist = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "neighbor_dist %g", v); }
    { auto a = ok; a.reach = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "reach %g", v); }
  }
  for (double v : {-1e-300, -1.0, nan, inf}) {
    { auto a = ok; a.max_speed = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "max_speed %g", v); }
    { auto a = ok; a.pref_speed = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "pref_speed %g", v); }
    { auto a = ok; a.below = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "below %g", v); }
    { auto a = ok; a.clear_xy = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "clear_xy %g", v); }
  }
  { auto a = ok; a.max_speed = 0.0; a.pref_speed = 0.0; a.below = 0.0; a.time_horizon = 1e-300; REQUIRE(rc_of(a) == RVO3D_OK, "the edges"); }
  for (int v : {0, -1, 17, 1 << 30}) { auto a = ok; a.max_neighbors = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "max_neighbors %d", v); }
  for (int v : {-1, 9, 1 << 30}) { auto a = ok; a.max_buildings = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "max_buildings %d", v); }
  for (int v : {1, 16}) { auto a = ok; a.max_neighbors = v; REQUIRE(rc_of(a) == RVO3D_OK, "max_neighbors %d", v); }
  for (int v : {0, 8}) { auto a = ok; a.max_buildings = v; REQUIRE(rc_of(a) == RVO3D_OK, "max_buildings %d", v); }
  REQUIRE(rc_of(ok, nullptr, 1.0, false) == RVO3D_OK, "no motion on a handle without sets");
  REQUIRE(rc_of(ok, nullptr, 0.0, true) == RVO3D_OK, "no motion, dt 0");
  REQUIRE(rc_of(ok, &g_motion, 1.0, false) == RVO3D_ERR_STATE, "a motion without attached sets");
  { rvo3d_building_motion m = g_motion; m.ends = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null ends"); }
  { rvo3d_building_motion m = g_motion; m.speed = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null speed"); }
  { rvo3d_building_motion m = g_motion; m.leg = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null leg"); }
  for (double dt : {-1.0, -1e-300, inf, -inf, nan}) REQUIRE(rc_of(ok, &g_motion, dt) == RVO3D_ERR_INVALID, "dt %g", dt);
  for (double dt : {-1.0, inf, nan}) REQUIRE(rc_of(ok, nullptr, dt) == RVO3D_ERR_INVALID, "dt %g without a motion", dt);
  { auto a = ok; a.reach = nan; REQUIRE(rc_of(a, &g_motion, 1.0, false) == RVO3D_ERR_INVALID, "the parameters before the motion"); }

  // ---- rule 4 on hand-computed pairs: j 4 m ahead on x, R = 1, tau = 2 ----
  {
    int br = -1;
    const OrcaV3 rel = orca_v3(4.0, 0.0, 0.0), vi = orca_v3(1.0, 0.0, 0.0);
    // head-on, closing at 2: w = (2, 0, 0) - (2, 0, 0) = 0 -> not dp < 0: a leg with a zero cross product
    OrcaPlane p = orca_plane(rel, orca_v3(2.0, 0.0, 0.0), 1.0, 2.0, 1.0, 0.5, vi, &br);
    REQUIRE(br == 1, "closing at rel / tau is on the legs' side: %d", br);
    // ... and on the cone's axis (ww = 0): the normal towards z x rel = +y, tilted back by alpha, sin(alpha) = R / |rel|
    REQUIRE(p.normal.x == -0.25 && std::fabs(p.normal.y - std::sqrt(15.0) / 4.0) < 1e-15 && p.normal.z == 0.0,
            "on the axis: %a %a %a", p.normal.x, p.normal.y, p.normal.z);
    {
      const OrcaPlane o = orca_plane(orca_v3(-4.0, 0.0, 0.0), orca_v3(-2.0, 0.0, 0.0), 1.0, 2.0, 1.0, 0.5, vi, &br);
      REQUIRE(o.normal.x == -p.normal.x && o.normal.y == -p.normal.y, "the other drone takes the opposite normal");
    }
    // receding at 1: w = (-3, 0, 0), dp = -12 < 0, dp^2 = 144 > 9: the cut-off circle, n = (-1, 0, 0), u = (0.5 - 3) n
    p = orca_plane(rel, orca_v3(-1.0, 0.0, 0.0), 1.0, 2.0, 1.0, 0.5, vi, &br);
    REQUIRE(br == 0 && p.normal.x == -1.0 && p.normal.y == 0.0 && p.point.x == 1.0 + 0.5 * 2.5, "cut-off: %a %a", p.normal.x, p.point.x);
    // overlapping: rel 0.5, w_rel 0: w = (-0.5, 0, 0), n = (-1, 0, 0), u = (1 - 0.5) n; a building takes it all
    p = orca_plane(orca_v3(0.5, 0.0, 0.0), orca_v3(0.0, 0.0, 0.0), 1.0, 2.0, 1.0, 1.0, vi, &br);
    REQUIRE(br == 2 && p.normal.x == -1.0 && p.point.x == 0.5, "overlap: %a %a", p.normal.x, p.point.x);
    // a zero-length w: the same place, the same velocity
    p = orca_plane(orca_v3(0.0, 0.0, 0.0), orca_v3(0.0, 0.0, 0.0), 1.0, 2.0, 1.0, 0.5, vi, &br);
    REQUIRE(br == 2 && p.normal.x == 1.0 && p.normal.y == 0.0 && p.normal.z == 0.0 && p.point.x == 1.5, "zero w: %a", p.point.x);
    // a planar pair stays planar
    p = orca_plane(orca_v3(3.0, 1.0, 0.0), orca_v3(1.0, 0.2, 0.0), 1.0, 2.0, 1.0, 1.0, orca_v3(1.0, 0.2, 0.7), &br);
    REQUIRE(p.normal.z == 0.0 && p.point.z == 0.7, "planar: %a %a", p.normal.z, p.point.z);
  }
  // ---- the slots: ascending (key, index), ties to the lower index ----
  {
    OrcaSlots<4> s;
    orca_slots_clear(s);
    const double keys[7] = {3.0, 1.0, 2.0, 1.0, 5.0, 0.5, 2.0};
    for (int i = 0; i < 7; ++i) orca_slots_insert(s, keys[i], i);
    REQUIRE(s.seen == 7 && s.idx[0] == 5 && s.idx[1] == 1 && s.idx[2] == 3 && s.idx[3] == 2, "slots %d %d %d %d", s.idx[0], s.idx[1], s.idx[2], s.idx[3]);
    REQUIRE(orca_slots_index(s, 2) == 3 && orca_slots_index(s, 7) == -1, "select chain");
  }
  // ---- the programs on cases with known answers ----
  {
    OrcaPlane pl[kOrcaMaxPlanes], pj[kOrcaMaxPlanes];
    ArrayStore S{pl}, J{pj};
    const OrcaV3 pref = orca_v3(1.0, 0.0, 0.0);
    OrcaResult r = orca_solve(S, J, 0, 0, 2.0, orca_v3(3.0, 0.0, 0.0));
    REQUIRE(r.status == 1 && r.v.x == 2.0 && r.v.y == 0.0, "no planes: pref clipped");
    pl[0] = OrcaPlane{{0.0, 0.0, 0.0}, {-1.0, 0.0, 0.0}};  // v_x <= 0
    r = orca_solve(S, J, 1, 0, 2.0, pref);
    REQUIRE(r.status == 2 && r.v.x == 0.0 && r.v.y == 0.0 && r.v.z == 0.0 && r.slack == 0.0, "one plane: the projection");
    pl[1] = OrcaPlane{{0.0, 0.5, 0.0}, {0.0, 1.0, 0.0}};   // v_y >= 0.5
    r = orca_solve(S, J, 2, 0, 2.0, pref);
    REQUIRE(r.status == 2 && r.v.x == 0.0 && r.v.y == 0.5 && r.v.z == 0.0, "two planes: on their line (%a %a %a)", r.v.x, r.v.y, r.v.z);
    pl[1] = OrcaPlane{{1.0, 0.0, 0.0}, {1.0, 0.0, 0.0}};   // v_x >= 1: no common point, the best is half way
    r = orca_solve(S, J, 2, 0, 2.0, pref);
    REQUIRE(r.status == 3 && std::fabs(r.v.x - 0.5) < 1e-12 && std::fabs(r.slack - 0.5) < 1e-12, "fallback: %a slack %a", r.v.x, r.slack);
    r = orca_solve(S, J, 2, 1, 2.0, pref);                 // ... with the first one a building's: it holds
    REQUIRE(r.status == 3 && r.v.x <= 1e-12 && std::fabs(r.slack - 1.0) < 1e-12, "hard plane: %a slack %a", r.v.x, r.slack);
    r = orca_solve(S, J, 1, 0, 0.0, pref);
    REQUIRE(r.v.x == 0.0 && r.v.y == 0.0 && r.v.z == 0.0, "max_speed 0");
  }
  // ---- the converter ----
  {
    double a[3];
    unsigned bits = vel_command(1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, a);
    REQUIRE(bits == 0u && std::fabs(a[0] - (std::sqrt(2.0) - 1.0)) < 1e-15 && std::fabs(a[1] - 0.5) < 1e-14 && a[2] == 0.0,
            "a left turn: %a %a %a", a[0], a[1], a[2]);
    bits = vel_command(1.0, 0.0, 0.0, 350.0, 0.0, 1.0, 0.0, 0.0, a);
    REQUIRE(bits == 0u && a[0] == 0.0 && std::fabs(a[1] - 10.0 / 90.0) < 1e-14, "across 360: %a", a[1]);
    bits = vel_command(1.0, 0.0, 0.0, 0.0, 0.0, -3.0, -0.3, 0.0, a);
    REQUIRE(bits == 3u && a[0] == 1.0 && a[1] == -1.0, "speed and yaw clipped: %u %a %a", bits, a[0], a[1]);
    bits = vel_command(0.0, 2.0, 0.0, 90.0, 30.0, 0.0, 0.0, 0.0, a);
    REQUIRE(bits == 1u && a[0] == -1.0 && a[1] == 0.0 && a[2] == 0.0, "a stop keeps the angles");
    bits = vel_command(0.0, 0.0, 0.0, 0.0, -80.0, 0.0, 0.0, 0.5, a);
    REQUIRE(bits == 4u && a[2] == 1.0, "pitch clipped");
  }
  std::printf("orca ok: %ld checks\n", g_checks);
  return 0;
}

template <class T>
static void read_n(std::FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}

int main(int argc, char** argv) {
  if (argc == 1) return self_test();
  if (argc != 3) { std::fprintf(stderr, "usage: %s [IN OUT]\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int32_t hdr[5];
  double par[9];
  read_n(f, hdr, 5); read_n(f, par, 9);
  const int n = hdr[0], nb = hdr[1], max_nbr = hdr[3], max_bld = hdr[4];
  const bool has_motion = hdr[2] != 0;
  if (n < 0 || nb < 0 || max_nbr < 1 || max_nbr > kOrcaMaxNeighbors || max_bld < 0 || max_bld > kOrcaMaxBuildings) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  const double tau = par[0], time_step = par[1], max_speed = par[2], pref_speed = par[3], nd = par[4], reach = par[5],
               below = par[6], clear_xy = par[7], dt = par[8];
  std::vector<double> dr((size_t)n * 10), bl((size_t)nb * 4), ends, speed;
  std::vector<uint8_t> leg;
  read_n(f, dr.data(), dr.size()); read_n(f, bl.data(), bl.size());
  if (has_motion) {
    ends.resize((size_t)nb * 4); speed.resize((size_t)nb); leg.resize((size_t)nb);
    read_n(f, ends.data(), ends.size()); read_n(f, speed.data(), speed.size()); read_n(f, leg.data(), leg.size());
  }
  std::fclose(f);

  std::vector<int32_t> ints((size_t)n * 3, 0);
  std::vector<double> vals((size_t)n * 4, 0.0), planes_out((size_t)n * kOrcaMaxPlanes * 6, 0.0);
  const double nd2 = nd * nd;
  for (int i = 0; i < n; ++i) {
    const double* d = &dr[(size_t)i * 10];
    OrcaSlots<kOrcaMaxNeighbors> nbr;
    orca_slots_clear(nbr);
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double* o = &dr[(size_t)j * 10];
      const double rx = o[0] - d[0], ry = o[1] - d[1], rz = o[2] - d[2];
      const double d2 = (rx * rx + ry * ry) + rz * rz;
      if (d2 < nd2) orca_slots_insert(nbr, d2, j);
    }
    OrcaSlots<kOrcaMaxBuildings> bs;
    orca_slots_clear(bs);
    for (int j = 0; j < nb; ++j) {
      const double* b = &bl[(size_t)j * 4];
      const BuildingPair q = building_pair(d[0], d[1], d[2], d[6], b[0], b[1], b[2], b[3], reach, below);
      if (q.pass) orca_slots_insert(bs, q.gap, j);
    }
    const int kb = bs.seen < max_bld ? bs.seen : max_bld, kn = nbr.seen < max_nbr ? nbr.seen : max_nbr;
    OrcaPlane pl[kOrcaMaxPlanes], pj[kOrcaMaxPlanes];
    ArrayStore S{pl}, J{pj};
    const OrcaV3 vi = orca_v3(d[3], d[4], d[5]);
    int br;
    for (int k = 0; k < kb; ++k) {
      const int j = orca_slots_index(bs, k);
      const double* b = &bl[(size_t)j * 4];
      MotionVel vb{0.0, 0.0};
      if (has_motion) vb = motion_velocity(b[0], b[1], leg[(size_t)j], &ends[(size_t)j * 4], speed[(size_t)j], dt);
      S.put(k, orca_plane(orca_v3(b[0] - d[0], b[1] - d[1], 0.0), orca_v3(d[3] - vb.x, d[4] - vb.y, 0.0),
                          (d[6] + b[3]) + clear_xy, tau, time_step, 1.0, vi, &br));
    }
    for (int k = 0; k < kn; ++k) {
      const int j = orca_slots_index(nbr, k);
      const double* o = &dr[(size_t)j * 10];
      S.put(kb + k, orca_plane(orca_v3(o[0] - d[0], o[1] - d[1], o[2] - d[2]), orca_v3(d[3] - o[3], d[4] - o[4], d[5] - o[5]),
                               d[6] + o[6], tau, time_step, 0.5, vi, &br));
    }
    const OrcaV3 pref = orca_v3(pref_speed * d[7], pref_speed * d[8], pref_speed * d[9]);
    const OrcaResult r = orca_solve(S, J, kb + kn, kb, max_speed, pref);
    ints[(size_t)i * 3] = kn; ints[(size_t)i * 3 + 1] = kb; ints[(size_t)i * 3 + 2] = r.status;
    double* v = &vals[(size_t)i * 4];
    v[0] = r.slack; v[1] = r.v.x; v[2] = r.v.y; v[3] = r.v.z;
    for (int k = 0; k < kb + kn; ++k) {
      double* o = &planes_out[((size_t)i * kOrcaMaxPlanes + k) * 6];
      o[0] = pl[k].point.x; o[1] = pl[k].point.y; o[2] = pl[k].point.z;
      o[3] = pl[k].normal.x; o[4] = pl[k].normal.y; o[5] = pl[k].normal.z;
    }
  }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  std::fwrite(ints.data(), 4, ints.size(), f);
  std::fwrite(vals.data(), 8, vals.size(), f);
  std::fwrite(planes_out.data(), 8, planes_out.size(), f);
  std::fclose(f);
  return 0;
}
