// shield_check.hip -- stand-alone CPU program over the rules of rvo3d_shield_action (csrc/rvo3d_shield_rules.hpp:
// shield_pref, shield_judged, shield_finish, shield_check; csrc/rvo3d_orca_rules.hpp: orca_plane, orca_slots_*, orca_solve,
// vel_command; csrc/rvo3d_building_kernels.hpp: building_pair; csrc/rvo3d_motion_kernels.hpp: motion_velocity).  Calls no
// HIP function and needs no GPU.
//   shield_check IN OUT
// IN:  int32 n, n_live, nb, has_motion, max_neighbors, max_buildings; double time_horizon, time_step, max_speed,
//      neighbor_dist, reach, below, clear_xy, dt; n x 13 doubles (px py pz vx vy vz r yaw pitch dest a[3]; dest 0 or 1);
//      nb x (x y h r) doubles; with has_motion: nb x (e0x e0y e1x e1y) doubles, nb speeds (double), nb legs (bytes).
//      Rows from n_live on are ghosts.
// OUT: n x 2 int32 (status, flags); n x 10 doubles (slack, v[3], pref[3], out_action[3]); n x 24 x 6 doubles (the planes,
//      zeros behind the last and for rows that are not judged); 4 int64 totals - what tests/test_shield_host.py compares
//      with tests/shield_ref.py.
// Without arguments it runs its own table of the argument checks and hand-computed cases.  Exit status 0 = all held.
#include "rvo3d_building_kernels.hpp"
#include "rvo3d_shield_rules.hpp"

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

static double g_ends[4], g_speed[1], g_act[3], g_out[3];
static uint8_t g_leg[1];
static const rvo3d_building_motion g_motion{g_ends, g_speed, g_leg};

static int rc_of(const rvo3d_shield_args& a, const rvo3d_building_motion* m = &g_motion, double dt = 1.0, bool attached = true) {
  const char* why = nullptr;
  const int rc = shield_check(&a, attached, m, dt, &why);
  REQUIRE(why != nullptr && ((rc == RVO3D_OK) == (why[0] == 0)), "status %d with reason '%s'", rc, why ? why : "(null)");
  return rc;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int self_test() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // ---- the argument checks ----
  rvo3d_shield_args ok{};
  ok.time_horizon = 5.0; ok.time_step = 1.0; ok.max_speed = 2.0; ok.neighbor_dist = 10.0;
  ok.max_neighbors = 10; ok.max_buildings = 4; ok.reach = 10.0; ok.below = 1.0; ok.clear_xy = 0.0;
  ok.action = g_act; ok.out_action = g_out;
  REQUIRE(rc_of(ok) == RVO3D_OK, "the plain call");
  { auto a = ok; a.out_action = g_act; REQUIRE(rc_of(a) == RVO3D_OK, "in place"); }
  const char* why = nullptr;
  REQUIRE(shield_check(nullptr, true, &g_motion, 1.0, &why) == RVO3D_ERR_INVALID, "null args");
  { auto a = ok; a.action = nullptr; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "null action"); }
  { auto a = ok; a.out_action = nullptr; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "null out_action"); }
  for (double v : {0.0, -1.0, nan, inf, -inf}) {
    { auto a = ok; a.time_horizon = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "time_horizon %g", v); }
    { auto a = ok; a.time_step = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "time_step %g", v); }
    { auto a = ok; a.neighbor_dist = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "neighbor_dist %g", v); }
    { auto a = ok; a.reach = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "reach %g", v); }
  }
  for (double v : {-1e-300, -1.0, nan, inf}) {
    { auto a = ok; a.max_speed = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "max_speed %g", v); }
    { auto a = ok; a.below = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "below %g", v); }
    { auto a = ok; a.clear_xy = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "clear_xy %g", v); }
  }
  { auto a = ok; a.max_speed = 0.0; a.below = 0.0; a.time_horizon = 1e-300; REQUIRE(rc_of(a) == RVO3D_OK, "the edges"); }
  for (int v : {0, -1, 17, 1 << 30}) { auto a = ok; a.max_neighbors = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "max_neighbors %d", v); }
  for (int v : {-1, 9, 1 << 30}) { auto a = ok; a.max_buildings = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "max_buildings %d", v); }
  for (int v : {1, 16}) { auto a = ok; a.max_neighbors = v; REQUIRE(rc_of(a) == RVO3D_OK, "max_neighbors %d", v); }
  for (int v : {0, 8}) { auto a = ok; a.max_buildings = v; REQUIRE(rc_of(a) == RVO3D_OK, "max_buildings %d", v); }
  REQUIRE(rc_of(ok, nullptr, 1.0, false) == RVO3D_OK, "no motion on a handle without sets");
  REQUIRE(rc_of(ok, &g_motion, 1.0, false) == RVO3D_ERR_STATE, "a motion without attached sets");
  { rvo3d_building_motion m = g_motion; m.ends = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null ends"); }
  { rvo3d_building_motion m = g_motion; m.speed = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null speed"); }
  { rvo3d_building_motion m = g_motion; m.leg = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null leg"); }
  for (double dt : {-1.0, -1e-300, inf, -inf, nan}) REQUIRE(rc_of(ok, &g_motion, dt) == RVO3D_ERR_INVALID, "dt %g", dt);
  for (double dt : {-1.0, inf, nan}) REQUIRE(rc_of(ok, nullptr, dt) == RVO3D_ERR_INVALID, "dt %g without a motion", dt);

  // ---- S1 on hand-computed cases: v = (1, 0, 0), heading (0, 0) ----
  {
    const double a0[3] = {0.0, 0.0, 0.0};
    OrcaV3 p = shield_pref(1.0, 0.0, 0.0, 0.0, 0.0, a0);
    REQUIRE(p.x == 1.0 && p.y == 0.0 && p.z == 0.0, "the action 0 keeps the velocity: %a %a %a", p.x, p.y, p.z);
    const double a1[3] = {5.0, 0.0, 0.0};   // the acceleration clamps at 1
    p = shield_pref(1.0, 0.0, 0.0, 0.0, 0.0, a1);
    REQUIRE(p.x == 2.0 && p.y == 0.0, "clamped acceleration: %a", p.x);
    const double a2[3] = {-3.0, 0.5, 0.5};  // the speed would go negative: 0
    p = shield_pref(0.5, 0.0, 0.0, 0.0, 0.0, a2);
    REQUIRE(p.x == 0.0 && p.y == 0.0 && p.z == 0.0, "a speed below 0: %a %a %a", p.x, p.y, p.z);
    const double a3[3] = {0.0, 0.0, 7.0};   // the pitch step clamps at 90: straight up
    p = shield_pref(1.0, 0.0, 0.0, 0.0, 30.0, a3);
    REQUIRE(std::fabs(p.x) < 1e-15 && p.z == 1.0, "pitch driven to 90: %a %a", p.x, p.z);
    const double a4[3] = {0.0, 1.0, 0.0};   // yaw 350 + 90 wraps to 80
    p = shield_pref(1.0, 0.0, 0.0, 350.0, 0.0, a4);
    REQUIRE(std::fabs(p.x - std::cos(80.0 * kShieldDeg2Rad)) < 1e-15 && std::fabs(p.y - std::sin(80.0 * kShieldDeg2Rad)) < 1e-15,
            "yaw across 360: %a %a", p.x, p.y);
    REQUIRE(shield_mod(440.0, 360.0) == 80.0 && shield_mod(-10.0, 360.0) == 350.0 && shield_mod(360.0, 360.0) == 0.0 &&
            shield_mod(-0.0, 360.0) == 0.0 && !std::signbit(shield_mod(-0.0, 360.0)), "np_mod");
    REQUIRE(shield_norm3(3.0, 4.0, 12.0) == 13.0, "the norm");
  }
  // ---- S5 ----
  {
    const double fin[3] = {0.1, -0.2, 0.3}, bad1[3] = {nan, 0.0, 0.0}, bad2[3] = {0.0, inf, 0.0}, bad3[3] = {0.0, 0.0, -inf};
    REQUIRE(shield_judged(true, false, fin), "a live, moving drone with a finite action");
    REQUIRE(!shield_judged(false, false, fin) && !shield_judged(true, true, fin), "a ghost, a parked drone");
    REQUIRE(!shield_judged(true, false, bad1) && !shield_judged(true, false, bad2) && !shield_judged(true, false, bad3), "non-finite");
  }
  // ---- S4: the identity keeps the bits (a -0 among them); an intervened row is the command ----
  {
    const double a[3] = {-0.0, 1.0 / 3.0, 5.0};
    double out[3] = {9.0, 9.0, 9.0};
    const OrcaV3 pref = orca_v3(1.0, 0.5, 0.0);
    unsigned f = shield_finish(1.0, 0.0, 0.0, 0.0, 0.0, a, pref, pref, out);
    REQUIRE(f == 0u && same_bits(out[0], a[0]) && same_bits(out[1], a[1]) && same_bits(out[2], a[2]), "identity");
    f = shield_finish(1.0, 0.0, 0.0, 0.0, 0.0, a, pref, orca_v3(1.0, 1.0, 0.0), out);
    double cmd[3];
    const unsigned bits = vel_command(1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, cmd);
    REQUIRE(f == (kShieldIntervened | bits) && bits == 0u && out[0] == cmd[0] && out[1] == cmd[1] && out[2] == cmd[2], "the command");
    f = shield_finish(1.0, 0.0, 0.0, 0.0, 0.0, a, pref, orca_v3(-3.0, -0.3, 0.0), out);
    REQUIRE(f == (kShieldIntervened | 3u) && out[0] == 1.0 && out[1] == -1.0, "a clipped command: %u", f);
  }
  std::printf("shield ok: %ld checks\n", g_checks);
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
  int32_t hdr[6];
  double par[8];
  read_n(f, hdr, 6); read_n(f, par, 8);
  const int n = hdr[0], n_live = hdr[1], nb = hdr[2], max_nbr = hdr[4], max_bld = hdr[5];
  const bool has_motion = hdr[3] != 0;
  if (n < 0 || n_live < 0 || n_live > n || nb < 0 || max_nbr < 1 || max_nbr > kOrcaMaxNeighbors || max_bld < 0 ||
      max_bld > kOrcaMaxBuildings) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  const double tau = par[0], time_step = par[1], max_speed = par[2], nd = par[3], reach = par[4], below = par[5],
               clear_xy = par[6], dt = par[7];
  constexpr int W = 13;
  std::vector<double> dr((size_t)n * W), bl((size_t)nb * 4), ends, speed;
  std::vector<uint8_t> leg;
  read_n(f, dr.data(), dr.size()); read_n(f, bl.data(), bl.size());
  if (has_motion) {
    ends.resize((size_t)nb * 4); speed.resize((size_t)nb); leg.resize((size_t)nb);
    read_n(f, ends.data(), ends.size()); read_n(f, speed.data(), speed.size()); read_n(f, leg.data(), leg.size());
  }
  std::fclose(f);

  std::vector<int32_t> ints((size_t)n * 2, 0);
  std::vector<double> vals((size_t)n * 10, 0.0), planes_out((size_t)n * kOrcaMaxPlanes * 6, 0.0);
  long long totals[4] = {0, 0, 0, 0};
  const double nd2 = nd * nd;
  for (int i = 0; i < n; ++i) {
    const double* d = &dr[(size_t)i * W];
    const double* a = d + 10;
    double* val = &vals[(size_t)i * 10];
    const bool live = i < n_live;
    if (!shield_judged(live, d[9] != 0.0, a)) {  // S5
      for (int k = 0; k < 3; ++k) val[7 + k] = live ? a[k] : 0.0;
      continue;
    }
    OrcaSlots<kOrcaMaxNeighbors> nbr;
    orca_slots_clear(nbr);
    for (int j = 0; j < n_live; ++j) {
      if (j == i) continue;
      const double* o = &dr[(size_t)j * W];
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
      const double* o = &dr[(size_t)j * W];
      S.put(kb + k, orca_plane(orca_v3(o[0] - d[0], o[1] - d[1], o[2] - d[2]), orca_v3(d[3] - o[3], d[4] - o[4], d[5] - o[5]),
                               d[6] + o[6], tau, time_step, o[9] != 0.0 ? 1.0 : 0.5, vi, &br));  // S2: a parked neighbour
    }
    const OrcaV3 pref = shield_pref(d[3], d[4], d[5], d[7], d[8], a);
    const OrcaResult r = orca_solve(S, J, kb + kn, kb, max_speed, pref);
    const unsigned flags = shield_finish(d[3], d[4], d[5], d[7], d[8], a, pref, r.v, val + 7);
    ints[(size_t)i * 2] = r.status; ints[(size_t)i * 2 + 1] = (int32_t)flags;
    val[0] = r.slack; val[1] = r.v.x; val[2] = r.v.y; val[3] = r.v.z; val[4] = pref.x; val[5] = pref.y; val[6] = pref.z;
    totals[kShieldJudged] += 1;
    totals[kShieldTotIntervened] += (flags & kShieldIntervened) != 0u;
    totals[kShieldTotFallback] += r.status == 3;
    totals[kShieldTotClipped] += (flags & kShieldIntervened) != 0u && (flags & 7u) != 0u;
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
  std::fwrite(totals, 8, 4, f);
  std::fclose(f);
  return 0;
}
