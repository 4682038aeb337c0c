// rvo_city_check.hip -- stand-alone CPU program over the host-callable halves of rvo3d_rvo_vel_city
// (csrc/rvo3d_rvo_city_kernels.hpp: city_disk, city_roots, city_blocks, city_select, city_last_offer, rvo_city_check;
// csrc/rvo3d_building_kernels.hpp: building_pair; csrc/rvo3d_motion_kernels.hpp: motion_velocity).  Calls no HIP
// function and needs no GPU.
//   rvo_city_check IN OUT
// IN:  int32 n, nb, has_motion; double reach, below, horizon, clear_xy, clear_z, dt; n x 20 doubles (px py pz r, the
//      candidate values 4 per axis, tc_min, des[3]); n x 3 int32 (values per axis); n x 2 uint64 (live, cone);
//      nb x (x y h r) doubles; with has_motion: nb x (e0x e0y e1x e1y) doubles, nb speeds (double), nb legs (bytes).
// OUT: n uint64 blocked masks; n int32 n_gated; n int32 tiers; n x 3 doubles out_vel - what
//      tests/test_rvo_city_host.py compares with tests/rvo_city_ref.py, bit for bit.
// Without arguments it runs its own table of the argument checks and of rule 2's branches.  Exit status 0 = all held.
#define RVO3D_RVO_CITY_RULES_ONLY
#include "rvo3d_rvo_city_kernels.hpp"

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

static double g_ends[4], g_speed[1], g_out[3];
static uint8_t g_leg[1];
static const rvo3d_building_motion g_motion{g_ends, g_speed, g_leg};

static int rc_of(const rvo3d_rvo_city_args& a, const rvo3d_building_motion* m = &g_motion, double dt = 1.0,
                 bool attached = true) {
  const char* why = nullptr;
  const int rc = rvo_city_check(&a, attached, m, dt, &why);
  REQUIRE(why != nullptr && ((rc == RVO3D_OK) == (why[0] == 0)), "status %d with reason '%s'", rc, why ? why : "(null)");
  return rc;
}

static int self_test() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // ---- the argument checks ----
  rvo3d_rvo_city_args ok{};
  ok.vmax[0] = ok.vmax[1] = ok.vmax[2] = 2.0;
  ok.acceler = 0.5; ok.reach = 10.0; ok.below = 1.0; ok.horizon = 5.0; ok.out_vel = g_out;
  REQUIRE(rc_of(ok) == RVO3D_OK, "the plain call");
  const char* why = nullptr;
  REQUIRE(rvo_city_check(nullptr, true, &g_motion, 1.0, &why) == RVO3D_ERR_INVALID, "null args");
  { auto a = ok; a.out_vel = nullptr; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "null out_vel"); }
  for (double v : {-1e-300, 1.0000000000000002, nan, inf, -inf}) { auto a = ok; a.acceler = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "acceler %g", v); }
  for (double v : {0.0, 1.0}) { auto a = ok; a.acceler = v; REQUIRE(rc_of(a) == RVO3D_OK, "acceler %g", v); }
  for (double v : {0.0, -1.0, nan, inf, -inf}) { auto a = ok; a.reach = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "reach %g", v); }
  { auto a = ok; a.reach = 1e-300; REQUIRE(rc_of(a) == RVO3D_OK, "a tiny reach"); }
  for (double v : {-1e-300, -1.0, nan, inf}) { auto a = ok; a.below = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "below %g", v); }
  { auto a = ok; a.below = 0.0; REQUIRE(rc_of(a) == RVO3D_OK, "below 0"); }
  for (double v : {0.0, -1.0, nan, inf, -inf}) { auto a = ok; a.horizon = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "horizon %g", v); }
  for (double v : {-1e-300, -1.0, nan, inf}) {
    { auto a = ok; a.clear_xy = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "clear_xy %g", v); }
    { auto a = ok; a.clear_z = v; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "clear_z %g", v); }
  }
  { auto a = ok; a.clear_xy = 0.5; a.clear_z = 2.0; REQUIRE(rc_of(a) == RVO3D_OK, "clearances"); }
  REQUIRE(rc_of(ok, nullptr, 1.0, false) == RVO3D_OK, "no motion on a handle without sets");
  REQUIRE(rc_of(ok, nullptr, 0.0, true) == RVO3D_OK, "no motion, dt 0");
  REQUIRE(rc_of(ok, &g_motion, 1.0, false) == RVO3D_ERR_STATE, "a motion without attached sets");
  { rvo3d_building_motion m = g_motion; m.ends = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null ends"); }
  { rvo3d_building_motion m = g_motion; m.speed = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null speed"); }
  { rvo3d_building_motion m = g_motion; m.leg = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null leg"); }
  for (double dt : {-1.0, -1e-300, inf, -inf, nan}) REQUIRE(rc_of(ok, &g_motion, dt) == RVO3D_ERR_INVALID, "dt %g", dt);
  for (double dt : {-1.0, inf, nan}) REQUIRE(rc_of(ok, nullptr, dt) == RVO3D_ERR_INVALID, "dt %g without a motion", dt);
  REQUIRE(rc_of(ok, &g_motion, 0.0) == RVO3D_OK, "dt 0");
  // the parameters come first: a refused horizon is refused whatever the motion
  { auto a = ok; a.horizon = nan; REQUIRE(rc_of(a, &g_motion, 1.0, false) == RVO3D_ERR_INVALID, "horizon before the motion"); }

  // ---- rule 2, branch by branch: a drone at (-5, 0, 2), r 0.25, a building at the origin, r_b 1, h 6 ----
  {
    const BuildingPair q = building_pair(-5.0, 0.0, 2.0, 0.25, 0.0, 0.0, 6.0, 1.0, 10.0, 1.0);
    REQUIRE(q.pass && q.ex == -5.0 && q.ey == 0.0, "the gate");
    REQUIRE(!building_pair(-5.0, 0.0, 7.0, 0.25, 0.0, 0.0, 6.0, 1.0, 10.0, 1.0).pass, "a roof 1 m below does not pass");
    REQUIRE(!building_pair(-5.0, 0.0, 2.0, 0.25, 0.0, 0.0, -inf, 1.0, 10.0, 1.0).pass, "a filler does not pass");
    const CityDisk k = city_disk(q.ex, q.ey, 0.25, 1.0, 6.0, 0.0, 0.0);
    REQUIRE(k.cq == 25.0 - 1.5625 && k.H == 6.0, "the disk");
    CityRoots r = city_roots(k, 1.0, 0.0);  // head-on: enters at 3.75, leaves at 6.25
    REQUIRE(r.hit && r.t_in == 3.75 && r.t_out == 6.25, "head-on: [%a, %a]", r.t_in, r.t_out);
    REQUIRE(city_blocks(r, 2.0, 0.0, k.H, 5.0), "blocked");
    REQUIRE(!city_blocks(r, 2.0, 0.0, k.H, 3.5), "beyond the horizon");
    REQUIRE(!city_blocks(r, 2.0, 1.5, k.H, 5.0), "a climber: 7.625 m up on arrival");
    REQUIRE(city_blocks(r, 2.0, 1.0, k.H, 5.0), "a slower climber: 5.75 m on arrival");
    REQUIRE(!city_roots(k, -1.0, 0.0).hit, "moving away");
    REQUIRE(!city_roots(k, 0.0, 1.0).hit, "passing by: disc <= 0");
    REQUIRE(!city_roots(k, 0.0, 0.0).hit, "standing outside: disc == 0");
    // over the roof at (0, 0, 8): inside the disk
    const CityDisk in = city_disk(0.0, 0.0, 0.25, 1.0, 6.0, 0.0, 0.0);
    r = city_roots(in, 0.0, 0.0);
    REQUIRE(r.hit && r.t_in == 0.0 && r.t_out == inf, "hovering: a == 0");
    REQUIRE(!city_blocks(r, 8.0, 0.0, in.H, 5.0) && !city_blocks(r, 8.0, -0.25, in.H, 5.0), "hovering over the roof is free");
    REQUIRE(city_blocks(r, 8.0, -0.5, in.H, 5.0), "sinking onto the roof within the horizon is blocked");
    r = city_roots(in, 1.0, 0.0);
    REQUIRE(r.hit && r.t_in == 0.0 && r.t_out == 1.25, "leaving the disk: %a", r.t_out);
    REQUIRE(!city_blocks(r, 8.0, -1.5, in.H, 5.0) && city_blocks(r, 8.0, -2.0, in.H, 5.0), "... and sinking while it leaves");
    // clearances widen the disk and raise the roof
    const CityDisk wide = city_disk(q.ex, q.ey, 0.25, 1.0, 6.0, 0.75, 2.0);
    r = city_roots(wide, 1.0, 0.0);
    REQUIRE(r.hit && r.t_in == 3.0 && wide.H == 8.0 && city_blocks(r, 2.0, 1.5, wide.H, 5.0), "clear_xy, clear_z");
  }
  // ---- tier 3's order: the largest tb, then the least dd, then the first ----
  {
    const double des[3] = {1.0, 0.0, 0.0};
    CityLast s{false, 0.0, 0.0, {0.0, 0.0, 0.0}};
    city_last_offer(s, 1.0, 0.0, 1.0, 0.0, des);
    city_last_offer(s, 2.0, 0.0, 2.0, 0.0, des);
    REQUIRE(s.v[1] == 2.0, "a later hit wins");
    city_last_offer(s, 2.0, 0.0, -2.0, 0.0, des);
    REQUIRE(s.v[1] == 2.0, "equal tb and dd: the first stays");
    city_last_offer(s, 2.0, 0.5, 0.0, 0.0, des);
    REQUIRE(s.v[0] == 0.5, "equal tb: the closer to des");
    city_last_offer(s, 1.5, 1.0, 0.0, 0.0, des);
    REQUIRE(s.v[0] == 0.5, "an earlier hit loses");
  }
  std::printf("rvo city ok: %ld checks\n", g_checks);
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
  int32_t hdr[3];
  double par[6];
  read_n(f, hdr, 3); read_n(f, par, 6);
  const int n = hdr[0], nb = hdr[1];
  const bool has_motion = hdr[2] != 0;
  if (n < 0 || nb < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
  const double reach = par[0], below = par[1], horizon = par[2], clear_xy = par[3], clear_z = par[4], dt = par[5];
  std::vector<double> dr((size_t)n * 20), bl((size_t)nb * 4), ends, speed;
  std::vector<int32_t> cnts((size_t)n * 3);
  std::vector<uint64_t> masks((size_t)n * 2);
  std::vector<uint8_t> leg;
  read_n(f, dr.data(), dr.size()); read_n(f, cnts.data(), cnts.size()); read_n(f, masks.data(), masks.size());
  read_n(f, bl.data(), bl.size());
  if (has_motion) {
    ends.resize((size_t)nb * 4); speed.resize((size_t)nb); leg.resize((size_t)nb);
    read_n(f, ends.data(), ends.size()); read_n(f, speed.data(), speed.size()); read_n(f, leg.data(), leg.size());
  }
  std::fclose(f);

  std::vector<double> vb((size_t)nb * 2, 0.0);
  for (int j = 0; j < nb && has_motion; ++j) {
    const double* b = &bl[(size_t)j * 4];
    if (!motion_live(b[2])) continue;
    const MotionVel v = motion_velocity(b[0], b[1], leg[(size_t)j], &ends[(size_t)j * 4], speed[(size_t)j], dt);
    vb[(size_t)j * 2] = v.x; vb[(size_t)j * 2 + 1] = v.y;
  }
  std::vector<uint64_t> blocked((size_t)n, 0);
  std::vector<int32_t> gated((size_t)n, 0), tiers((size_t)n, 0);
  std::vector<double> out((size_t)n * 3, 0.0);
  for (int i = 0; i < n; ++i) {
    const double* d = &dr[(size_t)i * 20];
    const double *vals = d + 4, tc_min = d[16], *des = d + 17;
    const int cnt[3] = {cnts[(size_t)i * 3], cnts[(size_t)i * 3 + 1], cnts[(size_t)i * 3 + 2]};
    if (cnt[0] < 0 || cnt[0] > 4 || cnt[1] < 0 || cnt[1] > 4 || cnt[2] < 0 || cnt[2] > 4) { std::fprintf(stderr, "bad counts\n"); return 2; }
    const unsigned long long live = masks[(size_t)i * 2], cone = masks[(size_t)i * 2 + 1];
    unsigned long long blk = 0;
    double tb[64];
    for (double& t : tb) t = safety_inf();
    for (int j = 0; j < nb; ++j) {
      const double* b = &bl[(size_t)j * 4];
      const BuildingPair q = building_pair(d[0], d[1], d[2], d[3], b[0], b[1], b[2], b[3], reach, below);
      if (!q.pass) continue;
      ++gated[(size_t)i];
      const CityDisk k = city_disk(q.ex, q.ey, d[3], b[3], b[2], clear_xy, clear_z);
      for (int ix = 0; ix < cnt[0]; ++ix)
        for (int iy = 0; iy < cnt[1]; ++iy) {
          const CityRoots r = city_roots(k, vals[ix] - vb[(size_t)j * 2], vals[4 + iy] - vb[(size_t)j * 2 + 1]);
          if (!r.hit) continue;
          for (int iz = 0; iz < cnt[2]; ++iz) {
            const int c = (ix * cnt[1] + iy) * cnt[2] + iz;
            if (((live >> c) & 1ull) && city_blocks(r, d[2], vals[8 + iz], k.H, horizon)) {
              blk |= 1ull << c;
              tb[c] = r.t_in < tb[c] ? r.t_in : tb[c];
            }
          }
        }
    }
    blocked[(size_t)i] = blk;
    double* o = &out[(size_t)i * 3];
    int tier = city_select(cnt, [&](int k, int t) { return vals[4 * k + t]; }, des, tc_min, live, cone, blk, o);
    if (tier == 0) {
      tier = live ? 3 : 4;
      CityLast best{false, 0.0, 0.0, {0.0, 0.0, 0.0}};
      for (int ix = 0; ix < cnt[0]; ++ix)
        for (int iy = 0; iy < cnt[1]; ++iy)
          for (int iz = 0; iz < cnt[2]; ++iz) {
            const int c = (ix * cnt[1] + iy) * cnt[2] + iz;
            if ((live >> c) & 1ull) city_last_offer(best, tb[c], vals[ix], vals[4 + iy], vals[8 + iz], des);
          }
      o[0] = best.v[0]; o[1] = best.v[1]; o[2] = best.v[2];
    }
    tiers[(size_t)i] = tier;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  std::fwrite(blocked.data(), 8, blocked.size(), f);
  std::fwrite(gated.data(), 4, gated.size(), f);
  std::fwrite(tiers.data(), 4, tiers.size(), f);
  std::fwrite(out.data(), 8, out.size(), f);
  std::fclose(f);
  return 0;
}
