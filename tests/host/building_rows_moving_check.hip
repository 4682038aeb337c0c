// building_rows_moving_check.hip -- stand-alone CPU program over the host-callable halves of rvo3d_building_rows_moving
// (csrc/rvo3d_building_kernels.hpp: building_row_moving, building_rows_moving_check, the stage geometry;
// csrc/rvo3d_motion_kernels.hpp: motion_velocity next to motion_move).  Calls no HIP function and needs no GPU.
//   building_rows_moving_check IN OUT
// IN:  int32 n, nb, k, has_motion; double reach, below, dt; n x (px py pz vx vy r) doubles; nb x (x y h r) doubles; with
//      has_motion: nb x (e0x e0y e1x e1y) doubles, nb speeds (double), nb legs (bytes).
// OUT: n int32 counts; n*k*8 float rows; nb x (vb_x vb_y) doubles - what tests/test_building_rows_moving_host.py compares
// with tests/building_rows_moving_ref.py, bit for bit.
// Without arguments it runs its own table of the argument checks, of the geometry and of the velocity rule's branches.
// Exit status 0 = all held.
#include "rvo3d_building_kernels.hpp"

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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static double g_ends[4], g_speed[1];
static uint8_t g_leg[1];
static const rvo3d_building_motion g_motion{g_ends, g_speed, g_leg};

static int rc_of(rvo3d_building_rows_args a, const rvo3d_building_motion* m = &g_motion, double dt = 1.0,
                 bool attached = true, int W = 102, int64_t rows_n = 32) {
  const char* why = nullptr;
  const int rc = building_rows_moving_check(&a, W, rows_n, attached, m, dt, &why);
  REQUIRE(why != nullptr && ((rc == RVO3D_OK) == (why[0] == 0)), "status %d with reason '%s'", rc, why ? why : "(null)");
  return rc;
}

static int self_test() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  static float buf[32 * 200], dense[32 * 102];
  // ---- the argument checks, with 8k ----
  const rvo3d_building_rows_args ok{4, 5.0, 2.0, buf, 32, 0, nullptr, nullptr};
  REQUIRE(rc_of(ok) == RVO3D_OK, "the plain stand-alone call");
  const char* why = nullptr;
  REQUIRE(building_rows_moving_check(nullptr, 102, 32, true, &g_motion, 1.0, &why) == RVO3D_ERR_INVALID, "null args");
  { auto a = ok; a.k = 0; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "k = 0"); }
  { auto a = ok; a.k = 9; a.row_ld = 100; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "k = 9"); }
  { auto a = ok; a.k = 1; REQUIRE(rc_of(a) == RVO3D_OK, "k = 1"); }
  { auto a = ok; a.k = 8; a.row_ld = 64; REQUIRE(rc_of(a) == RVO3D_OK, "k = 8"); a.row_ld = 63; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "k = 8, one too small"); }
  for (double reach : {0.0, -1.0, nan, inf, -inf}) { auto a = ok; a.reach = reach; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "reach %g", reach); }
  for (double below : {-1e-300, -1.0, nan, inf}) { auto a = ok; a.below = below; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "below %g", below); }
  { auto a = ok; a.rows = nullptr; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "null rows"); }
  { auto a = ok; a.row_ld = 31; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "row_ld one too small"); }
  { auto a = ok; a.row_ld = 24; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "row_ld = 6k is too small"); }
  { auto a = ok; a.col0 = 7; a.row_ld = 39; REQUIRE(rc_of(a) == RVO3D_OK, "col0 = 7"); a.row_ld = 38; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "col0 = 7, one too small"); }
  { auto a = ok; a.col0 = -1; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "negative col0"); }
  { auto a = ok; a.row_ld = 31; const char* w = nullptr; building_rows_moving_check(&a, 102, 32, true, nullptr, 0.0, &w);
    REQUIRE(std::strstr(w, "8 * k") != nullptr, "the reason names 8 * k: '%s'", w); }
  // widen mode: W = 102, k = 3 -> 126 floats
  const rvo3d_building_rows_args wide{3, 5.0, 2.0, buf, 126, 12, nullptr, dense};
  REQUIRE(rc_of(wide) == RVO3D_OK, "the plain widen call");
  { auto a = wide; a.col0 = 0; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "widen with col0 = 0"); }
  { auto a = wide; a.col0 = 13; a.row_ld = 200; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "widen with col0 = 13"); }
  { auto a = wide; a.row_ld = 125; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "widen, row_ld one too small"); }
  { auto a = wide; a.k = 4; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "widen, k = 4 needs 134"); a.row_ld = 134; REQUIRE(rc_of(a) == RVO3D_OK, "widen, k = 4 at 134"); }
  { auto a = wide; a.obs = buf; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "obs == rows"); }
  { auto a = wide; a.obs = buf + 31 * 126 + 125; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "obs starts on the last float of rows"); }
  { auto a = wide; a.obs = buf + 31 * 126 + 126; REQUIRE(rc_of(a) == RVO3D_OK, "obs starts right behind rows"); }
  { auto a = wide; a.row_ld = 140; a.obs = buf + 31 * 140 + 125; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "the last row counts W + 8k floats"); }
  { auto a = wide; a.row_ld = 140; a.obs = buf + 31 * 140 + 126; REQUIRE(rc_of(a) == RVO3D_OK, "... and no more"); }
  { auto a = wide; a.rows = dense + 32 * 102 - 1; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "rows start on the last float of obs"); }
  { auto a = wide; a.rows = dense + 32 * 102; REQUIRE(rc_of(a) == RVO3D_OK, "rows start right behind obs"); }
  // the motion and dt
  REQUIRE(rc_of(ok, nullptr, 1.0, false) == RVO3D_OK, "no motion on a handle without sets");
  REQUIRE(rc_of(ok, nullptr, 0.0, true) == RVO3D_OK, "no motion, dt 0");
  REQUIRE(rc_of(ok, &g_motion, 1.0, false) == RVO3D_ERR_STATE, "a motion without attached sets");
  { rvo3d_building_motion m = g_motion; m.ends = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null ends"); }
  { rvo3d_building_motion m = g_motion; m.speed = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null speed"); }
  { rvo3d_building_motion m = g_motion; m.leg = nullptr; REQUIRE(rc_of(ok, &m) == RVO3D_ERR_INVALID, "null leg"); }
  for (double dt : {-1.0, -1e-300, inf, -inf, nan}) REQUIRE(rc_of(ok, &g_motion, dt) == RVO3D_ERR_INVALID, "dt %g", dt);
  for (double dt : {-1.0, inf, nan}) REQUIRE(rc_of(ok, nullptr, dt) == RVO3D_ERR_INVALID, "dt %g without a motion", dt);
  REQUIRE(rc_of(ok, &g_motion, 0.0) == RVO3D_OK, "dt 0");
  // the row checks come first: a refused row_ld is refused whatever the motion
  { auto a = ok; a.row_ld = 31; REQUIRE(rc_of(a, &g_motion, 1.0, false) == RVO3D_ERR_INVALID, "row_ld before the motion"); }

  // ---- the geometry: LDS of every fleet size and k at rows of eight, the stage's odd stride ----
  for (int n = 1; n <= kMaxThreads; ++n)
    for (int k = 1; k <= kBldSlots; ++k) {
      const size_t b = building_lds_bytes(n, k, kBldRowFloatsMoving);
      REQUIRE(b <= 64 * 1024 && b > building_lds_bytes(n, k), "n %d k %d: %zu bytes of LDS", n, k, b);
      const int s = building_stage_stride(k, kBldRowFloatsMoving);
      REQUIRE(s == 8 * k + 1 && s % 2 == 1, "stride of k %d", k);
      REQUIRE(building_stage_stride(k) == 6 * k + 1, "the stride of rows of six is what it was, k %d", k);
    }
  REQUIRE(building_lds_bytes(512, 8, kBldRowFloatsMoving) == 16384 + 128 * 65 * 4, "T = 512, k = 8: 16 KiB + 32.5 KiB");
  REQUIRE(building_lds_bytes(512, 8) == 16384 + 128 * 49 * 4, "... and 16 KiB + 24.5 KiB as before");

  // ---- rule 2, branch by branch.  A static building does not read ends: a null pointer would trap ----
  {
    MotionVel v = motion_velocity(1.0, 2.0, 1, nullptr, 0.0, 1.0);
    REQUIRE(v.x == 0.0 && v.y == 0.0 && !std::signbit(v.x), "speed 0");
    v = motion_velocity(1.0, 2.0, 1, nullptr, nan, 1.0);
    REQUIRE(v.x == 0.0 && v.y == 0.0, "NaN speed");
    v = motion_velocity(1.0, 2.0, 1, nullptr, 1.5, 0.0);
    REQUIRE(v.x == 0.0 && v.y == 0.0, "dt 0");
    v = motion_velocity(1.0, 2.0, 1, nullptr, -1.0, 1.0);
    REQUIRE(v.x == 0.0 && v.y == 0.0, "a negative speed");
    const double ends[4] = {1.0, 2.0, 4.0, 6.0};  // endpoint 0 = (1, 2), endpoint 1 = (4, 6): 5 m apart
    v = motion_velocity(1.0, 2.0, 0, ends, 1.0, 1.0);  // d == 0: on the endpoint it approaches
    REQUIRE(v.x == 0.0 && v.y == 0.0, "d == 0: (%a, %a)", v.x, v.y);
    v = motion_velocity(1.0, 2.0, 1, ends, 5.0, 1.0);  // d == step exactly: arrival
    REQUIRE(v.x == 3.0 && v.y == 4.0, "d == step: (%a, %a)", v.x, v.y);
    v = motion_velocity(1.0, 2.0, 1, ends, 2.5, 2.0);  // ... with dt = 2: the way over dt
    REQUIRE(v.x == 1.5 && v.y == 2.0, "d == step, dt 2: (%a, %a)", v.x, v.y);
    v = motion_velocity(1.0, 2.0, 1, ends, 10.0, 2.0);  // d < step: still the way over dt, not the speed
    REQUIRE(v.x == 1.5 && v.y == 2.0, "d < step: (%a, %a)", v.x, v.y);
    const double s = std::nextafter(5.0, 0.0);        // d just above step: cruise
    v = motion_velocity(1.0, 2.0, 1, ends, s, 1.0);
    REQUIRE(same_bits(v.x, (3.0 / 5.0) * s) && same_bits(v.y, (4.0 / 5.0) * s) && v.x < 3.0, "d just above step: (%a, %a)", v.x, v.y);
    v = motion_velocity(4.0, 6.0, 2, ends, 1.0, 1.0);  // leg & 1: leg 2 approaches endpoint 0
    REQUIRE(same_bits(v.x, (-3.0 / 5.0) * 1.0) && same_bits(v.y, (-4.0 / 5.0) * 1.0), "leg & 1");
    // next to motion_move: the same branch, and at dt = 1 the cruise step is the velocity
    unsigned long long z = 88172645463325252ull;
    auto uni = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (double)(z >> 11) / 9007199254740992.0; };
    int arrivals = 0, cruises = 0;
    for (int i = 0; i < 20000; ++i) {
      const double x = uni() * 20.0, y = uni() * 16.0, e[4] = {x, y, x + (uni() - 0.5) * 6.0, y + (uni() - 0.5) * 6.0};
      const double sp = 0.3 + uni() * 1.2;
      const MotionStep m = motion_move(x, y, 1, e, sp, 1.0);
      const MotionVel w = motion_velocity(x, y, 1, e, sp, 1.0);
      const bool arrived = m.leg != 1;
      if (arrived) { ++arrivals; REQUIRE(same_bits(w.x, e[2] - x) && same_bits(w.y, e[3] - y), "arrival %d", i); }
      else { ++cruises; REQUIRE(same_bits(x + w.x, m.x) && same_bits(y + w.y, m.y), "cruise %d", i); }
    }
    REQUIRE(arrivals > 500 && cruises > 500, "arrivals %d cruises %d", arrivals, cruises);
  }

  // ---- the row: no motion -> the row of six and two +0.0; a building moving with its drone; one aimed at a standing drone ----
  {
    float f6[6], f8[8];
    building_row(3.0, 4.0, 2.0, -0.75, -1.0, 0.25, 0.0, 0.0, 6.0, 1.0, f6);
    building_row_moving(3.0, 4.0, 2.0, -0.75, -1.0, 0.25, 0.0, 0.0, 6.0, 1.0, 0.0, 0.0, f8);
    REQUIRE(std::memcmp(f6, f8, 24) == 0 && f6[5] > 0.f, "vb = 0: the six floats");
    const float zero = 0.f;
    REQUIRE(std::memcmp(&f8[6], &zero, 4) == 0 && std::memcmp(&f8[7], &zero, 4) == 0, "vb = 0: +0.0 twice");
    building_row_moving(3.0, 4.0, 2.0, -0.75, -1.0, 0.25, 0.0, 0.0, 6.0, 1.0, -0.75, -1.0, f8);
    REQUIRE(std::memcmp(f6, f8, 20) == 0 && f8[5] == 0.f && f8[6] == -0.75f && f8[7] == -1.0f, "moving with the drone: urg_rel 0");
    building_row(3.0, 4.0, 2.0, 0.0, 0.0, 0.25, 0.0, 0.0, 6.0, 1.0, f6);
    building_row_moving(3.0, 4.0, 2.0, 0.0, 0.0, 0.25, 0.0, 0.0, 6.0, 1.0, 0.6, 0.8, f8);
    REQUIRE(f6[5] == 0.f && f8[5] > 0.f && f8[5] < 5.f, "aimed at a standing drone: urg 0, urg_rel %g", (double)f8[5]);
    building_row_moving(3.0, 4.0, 2.0, 0.0, 0.0, 0.25, 0.0, 0.0, 6.0, 1.0, -0.001, -0.0, f8);
    REQUIRE(f8[6] == 0.f && !std::signbit(f8[6]) && !std::signbit(f8[7]), "no -0.0 in the velocity columns");
  }
  std::printf("building rows moving ok: %ld checks\n", g_checks);
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
  int32_t hdr[4];
  double par[3];
  read_n(f, hdr, 4); read_n(f, par, 3);
  const int n = hdr[0], nb = hdr[1], k = hdr[2];
  const bool has_motion = hdr[3] != 0;
  if (n < 0 || nb < 0 || k < 1 || k > kBldSlots) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> dr((size_t)n * 6), bl((size_t)nb * 4), ends, speed;
  std::vector<uint8_t> leg;
  read_n(f, dr.data(), dr.size()); read_n(f, bl.data(), bl.size());
  if (has_motion) {
    ends.resize((size_t)nb * 4); speed.resize((size_t)nb); leg.resize((size_t)nb);
    read_n(f, ends.data(), ends.size()); read_n(f, speed.data(), speed.size()); read_n(f, leg.data(), leg.size());
  }
  std::fclose(f);

  std::vector<double> vb((size_t)nb * 2, 0.0);
  for (int j = 0; j < nb && has_motion; ++j) {
    const double* b = &bl[(size_t)j * 4];
    if (!motion_live(b[2])) continue;
    const MotionVel v = motion_velocity(b[0], b[1], leg[(size_t)j], &ends[(size_t)j * 4], speed[(size_t)j], par[2]);
    vb[(size_t)j * 2] = v.x; vb[(size_t)j * 2 + 1] = v.y;
  }
  std::vector<int32_t> cnt((size_t)n);
  std::vector<float> rows((size_t)n * k * kBldRowFloatsMoving, 0.f);
  for (int i = 0; i < n; ++i) {
    const double* d = &dr[(size_t)i * 6];
    BuildingSlots s;
    building_slots_clear(s);
    for (int j = 0; j < nb; ++j) {
      const double* b = &bl[(size_t)j * 4];
      const BuildingPair q = building_pair(d[0], d[1], d[2], d[5], b[0], b[1], b[2], b[3], par[0], par[1]);
      if (q.pass) building_slots_insert(s, q.gap, j);
    }
    cnt[(size_t)i] = s.passing < k ? s.passing : k;
    for (int t = 0; t < k; ++t)
      if (s.idx[t] >= 0) {
        const size_t j = (size_t)s.idx[t];
        const double* b = &bl[j * 4];
        building_row_moving(d[0], d[1], d[2], d[3], d[4], d[5], b[0], b[1], b[2], b[3], vb[j * 2], vb[j * 2 + 1],
                            &rows[((size_t)i * k + t) * kBldRowFloatsMoving]);
      }
  }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  std::fwrite(cnt.data(), 4, cnt.size(), f);
  std::fwrite(rows.data(), 4, rows.size(), f);
  std::fwrite(vb.data(), 8, vb.size(), f);
  std::fclose(f);
  return 0;
}
