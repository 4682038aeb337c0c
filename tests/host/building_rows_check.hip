// building_rows_check.hip -- stand-alone CPU program over the host-callable halves of rvo3d_building_rows
// (csrc/rvo3d_building_kernels.hpp): the per-building arithmetic (building_pair / building_time / building_row), the
// k-slot insertion and the argument checks.  Calls no HIP function and needs no GPU.
//   building_rows_check IN OUT
// IN:  int32 n, nb, k; double reach, below; n x (px py pz vx vy r) doubles; nb x (x y h r) doubles.
// OUT: n int32 counts; n*k*6 float rows; n*nb x (d gap t) doubles; n*nb pass bytes - what
// tests/test_building_rows_host.py compares with tests/building_rows_ref.py, bit for bit.
// Without arguments it runs its own table of the argument checks and of the geometry.  Exit status 0 = all held.
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

static int rc_of(rvo3d_building_rows_args a, int W = 102, int64_t rows_n = 32) {
  const char* why = nullptr;
  const int rc = building_rows_check(&a, W, rows_n, &why);
  REQUIRE(why != nullptr && ((rc == RVO3D_OK) == (why[0] == 0)), "status %d with reason '%s'", rc, why ? why : "(null)");
  return rc;
}

static int self_test() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  static float buf[32 * 200], dense[32 * 102];
  const rvo3d_building_rows_args ok{4, 5.0, 2.0, buf, 24, 0, nullptr, nullptr};
  REQUIRE(rc_of(ok) == RVO3D_OK, "the plain stand-alone call");
  const char* why = nullptr;
  REQUIRE(building_rows_check(nullptr, 102, 32, &why) == RVO3D_ERR_INVALID, "null args");
  { auto a = ok; a.k = 0; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "k = 0"); }
  { auto a = ok; a.k = 9; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "k = 9"); }
  { auto a = ok; a.k = 1; REQUIRE(rc_of(a) == RVO3D_OK, "k = 1"); }
  { auto a = ok; a.k = 8; a.row_ld = 48; REQUIRE(rc_of(a) == RVO3D_OK, "k = 8"); }
  for (double reach : {0.0, -1.0, nan, inf, -inf}) { auto a = ok; a.reach = reach; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "reach %g", reach); }
  for (double below : {-1e-300, -1.0, nan, inf}) { auto a = ok; a.below = below; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "below %g", below); }
  { auto a = ok; a.below = 0.0; REQUIRE(rc_of(a) == RVO3D_OK, "below = 0"); }
  { auto a = ok; a.rows = nullptr; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "null rows"); }
  { auto a = ok; a.row_ld = 23; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "row_ld one too small"); }
  { auto a = ok; a.col0 = 7; a.row_ld = 31; REQUIRE(rc_of(a) == RVO3D_OK, "col0 = 7"); a.row_ld = 30; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "col0 = 7, one too small"); }
  { auto a = ok; a.col0 = -1; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "negative col0"); }
  // widen mode: W = 102, k = 4 -> 126 floats
  const rvo3d_building_rows_args wide{4, 5.0, 2.0, buf, 126, 12, nullptr, dense};
  REQUIRE(rc_of(wide) == RVO3D_OK, "the plain widen call");
  { auto a = wide; a.col0 = 0; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "widen with col0 = 0"); }
  { auto a = wide; a.col0 = 13; a.row_ld = 200; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "widen with col0 = 13"); }
  { auto a = wide; a.row_ld = 125; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "widen, row_ld one too small"); }
  { auto a = wide; a.obs = buf; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "obs == rows"); }
  { auto a = wide; a.obs = buf + 31 * 126 + 125; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "obs starts on the last float of rows"); }
  { auto a = wide; a.obs = buf + 31 * 126 + 126; REQUIRE(rc_of(a) == RVO3D_OK, "obs starts right behind rows"); }
  { auto a = wide; a.rows = dense + 32 * 102 - 1; REQUIRE(rc_of(a) == RVO3D_ERR_INVALID, "rows start on the last float of obs"); }
  { auto a = wide; a.rows = dense + 32 * 102; REQUIRE(rc_of(a) == RVO3D_OK, "rows start right behind obs"); }

  // the geometry: LDS of every fleet size and k, the stage's odd stride
  for (int n = 1; n <= kMaxThreads; ++n)
    for (int k = 1; k <= kBldSlots; ++k) {
      REQUIRE(building_lds_bytes(n, k) <= 64 * 1024, "n %d k %d: %zu bytes of LDS", n, k, building_lds_bytes(n, k));
      REQUIRE(building_stage_stride(k) % 2 == 1 && building_stage_stride(k) >= kBldRowFloats * k, "stride of k %d", k);
    }

  // the slots: ascending (gap, index); a ninth candidate falls off the end; ties keep the lower index first
  BuildingSlots s;
  building_slots_clear(s);
  const double gaps[] = {3.0, 1.0, 2.0, 1.0, 0.5, 2.0, 7.0, 6.0, 5.0, 0.5, 9.0};
  for (int i = 0; i < 11; ++i) building_slots_insert(s, gaps[i], i);
  const int want[] = {4, 9, 1, 3, 2, 5, 0, 8};
  for (int i = 0; i < kBldSlots; ++i) REQUIRE(s.idx[i] == want[i] && s.gap[i] == gaps[want[i]], "slot %d holds %d", i, s.idx[i]);
  REQUIRE(s.passing == 11, "passing %d", s.passing);

  // r2 never returns -0.0
  const double z = building_r2(-0.001);
  REQUIRE(z == 0.0 && !std::signbit(z), "r2(-0.001) is -0.0");
  // ... and the float32 form without the division is float32 of it: a sweep, the values next to the 2^24 switch, -0.0
  for (long i = -300000; i <= 300000; ++i) {
    const double v = (double)i * 0.00731 + 1e-7 * (double)(i % 7);
    const float a = building_r2f(v), b = (float)building_r2(v);
    REQUIRE(std::memcmp(&a, &b, 4) == 0, "r2f(%a) = %a, r2 = %a", v, (double)a, (double)b);
  }
  for (double v : {-0.001, -0.0, 0.0, 0.005, 0.015, 167772.155, 167772.16, 167772.165, -167772.16, 1e7, -3e9, 5.0}) {
    const float a = building_r2f(v), b = (float)building_r2(v);
    REQUIRE(std::memcmp(&a, &b, 4) == 0 && !(a == 0.f && std::signbit(a)), "r2f(%a) = %a, r2 = %a", v, (double)a, (double)b);
  }
  std::printf("building rows ok: %ld checks\n", g_checks);
  return 0;
}

template <class T>
static void read_n(std::FILE* f, T* p, size_t n) {
  if (std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}

int main(int argc, char** argv) {
  if (argc == 1) return self_test();
  if (argc != 3) { std::fprintf(stderr, "usage: %s [IN OUT]\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int32_t hdr[3];
  double gatep[2];
  read_n(f, hdr, 3); read_n(f, gatep, 2);
  const int n = hdr[0], nb = hdr[1], k = hdr[2];
  if (n < 0 || nb < 0 || k < 1 || k > kBldSlots) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> dr((size_t)n * 6), bl((size_t)nb * 4);
  read_n(f, dr.data(), dr.size()); read_n(f, bl.data(), bl.size());
  std::fclose(f);

  std::vector<int32_t> cnt((size_t)n);
  std::vector<float> rows((size_t)n * k * kBldRowFloats, 0.f);
  std::vector<double> pairs((size_t)n * nb * 3);
  std::vector<unsigned char> pass((size_t)n * nb);
  for (int i = 0; i < n; ++i) {
    const double* d = &dr[(size_t)i * 6];
    BuildingSlots s;
    building_slots_clear(s);
    for (int j = 0; j < nb; ++j) {
      const double* b = &bl[(size_t)j * 4];
      const BuildingPair q = building_pair(d[0], d[1], d[2], d[5], b[0], b[1], b[2], b[3], gatep[0], gatep[1]);
      double* o = &pairs[((size_t)i * nb + j) * 3];
      o[0] = q.d; o[1] = q.gap; o[2] = building_time(q.ex, q.ey, d[3], d[4], d[5] + b[3]);
      pass[(size_t)i * nb + j] = q.pass ? 1 : 0;
      if (q.pass) building_slots_insert(s, q.gap, j);
    }
    cnt[(size_t)i] = s.passing < k ? s.passing : k;
    for (int t = 0; t < k; ++t)
      if (s.idx[t] >= 0) {
        const double* b = &bl[(size_t)s.idx[t] * 4];
        building_row(d[0], d[1], d[2], d[3], d[4], d[5], b[0], b[1], b[2], b[3], &rows[((size_t)i * k + t) * kBldRowFloats]);
      }
  }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  std::fwrite(cnt.data(), 4, cnt.size(), f);
  std::fwrite(rows.data(), 4, rows.size(), f);
  std::fwrite(pairs.data(), 8, pairs.size(), f);
  std::fwrite(pass.data(), 1, pass.size(), f);
  std::fclose(f);
  return 0;
}
