// drone_counts_check.hip -- stand-alone check of the per-env drone counts' host set-up (csrc/rvo3d_host_setup.hpp:
// check_drone_counts, pick_counted_kernel, counted_geometry).  Calls no HIP function and needs no GPU;
// tests/test_drone_counts_host.py builds it with the host sanitizers and runs it.  Exit status 0 = every check held.
#include "rvo3d_params.hpp"
#include "rvo3d_lds.hpp"
#include "rvo3d_host_setup.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static rvo3d_config config(int E, int N, int nm) {
  rvo3d_config c{};
  c.num_envs = E; c.num_drones = N; c.max_points = 2; c.num_buildings = 0; c.neighbors_num = nm;
  c.env_train = 1; c.device = 0; c.action_decimals = -1;
  c.map_size[0] = 30.0; c.map_size[1] = 30.0; c.map_size[2] = 8.0;
  return c;
}

// a. the validator: every entry 1..N, NULL detaches, more than 256 drones are refused either way
static void check_validator() {
  bool detach = false;
  std::string err;
  for (int N = 2; N <= 256; ++N) {
    std::vector<int32_t> c = {1, N, (N + 1) / 2, N > 2 ? N - 1 : 1};
    REQUIRE(check_drone_counts(4, N, c.data(), detach, err) == RVO3D_OK && !detach, "N = %d: counts in range", N);
    for (int32_t bad : {0, -1, N + 1, 0x7fffffff}) {
      std::vector<int32_t> b = c;
      b[2] = bad;
      err.clear();
      REQUIRE(check_drone_counts(4, N, b.data(), detach, err) == RVO3D_ERR_INVALID && !err.empty(), "N = %d: count %d", N,
              (int)bad);
    }
    REQUIRE(check_drone_counts(4, N, nullptr, detach, err) == RVO3D_OK && detach, "N = %d: NULL detaches", N);
  }
  const int32_t one[1] = {5};
  for (int N : {257, 300, 512}) {
    err.clear();
    REQUIRE(check_drone_counts(1, N, one, detach, err) == RVO3D_ERR_INVALID && err.find("256") != std::string::npos,
            "N = %d is beyond the rings", N);
    REQUIRE(check_drone_counts(1, N, nullptr, detach, err) == RVO3D_ERR_INVALID, "N = %d, NULL", N);
  }
}

// b. the picker and its geometry for every num_drones: a padded compile-time ring that holds the layout, with the
//    handle's own number of waves; whole envs per workgroup; LDS as the ring's plain kernel needs it
static void check_picker() {
  for (int nm : {0, 3, 10})
    for (int E : {1, 2, 7})
      for (int N = 2; N <= 256; ++N) {
        const rvo3d_config cfg = config(E, N, nm);
        Params P;
        Cold C;
        Geometry G{}, K{};
        std::string err;
        REQUIRE(plan_env(&cfg, 0, P, C, G, err) == RVO3D_OK, "plan_env N = %d: %s", N, err.c_str());
        const Pick k = pick_counted_kernel(P);
        REQUIRE(k.pad && k.nfix >= N, "N = %d runs on ring %d", N, k.nfix);
        REQUIRE(k.nfix == 32 || k.nfix == 64 || k.nfix == 128 || k.nfix == 192 || k.nfix == 256, "ring %d", k.nfix);
        REQUIRE(k.nfix == 32 || k.nfix - 64 < N, "N = %d: ring %d is not the smallest", N, k.nfix);
        REQUIRE((k.nfix + 63) / 64 == P.nw, "N = %d: ring %d has the handle's %d waves (the stage-G arrays)", N, k.nfix, P.nw);
        bool two_phase = true;
        REQUIRE(counted_geometry(0, P, G, K, two_phase, err) == RVO3D_OK, "geometry N = %d: %s", N, err.c_str());
        const int epb = k.nfix <= 64 ? 64 / k.nfix : 1;
        REQUIRE(K.threads == (k.nfix <= 64 ? 64 : k.nfix) && K.threads <= kMaxThreads, "threads");
        REQUIRE(K.blocks == (E + epb - 1) / epb && (long)K.blocks * epb >= E, "blocks cover the envs");
        REQUIRE(K.lds == (int)lds_bytes(K.threads, nm, epb, k.nfix, P.nw) && K.lds <= 64 * 1024, "lds %d", K.lds);
        // the two-phase table was made for the handle's workgroup: it may only be used where the shapes agree
        REQUIRE(two_phase == (epb == P.epb && K.threads == G.threads), "two-phase");
        if (N == 64 && E >= 1) REQUIRE(two_phase, "the headline shape keeps the two-phase row writer");
        if (N <= 16 && E > 2) REQUIRE(!two_phase, "N = %d packs more envs per wave without counts", N);
        // a plain handle of exactly the ring's size runs the same geometry
        if (N == k.nfix && E >= 2) REQUIRE(K.threads == G.threads && K.lds == G.lds, "N = ring: the plain kernel's geometry");
      }
  Params big;
  std::memset(&big, 0, sizeof big);
  big.N = 300; big.E = 1; big.nw = 8;
  Geometry G{}, K{};
  bool tp = false;
  std::string err;
  REQUIRE(pick_counted_kernel(big).nfix == 0, "no counted kernel beyond 256 drones");
  REQUIRE(counted_geometry(0, big, G, K, tp, err) == RVO3D_ERR_INVALID && !err.empty(), "300 drones are refused");
}

int main() {
  check_validator();
  check_picker();
  std::printf("drone counts ok (%ld checks)\n", g_checks);
  return 0;
}
