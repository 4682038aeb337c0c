// safety_account_check.hip -- stand-alone check of the episode fold behind rvo3d_eval_account_safety
// (csrc/rvo3d_safety_kernels.hpp: eval_safety_fold / eval_safety_keep, driven by the decision of eval_account_env as the
// account kernel drives them), against the rules of include/rvo3d.h restated here step by step.  Calls no HIP function and
// needs no GPU; tests/test_safety_host.py builds it with the host sanitizers and runs it.
// Exit status 0 = every check held.
#include "rvo3d_safety_kernels.hpp"

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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static const double kInf = std::numeric_limits<double>::infinity();

struct Rec { double sep, bclear, wall; int64_t near; int32_t len; };

// One env as EvalSafetyFold runs it on the device: the decision first, then the fold, the record in the decision's slot,
// then what the env goes on with.
struct Env {
  int32_t ep_len = 0, counted = 0, quota, max_ep_len;
  EvalSafetyRun run{kInf, kInf, kInf, 0};
  std::vector<Rec> rec;
  Env(int32_t quota_, int32_t max_ep_len_) : quota(quota_), max_ep_len(max_ep_len_), rec((size_t)quota_, Rec{-1, -1, -1, -1, -1}) {}
  bool step(const EvalSafetyRun& s, bool any_done) {
    EvalEnvIn in{};
    in.ep_len = ep_len; in.counted = counted; in.n = 2; in.max_ep_len = max_ep_len; in.quota = quota;
    in.any_done = any_done;
    const EvalEnvOut o = eval_account_env(in);
    const EvalSafetyRun f = eval_safety_fold(run, s);
    if (o.record) {
      REQUIRE(counted >= 0 && counted < quota, "record slot %d outside the quota %d", counted, quota);
      rec[(size_t)counted] = Rec{f.sep, f.bclear, f.wall, f.near, o.rec_len};
    }
    run = eval_safety_keep(f, o.ended);
    ep_len = o.ep_len; counted = o.counted;
    return o.ended;
  }
};

int main() {
  // the minimum rule: from +inf, x < m ? x : m
  REQUIRE(same_bits(safety_min(1.0, kInf), 1.0) && same_bits(safety_min(kInf, 1.0), 1.0), "min against +inf");
  REQUIRE(same_bits(safety_min(kInf, kInf), kInf), "min of +inf and +inf");
  REQUIRE(same_bits(safety_min(-2.5, -2.0), -2.5) && same_bits(safety_min(-2.0, -2.5), -2.5), "min of negatives");
  REQUIRE(same_bits(safety_min(0.0, 0.0), 0.0), "min of zeros");

  // running minima: each of the three follows its own smallest step value, near adds up
  {
    Env e(2, 100);
    const EvalSafetyRun steps[] = {{3.0, kInf, 1.5, 0}, {2.0, 4.0, 1.75, 2}, {2.5, 5.0, -0.125, 1}, {kInf, kInf, kInf, 0}};
    const EvalSafetyRun want[] = {{3.0, kInf, 1.5, 0}, {2.0, 4.0, 1.5, 2}, {2.0, 4.0, -0.125, 3}, {2.0, 4.0, -0.125, 3}};
    for (int t = 0; t < 4; ++t) {
      REQUIRE(!e.step(steps[t], false), "step %d ended", t);
      REQUIRE(same_bits(e.run.sep, want[t].sep) && same_bits(e.run.bclear, want[t].bclear) &&
                  same_bits(e.run.wall, want[t].wall) && e.run.near == want[t].near,
              "running values behind step %d: %a %a %a %lld", t, e.run.sep, e.run.bclear, e.run.wall, (long long)e.run.near);
    }
    REQUIRE(e.counted == 0 && e.ep_len == 4, "nothing recorded in mid-episode");

    // the episode ends: the record holds the running values INCLUDING this step's, in slot counted (< quota), and the
    // running values start again at +inf and 0
    REQUIRE(e.step({0.0, 4.5, 0.25, 5}, true), "collision ends the episode");
    REQUIRE(e.counted == 1 && e.ep_len == 0, "counted %d ep_len %d", e.counted, e.ep_len);
    REQUIRE(same_bits(e.rec[0].sep, 0.0) && same_bits(e.rec[0].bclear, 4.0) && same_bits(e.rec[0].wall, -0.125) &&
                e.rec[0].near == 8 && e.rec[0].len == 5, "record 0: %a %a %a %lld", e.rec[0].sep, e.rec[0].bclear,
            e.rec[0].wall, (long long)e.rec[0].near);
    REQUIRE(e.rec[1].len == -1, "slot 1 written early");
    REQUIRE(same_bits(e.run.sep, kInf) && same_bits(e.run.bclear, kInf) && same_bits(e.run.wall, kInf) && e.run.near == 0,
            "running values not reset behind the episode's end");

    // the next episode knows nothing of the last one; a one-step episode records its own step alone
    REQUIRE(e.step({7.0, kInf, 2.0, 0}, true), "second episode");
    REQUIRE(e.counted == 2, "counted %d", e.counted);
    REQUIRE(same_bits(e.rec[1].sep, 7.0) && same_bits(e.rec[1].bclear, kInf) && same_bits(e.rec[1].wall, 2.0) &&
                e.rec[1].near == 0 && e.rec[1].len == 1, "record 1");

    // past its quota the env goes on: it folds, ends and resets, and no record is touched
    const std::vector<Rec> before = e.rec;
    REQUIRE(!e.step({-1.0, -1.0, -1.0, 9}, false), "past the quota, mid-episode");
    REQUIRE(same_bits(e.run.sep, -1.0) && e.run.near == 9, "past the quota the running values still fold");
    REQUIRE(e.step({-2.0, 1.0, 1.0, 1}, true), "past the quota, the episode ends");
    REQUIRE(e.counted == 2, "counted grew past the quota: %d", e.counted);
    for (size_t k = 0; k < before.size(); ++k)
      REQUIRE(std::memcmp(&before[k], &e.rec[k], sizeof(Rec)) == 0, "record %zu changed past the quota", k);
    REQUIRE(same_bits(e.run.sep, kInf) && e.run.near == 0, "running values not reset past the quota");
  }

  // a timeout ends the episode as a collision does (len == max_ep_len), and records the fold of all its steps
  {
    Env e(1, 3);
    REQUIRE(!e.step({5.0, 6.0, 7.0, 1}, false) && !e.step({4.0, 6.5, 7.5, 1}, false), "before the timeout");
    REQUIRE(e.step({4.5, 5.5, 8.0, 1}, false), "timeout at len == max_ep_len");
    REQUIRE(same_bits(e.rec[0].sep, 4.0) && same_bits(e.rec[0].bclear, 5.5) && same_bits(e.rec[0].wall, 7.0) &&
                e.rec[0].near == 3 && e.rec[0].len == 3, "timeout record");
  }

  // near pair-steps add up in 64 bits
  {
    EvalSafetyRun run{kInf, kInf, kInf, (int64_t)1 << 40};
    const EvalSafetyRun f = eval_safety_fold(run, {1.0, 1.0, 1.0, 130816});
    REQUIRE(f.near == ((int64_t)1 << 40) + 130816, "64-bit near sum");
  }

  // the scan's geometry: lanes per env, threads and LDS for every fleet size
  for (int n = 1; n <= kMaxThreads; ++n) {
    const int L = safety_lanes_per_env(n), T = safety_threads(n);
    REQUIRE(L >= n && T % L == 0 && T % 64 == 0 && T <= kMaxThreads, "n %d: L %d T %d", n, L, T);
    REQUIRE(n > 64 ? (L == T && T - n < 64) : ((L & (L - 1)) == 0 && L == eval_lanes_per_env(n) && T == 256), "n %d: L %d T %d", n, L, T);
    REQUIRE(safety_lds_bytes(n) <= 64 * 1024, "n %d: %zu bytes of LDS", n, safety_lds_bytes(n));
  }

  std::printf("safety account ok: %ld checks\n", g_checks);
  return 0;
}
