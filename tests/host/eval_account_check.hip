// eval_account_check.hip -- stand-alone check of the evaluator's per-env episode decision
// (csrc/rvo3d_eval_kernels.hpp: eval_account_env, the pure function eval_account_kernel calls), against the
// bookkeeping of post_train.policy_test (train/policy/post_train.py:78-105) restated here case by case.  Calls no HIP
// function and needs no GPU; tests/test_eval_host.py builds it with the host sanitizers and runs it.
// Exit status 0 = every check held.
#include "rvo3d_eval_kernels.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

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

// an env in mid-episode: 4 steps done, 3 drones, nothing ends
static EvalEnvIn base() {
  EvalEnvIn in{};
  in.ep_len = 4; in.ep_ret = -1.25; in.speed_sum = 2.0; in.counted = 0;
  in.norm_sum = 1.5; in.n = 3; in.reward0 = 0.5f;
  in.any_done = false; in.all_finish = false; in.all_info = false;
  in.max_ep_len = 150; in.quota = 2;
  return in;
}

// the running values, the record and the ended byte an env must leave with, from the loop's own text
static void expect(const EvalEnvIn& in, bool ended, int flags, const char* what) {
  const EvalEnvOut o = eval_account_env(in);
  const double speed = in.norm_sum / (double)in.n;
  const double ssum = in.speed_sum + speed, ret = in.ep_ret + (double)in.reward0;
  const int len = in.ep_len + 1;
  REQUIRE(o.ended == ended, "%s: ended %d", what, (int)o.ended);
  REQUIRE(o.record == (ended && in.counted < in.quota), "%s: record %d", what, (int)o.record);
  REQUIRE(o.counted == in.counted + (o.record ? 1 : 0), "%s: counted %d", what, o.counted);
  if (ended) {
    REQUIRE(o.ep_len == 0 && same_bits(o.ep_ret, 0.0) && same_bits(o.speed_sum, 0.0), "%s: running values not zeroed", what);
  } else {
    REQUIRE(o.ep_len == len && same_bits(o.ep_ret, ret) && same_bits(o.speed_sum, ssum), "%s: running values", what);
  }
  if (o.record) {
    REQUIRE(o.rec_len == len, "%s: rec_len %d", what, o.rec_len);
    REQUIRE(same_bits(o.rec_ret, ret), "%s: rec_ret %a", what, o.rec_ret);
    REQUIRE(same_bits(o.rec_speed, ssum / (double)len), "%s: rec_speed %a", what, o.rec_speed);
    REQUIRE(o.rec_flags == flags, "%s: flags %d, expected %d", what, (int)o.rec_flags, flags);
  }
}

int main() {
  // nothing ends
  expect(base(), false, 0, "mid-episode");
  { EvalEnvIn in = base(); in.all_info = true; expect(in, false, 0, "all arrived does not end an episode"); }

  // each end condition alone, and every combination of the four inputs
  for (int m = 0; m < 16; ++m) {
    EvalEnvIn in = base();
    in.any_done = (m & 1) != 0; in.all_finish = (m & 2) != 0; in.all_info = (m & 4) != 0;
    const bool timeout = (m & 8) != 0;
    in.max_ep_len = timeout ? in.ep_len + 1 : 150;
    const bool ended = in.any_done || in.all_finish || timeout;
    const int flags = (in.all_info ? 1 : 0) | (in.all_finish ? 2 : 0) | (in.any_done ? 4 : 0) | (timeout ? 8 : 0);
    char what[32];
    std::snprintf(what, sizeof what, "combination %d", m);
    expect(in, ended, flags, what);
  }

  // the timeout is len == max_ep_len, len = ep_len + 1 (the trainer's is >): one short, exact, one past
  { EvalEnvIn in = base(); in.max_ep_len = in.ep_len + 2; expect(in, false, 0, "len == max_ep_len - 1"); }
  { EvalEnvIn in = base(); in.max_ep_len = in.ep_len + 1; expect(in, true, 8, "len == max_ep_len"); }
  { EvalEnvIn in = base(); in.max_ep_len = in.ep_len; expect(in, false, 0, "len == max_ep_len + 1"); }
  { EvalEnvIn in = base(); in.ep_len = 0; in.max_ep_len = 1; expect(in, true, 8, "max_ep_len 1, first step"); }

  // quota: the last slot is still recorded; past it no record, but the episode ends all the same
  { EvalEnvIn in = base(); in.any_done = true; in.counted = 1; expect(in, true, 4, "last slot of the quota"); }
  for (int counted : {2, 3, 1000}) {
    EvalEnvIn in = base(); in.all_finish = true; in.all_info = true; in.counted = counted;
    expect(in, true, 3, "quota reached");
    const EvalEnvOut o = eval_account_env(in);
    REQUIRE(!o.record && o.counted == counted && o.ended && o.ep_len == 0, "quota reached: counted %d", o.counted);
  }

  // non-finite rewards are carried, not sanitised
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  { EvalEnvIn in = base(); in.reward0 = inf;
    const EvalEnvOut o = eval_account_env(in); REQUIRE(o.ep_ret == (double)inf && !o.ended, "+inf carried"); }
  { EvalEnvIn in = base(); in.reward0 = -inf; in.any_done = true;
    const EvalEnvOut o = eval_account_env(in); REQUIRE(o.record && o.rec_ret == -(double)inf && o.ep_ret == 0.0, "-inf recorded"); }
  { EvalEnvIn in = base(); in.reward0 = nan;
    const EvalEnvOut o = eval_account_env(in); REQUIRE(std::isnan(o.ep_ret) && !o.ended, "nan carried"); }
  { EvalEnvIn in = base(); in.ep_ret = (double)inf; in.reward0 = -inf; in.all_finish = true;
    const EvalEnvOut o = eval_account_env(in);
    REQUIRE(o.record && std::isnan(o.rec_ret) && same_bits(o.ep_ret, 0.0), "inf - inf recorded as nan, then zeroed"); }
  { EvalEnvIn in = base(); in.ep_ret = (double)nan;
    const EvalEnvOut o = eval_account_env(in); REQUIRE(std::isnan(o.ep_ret), "nan stays"); }

  // N = 1: the mean speed is the one drone's norm, bit for bit
  { EvalEnvIn in = base(); in.n = 1; in.norm_sum = 0.1 + 0.2; in.speed_sum = 0.0; in.ep_len = 0;
    const EvalEnvOut o = eval_account_env(in);
    REQUIRE(same_bits(o.speed_sum, 0.1 + 0.2), "N = 1 speed %a", o.speed_sum);
    expect(in, false, 0, "N = 1"); }
  { EvalEnvIn in = base(); in.n = 1; in.any_done = true; in.all_finish = true; in.all_info = true; in.max_ep_len = 5;
    expect(in, true, 15, "N = 1, everything at once"); }

  // lanes per env: the smallest power of two >= n, at most a wave
  for (int n = 1; n <= 512; ++n) {
    const int l = eval_lanes_per_env(n);
    REQUIRE(l >= 1 && l <= 64 && (l & (l - 1)) == 0, "lanes %d for n %d", l, n);
    REQUIRE(n > 64 ? l == 64 : (l >= n && l / 2 < n), "lanes %d for n %d", l, n);
  }

  std::printf("eval account ok: %ld checks\n", g_checks);
  return 0;
}
