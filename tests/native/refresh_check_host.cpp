// The host checks of gs_learner_refresh that need no device (csrc/refresh.h: gs_refresh_check, gs_refresh_sizes), run stand-alone:
// every GS_E_INVALID rule of the config, the valid configs, and the scratch sizes at the limits of n.  Prints "ok" lines; exit status 1
// on the first mismatch.  tests/test_refresh.py builds and runs it; built with -fsanitize=address,undefined it runs clean.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "refresh.h"

static int failures = 0;

static void expect(bool refused, const gs_refresh_config* cfg, int32_t n, const char* what) {
  const std::string why = gs_refresh_check(cfg, n);
  if (why.empty() == refused) {
    std::printf("MISMATCH %s: %s\n", what, why.empty() ? "accepted" : why.c_str());
    ++failures;
  }
}

int main() {
  static_assert(sizeof(gs_refresh_config) == 72 && sizeof(gs_refresh_config) % 8 == 0, "gs_refresh_config");
  gs_refresh_config ok{};
  ok.struct_size = (int32_t)sizeof(gs_refresh_config);
  ok.groups = GS_REFRESH_TD_POLICY; ok.bootstrap_mask = 3; ok.stochastic = 1; ok.gamma = 0.99; ok.alpha = 0.2; ok.reward_scale = 1.0;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  expect(true, nullptr, 1, "NULL config");
  expect(false, &ok, 1, "n = 1");
  expect(false, &ok, 1 << 24, "n = 2^24");
  expect(true, &ok, 0, "n = 0");
  expect(true, &ok, -5, "n < 0");
  expect(true, &ok, (1 << 24) + 1, "n = 2^24 + 1");
  expect(true, &ok, std::numeric_limits<int32_t>::max(), "n = INT32_MAX");
  for (int g = 1; g <= GS_REFRESH_ALL; ++g) { gs_refresh_config c = ok; c.groups = g; expect(false, &c, 33, "every group set"); }
  for (int g : {0, 16, 17, 31, -1, 1 << 30}) { gs_refresh_config c = ok; c.groups = g; expect(true, &c, 33, "groups"); }
  for (int s : {64, 0, 80, -72}) { gs_refresh_config c = ok; c.struct_size = s; expect(true, &c, 33, "struct_size"); }
  for (double a : {nan, inf, -inf, -0.5}) { gs_refresh_config c = ok; c.alpha = a; expect(true, &c, 33, "alpha"); }
  for (double a : {0.0, 1e300}) { gs_refresh_config c = ok; c.alpha = a; expect(false, &c, 33, "alpha"); }
  for (int s : {2, -1}) { gs_refresh_config c = ok; c.stochastic = s; expect(true, &c, 33, "stochastic"); }
  { gs_refresh_config c = ok; c.stochastic = 0; expect(false, &c, 33, "stochastic = 0"); }
  std::printf("checks: %s\n", failures ? "FAILED" : "ok");

  // the scratch of the largest batch the entry takes, at the widest ABI shapes: no product wraps, and a buffer of each size indexes
  // its last element where the kernels do
  const int before = failures;
  const GsRefreshSizes big = gs_refresh_sizes(1 << 24, 4096, 128);
  if (big.rows != (size_t)1 << 24 || big.pairs != (size_t)1 << 25 || big.obs != ((size_t)1 << 24) * 4096 || big.act != ((size_t)1 << 24) * 128 ||
      big.pre != ((size_t)1 << 25) * 128 || big.twin != (size_t)1 << 25) ++failures;
  for (int n : {1, 33, 64, 65, 185}) {
    const int D = 71, A = 3;
    const GsRefreshSizes s = gs_refresh_sizes(n, D, A);
    std::vector<double> obs(s.obs, 0.0), act(s.act, 0.0), twin(s.twin, 0.0);
    std::vector<float> pre(s.pre, 0.0f);
    std::vector<int32_t> pairs(s.pairs, 0);
    obs[(size_t)(n - 1) * D + (D - 1)] = 1.0; act[(size_t)(n - 1) * A + (A - 1)] = 1.0; twin[(size_t)n + (n - 1)] = 1.0;
    pre[(size_t)(n - 1) * (2 * A) + (2 * A - 1)] = 1.0f; pairs[2 * (size_t)(n - 1) + 1] = 1;
    if (obs.back() != 1.0 || act.back() != 1.0 || twin.back() != 1.0 || pre.back() != 1.0f || pairs.back() != 1) ++failures;
  }
  std::printf("sizes: %s\n", failures == before ? "ok" : "FAILED");
  // the clamp every kernel applies to a batch index
  const long long N = 185;
  const long long in[] = {-7, -1, 0, 1, 184, 185, 1ll << 31}, want[] = {0, 0, 0, 1, 184, 184, 184};
  const int before2 = failures;
  for (int k = 0; k < 7; ++k) if (GS_RF_CLAMP(in[k], N) != want[k]) ++failures;
  std::printf("clamp: %s\n", failures == before2 ? "ok" : "FAILED");
  return failures ? 1 : 0;
}
