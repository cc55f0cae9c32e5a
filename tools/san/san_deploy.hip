// TEST INFRASTRUCTURE ONLY: the product's deployed-observation law (csrc/quad_deploy.h, through the host
// shim tests/native_deploy/deploy_host.hip) under ASan + UBSan on the host: random, out-of-bounds and
// non-finite positions, timestamps, alphas and velocities; estimator state carried.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../tests/native_deploy/deploy_host.hip"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double urand() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return double(rng_state >> 11) * 0x1p-53;
}
static float special(int k) {
  const float inf = std::numeric_limits<float>::infinity();
  const float v[8] = {0.f, -0.f, inf, -inf, std::nanf(""), 3.4e38f, -3.4e38f, 1e-45f};
  return v[k & 7];
}

int main() {
  QuadCfg cfg;
  default_cfg_fill(QUAD_ENV_HOVER, QUAD_WRAP_NONE, &cfg);
  const int n = 4096;
  std::vector<float> pos(3 * n), s(12 * n), tg(3 * n), obs(12 * n);
  std::vector<double> t(n), vel(3 * n), so(8 * n);
  long bad = 0;
  const double alphas[6] = {0.0, 0.8, 1.0, -1.0, std::nan(""), std::numeric_limits<double>::infinity()};
  for (int pass = 0; pass < 6; pass++) {
    const double scale = pass == 0 ? 1.0 : (pass == 1 ? 1e30 : 10.0);
    double now = 0.0;
    for (int i = 0; i < n; i++) {
      for (int j = 0; j < 3; j++) pos[3 * i + j] = float((2.0 * urand() - 1.0) * scale);
      for (int j = 0; j < 12; j++) s[12 * i + j] = float((2.0 * urand() - 1.0) * scale);
      for (int j = 0; j < 3; j++) tg[3 * i + j] = float((2.0 * urand() - 1.0) * scale);
      now += i % 13 == 0 ? 0.0 : (i % 17 == 0 ? 0.5 : (i % 19 == 0 ? -0.01 : 0.01));  // dt = 0, > max_dt, < 0
      t[i] = now;
      if (pass >= 2 && i % 7 == 0) pos[3 * i + int(urand() * 3)] = special(i / 7);
      if (pass >= 2 && i % 11 == 0) s[12 * i + int(urand() * 12)] = special(i / 11);
      if (pass >= 3 && i % 23 == 0) t[i] = double(special(i / 23));
    }
    double st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (host_est_calls(alphas[pass], pass == 5 ? std::nan("") : 0.1, pos.data(), t.data(), n, st, vel.data(), so.data()) != 0)
      return 1;
    if (host_deploy_obs(&cfg, s.data(), tg.data(), vel.data(), n, obs.data()) != 0) return 1;
    for (int i = 0; i < 12 * n; i++) bad += !(std::isnan(obs[i]) || (obs[i] >= -1.f && obs[i] <= 1.f));
    if (pass == 0)  // finite inputs, alpha 0: every velocity and observation is finite
      for (int i = 0; i < 3 * n; i++) bad += !std::isfinite(vel[i]);
  }
  if (host_est_calls(0.5, 0.1, nullptr, t.data(), n, nullptr, vel.data(), so.data()) != -1) return 1;
  if (bad) {
    std::printf("san_deploy: %ld values outside their range\n", bad);
    return 1;
  }
  std::printf("san_deploy OK\n");
  return 0;
}
