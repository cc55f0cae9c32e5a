// TEST INFRASTRUCTURE ONLY: the product's PID control law (csrc/quad_pid.h, through the host shim
// tests/native_pid/pid_host.hip) under ASan + UBSan on the host: random, saturated and non-finite
// states, targets and gains, both modes, integrators carried.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../tests/native_pid/pid_host.hip"

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
  std::vector<float> s(12 * n), t(9 * n), a(4 * n);
  std::vector<double> d(6 * n), io(6 * n);
  long bad = 0;
  for (int pass = 0; pass < 6; pass++) {
    QuadPidGains g;
    host_pid_default_gains(&g);
    if (pass == 2) { g.kd_att = 0.0; g.kp_att = 0.0; }          // 0 / 0 attitude ratio
    if (pass == 3) { g.kd_yaw = 0.0; g.mass = 1e300; }           // division by zero, overflow
    if (pass == 4) { g.tilt_max = std::nan(""); g.axy_max = -1.0; }  // NaN and inverted clips
    const double scale = pass == 0 ? 1.0 : (pass == 1 ? 1e6 : 10.0);
    for (int i = 0; i < n; i++) {
      for (int j = 0; j < 12; j++) s[12 * i + j] = float((2.0 * urand() - 1.0) * scale);
      for (int j = 0; j < 9; j++) t[9 * i + j] = float((2.0 * urand() - 1.0) * scale);
      if (pass >= 1 && pass <= 4 && i % 7 == 0) s[12 * i + int(urand() * 12)] = special(i / 7);
      if (pass >= 1 && pass <= 4 && i % 11 == 0) t[9 * i + int(urand() * 9)] = special(i / 11);
      if (pass == 5) { t[9 * i + 3] = 0.f; t[9 * i + 4] = i % 2 ? 1e-7f : 0.f; }  // the velocity-norm switch
    }
    for (int mode = 0; mode < 2; mode++) {
      double integ[6] = {0, 0, 0, 0, 0, 0};
      if (host_pid_calls(&cfg, &g, mode, s.data(), t.data(), n, integ, a.data(), d.data(), io.data()) != 0) return 1;
      if (pass == 0 || pass == 5)  // finite inputs and gains: every action is finite and inside [-1, 1]
        for (int i = 0; i < 4 * n; i++) bad += !(a[i] >= -1.f && a[i] <= 1.f);
    }
    if (host_pid_calls(&cfg, &g, 2, s.data(), t.data(), n, nullptr, a.data(), d.data(), io.data()) != -1) return 1;
  }
  if (bad) {
    std::printf("san_pid: %ld actions outside [-1, 1]\n", bad);
    return 1;
  }
  std::printf("san_pid OK\n");
  return 0;
}
