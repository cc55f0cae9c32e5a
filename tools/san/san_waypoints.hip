// TEST INFRASTRUCTURE ONLY: the product's waypoint tracker (csrc/quad_waypoints.h, through the host shim
// tests/native_waypoints/waypoints_host.hip) under ASan + UBSan on the host: random, huge and non-finite
// positions, rewards and waypoints, sets of 1 .. 9 points, every flag combination.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../tests/native_waypoints/waypoints_host.hip"

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
  const int n = 512;
  std::vector<float> pos(3 * n), rew(n), target(3 * (n + 1));
  std::vector<unsigned char> te(n), tr(n);
  std::vector<double> track(6 * n), wp(3 * 9);
  long bad = 0;
  for (int pass = 0; pass < 64; pass++) {
    const int cnt = 1 + pass % 9;
    const double scale = pass % 4 == 1 ? 1e30 : 1.0;
    for (int j = 0; j < 3 * cnt; j++) wp[j] = (2.0 * urand() - 1.0) * scale;
    if (pass % 8 == 7) wp[int(urand() * 3 * cnt)] = double(special(pass / 8));
    for (int i = 0; i < n; i++) {
      const int k = int(urand() * cnt);
      for (int j = 0; j < 3; j++) pos[3 * i + j] = float(wp[3 * k + j] + (2.0 * urand() - 1.0) * 0.3 * scale);
      rew[i] = float(2.0 * urand() - 1.0);
      if (pass >= 16 && i % 7 == 0) pos[3 * i + int(urand() * 3)] = special(i / 7);
      if (pass >= 16 && i % 11 == 0) rew[i] = special(i / 11);
      te[i] = pass % 3 == 0 && urand() < 0.01;
      tr[i] = pass % 3 == 1 && urand() < 0.01;
    }
    const float radius = pass % 5 == 0 ? 0.f : (pass % 5 == 1 ? std::numeric_limits<float>::infinity() : 0.25f);
    float pos0[3];
    const int steps = host_lap(wp.data(), cnt, radius, pos.data(), rew.data(), te.data(), tr.data(), n, track.data(),
                               target.data(), pos0);
    if (steps < 0 || steps > n) return 1;
    for (int i = 0; i < n; i++) {
      const double* o = track.data() + 6 * i;
      bad += !(o[0] >= 0 && o[0] < cnt) || !(o[4] >= 0 && o[4] <= 3) || o[3] > i + 1 || o[1] > o[3];
    }
    if (radius == 0.f) bad += track[6 * (n - 1) + 1] != 0;  // strict <: nothing is ever reached
  }
  if (host_lap(nullptr, 1, 0.25f, pos.data(), rew.data(), te.data(), tr.data(), n, track.data(), target.data(),
               nullptr) != -1)
    return 1;
  if (bad) {
    std::printf("san_waypoints: %ld values outside their range\n", bad);
    return 1;
  }
  std::printf("san_waypoints OK\n");
  return 0;
}
