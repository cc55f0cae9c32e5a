/* brax_act_ulp.c -- the ulp bounds csrc/brax_actor.h states for silu_f32 and softplus_f32, from a sweep over every
 * float32 input in the working range [-87, 88] against float64 (host only; no GPU).
 *
 *   cc -O2 -fopenmp -o brax_act_ulp tools/diag/brax_act_ulp.c -lm && ./brax_act_ulp
 *
 * The scalar models are the header's expressions with each libm call taken (a) correctly rounded and (b) one ulp
 * off in either direction, the bound HIP documents for the device's expf and log1pf; every other operation is an
 * IEEE float32 operation, as on the device. Prints the largest error of each form in ulps of the float64 result
 * rounded to float32. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static float bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static float off(float x, int d) { return d == 0 ? x : (d > 0 ? nextafterf(x, INFINITY) : nextafterf(x, -INFINITY)); }
static double ulps(float got, double ref) {
  const float r = (float)ref;
  const double sp = (double)nextafterf(fabsf(r), INFINITY) - (double)fabsf(r);
  return fabs((double)got - ref) / sp;
}
static float silu_model(float x, int de) {
  const float e = off((float)exp(-(double)x), de);
  return x / (1.0f + e);
}
static float softplus_model(float x, int de, int dl) {
  const float t = fabsf(x);
  const float e = off((float)exp(-(double)t), de);
  const float l = off((float)log1p((double)e), dl);
  const float m = x > 0.0f ? x : 0.0f;
  return m + l;
}

int main(void) {
  const uint32_t hi_pos = 0x42b00000u /* 88 */, hi_neg = 0x42ae0000u /* 87 */;
  double silu0 = 0, silu1 = 0, sp0 = 0, sp1 = 0;
  float a_silu0 = 0, a_silu1 = 0, a_sp0 = 0, a_sp1 = 0;
#pragma omp parallel
  {
    double s0 = 0, s1 = 0, p0 = 0, p1 = 0;
    float as0 = 0, as1 = 0, ap0 = 0, ap1 = 0;
#pragma omp for schedule(static, 1 << 16)
    for (int64_t k = -(int64_t)hi_neg; k <= (int64_t)hi_pos; k++) {
      const float x = k < 0 ? -bits_f((uint32_t)(-k)) : bits_f((uint32_t)k);
      const double xd = (double)x;
      const double rs = xd / (1.0 + exp(-xd));
      const double rp = (xd > 0 ? xd : 0.0) + log1p(exp(-fabs(xd)));
      for (int de = -1; de <= 1; de++) {
        const double u = ulps(silu_model(x, de), rs);
        if (de == 0 && u > s0) { s0 = u; as0 = x; }
        if (u > s1) { s1 = u; as1 = x; }
        for (int dl = -1; dl <= 1; dl++) {
          const double v = ulps(softplus_model(x, de, dl), rp);
          if (de == 0 && dl == 0 && v > p0) { p0 = v; ap0 = x; }
          if (v > p1) { p1 = v; ap1 = x; }
        }
      }
    }
#pragma omp critical
    {
      if (s0 > silu0) { silu0 = s0; a_silu0 = as0; }
      if (s1 > silu1) { silu1 = s1; a_silu1 = as1; }
      if (p0 > sp0) { sp0 = p0; a_sp0 = ap0; }
      if (p1 > sp1) { sp1 = p1; a_sp1 = ap1; }
    }
  }
  printf("silu     correctly rounded libm: %.3f ulp at %a; libm within 1 ulp: %.3f ulp at %a\n", silu0, a_silu0, silu1, a_silu1);
  printf("softplus correctly rounded libm: %.3f ulp at %a; libm within 1 ulp: %.3f ulp at %a\n", sp0, a_sp0, sp1, a_sp1);
  return 0;
}
