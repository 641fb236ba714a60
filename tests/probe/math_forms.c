/* tests/probe/math_forms.c — csrc/macm_math.h against its earlier forms (macm_math_parent.h, kept
 * verbatim), both built for the host in one library (tests/test_math_forms.py, ctypes):
 *   gcc -O2 -shared -fPIC -ffp-contract=off -I gym-macm_amd/csrc tests/probe/math_forms.c -lm -o LIB
 * Every comparison is on bits. Each function returns the number of mismatching inputs and stores
 * the first one. */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "macm_math.h"

/* the earlier forms under other names: the two headers define the same functions and tables */
#define macm_sincos parent_macm_sincos
#define macm_sincos_pair parent_macm_sincos_pair
#define macm_action_trig_raw parent_macm_action_trig_raw
#define macm_action_trig parent_macm_action_trig
#define obs_atan2_core parent_obs_atan2_core
#define obs_atan2_finish parent_obs_atan2_finish
#define obs_atan2 parent_obs_atan2
#define kTrigFixNear parent_kTrigFixNear
#define kTrigFixFar parent_kTrigFixFar
#include "macm_math_parent.h"
#undef macm_sincos
#undef macm_sincos_pair
#undef macm_action_trig_raw
#undef macm_action_trig
#undef obs_atan2_core
#undef obs_atan2_finish
#undef obs_atan2
#undef kTrigFixNear
#undef kTrigFixFar

static int same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
static int samef(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

/* obs_atan2(y, x), and the split form the TDM pair lanes use (one core, both directions) */
size_t forms_atan2_n(const double* y, const double* x, size_t n, size_t* first) {
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) {
    int ok = same(obs_atan2(y[i], x[i]), parent_obs_atan2(y[i], x[i]));
    const double cn = obs_atan2_core(fabs(x[i]), fabs(y[i])), cp = parent_obs_atan2_core(fabs(x[i]), fabs(y[i]));
    ok &= same(obs_atan2_finish(cn, -y[i], -x[i]), parent_obs_atan2_finish(cp, -y[i], -x[i]));
    if (!(x[i] == 0.0 && y[i] == 0.0)) ok &= same(cn, cp); /* 0 / 0: the core's NaN is replaced by finish */
    if (!ok && bad++ == 0) *first = i;
  }
  return bad;
}

/* the earlier obs_atan2 alone: the reference of tests/test_gpu_f64_forms.py */
void forms_parent_atan2_n(const double* y, const double* x, double* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = parent_obs_atan2(y[i], x[i]);
}

/* the current obs_atan2 alone: the atan2 of tests/tdm_obs_ref.py */
void forms_obs_atan2_n(const double* y, const double* x, double* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = obs_atan2(y[i], x[i]);
}

/* the float32 quantities the step derives from the four doubles: every (k0, k1), cc = 1 and
 * 1/sqrt(2), F = 20 and 16, and the melee-ray offsets (range 2) */
static int forces_same(const double* p, const double* q) {
  static const double kCc[2] = {1.0, 7.07106781186547461715e-01}, kF[2] = {20.0, 16.0};
  int ok = 1;
  for (int k0 = -1; k0 <= 1; ++k0)
    for (int k1 = -1; k1 <= 1; ++k1)
      for (int c = 0; c < 2; ++c)
        for (int f = 0; f < 2; ++f) {
          ok &= samef((float)((p[1] * k0 + p[3] * k1) * kCc[c] * kF[f]), (float)((q[1] * k0 + q[3] * k1) * kCc[c] * kF[f]));
          ok &= samef((float)((p[0] * k0 + p[2] * k1) * kCc[c] * kF[f]), (float)((q[0] * k0 + q[2] * k1) * kCc[c] * kF[f]));
        }
  ok &= samef((float)(2.0 * p[1]), (float)(2.0 * q[1])) & samef((float)(2.0 * p[0]), (float)(2.0 * q[0]));
  return ok;
}

static int trig_same(float a) {
  double p[4], q[4];
  macm_action_trig(a, &p[0], &p[1], &p[2], &p[3]);
  parent_macm_action_trig(a, &q[0], &q[1], &q[2], &q[3]);
  int ok = same(p[0], q[0]) & same(p[1], q[1]) & same(p[2], q[2]) & same(p[3], q[3]);
  if (fabsf(a) < 4.0f) { /* the pair form itself, without the table on top */
    double u[4], v[4];
    macm_sincos_pair((double)a, &u[0], &u[1], &u[2], &u[3]);
    parent_macm_sincos_pair((double)a, &v[0], &v[1], &v[2], &v[3]);
    ok &= same(u[0], v[0]) & same(u[1], v[1]) & same(u[2], v[2]) & same(u[3], v[3]);
  }
  return ok & forces_same(p, q);
}

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

/* every float32 with bits lo, lo + stride, ... <= hi, and its negative */
size_t forms_trig_bits(uint32_t lo, uint32_t hi, uint32_t stride, uint32_t* first) {
  size_t bad = 0;
  for (uint64_t u = lo; u <= hi; u += stride) {
    const int ok = trig_same(from_bits((uint32_t)u)) & trig_same(from_bits((uint32_t)u | 0x80000000u));
    if (!ok && bad++ == 0) *first = (uint32_t)u;
  }
  return bad;
}

size_t forms_trig_n(const float* a, size_t n, size_t* first) {
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i)
    if (!trig_same(a[i]) && bad++ == 0) *first = i;
  return bad;
}
