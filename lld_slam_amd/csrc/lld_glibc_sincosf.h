// lld_glibc_sincosf.h — sinf / cosf as glibc >= 2.28 computes them (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, sincosf.h: the
// float argument widened to double, quadrant by the 2^24-prescaled 2/pi, one multiply-subtract with pi/2, degree-8 cosine /
// degree-7 sine polynomials in double, one rounding to float).  Constants checked against the libm.so.6 of glibc 2.35
// (__sincosf_table).  Only the branches reachable from |x| < 120 are restated: the descriptor's argument angle*factorPI lies in
// [0, 2pi).  Every double operation is a separately rounded multiply or add, so the host build (tools/check_sincosf.c, compiled
// with -ffp-contract=off) and the device build compute the same values; that tool compares both functions with the host's libm
// over every float angle in [0, 360).
#ifndef LLD_GLIBC_SINCOSF_H
#define LLD_GLIBC_SINCOSF_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LLD_SC_FN __host__ __device__ static inline
#if defined(__HIP_DEVICE_COMPILE__)
#define LLD_SC_MUL(a, b) __dmul_rn((a), (b))
#define LLD_SC_ADD(a, b) __dadd_rn((a), (b))
#endif
#else
#define LLD_SC_FN static inline
#endif
#ifndef LLD_SC_MUL
#define LLD_SC_MUL(a, b) ((a) * (b))
#define LLD_SC_ADD(a, b) ((a) + (b))
#endif

// sincos_t of glibc: {hpi_inv * 2^24, hpi, c0, c1, s1, c2, s2, c3, s3, c4}; entry 1 is used in quadrants 2 and 3
LLD_SC_FN double lld_sc_tab(int t, int i) {
  const double T0[10] = {0x1.45f306dc9c883p+23, 0x1.921fb54442d18p+0, 0x1p0, -0x1.ffffffd0c621cp-2, -0x1.555545995a603p-3,
                         0x1.55553e1068f19p-5, 0x1.1107605230bc4p-7, -0x1.6c087e89a359dp-10, -0x1.994eb3774cf24p-13, 0x1.99343027bf8c3p-16};
  const double T1[10] = {0x1.45f306dc9c883p+23, 0x1.921fb54442d18p+0, -0x1p0, 0x1.ffffffd0c621cp-2, -0x1.555545995a603p-3,
                         -0x1.55553e1068f19p-5, 0x1.1107605230bc4p-7, 0x1.6c087e89a359dp-10, -0x1.994eb3774cf24p-13, -0x1.99343027bf8c3p-16};
  return t ? T1[i] : T0[i];
}

LLD_SC_FN uint32_t lld_sc_abstop12(float f) { uint32_t u; memcpy(&u, &f, 4); return (u >> 20) & 0x7ffu; }

// sinf_poly: (n & 1) == 0 -> sine polynomial, else cosine
LLD_SC_FN float lld_sc_poly(double x, double x2, int t, int n) {
  if ((n & 1) == 0) {
    const double x3 = LLD_SC_MUL(x, x2);
    const double s1 = LLD_SC_ADD(lld_sc_tab(t, 6), LLD_SC_MUL(x2, lld_sc_tab(t, 8)));
    const double x7 = LLD_SC_MUL(x3, x2);
    const double s = LLD_SC_ADD(x, LLD_SC_MUL(x3, lld_sc_tab(t, 4)));
    return (float)LLD_SC_ADD(s, LLD_SC_MUL(x7, s1));
  }
  const double x4 = LLD_SC_MUL(x2, x2);
  const double c2 = LLD_SC_ADD(lld_sc_tab(t, 7), LLD_SC_MUL(x2, lld_sc_tab(t, 9)));
  const double c1 = LLD_SC_ADD(lld_sc_tab(t, 2), LLD_SC_MUL(x2, lld_sc_tab(t, 3)));
  const double x6 = LLD_SC_MUL(x4, x2);
  const double c = LLD_SC_ADD(c1, LLD_SC_MUL(x4, lld_sc_tab(t, 5)));
  return (float)LLD_SC_ADD(c, LLD_SC_MUL(x6, c2));
}

// cosine != 0: cosf(y), else sinf(y); valid for 0 <= y < 120
LLD_SC_FN float lld_glibc_sincosf(float y, int cosine) {
  double x = y;
  if (lld_sc_abstop12(y) < lld_sc_abstop12(0x1.921fb6p-1f)) {
    if (lld_sc_abstop12(y) < lld_sc_abstop12(0x1p-12f)) return cosine ? 1.0f : y;
    return lld_sc_poly(x, LLD_SC_MUL(x, x), 0, cosine ? 1 : 0);
  }
  const double r = LLD_SC_MUL(x, lld_sc_tab(0, 0));
  const int n = ((int32_t)r + 0x800000) >> 24;
  x = LLD_SC_ADD(x, -LLD_SC_MUL((double)n, lld_sc_tab(0, 1)));
  const double s = ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0;   // sign[4] = {1, -1, -1, 1}
  const int t = (n & 2) ? 1 : 0;
  return lld_sc_poly(LLD_SC_MUL(x, s), LLD_SC_MUL(x, x), t, cosine ? (n ^ 1) : n);
}

#endif
