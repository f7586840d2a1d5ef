/* Compares the sinf / cosf restatement the descriptor kernel uses (lld_slam_amd/csrc/lld_glibc_sincosf.h, compiled here for the
 * host with -ffp-contract=off, i.e. the same separately rounded operations as the device build) with the host's libm for every
 * float angle in [0, 360) (or every k-th one: first argument), on the argument computeOrbDescriptor forms: angle * factorPI.
 *   gcc -O2 -ffp-contract=off -I lld_slam_amd/csrc tools/check_sincosf.c -o check_sincosf -lm && ./check_sincosf */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lld_glibc_sincosf.h"

int main(int argc, char** argv) {
  const unsigned stride = argc > 1 ? (unsigned)strtoul(argv[1], NULL, 10) : 1u;
  const float factor_pi = (float)(3.14159265358979323846 / 180.0);
  const float lim = 360.f;
  uint32_t hi; memcpy(&hi, &lim, 4);
  long n = 0, nc = 0, ns = 0;
  for (uint32_t u = 0; u < hi; u += stride) {
    float ang; memcpy(&ang, &u, 4);
    volatile float arg = ang * factor_pi;
    const float a = cosf(arg), b = sinf(arg), ma = lld_glibc_sincosf(arg, 1), mb = lld_glibc_sincosf(arg, 0);
    if (memcmp(&a, &ma, 4)) { if (nc < 5) printf("cos differs: angle %a arg %a libm %a restated %a\n", ang, arg, a, ma); nc++; }
    if (memcmp(&b, &mb, 4)) { if (ns < 5) printf("sin differs: angle %a arg %a libm %a restated %a\n", ang, arg, b, mb); ns++; }
    n++;
  }
  printf("angles %ld cos_diff %ld sin_diff %ld\n", n, nc, ns);
  return (nc || ns) ? 1 : 0;
}
