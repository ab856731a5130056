/* Host check of fmx_common.hpp's mdiv_rank (test infrastructure): the rank outputs' quotient
 * k / n for an integer numerator k = 2 #less + #equal - 1 in [0, 2 A] and n = 2 (len - 1),
 * from r = RN(1 / (len - 1)) / 2 -- q0 = RN(k r), rem = fma(-q0, n, k), q = fma(rem, r, q0)
 * -- with mdiv's exponent guard replaced by a test of the integer: k = 0 takes the IEEE
 * divide, every k >= 1 the three-operation path.  Checked bit for bit against (double)k / n,
 * and against mdiv with its exponent guard (the two must choose the same path):
 *   - every k in [0, 2 len] for every len in [2, LEN_FULL] (default 8200) and for the longest
 *     rows (len in [65436, 65535]): the guard boundary k = 0, k = 1 and k = 2 len included;
 *   - NR random (len, k) pairs with len up to 65535.
 * Exit status 0 = pass.
 *   gcc -O2 -ffp-contract=off -o mdiv_rank_check mdiv_rank_check.c -lm && ./mdiv_rank_check [LEN_FULL] [NR] */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static uint64_t ubits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

static int guard_old;                           /* mdiv's exponent guard fired */
static double mdiv(double x, double n, double r) {
  const double q0 = x * r;
  const uint32_t e = (uint32_t)(ubits(q0) >> 52) & 0x7ffu;
  guard_old = e - 64u > 1958u - 64u;
  if (guard_old) return x / n;
  const double rem = fma(-q0, n, x);
  return fma(rem, r, q0);
}
static double mdiv_rank(int k, double n, double r) {
  const double x = (double)k;
  if (k == 0) return x / n;
  const double q0 = x * r;
  const double rem = fma(-q0, n, x);
  return fma(rem, r, q0);
}

static long bad = 0, tot = 0;
static void one(int len, int k) {
  const double den = (double)(len - 1);
  const double rden = 1.0 / den;
  const double n = 2.0 * den, r = 0.5 * rden;
  const double a = mdiv_rank(k, n, r), b = mdiv((double)k, n, r), c = (double)k / n;
  ++tot;
  if (ubits(a) != ubits(c) || ubits(b) != ubits(c) || guard_old != (k == 0)) {
    if (bad < 10) fprintf(stderr, "mismatch len=%d k=%d: %a / %a vs %a (old guard %d)\n", len, k, a, b, c, guard_old);
    ++bad;
  }
}

int main(int argc, char** argv) {
  const int full = argc > 1 ? atoi(argv[1]) : 8200;
  const long nr = argc > 2 ? atol(argv[2]) : 30000000;
  for (int len = 2; len <= full; ++len)
    for (int k = 0; k <= 2 * len; ++k) one(len, k);
  for (int len = 65436; len <= 65535; ++len)
    for (int k = 0; k <= 2 * len; ++k) one(len, k);
  for (long i = 0; i < nr; ++i) {
    const int len = 2 + (int)(rnd() % 65534);
    one(len, (int)(rnd() % (2 * (uint64_t)len + 1)));
  }
  printf("mdiv_rank_check: %ld cases, %ld mismatches\n", tot, bad);
  return bad ? 1 : 0;
}
