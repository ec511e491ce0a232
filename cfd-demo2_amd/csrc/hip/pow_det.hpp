// pow_det(x > 0, y): x^y with the same bits on the host, on the device and in a
// numpy restatement (tests/visc_ref.py).  Library pow is not the same bits in
// those three; this is, because it uses only IEEE double + - * /, frexp, ldexp
// and rint, each exact or correctly rounded everywhere, in one fixed order
// (-ffp-contract=off: nothing is fused).
//
//   x = m 2^e,  m in [sqrt(1/2), sqrt(2))          frexp, one doubling
//   ln m = 2 t (1 + t^2/3 + ... + t^20/21),  t = (m - 1) / (m + 1)      Horner, kPowDetLnTerms = 10
//   L = y (e ln2 + ln m)
//   k = rint(L / ln2),  r = L - k ln2;  exp r = 1 + r (1 + r/2 (1 + ... r/13))   Horner, kPowDetExpDegree = 13
//   x^y = ldexp(exp r, k)
//
// Truncation.  |t| <= (sqrt 2 - 1) / (sqrt 2 + 1) = 0.172, t^2 <= 0.0295: the
// first dropped term of the logarithm's series is t^22 / 23 <= 7e-19 of the
// leading one (the tail is below 1.04 times it).  |r| <= ln2 / 2 = 0.347: the
// first dropped term of the exponential is r^14 / 14! <= 4.3e-18 (tail below
// 1.03 times it).  Together below 1e-17 (1 + |L|) relative: nine decades under
// float32's epsilon of 6e-8.  Rounding: about a dozen operations of at most
// 2^-53 each in either series, and the absolute error of L and of k ln2, a few
// 2^-53 |L|, becomes a relative error of the result.  The stated bound, which
// tests/test_visc.py holds it to against math.pow:
//   |pow_det(x, y) - x^y| <= (16 + 8 |y ln x|) 2^-53 x^y
// With |y ln x| <= 10 in both viscosity models that is 1.1e-14.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CFD_POW_DET_HD __host__ __device__
#else
#define CFD_POW_DET_HD
#endif

namespace cfd2 {

constexpr int kPowDetLnTerms = 10;    // the series of ln m runs to t^(2 * 10) / 21
constexpr int kPowDetExpDegree = 13;  // the series of exp r runs to r^13 / 13!
constexpr double kPowDetLn2 = 0.6931471805599453;     // 0x3FE62E42FEFA39EF
constexpr double kPowDetSqrtHalf = 0.7071067811865476;  // 0x3FE6A09E667F3BCD

CFD_POW_DET_HD inline double pow_det(double x, double y) {
  int e;
  double m = frexp(x, &e);  // [1/2, 1)
  if (m < kPowDetSqrtHalf) {
    m = m * 2.0;
    e -= 1;
  }
  const double t = (m - 1.0) / (m + 1.0), t2 = t * t;
  double s = 1.0 / (double)(2 * kPowDetLnTerms + 1);
  for (int k = kPowDetLnTerms - 1; k >= 0; --k) s = s * t2 + 1.0 / (double)(2 * k + 1);
  const double lnm = 2.0 * t * s;
  const double L = y * ((double)e * kPowDetLn2 + lnm);
  const double k = rint(L / kPowDetLn2);
  const double r = L - k * kPowDetLn2;
  double p = 1.0;
  for (int j = kPowDetExpDegree; j >= 1; --j) p = 1.0 + r * p / (double)j;
  return ldexp(p, (int)k);
}

}  // namespace cfd2
