// xk_chi2_quantile.h -- chi-square quantile on the HOST for the degrees of freedom the table (xk_chi2_table.h) does not reach:
// boost::math::quantile(chi_squared(dof), p) = 2 P^-1(dof / 2, p), P the regularised lower incomplete gamma function.  A persistent
// feature's track grows by one observation per frame for as long as the feature lives (slam_update.cpp:196-199 takes the quantile at
// dof = 2 * track size), so its dof has no bound; no device code computes quantiles.
#pragma once
#include <cmath>

// P(a, x): the series below x < a + 1, the continued fraction of Q = 1 - P (modified Lentz) above.  Near x = a either one takes
// O(sqrt(a)) terms, hence the generous caps.
static inline double xk_gamma_p(double a, double x) {
  if (!(x > 0.0)) return 0.0;
  const double lead = std::exp(a * std::log(x) - x - std::lgamma(a));
  if (x < a + 1.0) {
    double ap = a, term = 1.0 / a, sum = term;
    for (int i = 0; i < 200000; ++i) {
      ap += 1.0;
      term *= x / ap;
      sum += term;
      if (term < sum * 1e-17) break;
    }
    return sum * lead;
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, f = d;
  for (int i = 1; i < 200000; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (std::fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double step = d * c;
    f *= step;
    if (std::fabs(step - 1.0) < 1e-16) break;
  }
  return 1.0 - lead * f;
}

// -> x with P(dof / 2, x / 2) = p, or NaN for p outside (0, 1) or dof < 1.  Newton from the Wilson-Hilferty estimate, every step kept
// inside the bracket the signs seen so far leave (bisection, or doubling while there is no upper end yet).
static inline double xk_chi2_quantile_host(double p, int dof) {
  if (!(p > 0.0 && p < 1.0) || dof < 1) return std::nan("");
  const double a = 0.5 * dof;
  double zlo = -40.0, zhi = 40.0;             // standard normal quantile of p by bisection (a start value only)
  for (int i = 0; i < 100; ++i) {
    const double zm = 0.5 * (zlo + zhi);
    if (0.5 * std::erfc(-zm * M_SQRT1_2) < p) zlo = zm; else zhi = zm;
  }
  const double z = 0.5 * (zlo + zhi), s = 2.0 / (9.0 * dof), t = 1.0 - s + z * std::sqrt(s);
  double x = dof * t * t * t;
  if (!(x > 0.0)) x = 1e-3;
  double lo = 0.0, hi = INFINITY;
  for (int it = 0; it < 200; ++it) {
    const double f = xk_gamma_p(a, 0.5 * x) - p;
    if (f > 0.0) hi = x; else lo = x;
    const double pdf = 0.5 * std::exp((a - 1.0) * std::log(0.5 * x) - 0.5 * x - std::lgamma(a));
    double xn = x - f / pdf;
    if (!(xn > lo && xn < hi)) xn = std::isinf(hi) ? 2.0 * x : 0.5 * (lo + hi);
    const bool done = std::fabs(xn - x) <= 4e-16 * std::fabs(xn);
    x = xn;
    if (done) break;
  }
  return x;
}
