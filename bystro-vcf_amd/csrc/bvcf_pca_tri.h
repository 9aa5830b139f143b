#pragma once
// bvcf_pca_tri.h — the top eigenpairs of a symmetric tridiagonal matrix, the host step between the two device steps of
// --pca (bvcf_pca.hip.h: Householder tridiagonalisation in front, back-transformation behind).  Plain C++17, no HIP.
//
// T has the diagonal d[0, n) and the off-diagonal e[0, n-1).  pca_tri::solve gives the k algebraically largest eigenvalues,
// descending, and a unit-norm vector for each:
//   values   Sturm-count bisection inside the Gershgorin interval, run until the interval cannot shrink (its midpoint is one of
//            its ends): the count of eigenvalues below x is the number of negative q_i in q_0 = d_0 - x,
//            q_i = d_i - x - e_{i-1}^2 / q_{i-1}, a q_i inside +-pivmin taken as -pivmin.  An interval that straddles 0 halves
//            down through the subnormals, about 1 100 steps: only a tridiagonal with an exactly zero eigenvalue among its top
//            k pays that.
//   vectors  inverse iteration: T - lambda I is factored once by elimination with row interchanges, a pivot inside +-pivot_min
//            replaced by +-pivot_min (the shifted matrix is singular to working precision: that is the point); kIters times
//            the start vector is solved for, made orthogonal by modified Gram-Schmidt (two passes) to the vectors already found
//            whose eigenvalue lies within the cluster threshold, and normalised.  The start vector of vector a comes from a fixed
//            generator seeded with a, so two vectors of one cluster start differently and the result is a function of
//            (d, e, n, k) alone.
// The matrix is scaled by a power of two (exact) so that its largest entry lies in [1, 2): thresholds are then plain
// numbers and the solves cannot overflow from a tiny norm; the values are scaled back.  e_i = 0 needs no special case: the
// count and the factorisation both run over a block-diagonal matrix as over any other, and a vector then lives in the blocks
// that hold its eigenvalue (up to rounding).  n = 1, 2 and the zero matrix work: the zero matrix gives zeros and the unit
// vectors e_0 .. e_{k-1}.  Every output is finite for finite input.
//
// No contraction: a*b+c is two roundings on every compiler, so the bytes do not depend on the host's FMA support.
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#pragma STDC FP_CONTRACT OFF

namespace pca_tri {

constexpr int kIters = 5;                    // solves per vector: two reach working precision for a separated eigenvalue,
                                             // the rest let Gram-Schmidt settle inside a cluster
constexpr double kEps = 0x1p-52;
constexpr double kBig = 0x1p500, kSmall = 0x1p-500;  // a solve that grows past kBig is scaled by kSmall as a whole

// the cluster threshold over the scaled matrix of one-norm `norm1`: two eigenvalues nearer than this share a Gram-Schmidt
// group.  1e-3 of the norm is LAPACK dstein's; norm1 / n keeps U^T U - I inside n 2^-52 for the small n where 1e-3 would let
// a vector carry 10^3 roundings of its neighbour
inline double cluster_threshold(double norm1, uint32_t n) { return norm1 * std::max(1e-3, 1.0 / (double)n); }

// the number of eigenvalues of (d, e) below x
inline uint32_t count_below(const double *d, const double *e, uint32_t n, double x, double pivmin) {
  uint32_t c = 0;
  double q = d[0] - x;
  if (fabs(q) < pivmin) q = -pivmin;
  c += q < 0.0;
  for (uint32_t i = 1; i < n; i++) {
    q = d[i] - x - e[i - 1] * e[i - 1] / q;
    if (fabs(q) < pivmin) q = -pivmin;
    c += q < 0.0;
  }
  return c;
}

// splitmix64 -> a double in [-1, 1) that is never 0 (the low bit of the 53 is set)
struct Rng {
  uint64_t s;
  double next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(int64_t)((z >> 11) | 1ull) * 0x1p-52 - 1.0;
  }
};

// T - lambda I = P L U: u0 the diagonal of U, u1 / u2 its two superdiagonals, l the multipliers, sw[i] = rows i and i + 1
// were interchanged before column i was eliminated
struct Lu {
  std::vector<double> u0, u1, u2, l;
  std::vector<uint8_t> sw;
};

inline double guard_pivot(double p, double pivot_min) { return fabs(p) < pivot_min ? (p < 0.0 ? -pivot_min : pivot_min) : p; }

inline void factor(const double *d, const double *e, uint32_t n, double lambda, double pivot_min, Lu &f) {
  f.u0.assign(n, 0.0);
  f.u1.assign(n, 0.0);
  f.u2.assign(n, 0.0);
  f.l.assign(n, 0.0);
  f.sw.assign(n, 0);
  double cur_d = d[0] - lambda, cur_u = n > 1 ? e[0] : 0.0;
  for (uint32_t i = 0; i + 1 < n; i++) {
    const double sub = e[i], next_d = d[i + 1] - lambda, next_u = i + 2 < n ? e[i + 1] : 0.0;
    if (fabs(cur_d) >= fabs(sub)) {
      const double piv = guard_pivot(cur_d, pivot_min), m = sub / piv;
      f.u0[i] = piv;
      f.u1[i] = cur_u;
      f.l[i] = m;
      cur_d = next_d - m * cur_u;
      cur_u = next_u;
    } else {
      const double piv = guard_pivot(sub, pivot_min), m = cur_d / piv;
      f.u0[i] = piv;
      f.u1[i] = next_d;
      f.u2[i] = next_u;
      f.l[i] = m;
      f.sw[i] = 1;
      cur_d = cur_u - m * next_d;
      cur_u = -(m * next_u);
    }
  }
  f.u0[n - 1] = guard_pivot(cur_d, pivot_min);
}

// x <- (P L U)^-1 x, up to a power of two
inline void solve_lu(const Lu &f, uint32_t n, double *x) {
  for (uint32_t i = 0; i + 1 < n; i++) {
    if (f.sw[i]) std::swap(x[i], x[i + 1]);
    x[i + 1] -= f.l[i] * x[i];
  }
  for (uint32_t i = n; i-- > 0;) {
    double v = x[i];
    if (i + 1 < n) v -= f.u1[i] * x[i + 1];
    if (i + 2 < n) v -= f.u2[i] * x[i + 2];
    v /= f.u0[i];
    x[i] = v;
    if (fabs(v) > kBig)  // (the system is linear: what is solved and what is still right-hand side scale together)
      for (uint32_t t = 0; t < n; t++) x[t] *= kSmall;
  }
}

// x / ||x||, through the largest magnitude so that the squares neither overflow nor vanish; false for a zero or non-finite x
inline bool normalise(double *x, uint32_t n) {
  double m = 0.0;
  for (uint32_t i = 0; i < n; i++) m = std::max(m, fabs(x[i]));
  if (!(m > 0.0) || !std::isfinite(m)) return false;
  double s = 0.0;
  for (uint32_t i = 0; i < n; i++) {
    x[i] /= m;
    s += x[i] * x[i];
  }
  s = sqrt(s);
  for (uint32_t i = 0; i < n; i++) x[i] /= s;
  return true;
}

// values[0, k) descending, z[a * n, (a + 1) * n) the unit vector of values[a].  0, or -1 for bad arguments (n == 0, k == 0,
// k > n, a non-finite entry)
inline int solve(const double *d_in, const double *e_in, uint32_t n, uint32_t k, double *values, double *z) {
  if (!d_in || (!e_in && n > 1) || !values || !z || n == 0 || k == 0 || k > n) return -1;
  double amax = 0.0;
  for (uint32_t i = 0; i < n; i++) {
    if (!std::isfinite(d_in[i]) || (i + 1 < n && !std::isfinite(e_in[i]))) return -1;
    amax = std::max(amax, fabs(d_in[i]));
    if (i + 1 < n) amax = std::max(amax, fabs(e_in[i]));
  }
  if (amax == 0.0) {
    for (uint32_t a = 0; a < k; a++) {
      values[a] = 0.0;
      for (uint32_t i = 0; i < n; i++) z[(size_t)a * n + i] = i == a ? 1.0 : 0.0;
    }
    return 0;
  }
  int ex = 0;
  (void)frexp(amax, &ex);  // amax = f 2^ex, f in [0.5, 1): entries times 2^(1 - ex) have their largest in [1, 2)
  std::vector<double> d(n), e(n > 1 ? n - 1 : 0);
  for (uint32_t i = 0; i < n; i++) d[i] = ldexp(d_in[i], 1 - ex);
  for (uint32_t i = 0; i + 1 < n; i++) e[i] = ldexp(e_in[i], 1 - ex);

  double gl = d[0], gu = d[0], norm1 = 0.0;
  for (uint32_t i = 0; i < n; i++) {
    const double r = (i ? fabs(e[i - 1]) : 0.0) + (i + 1 < n ? fabs(e[i]) : 0.0);
    gl = std::min(gl, d[i] - r);
    gu = std::max(gu, d[i] + r);
    norm1 = std::max(norm1, fabs(d[i]) + r);
  }
  // (the largest entry is at least 1: plain multiples of the rounding unit serve as the smallest pivots)
  const double pivmin = 0x1p-1000, pivot_min = kEps * norm1, slack = 2.0 * kEps * norm1 * (double)n + 2.0 * pivmin;
  gl -= slack;
  gu += slack;

  // eigenvalue a (descending) is number m = n - 1 - a ascending: the largest x with count_below(x) <= m
  for (uint32_t a = 0; a < k; a++) {
    const uint32_t m = n - 1 - a;
    double lo = gl, hi = a ? std::min(gu, values[a - 1]) : gu;  // count_below(lo) <= m < count_below(hi), or hi is a known bound
    if (hi < lo) hi = lo;
    for (;;) {
      const double mid = lo + (hi - lo) / 2.0;
      if (!(mid > lo) || !(mid < hi)) break;
      if (count_below(d.data(), e.data(), n, mid, pivmin) <= m)
        lo = mid;
      else
        hi = mid;
    }
    values[a] = hi;
  }
  // (a later value is bisected below an earlier one's lower end: the sequence is descending by construction)

  const double thr = cluster_threshold(norm1, n);
  Lu f;
  std::vector<double> x(n);
  for (uint32_t a = 0; a < k; a++) {
    double *za = z + (size_t)a * n;
    uint32_t first = a;  // vectors first .. a - 1 are this one's cluster: a chain of neighbours each within thr
    while (first > 0 && values[first - 1] - values[first] <= thr) first--;
    factor(d.data(), e.data(), n, values[a], pivot_min, f);
    Rng rng{0x5EEDull * 0x100000001B3ull + a};
    for (uint32_t i = 0; i < n; i++) x[i] = rng.next();
    for (int it = 0; it < kIters; it++) {
      solve_lu(f, n, x.data());
      bool ok = normalise(x.data(), n);
      // (twice: the solve grows the directions already found again, what the first pass leaves of x is then small against what
      // it removed and carries that cancellation; the second pass works on a normalised vector that is orthogonal to rounding)
      for (int pass = 0; pass < 2 && ok && first < a; pass++) {
        for (uint32_t b = first; b < a; b++) {
          const double *zb = z + (size_t)b * n;
          double dot = 0.0;
          for (uint32_t i = 0; i < n; i++) dot += zb[i] * x[i];
          for (uint32_t i = 0; i < n; i++) x[i] -= dot * zb[i];
        }
        ok = normalise(x.data(), n);
      }
      if (!ok) {  // (the start lay in the span already found, to rounding: the next numbers of the same generator)
        for (uint32_t i = 0; i < n; i++) x[i] = rng.next();
      }
    }
    if (!normalise(x.data(), n)) {
      for (uint32_t i = 0; i < n; i++) x[i] = i == a ? 1.0 : 0.0;
    }
    for (uint32_t i = 0; i < n; i++) za[i] = x[i];
  }
  for (uint32_t a = 0; a < k; a++) values[a] = ldexp(values[a], ex - 1);
  return 0;
}

}  // namespace pca_tri
