// Which form of R_n each tap pair of the generic K_sinc tap loops uses (sinc_block.h, "tap loops"): the rule behind the per-NT
// tables of get_sinc_table (sinc.hip).  Host arithmetic on an integer, nothing of HIP: tests/sinc_tap_modes_table.cpp compiles
// this header alone and prints the rule as a table.
#pragma once
#include <math.h>
#include <vector>

namespace par {

constexpr int kChunk = 4;         // taps per chunk of the n loop: the forms change at chunk boundaries only
constexpr int kPoly2From = 5;     // rows n >= 5: (A_n, B_n, n, C_n) with A = win/(pi n^2), B = A/n^2, C = B/n^2
struct TapModes {
  int p1_from;                    // rows n >= p1_from: (A_n, B_n, n, -) linear minimax;  p1_from = 1 (mod kChunk), >= 5
  int p0_from;                    // rows n >= p0_from: (A_n, n A_n, n, -) constant;       p0_from = 1 (mod kChunk), >= p1_from
};
// worst-case error, summed over the pairs that use the form, against the 1e-5 the reference is matched to
constexpr double kPoly1Budget = 3.0e-7;      // linear minimax rows
constexpr double kPoly0Budget = 1.5e-6;      // constant rows

// Which polynomial form each tap pair uses (see TapModes): worst-case error of a pair = approximation error of R_n
// over q in [0, 1/4] times the largest the bracket n(G+H) + s(G-H) can get for unit-peak input, 2n + 1.  The forms
// start at the first chunk boundary from which the errors of ALL pairs further out sum to less than the budget.
inline void choose_tap_modes(int NT, TapModes* tm, std::vector<double>* lin_a, std::vector<double>* lin_b,
                             std::vector<double>* cst) {
  std::vector<double> e0(NT + kChunk, 0.0), e1(NT + kChunk, 0.0);
  lin_a->assign(NT + kChunk, 0.0);
  lin_b->assign(NT + kChunk, 0.0);
  cst->assign(NT + kChunk, 0.0);
  for (int n = 1; n < NT; ++n) {
    const double win = (double)(float)(0.5 + 0.5 * cos(M_PI * (double)n / (double)NT));
    const double K = win / M_PI, n2 = (double)n * (double)n;
    if (K <= 0.0) continue;
    const double f0 = K / n2, f1 = K / (n2 - 0.25);
    (*cst)[n] = 0.5 * (f0 + f1);                          // constant minimax: mid-range
    e0[n] = 0.5 * (f1 - f0) * (2.0 * n + 1.0);
    // linear minimax of the convex f(q) = K/(n^2 - q) on [0, 1/4]: chord slope, intercept halfway between the chord
    // and the parallel tangent (touching at q* with f'(q*) = slope)
    const double slope = (f1 - f0) / 0.25;
    const double qs = n2 - sqrt(K / slope);
    const double gap = (f0 + slope * qs) - K / (n2 - qs);
    (*lin_b)[n] = slope;
    (*lin_a)[n] = f0 - 0.5 * gap;
    e1[n] = 0.5 * gap * (2.0 * n + 1.0);
  }
  auto first_from = [&](const std::vector<double>& e, double budget) {
    int from = ((NT + kChunk) / kChunk) * kChunk + 1;     // beyond every chunk: form unused
    double tail = 0.0;
    for (int n0 = ((NT - 1) / kChunk) * kChunk + 1; n0 >= kPoly2From; n0 -= kChunk) {
      for (int n = n0; n < n0 + kChunk && n < NT; ++n) tail += e[n];
      if (tail > budget) break;
      from = n0;
    }
    return from;
  };
  tm->p1_from = first_from(e1, kPoly1Budget);
  tm->p0_from = first_from(e0, kPoly0Budget);
  if (tm->p0_from < tm->p1_from) tm->p0_from = tm->p1_from;
}

}  // namespace par
