// Pareto-smoothed importance sampling of one dyad's tail (Vehtari, Simpson, Gelman, Yao & Gabry; the fit of
// Zhang & Stephens 2009 as the R package loo's gpdfit does it, r_eff = 1): plain C++ for the host and the device
// (k_loo_accumulate, kernels_loo.hpp; tests/cpp/check_psis_tail.cpp on the CPU), as ccs_plan.hpp and pipe_plan.hpp.
//
// A tail is given by a callable l(i), i = 0..M: the M + 1 smallest pointwise log-likelihoods of the dyad in
// ascending order.  With c = l(0) the log ratios are lr = c - l <= 0; l(0..M-1) are the tail (the M largest lr),
// l(M) is the cutoff.  In ascending order of lr, lr_(m) = c - l(M - m), m = 1..M.
//
//     x_m = exp(lr_(m)) - exp(lr_cut) (psis_x),  G = 30 + floor(sqrt(M)),  xstar = x_q, q = floor(M/4 + 0.5)
//     theta_j = 1/x_M + (1 - sqrt(G/(j - 0.5))) / (3 xstar),  k_j = mean_m log1p(-theta_j x_m),
//     L_j = M (log(-theta_j/k_j) - k_j - 1),  w_j = 1 / sum_i exp(L_i - L_j),  theta = sum_j w_j theta_j,
//     k = mean_m log1p(-theta x_m),  sigma = -k/theta,  k <- (M k + 5)/(M + 10)
//     lw_(m) = min(0, log(exp(lr_cut) + sigma expm1(-k log1p(-p_m))/k)),  p_m = (m - 0.5)/M
//
// The weights w_j are a softmax of L_j; they are summed in one sweep over j with a running maximum (nothing of
// length G is stored), which is the same quantity rounded in another order.  A tail is not fitted (k = +inf, the
// raw lr are kept) if M < 5, if lr_(M) - lr_(1) < DBL_EPSILON/100, if xstar <= 0 or if any theta_j, k_j, L_j, theta,
// k or sigma is not finite.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PSIS_HD __host__ __device__ inline
#else
#define PSIS_HD inline
#endif

namespace dlsm {

constexpr double PSIS_MIN_SPREAD = 2.220446049250313e-16 / 100.0;      // DBL_EPSILON / 100
constexpr int PSIS_MIN_TAIL = 5;

// M = min(floor(S/5), ceil(3 sqrt(S))), in integers: the smallest c with c c >= 9 S
PSIS_HD int psis_tail_length(long long S) {
    long long c = (long long)(3.0 * sqrt((double)S));
    while (c * c < 9 * S) ++c;
    while (c > 0 && (c - 1) * (c - 1) >= 9 * S) --c;
    const long long f = S / 5;
    return (int)(f < c ? f : c);
}

PSIS_HD bool psis_finite(double v) { return fabs(v) < __builtin_inf(); }

// one more term v of a streaming log-sum-exp m + log(r) (empty: m = -inf, r = 0); v = -inf adds nothing
PSIS_HD void psis_lse_add(double &m, double &r, double v) {
    if (v == -__builtin_inf()) return;
    const double d = v - m;
    const double e = exp(-fabs(d));
    r = d > 0.0 ? fma(r, e, 1.0) : r + e;
    m = fmax(m, v);
}

struct PsisFit {
    double k, sigma, ecut;        // the adjusted shape (+inf: not fitted), the scale, exp(lr_cut)
    bool fitted;
};

// x = exp(c - li) - exp(c - lcut) of a tail value li <= lcut, ecut = exp(c - lcut): the difference as the definition
// writes it.  (Not ecut expm1(lcut - li), which is the more accurate near the cutoff: for a tail value 1e-70 below
// the cutoff it is positive where every evaluation of the definition in float64 or in extended precision gives 0,
// and xstar == 0 decides fitted / unfitted - measured on saturated dyads, |eta| of 800: a fifth of them changed
// class.)
PSIS_HD double psis_x(double c, double li, double ecut) { return exp(c - li) - ecut; }

// mean_m log1p(-theta x_m) of the tail l (c = l(0), ecut = exp(c - l(M)))
template <class Tail>
PSIS_HD double psis_mean_log1p(const Tail &l, int M, double c, double ecut, double theta) {
    double sum = 0.0;
    for (int m = 1; m <= M; ++m) sum += log1p(-theta * psis_x(c, l(M - m), ecut));
    return sum / (double)M;
}

template <class Tail>
PSIS_HD PsisFit psis_fit(const Tail &l, int M) {
    PsisFit f;
    f.k = __builtin_inf(); f.sigma = 0.0; f.ecut = 0.0; f.fitted = false;
    if (M < PSIS_MIN_TAIL) return f;
    const double c = l(0), lcut = l(M);
    const double ecut = exp(c - lcut);
    f.ecut = ecut;
    if (!(l(M - 1) - c >= PSIS_MIN_SPREAD)) return f;         // lr_(M) - lr_(1), lr_(M) = 0
    int sq = 0;
    while ((sq + 1) * (sq + 1) <= M) ++sq;
    const int G = 30 + sq, q = (M + 2) / 4;
    const double dG = (double)G, dM = (double)M;
    const double xM = psis_x(c, c, ecut), xstar = psis_x(c, l(M - q), ecut);
    if (!(xstar > 0.0)) return f;
    double lmax = -__builtin_inf(), den = 0.0, num = 0.0;     // sum_j exp(L_j - lmax) (1, theta_j)
    for (int j = 1; j <= G; ++j) {
        const double theta_j = 1.0 / xM + (1.0 - sqrt(dG / ((double)j - 0.5))) / (3.0 * xstar);
        const double k_j = psis_mean_log1p(l, M, c, ecut, theta_j);
        const double L_j = dM * (log(-theta_j / k_j) - k_j - 1.0);
        if (!(psis_finite(theta_j) && psis_finite(k_j) && psis_finite(L_j))) return f;
        const double d = L_j - lmax;
        const double e = exp(-fabs(d));
        if (d > 0.0) { den = fma(den, e, 1.0); num = fma(num, e, theta_j); lmax = L_j; }
        else { den += e; num = fma(e, theta_j, num); }
    }
    const double theta = num / den;
    const double k = psis_mean_log1p(l, M, c, ecut, theta);
    const double sigma = -k / theta;
    if (!(psis_finite(theta) && psis_finite(k) && psis_finite(sigma))) return f;
    f.k = (dM * k + 5.0) / (dM + 10.0);
    f.sigma = sigma;
    f.fitted = true;
    return f;
}

// the smoothed log weight lw_(m), m = 1..M, of a fitted tail
PSIS_HD double psis_smoothed(const PsisFit &f, int m, int M) {
    const double lp = log1p(-((double)m - 0.5) / (double)M);
    const double qv = f.k == 0.0 ? -f.sigma * lp : f.sigma * expm1(-f.k * lp) / f.k;
    return fmin(0.0, log(f.ecut + qv));
}

}  // namespace dlsm
