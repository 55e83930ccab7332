// dx_moments_host.h -- the parts of the posterior pair / lag-1 statistics (dangx_moments_pairs) that need no device: the check of
// a pair list against the selection, and the lag-1 update and read-out expressions.  The kernels of dangx_moments.hip and the host
// mirror of the template-amplitude rows evaluate the SAME inline functions (explicit fma), and a stand-alone host program can
// include this file without the HIP runtime.
//
// Lag-1 state of one series x_1..x_n: r = x_1 (first sample), prev = x_n, P = sum_{t=2..n} (x_t - r)(x_{t-1} - r).  With the
// running mean and d = mean - r,
//     sum_{t=2..n} (x_t - mean)(x_{t-1} - mean) = P - (n + 1) d^2 + d (x_n - r)
// (expand with y_t = x_t - r, y_1 = 0, sum y_t = n d), so an offset |mean| >> spread costs no more than it costs the mean itself.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define DX_HD __host__ __device__ __forceinline__
#else
#define DX_HD inline
#endif

#define DX_MOM_MAX_PAIRS 64   // == DANGX_MAX_PAIRS (include/dangx.h)

// sample t >= 2 of a series (the first sample sets r = prev = x and leaves P = 0)
DX_HD void dx_lag_update(double x, double& prev, double r, double& P) {
    P = fma(x - r, prev - r, P);
    prev = x;
}

// rho1 = [sum_{t=2..n} (x_t - mean)(x_{t-1} - mean)] / m2; 0/0 = NaN for a series that never moved and for n = 1
DX_HD double dx_lag_rho1(double mean, double m2, double prev, double r, double P, double n) {
    const double d = mean - r;
    const double s = fma(d, prev - r, fma(-(n + 1.0) * d, d, P));
    return s / m2;
}

// AR(1) effective sample size n (1 - rho)/(1 + rho), rho = max(rho1, 0); NaN stays NaN
DX_HD double dx_lag_ess(double rho1, double n) {
    const double rho = rho1 < 0.0 ? 0.0 : rho1;
    return n * (1.0 - rho) / (1.0 + rho);
}

// pair term of one sample: C += (a - mean_a_old) (b - mean_b_new), mean_b_new by the fma of Welford's update
DX_HD double dx_pair_update(double a, double b, double ma, double mb, double C, double inv_n) {
    return fma(a - ma, b - fma(b - mb, inv_n, mb), C);
}

DX_HD double dx_pair_stat(double C, double m2a, double m2b, int stat, double dn) {
    return stat == 0 ? C / dn : C / sqrt(m2a * m2b);
}

// pairs[p] = {comp_a, what_a, plane_a, comp_b, what_b, plane_b} against the selection words sel[ncomp] (include/dangx.h),
// nind[l] = indices of component l, global[l] != 0: template / monopole / hi_fit member.  "" = fine, else the cause.
inline std::string dx_pairs_check(int npairs, const int32_t* pairs, int ncomp, int nmaps, const int32_t* sel, const int* nind, const int* global) {
    if (npairs < 0) return "the number of pairs is negative";
    if (npairs > DX_MOM_MAX_PAIRS) return "more than DANGX_MAX_PAIRS (" + std::to_string(DX_MOM_MAX_PAIRS) + ") pairs";
    if (npairs > 0 && !pairs) return "no pair list given";
    for (int p = 0; p < npairs; ++p) {
        const int32_t* q = pairs + 6 * p;
        const std::string at = "pair " + std::to_string(p) + ": ";
        for (int h = 0; h < 2; ++h) {
            const int l = q[3 * h], w = q[3 * h + 1], k = q[3 * h + 2];
            if (l < 0 || l >= ncomp) return at + "component index out of range";
            if (w < 0 || w > nind[l]) return at + "what must be 0 (amplitude) or 1 + index number of the component";
            if (k < 0 || k >= nmaps) return at + "plane out of range";
            if (w == 0 && global[l]) return at + "a template / monopole / hi_fit amplitude is not a pixel plane";
            if (!((sel[l] >> (w == 0 ? k : 3 + 3 * (w - 1) + k)) & 1)) return at + "a plane that is not selected";
        }
        if (q[0] == q[3] && q[1] == q[4] && q[2] == q[5]) return at + "a plane paired with itself (a == b)";
    }
    return "";
}
