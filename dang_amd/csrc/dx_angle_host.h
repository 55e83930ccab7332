// dx_angle_host.h -- the parts of the posterior polarisation angle (dangx_moments_angles, include/dangx.h) that need no device:
// the check of an angle list against the model's shape, the grouping of the angles into the segments k_moments_angle works on,
// the sample's two direction cosines, the read-out of one chain and of several.  dangx_moments.hip, dangx_chains.hip and every
// host-side check evaluate the SAME inline functions (contraction off, one fixed operation order), and a stand-alone host program
// can include this file without the HIP runtime.
//
// An angle is spec[a] = {comp, band}: the polarisation angle psi = atan2(U, Q) / 2 of the signal of component comp at that band.
// It is a circular quantity (psi and psi + pi are the same direction), so what is accumulated is the mean of the unit vector
// (c, s) = (cos 2 psi, sin 2 psi) = (sQ, sU) / P of every sample, sQ, sU, P being the signals' rounded samples (dx_signal_host.h).
// NO SIGN CONVENTION IS APPLIED: the angle is that of the Q, U maps as the model holds them (a caller whose maps follow the
// HEALPix convention and who wants IAU angles negates U, i.e. psi, as ever).
// P == 0 gives c = s = NaN and NaN stays in the accumulators: nothing is skipped, as for the signals.
// A segment is one component with at most DX_ANG_SEG_BANDS bands: a thread reads a pixel's Q and U amplitude and index values
// once per segment and evaluates the SED once per band and plane.
#pragma once
#include "dx_signal_host.h"

#define DX_ANG_MAX 64         // == DANGX_MAX_ANGLES (include/dangx.h)
#define DX_ANG_SEG_BANDS 8    // bands of one segment
#define DX_ANG_MAX_CHAINS 8   // == DANGX_MAX_CHAINS

// stat of a read-out; DX_ANG_BETWEEN over several chains only
enum { DX_ANG_MEAN = 0, DX_ANG_STD = 1, DX_ANG_R = 2, DX_ANG_C = 3, DX_ANG_S = 4, DX_ANG_BETWEEN = 5 };

// (cos 2 psi, sin 2 psi) of one sample from the two rounded signal samples: P as signal kind 3 forms it, two IEEE divisions
DX_HD void dx_angle_cs(double sq, double su, double& c, double& s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = dx_signal_pol(sq, su);
    c = sq / p;
    s = su / p;
}

// the running mean of k_moments_accum, without its m2: sample x, the new sample count's 1/n
DX_HD double dx_angle_mean(double x, double m, double inv_n) { return fma(x - m, inv_n, m); }

// mean resultant length, clamped: rounding can give 1 + eps where a chain never moved, whose std must be 0 and not NaN.
// Written as a comparison: fmin would drop a NaN, which has to propagate.
DX_HD double dx_angle_R(double C, double S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = C * C;
    const double b = S * S;
    const double r = sqrt(a + b);
    return r > 1.0 ? 1.0 : r;
}

// How far below 1 the resultant length of a chain that NEVER MOVED can come out, in units of u = 2^-53 (the spacing of doubles
// just below 1).  Every sample is then the same (c, s) and the running means are that pair exactly (fma(x - x, 1/n, x) = x).
// P = sqrt(fl(sQ^2) + fl(sU^2)) carries two rounded products and a rounded sum (2u on the argument, u after the root) and the
// root's own rounding: 2u.  c = sQ / P and s = sU / P add u each, so the true length of (c, s) lies within 3u of 1.  R is formed
// from (c, s) by the same four operations: 2u more.  Hence R >= 1 - 5u (R is a double, and the terms of second order are far
// less than the spacing u).  Above 1 the clamp of dx_angle_R has already cut.
#define DX_ANG_UNIT_SLACK 5

// circular standard deviation of psi (radians) of a resultant length: 0.5 sqrt(-2 log R); +inf at R = 0; exactly 0 where R is
// within the rounding of a unit vector's length of 1 (DX_ANG_UNIT_SLACK) -- the clamp alone gives 0 only where that rounding
// went up, and a chain that never moved would otherwise read 7.45e-9 rad in the pixels where it went down.  What is given up
// is nothing: below 0.5 sqrt(2 * 5u) = 1.7e-8 rad the expression returns the rounding of R, not a spread.  NaN propagates.
DX_HD double dx_angle_spread(double R) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (R >= 1.0 - DX_ANG_UNIT_SLACK * 0x1p-53) return 0.0;
    const double l = log(R);
    return 0.5 * sqrt(-2.0 * l);
}

// stats 0..4 of one chain's (or the pooled) pair
DX_HD double dx_angle_stat(int stat, double C, double S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (stat == DX_ANG_C) return C;
    if (stat == DX_ANG_S) return S;
    if (stat == DX_ANG_MEAN) return 0.5 * atan2(S, C);
    const double R = dx_angle_R(C, S);
    return stat == DX_ANG_R ? R : dx_angle_spread(R);
}

// ---- several chains

struct DxAngPar {             // what depends on the sample counts only, by value
    int K;
    int pad_;
    double w[DX_ANG_MAX_CHAINS];   // n_k / N
    double kd;                     // K
};

inline DxAngPar dx_angle_par(int K, const long long* n) {
    DxAngPar p{};
    p.K = K;
    long long N = 0;
    for (int k = 0; k < K && k < DX_ANG_MAX_CHAINS; ++k) N += n[k];
    for (int k = 0; k < K && k < DX_ANG_MAX_CHAINS; ++k) p.w[k] = (double)n[k] / (double)N;
    p.kd = (double)K;
    return p;
}

// f(k) for k0 <= k < min(K, DX_ANG_MAX_CHAINS) with k a constant in every copy (the device keeps the small arrays in registers)
template <int k, class F>
DX_HD void dx_angle_each(int K, F&& f) {
    if constexpr (k < DX_ANG_MAX_CHAINS) {
        if (k < K) f(k);
        dx_angle_each<k + 1>(K, f);
    }
}

// pooled mean of one plane: sum_k (n_k / N) x_k in list order, every product and every sum rounded
DX_HD double dx_angle_pool(const DxAngPar& p, const double (&x)[DX_ANG_MAX_CHAINS]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double acc = p.w[0] * x[0];
    dx_angle_each<1>(p.K, [&](int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double t = p.w[k] * x[k];
        acc = acc + t;
    });
    return acc;
}

// BETWEEN: the circular std of the chains' mean directions u_k = (C_k, S_k) / |(C_k, S_k)|
DX_HD double dx_angle_between(const DxAngPar& p, const double (&C)[DX_ANG_MAX_CHAINS], const double (&S)[DX_ANG_MAX_CHAINS]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double cb = 0.0, sb = 0.0;
    dx_angle_each<0>(p.K, [&](int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double a = C[k] * C[k];
        const double b = S[k] * S[k];
        const double r = sqrt(a + b);
        const double uc = C[k] / r, us = S[k] / r;
        cb = k == 0 ? uc : cb + uc;
        sb = k == 0 ? us : sb + us;
    });
    return dx_angle_spread(dx_angle_R(cb / p.kd, sb / p.kd));
}

// stats 0..5 of one element over the chains
DX_HD double dx_angle_chains_stat(int stat, const DxAngPar& p, const double (&C)[DX_ANG_MAX_CHAINS], const double (&S)[DX_ANG_MAX_CHAINS]) {
    if (stat == DX_ANG_BETWEEN) return dx_angle_between(p, C, S);
    return dx_angle_stat(stat, dx_angle_pool(p, C), dx_angle_pool(p, S));
}

// "" or why `stat` cannot be read from nchains chains (1: a single chain's read-out)
inline std::string dx_angle_stat_check(int stat, int nchains) {
    if (stat < DX_ANG_MEAN || stat > DX_ANG_BETWEEN)
        return "the stat of an angle must be 0 (circular mean), 1 (circular std), 2 (mean resultant length), 3 (mean cos 2psi), 4 (mean sin 2psi) "
               "or 5 (between-chain circular std)";
    if (stat == DX_ANG_BETWEEN && nchains < 2) return "stat 5 (between-chain circular std) needs several chains (dangx_chains_get_angle)";
    return "";
}

// ---- registration

struct DxAngSeg {
    int comp, nb;
    int band[DX_ANG_SEG_BANDS];
    int ang[DX_ANG_SEG_BANDS];    // the angle registered at that band
};

// spec[a] = {comp, band} against the model: set[l] != 0: component l is set, global[l] != 0: template / monopole / hi_fit member,
// tcmb[l] != 0: a T_cmb component.  "" = fine, else the cause.
inline std::string dx_angle_check(int nang, const int32_t* spec, int ncomp, int nbands, int nmaps, const int* set, const int* global,
                                  const int* tcmb) {
    if (nang < 0) return "the number of angles is negative";
    if (nang > DX_ANG_MAX) return "more than DANGX_MAX_ANGLES (" + std::to_string(DX_ANG_MAX) + ") angles";
    if (nang > 0 && !spec) return "no angle list given";
    if (nang > 0 && nmaps != 3) return "a polarisation angle needs Q and U: nmaps == 3";
    for (int a = 0; a < nang; ++a) {
        const int l = spec[2 * a], j = spec[2 * a + 1];
        const std::string at = "angle " + std::to_string(a) + ": ";
        if (l < 0 || l >= ncomp) return at + "component index out of range";
        if (!set[l]) return at + "the component is not set";
        if (j < 0 || j >= nbands) return at + "band index out of range";
        if (global[l]) return at + "a template / monopole / hi_fit member has one amplitude per band and a fixed map: its angle is the map's";
        if (tcmb[l]) return at + "the signal of a T_cmb component is a bare SED and has no direction";
        for (int o = 0; o < a; ++o)
            if (spec[2 * o] == l && spec[2 * o + 1] == j) return at + "the same angle twice";
    }
    return "";
}

// the segments of a checked list: components in ascending order, the bands of a component in ascending order, DX_ANG_SEG_BANDS
// to a segment
inline std::vector<DxAngSeg> dx_angle_plan(int nang, const int32_t* spec, int ncomp, int nbands) {
    std::vector<DxAngSeg> segs;
    for (int l = 0; l < ncomp; ++l) {
        DxAngSeg cur{l, 0, {}, {}};
        for (int j = 0; j < nbands; ++j)
            for (int a = 0; a < nang; ++a) {
                if (spec[2 * a] != l || spec[2 * a + 1] != j) continue;
                cur.band[cur.nb] = j;
                cur.ang[cur.nb++] = a;
                if (cur.nb == DX_ANG_SEG_BANDS) {
                    segs.push_back(cur);
                    cur = DxAngSeg{l, 0, {}, {}};
                }
            }
        if (cur.nb) segs.push_back(cur);
    }
    return segs;
}
