// dx_rank_host.h -- the definitions of the rank-normalised and the folded R-hat (Vehtari, Gelman, Simpson, Carpenter and Buerkner,
// Bayesian Analysis 16 (2021) 667) read from the per-pixel histograms of SEVERAL chains (dangx_chains_hist_rank, include/dangx.h).
// k_chains_rank of dangx_chains.hip, every host-side check and a stand-alone host program evaluate the SAME inline functions
// (explicit fma, one fixed operation order), and this file needs no HIP runtime.
//
// The samples of one bin are ties and ties take the average rank, so a pixel's K records are a sufficient statistic of the
// rank-normalised R-hat of the binned trace: nothing is approximated beyond the bin width.
//
// Chain k of K holds the counters c[k][b], b = 0 .. nbins-1 (dx_hist_count).  C[b] = sum_k c[k][b] in 64-bit integers,
// S = sum_b C[b], cum[b] = sum_{b' < b} C[b'].
//   score of a non-empty bin: twice its mid-rank is the integer u = 2 cum[b] + C[b] + 1; u' = min(u, 2S + 2 - u);
//       p = (u' - 0.75) / (2S + 0.5)   -- Blom's (r - 3/8) / (S + 1/4) on the tail that is at most 1/2; both operands are exact
//                                         in f64 (S <= 8 (2^32 - 1)), so p carries one rounding
//       z[b] = -dx_norm_ppf(p) where u' == u, +dx_norm_ppf(p) otherwise: antisymmetric by construction; 1 - p is never formed
//   per-chain moments of the scores, bins in ascending order, c = c[k][b] > 0 (weighted Welford; every added term >= 0):
//       n_k += c;  d = z - mean_k;  mean_k = fma(d, c / n_k, mean_k);  m2_k = fma(c d, z - mean_k, m2_k)
//   statistic, for n_0 = .. = n_{K-1} = n >= 2 OF THIS PIXEL (counted samples; anything else gives NaN):
//       W = (sum_k m2_k) / (K (n - 1));  B/n by dx_chains_Bn_of;  R-hat = sqrt(((n - 1)/n W + B/n) / W)
//       NaN where S = 0 or every sample lies in one bin (0/0), +inf where W = 0 and the means differ -- as dx_chains_rhat
//   folded: m = the first bin with C[b] > 0 && (double)(cum[b] + C[b]) >= 0.5 (double)S (dx_hist_qstep's rule at q = 0.5);
//       f[k][0] = c[k][m], f[k][e] = c[k][m - e] + c[k][m + e] for e = 1 .. nbins-1, terms outside the record 0; the statistic
//       above with f for c and e for b: the fold |x - median| on bin centres
//   stat 0 = bulk (rank-normalised), 1 = folded, 2 = the larger of the two (NaN if either is NaN)
// Not split: the histograms are not batched; drift inside a chain is dx_batches_host.h's split R-hat.
#pragma once
#include "dx_chains_host.h"
#include "dx_hist_host.h"

enum { DX_RK_BULK = 0, DX_RK_FOLDED = 1, DX_RK_MAX = 2 };

// -Phi^-1(p) = |z| >= 0 for p in (0, 1/2]: Wichura's algorithm AS 241 (Applied Statistics 37 (1988) 477), routine PPND16, its
// central branch (|p - 1/2| <= 0.425) and the first of its two tail branches (r = sqrt(-log p) <= 5).
// Domain: p >= 0.625 / (8 (2^32 - 1) + 0.25) = 1.8e-11, the smallest p a score takes, where r = 4.98 and |z| = 6.7; the second
//   tail branch (r > 5, p < 1.4e-11) lies outside it and is not carried.
// dx_norm_ppf(0.5) == 0 exactly: q = 0 multiplies the quotient.
// Absolute error <= 1e-12 on the domain.  PPND16's rational functions are good to about 1e-16 RELATIVE (Wichura, sect. 3), i.e.
//   7e-16 at |z| = 6.7; evaluated in f64 each Horner form adds a few ulp, and the tail branch sees the error of log and of sqrt
//   through r: dz/dr = 2 r p / phi(z) <= 2 r / z <= 3.3 on the branch, r is good to 2 ulp of 5 (1.8e-15), which gives 6e-15.
//   1e-12 leaves two orders above that sum for a device library whose log is good to a few ulp only; measured (host, glibc):
//   3.2e-15 against a 40-digit evaluation over 4000 log-spaced p of the domain.
DX_HD double dx_norm_ppf(double p) {
    const double q = 0.5 - p;   // >= 0; exact for p >= 1/4
    if (q <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = fma(fma(fma(fma(fma(fma(fma(2.5090809287301226727e+3, r, 3.3430575583588128105e+4), r, 6.7265770927008700853e+4), r,
                                               4.5921953931549871457e+4), r, 1.3731693765509461125e+4), r, 1.9715909503065514427e+3), r,
                                   1.3314166789178437745e+2), r, 3.3871328727963666080e+0);
        const double den = fma(fma(fma(fma(fma(fma(fma(5.2264952788528545610e+3, r, 2.8729085735721942674e+4), r, 3.9307895800092710610e+4), r,
                                               2.1213794301586595867e+4), r, 5.3941960214247511077e+3), r, 6.8718700749205790830e+2), r,
                                   4.2313330701600911252e+1), r, 1.0);
        return q * num / den;
    }
    const double r = sqrt(-log(p)) - 1.6;
    const double num = fma(fma(fma(fma(fma(fma(fma(7.74545014278341407640e-4, r, 2.27238449892691845833e-2), r, 2.41780725177450611770e-1), r,
                                           1.27045825245236838258e+0), r, 3.64784832476320460504e+0), r, 5.76949722146069140550e+0), r,
                               4.63033784615654529590e+0), r, 1.42343711074968357734e+0);
    const double den = fma(fma(fma(fma(fma(fma(fma(1.05075007164441684324e-9, r, 5.47593808499534494600e-4), r, 1.51986665636164571966e-2), r,
                                           1.48103976427480074590e-1), r, 6.89767334985100004550e-1), r, 1.67638483018380384940e+0), r,
                               2.05319162663775882187e+0), r, 1.0);
    return num / den;
}

// the score of a bin that holds C > 0 of the S samples, cum of them below it
DX_HD double dx_rank_score(unsigned long long cum, unsigned long long C, unsigned long long S) {
    const unsigned long long u = 2 * cum + C + 1, v = 2 * S + 2 - u, t = u < v ? u : v;
    const double z = dx_norm_ppf(((double)t - 0.75) / ((double)(2 * S) + 0.5));
    return t == u ? -z : z;
}

// the running triples of the K chains; a kernel indexes them by constants only (dx_chains_each), so they live in registers
struct DxRankState {
    double n[DX_CHAINS_MAX], mean[DX_CHAINS_MAX], m2[DX_CHAINS_MAX];
};

DX_HD void dx_rank_reset(DxRankState& s) {
    dx_chains_each<0>(DX_CHAINS_MAX, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        s.n[k] = 0.0; s.mean[k] = 0.0; s.m2[k] = 0.0;
    });
}

// c > 0 samples of score z into one chain's triple
DX_HD void dx_rank_update(double c, double z, double& n, double& mean, double& m2) {
    n += c;
    const double d = z - mean;
    mean = fma(d, c / n, mean);
    m2 = fma(c * d, z - mean, m2);
}

// one bin (or one distance of the fold) of a score walk: C = its pooled count, cum = the pooled count before it (updated),
// count(std::integral_constant<int, k>) = chain k's count of it
template <class Count>
DX_HD void dx_rank_bin(int K, unsigned long long C, unsigned long long& cum, unsigned long long S, DxRankState& s, Count count) {
    if (C == 0) return;
    const double z = dx_rank_score(cum, C, S);
    dx_chains_each<0>(K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const unsigned long long c = count(kc);
        if (c > 0) dx_rank_update((double)c, z, s.n[k], s.mean[k], s.m2[k]);
    });
    cum += C;
}

// one bin of the first walk: the pooled total and the lowest / highest non-empty bin (first starts at -1)
DX_HD void dx_rank_total_step(unsigned long long C, int b, unsigned long long& S, int& first, int& last) {
    S += C;
    if (C > 0) {
        if (first < 0) first = b;
        last = b;
    }
}

// one bin of the search for the pooled median bin: true when bin b is the first with C > 0 && cum + C >= half (half = 0.5 S)
DX_HD bool dx_rank_median_step(unsigned long long C, int b, double half, unsigned long long& cum, int& m) {
    if (C > 0 && (double)(cum + C) >= half) { m = b; return true; }
    cum += C;
    return false;
}

DX_HD double dx_rank_finish(int K, const DxRankState& s) {
    const double n = s.n[0];
    bool ok = n >= 2.0;
    double sum = s.m2[0];
    dx_chains_each<1>(K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        ok = ok && s.n[k] == n;
        sum += s.m2[k];
    });
    if (!ok) return (double)NAN;
    const double W = sum / ((double)K * (n - 1.0));
    return sqrt(fma((n - 1.0) / n, W, dx_chains_Bn_of(K, (double)K, (double)(K - 1), s.mean)) / W);
}

// stat 2 of the other two: NaN if either is NaN
DX_HD double dx_rank_larger(double bulk, double folded) {
    if (bulk != bulk || folded != folded) return (double)NAN;
    return folded > bulk ? folded : bulk;
}

// chain k's count at distance e of bin m: count(kc, b) reads a bin inside the record
template <class KC, class Count>
DX_HD unsigned long long dx_rank_fold_count(KC kc, int m, int e, int nbins, Count count) {
    unsigned long long f = m + e < nbins ? (unsigned long long)count(kc, m + e) : 0ull;
    if (e > 0 && m - e >= 0) f += count(kc, m - e);
    return f;
}

// The folded statistic of one pixel around its pooled median bin m, S > 0: count(std::integral_constant<int, k>, b) = c[k][b] for
// 0 <= b < nbins; first <= m <= last the lowest and the highest non-empty pooled bin (beyond them every distance is empty and
// adds nothing, so the walk stops there).  The kernel and the host walk below come through here.
template <class Count>
DX_HD double dx_rank_folded_of(int K, int nbins, int m, int first, int last, unsigned long long S, Count count) {
    DxRankState s;
    dx_rank_reset(s);
    unsigned long long cum = 0;
    const int reach = m - first > last - m ? m - first : last - m;
    for (int e = 0; e <= reach; ++e) {
        unsigned long long F = 0;
        dx_chains_each<0>(K, [&](auto kc) { F += dx_rank_fold_count(kc, m, e, nbins, count); });
        dx_rank_bin(K, F, cum, S, s, [&](auto kc) { return dx_rank_fold_count(kc, m, e, nbins, count); });
    }
    return dx_rank_finish(K, s);
}

// the whole walks over K records in memory (host checks; k_chains_rank takes the same steps, the unfolded ones over 16-byte pieces)
inline double dx_rank_stat(const uint32_t* const* rec, int K, int nbins, int bits, int stat) {
    const auto count = [&](auto kc, int b) { return dx_hist_count(rec[decltype(kc)::value], b, bits); };
    const auto pooled = [&](int b) {
        unsigned long long C = 0;
        dx_chains_each<0>(K, [&](auto kc) { C += count(kc, b); });
        return C;
    };
    unsigned long long S = 0;
    int first = -1, last = -1;
    for (int b = 0; b < nbins; ++b) dx_rank_total_step(pooled(b), b, S, first, last);
    if (S == 0) return (double)NAN;
    double bulk = 0.0, folded = 0.0;
    if (stat != DX_RK_FOLDED) {
        DxRankState s;
        dx_rank_reset(s);
        unsigned long long cum = 0;
        for (int b = 0; b < nbins; ++b) dx_rank_bin(K, pooled(b), cum, S, s, [&](auto kc) { return count(kc, b); });
        bulk = dx_rank_finish(K, s);
        if (stat == DX_RK_BULK) return bulk;
    }
    unsigned long long cum = 0;
    int m = 0;
    for (int b = 0; b < nbins; ++b)
        if (dx_rank_median_step(pooled(b), b, 0.5 * (double)S, cum, m)) break;
    folded = dx_rank_folded_of(K, nbins, m, first, last, S, count);
    return stat == DX_RK_FOLDED ? folded : dx_rank_larger(bulk, folded);
}

// the arguments of a read-out: "" = fine, else the cause
inline std::string dx_rank_check(int K, int nbins, int bits, int stat) {
    if (K < 2 || K > DX_CHAINS_MAX) return "the rank-normalised R-hat takes 2 to " + std::to_string(DX_CHAINS_MAX) + " chains, not " + std::to_string(K);
    const std::string shape = dx_hist_shape_check(nbins, bits);
    if (!shape.empty()) return shape;
    if (stat < DX_RK_BULK || stat > DX_RK_MAX)
        return "the stat of a rank-normalised R-hat must be 0 (bulk), 1 (folded) or 2 (the larger of the two), not " + std::to_string(stat);
    return "";
}
