// dx_chains_host.h -- the definitions of the read-outs over SEVERAL chains (dangx_chains_*, include/dangx.h): pooled mean / M2 /
// pair term by Chan's pairwise fold, within- and between-chain variance, Gelman-Rubin R-hat (Gelman et al., BDA3 eq. 11.4), the
// pooled AR(1) effective sample size.  The kernels of dangx_moments.hip, the host mirror of the template-amplitude rows and a
// stand-alone host program evaluate the SAME inline functions (explicit fma, one fixed operation order), and this file needs no
// HIP runtime.
//
// Chains k = 0..K-1, 2 <= K <= DX_CHAINS_MAX, chain k with n_k >= 1 samples; per element mean_k and m2_k = sum_t (x_t - mean_k)^2.
//   fold (list order, from chain 0's own values), running (n, mu, M) and the next chain:
//       d = mean_k - mu;  n' = n + n_k;  mu += d (n_k / n');  M += m2_k + d^2 (n n_k / n')        -- every added term >= 0
//     and for a pair of planes  C += C_k + d_a d_b (n n_k / n')  with d_a, d_b of the same fold.  The integer ratios are formed
//     once on the host in f64 (dx_chains_par).
//   W   = (sum_k m2_k) / (K (n - 1))
//   B/n = sum_k (d_k - dbar)^2 / (K - 1),  d_k = mean_k - mean_0,  dbar = (sum_k d_k) / K: an offset far larger than the spread
//         costs what it costs the means
//   R-hat = sqrt(((n - 1)/n W + B/n) / W): 0/0 = NaN where no chain ever moved, +inf where only the means differ
//   pooled ESS = sum_k ESS_k (dx_lag_rho1 / dx_lag_ess of dx_moments_host.h)
// W, B/n and R-hat need n_k = n >= 2 for every chain; the callers refuse anything else.
#pragma once
#include "dx_moments_host.h"

#include <type_traits>

#define DX_CHAINS_MAX 8   // == DANGX_MAX_CHAINS (include/dangx.h)

// stat of a plane / signal / template-row read-out
enum { DX_CH_MEAN = 0, DX_CH_STD = 1, DX_CH_RHAT = 2, DX_CH_W = 3, DX_CH_BN = 4, DX_CH_ESS = 5 };

struct DxChainsPar {          // everything of a read-out that depends on the sample counts only, by value
    int K;
    int pad_;
    double w[DX_CHAINS_MAX];   // w[k] = n_k / n'            (k >= 1; n' = n_0 + .. + n_k)
    double c[DX_CHAINS_MAX];   // c[k] = (n' - n_k) n_k / n' (k >= 1)
    double cnt[DX_CHAINS_MAX]; // n_k
    double dn;                 // N - ddof
    double f;                  // (n - 1) / n          } equal counts only
    double kn1;                // K (n - 1)            }
    double km1;                // K - 1
    double kd;                 // K
};

inline DxChainsPar dx_chains_par(int K, const long long* n, int ddof) {
    DxChainsPar p{};
    p.K = K;
    long long run = 0;
    for (int k = 0; k < K && k < DX_CHAINS_MAX; ++k) {
        const long long before = run;
        run += n[k];
        p.cnt[k] = (double)n[k];
        p.w[k] = (double)n[k] / (double)run;
        p.c[k] = (double)before * (double)n[k] / (double)run;
    }
    p.dn = (double)(run - ddof);
    p.f = (double)(n[0] - 1) / (double)n[0];
    p.kn1 = (double)K * (double)(n[0] - 1);
    p.km1 = (double)(K - 1);
    p.kd = (double)K;
    return p;
}

// f(std::integral_constant<int, k>) for k0 <= k < min(K, DX_CHAINS_MAX), unrolled by recursion: whatever f indexes by k is indexed
// by a constant from the start, so the small arrays below live in registers on the device and a by-value DxChainsPar is read
// where it lies
// (MAX: the bound of the arrays, DX_CHAINS_MAX unless the caller holds more entries -- the 2K half-chains of dx_batches_host.h)
template <int k, int MAX = DX_CHAINS_MAX, class F>
DX_HD void dx_chains_each(int K, F&& f) {
    if constexpr (k < MAX) {
        if (k < K) f(std::integral_constant<int, k>());
        dx_chains_each<k + 1, MAX>(K, f);
    }
}

// one chain into the running (mu, M)
DX_HD void dx_chains_fold(double mean_k, double m2_k, double w, double c, double& mu, double& M) {
    const double d = mean_k - mu;
    mu = fma(d, w, mu);
    M = fma(d * d, c, M + m2_k);
}

DX_HD void dx_chains_pool(const DxChainsPar& p, const double (&mean)[DX_CHAINS_MAX], const double (&m2)[DX_CHAINS_MAX], double& mu, double& M) {
    double u = mean[0], S = m2[0];
    dx_chains_each<1>(p.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        dx_chains_fold(mean[k], m2[k], p.w[k], p.c[k], u, S);
    });
    mu = u;
    M = S;
}

DX_HD double dx_chains_W(const DxChainsPar& p, const double (&m2)[DX_CHAINS_MAX]) {
    double s = m2[0];
    dx_chains_each<1>(p.K, [&](auto kc) { s += m2[decltype(kc)::value]; });
    return s / p.kn1;
}

// B/n of the first K of N means, referred to mean[0]; kd = K, km1 = K - 1 as f64.  The one definition: the chains' (N =
// DX_CHAINS_MAX) and the half-chains' of dx_batches_host.h (N = 2 DX_CHAINS_MAX)
template <int N>
DX_HD double dx_chains_Bn_of(int K, double kd, double km1, const double (&mean)[N]) {
    double sum = 0.0;   // d_0 = 0
    dx_chains_each<1, N>(K, [&](auto kc) { sum += mean[decltype(kc)::value] - mean[0]; });
    const double dbar = sum / kd;
    double acc = dbar * dbar;   // (d_0 - dbar)^2
    dx_chains_each<1, N>(K, [&](auto kc) {
        const double e = (mean[decltype(kc)::value] - mean[0]) - dbar;
        acc = fma(e, e, acc);
    });
    return acc / km1;
}

DX_HD double dx_chains_Bn(const DxChainsPar& p, const double (&mean)[DX_CHAINS_MAX]) { return dx_chains_Bn_of(p.K, p.kd, p.km1, mean); }

DX_HD double dx_chains_rhat(const DxChainsPar& p, double W, double Bn) { return sqrt(fma(p.f, W, Bn) / W); }

// stats DX_CH_MEAN .. DX_CH_BN of one element.  An array a stat does not need (see dx_chains_needs_*) is never read.
DX_HD double dx_chains_stat(int stat, const DxChainsPar& p, const double (&mean)[DX_CHAINS_MAX], const double (&m2)[DX_CHAINS_MAX]) {
    if (stat == DX_CH_W) return dx_chains_W(p, m2);
    if (stat == DX_CH_BN) return dx_chains_Bn(p, mean);
    if (stat == DX_CH_RHAT) return dx_chains_rhat(p, dx_chains_W(p, m2), dx_chains_Bn(p, mean));
    double mu, M;
    dx_chains_pool(p, mean, m2, mu, M);
    return stat == DX_CH_MEAN ? mu : sqrt(M / p.dn);
}
DX_HD bool dx_chains_needs_mean(int stat) { return stat != DX_CH_W; }
DX_HD bool dx_chains_needs_m2(int stat) { return stat != DX_CH_BN; }   // the fold of the mean carries M along

// pooled ESS: chain k's term, added in list order to the sum so far (chain 0: acc = 0.0)
DX_HD double dx_chains_ess_add(double acc, double mean, double m2, double prev, double r, double P, double n) {
    return acc + dx_lag_ess(dx_lag_rho1(mean, m2, prev, r, P, n), n);
}

// pooled pair statistic of one element: stat 0 = covariance C / (N - ddof), 1 = correlation C / sqrt(M_a M_b).  The covariance
// reads no m2 (the arrays may hold anything)
DX_HD double dx_chains_pair(int stat, const DxChainsPar& p, const double (&ma)[DX_CHAINS_MAX], const double (&mb)[DX_CHAINS_MAX],
                            const double (&qa)[DX_CHAINS_MAX], const double (&qb)[DX_CHAINS_MAX], const double (&C)[DX_CHAINS_MAX]) {
    double mua = ma[0], mub = mb[0], Ma = stat ? qa[0] : 0.0, Mb = stat ? qb[0] : 0.0, Cc = C[0];
    dx_chains_each<1>(p.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const double da = ma[k] - mua, db = mb[k] - mub;
        Cc = fma(da * db, p.c[k], Cc + C[k]);
        dx_chains_fold(ma[k], stat ? qa[k] : 0.0, p.w[k], p.c[k], mua, Ma);
        dx_chains_fold(mb[k], stat ? qb[k] : 0.0, p.w[k], p.c[k], mub, Mb);
    });
    return dx_pair_stat(Cc, Ma, Mb, stat, p.dn);
}

// the counts a read-out needs: "" = fine, else the cause (the caller names the entry point)
inline std::string dx_chains_count_check(int K, const long long* n, int stat, int ddof, bool is_pair) {
    long long N = 0;
    for (int k = 0; k < K; ++k) N += n[k];
    if (!is_pair && stat >= DX_CH_RHAT && stat <= DX_CH_BN) {
        for (int k = 1; k < K; ++k)
            if (n[k] != n[0])
                return "R-hat, W and B/n need equal sample counts: chain " + std::to_string(k) + " holds " + std::to_string(n[k]) +
                       ", chain 0 holds " + std::to_string(n[0]);
        if (n[0] < 2) return "R-hat, W and B/n need at least 2 samples per chain (n = " + std::to_string(n[0]) + ")";
    }
    const bool uses_ddof = is_pair ? stat == 0 : stat == DX_CH_STD;
    if (uses_ddof && (ddof < 0 || N - ddof <= 0))
        return std::string(is_pair ? "covariance" : "standard deviation") + " needs 0 <= ddof < N (N = " + std::to_string(N) + ")";
    return "";
}
