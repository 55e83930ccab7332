// dx_batches_host.h -- the definitions of the BATCHED posterior accumulators (dangx_moments_batches*, dangx_chains_batches_*,
// include/dangx.h): the run cut into consecutive batches of L samples, each with its own (mean, m2), so that burn-in can be
// discarded after the run, and the batch-means Monte-Carlo standard error, the batch-means effective sample size and split R-hat
// of ONE chain can be read.  The kernels (dangx_moments.hip, dangx_chains.hip), a stand-alone host program and the tests
// evaluate the SAME inline functions (explicit fma, one fixed operation order); this file needs no HIP runtime.
//
// State of a registered plane: nbatch slots (mean_b, m2_b), zero-filled.  With c samples held, sample c + 1 goes to slot
// b = c / L as that slot's sample j = c % L + 1 by Welford's update (inv_n = 1 / j): a slot's first sample lands on zeros, so
// mean = x and m2 = 0 exactly.  When every slot is full (b == nbatch) the slots are merged in place first: for i = 0 ..
// nbatch/2 - 1 ascending, slot i = slots (2i, 2i+1) folded with dx_chains_fold(w = 1/2, c = L/2) from slot 2i's own values, the
// upper half is zeroed and L doubles (dx_batches_merge).
//
// Read-outs, per element, with nfull = count / L full slots, p = count % L samples in the open slot, `first` leading slots
// discarded as burn-in, B' = nfull - first.  Every fold over equal-count slots is dx_chains_fold from the first slot's own values,
// step i (1-based) with the host-formed ratios w = 1/(i+1), c = i L/(i+1) (dx_batches_par):
//   mean, std   over the samples [first L, count), open slot included: slots first.. folded in order, then the open slot with
//               w = p/N', c = B'L p/N' (N' = B'L + p); std = sqrt(M / (N' - ddof)).          needs 0 <= ddof < N'
//   MCSE        sqrt(S / (B'(B'-1))), S = Welford's M2 of the full slots' means in slot order from slot `first`'s mean:
//               d = m_b - u;  u = fma(d, 1/i, u);  S = fma(d, m_b - u, S).                    needs B' >= 2
//   ESS         (M_f / (B'L - 1)) / (S / (B'(B'-1))), M_f the folded M2 of the full slots; unclamped.   needs B' >= 2
//   split R-hat h = B'/2; the halves are the LAST 2h full slots (an odd B' drops its oldest), each folded to (mu, M);
//               W, B/n, R-hat = dx_chains_W / _Bn / _rhat with K = 2, n = hL.                 needs h >= 1, hL >= 2
// Over K chains (equal registration, L, nbatch and count): mean / std = the chains' own folds folded in list order; MCSE =
// sqrt(sum_k MCSE_k^2) / K; ESS = sum_k ESS_k; split R-hat over the 2K half-chains, W and B/n as above with 2K for K and the
// half-means referred to half 0 of chain 0.  NaN and inf follow the arithmetic: 0/0 where an element never moved, +inf where
// only the half-means differ.
#pragma once
#include "dx_chains_host.h"

#define DX_LAMBDA_INLINE __attribute__((always_inline))   // a loader lambda is part of the loop it is called from
// The loops over the slots.  A translation unit may ask for them unrolled (DX_BATCH_UNROLL, before this header is included): the
// loads of that many slots are then in flight at once; the folds stay in slot order, so the result is the same bits.
#if defined(DX_BATCH_UNROLL) && defined(__clang__)
#define DX_BATCH_STR_(x) #x
#define DX_BATCH_PRAGMA_(x) _Pragma(DX_BATCH_STR_(x))
#define DX_BATCH_LOOP DX_BATCH_PRAGMA_(unroll DX_BATCH_UNROLL)
#else
#define DX_BATCH_LOOP
#endif
#define DX_BATCH_MAX 32          // == DANGX_MAX_BATCHES (include/dangx.h)
#define DX_BATCH_MAX_PLANES 32   // == DANGX_MAX_BATCH_PLANES

enum { DX_BT_MEAN = 0, DX_BT_STD = 1, DX_BT_MCSE = 2, DX_BT_ESS = 3, DX_BT_RHAT = 4 };

struct DxBatchPar {           // everything of a read-out that depends on the counts only, by value
    int stat, first, nfull, open;   // open: 1 when the open slot holds samples (mean / std fold it in)
    int h, K;                 // slots per half; chains (1: a single chain)
    double w[DX_BATCH_MAX + 1];   // w[i] = 1/(i+1): step i of a fold of equal-count slots, and Welford's 1/(i+1) over the slot means
    double c[DX_BATCH_MAX + 1];   // c[i] = i L/(i+1)
    double wp, cp;            // the open slot onto B' full ones: p/N', B'L p/N'
    double dn;                // N' - ddof (over chains: K N' - ddof)
    double bb;                // B'(B'-1)
    double nm1;               // B'L - 1
    double f, hn1, hm1, hk;   // the halves: (n-1)/n, H (n-1), H - 1, H with n = hL and H = 2K half-chains
    double kd;                // K
    DxChainsPar half;         // dx_chains_par(2, {hL, hL}): the single chain's two halves through dx_chains_W / _Bn / _rhat
    DxChainsPar pool;         // dx_chains_par(K, {N', ..}, ddof): the chains' folds into one
};

inline DxBatchPar dx_batches_par(int stat, int first, int ddof, long long L, int nfull, long long partial, int K = 1) {
    DxBatchPar p{};
    p.stat = stat; p.first = first; p.nfull = nfull; p.open = partial > 0 ? 1 : 0; p.K = K;
    for (int i = 0; i <= DX_BATCH_MAX; ++i) {
        p.w[i] = 1.0 / (double)(i + 1);
        p.c[i] = (double)i * (double)L / (double)(i + 1);
    }
    const long long B = nfull - first, full = B * L, N = full + partial;
    p.wp = N > 0 ? (double)partial / (double)N : 0.0;
    p.cp = N > 0 ? (double)full * (double)partial / (double)N : 0.0;
    p.dn = (double)((long long)K * N - ddof);
    p.bb = (double)B * (double)(B - 1);
    p.nm1 = (double)(full - 1);
    p.h = (int)(B > 0 ? B / 2 : 0);
    const long long n = (long long)p.h * L, H = 2LL * K;
    p.f = n > 0 ? (double)(n - 1) / (double)n : 0.0;
    p.hn1 = (double)H * (double)(n - 1);
    p.hm1 = (double)(H - 1);
    p.hk = (double)H;
    p.kd = (double)K;
    const long long two[2] = {n > 0 ? n : 1, n > 0 ? n : 1};
    p.half = dx_chains_par(2, two, 0);
    long long cnt[DX_CHAINS_MAX];
    for (int k = 0; k < DX_CHAINS_MAX; ++k) cnt[k] = N > 0 ? N : 1;
    p.pool = dx_chains_par(K < 1 ? 1 : (K > DX_CHAINS_MAX ? DX_CHAINS_MAX : K), cnt, ddof);
    return p;
}

DX_HD bool dx_batches_needs_m2(int stat) { return stat != DX_BT_MEAN && stat != DX_BT_MCSE; }

// one slot mean into Welford's running (u, S) over the slot means, inv = 1 / (its 1-based number)
DX_HD void dx_batches_means_step(double m, double inv, double& u, double& S) {
    const double d = m - u;
    u = fma(d, inv, u);
    S = fma(d, m - u, S);
}

// a merge step: slot 2i+1 onto slot 2i's (mu, M); both hold L = 2 halfL samples, so w = L/2L and c = L L/2L
DX_HD void dx_batches_merge(double mean1, double m2_1, double halfL, double& mu, double& M) { dx_chains_fold(mean1, m2_1, 0.5, halfL, mu, M); }

// P below is DxBatchPar, on the device possibly qualified with the address space of the kernel arguments: the tables are read
// where they lie, never copied.  V elements side by side (1, or the 2 of a 16-byte access), every element through the same scalar functions.
// ld(b, want_m2, m, q): slot b's mean and, when wanted, m2 (else q = 0) of the V elements.

// slots [b0, b1) of equal counts folded from slot b0's own values
template <int V, class P, class Load>
DX_HD void dx_batches_fold(const P& p, int b0, int b1, bool want_m2, Load& ld, double (&mu)[V], double (&M)[V]) {
    ld(b0, want_m2, mu, M);
    DX_BATCH_LOOP
    for (int b = b0 + 1; b < b1; ++b) {
        double m[V], q[V];
        ld(b, want_m2, m, q);
        const int i = b - b0;
        for (int e = 0; e < V; ++e) dx_chains_fold(m[e], q[e], p.w[i], p.c[i], mu[e], M[e]);
    }
}

// (mu, M) of the samples [first L, count): the full slots from `first`, then the open one
template <int V, class P, class Load>
DX_HD void dx_batches_pool(const P& p, bool want_m2, Load& ld, double (&mu)[V], double (&M)[V]) {
    if (p.first < p.nfull) {
        dx_batches_fold<V>(p, p.first, p.nfull, want_m2, ld, mu, M);
        if (p.open) {
            double m[V], q[V];
            ld(p.nfull, want_m2, m, q);
            for (int e = 0; e < V; ++e) dx_chains_fold(m[e], q[e], p.wp, p.cp, mu[e], M[e]);
        }
    } else {
        ld(p.nfull, want_m2, mu, M);
    }
}

// S = Welford's M2 of the full slots' means from slot `first`, and (with want_m2) M = their folded M2, in ONE pass
template <int V, class P, class Load>
DX_HD void dx_batches_means(const P& p, bool want_m2, Load& ld, double (&S)[V], double (&M)[V]) {
    double u[V], mu[V];
    ld(p.first, want_m2, mu, M);
    for (int e = 0; e < V; ++e) { u[e] = mu[e]; S[e] = 0.0; }
    DX_BATCH_LOOP
    for (int b = p.first + 1; b < p.nfull; ++b) {
        double m[V], q[V];
        ld(b, want_m2, m, q);
        const int i = b - p.first;
        for (int e = 0; e < V; ++e) {
            dx_batches_means_step(m[e], p.w[i], u[e], S[e]);
            if (want_m2) dx_chains_fold(m[e], q[e], p.w[i], p.c[i], mu[e], M[e]);
        }
    }
}

template <class P>
DX_HD double dx_batches_mcse2(const P& p, double S) { return S / p.bb; }
template <class P>
DX_HD double dx_batches_ess(const P& p, double S, double M) { return (M / p.nm1) / dx_batches_mcse2(p, S); }

// the two halves of the last 2h full slots
template <int V, class P, class Load>
DX_HD void dx_batches_halves(const P& p, Load& ld, double (&muA)[V], double (&MA)[V], double (&muB)[V], double (&MB)[V]) {
    const int b0 = p.nfull - 2 * p.h;
    dx_batches_fold<V>(p, b0, b0 + p.h, true, ld, muA, MA);
    dx_batches_fold<V>(p, b0 + p.h, p.nfull, true, ld, muB, MB);
}

// every stat of ONE chain
template <int V, class Load>
DX_HD void dx_batches_stat(const DxBatchPar& p, Load ld, double (&r)[V]) {
    if (p.stat == DX_BT_MEAN || p.stat == DX_BT_STD) {
        double mu[V], M[V];
        dx_batches_pool<V>(p, p.stat == DX_BT_STD, ld, mu, M);
        for (int e = 0; e < V; ++e) r[e] = p.stat == DX_BT_MEAN ? mu[e] : sqrt(M[e] / p.dn);
    } else if (p.stat == DX_BT_MCSE || p.stat == DX_BT_ESS) {
        double S[V], M[V];
        dx_batches_means<V>(p, p.stat == DX_BT_ESS, ld, S, M);
        for (int e = 0; e < V; ++e) r[e] = p.stat == DX_BT_MCSE ? sqrt(dx_batches_mcse2(p, S[e])) : dx_batches_ess(p, S[e], M[e]);
    } else {
        double muA[V], MA[V], muB[V], MB[V];
        dx_batches_halves<V>(p, ld, muA, MA, muB, MB);
        for (int e = 0; e < V; ++e) {
            const double mean[DX_CHAINS_MAX] = {muA[e], muB[e]}, m2[DX_CHAINS_MAX] = {MA[e], MB[e]};
            r[e] = dx_chains_rhat(p.half, dx_chains_W(p.half, m2), dx_chains_Bn(p.half, mean));
        }
    }
}

#define DX_BATCH_HALVES (2 * DX_CHAINS_MAX)

// dx_chains_Bn over the H = 2K half-means, referred to half 0 of chain 0
template <class P>
DX_HD double dx_batches_Bn(const P& p, const double (&mean)[DX_BATCH_HALVES]) { return dx_chains_Bn_of(2 * p.K, p.hk, p.hm1, mean); }

// every stat over K chains.  ld(k, b, want_m2, m, q): chain k's slot b
template <int V, class P, class Load>
DX_HD void dx_chains_batches_stat(const P& p, Load ld, double (&r)[V]) {
    if (p.stat == DX_BT_MEAN || p.stat == DX_BT_STD) {
        double u[V], S[V];
        for (int k = 0; k < p.K; ++k) {   // running values only: the chains in a loop
            auto one = [&](int b, bool want, double (&m)[V], double (&q)[V]) DX_LAMBDA_INLINE { ld(k, b, want, m, q); };
            double mu[V], M[V];
            dx_batches_pool<V>(p, p.stat == DX_BT_STD, one, mu, M);
            for (int e = 0; e < V; ++e) {
                if (k == 0) { u[e] = mu[e]; S[e] = M[e]; }
                else dx_chains_fold(mu[e], M[e], p.pool.w[k], p.pool.c[k], u[e], S[e]);
            }
        }
        for (int e = 0; e < V; ++e) r[e] = p.stat == DX_BT_MEAN ? u[e] : sqrt(S[e] / p.dn);
    } else if (p.stat == DX_BT_MCSE || p.stat == DX_BT_ESS) {
        double acc[V];
        for (int e = 0; e < V; ++e) acc[e] = 0.0;
        for (int k = 0; k < p.K; ++k) {
            auto one = [&](int b, bool want, double (&m)[V], double (&q)[V]) DX_LAMBDA_INLINE { ld(k, b, want, m, q); };
            double S[V], M[V];
            dx_batches_means<V>(p, p.stat == DX_BT_ESS, one, S, M);
            for (int e = 0; e < V; ++e) acc[e] += p.stat == DX_BT_MCSE ? dx_batches_mcse2(p, S[e]) : dx_batches_ess(p, S[e], M[e]);
        }
        for (int e = 0; e < V; ++e) r[e] = p.stat == DX_BT_MCSE ? sqrt(acc[e]) / p.kd : acc[e];
    } else {
        double mean[V][DX_BATCH_HALVES] = {}, sumM[V];
        for (int e = 0; e < V; ++e) sumM[e] = 0.0;
        dx_chains_each<0>(p.K, [&](auto kc) DX_LAMBDA_INLINE {   // the 2K half-means stay in registers: constant subscripts
            constexpr int k = decltype(kc)::value;
            auto one = [&](int b, bool want, double (&m)[V], double (&q)[V]) DX_LAMBDA_INLINE { ld(k, b, want, m, q); };
            double muA[V], MA[V], muB[V], MB[V];
            dx_batches_halves<V>(p, one, muA, MA, muB, MB);
            for (int e = 0; e < V; ++e) {
                mean[e][2 * k] = muA[e]; mean[e][2 * k + 1] = muB[e];
                sumM[e] = k == 0 ? MA[e] + MB[e] : (sumM[e] + MA[e]) + MB[e];
            }
        });
        for (int e = 0; e < V; ++e) {
            const double W = sumM[e] / p.hn1;
            r[e] = sqrt(fma(p.f, W, dx_batches_Bn(p, mean[e])) / W);
        }
    }
}

// ---- host: the slot a sample goes to, and the checks

struct DxBatchPos { long long L; int nfull; long long partial; };
inline DxBatchPos dx_batches_pos(long long count, long long L) { return DxBatchPos{L, (int)(count / L), count % L}; }

// a registration: "" = fine, else the cause
inline std::string dx_batches_check(int nreg, const int32_t* planes, int nbatch, long long batch_len, int ncomp, int nmaps,
                                    const int32_t* sel, const int* nind, const int* global) {
    if (nreg < 0) return "the number of registrations is negative";
    if (nreg > DX_BATCH_MAX_PLANES) return "more than DANGX_MAX_BATCH_PLANES (" + std::to_string(DX_BATCH_MAX_PLANES) + ") registrations";
    if (nreg == 0) return "";
    if (nbatch < 2 || nbatch > DX_BATCH_MAX || (nbatch & 1))
        return "nbatch must be even and 2 .. DANGX_MAX_BATCHES (" + std::to_string(DX_BATCH_MAX) + "), not " + std::to_string(nbatch);
    if (batch_len < 1) return "batch_len must be at least 1, not " + std::to_string(batch_len);
    if (!planes) return "no plane list given";
    for (int r = 0; r < nreg; ++r) {
        const int32_t* p = planes + 3 * r;
        const std::string at = "registration " + std::to_string(r) + ": ";
        const int l = p[0], w = p[1], k = p[2];
        if (l < 0 || l >= ncomp) return at + "component index out of range";
        if (w < 0 || w > nind[l]) return at + "what must be 0 (amplitude) or 1 + index number of the component";
        if (k < 0 || k >= nmaps) return at + "plane out of range";
        if (w == 0 && global[l]) return at + "a template / monopole / hi_fit amplitude is not a pixel plane";
        if (!((sel[l] >> (w == 0 ? k : 3 + 3 * (w - 1) + k)) & 1)) return at + "a plane that is not selected";
        for (int o = 0; o < r; ++o)
            if (planes[3 * o] == l && planes[3 * o + 1] == w && planes[3 * o + 2] == k) return at + "the same plane twice";
    }
    return "";
}

// a read-out: "" = fine, else the cause
inline std::string dx_batches_stat_check(int stat, int first, int ddof, long long L, int nfull, long long partial) {
    if (stat < DX_BT_MEAN || stat > DX_BT_RHAT)
        return "the stat of a batch read-out must be 0 (mean), 1 (standard deviation), 2 (MCSE), 3 (batch-means ESS) or 4 (split R-hat)";
    if (first < 0 || first > nfull) return "first must be 0 .. the number of full batches (" + std::to_string(nfull) + "), not " + std::to_string(first);
    const long long B = nfull - first, N = B * L + partial;
    const std::string have = " (" + std::to_string(B) + " full batches of " + std::to_string(L) + " samples after first)";
    if (stat == DX_BT_MEAN || stat == DX_BT_STD) {
        if (N < 1) return "no sample after the discarded batches" + have;
        if (stat == DX_BT_STD && (ddof < 0 || N - ddof <= 0)) return "standard deviation needs 0 <= ddof < N' (N' = " + std::to_string(N) + ")";
        return "";
    }
    if (B < 2) return std::string(stat == DX_BT_MCSE ? "MCSE" : stat == DX_BT_ESS ? "batch-means ESS" : "split R-hat") + " needs B' >= 2" + have;
    if (stat == DX_BT_RHAT && (B / 2) * L < 2) return "split R-hat needs h L >= 2" + have;
    return "";
}
