// dx_chain.h -- the register-resident Metropolis chain (device code shared by dangx_mhreg.hip and dangx_fused.hip).
#pragma once
#include "dx_args.h"


template <bool V> struct BoolTag { static constexpr bool value = V; };

// the chain's exp: dx::exp_nr = the library routine minus its range selects (dx_math.h); -DDX_CHAIN_LIBEXP restores
// the library call for A/B timing
#ifdef DX_CHAIN_LIBEXP
#define CEXP(x) exp(x)
#define CEXPS(x) exp(x)
#define CEXPA(x) exp(x)
#define CEXP1(x) exp(x)
#else
#define CEXP(x) exp_nr(x)      // |x| < 1e9: power law, Planck factor (mbb_z)
#define CEXPS(x) exp_sat(x)    // |x| <= 1e16: the log-normal SED -(ln(nu/nu_p)/w)^2/2 of a chain whose width stays above 2^-16
#define CEXPA(x) exp_any(x)    // any x: the same SED for a narrow width (no bound), outside the proposal loops
#define CEXP1(x) exp_nr_v(x)   // a call site that runs once per proposal (dx_math.h: fma_vc); any x
#endif
// reciprocals of the rms and inside the modified-blackbody SED: v_rcp_f64 + two Newton steps (<= 1 ulp, 6 vector
// instructions) instead of the IEEE division sequence (11); -DDX_CHAIN_IEEEDIV restores a / b
#ifdef DX_CHAIN_IEEEDIV
#define CDIV(a, b) ((a) / (b))
#define CDIVE(a, b) ((a) / (b))
#define CRCPE(b) (1.0 / (b))
#else
#define CDIV(a, b) ((a) * fast_rcp(b))
// the same where b can be +inf or 0 (a Planck denominator exp(h nu / k T) - 1 at a temperature near 0: 1/inf = 0 in the
// reference's arithmetic, NaN from fast_rcp): outside the proposal loops, and in the chains that can get there (chain_finish)
#define CDIVE(a, b) ((a) * fast_rcp_ends(b))
#define CRCPE(b) fast_rcp_ends(b)
#endif

// the chain's residual: with DX_CHAIN_SCALED (default) the staged planes hold d/sigma and a/sigma (the amplitude is fixed
// during an index chain), so a band costs r = d' - a'*s; acc += r*r  (2 instructions per plane instead of 4) and the
// factor -1/2 is applied to the band sum; -DDX_CHAIN_UNSCALED restores ((d - a*s)/sigma), acc -= r*r/2 for A/B timing.
// Both forms carry the rounding of s scaled by the pixel's signal to noise; they differ in the last bits of lnL only.
#ifndef DX_CHAIN_UNSCALED
#define DX_CHAIN_SCALED 1
#endif
// lane-pair kernels: each lane draws the random numbers of every second step for both (1), or both draw all of them (0: A/B)
#ifndef DX_CHAIN_PAIR_RNG
#define DX_CHAIN_PAIR_RNG 1
#endif

namespace {

// The accept test of a Metropolis step (:443-454): diff >= 0 or exp(diff) > u3, u3 = u32(w) in [2^-33, 1).  The full-precision
// exp decides only where a cheap estimate cannot: e = v_exp_f32(float(diff) * float(log2e)) against uf, a float form of u3, with
// a relative margin M on either side.  What the margin has to cover, relative to exp(diff) / u3, where exp(diff) is near some u3:
//   * the exponent t = diff log2e lies in [-34, 0), and the three roundings to float (diff, log2e, the product; 2^-24 each) move
//     it by at most 34 * 3 * 2^-24 (1 + 2^-23) < 6.08e-6, i.e. e by a factor within 4.22e-6 of 1 (ln 2 of that);
//   * v_exp_f32, specified to 1 ulp and counted at 2: 2^-22 < 2.39e-7;
//   * uf = float(u3): 2^-24; with -DDX_ACCEPT_WORD, uf = fmaf(float(w), 2^-32, 2^-33) -- float(w) is within 2^-24 / (1 + 2^-24)
//     of w, hence the exact fma argument within that of u3, and the fma rounds once more: |uf - u3| < 2^-23 u3 = 1.2e-7 u3
//     (tests/test_gpu_draw_forms.py checks all 2^32 words): the larger of the two is counted;
//   * the product uf (1 +- M) rounded to float: 2^-24 < 6e-8; the margin constants are floats.
// In all < 4.64e-6 (second-order terms < 1e-10).  M = 2^-16 = 1.53e-5 is more than three times that -- the rule for M: the
// smallest power of two that is at least 3x the proven error.  Hence e > uf (1 + 2^-16) and e < uf (1 - 2^-16) decide exactly as
// the full comparison does (exp_nr_v is within 2^-52 of exp(diff)); beyond t = -34 both say reject (e <= 2^-34 (1 + 5e-6), 0 once
// it underflows, against uf >= 2^-33), and a NaN diff fails both bounds.  The remaining lanes (|e / uf - 1| <= 2^-16) take
// exp_nr_v against the fp64 u3, in a branch that the wavefront skips unless one of its lanes needs it.  Decisions are bit for
// bit those of the full test (tests/test_accept_certificate.py, tests/test_accept_margin_cpu.py): C3 +2.4 % (DESIGN.md, round
// 5).  The margin was 2^-12 until round 13 (-DDX_ACCEPT_MARGIN12 restores it): it adds to the likelihood bound W of mh_certain
// on both sides of the threshold (C3: the exact-branch share of cheap wave-steps 4.97 -> 4.46 % in the T launch, 7.03 -> 6.71 %
// in the Q+U launch; W is the larger part).  -DDX_ACCEPT_FULL restores the full test.
#ifdef DX_ACCEPT_MARGIN12
#define DX_ACC_UP 0x1.001p+0f
#define DX_ACC_DOWN 0x1.ffep-1f
#else
#define DX_ACC_UP 0x1.0001p+0f
#define DX_ACC_DOWN 0x1.fffep-1f
#endif
__device__ __forceinline__ bool mh_accept(double diff, double u3) {
#if defined(DX_ACCEPT_FULL) || defined(DX_CHAIN_LIBEXP)
    return (diff >= 0.0) || (CEXP1(diff) > u3);
#else
    const float e = __builtin_amdgcn_exp2f((float)diff * 0x1.715476p+0f);
    const float uf = (float)u3;
    bool acc = (diff >= 0.0) || (e > uf * DX_ACC_UP);
    const bool unsure = !(acc || e < uf * DX_ACC_DOWN);
    if (__builtin_amdgcn_ballot_w64(unsure) != 0ull) {
        if (unsure) acc = CEXP1(diff) > u3;
    }
    return acc;
#endif
}

// The same test for a diff known only as an interval: the fp64 chain's diff d lies in [dlo, dhi].  Decided (returns true) when
// every d in the interval takes the same decision by mh_accept's margins: dlo >= 0 or e(dlo) > uf (1 + 2^-16) accepts
// (exp is increasing), dhi < 0 and e(dhi) < uf (1 - 2^-16) rejects; a NaN bound decides nothing.
__device__ __forceinline__ bool mh_certain(double dlo, double dhi, float uf, bool& acc) {
    const float elo = __builtin_amdgcn_exp2f((float)dlo * 0x1.715476p+0f);
    const float ehi = __builtin_amdgcn_exp2f((float)dhi * 0x1.715476p+0f);
    acc = (dlo >= 0.0) || (elo > uf * DX_ACC_UP);
    return acc || ((dhi < 0.0) && (ehi < uf * DX_ACC_DOWN));
}
__device__ __forceinline__ bool mh_certain(double dlo, double dhi, double u3, bool& acc) { return mh_certain(dlo, dhi, (float)u3, acc); }

// The chain carries the accept uniform of a step as its Philox word.  u32f: the float of it that the cheap tests compare with.
// -DDX_ACCEPT_WORD forms it from the word in two 32-bit instructions and u32(w) only in the exact branches; OFF: it lowers the
// proposal loops by one or two vector instructions, but the addend 2^-33 takes a vector register for the whole kernel and the
// 5-band Q+U instance then spills 74 registers against 72.
__device__ __forceinline__ float u32f(uint32_t w) {
#ifdef DX_ACCEPT_WORD
    return u32f_word(w);
#else
    return (float)u32(w);
#endif
}
__device__ __forceinline__ bool mh_accept(double diff, uint32_t w) {
#if defined(DX_ACCEPT_WORD) && !defined(DX_ACCEPT_FULL) && !defined(DX_CHAIN_LIBEXP)
    const float e = __builtin_amdgcn_exp2f((float)diff * 0x1.715476p+0f);
    const float uf = u32f(w);
    bool acc = (diff >= 0.0) || (e > uf * DX_ACC_UP);
    const bool unsure = !(acc || e < uf * DX_ACC_DOWN);
    if (__builtin_amdgcn_ballot_w64(unsure) != 0ull) {
        if (unsure) acc = CEXP1(diff) > u32(w);
    }
    return acc;
#else
    return mh_accept(diff, u32(w));
#endif
}
__device__ __forceinline__ bool mh_certain(double dlo, double dhi, uint32_t w, bool& acc) { return mh_certain(dlo, dhi, u32f(w), acc); }


#ifdef DX_LNL_DIAG
// diagnostic (off by default): wave-steps the certified cheap likelihood evaluated [0], and of them those whose wavefront took
// the exact branch [1]; read and cleared by dangx_lnl_diag (dangx_planeset.hip: counts the k_plane_set chains)
__device__ unsigned long long g_lnl_diag[2];
__device__ __forceinline__ void lnl_diag_count(int k) {
    if (__lane_id() == __builtin_ctzll(__builtin_amdgcn_ballot_w64(true))) atomicAdd(&g_lnl_diag[k], 1ull);
}
#endif

// ---------------------------------------------------------------------------
// Register-resident form of the same chain (chisq likelihood, delta bandpasses, CH_POW / CH_MBB_BETA /
// CH_MBB_T) for compile-time band count NB and plane count SP: the cleaned data, 1/rms and the chain-
// invariant SED factor live in VGPRs (statically indexed, fully unrolled), per-band constants in SGPRs,
// and the kernel uses no LDS and no barrier.  The CU's vector register file (512 KB) is three times its
// LDS, so this form runs at 2-3 waves/SIMD where the LDS-column form is capped at 1-2.
// Arithmetic and operation order are identical to index_chain<MODE, SP, TB>.
//
// LP = 2 splits the bands of ONE pixel over two adjacent lanes (lane h of the pair owns bands [h*NB, (h+1)*NB) of the
// 2*NB bands): each lane stages and evaluates its half, the two partial band sums of lnL are exchanged with one
// cross-lane add per plane, and everything else (random numbers, prior, accept test) is computed by both lanes on
// identical inputs, so the pair never diverges.  It halves the registers a lane needs -- two planes of 20 bands drop
// from ~340 registers (one wave per SIMD) to the footprint of the 10-band kernel (two waves) -- at the price of the
// duplicated per-proposal work; the per-band constants then differ between the lanes of a pair and live in vector
// registers (K1, K2) instead of being scalar operands.
template <int LP>
struct BandPick {
    int half;  // which half of the bands this lane owns (always 0 for LP == 1)
    // per-band model constant for the lane's band j (j static): a scalar operand for LP == 1, else a select of two scalars
    __device__ __forceinline__ double operator()(const double* arr, int j, int nbh) const {
        if (LP == 1) return arr[j];
        const double a = arr[j], b = arr[nbh + j];
        return half ? b : a;
    }
    __device__ __forceinline__ double nu_c(const Model& M, int j, int nbh) const {
        if (LP == 1) return M.band[j].nu_c;
        const double a = M.band[j].nu_c, b = M.band[nbh + j].nu_c;
        return half ? b : a;
    }
};

// KT: a lane pair's per-band constants are read from a table in LDS (kt1 / kt2 point at the lane's first band) instead of being
// held in 2*NB registers -- for kernels that have the block's constant table anyway (k_plane_set)
// BP (LP == 1 only): some bands are bandpass-integrated (bp%id /= 'delta', src/dang_component_mod.f90:909-913, 949-954): such a
// band's SED is the tau-weighted sum over its samples in sample order, evaluated by a run-time loop around the same per-sample
// expressions -- sample tables (nu0, tau0, log(nu0/nu_ref)) through scalar loads, the reciprocal of the Planck denominator as in
// the delta form.  What is chain invariant per SAMPLE (the other index's exponential of a modified blackbody) has nowhere to
// live (85 values per pixel in bench.py --bandpass 16) and is evaluated again in every proposal: two exponentials per sample
// instead of one for the mbb sweeps.
// JF (CH_POW, delta bands): the chain carries the Jeffreys prior of the component labelled 'synch' (eval_jeffreys_prior,
// src/dang_lnl_mod.f90:242-304): every likelihood evaluation also leaves S = sum_j s_j^2 w_j in jS, where
// w_j = ln(nu_j/nu_ref)^2 sum_k sigma_kj^-4 is formed once per chain (form_w) -- the reference's
// sum_k sum_j ((1/sigma_kj)^2 (a_k s_j / a_k) ln(nu_j/nu_ref))^2 with the amplitude cancelled, so that where the reference
// divides 0 by 0 (or inf by inf, or meets a NaN amplitude) w_j is NaN and so is S.  The weights live in registers, or (KT:
// k_plane_set) in NB rows of the lane's LDS column behind the parked 1/rms.
// KEPT (k_plane_set; LP == 1, delta bands, no Jeffreys prior): chain_finish takes the chain-invariant factor from where it was
// formed before -- a beta chain's Planck factors from the column fcol (stride BLOCK) where the solve's sed_column left them
// (fcol null: evaluated as ever), a T chain's power-law factors set in F[] by the caller as the beta chain's closing
// evaluation left them (chain_finish, HAND).  Same operands, same operations: the same bits.
template <int MODE, int SP, int NB, int LP, bool KT = false, bool BP = false, bool JF = false, bool KEPT = false>
struct RegChain {
    static constexpr bool kBP = BP;
    static constexpr bool kJF = JF;
    static constexpr bool kKept = KEPT;
    static_assert(!KEPT || (LP == 1 && !BP && !JF && (MODE == CH_MBB_BETA || MODE == CH_MBB_T)), "kept factors: one-lane delta-band mbb chains");
    static_assert(!JF || (MODE == CH_POW && !BP), "Jeffreys chains: power law, delta bands");
    double D[SP][NB], F[NB], ISr[SP][NB];  // cleaned data, chain-invariant SED factor, 1/rms  (scaled form: d/rms, amp/rms)
    double bpa, bpb;                       // BP: CH_MBB_BETA: z = h/(k T), exp(z nu_ref) - 1; CH_MBB_T: beta + 1
    double K1[(LP > 1 && !KT) ? NB : 1], K2[(LP > 1 && !KT) ? NB : 1];  // LP > 1: the lane's per-band constants (see k1 / k2)
    const double *kt1, *kt2;
    double amp[SP];
    double W[(JF && !KT) ? NB : 1], jS;    // JF: the weights w_j (KT: in LDS at wcol), S of the last evaluation
    double* wcol;
    const double* fcol;                    // KEPT, CH_MBB_BETA

    __device__ __forceinline__ double w(int j) const { return KT ? wcol[j * BLOCK] : W[j]; }
    // the weights, from 1/rms of the lane's bands (is_of(kk, j)) and the amplitudes of the swept planes (amp[])
    template <class ISF>
    __device__ __forceinline__ void form_w(const Model& M, const Comp& c, ISF is_of) {
        bool bad = false;
#pragma unroll
        for (int kk = 0; kk < SP; ++kk) bad = bad || !(fabs(amp[kk]) > 0.0 && fabs(amp[kk]) < INFINITY);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double t0 = is_of(0, j) * is_of(0, j);
            double q = t0 * t0;
            if (SP == 2) { const double t1 = is_of(SP - 1, j) * is_of(SP - 1, j); q = fma(t1, t1, q); }
            const double l = k1(M, c, j);
            const double wj = bad ? __longlong_as_double(0x7ff8000000000000ll) : (l * l) * q;
            if (KT) wcol[j * BLOCK] = wj; else W[j] = wj;
        }
    }
    // S alone at index value th (a chain that starts from likelihood sums it was handed evaluates no likelihood first)
    __device__ __forceinline__ void jeff_eval(const Model& M, const Comp& c, double th) {
        double S = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) { const double e = CEXP(th * k1(M, c, j)); S = fma(e * e, w(j), S); }
        if (LP > 1) S += __shfl_xor(S, 1, 64);
        jS = S;
    }

    __device__ __forceinline__ double is(int kk, int j) const { return ISr[kk][j]; }
    __device__ __forceinline__ void set_is(int kk, int j, double v) { ISr[kk][j] = v; }
    // the constant that multiplies / offsets the sampled parameter at band j, and the band's constant factor
    __device__ __forceinline__ double k1(const Model& M, const Comp& c, int j) const {
        if (KT) return kt1[j];
        if (LP > 1) return K1[j];
        return (MODE == CH_MBB_T) ? M.band[j].nu_c : (MODE == CH_LOGN_NUP) ? c.lnu9[j] : c.lnr[j];
    }
    __device__ __forceinline__ double k2(const Comp& c, int j) const { return KT ? kt2[j] : (LP > 1) ? K2[j] : c.cst[j]; }
    // KT: rows of the block's table (dx_sed.h: sed_table_build with `ng` row blocks) for group member g, from the lane's band jb
    __device__ __forceinline__ void set_kt(const double* tab, int nbands, int ng, int g, int jb) {
        kt1 = tab + ((MODE == CH_MBB_T) ? TROWS * ng : (MODE == CH_LOGN_NUP) ? TROWS * g + 2 : TROWS * g) * nbands + jb;
        kt2 = tab + (TROWS * g + 1) * nbands + jb;
    }
    __device__ __forceinline__ void set_k(const Model& M, const Comp& c, const BandPick<LP>& pick) {
        if (LP > 1 && !KT) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                K1[j] = (MODE == CH_MBB_T) ? pick.nu_c(M, j, NB) : (MODE == CH_LOGN_NUP) ? pick(c.lnu9, j, NB) : pick(c.lnr, j, NB);
                K2[j] = (MODE == CH_LOGN_NUP || MODE == CH_LOGN_W) ? pick(c.cst, j, NB) : 0.0;
            }
        }
    }

    // BATCH (CH_MBB_T, CH_LOGN_*): chain_finish has decided, once per chain, that no proposal can leave the domains of the fast
    // helpers (a Planck denominator that overflows, a width below 2^-16).  CH_MBB_T: the tile's Planck denominators then share
    // one reciprocal.  Without it the band loop takes fast_rcp_ends / exp_any (dx_math.h), which hold for every argument.
    // OP: what the band loop does with the component's signal a/rms * s (the resident-residual form of k_plane_set, LNL_ADD /
    // LNL_SUB: D holds the FULL residual (d - sum of all members) / rms between the sweeps of a launch):
    //   LNL_EVAL  r = D - a' s, acc += r^2                      -- a likelihood evaluation (every proposal)
    //   LNL_ADD   r = D, D += a' s, acc += r^2                  -- the chain's FIRST evaluation, at the current index values: the
    //             member's own signal goes back into the cleaned data, and lnL of the current state is the residual's
    //   LNL_SUB   D -= a' s, acc += D^2                          -- after the chain, at the values it ended on: the residual again
    //             (the same residual bits as an EVAL there, so acc0 / acc1 are that evaluation's sums)
    // EOUT (CH_MBB_BETA, delta bands): the band's power-law factor e_j = exp((beta + 1) ln(nu_j / nu_ref)) also goes to eout[j]
    template <bool BATCH, int OP = 0, bool EOUT = false>
    __device__ __forceinline__ double lnl(const Model& M, const Comp& c, double th, double other, double& acc0, double& acc1,
                                          double* eout = nullptr) {
        static_assert(!EOUT || (MODE == CH_MBB_BETA && !BP), "the exported factor is the beta chain's");
        double s0 = 0.0, s1 = 0.0;
        if (MODE == CH_POW) s0 = th;
        else if (MODE == CH_MBB_BETA) s0 = th + 1.0;
        else if (MODE == CH_MBB_T) { s0 = mbb_z(th); s1 = CEXP(s0 * c.nu_ref) - 1.0; }
        else if (MODE == CH_LOGN_NUP) { s0 = log_pos(th); s1 = other; }  // log(nu/(nu_p*1e9)) = lnu9 - log(nu_p)
        else s1 = th;  // CH_LOGN_W
        acc0 = 0.0; acc1 = 0.0;
        double S = 0.0;  // JF: the prior's sum, beside chi^2 (not in the SUB pass: no prior is evaluated there)
        // log-normal: ln(nu/nu_p)/w as a product with 1/w (v_rcp_f64 + two Newton steps, once per evaluation) instead of one
        // IEEE division per band -- the expression the amplitude kernels use for the same SED (sed_tile), <= 1 ulp from it
#ifdef DX_CHAIN_IEEEDIV
        const double rs1 = 1.0 / s1;
#else
        const double rs1 = (MODE == CH_LOGN_NUP || MODE == CH_LOGN_W) ? (BATCH ? fast_rcp(s1) : fast_rcp_ends(s1)) : 0.0;
#endif
        // bands in tiles of TT: TT independent exp chains interleave, then accumulate in band order
        // (BP: one band at a time -- a bandpass-integrated band interleaves its own samples)
        constexpr int TT = BP ? 1 : (NB % 5 == 0) ? 5 : (NB % 4 == 0) ? 4 : (NB % 3 == 0) ? 3 : 1;
        static_assert(!BP || (LP == 1 && (MODE == CH_POW || MODE == CH_MBB_BETA || MODE == CH_MBB_T)), "bandpass chains: one lane, power law / mbb");
#pragma unroll
        for (int j0 = 0; j0 < NB; j0 += TT) {
            double s[TT];
            if (BP && M.band[j0].n != 0) {   // wave-uniform: LP == 1, j0 is the band number
                const Band& b = M.band[j0];
                const kptr nu = as_const(M.bp_nu0 + b.off);
                const kptr tau = as_const(M.bp_tau0 + b.off);
                const kptr lnr = as_const(c.bp_lnr + b.off);
                const int n = b.n;
                double sj = 0.0;
                if (MODE == CH_POW) {               // :909-913
#pragma unroll 4
                    for (int q = 0; q < n; ++q) sj = sj + tau[q] * CEXP(s0 * lnr[q]);
                } else if (MODE == CH_MBB_BETA) {   // :949-954, T fixed: tau * A / (e^{z nu} - 1) * (nu/nu_ref)^(beta+1)
#pragma unroll 4
                    for (int q = 0; q < n; ++q) sj = sj + (tau[q] * bpb) * CRCPE(CEXP(bpa * nu[q]) - 1.0) * CEXP(s0 * lnr[q]);
                } else {                            // CH_MBB_T, beta fixed
#pragma unroll 4
                    for (int q = 0; q < n; ++q) sj = sj + (tau[q] * s1) * CRCPE(CEXP(s0 * nu[q]) - 1.0) * CEXP(bpa * lnr[q]);
                }
                s[0] = sj;
            } else
            if (MODE == CH_MBB_T && TT > 1 && BATCH) {
                // one reciprocal for the tile's TT Planck denominators (prefix products, invert the last, peel backwards):
                // 3(TT-1) multiplications and one v_rcp_f64 + Newton instead of TT of them (v_rcp_f64 issues at a quarter of
                // the fma rate: 6 % of a temperature proposal).  Each 1/den_t carries <= 2(TT-1) more roundings.  Only for
                // chains that cannot reach a temperature where the product of TT denominators overflows (chain_finish).
                double den[TT], pre[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) den[t] = CEXP(s0 * k1(M, c, j0 + t)) - 1.0;
                pre[0] = den[0];
#pragma unroll
                for (int t = 1; t < TT; ++t) pre[t] = pre[t - 1] * den[t];
                double inv = s1 * fast_rcp(pre[TT - 1]);
#pragma unroll
                for (int t = TT - 1; t > 0; --t) {
                    s[t] = (inv * pre[t - 1]) * F[j0 + t];
                    inv *= den[t];
                }
                s[0] = inv * F[j0];
            } else
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const int j = j0 + t;
                if (MODE == CH_LOGN_NUP) {
                    const double l = (k1(M, c, j) - s0) * rs1;
                    s[t] = (BATCH ? CEXPS(-0.5 * (l * l)) : CEXPA(-0.5 * (l * l))) * k2(c, j);
                } else if (MODE == CH_LOGN_W) {
                    const double l = F[j] * rs1;
                    s[t] = (BATCH ? CEXPS(-0.5 * (l * l)) : CEXPA(-0.5 * (l * l))) * k2(c, j);
                } else {
                    const double e = CEXP(s0 * k1(M, c, j));
                    if (EOUT) eout[j] = e;
                    if (MODE == CH_POW) s[t] = e;
                    else if (MODE == CH_MBB_BETA) s[t] = F[j] * e;
                    else s[t] = (BATCH ? CDIV(s1, e - 1.0) : CDIVE(s1, e - 1.0)) * F[j];
                }
            }
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const int j = j0 + t;
#ifdef DX_CHAIN_SCALED
                if (OP == 1) {
                    const double r0 = D[0][j];
                    D[0][j] = fma(is(0, j), s[t], r0);
                    acc0 = fma(r0, r0, acc0);
                    if (SP == 2) {
                        const double r1 = D[SP - 1][j];
                        D[SP - 1][j] = fma(is(SP - 1, j), s[t], r1);
                        acc1 = fma(r1, r1, acc1);
                    }
                } else if (OP == 2) {
                    const double r0 = fma(-is(0, j), s[t], D[0][j]);
                    D[0][j] = r0;
                    acc0 = fma(r0, r0, acc0);
                    if (SP == 2) {
                        const double r1 = fma(-is(SP - 1, j), s[t], D[SP - 1][j]);
                        D[SP - 1][j] = r1;
                        acc1 = fma(r1, r1, acc1);
                    }
                } else {
                const double r0 = fma(-is(0, j), s[t], D[0][j]);
                acc0 = fma(r0, r0, acc0);
                if (SP == 2) {
                    const double r1 = fma(-is(SP - 1, j), s[t], D[SP - 1][j]);
                    acc1 = fma(r1, r1, acc1);
                }
                }
                if (JF && OP != 2) S = fma(s[t] * s[t], w(j), S);
#else
                const double r0 = (D[0][j] - amp[0] * s[t]) * is(0, j);
                acc0 = acc0 - 0.5 * (r0 * r0);
                if (SP == 2) {
                    const double r1 = (D[SP - 1][j] - amp[SP - 1] * s[t]) * is(SP - 1, j);
                    acc1 = acc1 - 0.5 * (r1 * r1);
                }
#endif
            }
        }
        if (LP > 1) {  // the other half's band sum: a + b on one lane, b + a on the other -- the same value
            acc0 += __shfl_xor(acc0, 1, 64);
            if (SP == 2) acc1 += __shfl_xor(acc1, 1, 64);
            if (JF && OP != 2) S += __shfl_xor(S, 1, 64);
        }
        if (JF && OP != 2) jS = S;
#ifdef DX_CHAIN_SCALED
        acc0 *= -0.5; acc1 *= -0.5;
#endif
        return acc0 + acc1;
    }

    // The LNL_ADD evaluation of a chain whose SED column at the current index values is still in the lane's LDS column
    // (k_plane_set keeps the member's column of the solve where its slot lies behind the parked 1/rms; scol: stride BLOCK): the
    // band loop of lnl<.., 1> with s_j read instead of evaluated.  The stored s_j = f_j * exp_nr(p0 lnr_j) of sed_column is the
    // product F[j] * e of lnl: f_j is F[j] (RegChain, KEPT), p0 = beta + 1 = s0, lnr_j = k1(j), all from the same table rows.
    __device__ __forceinline__ double lnl_add_kept(const double* scol, double& acc0, double& acc1) {
        static_assert(LP == 1 && !JF && !BP, "one lane, delta bands, no prior sum");
        acc0 = 0.0; acc1 = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double s = scol[j * BLOCK];
            const double r0 = D[0][j];
            D[0][j] = fma(is(0, j), s, r0);
            acc0 = fma(r0, r0, acc0);
            if (SP == 2) {
                const double r1 = D[SP - 1][j];
                D[SP - 1][j] = fma(is(SP - 1, j), s, r1);
                acc1 = fma(r1, r1, acc1);
            }
        }
        acc0 *= -0.5; acc1 *= -0.5;
        return acc0 + acc1;
    }

    // ---- the certified cheap evaluation (chain_finish; delta bands of CH_POW / CH_MBB_BETA / CH_MBB_T, scaled form)
    // A~ = sum over the pixel's bands and planes of r~^2, r~ = fma(-a', s~, D) in fp64 as the EVAL form, where s~ is the SED from
    // e = v_exp_f32(float(s0 log2e * k1)) -- the fp64 exponent s0 * k1 carried to fp32 -- and for CH_MBB_T 1/(e - 1) from
    // v_rcp_f32 (one by one: no batched reciprocal); everything else is the fp64 factors of the exact form (F, s1).
    __device__ __forceinline__ double lnl_cheap(const Model& M, const Comp& c, double th) {
        double s0 = 0.0, s1 = 0.0;
        if (MODE == CH_POW) s0 = th;
        else if (MODE == CH_MBB_BETA) s0 = th + 1.0;
        else { s0 = mbb_z(th); s1 = CEXP(s0 * c.nu_ref) - 1.0; }
        const double s0l = s0 * 0x1.71547652b82fep+0;  // log2(e)
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const float e = __builtin_amdgcn_exp2f((float)(s0l * k1(M, c, j)));
            double s;
            if (MODE == CH_POW) s = (double)e;
            else if (MODE == CH_MBB_BETA) s = F[j] * (double)e;
            else s = (s1 * F[j]) * (double)__builtin_amdgcn_rcpf(e - 1.0f);
            const double r0 = fma(-is(0, j), s, D[0][j]);
            acc0 = fma(r0, r0, acc0);
            if (SP == 2) {
                const double r1 = fma(-is(SP - 1, j), s, D[SP - 1][j]);
                acc1 = fma(r1, r1, acc1);
            }
        }
        double a = acc0 + acc1;
        if (LP > 1) a += __shfl_xor(a, 1, 64);
        return a;
    }

    // The bound, once per chain, for proposals th in [lo, hi].  Let s be the exact form's fp64 SED at band j and
    // |s - s~| <= E_j s~ (below).  With p~ = a' s~, R = D - a' s and R~ = D - p~ (real arithmetic on the fp64 operands),
    // |R - R~| <= E_j |p~| <= E_j (|D| + |R~|), so with G = sum E_j^2 D^2, Emax = max E_j and A = sum R~^2,
    //   |sum R^2 - sum R~^2| <= sum e (2 |R~| + e)  <=  2 sqrt(G A) + 2 Emax (1 + Emax) A + 2 G
    //                        <=  (2 Emax (1 + Emax) + lam) A + G / lam + 2 G         (any lam > 0: 2 sqrt(GA) <= G/lam + lam A)
    // and lam = sqrt(G / A_start) makes it tight where the chain stays near its start.  The fp64 roundings of both sums (at most
    // 2 NB + 4 roundings of nonnegative terms, < 2^-46 relative) and of this bound's own arithmetic are covered by the factor
    // (1 + 2^-40) and the term 2^-40 A; 2^-1000 covers squares that underflow.  lnL = -A / 2 halves it: |lnL - lnL~| <= wA A + wG.
    // Per band, with x = s0 k1 (|x| <= xmax_j over [lo, hi]):
    //   * the exponent carried to fp32: relative |x| (2^-24 + 2^-50) in e (s0 log2e and the product: 2^-53 each);
    //   * v_exp_f32 modelled at 2 ulp: 2^-22;  the exact form's exp_nr <= 1 ulp and its products: < 2^-46 in all;
    //   * CH_MBB_T: e - 1 is exact in fp32 (e >= 1); its relative error is e's amplified by 1/(1 - e^-x) <= 1 + 1/x, and
    //     x / (1 - e^-x) <= 1 + x; v_rcp_f32 at 2 ulp: 2^-22; the exact form's batched reciprocal: <= 2 (TT - 1) roundings;
    //   * second-order terms and the step from "relative to s" to "relative to s~": the factor 1 + 2^-8.
    // Returns false where the fp32 exponent could leave the normal range (|x log2e| > 125: e would overflow or lose its
    // precision) or T could reach 0: such chains take the exact evaluation for every proposal.
    __device__ __forceinline__ bool cheap_bound(const Model& M, const Comp& c, double lo, double hi, double a_start,
                                                double& wA, double& wG) {
        double G = 0.0, emax = 0.0, kmax = 0.0;
        double smax, zmin = 0.0;
        if (MODE == CH_POW) smax = fmax(fabs(lo), fabs(hi));
        else if (MODE == CH_MBB_BETA) smax = fmax(fabs(lo + 1.0), fabs(hi + 1.0));
        else { smax = mbb_z(lo); zmin = mbb_z(hi); }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double k = fabs(k1(M, c, j));
            kmax = fmax(kmax, k);
            double e;
            if (MODE == CH_MBB_T) e = (1.0 + smax * k) * 0x1p-24 + (2.0 + (double)__builtin_amdgcn_rcpf((float)(zmin * k))) * 0x1p-22;
            else e = (smax * k) * 0x1p-24 + 0x1p-22;
            e = e * (1.0 + 0x1p-8) + 0x1p-46;
            emax = fmax(emax, e);
#pragma unroll
            for (int kk = 0; kk < SP; ++kk) { const double t = e * D[kk][j]; G = fma(t, t, G); }
        }
        if (LP > 1) { G += __shfl_xor(G, 1, 64); emax = fmax(emax, __shfl_xor(emax, 1, 64)); kmax = fmax(kmax, __shfl_xor(kmax, 1, 64)); }
        // (any lam > 0 gives a bound: its own rounding, and 1/x from v_rcp_f32 above within the factor 1 + 2^-8, cost nothing)
        const double lam = fmax(sqrt(G * fast_rcp(fmax(a_start, 0x1p-900))), 0x1p-400);
        wA = 0.5 * ((2.0 * emax * (1.0 + emax) + lam) * (1.0 + 0x1p-40) + 0x1p-40);
        wG = 0.5 * ((G * fast_rcp(lam) + 2.0 * G) * (1.0 + 0x1p-40) + 0x1p-1000);
        const bool range = smax * kmax * 0x1.71547652b82fep+0 <= 125.0;
        return (MODE == CH_MBB_T) ? (range && lo > 0.0 && zmin > 0.0) : range;
    }
    // after the other components are removed: d -> d/rms, 1/rms -> amp/rms
    __device__ __forceinline__ void scale() {
#ifdef DX_CHAIN_SCALED
#pragma unroll
        for (int kk = 0; kk < SP; ++kk)
#pragma unroll
            for (int j = 0; j < NB; ++j) { D[kk][j] *= ISr[kk][j]; ISr[kk][j] *= amp[kk]; }
#endif
    }
};

// eval_sed of an "other" component for all NB bands of one plane, subtracted from D (static band index)
template <int NB, int LP>
__device__ __forceinline__ void subtract_other(const Model& M, const Comp& c2, int k, double amp2, double t0, double t1,
                                               double (&Dk)[NB], const BandPick<LP>& pick) {
    if ((c2.const_planes >> (k - 1)) & 1) {  // spatially constant indices: host-evaluated SED
#pragma unroll
        for (int j = 0; j < NB; ++j) Dk[j] -= amp2 * pick(c2.csed[k - 1], j, NB);
        return;
    }
    const Prep pr = sed_prep(c2, t0, t1);
    switch (c2.type) {
    case DANGX_POWERLAW:
#pragma unroll
        for (int j = 0; j < NB; ++j) Dk[j] -= amp2 * CEXP(pr.p0 * pick(c2.lnr, j, NB));
        break;
    case DANGX_MBB:
#pragma unroll
        for (int j = 0; j < NB; ++j) Dk[j] -= amp2 * (CDIVE(pr.p2, CEXP(pr.p1 * pick.nu_c(M, j, NB)) - 1.0) * CEXP(pr.p0 * pick(c2.lnr, j, NB)));
        break;
    case DANGX_FREEFREE:
#pragma unroll
        for (int j = 0; j < NB; ++j) Dk[j] -= amp2 * (ff_gaunt(pick(c2.lnu9, j, NB), pr.p0) / pr.p1 * pick(c2.cst, j, NB));
        break;
    case DANGX_LOGNORMAL: {
        const double rp1 = fast_rcp_ends(pr.p1);  // as sed_tile (dangx_ampreg.hip) forms it
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double l2 = (pick(c2.lnu9, j, NB) - pr.p2) * rp1;
            Dk[j] -= amp2 * (CEXPA(-0.5 * (l2 * l2)) * pick(c2.cst, j, NB));
        }
        break;
    }
    default:  // cmb
#pragma unroll
        for (int j = 0; j < NB; ++j) Dk[j] -= amp2 * pick(c2.cst, j, NB);
        break;
    }
}

// Q and U planes of one pixel whose "other" component has the same indices on both (always the case once a Q+U
// sweep has written them, :465): one SED evaluation per band serves both planes -- same values, same operations.
template <int NB, int LP>
__device__ __forceinline__ void subtract_other_pair(const Model& M, const Comp& c2, double ampa, double ampb, double t0, double t1,
                                                    double (&Da)[NB], double (&Db)[NB], const BandPick<LP>& pick) {
    const Prep pr = sed_prep(c2, t0, t1);
    switch (c2.type) {
    case DANGX_POWERLAW:
#pragma unroll
        for (int j = 0; j < NB; ++j) { const double s = CEXP(pr.p0 * pick(c2.lnr, j, NB)); Da[j] -= ampa * s; Db[j] -= ampb * s; }
        break;
    case DANGX_MBB:
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double s = CDIVE(pr.p2, CEXP(pr.p1 * pick.nu_c(M, j, NB)) - 1.0) * CEXP(pr.p0 * pick(c2.lnr, j, NB));
            Da[j] -= ampa * s; Db[j] -= ampb * s;
        }
        break;
    case DANGX_FREEFREE:
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double s = ff_gaunt(pick(c2.lnu9, j, NB), pr.p0) / pr.p1 * pick(c2.cst, j, NB);
            Da[j] -= ampa * s; Db[j] -= ampb * s;
        }
        break;
    case DANGX_LOGNORMAL: {
        const double rp1 = fast_rcp_ends(pr.p1);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double l2 = (pick(c2.lnu9, j, NB) - pr.p2) * rp1;
            const double s = CEXPA(-0.5 * (l2 * l2)) * pick(c2.cst, j, NB);
            Da[j] -= ampa * s; Db[j] -= ampb * s;
        }
        break;
    }
    default:  // cmb
#pragma unroll
        for (int j = 0; j < NB; ++j) { const double s = pick(c2.cst, j, NB); Da[j] -= ampa * s; Db[j] -= ampb * s; }
        break;
    }
}

// Second half of a register chain, from staged planes to the written index map: R holds the cleaned data and 1/rms of
// the lane's bands and the component's amplitudes; sample0/1 are its two current index values on the first plane.
// SCALE = false: the planes are already d/rms and amp/rms (a second chain of the same component on the same planes,
// k_index_mh_pair); final_value (nullable) receives the value the chain ends at.
// ADD / SUB (k_plane_set's resident-residual form, see RegChain::lnl): R.D arrives as the full residual and the first evaluation
// puts the component's own signal back (ADD); after the chain the signal at the values it ended on is taken out again (SUB).
// HAND (k_plane_set, the beta chain of a modified blackbody's pair; not with SUB): the chain hands e_j = exp((beta + 1) lnr_j) at
// the value it ended on to hand[j] -- the chain-invariant factor of the T chain that follows (RegChain, KEPT).  ONE exact
// evaluation at cur after the loop, by every lane, yields them and the closing sums of the lanes whose last accept was cheap;
// the other lanes keep their sums (the evaluation would return the same bits: it repeats the one that was accepted).
// scol (ADD, the chain's R is KEPT): the member's SED column at the current values, kept from the solve, or null.
template <int MODE, int SP, int NB, int LP, bool SCALE = true, bool ADD = false, bool SUB = false, bool HAND = false, class RC>
__device__ __forceinline__ unsigned long long chain_finish(const Model& M, const IndexArgs& a, const Comp& c, RC& R,
                                                           const BandPick<LP>& pick, double sample0, double sample1, int i, int half,
                                                           double chi[4], double* final_value = nullptr,
                                                           const double* acc_in = nullptr, double* acc_out = nullptr,
                                                           double* hand = nullptr, const double* scol = nullptr) {
    static_assert(!HAND || (MODE == CH_MBB_BETA && !SUB && !RC::kBP && LP == 1), "the hand-over is the one-lane delta-band beta chain's");
    // acc_in (k_plane_set, second chain of a component's pair): the likelihood sums of the state this chain starts from, as the
    // chain before it left them -- the same state, the same SED (another factorisation of it): no first evaluation.
    // acc_out: the sums of the state the chain ends on.
    const int npix = M.npix;
    double* out = c.idx + ((long long)a.nind * M.nmaps) * npix + i;
    const bool first = (a.nind == 0);
    constexpr bool JEFF = RC::kJF;
#if !defined(DX_CHAIN_SCALED)
    static_assert(!JEFF, "the Jeffreys chain exists in the scaled form");
#endif
    if (JEFF && SCALE) R.form_w(M, c, [&](int kk, int j) { return R.is(kk, j); });  // ISr is still 1/rms here
    if (SCALE) R.scale();
    // --- chain-invariant SED factor
    if (MODE == CH_MBB_BETA && RC::kKept && R.fcol) {
#pragma unroll
        for (int j = 0; j < NB; ++j) R.F[j] = R.fcol[j * BLOCK];
    } else if (MODE == CH_MBB_T && RC::kKept) {
        // F is the beta chain's hand-over
    } else if (MODE == CH_MBB_BETA) {
        const double z = mbb_z(sample1);
        const double A = CEXP(z * c.nu_ref) - 1.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) R.F[j] = CDIVE(A, CEXP(z * pick.nu_c(M, j, NB)) - 1.0);
        if (RC::kBP) { R.bpa = z; R.bpb = A; }   // bandpass-integrated bands: the same two numbers per SAMPLE (RegChain::lnl)
    } else if (MODE == CH_MBB_T) {
#pragma unroll
        for (int j = 0; j < NB; ++j) R.F[j] = CEXP((sample0 + 1.0) * pick(c.lnr, j, NB));
        if (RC::kBP) R.bpa = sample0 + 1.0;
    } else if (MODE == CH_LOGN_W) {
        {
            const double lp = log_pos(sample0);
#pragma unroll
            for (int j = 0; j < NB; ++j) R.F[j] = pick(c.lnu9, j, NB) - lp;
        }
    }
    const double other = first ? sample1 : sample0;  // the index that is not sampled
    // --- chain (gaussian / uniform prior inline; JEFF: the prior of an evaluation is jprior of the sum it left in R.jS; every
    // other Jeffreys configuration keeps the LDS form, decided on the host side)
    const unsigned long long gpix = (unsigned long long)(M.pix0 + i);
    const int q = a.nind;
    const bool gauss = c.prior_type[q] == DANGX_PRIOR_GAUSSIAN;
    const double pmean = c.gauss[q][0], pstd = c.gauss[q][1], lgden = c.lgden[q];
    // 1/(2 sigma^2) once per sweep; the proposal then multiplies ((x/d and x*(1/d) differ by <= 1 ulp of the prior term;
    // -DDX_CHAIN_IEEEDIV restores the division: 15 instructions of a ~400-instruction proposal)
    const double inv2v = 1.0 / (2 * (pstd * pstd));
    auto prior = [&](double v) -> double {
        if (!gauss) return 0.0;
#ifdef DX_CHAIN_IEEEDIV
        const double arg = ((v - pmean) * (v - pmean)) / (2 * (pstd * pstd));
#else
        const double arg = ((v - pmean) * (v - pmean)) * inv2v;
#endif
        return (arg > 745.0) ? -INFINITY : -arg - lgden;
    };
    // log(sqrt(S)): S is positive and normal unless the weights are NaN (an amplitude the reference divides by is 0 or not
    // finite) or the SEDs leave the range -- log_pos reads only the bits, those lanes take the library's routine
    auto jprior = [&](double S) -> double {
        double p = log_pos(sqrt(S));
        if (!(S >= 0x1p-1022 && S < INFINITY)) p = log(sqrt(S));
        return p;
    };
    unsigned long long nacc = 0;
    double cur = first ? sample0 : sample1;
    double a0, a1, c0, c1;
    const double step = c.step[q], lo = c.uni[q][0], hi = c.uni[q][1];
    const bool ml_opt = (a.ml_mode == DANGX_ML_OPTIMIZE);
    // the certified cheap likelihood (RegChain::lnl_cheap / cheap_bound): delta-band power law and modified
    // blackbody chains decide a step from an interval of the fp64 chain's diff and evaluate lnL exactly only for lanes whose
    // decision the interval cannot settle; -DDX_LNL_EXACT restores the exact evaluation of every proposal
#if defined(DX_LNL_EXACT) || !defined(DX_CHAIN_SCALED)
    constexpr bool kCert = false;
#else
    // (not for JEFF: the interval bounds the likelihood only, the prior moves with the SED too)
    constexpr bool kCert = !RC::kBP && !JEFF && (MODE == CH_POW || MODE == CH_MBB_BETA || MODE == CH_MBB_T);
#endif
    auto chain = [&](auto batch_tag) {
        constexpr bool B = decltype(batch_tag)::value;
        double lnl;
        if (acc_in) { a0 = acc_in[0]; a1 = acc_in[1]; lnl = a0 + a1; if (JEFF) R.jeff_eval(M, c, cur); }
        else if constexpr (ADD && RC::kKept) {
            if (scol) lnl = R.lnl_add_kept(scol, a0, a1);
            else lnl = R.template lnl<B, 1>(M, c, cur, other, a0, a1);
        }
        else lnl = R.template lnl<B, ADD ? 1 : 0>(M, c, cur, other, a0, a1);
        chi[0] = -2.0 * a0; chi[1] = -2.0 * a1;
        double lnl_old = lnl + (JEFF ? jprior(R.jS) : prior(cur));
        // cheap path state: lnl_old is exact (old_exact) or within wold of the exact chain's; a0 / a1 are the sums of the
        // state at cur (sums_exact) or must be evaluated there after the loop
        bool cert = false, old_exact = true, sums_exact = true;
        double wA = 0.0, wG = 0.0, wold = 0.0;
        if (kCert) {
            const bool ok = R.cheap_bound(M, c, lo, hi, -2.0 * lnl, wA, wG) && !ml_opt;
            cert = __builtin_amdgcn_ballot_w64(!ok) == 0ull;   // one decision per wavefront
        }
        // one step from the proposal and the accept uniform (:414-454; u3: the uniform's word)
        auto mh_step = [&](double prop, uint32_t u3) {
            if (prop < lo || prop > hi) return;                        // :415
            if constexpr (!kCert) {
                lnl = R.template lnl<B>(M, c, prop, other, c0, c1);
                const double lnl_new = lnl + (JEFF ? jprior(R.jS) : prior(prop));
                const double diff = lnl_new - lnl_old;
                const bool acc = ml_opt ? (diff > 0.0) : mh_accept(diff, u3);  // :443-454
                if (acc) { cur = prop; lnl_old = lnl_new; a0 = c0; a1 = c1; ++nacc; }
            } else {
                const double pp = prior(prop);
                bool acc = false, und = true;
                double lc = 0.0, wc = 0.0;
                if (cert) {
                    // the fp64 chain's diff d = (lnl + pp) - lnl_old, with |lnl - lc| <= wc and |lnl_old - lold| <= wold: d is
                    // within wc + wold of dc plus the four fp64 roundings of the two diffs (2^-49 of the operands covers them)
                    const double A = R.lnl_cheap(M, c, prop);
                    lc = -0.5 * A;
                    wc = fma(wA, A, wG);
                    const double dc = (lc + pp) - lnl_old;
                    const double W = (wc + wold) * (1.0 + 0x1p-40) + 0x1p-49 * ((fabs(lc) + fabs(pp)) + fabs(lnl_old));
                    und = !mh_certain(dc - W, dc + W, u3, acc);
#ifdef DX_LNL_DIAG
                    lnl_diag_count(0);
                    if (__builtin_amdgcn_ballot_w64(und) != 0ull) lnl_diag_count(1);
#endif
                }
                if (__builtin_amdgcn_ballot_w64(und) != 0ull) {
                    if (und) {
                        // the exact evaluation; after a cheap accept lnl_old is first re-evaluated at cur (the fp64 chain
                        // evaluated that same proposal: the same bits)
                        bool again = !old_exact;
#pragma unroll 1
                        for (;;) {
                            const double l = R.template lnl<B>(M, c, again ? cur : prop, other, c0, c1);
                            if (!again) { lnl = l; break; }
                            lnl_old = l + prior(cur);
                            again = false;
                        }
                        const double lnl_new = lnl + pp;
                        const double diff = lnl_new - lnl_old;
                        acc = ml_opt ? (diff > 0.0) : mh_accept(diff, u3);   // :443-454
                        if (acc) { lnl_old = lnl_new; a0 = c0; a1 = c1; }
                        old_exact = true;
                        wold = 0.0;
                    }
                }
                if (acc) {
                    cur = prop;
                    ++nacc;
                    sums_exact = und;
                    if (!und) { lnl_old = lc + pp; wold = wc; old_exact = false; }
                }
            }
        };
        // (the draw from the Philox words, the accept uniform as word 3: dx_rng.h, mh_accept)
        if (LP == 1 || DX_CHAIN_PAIR_RNG == 0) {
            for (int l = 1; l <= a.nsample; ++l) {
                uint32_t o[4];
                draw_words(a.seed, a.stream, gpix, (uint32_t)l, o);
                mh_step(cur + rand_normal_w(0.0, step, o[0], o[1], o[2]), o[3]);    // :414
            }
        } else {
            // Lane pairs: both lanes of a pixel would draw the SAME numbers for every step (a third of a proposal's instructions).
            // Instead lane h draws for step l + h, and the two steps take their numbers from the lane that made them: the random
            // numbers of a pixel are computed once per TWO steps -- the same draws, the same arithmetic, half the instructions.
            for (int l = 1; l <= a.nsample; l += 2) {
                uint32_t o[4];
                draw_words(a.seed, a.stream, gpix, (uint32_t)(l + half), o);
                const double g = rand_normal_w(0.0, step, o[0], o[1], o[2]);
                const double go = __shfl_xor(g, 1, 64);
                const uint32_t u3 = o[3], uo = (uint32_t)__shfl_xor((int)u3, 1, 64);
                mh_step(cur + (half == 0 ? g : go), half == 0 ? u3 : uo);                          // step l: the even lane's numbers
                if (l + 1 <= a.nsample) mh_step(cur + (half == 0 ? go : g), half == 0 ? uo : u3);  // step l + 1: the odd lane's
            }
        }
        // the sums of the state the chain ends on: the last accepted evaluation's (or the start's if nothing was accepted); after
        // a cheap accept they are an exact evaluation at cur -- the SUB pass computes exactly that residual
        if constexpr (SUB) {
            double s0_, s1_;
            (void)R.template lnl<B, 2>(M, c, cur, other, s0_, s1_);
            if (!sums_exact) { a0 = s0_; a1 = s1_; }
        } else if constexpr (HAND) {
            double s0_, s1_;
            (void)R.template lnl<B, 0, true>(M, c, cur, other, s0_, s1_, hand);
            if (!sums_exact) { a0 = s0_; a1 = s1_; }
        } else if (kCert) {
            if (__builtin_amdgcn_ballot_w64(!sums_exact) != 0ull) {
                if (!sums_exact) (void)R.template lnl<B>(M, c, cur, other, a0, a1);
            }
        }
    };
#ifdef DX_CHAIN_NO_BATCH_RCP
    chain(BoolTag<false>{});
#else
    if (MODE == CH_MBB_T && !RC::kBP) {
        // The chain evaluates the SED at its starting temperature and at proposals inside the hard bounds (:415) only.  If the
        // lowest of those keeps the sum of h nu / (k T) over a tile of five bands below 700, no product of five Planck
        // denominators can overflow and the whole chain takes the batched form; otherwise (T < 0.3 K at 857 GHz, T <= 0) the
        // one-by-one form -- decided once per chain, not per proposal (a branch inside the proposal costs what it saves).
        const double tmin = fmin(lo, cur);
#ifdef DX_BATCH_ALWAYS
        chain(BoolTag<true>{});
#elif defined(DX_BATCH_LANEWISE)
        if (tmin > 0.0 && mbb_z(tmin) * M.mbb_batch_z < 1.0) chain(BoolTag<true>{});
        else chain(BoolTag<false>{});
#else
        // (one decision per WAVEFRONT: the one-by-one form is right for every lane, and a branch the scalar unit takes
        // keeps the loop's control flow free of execution-mask bookkeeping)
        const bool unsafe = !(tmin > 0.0 && mbb_z(tmin) * M.mbb_batch_z < 1.0);
        if (__builtin_amdgcn_ballot_w64(unsafe) == 0ull) chain(BoolTag<true>{});
        else chain(BoolTag<false>{});
#endif
    } else if (MODE == CH_LOGN_NUP || MODE == CH_LOGN_W) {
        // The log-normal SED exp(-(ln(nu / nu_p) / w)^2 / 2): |ln(nu / nu_p)| < 2^11 for normal frequencies, so a width that stays
        // above 2^-16 keeps the argument inside exp_sat's range (2^53) and 1/w inside fast_rcp's; a chain whose width (the
        // fixed one, or the lowest it can propose) is narrower, 0 or NaN takes the forms that hold for every argument -- decided
        // once per chain and wavefront, as above.
        const double wmin = (MODE == CH_LOGN_W) ? fmin(lo, cur) : other;
        const bool unsafe = !(wmin >= 0x1p-16 && wmin < INFINITY);
        if (__builtin_amdgcn_ballot_w64(unsafe) == 0ull) chain(BoolTag<true>{});
        else chain(BoolTag<false>{});
    } else {
        chain(BoolTag<false>{});
    }
#endif
    if (final_value) *final_value = cur;
    if (acc_out) { acc_out[0] = a0; acc_out[1] = a1; }
    if (half != 0) {  // the pair's second lane carries the same chain: its sums and counts are the first lane's
        chi[0] = chi[1] = 0.0;
        return 0ull;
    }
#pragma unroll
    for (int kk = 0; kk < SP; ++kk) out[(long long)(a.s1 + kk - 1) * npix] = cur;  // :465, :483
    chi[2] = -2.0 * a0; chi[3] = -2.0 * a1;
    return nacc;
}

// Staging of a register chain: the component's index values, data_raw (:173-177) and 1/rms of the lane's bands, every
// other component removed (:180-196).  The caller has dealt with masked pixels.
template <int MODE, int SP, int NB, int LP, class RC>
__device__ __forceinline__ void index_chain_stage(const Model& M, const IndexArgs& a, const Comp& c, RC& R,
                                                  const BandPick<LP>& pick, int i, double& sample0, double& sample1) {
    const int npix = M.npix;
    const int jb = pick.half * NB;  // first band of this lane
    R.set_k(M, c, pick);
    load_theta(M, c, i, a.s1, sample0, sample1);  // sample(l) = c%indices(i, map_inds(1), l), :372-377
    // --- stage data_raw (:173-177) and rms: every load issued before the first use
    const long long bstride = (long long)M.nmaps * npix;
#pragma unroll
    for (int kk = 0; kk < SP; ++kk) {
        const int k = a.s1 + kk;
        R.amp[kk] = c.amp[(long long)(k - 1) * npix + i];
        const double* sigp = M.sig + (long long)(k - 1) * npix + i;
        const double* rmsp = M.rms + (long long)(k - 1) * npix + i;
        double rv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            R.D[kk][j] = sigp[(jb + j) * bstride];
            rv[j] = rmsp[(jb + j) * bstride];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (k == 1) R.D[kk][j] = (R.D[kk][j] - pick(M.offset, j, NB)) / pick(M.gain, j, NB);
            R.set_is(kk, j, CDIV(1.0, rv[j]));
        }
    }
    // --- remove every OTHER component (:180-196) in component_list order, next one prefetched
    {
        unsigned om = a.others;
        double na[SP], nt0[SP], nt1[SP];
        auto fetch = [&](int l) {
            const Comp& c2 = M.comp[l];
#pragma unroll
            for (int kk = 0; kk < SP; ++kk) {
                na[kk] = c2.amp[(long long)(a.s1 + kk - 1) * npix + i];
                nt0[kk] = nt1[kk] = 0.0;
                if (!((c2.const_planes >> (a.s1 + kk - 1)) & 1)) load_theta(M, c2, i, a.s1 + kk, nt0[kk], nt1[kk]);
            }
        };
        int l = om ? __builtin_ctz(om) : -1;
        if (l >= 0) fetch(l);
        while (l >= 0) {
            const Comp& c2 = M.comp[l];
            double ca[SP], ct0[SP], ct1[SP];
#pragma unroll
            for (int kk = 0; kk < SP; ++kk) { ca[kk] = na[kk]; ct0[kk] = nt0[kk]; ct1[kk] = nt1[kk]; }
            om &= om - 1;
            const int ln = om ? __builtin_ctz(om) : -1;
            if (ln >= 0) fetch(ln);
            const unsigned cp = (c2.const_planes >> (a.s1 - 1)) & 3u;
            if (SP == 2 && cp == 0 && ct0[0] == ct0[SP - 1] && ct1[0] == ct1[SP - 1]) {
                subtract_other_pair<NB, LP>(M, c2, ca[0], ca[SP - 1], ct0[0], ct1[0], R.D[0], R.D[SP - 1], pick);
            } else {
#pragma unroll
                for (int kk = 0; kk < SP; ++kk) subtract_other<NB, LP>(M, c2, a.s1 + kk, ca[kk], ct0[kk], ct1[kk], R.D[kk], pick);
            }
            l = ln;
        }
    }
}

// NB = bands per lane (all of them for LP == 1, half for LP == 2); half = which half this lane owns
template <int MODE, int SP, int NB, int LP, bool JF = false>
__device__ __forceinline__ unsigned long long index_chain_reg(const Model& M, const IndexArgs& a, int i, int half, double chi[4]) {
    const int npix = M.npix;
    const Comp& c = M.comp[a.comp];
    double* out = c.idx + ((long long)a.nind * M.nmaps) * npix + i;
    if (is_masked(M.mask[i])) {  // :362 cycle; index_map stays 0 (:223) and is copied back (:480-483)
        if (half == 0) {
#pragma unroll
            for (int kk = 0; kk < SP; ++kk) out[(long long)(a.s1 + kk - 1) * npix] = 0.0;
        }
        return 0ull;
    }
    const BandPick<LP> pick = {half};
    RegChain<MODE, SP, NB, LP, false, false, JF> R;
    double sample0, sample1;
    index_chain_stage<MODE, SP, NB, LP>(M, a, c, R, pick, i, sample0, sample1);
    return chain_finish<MODE, SP, NB, LP>(M, a, c, R, pick, sample0, sample1, i, half, chi);
}

// Two consecutive sweeps of ONE component on the same planes -- index nind, then index nind + 1 (the dust beta and dust T
// sweeps of every configuration) -- in one pass: nothing the second sweep removes from the data has changed (only the
// component's own index did), so its staged planes ARE the first sweep's; it needs a new chain-invariant factor and its
// own chain.  Same numbers as the two sweeps, bit for bit (the second sweep would have staged exactly these planes).
template <int MODEA, int MODEB, int SP, int NB, int LP>
__device__ __forceinline__ void index_chain_pair(const Model& M, const IndexArgs& a, const IndexArgs& b, int i, int half, double chi[4],
                                                 unsigned long long& nacc_a, unsigned long long& nacc_b) {
    const int npix = M.npix;
    const Comp& c = M.comp[a.comp];
    nacc_a = nacc_b = 0ull;
    if (is_masked(M.mask[i])) {
        if (half == 0) {
#pragma unroll
            for (int kk = 0; kk < SP; ++kk) {
                c.idx[((long long)a.nind * M.nmaps + (a.s1 + kk - 1)) * npix + i] = 0.0;
                c.idx[((long long)b.nind * M.nmaps + (a.s1 + kk - 1)) * npix + i] = 0.0;
            }
        }
        return;
    }
    const BandPick<LP> pick = {half};
    RegChain<MODEA, SP, NB, LP> RA;
    double sample0, sample1;
    index_chain_stage<MODEA, SP, NB, LP>(M, a, c, RA, pick, i, sample0, sample1);
    double chia[4] = {0.0, 0.0, 0.0, 0.0}, chib[4] = {0.0, 0.0, 0.0, 0.0}, va;
    nacc_a = chain_finish<MODEA, SP, NB, LP>(M, a, c, RA, pick, sample0, sample1, i, half, chia, &va);
    RegChain<MODEB, SP, NB, LP> RB;
    RB.set_k(M, c, pick);
#pragma unroll
    for (int kk = 0; kk < SP; ++kk) {
        RB.amp[kk] = RA.amp[kk];
#pragma unroll
        for (int j = 0; j < NB; ++j) { RB.D[kk][j] = RA.D[kk][j]; RB.ISr[kk][j] = RA.ISr[kk][j]; }
    }
    if (a.nind == 0) sample0 = va; else sample1 = va;
    nacc_b = chain_finish<MODEB, SP, NB, LP, false>(M, b, c, RB, pick, sample0, sample1, i, half, chib);
    chi[0] = chia[0]; chi[1] = chia[1]; chi[2] = chib[2]; chi[3] = chib[3];
}

}  // namespace
