// dx_schur_host.h -- the host algebra of the direct solve of a CG group with global-amplitude members (device_schur in
// dangx_solve.hip): the row <-> (member, band) tables the Schur kernels take (SchurArgs), the fluctuation term of every row, the
// equilibrated LU with complete pivoting of the small system and the residual norms of a refinement step.  Standard library and
// include/dangx.h only: tests/test_schur_host_cpu.py compiles it into a stand-alone program under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

#include "../../include/dangx.h"

// direct (Schur complement) solve of a group with global-amplitude members; rows <= DX_MAX_ROWS
constexpr int DX_MAX_ROWS = 32;
struct SchurArgs {
    int nrows;
    unsigned char rt[DX_MAX_ROWS], rj[DX_MAX_ROWS];  // row r <-> (global member rt[r], band rj[r])
    signed char ftarget[DX_MAX_ROWS];                // row that receives row r's fluctuation sum (running counter of
                                                     // compute_sample_vector, src/dang_cg_mod.f90:970-1094); -1 = dropped
    signed char bslot[DANGX_MAX_BANDS];              // LDS slot of band j (-1: no global row at that band)
    int nslots;
};

// fn(j, lf) for the fitted bands of one global member, in band order: band j carries the member's lf-th amplitude, global row
// trow + lf (initialize_x, src/dang_cg_mod.f90:1244-1279: the first nfit bands of the corr mask)
template <class F>
inline void dx_fitted_bands(unsigned corr_mask, int nfit, int nbands, F&& fn) {
    int lf = 0;
    for (int j = 0; j < nbands && lf < nfit; ++j)
        if ((corr_mask >> j) & 1) fn(j, lf++);
}

// the tables of a group of nt global members: member t owns rows trow[t] .. trow[t] + nfit[t] - 1 (nrows of them together, at most
// DX_MAX_ROWS: more fill nothing but nrows)
inline SchurArgs dx_schur_rows(int nt, const int* trow, const unsigned* corr_mask, const int* nfit, int nbands) {
    SchurArgs sa{};
    const int R = nt > 0 ? trow[nt - 1] + nfit[nt - 1] : 0;
    sa.nrows = R;
    for (int j = 0; j < DANGX_MAX_BANDS; ++j) sa.bslot[j] = -1;
    if (R > DX_MAX_ROWS) return sa;
    for (int t = 0; t < nt; ++t)
        dx_fitted_bands(corr_mask[t], nfit[t], nbands, [&](int j, int lf) {
            const int r = trow[t] + lf;
            sa.rt[r] = (unsigned char)t; sa.rj[r] = (unsigned char)j; sa.ftarget[r] = -1;
        });
    for (int j = 0; j < nbands; ++j)
        for (int r = 0; r < R; ++r)
            if (sa.rj[r] == j && sa.bslot[j] < 0) sa.bslot[j] = (signed char)sa.nslots++;
    int lrun = 0;  // the running row counter of compute_sample_vector (:970, :1057, :1071, :1094)
    for (int j = 0; j < nbands; ++j)
        for (int t = 0; t < nt; ++t) {
            const unsigned m = corr_mask[t];
            if ((m >> j) & 1) {
                int lt = 0;
                for (int jj = 0; jj < j; ++jj) lt += (m >> jj) & 1;
                if (lt < nfit[t] && lrun < R) sa.ftarget[trow[t] + lt] = (signed char)lrun;
                ++lrun;
            }
        }
    return sa;
}

// fluctuation term of every row from the rows' fluctuation sums fsum[0..R): the reference's through the running-counter mapping of
// compute_sample_vector, the textbook one (DANGX_FLUCT_CORRECT) on the natural rows; zero when nothing is drawn
inline std::vector<double> dx_schur_fluct(const double* fsum, int R, int ml_mode, int fluct, const SchurArgs& sa) {
    std::vector<double> fl(R, 0.0);
    if (ml_mode == DANGX_ML_SAMPLE && fluct != DANGX_FLUCT_REFERENCE)
        for (int r = 0; r < R; ++r) fl[r] = fsum[r];
    else if (ml_mode == DANGX_ML_SAMPLE)
        for (int r = 0; r < R; ++r)
            if (sa.ftarget[r] >= 0) fl[sa.ftarget[r]] += fsum[r];
    return fl;
}

// t + fl - S g0: the residual of the current amplitudes g0, as pass 1 sees it (S row-major R x R, unscaled)
inline std::vector<double> dx_schur_rhs(const double* S, const double* t, const std::vector<double>& fl, const std::vector<double>& g0, int R) {
    std::vector<double> res(R);
    for (int r = 0; r < R; ++r) {
        double v = t[r] + fl[r];
        for (int k = 0; k < R; ++k) v -= S[(size_t)r * R + k] * g0[k];
        res[r] = v;
    }
    return res;
}

// S g = t (+ fluctuation sums).  S is not symmetric when a monopole is fitted (its row weight is 1, :857), so:
// Gaussian elimination, on the system equilibrated by G's diagonal (row amplitudes span ~1e-6 for hi_fit to ~1e2),
// for the CORRECTION to the current amplitudes, S d = t - S g0, with complete pivoting.  A remaining pivot at
// rounding level (1e-10 in units of G's diagonal, where 1 = nothing absorbed by the diffuse members) means the
// global rows are degenerate with the diffuse members -- a template fitted at every band beside a pixel-independent
// SED such as the CMB, or spatially constant index maps (the state a run starts from).  The normal equations stay
// consistent; the free directions keep their current value (d = 0 there), which is what the reference's CG does
// with them too (a Krylov iterate never moves along the null space).
struct DxSchurLU {
    int R, rank = 0;
    int bad_row = -1;        // >= 0: that row of the global block has no support (diagonal zero or not finite); nothing is factored
    bool nonfinite = false;  // a non-finite entry met while pivoting; nothing may be solved
    std::vector<double> S;   // the scaled factors: U on and above the diagonal, the multipliers of L below
    std::vector<double> sc;  // 1 / sqrt(|G[r][r]|)
    std::vector<int> rp, cp; // row / column permutations

    // S_in: row-major R x R; diag[r] = G[r][r] = sum_u w_r s_r / sigma^2, before elimination
    DxSchurLU(const double* S_in, const double* diag, int R_) : R(R_), S(S_in, S_in + (size_t)R_ * R_), sc(R_), rp(R_), cp(R_) {
        for (int r = 0; r < R; ++r) {
            const double dg = std::fabs(diag[r]);
            if (!(dg > 0.0) || !std::isfinite(dg)) { bad_row = r; return; }
            sc[r] = 1.0 / std::sqrt(dg);
        }
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < R; ++k) S[(size_t)r * R + k] *= sc[r] * sc[k];
        // LU with complete pivoting, multipliers kept: rank = the number of pivots
        for (int c = 0; c < R; ++c) rp[c] = cp[c] = c;
        for (int c = 0; c < R; ++c) {
            int pr = c, pc = c;
            double best = -1.0;
            for (int r = c; r < R; ++r)
                for (int k = c; k < R; ++k) {
                    const double v = std::fabs(S[(size_t)r * R + k]);
                    if (!std::isfinite(v)) { nonfinite = true; return; }
                    if (v > best) { best = v; pr = r; pc = k; }
                }
            if (!(best > 1e-10)) break;
            if (pr != c) {
                for (int k = 0; k < R; ++k) std::swap(S[(size_t)pr * R + k], S[(size_t)c * R + k]);
                std::swap(rp[pr], rp[c]);
            }
            if (pc != c) {
                for (int r = 0; r < R; ++r) std::swap(S[(size_t)r * R + pc], S[(size_t)r * R + c]);
                std::swap(cp[pc], cp[c]);
            }
            for (int r = c + 1; r < R; ++r) {
                const double f = S[(size_t)r * R + c] / S[(size_t)c * R + c];
                S[(size_t)r * R + c] = f;  // L below the diagonal
                for (int k = c + 1; k < R; ++k) S[(size_t)r * R + k] -= f * S[(size_t)c * R + k];
            }
            ++rank;
        }
    }
    bool ok() const { return bad_row < 0 && !nonfinite; }

    // d = correction of the global amplitudes for a residual `res` of the (unscaled) global rows; free directions get 0
    void solve(const std::vector<double>& res, std::vector<double>& d) const {
        std::vector<double> y(R);
        for (int r = 0; r < R; ++r) y[r] = res[rp[r]] * sc[rp[r]];
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < std::min(r, rank); ++k) y[r] -= S[(size_t)r * R + k] * y[k];
        std::vector<double> z(R, 0.0);
        for (int r = rank - 1; r >= 0; --r) {
            double v = y[r];
            for (int k = r + 1; k < rank; ++k) v -= S[(size_t)r * R + k] * z[k];
            z[r] = v / S[(size_t)r * R + r];
        }
        d.assign(R, 0.0);
        for (int r = 0; r < rank; ++r) d[cp[r]] = z[r] * sc[cp[r]];
    }
    // the smallest pivot (at most 1): the pivots of complete pivoting bound |S^-1| up to the growth factor of an R x R elimination
    double minpiv() const {
        double m = 1.0;
        for (int c = 0; c < rank; ++c) m = std::min(m, std::fabs(S[(size_t)c * R + c]));
        return m;
    }
};

// one refinement step's view of the global rows.  rr: [0..R) the rows of b - A x at the current state without the fluctuation term,
// [R..2R) those rows of b, [2R..3R) the size of the rows' terms.  res[r] = the full residual; worst: its largest size relative to
// the row of b, worst_bw: relative to the size of the row's terms.  Rows along a free (degenerate) direction cannot be reduced by
// the global amplitudes alone; they are consistent through the diffuse members, so their residual is reported like any other.
struct DxSchurNorms { double worst, worst_bw; };
inline DxSchurNorms dx_schur_norms(const double* rr, const std::vector<double>& fl, int R, std::vector<double>& res) {
    DxSchurNorms n{0.0, 0.0};
    res.resize(R);
    for (int r = 0; r < R; ++r) {
        res[r] = rr[r] + fl[r];
        const double brow = std::fabs(rr[R + r] + fl[r]);
        n.worst = std::max(n.worst, std::fabs(res[r]) / std::max(brow, 1e-300));
        n.worst_bw = std::max(n.worst_bw, std::fabs(res[r]) / std::max(rr[2 * R + r] + std::fabs(fl[r]), 1e-300));
    }
    return n;
}
