// dx_hist_host.h -- the definitions of the per-pixel posterior histograms (dangx_moments_hist, include/dangx.h): the bin of a
// sample (with one range for the shard or with a range per pixel), the quantile walk, the mode, the counter limit and the check of
// a registration list.  k_moments_hist / k_hist_stat of
// dangx_moments.hip and every host-side check evaluate the SAME inline functions, and a stand-alone host program can include
// this file without the HIP runtime.
//
// A pixel's record is nbins counters of `bits` bits, bin 0 first; with bits = 16 two bins share a 32-bit word, the even bin in
// the low half.  Records are read and written as 32-bit words only.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#ifndef DX_HD
#if defined(__HIPCC__)
#define DX_HD __host__ __device__ __forceinline__
#else
#define DX_HD inline
#endif
#endif

#define DX_HIST_MAX 32          // == DANGX_MAX_HIST (include/dangx.h)
#define DX_HIST_MAX_Q 16        // quantiles of one read-out
#define DX_HIST_MAX_BYTES 128   // a record never crosses a 128-byte memory request
#define DX_HIST_SIGNAL (-1)     // == DANGX_HIST_SIGNAL: planes[r] = {sig, DX_HIST_SIGNAL, 0} reads registered signal sig, not a state plane

// x is counted iff it lies in the closed range: NaN fails both comparisons, +-inf one of them
DX_HD bool dx_hist_counted(double x, double lo, double hi) { return x >= lo && x <= hi; }

// scale = nbins / (hi - lo), formed once on the host in f64
inline double dx_hist_scale(double lo, double hi, int nbins) { return (double)nbins / (hi - lo); }

// bin of a counted sample.  A subtraction feeding a multiplication: nothing here can be contracted into an fma, so a float64
// restatement gives the same integer for every input
DX_HD int dx_hist_bin(double x, double lo, double scale, int nbins) {
    const int b = (int)((x - lo) * scale);
    return b < nbins - 1 ? b : nbins - 1;
}

// 32-bit words of a record, and the word / the increment of bin b in it
DX_HD int dx_hist_words(int nbins, int bits) { return nbins * bits / 32; }
DX_HD int dx_hist_word_of(int b, int bits) { return bits == 16 ? b >> 1 : b; }
DX_HD uint32_t dx_hist_one(int b, int bits) { return bits == 16 ? 1u << ((b & 1) * 16) : 1u; }
DX_HD uint32_t dx_hist_count(const uint32_t* rec, int b, int bits) {
    return bits == 16 ? (rec[b >> 1] >> ((b & 1) * 16)) & 0xffffu : rec[b];
}

// samples a counter of this width takes: accumulation refuses the sample that would exceed it
DX_HD long long dx_hist_limit(int bits) { return (1ll << bits) - 1; }

// lo + width * t with the product rounded before the sum (never an fma): the edges lo + width * b of a bin, restated the same
// way, then bracket every value of that bin
DX_HD double dx_hist_value(double lo, double width, double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = width * t;
    return lo + p;
}

// one bin of the quantile walk: c = the bin's count, cum = the sum before it (updated).  True when bin b is the first with
// c > 0 && cum + c >= target; out is then the quantile.  CT: uint32_t for one record, a 64-bit count for the bins of several
// chains summed (dangx_chains_hist_stat): the same expression for both
template <class CT>
DX_HD bool dx_hist_qstep(CT c, int b, double target, unsigned long long& cum, double lo, double width, double& out) {
    if (c > 0 && (double)(cum + c) >= target) {
        out = dx_hist_value(lo, width, (double)b + (target - (double)cum) / (double)c);
        return true;
    }
    cum += c;
    return false;
}

// one bin of the mode search: the fullest bin, the lowest on ties (best_c starts at 0, best_b at -1)
template <class CT>
DX_HD void dx_hist_mstep(CT c, int b, CT& best_c, int& best_b) {
    if (c > best_c) { best_c = c; best_b = b; }
}

DX_HD double dx_hist_mode_value(int best_b, double lo, double width) {
    return best_b < 0 ? (double)NAN : dx_hist_value(lo, width, (double)best_b + 0.5);
}

// ---- per-pixel ranges: a registration declared with range = {-inf, +inf} takes its bounds from two f64 maps lo[p], hi[p]
// (dangx_moments_hist_range_maps).  Every rule above holds with that pixel's bounds; the scale is formed per sample, one IEEE division.

#define DX_HIST_RANGE_GLOBAL 0   // one (lo, hi) for the whole shard
#define DX_HIST_RANGE_PIXEL 1    // lo[p], hi[p]

// range[r] = {-inf, +inf}: "per-pixel maps follow"
inline int dx_hist_range_kind(double lo, double hi) {
    return (std::isinf(lo) && lo < 0.0 && std::isinf(hi) && hi > 0.0) ? DX_HIST_RANGE_PIXEL : DX_HIST_RANGE_GLOBAL;
}

DX_HD double dx_hist_pixel_scale(double lo, double hi, int nbins) { return (double)nbins / (hi - lo); }

// pixel p is ON: both bounds finite, hi > lo, and neither hi - lo nor nbins / (hi - lo) overflows -- what dx_hist_check asks of a
// global range.  An off pixel (a masked one handed in as NaN is the normal case) counts nothing; its quantile and mode are NaN.
DX_HD bool dx_hist_pixel_on(double lo, double hi, int nbins) {
    return __builtin_isfinite(lo) && __builtin_isfinite(hi) && hi > lo && __builtin_isfinite(hi - lo) &&
           __builtin_isfinite(dx_hist_pixel_scale(lo, hi, nbins));
}

// bin of sample x at a pixel with bounds lo, hi; -1: not counted (an off pixel, or x outside the closed range)
DX_HD int dx_hist_pixel_bin(double x, double lo, double hi, int nbins) {
    if (!dx_hist_pixel_on(lo, hi, nbins) || !dx_hist_counted(x, lo, hi)) return -1;
    return dx_hist_bin(x, lo, dx_hist_pixel_scale(lo, hi, nbins), nbins);
}

// checksum of a pair of range maps: FNV-1a (64 bit) over the little-endian 64-bit words of lo[0..n) then hi[0..n).  Part of what
// "the same registration" means between chains and between a saved run and the context it is loaded into.
inline uint64_t dx_hist_range_checksum(const double* lo, const double* hi, long long n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (int part = 0; part < 2; ++part) {
        const double* v = part == 0 ? lo : hi;
        for (long long i = 0; i < n; ++i) {
            uint64_t u;
            std::memcpy(&u, &v[i], sizeof u);
            for (int k = 0; k < 8; ++k) {
                h ^= (u >> (8 * k)) & 0xffu;
                h *= 0x100000001b3ull;
            }
        }
    }
    return h;
}

// the whole walks over one record in memory (host checks; k_hist_stat takes the same steps over 16-byte pieces)
DX_HD unsigned long long dx_hist_total(const uint32_t* rec, int nbins, int bits) {
    unsigned long long n = 0;
    for (int b = 0; b < nbins; ++b) n += dx_hist_count(rec, b, bits);
    return n;
}

DX_HD double dx_hist_quantile(const uint32_t* rec, int nbins, int bits, double lo, double hi, double q) {
    const unsigned long long N = dx_hist_total(rec, nbins, bits);
    if (N == 0) return (double)NAN;
    const double target = q * (double)N, width = (hi - lo) / (double)nbins;
    unsigned long long cum = 0;
    double out = (double)NAN;
    for (int b = 0; b < nbins; ++b)
        if (dx_hist_qstep(dx_hist_count(rec, b, bits), b, target, cum, lo, width, out)) break;
    return out;
}

DX_HD double dx_hist_mode(const uint32_t* rec, int nbins, int bits, double lo, double hi) {
    uint32_t best_c = 0;
    int best_b = -1;
    for (int b = 0; b < nbins; ++b) dx_hist_mstep(dx_hist_count(rec, b, bits), b, best_c, best_b);
    return dx_hist_mode_value(best_b, lo, (hi - lo) / (double)nbins);
}

// the shape of a record: "" = fine, else the cause
inline std::string dx_hist_shape_check(int nbins, int bits) {
    if (nbins != 8 && nbins != 16 && nbins != 32 && nbins != 64) return "nbins must be 8, 16, 32 or 64";
    if (bits != 16 && bits != 32) return "bits must be 16 or 32";
    if (nbins * bits / 8 > DX_HIST_MAX_BYTES)
        return "a record of " + std::to_string(nbins * bits / 8) + " bytes exceeds 128 bytes (nbins * bits / 8 <= 128)";
    return "";
}

// planes[r] = {comp, what, plane} and range[r] = {lo, hi} AFTER the defaults were filled in (has_range[r] == 0: an amplitude plane
// that was given none) against the selection words sel[ncomp], nind[l] = indices of component l, global[l] != 0: template /
// monopole / hi_fit member.  kind (optional): kind[r] == DX_HIST_RANGE_PIXEL: the registration takes per-pixel maps, range[r] is the
// {-inf, +inf} that declared it and is not a pair of bounds.  nsig (optional, >= 0: the caller knows signal sources): the number of
// signals registered now; planes[r] = {sig, DX_HIST_SIGNAL, 0} then reads signal sig, which has no default range.  "" = fine, else
// the cause.
inline std::string dx_hist_check(int nreg, const int32_t* planes, const double* range, const int* has_range, int nbins, int bits,
                                 int ncomp, int nmaps, const int32_t* sel, const int* nind, const int* global, const int* kind = nullptr,
                                 int nsig = -1) {
    if (nreg < 0) return "the number of registrations is negative";
    if (nreg > DX_HIST_MAX) return "more than DANGX_MAX_HIST (" + std::to_string(DX_HIST_MAX) + ") registrations";
    const std::string shape = dx_hist_shape_check(nbins, bits);
    if (!shape.empty()) return shape;
    if (nreg > 0 && !planes) return "no plane list given";
    for (int r = 0; r < nreg; ++r) {
        const int32_t* p = planes + 3 * r;
        const std::string at = "registration " + std::to_string(r) + ": ";
        const int l = p[0], w = p[1], k = p[2];
        const bool signal = nsig >= 0 && w == DX_HIST_SIGNAL;
        if (signal) {
            if (nsig == 0) return at + "a signal source, and no signals are registered (dangx_moments_signals comes first)";
            if (l < 0 || l >= nsig) return at + "signal index out of range (" + std::to_string(nsig) + " signals registered)";
            if (k != 0) return at + "the third word of a signal source must be 0";
            if (!has_range[r]) return at + "a signal source has no default range: it needs an explicit range or range maps";
        } else {
        if (l < 0 || l >= ncomp) return at + "component index out of range";
        if (w < 0 || w > nind[l]) return at + "what must be 0 (amplitude) or 1 + index number of the component";
        if (k < 0 || k >= nmaps) return at + "plane out of range";
        if (w == 0 && global[l]) return at + "a template / monopole / hi_fit amplitude is not a pixel plane";
        if (!((sel[l] >> (w == 0 ? k : 3 + 3 * (w - 1) + k)) & 1)) return at + "a plane that is not selected";
        if (!has_range[r]) return at + "an amplitude plane needs an explicit range";
        }
        if (!(kind && kind[r] == DX_HIST_RANGE_PIXEL)) {
            const double lo = range[2 * r], hi = range[2 * r + 1];
            if (!std::isfinite(lo) || !std::isfinite(hi)) return at + "a non-finite bound";
            if (!(hi > lo)) return at + "the range needs hi > lo";
            if (!std::isfinite(dx_hist_scale(lo, hi, nbins)) || !std::isfinite(hi - lo)) return at + "a non-finite bound (hi - lo overflows)";
        }
        for (int o = 0; o < r; ++o)
            if (planes[3 * o] == l && planes[3 * o + 1] == w && planes[3 * o + 2] == k) return at + (signal ? "the same signal twice" : "the same plane twice");
    }
    return "";
}

// the sample count after the next accumulation against the counter width: "" = fine
inline std::string dx_hist_limit_check(long long new_count, int bits) {
    if (new_count > dx_hist_limit(bits))
        return "sample " + std::to_string(new_count) + " exceeds the limit of " + std::to_string(dx_hist_limit(bits)) + " samples of " +
               std::to_string(bits) + "-bit histogram counters";
    return "";
}
