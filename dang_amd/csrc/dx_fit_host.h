// dx_fit_host.h -- the parts of the posterior goodness-of-fit moments (dangx_moments_fit, include/dangx.h) that need no device: the
// check of an item list against the model's shape, the grouping of the items into the segments k_moments_fit works on, and the
// rounded expressions of a sample.  dangx_moments.hip and every host-side check evaluate the SAME inline functions, and a
// stand-alone host program can include this file without the HIP runtime.
//
// An item is spec[i] = {what, band, plane}, plane 0, 1, 2 = T, Q, U:
//   what 0  the residual of band `band` on that plane -- what write_maps' <band>_residual_k*.fits hold (src/dang_data_mod.f90:
//           619-634) and scripts/make_mean_maps.py averages into <band>_residual_mean.fits
//   what 1  the chi^2 map of that plane (chisq_k*.fits, :656-662, into chisq_mean.fits); band must be -1
// One sample at pixel p of plane k, in the expressions of update_sky_model + compute_chisq (src/dang_data_mod.f90:339-396,
// 494-526) as k_sky_chisq (dangx_entry.hip) evaluates them:
//   x_c(j)  the signal of component c at band j: dx_fit_product(amplitude, sed) of a diffuse member, dx_fit_product(
//           template_amplitudes(j, k), sed) of a template / hi_fit member, the bare sed of T_cmb; a monopole is skipped (it lives in
//           the band offset).  The product is ROUNDED: it never fuses into the sum that follows.
//   sky_j   = ((0.0 + x_0(j)) + x_1(j)) + ...  in component_list order
//   r_j     = dx_fit_residual: (sig - offset_j) / gain_j - sky_j on T, sig - sky_j on Q and U; at EVERY pixel, masked ones included
//   chi^2   = dx_fit_chisq(sum_j dx_fit_chi_term(r_j, rms_j), nbands) over ALL bands in band order, whichever residuals are
//           registered; taken at unmasked pixels only (the mask of plane T, as compute_chisq tests it).  At a masked pixel nothing
//           is accumulated and the read-outs give 0, as the reference's chi_map does.
//   A NaN / inf sample propagates; nothing else is skipped (no amp == 0 shortcut).
// Units are the model's (uK_RJ), as dangx_sky_model_chisq returns them: the division by conversion(j) that write_maps applies to a
// residual stays with the caller.
// The update is k_moments_accum's (Welford) on two f64 planes per item of the library's own, zero-filled: 16 B x npix per item.
// "Everything" (every plane's chi^2 map and every band's residual) is 33 items = 6.6 GB at the C3 workload (Nside 1024, 10 bands,
// IQU) and 63 items = 50 GB at C5 (Nside 2048, 20 bands): register what is looked at.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#ifndef DX_HD
#if defined(__HIPCC__)
#define DX_HD __host__ __device__ __forceinline__
#else
#define DX_HD inline
#endif
#endif

#define DX_FIT_MAX 128        // == DANGX_MAX_FIT (include/dangx.h)
#define DX_FIT_RESIDUAL 0
#define DX_FIT_CHISQ 1

// amplitude * sed, ROUNDED as a product (dx_signal_product's rule: the sum that follows must not fuse it into an fma)
DX_HD double dx_fit_product(double amp, double sed) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = amp * sed;
    return p;
}

// the running sky model: a rounded sum
DX_HD double dx_fit_sky_add(double sky, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s = sky + x;
    return s;
}

// plane 0 (T): the calibrated datum minus the model; planes 1, 2: the datum minus the model
DX_HD double dx_fit_residual(int plane, double sig, double offset, double gain, double sky) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (plane == 0) {
        const double d = sig - offset;
        const double c = d / gain;
        return c - sky;
    }
    return sig - sky;
}

// one band's term (r r) / (rms rms): two rounded products and an IEEE division
DX_HD double dx_fit_chi_term(double r, double rms) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = r * r;
    const double b = rms * rms;
    return a / b;
}

// the running sum over the bands, and the sample: the sum over nbands
DX_HD double dx_fit_chi_add(double chi, double term) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s = chi + term;
    return s;
}
DX_HD double dx_fit_chisq(double sum, int nbands) { return sum / nbands; }

struct DxFitSeg {             // a plane with at least one item
    int plane;
    int chi;                  // the chi^2 item of the plane, or -1
    std::vector<int> res;     // [nbands]: the residual item of band j, or -1
};

// spec[i] = {what, band, plane} against the model's shape.  "" = fine, else the cause, naming the item.
inline std::string dx_fit_check(int nfit, const int32_t* spec, int nbands, int nmaps) {
    if (nfit < 0) return "the number of fit items is negative";
    if (nfit > DX_FIT_MAX) return "more than DANGX_MAX_FIT (" + std::to_string(DX_FIT_MAX) + ") fit items";
    if (nfit > 0 && !spec) return "no fit item list given";
    for (int i = 0; i < nfit; ++i) {
        const int what = spec[3 * i], band = spec[3 * i + 1], plane = spec[3 * i + 2];
        const std::string at = "fit item " + std::to_string(i) + ": ";
        if (what != DX_FIT_RESIDUAL && what != DX_FIT_CHISQ) return at + "what must be 0 (the residual at a band) or 1 (the chi^2 map)";
        if (plane < 0 || plane > 2) return at + "plane must be 0, 1 or 2 (T, Q, U)";
        if (plane >= nmaps) return at + "a plane the model does not have";
        if (what == DX_FIT_CHISQ && band != -1) return at + "the chi^2 map sums over every band: band must be -1";
        if (what == DX_FIT_RESIDUAL && (band < 0 || band >= nbands)) return at + "band index out of range";
        for (int o = 0; o < i; ++o)
            if (spec[3 * o] == what && spec[3 * o + 1] == band && spec[3 * o + 2] == plane) return at + "the same fit item twice";
    }
    return "";
}

// the segments of a checked list: planes in ascending order, at most three
inline std::vector<DxFitSeg> dx_fit_plan(int nfit, const int32_t* spec, int nbands) {
    std::vector<DxFitSeg> segs;
    for (int k = 0; k < 3; ++k) {
        DxFitSeg s{k, -1, std::vector<int>((size_t)(nbands > 0 ? nbands : 0), -1)};
        bool any = false;
        for (int i = 0; i < nfit; ++i) {
            if (spec[3 * i + 2] != k) continue;
            any = true;
            if (spec[3 * i] == DX_FIT_CHISQ) s.chi = i;
            else s.res[(size_t)spec[3 * i + 1]] = i;
        }
        if (any) segs.push_back(s);
    }
    return segs;
}
