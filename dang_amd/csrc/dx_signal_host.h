// dx_signal_host.h -- the parts of the posterior component-signal moments (dangx_moments_signals, include/dangx.h) that need no
// device: the check of a signal list against the model's shape, the grouping of the signals into the segments k_moments_signal
// works on, and the two rounded expressions of a sample.  dangx_moments.hip and every host-side check evaluate the SAME inline
// functions, and a stand-alone host program can include this file without the HIP runtime.
//
// A signal is spec[s] = {comp, band, kind}: kind 0, 1, 2 = plane T, Q, U of eval_signal(band, pix, plane) of component comp
// (src/dang_component_mod.f90:754-776), kind 3 = P = sqrt(Q^2 + U^2) of that signal (nmaps == 3 only).
// A segment is one (component, plane class) -- class 0: T, class 1: Q+U -- with at most DX_SIG_SEG_BANDS bands, each band with the
// outputs wanted of it: a thread reads a pixel's amplitude and index values once per segment and evaluates the SED once per band.
#pragma once
#include <cmath>
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

#define DX_SIG_MAX 64         // == DANGX_MAX_SIGNALS (include/dangx.h)
#define DX_SIG_SEG_BANDS 8    // bands of one segment

// amplitude * sed, ROUNDED as a product: the subtraction of Welford's update that follows must not fuse it into an fma, or the
// sample is no longer the number a host restatement forms
DX_HD double dx_signal_product(double amp, double sed) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = amp * sed;
    return p;
}

// P = sqrt(sQ^2 + sU^2) of the two rounded samples: two rounded products, a rounded sum, sqrt
DX_HD double dx_signal_pol(double sq, double su) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = sq * sq;
    const double b = su * su;
    const double s = a + b;
    return sqrt(s);
}

// output slot of a kind inside its class: T -> 0; Q, U, P -> 0, 1, 2
DX_HD int dx_signal_class(int kind) { return kind == 0 ? 0 : 1; }
DX_HD int dx_signal_slot(int kind) { return kind == 0 ? 0 : kind - 1; }

struct DxSigBand {
    int band;
    int sig[3];       // the signal that wants output slot o of this band, or -1
};

struct DxSigSeg {
    int comp, cls, nb;
    DxSigBand b[DX_SIG_SEG_BANDS];
};

// spec[s] = {comp, band, kind} against the model: set[l] != 0: component l is set, global[l] != 0: template / monopole / hi_fit
// member.  "" = fine, else the cause.
inline std::string dx_signal_check(int nsig, const int32_t* spec, int ncomp, int nbands, int nmaps, const int* set, const int* global) {
    if (nsig < 0) return "the number of signals is negative";
    if (nsig > DX_SIG_MAX) return "more than DANGX_MAX_SIGNALS (" + std::to_string(DX_SIG_MAX) + ") signals";
    if (nsig > 0 && !spec) return "no signal list given";
    for (int s = 0; s < nsig; ++s) {
        const int l = spec[3 * s], j = spec[3 * s + 1], kind = spec[3 * s + 2];
        const std::string at = "signal " + std::to_string(s) + ": ";
        if (l < 0 || l >= ncomp) return at + "component index out of range";
        if (!set[l]) return at + "the component is not set";
        if (j < 0 || j >= nbands) return at + "band index out of range";
        if (kind < 0 || kind > 3) return at + "kind must be 0, 1, 2 (plane T, Q, U) or 3 (P)";
        if (kind == 3 ? nmaps != 3 : kind >= nmaps) return at + (kind == 3 ? "P needs nmaps == 3" : "a plane the model does not have");
        if (global[l])
            return at + "the signal of a template / monopole / hi_fit member is its amplitude (dangx_moments_get_template) times a fixed map";
        for (int o = 0; o < s; ++o)
            if (spec[3 * o] == l && spec[3 * o + 1] == j && spec[3 * o + 2] == kind) return at + "the same signal twice";
    }
    return "";
}

// the segments of a checked list: components in ascending order, class T before Q+U, the bands of a (component, class) in
// ascending order, DX_SIG_SEG_BANDS to a segment
inline std::vector<DxSigSeg> dx_signal_plan(int nsig, const int32_t* spec, int ncomp, int nbands) {
    std::vector<DxSigSeg> segs;
    for (int l = 0; l < ncomp; ++l)
        for (int cls = 0; cls < 2; ++cls) {
            DxSigSeg cur{l, cls, 0, {}};
            for (int j = 0; j < nbands; ++j) {
                DxSigBand b{j, {-1, -1, -1}};
                bool any = false;
                for (int s = 0; s < nsig; ++s)
                    if (spec[3 * s] == l && spec[3 * s + 1] == j && dx_signal_class(spec[3 * s + 2]) == cls) {
                        b.sig[dx_signal_slot(spec[3 * s + 2])] = s;
                        any = true;
                    }
                if (!any) continue;
                cur.b[cur.nb++] = b;
                if (cur.nb == DX_SIG_SEG_BANDS) {
                    segs.push_back(cur);
                    cur = DxSigSeg{l, cls, 0, {}};
                }
            }
            if (cur.nb) segs.push_back(cur);
        }
    return segs;
}
