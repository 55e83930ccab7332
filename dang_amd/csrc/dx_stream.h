// dx_stream.h -- device: the one loop by which the posterior-statistics kernels (dangx_moments.hip, dangx_chains.hip) visit a plane
// of doubles, and the one read-out loop over a pixel's histogram record.
//
// dx_stream: the blocks of a launch (blockIdx.x) stride over a plane of n doubles as 16-byte pairs.  The caller decides `vec` --
// every pointer it touches shares one 16-byte phase -- and names the address whose phase that is: a plane off the 16-byte grid
// shifts by its head element, thread 0 takes that odd first element and thread 1 the odd last one; without `vec` the plane goes
// element by element.  elem(i) handles element i, pair(i) elements i and i + 1 (i at phase 0); both evaluate the same
// expressions, so a result does not depend on which of them an element meets, i.e. on shard boundaries or buffer alignment.
//
// k_moments_signal (both forms) does NOT come through here: its item loop is scheduled by hand around the SED's register budget.
// Nor does k_chains_stat, which measured slower through it (the comment there); every other plane kernel does.
#pragma once
#include <cstdint>

#include "dx_args.h"
#include "dx_hist_host.h"

typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) dbl2 GD2;       // two doubles in global memory
typedef __attribute__((address_space(1))) uint32_t GU32;  // a 32-bit word in global memory
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 GU4;      // a 16-byte piece of a histogram record in global memory

__device__ __forceinline__ uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// load / store V consecutive doubles: one element through the pointer as it is, two as ONE 16-byte global access
template <int V> struct ChV;
template <> struct ChV<1> {
    static __device__ __forceinline__ void ld(const double* p, double (&v)[1]) { v[0] = *p; }
    static __device__ __forceinline__ void st(double* p, const double (&v)[1]) { *p = v[0]; }
};
template <> struct ChV<2> {
    static __device__ __forceinline__ void ld(const double* p, double (&v)[2]) { const dbl2 t = *(const GD2*)p; v[0] = t.x; v[1] = t.y; }
    static __device__ __forceinline__ void st(double* p, const double (&v)[2]) { *(GD2*)p = dbl2{v[0], v[1]}; }
};

template <class Elem, class Pair>
__device__ __forceinline__ void dx_stream(long long n, bool vec, uintptr_t phase_of, Elem elem, Pair pair) {
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    if (!vec) {   // no common 16-byte phase: element by element
        for (long long i = gid; i < n; i += stride) elem(i);
        return;
    }
    const long long head = ((phase_of & 15) != 0 && n > 0) ? 1 : 0;
    const long long npair = (n - head) / 2, tail = head + 2 * npair;   // tail < n: one element after the last pair
    if (gid == 0 && head) elem(0);
    if (gid == 1 && tail < n) elem(tail);
    for (long long p = gid; p < npair; p += stride) pair(head + 2 * p);
}

// The read-out of histogram records (k_hist_stat: one chain's; k_chains_hist: the sum of several chains'): a lane walks its own
// pixel's bins once for N and the mode, once more per quantile (those passes hit the cache).  a: the kernel's arguments (q, out,
// lo, hi, n, nbins, stat, nq); walk(i, f): f(count, bin) per bin of pixel i in bin order until f says stop; CT: its count type.
// PX: the registration has per-pixel ranges -- a carries lo_map / hi_map [n] beside the rest, a lane takes its pixel's bounds
// from them, and an off pixel (dx_hist_pixel_on) gives NaN for quantile and mode whatever its record holds.
template <bool PX, class CT, class Args, class Walk>
__device__ __forceinline__ void dx_hist_readout_impl(const Args& a, Walk walk) {
    double lo = a.lo, width = (a.hi - a.lo) / (double)a.nbins;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
        bool on = true;
        if constexpr (PX) {
            const double hi = a.hi_map[i];
            lo = a.lo_map[i];
            on = dx_hist_pixel_on(lo, hi, a.nbins);
            width = (hi - lo) / (double)a.nbins;
        }
        unsigned long long N = 0;
        CT best_c = 0;
        int best_b = -1;
        walk(i, [&](CT c, int b) { N += c; dx_hist_mstep(c, b, best_c, best_b); return false; });
        if (a.stat == 1) { a.out[i] = dx_hist_mode_value(on ? best_b : -1, lo, width); continue; }
        if (a.stat == 2) { a.out[i] = (double)N; continue; }
        for (int j = 0; j < a.nq; ++j) {
            double val = (double)NAN;
            if (N > 0 && on) {
                const double target = a.q[j] * (double)N;
                unsigned long long cum = 0;
                walk(i, [&](CT c, int b) { return dx_hist_qstep(c, b, target, cum, lo, width, val); });
            }
            a.out[(long long)j * a.n + i] = val;
        }
    }
}

template <class CT, class Args, class Walk>
__device__ __forceinline__ void dx_hist_readout(const Args& a, Walk walk) { dx_hist_readout_impl<false, CT>(a, walk); }
