// dx_rng.h -- counter-based random streams for the sampler kernels.
//
// The reference draws from the compiler's RANDOM_NUMBER after an unseeded
// RANDOM_SEED() (src/dang.f90:67; rand_normal src/dang_util_mod.f90:100-110),
// which is irreproducible and thread-order dependent.  The MI355X path keys
// every draw by (seed, stream, GLOBAL pixel, draw slot) through Philox4x32-10,
// so a sample does not depend on launch geometry or on how pixels are sharded.
//
//   counter = { pixel[31:0], draw ^ (pixel[63:32] << 16), stream[31:0], stream[63:32] }
//   key     = { seed[31:0], seed[63:32] }
//   u1 = words(0,1), u2 = words(2,3), each mapped to (0,1) with 53 bits.
// Draw slots:
//   amplitude phase, reference fluctuation term : draw = map number k (1..3)
//   amplitude phase, textbook fluctuation term  : draw = k + 4*(band+1)
//   index phase, step l (1..nsample)            : draw = l, ONE Philox call per step (uniform3):
//        proposal normal from u1 = words(0,1) [53 bits] and u2 = word 2 [32 bits];
//        accept uniform u3 = word 3 [32 bits]  (each 32-bit word maps to (w + 0.5) * 2^-32)
//   index phase, lnl_type=='prior' draw         : draw = 0 (uniform2)
#pragma once
#include "dx_rtc_compat.h"
#include "dx_math.h"
#include "dx_model.h"

namespace dx {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
#ifndef DX_PHILOX_MULHI  // one v_mad_u64_u32 per product (4.3 cycles) instead of v_mul_hi_u32 + v_mul_lo_u32 (4.1 + 4.0)
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
#else
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
#endif
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
    const unsigned long long x = ((unsigned long long)hi << 32) | lo;
    return ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ void uniform2(unsigned long long seed, unsigned long long stream,
                                         unsigned long long pix, uint32_t draw, double& u1, double& u2) {
    uint32_t o[4];
    philox4x32_10((uint32_t)pix, draw ^ ((uint32_t)(pix >> 32) << 16), (uint32_t)stream, (uint32_t)(stream >> 32),
                  (uint32_t)seed, (uint32_t)(seed >> 32), o);
    u1 = u53(o[0], o[1]);
    u2 = u53(o[2], o[3]);
}

__device__ __forceinline__ double u32(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

__device__ __forceinline__ void uniform3(unsigned long long seed, unsigned long long stream, unsigned long long pix,
                                         uint32_t draw, double& u1, double& u2, double& u3) {
    uint32_t o[4];
    philox4x32_10((uint32_t)pix, draw ^ ((uint32_t)(pix >> 32) << 16), (uint32_t)stream, (uint32_t)(stream >> 32),
                  (uint32_t)seed, (uint32_t)(seed >> 32), o);
    u1 = u53(o[0], o[1]);
    u2 = u32(o[2]);
    u3 = u32(o[3]);
}

// rand_normal, src/dang_util_mod.f90:100-110 (Box-Muller, sine branch only):
//   r = (-2 log u1)**0.5 ; theta = 2 pi u2 ; c = mean + stdev*r*sin(theta)
// sin(2 pi u2) is evaluated as sinpi(2 u2) (no rounding of theta); log by log_pos (u1 is normal).
__device__ __forceinline__ double rand_normal(double mean, double stdev, double u1, double u2) {
    // u1 in (0,1]: u53 rounds to exactly 1.0 for the one word pattern 2^53 - 1 (probability 2^-53 per draw); the argument
    // is then -0.0, where the reciprocal-square-root seed is -inf and the Goldschmidt steps give NaN -- sqrt(-0) = -0 in
    // the reference's arithmetic, i.e. a zero deviate: select it
    const double arg = -2.0 * log_pos(u1);
    const double r = (arg > 0.0) ? fast_sqrt(arg) : 0.0;
    // one explicit fma: "x + (mean + a*b)" at a call site with mean = 0 could otherwise be contracted into fma(a, b, x) in
    // one kernel and left as a rounded product plus an addition in another (see log_pos)
    return fma(stdev * r, sin_2pi(u2), mean);
}

// ---- The Metropolis step's draw, formed from the Philox words themselves.  The conversions u32 / u53,
// the reduction of sin_2pi and the scalings by powers of two are exact operations on integers that the forms above carry out
// in fp64, at twice the issue cost of a 32-bit instruction; the forms below reach the same bits with fewer of them.
// -DDX_DRAW_FP64 restores the forms above everywhere (or one by one: -DDX_SIN_FP64, -DDX_U1_LDEXP, -DDX_DRAW_BRANCH).
#ifdef DX_DRAW_FP64
#define DX_SIN_FP64 1
#define DX_U1_LDEXP 1
#define DX_DRAW_BRANCH 1
#endif

// the four words of one draw slot: u1 = words(0,1), u2 = word 2, u3 = word 3 (uniform3)
__device__ __forceinline__ void draw_words(unsigned long long seed, unsigned long long stream, unsigned long long pix, uint32_t draw,
                                           uint32_t o[4]) {
    philox4x32_10((uint32_t)pix, draw ^ ((uint32_t)(pix >> 32) << 16), (uint32_t)stream, (uint32_t)(stream >> 32),
                  (uint32_t)seed, (uint32_t)(seed >> 32), o);
}

// sin_2pi(u32(w)), bit for bit, for every word.  t = 2 u32(w) = (2w + 1) 2^-32 has an odd numerator, so rint never meets a
// tie and r = t - rint(t) is never 0: r 2^32 = (2w + 1) - k 2^32 lies in (-2^31, 2^31) and is congruent to 2w + 1, i.e. it is
// the 32-bit pattern (w << 1) | 1 read as a signed integer -- one v_cvt_f64_i32 and an exact scaling.  k == 1 where
// 2^31 < 2w + 1 < 3 2^31, i.e. 2^30 <= w < 3 2^30: bit 31 of w + 2^30; there r changes its sign (r != 0: a flip of the sign
// bit is the negation).  From z = r r on, the operations of sin_2pi.
__device__ __forceinline__ double sin_2pi_w(uint32_t w) {
#ifdef DX_SIN_FP64
    return sin_2pi(u32(w));
#else
    const double r0 = (double)(int)((w << 1) | 1u) * 0x1p-32;
    const uint32_t flip = (w + 0x40000000u) & 0x80000000u;
    const double r = __longlong_as_double(__double_as_longlong(r0) ^ (long long)((unsigned long long)flip << 32));
    const double z = r * r;
    double p = fma_vc(z, 0x1.2877020d52cf0p-31, -0x1.8a404211f9547p-26);
    p = fma_vc(z, p, 0x1.aaec32af93359p-21);
    p = fma_vc(z, p, -0x1.6fadb9f155744p-16);
    p = fma_vc(z, p, 0x1.e8f434d018d63p-12);
    p = fma_vc(z, p, -0x1.e3074fde8871fp-8);
    p = fma_vc(z, p, 0x1.50783487ee782p-4);
    p = fma_vc(z, p, -0x1.32d2cce62bd86p-1);
    p = fma_vc(z, p, 0x1.466bc6775aae2p+1);
    p = fma_vc(z, p, -0x1.4abbce625be53p+2);
    p = fma_vc(z, p, 0x1.921fb54442d18p+1);
    return r * p;
#endif
}

// u32(w) as a float, from the word in two 32-bit instructions: float(w) is within 2^-24 / (1 + 2^-24) of w, so the exact fma
// argument is within that of u32(w), and the fma rounds once more: |u32f_word(w) - u32(w)| < 2^-23 u32(w); 2^-33 for w = 0.
__device__ __forceinline__ float u32f_word(uint32_t w) { return fmaf((float)w, 0x1p-32f, 0x1p-33f); }

// 2^53 u53(hi, lo) = m + 1/2 with m = x >> 11 (the one rounding of u53 is that of this sum: m has 53 bits).  m's two words
// convert exactly and fma(m_hi, 2^32, m_lo) is exact, where the conversion of a 64-bit integer is two conversions and an ldexp.
__device__ __forceinline__ double u53_unscaled(uint32_t hi, uint32_t lo) {
    const uint32_t mh = hi >> 11, ml = (hi << 21) | (lo >> 11);
    return fma((double)mh, 0x1p+32, (double)ml) + 0.5;
}

// log_pos(u53(hi, lo)), bit for bit: the scaling by 2^-53 goes into the logarithm's integer exponent (log_pos_scaled: v >= 1/2
// is normal and its mantissa is u1's).  u1 == 1 is v == 2^53 and gives +0 as log_pos(1.0) does.
__device__ __forceinline__ double log_u53(uint32_t hi, uint32_t lo) {
#ifdef DX_U1_LDEXP
    return log_pos(u53(hi, lo));
#else
    return log_pos_scaled(u53_unscaled(hi, lo), -53);
#endif
}

// rand_normal(mean, stdev, u53(hi, lo), u32(w2)), bit for bit, from the words.  The radius is a select, not a branch: fast_sqrt
// of the argument -0 (u1 == 1) is a NaN that the select drops, and the proposal loop keeps its execution mask
// (-DDX_DRAW_BRANCH: the branch).
__device__ __forceinline__ double rand_normal_w(double mean, double stdev, uint32_t hi, uint32_t lo, uint32_t w2) {
    const double arg = -2.0 * log_u53(hi, lo);
#ifdef DX_DRAW_BRANCH
    const double r = (arg > 0.0) ? fast_sqrt(arg) : 0.0;
#else
    const double sq = fast_sqrt(arg);
    const double r = (arg > 0.0) ? sq : 0.0;
#endif
    return fma(stdev * r, sin_2pi_w(w2), mean);
}

// The textbook fluctuation term of unit (global pixel, plane k) at band j (0-based, the model's band number): eta_j / sigma_j
// with eta_j the band's own standard normal (draw slot k + 4 * (j + 1)) and is = 1 / sigma_j.  Member g's right-hand side takes
// fluct_band(...) * m_gj after band j's data term.  ONE function for every kernel that carries the term, so that they agree bit
// for bit on the draw (rand_normal ends in an fma of its own; the product with `is` cannot be contracted into it).
__device__ __forceinline__ double fluct_band(unsigned long long seed, unsigned long long stream, unsigned long long pix, int k,
                                             int j, double is) {
    double u1, u2;
    uniform2(seed, stream, pix, (uint32_t)(k + 4 * (j + 1)), u1, u2);
    return rand_normal(0.0, 1.0, u1, u2) * is;
}

}  // namespace dx
