// dx_math.h -- fp64 math helpers sized for the sampler kernels (gfx950).
//
// The Gibbs path is bound by fp64 transcendentals, and the device library's general-purpose
// log/sin/pow carry argument-range and special-case handling the path never needs
// (measured in ISA instructions on gfx950: exp 19 f64 ops, log 76, sin 108, pow 148).
// The helpers below are valid on the ranges the kernels use and keep <= 1-3 ulp accuracy; each states its domain, and
// tests/test_gpu_mathlib.py and tests/test_gpu_mathlib_helpers.py run every one of them on the device over that domain and at
// its ends ("Device math helpers", has the measured maxima).
#pragma once
#include "dx_rtc_compat.h"

namespace dx {

// r*p + c with the coefficient in a VECTOR register and the three-address encoding.  For a polynomial that is evaluated
// once per loop iteration the compiler keeps the coefficients in vector registers anyway (the scalar registers are taken
// by the band constants) and then emits  v_mov_b64 tmp, c ; v_fmac_f64 tmp, r, p  -- two instructions per Horner step
// (27 such copies in a Metropolis proposal); v_fma_f64 dst, r, p, c reads the same register without the copy.
// Only translation units that define DX_VCOEF (the register-chain kernels) get it: elsewhere (amplitude kernels, one
// normal deviate per tile) the longer live ranges cost spills and there is no loop to win in.
__device__ __forceinline__ double fma_vc(double r, double p, double c) {
#ifndef DX_VCOEF
    return fma(r, p, c);
#else
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(r), "v"(p), "v"(c));
    return d;
#endif
}

// 1/x for finite normal x, <= 1 ulp (measured 0.5; v_rcp_f64 is good to 2^-23; each Newton step squares the error).  Denormal
// results (|x| >= 2^1022) come out within one denormal spacing.  NOT for x = +-0, +-inf or denormal x: v_rcp_f64 gives the IEEE
// +-inf / +-0 there and the Newton steps make NaN of it (fma(-inf, 0, 1)) -- see fast_rcp_ends.
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}
// 1/x for EVERY x, with the IEEE values at the ends fast_rcp leaves out: +-inf -> +-0, and +-0 and the denormals whose
// reciprocal overflows -> +-inf, are v_rcp_f64's own results, which the Newton steps turn into NaN (fma(-inf, 0, 1)): where the
// seed is 0 or inf it is the result.  (Denormals within 2^-23 of 2^-1024 may give inf where 1/x is just below the largest
// double: the seed's own error.)  Every other argument: fast_rcp's operations, the same bits.  One v_cmp_class_f64 and two
// selects more: for call sites outside the proposal loops, and for the chains whose Planck denominator exp(h nu / k T) - 1
// can overflow (dx_chain.h)
__device__ __forceinline__ double fast_rcp_ends(double x) {
    const double r0 = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r0, 1.0);
    double r = fma(r0, e, r0);
    e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    return __builtin_amdgcn_class(r0, 0x264) ? r0 : r;   // the seed is -inf, -0, +0 or +inf
}
// 1/sqrt(x) for finite normal x > 0: Goldschmidt iteration on g ~ sqrt(x), h ~ 1/(2 sqrt(x)).  The second step's result carries
// the roundings of g0 = x y and of g1, h1 (half each: (eta0 + eta1 - eta2) / 2) and its own: relative error <= 2.5 * 2^-53, i.e.
// 1.25 to 2.5 ulp depending on where the result lies in its binade (measured 1.63 ulp; DESIGN.md has the recurrence).  NaN at
// x = 0 and x = +inf (the seed is inf / 0), garbage for x < 0 and denormal x: the call sites keep away (a sum of squares of
// finite nonzero 1/rms-scaled SEDs; rand_normal selects around its -0).
__device__ __forceinline__ double fast_rsqrt(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double r = fma(-g, h, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    r = fma(-g, h, 0.5);
    h = fma(h, r, h);
    return h + h;
}

// sqrt(x) for finite normal x > 0 by the same Goldschmidt iteration (relative error <= 2.5 * 2^-53 as above, measured 1.43 ulp;
// 8 vector instructions, the IEEE sqrt sequence is 15)
__device__ __forceinline__ double fast_sqrt(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double r = fma(-g, h, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    r = fma(-g, h, 0.5);
    return fma(g, r, g);
}


// Natural logarithm for x > 0, finite and NORMAL (uniform deviates in (0,1), frequencies, temperatures).
// Default: fdlibm's e_log.c scheme: x = 2^k * (1+f), sqrt(1/2) <= 1+f < sqrt(2), s = f/(2+f),
// log(1+f) = f - (f^2/2 - s*(f^2/2 + R(s^2))), |error| < 1 ulp.
// -DDX_LOG_TABLE: a table and no division.  x = 2^k z with z in [0.6875, 1.375) (the exponent and the top seven mantissa bits
// of x - 0.6875 as integers pick k and the subinterval j), log x = k ln2 + log c_j + log1p(r), r = fma(z, 1/c_j, -1),
// |r| <= 2^-7.  Row j holds 1/c_j (c_j is defined as its inverse) and log c_j as hi + lo, hi on the grid 2^-42 of ln2_hi so
// that w = k ln2_hi + log c_hi is exact.  1/c_j is a multiple of 2^-8 chosen so that |r| < 2^-8 (z < 1) or 2^-7 (z >= 1)
// over the subinterval: r is then exact (all but six subintervals, the nearest of them at z = 0.94, where |log x| >= 0.06
// dwarfs the rounding of r); the two subintervals at z = 1 have c = 1, so there is no cancellation between log c and
// log1p(r) near x = 1.  hi + lo = w + r exactly (Fast2Sum), and log1p(r) - r = r^2 q(r) with the Taylor terms to r^8
// (truncation < 2^-56 |r|).  <= 0.53 ulp (tests/test_gpu_mathlib.py), 32 issue cycles fewer per Box-Muller draw in the
// proposal loop -- but OFF: the gather sits on the proposal's serial path (Philox -> log -> sqrt -> proposal -> SEDs), and
// at two waves per SIMD its L1 latency costs more than the v_rcp_f64 it replaces: C3 -2.6 %.
struct alignas(32) LogRow { double invc, logc_hi, logc_lo, pad; };
static __device__ const LogRow log_tab[128] = {
    {0x1.7300000000000p+0, -0x1.7bede0a37b000p-2, 0x1.018783cb9801ap-48, 0.0}, {0x1.7100000000000p+0, -0x1.7664e1239e000p-2, 0x1.0c4fb6aeb27afp-44, 0.0},
    {0x1.6f00000000000p+0, -0x1.70d42e2789000p-2, -0x1.1aead337ee287p-45, 0.0}, {0x1.6d00000000000p+0, -0x1.6b3bb22359000p-2, -0x1.0f6257a933268p-44, 0.0},
    {0x1.6b00000000000p+0, -0x1.659b57303e000p-2, -0x1.f281db0af8efcp-46, 0.0}, {0x1.6900000000000p+0, -0x1.5ff3070a79000p-2, -0x1.e9e439f105039p-45, 0.0},
    {0x1.6700000000000p+0, -0x1.5a42ab0f4d000p-2, 0x1.e63af2df7ba69p-50, 0.0}, {0x1.6500000000000p+0, -0x1.548a2c3add000p-2, -0x1.3167e63081cf7p-45, 0.0},
    {0x1.6300000000000p+0, -0x1.4ec9732600000p-2, -0x1.34d7aaf04d104p-45, 0.0}, {0x1.6100000000000p+0, -0x1.4900680401000p-2, 0x1.8bccffe1a0f8cp-44, 0.0},
    {0x1.5f00000000000p+0, -0x1.432ef2a04f000p-2, 0x1.fb129931715adp-44, 0.0}, {0x1.5d867c3ece2a5p+0, -0x1.3edf463c17000p-2, 0x1.f08e4297f2c3fp-44, 0.0},
    {0x1.5c00000000000p+0, -0x1.3a64c55694000p-2, -0x1.7a71cbcd735d0p-44, 0.0}, {0x1.5a00000000000p+0, -0x1.347dd9a988000p-2, 0x1.5594dd4c58092p-45, 0.0},
    {0x1.5800000000000p+0, -0x1.2e8e2bae12000p-2, 0x1.67b1e99b72bd8p-45, 0.0}, {0x1.5600000000000p+0, -0x1.2895a13de8000p-2, -0x1.a8d7ad24c13f0p-44, 0.0},
    {0x1.54725e6bb82fep+0, -0x1.23ec5991ec000p-2, 0x1.6dbf448a2e522p-44, 0.0}, {0x1.5300000000000p+0, -0x1.1f8ff9e48a000p-2, -0x1.7946c040cbe77p-45, 0.0},
    {0x1.5100000000000p+0, -0x1.1980d2dd42000p-2, -0x1.b7b3a7a361c9ap-45, 0.0}, {0x1.4f00000000000p+0, -0x1.136870293b000p-2, 0x1.d3e8499d67123p-44, 0.0},
    {0x1.4d843bedc2c4cp+0, -0x1.0edd060b78000p-2, -0x1.044b52d8435f5p-47, 0.0}, {0x1.4c00000000000p+0, -0x1.0a324e2739000p-2, -0x1.c6bee7ef4030ep-47, 0.0},
    {0x1.4a00000000000p+0, -0x1.0402594b4d000p-2, -0x1.036b89ef42d7fp-48, 0.0}, {0x1.4880522014880p+0, -0x1.feb2233ea0000p-3, -0x1.f2c18de00938bp-45, 0.0},
    {0x1.4700000000000p+0, -0x1.f550a564b8000p-3, 0x1.323e3a09202fep-45, 0.0}, {0x1.4500000000000p+0, -0x1.e8c0252aa6000p-3, 0x1.6805b80e8e6ffp-45, 0.0},
    {0x1.4400000000000p+0, -0x1.e27076e2b0000p-3, 0x1.a342c2af0003cp-44, 0.0}, {0x1.4200000000000p+0, -0x1.d5c216b4fc000p-3, 0x1.1ba91bbca681bp-45, 0.0},
    {0x1.40782d10e6566p+0, -0x1.cc000c9db4000p-3, 0x1.d6e985d57aff9p-46, 0.0}, {0x1.3f00000000000p+0, -0x1.c2968558c2000p-3, 0x1.cfd73dee38a40p-45, 0.0},
    {0x1.3d00000000000p+0, -0x1.b5b519e8fc000p-3, 0x1.4b722ec011f31p-44, 0.0}, {0x1.3c00000000000p+0, -0x1.af3c94e80c000p-3, 0x1.a4e633fcd9066p-52, 0.0},
    {0x1.3a00000000000p+0, -0x1.a23bc1fe2c000p-3, 0x1.539cd91dc9f0bp-44, 0.0}, {0x1.3900000000000p+0, -0x1.9bb362e7e0000p-3, 0x1.1f2a8a1ce0ffcp-45, 0.0},
    {0x1.3700000000000p+0, -0x1.8e928de886000p-3, -0x1.a8154b13d72d5p-44, 0.0}, {0x1.3600000000000p+0, -0x1.87fa06520c000p-3, -0x1.22120401202fcp-44, 0.0},
    {0x1.3400000000000p+0, -0x1.7ab890210e000p-3, 0x1.bdb9072534a58p-45, 0.0}, {0x1.3300000000000p+0, -0x1.740f8f5404000p-3, 0x1.0b66c99018aa1p-44, 0.0},
    {0x1.3200000000000p+0, -0x1.6d60fe719e000p-3, 0x1.bc6e557134767p-44, 0.0}, {0x1.3000000000000p+0, -0x1.5ff3070a7a000p-3, 0x1.8586f183bebf2p-44, 0.0},
    {0x1.2f00000000000p+0, -0x1.59338d9982000p-3, -0x1.0ba68b7555d4ap-48, 0.0}, {0x1.2d00000000000p+0, -0x1.4ba36f39a6000p-3, 0x1.4354bb3f219e5p-44, 0.0},
    {0x1.2c00000000000p+0, -0x1.44d2b6ccb8000p-3, 0x1.70cc16135783cp-46, 0.0}, {0x1.2b00000000000p+0, -0x1.3dfc2b0ecc000p-3, -0x1.8a72a62b8c13fp-45, 0.0},
    {0x1.2900000000000p+0, -0x1.303d718e48000p-3, 0x1.680b5ce3ecb05p-50, 0.0}, {0x1.2800000000000p+0, -0x1.29552f8200000p-3, 0x1.5b967f4471dfcp-44, 0.0},
    {0x1.2700000000000p+0, -0x1.2266f190a6000p-3, 0x1.4d20ab840e7f6p-45, 0.0}, {0x1.2500000000000p+0, -0x1.1478584674000p-3, -0x1.563451027c750p-46, 0.0},
    {0x1.2400000000000p+0, -0x1.0d77e7cd08000p-3, -0x1.cb2cd2ee2f482p-44, 0.0}, {0x1.2300000000000p+0, -0x1.0671512ca6000p-3, 0x1.a47579cdc0a3dp-45, 0.0},
    {0x1.2100000000000p+0, -0x1.f0a30c0118000p-4, 0x1.d599e83368e91p-44, 0.0}, {0x1.2000000000000p+0, -0x1.e27076e2b0000p-4, 0x1.a342c2af0003cp-45, 0.0},
    {0x1.1f00000000000p+0, -0x1.d4313d66cc000p-4, 0x1.9454379135713p-45, 0.0}, {0x1.1e00000000000p+0, -0x1.c5e548f5bc000p-4, -0x1.d0c57585fbe06p-46, 0.0},
    {0x1.1c00000000000p+0, -0x1.a926d3a4ac000p-4, -0x1.563650bd22a9cp-44, 0.0}, {0x1.1b00000000000p+0, -0x1.9ab4246204000p-4, 0x1.8a64826787061p-45, 0.0},
    {0x1.1a00000000000p+0, -0x1.8c345d6318000p-4, -0x1.b20f5acb42a66p-44, 0.0}, {0x1.1900000000000p+0, -0x1.7da766d7b0000p-4, -0x1.2cc844480c89bp-44, 0.0},
    {0x1.1700000000000p+0, -0x1.60658a9374000p-4, -0x1.0c3b1dee9c4f8p-44, 0.0}, {0x1.1600000000000p+0, -0x1.51b073f060000p-4, -0x1.83f69278e686ap-44, 0.0},
    {0x1.1500000000000p+0, -0x1.42edcbea64000p-4, -0x1.bc0eeea7c9acdp-46, 0.0}, {0x1.1400000000000p+0, -0x1.341d7961bc000p-4, -0x1.1d09299837610p-44, 0.0},
    {0x1.1300000000000p+0, -0x1.253f62f0a0000p-4, -0x1.416f8fb69a701p-44, 0.0}, {0x1.1200000000000p+0, -0x1.16536eea38000p-4, 0x1.47c5e768fa309p-46, 0.0},
    {0x1.107fbbe011080p+0, -0x1.ffa6911ab8000p-5, -0x1.3088c98381a8fp-45, 0.0}, {0x1.0f00000000000p+0, -0x1.d276b8adb0000p-5, -0x1.6a423c78a64b0p-46, 0.0},
    {0x1.0e00000000000p+0, -0x1.b42dd71198000p-5, 0x1.c827ae5d6704cp-46, 0.0}, {0x1.0d00000000000p+0, -0x1.95c830ec90000p-5, 0x1.c148297c5feb8p-45, 0.0},
    {0x1.0c00000000000p+0, -0x1.77458f6330000p-5, 0x1.181dce586af09p-44, 0.0}, {0x1.0b00000000000p+0, -0x1.58a5bafc90000p-5, 0x1.b2b739570ad39p-45, 0.0},
    {0x1.0a00000000000p+0, -0x1.39e87b9fe8000p-5, -0x1.eafd480ad9015p-44, 0.0}, {0x1.0900000000000p+0, -0x1.1b0d989240000p-5, 0x1.3401e9ae889bbp-44, 0.0},
    {0x1.0800000000000p+0, -0x1.f829b0e780000p-6, -0x1.980267c7e09e4p-45, 0.0}, {0x1.0700000000000p+0, -0x1.b9fc027b00000p-6, 0x1.b9a010ae6922ap-44, 0.0},
    {0x1.0600000000000p+0, -0x1.7b91b07d60000p-6, 0x1.3b955b602ace4p-44, 0.0}, {0x1.0500000000000p+0, -0x1.3cea443470000p-6, 0x1.6a2c432d6a40bp-44, 0.0},
    {0x1.0400000000000p+0, -0x1.fc0a8b0fc0000p-7, -0x1.f1e7cf6d3a69cp-50, 0.0}, {0x1.0300000000000p+0, -0x1.7dc475f820000p-7, 0x1.eb1245b5da1f5p-44, 0.0},
    {0x1.0200000000000p+0, -0x1.fe02a6b100000p-8, -0x1.9e23f0dda40e4p-46, 0.0}, {0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0, 0.0},
    {0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0, 0.0}, {0x1.fa00000000000p-1, 0x1.82448a3880000p-7, 0x1.4554412c584e0p-44, 0.0},
    {0x1.f600000000000p-1, 0x1.432a925980000p-6, 0x1.98139928637fep-47, 0.0}, {0x1.f200000000000p-1, 0x1.c63d2ec150000p-6, -0x1.5439ce030a687p-44, 0.0},
    {0x1.ee00000000000p-1, 0x1.252f32f8d0000p-5, 0x1.83e9ae021b67bp-45, 0.0}, {0x1.ea00000000000p-1, 0x1.67c94f2d48000p-5, 0x1.dac20827cca0cp-44, 0.0},
    {0x1.e800000000000p-1, 0x1.894aa149f8000p-5, 0x1.9a19a8be97661p-44, 0.0}, {0x1.e400000000000p-1, 0x1.ccb73cddd8000p-5, 0x1.965c36e09f5fep-44, 0.0},
    {0x1.e000000000000p-1, 0x1.08598b59e4000p-4, -0x1.7e5dd7009902cp-46, 0.0}, {0x1.dc00000000000p-1, 0x1.2aa04a4470000p-4, 0x1.7a48ba8b1cb41p-44, 0.0},
    {0x1.da00000000000p-1, 0x1.3bdf5a7d20000p-4, -0x1.19bd0ad125895p-44, 0.0}, {0x1.d600000000000p-1, 0x1.5e95a4d978000p-4, 0x1.1cb7ce1d17171p-44, 0.0},
    {0x1.d200000000000p-1, 0x1.8197e2f410000p-4, -0x1.c0fe460d20041p-44, 0.0}, {0x1.d000000000000p-1, 0x1.9335e5d594000p-4, 0x1.3115c3abd47dap-45, 0.0},
    {0x1.cc00000000000p-1, 0x1.b6ac88dad4000p-4, 0x1.b1bdff50225c7p-44, 0.0}, {0x1.c800000000000p-1, 0x1.da72763844000p-4, 0x1.a89401fa71733p-46, 0.0},
    {0x1.c600000000000p-1, 0x1.ec739830a0000p-4, 0x1.11fcba80cdd10p-44, 0.0}, {0x1.c200000000000p-1, 0x1.08598b59e4000p-3, -0x1.7e5dd7009902cp-45, 0.0},
    {0x1.c000000000000p-1, 0x1.1178e8227e000p-3, 0x1.1ef78ce2d07f2p-45, 0.0}, {0x1.bc00000000000p-1, 0x1.23d712a49c000p-3, 0x1.00d238fd3df5cp-46, 0.0},
    {0x1.ba00000000000p-1, 0x1.2d1610c868000p-3, 0x1.39d6ccb81b4a1p-47, 0.0}, {0x1.b600000000000p-1, 0x1.3fb45a5992000p-3, 0x1.19713c0cae559p-44, 0.0},
    {0x1.b400000000000p-1, 0x1.4913d8333c000p-3, -0x1.53e43558124c4p-44, 0.0}, {0x1.b000000000000p-1, 0x1.5bf406b544000p-3, -0x1.27023eb68981cp-46, 0.0},
    {0x1.ae00000000000p-1, 0x1.6574ebe8c2000p-3, -0x1.98c1d34f0f462p-44, 0.0}, {0x1.aa00000000000p-1, 0x1.7898d85444000p-3, 0x1.8e67be3dbaf3fp-44, 0.0},
    {0x1.a800000000000p-1, 0x1.823c16551a000p-3, 0x1.e0ddb9a631e83p-46, 0.0}, {0x1.a600000000000p-1, 0x1.8beafeb390000p-3, -0x1.73d54aae92cd1p-47, 0.0},
    {0x1.a200000000000p-1, 0x1.9f6c40708a000p-3, -0x1.337d94bcd3f43p-44, 0.0}, {0x1.a000000000000p-1, 0x1.a93ed3c8ae000p-3, -0x1.8724350562169p-45, 0.0},
    {0x1.9e00000000000p-1, 0x1.b31d8575bc000p-3, 0x1.c794e562a63cbp-44, 0.0}, {0x1.9a00000000000p-1, 0x1.c6ffbc6f00000p-3, 0x1.ee138d3a69d43p-44, 0.0},
    {0x1.9800000000000p-1, 0x1.d1037f2656000p-3, -0x1.84a7e75b6f6e4p-47, 0.0}, {0x1.9600000000000p-1, 0x1.db13db0d48000p-3, 0x1.2806a847527e6p-44, 0.0},
    {0x1.9400000000000p-1, 0x1.e530effe72000p-3, -0x1.fdbdbb13f7c18p-44, 0.0}, {0x1.9000000000000p-1, 0x1.f991c6cb3c000p-3, -0x1.90d04cd7cc834p-44, 0.0},
    {0x1.8e00000000000p-1, 0x1.01eae5626c000p-2, 0x1.a43dcfade85aep-44, 0.0}, {0x1.8c00000000000p-1, 0x1.07138604d6000p-2, -0x1.e76324e912b17p-44, 0.0},
    {0x1.8a00000000000p-1, 0x1.0c42d67616000p-2, 0x1.7188b163ceae9p-45, 0.0}, {0x1.8800000000000p-1, 0x1.1178e8227e000p-2, 0x1.1ef78ce2d07f2p-44, 0.0},
    {0x1.8400000000000p-1, 0x1.1bf99635a7000p-2, -0x1.1ac89575c2125p-44, 0.0}, {0x1.8200000000000p-1, 0x1.214456d0ec000p-2, -0x1.caf0428b728a3p-44, 0.0},
    {0x1.8000000000000p-1, 0x1.269621134e000p-2, -0x1.1b61f10522625p-44, 0.0}, {0x1.7e00000000000p-1, 0x1.2bef07cdc9000p-2, 0x1.a9cfa4a5004f4p-45, 0.0},
    {0x1.7c00000000000p-1, 0x1.314f1e1d36000p-2, -0x1.8e27ad3213cb8p-45, 0.0}, {0x1.7a00000000000p-1, 0x1.36b6776be1000p-2, 0x1.16ecdb0f177c8p-46, 0.0},
    {0x1.7800000000000p-1, 0x1.3c25277333000p-2, 0x1.83b54b606bd5cp-46, 0.0}, {0x1.7600000000000p-1, 0x1.419b423d5f000p-2, -0x1.ce379226de3ecp-44, 0.0},
};

__device__ __forceinline__ double log_pos_scaled(double v, int e);
__device__ __forceinline__ double log_pos(double x) {
#ifdef DX_LOG_TABLE
    const unsigned long long ix = (unsigned long long)__double_as_longlong(x);
    const unsigned long long tmp = ix - 0x3fe6000000000000ull;
    const int k = (int)((long long)tmp >> 52);
    const LogRow t = log_tab[(unsigned int)(tmp >> 45) & 127u];
    const double z = __longlong_as_double((long long)(ix - (tmp & 0xfff0000000000000ull)));
    const double r = fma(z, t.invc, -1.0);
    const double kd = (double)k;
    const double w = fma(kd, 0x1.62e42fefa3800p-1, t.logc_hi);
    const double hi = w + r;
    const double lo = (w - hi) + r;
    const double tl = fma(kd, 0x1.ef35793c76730p-45, t.logc_lo) + lo;
    double q = fma_vc(r, -0.125, 0x1.2492492492492p-3);
    q = fma_vc(r, q, -0x1.5555555555555p-3);
    q = fma_vc(r, q, 0.2);
    q = fma_vc(r, q, -0.25);
    q = fma_vc(r, q, 0x1.5555555555555p-2);
    q = fma_vc(r, q, -0.5);
    return hi + fma(r * r, q, tl);
#else
    return log_pos_scaled(x, 0);   // (the constant folds away: the operations of the form below)
#endif
}

// log(v 2^e) for v > 0, finite and NORMAL, and an integer e with |e| < 2^20 (the product itself need not be formed, nor be
// normal): log_pos's default form (log_pos is this with e = 0) with e added to the integer exponent it reads from v's bits.
// The mantissa of v 2^e is v's, so every operation after that sees the operands log_pos(ldexp(v, e)) sees: the same bits
// wherever v 2^e is normal.  The Metropolis draw passes its 53-bit uniform as the integer-valued v = m + 1/2 >= 1/2 with
// e = -53 and saves the scaling (dx_rng.h: log_u53; tests/test_gpu_draw_forms.py compares it with log_pos(u53) on the device).
__device__ __forceinline__ double log_pos_scaled(double v, int e) {
#ifdef DX_LOG_TABLE
    return log_pos(ldexp(v, e));
#else
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    constexpr double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                     Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                     Lg7 = 1.479819860511658591e-01;
    unsigned long long ix = (unsigned long long)__double_as_longlong(v);
    int k = (int)(ix >> 52) - 1023 + e;
    ix = (ix & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;  // m in [1,2)
    double m = __longlong_as_double((long long)ix);
    if (m > 1.4142135623730951) { m *= 0.5; k += 1; }
    const double f = m - 1.0;
    const double s = f * fast_rcp(2.0 + f);
    const double dk = (double)k;
    const double z = s * s;
    const double w = z * z;
    // every sum of two products below is written as ONE explicit fma: left to the compiler, "a*b + c*d" may be contracted
    // either way, and two kernels that inline this function then differ in the last bit for a few arguments in a million
    // (found by comparing the fused and the separate launches over 12.6 M pixels)
    const double t1 = w * fma_vc(w, fma_vc(w, Lg6, Lg4), Lg2);
    const double R = fma(z, fma_vc(w, fma_vc(w, fma_vc(w, Lg7, Lg5), Lg3), Lg1), t1);
    const double hfsq = (0.5 * f) * f;
    const double inner = fma(s, hfsq + R, dk * ln2_lo);
    return fma(dk, ln2_hi, -((hfsq - inner) - f));
#endif
}

// exp(x) with the device library's own reduction and polynomial (ocml expD: n = rint(x log2e), r = x - n ln2 in two
// pieces, degree-11 Horner, ldexp) WITHOUT its two range selects (x > 1024 -> inf, x < -1075 -> 0): ldexp saturates to
// inf / 0 by itself, so every finite argument gives the library's result bit for bit; only x = +-inf differ (NaN instead
// of inf / 0), and the kernels never compare such a value with an outcome that depends on it (an accept test
// `exp(diff) > u` is false either way; `diff >= 0` is tested first).  Six of the library routine's 22 vector
// instructions are those selects: the Metropolis chains are vector-issue bound, so this is 1/8 of their proposal loop.
// exp_sat: for |x| <= 1e16 (tested out there: +inf, the denormals, +0).  Beyond 2^53 / log2e the product x log2e no longer
// resolves the integer part, the reduced argument is garbage and so is the polynomial's sign: on the device
// exp_sat(1e300) = -inf, exp_sat(-1e100) = -inf, exp_sat(-1e300) = +inf, exp_sat(-1e20) = -0 and exp_sat(+-inf) = NaN.  A call
// site whose argument has no bound (log-normal SED with a narrow width, Planck function at low temperature, an accept test
// on a difference of overflowing likelihoods) takes exp_any.
__device__ __forceinline__ double exp_sat(double x) {
    const double dn = rint(x * 0x1.71547652b82fep+0);
    const double r = fma(dn, -0x1.abc9e3b39803fp-56, fma(dn, -0x1.62e42fefa39efp-1, x));
    double p = fma(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
    p = fma(r, p, 0x1.71dee623fde64p-19);
    p = fma(r, p, 0x1.a01997c89e6b0p-16);
    p = fma(r, p, 0x1.a01a014761f6ep-13);
    p = fma(r, p, 0x1.6c16c1852b7b0p-10);
    p = fma(r, p, 0x1.1111111122322p-7);
    p = fma(r, p, 0x1.55555555502a1p-5);
    p = fma(r, p, 0x1.5555555555511p-3);
    p = fma(r, p, 0x1.000000000000bp-1);
    p = fma(r, p, 1.0);
    p = fma(r, p, 1.0);
    return ldexp(p, (int)dn);
}

// exp(x) for EVERY x: the argument is held at +-2^20, where ldexp has long saturated, by two compares and selects that let a
// NaN through -- exp_sat's own bits wherever exp_sat is right, +inf / +0 beyond and at +-inf (IEEE arithmetic on the function),
// NaN for NaN.  Six vector instructions more than exp_sat: for call sites outside the proposal loops, and the log-normal chains
// whose width can be that narrow (dx_chain.h)
__device__ __forceinline__ double exp_any(double x) {
    x = (x > 0x1p+20) ? 0x1p+20 : x;
    x = (x < -0x1p+20) ? -0x1p+20 : x;
    return exp_sat(x);
}

// 2^(j/128), j = 0..127, as hi + lo (lo = the rounding error of hi, |lo| < 2^-53 hi): the table of exp_nr's table form.  One
// copy per code object, read through the vector L1 by a 16-byte gather.
struct alignas(16) Exp2Pair { double hi, lo; };
static __device__ const Exp2Pair exp2_tab[128] = {
    {0x1.0000000000000p+0, 0x0.0p+0}, {0x1.0163da9fb3335p+0, 0x1.b61299ab8cdb7p-54},
    {0x1.02c9a3e778061p+0, -0x1.19083535b085dp-56}, {0x1.04315e86e7f85p+0, -0x1.0a31c1977c96ep-54},
    {0x1.059b0d3158574p+0, 0x1.d73e2a475b465p-55}, {0x1.0706b29ddf6dep+0, -0x1.c91dfe2b13c27p-55},
    {0x1.0874518759bc8p+0, 0x1.186be4bb284ffp-57}, {0x1.09e3ecac6f383p+0, 0x1.1487818316136p-54},
    {0x1.0b5586cf9890fp+0, 0x1.8a62e4adc610bp-54}, {0x1.0cc922b7247f7p+0, 0x1.01edc16e24f71p-54},
    {0x1.0e3ec32d3d1a2p+0, 0x1.03a1727c57b53p-59}, {0x1.0fb66affed31bp+0, -0x1.b9bedc44ebd7bp-57},
    {0x1.11301d0125b51p+0, -0x1.6c51039449b3ap-54}, {0x1.12abdc06c31ccp+0, -0x1.1b514b36ca5c7p-58},
    {0x1.1429aaea92de0p+0, -0x1.32fbf9af1369ep-54}, {0x1.15a98c8a58e51p+0, 0x1.2406ab9eeab0ap-55},
    {0x1.172b83c7d517bp+0, -0x1.19041b9d78a76p-55}, {0x1.18af9388c8deap+0, -0x1.11023d1970f6cp-54},
    {0x1.1a35beb6fcb75p+0, 0x1.e5b4c7b4968e4p-55}, {0x1.1bbe084045cd4p+0, -0x1.95386352ef607p-54},
    {0x1.1d4873168b9aap+0, 0x1.e016e00a2643cp-54}, {0x1.1ed5022fcd91dp+0, -0x1.1df98027bb78cp-54},
    {0x1.2063b88628cd6p+0, 0x1.dc775814a8495p-55}, {0x1.21f49917ddc96p+0, 0x1.2a97e9494a5eep-55},
    {0x1.2387a6e756238p+0, 0x1.9b07eb6c70573p-54}, {0x1.251ce4fb2a63fp+0, 0x1.ac155bef4f4a4p-55},
    {0x1.26b4565e27cddp+0, 0x1.2bd339940e9d9p-55}, {0x1.284dfe1f56381p+0, -0x1.a4c3a8c3f0d7ep-54},
    {0x1.29e9df51fdee1p+0, 0x1.612e8afad1255p-55}, {0x1.2b87fd0dad990p+0, -0x1.10adcd6381aa4p-59},
    {0x1.2d285a6e4030bp+0, 0x1.0024754db41d5p-54}, {0x1.2ecafa93e2f56p+0, 0x1.1ca0f45d52383p-56},
    {0x1.306fe0a31b715p+0, 0x1.6f46ad23182e4p-55}, {0x1.32170fc4cd831p+0, 0x1.a9ce78e18047cp-55},
    {0x1.33c08b26416ffp+0, 0x1.32721843659a6p-54}, {0x1.356c55f929ff1p+0, -0x1.b5cee5c4e4628p-55},
    {0x1.371a7373aa9cbp+0, -0x1.63aeabf42eae2p-54}, {0x1.38cae6d05d866p+0, -0x1.e958d3c9904bdp-54},
    {0x1.3a7db34e59ff7p+0, -0x1.5e436d661f5e3p-56}, {0x1.3c32dc313a8e5p+0, -0x1.efff8375d29c3p-54},
    {0x1.3dea64c123422p+0, 0x1.ada0911f09ebcp-55}, {0x1.3fa4504ac801cp+0, -0x1.7d023f956f9f3p-54},
    {0x1.4160a21f72e2ap+0, -0x1.ef3691c309278p-58}, {0x1.431f5d950a897p+0, -0x1.1c7dde35f7999p-55},
    {0x1.44e086061892dp+0, 0x1.89b7a04ef80d0p-59}, {0x1.46a41ed1d0057p+0, 0x1.c944bd1648a76p-54},
    {0x1.486a2b5c13cd0p+0, 0x1.3c1a3b69062f0p-56}, {0x1.4a32af0d7d3dep+0, 0x1.9cb62f3d1be56p-54},
    {0x1.4bfdad5362a27p+0, 0x1.d4397afec42e2p-56}, {0x1.4dcb299fddd0dp+0, 0x1.8ecdbbc6a7833p-54},
    {0x1.4f9b2769d2ca7p+0, -0x1.4b309d25957e3p-54}, {0x1.516daa2cf6642p+0, -0x1.f768569bd93efp-55},
    {0x1.5342b569d4f82p+0, -0x1.07abe1db13cadp-55}, {0x1.551a4ca5d920fp+0, -0x1.d689cefede59bp-55},
    {0x1.56f4736b527dap+0, 0x1.9bb2c011d93adp-54}, {0x1.58d12d497c7fdp+0, 0x1.295e15b9a1de8p-55},
    {0x1.5ab07dd485429p+0, 0x1.6324c054647adp-54}, {0x1.5c9268a5946b7p+0, 0x1.c4b1b816986a2p-60},
    {0x1.5e76f15ad2148p+0, 0x1.ba6f93080e65ep-54}, {0x1.605e1b976dc09p+0, -0x1.3e2429b56de47p-54},
    {0x1.6247eb03a5585p+0, -0x1.383c17e40b497p-54}, {0x1.6434634ccc320p+0, -0x1.c483c759d8933p-55},
    {0x1.6623882552225p+0, -0x1.bb60987591c34p-54}, {0x1.68155d44ca973p+0, 0x1.038ae44f73e65p-57},
    {0x1.6a09e667f3bcdp+0, -0x1.bdd3413b26456p-54}, {0x1.6c012750bdabfp+0, -0x1.2895667ff0b0dp-56},
    {0x1.6dfb23c651a2fp+0, -0x1.bbe3a683c88abp-57}, {0x1.6ff7df9519484p+0, -0x1.83c0f25860ef6p-55},
    {0x1.71f75e8ec5f74p+0, -0x1.16e4786887a99p-55}, {0x1.73f9a48a58174p+0, -0x1.0a8d96c65d53cp-54},
    {0x1.75feb564267c9p+0, -0x1.0245957316dd3p-54}, {0x1.780694fde5d3fp+0, 0x1.866b80a02162dp-54},
    {0x1.7a11473eb0187p+0, -0x1.41577ee04992fp-55}, {0x1.7c1ed0130c132p+0, 0x1.f124cd1164dd6p-54},
    {0x1.7e2f336cf4e62p+0, 0x1.05d02ba15797ep-56}, {0x1.80427543e1a12p+0, -0x1.27c86626d972bp-54},
    {0x1.82589994cce13p+0, -0x1.d4c1dd41532d8p-54}, {0x1.8471a4623c7adp+0, -0x1.8d684a341cdfbp-55},
    {0x1.868d99b4492edp+0, -0x1.fc6f89bd4f6bap-54}, {0x1.88ac7d98a6699p+0, 0x1.994c2f37cb53ap-54},
    {0x1.8ace5422aa0dbp+0, 0x1.6e9f156864b27p-54}, {0x1.8cf3216b5448cp+0, -0x1.0d55e32e9e3aap-56},
    {0x1.8f1ae99157736p+0, 0x1.5cc13a2e3976cp-55}, {0x1.9145b0b91ffc6p+0, -0x1.dd6792e582524p-54},
    {0x1.93737b0cdc5e5p+0, -0x1.75fc781b57ebcp-57}, {0x1.95a44cbc8520fp+0, -0x1.64b7c96a5f039p-56},
    {0x1.97d829fde4e50p+0, -0x1.d185b7c1b85d1p-54}, {0x1.9a0f170ca07bap+0, -0x1.173bd91cee632p-54},
    {0x1.9c49182a3f090p+0, 0x1.c7c46b071f2bep-56}, {0x1.9e86319e32323p+0, 0x1.824ca78e64c6ep-56},
    {0x1.a0c667b5de565p+0, -0x1.359495d1cd533p-54}, {0x1.a309bec4a2d33p+0, 0x1.6305c7ddc36abp-54},
    {0x1.a5503b23e255dp+0, -0x1.d2f6edb8d41e1p-54}, {0x1.a799e1330b358p+0, 0x1.bcb7ecac563c7p-54},
    {0x1.a9e6b5579fdbfp+0, 0x1.0fac90ef7fd31p-54}, {0x1.ac36bbfd3f37ap+0, -0x1.f9234cae76cd0p-55},
    {0x1.ae89f995ad3adp+0, 0x1.7a1cd345dcc81p-54}, {0x1.b0e07298db666p+0, -0x1.bdef54c80e425p-54},
    {0x1.b33a2b84f15fbp+0, -0x1.2805e3084d708p-57}, {0x1.b59728de5593ap+0, -0x1.c71dfbbba6de3p-54},
    {0x1.b7f76f2fb5e47p+0, -0x1.5584f7e54ac3bp-56}, {0x1.ba5b030a1064ap+0, -0x1.efcd30e54292ep-54},
    {0x1.bcc1e904bc1d2p+0, 0x1.23dd07a2d9e84p-55}, {0x1.bf2c25bd71e09p+0, -0x1.efdca3f6b9c73p-54},
    {0x1.c199bdd85529cp+0, 0x1.11065895048ddp-55}, {0x1.c40ab5fffd07ap+0, 0x1.b4537e083c60ap-54},
    {0x1.c67f12e57d14bp+0, 0x1.2884dff483cadp-54}, {0x1.c8f6d9406e7b5p+0, 0x1.1acbc48805c44p-56},
    {0x1.cb720dcef9069p+0, 0x1.503cbd1e949dbp-56}, {0x1.cdf0b555dc3fap+0, -0x1.dd83b53829d72p-55},
    {0x1.d072d4a07897cp+0, -0x1.cbc3743797a9cp-54}, {0x1.d2f87080d89f2p+0, -0x1.d487b719d8578p-54},
    {0x1.d5818dcfba487p+0, 0x1.2ed02d75b3707p-55}, {0x1.d80e316c98398p+0, -0x1.11ec18beddfe8p-54},
    {0x1.da9e603db3285p+0, 0x1.c2300696db532p-54}, {0x1.dd321f301b460p+0, 0x1.2da5778f018c3p-54},
    {0x1.dfc97337b9b5fp+0, -0x1.1a5cd4f184b5cp-54}, {0x1.e264614f5a129p+0, -0x1.7b627817a1496p-54},
    {0x1.e502ee78b3ff6p+0, 0x1.39e8980a9cc8fp-55}, {0x1.e7a51fbc74c83p+0, 0x1.2d522ca0c8de2p-54},
    {0x1.ea4afa2a490dap+0, -0x1.e9c23179c2893p-54}, {0x1.ecf482d8e67f1p+0, -0x1.c93f3b411ad8cp-54},
    {0x1.efa1bee615a27p+0, 0x1.dc7f486a4b6b0p-54}, {0x1.f252b376bba97p+0, 0x1.3a1a5bf0d8e43p-54},
    {0x1.f50765b6e4540p+0, 0x1.9d3e12dd8a18bp-54}, {0x1.f7bfdad9cbe14p+0, -0x1.dbb12d006350ap-54},
    {0x1.fa7c1819e90d8p+0, 0x1.74853f3a5931ep-55}, {0x1.fd3c22b8f71f1p+0, 0x1.2eb74966579e7p-57},
};

// exp_nr: exp(x) for |x| < 1.4e9 -- the SED arguments beta ln(nu/nu_ref) and h nu / (k T) with the clamp of mbb_z.
// Default: the reduction and polynomial of exp_sat without its v_rndne / v_cvt: n = rint(x log2e) comes out of ONE fma with
// 1.5 * 2^52 (the integer then sits in the low word of the sum, two's complement).  (The single rounding of x log2e + 2^52
// can pick the neighbouring n when x log2e is within an ulp of a half-integer; r is then just beyond ln2/2 and the result
// differs in the last bit at most.)  -DDX_EXP_RINT restores exp_sat everywhere.
// -DDX_EXP_TABLE: Tang's table form, x = (128 m + j) ln2/128 + r, |r| <= ln2/256, exp(x) = 2^m 2^(j/128) (1 + p(r)).
// k = 128 m + j from the same fma with 128 log2e; j is its low 7 bits and m = k >> 7 the funnel shift of the sum's two words
// (valid for |k| < 2^38); r in two Cody-Waite pieces (the high one has 36 bits, so kd * hi is exact for every k that does
// not saturate); p(r) = r + r^2 (1/2 + r/6 + r^2/24 + r^3/120) (truncation < 6e-19); T_hi + (T_hi p + T_lo) scaled by ldexp,
// which saturates to inf / 0 by itself.  12 fp64 and three 32-bit instructions and one gather instead of 17 fp64, <= 0.51 ulp
// (tests/test_gpu_mathlib.py) -- but OFF: the plane-set kernels hoist the ten gathers of a proposal (four registers each)
// and at 239 of 256 registers spill 117-272 VGPRs into the proposal loops.
__device__ __forceinline__ double exp_nr(double x) {
#if defined(DX_EXP_RINT)
    return exp_sat(x);
#elif defined(DX_EXP_TABLE)
    const double z = fma(x, 0x1.71547652b82fep+7, 0x1.8p+52);
    const double kd = z - 0x1.8p+52;
    double r = fma(kd, -0x1.62e42fefa0000p-8, x);
    r = fma(kd, -0x1.cf79abc9e3b3ap-47, r);
    const unsigned long long zb = (unsigned long long)__double_as_longlong(z);
    const unsigned int zlo = (unsigned int)zb, zhi = (unsigned int)(zb >> 32);
    const Exp2Pair t = exp2_tab[zlo & 127u];
    const int m = (int)__builtin_amdgcn_alignbit(zhi, zlo, 7u);
    double q = fma(r, 0x1.1111111111111p-7, 0x1.5555555555555p-5);
    q = fma(r, q, 0x1.5555555555555p-3);
    q = fma(r, q, 0.5);
    const double p = fma(r * r, q, r);
    return ldexp(t.hi + fma(t.hi, p, t.lo), m);
#else
    const double z = fma(x, 0x1.71547652b82fep+0, 0x1.8p+52);
    const double dn = z - 0x1.8p+52;
    const double r = fma(dn, -0x1.abc9e3b39803fp-56, fma(dn, -0x1.62e42fefa39efp-1, x));
    double p = fma(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
    p = fma(r, p, 0x1.71dee623fde64p-19);
    p = fma(r, p, 0x1.a01997c89e6b0p-16);
    p = fma(r, p, 0x1.a01a014761f6ep-13);
    p = fma(r, p, 0x1.6c16c1852b7b0p-10);
    p = fma(r, p, 0x1.1111111122322p-7);
    p = fma(r, p, 0x1.55555555502a1p-5);
    p = fma(r, p, 0x1.5555555555511p-3);
    p = fma(r, p, 0x1.000000000000bp-1);
    p = fma(r, p, 1.0);
    p = fma(r, p, 1.0);
    return ldexp(p, (int)(unsigned int)(unsigned long long)__double_as_longlong(z));  // the low word of z
#endif
}

// the same routine for a call site that runs once per loop iteration (the accept test): coefficients by fma_vc.  Bit for bit
// exp_sat, and its domain: |x| <= 1e16 (mh_accept calls it only where v_exp_f32 put exp(diff) next to a uniform: |diff| < 24)
__device__ __forceinline__ double exp_nr_v(double x) {
    const double dn = rint(x * 0x1.71547652b82fep+0);
    const double r = fma(dn, -0x1.abc9e3b39803fp-56, fma(dn, -0x1.62e42fefa39efp-1, x));
    double p = fma_vc(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
    p = fma_vc(r, p, 0x1.71dee623fde64p-19);
    p = fma_vc(r, p, 0x1.a01997c89e6b0p-16);
    p = fma_vc(r, p, 0x1.a01a014761f6ep-13);
    p = fma_vc(r, p, 0x1.6c16c1852b7b0p-10);
    p = fma_vc(r, p, 0x1.1111111122322p-7);
    p = fma_vc(r, p, 0x1.55555555502a1p-5);
    p = fma_vc(r, p, 0x1.5555555555511p-3);
    p = fma_vc(r, p, 0x1.000000000000bp-1);
    p = fma(r, p, 1.0);
    p = fma(r, p, 1.0);
    return ldexp(p, (int)dn);
}

// sin(2*pi*u) for u in [0,1): exact range reduction on u (t = 2u, k = rint(t) in {0,1,2}, r = t - k in [-1/2, 1/2] are
// all exact; sin(pi t) = (-1)^k sin(pi r)) and ONE odd polynomial for sin(pi r) on [-1/2, 1/2] (Taylor to r^21, truncation
// 1e-18; measured |error| <= 3.4e-16 against extended precision, libm's sin(2*pi*u) has 7e-16 from rounding 2*pi*u).
// 20 vector instructions and 11 coefficients; the library's sinpi evaluates a sine AND a cosine polynomial and selects
// (~36 instructions, twice the coefficients -- scalar registers the chain kernels do not have to spare).
__device__ __forceinline__ double sin_2pi(double u) {
    const double t = u + u;
    const double k = rint(t);
    double r = t - k;
    r = (k == 1.0) ? -r : r;
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
}

}  // namespace dx
