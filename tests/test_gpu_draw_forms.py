"""The Metropolis draw formed from the Philox words (dang_amd/csrc/dx_rng.h: sin_2pi_w, u53_unscaled / log_u53, rand_normal_w,
u32f_word; dx_math.h: log_pos_scaled) against the fp64 forms they replace, on the device, and the chains with the new forms
against the chains with every switch turned back.

A small device program of this file's own (the helpers are compared where they run: the mismatch count and the first mismatch
come back, not 2^32 values) is compiled in the plain build and under -DDX_VCOEF, the build of the chain kernels.  One child
process per build under its own time limit; a run that ends by a signal or a time limit is not started again.

The chains: the C3 sky at Nside 8 and the 20-band lane-pair sky at Nside 4 (the cases n8 and c5 of
tests/test_gpu_planeset_boundary.py), three iterations, once through the library's built-in kernels and once through the same
kernels compiled at run time with -DDX_DRAW_FP64 -DDX_ACCEPT_MARGIN12 (DANGX_PLANESET_RTC=1 sends the built-in shapes to the
run-time compiler): amplitudes, indices, both chi^2 and the accepted counts must agree in every bit."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NPAIRS = 1 << 26

PROGRAM = r'''
#include "dx_rng.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned long long u64;

// res[3 * c + 0] mismatches of check c, [3 * c + 1] the smallest mismatching index (word, or pair number), start ~0
__device__ void note(u64* res, int c, u64 at) { atomicAdd(&res[3 * c], 1ull); atomicMin(&res[3 * c + 1], at); }
__device__ bool differ(double a, double b) { return __double_as_longlong(a) != __double_as_longlong(b); }

// every 32-bit word: check 0 sin_2pi_w(w) == sin_2pi(u32(w)); 1 u32(w) == (2w + 1) 2^-33, formed exactly from the integer;
// 2 |u32f_word(w) - u32(w)| <= 2^-23 u32(w); 3 the same for float(u32(w)) with 2^-24
__global__ void k_words(u64* res) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const uint32_t w = (uint32_t)i;
        const double u = dx::u32(w);
        if (differ(dx::sin_2pi_w(w), dx::sin_2pi(u))) note(res, 0, i);
        if (differ(u, (double)(2ull * i + 1ull) * 0x1p-33)) note(res, 1, i);
        if (!(fabs((double)dx::u32f_word(w) - u) <= 0x1p-23 * u)) note(res, 2, i);
        if (!(fabs((double)(float)u - u) <= 0x1p-24 * u)) note(res, 3, i);
    }
}

// 64-bit word pairs (hi, lo): check 4 log_u53 == log_pos(u53); 5 rand_normal_w == rand_normal(u53, u32), third word from hi ^ lo;
// 6 u53_unscaled 2^-53 == u53
__device__ void pair_checks(u64* res, u64 at, uint32_t hi, uint32_t lo) {
    const double u1 = dx::u53(hi, lo);
    if (differ(dx::log_u53(hi, lo), dx::log_pos(u1))) note(res, 4, at);
    const uint32_t w2 = hi ^ (lo * 0x9E3779B9u);
    if (differ(dx::rand_normal_w(0.25, 0.7, hi, lo, w2), dx::rand_normal(0.25, 0.7, u1, dx::u32(w2)))) note(res, 5, at);
    if (differ(dx::u53_unscaled(hi, lo) * 0x1p-53, u1)) note(res, 6, at);
}
__global__ void k_random_pairs(u64* res, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n / 2) return;
    uint32_t o[4];
    dx::philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0x13u, 0u, 0x2545F491u, 0x4F6CDD1Du, o);
    pair_checks(res, 2 * i, o[0], o[1]);
    pair_checks(res, 2 * i + 1, o[2], o[3]);
}
__global__ void k_listed_pairs(u64* res, const u64* x, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pair_checks(res, (1ull << 40) + i, (uint32_t)(x[i] >> 32), (uint32_t)x[i]);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const u64 npairs = strtoull(argv[1], nullptr, 10);
    // the edges: all ones (u1 rounds to 1), all zeros, m = x >> 11 at 2^52 +- 1 and at 2^53 - 2, and m + 1/2 on either side of
    // sqrt(2) 2^k, where log_pos halves its mantissa, for every k; the 11 bits below m all clear and all set
    std::vector<u64> edge = {~0ull, 0ull, 1ull, 0x7ffull, 0x800ull};
    auto add_m = [&](u64 m) { if (m < (1ull << 53)) { edge.push_back(m << 11); edge.push_back((m << 11) | 0x7ffull); } };
    for (u64 d = 0; d <= 4; ++d) { add_m((1ull << 52) + d - 2); add_m((1ull << 53) - 1 - d); add_m(d); }
    for (int k = 0; k <= 52; ++k) {
        const u64 mk = (u64)floor(ldexp(1.4142135623730951, k));
        for (long long d = -4; d <= 4; ++d) if ((long long)mk + d >= 0) add_m((u64)((long long)mk + d));
    }
    const int NCHECK = 7;
    u64 h[3 * NCHECK];
    for (int c = 0; c < NCHECK; ++c) { h[3 * c] = 0; h[3 * c + 1] = ~0ull; h[3 * c + 2] = 0; }
    u64 *res, *dedge;
    if (hipMalloc(&res, sizeof(h)) != hipSuccess || hipMalloc(&dedge, edge.size() * sizeof(u64)) != hipSuccess) return 5;
    if (hipMemcpy(res, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) return 6;
    if (hipMemcpy(dedge, edge.data(), edge.size() * sizeof(u64), hipMemcpyHostToDevice) != hipSuccess) return 6;
    k_words<<<8192, 256>>>(res);
    k_random_pairs<<<(unsigned)((npairs / 2 + 255) / 256), 256>>>(res, npairs);
    k_listed_pairs<<<(unsigned)((edge.size() + 255) / 256), 256>>>(res, dedge, (u64)edge.size());
    if (hipDeviceSynchronize() != hipSuccess) return 7;
    if (hipMemcpy(h, res, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 8;
    const char* names[NCHECK] = {"sin_2pi_w", "u32_exact", "u32f_word", "u32f_double", "log_u53", "rand_normal_w", "u53_unscaled"};
    for (int c = 0; c < NCHECK; ++c) printf("%s %llu %llu\n", names[c], h[3 * c], h[3 * c + 1]);
    printf("edges %llu 0\n", (u64)edge.size());
    return 0;
}
'''

FAULTED = None


def run_program(defs):
    """{check: (mismatches, first mismatch)} of the device program compiled with `defs`"""
    global FAULTED
    if FAULTED:
        raise RuntimeError("the device program is not run again: " + FAULTED)
    d = tempfile.mkdtemp(prefix="dx_draw_forms_")
    src, exe = os.path.join(d, "draw_forms.hip"), os.path.join(d, "draw_forms")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "dang_amd", "csrc"),
                    "-o", exe, src] + defs, check=True, timeout=600)
    try:
        p = subprocess.run([exe, str(NPAIRS)], timeout=120, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        FAULTED = "it ran into its time limit"
        raise
    if p.returncode < 0 or p.returncode in (134, 139):
        FAULTED = "it ended by a signal (exit status %d)" % p.returncode
    p.check_returncode()
    out = {}
    for line in p.stdout.split("\n"):
        if line.strip():
            name, n, first = line.split()
            out[name] = (int(n), int(first))
    return out


@pytest.fixture(scope="module")
def results():
    cache = {}

    def get(build):
        if build not in cache:
            cache[build] = run_program({"plain": [], "vcoef": ["-DDX_VCOEF"]}[build])
            print(build, cache[build])
        return cache[build]
    return get


@pytest.mark.parametrize("build", ["plain", "vcoef"])
def test_word_forms_have_the_bits_of_the_fp64_forms(results, build):
    """all 2^32 words: sin_2pi_w(w) is sin_2pi(u32(w)); u32(w), which the exact branch forms when it needs it, is (2w + 1) 2^-33;
    both float forms of the accept uniform are within their bound.  2^26 random word pairs and the edges: the logarithm and the
    normal deviate from the words are those from u53."""
    r = results(build)
    assert r["edges"][0] > 400
    for name in ("sin_2pi_w", "u32_exact", "u32f_word", "u32f_double", "log_u53", "rand_normal_w", "u53_unscaled"):
        n, first = r[name]
        assert n == 0, "%s: %d mismatches, the first at %#x" % (name, n, first)


# ---------------------------------------------------------------------------------------------------------------- the chains
OLD_FORMS = "-DDX_DRAW_FP64 -DDX_ACCEPT_MARGIN12"


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name", ["n8", "c5"])
def test_chains_are_bit_for_bit_those_of_the_old_forms(built, name, monkeypatch):
    import test_gpu_planeset_boundary as B
    new, eng = B.run_case(name)
    assert not any(n.startswith("dxk::k_plane_set<") for n in eng.rtc_kernels()), "the default build's kernels are built in"
    monkeypatch.setenv("DANGX_PLANESET_RTC", "1")
    monkeypatch.setenv("DANGX_RTC_DEFS", OLD_FORMS)
    old, eng_old = B.run_case(name)
    assert any(n.startswith("dxk::k_plane_set<") for n in eng_old.rtc_kernels()), eng_old.rtc_kernels()
    assert sorted(new) == sorted(old)
    for k in sorted(new):
        assert _bits_equal(new[k], old[k]), (name, k, int(np.count_nonzero(new[k] != old[k])))
    assert int(new["accepted"].sum()) > 0
