"""Accuracy of the sampler kernels' fp64 exp and log (dang_amd/csrc/dx_math.h: exp_nr, log_pos, and their table forms
-DDX_EXP_TABLE / -DDX_LOG_TABLE) on the device.

A small HIP program that includes dx_math.h is compiled into a temporary directory and run over 8.1e6 exp and 1.1e7 log arguments from
the ranges the kernels use -- beta ln(nu/nu_ref), h nu / (k T), accept-test differences, uniform deviates, frequencies,
temperatures -- uniform and clustered at the table boundaries, at 1 and at the ends of the range.  The results are compared
with numpy.longdouble (x87 extended) references: at most 1 ulp, and the maximum is reported."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"   # as dang_amd/_build.py finds it

HARNESS = r'''
#include "dx_math.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

__global__ void k_eval(const double* x, double* y, long long n, int which) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = which == 0 ? dx::exp_nr(x[i]) : dx::log_pos(x[i]);
}

int main(int argc, char** argv) {
    // usage: harness which in.bin out.bin   (which: 0 = exp_nr, 1 = log_pos)
    if (argc != 4) return 2;
    const int which = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long long n = ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    std::vector<double> h(n);
    if (fread(h.data(), 8, n, f) != (size_t)n) return 4;
    fclose(f);
    double *dx_, *dy;
    if (hipMalloc(&dx_, n * 8) != hipSuccess || hipMalloc(&dy, n * 8) != hipSuccess) return 5;
    if (hipMemcpy(dx_, h.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess) return 6;
    k_eval<<<(unsigned)((n + 255) / 256), 256>>>(dx_, dy, n, which);
    if (hipDeviceSynchronize() != hipSuccess) return 7;
    if (hipMemcpy(h.data(), dy, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return 8;
    f = fopen(argv[3], "wb");
    if (!f || fwrite(h.data(), 8, n, f) != (size_t)n) return 9;
    fclose(f);
    hipFree(dx_); hipFree(dy);
    return 0;
}
'''


def _compile(defs):
    d = tempfile.mkdtemp(prefix="dx_mathlib_")
    src = os.path.join(d, "harness.hip")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(d, "harness")
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "dang_amd", "csrc"),
                    "-o", exe, src] + defs, check=True, timeout=600)

    def run(which, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        x.tofile(fin)
        subprocess.run([exe, str(which), fin, fout], check=True, timeout=300)
        return np.fromfile(fout, dtype=np.float64)
    return run


@pytest.fixture(scope="module")
def harness():
    """the kernels' build"""
    return _compile([])


@pytest.fixture(scope="module")
def harness_tables():
    """the table forms of exp_nr and log_pos (-DDX_EXP_TABLE -DDX_LOG_TABLE; off in the kernels, see dx_math.h)"""
    return _compile(["-DDX_EXP_TABLE", "-DDX_LOG_TABLE"])


def ulp_error(y, ref):
    """|y - ref| in units of the spacing of doubles at ref (ref in long double)."""
    r64 = ref.astype(np.float64)
    sp = np.spacing(np.abs(r64)).astype(np.longdouble)
    # below a power of two the spacing is half of the one np.spacing gives for the rounded value
    sp = np.where(np.abs(ref) < np.abs(r64.astype(np.longdouble)), np.spacing(np.nextafter(np.abs(r64), 0)).astype(np.longdouble), sp)
    return np.abs(y.astype(np.longdouble) - ref) / sp


def exp_arguments(rng):
    ln2n = np.log(2.0) / 128
    parts = [
        rng.uniform(-5, 5, 1_500_000) * rng.uniform(-6, 6, 1_500_000),   # beta ln(nu/nu_ref)
        rng.uniform(-30, 30, 1_500_000),
        rng.uniform(0, 60, 1_000_000),                                  # h nu / (k T) for T >= 1 K below 1.2 THz
        rng.uniform(-708, 709, 1_000_000),                              # the whole normal range
        -rng.exponential(2.0, 1_000_000),                               # accept-test differences
        rng.uniform(-1e-3, 1e-3, 500_000),                              # near 0
        rng.uniform(-1e-12, 1e-12, 100_000),
    ]
    # table-boundary clustering: (k + 1/2) ln2/128 +- a few ulp, and k ln2/128 +- a few ulp
    k = rng.integers(-60000, 60000, 1_000_000)
    half = (k + 0.5) * ln2n
    parts.append(half + np.spacing(np.abs(half) + 1e-300) * rng.integers(-8, 9, half.size))
    whole = k[:500_000] * ln2n
    parts.append(whole + np.spacing(np.abs(whole) + 1e-300) * rng.integers(-8, 9, whole.size))
    x = np.concatenate(parts)
    return x[(x > -708.0) & (x < 709.0)]


def log_arguments(rng):
    w = rng.integers(0, 2 ** 53, 3_000_000, dtype=np.int64)
    u53 = (w.astype(np.float64) + 0.5) * 2.0 ** -53                   # the proposal uniform (dx_rng.h: u53)
    parts = [
        u53,
        1.0 - rng.integers(1, 2 ** 20, 1_000_000).astype(np.float64) * 2.0 ** -53,   # u just below 1
        1.0 + rng.integers(1, 2 ** 20, 500_000).astype(np.float64) * 2.0 ** -52,     # just above 1
        rng.uniform(0.9, 1.1, 1_500_000),
        rng.uniform(0.6875, 1.375, 1_000_000),                          # one period of the table
        10.0 ** rng.uniform(0, 3.5, 1_000_000),                         # nu / 1e9, nu / nu_p
        10.0 ** rng.uniform(-1, 5.5, 1_000_000),                        # temperatures, T_e / 1e4
        10.0 ** rng.uniform(-300, 300, 500_000),                        # every normal exponent
        np.exp(rng.uniform(-700, 700, 500_000)),
    ]
    # subinterval boundaries of the table: z = 0.6875 + j 2^-8 (z < 1) and 1 + j 2^-7, scaled by 2^k, +- a few ulp
    j = rng.integers(0, 128, 1_000_000)
    z = np.where(j < 80, 0.6875 + j * 2.0 ** -8, 1.0 + (j - 80) * 2.0 ** -7)
    z = np.ldexp(z, rng.integers(-40, 40, j.size))
    parts.append(z + np.spacing(z) * rng.integers(-8, 9, z.size))
    x = np.concatenate(parts)
    return x[(x > 2.3e-308) & np.isfinite(x)]


def check_exp(harness, name):
    x = exp_arguments(np.random.default_rng(11))
    assert x.size >= 6_000_000
    y = harness(0, x)
    ref = np.exp(x.astype(np.longdouble))
    e = ulp_error(y, ref)
    worst = int(np.argmax(e))
    print("%s: %d arguments, max %.4f ulp at x = %r, mean %.4f" % (name, x.size, e[worst], x[worst], float(e.mean())))
    assert e.max() <= 1.0
    # saturation: ldexp gives inf above ~709.8 and 0 below ~-745 (|x| < 1.4e9), as the polynomial form does
    big = np.array([710.0, 800.0, 1e4, 1e6, 1e8, 1.3e9, -746.0, -800.0, -1e4, -1e6, -1e8, -1.3e9])
    yb = harness(0, big)
    assert np.all(np.isinf(yb[:6]) & (yb[:6] > 0)) and np.all(yb[6:] == 0.0), yb


@pytest.mark.gpu
def test_exp_nr_within_one_ulp(harness):
    check_exp(harness, "exp_nr")


@pytest.mark.gpu
def test_exp_nr_table_form_within_one_ulp(harness_tables):
    check_exp(harness_tables, "exp_nr (DX_EXP_TABLE)")


def check_log(harness, name):
    x = log_arguments(np.random.default_rng(12))
    assert x.size >= 6_000_000
    y = harness(1, x)
    ref = np.log(x.astype(np.longdouble))
    e = ulp_error(y, ref)
    e = np.where(x == 1.0, np.abs(y) * 1e300, e)   # log 1 = 0 exactly
    worst = int(np.argmax(e))
    print("%s: %d arguments, max %.4f ulp at x = %r, mean %.4f" % (name, x.size, e[worst], x[worst], float(e.mean())))
    assert e.max() <= 1.0
    assert harness(1, np.array([1.0]))[0] == 0.0


@pytest.mark.gpu
def test_log_pos_within_one_ulp(harness):
    check_log(harness, "log_pos")


@pytest.mark.gpu
def test_log_pos_table_form_within_one_ulp(harness_tables):
    check_log(harness_tables, "log_pos (DX_LOG_TABLE)")
