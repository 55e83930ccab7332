"""Compile-and-run harness for the device math and RNG helpers (dang_amd/csrc/dx_math.h, dx_rng.h), with the argument sets and
the extended-precision references the tests share.  A plain module: tests/test_gpu_mathlib.py and
tests/test_gpu_mathlib_helpers.py run the device program through it, tests/test_mathlib_refs_cpu.py pins the references.

A small HIP program that includes the two headers is compiled into a temporary directory; a function id selects the helper,
the input is a binary file of doubles or of 32/64-bit words, the output one of doubles or words.  One child process at a time,
each under its own timeout.  If a run ends by a signal or a timeout, FAULTED is set and every later run() fails without
starting the program again."""
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"   # as dang_amd/_build.py finds it

# name -> (id, input dtype, inputs per element, output dtype, outputs per element)
FUNCS = {
    "exp_nr": (0, np.float64, 1, np.float64, 1),
    "log_pos": (1, np.float64, 1, np.float64, 1),
    "fast_rcp": (2, np.float64, 1, np.float64, 1),
    "fast_rsqrt": (3, np.float64, 1, np.float64, 1),
    "fast_sqrt": (4, np.float64, 1, np.float64, 1),
    "exp_sat": (5, np.float64, 1, np.float64, 1),
    "exp_nr_v": (6, np.float64, 1, np.float64, 1),
    "sin_2pi": (7, np.float64, 1, np.float64, 1),
    "rand_normal": (8, np.float64, 4, np.float64, 1),      # mean, stdev, u1, u2
    "philox4x32_10": (9, np.uint32, 6, np.uint32, 4),      # c0 c1 c2 c3 k0 k1 -> four words
    "uniform2": (10, np.uint64, 4, np.float64, 2),         # seed, stream, pix, draw -> u1, u2
    "uniform3": (11, np.uint64, 4, np.float64, 3),         # seed, stream, pix, draw -> u1, u2, u3
    "u53": (12, np.uint64, 1, np.float64, 1),              # hi << 32 | lo
    "u32": (13, np.uint32, 1, np.float64, 1),
    "fast_rcp_ends": (14, np.float64, 1, np.float64, 1),
    "exp_any": (15, np.float64, 1, np.float64, 1),
}
_BY_ID = {v[0]: k for k, v in FUNCS.items()}

BUILDS = {
    "plain": [],
    "vcoef": ["-DDX_VCOEF"],
    "vcoef_rint": ["-DDX_VCOEF", "-DDX_EXP_RINT"],
    "mulhi": ["-DDX_PHILOX_MULHI"],
    "tables": ["-DDX_EXP_TABLE", "-DDX_LOG_TABLE"],
}

HARNESS = r'''
#include "dx_rng.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned long long u64;

__global__ void k_eval(const void* in, void* out, long long n, int which) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* x = (const double*)in;
    const uint32_t* w = (const uint32_t*)in;
    const u64* q = (const u64*)in;
    double* y = (double*)out;
    switch (which) {
    case 0: y[i] = dx::exp_nr(x[i]); break;
    case 1: y[i] = dx::log_pos(x[i]); break;
    case 2: y[i] = dx::fast_rcp(x[i]); break;
    case 3: y[i] = dx::fast_rsqrt(x[i]); break;
    case 4: y[i] = dx::fast_sqrt(x[i]); break;
    case 5: y[i] = dx::exp_sat(x[i]); break;
    case 6: y[i] = dx::exp_nr_v(x[i]); break;
    case 7: y[i] = dx::sin_2pi(x[i]); break;
    case 8: y[i] = dx::rand_normal(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]); break;
    case 9: {
        uint32_t o[4];
        dx::philox4x32_10(w[6 * i], w[6 * i + 1], w[6 * i + 2], w[6 * i + 3], w[6 * i + 4], w[6 * i + 5], o);
        uint32_t* yo = (uint32_t*)out + 4 * i;
        yo[0] = o[0]; yo[1] = o[1]; yo[2] = o[2]; yo[3] = o[3];
        break;
    }
    case 10: {
        double u1, u2;
        dx::uniform2(q[4 * i], q[4 * i + 1], q[4 * i + 2], (uint32_t)q[4 * i + 3], u1, u2);
        y[2 * i] = u1; y[2 * i + 1] = u2;
        break;
    }
    case 11: {
        double u1, u2, u3;
        dx::uniform3(q[4 * i], q[4 * i + 1], q[4 * i + 2], (uint32_t)q[4 * i + 3], u1, u2, u3);
        y[3 * i] = u1; y[3 * i + 1] = u2; y[3 * i + 2] = u3;
        break;
    }
    case 12: y[i] = dx::u53((uint32_t)(q[i] >> 32), (uint32_t)q[i]); break;
    case 13: y[i] = dx::u32(w[i]); break;
    case 14: y[i] = dx::fast_rcp_ends(x[i]); break;
    case 15: y[i] = dx::exp_any(x[i]); break;
    default: break;
    }
}

int main(int argc, char** argv) {
    // usage: harness which in.bin out.bin in_bytes_per_element out_bytes_per_element   (which: see tests/mathlib_harness.py)
    if (argc != 4 && argc != 6) return 2;
    const int which = atoi(argv[1]);
    const long long bin = argc == 6 ? atoll(argv[4]) : 8, bout = argc == 6 ? atoll(argv[5]) : 8;
    if (which < 0 || which > 15 || bin <= 0 || bout <= 0) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long long n = ftell(f) / bin;
    fseek(f, 0, SEEK_SET);
    std::vector<char> h((size_t)(n * bin)), o((size_t)(n * bout));
    if (fread(h.data(), bin, n, f) != (size_t)n) return 4;
    fclose(f);
    if (n == 0) return 4;
    void *din, *dout;
    if (hipMalloc(&din, n * bin) != hipSuccess || hipMalloc(&dout, n * bout) != hipSuccess) return 5;
    if (hipMemcpy(din, h.data(), n * bin, hipMemcpyHostToDevice) != hipSuccess) return 6;
    k_eval<<<(unsigned)((n + 255) / 256), 256>>>(din, dout, n, which);
    if (hipDeviceSynchronize() != hipSuccess) return 7;
    if (hipMemcpy(o.data(), dout, n * bout, hipMemcpyDeviceToHost) != hipSuccess) return 8;
    f = fopen(argv[3], "wb");
    if (!f || fwrite(o.data(), bout, n, f) != (size_t)n) return 9;
    fclose(f);
    (void)hipFree(din); (void)hipFree(dout);
    return 0;
}
'''

FAULTED = None   # why the device program is not started any more (a run that ended by a signal or a timeout)


def _compile(defs):
    """Compile the program with the given -D switches; returns run(which, x): `which` a name of FUNCS or its id."""
    d = tempfile.mkdtemp(prefix="dx_mathlib_")
    src = os.path.join(d, "harness.hip")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(d, "harness")
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "dang_amd", "csrc"),
                    "-o", exe, src] + defs, check=True, timeout=600)

    def run(which, x):
        global FAULTED
        if FAULTED:
            raise RuntimeError("the device program is not run again: " + FAULTED)
        fid, tin, nin, tout, nout = FUNCS[_BY_ID[which] if isinstance(which, int) else which]
        x = np.ascontiguousarray(x, dtype=tin)
        assert x.size % nin == 0 and x.size > 0
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        x.tofile(fin)
        try:
            p = subprocess.run([exe, str(fid), fin, fout, str(nin * x.itemsize), str(nout * np.dtype(tout).itemsize)], timeout=300)
        except subprocess.TimeoutExpired:
            FAULTED = "%s ran into its time limit" % _BY_ID[fid]
            raise
        if p.returncode < 0 or p.returncode in (134, 139):
            FAULTED = "%s ended by signal (exit status %d)" % (_BY_ID[fid], p.returncode)
        p.check_returncode()
        y = np.fromfile(fout, dtype=tout)
        assert y.size == (x.size // nin) * nout
        return y if nout == 1 else y.reshape(-1, nout)
    return run


def compile_build(name):
    return _compile(BUILDS[name])


LD = np.longdouble


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


# ---------------------------------------------------------------------------------------------- the uniforms, exactly
def u53_words(rng, n):
    """64-bit Philox word pairs (hi << 32 | lo)"""
    return rng.integers(0, 2 ** 64, n, dtype=np.uint64)


def u53_of(words):
    """dx::u53 in numpy: the same IEEE operations (conversion of a 53-bit integer is exact, the sum rounds to nearest even)"""
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def u32_of(words):
    return (np.asarray(words, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def u53_exact(word):
    """(floor(word / 2^11) + 1/2) / 2^53 in rational arithmetic, rounded to the nearest double (ties to even)"""
    return float(Fraction(2 * (int(word) >> 11) + 1, 2 ** 54))


def u32_exact(word):
    return float(Fraction(2 * int(word) + 1, 2 ** 33))


U53_EDGE_WORDS = [0, 2 ** 64 - 1, (2 ** 52 << 11) - 1, 2 ** 52 << 11, (2 ** 52 << 11) + 2 ** 11, (2 ** 52 << 11) - 2 ** 11,
                  (2 ** 52 << 11) + 2 ** 11 - 1, 2 ** 11 - 1, 2 ** 11, 2 ** 63, 2 ** 63 - 1, (2 ** 53 - 2) << 11]
U32_EDGE_WORDS = [0, 1, 2 ** 32 - 1, 2 ** 32 - 2, 2 ** 31, 2 ** 31 - 1, 2 ** 30, 3 * 2 ** 30]


def edge_words(bits, span=4096):
    """the `span` words on either side of u = 0, 1/4, 1/2, 3/4, 1 of a `bits`-bit uniform (w + 1/2) 2^-bits"""
    top = 2 ** bits
    parts = []
    for c in (0, top // 4, top // 2, 3 * (top // 4), top):
        lo, hi = max(c - span, 0), min(c + span, top)
        parts.append(np.arange(lo, hi, dtype=np.uint64))
    return np.concatenate(parts)


# ---------------------------------------------------------------------------------------------- argument sets
def rcp_arguments(rng, n=1_000_000):
    """positive magnitudes; the tests run both signs.  n per set"""
    parts = [
        np.exp2(rng.uniform(-1020, 1020, n)),                            # log-uniform over the normal range
        np.expm1(np.exp(rng.uniform(np.log(1e-6), np.log(700.0), n))),   # Planck denominators exp(t) - 1, t in [1e-6, 700]
        2.0 + rng.uniform(-0.293, 0.415, n),                             # log_pos: 2 + f
        10.0 ** rng.uniform(-3, 3, n),                                   # rms, widths
    ]
    return np.concatenate(parts)


def sqrt_arguments(rng, n=1_000_000):
    w = u53_words(rng, n)
    u = u53_of(w)
    near1 = 1.0 - np.arange(1, 2 ** 20 + 1, dtype=np.float64) * 2.0 ** -53     # the 2^20 deviates just below 1
    parts = [
        rcp_arguments(rng, n // 2),
        -2.0 * np.log(u),                                                # Box-Muller radicands
        -2.0 * np.log(near1),
        10.0 ** rng.uniform(-12, 12, n),                                 # sums of squares (Schur normalisation)
    ]
    x = np.concatenate(parts)
    return x[x > 0.0]


def sin_arguments(rng):
    """2e7 u32 deviates (1e7 words and their complements: 1 - u is the complement's deviate, exactly), 1e7 u53 deviates and
    the 4096 words on either side of u = 0, 1/4, 1/2, 3/4, 1 of both grids.  Returns (u of the u32 words, u of their
    complements, the other arguments)."""
    w = rng.integers(0, 2 ** 32, 10_000_000, dtype=np.uint64)
    w = np.concatenate([w, edge_words(32)]).astype(np.uint32)
    u = u32_of(w)
    uc = u32_of(~w)
    e53 = edge_words(53)
    rest = np.concatenate([u53_of(u53_words(rng, 10_000_000 - e53.size - 1)), (e53.astype(np.float64) + 0.5) * 2.0 ** -53,
                           np.array([u53_of([2 ** 64 - 1])[0]])])
    return u, uc, rest


MEANS = (0.0, 1.5, -3.0)
STDEVS = (1.0, 0.7, 1e-3)


def normal_arguments(rng, n=5_000_000):
    """(mean, stdev, u1, u2) rows: u1 a u53 deviate (with the small ones and those just below 1), u2 a u32 deviate (the
    Metropolis proposal, uniform3) or a u53 deviate (the prior draw and the amplitude fluctuations, uniform2)"""
    h = n // 2
    u1 = u53_of(u53_words(rng, n))
    c = n // 25
    u1[:c] = 1.0 - rng.integers(1, 2 ** 20, c).astype(np.float64) * 2.0 ** -53
    u1[c:2 * c] = (rng.integers(0, 2 ** 20, c).astype(np.float64) + 0.5) * 2.0 ** -53   # the smallest deviates
    e32, e53 = edge_words(32), edge_words(53)
    u2a = u32_of(rng.integers(0, 2 ** 32, h, dtype=np.uint64).astype(np.uint32))
    u2a[:min(e32.size, h)] = u32_of(e32.astype(np.uint32))[:h]
    u2b = u53_of(u53_words(rng, n - h))
    u2b[:min(e53.size, n - h)] = ((e53.astype(np.float64) + 0.5) * 2.0 ** -53)[:n - h]
    u2 = np.concatenate([u2a, u2b])
    perm = rng.permutation(n)      # decouple the clustered u1 from the clustered u2
    u1 = u1[perm]
    k = np.arange(n)
    m = np.array(MEANS)[k % 3]
    s = np.array(STDEVS)[(k // 3) % 3]
    return np.stack([m, s, u1, u2], axis=1)


# ---------------------------------------------------------------------------------------------- references (long double)
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)   # pi's two leading doubles, summed in long double


def ref_rcp(x):
    return LD(1) / x.astype(LD)


def ref_sqrt(x):
    return np.sqrt(x.astype(LD))


def ref_rsqrt(x):
    return LD(1) / np.sqrt(x.astype(LD))


def ref_exp(x):
    return np.exp(x.astype(LD))


def ref_log(x):
    return np.log(x.astype(LD))


def ref_sin_2pi(u):
    """the exact reduction (t = 2u, k = rint t, r = t - k are exact in double), then (-1)^k sinl(pi r)"""
    t = u + u
    k = np.rint(t)
    r = t - k
    s = np.sin(PI_LD * r.astype(LD))
    return np.where(k == 1.0, -s, s)


def ref_normal(m, s, u1, u2):
    """Box-Muller, sine branch: mean + stdev sqrt(-2 log u1) sin(2 pi u2); also returns r = sqrt(-2 log u1)"""
    r = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    return m.astype(LD) + s.astype(LD) * r * ref_sin_2pi(u2), r
