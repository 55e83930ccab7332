"""Every device math and RNG helper of dang_amd/csrc/dx_math.h and dx_rng.h on the device, in the builds the chains use.

tests/test_gpu_mathlib.py covers exp_nr and log_pos in the default build.  Here: fast_rcp, fast_rsqrt, fast_sqrt, exp_sat, exp_nr_v,
sin_2pi, rand_normal, philox4x32_10, uniform2, uniform3, u53 and u32, in the plain build, under -DDX_VCOEF (the register-chain,
plane-set, fused and run-time specialised kernels: fma_vc is inline v_fma_f64 assembly there), -DDX_VCOEF -DDX_EXP_RINT and
-DDX_PHILOX_MULHI.  References are numpy.longdouble (pinned against mpmath by tests/test_mathlib_refs_cpu.py), the bounds are
the headers' own claims, and every test prints its measured maximum and the argument where it occurs."""
import functools

import numpy as np
import pytest

import mathlib_harness as H
import oracle_ffi as O
from mathlib_harness import LD, ulp_error

pytestmark = pytest.mark.gpu


class Device:
    """the device program in each build: compiled once per module, on first use"""

    def __init__(self):
        self.builds = {}

    def __call__(self, build, fn, x):
        if build not in self.builds:
            self.builds[build] = H.compile_build(build)
        return self.builds[build](fn, x)


@pytest.fixture(scope="module")
def dev():
    return Device()


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def report(name, x, e, unit="ulp"):
    worst = int(np.argmax(e))
    print("%s: %d arguments, max %.4f %s at x = %r, mean %.4f" % (name, x.shape[0], float(e[worst]), unit, x[worst].tolist(), float(e.mean())))
    return float(e[worst])


@functools.lru_cache(maxsize=None)
def rcp_args():
    x = H.rcp_arguments(np.random.default_rng(21))
    return np.concatenate([x, -x])


@functools.lru_cache(maxsize=None)
def sqrt_args():
    return H.sqrt_arguments(np.random.default_rng(22))


@functools.lru_cache(maxsize=None)
def exp_args():
    return H.exp_arguments(np.random.default_rng(11))


@functools.lru_cache(maxsize=None)
def sin_args():
    return H.sin_arguments(np.random.default_rng(23))


@functools.lru_cache(maxsize=None)
def normal_args():
    return H.normal_arguments(np.random.default_rng(24))


# ------------------------------------------------------------------------------------------------ reciprocal, square roots
def test_fast_rcp_within_one_ulp(dev):
    """1/x, both signs: log-uniform over [2^-1020, 2^1020], the Planck denominators exp(t) - 1 for t in [1e-6, 700], log_pos's
    2 + f, and 1e-3 .. 1e3.  <= 1 ulp (dx_math.h).  fast_rcp_ends is the same bits on all of them."""
    x = rcp_args()
    assert 4_000_000 <= x.size <= 10_000_000
    y = dev("plain", "fast_rcp", x)
    assert report("fast_rcp", x, ulp_error(y, H.ref_rcp(x))) <= 1.0
    assert same_bits(dev("plain", "fast_rcp_ends", x), y)
    assert same_bits(dev("vcoef", "fast_rcp", x), y)


SQRT_REL = 2.5 * 2.0 ** -53 * (1 + 2.0 ** -20)


def relative_error(y, ref):
    """|y - ref| / |ref| in units of 2^-53 (half the spacing of doubles at 1)"""
    return np.abs(y.astype(LD) - ref) / np.abs(ref) * LD(2) ** 53


def check_goldschmidt(name, x, y, ref):
    """The Goldschmidt pair of dx_math.h carries four roundings into its result ("Device math helpers"): relative
    error <= 2.5 * 2^-53, which is between 1.25 and 2.5 ulp depending on where the result lies in its binade -- not the 1 ulp
    the header used to claim (measured: 1.43 ulp fast_sqrt, 1.63 ulp fast_rsqrt)."""
    report(name, x, ulp_error(y, ref))
    assert report(name + ", relative", x, relative_error(y, ref), "2^-53") <= SQRT_REL * 2.0 ** 53


def test_fast_sqrt_within_its_bound(dev):
    """sqrt(x): fast_rcp's magnitudes, the Box-Muller radicands -2 log(u) over u53 deviates with the 2^20 values just below 1,
    and sums of squares in 1e-12 .. 1e12."""
    x = sqrt_args()
    assert 3_000_000 <= x.size <= 10_000_000
    y = dev("plain", "fast_sqrt", x)
    check_goldschmidt("fast_sqrt", x, y, H.ref_sqrt(x))
    assert same_bits(dev("vcoef", "fast_sqrt", x), y)


def test_fast_rsqrt_within_its_bound(dev):
    """1/sqrt(x) on fast_sqrt's arguments"""
    x = sqrt_args()
    y = dev("plain", "fast_rsqrt", x)
    check_goldschmidt("fast_rsqrt", x, y, H.ref_rsqrt(x))


# ------------------------------------------------------------------------------------------------ exponentials
def test_exp_sat_within_one_ulp(dev):
    x = exp_args()
    assert 6_000_000 <= x.size <= 10_000_000
    y = dev("plain", "exp_sat", x)
    assert report("exp_sat", x, ulp_error(y, H.ref_exp(x))) <= 1.0


@pytest.mark.parametrize("build", ["plain", "vcoef", "vcoef_rint", "mulhi"])
def test_exp_sat_and_exp_nr_v_are_the_same_bits(dev, build):
    """exp_nr_v is exp_sat with its coefficients through fma_vc: bit-equal on every argument, in every build -- and to the plain
    build's exp_sat, which test_exp_sat_within_one_ulp holds to 1 ulp."""
    x = exp_args()
    base = dev("plain", "exp_sat", x)
    assert same_bits(dev(build, "exp_sat", x), base)
    assert same_bits(dev(build, "exp_nr_v", x), base)


@pytest.mark.parametrize("build", ["plain", "vcoef"])
def test_exp_nr_against_exp_sat(dev, build):
    """exp_nr takes n = rint(x log2e) out of one fma: <= 1 ulp, and it differs from exp_sat in the last bit at most, and only
    where x log2e lies within two double spacings of a half-integer (dx_math.h)."""
    x = exp_args()
    y = dev(build, "exp_nr", x)
    assert report("exp_nr (%s)" % build, x, ulp_error(y, H.ref_exp(x))) <= 1.0
    ys = dev(build, "exp_sat", x)
    d = y.view(np.int64) - ys.view(np.int64)
    t = x.astype(LD) * (LD(1) / np.log(LD(2)))
    dist = np.abs(t - np.floor(t) - LD(0.5))
    near = dist <= 2 * np.spacing(np.abs(t.astype(np.float64))).astype(LD)
    print("exp_nr (%s) differs from exp_sat at %d of %d arguments, %d of them near a half-integer (of %d such)"
          % (build, int((d != 0).sum()), x.size, int(((d != 0) & near).sum()), int(near.sum())))
    assert np.abs(d).max() <= 1
    assert not np.any((d != 0) & ~near)


def test_exp_nr_is_exp_sat_under_exp_rint(dev):
    x = exp_args()
    assert same_bits(dev("vcoef_rint", "exp_nr", x), dev("plain", "exp_sat", x))


def test_exp_nr_saturates_under_vcoef(dev):
    """the saturation test of tests/test_gpu_mathlib.py in the chain kernels' build"""
    big = np.array([710.0, 800.0, 1e4, 1e6, 1e8, 1.3e9, -746.0, -800.0, -1e4, -1e6, -1e8, -1.3e9])
    for build in ("vcoef", "vcoef_rint"):
        yb = dev(build, "exp_nr", big)
        assert np.all(np.isinf(yb[:6]) & (yb[:6] > 0)) and np.all(yb[6:] == 0.0), (build, yb)


# ------------------------------------------------------------------------------------------------ sine
def test_sin_2pi(dev):
    """sin(2 pi u) on 2e7 u32 deviates (1e7 words and their complements), 1e7 u53 deviates and the 4096 words on either side of
    u = 0, 1/4, 1/2, 3/4, 1.  Reference: the exact reduction, then sinl(pi r).

    Bounds: |error| <= 3.4e-16 (dx_math.h); the sign is right and |y| <= 1; sin_2pi(1 - u) == -sin_2pi(u) bit for bit on the u32
    values, where 1 - u is exact; relative error <= 4 ulp.  The 4 ulp: a CPU restatement of the same IEEE operations measured
    2.98 ulp (3.31e-16 absolute) over 3e7 such arguments; the margin up to 4 covers arguments that were not sampled."""
    u, uc, rest = sin_args()
    assert np.array_equal(1.0 - u, uc)
    yu, yc = dev("plain", "sin_2pi", u), dev("plain", "sin_2pi", uc)
    assert same_bits(yc, -yu)
    worst_abs = worst_rel = 0.0
    for name, x, y in (("u32", u, yu), ("1 - u32", uc, yc), ("u53", rest, dev("plain", "sin_2pi", rest))):
        ref = H.ref_sin_2pi(x)
        assert not np.isnan(y).any()
        assert np.abs(y).max() <= 1.0
        zero = ref == 0
        assert np.all(y[zero] == 0.0)
        assert np.array_equal(np.sign(y[~zero]), np.sign(ref[~zero]).astype(np.float64))
        ea = np.abs(y.astype(LD) - ref).astype(np.float64)
        er = np.where(zero, 0.0, ulp_error(y, np.where(zero, LD(1), ref)).astype(np.float64))
        worst_abs = max(worst_abs, report("sin_2pi, %s, absolute" % name, x, ea / 1e-16, "e-16"))
        worst_rel = max(worst_rel, report("sin_2pi, %s, relative" % name, x, er))
    assert worst_abs <= 3.4
    assert worst_rel <= 4.0


# ------------------------------------------------------------------------------------------------ DX_VCOEF against the plain build
@pytest.mark.parametrize("build", ["vcoef", "vcoef_rint"])
def test_vcoef_build_is_bit_equal(dev, build):
    """fma_vc's inline v_fma_f64 is the same operation as fma: log_pos, exp_nr_v, sin_2pi and rand_normal give the plain build's
    bits on all of their arguments; any difference is a bug in the assembly constraints."""
    u, uc, rest = sin_args()
    sets = [("log_pos", H.log_arguments(np.random.default_rng(12))), ("exp_nr_v", exp_args()), ("sin_2pi", u), ("sin_2pi", uc),
            ("sin_2pi", rest), ("rand_normal", normal_args())]
    for fn, x in sets:
        a, b = dev("plain", fn, x), dev(build, fn, x)
        bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
        print("%s (%s): %d arguments, %d differ" % (fn, build, a.size, bad.size))
        assert bad.size == 0, (fn, x[bad[:4]], a[bad[:4]], b[bad[:4]])


# ------------------------------------------------------------------------------------------------ Philox and the uniforms
KAT = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


@pytest.mark.parametrize("build", ["plain", "mulhi", "vcoef"])
def test_philox_known_answers(dev, build):
    """Random123 kat_vectors for philox4x32-10 (as tests/test_oracle_cpu.py holds the oracle to), in both multiply forms"""
    w = np.array([c + k for c, k, _ in KAT], dtype=np.uint32)
    out = dev(build, "philox4x32_10", w)
    assert out.tolist() == [o for _, _, o in KAT]


SEEDS = [1234, 0xDEADBEEF12345678, 2 ** 64 - 1]
STREAMS = [77, 0x8000000000000001, 0xFFFFFFFF00000000]
PIXELS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 48 - 1]
DRAWS = [0, 1, 3, 44, 65535, 65536]


@pytest.mark.parametrize("build", ["plain", "mulhi", "vcoef"])
def test_uniforms_equal_the_oracle(dev, build):
    """uniform2 and uniform3 bit-equal to the oracle's, with high words set in the seed and the stream and pixel labels past 2^32"""
    grid = [(s, t, p, d) for s in SEEDS for t in STREAMS for p in PIXELS for d in DRAWS]
    w = np.array(grid, dtype=np.uint64)
    u2 = dev(build, "uniform2", w)
    u3 = dev(build, "uniform3", w)
    r2 = np.array([O.uniform2(*g) for g in grid])
    r3 = np.array([O.uniform3(*g) for g in grid])
    assert same_bits(u2, r2)
    assert same_bits(u3, r3)
    # the labels past 2^32 are streams of their own while the draw slot stays below 2^16 (the pixel's high word is folded in above it)
    low = [i for i, g in enumerate(grid) if g[3] < 65536]
    assert len({tuple(r3[i].tolist()) for i in low}) == len(low)


def test_u53_and_u32_exact(dev):
    """(w + 1/2) 2^-bits against rational arithmetic rounded to nearest even: 0, all ones (exactly 1.0 for u53), either side of
    2^52 << 11 where w + 1/2 stops being representable, and 1e5 random words"""
    rng = np.random.default_rng(25)
    w53 = np.concatenate([np.array(H.U53_EDGE_WORDS, dtype=np.uint64), H.u53_words(rng, 100_000)])
    y = dev("plain", "u53", w53)
    ref = np.array([H.u53_exact(w) for w in w53.tolist()])
    assert same_bits(y, ref)
    assert y[1] == 1.0 and y[0] == 2.0 ** -54
    assert y.min() > 0.0 and y.max() <= 1.0
    w32 = np.concatenate([np.array(H.U32_EDGE_WORDS, dtype=np.uint32), rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)])
    y = dev("plain", "u32", w32)
    ref = np.array([H.u32_exact(w) for w in w32.tolist()])
    assert same_bits(y, ref)
    assert y.min() > 0.0 and y.max() < 1.0


# ------------------------------------------------------------------------------------------------ the normal deviate
def test_rand_normal(dev):
    """5e6 (u1, u2) pairs from the u53 and u32 grids, mean and stdev from {0, 1.5, -3} x {1, 0.7, 1e-3}, against long-double
    Box-Muller (sine branch).  Tolerance stdev r (3.4e-16 + 4 2^-53) + 2^-53 |ref|: the sine's absolute bound, 1 ulp each from
    log and sqrt propagated through r = sqrt(-2 log u1) and the rounding of stdev r, and the final fma's rounding."""
    a = normal_args()
    assert a.shape == (5_000_000, 4)
    y = dev("plain", "rand_normal", a)
    assert not np.isnan(y).any()
    ref, r = H.ref_normal(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    tol = a[:, 1].astype(LD) * r * (LD(3.4e-16) + 4 * LD(2) ** -53) + LD(2) ** -53 * np.abs(ref)
    e = (np.abs(y.astype(LD) - ref) / tol).astype(np.float64)
    assert report("rand_normal, |error| / tolerance", a, e, "") <= 1.0


def test_rand_normal_at_u1_equal_one(dev):
    """u53 gives exactly 1.0 for 2048 word patterns: the radicand is -0 and the deviate is the mean itself, for every u2"""
    rng = np.random.default_rng(26)
    u2 = np.concatenate([H.u32_of(H.edge_words(32).astype(np.uint32)), (H.edge_words(53).astype(np.float64) + 0.5) * 2.0 ** -53,
                         H.u32_of(rng.integers(0, 2 ** 32, 50_000, dtype=np.uint64).astype(np.uint32)), H.u53_of(H.u53_words(rng, 50_000))])
    a = np.concatenate([np.stack([np.full(u2.size, m), np.full(u2.size, s), np.ones(u2.size), u2], axis=1) for m in H.MEANS for s in H.STDEVS])
    for build in ("plain", "vcoef"):
        y = dev(build, "rand_normal", a)
        assert same_bits(y, a[:, 0]), build


# ------------------------------------------------------------------------------------------------ the ends of the domains
MAXD = np.finfo(np.float64).max
DENORM = 5e-324
MINN = 2.0 ** -1022


def test_fast_rcp_domain(dev):
    """fast_rcp is stated for finite normal x: exact at the ends of that range (min normal, 2^1022), and within one spacing
    of the denormal result for 2^1023 and the largest double.  At 0, at denormals whose reciprocal overflows and at +-inf the
    Newton steps turn v_rcp_f64's IEEE result into NaN (printed, the header says so); fast_rcp_ends gives what IEEE division
    gives at every one of them: 1/0 = inf, 1/denormal = inf (overflow) or finite, 1/inf = 0."""
    x = np.array([MINN, 2.0 ** 1022, 2.0 ** 1023, MAXD, -MINN, -2.0 ** 1022, -2.0 ** 1023, -MAXD])
    for fn in ("fast_rcp", "fast_rcp_ends"):
        y = dev("plain", fn, x)
        print(fn, "at", x.tolist(), "->", y.tolist())
        assert np.array_equal(y[[0, 1, 4, 5]], 1.0 / x[[0, 1, 4, 5]])
        assert np.all(np.abs(y[[2, 3, 6, 7]] - 1.0 / x[[2, 3, 6, 7]]) <= 5e-324)
    ends = np.array([0.0, -0.0, DENORM, -DENORM, 2.0 ** -1030, np.inf, -np.inf])
    print("fast_rcp at", ends.tolist(), "->", dev("plain", "fast_rcp", ends).tolist())
    for build in ("plain", "vcoef"):
        y = dev(build, "fast_rcp_ends", ends)
        print("fast_rcp_ends (%s) at" % build, ends.tolist(), "->", y.tolist())
        assert same_bits(y, np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf, 0.0, -0.0]))
    # denormals whose reciprocal is finite: <= 1 ulp like the normal range, down to 2^-1024 (1 + 2^-20) -- closer to 2^-1024 the
    # seed's own error (2^-23) can carry it past the largest double: inf where IEEE division gives a finite value, printed
    print("fast_rcp_ends at 2^-1024 + 5e-324 ->", dev("plain", "fast_rcp_ends", np.array([2.0 ** -1024 + 5e-324])).tolist())
    d = np.array([2.0 ** -1023, 3 * 2.0 ** -1024, 2.0 ** -1022 - 5e-324, 2.0 ** -1024 * (1 + 2.0 ** -20)])
    y = dev("plain", "fast_rcp_ends", d)
    print("fast_rcp_ends at", d.tolist(), "->", y.tolist())
    assert ulp_error(y, H.ref_rcp(d)).max() <= 1.0
    assert np.isnan(dev("plain", "fast_rcp_ends", np.array([np.nan])))[0]


def test_fast_sqrt_and_rsqrt_domain(dev):
    """finite normal x > 0: the bound holds at min normal, 2^1022, 2^1023 and the largest double.  (Beyond: NaN at 0 and +inf,
    where the reference's arithmetic gives 0 / inf; rand_normal selects around its -0, the Schur sums are positive and finite.)"""
    x = np.array([MINN, 2.0 ** 1022, 2.0 ** 1023, MAXD])
    ys, yr = dev("plain", "fast_sqrt", x), dev("plain", "fast_rsqrt", x)
    print("fast_sqrt at", x.tolist(), "->", ys.tolist(), "fast_rsqrt ->", yr.tolist())
    assert relative_error(ys, H.ref_sqrt(x)).max() <= SQRT_REL * 2.0 ** 53
    assert relative_error(yr, H.ref_rsqrt(x)).max() <= SQRT_REL * 2.0 ** 53
    ends = np.array([0.0, DENORM, np.inf])
    print("beyond the domain:", ends.tolist(), "fast_sqrt ->", dev("plain", "fast_sqrt", ends).tolist(),
          "fast_rsqrt ->", dev("plain", "fast_rsqrt", ends).tolist())


EXP_DOMAIN = [710.0, 746.0, 1e4, 1.4e9, 2.0 ** 31 / np.log2(np.e) - 1, 2.0 ** 31 / np.log2(np.e) + 1, 1e10, 4e15, 1e16]
EXP_BEYOND = [1e20, 1e100, 1e300, MAXD, np.inf]


def check_exp_ends(name, x, y):
    """IEEE arithmetic on the mathematical function: +inf above the range, the denormal or +0 below it"""
    with np.errstate(over="ignore", under="ignore"):
        ref = np.exp(x.astype(LD)).astype(np.float64)
    print(name, [(a, b) for a, b in zip(x.tolist(), y.tolist())])
    assert not np.isnan(y).any(), (name, x[np.isnan(y)])
    assert not np.signbit(y).any(), (name, x[np.signbit(y)], y[np.signbit(y)])
    with np.errstate(invalid="ignore"):
        ok = (y == ref) | (np.abs(y - ref) <= 5e-324)
    assert ok.all(), (name, x[~ok], y[~ok])


@pytest.mark.parametrize("build", ["plain", "vcoef"])
def test_exp_sat_and_exp_nr_v_domain(dev, build):
    """exp_sat and exp_nr_v hold for |x| <= 1e16 (dx_math.h): +inf, a denormal or +0 out there, never a NaN or a wrong sign.
    Beyond (|x| >~ 2^53 the reduction no longer resolves the integer part, +-inf gives NaN) call sites take exp_any, which
    gives the IEEE value for every argument, the infinities included, and keeps a NaN."""
    x = np.array(EXP_DOMAIN + [-v for v in EXP_DOMAIN])
    for fn in ("exp_sat", "exp_nr_v", "exp_any"):
        check_exp_ends("%s (%s)" % (fn, build), x, dev(build, fn, x))
    xb = np.array(EXP_BEYOND + [-v for v in EXP_BEYOND])
    check_exp_ends("exp_any (%s)" % build, xb, dev(build, "exp_any", xb))
    assert np.isnan(dev(build, "exp_any", np.array([np.nan])))[0]
    print("exp_sat beyond its domain (%s):" % build, list(zip(xb.tolist(), dev(build, "exp_sat", xb).tolist())))


def test_exp_any_is_exp_sat_on_its_domain(dev):
    x = exp_args()
    assert same_bits(dev("plain", "exp_any", x), dev("plain", "exp_sat", x))
