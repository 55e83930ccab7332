"""The references and argument sets of tests/test_gpu_mathlib_helpers.py themselves (tests/mathlib_harness.py), without a
device: a wrong reference must not excuse a kernel.

The long-double references against mpmath at 40 digits; the rational model of u53 / u32 against the oracle's uniforms; the
argument generators keep their sizes and stay inside each helper's stated domain."""
import numpy as np
import pytest

import mathlib_harness as H
import oracle_ffi as O
from mathlib_harness import LD

N = 10_000
# long double carries 64 bits, 11 more than a double: a few of its roundings stay below 2^-9 of a double's last place
REF_ULP = 2.0 ** -9


def _sample(x, n=N, seed=31):
    return x[np.random.default_rng(seed).choice(x.shape[0], n, replace=False)]


def _mpf(r):
    """a long double as an mpmath number, exactly: the mantissa's leading double and its remainder"""
    import mpmath as mp
    m, e = np.frexp(r)
    hi = float(m)
    return mp.ldexp(mp.mpf(hi) + mp.ldexp(mp.mpf(float((m - LD(hi)) * LD(2) ** 64)), -64), int(e))


def _check(ref, exact, what):
    """ref (long double) against exact (mpmath) in units of the spacing of doubles at the value"""
    mp = pytest.importorskip("mpmath")
    e = np.array([float(abs(_mpf(r) - v) / mp.mpf(float(np.spacing(abs(float(v))))))
                  for r, v in zip(ref, exact)])
    print("%s: max %.3e ulp of a double" % (what, e.max()))
    assert e.max() <= REF_ULP


def test_long_double_is_extended_precision():
    assert np.finfo(LD).nmant >= 63


def test_reference_rcp_sqrt_rsqrt():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    x = _sample(H.rcp_arguments(np.random.default_rng(21), 20_000))
    _check(H.ref_rcp(x), [1 / mp.mpf(float(v)) for v in x], "1/x")
    x = _sample(H.sqrt_arguments(np.random.default_rng(22), 20_000))
    _check(H.ref_sqrt(x), [mp.sqrt(mp.mpf(float(v))) for v in x], "sqrt")
    _check(H.ref_rsqrt(x), [1 / mp.sqrt(mp.mpf(float(v))) for v in x], "1/sqrt")


def test_reference_exp_and_log():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    x = _sample(H.exp_arguments(np.random.default_rng(11)))
    _check(H.ref_exp(x), [mp.exp(mp.mpf(float(v))) for v in x], "exp")
    x = _sample(H.log_arguments(np.random.default_rng(12)))
    x = x[x != 1.0]
    _check(H.ref_log(x), [mp.log(mp.mpf(float(v))) for v in x], "log")


def test_reference_sin_2pi():
    """relative to the value: the sine's 4 ulp bound is relative, and near u = 1/2 the values are tiny"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    u, uc, rest = H.sin_arguments(np.random.default_rng(23))
    x = np.concatenate([_sample(u, N // 2), _sample(rest, N // 2), u[-5 * 8192::64], rest[-5 * 8192 - 1::64]])
    ref = H.ref_sin_2pi(x)
    exact = [mp.sinpi(2 * mp.mpf(float(v))) for v in x]
    nz = np.array([v != 0 for v in exact])
    assert np.all(ref[~nz] == 0)
    _check(ref[nz], [v for v in exact if v != 0], "sin(2 pi u)")


def test_reference_normal():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    a = _sample(H.normal_arguments(np.random.default_rng(24), 200_000))
    ref, r = H.ref_normal(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    rr = [mp.sqrt(-2 * mp.log(mp.mpf(float(u1)))) for u1 in a[:, 2]]
    _check(r, rr, "sqrt(-2 log u1)")
    # the sum with the mean cancels: absolute, in units of the test's own tolerance
    ex = [mp.mpf(float(m)) + mp.mpf(float(s)) * q * mp.sinpi(2 * mp.mpf(float(u2))) for (m, s, _, u2), q in zip(a, rr)]
    tol = a[:, 1] * r.astype(np.float64) * (3.4e-16 + 4 * 2.0 ** -53) + 2.0 ** -53 * np.abs(ref.astype(np.float64))
    e = np.array([float(abs(_mpf(v) - w)) for v, w in zip(ref, ex)]) / tol
    print("rand_normal reference: max %.3e of the tolerance" % e.max())
    assert e.max() <= REF_ULP


def test_pi_constant():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    assert abs(_mpf(H.PI_LD) - mp.pi) < mp.mpf(2) ** -64


def test_uniform_models_against_the_oracle():
    """the rational model of u53 / u32 and the numpy restatement equal the oracle's uniforms on the Philox words"""
    rng = np.random.default_rng(32)
    for _ in range(2000):
        seed, stream, pix = (int(v) for v in rng.integers(0, 2 ** 64, 3, dtype=np.uint64))
        draw = int(rng.integers(0, 2 ** 32))
        ctr = [pix & 0xffffffff, draw ^ (((pix >> 32) << 16) & 0xffffffff), stream & 0xffffffff, stream >> 32]
        o = O.philox(ctr, [seed & 0xffffffff, seed >> 32])
        u2 = O.uniform2(seed, stream, pix, draw)
        u3 = O.uniform3(seed, stream, pix, draw)
        assert u2 == (H.u53_exact(o[0] << 32 | o[1]), H.u53_exact(o[2] << 32 | o[3]))
        assert u3 == (H.u53_exact(o[0] << 32 | o[1]), H.u32_exact(o[2]), H.u32_exact(o[3]))
    w = np.concatenate([np.array(H.U53_EDGE_WORDS, dtype=np.uint64), H.u53_words(rng, 20_000)])
    assert np.array_equal(H.u53_of(w), np.array([H.u53_exact(v) for v in w.tolist()]))
    assert H.u53_exact(2 ** 64 - 1) == 1.0 and H.u53_exact(0) == 2.0 ** -54
    w = np.concatenate([np.array(H.U32_EDGE_WORDS, dtype=np.uint32), rng.integers(0, 2 ** 32, 20_000, dtype=np.uint64).astype(np.uint32)])
    assert np.array_equal(H.u32_of(w), np.array([H.u32_exact(v) for v in w.tolist()]))


def test_argument_sets_keep_their_sizes_and_domains():
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    x = H.rcp_arguments(np.random.default_rng(21))
    assert x.size == 4_000_000 and x.min() >= tiny and x.max() <= 2.0 ** 1020      # finite, normal, and so is 1/x
    assert x[:1_000_000].min() < 2.0 ** -1000 and x[:1_000_000].max() > 2.0 ** 1000
    assert x[1_000_000:2_000_000].min() < 1.1e-6 and x[1_000_000:2_000_000].max() > 1e300
    assert 2.0 - 0.293 <= x[2_000_000:3_000_000].min() and x[2_000_000:3_000_000].max() <= 2.415
    x = H.sqrt_arguments(np.random.default_rng(22))
    assert 3_000_000 <= x.size <= 10_000_000 and x.min() >= tiny and x.max() < huge
    assert np.count_nonzero(x < 2.0 ** -32) >= 2 ** 20 - 1                         # the radicands of u just below 1
    x = H.exp_arguments(np.random.default_rng(11))
    assert 6_000_000 <= x.size <= 10_000_000 and x.min() > -708.0 and x.max() < 709.0
    u, uc, rest = H.sin_arguments(np.random.default_rng(23))
    assert u.size == uc.size and 20_000_000 <= u.size + uc.size <= 20_100_000 and rest.size == 10_000_000
    for v in (u, uc):
        assert v.min() > 0.0 and v.max() < 1.0 and np.array_equal(v * 2.0 ** 33 % 2, np.ones(v.size))   # (w + 1/2) 2^-32
    assert np.array_equal(1.0 - u, uc)
    assert rest.min() > 0.0 and rest.max() == 1.0 and np.count_nonzero(rest == 1.0) <= 4098
    for c in (0.25, 0.5, 0.75):
        assert np.count_nonzero(np.abs(u - c) < 4097 * 2.0 ** -32) >= 8192
        assert np.count_nonzero(np.abs(rest - c) < 4097 * 2.0 ** -53) >= 8192
    a = H.normal_arguments(np.random.default_rng(24))
    assert a.shape == (5_000_000, 4)
    assert {tuple(r) for r in np.unique(a[:, :2], axis=0).tolist()} == {(m, s) for m in H.MEANS for s in H.STDEVS}
    assert a[:, 2].min() > 0.0 and a[:, 2].max() < 1.0 and a[:, 3].min() > 0.0 and a[:, 3].max() <= 1.0
    assert np.count_nonzero(a[:, 2] > 1.0 - 2.0 ** -32) >= 190_000 and np.count_nonzero(a[:, 2] < 2.0 ** -32) >= 190_000
