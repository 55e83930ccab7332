"""The accept test's margin of 2^-16 and the accept uniform formed as a float from its Philox word (dang_amd/csrc/dx_chain.h:
mh_accept, mh_certain, u32f), emulated on the CPU with the pieces of tests/test_accept_certificate.py and
tests/test_lnl_certificate.py.

The kernels compare e = v_exp_f32(float(diff) * float(log2e)) with uf (1 +- 2^-16), uf = float(u32(w)) or, with
-DDX_ACCEPT_WORD, fmaf(float(w), 2^-32, 2^-33), and run
the full fp64 comparison exp(diff) > u32(w) where neither bound decides.  Over 1e8 (diff, word) pairs clustered within a few
margins of the threshold (and the words 0 and 2^32 - 1), with v_exp_f32 moved by two float ulps either way, every decision the
cheap test takes must be the full comparison's, and the interval form must never decide against it."""
import numpy as np

import test_accept_certificate as AC
import test_lnl_certificate as LC

MARGIN = 2.0 ** -16
UP, DOWN = np.float32(1.0 + MARGIN), np.float32(1.0 - MARGIN)
CHUNK = 10_000_000


def test_margin_constants_are_the_kernels():
    assert float(UP) == float.fromhex("0x1.0001p+0") and float(DOWN) == float.fromhex("0x1.fffep-1")


def u32f(w):
    """fmaf(float(w), 2^-32, 2^-33): the product and the sum are exact in double (34 bits at most), so one rounding to float"""
    return (w.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def exp2f(diff):
    """v_exp_f32(float(diff) * float(log2e)), correctly rounded; moved(e, wobble) is that result `wobble` float ulps away
    (tests/test_lnl_certificate.py: f32_op)"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = diff.astype(np.float32) * AC.LOG2E_F
        e = LC.exp2f(t, 0.0)
        return np.where(t < -126, np.float32(0), e)            # denormal results flushed (or not: both tiny)


def moved(e, wobble):
    return LC.f32_op(e, wobble)


def certificate(diff, e, uf, wobble):
    """(decided, accept) of mh_accept(diff, word) before its exact branch; e = exp2f(diff), uf = u32f(word)"""
    with np.errstate(invalid="ignore"):
        ew = moved(e, wobble)
        acc = (diff >= 0.0) | (ew > uf * UP)
        return acc | (ew < uf * DOWN), acc


def certain(dlo, dhi, elo, ehi, uf, wobble):
    """(decided, accept) of mh_certain(dlo, dhi, word): the lower end's exp moved up and the upper end's down, and the reverse"""
    with np.errstate(invalid="ignore"):
        acc = (dlo >= 0.0) | (moved(elo, wobble) > uf * UP)
        return acc | ((dhi < 0.0) & (moved(ehi, -wobble) < uf * DOWN)), acc


def pairs(rng, n):
    w = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    w[:n // 50] = 0                                              # u3 = 2^-33
    w[n // 50:n // 25] = 2 ** 32 - 1                             # u3 = 1 - 2^-33
    w[n // 25:n // 20] = rng.integers(0, 2 ** 12, n // 20 - n // 25).astype(np.uint32)        # the smallest uniforms
    w[n // 20:n // 16] = rng.integers(2 ** 24, 2 ** 25, n // 16 - n // 20).astype(np.uint32)  # float(w) begins to round
    u3 = (w.astype(np.float64) + 0.5) * 2.0 ** -32               # dx_rng.h: u32
    lu = np.log(u3)
    kind = rng.integers(0, 4, n)
    near = lu + rng.uniform(-4.0, 4.0, n) * MARGIN               # within a few margins
    nearer = lu + rng.uniform(-1.5, 1.5, n) * MARGIN             # ... mostly inside the undecided band's edges
    at = lu + rng.uniform(-1e-7, 1e-7, n)
    rel = lu * (1.0 + rng.uniform(-2.0, 2.0, n) * MARGIN)
    return np.where(kind == 0, near, np.where(kind == 1, nearer, np.where(kind == 2, at, rel))), w, u3


def test_cheap_decisions_are_the_full_comparisons():
    rng = np.random.default_rng(2027)
    total = undecided = undecided12 = 0
    for _ in range(10):
        diff, w, u3 = pairs(rng, CHUNK)
        truth, rel = AC.full(diff, u3)
        e = exp2f(diff)
        # the interval form: d lies in [dlo, dhi], widths from 0 to a few margins
        wl = rng.uniform(0.0, 3.0, CHUNK) * MARGIN * (rng.uniform(size=CHUNK) < 0.8)
        wh = rng.uniform(0.0, 3.0, CHUNK) * MARGIN * (rng.uniform(size=CHUNK) < 0.8)
        dlo, dhi = diff - wl, diff + wh
        elo, ehi = exp2f(dlo), exp2f(dhi)
        # both float forms of the uniform: from the word (-DDX_ACCEPT_WORD) and float(u32(w)) (the default)
        for form, uf in enumerate((u32f(w), u3.astype(np.float32))):
            for wobble in (-2.0, 0.0, 2.0):
                decided, acc = certificate(diff, e, uf, wobble)
                assert np.array_equal(acc[decided], truth[decided])
                # where it decides, exp(diff) is so far from u3 that no <= 1 ulp fp64 exp decides otherwise
                assert np.all((rel[decided] > 2.0 ** -40) | (diff[decided] >= 0))
                if wobble == 0.0 and form == 0:
                    undecided += int((~decided).sum())
                    d12, _ = AC.certificate(diff, u3, 0.0)
                    undecided12 += int((~d12).sum())
                decided, acc = certain(dlo, dhi, elo, ehi, uf, wobble)
                assert np.array_equal(acc[decided], truth[decided])
                assert np.all((rel[decided] > 2.0 ** -40) | (diff[decided] >= 0))
        total += diff.size
    assert total >= 100_000_000
    print("undecided: %d of %d at the margin 2^-16, %d at 2^-12 with float(u3)" % (undecided, total, undecided12))
    assert 0 < undecided < undecided12


def test_float_uniform_is_within_2_to_minus_23():
    rng = np.random.default_rng(7)
    w = np.concatenate([rng.integers(0, 2 ** 32, 20_000_000, dtype=np.uint64), np.arange(0, 2 ** 16, dtype=np.uint64),
                        2 ** 32 - 1 - np.arange(0, 2 ** 16, dtype=np.uint64), 2 ** 24 + np.arange(-64, 64, dtype=np.int64).astype(np.uint64)])
    w = w.astype(np.uint32)
    u3 = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    assert np.all(np.abs(u32f(w).astype(np.float64) - u3) <= 2.0 ** -23 * u3)
    assert u32f(np.array([0], dtype=np.uint32))[0] == np.float32(2.0 ** -33)


def test_far_and_special_cases():
    w = np.array([0, 2 ** 31, 2 ** 32 - 1, 2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30, 42949, 42949], dtype=np.uint32)
    u3 = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    diff = np.array([-1e300, -800.0, -1e-20, 0.0, 1e300, np.inf, -np.inf, np.nan, -87.5, -110.0, float(np.log(u3[10])), -2.0])
    truth, _ = AC.full(diff, u3)
    e, uf = exp2f(diff), u32f(w)
    for wobble in (-2.0, 0.0, 2.0):
        decided, acc = certificate(diff, e, uf, wobble)
        assert np.array_equal(acc[decided], truth[decided])
        assert not decided[7]                                   # NaN: the full comparison decides (reject)
        assert decided[[0, 1, 3, 4, 5, 6, 8, 9, 11]].all()
        decided, acc = certain(diff, diff, e, e, uf, wobble)
        assert np.array_equal(acc[decided], truth[decided])
        assert not decided[7]
