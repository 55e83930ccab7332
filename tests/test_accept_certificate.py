"""The Metropolis accept test's certificate (dang_amd/csrc/dx_chain.h: mh_accept), emulated on the CPU.

The kernels decide diff >= 0 or exp(diff) > u3 from e = v_exp_f32(float(diff) * float(log2e)) whenever e is more than 2^-12
away from u3 (relative), and run the full fp64 comparison otherwise.  This checks, over 1e8 (diff, u3) pairs clustered at the
threshold plus the far and special cases, that every decision the certificate takes is the full comparison's: v_exp_f32 is
modelled as the correctly rounded 2^t moved by two float ulps either way (the instruction is specified to 1 ulp), and the
reference is exp in extended precision, which any <= 1 ulp fp64 exp agrees with wherever the certificate decides."""
import numpy as np

LOG2E_F = np.float32(1.4426950408889634)
UP = np.float32(1.0 + 2.0 ** -12)
DOWN = np.float32(1.0 - 2.0 ** -12)


def certificate(diff, u3, wobble):
    """(decided, accept) as mh_accept computes them before the fallback; wobble scales e by (1 + wobble * 2^-22)."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = diff.astype(np.float32) * LOG2E_F
        e = np.exp2(t.astype(np.float64)).astype(np.float32)
        e = np.where(t < -126, np.float32(0), e)                           # denormal results flushed (or not: both tiny)
        e = (e.astype(np.float64) * (1.0 + wobble * 2.0 ** -22)).astype(np.float32)
        uf = u3.astype(np.float32)
        acc = (diff >= 0.0) | (e > uf * UP)
        decided = acc | (e < uf * DOWN)
    return decided, acc


def full(diff, u3):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ex = np.exp(diff.astype(np.longdouble))
        return (diff >= 0.0) | (ex > u3), np.abs(ex / u3.astype(np.longdouble) - 1)


def pairs(rng, n):
    u3 = (rng.integers(0, 2 ** 32, n).astype(np.float64) + 0.5) * 2.0 ** -32      # dx_rng.h: u32
    kind = rng.integers(0, 4, n)
    near = np.log(u3) * (1.0 + rng.uniform(-4e-4, 4e-4, n)) + rng.uniform(-4e-4, 4e-4, n)
    nearer = np.log(u3) + rng.uniform(-1e-7, 1e-7, n)
    wide = -rng.exponential(5.0, n)
    diff = np.where(kind == 0, near, np.where(kind == 1, nearer, np.where(kind == 2, wide, near * 0.999)))
    return diff, u3


def test_certificate_decides_as_the_full_comparison():
    rng = np.random.default_rng(2024)
    total, undecided = 0, 0
    for _ in range(10):
        diff, u3 = pairs(rng, 10_000_000)
        truth, rel = full(diff, u3)
        for wobble in (-2.0, 0.0, 2.0):
            decided, acc = certificate(diff, u3, wobble)
            assert np.array_equal(acc[decided], truth[decided])
            # where the certificate decides, exp(diff) is so far from u3 that no <= 1 ulp fp64 exp decides otherwise
            assert np.all((rel[decided] > 2.0 ** -40) | (diff[decided] >= 0))
            if wobble == 0.0:
                undecided += int((~decided).sum())
        total += diff.size
    assert total >= 100_000_000
    print("undecided by the certificate: %d of %d (clustered at the threshold)" % (undecided, total))
    assert 0 < undecided < total


def test_certificate_far_and_special_cases():
    u3 = np.array([2.0 ** -33, 0.5, 1.0 - 2.0 ** -33, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 1e-5, 1e-5])
    diff = np.array([-1e300, -800.0, -1e-20, 0.0, 1e300, np.inf, -np.inf, np.nan, -87.5, -110.0, -11.512925464970229, -2.0])
    truth, _ = full(diff, u3)
    for wobble in (-2.0, 0.0, 2.0):
        decided, acc = certificate(diff, u3, wobble)
        assert np.array_equal(acc[decided], truth[decided])
        assert not decided[7]                                   # NaN: the full comparison decides (reject)
        assert decided[[0, 1, 3, 4, 5, 6, 8, 9, 11]].all()
