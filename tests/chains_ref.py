"""Long-double references and tolerances of the read-outs over several chains (dangx_chains_*), shared by test_chains_cpu.py and
test_gpu_chains.py.  No device, no library: numpy only.

Every function takes the chains' samples as a list of stacks xs[k] of shape [n_k][...] and returns (reference, tolerance) arrays
over the trailing shape.  With eps = 2^-52, N = sum n_k, big = max |x| over all samples and s the standard deviation (ddof 0):
    pooled mean   8 N eps big                     } the project's single-chain bounds (tests/test_gpu_moments*.py) with N for n:
    pooled std    16 N eps (s + big)              } the reference is the two-pass evaluation on the concatenated samples
    pooled corr   16 N eps (1 + big_a/s_a + big_b/s_b);   cov: that x s_a s_b N / (N - ddof)
    W             16 n eps (1 + big/s)^2 W,  s^2 = sum_k m2_k / (K n) the within-chain variance
    B/n           (2 D e + e^2) K / (K - 1),  e = 16 n eps big (twice the bound of a mean: d_k is a difference of two),  D = max |d_k|
    R-hat^2       tol_B / W + B tol_W / W^2 + 4 eps R^2  (the two above through the quotient; the last term is the rounding of the
                  fma, the division, the square root and of squaring the returned value: half an ulp each, doubled by the square)
    pooled ESS    2 n K x the largest rho1 tolerance 16 n eps (1 + big_k/s_k) of a chain (K terms of the single-chain ESS bound)."""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _two_pass(x):
    x = x.astype(LD)
    mean = x.mean(axis=0)
    d = x - mean
    m2 = (d * d).sum(axis=0)
    return mean, d, m2, np.abs(x).max(axis=0)


def pooled(xs, ddof=0):
    """{'mean': (ref, tol), 'std': (ref, tol)} of the concatenated samples"""
    x = np.concatenate(xs, axis=0)
    N = len(x)
    mean, d, m2, big = _two_pass(x)
    s = np.sqrt(m2 / N)
    return {"mean": (mean, 8 * N * EPS * big + 1e-300), "std": (np.sqrt(m2 / (N - ddof)), 16 * N * EPS * (s + big) + 1e-300)}


def pooled_pair(xa, xb, ddof=0):
    """{'corr': (ref, tol), 'cov': (ref, tol)} of the concatenated samples of two planes"""
    a, b = np.concatenate(xa, axis=0), np.concatenate(xb, axis=0)
    N = len(a)
    _, da_, m2a, biga = _two_pass(a)
    _, db_, m2b, bigb = _two_pass(b)
    sa, sb = np.sqrt(m2a / N), np.sqrt(m2b / N)
    C = (da_ * db_).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = C / np.sqrt(m2a * m2b)
        tol = 16 * N * EPS * (1 + biga / sa + bigb / sb)
        return {"corr": (corr, tol), "cov": (C / (N - ddof), tol * sa * sb * N / (N - ddof))}


def between(xs, eta=0.0):
    """{'W', 'B', 'rhat2', 'ess'}: (ref, tol) from the per-chain long-double moments; equal counts n >= 2.
    eta: every sample the device saw may differ from xs by up to eta (a signal restated on the host): a mean then moves by at most
    eta, a difference of means by 2 eta, and m2_k by at most 2 eta sqrt(n m2_k) + n eta^2 (Cauchy-Schwarz)."""
    K, n = len(xs), len(xs[0])
    assert all(len(x) == n for x in xs) and n >= 2
    mom = [_two_pass(x) for x in xs]
    means = np.stack([m[0] for m in mom])
    m2 = np.stack([m[2] for m in mom])
    big = np.stack([m[3] for m in mom]).max(axis=0)
    W = m2.sum(axis=0) / (K * (n - 1))
    s = np.sqrt(m2.sum(axis=0) / (K * n))
    d = means - means[0]
    B = ((d - d.mean(axis=0)) ** 2).sum(axis=0) / (K - 1)
    e = 16 * n * EPS * big + 2 * eta
    D = np.abs(d).max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        tolW = 16 * n * EPS * (1 + big / s) ** 2 * W + (2 * eta * np.sqrt(n * m2) + n * eta * eta).sum(axis=0) / (K * (n - 1))
        tolB = (2 * D * e + e * e) * K / (K - 1)
        R2 = (LD(n - 1) / n * W + B) / W
        tolR2 = tolB / W + B * tolW / (W * W) + 4 * EPS * R2
        ess = np.zeros_like(W)
        tolE = np.zeros_like(W)
        for x, (mean, dk, q, bk) in zip(xs, mom):
            rho = (dk[1:] * dk[:-1]).sum(axis=0) / q
            r = np.where(rho < 0, LD(0), rho)
            ess = ess + n * (1 - r) / (1 + r)
            tolE = np.maximum(tolE, 16 * n * EPS * (1 + bk / np.sqrt(q / n)))
        tolE = 2 * n * K * tolE
    return {"W": (W, tolW + 1e-300), "B": (B, tolB + 1e-300), "rhat2": (R2, tolR2), "ess": (ess, tolE)}


def compare(dev, ref, tol, what, min_finite=None):
    """NaN and +-inf exactly where the reference has them; elsewhere within tol.  Prints the worst error / tolerance."""
    dev = np.asarray(dev)
    ref = np.asarray(ref)
    tol = np.broadcast_to(np.asarray(tol), ref.shape)
    nan_ref, inf_ref = np.isnan(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(dev), nan_ref), (what, "NaN positions differ", int(np.isnan(dev).sum()), int(nan_ref.sum()))
    assert np.array_equal(np.isinf(dev), inf_ref) and (dev[inf_ref] == ref[inf_ref]).all(), (what, "infinities differ")
    if min_finite is not None:
        assert (~nan_ref).mean() >= min_finite, (what, "finite fraction of the reference", float((~nan_ref).mean()))
    ok = ~(nan_ref | inf_ref)
    if ok.any():
        err = np.abs(dev.astype(LD)[ok] - ref[ok])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = float(np.nanmax(np.where(err == 0, LD(0), err / tol[ok])))
        print("%-52s worst error / tolerance %.3g" % (what, worst))
        assert ((err <= tol[ok]) | (err == 0)).all(), (what, worst)


def compare_rhat(dev, between_ref, what, min_finite=None):
    """the device's R-hat, squared, against R-hat^2 of the reference"""
    dev = np.asarray(dev)
    with np.errstate(over="ignore", invalid="ignore"):
        compare(dev.astype(LD) ** 2, between_ref["rhat2"][0], between_ref["rhat2"][1], what, min_finite)
