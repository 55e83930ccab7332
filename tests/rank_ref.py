"""Reference and tolerance of the rank-normalised and the folded R-hat read from the histograms of several chains
(dangx_chains_hist_rank; definitions in dang_amd/csrc/dx_rank_host.h), shared by test_chains_rank_cpu.py and
test_gpu_chains_rank.py.  No device, no library: numpy and the standard library only.

From the integer counts [K][npix][nbins] the scores are formed in long double: p = (u' - 0.75) / (2S + 0.5) as an exact rational
rounded once to a double (what the definition's f64 quotient of two exact operands gives), then statistics.NormalDist().inv_cdf
on the tail p <= 1/2 -- within 3.9e-15 of Phi^-1 over [1e-11, 0.5] against a 40-digit evaluation -- and the sign by the side of the
tail.  Every chain is then EXPANDED to its series of scores (a bin's count times its score, bins ascending) and (ref, tol) of
R-hat^2 are those of chains_ref.between(xs, eta=ETA): the statistic of the binned trace, evaluated as for any other series.

ETA = the absolute error bound stated at dx_norm_ppf (1e-12) + 1e-14 for the reference's own scores: every score the code under
test saw may differ from the reference's by that much, which `between` carries into W and B/n.

The weighted update and the bound of `between`.  `between` allows 16 n eps big on a mean and 16 n eps (1 + big/s)^2 W >=
16 n eps big^2 on W (W / s^2 = n / (n - 1)), big = max |z|.  One weighted step of c samples has six roundings (d, c / n_k, the
fma of the mean, c d, z - mean, the fma of m2; c and n_k are integers below 2^53, exact).  The mean moves by d c / n_k with an
error of at most 3 eps big per step, and a chain takes at most min(n, nbins) <= n steps: within 16 n eps big.  The term added to
m2 is c d (z - mean); z - mean = d (1 - c / n_k) is a difference that CANCELS when the bin holds nearly all of the chain's
samples so far, with an absolute error of eps |mean| <= eps big whatever is left of it, so the step's absolute error is at most
c |d| (eps big) + 3 eps (c d (z - mean)) <= 2 c eps big^2 + 3 eps (the term).  Summed over a chain's steps (sum c = n):
2 n eps big^2 + 3 eps m2_k, and in W, divided by K (n - 1) and summed over K chains: about 2 eps big^2 + 3 eps W -- below the
16 n eps big^2 the bound already allows for every n >= 2.  So no term is added for the weighted pass; the n in the bound is
needed, though: the relative error of W does grow like n eps where one bin holds almost everything (the records of 2^32 - 1
samples of test_chains_rank_cpu.py show it).  With eta = 1e-12 the eta terms dominate the tolerance for small n.

A chain that cannot be expanded (2^32 - 1 samples) goes through the same formulas with the counts as weights (weighted=True):
the two are the same sums, which test_chains_rank_cpu.py checks on small records."""
import statistics
from fractions import Fraction

import numpy as np

import chains_ref as cr

LD = cr.LD
PPF_BOUND = 1e-12              # stated at dx_norm_ppf
ETA = PPF_BOUND + 1e-14
PPF_PMIN = 0.625 / (8 * (2 ** 32 - 1) + 0.25)
_INV = statistics.NormalDist().inv_cdf


def ppf_points(n=400):
    """n log-spaced p over dx_norm_ppf's domain [PPF_PMIN, 0.5], both ends included"""
    p = np.exp(np.linspace(np.log(PPF_PMIN), np.log(0.5), n))
    p[0], p[-1] = PPF_PMIN, 0.5
    return p


def ppf_ref(p):
    """-Phi^-1(p) >= 0 for p in (0, 1/2]"""
    return np.array([-_INV(float(v)) if v < 0.5 else 0.0 for v in np.atleast_1d(p)], dtype=LD)


def scores(C):
    """pooled counts [npix][nbins] -> scores [npix][nbins] in long double (NaN in an empty bin)"""
    C = np.asarray(C).astype(object)
    z = np.full(C.shape, np.nan, dtype=LD)
    for i, row in enumerate(C):
        S = int(sum(row))
        cum = 0
        for b, c in enumerate(row):
            c = int(c)
            if c == 0:
                continue
            u = 2 * cum + c + 1
            t = min(u, 2 * S + 2 - u)
            p = float(Fraction(4 * t - 3, 8 * S + 2))          # (t - 0.75) / (2S + 0.5), one rounding
            a = 0.0 if p == 0.5 else -_INV(p)                   # |z|
            z[i, b] = LD(-a if t == u else a)
            cum += c
    return z


def median_bin(C):
    """first bin with C[b] > 0 and cum[b] + C[b] >= S / 2 (integers below 2^53: the f64 comparison of the definition is exact)"""
    C = np.asarray(C).astype(object)
    m = np.zeros(len(C), dtype=int)
    for i, row in enumerate(C):
        S, cum = int(sum(row)), 0
        for b, c in enumerate(row):
            if c > 0 and 2 * (cum + int(c)) >= S:
                m[i] = b
                break
            cum += int(c)
    return m


def fold(counts):
    """counts [K][npix][nbins] -> f [K][npix][nbins]: f[k][i][e] = c[m - e] + c[m + e] around pixel i's pooled median bin m"""
    counts = np.asarray(counts).astype(np.int64)
    K, npix, nb = counts.shape
    m = median_bin(counts.sum(axis=0))
    f = np.zeros_like(counts)
    for i in range(npix):
        for e in range(nb):
            if m[i] + e < nb:
                f[:, i, e] += counts[:, i, m[i] + e]
            if e > 0 and m[i] - e >= 0:
                f[:, i, e] += counts[:, i, m[i] - e]
    return f


def _weighted_between(z, c, eta):
    """chains_ref.between's formulas for one pixel with the counts c [K][nbins] as weights of the scores z [nbins]"""
    K = len(c)
    n = int(c[0].sum())
    w = c.astype(LD)
    zz = np.where(c.sum(axis=0) > 0, z, LD(0))
    means = (w * zz).sum(axis=1) / n
    d0 = zz[None, :] - means[:, None]
    m2 = (w * d0 * d0).sum(axis=1)
    big = np.abs(zz).max()
    W = m2.sum() / (K * (n - 1))
    s = np.sqrt(m2.sum() / (K * n))
    d = means - means[0]
    B = ((d - d.mean()) ** 2).sum() / (K - 1)
    e = 16 * n * cr.EPS * big + 2 * eta
    D = np.abs(d).max()
    with np.errstate(invalid="ignore", divide="ignore"):
        tolW = 16 * n * cr.EPS * (1 + big / s) ** 2 * W + (2 * eta * np.sqrt(n * m2) + n * eta * eta).sum() / (K * (n - 1))
        tolB = (2 * D * e + e * e) * K / (K - 1)
        R2 = (LD(n - 1) / n * W + B) / W
        return R2, tolB / W + B * tolW / (W * W) + 4 * cr.EPS * R2


def _rhat2_of(counts, weighted):
    counts = np.asarray(counts).astype(np.int64)
    K, npix, nb = counts.shape
    z = scores(counts.sum(axis=0))
    n = counts.sum(axis=2)                                      # [K][npix]
    ok = (n == n[0]).all(axis=0) & (n[0] >= 2)
    ref = np.full(npix, np.nan, dtype=LD)
    tol = np.full(npix, np.nan, dtype=LD)
    if weighted:
        for i in np.nonzero(ok)[0]:
            ref[i], tol[i] = _weighted_between(z[i], counts[:, i], ETA)
        return ref, tol
    for nv in np.unique(n[0][ok]):                              # the pixels of one n together
        idx = np.nonzero(ok & (n[0] == nv))[0]
        xs = [np.stack([np.repeat(z[i], counts[k, i]) for i in idx], axis=1) for k in range(K)]
        r, t = cr.between(xs, eta=ETA)["rhat2"]
        ref[idx], tol[idx] = r, t
    return ref, tol


def rhat2(counts, stat, weighted=False):
    """(ref, tol) of R-hat^2 over the pixels of counts [K][npix][nbins]; stat 'bulk', 'folded' or 'max'.  NaN where the chains'
    totals differ or are below 2, or where no chain ever left one bin; +inf where W = 0 and the means differ.  The larger of
    two values moves by no more than the one of them that moved most: the tolerance of 'max' is the larger of the two."""
    if stat == "bulk":
        return _rhat2_of(counts, weighted)
    if stat == "folded":
        return _rhat2_of(fold(counts), weighted)
    (rb, tb), (rf, tf) = rhat2(counts, "bulk", weighted), rhat2(counts, "folded", weighted)
    with np.errstate(invalid="ignore"):
        ref = np.where(np.isnan(rb) | np.isnan(rf), LD(np.nan), np.maximum(rb, rf))
        return ref, np.fmax(tb, tf)


def compare(dev, counts, stat, what, min_finite=None, weighted=False):
    """the read-out `dev` (R-hat), squared, against the reference of the records `counts`; returns the reference R-hat^2"""
    ref, tol = rhat2(counts, stat, weighted)
    with np.errstate(over="ignore", invalid="ignore"):
        cr.compare(np.asarray(dev).astype(LD) ** 2, ref, tol, what, min_finite)
    return ref


def unpack(words, nbins, bits):
    """records [..][nbins * bits / 32] uint32 -> counts [..][nbins] (with 16 bits the even bin in the low half)"""
    w = np.asarray(words, dtype=np.uint32)
    if bits == 32:
        return w.astype(np.int64)
    out = np.empty(w.shape[:-1] + (nbins,), dtype=np.int64)
    out[..., 0::2] = w & 0xffff
    out[..., 1::2] = w >> 16
    return out


def pack(counts, bits):
    c = np.asarray(counts).astype(np.uint64)
    if bits == 32:
        return c.astype(np.uint32)
    return (c[..., 0::2] | (c[..., 1::2] << np.uint64(16))).astype(np.uint32)
