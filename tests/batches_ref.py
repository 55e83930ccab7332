"""Long-double references and tolerances of the batched posterior accumulators (dangx_moments_batches*, dangx_chains_batches_*),
shared by test_moments_batches_cpu.py and test_gpu_moments_batches.py.  No device, no library: numpy and tests/chains_ref.py, whose
functions and bounds everything here is built on -- no constant of its own.

x is a chain's samples [n][...]; L, nfull, partial the batch state after n samples (replay); `first` leading batches discarded,
B' = nfull - first.
    mean, std    cr.pooled([x[first L:]], ddof)
    split R-hat  cr.between([half A, half B])["rhat2"] on the last 2 (B' // 2) full batches (several chains: the 2K halves in chain
                 order); the device value is compared squared (cr.compare_rhat)
    MCSE^2       B / B' with B the "B" formula of cr.between on the list of full batches (the variance of the batch means), tolerance
                 that function's tolB / B', e = 16 L eps big
    ESS          var / MCSE^2, var = M_f / (B'L - 1); through the quotient tol_var / MCSE^2 + var tol_MCSE2 / MCSE^4 + 4 eps ESS with
                 tol_var = 2 std tol_std + tol_std^2 from cr.pooled."""
import numpy as np

import chains_ref as cr

EPS, LD = cr.EPS, cr.LD
STATS = ("mean", "std", "mcse", "ess_bm", "split_rhat")


def replay(n, nbatch, L0):
    """(L, nfull, partial) after n accumulations: all batches full -> merged before the next sample, L doubles"""
    L = L0
    for c in range(n):
        if c // L == nbatch:
            L *= 2
    return L, n // L, n % L


def host_batches(x, nbatch, L0):
    """the accumulate / merge scheme in long double: (L, [(mean, m2) per slot]) -- what raw() holds, up to rounding"""
    L, n = L0, len(x)
    slots = [None] * nbatch
    for c in range(n):
        if c // L == nbatch:
            slots = [np.concatenate([slots[2 * i], slots[2 * i + 1]]) for i in range(nbatch // 2)] + [None] * (nbatch // 2)
            L *= 2
        b = c // L
        slots[b] = x[c:c + 1] if slots[b] is None else np.concatenate([slots[b], x[c:c + 1]])
    return L, slots


def needs(stat, L, nfull, partial, first, ddof=0):
    """whether the read-out is defined (the library refuses it otherwise)"""
    B = nfull - first
    if not 0 <= first <= nfull:
        return False
    if stat in ("mean", "std"):
        N = B * L + partial
        return N >= 1 and (stat == "mean" or 0 <= ddof < N)
    if B < 2:
        return False
    return stat != "split_rhat" or (B // 2) * L >= 2


def halves(x, L, nfull, first):
    h = (nfull - first) // 2
    return [x[(nfull - 2 * h) * L:(nfull - h) * L], x[(nfull - h) * L:nfull * L]]


def _full_batches(x, L, nfull, first):
    return [x[b * L:(b + 1) * L] for b in range(first, nfull)]


def _B(batches):
    """cr.between's "B" and its tolerance on a list of equal-length stacks (any length >= 1: between itself asks for n >= 2
    because of W, which is not wanted here)"""
    K, n = len(batches), len(batches[0])
    mom = [cr._two_pass(b) for b in batches]
    means = np.stack([m[0] for m in mom])
    big = np.stack([m[3] for m in mom]).max(axis=0)
    d = means - means[0]
    B = ((d - d.mean(axis=0)) ** 2).sum(axis=0) / (K - 1)
    e = 16 * n * EPS * big
    D = np.abs(d).max(axis=0)
    return B, (2 * D * e + e * e) * K / (K - 1) + 1e-300


def mcse2(x, L, nfull, first):
    Bp = nfull - first
    B, tolB = _B(_full_batches(x, L, nfull, first))
    return B / Bp, tolB / Bp


def ess(x, L, nfull, first):
    m2ref, m2tol = mcse2(x, L, nfull, first)
    pm = cr.pooled([x[first * L:nfull * L]], 1)
    std, tol_std = pm["std"]
    var, tol_var = std * std, 2 * std * tol_std + tol_std * tol_std
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = var / m2ref
        tol = tol_var / m2ref + var * m2tol / (m2ref * m2ref) + 4 * EPS * ref
    return ref, tol


def check(get, x, L, nfull, partial, first, ddof, what, chains=None):
    """get(stat) -> device values over the trailing shape of x; every stat that is defined against its reference.  chains: the
    samples of all chains (get then reads over them) -- mean / std pooled, R-hat over the 2K halves, MCSE and ESS combined."""
    xs = [x] if chains is None else list(chains)
    K = len(xs)
    done = []
    for stat in STATS:
        if not needs(stat, L, nfull, partial, first, ddof if K == 1 else 0):
            continue
        dev = np.asarray(get(stat))
        name = "%s %s first %d ddof %d" % (what, stat, first, ddof)
        if stat in ("mean", "std"):
            ref, tol = cr.pooled([c[first * L:] for c in xs], ddof if stat == "std" else 0)[stat]
            cr.compare(dev, ref, tol, name)
        elif stat == "mcse":
            parts = [mcse2(c, L, nfull, first) for c in xs]
            ref, tol = sum(p[0] for p in parts) / (K * K), sum(p[1] for p in parts) / (K * K)
            cr.compare(dev.astype(LD) ** 2, ref, tol, name + " (squared)")
        elif stat == "ess_bm":
            parts = [ess(c, L, nfull, first) for c in xs]
            cr.compare(dev, sum(p[0] for p in parts), sum(p[1] for p in parts), name)
        else:
            hs = [h for c in xs for h in halves(c, L, nfull, first)]
            cr.compare_rhat(dev, cr.between(hs), name)
        done.append(stat)
    return done
