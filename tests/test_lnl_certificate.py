"""The certified cheap likelihood of the register chains (dang_amd/csrc/dx_chain.h: RegChain::lnl_cheap, cheap_bound and
mh_certain), emulated on the CPU.

A proposal's lnL = -A/2, A = sum over bands and planes of (D - a' s)^2.  The kernels evaluate A~ with the SED from v_exp_f32
(and v_rcp_f32 for the Planck denominator), carry a bound |lnL - lnL~| <= wA A~ + wG, and decide a step from the interval of
the diff only where every value in it decides alike.  This checks, over 1e7 (pixel, proposal) cases per SED form with the fp32
instructions modelled at +-2 ulp, that the bound covers the exact likelihood (evaluated in extended precision: any fp64
evaluation within 2^-46 of it is covered too) and that every decided step is the exact decision.  Cases: signal to noise up to
1e5, tiny and huge amplitudes, temperatures at the prior bounds, diffs clustered at the accept threshold."""
import numpy as np

LOG2E = np.log2(np.e)
H_OVER_K = 0.04799243073366221    # h / k_B in K / GHz: x = h nu / (k T) with nu in GHz
NB = 10
NU = np.array([20.0 * (857.0 / 20.0) ** (j / (NB - 1)) for j in range(NB)])
UP, DOWN = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 - 2.0 ** -12)


def f32_op(x, wobble):
    """A float32 instruction result moved by `wobble` ulps (the instructions are specified to 1 ulp; modelled at 2)."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isfinite(x), x * np.float32(1.0 + wobble * 2.0 ** -23), x).astype(np.float32)


def exp2f(y, wobble):
    with np.errstate(over="ignore", under="ignore"):
        return f32_op(np.exp2(y.astype(np.float64)).astype(np.float32), wobble)


def sed_setup(mode, rng, n):
    """(k1 per band, lo, hi, F per band and case, nu_ref) of one chain type with its prior bounds."""
    if mode == "pow":
        lo, hi, ref = -4.1, -2.1, 30.0
        return np.log(NU / ref), lo, hi, np.ones((n, NB)), ref
    if mode == "beta":
        lo, hi, ref = 0.6, 2.6, 353.0
        T = rng.uniform(4.6, 34.6, (n, 1))
        z = H_OVER_K / T
        F = np.expm1(z * ref) / np.expm1(z * NU)
        return np.log(NU / ref), lo, hi, F, ref
    lo, hi, ref = 4.6, 34.6, 353.0
    beta = rng.uniform(0.6, 2.6, (n, 1))
    return NU.copy(), lo, hi, (NU / ref) ** (beta + 1.0), ref


def sed_exact(mode, th, k1, F, ref):
    th = th.astype(np.longdouble)[:, None]
    if mode == "pow":
        return np.exp(th * k1.astype(np.longdouble))
    if mode == "beta":
        return F.astype(np.longdouble) * np.exp((th + 1) * k1.astype(np.longdouble))
    z = H_OVER_K / th
    return np.expm1(z * ref) / np.expm1(z * k1.astype(np.longdouble)) * F.astype(np.longdouble)


def sed_cheap(mode, th, k1, F, ref, wob):
    if mode == "pow":
        s0 = th
    elif mode == "beta":
        s0 = th + 1.0
    else:
        s0 = H_OVER_K / th
    y = ((s0 * LOG2E)[:, None] * k1[None, :]).astype(np.float32)
    e = exp2f(y, wob)
    if mode == "pow":
        return e.astype(np.float64)
    if mode == "beta":
        return F * e.astype(np.float64)
    s1 = np.expm1(s0 * ref)[:, None]
    with np.errstate(divide="ignore"):
        r = f32_op(np.float32(1.0) / (e - np.float32(1.0)), -wob)
    return (s1 * F) * r.astype(np.float64)


def cheap_bound(mode, k1, lo, hi, D, a_start):
    """wA, wG as RegChain::cheap_bound forms them (D: (n, SP, NB))."""
    k = np.abs(k1)
    if mode == "mbb_t":
        zmax, zmin = H_OVER_K / lo, H_OVER_K / hi
        e = (1.0 + zmax * k) * 2.0 ** -24 + (2.0 + 1.0 / (zmin * k)) * 2.0 ** -22
    else:
        smax = max(abs(lo), abs(hi)) if mode == "pow" else max(abs(lo + 1), abs(hi + 1))
        e = (smax * k) * 2.0 ** -24 + 2.0 ** -22
    e = e * (1.0 + 2.0 ** -8) + 2.0 ** -46
    G = ((e[None, None, :] * D) ** 2).sum(axis=(1, 2))
    emax = e.max()
    lam = np.maximum(np.sqrt(G / np.maximum(a_start, 2.0 ** -900)), 2.0 ** -400)
    wA = 0.5 * ((2.0 * emax * (1.0 + emax) + lam) * (1.0 + 2.0 ** -40) + 2.0 ** -40)
    wG = 0.5 * ((G / lam + 2.0 * G) * (1.0 + 2.0 ** -40) + 2.0 ** -1000)
    return wA, wG


def mh_certain(dlo, dhi, u3, wob):
    with np.errstate(over="ignore", invalid="ignore"):
        uf = u3.astype(np.float32)
        elo = exp2f(dlo.astype(np.float32) * np.float32(LOG2E), wob)
        ehi = exp2f(dhi.astype(np.float32) * np.float32(LOG2E), -wob)
        acc = (dlo >= 0.0) | (elo > uf * UP)
        return acc | ((dhi < 0.0) & (ehi < uf * DOWN)), acc


def one_chunk(mode, rng, n, wob):
    sp = rng.integers(1, 3)
    k1, lo, hi, F, ref = sed_setup(mode, rng, n)
    snr = 10.0 ** rng.uniform(-3, 5, (n, 1, 1))                 # |a s / sigma| from 1e-3 to 1e5
    amp = snr * rng.choice([-1.0, 1.0], (n, sp, 1)) * rng.uniform(0.5, 1.5, (n, sp, NB))
    cur = rng.uniform(lo, hi, n)
    edge = rng.uniform(size=n) < 0.1                            # proposals at the prior bounds
    prop = np.where(edge, np.where(rng.uniform(size=n) < 0.5, lo, hi), np.clip(cur + rng.normal(0, 0.05 * (hi - lo), n), lo, hi))
    s_cur = sed_exact(mode if mode != "mbb_t" else "mbb_t", cur, k1, F, ref)
    D = (amp * s_cur[:, None, :].astype(np.float64) + rng.standard_normal((n, sp, NB))).astype(np.float64)
    A_cur = ((D.astype(np.longdouble) - amp * s_cur[:, None, :]) ** 2).sum(axis=(1, 2))
    wA, wG = cheap_bound(mode, k1, lo, hi, D, A_cur.astype(np.float64))
    s_t = sed_exact(mode, prop, k1, F, ref)
    A_true = ((D.astype(np.longdouble) - amp * s_t[:, None, :]) ** 2).sum(axis=(1, 2))
    s_c = sed_cheap(mode, prop, k1, F, ref, wob)
    with np.errstate(over="ignore", invalid="ignore"):
        r = D - amp * s_c[:, None, :]
        A_c = (r * r).sum(axis=(1, 2))
    w = wA * A_c + wG
    ok = np.isfinite(w)
    # the bound covers the exact likelihood
    err = np.abs(0.5 * (A_true - A_c.astype(np.longdouble)))
    assert np.all(err[ok] <= w[ok].astype(np.longdouble)), (mode, float((err[ok] / w[ok]).max()))
    # decisions: thresholds clustered at the diff (the interval's width and 2^-40 of it), and far
    lnl_old = -0.5 * A_cur
    diff_true = (-0.5 * A_true) - lnl_old
    kind = rng.integers(0, 3, n)
    t = np.where(kind == 0, diff_true + rng.uniform(-3, 3, n) * w, np.where(kind == 1, diff_true * (1 + rng.uniform(-1e-12, 1e-12, n)),
                 diff_true - rng.exponential(3.0, n))).astype(np.float64)
    t = np.minimum(t, -2.0 ** -33)
    u3 = np.clip(np.exp(t), 2.0 ** -33, 1 - 2.0 ** -33)
    truth = (diff_true >= 0) | (np.exp(diff_true) > u3.astype(np.longdouble))
    dc = (-0.5 * A_c) - lnl_old.astype(np.float64)
    W = w * (1.0 + 2.0 ** -40) + 2.0 ** -49 * (np.abs(0.5 * A_c) + np.abs(lnl_old.astype(np.float64)))
    decided, acc = mh_certain(dc - W, dc + W, u3, wob)
    assert np.array_equal(acc[decided], truth[decided]), mode
    rel = np.abs(np.exp(diff_true) / u3.astype(np.longdouble) - 1)
    assert np.all((rel[decided] > 2.0 ** -40) | (diff_true[decided] >= 0))
    return int(decided.sum()), n


def test_cheap_likelihood_decides_as_the_exact_chain():
    rng = np.random.default_rng(2026)
    for mode in ("pow", "beta", "mbb_t"):
        dec = tot = 0
        for c in range(20):
            d, n = one_chunk(mode, rng, 500_000, (-2.0, 0.0, 2.0)[c % 3])
            dec += d
            tot += n
        assert tot >= 10_000_000
        print("%s: decided by the certificate %d of %d" % (mode, dec, tot))
        assert 0 < dec < tot


def test_non_finite_cheap_values_decide_nothing():
    u3 = np.full(4, 0.5)
    dlo = np.array([np.nan, -np.inf, -np.inf, np.nan])
    dhi = np.array([np.nan, np.nan, np.inf, 1.0])
    decided, _ = mh_certain(dlo, dhi, u3, 0.0)
    assert not decided.any()
