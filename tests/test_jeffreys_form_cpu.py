"""The factorised Jeffreys sum of the register chains (dang_amd/csrc/dx_chain.h: RegChain::form_w / lnl, S = sum_j s_j^2 w_j with
w_j = ln(nu_j/nu_ref)^2 sum_k sigma_kj^-4) emulated in numpy, against the reference's operation order as the oracle states it
(oracle/dang_oracle.c:876-891: sum_k sum_j ((1/sigma)^2 (a s / a) ln(nu_j/nu_ref))^2).  Both take the same SED values s_j: the
test is about the factorisation, the order of the sums and the NaN rule.  No GPU."""
import numpy as np
import pytest

from dang_amd import synth

EPS = 2.0 ** -52
NPIX = 100000
NB = 10


def _case(nplanes, seed):
    rng = np.random.default_rng(seed)
    nu = np.array(synth.band_freqs_ghz(NB))
    _, nu_ref, asig, idx = synth.PHYS["synch"]
    mean, sig = idx[0][1], idx[0][2]
    lnr = np.log(nu / nu_ref)                                       # [NB]
    beta = rng.uniform(mean - 10 * sig, mean + 10 * sig, NPIX)      # over the uniform bounds of make_sky
    amp = asig * rng.standard_normal((nplanes, NPIX))
    amp[np.abs(amp) < 1e-3] = 1e-3
    s = np.exp(beta[None, :] * lnr[:, None])                        # [NB, NPIX]
    snr = 10.0 ** rng.uniform(0.0, 5.0, (nplanes, NB, NPIX))        # signal to noise 1 .. 1e5 per band and plane
    sigma = np.abs(amp)[:, None, :] * s[None] / snr
    return lnr, amp, s, sigma


def _reference(lnr, amp, s, sigma):
    """k outer, j inner, one running sum (oracle/dang_oracle.c:881-887)"""
    tot = np.zeros(s.shape[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(amp.shape[0]):
            for j in range(NB):
                ss = amp[k] * s[j]
                rr = 1.0 / sigma[k, j]
                t = (rr * rr) * (ss / amp[k]) * lnr[j]
                tot = tot + t * t
        return np.log(np.sqrt(tot))


def _kernel(lnr, amp, s, sigma):
    """form_w once per chain, then S = sum_j (s_j s_j) w_j in band order; a zero or non-finite amplitude makes every weight NaN"""
    bad = np.zeros(s.shape[1], dtype=bool)
    for k in range(amp.shape[0]):
        bad |= ~((np.abs(amp[k]) > 0.0) & (np.abs(amp[k]) < np.inf))
    S = np.zeros(s.shape[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(NB):
            q = np.zeros(s.shape[1])
            for k in range(amp.shape[0]):
                isr = 1.0 / sigma[k, j]
                t = isr * isr
                q = q + t * t
            w = np.where(bad, np.nan, (lnr[j] * lnr[j]) * q)
            S = S + (s[j] * s[j]) * w
        return np.log(np.sqrt(S))


@pytest.mark.parametrize("nplanes", [1, 2])
def test_factorised_sum_matches_the_reference_order(nplanes):
    lnr, amp, s, sigma = _case(nplanes, 20 + nplanes)
    ref, ker = _reference(lnr, amp, s, sigma), _kernel(lnr, amp, s, sigma)
    assert np.isfinite(ref).all() and np.isfinite(ker).all()
    d = np.abs(ker - ref).max()
    print("planes %d: max |log sqrt S_kernel - log sqrt S_ref| = %.2f eps (|log sqrt S| up to %.1f)" % (nplanes, d / EPS, np.abs(ref).max()))
    assert d <= 64 * EPS


@pytest.mark.parametrize("nplanes", [1, 2])
@pytest.mark.parametrize("value", [0.0, np.inf, -np.inf, np.nan])
def test_nan_rule(nplanes, value):
    """an amplitude of 0, +-inf or NaN on any swept plane: the reference's prior is NaN (0/0, inf/inf), and so is the kernel's
    form, whose amplitude has cancelled; every other pixel is untouched.  A NaN diff is never accepted."""
    lnr, amp, s, sigma = _case(nplanes, 7)
    lnr, amp, s, sigma = lnr, amp[:, :1000], s[:, :1000], sigma[:, :, :1000]
    clean = _kernel(lnr, amp, s, sigma)
    hit = np.arange(0, 1000, 97)
    amp = amp.copy()
    amp[nplanes - 1, hit] = value            # the last plane only: with two planes the first stays finite and non-zero
    ref, ker = _reference(lnr, amp, s, sigma), _kernel(lnr, amp, s, sigma)
    assert np.isnan(ref[hit]).all() and np.isnan(ker[hit]).all()
    rest = np.setdiff1d(np.arange(1000), hit)
    assert np.array_equal(ker[rest], clean[rest]) and np.isfinite(ref[rest]).all()
    diff = ker[hit] - clean[hit]             # lnl_new - lnl_old with a NaN prior on either side
    for u in (0.5, 2.0 ** -33):
        with np.errstate(invalid="ignore"):
            assert not ((diff >= 0.0) | (np.exp(diff) > u)).any()   # sample mode (mh_accept)
            assert not (diff > 0.0).any()                            # optimize mode
