"""Posterior pair and lag-1 statistics accumulated on the device (dangx_moments_pairs): against a long-double two-pass evaluation
of the definitions on the same samples pulled to the host, at large offsets and sample counts, across shards and alignments, the
chain left as it is, the launch counts, the template rows and the error cases.

Definitions (include/dangx.h): with mean and m2 = sum (x_t - mean)^2 of the n samples of a pixel,
    rho1 = [sum_{t=2..n} (x_t - mean)(x_{t-1} - mean)] / m2,     ESS = n (1 - rho)/(1 + rho), rho = max(rho1, 0),
    cov = C / (n - ddof), C = sum (a_t - mean_a)(b_t - mean_b),   corr = C / sqrt(m2_a m2_b),
0/0 = NaN where a variance is zero.  Tolerances, with big = max|x| and s the standard deviation (ddof 0):
    rho1: 16 n eps (1 + big/s);  corr: 16 n eps (1 + big_a/s_a + big_b/s_b);  cov: the corr tolerance x s_a s_b n/(n - ddof);
    ESS: 2 n x the rho1 tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import dang_amd as da
from dang_amd import synth

from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GLOBAL = ("template", "monopole", "hi_fit")
LD = np.longdouble


def _engine(case):
    dpar, ddata, bands, comps, meta = case
    return da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)


def _snapshot(eng):
    out = {}
    for l, c in enumerate(eng.component_list):
        if c.type in GLOBAL:
            out[l] = (eng.get_template_amplitudes(l), None)
        else:
            out[l] = (eng.get_amplitude(l), eng.get_indices(l) if c.nindices else None)
    return out


def _planes(word, what):
    bits = (int(word) >> (0 if what == 0 else 3 + 3 * (what - 1))) & 7
    return [k for k in range(3) if (bits >> k) & 1]


def _series(samples, l, what):
    """[n][nmaps][npix] (template rows: [n][nmaps][nbands]) of (component, what) over the snapshots"""
    if what == 0:
        return np.stack([s[l][0] for s in samples])
    return np.stack([s[l][1][what - 1] for s in samples])


def _two_pass(xs):
    """mean-removed samples, m2, s and big of a stack [n][...] in long double"""
    x = xs.astype(LD)
    d = x - x.mean(axis=0)
    m2 = (d * d).sum(axis=0)
    return d, m2, np.sqrt(m2 / len(x)), np.abs(x).max(axis=0)


def _ref_lag(xs):
    n = len(xs)
    d, m2, s, big = _two_pass(xs)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = (d[1:] * d[:-1]).sum(axis=0) / m2
        r = np.where(rho < 0, LD(0), rho)
        ess = n * (1 - r) / (1 + r)
        tol = 16 * n * EPS * (1 + big / s)
    return rho, ess, tol


def _ref_pair(xa, xb, ddof):
    n = len(xa)
    da_, m2a, sa, biga = _two_pass(xa)
    db_, m2b, sb, bigb = _two_pass(xb)
    C = (da_ * db_).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = C / np.sqrt(m2a * m2b)
        tol = 16 * n * EPS * (1 + biga / sa + bigb / sb)
        cov = C / (n - ddof) if n - ddof > 0 else None
        tolc = tol * sa * sb * n / (n - ddof) if n - ddof > 0 else None
    return corr, tol, cov, tolc


def _compare(dev, ref, tol, what, min_finite=None):
    """NaN exactly where the reference has it; elsewhere within tol.  Prints the worst error / tolerance."""
    nan_ref = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan_ref), (what, "NaN positions differ", int(np.isnan(dev).sum()), int(nan_ref.sum()))
    if min_finite is not None:
        assert (~nan_ref).mean() >= min_finite, (what, "finite fraction of the reference", float((~nan_ref).mean()))
    ok = ~nan_ref
    if ok.any():
        err = np.abs(dev.astype(LD)[ok] - ref[ok])
        worst = float((err / tol[ok]).max())
        print("%-44s worst error / tolerance %.3g" % (what, worst))
        assert (err <= tol[ok]).all(), (what, worst)


def _check_second_order(eng, sel, pairs, samples, min_finite=None, ddofs=(0, 1)):
    n = len(samples)
    assert eng.moments_count() == n
    rhos = {}
    for l, c in enumerate(eng.component_list):
        for what in range(1 + c.nindices):
            ks = _planes(sel[l], what)
            if not ks:
                continue
            rho, ess, tol = _ref_lag(_series(samples, l, what))
            if what == 0 and c.type in GLOBAL:
                dev_r, dev_e = eng.moments_get_template(l, "rho1"), eng.moments_get_template(l, "ess")
            else:
                dev_r, dev_e = eng.moments_get(l, what, "rho1"), eng.moments_get(l, what, "ess", ddof=5)   # ddof is ignored
            for k in ks:
                glob = what == 0 and c.type in GLOBAL
                _compare(dev_r[k], rho[k], tol[k], "rho1 %s what %d plane %d" % (c.label, what, k), None if glob else min_finite)
                _compare(dev_e[k], ess[k], 2 * n * tol[k], "ess  %s what %d plane %d" % (c.label, what, k))
                rhos[(l, what, k)] = dev_r[k]
    for p, (a, b) in enumerate(pairs):
        xa, xb = _series(samples, a[0], a[1])[:, a[2]], _series(samples, b[0], b[1])[:, b[2]]
        for ddof in ddofs:
            corr, tol, cov, tolc = _ref_pair(xa, xb, ddof)
            if ddof == ddofs[0]:
                _compare(eng.moments_get_pair(p, "corr"), corr, tol, "corr pair %d %s %s" % (p, a, b), min_finite)
            if cov is not None:
                dev = eng.moments_get_pair(p, "cov", ddof)
                assert not np.isnan(dev).any()
                err = np.abs(dev.astype(LD) - cov)
                fin = np.isfinite(tolc)                       # a variance of zero: the covariance is exactly 0
                assert (dev[~fin] == 0).all() and (cov[~fin] == 0).all()
                assert (err[fin] <= tolc[fin] + 1e-300).all(), ("cov", p, ddof, float((err[fin] / (tolc[fin] + 1e-300)).max()))
    return rhos


def test_against_the_host(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    sel = da.moments_begin(dpar, ddata)
    pairs = da.moments_pairs(dpar, ddata)
    assert pairs == da.default_moment_pairs(dpar, comps, sel) and len(pairs) == 12
    samples = []
    for it in range(1, 10):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(_snapshot(eng))
    rhos = _check_second_order(eng, sel, pairs, samples, min_finite=0.75)
    # the chain really is autocorrelated (a rejected proposal repeats the sample): a white series would not test the lag state
    idx = [v[np.isfinite(v)] for (l, what, k), v in rhos.items() if what > 0]
    assert any(v.size and v.max() > 0.1 and v.std() > 0 for v in idx)
    pm = da.posterior_maps(ddata)
    assert all({"rho1", "ess"} <= set(e) for e in pm.values())
    ess = pm[("dust", "beta")]["ess"][0]
    assert np.nanmax(ess) <= 9.0 and np.nanmin(ess) > 0


def _ar1(rng, n, shape, offset, spread=3.0, coef=0.6, hold=0.5):
    """AR(1) series of the given spread about `offset`, about half of the steps held (x_t = x_{t-1}); pixel 0 never moves."""
    x = np.empty((n,) + shape)
    v = rng.standard_normal(shape) * spread
    x[0] = offset + v
    for t in range(1, n):
        new = coef * v + np.sqrt(1 - coef * coef) * spread * rng.standard_normal(shape)
        v = np.where(rng.random(shape) < hold, v, new)
        x[t] = offset + v
    x[..., 0] = x[0][..., 0]
    return x


OFFSETS = (0.0, -3.1, 1.0e6)


def _synthetic_states(comps, meta, n, seed):
    """{l: (amplitudes [n][3][npix], indices [n][nind][3][npix] or None)}: every offset meets every other in a default pair"""
    rng = np.random.default_rng(seed)
    out = {}
    for l, c in enumerate(comps):
        a = _ar1(rng, n, (3, meta["npix"]), OFFSETS[(l + 2) % 3])
        x = None
        if c.nindices:
            x = np.stack([_ar1(rng, n, (3, meta["npix"]), OFFSETS[(l + j) % 3]) for j in range(c.nindices)], axis=1)
        out[l] = (a, x)
    return out


def _feed(engines, bounds, comps, states, n):
    """the states, one accumulate each, into every engine list entry (whole sky: bounds None); returns the samples as snapshots"""
    samples = []
    for t in range(n):
        for l, c in enumerate(comps):
            a, x = states[l]
            for e, (b0, b1) in zip(engines, bounds):
                e.put_amplitude(l, np.ascontiguousarray(a[t][:, b0:b1]))
                if x is not None:
                    e.put_indices(l, np.ascontiguousarray(x[t][:, :, b0:b1]))
        for e in engines:
            e.moments_accumulate()
        samples.append({l: (states[l][0][t], states[l][1][t] if states[l][1] is not None else None) for l in states})
    return samples


@pytest.mark.parametrize("n", [64, 1, 2])
def test_large_offset_and_sample_count(built, n):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    eng.moments_begin(None)
    sel = eng._moment_sel
    pairs = da.moments_pairs(dpar, ddata, pairs=da.default_moment_pairs(dpar, comps, sel))
    assert len(pairs) == 24       # every plane selected: 3 each of synch and synch_P, 9 each of dust and dust_P
    states = _synthetic_states(comps, meta, n, seed=11)
    samples = _feed([eng], [(0, meta["npix"])], comps, states, n)
    rhos = _check_second_order(eng, sel, pairs, samples, ddofs=(0, 1))
    if n == 1:
        assert all(np.isnan(v).all() for v in rhos.values())
        assert all(np.isnan(eng.moments_get_pair(p, "corr")).all() and not eng.moments_get_pair(p, "cov").any() for p in range(len(pairs)))
    if n == 2:      # (x2 - m)(x1 - m) / ((x1 - m)^2 + (x2 - m)^2) = -1/2 wherever the two samples differ
        for (l, what, k), v in rhos.items():
            xs = _series(samples, l, what)[:, k]
            moved = xs[0] != xs[1]
            assert moved.any() and np.isnan(v[~moved]).all()
            tol = 16 * 2 * EPS * (1 + np.abs(xs).max(axis=0) / (np.abs(xs[1] - xs[0]) / 2 + 1e-300))
            assert (np.abs(v[moved] + 0.5) <= tol[moved]).all()
    if n == 64:     # pixel 0 never moved: 0/0
        assert all(np.isnan(v[0]) and np.isfinite(v[1:]).all() for v in rhos.values())


def _all_new(eng, npairs):
    out = {}
    sel = eng._moment_sel
    for l, c in enumerate(eng.component_list):
        for what in range(1 + c.nindices):
            if _planes(sel[l], what):
                for stat in ("rho1", "ess"):
                    out[(l, what, stat)] = eng.moments_get(l, what, stat)
    for p in range(npairs):
        out[(p, "corr")] = eng.moments_get_pair(p, "corr")
        out[(p, "cov")] = eng.moments_get_pair(p, "cov", 1)
    return out


def test_shards_and_determinism(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    whole, again = _engine(case), _engine(make_case("C2", nside=4))
    bounds = [0, 63, 130, meta["npix_global"]]        # odd lengths: planes (and the two planes of a pair) off the 16-byte grid
    shards = shard_engines(case, 3, bounds=bounds)
    for e in [whole, again] + shards:
        e.moments_begin(None)
    pairs = da.default_moment_pairs(dpar, comps, whole._moment_sel)
    for engs in ([whole], [again], shards):
        assert da.moments_pairs(dpar, ddata, pairs=pairs, engines=engs) == pairs
    n = 6
    states = _synthetic_states(comps, meta, n, seed=5)
    _feed([whole], [(0, meta["npix"])], comps, states, n)
    _feed([again], [(0, meta["npix"])], comps, states, n)
    _feed(shards, list(zip(bounds[:-1], bounds[1:])), comps, states, n)
    mw, ma = _all_new(whole, len(pairs)), _all_new(again, len(pairs))
    ms = [_all_new(e, len(pairs)) for e in shards]
    assert any(np.isfinite(v).any() for v in mw.values())
    for k, v in mw.items():
        assert np.array_equal(v, ma[k], equal_nan=True), ("two runs", k)
        assert np.array_equal(v, np.concatenate([m[k] for m in ms], axis=-1), equal_nan=True), ("shards", k)
    for stat, ddof in (("corr", 0), ("cov", 1)):
        pw = da.posterior_pair_maps(ddata, stat, ddof, engines=[whole])
        ps = da.posterior_pair_maps(ddata, stat, ddof, engines=shards)
        assert list(pw) == list(ps) and len(pw) == len(pairs)
        for p, k in enumerate(pw):
            assert np.array_equal(pw[k], ps[k], equal_nan=True) and np.array_equal(pw[k], mw[(p, stat)], equal_nan=True)
    pw, ps = da.posterior_maps(ddata, engines=[whole]), da.posterior_maps(ddata, engines=shards)
    for k in pw:
        for stat in ("mean", "std", "rho1", "ess"):
            assert np.array_equal(pw[k][stat], ps[k][stat], equal_nan=True), (k, stat)


def test_adopted_buffers_moved_off_the_grid(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    assert eng._adopted
    sel = da.moments_begin(dpar, ddata)
    pairs = da.moments_pairs(dpar, ddata)
    samples = []
    for it in range(1, 5):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(_snapshot(eng))
    # the dust_P maps move to new caller buffers, one double off the 16-byte grid: accumulation follows them
    ld = [c.label for c in comps].index("dust_P")
    npix, nmaps = meta["npix"], meta["nmaps"]
    amp_old, idx_old = eng._adopted[ld]
    abuf = torch.empty(nmaps * npix + 1, dtype=torch.float64, device=dev)
    ibuf = torch.empty(2 * nmaps * npix + 1, dtype=torch.float64, device=dev)
    amp_new, idx_new = abuf[1:].view(nmaps, npix), ibuf[1:].view(2, nmaps, npix)
    amp_new.copy_(amp_old)
    idx_new.copy_(idx_old)
    torch.cuda.synchronize()
    eng._chk(eng.lib.dangx_adopt_device_state(eng.h, ld, ctypes.c_void_p(amp_new.data_ptr()), ctypes.c_void_p(idx_new.data_ptr())))
    eng._adopted[ld] = (amp_new, idx_new)
    comps[ld].amplitude, comps[ld].indices = amp_new, idx_new
    for it in range(5, 9):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(_snapshot(eng))
    assert not torch.equal(idx_new, idx_old)
    _check_second_order(eng, sel, pairs, samples)
    for p in range(len(pairs)):
        for stat, ddof in (("corr", 0), ("cov", 0), ("cov", 1)):
            h = eng.moments_get_pair(p, stat, ddof)
            d = eng.moments_get_pair(p, stat, ddof, device=True)
            assert d.is_cuda and np.array_equal(d.cpu().numpy(), h, equal_nan=True), (p, stat, ddof)
    for l, c in enumerate(comps):
        for what in range(1 + c.nindices):
            if _planes(sel[l], what):
                for stat in ("rho1", "ess"):
                    h = eng.moments_get(l, what, stat)
                    d = eng.moments_get(l, what, stat, device=True)
                    assert np.array_equal(d.cpu().numpy(), h, equal_nan=True), (c.label, what, stat)


def _run(nit, second_order):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    da.moments_begin(dpar, ddata)
    if second_order:
        da.moments_pairs(dpar, ddata)
    for it in range(1, nit + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    return eng, _snapshot(eng), ddata.chisq, da.posterior_maps(ddata)


def test_nothing_else_moves(built):
    e1, s1, chi1, p1 = _run(5, True)
    e2, s2, chi2, p2 = _run(5, False)
    assert chi1 == chi2
    for l in s1:
        assert np.array_equal(s1[l][0], s2[l][0])
        if s1[l][1] is not None:
            assert np.array_equal(s1[l][1], s2[l][1])
    assert p1.keys() == p2.keys()
    for k in p2:
        assert set(p2[k]) == {"n", "mean", "std"} and set(p1[k]) == {"n", "mean", "std", "rho1", "ess"}
        assert np.array_equal(p1[k]["mean"], p2[k]["mean"]) and np.array_equal(p1[k]["std"], p2[k]["std"])


@pytest.mark.parametrize("with_pairs,launches", [(False, 3), (True, 6)])
def test_profile_family(built, with_pairs, launches):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    eng.profile(True)
    da.moments_begin(dpar, ddata)
    da.moments_pairs(dpar, ddata, pairs=None if with_pairs else [], lag1=True)
    for it in (1, 2, 3):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    prof = eng.profile_get()
    assert prof["k_moments"]["launches"] == launches and prof["k_moments"]["total_ms"] > 0


def test_template_amplitudes(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 3, 4), amplitudes=(3.0, -2.0, 5.0))
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    sel = da.moments_begin(dpar, ddata)
    lt, lm = len(comps) - 2, len(comps) - 1
    with pytest.raises(da.DangxError, match="template"):
        eng.moments_pairs([((lt, 0, 1), (1, 0, 0))])
    pairs = da.moments_pairs(dpar, ddata)
    assert all(a[0] < lt and b[0] < lt for a, b in pairs)
    samples = []
    for it in range(1, 10):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(_snapshot(eng))
    assert np.std(np.stack([s[lt][0] for s in samples]), axis=0)[1].max() > 0
    rhos = _check_second_order(eng, sel, pairs, samples)
    assert np.isfinite(rhos[(lt, 0, 1)][[2, 3, 4]]).all() and np.isfinite(rhos[(lm, 0, 0)][[0, 3, 4]]).all()   # the fitted bands
    ta = eng.moments_get_template(lm, "rho1", out=np.full((3, meta["nbands"]), 7.0))
    assert (ta[1:] == 7.0).all()


def test_errors(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    good = [((1, 0, 0), (1, 1, 0))]
    with pytest.raises(da.DangxError, match="begin"):
        eng.moments_pairs(good)
    ld = [c.label for c in comps].index("dust_P")
    sel = np.zeros(len(comps), dtype=np.int32)
    sel[1] = 1 | (1 << 3)                              # synch: amplitude and beta on T
    sel[ld] = (1 << 1) | (1 << (3 + 1))                # dust_P: amplitude and beta on Q
    eng.moments_begin(sel)
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="before the first"):
        eng.moments_pairs(good)
    with pytest.raises(da.DangxError, match="not tracked"):
        eng.moments_get(1, 0, "rho1")
    eng.moments_begin(sel)
    eng.moments_pairs(good + [((ld, 0, 1), (ld, 1, 1))], lag1=True)
    with pytest.raises(da.DangxError, match="not selected"):
        eng.moments_pairs([((1, 0, 0), (ld, 0, 2))])
    with pytest.raises(da.DangxError, match="a == b"):
        eng.moments_pairs([((1, 1, 0), (1, 1, 0))])
    with pytest.raises(da.DangxError, match="DANGX_MAX_PAIRS"):
        eng.moments_pairs(good * 65)
    with pytest.raises(da.DangxError, match="what"):
        eng.moments_pairs([((1, 0, 0), (1, 2, 0))])    # the synchrotron has one index
    # after the failures the earlier registration still works
    assert len(eng._moment_pairs) == 2
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="ddof"):
        eng.moments_get_pair(0, "cov", ddof=1)         # n = 1
    assert not eng.moments_get_pair(1, "cov").any() and np.isnan(eng.moments_get(1, 1, "rho1")[0]).all()
    eng.moments_accumulate()
    assert eng.moments_get_pair(1, "cov", ddof=1).shape == (meta["npix"],)
    with pytest.raises(da.DangxError, match="pair index out of range"):
        eng.moments_get_pair(2, "corr")
    with pytest.raises(da.DangxError, match="pair index out of range"):
        eng.moments_get_pair(-1, "corr")
    with pytest.raises(da.DangxError, match="stat"):
        eng.moments_get_pair(0, 2)
    # a second registration replaces the first; begin drops everything
    eng.moments_begin(sel)
    eng.moments_pairs(good, lag1=False)
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="not tracked"):
        eng.moments_get(1, 0, "ess")
    with pytest.raises(da.DangxError, match="pair index out of range"):
        eng.moments_get_pair(1, "corr")
    eng.moments_begin(sel)
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="pair index out of range"):
        eng.moments_get_pair(0, "corr")
