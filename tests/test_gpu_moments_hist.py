"""Per-pixel posterior histograms accumulated on the device (dangx_moments_hist) and their read-out as quantile / mode / count
maps: against a NumPy restatement of the definitions on the same samples pulled to the host, on a real chain and on synthetic
states with planted edge samples, across shards and alignments, the chain and every other summary left as they are, the launch
counts and the error cases.

Definitions (include/dangx.h, dang_amd/csrc/dx_hist_host.h): a sample x is counted iff lo <= x <= hi; its bin is
min(int((x - lo) * scale), nbins - 1) with scale = nbins / (hi - lo) in float64 -- restated here with the same two float64
operations, so the counters must agree integer for integer.  N = the sum of a pixel's counters.  Quantile q: target = q N, the
first bin b with c_b > 0 and cum + c_b >= target gives lo + width (b + (target - cum) / c_b), width = (hi - lo) / nbins; it lies
in the closed bin of the ceil(q N)-th smallest counted sample.  The restated walk may differ from the device's by the rounding of
its last two operations (a product and a sum of magnitude <= 2 max(|lo|, |hi|)): tolerance 4 eps max(|lo|, |hi|)."""
import ctypes

import numpy as np
import pytest
import torch

import dang_amd as da
from dang_amd import synth

from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
QS = (0.025, 0.16, 0.5, 0.84, 0.975)


def _engine(case):
    dpar, ddata, bands, comps, meta = case
    return da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)


def _snapshot(eng):
    return {l: (eng.get_amplitude(l), eng.get_indices(l) if c.nindices else None) for l, c in enumerate(eng.component_list)}


def _series(samples, plane):
    """[n][npix] of plane (l, what, k) over the snapshots"""
    l, what, k = plane
    return np.stack([s[l][0][k] if what == 0 else s[l][1][what - 1][k] for s in samples])


def _ref_bins(xs, lo, hi, nbins):
    """(counted [n][npix] bool, bin [n][npix]) by the bin rule in float64"""
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(nbins) / (hi - lo)
    with np.errstate(invalid="ignore"):
        counted = (xs >= lo) & (xs <= hi)
    b = np.zeros(xs.shape, dtype=np.int64)
    b[counted] = np.minimum(((xs[counted] - lo) * scale).astype(np.int64), nbins - 1)
    return counted, b


def _ref_counts(xs, lo, hi, nbins):
    counted, b = _ref_bins(xs, lo, hi, nbins)
    c = np.zeros((xs.shape[1], nbins), dtype=np.int64)
    pix = np.broadcast_to(np.arange(xs.shape[1]), xs.shape)
    np.add.at(c, (pix[counted], b[counted]), 1)
    return c


def _ref_quantile(c, lo, hi, q):
    """the walk of the definition over counts [npix][nbins]: (value [npix], bin [npix]); NaN / -1 where N = 0"""
    lo, hi = np.float64(lo), np.float64(hi)
    nbins = c.shape[1]
    N = c.sum(axis=1)
    target = np.float64(q) * N.astype(np.float64)
    before = np.cumsum(c, axis=1) - c
    hit = (c > 0) & ((before + c).astype(np.float64) >= target[:, None])
    b = np.argmax(hit, axis=1)
    rows = np.arange(len(c))
    cb, cum = c[rows, b].astype(np.float64), before[rows, b].astype(np.float64)
    width = (hi - lo) / np.float64(nbins)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = lo + width * (b.astype(np.float64) + (target - cum) / cb)
    val[N == 0] = np.nan
    return val, np.where(N == 0, -1, b)


def _check_registration(eng, reg, plane, rng_, nbins, bits, xs, what):
    """every check of one registration against the samples xs [n][npix]; returns (counts, quantiles [len(QS)][npix])"""
    lo, hi = rng_
    n, npix = xs.shape
    ref = _ref_counts(xs, lo, hi, nbins)
    got = eng.moments_hist_get(reg)
    assert got.dtype == (np.uint16 if bits == 16 else np.uint32) and got.shape == (npix, nbins)
    assert np.array_equal(got.astype(np.int64), ref), (what, "counters")
    counted, bins = _ref_bins(xs, lo, hi, nbins)
    nn = eng.moments_hist_stat(reg, "n")
    assert np.array_equal(nn, ref.sum(axis=1).astype(np.float64)), (what, "n")
    assert (nn[counted.all(axis=0)] == n).all()
    width = (np.float64(hi) - np.float64(lo)) / np.float64(nbins)
    tol = 4 * EPS * max(abs(lo), abs(hi))
    qd = eng.moments_hist_stat(reg, "quantile", q=QS)
    assert qd.shape == (len(QS), npix)
    some = nn > 0
    srt = np.sort(np.where(counted, xs, np.inf), axis=0)     # a pixel's counted samples first, in order
    for j, q in enumerate(QS):
        val, b = _ref_quantile(ref, lo, hi, q)
        assert np.array_equal(np.isnan(qd[j]), ~some) and np.array_equal(np.isnan(val), ~some), (what, q, "NaN exactly where N = 0")
        err = np.abs(qd[j][some] - val[some])
        print("%-40s q %.3f worst error / tolerance %.3g" % (what, q, float(err.max() / tol) if some.any() else 0.0))
        assert (err <= tol).all(), (what, q, float(err.max() / tol))
        # the closed bin of the ceil(q N)-th smallest counted sample
        pix = np.flatnonzero(some)
        k = np.ceil(np.float64(q) * nn[pix]).astype(np.int64)
        assert ((k >= 1) & (k <= nn[pix])).all()
        ok_k, bk = _ref_bins(srt[k - 1, pix][None, :], lo, hi, nbins)
        assert ok_k.all()
        bk = bk[0].astype(np.float64)
        inside = (np.float64(lo) + width * bk <= qd[j][pix]) & (qd[j][pix] <= np.float64(lo) + width * (bk + 1.0))
        assert inside.all(), (what, q, pix[~inside], "order statistic")
    mode = eng.moments_hist_stat(reg, "mode")
    assert np.array_equal(np.isnan(mode), ~some)
    bm = np.argmax(ref, axis=1).astype(np.float64)          # the first of the fullest bins
    assert np.array_equal(mode[some], (np.float64(lo) + width * (bm + 0.5))[some]), (what, "mode")
    return got, qd


def test_a_real_chain(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    sel = da.moments_begin(dpar, ddata)
    planes = da.moments_hist(dpar, ddata)
    assert planes == da.default_hist_planes(dpar, comps, sel) and len(planes) == 9      # synch 1 + 2, dust 2 + 4
    assert eng._moment_hist["nbins"] == 64 and eng._moment_hist["bits"] == 16
    samples = []
    for it in range(1, 10):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(_snapshot(eng))
    assert eng.moments_count() == 9
    spread = 0
    for r, plane in enumerate(planes):
        l, what, k = plane
        rg = tuple(comps[l].uni_prior[what - 1])
        assert eng._moment_hist["ranges"][r] == rg
        xs = _series(samples, plane)
        got, qd = _check_registration(eng, r, plane, rg, 64, 16, xs, "%s what %d plane %d" % (comps[l].label, what, k))
        spread += int(((got > 0).sum(axis=1) > 1).sum())
    assert spread > 0                                # the chain moved across bins somewhere
    pq = da.posterior_quantile_maps(ddata)
    assert list(pq) == [(comps[l].label, comps[l].ind_label[w - 1], k) for l, w, k in planes]
    e = pq[("dust", "beta", 0)]
    assert e["q"].shape == (3, meta["npix"]) and e["nbins"] == 64 and (e["n"] <= 9).all() and e["n"].max() == 9
    some = e["n"] > 0                                # a pixel whose samples all lie outside the prior's range holds NaN
    assert some.any() and np.array_equal(np.isnan(e["q"][1]), ~some)
    assert (e["q"][0][some] <= e["q"][1][some]).all() and (e["q"][1][some] <= e["q"][2][some]).all()


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
HALF = 12.0
# fixed pixels of every registered plane
P_STILL, P_LO, P_HI, P_EDGES, P_OUTSIDE, P_NONFINITE, P_MIXED, FIRST_ORDINARY = 0, 1, 2, 3, 4, 5, 6, 7


def _offset(l, what):
    return OFFSETS[(l + 2) % 3] if what == 0 else OFFSETS[(l + what - 1) % 3]


def _hist_planes(comps):
    """the amplitude on T and every index plane of every component: 24 registrations for C2"""
    return [(l, w, k) for l, c in enumerate(comps) for w in range(1 + c.nindices) for k in ((0,) if w == 0 else (0, 1, 2))]


def _synthetic_states(comps, meta, n, seed, nbins):
    """{l: (amplitudes [n][3][npix], indices [n][nind][3][npix] or None)} with the planted pixels"""
    rng = np.random.default_rng(seed)
    out = {}
    for l, c in enumerate(comps):
        planes = [_ar1(rng, n, (3, meta["npix"]), _offset(l, w)) for w in range(1 + c.nindices)]
        for w, x in enumerate(planes):
            off = _offset(l, w)
            lo, hi = np.float64(off - HALF), np.float64(off + HALF)
            t = np.arange(n)
            x[:, :, P_STILL] = off + 1.7
            x[:, :, P_LO] = lo
            x[:, :, P_HI] = hi
            x[:, :, P_EDGES] = (lo + (hi - lo) * ((t % (nbins - 1)) + 1) / nbins)[:, None]                   # every interior edge in turn
            x[:, :, P_OUTSIDE] = np.where(t % 2 == 0, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf))[:, None]
            x[:, :, P_NONFINITE] = np.array([np.nan, np.inf, -np.inf])[t % 3][:, None]
            m = x[:, :, P_MIXED].copy()
            m[t % 4 == 1] = np.nan
            m[t % 4 == 3] = np.nextafter(hi, np.inf)
            x[:, :, P_MIXED] = m
        out[l] = (planes[0], np.stack(planes[1:], axis=1) if c.nindices else None)
    return out


def _feed(engines, bounds, comps, states, n):
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


@pytest.mark.parametrize("nbins,bits", [(64, 16), (8, 16), (32, 32)])
@pytest.mark.parametrize("n", [64, 1])
def test_synthetic_states_and_planted_samples(built, n, nbins, bits):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    eng.moments_begin(None)
    planes = _hist_planes(comps)
    assert len(planes) == 24 and any(w == 0 for l, w, k in planes)
    ranges = [(_offset(l, w) - HALF, _offset(l, w) + HALF) for l, w, k in planes]
    assert da.moments_hist(dpar, ddata, planes=planes, ranges=ranges, nbins=nbins, bits=bits) == planes
    states = _synthetic_states(comps, meta, n, seed=11, nbins=nbins)
    samples = _feed([eng], [(0, meta["npix"])], comps, states, n)
    assert eng.moments_count() == n
    wide = total = 0
    for r, plane in enumerate(planes):
        xs = _series(samples, plane)
        got, qd = _check_registration(eng, r, plane, ranges[r], nbins, bits, xs, "plane %s" % (plane,))
        got = got.astype(np.int64)
        lo, hi = ranges[r]
        width = (np.float64(hi) - np.float64(lo)) / nbins
        assert got[P_LO, 0] == n and got[P_HI, nbins - 1] == n and got[P_LO].sum() == n and got[P_HI].sum() == n
        assert got[P_EDGES].sum() == n and (got[P_EDGES, 0] == 0)                    # an interior edge opens its bin: never bin 0
        if n >= nbins - 1:
            assert (got[P_EDGES, 1:] > 0).all()
        # a pixel that never moves: one bin holds everything, and every quantile
        assert (got[P_STILL] > 0).sum() == 1 and got[P_STILL].max() == n
        b = np.float64(np.argmax(got[P_STILL]))
        assert ((qd[:, P_STILL] >= lo + width * b) & (qd[:, P_STILL] <= lo + width * (b + 1))).all()
        # all samples outside (by one ulp, or not finite): N = 0, NaN quantile and mode
        for p in (P_OUTSIDE, P_NONFINITE):
            assert got[p].sum() == 0 and np.isnan(qd[:, p]).all() and np.isnan(eng.moments_hist_stat(r, "mode")[p])
            assert eng.moments_hist_stat(r, "n")[p] == 0
        assert got[P_MIXED].sum() == n - np.isin(np.arange(n) % 4, (1, 3)).sum()
        wide += int(((got[FIRST_ORDINARY:] > 0).sum(axis=1) >= 4).sum())
        total += got[FIRST_ORDINARY:].shape[0]
    if n == 64 and nbins == 64:       # a condition on the inputs: the ordinary pixels really spread over bins
        assert wide >= total / 2, (wide, total)


def _all(eng, nreg):
    out = {}
    for r in range(nreg):
        out[(r, "counts")] = eng.moments_hist_get(r)
        out[(r, "q")] = eng.moments_hist_stat(r, "quantile", q=QS)
        out[(r, "mode")] = eng.moments_hist_stat(r, "mode")
        out[(r, "n")] = eng.moments_hist_stat(r, "n")
    return out


def _cat(parts, key):
    return np.concatenate([m[key] for m in parts], axis=0 if key[1] == "counts" else -1)


def test_shards_and_determinism(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    whole, again = _engine(case), _engine(make_case("C2", nside=4))
    b3, b2 = [0, 63, 130, meta["npix_global"]], [0, 1, meta["npix_global"]]      # odd lengths; a one-pixel shard
    shards3, shards2 = shard_engines(case, 3, bounds=b3), shard_engines(case, 2, bounds=b2)
    planes = _hist_planes(comps)
    ranges = [(_offset(l, w) - HALF, _offset(l, w) + HALF) for l, w, k in planes]
    groups = ([whole], [again], shards3, shards2)
    for engs in groups:
        for e in engs:
            e.moments_begin(None)
        assert da.moments_hist(dpar, ddata, planes=planes, ranges=ranges, nbins=32, bits=16, engines=engs) == planes
    n = 6
    states = _synthetic_states(comps, meta, n, seed=5, nbins=32)
    for engs, bounds in zip(groups, ([0, meta["npix"]], [0, meta["npix"]], b3, b2)):
        _feed(engs, list(zip(bounds[:-1], bounds[1:])), comps, states, n)
    mw, ma = _all(whole, len(planes)), _all(again, len(planes))
    m3, m2 = [_all(e, len(planes)) for e in shards3], [_all(e, len(planes)) for e in shards2]
    assert any(np.isfinite(v).any() for k, v in mw.items() if k[1] == "q")
    for k, v in mw.items():
        assert np.array_equal(v, ma[k], equal_nan=True), ("two runs", k)
        assert np.array_equal(v, _cat(m3, k), equal_nan=True), ("three shards", k)
        assert np.array_equal(v, _cat(m2, k), equal_nan=True), ("a one-pixel shard", k)
    pw = da.posterior_quantile_maps(ddata, q=QS, engines=[whole])
    for shards in (shards3, shards2):
        ps = da.posterior_quantile_maps(ddata, q=QS, engines=shards)
        assert list(pw) == list(ps) and len(pw) == len(planes)
        for r, k in enumerate(pw):
            for name in ("q", "mode", "n"):
                assert np.array_equal(pw[k][name], ps[k][name], equal_nan=True), (k, name)
                assert np.array_equal(pw[k][name], mw[(r, name)], equal_nan=True)
            assert pw[k]["range"] == ps[k]["range"] == ranges[r] and ps[k]["nbins"] == 32
    shards2[1].moments_accumulate()
    with pytest.raises(da.DangxError, match="different sample counts"):
        da.posterior_quantile_maps(ddata, engines=shards2)


def test_adopted_buffers_moved_off_the_grid(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    assert eng._adopted
    da.moments_begin(dpar, ddata)
    planes = da.moments_hist(dpar, ddata, nbins=16, bits=32)
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
    assert any(p[0] == ld for p in planes)
    for r, plane in enumerate(planes):
        l, what, k = plane
        rg = tuple(comps[l].uni_prior[what - 1])
        got, _ = _check_registration(eng, r, plane, rg, 16, 32, _series(samples, plane), "adopted %s" % (plane,))
        assert got.sum() > 0


def _run(nit, hist):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    eng.profile(True)
    da.moments_begin(dpar, ddata)
    if hist == "first":
        da.moments_hist(dpar, ddata)
    da.moments_pairs(dpar, ddata)
    if hist == "last":
        da.moments_hist(dpar, ddata)
    for it in range(1, nit + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    return eng, _snapshot(eng), ddata.chisq, da.posterior_maps(ddata), da.posterior_pair_maps(ddata), ddata


def test_nothing_else_moves(built):
    e0, s0, chi0, p0, c0, d0 = _run(3, None)
    e1, s1, chi1, p1, c1, d1 = _run(3, "first")        # either order of the two registrations: neither drops the other
    e2, s2, chi2, p2, c2, d2 = _run(3, "last")
    for e, s, chi, p, c in ((e1, s1, chi1, p1, c1), (e2, s2, chi2, p2, c2)):
        assert chi == chi0
        for l in s0:
            assert np.array_equal(s[l][0], s0[l][0])
            if s0[l][1] is not None:
                assert np.array_equal(s[l][1], s0[l][1])
        assert p.keys() == p0.keys() and c.keys() == c0.keys() and len(c0) == 12
        for k in p0:
            assert set(p[k]) == set(p0[k]) == {"n", "mean", "std", "rho1", "ess"}
            for stat in ("mean", "std", "rho1", "ess"):
                assert np.array_equal(p[k][stat], p0[k][stat], equal_nan=True), (k, stat)
        for k in c0:
            assert np.array_equal(c[k], c0[k], equal_nan=True), k
    prof0, prof1, prof2 = e0.profile_get(), e1.profile_get(), e2.profile_get()
    assert prof0["k_moments"]["launches"] == prof1["k_moments"]["launches"] == prof2["k_moments"]["launches"] == 6
    assert "k_hist" not in prof0
    assert prof1["k_hist"]["launches"] == prof2["k_hist"]["launches"] == 3 and prof1["k_hist"]["total_ms"] > 0
    assert {k: v["launches"] for k, v in prof0.items()} == {k: v["launches"] for k, v in prof1.items() if k != "k_hist"}
    # both registration orders give the same histograms; the host and device getters agree bit for bit
    for r in range(9):
        h = e1.moments_hist_get(r)
        assert np.array_equal(h, e2.moments_hist_get(r))
        d = e1.moments_hist_get(r, device=True)
        assert d.is_cuda and d.dtype == torch.int16 and np.array_equal(d.cpu().numpy().view(np.uint16), h)
        for stat, q in (("quantile", QS), ("mode", None), ("n", None)):
            hs = e1.moments_hist_stat(r, stat, q=q)
            ds = e1.moments_hist_stat(r, stat, q=q, device=True)
            assert ds.is_cuda and np.array_equal(ds.cpu().numpy(), hs, equal_nan=True), (r, stat)


def test_five_iterations_with_and_without(built):
    """Five iterations with pairs and lag-1 registered, with and without histograms: the chain, chi^2 and every map bit-identical."""
    e0, s0, chi0, p0, c0, d0 = _run(5, None)
    e1, s1, chi1, p1, c1, d1 = _run(5, "last")
    assert chi1 == chi0
    for l in s0:
        assert np.array_equal(s1[l][0], s0[l][0]) and (s0[l][1] is None or np.array_equal(s1[l][1], s0[l][1]))
    for k in p0:
        for stat in ("mean", "std", "rho1", "ess"):
            assert np.array_equal(p1[k][stat], p0[k][stat], equal_nan=True), (k, stat)
    for k in c0:
        assert np.array_equal(c1[k], c0[k], equal_nan=True), k
    n5 = da.posterior_quantile_maps(d1)[("synch", "beta", 0)]["n"]
    assert (n5 <= 5).all() and n5.max() == 5


def test_template_amplitudes_are_refused(built):
    """A template / monopole / hi_fit amplitude is a row of c%template_amplitudes, not a pixel plane: refused by that name (not as
    'not selected') through the library, whose own table of global-amplitude members dangx_moments_hist builds."""
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 3, 4), amplitudes=(3.0, -2.0, 5.0))
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    sel = da.moments_begin(dpar, ddata)
    lt, lm = len(comps) - 2, len(comps) - 1
    assert (int(sel[lt]) >> 1) & 1 and int(sel[lm]) & 1           # their rows are selected: the refusal is not 'not selected'
    planes = da.moments_hist(dpar, ddata)                         # the defaults leave them out
    assert len(planes) == 9 and all(l < lt for l, w, k in planes)
    for plane in ((lt, 0, 1), (lt, 0, 2), (lm, 0, 0)):
        with pytest.raises(da.DangxError, match="template / monopole / hi_fit amplitude is not a pixel plane"):
            eng.moments_hist([plane], ranges=[(-10.0, 10.0)])
        with pytest.raises(da.DangxError, match="template / monopole / hi_fit amplitude is not a pixel plane"):
            eng.moments_hist([(1, 1, 0), plane], ranges=[None, (-10.0, 10.0)])
    assert eng._moment_hist["planes"] == planes                   # the earlier registration stays
    da.gibbs_iteration(dpar, ddata, 1)
    da.moments_accumulate(ddata)
    assert eng.moments_hist_stat(len(planes) - 1, "n").max() == 1
    with pytest.raises(da.DangxError, match="out of range"):
        eng.moments_hist_stat(len(planes), "n")


def test_errors(built):
    """Every error of dangx_moments_hist / _hist_get / _hist_stat except two: the template amplitude (the test above: C2 has no
    such member) and a failed allocation, which cannot be produced on a shared device without exhausting its memory -- that path
    frees what it had allocated and leaves the registration as it was, as the other failures here show for theirs."""
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    good = [(1, 1, 0)]
    with pytest.raises(da.DangxError, match="begin"):
        eng.moments_hist(good)
    ld = [c.label for c in comps].index("dust_P")
    sel = np.zeros(len(comps), dtype=np.int32)
    sel[1] = 1 | (1 << 3)                              # synch: amplitude and beta on T
    sel[ld] = (1 << 1) | (1 << (3 + 1)) | (1 << (6 + 1))   # dust_P: amplitude, beta and T on Q
    eng.moments_begin(sel)
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="before the first"):
        eng.moments_hist(good)
    with pytest.raises(da.DangxError, match="out of range"):
        eng.moments_hist_stat(0, "n")                  # nothing registered
    eng.moments_begin(sel)
    with pytest.raises(da.DangxError, match="no sample accumulated"):
        eng.moments_hist(good) or eng.moments_hist_stat(0, "n")
    eng.moments_begin(sel)
    first = [(1, 1, 0), (ld, 1, 1), (1, 0, 0)]
    eng.moments_hist(first, ranges=[None, (1.0, 2.0), (-50.0, 50.0)], nbins=16, bits=32)
    assert eng._moment_hist["ranges"][0] == tuple(comps[1].uni_prior[0])
    bad = [
        ("not selected", dict(planes=[(1, 1, 1)])),
        ("not selected", dict(planes=[(ld, 2, 2)])),
        ("what", dict(planes=[(1, 2, 0)])),                               # the synchrotron has one index
        ("component index", dict(planes=[(len(comps), 1, 0)])),
        ("plane out of range", dict(planes=[(1, 1, 3)])),
        ("explicit range", dict(planes=[(1, 0, 0)])),                     # an amplitude plane has no default
        ("explicit range", dict(planes=[(1, 1, 0), (1, 0, 0)], ranges=[(2.0, 3.0), None])),
        ("nbins must be", dict(planes=good, nbins=12)),
        ("nbins must be", dict(planes=good, nbins=128)),
        ("bits must be", dict(planes=good, bits=8)),
        ("128 bytes", dict(planes=good, nbins=64, bits=32)),
        ("hi > lo", dict(planes=good, ranges=[(2.0, 2.0)])),
        ("hi > lo", dict(planes=good, ranges=[(3.0, 2.0)])),
        ("non-finite", dict(planes=good, ranges=[(-np.inf, 2.0)])),
        ("non-finite", dict(planes=good, ranges=[(0.0, np.inf)])),
        ("non-finite", dict(planes=good, ranges=[(0.0, np.nan)])),
        ("DANGX_MAX_HIST", dict(planes=good * 33)),
        ("the same plane twice", dict(planes=[(1, 1, 0), (ld, 1, 1), (1, 1, 0)])),
    ]
    for match, kw in bad:
        with pytest.raises(da.DangxError, match=match):
            eng.moments_hist(**kw)
    # after the failures the earlier registration is what accumulates
    assert eng._moment_hist["planes"] == first and eng._moment_hist["nbins"] == 16
    eng.moments_accumulate()
    c = eng.moments_hist_get(1)
    assert c.dtype == np.uint32 and c.shape == (meta["npix"], 16) and (c.sum(axis=1) <= 1).all()
    assert eng.moments_hist_get(2).sum() + (eng.moments_hist_stat(2, "n") == 0).sum() == meta["npix"]
    for reg in (3, -1):
        with pytest.raises(da.DangxError, match="out of range"):
            eng.moments_hist_get(reg)
        with pytest.raises(da.DangxError, match="out of range"):
            eng.moments_hist_stat(reg, "mode")
    with pytest.raises(da.DangxError, match="stat"):
        eng.moments_hist_stat(0, 3)
    for q in ([0.0], [1.0], [0.5, 1.5], [np.nan], [-0.1]):
        with pytest.raises(da.DangxError, match="strictly inside"):
            eng.moments_hist_stat(0, "quantile", q=q)
    with pytest.raises(da.DangxError, match="quantiles"):
        eng.moments_hist_stat(0, "quantile", q=[0.5] * 17)
    with pytest.raises(da.DangxError, match="quantiles"):
        eng.moments_hist_stat(0, "quantile", q=[])
    assert eng.moments_hist_stat(0, "quantile", q=[0.5] * 16).shape == (16, meta["npix"])
    # a second registration replaces the first (nothing accumulated yet); the pairs stay; begin drops everything
    eng.moments_begin(sel)
    eng.moments_pairs([((1, 0, 0), (1, 1, 0))], lag1=True)
    eng.moments_hist(first, ranges=[None, (1.0, 2.0), (-50.0, 50.0)])
    eng.moments_hist(good, nbins=8)
    eng.moments_accumulate()
    assert eng.moments_hist_get(0).shape == (meta["npix"], 8)
    with pytest.raises(da.DangxError, match="out of range"):
        eng.moments_hist_get(1)
    assert eng.moments_get_pair(0, "cov").shape == (meta["npix"],)
    eng.moments_begin(sel)
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="out of range"):
        eng.moments_hist_stat(0, "n")
    with pytest.raises(da.DangxError, match="moments_hist was not called"):
        eng.moments_hist_get(0)
    with pytest.raises(da.DangxError, match="moments_hist was not called"):
        da.posterior_quantile_maps(ddata)


def test_counter_limit_is_refused_before_anything_is_touched(built):
    """16-bit counters take 65 535 samples: sample 65 536 is refused by name, and neither the count, the moments nor a counter
    moves.  The count is brought to the limit on a one-plane selection (each accumulation is two small launches)."""
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    sel = np.zeros(len(comps), dtype=np.int32)
    sel[1] = 1 << 3                                    # synch beta on T
    eng.moments_begin(sel)
    eng.moments_hist([(1, 1, 0)], nbins=8, bits=16)
    lib, h = eng.lib, eng.h
    for _ in range(65535):
        if lib.dangx_moments_accumulate(h):
            raise AssertionError(lib.dangx_last_error(h))
    assert eng.moments_count() == 65535
    before, mean = eng.moments_hist_get(0), eng.moments_get(1, 1, "mean")
    assert (before.astype(np.int64).sum(axis=1) == 65535).all() and before.max() == 65535     # a pixel that never moved: a full counter
    with pytest.raises(da.DangxError, match="65535"):
        eng.moments_accumulate()
    assert eng.moments_count() == 65535
    assert np.array_equal(eng.moments_hist_get(0), before) and np.array_equal(eng.moments_get(1, 1, "mean"), mean)
