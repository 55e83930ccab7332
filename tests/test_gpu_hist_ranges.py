"""Per-pixel histogram ranges on the device (dangx_moments_hist with range {-inf, +inf}, dangx_moments_hist_range_maps): the counters
against a NumPy restatement of the per-pixel rule on the same samples pulled to the host, integer for integer, on a real chain
whose ranges come from a pilot stretch (hist_ranges_from_moments) and on synthetic states, across shards and alignments; the chain
and every other summary left as they are; several chains, holders, save and restore; the error cases.

Definitions (include/dangx.h, dang_amd/csrc/dx_hist_host.h): pixel p is ON when lo[p], hi[p] are finite, hi[p] > lo[p] and neither
hi[p] - lo[p] nor nbins / (hi[p] - lo[p]) overflows; for an on pixel a sample x is counted iff lo[p] <= x <= hi[p] and its bin is
min(int((x - lo[p]) * scale_p), nbins - 1) with scale_p = nbins / (hi[p] - lo[p]) in float64 -- restated here with the same float64
operations.  An off pixel counts nothing: N = 0, NaN quantile and mode.  The restated quantile walk may differ from the device's by
the rounding of its last two operations (a product and a sum of magnitude <= 2 max(|lo[p]|, |hi[p]|)): tolerance
4 eps max(|lo[p]|, |hi[p]|) per pixel, the bound of tests/test_gpu_moments_hist.py with the pixel's own bounds."""
import ctypes

import numpy as np
import pytest
import torch

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import api, synth

import test_gpu_moments_hist as th
import test_gpu_moments_signal as ts
from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
QS = (0.025, 0.16, 0.5, 0.84, 0.975)
NPIX = 192
# planted pixels of every range map: every kind of off pixel, a pixel whose samples all lie outside, one with samples exactly on
# its bounds, a masked one (NaN, the normal case)
P_NAN, P_HI_INF, P_LO_INF, P_EQUAL, P_REVERSED, P_OVERFLOW, P_TINY, P_ALL_OUT, P_ON_EDGES, P_LO_NAN = 20, 21, 22, 23, 24, 25, 26, 27, 28, 29
OFF_PIXELS = (P_NAN, P_HI_INF, P_LO_INF, P_EQUAL, P_REVERSED, P_OVERFLOW, P_TINY, P_LO_NAN)


def _on(lo, hi, nbins):
    with np.errstate(all="ignore"):
        return np.isfinite(lo) & np.isfinite(hi) & (hi > lo) & np.isfinite(hi - lo) & np.isfinite(np.float64(nbins) / (hi - lo))


def _ref_bins(xs, lo, hi, nbins):
    """(counted [n][npix] bool, bin [n][npix]) by the per-pixel rule in float64; xs [n][npix], lo, hi [npix]"""
    on = _on(lo, hi, nbins)
    with np.errstate(all="ignore"):
        scale = np.float64(nbins) / (hi - lo)
        counted = on[None, :] & (xs >= lo[None, :]) & (xs <= hi[None, :])
        raw = (xs - lo[None, :]) * scale[None, :]
    b = np.zeros(xs.shape, dtype=np.int64)
    b[counted] = np.minimum(raw[counted].astype(np.int64), nbins - 1)
    return counted, b


def _ref_counts(xs, lo, hi, nbins):
    counted, b = _ref_bins(xs, lo, hi, nbins)
    c = np.zeros((xs.shape[1], nbins), dtype=np.int64)
    pix = np.broadcast_to(np.arange(xs.shape[1]), xs.shape)
    np.add.at(c, (pix[counted], b[counted]), 1)
    return c


def _ref_quantile(c, lo, hi, q):
    """the walk of the definition over counts [npix][nbins] with every pixel's own bounds: (value, bin); NaN / -1 where N = 0 or off"""
    nbins = c.shape[1]
    N = c.sum(axis=1)
    target = np.float64(q) * N.astype(np.float64)
    before = np.cumsum(c, axis=1) - c
    hit = (c > 0) & ((before + c).astype(np.float64) >= target[:, None])
    b = np.argmax(hit, axis=1)
    rows = np.arange(len(c))
    cb, cum = c[rows, b].astype(np.float64), before[rows, b].astype(np.float64)
    with np.errstate(all="ignore"):
        width = (hi - lo) / np.float64(nbins)
        val = lo + width * (b.astype(np.float64) + (target - cum) / cb)
    none = (N == 0) | ~_on(lo, hi, nbins)
    val[none] = np.nan
    return val, np.where(none, -1, b)


def _check(eng, reg, lo, hi, nbins, bits, xs, what, stat=None, get=None):
    """every check of one per-pixel registration against the samples xs [n][npix]; returns (counts, quantiles [len(QS)][npix]).
    stat / get: the read-outs to check (default: the engine's own)"""
    stat = stat or (lambda s, q=None: eng.moments_hist_stat(reg, s, q=q))
    n, npix = xs.shape
    ref = _ref_counts(xs, lo, hi, nbins)
    got = (get or (lambda: eng.moments_hist_get(reg)))()
    assert got.dtype == (np.uint16 if bits == 16 else np.uint32) and got.shape == (npix, nbins)
    assert np.array_equal(got.astype(np.int64), ref), (what, "counters", np.flatnonzero((got.astype(np.int64) != ref).any(axis=1))[:8])
    on = _on(lo, hi, nbins)
    assert (ref[~on] == 0).all()
    counted, bins = _ref_bins(xs, lo, hi, nbins)
    nn = stat("n")
    assert np.array_equal(nn, ref.sum(axis=1).astype(np.float64)), (what, "n")
    with np.errstate(all="ignore"):
        width = (hi - lo) / np.float64(nbins)
        tol = 4 * EPS * np.maximum(np.abs(lo), np.abs(hi))
    qd = stat("quantile", QS)
    assert qd.shape == (len(QS), npix)
    some = nn > 0
    srt = np.sort(np.where(counted, xs, np.inf), axis=0)
    worst = 0.0
    for j, q in enumerate(QS):
        val, b = _ref_quantile(ref, lo, hi, q)
        assert np.array_equal(np.isnan(qd[j]), ~some) and np.array_equal(np.isnan(val), ~some), (what, q, "NaN exactly where N = 0")
        err = np.abs(qd[j][some] - val[some])
        if some.any():
            worst = max(worst, float((err / tol[some]).max()))
        assert (err <= tol[some]).all(), (what, q, float((err / tol[some]).max()))
        pix = np.flatnonzero(some)                          # the closed bin of the ceil(q N)-th smallest counted sample
        k = np.ceil(np.float64(q) * nn[pix]).astype(np.int64)
        assert ((k >= 1) & (k <= nn[pix])).all()
        ok_k, bk = _ref_bins(srt[k - 1, pix][None, :], lo[pix], hi[pix], nbins)
        assert ok_k.all()
        bk = bk[0].astype(np.float64)
        inside = (lo[pix] + width[pix] * bk <= qd[j][pix]) & (qd[j][pix] <= lo[pix] + width[pix] * (bk + 1.0))
        assert inside.all(), (what, q, pix[~inside], "order statistic")
    print("%-44s worst quantile error / tolerance %.3g" % (what, worst))
    mode = stat("mode")
    assert np.array_equal(np.isnan(mode), ~some)
    bm = np.argmax(ref, axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        assert np.array_equal(mode[some], (lo + width * (bm + 0.5))[some]), (what, "mode")
    return got, qd


def _plant_off(lo, hi):
    """the off kinds and the pixel nothing falls into, written into a pair of range maps (numpy, in place)"""
    lo[P_NAN] = hi[P_NAN] = np.nan
    hi[P_HI_INF] = np.inf
    lo[P_LO_INF] = -np.inf
    hi[P_EQUAL] = lo[P_EQUAL] = 1.25
    lo[P_REVERSED], hi[P_REVERSED] = 3.0, 2.0
    lo[P_OVERFLOW], hi[P_OVERFLOW] = -1.7e308, 1.7e308
    lo[P_TINY], hi[P_TINY] = 0.0, 5e-324                    # nbins / (hi - lo) overflows
    lo[P_LO_NAN], hi[P_LO_NAN] = np.nan, 1.0
    lo[P_ALL_OUT], hi[P_ALL_OUT] = 1e30, 2e30               # an on pixel that no sample reaches


def _amp_planes(comps, sel):
    return [(l, 0, k) for l, c in enumerate(comps) if c.type not in da.posterior.GLOBAL_TYPES for k in range(3) if (int(sel[l]) >> k) & 1]


PILOT, NIT = 4, 9


def _real_run(ranges_for=None, nbins=64, bits=16):
    """a C2 chain at Nside 4: PILOT iterations with moments, then NIT more with a sample taken after each.  ranges_for(planes,
    pilot ranges as numpy pairs) -> the ranges to register for the amplitude planes (None: no histograms).  Returns (engine,
    planes, the ranges registered, the NIT snapshots)."""
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = th._engine(case)
    sel = da.moments_begin(dpar, ddata)
    for it in range(1, PILOT + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    planes = _amp_planes(comps, sel)
    assert len(planes) >= 3
    pilot = da.hist_ranges_from_moments(ddata, planes, nsigma=2)          # the small factor makes samples fall outside
    assert all(lo.is_cuda and hi.is_cuda and tuple(lo.shape) == (NPIX,) for lo, hi in pilot)
    for (l, w, k), (lo, hi) in zip(planes, pilot):
        mean, std = eng.moments_get(l, w, "mean")[k], eng.moments_get(l, w, "std")[k]
        still = ~(std > 0)
        assert np.array_equal(np.isnan(lo.cpu().numpy()), still) and np.array_equal(np.isnan(hi.cpu().numpy()), still)
        assert np.array_equal(lo.cpu().numpy()[~still], (mean - 2.0 * std)[~still]) and np.array_equal(hi.cpu().numpy()[~still], (mean + 2.0 * std)[~still])
    da.moments_begin(dpar, ddata)
    ranges = None
    if ranges_for is not None:
        ranges = ranges_for(planes, [(lo.cpu().numpy().copy(), hi.cpu().numpy().copy()) for lo, hi in pilot])
        assert da.moments_hist(dpar, ddata, planes=planes, ranges=ranges, nbins=nbins, bits=bits) == planes
        assert eng._moment_hist["kinds"] == ["pixel"] * len(planes) and eng._moment_hist["ranges"] == [None] * len(planes)
    samples = []
    for it in range(PILOT + 1, PILOT + NIT + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(th._snapshot(eng))
    return eng, planes, ranges, samples, ddata


@pytest.fixture(scope="module")
def plain_run(built):
    """the chain without histograms: its samples tell where to plant a range whose bounds are samples themselves"""
    eng, planes, _, samples, _ = _real_run()
    return planes, samples


# ---- 1. state planes on a real chain

@pytest.mark.parametrize("nbins,bits", [(64, 16), (8, 32)])
def test_a_real_chain_with_ranges_from_a_pilot(built, plain_run, nbins, bits):
    planes0, samples0 = plain_run

    def ranges_for(planes, pilot):
        assert planes == planes0
        out = []
        for plane, (lo, hi) in zip(planes, pilot):
            xs = th._series(samples0, plane)
            _plant_off(lo, hi)
            lo[P_ON_EDGES], hi[P_ON_EDGES] = xs[:, P_ON_EDGES].min(), xs[:, P_ON_EDGES].max()      # samples exactly on lo[p] and on hi[p]
            # device tensors and host arrays: both forms of the hand-over
            out.append((torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()) if len(out) % 2 == 0 else (lo, hi))
        return out

    eng, planes, ranges, samples, ddata = _real_run(ranges_for, nbins, bits)
    assert eng.moments_count() == NIT
    outside = spread = 0
    for r, plane in enumerate(planes):
        xs = th._series(samples, plane)
        assert np.array_equal(xs, th._series(samples0, plane))                 # the chain does not depend on what is registered
        lo, hi = (m.cpu().numpy() if torch.is_tensor(m) else m for m in ranges[r])
        glo, ghi = eng.moments_hist_range_get(r)
        assert np.array_equal(glo, lo, equal_nan=True) and np.array_equal(ghi, hi, equal_nan=True)
        dlo, dhi = eng.moments_hist_range_get(r, device=True)
        assert dlo.is_cuda and np.array_equal(dlo.cpu().numpy(), lo, equal_nan=True) and np.array_equal(dhi.cpu().numpy(), hi, equal_nan=True)
        got, qd = _check(eng, r, lo, hi, nbins, bits, xs, "real chain %s %dx%d" % (plane, nbins, bits))
        got = got.astype(np.int64)
        nn = got.sum(axis=1)
        assert (nn[list(OFF_PIXELS)] == 0).all() and nn[P_ALL_OUT] == 0 and np.isnan(qd[:, list(OFF_PIXELS) + [P_ALL_OUT]]).all()
        if xs[:, P_ON_EDGES].min() < xs[:, P_ON_EDGES].max():                  # the pixel moved: its extremes sit in the end bins
            assert nn[P_ON_EDGES] == NIT and got[P_ON_EDGES, 0] >= 1 and got[P_ON_EDGES, nbins - 1] >= 1
        ordinary = np.setdiff1d(np.arange(NPIX), list(OFF_PIXELS) + [P_ALL_OUT, P_ON_EDGES])
        outside += int((nn[ordinary] < NIT).sum())
        spread += int(((got[ordinary] > 0).sum(axis=1) > 1).sum())
    assert outside > 0 and spread > 0                # conditions on the inputs: samples fell outside 2 sigma, and pixels spread over bins
    pq = da.posterior_quantile_maps(ddata, q=QS)
    comps = eng.component_list
    assert list(pq) == [(comps[l].label, "amplitude", k) for l, w, k in planes]
    e = pq[list(pq)[0]]
    assert np.array_equal(e["range"][0], ranges[0][0].cpu().numpy(), equal_nan=True) and np.array_equal(e["range"][1], ranges[0][1].cpu().numpy(), equal_nan=True)
    assert np.array_equal(e["q"], eng.moments_hist_stat(0, "quantile", q=QS), equal_nan=True) and e["nbins"] == nbins


# ---- 2. alignment: shards with odd pix0 and odd npix, adopted tensors off the 16-byte grid

def _synthetic_ranges(planes, npix, seed):
    """per-pixel bounds about the offsets th._synthetic_states uses: widths that vary from pixel to pixel, the planted pixels of
    both this file and that one (there P_LO holds the sample off - HALF, P_HI off + HALF: made the pixel's own bounds here)"""
    rng = np.random.default_rng(seed)
    out = []
    for l, w, k in planes:
        off = th._offset(l, w)
        lo = off - th.HALF * rng.uniform(0.2, 1.0, npix)
        hi = off + th.HALF * rng.uniform(0.2, 1.0, npix)
        lo[th.P_LO], hi[th.P_HI] = off - th.HALF, off + th.HALF
        _plant_off(lo, hi)
        out.append((lo, hi))
    return out


def _all(eng, nreg):
    out = {}
    for r in range(nreg):
        out[(r, "counts")] = eng.moments_hist_get(r)
        out[(r, "q")] = eng.moments_hist_stat(r, "quantile", q=QS)
        out[(r, "mode")] = eng.moments_hist_stat(r, "mode")
        out[(r, "n")] = eng.moments_hist_stat(r, "n")
    return out


def test_shards_with_odd_boundaries(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    whole = th._engine(case)
    b3, b2 = [0, 63, 130, NPIX], [0, 1, NPIX]            # odd pix0 and odd npix; a one-pixel shard
    shards3, shards2 = shard_engines(case, 3, bounds=b3), shard_engines(case, 2, bounds=b2)
    planes = th._hist_planes(comps)
    ranges = _synthetic_ranges(planes, NPIX, seed=3)
    groups = ([whole], shards3, shards2)
    for engs in groups:
        for e in engs:
            e.moments_begin(None)
        assert da.moments_hist(dpar, ddata, planes=planes, ranges=ranges, nbins=32, bits=16, engines=engs) == planes
    n = 6
    states = th._synthetic_states(comps, meta, n, seed=5, nbins=32)
    samples = None
    for engs, bounds in zip(groups, ([0, NPIX], b3, b2)):
        samples = th._feed(engs, list(zip(bounds[:-1], bounds[1:])), comps, states, n)
    for r, plane in enumerate(planes):
        lo, hi = ranges[r]
        got, qd = _check(whole, r, lo, hi, 32, 16, th._series(samples, plane), "whole %s" % (plane,))
        assert got[th.P_LO, 0] == n and got[th.P_HI, 31] == n                  # samples exactly on lo[p] and on hi[p]
        assert (got[list(OFF_PIXELS) + [P_ALL_OUT]] == 0).all()
    mw = _all(whole, len(planes))
    m3, m2 = [_all(e, len(planes)) for e in shards3], [_all(e, len(planes)) for e in shards2]
    for k, v in mw.items():
        assert np.array_equal(v, th._cat(m3, k), equal_nan=True), ("three shards", k)
        assert np.array_equal(v, th._cat(m2, k), equal_nan=True), ("a one-pixel shard", k)
    for s, e in enumerate(shards3):                     # every context holds its slice of the maps
        glo, ghi = e.moments_hist_range_get(2)
        assert np.array_equal(glo, ranges[2][0][b3[s]:b3[s + 1]], equal_nan=True) and np.array_equal(ghi, ranges[2][1][b3[s]:b3[s + 1]], equal_nan=True)
    pw, ps = da.posterior_quantile_maps(ddata, q=QS, engines=[whole]), da.posterior_quantile_maps(ddata, q=QS, engines=shards3)
    for r, k in enumerate(pw):
        assert np.array_equal(pw[k]["q"], ps[k]["q"], equal_nan=True)
        for i in (0, 1):                                # 'range': the pair of maps, shards side by side
            assert np.array_equal(ps[k]["range"][i], ranges[r][i], equal_nan=True) and np.array_equal(pw[k]["range"][i], ranges[r][i], equal_nan=True)


def test_adopted_tensors_off_the_grid(built):
    """Planes of adopted device tensors one double off the 16-byte grid: registered there, the range maps share that phase (pairs
    behind a head element); adopted again ON the grid afterwards, x and the maps differ in phase (element by element)."""
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    assert eng._adopted
    ld = [c.label for c in comps].index("dust_P")
    npix, nmaps = meta["npix"], meta["nmaps"]

    def adopt(shift):
        amp_old, idx_old = eng._adopted[ld]
        abuf = torch.empty(nmaps * npix + 2, dtype=torch.float64, device=dev)
        ibuf = torch.empty(2 * nmaps * npix + 2, dtype=torch.float64, device=dev)
        assert abuf.data_ptr() % 16 == 0 and ibuf.data_ptr() % 16 == 0
        amp_new, idx_new = abuf[shift:shift + nmaps * npix].view(nmaps, npix), ibuf[shift:shift + 2 * nmaps * npix].view(2, nmaps, npix)
        amp_new.copy_(amp_old)
        idx_new.copy_(idx_old)
        torch.cuda.synchronize()
        eng._chk(eng.lib.dangx_adopt_device_state(eng.h, ld, ctypes.c_void_p(amp_new.data_ptr()), ctypes.c_void_p(idx_new.data_ptr())))
        eng._adopted[ld] = (amp_new, idx_new)
        comps[ld].amplitude, comps[ld].indices = amp_new, idx_new

    adopt(1)                                             # off the grid before anything is registered
    eng.moments_begin(None)
    planes = [(ld, 0, 1), (ld, 0, 2), (ld, 1, 1), (ld, 2, 2)]
    n = 8
    rng = np.random.default_rng(9)
    series = {p: th._ar1(rng, n, (npix,), th._offset(p[0], p[1])) for p in planes}
    ranges = _synthetic_ranges(planes, npix, seed=4)
    assert da.moments_hist(dpar, ddata, planes=planes, ranges=[(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)) for lo, hi in ranges],
                           nbins=16, bits=32) == planes
    for t in range(n):
        if t == n // 2:
            adopt(0)                                     # back onto the grid: the maps keep the phase they were given
        amp, idx = eng._adopted[ld]
        for (l, w, k), xs in series.items():
            (amp[k] if w == 0 else idx[w - 1][k]).copy_(torch.from_numpy(xs[t]).to(dev))
        torch.cuda.synchronize()
        da.moments_accumulate(ddata)
        eng.synchronize()                                # the sample is taken before the next one is written over it
    for r, plane in enumerate(planes):
        got, _ = _check(eng, r, ranges[r][0], ranges[r][1], 16, 32, series[plane], "adopted %s" % (plane,))
        assert got.sum() > 0


# ---- 3. signals as sources

T_, Q_, U_, P_ = 0, 1, 2, 3
# T of a power law (synch) at a delta band; Q, U and P of a modified blackbody (dust_P) at a delta band; its P at an integrated band,
# so that the bandpass form of the kernel runs with histograms too
SIG_SPECS = [(1, 0, T_), (5, 2, Q_), (5, 2, U_), (5, 2, P_), (5, 1, P_)]


def _signal_context(states=None, hist=None, nbins=64, bits=16, fresh=False):
    """a C2 context at Nside 4 with every second band integrated and SIG_SPECS registered; hist: the ranges of a histogram on every
    signal (None: no histograms).  states: fed one by one with a sample taken after each; fresh: moments_begin + moments_signals
    anew before every sample, so that the mean after it IS the sample (Welford from zero with n = 1 is exact) -- returns those."""
    case = make_case("C2", nside=4, start="truth", tweak=ts._bandpass_tweak)
    dpar, ddata, bands, comps, meta = case
    eng = ts._engine(case)
    assert bands[1].id != "delta" and bands[0].id == "delta" and bands[2].id == "delta"
    assert comps[1].type == "power-law" and comps[5].type == "mbb"
    eng.profile(True)

    def register():
        eng.moments_begin(None)
        eng.moments_signals(SIG_SPECS)
        if hist is not None:
            eng.moments_hist([("signal", s) for s in range(len(SIG_SPECS))], ranges=hist, nbins=nbins, bits=bits)

    register()
    xs = []
    for st in states or []:
        if fresh:
            register()
        for l, (a, x) in st.items():
            eng.put_amplitude(l, np.ascontiguousarray(a))
            if x is not None:
                eng.put_indices(l, np.ascontiguousarray(x))
        eng.moments_accumulate()
        if fresh:
            xs.append([eng.moments_get_signal(s, "mean") for s in range(len(SIG_SPECS))])
    return eng, case, (np.array(xs) if fresh else None)


@pytest.mark.parametrize("nbins,bits", [(64, 16), (8, 32)])
def test_histograms_of_signals(built, nbins, bits):
    n = 7
    states = ts._states(make_case("C2", nside=4, start="truth", tweak=ts._bandpass_tweak), n)
    B, _, xs = _signal_context(states, fresh=True)                      # xs [n][signal][npix]: the device's own samples
    assert xs.shape == (n, len(SIG_SPECS), NPIX) and np.isfinite(xs).all() and (xs[:, 3] >= 0).all()
    ranges, maps = [], []
    for s in range(len(SIG_SPECS)):
        x = xs[:, s]
        lo = x.min(axis=0) + 0.3 * (x.max(axis=0) - x.min(axis=0))      # the lower samples fall outside
        hi = x.max(axis=0).copy()                                       # the largest sample exactly on hi[p]
        _plant_off(lo, hi)
        lo[P_ON_EDGES] = x[:, P_ON_EDGES].min()                         # ... and here the smallest exactly on lo[p]
        if s == 0:                                                      # one histogram with ONE range for the shard
            g = (float(np.quantile(x, 0.2)), float(np.quantile(x, 0.9)))
            ranges.append(g)
            maps.append((np.full(NPIX, g[0]), np.full(NPIX, g[1])))
        else:
            ranges.append((lo, hi) if s % 2 else (torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()))
            maps.append((lo, hi))
    A, case, _ = _signal_context(states, hist=ranges, nbins=nbins, bits=bits)
    C, _, _ = _signal_context(states)                                   # the same states, no histogram
    assert A._moment_hist["sources"] == ["signal"] * 5 and A._moment_hist["kinds"] == ["global"] + ["pixel"] * 4
    assert A._moment_hist["planes"] == [(s, L.HIST_SIGNAL, 0) for s in range(5)]
    counted_some = outside_some = 0
    for s in range(len(SIG_SPECS)):
        lo, hi = maps[s]
        got, qd = _check(A, s, lo, hi, nbins, bits, xs[:, s], "signal %s %dx%d" % (SIG_SPECS[s], nbins, bits))
        got = got.astype(np.int64)
        nn = got.sum(axis=1)
        counted_some += int((nn > 0).sum())
        outside_some += int((nn < n).sum())
        if s:
            assert (nn[list(OFF_PIXELS) + [P_ALL_OUT]] == 0).all()
            assert nn[P_ON_EDGES] == n and got[P_ON_EDGES, 0] >= 1 and got[P_ON_EDGES, nbins - 1] >= 1
        # mean and m2 are what the plain form gives on the same samples, bit for bit
        for stat, ddof in (("mean", 0), ("std", 0), ("std", 1)):
            assert ts._same_bits(A.moments_get_signal(s, stat, ddof), C.moments_get_signal(s, stat, ddof)), (s, stat)
    assert counted_some > 0 and outside_some > 0
    # no launch more than without the histograms: the HIST forms take the place of the plain ones, and no k_hist launch at all
    pa, pc = A.profile_get(), C.profile_get()
    ma, mc = A.profile_get(by_planes=True), C.profile_get(by_planes=True)
    assert pa["k_signal"]["launches"] == pc["k_signal"]["launches"] == 2 * n and "k_hist" not in pa
    assert ma[("k_signal", 2)]["launches"] == mc[("k_signal", 2)]["launches"] == n            # the bandpass form, once per sample
    assert {k: v["launches"] for k, v in pa.items()} == {k: v["launches"] for k, v in pc.items()}
    # keyed as posterior_signal_maps keys them
    dpar, ddata, bands, comps, meta = case
    pq = da.posterior_quantile_maps(ddata, q=QS, engines=[A])
    assert list(pq) == [(comps[l].label, bands[j].label, "TQUP"[k]) for l, j, k in SIG_SPECS] == list(da.posterior_signal_maps(ddata, engines=[A]))
    first, last = pq[list(pq)[0]], pq[list(pq)[4]]
    assert first["range"] == ranges[0] and np.array_equal(last["range"][0], maps[4][0], equal_nan=True)
    assert np.array_equal(last["q"], A.moments_hist_stat(4, "quantile", q=QS), equal_nan=True)
    # ranges from a pilot: a signal's own moments, the lower bound of P not below 0
    pr = da.hist_ranges_from_moments(ddata, [("signal", 0), ("signal", 3)], nsigma=50.0, engines=[C])
    m3, s3 = C.moments_get_signal(3, "mean"), C.moments_get_signal(3, "std")
    lo3 = pr[1][0].cpu().numpy()
    assert (lo3[s3 > 0] >= 0).all() and (lo3[(s3 > 0) & (m3 - 50.0 * s3 < 0)] == 0).all() and ((m3 - 50.0 * s3 < 0) & (s3 > 0)).any()
    assert np.array_equal(pr[1][1].cpu().numpy()[s3 > 0], (m3 + 50.0 * s3)[s3 > 0])
    m0, s0 = C.moments_get_signal(0, "mean"), C.moments_get_signal(0, "std")
    assert np.array_equal(pr[0][0].cpu().numpy()[s0 > 0], (m0 - 50.0 * s0)[s0 > 0])           # T is not clipped


def test_signal_source_errors(built):
    case = make_case("C2", nside=4, start="truth")
    eng = ts._engine(case)
    eng.moments_begin(None)
    with pytest.raises(da.DangxError, match="registration 0: a signal source, and no signals are registered"):
        eng.moments_hist([("signal", 0)], ranges=[(0.0, 1.0)])
    eng.moments_signals(SIG_SPECS[:3])
    with pytest.raises(da.DangxError, match=r"registration 1: signal index out of range .3 signals registered"):
        eng.moments_hist([("signal", 0), ("signal", 3)], ranges=[(0.0, 1.0), (0.0, 1.0)])
    with pytest.raises(da.DangxError, match="registration 0: signal index out of range"):
        eng.moments_hist([(-1, L.HIST_SIGNAL, 0)], ranges=[(0.0, 1.0)])
    with pytest.raises(da.DangxError, match="registration 1: the same signal twice"):
        eng.moments_hist([("signal", 2), ("signal", 2)], ranges=[(0.0, 1.0), (0.0, 2.0)])
    for ranges in (None, [None, (0.0, 1.0)]):
        with pytest.raises(da.DangxError, match="registration 0: a signal source has no default range"):
            eng.moments_hist([("signal", 1), (1, 1, 0)], ranges=ranges)
    assert eng._moment_hist is None                                      # nothing was registered by the refused calls
    eng.moments_hist([("signal", 1), (1, 1, 0)], ranges=[(0.0, 1.0), None])   # a signal beside a state plane with its default range
    with pytest.raises(da.DangxError, match="dangx_moments_signals: histogram registration 0 reads signal 1 of the present list: drop the histograms first"):
        eng.moments_signals(SIG_SPECS[:2])
    eng.moments_accumulate()
    assert eng.moments_hist_stat(0, "n").shape == (NPIX,)
    eng.moments_begin(None)                                              # begin drops everything
    eng.moments_signals(SIG_SPECS[:3])
    eng.moments_hist([("signal", 1)], ranges=[(0.0, 1.0)])
    eng.moments_hist([])                                                 # the histograms dropped: the list may be replaced
    eng.moments_signals(SIG_SPECS[:2])
    eng.moments_accumulate()


# ---- 4. nothing else moves

def _run(nit, per_pixel, plain=True):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = th._engine(case)
    eng.profile(True)
    sel = da.moments_begin(dpar, ddata)
    da.moments_pairs(dpar, ddata)
    planes = da.default_hist_planes(dpar, comps, sel) if plain else []
    ranges = [None] * len(planes)
    if per_pixel:
        amps = _amp_planes(comps, sel)
        maps = _synthetic_ranges(amps, NPIX, seed=8)
        for (lo, hi) in maps:                           # wide enough to count a real chain's amplitudes somewhere
            on = _on(lo, hi, 64)
            lo[on], hi[on] = -1e3, 1e3
        planes, ranges = planes + amps, ranges + maps
    da.moments_hist(dpar, ddata, planes=planes, ranges=ranges)
    for it in range(1, nit + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    return eng, th._snapshot(eng), ddata.chisq, da.posterior_maps(ddata), da.posterior_pair_maps(ddata)


def test_nothing_else_moves(built):
    n = 3
    e0, s0, chi0, p0, c0 = _run(n, False)
    e1, s1, chi1, p1, c1 = _run(n, True)
    e2, s2, chi2, p2, c2 = _run(n, True, plain=False)
    for s, chi, p, c in ((s1, chi1, p1, c1), (s2, chi2, p2, c2)):
        assert chi == chi0
        for l in s0:
            assert np.array_equal(s[l][0], s0[l][0]) and (s0[l][1] is None or np.array_equal(s[l][1], s0[l][1]))
        assert p.keys() == p0.keys() and c.keys() == c0.keys()
        for k in p0:
            for stat in ("mean", "std", "rho1", "ess"):
                assert np.array_equal(p[k][stat], p0[k][stat], equal_nan=True), (k, stat)
        for k in c0:
            assert np.array_equal(c[k], c0[k], equal_nan=True), k
    nplain = len(e0._moment_hist["planes"])
    assert nplain == 9 and e1._moment_hist["kinds"][:nplain] == ["global"] * nplain and "pixel" in e1._moment_hist["kinds"]
    for r in range(nplain):                             # the histograms of the plain registrations are the same bits
        assert np.array_equal(e0.moments_hist_get(r), e1.moments_hist_get(r))
        assert np.array_equal(e0.moments_hist_stat(r, "quantile", q=QS), e1.moments_hist_stat(r, "quantile", q=QS), equal_nan=True)
    assert sum(int(e1.moments_hist_get(r).sum()) for r in range(nplain, len(e1._moment_hist["planes"]))) > 0
    # launches: one more histogram launch per accumulation only where per-pixel registrations exist, told apart by its mark
    prof = [e.profile_get() for e in (e0, e1, e2)]
    marked = [e.profile_get(by_planes=True) for e in (e0, e1, e2)]
    assert prof[0]["k_hist"]["launches"] == n and ("k_hist", 2) not in marked[0]
    assert prof[1]["k_hist"]["launches"] == 2 * n and marked[1][("k_hist", 2)]["launches"] == n
    assert prof[2]["k_hist"]["launches"] == n and marked[2][("k_hist", 2)]["launches"] == n
    assert all("k_signal" not in p for p in prof)
    for p in prof[1:]:
        assert {k: v["launches"] for k, v in p.items() if k != "k_hist"} == {k: v["launches"] for k, v in prof[0].items() if k != "k_hist"}


# ---- 5. several chains and transport

def _fed(case, planes, ranges, states, first, last, nbins=16, bits=16, load=None):
    """an engine with the per-pixel registrations, fed samples first..last-1 of `states` (after moments_load of `load`)"""
    dpar, ddata, bands, comps, meta = case
    eng = da.Engine(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    eng.moments_begin(None)
    eng.moments_hist(planes, ranges=ranges, nbins=nbins, bits=bits)
    if load:
        da.moments_load(None, load, engines=[eng])
    cut = {l: (a[first:last], None if x is None else x[first:last]) for l, (a, x) in states.items()}
    th._feed([eng], [(0, NPIX)], comps, cut, last - first)
    return eng


def test_several_chains_holders_save_and_restore(built, tmp_path):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    planes = [(1, 0, 0), (2, 1, 0), (5, 2, 2)]
    ranges = _synthetic_ranges(planes, NPIX, seed=21)
    mixed = [ranges[0], (th._offset(2, 1) - th.HALF, th._offset(2, 1) + th.HALF), ranges[2]]      # a global range between two per-pixel ones
    n = 10
    sa, sb = (th._synthetic_states(comps, meta, n, seed=s, nbins=16) for s in (31, 32))
    A, B = _fed(case, planes, mixed, sa, 0, n), _fed(case, planes, mixed, sb, 0, n)
    assert A._moment_hist["kinds"] == ["pixel", "global", "pixel"]
    for r in (0, 2):
        lo, hi = ranges[r]
        xa, xb = th._series([{l: (sa[l][0][t], None if sa[l][1] is None else sa[l][1][t]) for l in sa} for t in range(n)], planes[r]), \
            th._series([{l: (sb[l][0][t], None if sb[l][1] is None else sb[l][1][t]) for l in sb} for t in range(n)], planes[r])
        both = np.concatenate([xa, xb])                  # the bins of the two chains summed are the bins of all their samples
        summed = lambda: (A.moments_hist_get(r).astype(np.uint32) + B.moments_hist_get(r).astype(np.uint32)).astype(np.uint16)
        _check(None, r, lo, hi, 16, 16, both, "two chains, registration %d" % r,
               stat=lambda s, q=None: da.chains_hist_stat([A, B], r, s, q=q), get=summed)
    want = {(r, s): da.chains_hist_stat([A, B], r, s, q=QS if s == "quantile" else None) for r in range(3) for s in ("quantile", "mode", "n")}
    rank = {(r, s): da.chains_hist_rank([A, B], r, s) for r in range(3) for s in ("bulk", "folded", "max")}
    assert any(np.isfinite(v).any() for v in rank.values())
    # the rank R-hat reads records alone: the same records under a global range give the same bits
    G = [_fed(case, planes, [(-1.0, 1.0)] * 3, s, 0, n) for s in (sa, sb)]
    for g, live in zip(G, (A, B)):
        for r in range(3):
            g.moments_section_put("HIST", r, 0, live.moments_section_get("HIST", r, 0))
    for (r, s), v in rank.items():
        assert np.array_equal(da.chains_hist_rank(G, r, s), v, equal_nan=True), (r, s)
    # a chain whose maps differ in one pixel is refused, by its number
    other = [(ranges[0][0].copy(), ranges[0][1].copy()), mixed[1], ranges[2]]
    other[0][1][100] = np.nextafter(other[0][1][100], np.inf)
    C = _fed(case, planes, other, sb, 0, n)
    with pytest.raises(da.DangxError, match="chain 1: histogram registration 0 is not the registration of chain 0"):
        da.chains_hist_stat([A, C], 0, "quantile", q=QS)
    with pytest.raises(da.DangxError, match="chain 1: histogram registration 0 is not the registration of chain 0"):
        da.chains_hist_rank([A, C], 0, "max")
    da.chains_hist_stat([A, C], 2, "quantile", q=QS)      # its other registrations are the same
    # a holder fed HEAD, HIST and HIST_RANGE answers as the live chain does
    assert A.moments_sections().count((L.SEC_HIST_RANGE, 0, 0)) == 1 and (L.SEC_HIST_RANGE, 1, 0) not in A.moments_sections()
    assert A.moments_section_bytes("HIST_RANGE", 0) == 16 * NPIX

    def holder(live, with_range, device):
        h = api._holder_engine(live)
        h.moments_begin_like(live)
        h.moments_section_put("HEAD", 0, 0, live.moments_section_get("HEAD"))
        for f, a, b in live.moments_sections():
            if f == L.SEC_HIST or (f == L.SEC_HIST_RANGE and with_range):
                buf = live.moments_section_get(f, a, b, device=device)
                live.synchronize()
                h.moments_section_put(f, a, b, buf)
                h.synchronize()
        return h

    for device in (False, True):
        Ah, Bh = holder(A, True, device), holder(B, True, device)
        for engs in ([A, Bh], [Ah, B], [Ah, Bh]):
            for (r, s), v in want.items():
                assert np.array_equal(da.chains_hist_stat(engs, r, s, q=QS if s == "quantile" else None), v, equal_nan=True), (r, s, device)
        glo, ghi = Ah.moments_hist_range_get(0)
        assert np.array_equal(glo, ranges[0][0], equal_nan=True) and np.array_equal(ghi, ranges[0][1], equal_nan=True)
    # a holder at position 0 without HIST_RANGE: quantile and mode name the chain and the section; N and the rank R-hat do not need it
    A0 = holder(A, False, False)
    for s in ("quantile", "mode"):
        with pytest.raises(da.DangxError, match=r"chain 0.*HIST_RANGE\(0\)"):
            da.chains_hist_stat([A0, B], 0, s, q=QS if s == "quantile" else None)
    assert np.array_equal(da.chains_hist_stat([A0, B], 0, "n"), want[(0, "n")])
    assert np.array_equal(da.chains_hist_rank([A0, B], 0, "max"), rank[(0, "max")], equal_nan=True)
    assert np.array_equal(da.chains_hist_stat([A0, B], 1, "quantile", q=QS), want[(1, "quantile")], equal_nan=True)     # the global one
    assert np.array_equal(da.chains_hist_stat([A, holder(B, False, False)], 0, "quantile", q=QS), want[(0, "quantile")], equal_nan=True)
    with pytest.raises(da.DangxError, match=r"HIST_RANGE\(0\).*checksum"):        # maps that are not the registration's
        A0.moments_section_put("HIST_RANGE", 0, 0, C.moments_section_get("HIST_RANGE", 0, 0))
    with pytest.raises(da.DangxError, match=r"HIST_RANGE\(0\).*checksum"):
        A.moments_section_put("HIST_RANGE", 0, 0, C.moments_section_get("HIST_RANGE", 0, 0))
    A.moments_section_put("HIST_RANGE", 0, 0, A.moments_section_get("HIST_RANGE", 0, 0))              # its own: accepted
    # the maps by name, shards being one engine per chain
    cq = da.chains_quantile_maps([[A], [B]], q=QS)
    assert list(cq) == [(comps[l].label, da.posterior._plane_name(comps[l], w), k) for l, w, k in planes]
    first = cq[list(cq)[0]]
    assert np.array_equal(first["q"], want[(0, "quantile")], equal_nan=True) and np.array_equal(first["range"][0], ranges[0][0], equal_nan=True)
    assert cq[list(cq)[1]]["range"] == mixed[1]
    cr = da.chains_rank_maps([[A0], [B]])
    assert np.array_equal(cr[list(cr)[0]]["rhat_max"], rank[(0, "max")], equal_nan=True)
    assert np.array_equal(cr[list(cr)[0]]["range"][0], ranges[0][0], equal_nan=True)       # B, a live chain, holds the maps
    # holders only, none fed HIST_RANGE (the rank R-hat moves no such section): the same statistic, 'range' None for the per-pixel
    # registrations and the two numbers for the global one
    ch = da.chains_rank_maps([[A0], [holder(B, False, False)]])
    for k, key in enumerate(cr):
        assert np.array_equal(ch[key]["rhat_max"], cr[key]["rhat_max"], equal_nan=True)
        assert ch[key]["range"] == (mixed[1] if k == 1 else None)
    # save, a fresh engine with the same registrations, load, more samples: the uninterrupted run
    path = str(tmp_path / "run.moments")
    half = _fed(case, planes, mixed, sa, 0, 6)
    da.moments_save(None, path, engines=[half])
    resumed = _fed(case, planes, mixed, sa, 6, n, load=path)
    assert resumed.moments_count() == n
    for r in range(3):
        assert np.array_equal(resumed.moments_hist_get(r), A.moments_hist_get(r))
        assert np.array_equal(resumed.moments_hist_stat(r, "quantile", q=QS), A.moments_hist_stat(r, "quantile", q=QS), equal_nan=True)
    with pytest.raises(da.DangxError, match="the histogram registrations"):        # a registration with other maps
        _fed(case, planes, other, sa, 6, n, load=path)


# ---- 6. errors, each by message

def test_errors(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = th._engine(case)
    eng.moments_begin(None)
    lo, hi = np.full(NPIX, -1.0), np.full(NPIX, 1.0)
    inf = np.inf
    eng.moments_hist([(1, 0, 0), (1, 1, 0)], ranges=[(-inf, inf), (-4.0, -2.0)])       # declared through the library's own sentinel
    assert eng._moment_hist["kinds"] == ["pixel", "global"] and eng._moment_hist["ranges"] == [None, (-4.0, -2.0)]
    with pytest.raises(da.DangxError, match="registration 1 has a global range: it did not declare per-pixel maps"):
        eng.moments_hist_range_maps(1, lo, hi)
    with pytest.raises(da.DangxError, match="histogram registration out of range .2 registered"):
        eng.moments_hist_range_maps(2, lo, hi)
    with pytest.raises(da.DangxError, match="registration 0 has no range maps yet"):
        eng.moments_hist_range_get(0)
    with pytest.raises(da.DangxError, match="dangx_moments_accumulate: histogram registration 0 declared per-pixel ranges and has no maps"):
        eng.moments_accumulate()
    assert eng.moments_count() == 0
    with pytest.raises(da.DangxError, match=r"HIST_RANGE\(1\): histogram registration 1 has a global range"):
        eng.moments_section_bytes("HIST_RANGE", 1)
    with pytest.raises(da.DangxError, match=r"HIST_RANGE\(0\): histogram registration 0 has no range maps yet"):
        eng.moments_section_get("HIST_RANGE", 0)
    with pytest.raises(da.DangxError, match="family must be 0 .HEAD. .. 6 .HIST_RANGE."):
        eng.moments_section_bytes(7, 0)
    glo, ghi = eng.moments_hist_range_get(1)             # a global range: its constants, spread over the shard
    assert (glo == -4.0).all() and (ghi == -2.0).all() and glo.shape == (NPIX,)
    dlo, dhi = eng.moments_hist_range_get(1, device=True)
    assert (dlo.cpu().numpy() == -4.0).all() and (dhi.cpu().numpy() == -2.0).all()
    eng.moments_hist_range_maps(0, lo, hi)
    eng.moments_hist_range_maps(0, lo - 1.0, hi)         # a second call replaces the first
    assert np.array_equal(eng.moments_hist_range_get(0)[0], lo - 1.0)
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="dangx_moments_hist_range_maps is legal only before the first dangx_moments_accumulate"):
        eng.moments_hist_range_maps(0, lo, hi)
    for bad in ((-inf, 2.0), (0.0, inf), (inf, -inf), (0.0, np.nan)):                # any other non-finite bound stays the error it is
        eng.moments_begin(None)
        with pytest.raises(da.DangxError, match="non-finite"):
            eng.moments_hist([(1, 0, 0)], ranges=[bad])
    eng.moments_begin(None)
    with pytest.raises(AssertionError):
        eng.moments_hist([(1, 0, 0)], ranges=[(lo[:10], hi[:10])])                     # maps of another length
    eng.moments_begin(None)                              # moments_begin dropped everything: nothing registered, nothing refused
    eng.moments_accumulate()
    assert eng.moments_count() == 1
