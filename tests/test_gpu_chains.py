"""Read-outs over several chains (dangx_chains_*): Gelman-Rubin R-hat, W, B/n, the pooled mean / std / ESS / pair statistics /
quantiles, combined on the device from the per-chain accumulators.  Against closed forms on planted samples, against a long-double
evaluation of the definitions on the same samples (references and tolerances: tests/chains_ref.py), across shards, alignments and
streams, with everything else left as it is, and the error cases.

Not covered here: contexts on different devices (the check exists; one device cannot make such a pair)."""
import ctypes

import numpy as np
import pytest
import torch

import dang_amd as da
from dang_amd import synth

import chains_ref as cr
import test_gpu_moments_hist as th
import test_gpu_moments_pairs as tp
import test_gpu_moments_signal as ts
from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

EPS = cr.EPS
GLOBAL = tp.GLOBAL
NPIX = 192
STATS = ("mean", "std", "rhat", "W", "B", "ess")


def _engine(case):
    dpar, ddata, bands, comps, meta = case
    return da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)


@pytest.fixture(scope="module")
def four(built):
    """four independent whole-sky C2 contexts at Nside 4; every test restarts their accumulators with moments_begin"""
    cases = [make_case("C2", nside=4) for _ in range(4)]
    return cases, [_engine(c) for c in cases]


def _feed_chain(eng, comps, states, n):
    return tp._feed([eng], [(0, NPIX)], comps, states, n)


def _check_planes(engs, sel, samples, what_for, ddof=1, between=True, min_finite=None, stats=STATS):
    """every selected plane of every component over the chains `engs` against the long-double references on samples[k] (snapshots)"""
    got = {}
    for l, c in enumerate(engs[0].component_list):
        for what in range(1 + c.nindices):
            ks = tp._planes(sel[l], what)
            if not ks:
                continue
            glob = what == 0 and c.type in GLOBAL
            xs = [tp._series(s, l, what) for s in samples]
            get = (lambda stat: da.chains_get_template(engs, l, stat, ddof)) if glob else (lambda stat: da.chains_get(engs, l, what, stat, ddof))
            pm = cr.pooled(xs, ddof)
            bw = cr.between(xs) if between else None
            for k in ks:
                name = "%s %s what %d plane %d" % (what_for, c.label, what, k)
                for stat in ("mean", "std"):
                    cr.compare(get(stat)[k], pm[stat][0][k], pm[stat][1][k], "pooled %s %s" % (stat, name))
                if not between:
                    continue
                for stat in ("W", "B"):
                    cr.compare(get(stat)[k], bw[stat][0][k], bw[stat][1][k], "%s %s" % (stat, name))
                r = get("rhat")[k]
                cr.compare(r.astype(cr.LD) ** 2, bw["rhat2"][0][k], bw["rhat2"][1][k], "R-hat^2 %s" % name, None if glob else min_finite)
                got[(l, what, k)] = r
                if "ess" in stats:
                    cr.compare(get("ess")[k], bw["ess"][0][k], bw["ess"][1][k], "pooled ESS %s" % name)
    return got


def _check_pairs(engs, pairs, samples, what_for, ddofs=(0, 1)):
    for p, (a, b) in enumerate(pairs):
        xa = [tp._series(s, a[0], a[1])[:, a[2]] for s in samples]
        xb = [tp._series(s, b[0], b[1])[:, b[2]] for s in samples]
        for ddof in ddofs:
            pp = cr.pooled_pair(xa, xb, ddof)
            if ddof == ddofs[0]:
                cr.compare(da.chains_get_pair(engs, p, "corr"), *pp["corr"], "%s pooled corr pair %d" % (what_for, p))
            dev = da.chains_get_pair(engs, p, "cov", ddof)
            ref, tol = pp["cov"]
            fin = np.isfinite(tol)                       # a variance of zero: the covariance is exactly 0
            assert not np.isnan(dev).any() and (dev[~fin] == 0).all() and (ref[~fin] == 0).all()
            cr.compare(dev[fin], ref[fin], tol[fin] + 1e-300, "%s pooled cov pair %d ddof %d" % (what_for, p, ddof))


# ---- 1. planted samples with a closed form

def _planted(comps, k, c, off, n=8, apart=False):
    """chain k: (t + c k) s_p + off with s_p a power of two per pixel; pixel 0 holds `off` in every chain, and with `apart` pixel 1
    holds off + k: chains that differ in their means alone"""
    s = 2.0 ** ((np.arange(NPIX) % 7) - 3)
    x = (np.arange(n)[:, None] + c * k) * s[None, :] + off                 # [n][npix]
    x[:, 0] = off
    if apart:
        x[:, 1] = off + k
    out = {}
    for l, cc in enumerate(comps):
        a = np.repeat(x[:, None, :], 3, axis=1)
        out[l] = (a, np.repeat(a[:, None], cc.nindices, axis=1) if cc.nindices else None)
    return out, s


@pytest.mark.parametrize("off", tp.OFFSETS)
@pytest.mark.parametrize("c", [0, 1, 4])
def test_planted_samples_with_a_closed_form(four, c, off):
    cases, engs = four
    comps = cases[0][3]
    samples = []
    for k, e in enumerate(engs):
        e.moments_begin(None)
        e.moments_pairs([], lag1=True)
        states, s = _planted(comps, k, c, off)
        samples.append(_feed_chain(e, comps, states, 8))
    sel = engs[0]._moment_sel
    rh = _check_planes(engs, sel, samples, "planted c %d off %g" % (c, off))
    for (l, what, k), r in rh.items():
        assert np.isnan(r[0]) and np.isfinite(r[1:]).all()                  # the pixel no chain ever moved, and nowhere else
        ess = da.chains_get(engs, l, what, "ess")[k]
        assert np.isnan(ess[0]) and np.isfinite(ess[1:]).all()
        if off == 0.0:          # every input is exact
            W, B = da.chains_get(engs, l, what, "W")[k][1:], da.chains_get(engs, l, what, "B")[k][1:]
            s2 = (s * s)[1:]
            assert (np.abs(W - 6 * s2) <= 64 * EPS * 6 * s2).all()
            assert (np.abs(B - 5 * c * c * s2 / 3) <= 64 * EPS * 5 * c * c * s2 / 3).all()
            r2 = 7 / 8 + 5 * c * c / 18
            assert (np.abs(r[1:] ** 2 - r2) <= 64 * EPS * r2).all()
            assert (np.abs(r[1:] - np.sqrt(r2)) <= 64 * EPS * np.sqrt(r2)).all()


def test_chains_that_differ_in_their_means_alone(four):
    cases, engs = four
    comps = cases[0][3]
    for k, e in enumerate(engs):
        e.moments_begin(None)
        e.moments_pairs([], lag1=True)
        _feed_chain(e, comps, _planted(comps, k, 1, 0.0, apart=True)[0], 8)
    for l, c in enumerate(comps):
        for what in range(1 + c.nindices):
            r, W, B, ess = (da.chains_get(engs, l, what, st) for st in ("rhat", "W", "B", "ess"))
            assert np.isnan(r[:, 0]).all() and (r[:, 1] == np.inf).all() and np.isfinite(r[:, 2:]).all()
            assert (W[:, :2] == 0).all() and (B[:, 0] == 0).all() and (B[:, 1] == 5 / 3).all()
            assert np.isnan(ess[:, :2]).all() and np.isfinite(ess[:, 2:]).all()
            assert (da.chains_get(engs, l, what, "mean")[:, 1] == 1.5).all()


# ---- 2. against long double on the same samples

@pytest.mark.parametrize("counts", [(5, 64, 2), (64, 64, 64)], ids=["n5_64_2", "n64"])
def test_against_long_double(four, counts):
    cases, engs = four
    engs = engs[:3]
    dpar, ddata, bands, comps, meta = cases[0]
    samples = []
    pairs = None
    for k, (e, n) in enumerate(zip(engs, counts)):
        e.moments_begin(None)
        pairs = da.default_moment_pairs(dpar, comps, e._moment_sel)
        e.moments_pairs(pairs, lag1=True)
        samples.append(_feed_chain(e, comps, tp._synthetic_states(comps, meta, n, seed=11 + 7 * k), n))
    assert len(pairs) == 24
    equal = len(set(counts)) == 1
    rh = _check_planes(engs, engs[0]._moment_sel, samples, "n %s" % (counts,), between=equal)
    _check_pairs(engs, pairs, samples, "n %s" % (counts,))
    if equal:
        # _ar1 never moves pixel 0 within a chain, and the chains hold different values there: W = 0, B/n > 0
        assert all(r[0] == np.inf and np.isfinite(r[1:]).all() for r in rh.values())
        assert any((r[1:] > 1.0).any() for r in rh.values())
    else:
        for stat in ("rhat", "W", "B"):
            with pytest.raises(da.DangxError, match="equal sample counts.*chain 1 holds 64"):
                da.chains_get(engs, 1, 0, stat)
        ess = da.chains_get(engs, 1, 0, "ess")                                        # the pooled ESS needs no equal counts:
        assert ess.shape == (3, NPIX) and np.isnan(ess[:, 0]).all()                    # NaN wherever a chain's two samples agree


# ---- 3. pooled quantiles

@pytest.mark.parametrize("nbins,bits", [(16, 16), (8, 32)])
def test_pooled_quantiles(four, nbins, bits):
    cases, engs = four
    dpar, ddata, bands, comps, meta = cases[0]
    planes = th._hist_planes(comps)
    ranges = [(th._offset(l, w) - th.HALF, th._offset(l, w) + th.HALF) for l, w, k in planes]
    counts = (5, 7, 4)
    states = [th._synthetic_states(comps, meta, n, seed=3 + k, nbins=nbins) for k, n in enumerate(counts)]
    for e in engs:
        e.moments_begin(None)
        e.moments_hist(planes, ranges=ranges, nbins=nbins, bits=bits)
    samples = []
    for e, st, n in zip(engs[:3], states, counts):
        samples += th._feed([e], [(0, NPIX)], comps, st, n)
        th._feed([engs[3]], [(0, NPIX)], comps, st, n)                 # the fourth engine takes every sample of every chain
    assert engs[3].moments_count() == sum(counts)
    qs = (0.16, 0.5, 0.84)
    for r, plane in enumerate(planes):
        lo, hi = ranges[r]
        n_all, mode_all, q_all = (engs[3].moments_hist_stat(r, "n"), engs[3].moments_hist_stat(r, "mode"),
                                  engs[3].moments_hist_stat(r, "quantile", q=qs))
        n_p, mode_p, q_p = (da.chains_hist_stat(engs[:3], r, "n"), da.chains_hist_stat(engs[:3], r, "mode"),
                            da.chains_hist_stat(engs[:3], r, "quantile", q=qs))
        assert ts._same_bits(n_p, n_all) and ts._same_bits(mode_p, mode_all) and ts._same_bits(q_p, q_all), plane
        # the rule restated: the chains' counters summed as integers
        c = sum(e.moments_hist_get(r).astype(np.int64) for e in engs[:3])
        assert np.array_equal(c, th._ref_counts(th._series(samples, plane), lo, hi, nbins))
        assert np.array_equal(n_p, c.sum(axis=1).astype(np.float64))
        some = n_p > 0
        width = (np.float64(hi) - np.float64(lo)) / np.float64(nbins)
        assert np.array_equal(np.isnan(mode_p), ~some)
        assert np.array_equal(mode_p[some], (np.float64(lo) + width * (np.argmax(c, axis=1).astype(np.float64) + 0.5))[some])
        for j, q in enumerate(qs):
            val, _ = th._ref_quantile(c, lo, hi, q)
            assert np.array_equal(np.isnan(q_p[j]), ~some)
            assert (np.abs(q_p[j][some] - val[some]) <= 4 * EPS * max(abs(lo), abs(hi))).all(), (plane, q)
        assert some.sum() >= NPIX - 3 and (n_p[th.P_LO] == sum(counts))
    d = da.chains_hist_stat(engs[:3], 3, "quantile", q=qs, device=True)
    engs[0].synchronize()
    assert ts._same_bits(d.cpu().numpy(), da.chains_hist_stat(engs[:3], 3, "quantile", q=qs))


# ---- 4. and 5. a real run: four chains from dispersed starts, every statistic against the host, the signals too

def _disperse(eng, sign):
    """the sampled index planes shifted by sign * (1 prior sigma), inside the uniform prior"""
    for l, c in enumerate(eng.component_list):
        if not c.nindices or not any(c.sample_index):
            continue
        x = eng.get_indices(l)
        for j in range(c.nindices):
            if c.sample_index[j]:
                x[j] = np.clip(x[j] + sign * c.gauss_prior[j][1], c.uni_prior[j][0], c.uni_prior[j][1])
        eng.put_indices(l, x)


@pytest.fixture(scope="module")
def real_run(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    _engine(case)
    runs = [(dpar, ddata)] + [da.open_chain(dpar, ddata, 1234 + k) for k in (1, 2, 3)]
    assert [p.seed for p, _ in runs] == [1234, 1235, 1236, 1237] and dpar.seed == 1234
    for sign, (p, d) in zip((0, 1, -1, 1), runs):
        if sign:
            assert d.sig_map is ddata.sig_map and d.masks is ddata.masks and d.engine is not ddata.engine
            assert d.engine.pix0 == ddata.engine.pix0 and d.engine.npix_global == ddata.engine.npix_global
            _disperse(d.engine, sign)
    specs = None
    for p, d in runs:
        sel = da.moments_begin(p, d)
        pairs = da.moments_pairs(p, d)
        hist = da.moments_hist(p, d)
        specs = da.moments_signals(p, d)
    samples = [[] for _ in runs]
    signals = [{s: [] for s in specs} for _ in runs]
    for it in range(1, 10):
        for k, (p, d) in enumerate(runs):
            da.gibbs_iteration(p, d, it)
            da.moments_accumulate(d)
            samples[k].append(tp._snapshot(d.engine))
            for s, x in ts._host_samples(d.engine, specs).items():
                signals[k][s].append(x)
    return {"case": case, "runs": runs, "sel": sel, "pairs": pairs, "hist": hist, "specs": specs, "samples": samples, "signals": signals}


def test_a_real_run(real_run):
    runs, sel, pairs, samples = real_run["runs"], real_run["sel"], real_run["pairs"], real_run["samples"]
    engs = [d.engine for _, d in runs]
    comps = engs[0].component_list
    assert len(pairs) == 12 and any(c.type not in GLOBAL and any(c.sample_index) for c in comps if c.nindices)
    _check_planes(engs, sel, samples, "real run", min_finite=0.75)
    _check_pairs(engs, pairs, samples, "real run")
    # the four chains' states differ from each other
    last = [s[-1] for s in samples]
    for a in range(4):
        for b in range(a + 1, 4):
            assert any(not np.array_equal(last[a][l][0], last[b][l][0]) for l in last[a]), (a, b)
    # the pooled histograms: the rule restated on the samples of all chains
    h = engs[0]._moment_hist
    for r, plane in enumerate(real_run["hist"]):
        lo, hi = h["ranges"][r]
        c = th._ref_counts(np.concatenate([th._series(s, plane) for s in samples]), lo, hi, h["nbins"])
        assert np.array_equal(da.chains_hist_stat(engs, r, "n"), c.sum(axis=1).astype(np.float64))
        val, _ = th._ref_quantile(c, lo, hi, 0.5)
        med = da.chains_hist_stat(engs, r, "quantile", q=[0.5])[0]
        assert np.array_equal(np.isnan(med), np.isnan(val))
        assert (np.abs(med - val)[~np.isnan(val)] <= 4 * EPS * max(abs(lo), abs(hi))).all()
    # the maps by name carry the documented keys with the values of the thin getters
    chains = [d for _, d in runs]
    pm, single = da.chains_posterior_maps(chains, ddof=1), da.posterior_maps(chains[0])
    assert list(pm) == list(single)
    for key, e in pm.items():
        assert set(e) == {"n", "nchains", "mean", "std", "rhat", "W", "B", "ess"} and e["n"] == 9 and e["nchains"] == 4
    ld = [c.label for c in comps].index("dust")
    for stat in STATS:
        assert ts._same_bits(pm[("dust", "beta")][stat], da.chains_get(engs, ld, 1, stat, 1)), stat
    pp = da.chains_pair_maps(chains, "cov", ddof=1)
    assert list(pp) == list(da.posterior_pair_maps(chains[0])) and ts._same_bits(list(pp.values())[3], da.chains_get_pair(engs, 3, "cov", 1))
    qm = da.chains_quantile_maps(chains)
    assert list(qm) == list(da.posterior_quantile_maps(chains[0]))
    assert ts._same_bits(list(qm.values())[0]["q"], da.chains_hist_stat(engs, 0, "quantile", q=(0.16, 0.5, 0.84)))
    filled = da.chains_posterior_maps(chains, masked_value=-1.6375e30)
    m = np.asarray(runs[0][1].masks)[0] == 0
    assert m.any() and (filled[("dust", "beta")]["rhat"][:, m] == -1.6375e30).all()


def test_chain_zero_is_the_run_made_alone(real_run):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    da.moments_begin(dpar, ddata)
    for it in range(1, 10):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    alone, first = tp._snapshot(eng), real_run["samples"][0][-1]
    for l in alone:
        assert np.array_equal(alone[l][0], first[l][0])
        if alone[l][1] is not None:
            assert np.array_equal(alone[l][1], first[l][1])
    p0, p1 = da.posterior_maps(ddata), da.posterior_maps(real_run["runs"][0][1])
    for k in p0:
        assert ts._same_bits(p0[k]["mean"], p1[k]["mean"]) and ts._same_bits(p0[k]["std"], p1[k]["std"])


def test_signals_of_the_real_run(real_run):
    runs, specs, signals = real_run["runs"], real_run["specs"], real_run["signals"]
    engs = [d.engine for _, d in runs]
    assert any(k == 3 for _, _, k in specs) and len(specs) >= 4
    for s, spec in enumerate(specs):
        xs = [np.stack(sig[spec]) for sig in signals]
        with np.errstate(invalid="ignore"):
            big = np.max([np.abs(x).max(axis=0) for x in xs], axis=0)
        # a P sample restated on the host differs from the device's by up to 4 eps P (two rounded products, a rounded sum, a root)
        eta = 4 * EPS * big if spec[2] == 3 else 0.0 * big
        for ddof in (0, 1):
            pm = cr.pooled(xs, ddof)
            cr.compare(da.chains_get_signal(engs, s, "mean", ddof), pm["mean"][0], pm["mean"][1] + eta, "signal %s pooled mean" % (spec,))
            cr.compare(da.chains_get_signal(engs, s, "std", ddof), pm["std"][0], pm["std"][1] + 2 * eta, "signal %s pooled std" % (spec,))
        bw = cr.between(xs, eta=eta)
        for stat in ("W", "B"):
            cr.compare(da.chains_get_signal(engs, s, stat), *bw[stat], "signal %s %s" % (spec, stat))
        cr.compare_rhat(da.chains_get_signal(engs, s, "rhat"), bw, "signal %s R-hat^2" % (spec,))
    sm = da.chains_signal_maps([d for _, d in runs], ddof=1)
    assert list(sm) == list(da.posterior_signal_maps(runs[0][1]))
    e = list(sm.values())[-1]
    assert set(e) == {"n", "nchains", "mean", "std", "rhat", "W", "B"} and e["n"] == 9 and e["nchains"] == 4
    assert ts._same_bits(e["W"], da.chains_get_signal(engs, len(specs) - 1, "W", 1))
    with pytest.raises(da.DangxError, match="stat of a signal"):
        da.chains_get_signal(engs, 0, "ess")


# ---- 6. shards, alignment, determinism

def _every_map(chains):
    out = {}
    for key, e in da.chains_posterior_maps(chains, ddof=1).items():
        out.update({(key, stat): e[stat] for stat in STATS})
    out.update({(key, "corr"): v for key, v in da.chains_pair_maps(chains).items()})
    out.update({(key, "cov"): v for key, v in da.chains_pair_maps(chains, "cov", ddof=1).items()})
    for key, e in da.chains_quantile_maps(chains).items():
        out.update({(key, name): e[name] for name in ("q", "mode", "n")})
    return out


def _off_the_grid(dev):
    """a whole-sky C2 context whose state lives in caller buffers one double off the 16-byte grid (adopted before moments_begin:
    its accumulators take that phase, so a read-out over it and an ordinary chain has no common 16-byte phase)"""
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    keep = []
    for l, c in enumerate(comps):
        amp_old, idx_old = eng._adopted[l]
        abuf = torch.empty(amp_old.numel() + 1, dtype=torch.float64, device=dev)
        amp_new = abuf[1:].view(amp_old.shape)
        amp_new.copy_(amp_old)
        idx_new = None
        if idx_old is not None:
            ibuf = torch.empty(idx_old.numel() + 1, dtype=torch.float64, device=dev)
            idx_new = ibuf[1:].view(idx_old.shape)
            idx_new.copy_(idx_old)
        torch.cuda.synchronize()
        assert amp_new.data_ptr() % 16 == 8
        eng._chk(eng.lib.dangx_adopt_device_state(eng.h, l, ctypes.c_void_p(amp_new.data_ptr()),
                                                  ctypes.c_void_p(idx_new.data_ptr()) if idx_new is not None else None))
        eng._adopted[l] = (amp_new, idx_new)
        keep.append((amp_new, idx_new))
    return eng, keep


def test_shards_alignment_and_determinism(four):
    cases, engs = four
    whole = engs[:3]
    dpar, ddata, bands, comps, meta = cases[0]
    bounds = [0, 63, 130, meta["npix_global"]]        # odd lengths: planes off the 16-byte grid
    sharded = [shard_engines(cases[k], 3, bounds=bounds) for k in range(3)]
    odd, keep = _off_the_grid(torch.device("cuda", 0))
    moved = [whole[0], odd, whole[2]]
    n = 6
    planes = th._hist_planes(comps)
    ranges = [(th._offset(l, w) - th.HALF, th._offset(l, w) + th.HALF) for l, w, k in planes]
    states = [th._synthetic_states(comps, meta, n, seed=5 + k, nbins=16) for k in range(3)]
    for k in range(3):
        for group, bnds in (([whole[k]], [(0, NPIX)]), (sharded[k], list(zip(bounds[:-1], bounds[1:]))), ([odd] if k == 1 else [], [(0, NPIX)])):
            if not group:
                continue
            for e in group:
                e.moments_begin(None)
                e.moments_pairs(da.default_moment_pairs(dpar, comps, e._moment_sel), lag1=True)
                e.moments_hist(planes, ranges=ranges, nbins=16, bits=16)
            th._feed(group, bnds, comps, states[k], n)
    a, again = _every_map([[e] for e in whole]), _every_map([[e] for e in whole])
    b, c = _every_map(sharded), _every_map([[e] for e in moved])
    assert len(a) > 100 and any(np.isfinite(v).any() for v in a.values())
    for key, v in a.items():
        assert ts._same_bits(v, again[key]), ("two calls", key)
        assert ts._same_bits(v, b[key]), ("shards", key)
        assert ts._same_bits(v, c[key]), ("alignment", key)
    for stat in STATS:                                  # the device form writes the same bits
        d = da.chains_get(moved, 2, 1, stat, 1, device=True)
        moved[0].synchronize()
        assert ts._same_bits(d.cpu().numpy(), da.chains_get(whole, 2, 1, stat, 1)), stat
    d = da.chains_get_pair(sharded_col(sharded, 1), 5, "corr", device=True)
    sharded[0][1].synchronize()
    assert ts._same_bits(d.cpu().numpy(), da.chains_get_pair(whole, 5, "corr")[bounds[1]:bounds[2]])
    del keep


def sharded_col(sharded, s):
    return [chain[s] for chain in sharded]


# ---- 7. streams

def test_streams(built):
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    cases = [make_case("C2", nside=4) for _ in range(2)]
    engs = []
    for case, s in zip(cases, (s0, s1)):
        dpar, ddata, bands, comps, meta = case
        engs.append(da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0, stream=s.cuda_stream))
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 2, 2, 3, NPIX))          # [sample][chain][index][plane][pix]
    ld = 2                                               # dust: two indices
    for e in engs:
        e.moments_begin(None)
    for k, e in enumerate(engs):
        e.put_indices(ld, x[0][k])
        e.moments_accumulate()
    out = torch.full((3, NPIX), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    da.chains_get(engs, ld, 1, "mean", device=True, out=out)
    for k, e in enumerate(engs):                          # a further sample on both chains at once, behind the read-out
        e.put_indices(ld, x[1][k])
        e.moments_accumulate()
    torch.cuda.synchronize()
    first = x[0][0][0] + (x[0][1][0] - x[0][0][0]) * 0.5
    assert np.array_equal(out.cpu().numpy(), first)
    both = da.chains_get(engs, ld, 1, "mean")
    assert not np.array_equal(both, first) and engs[0].moments_count() == engs[1].moments_count() == 2


# ---- 8. nothing else moves

def _launches(eng):
    return {k: v["launches"] for k, v in eng.profile_get().items()}


def _accumulators(eng, npairs, nreg, nsig):
    out = {"state": tp._snapshot(eng)}
    sel = eng._moment_sel
    for l, c in enumerate(eng.component_list):
        for what in range(1 + c.nindices):
            if tp._planes(sel[l], what):
                for stat in ("mean", "std", "rho1"):
                    out[(l, what, stat)] = eng.moments_get(l, what, stat)
    for p in range(npairs):
        out[("pair", p)] = eng.moments_get_pair(p, "cov")
    for r in range(nreg):
        out[("hist", r)] = eng.moments_hist_get(r)
    for s in range(nsig):
        out[("sig", s)] = eng.moments_get_signal(s, "std")
    return out


def test_nothing_else_moves(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    _engine(case)
    runs = [(dpar, ddata), da.open_chain(dpar, ddata, 99)]
    for p, d in runs:
        d.engine.profile(True)
        da.moments_begin(p, d)
        pairs, hist, specs = da.moments_pairs(p, d), da.moments_hist(p, d), da.moments_signals(p, d)
    engs = [d.engine for _, d in runs]

    def step(it):
        before = [_launches(e) for e in engs]
        for p, d in runs:
            da.gibbs_iteration(p, d, it)
            da.moments_accumulate(d)
        after = [_launches(e) for e in engs]
        return [{k: a[k] - b.get(k, 0) for k in a} for a, b in zip(after, before)]

    step(1)
    base = step(2)
    assert all("k_chains" not in b and b["k_moments"] == 2 for b in base)
    held = [_accumulators(e, len(pairs), len(hist), len(specs)) for e in engs]
    mark = [_launches(e) for e in engs]
    nread = 0
    for stat in STATS:
        da.chains_get(engs, 2, 1, stat)
        nread += 1
    da.chains_get_pair(engs, 0, "corr")
    da.chains_hist_stat(engs, 0, "quantile", q=[0.5])
    da.chains_get_signal(engs, 0, "rhat")
    da.chains_get(engs, 2, 0, "rhat", device=True)
    nread += 4
    engs[0].synchronize()
    now = [_launches(e) for e in engs]
    assert now[0].pop("k_chains") == nread and "k_chains" not in now[1]        # under their own id, on the first chain's context
    assert now == mark                                                           # every other id as it was
    for e, h in zip(engs, held):
        g = _accumulators(e, len(pairs), len(hist), len(specs))
        assert g.keys() == h.keys()
        for key in h:
            if key == "state":
                for l in h[key]:
                    assert np.array_equal(h[key][l][0], g[key][l][0]) and (h[key][l][1] is None or np.array_equal(h[key][l][1], g[key][l][1]))
            else:
                assert ts._same_bits(np.asarray(h[key], dtype=np.float64), np.asarray(g[key], dtype=np.float64)), key
    again = step(3)
    for a, b in zip(again, base):
        a.pop("k_chains", None)
        assert a == b


# ---- 9. template rows

def test_template_rows(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    runs = [(dpar, ddata)] + [da.open_chain(dpar, ddata, 500 + k) for k in (1, 2)]
    for p, d in runs[1:]:
        assert d.sig_map is ddata.sig_map                     # the same HBM, adopted again
        assert d.engine._adopted and d.engine._adopted[1][0].data_ptr() != ddata.engine._adopted[1][0].data_ptr()
    lt = len(comps) - 1
    samples = [[] for _ in runs]
    for p, d in runs:
        sel = da.moments_begin(p, d)
        da.moments_pairs(p, d)
    for it in range(1, 7):
        for k, (p, d) in enumerate(runs):
            da.gibbs_iteration(p, d, it)
            da.moments_accumulate(d)
            samples[k].append(tp._snapshot(d.engine))
    engs = [d.engine for _, d in runs]
    assert np.std(np.stack([s[lt][0] for s in samples[1]]), axis=0)[1].max() > 0
    assert not np.array_equal(samples[0][-1][lt][0], samples[1][-1][lt][0])
    rh = _check_planes(engs, sel, samples, "template run")
    assert np.isfinite(rh[(lt, 0, 1)][[2, 3, 4]]).all()                           # the fitted bands
    ta = da.chains_get_template(engs, lt, "rhat", out=np.full((3, meta["nbands"]), 7.0))
    assert (ta[0] == 7.0).all()                                                   # the template has no row on T
    with pytest.raises(da.DangxError, match="dangx_chains_get_template"):
        da.chains_get(engs, lt, 0, "mean")
    with pytest.raises(da.DangxError, match="not a template"):
        da.chains_get_template(engs, 1, "mean")
    assert da.chains_posterior_maps([d for _, d in runs])[(comps[lt].label, "amplitude")]["rhat"].shape == (3, meta["nbands"])


# ---- 10. errors

def _refused(match, fn, *args, shape=(3, NPIX), **kw):
    """raises DangxError naming the cause and leaves the output untouched"""
    out = np.full(shape, 7.0)
    with pytest.raises(da.DangxError, match=match):
        fn(*args, out=out, **kw)
    assert (out == 7.0).all()


def test_errors(four):
    cases, engs = four
    dpar, ddata, bands, comps, meta = cases[0]
    a, b, c, d = engs
    ld = [cc.label for cc in comps].index("dust_P")
    sel = np.zeros(len(comps), dtype=np.int32)
    sel[1] = 1 | (1 << 3)                              # synch: amplitude and beta on T
    sel[ld] = (1 << 1) | (1 << (3 + 1))                # dust_P: amplitude and beta on Q
    good = [((1, 0, 0), (1, 1, 0))]

    def restart(e, sel=sel, pairs=good, lag1=True, hist=(1.0, 5.0, 16, 16), specs=((1, 0, 0),), n=2):
        e.moments_begin(sel)
        e.moments_pairs(pairs, lag1=lag1)
        e.moments_hist([(1, 1, 0)], ranges=[hist[:2]], nbins=hist[2], bits=hist[3])
        e.moments_signals(list(specs))
        for _ in range(n):
            e.moments_accumulate()

    for case, e in zip(cases, engs):                    # earlier tests planted non-finite samples: back to the cases' own states
        for l, cc in enumerate(case[3]):
            e.put_amplitude(l, cc.amplitude)
            if cc.nindices:
                e.put_indices(l, cc.indices)
    for e in (a, b, c):
        restart(e)
    assert np.isfinite(da.chains_get([a, b, c], 1, 0, "W")[0]).all()             # the set is fine as it stands
    _refused("nchains must be 2", da.chains_get, [a], 1, 0, "mean")
    _refused("nchains must be 2", da.chains_get, [a, b, c, d, a, b, c, d, a], 1, 0, "mean")
    _refused("chain 2 is the same context as chain 0", da.chains_get, [a, b, a], 1, 0, "mean")
    _refused("chain 1 is the same context as chain 0", da.chains_get_pair, [a, a], 0, "corr", shape=(NPIX,))
    sh = shard_engines(cases[3], 2)
    for e in sh:
        restart(e)
    _refused("chain 1 differs from chain 0 in npix / pix0 / nmaps", da.chains_get, [sh[0], sh[1]], 1, 0, "mean", shape=(3, NPIX // 2))
    _refused("chain 1 differs from chain 0 in npix / pix0 / nmaps", da.chains_get, [a, sh[0]], 1, 0, "mean")
    d.moments_end()
    _refused("chain 2: dangx_moments_begin was not called", da.chains_get, [a, b, d], 1, 0, "mean")
    restart(d, n=0)
    _refused("chain 1: no sample accumulated", da.chains_get, [a, d, b], 1, 0, "mean")
    _refused("chain 1: no sample accumulated", da.chains_hist_stat, [a, d], 0, "n", shape=(NPIX,))
    # a plane that some chain did not select
    other = sel.copy()
    other[ld] = 1 << 1
    restart(d, sel=other)
    _refused("chain 2: a plane of this component and what is not selected", da.chains_get, [a, b, d], ld, 1, "mean")
    _refused("chain 0: a plane of this component and what is not selected", da.chains_get, [a, b], 2, 0, "mean")
    assert np.isfinite(da.chains_get([a, b, d], ld, 0, "mean")[1]).all()
    # registrations that are not the same in every chain
    restart(d, pairs=[((1, 0, 0), (ld, 0, 1))])
    _refused("chain 1: pair 0 is not the registration of chain 0", da.chains_get_pair, [a, d], 0, "corr", shape=(NPIX,))
    _refused("pair index out of range", da.chains_get_pair, [a, b], 1, "corr", shape=(NPIX,))
    _refused("stat of a pair", da.chains_get_pair, [a, b], 0, 2, shape=(NPIX,))
    for hist in ((1.0, 5.5, 16, 16), (0.5, 5.0, 16, 16), (1.0, 5.0, 8, 16), (1.0, 5.0, 16, 32)):
        restart(d, hist=hist)
        _refused("chain 2: histogram registration 0 is not the registration of chain 0", da.chains_hist_stat, [a, b, d], 0, "n", shape=(NPIX,))
    _refused("histogram registration out of range", da.chains_hist_stat, [a, b], 1, "n", shape=(NPIX,))
    _refused("strictly inside", da.chains_hist_stat, [a, b], 0, "quantile", q=[0.5, 1.0], shape=(2, NPIX))
    restart(d, specs=((1, 1, 0),))
    _refused("chain 1: signal 0 is not the registration of chain 0", da.chains_get_signal, [a, d], 0, "mean", shape=(NPIX,))
    _refused("signal index out of range", da.chains_get_signal, [a, b], 1, "mean", shape=(NPIX,))
    # the counts
    restart(d, n=3)
    for stat in ("rhat", "W", "B"):
        _refused("equal sample counts: chain 2 holds 3, chain 0 holds 2", da.chains_get, [a, b, d], 1, 0, stat)
        _refused("equal sample counts", da.chains_get_signal, [a, d], 0, stat, shape=(NPIX,))
    assert np.isfinite(da.chains_get([a, b, d], 1, 0, "std", 1)[0]).all()
    restart(c, n=1)
    restart(d, n=1)
    _refused("at least 2 samples per chain", da.chains_get, [c, d], 1, 0, "rhat")
    _refused("needs 0 <= ddof < N", da.chains_get, [c, d], 1, 0, "std", 2)
    _refused("needs 0 <= ddof < N", da.chains_get_pair, [c, d], 0, "cov", 2, shape=(NPIX,))
    assert (da.chains_get([c, d], 1, 0, "std", 1)[0] == 0).all()                 # two equal samples
    # lag-1 missing in one chain
    restart(d, lag1=False)
    _refused("chain 1: the lag-1 autocorrelation is not tracked", da.chains_get, [a, d], 1, 0, "ess")
    _refused("stat must be 0", da.chains_get, [a, b], 1, 0, 6)
    _refused("what must be 0", da.chains_get, [a, b], 1, 3, "mean")
    _refused("component index out of range", da.chains_get, [a, b], len(comps), 0, "mean")
    # the device forms check the same way
    out = torch.full((3, NPIX), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(da.DangxError, match="chain 1: the lag-1"):
        da.chains_get([a, d], 1, 0, "ess", device=True, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all().item()
