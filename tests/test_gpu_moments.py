"""Posterior moments accumulated on the device (dangx_moments_*): against np.mean / np.std of the same samples pulled to the host,
the selection, the chain left as it is, determinism and shard independence, the device getter, the error cases and the profile."""
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


def _engine(case):
    dpar, ddata, bands, comps, meta = case
    return da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)


def _snapshot(eng):
    """The chain state as the host sees it: {l: amplitude [nmaps][npix] or template amplitudes [nmaps][nbands], indices or None}."""
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


def _check_moments(eng, sel, samples, ddofs=(0, 1)):
    """Device mean / std of every selected plane against np.mean / np.std of the stacked host samples.  Tolerances: the mean of
    n samples by Welford's update is within ~2 n eps max|x| of the exact one (one rounding per step, each at most eps times the
    running mean's size), np.mean within log2(n) eps max|x|: 8 n eps max|x| bounds their difference.  The standard deviation's
    error is bounded by the rounding of the deviations d = x - mean (eps max|x| each, n of them) and of the sums of their squares
    (n eps s): 16 n eps (s + max|x|), i.e. ~1e-12 relative for the index and amplitude maps here."""
    n = len(samples)
    assert eng.moments_count() == n
    for l, c in enumerate(eng.component_list):
        for what in range(1 + c.nindices):
            ks = _planes(sel[l], what)
            if not ks:
                continue
            if what == 0:
                xs = np.stack([s[l][0] for s in samples])
            else:
                xs = np.stack([s[l][1][what - 1] for s in samples])
            big = np.abs(xs).max(axis=0)
            ref_m = np.mean(xs, axis=0)
            if what == 0 and c.type in GLOBAL:
                dev_m = eng.moments_get_template(l, "mean")
            else:
                dev_m = eng.moments_get(l, what, "mean")
            for k in ks:
                err = np.abs(dev_m[k] - ref_m[k])
                assert (err <= 8 * n * EPS * big[k] + 1e-300).all(), (c.label, what, k, err.max())
            for ddof in ddofs:
                if n - ddof <= 0:
                    continue
                ref_s = np.std(xs, axis=0, ddof=ddof)
                if what == 0 and c.type in GLOBAL:
                    dev_s = eng.moments_get_template(l, "std", ddof)
                else:
                    dev_s = eng.moments_get(l, what, "std", ddof)
                for k in ks:
                    err = np.abs(dev_s[k] - ref_s[k])
                    tol = 16 * n * EPS * (ref_s[k] + big[k]) + 1e-300
                    assert (err <= tol).all(), (c.label, what, k, ddof, (err / tol).max())


def test_moments_match_host_samples(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    sel = da.moments_begin(dpar, ddata)
    samples = []
    for it in range(1, 10):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(_snapshot(eng))
    # the samples really move: a constant chain would not test the update
    assert np.std(np.stack([s[1][1] for s in samples]), axis=0).max() > 0
    _check_moments(eng, sel, samples)
    # n = 1 gives the sample itself and zero spread, exactly
    eng.moments_begin(sel)
    eng.moments_accumulate()
    one = _snapshot(eng)
    for l, c in enumerate(comps):
        if c.nindices:
            k = _planes(sel[l], 1)
            if k:
                assert np.array_equal(eng.moments_get(l, 1, "mean")[k], one[l][1][0][k])
                assert not eng.moments_get(l, 1, "std")[k].any()


def test_moments_of_template_amplitudes(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 3, 4), amplitudes=(3.0, -2.0, 5.0))
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    sel = da.moments_begin(dpar, ddata)
    lt, lm = len(comps) - 2, len(comps) - 1
    assert sel[lt] == 0b110 and sel[lm] == 0b001
    samples = []
    for it in range(1, 10):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        samples.append(_snapshot(eng))
    assert np.std(np.stack([s[lt][0] for s in samples]), axis=0)[1].max() > 0
    _check_moments(eng, sel, samples)
    # the rows that are not selected are left as they were
    ta = eng.moments_get_template(lm, "mean", out=np.full((3, meta["nbands"]), 7.0))
    assert (ta[1:] == 7.0).all()


def test_burn_in_and_thinning(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    burn, thin = 3, 2
    samples, sel = [], None
    for it in range(1, 12):
        da.gibbs_iteration(dpar, ddata, it)
        if it == burn:
            sel = da.moments_begin(dpar, ddata)
        if it > burn and (it - burn) % thin == 0:
            da.moments_accumulate(ddata)
            samples.append(_snapshot(eng))
    assert eng.moments_count() == len(samples) == 4
    _check_moments(eng, sel, samples)


def test_selection_leaves_other_planes_untouched(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    ld = [c.label for c in comps].index("dust_P")
    sel = np.zeros(len(comps), dtype=np.int32)
    sel[ld] = (1 << 1) | (1 << (3 + 3 * 1 + 2))     # amplitude Q, index 2 (T) on U
    eng.moments_begin(sel)
    for it in (1, 2, 3):
        da.gibbs_iteration(dpar, ddata, it)
        eng.moments_accumulate()
    sentinel = -12345.5
    a = eng.moments_get(ld, 0, "mean", out=np.full((3, meta["npix"]), sentinel))
    assert (a[[0, 2]] == sentinel).all() and (a[1] != sentinel).all()
    t = eng.moments_get(ld, 2, "std", out=np.full((3, meta["npix"]), sentinel))
    assert (t[:2] == sentinel).all() and (t[2] != sentinel).all()
    with pytest.raises(da.DangxError, match="nothing selected"):
        eng.moments_get(ld, 1, "mean")                  # index 1 (beta): nothing selected
    with pytest.raises(da.DangxError, match="nothing selected"):
        eng.moments_get(0, 0, "mean")                   # another component
    bad = sel.copy()
    bad[0] = 1 << 3                                      # the CMB has no index
    with pytest.raises(da.DangxError, match="does not have"):
        eng.moments_begin(bad)


def _run(case, nit, accumulate):
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    if accumulate:
        da.moments_begin(dpar, ddata, sel=None)
    for it in range(1, nit + 1):
        da.gibbs_iteration(dpar, ddata, it)
        if accumulate:
            da.moments_accumulate(ddata)
    return eng, _snapshot(eng), ddata.chisq


def test_chain_is_not_perturbed(built):
    e1, s1, chi1 = _run(make_case("C2", nside=4), 5, accumulate=True)
    e2, s2, chi2 = _run(make_case("C2", nside=4), 5, accumulate=False)
    assert chi1 == chi2
    for l in s1:
        assert np.array_equal(s1[l][0], s2[l][0])
        if s1[l][1] is not None:
            assert np.array_equal(s1[l][1], s2[l][1])
    assert e1.moments_count() == 5


def _all_moments(eng):
    out = {}
    sel = eng._moment_sel
    for l, c in enumerate(eng.component_list):
        for what in range(1 + c.nindices):
            if _planes(sel[l], what):
                for stat in ("mean", "std"):
                    out[(l, what, stat)] = eng.moments_get(l, what, stat)
    return out


def test_deterministic_and_shard_independent(built):
    e1, _, _ = _run(make_case("C2", nside=4), 4, accumulate=True)
    e2, _, _ = _run(make_case("C2", nside=4), 4, accumulate=True)
    m1, m2 = _all_moments(e1), _all_moments(e2)
    assert m1.keys() == m2.keys() and all(np.array_equal(m1[k], m2[k]) for k in m1)
    # one context and three pixel shards (odd lengths: planes that start off the 16-byte grid) fed the same states
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    whole = _engine(case)
    bounds = [0, 63, 130, meta["npix_global"]]
    shards = shard_engines(case, 3, bounds=bounds)
    for e in [whole] + shards:
        e.moments_begin(None)
    rng = np.random.default_rng(5)
    for _ in range(5):
        for l, c in enumerate(comps):
            a = rng.standard_normal((3, meta["npix"])) * 10.0
            whole.put_amplitude(l, a)
            for e, b0, b1 in zip(shards, bounds[:-1], bounds[1:]):
                e.put_amplitude(l, a[:, b0:b1])
            if c.nindices:
                x = rng.uniform(-3.0, 20.0, size=(c.nindices, 3, meta["npix"]))
                whole.put_indices(l, x)
                for e, b0, b1 in zip(shards, bounds[:-1], bounds[1:]):
                    e.put_indices(l, x[:, :, b0:b1])
        for e in [whole] + shards:
            e.moments_accumulate()
    mw = _all_moments(whole)
    ms = [_all_moments(e) for e in shards]
    for k, v in mw.items():
        assert np.array_equal(v, np.concatenate([m[k] for m in ms], axis=-1)), k
    # posterior_maps over the shard contexts: the same maps side by side
    pw = da.posterior_maps(ddata, engines=[whole])
    ps = da.posterior_maps(ddata, engines=shards)
    assert pw.keys() == ps.keys()
    for k in pw:
        assert np.array_equal(pw[k]["mean"], ps[k]["mean"]) and np.array_equal(pw[k]["std"], ps[k]["std"]) and ps[k]["n"] == 5
    shards[0].moments_accumulate()
    with pytest.raises(da.DangxError, match="different sample counts"):
        da.posterior_maps(ddata, engines=shards)


def test_device_getter_and_adopted_buffers(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    assert eng._adopted
    sel = da.moments_begin(dpar, ddata)
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
    assert not torch.equal(idx_new, idx_old)       # the chain went on in the new buffers
    _check_moments(eng, sel, samples)
    for l, c in enumerate(comps):
        for what in range(1 + c.nindices):
            if not _planes(sel[l], what) or (what == 0 and c.type in GLOBAL):
                continue
            for stat, ddof in (("mean", 0), ("std", 0), ("std", 1)):
                h = eng.moments_get(l, what, stat, ddof)
                d = eng.moments_get(l, what, stat, ddof, device=True)
                assert d.is_cuda and np.array_equal(d.cpu().numpy(), h), (c.label, what, stat, ddof)


def test_errors(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    with pytest.raises(da.DangxError, match="begin"):
        eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="begin"):
        eng.moments_get(1, 0, "mean")
    eng.moments_begin(None)
    with pytest.raises(da.DangxError, match="no sample"):
        eng.moments_get(1, 0, "mean")
    eng.moments_accumulate()
    eng.moments_accumulate()
    assert eng.moments_count() == 2
    eng.moments_get(1, 0, "std", ddof=1)
    with pytest.raises(da.DangxError, match="ddof"):
        eng.moments_get(1, 0, "std", ddof=2)
    with pytest.raises(da.DangxError, match="out of range"):
        eng.moments_get(len(comps), 0, "mean")
    with pytest.raises(da.DangxError, match="what"):
        eng.moments_get(1, 3, "mean")
    with pytest.raises(da.DangxError, match="nothing selected"):
        eng.moments_get(1, 2, "mean")                    # synchrotron has one index
    # dust becomes a one-index component: its accumulators no longer fit
    ld = [c.label for c in comps].index("dust")
    c2 = da.DangComps(**{**comps[ld].__dict__})
    c2.type, c2.nindices = "power-law", 1
    for q in ("ind_label", "sample_index", "index_mode", "lnl_type", "prior_type", "gauss_prior", "uni_prior", "step_size", "pol_flag"):
        setattr(c2, q, list(getattr(c2, q))[:1])
    eng.set_component(ld, c2)
    with pytest.raises(da.DangxError, match="changed type or nindices"):
        eng.moments_accumulate()
    assert eng.moments_count() == 2
    eng.moments_end()
    with pytest.raises(da.DangxError, match="begin"):
        eng.moments_count()


def test_profile_family(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    eng.profile(True)
    for it in (1, 2):
        da.gibbs_iteration(dpar, ddata, it)
    assert "k_moments" not in eng.profile_get()
    da.moments_begin(dpar, ddata)
    for it in (3, 4, 5):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    prof = eng.profile_get()
    assert prof["k_moments"]["launches"] == 3 and prof["k_moments"]["total_ms"] > 0
