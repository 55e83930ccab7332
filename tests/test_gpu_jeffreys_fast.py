"""The Jeffreys prior of the synchrotron index (eval_jeffreys_prior, src/dang_lnl_mod.f90:242-304) on the register chain, the
fused solve + sweep and the plane-set launch: power law labelled 'synch', delta bands, chisq likelihood, per-pixel mode.
Every model is a tests/util.make_case one with the synchrotron components on prior_type 'jeffreys' and the polarisation set
relabelled 'synch' (synth.make_sky suffixes it; only the exact label has a non-trivial prior).  Nothing in Engine keys on
unique labels (the per-index statistics dictionaries are keyed by label, which no test here reads)."""
import copy

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L

from util import MAPN, TOL_AMP, TOL_INDEX, make_case, pair, shard_engines

pytestmark = pytest.mark.gpu


def _jeffreys(dpar, ddata, bands, comps):
    for c in comps:
        if c.label in ("synch", "synch_P"):
            c.label = "synch"
            c.prior_type = ["jeffreys"] * c.nindices


def _tight(dpar, ddata, bands, comps):
    """uniform bounds at +-1.5 sigma of the prior around its mean: out-of-bounds proposals occur"""
    _jeffreys(dpar, ddata, bands, comps)
    for c in comps:
        if c.label == "synch":
            m, s = c.gauss_prior[0]
            c.uni_prior = [[m - 1.5 * s, m + 1.5 * s]]
            c.indices[0] = np.clip(c.indices[0], m - 1.4 * s, m + 1.4 * s)


def _engines(case):
    dpar, ddata, bands, comps, meta = case
    return [da.Engine(bands, copy.deepcopy(comps), ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0) for _ in range(2)]


def _sweeps(comps, group, flag, it):
    return [(l, j, da.stream_id(it, 1, l, j, flag)) for l, c in enumerate(comps) for j in range(c.nindices)
            if c.cg_group == group and c.sample_index[j] and flag in c.pol_flag[j]]


def _synch(comps, group):
    return next(l for l, c in enumerate(comps) if c.label == "synch" and c.cg_group == group)


def _iterations(case, its, ml_mode):
    """Gibbs iterations through Engine.plane_set_sample against the oracle's loop in the reference's order (every solve, then
    every sweep): accepted counts equal per sweep; afterwards indices, amplitudes and chi^2."""
    dpar, ddata, bands, comps, meta = case
    eng, orc = pair(case)
    nmaps = meta["nmaps"]
    for it in its:
        got = {}
        for g in dpar.cg_groups:
            f = g.pol_flag[0]
            sw = _sweeps(comps, g.cg_group, f, it)
            bad, accs = eng.plane_set_sample(g.cg_group, f, ml_mode, dpar.seed, da.stream_id(it, 0, g.cg_group, 0, f), sw, dpar.nsample, dpar.seed)
            assert bad == 0
            for (l, j, _), a in zip(sw, accs):
                got[(l, j, f)] = a
        for g in dpar.cg_groups:
            f = g.pol_flag[0]
            orc.amp_sample_direct(g.cg_group, f, ml_mode, dpar.seed, da.stream_id(it, 0, g.cg_group, 0, f), "reference")
        for l, c in enumerate(comps):
            for j in range(c.nindices):
                if c.sample_index[j]:
                    f = c.pol_flag[j][0]
                    o = orc.sample_index_mh(l, j, MAPN[f], dpar.nsample, ml_mode, dpar.seed, da.stream_id(it, 1, l, j, f))
                    assert got[(l, j, f)] == o, (it, l, j, got[(l, j, f)], o)
    for l, c in enumerate(comps):
        a, b = eng.get_amplitude(l), orc.amplitude(l)
        assert np.abs(a - b).max() <= TOL_AMP * max(np.abs(b).max(), 1e-30), l
        if c.nindices:
            d = np.abs(eng.get_indices(l) - orc.indices(l)).max()
            print("component %d: max index difference %.3e" % (l, d))
            assert d <= TOL_INDEX, (l, d)
    ochi, _ = orc.chisq(1, nmaps, 1.0)
    chi = eng.chisq_current(1, nmaps) / meta["nbands"]
    assert abs(chi - ochi) <= 1e-8 * ochi, (chi, ochi)
    return eng


def test_jeffreys_iteration_is_one_launch_per_plane_set(built):
    """C3 with both synchrotron components on the Jeffreys prior: an iteration is the two plane-set launches and the chi^2
    reductions, as for the gaussian model (test_gpu_round4.py::test_plane_set_launches_stay_under_band_calibration) -- no
    stand-alone sweep, no LDS-form chain.  (Before the register chain carried the prior the synchrotron sweeps ran as
    k_index_mh launches and each plane set fell back to one launch per step.)"""
    case = make_case("C3", nside=8, start="truth", tweak=_jeffreys)
    dpar, ddata, bands, comps, meta = case
    eng, _ = pair(case)
    for it in (2, 3):
        eng.profile(True)
        da.gibbs_iteration(dpar, ddata, it)
        prof = eng.profile_get()
        eng.profile(False)
        assert set(prof) <= {"k_amp_index", "k_reduce"} and prof["k_amp_index"]["launches"] == 2, prof
        assert "k_index_mh" not in prof, prof
    assert eng.rtc_kernels() == []      # the C3 shape is built in


@pytest.mark.parametrize("ml_mode", ["sample", "optimize"])
@pytest.mark.parametrize("config,nbands", [("C3", None), ("C1", None), ("C2", 7)])
def test_jeffreys_iterations_match_the_oracle(built, ml_mode, config, nbands):
    """Three whole iterations against the oracle: C3 (built in), C1 (3 bands, one plane) and C2 with 7 bands (specialised at run
    time: the item code of the synchrotron sweep is CH_POW + 16 = 17)."""
    kw = dict(nbands=nbands) if nbands else {}
    case = make_case(config, nside=8, start="truth", tweak=_jeffreys, **kw)
    eng = _iterations(case, (1, 2, 3), ml_mode)
    names = eng.rtc_kernels()
    if config == "C2":
        for sp in (1, 2):
            assert "dxk::k_plane_set<%d, 7, 3, 1, 1, 17, 10, 0, 0, 0>" % sp in names, names
    if config == "C1":
        assert "dxk::k_plane_set<1, 3, 2, 1, 1, 17, 10, 0, 0, 0>" in names, names


@pytest.mark.parametrize("group,flag", [(1, L.FLAG_T), (2, L.FLAG_QU)])
def test_jeffreys_sweep_and_fused_entry(built, group, flag):
    """C3 at Nside 4 with tight uniform bounds.  The stand-alone sweep against the oracle (register kernel, not the LDS form);
    amp_index_sample == amp_sample + index_sample and the plane-set launch == the separate launches, bit for bit."""
    case = make_case("C3", nside=4, start="truth", tweak=_tight)
    dpar, ddata, bands, comps, meta = case
    ls = _synch(comps, group)
    eng, orc = pair(case)
    acc = eng.index_sample(ls, 0, MAPN[flag], 10, "sample", 7, 31)
    assert acc == orc.sample_index_mh(ls, 0, MAPN[flag], 10, "sample", 7, 31)
    assert np.abs(eng.get_indices(ls) - orc.indices(ls)).max() <= TOL_INDEX
    # the profile has one bucket for the register and the LDS form of a sweep; which one ran shows where the kernel is specialised
    # at run time: the same sweep on 9 bands
    e9, o9 = pair(make_case("C3", nside=4, nbands=9, start="truth", tweak=_tight))
    assert e9.index_sample(ls, 0, MAPN[flag], 10, "sample", 7, 31) == o9.sample_index_mh(ls, 0, MAPN[flag], 10, "sample", 7, 31)
    assert np.abs(e9.get_indices(ls) - o9.indices(ls)).max() <= TOL_INDEX
    assert e9.rtc_kernels() == ["dxk::k_index_mh_reg<1, %d, 9, 1, true>" % (1 if flag == L.FLAG_T else 2)], e9.rtc_kernels()
    lo, hi = comps[ls].uni_prior[0]
    v = eng.get_indices(ls)[0]
    assert ((v >= lo) & (v <= hi))[:, ddata.masks[0] != 0].all()
    # --- fused entry against the two calls
    fus, two = _engines(case)
    for it in (1, 2):
        sa, si = da.stream_id(it, 0, group, 0, flag), da.stream_id(it, 1, ls, 0, flag)
        fus.profile(True)
        bad_f, acc_f = fus.amp_index_sample(group, flag, "sample", 11, sa, ls, 0, MAPN[flag], 10, 11, si)
        assert "k_amp_index" in fus.profile_get()
        fus.profile(False)
        _, bad_t = two.amp_sample(group, flag, "sample", 11, sa)
        acc_t = two.index_sample(ls, 0, MAPN[flag], 10, "sample", 11, si)
        assert (bad_f, acc_f) == (bad_t, acc_t)
        for l, c in enumerate(comps):
            assert np.array_equal(fus.get_amplitude(l), two.get_amplitude(l)), (it, l)
            if c.nindices:
                assert np.array_equal(fus.get_indices(l), two.get_indices(l)), (it, l)
        s1, s2 = (1, 1) if flag == L.FLAG_T else (2, 3)
        for which in (0, 1):
            assert fus.chisq_cached(which, s1, s2) == two.chisq_cached(which, s1, s2), (it, which)
    # --- the plane-set launch against the separate launches: the same maps bit for bit (same proposals, same accept decisions),
    # as test_gpu_fused.py::test_plane_set_entry_is_the_separate_calls_where_the_kernel_does_not_apply asks of the gaussian model
    ps, sep = _engines(case)
    sw = _sweeps(comps, group, flag, 2)
    ps.profile(True)
    _, accs = ps.plane_set_sample(group, flag, "sample", 11, 5, sw, 10, 11)
    assert set(ps.profile_get()) <= {"k_amp_index", "k_reduce"}
    ps.profile(False)
    sep.amp_sample(group, flag, "sample", 11, 5)
    accs_sep = [sep.index_sample(l, j, MAPN[flag], 10, "sample", 11, st) for l, j, st in sw]
    assert list(accs) == accs_sep
    for l, c in enumerate(comps):
        assert np.array_equal(ps.get_amplitude(l), sep.get_amplitude(l)), l
        if c.nindices:
            assert np.array_equal(ps.get_indices(l), sep.get_indices(l)), l


def test_jeffreys_lane_pairs(built):
    """C5 at Nside 4: 20 bands, the Q+U chains as lane pairs (the prior's sum crosses the pair like the likelihood's)."""
    eng = _iterations(make_case("C5", nside=4, start="truth", tweak=_jeffreys), (1, 2), "sample")
    assert any(n.startswith("dxk::k_plane_set<2, 20, 6, 2, 1, 17,") for n in eng.rtc_kernels()), eng.rtc_kernels()


@pytest.mark.parametrize("ml_mode", ["sample", "optimize"])
def test_jeffreys_nan_rule(built, ml_mode):
    """The reference divides by c%amplitude(i, k): where it is exactly 0 on a swept plane the prior is NaN, every diff is NaN and
    no proposal is accepted, in both modes.  Three unmasked pixels of T, three of Q only (U non-zero)."""
    picks = {}

    def tweak(dpar, ddata, bands, comps):
        _jeffreys(dpar, ddata, bands, comps)
        live = np.flatnonzero(ddata.masks[0] != 0)
        picks["T"], picks["Q"] = live[[1, 70, -2]], live[[3, 50, -5]]
        for c in comps:
            if c.label == "synch":
                if c.cg_group == 1:
                    c.amplitude[0, picks["T"]] = 0.0
                else:
                    c.amplitude[1, picks["Q"]] = 0.0
                    assert (c.amplitude[2, picks["Q"]] != 0.0).all()

    case = make_case("C3", nside=4, start="truth", tweak=tweak)
    dpar, ddata, bands, comps, meta = case
    eng, orc = pair(case)
    for group, flag, key in ((1, L.FLAG_T, "T"), (2, L.FLAG_QU, "Q")):
        ls = _synch(comps, group)
        start = comps[ls].indices.copy()
        acc = eng.index_sample(ls, 0, MAPN[flag], 10, ml_mode, 9, 77)
        assert acc == orc.sample_index_mh(ls, 0, MAPN[flag], 10, ml_mode, 9, 77)
        got, ref = eng.get_indices(ls), orc.indices(ls)
        planes = [0] if flag == L.FLAG_T else [1, 2]
        for k in planes:
            assert np.array_equal(got[0, k, picks[key]], start[0, planes[0], picks[key]]), (key, k)
        assert np.abs(got - ref).max() <= TOL_INDEX
        assert acc > 0


def test_jeffreys_shards_equal_one_context(built):
    """C3 at Nside 8 as two pixel-shard contexts, two iterations: bit-equal to the one-context maps."""
    case = make_case("C3", nside=8, start="truth", tweak=_jeffreys)
    dpar, ddata, bands, comps, meta = case
    one = da.Engine(bands, copy.deepcopy(comps), ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    engs = shard_engines(case, 2)
    for it in (2, 3):
        for g in dpar.cg_groups:
            f = g.pol_flag[0]
            sw = _sweeps(comps, g.cg_group, f, it)
            sa = da.stream_id(it, 0, g.cg_group, 0, f)
            for e in [one] + engs:
                e.plane_set_sample(g.cg_group, f, "sample", dpar.seed, sa, sw, dpar.nsample, dpar.seed)
    for l, c in enumerate(comps):
        assert np.array_equal(one.get_amplitude(l), np.concatenate([e.get_amplitude(l) for e in engs], axis=-1)), l
        if c.nindices:
            assert np.array_equal(one.get_indices(l), np.concatenate([e.get_indices(l) for e in engs], axis=-1)), l
