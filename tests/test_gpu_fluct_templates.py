"""The textbook fluctuation term (fluct_mode='correct') in CG groups with fitted `template` members: the model of
tests/test_oracle_templates_cpu.py -- a Q/U template fitted at the last two bands in the Q+U group -- on C3 and C2.  The Schur
passes draw one normal per band for the diffuse rows; global row (template, band j) receives compute_rhs' row operator applied to
sigma_j * eta_j, from the same draws, on its natural row.  Groups with a monopole / hi_fit member and the CG solver stay refused."""
import copy

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L

from fluct_helpers import perturbed_data, unmasked
from test_oracle_templates_cpu import add_globals
from util import TOL_AMP, make_case, shard_engines

pytestmark = pytest.mark.gpu

CONFIGS = [("C3", 4), ("C2", 4)]


def _case(config, nside, which="template"):
    def tweak(dpar, ddata, bands, comps):
        nb = ddata.sig_map.shape[0]
        if which == "template":
            add_globals(dpar, ddata, bands, comps, ("template",), 2, fit_bands=[nb - 2, nb - 1])
        else:
            add_globals(dpar, ddata, bands, comps, ("monopole",), 1, fit_bands=[0, nb - 2, nb - 1])
    return make_case(config, nside=nside, start="truth", tweak=tweak)


def _engine(case, ddata=None):
    dpar, dd, bands, comps, meta = case
    return da.Engine(bands, copy.deepcopy(comps), dd if ddata is None else ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)


def _sweeps(comps, group, flag, it):
    return [(l, j, da.stream_id(it, 1, l, j, flag)) for l, c in enumerate(comps) for j in range(c.nindices)
            if c.cg_group == group and c.sample_index[j] and flag in c.pol_flag[j]]


@pytest.mark.parametrize("config,nside", CONFIGS)
def test_template_group_accepts_the_textbook_term(built, config, nside):
    case = _case(config, nside)
    eng = _engine(case)
    nullity, bad = eng.amp_sample(2, L.FLAG_QU, "sample", 5, 29, fluct_mode="correct")
    (resid, backward), nref = eng.schur_info()
    print("residual of the global rows %.3e (backward %.3e), %d refinement steps" % (resid, backward, nref))
    assert nullity == 0 and bad == 0
    assert resid <= 1e-12


@pytest.mark.parametrize("config,nside", CONFIGS)
def test_template_group_sample_is_the_optimize_solve_on_perturbed_data(built, config, nside):
    """amp_sample(correct) on d against amp_sample(optimize) of a second engine on d + sigma * eta: diffuse amplitudes to TOL_AMP of
    the map's maximum, template amplitudes to TOL_AMP of theirs (the bound for two evaluation orders of one solve)."""
    case = _case(config, nside)
    dpar, ddata, bands, comps, meta = case
    seed, stream = 5, 21 + L.FLAG_QU
    a, b = _engine(case), _engine(case, perturbed_data(ddata, [(L.FLAG_QU, stream)], seed, meta["pix0"]))
    assert a.amp_sample(2, L.FLAG_QU, "sample", seed, stream, fluct_mode="correct") == (0, 0)
    assert b.amp_sample(2, L.FLAG_QU, "optimize", seed, stream) == (0, 0)
    live = unmasked(ddata, L.FLAG_QU)
    worst = 0.0
    for l, c in enumerate(comps):
        if c.cg_group != 2:
            continue
        if c.type == "template":
            x, y = a.get_template_amplitudes(l), b.get_template_amplitudes(l)
            assert np.abs(y).max() > 0.0
            r = np.abs(x - y).max() / np.abs(y).max()
            print("template %d: %.3e of the largest amplitude" % (l, r))
            assert r <= TOL_AMP, (l, r)
        else:
            for k in (2, 3):
                x, y = a.get_amplitude(l)[k - 1, live], b.get_amplitude(l)[k - 1, live]
                assert np.abs(x - np.asarray(c.amplitude)[k - 1, live]).max() > 0.0
                r = np.abs(x - y).max() / np.abs(y).max()
                worst = max(worst, r)
                assert r <= TOL_AMP, (l, k, r)
    print("diffuse members: worst %.3e of the map's maximum" % worst)


def _assert_close(a, b, comps, tol_amp, tol_idx, what):
    for l, c in enumerate(comps):
        x, y = a.get_amplitude(l), b.get_amplitude(l)
        assert np.abs(x - y).max() <= tol_amp * max(np.abs(y).max(), 1e-30), (what, l)
        if c.nindices:
            assert np.abs(a.get_indices(l) - b.get_indices(l)).max() <= tol_idx, (what, l)
        if c.type == "template":
            x, y = a.get_template_amplitudes(l), b.get_template_amplitudes(l)
            assert np.abs(x - y).max() <= tol_amp * max(np.abs(y).max(), 1e-30), (what, l)


@pytest.mark.parametrize("config,nside", CONFIGS)
def test_one_call_form_is_the_two_calls(built, config, nside):
    """plane_set_sample(correct) == amp_sample(correct) followed by plane_sweeps_sample, on both groups, two iterations:
    amplitudes 1e-10 of the maximum, indices 1e-12, accepted counts equal."""
    case = _case(config, nside)
    dpar, ddata, bands, comps, meta = case
    one, two = _engine(case), _engine(case)
    for it in (2, 3):
        for g in dpar.cg_groups:
            f = g.pol_flag[0]
            sw = _sweeps(comps, g.cg_group, f, it)
            s = da.stream_id(it, 0, g.cg_group, 0, f)
            bad, acc = one.plane_set_sample(g.cg_group, f, "sample", dpar.seed, s, sw, dpar.nsample, dpar.seed, fluct_mode="correct")
            _, bad2 = two.amp_sample(g.cg_group, f, "sample", dpar.seed, s, fluct_mode="correct")
            acc2 = two.plane_sweeps_sample(f, sw, dpar.nsample, "sample", dpar.seed)
            assert bad == bad2 == 0 and acc == acc2, (it, g.cg_group, acc, acc2)
        _assert_close(one, two, comps, 1e-10, 1e-12, "one call / two calls, iteration %d" % it)


@pytest.mark.parametrize("config,nside", CONFIGS)
def test_template_group_over_three_contexts(built, config, nside):
    """Three pixel-shard contexts share the Schur rows (and the fluctuation sums of the global rows): the state of one context on
    the whole sky to 1e-9."""
    case = _case(config, nside)
    dpar, ddata, bands, comps, meta = case
    whole = _engine(case)
    engs = shard_engines(case, 3)
    bounds = [e.pix0 for e in engs] + [meta["npix"]]
    for it in (2, 3):
        for g in dpar.cg_groups:
            f = g.pol_flag[0]
            sw = _sweeps(comps, g.cg_group, f, it)
            s = da.stream_id(it, 0, g.cg_group, 0, f)
            bad, _ = whole.plane_set_sample(g.cg_group, f, "sample", dpar.seed, s, sw, dpar.nsample, dpar.seed, fluct_mode="correct")
            nul, bad3, _ = da.sky_plane_set_sample(engs, g.cg_group, f, "sample", dpar.seed, s, sw, dpar.nsample, dpar.seed, fluct_mode="correct")
            assert (nul, bad3) == (0, bad) and bad == 0
    for l, c in enumerate(comps):
        full = whole.get_amplitude(l)
        for q, e in enumerate(engs):
            part = e.get_amplitude(l)
            assert np.abs(part - full[:, bounds[q]:bounds[q + 1]]).max() <= 1e-9 * max(np.abs(full).max(), 1e-30), (l, q)
            if c.nindices:
                assert np.abs(e.get_indices(l) - whole.get_indices(l)[:, :, bounds[q]:bounds[q + 1]]).max() <= 1e-9, (l, q)
            if c.type == "template":
                ta = whole.get_template_amplitudes(l)
                assert np.abs(e.get_template_amplitudes(l) - ta).max() <= 1e-9 * np.abs(ta).max(), (l, q)


def test_what_stays_refused(built):
    """A group with a monopole member, and the CG solver, refuse the textbook term and say so."""
    eng = _engine(_case("C2", 4, "monopole"))
    with pytest.raises(da.DangxError, match="monopole"):
        eng.amp_sample(1, L.FLAG_T, "sample", 5, 7, fluct_mode="correct")
    with pytest.raises(da.DangxError, match="monopole"):
        eng.plane_set_sample(1, L.FLAG_T, "sample", 5, 7, [(1, 0, 9)], 3, 5, fluct_mode="correct")
    eng.amp_sample(1, L.FLAG_T, "sample", 5, 7)                              # the reference's term still runs
    for e, group, flag in ((eng, 2, L.FLAG_QU), (_engine(_case("C2", 4)), 2, L.FLAG_QU), (_engine(_case("C2", 4)), 1, L.FLAG_T)):
        with pytest.raises(da.DangxError, match="DANGX_SOLVER_CG"):
            e.amp_sample(group, flag, "sample", 5, 7, solver="cg", fluct_mode="correct")
