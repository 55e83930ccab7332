"""The certified cheap likelihood of the register chains (dang_amd/csrc/dx_chain.h: RegChain::lnl_cheap / cheap_bound) on skies
that push many proposals into its exact branch: the noise scaled down by up to 1e4 (signal to noise 1e5 and more, so the
bound, which grows with |a s / sigma|, is wide), and proposal bounds that reach an exponent outside the fp32 range (every
proposal exact).  The chains must still decide as the oracle's fp64 chain: index maps within 1e-12, accepted counts equal."""
import numpy as np
import pytest

import dang_amd as da

from util import MAPN, assert_amps_close, assert_indices_close, make_case, pair

pytestmark = pytest.mark.gpu


def _sharpen(scale):
    def tweak(dpar, ddata, bands, comps):
        ddata.rms_map = np.ascontiguousarray(ddata.rms_map * scale)
    return tweak


def _wide_bounds(dpar, ddata, bands, comps):
    for c in comps:
        if c.type == "power-law":
            c.uni_prior = [[-60.0, 40.0]]          # |beta ln(nu/nu_ref)| log2e > 125 at 857 GHz: the exact form throughout


def _iterations(case, n):
    dpar, ddata, bands, comps, meta = case
    eng, orc = pair(case)
    for it in range(1, n + 1):
        for g in dpar.cg_groups:
            for f in g.pol_flag:
                s = da.stream_id(it, 0, g.cg_group, 0, f)
                _, bad = eng.amp_sample(g.cg_group, f, "sample", dpar.seed, s)
                assert bad == orc.amp_sample_direct(g.cg_group, f, "sample", dpar.seed, s, "reference")
        for l, c in enumerate(comps):
            for j in range(c.nindices):
                if c.sample_index[j]:
                    for f in c.pol_flag[j]:
                        s = da.stream_id(it, 1, l, j, f)
                        ag = eng.index_sample(l, j, MAPN[f], dpar.nsample, "sample", dpar.seed, s)
                        assert ag == orc.sample_index_mh(l, j, MAPN[f], dpar.nsample, "sample", dpar.seed, s)
        assert_amps_close(eng, orc, len(comps), 1e-9, "iteration %d" % it)
        assert_indices_close(eng, orc, comps, 1e-12, "iteration %d" % it)
    return eng, orc


@pytest.mark.parametrize("scale", [1e-2, 1e-4])
def test_high_snr_index_sweeps_match_the_oracle(built, scale):
    _iterations(make_case("C3", nside=8, start="truth", tweak=_sharpen(scale)), 3)


def test_out_of_range_exponents_take_the_exact_form(built):
    _iterations(make_case("C3", nside=8, start="truth", tweak=_wide_bounds), 2)


@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_plane_set_iterations_match_the_oracle(built, scale):
    """da.gibbs_iteration (the k_plane_set launches the benchmark times: ADD / SUB residual forms, paired dust chains whose
    second chain starts from the first one's sums) against the oracle's solve-then-sweep order."""
    case = make_case("C3", nside=8, start="truth", tweak=_sharpen(scale))
    dpar, ddata, bands, comps, meta = case
    eng, orc = _iterations(case, 1)
    for it in (2, 3):
        da.gibbs_iteration(dpar, ddata, it)
        for g in dpar.cg_groups:
            for f in g.pol_flag:
                orc.amp_sample_direct(g.cg_group, f, "sample", dpar.seed, da.stream_id(it, 0, g.cg_group, 0, f), "reference")
        for l, c in enumerate(comps):
            for j in range(c.nindices):
                if c.sample_index[j]:
                    for f in c.pol_flag[j]:
                        orc.sample_index_mh(l, j, MAPN[f], dpar.nsample, "sample", dpar.seed, da.stream_id(it, 1, l, j, f))
        assert_amps_close(eng, orc, len(comps), 1e-9, "iteration %d" % it)
        assert_indices_close(eng, orc, comps, 1e-12, "iteration %d" % it)
