"""Posterior moments, host side: the default selection of what a run samples, and posterior_maps' assembly and masked-pixel fill
(healpy's UNSEEN, as scripts/make_mean_maps.py writes it) on host arrays.  No device needed."""
import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import synth

T, Q, U = 1, 2, 4
AMP_T, AMP_QU = T, Q | U


def idx(j, planes):
    return planes << (3 + 3 * j)


# label -> selection word; the T set samples its amplitude in group 1 (T), the polarisation set in group 2 (Q+U); indices as
# synth.PHYS marks them sampled (ff T_e, ame w and both dust2 indices are fixed)
EXPECT = {
    "cmb": AMP_T, "synch": AMP_T | idx(0, T), "dust": AMP_T | idx(0, T) | idx(1, T), "ff": AMP_T, "ame": AMP_T | idx(0, T), "dust2": AMP_T,
    "cmb_P": AMP_QU, "synch_P": AMP_QU | idx(0, Q | U), "dust_P": AMP_QU | idx(0, Q | U) | idx(1, Q | U), "ff_P": AMP_QU,
    "ame_P": AMP_QU | idx(0, Q | U), "dust2_P": AMP_QU,
}


@pytest.mark.parametrize("config", ["C1", "C2", "C3", "C5"])
def test_default_selection_of_the_synthetic_models(config):
    dpar, ddata, bands, comps, meta = synth.make_sky(config, nside=1)
    sel = da.default_moment_selection(dpar, comps)
    assert sel.dtype == np.int32 and sel.shape == (len(comps),)
    assert [int(s) for s in sel] == [EXPECT[c.label] for c in comps]
    if config == "C3":   # 12 amplitude planes and 9 index planes
        assert sum(bin(int(s) & 7).count("1") for s in sel) == 12
        assert sum(bin(int(s) >> 3).count("1") for s in sel) == 9


def test_default_selection_follows_the_flags():
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=1, device="cpu", as_numpy=False)
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 4))
    sel = da.default_moment_selection(dpar, comps)
    assert sel[-2] == AMP_QU and sel[-1] == AMP_T            # template rows Q, U (group 2); monopole row T (group 1)
    comps[1].sample_amplitude = False                          # synch: index only
    comps[2].sample_index = [True, False]                      # dust: T fixed
    comps[5].pol_flag = [[L.FLAG_Q], [L.FLAG_U]]               # dust_P: beta on Q, T on U
    dpar.cg_groups[1].pol_flag = [L.FLAG_Q, L.FLAG_U]          # group 2 in two passes: still Q and U
    sel = da.default_moment_selection(dpar, comps)
    assert sel[1] == idx(0, T)
    assert sel[2] == AMP_T | idx(0, T)
    assert sel[5] == AMP_QU | idx(0, Q) | idx(1, U)
    dpar.cg_groups = [g for g in dpar.cg_groups if g.cg_group != 2]   # no group samples the polarisation amplitudes
    sel = da.default_moment_selection(dpar, comps)
    assert sel[3] == 0 and sel[-2] == 0


class _FakeEngine:
    """What posterior_maps reads of an Engine, over host arrays: one shard of a 2-component sky with a fixed set of moments."""

    def __init__(self, comps, masks, means, stds, sel, n=7):
        self.component_list, self.ddata = comps, da.DangData(sig_map=None, rms_map=None, masks=masks)
        self._means, self._stds, self._moment_sel, self._n = means, stds, np.asarray(sel, dtype=np.int32), n

    def moments_count(self):
        return self._n

    def moments_get(self, l, what, stat, ddof=0):
        return (self._means if stat == "mean" else self._stds)[(l, what)].copy()

    def moments_get_template(self, l, stat, ddof=0):
        return np.full((3, 2), 1.0 if stat == "mean" else 0.5)


def _shard(rng, npix, masked):
    comps = [da.DangComps(label="synch", type="power-law", nu_ref=30.0, nindices=1, ind_label=["beta"]),
             da.DangComps(label="tmpl", type="template", nu_ref=100.0)]
    masks = np.ones((3, npix))
    masks[0, masked] = 0.0
    masks[1:, :] = 1.0                      # only plane 1 is tested, as the reference does
    means = {(0, 0): rng.standard_normal((3, npix)), (0, 1): rng.standard_normal((3, npix))}
    stds = {(0, 0): rng.random((3, npix)), (0, 1): rng.random((3, npix))}
    return comps, masks, means, stds


def test_posterior_maps_fill_and_assembly_on_host_arrays():
    rng = np.random.default_rng(1)
    sel = [T | idx(0, T), Q | U]
    parts = [_shard(rng, 5, [1, 4]), _shard(rng, 4, [0])]
    engs = [_FakeEngine(c, m, mu, sd, sel) for c, m, mu, sd in parts]
    plain = da.posterior_maps(None, engines=engs)
    assert set(plain) == {("synch", "amplitude"), ("synch", "beta"), ("tmpl", "amplitude")}
    for (l, what), key in (((0, 0), ("synch", "amplitude")), ((0, 1), ("synch", "beta"))):
        assert plain[key]["n"] == 7
        assert np.array_equal(plain[key]["mean"], np.concatenate([p[2][(l, what)] for p in parts], axis=-1))
        assert np.array_equal(plain[key]["std"], np.concatenate([p[3][(l, what)] for p in parts], axis=-1))
    assert (plain[("tmpl", "amplitude")]["std"] == 0.5).all()      # global amplitudes: never masked
    unseen = -1.6375e30
    filled = da.posterior_maps(None, masked_value=unseen, engines=engs)
    masked = np.zeros(9, dtype=bool)
    masked[[1, 4, 5]] = True
    for key in (("synch", "amplitude"), ("synch", "beta")):
        for stat in ("mean", "std"):
            f, p = filled[key][stat], plain[key][stat]
            assert (f[:, masked] == unseen).all()                  # every plane of a masked pixel
            assert np.array_equal(f[:, ~masked], p[:, ~masked])
    assert (filled[("tmpl", "amplitude")]["std"] == 0.5).all()
    engs[1]._n = 6
    with pytest.raises(da.DangxError, match="different sample counts"):
        da.posterior_maps(None, engines=engs)
