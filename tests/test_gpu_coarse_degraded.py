"""GPU parity for the DEGRADED coarse model (dangx_set_coarse_model / DangComps.coarse_model = 'degraded'): a chain at a
coarser Nside reads the swept component's amplitude and index maps degraded like the data, and the degraded mask.

Specification by equivalence: for a model of diffuse components a DEGRADED sweep at Nside Nc is the reference's ordinary
full-resolution sweep run on a surrogate sky at Nside Nc -- data = udgrade_ring(data_raw - others), rms = udgrade_rms,
mask = udgrade_mask, the swept component's amplitude / indices = udgrade_ring of its maps, every other component's
amplitude 0, gain 1, offset 0 -- which the oracle already runs (Oracle.sample_index_mh / sample_index_fullsky).  One
difference by design: a skipped (masked) coarse pixel keeps its starting value idx_c where the reference's per-pixel sweep
writes 0 (a dust temperature of 0 would make the SEDs of the unmasked children of such a pixel NaN)."""
import copy

import numpy as np
import pytest

import dang_amd as da

import oracle_ffi as O
from util import make_case, pair

pytestmark = pytest.mark.gpu

MAPN = {1: 1, 8: -1}


def _planes(map_n):
    return [0] if map_n == 1 else [1, 2]


def _surrogate(case_fn, eng, comps, l, nside, cnside):
    """(Oracle on the surrogate sky at Nside cnside, its component list) for a sweep of component l, from the engine's
    current full-resolution state."""
    dpar, ddata, bands, comps0, meta = case_fn(nside)
    cur = copy.deepcopy(comps)
    for m, c in enumerate(cur):
        c.amplitude = eng.get_amplitude(m)
        if c.nindices:
            c.indices = eng.get_indices(m)
    # the others' signal at full resolution: the sky model without component l
    wo = copy.deepcopy(cur)
    wo[l].amplitude = np.zeros_like(wo[l].amplitude)
    others, _ = O.Oracle(bands, wo, ddata).sky_model()
    nb, nmaps, _ = ddata.sig_map.shape
    cleaned = np.asarray(ddata.sig_map) - others
    s_dpar, s_ddata, s_bands, s_comps, s_meta = case_fn(cnside)
    up = lambda mode, m: O.udgrade(mode, m, nside, cnside)   # noqa: E731
    s_ddata.sig_map = np.array([[up(0, cleaned[j, k]) for k in range(nmaps)] for j in range(nb)])
    s_ddata.rms_map = np.array([[up(1, np.asarray(ddata.rms_map)[j, k]) for k in range(nmaps)] for j in range(nb)])
    s_ddata.masks = np.array([up(2, np.asarray(ddata.masks)[k]) for k in range(np.asarray(ddata.masks).shape[0])])
    s_ddata.gain, s_ddata.offset = np.ones(nb), np.zeros(nb)
    for m, c in enumerate(s_comps):
        c.amplitude = np.zeros((nmaps, 12 * cnside * cnside))
        if m == l:
            c.amplitude = np.array([up(0, cur[l].amplitude[k]) for k in range(nmaps)])
            c.indices = np.array([[up(0, cur[l].indices[n, k]) for k in range(nmaps)] for n in range(c.nindices)])
        c.step_size = list(cur[m].step_size)
        c.tuned = list(cur[m].tuned)
    return O.Oracle(s_bands, s_comps, s_ddata), s_comps


def _mask_c(ddata, nside, cnside):
    return O.udgrade(2, np.asarray(ddata.masks)[0], nside, cnside)


@pytest.mark.parametrize("lnl,ml_mode,cnside,prior", [("chisq", "sample", 4, None), ("chisq", "optimize", 4, None),
                                                      ("chisq", "sample", 2, None), ("chisq", "sample", 1, None),
                                                      ("marginal", "sample", 2, None), ("prior", "sample", 4, None),
                                                      ("chisq", "sample", 2, "jeffreys"), ("chisq", "optimize", 4, "jeffreys")])
def test_degraded_sweep_is_the_reference_sweep_on_the_surrogate_sky(built, lnl, ml_mode, cnside, prior):
    nside = 16 if prior is None else 8

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.lnl_type = [lnl] * c.nindices
            c.sample_nside = [cnside] * c.nindices
            c.coarse_model = ["degraded"] * c.nindices
            if prior:
                c.prior_type = [prior] * c.nindices
    case_fn = lambda ns: make_case("C2", nside=ns, start="truth", tweak=tweak)   # noqa: E731
    case = case_fn(nside)
    dpar, ddata, bands, comps, meta = case
    eng, _ = pair(case)
    live = _mask_c(ddata, nside, cnside) > 0.5
    swept = 0
    for l, c in enumerate(comps):
        for j in range(c.nindices):
            if not c.sample_index[j]:
                continue
            map_n = MAPN[c.pol_flag[j][0]]
            s = da.stream_id(2, 1, l, j, c.pol_flag[j][0])
            sorc, s_comps = _surrogate(case_fn, eng, comps, l, nside, cnside)
            ag = eng.index_sample_coarse(l, j, map_n, 10, ml_mode, 7, s, cnside)
            ao = sorc.sample_index_mh(l, j, map_n, 10, ml_mode, 7, s)
            assert ao >= 0 and ag == ao, (l, j, ag, ao)
            got = eng.get_indices(l)
            for k in _planes(map_n):
                coarse = np.where(live, sorc.indices(l)[j, k], s_comps[l].indices[j, k])   # skipped: the starting value
                want = O.udgrade(0, coarse, cnside, nside)
                assert np.abs(got[j, k] - want).max() <= 1e-12, (l, j, k)
            swept += 1
    assert swept >= 3


def test_degraded_differs_from_reference_and_reference_is_the_default(built):
    """The switch changes the result (the reference reads unrelated full-resolution pixels); REFERENCE set explicitly is
    bit-identical to never setting it."""
    nside, cnside = 16, 4

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.sample_nside = [cnside] * c.nindices
    results = {}
    for mode in ("unset", "reference", "degraded"):
        case = make_case("C2", nside=nside, start="truth", tweak=tweak)
        dpar, ddata, bands, comps, meta = case
        if mode != "unset":
            for c in comps:
                c.coarse_model = [mode] * c.nindices
        eng, _ = pair(case)
        acc = [eng.index_sample_coarse(l, j, MAPN[c.pol_flag[j][0]], 10, "sample", 7, da.stream_id(2, 1, l, j, c.pol_flag[j][0]), cnside)
               for l, c in enumerate(comps) for j in range(c.nindices) if c.sample_index[j]]
        results[mode] = (acc, [eng.get_indices(l) for l, c in enumerate(comps) if c.nindices])
    assert results["unset"][0] == results["reference"][0]
    for a, b in zip(results["unset"][1], results["reference"][1]):
        assert np.array_equal(a, b)
    assert any(not np.array_equal(a, b) for a, b in zip(results["reference"][1], results["degraded"][1]))


def test_reference_partials_buffers_are_unchanged_by_the_switch(built):
    nside, cnside = 8, 2

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.sample_nside = [cnside] * c.nindices
    bufs = []
    for mode in ("reference", "degraded"):
        case = make_case("C2", nside=nside, start="truth", tweak=tweak, rank=0, nranks=2)
        dpar, ddata, bands, comps, meta = case
        for c in comps:
            c.coarse_model = [mode] * c.nindices
        eng, _ = pair(case)
        np_, ni = eng.coarse_sizes(1, cnside)
        assert np_ == 2 * (2 * meta["nbands"] + 1) * 12 * cnside * cnside and ni == 12 * cnside * cnside + 1
        bufs.append(eng.coarse_partials(1, 1, cnside))
        assert eng.coarse_model_size(1, 1, cnside) == (0 if mode == "reference" else (1 + 1 + 1) * 12 * cnside * cnside)
    assert np.array_equal(bufs[0], bufs[1])


@pytest.mark.parametrize("nshards", [1, 3])
def test_degraded_sweeps_over_several_contexts_of_one_process(built, nshards):
    nside, cnside = 8, 2

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.sample_nside = [cnside] * c.nindices
            c.coarse_model = ["degraded"] * c.nindices
    whole = make_case("C2", nside=nside, start="truth", tweak=tweak)
    dpar, ddata, bands, comps, meta = whole
    ref, _ = pair(whole)
    shards = [make_case("C2", nside=nside, start="truth", tweak=tweak, rank=r, nranks=nshards) for r in range(nshards)]
    engs = [da.Engine(x[2], x[3], x[1], npix_global=x[4]["npix_global"], pix0=x[4]["pix0"], device=0) for x in shards]
    for l, c in enumerate(comps):
        for j in range(c.nindices):
            if not c.sample_index[j]:
                continue
            f = c.pol_flag[j][0]
            s = da.stream_id(2, 1, l, j, f)
            a_ref = ref.index_sample_coarse(l, j, MAPN[f], 10, "sample", 7, s, cnside)
            a_multi = da.index_sample_coarse_multi(engs, l, j, MAPN[f], 10, "sample", 7, s, cnside)
            assert a_ref == a_multi, (l, j, a_ref, a_multi)
    for l, c in enumerate(comps):
        if not c.nindices:
            continue
        got = np.concatenate([e.get_indices(l) for e in engs], axis=-1)
        if nshards == 1:
            assert np.array_equal(got, ref.get_indices(l))
        assert np.abs(got - ref.get_indices(l)).max() <= 1e-12


def test_degraded_chain_without_finished_model_sums_raises(built):
    nside, cnside = 8, 2

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.sample_nside = [cnside] * c.nindices
            c.coarse_model = ["degraded"] * c.nindices
    case = make_case("C2", nside=nside, start="truth", tweak=tweak, rank=0, nranks=1)
    eng, _ = pair(case)
    part = eng.coarse_partials(1, 1, cnside)
    with pytest.raises(da.DangxError, match="DANGX_COARSE_DEGRADED"):
        eng.coarse_chains(1, 0, 1, 10, "sample", 7, 1, cnside, part)
    # finished, then the state changes (an index sweep writes the maps): stale again
    eng.coarse_model_finish(1, 1, cnside, eng.coarse_model_partials(1, 1, cnside))
    eng.index_sample(2, 0, 1, 2, "sample", 7, 3)
    eng.coarse_model_finish(1, 1, cnside, eng.coarse_model_partials(1, 1, cnside))
    eng.put_amplitude(1, eng.get_amplitude(1))
    with pytest.raises(da.DangxError, match="DANGX_COARSE_DEGRADED"):
        eng.coarse_chains(1, 0, 1, 10, "sample", 7, 1, cnside, part)
    # a reference-model component has no model buffer
    with pytest.raises(da.DangxError, match="model buffer"):
        eng.set_coarse_model(1, 0, "reference")
        eng.coarse_model_partials(1, 1, cnside)


@pytest.mark.parametrize("tuned", [True, False])
def test_degraded_fullsky_chain_is_the_reference_chain_on_the_surrogate_sky(built, tuned):
    nside, cnside = 8, 2

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.index_mode = [1] * c.nindices
            c.tuned = [tuned] * max(c.nindices, 1)
            c.sample_nside = [cnside] * c.nindices
            c.coarse_model = ["degraded"] * c.nindices
            c.step_size = [0.6 * g[1] for g in c.gauss_prior]
    case_fn = lambda ns: make_case("C2", nside=ns, start="truth", tweak=tweak)   # noqa: E731
    case = case_fn(nside)
    dpar, ddata, bands, comps, meta = case
    eng, _ = pair(case)
    for l, c in enumerate(comps):
        for j in range(c.nindices):
            if not c.sample_index[j]:
                continue
            f = c.pol_flag[j][0]
            map_n = MAPN[f]
            s = da.stream_id(2, 1, l, j, f)
            sorc, s_comps = _surrogate(case_fn, eng, comps, l, nside, cnside)
            # the full-sky chain starts at c%indices(0, map_inds(1), :): the surrogate's pixel 0 carries the full sky's
            first = eng.get_indices(l)[:, :, 0]
            sorc.indices(l)[:, :, 0] = first
            was_tuned = c.tuned[j]          # (the tuner marks every index of the component tuned)
            ag = da.sample_index_mh_fullsky(dpar, ddata, l, j, map_n, s, sample_nside=cnside)
            ao, tuned_o, step_o = sorc.sample_index_fullsky(l, j, map_n, dpar.nsample, dpar.ml_mode, dpar.seed, s, tuned=was_tuned)
            assert ag == ao, (l, j, ag, ao)
            assert c.step_size[j] == step_o
            got = eng.get_indices(l)
            for k in _planes(map_n):
                assert np.abs(got[j, k] - sorc.indices(l)[j, k, 0]).max() <= 1e-13
                assert np.all(got[j, k] == got[j, k, 0])


def test_degraded_fullsky_over_three_contexts_agrees_with_one(built):
    nside, cnside = 8, 2

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.index_mode = [1] * c.nindices
            c.sample_nside = [cnside] * c.nindices
            c.coarse_model = ["degraded"] * c.nindices
            c.step_size = [0.6 * g[1] for g in c.gauss_prior]
    from util import shard_engines
    whole = make_case("C2", nside=nside, start="truth", tweak=tweak)
    dpar, ddata, bands, comps, meta = whole
    one, _ = pair(whole)
    engs = shard_engines(whole, 3)
    for l, c in enumerate(comps):
        for j in range(c.nindices):
            if not c.sample_index[j]:
                continue
            f = c.pol_flag[j][0]
            s = da.stream_id(2, 1, l, j, f)
            a1 = da.sample_index_mh_fullsky(dpar, ddata, l, j, MAPN[f], s, sample_nside=cnside)
            a3 = da.sample_index_mh_fullsky(dpar, ddata, l, j, MAPN[f], s, sample_nside=cnside, engines=engs)
            assert a1 == a3, (l, j, a1, a3)
    for l, c in enumerate(comps):
        if c.nindices:
            got = np.concatenate([e.get_indices(l) for e in engs], axis=-1)
            assert np.abs(got - one.get_indices(l)).max() <= 1e-12


def _piecewise_sky(nside, cnside, l, j, seed=3):
    """C2 at `nside` whose index j of component l is constant on Nside-`cnside` pixels, amplitudes at the truth, the data
    rebuilt from that truth plus the rms's noise.  Returns (case, true coarse index map, truth components)."""
    from dang_amd import synth
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=nside, start="truth")
    rng = np.random.default_rng(seed)
    beta_c = comps[l].indices[j, 0, 0] + 0.15 * rng.standard_normal(12 * cnside * cnside)
    beta = O.udgrade(0, beta_c, cnside, nside)
    for k in range(comps[l].indices.shape[1]):
        comps[l].indices[j, k] = beta
    truth = copy.deepcopy(comps)
    sky, _ = O.Oracle(bands, truth, ddata).sky_model()
    ddata.sig_map = sky + rng.standard_normal(sky.shape) * np.asarray(ddata.rms_map)
    return (dpar, ddata, bands, comps, meta), beta_c, truth


def _beta_sigma(case, truth, l, j, beta_c, nside, cnside):
    """Posterior width of index j of component l per coarse pixel at fixed (degraded, true) amplitude: 1 / sqrt of the chisq
    curvature, sum over bands of (a_c ds_j/dbeta / rms_c)^2, with ds_j/dbeta by a central difference of the oracle's SED."""
    dpar, ddata, bands, comps, meta = case
    orc = O.Oracle(bands, truth, ddata)
    amp_c = O.udgrade(0, truth[l].amplitude[0], nside, cnside)
    curv = np.zeros(12 * cnside * cnside)
    h = 1e-5
    for b in range(meta["nbands"]):
        rms_c = O.udgrade(1, np.asarray(ddata.rms_map)[b, 0], nside, cnside)
        other = truth[l].indices[1 - j, 0, 0] if truth[l].nindices > 1 else 0.0
        th = lambda v: [v, other] if j == 0 else [other, v]   # noqa: E731
        ds = np.array([(orc.eval_sed(l, b, th(x + h)) - orc.eval_sed(l, b, th(x - h))) / (2 * h) for x in beta_c])
        curv += (amp_c * ds / rms_c) ** 2
    return 1.0 / np.sqrt(curv)


def test_degraded_optimize_recovers_a_piecewise_constant_beta(built):
    """Nside 32 data whose synchrotron beta is constant on Nside-8 pixels, every amplitude at the truth: optimize sweeps at
    Nc = 8 of the DEGRADED model must land on the true beta of every unmasked coarse pixel within 5 sigma + step / 10.
    sigma: the beta posterior's width at fixed amplitude, 1 / sqrt(sum_band (a_c ds/dbeta / rms_c)^2) with the degraded
    amplitude a_c and rms_c (the degraded data are the truth plus the children's mean noise, whose rms is exactly rms_c).
    step / 10: how close 4 x 50 greedy proposals of width `step` get to the optimum (the distance roughly halves per
    acceptance, and a proposal is accepted with probability ~ distance / step)."""
    nside, cnside, l, j = 32, 8, 1, 0          # synch beta, T plane
    case, beta_c, truth = _piecewise_sky(nside, cnside, l, j)
    dpar, ddata, bands, comps, meta = case
    for c in comps:
        c.sample_nside = [cnside] * c.nindices
        c.coarse_model = ["degraded"] * c.nindices
    comps[l].indices[j] = beta_c.mean() + 0.2           # start away from the truth
    step = comps[l].step_size[j]
    eng = da.Engine(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    for rnd in range(4):
        eng.index_sample_coarse(l, j, 1, 50, "optimize", 7, da.stream_id(2 + rnd, 1, l, j, 1), cnside)
    got_c = O.udgrade(0, eng.get_indices(l)[j, 0], nside, cnside)
    sigma = _beta_sigma(case, truth, l, j, beta_c, nside, cnside)
    live = _mask_c(ddata, nside, cnside) > 0.5
    err = np.abs(got_c - beta_c)[live]
    assert np.all(err <= 5.0 * sigma[live] + 0.1 * step), (err.max(), sigma[live].max(), step)


def test_whole_iterations_at_a_coarse_nside_end_near_the_full_resolution_chisq(built):
    """Whole Gibbs iterations at Nside 32 on a sky the coarse model can represent -- every true amplitude and index constant on
    Nside-8 pixels (the coarse means of the synthetic truth, the data rebuilt from them): with every index at Nc = 8 and the
    DEGRADED model, ddata.chisq ends within a factor 2 of the full-resolution run's.  (The synthetic truth itself varies pixel to
    pixel in amplitude and index; a coarse chain then sees only the children's mean amplitude, and even the exact coarse means
    of the true indices leave chi^2 ~ 130 at this size: that is the coarse parametrisation, not the sampler.)"""
    from dang_amd import synth
    nside, cnside = 32, 8
    coarse = lambda m: O.udgrade(0, O.udgrade(0, m, nside, cnside), cnside, nside)   # noqa: E731
    chis = {}
    for model in ("full", "degraded"):
        dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=nside, start="truth")
        for c in comps:
            for k in range(c.amplitude.shape[0]):
                c.amplitude[k] = coarse(c.amplitude[k])
            for n in range(c.nindices):
                for k in range(c.indices.shape[1]):
                    c.indices[n, k] = coarse(c.indices[n, k])
        sky, _ = O.Oracle(bands, copy.deepcopy(comps), ddata).sky_model()
        ddata.sig_map = sky + np.random.default_rng(5).standard_normal(sky.shape) * np.asarray(ddata.rms_map)
        if model != "full":
            for c in comps:
                c.sample_nside = [cnside] * c.nindices
                c.coarse_model = [model] * c.nindices
        da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
        for it in range(1, 4):
            da.gibbs_iteration(dpar, ddata, it)
        chis[model] = ddata.chisq
    assert np.isfinite(chis["degraded"]) and chis["degraded"] <= 2.0 * chis["full"], chis


def _degraded_coarse_job(rank=0, world=1):
    """Per-pixel DEGRADED sweeps (Nside 8 -> 2) on a sharded sky: the degrade sums and the model channels go through the
    dangx_set_allreduce callback."""
    from test_gpu_multirank import _shard

    def tweak(dpar, ddata, bands, comps):
        for c in comps:
            c.sample_nside = [2] * c.nindices
            c.coarse_model = ["degraded"] * c.nindices
    case = make_case("C2", nside=8, start="truth", tweak=tweak)
    dpar, ddata, bands, comps, meta = case
    ddata, comps, p0, n = _shard(case, rank, world)
    ddata.nump = case[1].nump
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=p0, device=0)
    info = da.sample_spectral_parameters(dpar, ddata, it=2)
    out = {"acc": np.array([a for (_, _, _, a) in info], dtype=np.float64)}
    for l, c in enumerate(comps):
        if c.nindices:
            out["idx%d" % l] = eng.get_indices(l)
    return out


def _degraded_worker(rank, world, port, out):
    import os
    import sys
    import torch
    import torch.distributed as td
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    td.init_process_group("gloo", rank=rank, world_size=world)
    from dang_amd import dist
    res = {}
    cj = _degraded_coarse_job(rank, world)
    res["acc_r%d" % rank] = cj["acc"]
    for k, v in cj.items():
        if k.startswith("idx"):
            g = dist.gather_maps(torch.from_numpy(v), 768, dst=0)
            if rank == 0:
                res[k] = g.numpy()
    gathered = [None] * world
    td.all_gather_object(gathered, {k: v for k, v in res.items() if k.startswith("acc")})
    if rank == 0:
        for g in gathered:
            res.update(g)
        np.savez(out, **res)
    td.barrier()
    td.destroy_process_group()


def test_two_ranks_run_the_degraded_sweeps_of_one(built, tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port
    out = str(tmp_path / "d.npz")
    mp.spawn(_degraded_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = np.load(out)
    one = _degraded_coarse_job()
    assert np.array_equal(got["acc_r0"], got["acc_r1"]) and np.array_equal(got["acc_r0"], one["acc"])
    for k, v in one.items():
        if k.startswith("idx"):
            assert np.abs(got[k] - v).max() <= 1e-12, k
