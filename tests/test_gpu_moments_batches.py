"""Batched posterior accumulators (dangx_moments_batches*, dangx_chains_batches_*): burn-in discarded after the run, the batch-means
Monte-Carlo error and effective sample size, split R-hat of one chain and of several.  Exactness of the slots before any merge,
every read-out against a long-double evaluation of the definitions on the same planted samples (references and tolerances:
tests/batches_ref.py), a merge against a late registration, several chains, shards / alignment / determinism, the launches and
accumulators that must not move, streams, and the error cases.  C2 at Nside 4 throughout."""
import numpy as np
import pytest
import torch

import dang_amd as da
from dang_amd import synth

import batches_ref as br
import chains_ref as cr
import test_gpu_chains as tg
import test_gpu_moments_pairs as tp
import test_gpu_moments_signal as ts
from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

EPS = cr.EPS
NPIX = 192
WHOLE = [(0, NPIX)]


@pytest.fixture(scope="module")
def four(built):
    """four independent whole-sky C2 contexts at Nside 4; every test restarts their accumulators with moments_begin"""
    cases = [make_case("C2", nside=4) for _ in range(4)]
    return cases, [tg._engine(c) for c in cases]


def _reg_planes(comps):
    """an index plane on T, the second index of a two-index component on Q, an amplitude plane on U"""
    l1 = next(l for l, c in enumerate(comps) if c.nindices >= 1)
    l2 = next(l for l, c in enumerate(comps) if c.nindices >= 2)
    return [(l1, 1, 0), (l2, 2, 1), (l2, 0, 2)]


def _states(comps, x):
    """every plane of every component holds the series x [n][npix]"""
    out = {}
    for l, c in enumerate(comps):
        a = np.repeat(x[:, None, :], 3, axis=1)
        out[l] = (a, np.repeat(a[:, None], c.nindices, axis=1) if c.nindices else None)
    return out


def _start(e, comps, nbatch, L0, planes=None):
    e.moments_begin(None)
    e.moments_batches(planes if planes is not None else _reg_planes(comps), nbatch=nbatch, batch_len=L0)


def _feed(engs, bounds, comps, x):
    tp._feed(engs, bounds, comps, _states(comps, x), len(x))


def _info(e):
    i = e.moments_batches_info()
    return i["batch_len"], i["nfull"], i["partial"]


def _power_of_two_series(n, off=0.0):
    """t s_p + off with s_p a power of two per pixel: every mean and fold of it is exact when off = 0"""
    s = 2.0 ** ((np.arange(NPIX) % 7) - 3)
    return np.arange(n)[:, None] * s[None, :] + off, s


# ---- 1. exactness before any merge

def test_exactness_before_any_merge(four):
    cases, engs = four
    comps = cases[0][3]
    planes = _reg_planes(comps)
    a, b = engs[0], engs[1]
    rng = np.random.default_rng(3)
    x = tp._ar1(rng, 12, (NPIX,), -3.1)
    _start(a, comps, 4, 3)
    _feed([a], WHOLE, comps, x[:3])
    assert _info(a) == (3, 1, 0)
    for r, (l, what, k) in enumerate(planes):
        mean, m2 = a.moments_batches_raw(r, 0)
        assert ts._same_bits(mean, a.moments_get(l, what, "mean")[k])
        for ddof in (0, 1):
            assert ts._same_bits(a.moments_batches_get(r, "std", 0, ddof), a.moments_get(l, what, "std", ddof)[k]), (r, ddof)
        assert ts._same_bits(a.moments_batches_get(r, "mean"), mean)
    _feed([a], WHOLE, comps, x[3:])
    assert _info(a) == (3, 4, 0)
    for bt in range(4):
        b.moments_begin(None)
        _feed([b], WHOLE, comps, x[3 * bt:3 * bt + 3])
        for r, (l, what, k) in enumerate(planes):
            mean, m2 = a.moments_batches_raw(r, bt)
            assert ts._same_bits(mean, b.moments_get(l, what, "mean")[k]), (bt, r)
            assert ts._same_bits(np.sqrt(m2 / 3.0), b.moments_get(l, what, "std")[k]), (bt, r)
            assert m2[0] == 0                                                # the pixel that never moves
    md, qd = a.moments_batches_raw(0, 2, device=True)                       # the device form copies the same bits
    mh, qh = a.moments_batches_raw(0, 2)
    assert ts._same_bits(md.cpu().numpy(), mh) and ts._same_bits(qd.cpu().numpy(), qh)


# ---- 2. against long double, with merges

CASES = [(37, 4, 1), (64, 2, 2), (96, 32, 1), (33, 2, 1)]


@pytest.mark.parametrize("off", tp.OFFSETS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_nb%d_L%d" % c)
def test_against_long_double_with_merges(four, case, off):
    cases, engs = four
    comps = cases[0][3]
    planes = _reg_planes(comps)
    n, nbatch, L0 = case
    L, nfull, partial = br.replay(n, nbatch, L0)
    rng = np.random.default_rng(100 * n + nbatch)
    x = tp._ar1(rng, n, (NPIX,), off)                                        # pixel 0 never moves
    h = nfull // 2
    x[:, 1] = off + (np.arange(n) >= (nfull - h) * L)                         # first = 0: the halves differ in their means alone
    e = engs[0]
    _start(e, comps, nbatch, L0)
    _feed([e], WHOLE, comps, x)
    assert _info(e) == (L, nfull, partial)
    for first in sorted({f for f in (0, 1, nfull - 2) if 0 <= f <= nfull}):
        for ddof in (0, 1):
            for r in range(len(planes)):
                got = {}

                def get(stat):
                    got[stat] = e.moments_batches_get(r, stat, first, ddof)
                    return got[stat]

                done = br.check(get, x, L, nfull, partial, first, ddof, "%s off %g reg %d" % (case, off, r))
                for stat in br.STATS:
                    if stat not in done:
                        with pytest.raises(da.DangxError, match="needs|no sample"):
                            e.moments_batches_get(r, stat, first, ddof)
                if "split_rhat" in done and first == 0:                      # NaN where the pixel never moved and nowhere else
                    rh, es = got["split_rhat"], got["ess_bm"]
                    assert np.isnan(rh[0]) and rh[1] == np.inf and np.isfinite(rh[2:]).all()
                    assert np.isnan(es[0]) and np.isfinite(es[1:]).all()
    d = e.moments_batches_get(1, "mean", 0, 0, device=True)
    assert ts._same_bits(d.cpu().numpy(), e.moments_batches_get(1, "mean"))


# ---- 3. a merge equals a late registration

def test_merge_equals_late_registration(four):
    cases, engs = four
    comps = cases[0][3]
    planes = _reg_planes(comps)
    a, b = engs[0], engs[1]
    rng = np.random.default_rng(9)
    exact, _ = _power_of_two_series(8)
    for x, bitwise in ((tp._ar1(rng, 8, (NPIX,), 1.0e6), False), (exact, True)):
        _start(a, comps, 2, 1)
        _start(b, comps, 2, 4)
        _feed([a], WHOLE, comps, x)
        _feed([b], WHOLE, comps, x)
        assert _info(a) == _info(b) == (4, 2, 0)
        for r in range(len(planes)):
            for bt in (0, 1):
                (ma, qa), (mb, qb) = a.moments_batches_raw(r, bt), b.moments_batches_raw(r, bt)
                pm = cr.pooled([x[4 * bt:4 * bt + 4]], 0)
                for m, q in ((ma, qa), (mb, qb)):
                    cr.compare(m, *pm["mean"], "batch %d mean" % bt)
                    cr.compare(np.sqrt(q / 4.0), *pm["std"], "batch %d std" % bt)
                if bitwise:
                    assert ts._same_bits(ma, mb) and ts._same_bits(qa, qb), (r, bt)


# ---- 4. several chains

def _chains_check(engs, xs, L, nfull, partial, first, ddof, what, nreg=3):
    for r in range(nreg):
        done = br.check(lambda stat: da.chains_batches_get(engs, r, stat, first, ddof), None, L, nfull, partial, first, ddof,
                        "%s reg %d" % (what, r), chains=xs)
        assert done == list(br.STATS)


def test_several_chains(four):
    cases, engs = four
    comps = cases[0][3]
    rng = np.random.default_rng(21)
    xs = [tp._ar1(rng, 16, (NPIX,), -3.1 + 0.7 * k) for k in range(4)]
    for e, x in zip(engs, xs):
        _start(e, comps, 4, 1)
        _feed([e], WHOLE, comps, x)
    assert all(_info(e) == (4, 4, 0) for e in engs)
    for first in (0, 1):
        _chains_check(engs, xs, 4, 4, 0, first, 1, "four chains first %d" % first)
    _chains_check(engs[:2], xs[:2], 4, 4, 0, 2, 0, "two chains first 2")
    # a chain displaced in its second half only, every whole-chain mean equal: chains 0-2 hold z_t + delta / 2, chain 3 holds z_t
    # and from t = 8 on z_t + delta, z_t = ((t mod 8) - 3.5) s.  The whole chains agree in their means (B/n = 0: R-hat =
    # sqrt(15/16)); the 8 halves have means delta/2 (six of them), 0 and delta and each M = 42 s^2: W = 6 s^2, B/n = delta^2 / 14
    s = 2.0 ** ((np.arange(NPIX) % 7) - 3)
    z = ((np.arange(16) % 8) - 3.5)[:, None] * s[None, :]
    delta = 8.0 * s
    xs = [z + delta / 2 for _ in range(3)] + [z + delta * (np.arange(16) >= 8)[:, None]]
    for e, x in zip(engs, xs):
        _start(e, comps, 4, 1)
        _feed([e], WHOLE, comps, x)
    l, what, k = _reg_planes(comps)[0]
    plain = da.chains_get(engs, l, what, "rhat")[k]
    split = da.chains_batches_get(engs, 0, "split_rhat")
    r2 = 7 / 8 + (64 / 14) / 6
    assert (plain < 1.1).all() and (np.abs(plain ** 2 - 15 / 16) <= 64 * EPS).all()
    assert (split > 1.1).all() and (np.abs(split ** 2 - r2) <= 64 * EPS * r2).all()
    cr.compare_rhat(split, cr.between([hh for x in xs for hh in br.halves(x, 4, 4, 0)]), "displaced chain, split R-hat^2")
    # refusals: count, L, registration
    engs[3].moments_accumulate()
    with pytest.raises(da.DangxError, match="chain 3: batch read-outs need equal sample counts: it holds 17, chain 0 holds 16"):
        da.chains_batches_get(engs, 0, "mean")
    _start(engs[3], comps, 4, 3)
    _feed([engs[3]], WHOLE, comps, xs[3])
    assert _info(engs[3]) == (6, 2, 4)
    with pytest.raises(da.DangxError, match="chain 3: the batch length is 6, chain 0 has 4"):
        da.chains_batches_get(engs, 0, "mean")
    _start(engs[2], comps, 8, 1)
    _feed([engs[2]], WHOLE, comps, xs[2])
    with pytest.raises(da.DangxError, match="chain 2: nbatch is 8, chain 0 has 4"):
        da.chains_batches_get(engs[:3], 0, "mean")
    _start(engs[1], comps, 4, 1, planes=_reg_planes(comps)[::-1])
    _feed([engs[1]], WHOLE, comps, xs[1])
    with pytest.raises(da.DangxError, match="chain 1: batch registration 0 is not the registration of chain 0"):
        da.chains_batches_get(engs[:2], 0, "mean")
    engs[1].moments_begin(None)
    engs[1].moments_accumulate()
    with pytest.raises(da.DangxError, match="chain 0: no batches are registered|chain 1: batch registration 0 is not"):
        da.chains_batches_get([engs[0], engs[1]], 0, "mean")
    out = np.full(NPIX, 7.0)
    with pytest.raises(da.DangxError, match="batch registration out of range"):
        da.chains_batches_get([engs[0], engs[2]], 3, "mean", out=out)
    assert (out == 7.0).all()


# ---- 5. shards, alignment, determinism

def _every_readout(engs, nreg, nbatch, first):
    """{key: sky map} of every stat and every raw slot of the shard engines `engs`, side by side"""
    out = {}
    for r in range(nreg):
        for stat in br.STATS:
            out[(r, stat)] = np.concatenate([e.moments_batches_get(r, stat, first, 1) for e in engs])
        for bt in range(nbatch):
            raws = [e.moments_batches_raw(r, bt) for e in engs]
            out[(r, "raw mean", bt)] = np.concatenate([m for m, _ in raws])
            out[(r, "raw m2", bt)] = np.concatenate([q for _, q in raws])
    return out


def test_shards_alignment_and_determinism(four):
    cases, engs = four
    comps = cases[0][3]
    whole, again = engs[0], engs[1]
    bounds = [0, 63, 130, NPIX]                                               # odd lengths: planes off the 16-byte grid
    shards = shard_engines(cases[2], 3, bounds=bounds)
    odd, keep = tg._off_the_grid(torch.device("cuda", 0))                     # state in caller buffers one double off the grid
    rng = np.random.default_rng(17)
    n, nbatch, L0 = 21, 4, 1                                                  # merges at 4, 8 and 16: L = 8, two full batches + 5
    x = tp._ar1(rng, n, (NPIX,), -3.1)
    groups = (([whole], WHOLE), ([again], WHOLE), (shards, list(zip(bounds[:-1], bounds[1:]))), ([odd], WHOLE))
    for group, bnds in groups:
        for e in group:
            _start(e, comps, nbatch, L0)
        _feed(group, bnds, comps, x)
        assert all(_info(e) == (8, 2, 5) for e in group)
    ref = _every_readout([whole], 3, nbatch, 0)
    assert any(np.isfinite(v).all() for v in ref.values()) and len(ref) == 3 * (5 + 2 * nbatch)
    for name, group in (("two runs", [again]), ("shards", shards), ("alignment", [odd])):
        got = _every_readout(group, 3, nbatch, 0)
        for key, v in ref.items():
            assert ts._same_bits(v, got[key]), (name, key)
    for stat in br.STATS:                                                     # over chains: aligned, misaligned and sharded sets
        a = da.chains_batches_get([whole, again], 1, stat, 0, 1)
        assert ts._same_bits(a, da.chains_batches_get([whole, odd], 1, stat, 0, 1)), stat
        d = da.chains_batches_get([whole, odd], 1, stat, 0, 1, device=True)
        whole.synchronize()
        assert ts._same_bits(d.cpu().numpy(), a), stat
    sh2 = shard_engines(cases[3], 3, bounds=bounds)
    for e in sh2:
        _start(e, comps, nbatch, L0)
    _feed(sh2, list(zip(bounds[:-1], bounds[1:])), comps, x)
    for stat in br.STATS:
        a = da.chains_batches_get([whole, again], 2, stat, 0, 1)
        b = np.concatenate([da.chains_batches_get([s0, s1], 2, stat, 0, 1) for s0, s1 in zip(shards, sh2)])
        assert ts._same_bits(a, b), stat
    del keep


# ---- 6. nothing else moves

def test_nothing_else_moves(built):
    runs, datas = [], []
    for with_batches in (False, True):
        case = make_case("C2", nside=4)
        dpar, ddata, bands, comps, meta = case
        eng = tg._engine(case)
        eng.profile(True)
        da.moments_begin(dpar, ddata)
        pairs, hist, specs = da.moments_pairs(dpar, ddata), da.moments_hist(dpar, ddata), da.moments_signals(dpar, ddata)
        if with_batches:
            planes = da.moments_batches(dpar, ddata, nbatch=2, batch_len=1)
            assert planes == da.default_hist_planes(dpar, comps, eng._moment_sel) and planes
        steps = []
        for it in range(1, 6):
            before = tg._launches(eng)
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
            after = tg._launches(eng)
            steps.append({k: after[k] - before.get(k, 0) for k in after})
        datas.append(ddata)
        runs.append((eng, steps, tg._accumulators(eng, len(pairs), len(hist), len(specs))))
    (e0, s0, a0), (e1, s1, a1) = runs
    assert all("k_batch" not in s and s["k_moments"] == 2 and s["k_hist"] == 1 for s in s0)     # nothing registered: no launch
    # registered: one launch per accumulation, one more where every slot was full (nbatch 2, L0 1: before samples 3 and 5)
    assert [s.pop("k_batch") for s in s1] == [1, 1, 2, 1, 2]
    assert s1 == s0                                                                          # every other id as it was
    assert _info(e1) == (4, 1, 1)
    assert a0.keys() == a1.keys()
    for key in a0:
        if key == "state":
            for l in a0[key]:
                assert np.array_equal(a0[key][l][0], a1[key][l][0])
                assert a0[key][l][1] is None or np.array_equal(a0[key][l][1], a1[key][l][1])
        else:
            assert ts._same_bits(np.asarray(a0[key], dtype=np.float64), np.asarray(a1[key], dtype=np.float64)), key
    # the read-outs launch nothing under the accumulation ids, and the maps by name carry the thin getters' values
    mark = tg._launches(e1)
    pm = da.posterior_batch_maps(datas[1], first=0, ddof=1)
    assert tg._launches(e1) == mark
    key = list(pm)[0]
    assert set(pm[key]) == {"n", "first", "batch_len", "nfull", "partial", "mean", "std"} and pm[key]["n"] == 5
    assert ts._same_bits(pm[key]["std"], e1.moments_batches_get(0, "std", 0, 1))


# ---- 7. streams

def test_streams(built):
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    cases = [make_case("C2", nside=4) for _ in range(2)]
    engs = []
    for case, s in zip(cases, (s0, s1)):
        dpar, ddata, bands, comps, meta = case
        engs.append(da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0, stream=s.cuda_stream))
    comps = cases[0][3]
    ld = next(l for l, c in enumerate(comps) if c.nindices >= 2)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 2, 2, 3, NPIX))          # [sample][chain][index][plane][pix]
    for e in engs:
        e.moments_begin(None)
        e.moments_batches([(ld, 1, 0)], nbatch=2, batch_len=2)
    for k, e in enumerate(engs):
        e.put_indices(ld, x[0][k])
        e.moments_accumulate()
    out = torch.full((NPIX,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    da.chains_batches_get(engs, 0, "mean", device=True, out=out)
    for k, e in enumerate(engs):                          # a further sample on both chains at once, behind the read-out
        e.put_indices(ld, x[1][k])
        e.moments_accumulate()
    torch.cuda.synchronize()
    first = x[0][0][0][0] + (x[0][1][0][0] - x[0][0][0][0]) * 0.5
    assert np.array_equal(out.cpu().numpy(), first)
    both = da.chains_batches_get(engs, 0, "mean")
    assert not np.array_equal(both, first) and _info(engs[0]) == _info(engs[1]) == (2, 1, 0)


# ---- 8. errors

def test_errors(four):
    cases, engs = four
    comps = cases[0][3]
    planes = _reg_planes(comps)
    e = engs[0]
    for l, cc in enumerate(comps):                         # earlier tests planted other samples: back to the case's own state
        e.put_amplitude(l, cc.amplitude)
        if cc.nindices:
            e.put_indices(l, cc.indices)
    lt, l2 = planes[0][0], planes[1][0]
    sel = np.zeros(len(comps), dtype=np.int32)
    sel[lt] = 1 | (1 << 3)                                 # amplitude and the first index on T
    e.moments_end()
    with pytest.raises(da.DangxError, match="dangx_moments_begin was not called"):
        e.moments_batches(planes)
    e.moments_begin(sel)
    with pytest.raises(da.DangxError, match="no batches are registered"):
        e.moments_batches_info()
    good = [(lt, 1, 0), (lt, 0, 0)]
    e.moments_batches(good, nbatch=4, batch_len=2)
    for bad, kw, match in (([(lt, 1, 1)], {}, "registration 0: a plane that is not selected"),
                           ([(l2, 2, 0)], {}, "registration 0: a plane that is not selected"),
                           ([(lt, 1, 0), (lt, 1, 0)], {}, "registration 1: the same plane twice"),
                           ([(len(comps), 0, 0)], {}, "component index out of range"),
                           ([(lt, 3, 0)], {}, "what must be 0"),
                           ([(lt, 1, 3)], {}, "plane out of range"),
                           (good, {"nbatch": 3}, "nbatch must be even and 2 .. DANGX_MAX_BATCHES \\(32\\), not 3"),
                           (good, {"nbatch": 0}, "nbatch must be even"),
                           (good, {"nbatch": 34}, "nbatch must be even"),
                           (good, {"batch_len": 0}, "batch_len must be at least 1"),
                           ([(lt, 0, 0)] * 33, {}, "more than DANGX_MAX_BATCH_PLANES")):
        with pytest.raises(da.DangxError, match="dangx_moments_batches: .*" + match):
            e.moments_batches(bad, **kw)
        assert e._moment_batches["planes"] == good          # an earlier registration survives a refused one
    # independent of pairs / hist / signals, either order
    e.moments_pairs([((lt, 0, 0), (lt, 1, 0))], lag1=True)
    e.moments_hist([(lt, 1, 0)], ranges=[(-10.0, 10.0)], nbins=16, bits=16)
    e.moments_signals([(lt, 0, 0)])
    with pytest.raises(da.DangxError, match="no sample accumulated"):
        e.moments_batches_get(0, "mean")
    for _ in range(5):
        e.moments_accumulate()
    assert _info(e) == (2, 2, 1) and e.moments_count() == 5
    assert np.isfinite(e.moments_get_pair(0, "cov")).all() and e.moments_hist_get(0).shape == (NPIX, 16)
    assert ts._same_bits(e.moments_batches_get(1, "mean"), e.moments_get(lt, 0, "mean")[0])   # five equal samples: exact
    with pytest.raises(da.DangxError, match="legal only before the first dangx_moments_accumulate"):
        e.moments_batches(good)
    out = np.full(NPIX, 7.0)
    for args, match in (((2, "mean"), "batch registration out of range \\(2 registered\\)"),
                        ((0, 5), "stat of a batch read-out must be 0"),
                        ((0, "mean", 3), "first must be 0 .. the number of full batches \\(2\\), not 3"),
                        ((0, "mean", -1), "first must be 0"),
                        ((0, "std", 0, 5), "standard deviation needs 0 <= ddof < N' \\(N' = 5\\)"),
                        ((0, "std", 2, 1), "standard deviation needs 0 <= ddof < N' \\(N' = 1\\)"),
                        ((0, "mcse", 1), "MCSE needs B' >= 2"),
                        ((0, "ess_bm", 1), "batch-means ESS needs B' >= 2"),
                        ((0, "split_rhat", 1), "split R-hat needs B' >= 2")):
        with pytest.raises(da.DangxError, match=match):
            e.moments_batches_get(*args, out=out)
        assert (out == 7.0).all()
    assert np.isnan(e.moments_batches_get(0, "split_rhat")).all()            # h L = 2: fine, and the state never moved
    with pytest.raises(da.DangxError, match="batch out of range \\(nbatch = 4\\)"):
        e.moments_batches_raw(0, 4)
    # h L >= 2 by name: batches of one sample
    e.moments_begin(sel)
    e.moments_batches(good, nbatch=4, batch_len=1)
    for _ in range(3):
        e.moments_accumulate()
    with pytest.raises(da.DangxError, match="split R-hat needs h L >= 2"):
        e.moments_batches_get(0, "split_rhat")
    assert e.moments_batches_get(0, "mcse").shape == (NPIX,)
    # nreg = 0 removes the registration; begin and end drop it
    e.moments_begin(sel)
    e.moments_batches(good)
    e.moments_batches([])
    with pytest.raises(da.DangxError, match="no batches are registered"):
        e.moments_batches_info()
    e.moments_batches(good)
    e.moments_begin(sel)
    with pytest.raises(da.DangxError, match="no batches are registered"):
        e.moments_batches_info()
    # the device form checks the same way
    e.moments_batches(good)
    e.moments_accumulate()
    dev = torch.full((NPIX,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(da.DangxError, match="MCSE needs B' >= 2"):
        e.moments_batches_get(0, "mcse", device=True, out=dev)
    torch.cuda.synchronize()
    assert (dev == 7.0).all().item()


def test_template_and_monopole_rows_are_refused(built):
    """A template / monopole / hi_fit amplitude is a row of c%template_amplitudes, not a pixel plane: refused by that name (not as
    'not selected', its rows ARE selected) through the library, whose own table of global-amplitude members dangx_moments_batches
    builds; the earlier registration survives, and goes on accumulating."""
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 3, 4), amplitudes=(3.0, -2.0, 5.0))
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    sel = da.moments_begin(dpar, ddata)
    lt, lm = len(comps) - 2, len(comps) - 1
    assert (int(sel[lt]) >> 1) & 1 and int(sel[lm]) & 1           # their rows are selected: the refusal is not 'not selected'
    planes = da.moments_batches(dpar, ddata, nbatch=4, batch_len=2)   # the defaults leave them out
    assert planes and all(l < lt for l, w, k in planes) and planes == da.default_hist_planes(dpar, comps, sel)
    for r, plane in enumerate(((lt, 0, 1), (lt, 0, 2), (lm, 0, 0))):
        with pytest.raises(da.DangxError, match="dangx_moments_batches: registration 0: a template / monopole / hi_fit amplitude is not a pixel plane"):
            eng.moments_batches([plane], nbatch=4, batch_len=2)
        with pytest.raises(da.DangxError, match="dangx_moments_batches: registration 1: a template / monopole / hi_fit amplitude is not a pixel plane"):
            eng.moments_batches([planes[0], plane])
        assert eng._moment_batches == {"planes": planes, "nbatch": 4, "batch_len": 2}     # the earlier registration stays
    for it in (1, 2, 3):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    assert _info(eng) == (2, 1, 1)
    l, what, k = planes[-1]
    mean, m2 = eng.moments_batches_raw(len(planes) - 1, 1)       # the open batch holds the third sample alone: exactly the state
    assert ts._same_bits(mean, eng.get_indices(l)[what - 1][k]) and not m2.any()
    with pytest.raises(da.DangxError, match="batch registration out of range"):
        eng.moments_batches_get(len(planes), "mean")
