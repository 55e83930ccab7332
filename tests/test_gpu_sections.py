"""Sections of the accumulator state on the device (dangx_moments_section_*, dangx_moments_begin_like): holders given a chain's
sections answer every read-out over several chains bit for bit as the live chain does; a saved and restored run continues as the
uninterrupted one; chains of another process reach the read-outs through dist_chains.  Every comparison is bit for bit."""
import datetime
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as td
import torch.multiprocessing as mp

import dang_amd as da
from dang_amd import api, synth

import test_gpu_chains as tc
import test_gpu_moments_hist as th
from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

NPIX = 192
QS = (0.16, 0.5, 0.84)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _register(p, d, nbins=16, bits=16, nbatch=4, batch_len=1, lag1=True, ranges=None):
    reg = {"sel": da.moments_begin(p, d), "pairs": da.moments_pairs(p, d, lag1=lag1)}
    reg["hist"] = da.moments_hist(p, d, nbins=nbins, bits=bits, ranges=ranges)
    reg["specs"] = da.moments_signals(p, d)
    reg["batches"] = da.moments_batches(p, d, nbatch=nbatch, batch_len=batch_len)
    return reg


def _chain(seed, sign, nsamples, nbins=16, bits=16):
    """a whole-sky C2 chain at Nside 4 from a dispersed start with every registration, `nsamples` samples taken"""
    case = make_case("C2", nside=4)
    dpar, ddata = case[0], case[1]
    dpar.seed = seed
    eng = tc._engine(case)
    if sign:
        tc._disperse(eng, sign)
    reg = _register(dpar, ddata, nbins, bits)
    for it in range(1, nsamples + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    return eng, reg


def _export(live, holder, device=True):
    """every section of `live`, one at a time, into `holder` (made a holder like `live` here)"""
    holder.moments_begin_like(live)
    holder.moments_section_put("HEAD", 0, 0, live.moments_section_get("HEAD"))
    for f, a, b in live.moments_sections():
        buf = live.moments_section_get(f, a, b, device=device)
        assert (buf.numel() if device else buf.size) == live.moments_section_bytes(f, a, b)
        if device:
            live.synchronize()
        holder.moments_section_put(f, a, b, buf)
        holder.synchronize()
    return holder


def _readouts(engs, reg, equal=True, batches=True):
    """every read-out family over the chains `engs`, for every stat each accepts"""
    out = {}
    e0 = engs[0]
    for l, c in enumerate(e0.component_list):
        for what in range(1 + c.nindices):
            if not (int(reg["sel"][l]) >> (0 if what == 0 else 3 + 3 * (what - 1))) & 7:
                continue
            for stat in range(6):
                if stat in (2, 3, 4) and not equal:
                    continue
                glob = what == 0 and c.type in tc.GLOBAL
                out[("get", l, what, stat)] = da.chains_get_template(engs, l, stat, 1) if glob else da.chains_get(engs, l, what, stat, 1)
    for s in range(len(reg["specs"])):
        for stat in range(5 if equal else 2):
            out[("signal", s, stat)] = da.chains_get_signal(engs, s, stat, 1)
    for p in range(len(reg["pairs"])):
        for stat in (0, 1):
            out[("pair", p, stat)] = da.chains_get_pair(engs, p, stat, 1)
    for r in range(len(reg["hist"])):
        out[("hist", r, "q")] = da.chains_hist_stat(engs, r, "quantile", q=QS)
        out[("hist", r, "mode")] = da.chains_hist_stat(engs, r, "mode")
        out[("hist", r, "n")] = da.chains_hist_stat(engs, r, "n")
        for stat in range(3):
            out[("rank", r, stat)] = da.chains_hist_rank(engs, r, stat)
    if batches and equal:
        for r in range(len(reg["batches"])):
            for first in (0, 1):
                for stat in range(5):
                    out[("batch", r, stat, first)] = da.chains_batches_get(engs, r, stat, first, 1)
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys() and len(a) > 20
    assert any(np.isfinite(v).any() for v in a.values())
    for key in a:
        assert _same(a[key], b[key]), (what, key)


# ---- 1. holders equal live chains

@pytest.mark.parametrize("nbins,bits", [(16, 16), (8, 32)])
def test_holders_equal_live_chains(built, nbins, bits):
    runs = [_chain(1234 + k, sign, 8, nbins, bits) for k, sign in enumerate((0, 1, -1))]
    (A, reg), (B, _), (C, _) = runs
    assert reg["pairs"] and reg["hist"] and reg["specs"] and reg["batches"] and A._moment_lag1
    want = _readouts([A, B, C], reg)
    Bh, Ch = _export(B, api._holder_engine(B)), _export(C, api._holder_engine(C))
    assert Bh.moments_count() == 8 and Bh.moments_batches_info() == B.moments_batches_info()
    _assert_same(_readouts([A, Bh, Ch], reg), want, "holders behind a live chain")
    # a holder at position 0 (the read-out runs on its stream, through its scratch buffer)
    Ah = _export(A, api._holder_engine(A))
    _assert_same(_readouts([Ah, B, Ch], reg), want, "a holder at position 0")
    _assert_same(_readouts([Ah, Bh, Ch], reg), want, "holders only")
    # the maps by name take holders as they take live chains
    pm, ph = da.chains_posterior_maps([[A], [B], [C]], ddof=1), da.chains_posterior_maps([[Ah], [Bh], [C]], ddof=1)
    assert list(pm) == list(ph) and all(_same(pm[k][s], ph[k][s]) for k in pm for s in ("mean", "std", "rhat", "W", "B", "ess"))
    # the device form of a get and the host form give the same bytes, and a section put back into its live chain changes nothing
    for f, a, b in A.moments_sections():
        host = A.moments_section_get(f, a, b)
        dev = A.moments_section_get(f, a, b, device=True)
        A.synchronize()
        assert _same(host, dev.cpu().numpy()), (f, a, b)
        A.moments_section_put(f, a, b, dev)
        A.synchronize()
    _assert_same(_readouts([A, B, C], reg), want, "after putting a chain's sections back into it")


def test_holders_with_unequal_counts(built):
    runs = [_chain(77 + k, sign, n) for k, (sign, n) in enumerate(((0, 5), (1, 8), (-1, 2)))]
    (A, reg), (B, _), (C, _) = runs
    want = _readouts([A, B, C], reg, equal=False)
    Bh, Ch = _export(B, api._holder_engine(B)), _export(C, api._holder_engine(C))
    assert [e.moments_count() for e in (A, Bh, Ch)] == [5, 8, 2]
    _assert_same(_readouts([A, Bh, Ch], reg, equal=False), want, "unequal counts")
    with pytest.raises(da.DangxError, match="equal sample counts"):
        da.chains_get([A, Bh, Ch], 1, 0, "rhat")


def test_template_rows_through_holders(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    runs = [(dpar, ddata)] + [da.open_chain(dpar, ddata, 500 + k) for k in (1, 2)]
    lt = len(comps) - 1
    for p, d in runs:
        reg = {"sel": da.moments_begin(p, d), "pairs": da.moments_pairs(p, d), "hist": [], "specs": [], "batches": []}
    for it in range(1, 7):
        for p, d in runs:
            da.gibbs_iteration(p, d, it)
            da.moments_accumulate(d)
    engs = [d.engine for _, d in runs]
    assert (int(reg["sel"][lt]) & 7) == 6                                                    # the template's Q and U rows
    assert engs[1].moments_section_bytes("PLANES", lt, 0) == 5 * 2 * meta["nbands"] * 8      # ... in five parts
    want = _readouts(engs, reg)
    assert np.isfinite(want[("get", lt, 0, 0)][1:, [2, 3, 4]]).all() and not _same(want[("get", lt, 0, 1)][1:, [2, 3, 4]], np.zeros((2, 3)))
    for device in (False, True):
        holders = [_export(e, api._holder_engine(e), device=device) for e in engs[1:]]
        _assert_same(_readouts([engs[0]] + holders, reg), want, "template run, device %s" % device)
    _assert_same(_readouts([holders[0], engs[0], holders[1]], reg), _readouts([engs[1], engs[0], engs[2]], reg), "template rows, a holder at 0")
    empty = api._holder_engine(engs[1])
    empty.moments_begin_like(engs[1])
    empty.moments_section_put("HEAD", 0, 0, engs[1].moments_section_get("HEAD"))
    with pytest.raises(da.DangxError, match=r"chain 1: section PLANES\(%d, 0\) was not put" % lt):
        da.chains_get_template([engs[0], empty], lt, "mean")


# ---- 2. an odd shard at an odd pix0, through the host forms

def test_odd_shard_through_the_host_forms(built):
    cases = [make_case("C2", nside=4) for _ in range(3)]
    dpar, ddata, bands, comps, meta = cases[0]
    bounds = [0, 1, 96, NPIX]                            # the middle shard: pixels 1..95
    planes = th._hist_planes(comps)
    ranges = [(th._offset(l, w) - th.HALF, th._offset(l, w) + th.HALF) for l, w, k in planes]
    specs = da.default_signal_specs(dpar, comps, bands)
    mid, reg = [], None
    for k in range(3):
        shards = shard_engines(cases[k], 3, bounds=bounds)
        for e in shards:
            e.moments_begin(None)
            pairs = da.default_moment_pairs(dpar, comps, e._moment_sel)
            e.moments_pairs(pairs, lag1=True)
            e.moments_hist(planes, ranges=ranges, nbins=16, bits=16)
            e.moments_signals(specs)
            e.moments_batches(planes[:2], nbatch=4, batch_len=1)
        th._feed(shards, list(zip(bounds[:-1], bounds[1:])), comps, th._synthetic_states(comps, meta, 6, seed=5 + k, nbins=16), 6)
        mid.append(shards[1])
        reg = {"sel": shards[1]._moment_sel, "pairs": pairs, "hist": planes, "specs": specs, "batches": planes[:2]}
    assert mid[0].npix == 95 and mid[0].pix0 == 1
    want = _readouts(mid, reg)
    holders = [_export(e, api._holder_engine(e), device=False) for e in mid[1:]]
    # a holder's planes are packed: with 95 pixels consecutive planes alternate their 16-byte phase, the live planes do not
    assert mid[0].moments_section_bytes("PLANES", 1, 0) == 5 * 3 * 95 * 8 and mid[0].moments_section_bytes("HIST", 0, 0) == 95 * 32
    _assert_same(_readouts([mid[0]] + holders, reg), want, "odd shard")
    _assert_same(_readouts([holders[1], mid[0], holders[0]], reg), _readouts([mid[2], mid[0], mid[1]], reg), "odd shard, a holder at position 0")


# ---- 3. holder memory and refusals

def test_holder_memory_and_refusals(built):
    runs = [_chain(900 + k, sign, 4) for k, sign in enumerate((0, 1))]
    (A, reg), (B, _) = runs
    for e in (A, B):
        e.profile(True)
    A.synchronize(); B.synchronize()
    mark = [tc._launches(e) for e in (A, B)]
    held = [tc._accumulators(e, len(reg["pairs"]), len(reg["hist"]), len(reg["specs"])) for e in (A, B)]
    mark = [tc._launches(e) for e in (A, B)]
    H = api._holder_engine(B)
    H.moments_begin_like(B)
    assert H.moments_held_bytes() == 0 and A.moments_held_bytes() == 0
    with pytest.raises(da.DangxError, match="chain 1: section HEAD was not put"):
        da.chains_get([A, H], 5, 1, "mean")
    H.moments_section_put("HEAD", 0, 0, B.moments_section_get("HEAD"))
    H.moments_section_put("PLANES", 5, 1, B.moments_section_get("PLANES", 5, 1))
    H.moments_section_put("HIST", 0, 0, B.moments_section_get("HIST", 0, 0, device=True))
    H.synchronize()
    r256 = lambda n: -(-n // 256) * 256
    assert H.moments_held_bytes() == r256(B.moments_section_bytes("PLANES", 5, 1)) + r256(B.moments_section_bytes("HIST", 0, 0))
    assert B.moments_section_bytes("PLANES", 5, 1) == 5 * 2 * NPIX * 8 and B.moments_section_bytes("HIST", 0, 0) == NPIX * 32
    assert _same(da.chains_get([A, H], 5, 1, "rhat"), da.chains_get([A, B], 5, 1, "rhat"))
    assert _same(da.chains_hist_rank([A, H], 0, "max"), da.chains_hist_rank([A, B], 0, "max"))
    # a read-out that needs a section that was not put: by name, and nothing is written
    out = np.full((3, NPIX), 7.0)
    with pytest.raises(da.DangxError, match=r"chain 1: section PLANES\(5, 0\) was not put into this holder"):
        da.chains_get([A, H], 5, 0, "mean", out=out)
    assert (out == 7.0).all()
    with pytest.raises(da.DangxError, match=r"chain 1: section HIST\(1\) was not put"):
        da.chains_hist_stat([A, H], 1, "mode")
    with pytest.raises(da.DangxError, match=r"chain 0: section PAIR\(0\) was not put"):
        da.chains_get_pair([H, A], 0, "corr")
    with pytest.raises(da.DangxError, match=r"section SIGNAL\(0\) was not put"):
        da.chains_get_signal([A, H], 0, "mean")
    with pytest.raises(da.DangxError, match=r"section BATCHES\(0\) was not put"):
        da.chains_batches_get([A, H], 0, "mean")
    # mean and m2 alone: R-hat is served, the pooled ESS names what is missing
    H.moments_section_put("PLANES", 5, 2, B.moments_section_get("PLANES", 5, 2)[:2 * 2 * NPIX * 8].copy())
    assert _same(da.chains_get([A, H], 5, 2, "rhat"), da.chains_get([A, B], 5, 2, "rhat"))
    with pytest.raises(da.DangxError, match=r"section PLANES\(5, 2\) with its lag-1 parts was not put"):
        da.chains_get([A, H], 5, 2, "ess")
    with pytest.raises(da.DangxError, match="holder"):
        H.moments_accumulate()
    with pytest.raises(da.DangxError, match="holder"):
        H.moments_get(5, 1, "mean")
    with pytest.raises(da.DangxError, match=r"section PAIR\(0\) is %d bytes, not %d" % (NPIX * 8, NPIX * 8 - 8)):
        H.moments_section_put("PAIR", 0, 0, np.zeros(NPIX * 8 - 8, dtype=np.uint8))
    with pytest.raises(da.DangxError, match="bytes, not"):
        A.moments_section_put("HIST", 0, 0, np.zeros(NPIX * 32 + 4, dtype=np.uint8))
    with pytest.raises(da.DangxError, match="host section"):
        H.moments_section_get("HEAD", 0, 0, device=True, out=torch.zeros(104, dtype=torch.uint8, device="cuda"))
    # a HEAD of another registration is refused, naming what differs -- by a live context and by a holder alike
    case = make_case("C2", nside=4)
    other = tc._engine(case)
    lo, hi = A._moment_hist["ranges"][0]
    n = len(reg["hist"])
    for kw, match in ((dict(ranges=[(lo, hi + 0.5)] + [None] * (n - 1)), "histogram registrations"), (dict(nbatch=6), "nbatch is 6 there and 4 here"),
                      (dict(lag1=False), "lag-1 is missing there and tracked here")):
        _register(case[0], case[1], **kw)
        da.moments_accumulate(case[1])
        head = other.moments_section_get("HEAD")
        for target in (A, H):
            with pytest.raises(da.DangxError, match=match):
                target.moments_section_put("HEAD", 0, 0, head)
    with pytest.raises(da.DangxError, match="truncated or foreign|bytes, not"):
        A.moments_section_put("HEAD", 0, 0, B.moments_section_get("HEAD")[:-1].copy())
    assert A.moments_count() == 4 and H.moments_count() == 4
    H.moments_begin_like(B)
    assert H.moments_held_bytes() == 0
    # nothing moved on the live chains: no launch but the read-outs' own on the first chain, every accumulator as it was
    A.synchronize(); B.synchronize()
    now = [tc._launches(e) for e in (A, B)]
    assert now[0].pop("k_chains") > 0 and "k_chains" not in now[1]
    mark[0].pop("k_chains", None)
    assert now == mark
    for e, h in zip((A, B), held):
        g = tc._accumulators(e, len(reg["pairs"]), len(reg["hist"]), len(reg["specs"]))
        for key in h:
            if key != "state":
                assert _same(np.asarray(h[key], dtype=np.float64), np.asarray(g[key], dtype=np.float64)), key


# ---- 4. save / restore continues the run

def _template_run():
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    reg = _register(dpar, ddata, nbatch=4, batch_len=1)
    return dpar, ddata, reg


def _single_readouts(ddata):
    out = {}
    for key, e in da.posterior_maps(ddata, ddof=1).items():
        out.update({("moments", key, s): e[s] for s in ("mean", "std", "rho1", "ess")})
    out.update({("pair", key): v for key, v in da.posterior_pair_maps(ddata).items()})
    for key, e in da.posterior_quantile_maps(ddata).items():
        out.update({("hist", key, s): e[s] for s in ("q", "mode", "n")})
    for key, e in da.posterior_signal_maps(ddata, ddof=1).items():
        out.update({("signal", key, s): e[s] for s in ("mean", "std")})
    for first in (0, 1):
        for key, e in da.posterior_batch_maps(ddata, first=first, ddof=1).items():
            out.update({("batch", first, key, s): v for s, v in e.items() if isinstance(v, np.ndarray)})
            out[("batch", first, key, "info")] = np.array([e["batch_len"], e["nfull"], e["partial"]])
    return out


def test_save_restore_continues_the_run(built, tmp_path):
    dpar, A, reg = _template_run()
    for it in range(1, 12):
        da.gibbs_iteration(dpar, A, it)
        da.moments_accumulate(A)
    want = _single_readouts(A)
    lt = len(A.engine.component_list) - 1
    assert ("moments", ("tmpl", "amplitude"), "rho1") in want and want[("moments", ("tmpl", "amplitude"), "mean")].shape[1] == A.engine.nbands
    dpar, B, _ = _template_run()
    for it in range(1, 6):
        da.gibbs_iteration(dpar, B, it)
        da.moments_accumulate(B)
    assert B.engine.moments_batches_info() == {"batch_len": 2, "nfull": 2, "partial": 1}   # one merge behind, a batch half full
    path = str(tmp_path / "run.moments")
    da.moments_save(B, path)
    e = B.engine
    state = [(e.get_amplitude(l), e.get_indices(l) if c.nindices else None,
              e.get_template_amplitudes(l) if c.type in tc.GLOBAL else None) for l, c in enumerate(e.component_list)]
    e.moments_end()
    # a fresh engine: the same registrations, the chain state pushed, the accumulators loaded
    dpar, R, _ = _template_run()
    for l, (a, x, ta) in enumerate(state):
        R.engine.put_amplitude(l, a)
        if x is not None:
            R.engine.put_indices(l, x)
        if ta is not None:
            R.engine.put_template_amplitudes(l, ta)
    da.moments_load(R, path)
    assert R.engine.moments_count() == 5 and R.engine.moments_batches_info() == {"batch_len": 2, "nfull": 2, "partial": 1}
    for it in range(6, 12):
        da.gibbs_iteration(dpar, R, it)
        da.moments_accumulate(R)
    assert R.engine.moments_batches_info() == {"batch_len": 4, "nfull": 2, "partial": 3}   # the second merge fell after the restore
    got = _single_readouts(R)
    assert got.keys() == want.keys() and len(want) > 40
    for key in want:
        assert _same(got[key], want[key]), key
    assert lt > 0
    # a context registered differently refuses the file, naming the difference, and keeps what it holds
    dpar, D, _ = _template_run()
    _register(dpar, D, nbatch=6)
    da.moments_accumulate(D)
    with pytest.raises(da.DangxError, match="nbatch is 4 there and 6 here"):
        da.moments_load(D, path)
    assert D.engine.moments_count() == 1
    open(path + ".cut", "wb").write(open(path, "rb").read()[:-9])
    with pytest.raises(da.DangxError, match="truncated"):
        da.moments_load(R, path + ".cut")


# ---- 5. two processes

SEEDS = (4321, 4322)
MAPS = (("posterior", lambda c: da.chains_posterior_maps(c, ddof=1)), ("pair", da.chains_pair_maps), ("quantile", da.chains_quantile_maps),
        ("rank", da.chains_rank_maps), ("batch", lambda c: da.chains_batch_maps(c, first=1, ddof=1)), ("signal", lambda c: da.chains_signal_maps(c, ddof=1)))


def _flat(maps):
    out = {}
    for key, e in maps.items():
        if isinstance(e, dict):
            out.update({repr((key, s)): np.asarray(v) for s, v in e.items() if isinstance(v, np.ndarray)})
        else:
            out[repr(key)] = np.asarray(e)
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    # the chain runs before the process group exists: its sampling has no sum over the ranks (each rank holds the whole sky)
    eng, reg = _chain(SEEDS[rank], (0, 1)[rank], 6)
    td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    res = {}
    dc = da.dist_chains([[eng]], dst=0)
    for name, fn in MAPS:
        m = fn(dc)
        assert (m is None) == (rank != 0), name
        if m is not None:
            res.update({name + ":" + k: v for k, v in _flat(m).items()})
        if name == "rank":
            # the holders never held more than ONE registration's records per remote chain
            res["peak"] = np.array([dc.peak_held, -(-eng.moments_section_bytes("HIST", 0, 0) // 256) * 256, len(reg["hist"])])
    both = da.dist_chains([[eng]], dst=None)
    res.update({"all:" + k: v for k, v in _flat(da.chains_rank_maps(both)).items()})
    res.update({"all:" + k: v for k, v in _flat(da.chains_posterior_maps(both, ddof=1)).items()})
    # a rank registered differently: BOTH ranks raise, at once (no rank waits in a collective for the other)
    case = make_case("C2", nside=4)
    odd = tc._engine(case)
    _register(case[0], case[1], nbatch=6 if rank == 1 else 4)
    da.moments_accumulate(case[1])
    t0 = time.time()
    try:
        da.dist_chains([[odd]], dst=0)
        res["mismatch"] = np.array(["no error"])
    except da.DangxError as ex:
        res["mismatch"] = np.array([str(ex)])
    res["mismatch_seconds"] = np.array([time.time() - t0])
    np.savez(out + ".%d.npz" % rank, **res)
    td.barrier()
    td.destroy_process_group()


def _spawn(fn, args, nprocs, limit):
    """mp.spawn under a time limit of its own: workers that outlive it are ended and the test fails"""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.time() + limit
    while not ctx.join(timeout=1.0):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the spawned ranks did not finish within %d s" % limit)


def test_two_processes(built, tmp_path):
    out = str(tmp_path / "res")
    _spawn(_dist_worker, (2, _free_port(), out), 2, 120)
    r0, r1 = (np.load(out + ".%d.npz" % r) for r in (0, 1))
    # one process, the same two chains run locally with the same seeds
    local = [[_chain(SEEDS[k], (0, 1)[k], 6)[0]] for k in range(2)]
    want = {}
    for name, fn in MAPS:
        want.update({name + ":" + k: v for k, v in _flat(fn(local)).items()})
    assert len(want) > 40 and any(k.startswith("batch:") for k in want) and any(k.startswith("rank:") for k in want)
    assert sorted(k for k in r0.files if ":" in k and not k.startswith("all:")) == sorted(want)
    for k, v in want.items():
        assert _same(r0[k], v), k
    assert not [k for k in r1.files if ":" in k and not k.startswith("all:")]          # rank 1 got None
    # dst=None: both ranks hold the maps, and they are the one-process maps (rank 1 reads rank 0's chain through a holder at 0)
    for r in (r0, r1):
        got = [k for k in r.files if k.startswith("all:")]
        assert len(got) > 10
        for k in got:
            name = ("rank:" if "rhat_" in k else "posterior:") + k[4:]
            assert _same(r[k], want[name]), k
    for r in (r0, r1):
        assert "registered differently" in str(r["mismatch"][0]) and "nbatch is 6 there and 4 here" in str(r["mismatch"][0])
        assert float(r["mismatch_seconds"][0]) < 30
    peak, one, nreg = (int(v) for v in r0["peak"])
    assert nreg >= 2 and peak == one
    assert int(r1["peak"][0]) == 0
