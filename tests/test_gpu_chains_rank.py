"""Rank-normalised and folded R-hat read from the histograms of several chains on the device (dangx_chains_hist_rank,
k_chains_rank): closed forms planted through real accumulation, the long-double reference of tests/rank_ref.py on the records the
chains hold, the case the statistic exists for (chains that agree in the mean and differ in spread), the shapes of the launch,
dx_norm_ppf evaluated on the device, everything else left as it is, streams and the error cases.

Samples are planted on one index plane with put_indices + moments_accumulate; with the range (0, nbins) the bin of x is floor(x)."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import dang_amd as da

import chains_ref as cr
import rank_ref as rr
from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = cr.EPS
NPIX = 192
STATS = ("bulk", "folded", "max")
LC = 1          # the component whose first index carries the planted samples (C2: synch)


def _engine(case, stream=None):
    dpar, ddata, bands, comps, meta = case
    kw = {} if stream is None else {"stream": stream}
    return da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0, **kw)


@pytest.fixture(scope="module")
def eight(built):
    """eight independent whole-sky C2 contexts at Nside 4; every test restarts their accumulators"""
    cases = [make_case("C2", nside=4) for _ in range(8)]
    assert cases[0][3][LC].nindices >= 1
    return [_engine(c) for c in cases]


def _begin(engs, lo, hi, nbins, bits, hist=True):
    sel = np.zeros(len(engs[0].component_list), dtype=np.int32)
    sel[LC] = 1 << 3                                   # index 1 on T
    for e in engs:
        e.moments_begin(sel)
        if hist:
            e.moments_hist([(LC, 1, 0)], ranges=[(lo, hi)], nbins=nbins, bits=bits)


def _plant(e, xs, sl=slice(None)):
    """xs [n][npix of the sky]: one accumulation per sample, the shard's pixels sl"""
    nind = e.component_list[LC].nindices
    for x in xs:
        ind = np.empty((nind, 3, e.npix))
        ind[:] = x[sl]
        e.put_indices(LC, ind)
        e.moments_accumulate()


def _records(engs):
    return np.stack([e.moments_hist_get(0).astype(np.int64) for e in engs])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. closed forms

def test_closed_forms_through_real_accumulation(eight):
    """pixels i % 3 == 0: both chains hold the same samples, R-hat^2 = (n - 1)/n; == 1: bins a < b, chain 0 holds 7 samples in a
    and 1 in b, chain 1 the mirror image, R-hat^2 = 7/8 + 36/16 = 3.125 for every stat; == 2: each chain in one bin, +inf where
    the two bins differ and NaN where they do not"""
    engs, n, nbins = eight[:2], 8, 8
    rng = np.random.default_rng(1)
    pix = np.arange(NPIX)
    x = np.empty((2, n, NPIX))
    same = rng.integers(0, nbins, (n, NPIX)) + 0.5
    a, b = pix % 5, 5 + pix % 3                                        # a < b
    t = np.arange(n)[:, None]
    two = [np.where(t < n - 1, a, b) + 0.25, np.where(t < 1, a, b) + 0.75]
    one = [np.broadcast_to(pix % 7 + 0.5, (n, NPIX)), np.broadcast_to((pix % 7 + (pix // 3) % 2) + 0.5, (n, NPIX))]
    for k in range(2):
        x[k] = np.where(pix % 3 == 0, same, np.where(pix % 3 == 1, two[k], one[k]))
    _begin(engs, 0.0, float(nbins), nbins, 16)
    for k, e in enumerate(engs):
        _plant(e, x[k])
    rec = _records(engs)
    assert (rec.sum(axis=2) == n).all()
    apart = (pix % 3 == 2) & ((pix // 3) % 2 == 1)
    together = (pix % 3 == 2) & ~apart
    assert apart.sum() > 10 and together.sum() > 10
    for st in STATS:
        r = da.chains_hist_rank(engs, 0, st)
        assert r.shape == (NPIX,)
        m = pix % 3 == 0
        moved = m & ((rec[0] > 0).sum(axis=1) > 1)                      # eight samples in one bin: a trace that never moved
        assert moved.sum() > 50 and np.isnan(r[m & ~moved]).all()
        assert (np.abs(r[moved] ** 2 - 7 / 8) <= 64 * EPS * 7 / 8).all(), st
        m = pix % 3 == 1
        assert (np.abs(r[m] ** 2 - 3.125) <= 64 * EPS * 3.125).all(), (st, r[m])
        assert (r[apart] == np.inf).all() and np.isnan(r[together]).all(), st


# ---- 2. against the long-double reference on the records

def _binned_samples(rng, K, n, nbins):
    """[K][n][NPIX] in (0, nbins): chains of a pixel about neighbouring centres with one spread; a few samples leave the range"""
    width = rng.uniform(0.4, nbins / 5.0, NPIX)
    centre = rng.uniform(0.3 * nbins, 0.7 * nbins, NPIX) + rng.normal(0.0, 0.4, (K, 1, NPIX)) * width
    x = np.clip(centre + width * rng.standard_normal((K, n, NPIX)), 0.01, nbins - 0.01)
    x[1, n // 2, 3] = nbins + 1.0                       # chain 1 loses a sample of pixel 3 above the range,
    x[0, 1, 50] = np.nan                                # chain 0 one of pixel 50,
    x[K - 1, 2, 100] = -0.5                             # the last chain one of pixel 100 below it
    return x


def _counts_of(x, nbins):
    """the records the definition of a bin gives for samples in the range (0, nbins): [K][NPIX][nbins]"""
    K, n, npix = x.shape
    c = np.zeros((K, npix, nbins), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = (x >= 0) & (x <= nbins)
    for k in range(K):
        for t in range(n):
            p = np.flatnonzero(ok[k, t])
            np.add.at(c[k], (p, np.minimum(x[k, t, p].astype(np.int64), nbins - 1)), 1)
    return c


@pytest.mark.parametrize("nbins,bits", [(8, 16), (64, 16), (32, 32)])
def test_against_the_reference(eight, nbins, bits):
    n = 16
    x = _binned_samples(np.random.default_rng(nbins + bits), 8, n, nbins)
    _begin(eight, 0.0, float(nbins), nbins, bits)
    for k, e in enumerate(eight):
        _plant(e, x[k])
    rec = _records(eight)
    assert np.array_equal(rec, _counts_of(x, nbins))
    for K in (2, 3, 8):
        for st in STATS:
            r = da.chains_hist_rank(eight[:K], 0, st)
            ref = rr.compare(r, rec[:K], st, "K %d nbins %d bits %d %s" % (K, nbins, bits, st), min_finite=0.95)
            assert np.isnan(r[[3, 50]]).all() and np.isnan(r[100]) == (K == 8)     # where a chain holds a sample less
            assert (np.isfinite(ref) & (ref > 1.0)).sum() > 20


# ---- 3. what it is for

def _spread_samples(seed=4, K=4, n=64):
    """[K][n][NPIX] about one centre per pixel; chain 0 three times as wide as the others"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((K, n, NPIX))
    x[0] *= 3.0
    return x


def test_chains_that_agree_in_the_mean_and_differ_in_spread(eight):
    engs, nbins = eight[:4], 64
    x = _spread_samples()
    assert np.abs(x).max() < 15.0                                       # the range covers every planted sample
    # the reference first: the classic R-hat sees nothing, the folded one does
    classic = cr.between([x[k] for k in range(4)])
    counts = _counts_of((x + 15.0) * (nbins / 30.0), nbins)
    folded2, _ = rr.rhat2(counts, "folded")
    assert np.median(np.sqrt(classic["rhat2"][0])) < 1.01 and np.median(np.sqrt(folded2)) > 1.1
    _begin(engs, -15.0, 15.0, nbins, 16)
    for k, e in enumerate(engs):
        _plant(e, x[k])
    rec = _records(engs)
    assert (rec.sum(axis=2) == 64).all()
    c = da.chains_get(engs, LC, 1, "rhat")[0]
    cr.compare_rhat(c, classic, "classic R-hat^2, one chain three times as wide", min_finite=1.0)
    f = da.chains_hist_rank(engs, 0, "folded")
    rr.compare(f, rec, "folded", "folded R-hat^2, one chain three times as wide", min_finite=1.0)
    assert np.median(f) > 1.1 and np.median(c) < 1.01
    m = da.chains_hist_rank(engs, 0, "max")
    assert _same_bits(m, np.maximum(f, da.chains_hist_rank(engs, 0, "bulk")))
    maps = da.chains_rank_maps([[e] for e in engs])
    comp = engs[0].component_list[LC]
    key = (comp.label, comp.ind_label[0], 0)
    assert list(maps) == [key] and maps[key]["nbins"] == 64 and maps[key]["range"] == (-15.0, 15.0)
    assert _same_bits(maps[key]["rhat_folded"], f) and _same_bits(maps[key]["rhat_max"], m)


# ---- 4. the shapes of the launch

def test_shards_device_form_and_determinism(built):
    """Nside 8 in two shards of 385 + 383 pixels (more than one block, a partial last wave) against the whole sky"""
    K, n, nbins = 2, 6, 32
    npix = 768
    bounds = [0, 385, npix]
    cases = [make_case("C2", nside=8) for _ in range(K)]
    whole = [_engine(c) for c in cases]
    sharded = [shard_engines(c, 2, bounds=bounds) for c in cases]      # [chain][shard]
    rng = np.random.default_rng(12)
    width = rng.uniform(0.5, 6.0, npix)
    x = np.clip(16.0 + rng.normal(0, 1.0, (K, 1, npix)) * width + width * rng.standard_normal((K, n, npix)), 0.01, nbins - 0.01)
    x[1, 2, 384] = nbins + 3.0                                          # the last pixel of the first shard loses a sample
    _begin(whole + [e for ch in sharded for e in ch], 0.0, float(nbins), nbins, 16)
    for k in range(K):
        _plant(whole[k], x[k])
        for s, e in enumerate(sharded[k]):
            _plant(e, x[k], slice(bounds[s], bounds[s + 1]))
    for st in STATS:
        w = da.chains_hist_rank(whole, 0, st)
        assert w.shape == (npix,) and np.isnan(w[384]) and np.isfinite(w).sum() > 700
        parts = [da.chains_hist_rank([ch[s] for ch in sharded], 0, st) for s in range(2)]
        assert parts[0].shape == (385,) and parts[1].shape == (383,)
        assert _same_bits(np.concatenate(parts), w), st
        assert _same_bits(da.chains_hist_rank(whole, 0, st), w), (st, "two calls")
        d = da.chains_hist_rank(whole, 0, st, device=True)
        whole[0].synchronize()
        assert _same_bits(d.cpu().numpy(), w), (st, "device form")
        d = da.chains_hist_rank([ch[1] for ch in sharded], 0, st, device=True)
        sharded[0][1].synchronize()
        assert _same_bits(d.cpu().numpy(), w[385:]), (st, "device form of a shard")
    maps = da.chains_rank_maps(sharded)
    (key, e), = maps.items()
    assert _same_bits(e["rhat_max"], da.chains_hist_rank(whole, 0, "max")) and e["rhat_rank"].shape == (npix,)
    rr.compare(da.chains_hist_rank(whole, 0, "max"), _records(whole), "max", "Nside 8 max", min_finite=0.95)


# ---- 5. dx_norm_ppf on the device

PPF_PROGRAM = r'''
#include <hip/hip_runtime.h>
#include "dx_rank_host.h"
#include <cstdio>
#include <vector>

__global__ void k_ppf(const double* p, double* z, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) z[i] = dx_norm_ppf(p[i]);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long long n = ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    if (n <= 0) return 4;
    std::vector<double> h((size_t)n), o((size_t)n);
    if (fread(h.data(), 8, (size_t)n, f) != (size_t)n) return 4;
    fclose(f);
    double *din, *dout;
    if (hipMalloc(&din, n * 8) != hipSuccess || hipMalloc(&dout, n * 8) != hipSuccess) return 5;
    if (hipMemcpy(din, h.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess) return 6;
    k_ppf<<<(unsigned)((n + 255) / 256), 256>>>(din, dout, n);
    if (hipDeviceSynchronize() != hipSuccess) return 7;
    if (hipMemcpy(o.data(), dout, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return 8;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(o.data(), 8, (size_t)n, f) != (size_t)n) return 9;
    fclose(f);
    (void)hipFree(din); (void)hipFree(dout);
    return 0;
}
'''


def test_norm_ppf_on_the_device(built):
    """a stand-alone HIP program, one child process under its own timeout; nothing is started after it"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    p = rr.ppf_points(400)
    with tempfile.TemporaryDirectory(prefix="dx_rank_ppf_") as d:
        src, exe, fin, fout = (os.path.join(d, f) for f in ("ppf.hip", "ppf", "in.bin", "out.bin"))
        with open(src, "w") as f:
            f.write(PPF_PROGRAM)
        subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "dang_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "include"), "-o", exe, src], check=True, timeout=600)
        p.tofile(fin)
        r = subprocess.run([exe, fin, fout], timeout=120)
        assert r.returncode == 0, "the device program ended with status %d" % r.returncode
        z = np.fromfile(fout, dtype=np.float64)
    assert z.shape == p.shape and z[-1] == 0.0 and (z >= 0).all()
    err = np.abs(z.astype(rr.LD) - rr.ppf_ref(p))
    print("dx_norm_ppf (device): worst |error| %.3g of the stated %.3g" % (float(err.max()), rr.PPF_BOUND))
    assert (err <= rr.PPF_BOUND).all()


# ---- 6. nothing else moves

def _launches(eng):
    return {k: v["launches"] for k, v in eng.profile_get().items()}


def _held(e):
    return {"idx": e.get_indices(LC), "amp": e.get_amplitude(LC), "mean": e.moments_get(LC, 1, "mean"), "std": e.moments_get(LC, 1, "std"),
            "hist": e.moments_hist_get(0).astype(np.float64), "n": e.moments_hist_stat(0, "n"), "count": np.float64(e.moments_count())}


def test_nothing_else_moves(eight):
    engs = eight[:3]
    x = _binned_samples(np.random.default_rng(9), 3, 5, 16)
    for e in engs:
        e.profile(True)
    try:
        _begin(engs, 0.0, 16.0, 16, 16)
        for k, e in enumerate(engs):
            _plant(e, x[k])
        held = [_held(e) for e in engs]
        mark = [_launches(e) for e in engs]
        for st in STATS:
            da.chains_hist_rank(engs, 0, st)
        da.chains_hist_rank(engs, 0, "max", device=True)
        engs[0].synchronize()
        now = [_launches(e) for e in engs]
        assert now[0].pop("k_chains") - mark[0].pop("k_chains", 0) == 4           # under their own id, on the first chain's context
        assert now == mark                                                         # every other id of every chain as it was
        for e, h in zip(engs, held):
            g = _held(e)
            for key in h:
                assert _same_bits(h[key], g[key]), key
    finally:
        for e in engs:
            e.profile(False)


# ---- 7. streams

def test_streams(built):
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    engs = [_engine(make_case("C2", nside=4), s.cuda_stream) for s in (s0, s1)]
    x = _binned_samples(np.random.default_rng(21), 2, 12, 16)
    _begin(engs, 0.0, 16.0, 16, 32)
    for k, e in enumerate(engs):
        _plant(e, x[k, :6])
    first = da.chains_hist_rank(engs, 0, "max")
    assert np.isfinite(first).sum() > 150
    out = torch.full((NPIX,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert da.chains_hist_rank(engs, 0, "max", device=True, out=out) is out
    for k, e in enumerate(engs):                         # further samples on both chains at once, behind the read-out
        _plant(e, x[k, 6:])
    torch.cuda.synchronize()
    assert _same_bits(out.cpu().numpy(), first)
    assert not _same_bits(da.chains_hist_rank(engs, 0, "max"), first) and engs[1].moments_count() == 12


# ---- 8. errors

def _refused(match, engs, reg, stat):
    """raises DangxError naming the cause and leaves the output untouched"""
    out = np.full(NPIX, 7.0)
    with pytest.raises(da.DangxError, match=match):
        da.chains_hist_rank(engs, reg, stat, out=out)
    assert (out == 7.0).all()


def test_errors(eight):
    a, b, c = eight[:3]
    x = _binned_samples(np.random.default_rng(2), 3, 3, 16)
    _begin([a, b, c], 0.0, 16.0, 16, 16)
    for k, e in enumerate((a, b, c)):
        _plant(e, x[k])
    assert np.isfinite(da.chains_hist_rank([a, b, c], 0, "bulk")).any()            # the set is fine as it stands
    _refused("stat of a rank-normalised R-hat must be 0 .bulk., 1 .folded. or 2", [a, b, c], 0, 3)
    _refused("stat of a rank-normalised R-hat", [a, b], 0, -1)
    _refused("nchains must be 2", [a], 0, "bulk")
    _refused("chain 2 is the same context as chain 0", [a, b, a], 0, "bulk")
    _refused("histogram registration out of range .1 registered.", [a, b], 1, "bulk")
    _begin([c], 0.0, 16.0, 8, 16)                                                  # nbins differs in one chain
    _plant(c, x[2])
    _refused("chain 2: histogram registration 0 is not the registration of chain 0 .plane, lo, hi, nbins and bits", [a, b, c], 0, "max")
    _begin([c], 0.0, 16.0, 16, 16)
    _refused("chain 2: no sample accumulated", [a, b, c], 0, "max")
    _begin([a, b], 0.0, 16.0, 16, 16, hist=False)                                  # no histograms registered
    for k, e in enumerate((a, b)):
        _plant(e, x[k])
    _refused("histogram registration out of range .0 registered.", [a, b], 0, "folded")
    with pytest.raises(da.DangxError, match="moments_hist was not called"):
        da.chains_rank_maps([[a], [b]])
    out = torch.full((NPIX,), 7.0, dtype=torch.float64, device="cuda")               # the device form checks the same way
    with pytest.raises(da.DangxError, match="0 registered"):
        da.chains_hist_rank([a, b], 0, "bulk", device=True, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all().item()
