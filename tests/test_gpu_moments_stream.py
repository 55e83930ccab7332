"""The one loop by which the posterior-statistics kernels visit a plane (csrc/dx_stream.h: odd first element, 16-byte pairs, odd
last element, or element by element where the pointers share no 16-byte phase), at the smallest sizes where its branches differ.

Shards of 1, 2 and 3 pixels of the 12-pixel sky (C2, IQU, Nside 1; bounds 0, 1, 3, 6, 12) give head in {0, 1} x pairs in {0, 1} x
"tail present / absent": with an odd pixel count consecutive planes of a buffer lie at different 16-byte phases.  Every context runs
once with its state where the library allocates it, and once with every component's buffers moved, after two of the four samples,
to caller memory one double off the 16-byte grid: the chain's planes then share no phase with their accumulators.

Four planted states per chain go in through put_amplitude / put_indices.  Every read-out of a shard must equal, bit for bit, the
matching slice of the whole 12-pixel context fed the same states -- which the other suites hold to the host references -- and the
device form of every getter must equal its host form bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import dang_amd as da

from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

BOUNDS = [0, 1, 3, 6, 12]
NSAMP = 4
NBINS, BITS = 8, 16
QUANTILE = [0.5]


def _states(comps, seed):
    """NSAMP planted states [{l: (amplitude [nmaps][12], indices [nind][nmaps][12] or None)}]; an index is drawn from its prior
    range widened by a tenth on either side, so that a histogram over the prior range leaves some samples uncounted"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(NSAMP):
        st = {}
        for l, c in enumerate(comps):
            amp = 10.0 * rng.standard_normal(c.amplitude.shape) + 3.0 * l
            idx = None
            if c.nindices:
                idx = np.empty(c.indices.shape)
                for j in range(c.nindices):
                    lo, hi = c.uni_prior[j]
                    idx[j] = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), idx[j].shape)
            st[l] = (amp, idx)
        out.append(st)
    return out


def _registrations(comps):
    """one pair per component that has an index, alternately within one plane number and across two (with an odd pixel count: the
    same and different 16-byte phases), and one histogram on the first index plane there is"""
    with_idx = [l for l, c in enumerate(comps) if c.nindices]
    pairs = [((l, 0, j % 3), (l, 1, (j + j % 2) % 3)) for j, l in enumerate(with_idx)]
    return pairs, [(with_idx[0], 1, 0)]


def _move_off_the_grid(e):
    """every component's maps into caller buffers that start one double past a 16-byte boundary"""
    dev = torch.device("cuda", 0)
    for l, c in enumerate(e.component_list):
        amp = torch.empty(e.nmaps * e.npix + 1, dtype=torch.float64, device=dev)[1:].view(e.nmaps, e.npix)
        amp.copy_(torch.from_numpy(e.get_amplitude(l)))
        idx = None
        if c.nindices:
            idx = torch.empty(c.nindices * e.nmaps * e.npix + 1, dtype=torch.float64, device=dev)[1:].view(c.nindices, e.nmaps, e.npix)
            idx.copy_(torch.from_numpy(e.get_indices(l)))
        assert amp.data_ptr() % 16 == 8 and (idx is None or idx.data_ptr() % 16 == 8)
        torch.cuda.synchronize()
        e._chk(e.lib.dangx_adopt_device_state(e.h, l, ctypes.c_void_p(amp.data_ptr()),
                                              ctypes.c_void_p(idx.data_ptr()) if idx is not None else None))
        e._adopted[l] = (amp, idx)   # keeps the buffers alive


def _run_chain(case, seed, nshards, move):
    """the engines of one chain (shard order), registered and fed the NSAMP planted states of `seed`"""
    comps = case[3]
    engs = shard_engines(case, nshards, bounds=BOUNDS if nshards > 1 else None)
    pairs, hplanes = _registrations(comps)
    for e in engs:
        e.moments_begin(None)
        e.moments_pairs(pairs, lag1=True)
        e.moments_hist(hplanes, nbins=NBINS, bits=BITS)
    for t, st in enumerate(_states(comps, seed)):
        for e in engs:
            if move and t == NSAMP // 2:
                _move_off_the_grid(e)
            sl = slice(e.pix0, e.pix0 + e.npix)
            for l, (amp, idx) in st.items():
                e.put_amplitude(l, amp[:, sl])
                if idx is not None:
                    e.put_indices(l, idx[:, :, sl])
            e.moments_accumulate()
    return engs


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _readouts(chains):
    """{key: array with the pixel as its last axis} of every read-out of one shard: chains = that shard's engine of each chain.
    Each is taken in its host and in its device form, which must agree bit for bit."""
    out = {}

    def take(key, host, device, sync):
        h = host()
        d = device()
        sync.synchronize()
        d = d.cpu().numpy()
        if d.dtype != h.dtype:                     # the raw counters come back as signed integers of the same width
            d = d.view(h.dtype)
        assert _same_bits(h, d), ("device form differs from host form", key)
        out[key] = h

    comps = chains[0].component_list
    pairs, hplanes = _registrations(comps)
    for c, e in enumerate(chains):
        assert e.moments_count() == NSAMP
        for l, comp in enumerate(comps):
            for what in range(1 + comp.nindices):
                for stat, ddof in (("mean", 0), ("std", 1), ("rho1", 0), ("ess", 0)):
                    take((c, l, what, stat), lambda: e.moments_get(l, what, stat, ddof), lambda: e.moments_get(l, what, stat, ddof, device=True), e)
        for p in range(len(pairs)):
            for stat, ddof in (("cov", 1), ("corr", 0)):
                take((c, "pair", p, stat), lambda: e.moments_get_pair(p, stat, ddof), lambda: e.moments_get_pair(p, stat, ddof, device=True), e)
        take((c, "hist", "counts"), lambda: e.moments_hist_get(0).T, lambda: e.moments_hist_get(0, device=True).T, e)
        take((c, "hist", "quantile"), lambda: e.moments_hist_stat(0, "quantile", QUANTILE),
             lambda: e.moments_hist_stat(0, "quantile", QUANTILE, device=True), e)
    for l, comp in enumerate(comps):
        for what in range(1 + comp.nindices):
            for stat in ("rhat", "ess"):
                take(("chains", l, what, stat), lambda: da.chains_get(chains, l, what, stat), lambda: da.chains_get(chains, l, what, stat, device=True),
                     chains[0])
    for p in range(len(pairs)):
        take(("chains", "pair", p), lambda: da.chains_get_pair(chains, p, "corr"), lambda: da.chains_get_pair(chains, p, "corr", device=True), chains[0])
    return out


@pytest.fixture(scope="module")
def case(built):
    return make_case("C2", nside=1)


@pytest.fixture(scope="module")
def whole(case):
    """the read-outs of the 12-pixel context over two chains: the reference, computed once and left as it is"""
    chains = [_run_chain(case, seed, 1, False)[0] for seed in (11, 12)]
    ref = _readouts(chains)
    counts = ref[(0, "hist", "counts")]
    assert 0 < counts.sum() < counts.shape[-1] * NSAMP          # some samples counted, some outside the range
    assert all(np.isfinite(ref[("chains", l, 0, "rhat")]).all() for l in range(len(case[3])))
    for v in ref.values():
        v.setflags(write=False)
    return ref


@pytest.fixture(scope="module", params=["library", "off_grid"])
def sharded(case, request):
    """per shard, that shard's engine of each of the two chains"""
    a, b = (_run_chain(case, seed, len(BOUNDS) - 1, request.param == "off_grid") for seed in (11, 12))
    return list(zip(a, b))


@pytest.mark.parametrize("shard", [0, 1, 2])
def test_shard_equals_whole(whole, sharded, shard):
    chains = list(sharded[shard])
    p0, p1 = BOUNDS[shard], BOUNDS[shard + 1]
    assert chains[0].npix == p1 - p0 == shard + 1 and chains[0].pix0 == p0
    got = _readouts(chains)
    assert got.keys() == whole.keys() and len(got) > 60
    for key, ref in whole.items():
        assert _same_bits(got[key], np.ascontiguousarray(ref[..., p0:p1])), key
