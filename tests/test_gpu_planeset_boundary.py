"""The plane-set launches (dang_amd/csrc/dx_kern_planeset.h: k_plane_set) against maps recorded from the commit before the
chain-boundary evaluations were shared (the dust pair's Planck factors and SED column kept from the solve, one evaluation at
the beta -> T hand-over): amplitude maps, index maps, both chi^2 sums and the accepted
counts after three iterations must be the recorded BITS (tests/golden/planeset_parent_bits.npz, written by record() below on
the same device family).  The cases cover every form the boundary code takes: a partial block and several blocks, skies whose
proposals go through the exact branch after cheap accepts (noise / 1e4), chains without the certificate (bounds outside the fp32
exponent range, ml_mode optimize, the Jeffreys prior), band calibration on T, the sweeps-only launch, a shape specialised at run
time, and the 20-band lane-pair model with a log-normal item, which must not change at all."""
import os

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L

from util import make_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planeset_parent_bits.npz")
ITERATIONS = 3


def _sharpen(scale):
    def tweak(dpar, ddata, bands, comps):
        ddata.rms_map = np.ascontiguousarray(ddata.rms_map * scale)
    return tweak


def _wide_bounds(dpar, ddata, bands, comps):
    for c in comps:
        if c.type == "power-law":
            c.uni_prior = [[-60.0, 40.0]]          # |beta ln(nu/nu_ref)| log2e > 125 at 857 GHz: the exact form throughout


def _jeffreys(dpar, ddata, bands, comps):
    for c in comps:
        if c.label in ("synch", "synch_P"):
            c.label = "synch"
            c.prior_type = ["jeffreys"] * c.nindices


def _calibration(nbands):   # bench.py --calibrated's values
    return dict(gain=[1.0 + 0.01 * ((j % 3) - 1) for j in range(nbands)], offset=[0.5 * ((j % 4) - 1.5) for j in range(nbands)])


# name -> (make_case arguments, ml_mode, sweeps-only form)
CASES = {
    "n4": (dict(config="C3", nside=4, start="truth"), "sample", False),
    "n8": (dict(config="C3", nside=8, start="truth"), "sample", False),
    "sharp": (dict(config="C3", nside=8, start="truth", tweak=_sharpen(1e-4)), "sample", False),
    "wide": (dict(config="C3", nside=8, start="truth", tweak=_wide_bounds), "sample", False),
    "optimize": (dict(config="C3", nside=8, start="truth"), "optimize", False),
    "calibrated": (dict(config="C3", nside=8, start="truth", **_calibration(10)), "sample", False),
    "sweeps_only": (dict(config="C3", nside=8, start="truth"), "sample", True),
    "jeffreys": (dict(config="C3", nside=8, start="truth", tweak=_jeffreys), "sample", False),
    "rtc7": (dict(config="C3", nside=8, nbands=7, start="truth"), "sample", False),
    "c5": (dict(config="C5", nside=4, start="truth"), "sample", False),
}


def _planes(flag):
    return {L.FLAG_T: (1, 1), L.FLAG_Q: (2, 2), L.FLAG_U: (3, 3), L.FLAG_QU: (2, 3)}[flag]


def run_case(name):
    """{array name: array} of the state after ITERATIONS iterations of the case's plane-set launches"""
    kw, ml_mode, sweeps_only = CASES[name]
    dpar, ddata, bands, comps, meta = make_case(**kw)
    eng = da.Engine(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    accepted, chi = [], []
    for it in range(1, ITERATIONS + 1):
        for g in dpar.cg_groups:
            f = g.pol_flag[0]
            sw = [(l, j, da.stream_id(it, 1, l, j, f)) for l, c in enumerate(comps) for j in range(c.nindices)
                  if c.cg_group == g.cg_group and c.sample_index[j] and f in c.pol_flag[j]]
            sa = da.stream_id(it, 0, g.cg_group, 0, f)
            if sweeps_only:
                _, bad = eng.amp_sample(g.cg_group, f, ml_mode, dpar.seed, sa)
                accs = eng.plane_sweeps_sample(f, sw, dpar.nsample, ml_mode, dpar.seed)
            else:
                bad, accs = eng.plane_set_sample(g.cg_group, f, ml_mode, dpar.seed, sa, sw, dpar.nsample, dpar.seed)
            assert bad == 0
            accepted += list(accs)
            for which in (0, 1):
                v = eng.chisq_cached(which, *_planes(f))
                chi.append(np.nan if v is None else v)
    out = {"accepted": np.asarray(accepted, dtype=np.int64), "chisq": np.asarray(chi, dtype=np.float64)}
    for l, c in enumerate(comps):
        out["amp%d" % l] = np.ascontiguousarray(eng.get_amplitude(l), dtype=np.float64)
        if c.nindices:
            out["idx%d" % l] = np.ascontiguousarray(eng.get_indices(l), dtype=np.float64)
    return out, eng


def record(path):
    """writes the fixture from the build that is loaded (run once, on the parent commit)"""
    arrays = {}
    for name in CASES:
        out, _ = run_case(name)
        for k, v in out.items():
            arrays[name + "/" + k] = v
    np.savez_compressed(path, **arrays)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(CASES))
def test_plane_set_bits_are_the_parents(built, golden, name):
    out, eng = run_case(name)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(name + "/"))
    assert keys == sorted(out), (keys, sorted(out))
    for k in keys:
        want, got = golden[name + "/" + k], out[k]
        assert want.shape == got.shape and want.dtype == got.dtype, (name, k)
        ne = int(np.count_nonzero(want.view(np.int64) != got.view(np.int64)))
        print("%s/%s: %d of %d values differ in their bits" % (name, k, ne, want.size))
        assert ne == 0, (name, k, ne)
    if name == "rtc7":
        assert any(n.startswith("dxk::k_plane_set<") for n in eng.rtc_kernels()), eng.rtc_kernels()
