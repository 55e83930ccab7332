"""The reference-side routines of the second-order posterior summaries (fortran/reference_side/dang_gpu_mod.f90:
posterior_pairs_gpu, posterior_to_host_gpu with stat 2 / 3, posterior_pair_to_host_gpu) RUN on the GPU through dang_gpu_drive.f90
with DANG_POSTERIOR and DANG_POSTERIOR_PAIRS set, against the Python path of the same problem and seeds: bit for bit where the two
paths leave the same final state, else within test_gpu_moments_pairs' tolerances (rho1: 16 n eps (1 + big/s), ESS: 2 n times
that, correlation: 16 n eps (1 + big_a/s_a + big_b/s_b)).  With DANG_POSTERIOR alone the result file keeps its length."""
import os

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _build, fdrive

from util import make_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NITER = 5


def _planes(word, what):
    bits = (int(word) >> (0 if what == 0 else 3 + 3 * (what - 1))) & 7
    return [k for k in range(3) if (bits >> k) & 1]


def _close(theirs, mine, tol, same, what):
    assert np.array_equal(np.isnan(theirs), np.isnan(mine)), what
    if same:
        assert np.array_equal(theirs, mine, equal_nan=True), what
    else:
        ok = ~np.isnan(mine)
        assert (np.abs(theirs[ok] - mine[ok]) <= tol[ok]).all(), what


def test_reference_side_pairs_match_the_python_path(built, tmp_path):
    if _build.build_reference_drive() is None:
        pytest.skip("flang not available")
    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    fin, fout, fold = str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "old.bin")
    fdrive.write_problem(fin, dpar, ddata, comps, meta, NITER)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fout, nctx=1, mode="fused", posterior=(1, 1), pairs=True)
    got = fdrive.read_result(fout, comps, meta, posterior=True, pairs=True)
    post = got["post"]
    n = post["n"]
    assert n == NITER - 1
    # the existing switch alone: the file read_result(posterior=True) has always read, to the last double
    assert "dang_gpu_drive ok" in fdrive.run(fin, fold, nctx=1, mode="fused", posterior=(1, 1))
    old = fdrive.read_result(fold, comps, meta, posterior=True)
    assert set(old["post"]) == {"n", "mean", "std"}
    extra = 2 * sum(3 * meta["npix"] * (1 + c.nindices) for c in comps) + 1 + post["corr"].size
    assert os.path.getsize(fout) - os.path.getsize(fold) == 8 * extra

    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    sel = da.moments_begin(dpar, ddata)
    pairs = da.moments_pairs(dpar, ddata)
    assert post["corr"].shape == (len(pairs), meta["npix"])
    samples = []
    for it in range(1, NITER + 1):
        if it == 1:
            da.sample_cg_groups(dpar, ddata, it=1)
        else:
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
            samples.append({l: (eng.get_amplitude(l), eng.get_indices(l) if c.nindices else None) for l, c in enumerate(comps)})
    same = all(np.array_equal(got["amp"][l], samples[-1][l][0]) and (c.nindices == 0 or np.array_equal(got["ind"][l], samples[-1][l][1]))
               for l, c in enumerate(comps))

    def series(l, what, k):
        return np.stack([s[l][0][k] if what == 0 else s[l][1][what - 1][k] for s in samples])

    def spread(xs):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.abs(xs).max(axis=0) / xs.std(axis=0)

    checked = 0
    for l, c in enumerate(comps):
        for what in range(1 + c.nindices):
            for k in _planes(sel[l], what):
                tol = 16 * n * EPS * (1 + spread(series(l, what, k)))
                for stat, f in (("rho1", 1), ("ess", 2 * n)):
                    mine = eng.moments_get(l, what, stat)[k]
                    theirs = (post[stat]["amp"][l] if what == 0 else post[stat]["ind"][l][what - 1])[k]
                    _close(theirs, mine, f * tol, same, (c.label, what, stat, k))
                    checked += 1
    assert checked == 2 * sum(bin(int(s)).count("1") for s in sel)
    for p, (a, b) in enumerate(pairs):
        tol = 16 * n * EPS * (1 + spread(series(*a)) + spread(series(*b)))
        _close(post["corr"][p], eng.moments_get_pair(p, "corr"), tol, same, ("corr", p))
