"""The reference-side routines of the per-pixel posterior histograms (fortran/reference_side/dang_gpu_mod.f90: posterior_hist_gpu,
posterior_quantile_to_host_gpu, posterior_hist_n_to_host_gpu) RUN on the GPU through dang_gpu_drive.f90 with DANG_POSTERIOR and
DANG_POSTERIOR_HIST set, against the Python path of the same problem and seeds: the counted samples N exactly, the 0.16 / 0.5 /
0.84 quantiles bit for bit where the two paths leave the same final state, else within test_gpu_moments_hist's tolerance
4 eps max(|lo|, |hi|).  Without the switch the result file keeps its length."""
import os

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _build, fdrive

from util import make_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NITER = 5
QS = (0.16, 0.5, 0.84)


def test_reference_side_histograms_match_the_python_path(built, tmp_path):
    if _build.build_reference_drive() is None:
        pytest.skip("flang not available")
    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    fin, fout, fold = str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "old.bin")
    fdrive.write_problem(fin, dpar, ddata, comps, meta, NITER)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fout, nctx=1, mode="fused", posterior=(1, 1), hist=64)
    got = fdrive.read_result(fout, comps, meta, posterior=True, hist=True)
    post = got["post"]
    assert post["n"] == NITER - 1
    # the existing switch alone: the file read_result(posterior=True) has always read, to the last double
    assert "dang_gpu_drive ok" in fdrive.run(fin, fold, nctx=1, mode="fused", posterior=(1, 1))
    old = fdrive.read_result(fold, comps, meta, posterior=True)
    assert set(old["post"]) == {"n", "mean", "std"}
    nreg = len(post["hist"])
    assert os.path.getsize(fout) - os.path.getsize(fold) == 8 * (1 + nreg * 4 * meta["npix"])

    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    da.moments_begin(dpar, ddata)
    planes = da.moments_hist(dpar, ddata, nbins=64, bits=16)
    assert nreg == len(planes) == 9            # the same default planes in the same order
    for it in range(1, NITER + 1):
        if it == 1:
            da.sample_cg_groups(dpar, ddata, it=1)
        else:
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
    same = all(np.array_equal(got["amp"][l], eng.get_amplitude(l)) and (c.nindices == 0 or np.array_equal(got["ind"][l], eng.get_indices(l)))
               for l, c in enumerate(comps))
    print("the two paths leave the same final state:", same)
    for r, (l, what, k) in enumerate(planes):
        lo, hi = comps[l].uni_prior[what - 1]
        mine_n = eng.moments_hist_stat(r, "n")
        mine_q = eng.moments_hist_stat(r, "quantile", q=QS)
        theirs = post["hist"][r]
        assert np.array_equal(theirs["n"], mine_n), (r, "N")
        assert mine_n.max() == NITER - 1
        assert np.array_equal(np.isnan(theirs["q"]), np.isnan(mine_q)), r
        if same:
            assert np.array_equal(theirs["q"], mine_q, equal_nan=True), (r, "quantiles")
        else:
            ok = ~np.isnan(mine_q)
            assert (np.abs(theirs["q"][ok] - mine_q[ok]) <= 4 * EPS * max(abs(lo), abs(hi))).all(), (r, "quantiles")
