"""The reference-side routines of the goodness-of-fit moments (fortran/reference_side/dang_gpu_mod.f90: posterior_fit_gpu,
posterior_fit_to_host_gpu) RUN on the GPU through dang_gpu_drive.f90 with DANG_POSTERIOR and DANG_POSTERIOR_FIT=1, against the
Python path of the same problem and seeds: the default items in the same order, their mean and std maps bit for bit.  Without
the switch the result file is byte for byte what DANG_POSTERIOR alone gives."""
import numpy as np
import pytest

import dang_amd as da
from dang_amd import _build, fdrive

from util import make_case

pytestmark = pytest.mark.gpu

NITER = 5


def test_reference_side_fit_items_match_the_python_path(built, tmp_path):
    if _build.build_reference_drive() is None:
        pytest.skip("flang not available")
    dpar, ddata, bands, comps, meta = make_case("C2", nside=4)
    fin, fout, fold = (str(tmp_path / n) for n in ("in.bin", "out.bin", "old.bin"))
    fdrive.write_problem(fin, dpar, ddata, comps, meta, NITER)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fout, nctx=1, mode="fused", posterior=(1, 1), fit=True)
    got = fdrive.read_result(fout, comps, meta, posterior=True, fit=True)
    post = got["post"]
    assert post["n"] == NITER - 1
    # without the switch: the file read_result(posterior=True) has always read; the new one is that file plus the fit items (the
    # timing, one double, differs from run to run and is blanked)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fold, nctx=1, mode="fused", posterior=(1, 1))
    old = fdrive.read_result(fold, comps, meta, posterior=True)
    assert set(old["post"]) == {"n", "mean", "std"}
    a, c = (np.fromfile(f, dtype=np.float64) for f in (fold, fout))
    a[2] = c[2] = 0.0
    nfit = len(post["fit"])
    assert c.size - a.size == 1 + nfit * (3 + 2 * meta["npix"]) and c[:a.size].tobytes() == a.tobytes()

    dpar, ddata, bands, comps, meta = make_case("C2", nside=4)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    da.moments_begin(dpar, ddata)
    specs = da.moments_fit(dpar, ddata)
    assert [s["spec"] for s in post["fit"]] == specs and nfit == 3 * (1 + meta["nbands"]) == 18   # the same default items in the same order
    for it in range(1, NITER + 1):
        if it == 1:
            da.sample_cg_groups(dpar, ddata, it=1)
        else:
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
    moved = False
    for i, spec in enumerate(specs):
        mine_m, mine_s = eng.moments_get_fit(i, "mean"), eng.moments_get_fit(i, "std")
        theirs = post["fit"][i]
        assert np.array_equal(theirs["mean"], mine_m, equal_nan=True), (spec, "mean")
        assert np.array_equal(theirs["std"], mine_s, equal_nan=True), (spec, "std")
        moved = moved or (mine_s[np.isfinite(mine_s)] > 0).any()
    assert moved
