"""The reference-side routines of the posterior polarisation angle (fortran/reference_side/dang_gpu_mod.f90: posterior_angle_gpu,
posterior_angle_to_host_gpu) RUN on the GPU through dang_gpu_drive.f90 with DANG_POSTERIOR and DANG_POSTERIOR_ANGLE=1, against
the Python path of the same problem and seeds: the default angles in the same order, their circular mean, circular standard
deviation and mean resultant length maps bit for bit.  Without the switch the result file is what DANG_POSTERIOR alone gives."""
import numpy as np
import pytest

import dang_amd as da
from dang_amd import _build, fdrive

from util import make_case

pytestmark = pytest.mark.gpu

NITER = 5


def test_reference_side_angles_match_the_python_path(built, tmp_path):
    if _build.build_reference_drive() is None:
        pytest.skip("flang not available")
    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    fin, fout, fold = (str(tmp_path / n) for n in ("in.bin", "out.bin", "old.bin"))
    fdrive.write_problem(fin, dpar, ddata, comps, meta, NITER)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fout, nctx=1, mode="fused", posterior=(1, 1), angle=True)
    got = fdrive.read_result(fout, comps, meta, posterior=True, angle=True)
    post = got["post"]
    assert post["n"] == NITER - 1
    # without the switch: the file read_result(posterior=True) has always read; the new one is that file plus the angles (the
    # timing, one double, differs from run to run and is blanked)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fold, nctx=1, mode="fused", posterior=(1, 1))
    assert set(fdrive.read_result(fold, comps, meta, posterior=True)["post"]) == {"n", "mean", "std"}
    a, c = (np.fromfile(f, dtype=np.float64) for f in (fold, fout))
    a[2] = c[2] = 0.0
    nang = len(post["angle"])
    assert c.size - a.size == 1 + nang * (2 + 3 * meta["npix"]) and c[:a.size].tobytes() == a.tobytes()

    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    da.moments_begin(dpar, ddata)
    specs = da.moments_angles(dpar, ddata)
    assert [s["spec"] for s in post["angle"]] == specs and nang == 2       # the same default angles in the same order
    for it in range(1, NITER + 1):
        if it == 1:
            da.sample_cg_groups(dpar, ddata, it=1)
        else:
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
    spread = False
    for s, spec in enumerate(specs):
        theirs = post["angle"][s]
        for st in ("psi", "psi_std", "R"):
            mine = eng.moments_get_angle(s, st)
            assert np.array_equal(theirs[st], mine, equal_nan=True), (spec, st)
        std = eng.moments_get_angle(s, "psi_std")
        spread = spread or (std[np.isfinite(std)] > 0).any()
    assert spread
