"""The reference-side switch of the fluctuation term (fortran/reference_side/dang_gpu_mod.f90: gpu_fluct_mode, set by
dang_gpu_drive.f90 from DANG_FLUCT) RUN on the GPU: two iterations of C2 with DANG_FLUCT=correct leave the maps of the Python
path with fluct_mode='correct', bit for bit -- and not those of the reference's term."""
import numpy as np
import pytest

import dang_amd as da
from dang_amd import _build, fdrive

from util import make_case

pytestmark = pytest.mark.gpu

NITER = 2


def test_reference_side_correct_mode_matches_the_python_path(built, tmp_path):
    if _build.build_reference_drive() is None:
        pytest.skip("flang not available")
    dpar, ddata, bands, comps, meta = make_case("C2", nside=4)
    fin, fout, fref = (str(tmp_path / n) for n in ("in.bin", "out.bin", "ref.bin"))
    fdrive.write_problem(fin, dpar, ddata, comps, meta, NITER)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fout, nctx=1, mode="fused", fluct_mode="correct")
    assert "dang_gpu_drive ok" in fdrive.run(fin, fref, nctx=1, mode="fused")
    got, ref = fdrive.read_result(fout, comps, meta), fdrive.read_result(fref, comps, meta)

    dpar, ddata, bands, comps, meta = make_case("C2", nside=4)
    dpar.fluct_mode = "correct"
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    da.sample_cg_groups(dpar, ddata, it=1)
    for it in range(2, NITER + 1):
        da.gibbs_iteration(dpar, ddata, it)
    differs = False
    for l, c in enumerate(comps):
        assert np.array_equal(got["amp"][l], eng.get_amplitude(l)), l
        differs = differs or not np.array_equal(got["amp"][l], ref["amp"][l])
        if c.nindices:
            assert np.array_equal(got["ind"][l], eng.get_indices(l)), l
    assert differs      # the switch reached the solves
