"""The reference-side routines of the component-signal moments (fortran/reference_side/dang_gpu_mod.f90: posterior_signal_gpu,
posterior_signal_to_host_gpu) RUN on the GPU through dang_gpu_drive.f90 with DANG_POSTERIOR and DANG_POSTERIOR_SIGNAL=1, against
the Python path of the same problem and seeds: the default signals in the same order, their mean and std maps bit for bit.
Without the switch the result file is byte for byte what DANG_POSTERIOR alone gives."""
import os

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _build, fdrive

from util import make_case

pytestmark = pytest.mark.gpu

NITER = 5


def test_reference_side_signals_match_the_python_path(built, tmp_path):
    if _build.build_reference_drive() is None:
        pytest.skip("flang not available")
    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    fin, fout, fold, fold2 = (str(tmp_path / n) for n in ("in.bin", "out.bin", "old.bin", "old2.bin"))
    fdrive.write_problem(fin, dpar, ddata, comps, meta, NITER)
    assert "dang_gpu_drive ok" in fdrive.run(fin, fout, nctx=1, mode="fused", posterior=(1, 1), signal=True)
    got = fdrive.read_result(fout, comps, meta, posterior=True, signal=True)
    post = got["post"]
    assert post["n"] == NITER - 1
    # without the switch: the file read_result(posterior=True) has always read; the new one is that file plus the signals.
    # The timing (one double, `secs`) differs from run to run: two runs without the switch are compared with it blanked
    assert "dang_gpu_drive ok" in fdrive.run(fin, fold, nctx=1, mode="fused", posterior=(1, 1))
    assert "dang_gpu_drive ok" in fdrive.run(fin, fold2, nctx=1, mode="fused", posterior=(1, 1))
    old = fdrive.read_result(fold, comps, meta, posterior=True)
    assert set(old["post"]) == {"n", "mean", "std"}
    a, b, c = (np.fromfile(f, dtype=np.float64) for f in (fold, fold2, fout))
    a[2] = b[2] = c[2] = 0.0
    assert a.tobytes() == b.tobytes()
    nsig = len(post["signal"])
    assert c.size - a.size == 1 + nsig * (3 + 2 * meta["npix"]) and c[:a.size].tobytes() == a.tobytes()

    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    da.moments_begin(dpar, ddata)
    specs = da.moments_signals(dpar, ddata)
    assert [s["spec"] for s in post["signal"]] == specs and nsig == 8       # the same default signals in the same order
    for it in range(1, NITER + 1):
        if it == 1:
            da.sample_cg_groups(dpar, ddata, it=1)
        else:
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
    same = all(np.array_equal(got["amp"][l], eng.get_amplitude(l)) and (c.nindices == 0 or np.array_equal(got["ind"][l], eng.get_indices(l)))
               for l, c in enumerate(comps))
    print("the two paths leave the same final state:", same)
    moved = False
    for s, spec in enumerate(specs):
        mine_m, mine_s = eng.moments_get_signal(s, "mean"), eng.moments_get_signal(s, "std")
        theirs = post["signal"][s]
        assert np.array_equal(theirs["mean"], mine_m, equal_nan=True), (spec, "mean")
        assert np.array_equal(theirs["std"], mine_s, equal_nan=True), (spec, "std")
        moved = moved or (mine_s[np.isfinite(mine_s)] > 0).any()
    assert moved
