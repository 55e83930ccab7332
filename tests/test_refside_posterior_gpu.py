"""The reference-side posterior routines (fortran/reference_side/dang_gpu_mod.f90: posterior_begin_gpu, posterior_accumulate_gpu,
posterior_to_host_gpu) RUN on the GPU through dang_gpu_drive.f90 with DANG_POSTERIOR set: the loop of program dang with burn-in 1
and thinning 1, and the arrays write_maps(dpar, 'mean' / 'std') would write against the Python path's moments of the same
problem and seeds."""
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


def test_reference_side_posterior_matches_the_python_path(built, tmp_path):
    if _build.build_reference_drive() is None:
        pytest.skip("flang not available")
    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    fdrive.write_problem(fin, dpar, ddata, comps, meta, NITER)
    out = fdrive.run(fin, fout, nctx=1, mode="fused", posterior=(1, 1))
    assert "dang_gpu_drive ok" in out
    got = fdrive.read_result(fout, comps, meta, posterior=True)
    post = got["post"]
    assert post["n"] == NITER - 1

    # the Python path: the same loop (iteration 1 the amplitude phase only, as the drive runs it), accumulating after iteration 1
    dpar, ddata, bands, comps, meta = make_case("C2", nside=8)
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
    sel = da.moments_begin(dpar, ddata)
    samples = []
    for it in range(1, NITER + 1):
        if it == 1:
            da.sample_cg_groups(dpar, ddata, it=1)
        else:
            da.gibbs_iteration(dpar, ddata, it)
        if it > 1:
            da.moments_accumulate(ddata)
            samples.append({l: (eng.get_amplitude(l), eng.get_indices(l) if c.nindices else None) for l, c in enumerate(comps)})
    assert eng.moments_count() == post["n"]
    # first the chains: where the two paths leave the same final state bit for bit, the moments must be bit for bit too
    same = all(np.array_equal(got["amp"][l], samples[-1][l][0]) and (c.nindices == 0 or np.array_equal(got["ind"][l], samples[-1][l][1]))
               for l, c in enumerate(comps))
    n = post["n"]
    checked = 0
    for l, c in enumerate(comps):
        for what in range(1 + c.nindices):
            ks = _planes(sel[l], what)
            if not ks:
                continue
            xs = np.stack([s[l][0] if what == 0 else s[l][1][what - 1] for s in samples])
            big = np.abs(xs).max(axis=0)
            for stat in ("mean", "std"):
                mine = eng.moments_get(l, what, stat)
                theirs = post[stat]["amp"][l] if what == 0 else post[stat]["ind"][l][what - 1]
                for k in ks:
                    if same:
                        assert np.array_equal(theirs[k], mine[k]), (c.label, what, stat, k)
                    else:   # test_gpu_moments' tolerances
                        tol = 8 * n * EPS * big[k] if stat == "mean" else 16 * n * EPS * (np.abs(mine[k]) + big[k])
                        assert (np.abs(theirs[k] - mine[k]) <= tol + 1e-300).all(), (c.label, what, stat, k)
                    checked += 1
    assert checked == 2 * sum(bin(int(s)).count("1") for s in sel)
