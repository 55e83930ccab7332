"""The textbook fluctuation term (DANGX_FLUCT_CORRECT) in the oracle alone: a CORRECT sample on the data d is the OPTIMIZE solve
on d + sigma * eta, eta the per-band normals of draw slot k + 4 * (band + 1) (fluct_helpers.py).  Pins the definition that the
GPU tests of the plane-set kernel's textbook term rely on (test_gpu_fluct_fast.py)."""
import copy

import numpy as np
import pytest

import oracle_ffi as O
from fluct_helpers import perturbed_data, unmasked
from util import TOL_AMP, make_case

SEED = 5


@pytest.mark.parametrize("config,nside", [("C3", 4), ("C5", 2)])
def test_correct_sample_is_the_optimize_solve_on_perturbed_data(config, nside):
    dpar, ddata, bands, comps, meta = make_case(config, nside=nside, start="truth")
    solves = [(g.pol_flag[0], 21 + g.pol_flag[0]) for g in dpar.cg_groups]
    a = O.Oracle(bands, copy.deepcopy(comps), ddata)
    b = O.Oracle(bands, copy.deepcopy(comps), perturbed_data(ddata, solves, SEED))
    for g, (f, s) in zip(dpar.cg_groups, solves):
        assert a.amp_sample_direct(g.cg_group, f, "sample", SEED, s, "correct") == 0
        assert b.amp_sample_direct(g.cg_group, f, "optimize", SEED, s, "correct") == 0
    worst = 0.0
    for l, c in enumerate(comps):
        live = unmasked(ddata, dpar.cg_groups[c.cg_group - 1].pol_flag[0])
        x, y = a.amplitude(l)[:, live], b.amplitude(l)[:, live]
        assert np.abs(x - np.asarray(comps[l].amplitude)[:, live]).max() > 0.0      # the solve has moved them
        worst = max(worst, np.abs(x - y).max() / np.abs(y).max())
    print("%s: largest relative difference %.2e" % (config, worst))
    assert worst <= TOL_AMP
