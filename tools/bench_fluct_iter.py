#!/usr/bin/env python3
"""Whole Gibbs iterations (da.gibbs_iteration) of the C3 model with the amplitude solves on either fluctuation term: 'correct'
(the textbook term, one normal per band: the mode whose samples are posterior draws; k_plane_set<.., SOLVE = 2, ..>) or
'reference' (compute_sample_vector's).  Prints ms per iteration and the launch profile by kernel family.
usage: tools/bench_fluct_iter.py [nside] [steps] [correct|reference] [--template] [--blocks N]
  --template   the model of tools/bench_template_iter.py: a Q/U template fitted at the last three bands in the Q+U group (the Schur
               passes; with 'correct' the run-time-typed ones)
  --blocks N   N timed blocks of `steps` iterations each (the block-to-block spread)
DANGX_PLANESET=0 in the environment takes the separate launches (k_amp_direct, the stand-alone sweeps, the chi^2 pass): what a
'correct' iteration ran before the plane-set kernel carried the term."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dang_amd as da  # noqa: E402
from dang_amd import synth  # noqa: E402

argv = sys.argv[1:]
blocks = int(argv[argv.index("--blocks") + 1]) if "--blocks" in argv else 1
if "--blocks" in argv:
    del argv[argv.index("--blocks"):argv.index("--blocks") + 2]
args = [a for a in argv if not a.startswith("--")]
template = "--template" in argv
nside = int(args[0]) if len(args) > 0 else 1024
steps = int(args[1]) if len(args) > 1 else 5
mode = args[2] if len(args) > 2 else "correct"
assert mode in ("correct", "reference"), mode
dev = torch.device("cuda", 0)
dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=nside, device=dev, as_numpy=False, start="truth" if template else "prior",
                                                 fluct_mode=mode)
if template:
    nb = meta["nbands"]
    synth.add_qu_template(ddata, comps, meta, fit_bands=tuple(range(nb - 3, nb)), amplitudes=(2.0, -1.5, 0.7))
eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
for it in (1, 2):
    da.gibbs_iteration(dpar, ddata, it, want_counts=False)
it = 3
for b in range(blocks):
    eng.profile(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        da.gibbs_iteration(dpar, ddata, it, want_counts=False)
        it += 1
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    prof = eng.profile_get()
    eng.profile(False)
    print("%s%s C3, nside %d, block %d: %.3f ms per Gibbs iteration (%.2f it/s); chisq %.6f; NUMSAMPLE %d"
          % (mode, " + template" if template else "", nside, b, 1e3 * dt, 1.0 / dt, ddata.chisq, dpar.nsample))
for k, v in prof.items():
    print("  %-14s %4d launches per iteration, %8.3f ms per iteration" % (k, v["launches"] // steps, v["total_ms"] / steps))
