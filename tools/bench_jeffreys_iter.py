#!/usr/bin/env python3
"""Whole Gibbs iterations of the C3 model with both synchrotron components on the Jeffreys prior (COMP_*_PRIOR = jeffreys; the
polarisation set relabelled 'synch': eval_jeffreys_prior is non-trivial for that label only, src/dang_lnl_mod.f90:289).  Prints ms
per iteration and the launch profile.  usage: tools/bench_jeffreys_iter.py [nside] [steps] [--plain]   (--plain: the gaussian C3
model from the same build, for the gap)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dang_amd as da  # noqa: E402
from dang_amd import synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
plain = "--plain" in sys.argv[1:]
nside = int(args[0]) if len(args) > 0 else 1024
steps = int(args[1]) if len(args) > 1 else 5
dev = torch.device("cuda", 0)
dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=nside, device=dev, as_numpy=False)
if not plain:
    for c in comps:
        if c.label in ("synch", "synch_P"):
            c.label = "synch"
            c.prior_type = ["jeffreys"] * c.nindices
eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
for it in (1, 2):
    da.gibbs_iteration(dpar, ddata, it)
eng.profile(True)
torch.cuda.synchronize()
t0 = time.perf_counter()
for it in range(3, 3 + steps):
    da.gibbs_iteration(dpar, ddata, it)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
print("%s C3, nside %d: %.2f ms per Gibbs iteration (%.2f it/s); chisq %.6f; NUMSAMPLE %d"
      % ("plain" if plain else "jeffreys", nside, 1e3 * dt, 1.0 / dt, ddata.chisq, dpar.nsample))
for k, v in eng.profile_get().items():
    print("  %-14s %4d launches per iteration, %8.3f ms per iteration" % (k, v["launches"] // steps, v["total_ms"] / steps))
