#!/usr/bin/env python3
"""Whole Gibbs iterations of the C3 model with every sampled index drawn per pixel at a COARSER Nside (sample_nside < nside, SURVEY
8f rank 4): stage the cleaned data, degrade data / rms / mask, one chain per coarse pixel, write the coarse index map back.

usage: tools/bench_coarse_iter.py [nside] [sample_nside] [steps] [--coarse-model {reference,degraded}]
--coarse-model degraded: the chains read the degraded amplitude / index maps (DANGX_COARSE_DEGRADED); default reference."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dang_amd as da  # noqa: E402
from dang_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("nside", nargs="?", type=int, default=1024)
ap.add_argument("sample_nside", nargs="?", type=int, default=128)
ap.add_argument("steps", nargs="?", type=int, default=3)
ap.add_argument("--coarse-model", choices=("reference", "degraded"), default="reference")
args = ap.parse_args()
nside, coarse, steps = args.nside, args.sample_nside, args.steps
dev = torch.device("cuda", 0)
dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=nside, device=dev, as_numpy=False)
for c in comps:
    c.sample_nside = [coarse] * c.nindices
    c.coarse_model = [args.coarse_model] * c.nindices
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
model = "" if args.coarse_model == "reference" else " (coarse model %s)" % args.coarse_model
print("index sampling at Nside %d of %d%s: %.2f ms per Gibbs iteration (%.2f it/s); chisq %.6f" % (coarse, nside, model, 1e3 * dt, 1.0 / dt,
                                                                                                  ddata.chisq))
for k, v in eng.profile_get().items():
    print("  %-14s %4d launches per iteration, %8.3f ms per iteration" % (k, v["launches"] // steps, v["total_ms"] / steps))
