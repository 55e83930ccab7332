#!/usr/bin/env python3
"""What accumulating the posterior moments costs (dangx_moments_accumulate: k_moments_accum over every selected plane) in whole Gibbs
iterations of the C3 model: blocks of iterations without and with accumulation after every iteration, alternating in one process;
then the k_moments kernel time from the profile and its bandwidth in algorithmic bytes (5 x 8 B per selected element) against the
6.29 TB/s measured copy ceiling of the MI355X.
    python3 tools/bench_moments.py [nside=1024] [steps per block=10] [rounds=5]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dang_amd as da  # noqa: E402
from dang_amd import synth  # noqa: E402

COPY_CEILING_TBS = 6.29

nside = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda", 0)
dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=nside, device=dev, as_numpy=False)
eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
it = 1
for _ in range(2):
    da.gibbs_iteration(dpar, ddata, it, want_counts=False)
    it += 1
sel = da.moments_begin(dpar, ddata)
planes = sum(bin(int(s) & 7).count("1") + bin(int(s) >> 3).count("1") for s in sel)
da.moments_accumulate(ddata)   # first accumulation: the segment table's upload


def block(acc):
    global it
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        da.gibbs_iteration(dpar, ddata, it, want_counts=False)
        if acc:
            da.moments_accumulate(ddata)
        it += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


plain, acc = [], []
for _ in range(rounds):
    plain.append(block(False))
    acc.append(block(True))
eng.profile(True)
for _ in range(steps):
    da.moments_accumulate(ddata)
prof = eng.profile_get()["k_moments"]
eng.profile(False)
k_ms = prof["total_ms"] / prof["launches"]
nbytes = 5 * 8 * planes * meta["npix"]
p, a = float(np.median(plain)), float(np.median(acc))
print("C3 at Nside %d: %d selected planes (%d amplitude, %d index) of %d pixels; %d samples accumulated"
      % (nside, planes, sum(bin(int(s) & 7).count("1") for s in sel), sum(bin(int(s) >> 3).count("1") for s in sel), meta["npix"],
         eng.moments_count()))
print("ms per Gibbs iteration, median of %d blocks of %d: without accumulation %.3f (spread %.3f .. %.3f), with accumulation every "
      "iteration %.3f (spread %.3f .. %.3f): +%.3f ms" % (rounds, steps, p, min(plain), max(plain), a, min(acc), max(acc), a - p))
print("k_moments: %.3f ms per launch (%d launches, profiled alone); %.2f GB algorithmic (5 x 8 B x %d planes x %d pixels) -> %.2f TB/s, "
      "%.2f of the %.2f TB/s copy ceiling" % (k_ms, prof["launches"], nbytes * 1e-9, planes, meta["npix"], nbytes / k_ms * 1e-9,
                                              nbytes / k_ms * 1e-9 / COPY_CEILING_TBS, COPY_CEILING_TBS))
print("accumulation overhead beyond the kernel: %.3f ms per iteration" % (a - p - k_ms))
