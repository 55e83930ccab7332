#!/usr/bin/env python3
"""What the host-staged rehearsal path of dist_chains costs: chains_rank_maps over two gloo ranks on ONE device (each rank runs one
C2 chain with the default histograms, 64 bins x 16 bit), beside the same call in one process on the same two chains.  The gloo path
stages every section through the host (device -> host -> socket -> host -> device); it states a price, not a target -- the nccl
path moves device tensors and needs a node with several GPUs.
    python3 tools/bench_dist_chains.py [nside=256] [samples=3] [repeats=3]"""
import datetime
import os
import socket
import sys
import time

import torch.distributed as td
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chain(nside, seed, nsamples):
    import torch
    import dang_amd as da
    from dang_amd import synth
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=nside, device=torch.device("cuda", 0), as_numpy=False)
    dpar.seed = seed
    da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    da.moments_begin(dpar, ddata)
    planes = da.moments_hist(dpar, ddata, nbins=64, bits=16)
    for it in range(1, nsamples + 1):
        da.gibbs_iteration(dpar, ddata, it, want_counts=False)
        da.moments_accumulate(ddata)
    ddata.engine.synchronize()
    return ddata, len(planes), meta["npix"]


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def worker(rank, world, port, nside, nsamples, repeats):
    sys.path.insert(0, ROOT)
    import dang_amd as da
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    ddata, nreg, npix = chain(nside, 1234 + rank, nsamples)      # before the process group: every rank holds the whole sky
    td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    dc = da.dist_chains([ddata], dst=0)
    ts = timed(lambda: da.chains_rank_maps(dc), repeats)
    if rank == 0:
        print("two gloo ranks, Nside %d (%d pixels), %d histogram registrations of %.3f GB each: chains_rank_maps %s s; peak held %.3f GB"
              % (nside, npix, nreg, npix * 128e-9, " ".join("%.3f" % t for t in ts), dc.peak_held * 1e-9), flush=True)
    td.barrier()
    td.destroy_process_group()


if __name__ == "__main__":
    nside = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    nsamples = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(worker, args=(2, port, nside, nsamples, repeats), nprocs=2, join=True)
    import dang_amd as da
    chains = [chain(nside, 1234 + k, nsamples)[0] for k in range(2)]
    ts = timed(lambda: da.chains_rank_maps(chains), repeats)
    print("one process, the same two chains: chains_rank_maps %s s" % " ".join("%.3f" % t for t in ts))
