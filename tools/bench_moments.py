#!/usr/bin/env python3
"""What accumulating the posterior moments costs (dangx_moments_accumulate: k_moments_accum over every selected plane) in whole Gibbs
iterations of the C3 model: blocks of iterations without and with accumulation after every iteration, alternating in one process;
then the k_moments kernel time from the profile and its bandwidth in algorithmic bytes (5 x 8 B per selected element) against the
6.29 TB/s measured copy ceiling of the MI355X.
    python3 tools/bench_moments.py [nside=1024] [steps per block=10] [rounds=5] [--lag1] [--pairs default] [--hist [nbins=64] [--range-maps | --signals]] [--signals [--bandpass]] [--chains K [--samples N]] [--batches NB] [--sections] [--angles] [--fit]
--lag1 / --pairs default: after the above, `rounds` alternating rounds of `steps` accumulations each of (a) the plain accumulate,
(b) with lag-1 tracking (k_moments_accum_lag: 10 x 8 B per selected element) and (c) with the default pairs (k_moments_pairs: 6 x 8 B
per pair element, timed apart from the mean launch that follows it); per launch the algorithmic bytes, the achieved bytes/s and
their ratio to (a) in the same round.
--hist [nbins]: alternating rounds of (a) the plain accumulate and (h) the histogram launch (k_moments_hist, 16-bit counters) on the
default index planes, at nbins and at 16 bins; per launch the line-granular traffic -- 8 B of x plus the record's 128-byte request
read and written once per counted pixel -- its bytes/s and the ratio to
(a)'s algorithmic bytes/s in the same round; then the read-out of three quantiles of one plane and the records' memory.
--hist --range-maps: in every round also (p) the same planes registered with per-pixel ranges -- maps that hold every plane's
default bounds in every pixel, so that the same pixels are counted -- which go through the form of the launch that streams lo and
hi beside x (k_moments_hist_px): 16 B more per pixel and plane; its time over (h)'s of the same round against the byte ratio.
--hist --signals: histograms that read the default signals (one range per signal, from a pilot of three iterations), filled by the
HIST form of the signal launch itself: alternating rounds of (s) the plain signal launch, (h) the scalar-range k_moments_hist launch
over as many index planes as there are signals and (f) the fused launch; (f) against (s) + (h), what an unfused form would cost at
best.  Nothing else of --hist or --signals is run.
--signals: alternating rounds of (a) the plain accumulate and (s) the signal launch (k_moments_signal) on the default signals; per
launch the algorithmic bytes -- per segment (amplitude planes + index planes read + 4 x outputs) x 8 B x pixels -- its bytes/s and
the ratio to (a)'s in the same round.
--signals --bandpass: every second band of the model becomes an integrated bandpass of nine samples (the bands of the default
signals among them), and only the signal launch is timed -- the bandpass form of k_moments_signal, a launch of its own; no Gibbs
iteration is run.
--chains K: K chains over the same data (open_chain), three samples each with lag-1 and one histogram plane (64 bins x 16 bit);
`rounds` alternating rounds of `steps` read-outs each, timed with events on the stream: (y) the single-chain std read-out
(k_moments_finish: 2 x 8 B per element), (r) R-hat over the chains ((2 K + 1) x 8 B), (e) the pooled ESS ((5 K + 1) x 8 B) and (q)
three pooled quantiles (K x 128 B + 3 x 8 B per pixel); per read-out its bytes/s and the ratio to (y) in the same round; then the
rank-normalised R-hat of the same histograms (k_chains_rank: K x 128 B + 8 B per pixel) as (b) bulk, (f) folded and (m) the
larger of the two, each also as its time over (q)'s of the same round.  --samples N: N samples per chain instead of three (the
rank read-outs form one score per non-empty bin, so their time grows with the bins the samples reach).  Nothing else of the above
is run.
--batches NB: the batched accumulators (dangx_moments_batches) with NB batches on up to four of the default index planes, two chains.
`rounds` alternating rounds in one process of (a) the plain k_moments_accum launch and (b) the batch launch of the same
accumulations (5 x 8 B per element each; batches long enough that no merge falls into the round), per byte; then, after NB
samples with batches of one sample (every batch full), rounds of (y) the single-chain std read-out, (s) split R-hat of one chain
(k_batches_stat: (2 NB + 1) x 8 B per element) and (c) of two chains (k_chains_batches: (4 NB + 1) x 8 B); then the time of the
merges the next 3 NB + 1 accumulations cause.  Nothing else of the above is run.
--sections: one chain with lag-1 and one histogram plane (64 bins x 16 bit); three alternating rounds in one process of (c) a plain
hipMemcpyAsync device to device, (s) the same on a stream of its own, (g) dangx_moments_section_get_dev and (p) _put_dev into a
holder, of the same bytes: the histogram's records (one copy) and a PLANES section (one copy per plane and part); `steps` copies
per timing, wall time around a device synchronisation.  Nothing else of the above is run.
--angles: the polarisation-angle launch (k_moments_angle) on the default angles against the signal launch (k_moments_signal) on the
{Q, U, P} signals of the same (component, band): `rounds` alternating rounds in one process of `steps` accumulations each with (s)
the signals alone and (g) the angles alone registered, an empty selection, after two Gibbs iterations; per launch the time, the
algorithmic bytes -- per component the Q and U amplitude and index planes read once, and per output two accumulator planes read and
written -- and their bytes/s; then (g) / (s) over the rounds.  Nothing else of the above is run.
--fit: the goodness-of-fit launch (k_moments_fit) on the default fit items (every plane's chi^2 map and every band's residual)
against the plain accumulate: `rounds` alternating rounds in one process of `steps` accumulations each with (a) the default
selection alone and (f) the fit items alone registered, after two Gibbs iterations; per launch the time, the algorithmic bytes --
per plane data and rms of every band, every component's amplitude and index planes, the mask, and 32 B per item -- their bytes/s
and (f)'s rate over (a)'s; then whole iterations with an accumulation after each, without and with the fit items.  Nothing else of
the above is run."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dang_amd as da  # noqa: E402
from dang_amd import synth  # noqa: E402

COPY_CEILING_TBS = 6.29

argv = list(sys.argv[1:])
hist_bins = 0
if "--hist" in argv:
    i = argv.index("--hist")
    hist_bins = 64
    if i + 1 < len(argv) and argv[i + 1].isdigit():
        hist_bins = int(argv.pop(i + 1))
nchains = 0
if "--chains" in argv:
    i = argv.index("--chains")
    nchains = int(argv.pop(i + 1))
nsamples = 3
if "--samples" in argv:
    i = argv.index("--samples")
    nsamples = int(argv.pop(i + 1))
nbat = 0
if "--batches" in argv:
    i = argv.index("--batches")
    nbat = int(argv.pop(i + 1))
args = [a for a in argv if not a.startswith("--") and a != "default"]
want_lag1 = "--lag1" in sys.argv
want_pairs = "--pairs" in sys.argv
if want_pairs and sys.argv[sys.argv.index("--pairs") + 1:][:1] != ["default"]:
    sys.exit("--pairs takes 'default'")
nside = int(args[0]) if len(args) > 0 else 1024
steps = int(args[1]) if len(args) > 1 else 10
rounds = int(args[2]) if len(args) > 2 else 5
dev = torch.device("cuda", 0)
want_bandpass = "--bandpass" in sys.argv
dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=nside, device=dev, as_numpy=False, start="truth" if want_bandpass else "prior")
if want_bandpass:
    rng = np.random.default_rng(4)
    for b in bands[1::2]:
        nu = b.nu_c * 1e9 * np.linspace(0.9, 1.1, 9)
        tau = rng.uniform(0.2, 1.0, nu.size)
        b.id, b.nu0, b.tau0 = "bp", nu, tau / tau.sum()
eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
if want_bandpass:
    da.moments_begin(dpar, ddata, sel=np.zeros(len(comps), dtype=np.int32))
    specs = da.moments_signals(dpar, ddata)
    assert all(bands[j].id != "delta" for l, j, k in specs)
    da.moments_accumulate(ddata)   # table upload
    for r in range(rounds):
        eng.profile(True)
        for _ in range(steps):
            da.moments_accumulate(ddata)
        prof = eng.profile_get()["k_signal"]
        eng.profile(False)
        print("round %d: bandpass form, %d signals at integrated bands of 9 samples: %.3f ms per launch (%d launches)"
              % (r + 1, len(specs), prof["total_ms"] / prof["launches"], prof["launches"]))
    sys.exit(0)
if "--angles" in sys.argv:
    npx = meta["npix"]
    for it in (1, 2):
        da.gibbs_iteration(dpar, ddata, it, want_counts=False)
    angles = da.default_angle_specs(dpar, comps, bands)
    sigs = [(l, j, k) for l, j in angles for k in (1, 2, 3)]
    none = np.zeros(len(comps), dtype=np.int32)
    src = sum(2 * (1 + comps[l].nindices) for l in sorted({l for l, j in angles}))      # Q and U: amplitude + index planes
    g_planes, s_planes = src + 4 * len(angles), src + 4 * len(sigs)

    def per_launch(register, family):
        da.moments_begin(dpar, ddata, sel=none)
        register()
        da.moments_accumulate(ddata)   # table upload
        eng.profile(True)
        for _ in range(steps):
            da.moments_accumulate(ddata)
        prof = eng.profile_get()
        eng.profile(False)
        assert set(prof) == {family}, prof
        return prof[family]["total_ms"] / prof[family]["launches"]

    print("C3 at Nside %d, %d pixels: angles %s; (s) k_moments_signal on their %d {Q, U, P} signals, %d planes of 8 B per pixel; (g) "
          "k_moments_angle, %d planes" % (nside, npx, [(comps[l].label, bands[j].label) for l, j in angles], len(sigs), s_planes, g_planes))
    s_all, g_all = [], []
    for r in range(rounds):
        s_ms = per_launch(lambda: da.moments_signals(dpar, ddata, specs=sigs), "k_signal")
        g_ms = per_launch(lambda: da.moments_angles(dpar, ddata, specs=angles), "k_angle")
        s_all.append(s_ms)
        g_all.append(g_ms)
        print("round %d: (s) %.3f ms, %.2f GB algorithmic -> %.2f TB/s; (g) %.3f ms, %.2f GB -> %.2f TB/s; (g) / (s) = %.3f"
              % (r + 1, s_ms, 8e-9 * s_planes * npx, 8e-9 * s_planes * npx / s_ms, g_ms, 8e-9 * g_planes * npx, 8e-9 * g_planes * npx / g_ms,
                 g_ms / s_ms))
    print("(s) median %.3f ms (spread %.3f .. %.3f); (g) median %.3f ms (spread %.3f .. %.3f); target: (g) <= (s) within the spread"
          % (float(np.median(s_all)), min(s_all), max(s_all), float(np.median(g_all)), min(g_all), max(g_all)))
    print("accumulators: 16 B x %d pixels x %d angles = %.2f GB" % (npx, len(angles), 16.0 * npx * len(angles) * 1e-9))
    sys.exit(0)
if "--fit" in sys.argv:
    npx, nb = meta["npix"], meta["nbands"]
    for it in (1, 2):
        da.gibbs_iteration(dpar, ddata, it, want_counts=False)
    fit = da.default_fit_specs(dpar, comps, bands)
    none = np.zeros(len(comps), dtype=np.int32)
    sel = da.default_moment_selection(dpar, comps)
    a_planes = 5 * sum(bin(int(w)).count("1") for w in sel)
    state = sum(1 + c.nindices for c in comps)          # every component's amplitude and index planes are read on every plane
    fit_planes = sorted({k for _, _, k in fit})
    f_bytes = sum(16 * nb + 8 * state + 8 + 32 * sum(1 for s in fit if s[2] == k) for k in fit_planes)

    def per_launch(register, family):
        register()
        da.moments_accumulate(ddata)   # table upload
        eng.profile(True)
        for _ in range(steps):
            da.moments_accumulate(ddata)
        prof = eng.profile_get()
        eng.profile(False)
        assert set(prof) == {family}, prof
        return prof[family]["total_ms"] / prof[family]["launches"]

    def fit_only():
        da.moments_begin(dpar, ddata, sel=none)
        da.moments_fit(dpar, ddata, specs=fit)

    print("C3 at Nside %d, %d pixels, %d bands: (a) k_moments_accum on the default selection, %d x 8 B per pixel; (f) k_moments_fit on the "
          "default %d items (%d planes): %d B per pixel = data + rms %d, state %d, mask %d, items %d"
          % (nside, npx, nb, a_planes, len(fit), len(fit_planes), f_bytes, 16 * nb * len(fit_planes), 8 * state * len(fit_planes),
             8 * len(fit_planes), 32 * len(fit)))
    a_all, f_all, ratio = [], [], []
    for r in range(rounds):
        a_ms = per_launch(lambda: da.moments_begin(dpar, ddata), "k_moments")
        f_ms = per_launch(fit_only, "k_fit")
        a_bw, f_bw = 8e-9 * a_planes * npx / a_ms, 1e-9 * f_bytes * npx / f_ms
        a_all.append(a_ms); f_all.append(f_ms); ratio.append(f_bw / a_bw)
        print("round %d: (a) %.3f ms, %.2f GB algorithmic -> %.2f TB/s; (f) %.3f ms, %.2f GB -> %.2f TB/s = %.3f of (a)"
              % (r + 1, a_ms, 8e-9 * a_planes * npx, a_bw, f_ms, 1e-9 * f_bytes * npx, f_bw, f_bw / a_bw))
    print("(a) median %.3f ms (spread %.3f .. %.3f); (f) median %.3f ms (spread %.3f .. %.3f); (f) / (a) per byte: median %.3f (spread %.3f .. %.3f)"
          % (float(np.median(a_all)), min(a_all), max(a_all), float(np.median(f_all)), min(f_all), max(f_all), float(np.median(ratio)),
             min(ratio), max(ratio)))
    # whole iterations: the default selection accumulated after every iteration, without and with the fit items, alternating
    it = 2
    walls = {False: [], True: []}
    for r in range(rounds):
        for with_fit in (False, True):
            da.moments_begin(dpar, ddata)
            if with_fit:
                da.moments_fit(dpar, ddata, specs=fit)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                it += 1
                da.gibbs_iteration(dpar, ddata, it, want_counts=False)
                da.moments_accumulate(ddata)
            torch.cuda.synchronize()
            walls[with_fit].append((time.perf_counter() - t0) / steps * 1e3)
        print("round %d: iteration + accumulate %.2f ms without, %.2f ms with the fit items" % (r + 1, walls[False][-1], walls[True][-1]))
    print("per iteration: median %.2f ms without, %.2f ms with (+%.2f ms)" % (float(np.median(walls[False])), float(np.median(walls[True])),
                                                                           float(np.median(walls[True])) - float(np.median(walls[False]))))
    print("accumulators: 16 B x %d pixels x %d items = %.2f GB" % (npx, len(fit), 16.0 * npx * len(fit) * 1e-9))
    sys.exit(0)
if "--sections" in sys.argv:
    import ctypes
    from dang_amd import api
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    sel = da.moments_begin(dpar, ddata)
    da.moments_pairs(dpar, ddata, pairs=[], lag1=True)
    hp = da.moments_hist(dpar, ddata, planes=da.default_hist_planes(dpar, comps, sel)[:1], nbins=64, bits=16)
    da.gibbs_iteration(dpar, ddata, 1, want_counts=False)
    da.moments_accumulate(ddata)
    holder = api._holder_engine(eng)
    holder.moments_begin_like(eng)
    side = torch.cuda.Stream()
    l, what, _ = hp[0]
    print("C3 at Nside %d, %d pixels: sections of one chain, get_dev / put_dev (into a holder) against hipMemcpyAsync device to device of the "
          "same bytes, %d copies per timing" % (nside, meta["npix"], steps))
    for name, sec in (("HIST(0), 64 bins x 16 bit", ("HIST", 0, 0)), ("PLANES(%s, %d), five parts" % (comps[l].label, what), ("PLANES", l, what))):
        n = eng.moments_section_bytes(*sec)
        a = torch.empty(n, dtype=torch.uint8, device=dev)
        b = torch.empty(n, dtype=torch.uint8, device=dev)
        eng.moments_section_get(*sec, device=True, out=a)
        holder.moments_section_put(*sec, a)            # the holder's buffer exists from here on
        torch.cuda.synchronize()

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        forms = [("c", "hipMemcpyAsync", lambda: hip.hipMemcpyAsync(b.data_ptr(), a.data_ptr(), n, 3, None)),
                 ("s", "hipMemcpyAsync on a stream of its own", lambda: hip.hipMemcpyAsync(b.data_ptr(), a.data_ptr(), n, 3, side.cuda_stream)),
                 ("g", "section_get_dev", lambda: eng.moments_section_get(*sec, device=True, out=b)),
                 ("p", "section_put_dev", lambda: holder.moments_section_put(*sec, a))]
        ratio = {"s": [], "g": [], "p": []}
        print("%s: %.3f GB" % (name, n * 1e-9))
        for r in range(3):
            line, c_ms = "  round %d:" % (r + 1), None
            for key, what_, fn in forms:
                ms = timed(fn)
                if key == "c":
                    c_ms = ms
                else:
                    ratio[key].append(ms / c_ms)
                line += " (%s) %s %.3f ms, %.0f GB/s copied%s;" % (key, what_, ms, n / ms * 1e-6, "" if key == "c" else " = %.3f x (c)'s time" % (ms / c_ms))
            print(line)
        for key in "sgp":
            print("  (%s) time / (c)'s: median %.3f (spread %.3f .. %.3f)" % (key, float(np.median(ratio[key])), min(ratio[key]), max(ratio[key])))
    sys.exit(0)
if nchains:
    runs = [(dpar, ddata)] + [da.open_chain(dpar, ddata, dpar.seed + k) for k in range(1, nchains)]
    engs = [d.engine for _, d in runs]
    for p, d in runs:
        sel = da.moments_begin(p, d)
        da.moments_pairs(p, d, pairs=[], lag1=True)
        hp = da.moments_hist(p, d, planes=da.default_hist_planes(p, comps, sel)[:1], nbins=64, bits=16)
    for it in range(1, nsamples + 1):
        for p, d in runs:
            da.gibbs_iteration(p, d, it, want_counts=False)
            da.moments_accumulate(d)
    l, what, _ = hp[0]
    nplanes = bin((int(sel[l]) >> (3 + 3 * (what - 1))) & 7).count("1")
    npx = meta["npix"]
    out = torch.zeros((meta["nmaps"], npx), dtype=torch.float64, device=dev)
    outq = torch.zeros((3, npx), dtype=torch.float64, device=dev)
    q3 = (0.16, 0.5, 0.84)

    def timed(fn):
        fn()   # first use: scratch, events
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    out1 = torch.zeros((npx,), dtype=torch.float64, device=dev)
    forms = [("y", "single-chain std", 2 * 8 * nplanes, lambda: eng._chk(eng.lib.dangx_moments_get_dev(eng.h, l, what, 1, 0, out.data_ptr()))),
             ("r", "R-hat", (2 * nchains + 1) * 8 * nplanes, lambda: da.chains_get(engs, l, what, "rhat", device=True, out=out)),
             ("e", "pooled ESS", (5 * nchains + 1) * 8 * nplanes, lambda: da.chains_get(engs, l, what, "ess", device=True, out=out)),
             ("q", "3 pooled quantiles", nchains * 128 + 3 * 8, lambda: da.chains_hist_stat(engs, 0, "quantile", q=q3, device=True, out=outq))]
    forms += [(key, "%s rank R-hat" % stat, nchains * 128 + 8, lambda stat=stat: da.chains_hist_rank(engs, 0, stat, device=True, out=out1))
              for key, stat in (("b", "bulk"), ("f", "folded"), ("m", "max"))]
    ratios = {k: [] for k, _, _, _ in forms[1:]}
    to_q = {k: [] for k in "bfm"}                       # the time of a rank read-out over the quantile read-out's of the same round
    print("C3 at Nside %d, %d chains of %d samples, %s index %d: %d planes of %d pixels" % (nside, nchains, engs[0].moments_count(),
                                                                                          comps[l].label, what, nplanes, npx))
    for r in range(rounds):
        line, y_bw, q_ms = "round %d:" % (r + 1), None, None
        for key, name, per_pix, fn in forms:
            ms = timed(fn)
            bw = per_pix * npx / ms * 1e-9
            if key == "y":
                y_bw = bw
            else:
                ratios[key].append(bw / y_bw)
            if key == "q":
                q_ms = ms
            if key in to_q:
                to_q[key].append(ms / q_ms)
            line += " (%s) %s %.3f ms, %.3f GB -> %.2f TB/s%s;" % (key, name, ms, per_pix * npx * 1e-9, bw, "" if key == "y" else " = %.3f of (y)" % (bw / y_bw))
        print(line)
    for key, name, _, _ in forms[1:]:
        print("(%s) %s / (y): median %.3f (spread %.3f .. %.3f)%s" % (key, name, float(np.median(ratios[key])), min(ratios[key]), max(ratios[key]),
                                                                     "" if key in "qbfm" else "; expected >= 0.8"))
    for key, name, _, _ in forms[-3:]:
        print("(%s) %s, time / (q)'s: median %.3f (spread %.3f .. %.3f)" % (key, name, float(np.median(to_q[key])), min(to_q[key]), max(to_q[key])))
    sys.exit(0)
if nbat:
    npx = meta["npix"]
    runs = [(dpar, ddata), da.open_chain(dpar, ddata, dpar.seed + 1)]
    engs = [d.engine for _, d in runs]
    for p, d in runs:
        da.gibbs_iteration(p, d, 1, want_counts=False)
    sel = da.moments_begin(dpar, ddata)
    nsel = sum(bin(int(w) & 7).count("1") + bin(int(w) >> 3).count("1") for w in sel)
    bp = da.default_hist_planes(dpar, comps, sel)[:4]
    da.moments_batches(dpar, ddata, planes=bp, nbatch=nbat, batch_len=1 << 40)
    da.moments_accumulate(ddata)   # table upload
    print("C3 at Nside %d: %d selected planes, %d batch planes x %d batches of %d pixels = %.2f GB of batch accumulators"
          % (nside, nsel, len(bp), nbat, npx, 16.0 * npx * len(bp) * nbat * 1e-9))
    ratios = []
    for r in range(rounds):
        eng.profile(True)
        for _ in range(steps):
            da.moments_accumulate(ddata)
        prof = eng.profile_get()
        eng.profile(False)
        a_ms, b_ms = (prof[k]["total_ms"] / prof[k]["launches"] for k in ("k_moments", "k_batch"))
        a_bw, b_bw = 40.0 * nsel * npx / a_ms * 1e-9, 40.0 * len(bp) * npx / b_ms * 1e-9
        ratios.append(b_bw / a_bw)
        print("round %d: (a) plain %.3f ms, %.2f GB -> %.2f TB/s; (b) batch launch %.3f ms, %.2f GB -> %.2f TB/s = %.3f of (a)"
              % (r + 1, a_ms, 40.0 * nsel * npx * 1e-9, a_bw, b_ms, 40.0 * len(bp) * npx * 1e-9, b_bw, b_bw / a_bw))
    print("(b) / (a) per byte: median %.3f (spread %.3f .. %.3f)" % (float(np.median(ratios)), min(ratios), max(ratios)))
    for p, d in runs:
        da.moments_begin(p, d, sel=sel)
        da.moments_batches(p, d, planes=bp, nbatch=nbat, batch_len=1)
    for it in range(nbat):
        for p, d in runs:
            da.moments_accumulate(d)
    assert eng.moments_batches_info() == {"batch_len": 1, "nfull": nbat, "partial": 0}
    l, what, _ = bp[0]
    nplanes = bin((int(sel[l]) >> (3 + 3 * (what - 1))) & 7).count("1")
    out3 = torch.zeros((meta["nmaps"], npx), dtype=torch.float64, device=dev)
    out1 = torch.zeros((npx,), dtype=torch.float64, device=dev)

    def timed(fn):
        fn()   # first use: scratch, events
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    forms = [("y", "single-chain std", 2 * 8 * nplanes, lambda: eng._chk(eng.lib.dangx_moments_get_dev(eng.h, l, what, 1, 0, out3.data_ptr()))),
             ("s", "split R-hat, one chain", (2 * nbat + 1) * 8, lambda: eng._chk(eng.lib.dangx_moments_batches_get_dev(eng.h, 0, 4, 0, 0, out1.data_ptr()))),
             ("c", "split R-hat, two chains", (4 * nbat + 1) * 8, lambda: da.chains_batches_get(engs, 0, "split_rhat", device=True, out=out1))]
    ratios = {k: [] for k, _, _, _ in forms[1:]}
    rates = {k: [] for k, _, _, _ in forms}
    for r in range(rounds):
        line, y_bw = "round %d:" % (r + 1), None
        for key, name, per_pix, fn in forms:
            ms = timed(fn)
            bw = per_pix * npx / ms * 1e-9
            if key == "y":
                y_bw = bw
            else:
                ratios[key].append(bw / y_bw)
            rates[key].append(bw)
            line += " (%s) %s %.3f ms, %.3f GB -> %.2f TB/s%s;" % (key, name, ms, per_pix * npx * 1e-9, bw, "" if key == "y" else " = %.3f of (y)" % (bw / y_bw))
        print(line)
    for key, name, _, _ in forms[1:]:
        print("(%s) %s / (y): median %.3f (spread %.3f .. %.3f); expected >= 0.8" % (key, name, float(np.median(ratios[key])), min(ratios[key]), max(ratios[key])))
    # (y) moves 0.2 GB that the accumulations just wrote: where it reads above the copy ceiling it is partly served from cache, and
    # the ratios to it are ratios to an inflated denominator -- hence the ratios to the ceiling as well
    for key, name, _, _ in forms:
        print("(%s) %s / the %.2f TB/s copy ceiling: %.3f .. %.3f" % (key, name, COPY_CEILING_TBS, min(rates[key]) / COPY_CEILING_TBS,
                                                                  max(rates[key]) / COPY_CEILING_TBS))
    eng.profile(True)
    for _ in range(3 * nbat + 1):
        da.moments_accumulate(ddata)
    mg = eng.profile_get(by_planes=True).get(("k_batch", 2))
    eng.profile(False)
    print("k_batches_merge: %.3f ms per merge (%d merges of %d planes x %d batches, %.2f GB read + written each)"
          % (mg["total_ms"] / mg["launches"], mg["launches"], len(bp), nbat, (2 + 1 + 1) * 8.0 * nbat * len(bp) * npx * 1e-9))
    sys.exit(0)
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


def launches(mode):
    """ms per launch of `steps` accumulations after a fresh begin: mode 'plain' | 'lag1' | 'pairs' -> (mean launch, pair launch or None)"""
    da.moments_begin(dpar, ddata, sel=sel)
    npairs = 0
    if mode == "lag1":
        da.moments_pairs(dpar, ddata, pairs=[], lag1=True)
    elif mode == "pairs":
        npairs = len(da.moments_pairs(dpar, ddata, lag1=False))
    da.moments_accumulate(ddata)   # table upload; with lag-1 the first-sample form of the kernel
    eng.profile(True)
    for _ in range(steps):
        da.moments_accumulate(ddata)
    tot = eng.profile_get()["k_moments"]
    pr = eng.profile_get(by_planes=True).get(("k_moments", 2))
    eng.profile(False)
    if pr is None:
        return tot["total_ms"] / tot["launches"], None, npairs
    return (tot["total_ms"] - pr["total_ms"]) / (tot["launches"] - pr["launches"]), pr["total_ms"] / pr["launches"], npairs


if want_lag1 or want_pairs:
    npx = meta["npix"]
    res = {"plain": [], "lag1": [], "pairs": []}
    for r in range(rounds):
        a_ms = launches("plain")[0]
        a_bw = 5 * 8 * planes * npx / a_ms * 1e-9
        res["plain"].append(a_bw)
        line = "round %d: (a) plain %.3f ms, %.2f GB -> %.2f TB/s" % (r + 1, a_ms, 5 * 8 * planes * npx * 1e-9, a_bw)
        if want_lag1:
            b_ms = launches("lag1")[0]
            b_bw = 10 * 8 * planes * npx / b_ms * 1e-9
            res["lag1"].append(b_bw / a_bw)
            line += "; (b) lag-1 %.3f ms, %.2f GB -> %.2f TB/s = %.3f of (a)" % (b_ms, 10 * 8 * planes * npx * 1e-9, b_bw, b_bw / a_bw)
        if want_pairs:
            _, c_ms, npairs = launches("pairs")
            c_bw = 6 * 8 * npairs * npx / c_ms * 1e-9
            res["pairs"].append(c_bw / a_bw)
            line += "; (c) %d pairs %.3f ms, %.2f GB -> %.2f TB/s = %.3f of (a)" % (npairs, c_ms, 6 * 8 * npairs * npx * 1e-9, c_bw, c_bw / a_bw)
        print(line)
    print("(a) over the rounds: %.2f .. %.2f TB/s" % (min(res["plain"]), max(res["plain"])))
    for key, name in (("lag1", "(b) lag-1"), ("pairs", "(c) pairs")):
        if res[key]:
            print("%s / (a): median %.3f (spread %.3f .. %.3f); target >= 0.9" % (name, float(np.median(res[key])), min(res[key]), max(res[key])))


def hist_launches(nbins, bits=16, range_maps=False):
    """(ms per k_moments_hist launch, ms per plain k_moments launch beside it, registrations, counted pixels per launch, read-out ms);
    range_maps: every plane's default bounds as a pair of per-pixel maps (the launch that streams them)"""
    da.moments_begin(dpar, ddata, sel=sel)
    ranges = None
    if range_maps:
        hp = da.default_hist_planes(dpar, comps, sel)
        one = torch.ones(meta["npix"], dtype=torch.float64, device=dev)
        ranges = [(one * float(comps[l].uni_prior[w - 1][0]), one * float(comps[l].uni_prior[w - 1][1])) for l, w, k in hp]
    hp = da.moments_hist(dpar, ddata, ranges=ranges, nbins=nbins, bits=bits)
    da.moments_accumulate(ddata)   # table upload
    eng.profile(True)
    for _ in range(steps):
        da.moments_accumulate(ddata)
    prof = eng.profile_get()
    eng.profile(False)
    counted = sum(float(eng.moments_hist_stat(r, "n", device=True).sum()) for r in range(len(hp))) / (steps + 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.moments_hist_stat(0, "quantile", q=(0.16, 0.5, 0.84), device=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return (prof["k_hist"]["total_ms"] / prof["k_hist"]["launches"], prof["k_moments"]["total_ms"] / prof["k_moments"]["launches"],
            len(hp), counted, (t1 - t0) * 1e3)


if hist_bins and "--signals" not in sys.argv:
    npx = meta["npix"]
    forms = [hist_bins] + ([16] if hist_bins != 16 else [])
    ratios = {nb: [] for nb in forms}
    px_ratios = []
    for r in range(rounds):
        a_ms = launches("plain")[0]
        a_bw = 5 * 8 * planes * npx / a_ms * 1e-9
        line = "round %d: (a) plain %.3f ms -> %.2f TB/s" % (r + 1, a_ms, a_bw)
        for nb in forms:
            h_ms, m_ms, nreg, counted, q_ms = hist_launches(nb)
            traffic = 8.0 * nreg * npx + 2 * 128.0 * counted
            h_bw = traffic / h_ms * 1e-9
            ratios[nb].append(h_bw / a_bw)
            line += "; (h) %d bins x 16 bit on %d planes %.3f ms, %.2f GB line-granular (%.0f counted pixels) -> %.2f TB/s = %.3f of (a)" \
                    "; k_moments beside it %.3f ms; 3 quantiles of one plane %.3f ms" % (nb, nreg, h_ms, traffic * 1e-9, counted, h_bw,
                                                                                       h_bw / a_bw, m_ms, q_ms)
            if "--range-maps" in sys.argv and nb == hist_bins:
                p_ms, _, _, p_counted, pq_ms = hist_launches(nb, range_maps=True)
                p_traffic = traffic + 16.0 * nreg * npx
                px_ratios.append((p_ms / h_ms, p_traffic / traffic))
                line += "; (p) per-pixel ranges %.3f ms, %.2f GB (%.0f counted pixels) = %.3f of (h)'s time at %.3f of its bytes; 3 quantiles %.3f ms" \
                        % (p_ms, p_traffic * 1e-9, p_counted, p_ms / h_ms, p_traffic / traffic, pq_ms)
        print(line)
    for nb in forms:
        print("(h) %d bins / (a): median %.3f (spread %.3f .. %.3f)" % (nb, float(np.median(ratios[nb])), min(ratios[nb]), max(ratios[nb])))
    if px_ratios:
        t = [a for a, b in px_ratios]
        byte = float(np.median([b for a, b in px_ratios]))
        print("(p) / (h) time: median %.3f (spread %.3f .. %.3f); byte ratio %.3f; bound byte ratio x 1.10 = %.3f"
              % (float(np.median(t)), min(t), max(t), byte, 1.10 * byte))
    nreg = len(da.default_hist_planes(dpar, comps, sel))
    print("records: %d B x %d pixels x %d planes = %.2f GB at %d bins x 16 bit" % (hist_bins * 2, npx, nreg, hist_bins * 2.0 * npx * nreg * 1e-9, hist_bins))
    da.moments_begin(dpar, ddata, sel=sel)   # drops the records


def signal_planes(specs):
    """planes of 8 B per pixel one launch moves: per (component, plane class) the amplitude and index planes read once, and per
    output its mean and m2 read and written"""
    total = 0
    for l, cls in sorted({(l, 0 if k == 0 else 1) for l, j, k in specs}):
        kinds = {k for ll, j, k in specs if ll == l and (0 if k == 0 else 1) == cls}
        read = 1 if cls == 0 else (2 if (3 in kinds or {1, 2} <= kinds) else 1)
        total += read * (1 + comps[l].nindices) + 4 * sum(1 for ll, j, k in specs if ll == l and (0 if k == 0 else 1) == cls)
    return total


def signal_launches():
    da.moments_begin(dpar, ddata, sel=sel)
    specs = da.moments_signals(dpar, ddata)
    da.moments_accumulate(ddata)   # table upload
    eng.profile(True)
    for _ in range(steps):
        da.moments_accumulate(ddata)
    prof = eng.profile_get()
    eng.profile(False)
    return prof["k_signal"]["total_ms"] / prof["k_signal"]["launches"], prof["k_moments"]["total_ms"] / prof["k_moments"]["launches"], specs


if "--signals" in sys.argv and hist_bins:
    npx = meta["npix"]
    da.moments_begin(dpar, ddata, sel=sel)
    specs = da.moments_signals(dpar, ddata)
    for it in range(1001, 1004):                      # the pilot: three samples of the signals
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    sources = [("signal", s) for s in range(len(specs))]
    inf = float("inf")
    granges = [(float(torch.nan_to_num(lo, nan=inf).min()), float(torch.nan_to_num(hi, nan=-inf).max()))
               for lo, hi in da.hist_ranges_from_moments(ddata, sources, nsigma=5.0)]
    hp_n = da.default_hist_planes(dpar, comps, sel)[:len(specs)]
    assert len(hp_n) == len(specs), "fewer default index planes than default signals"

    def timed(register, family):
        da.moments_begin(dpar, ddata, sel=sel)
        nreg = register()
        da.moments_accumulate(ddata)   # table upload
        eng.profile(True)
        for _ in range(steps):
            da.moments_accumulate(ddata)
        prof = eng.profile_get()
        eng.profile(False)
        counted = sum(float(eng.moments_hist_stat(r, "n", device=True).sum()) for r in range(nreg)) / (steps + 1)
        return prof[family]["total_ms"] / prof[family]["launches"], counted

    def reg_fused():
        da.moments_signals(dpar, ddata)
        da.moments_hist(dpar, ddata, planes=sources, ranges=granges, nbins=hist_bins, bits=16)
        return len(sources)

    res = []
    for r in range(rounds):
        s_ms = signal_launches()[0]
        h_ms, h_counted = timed(lambda: len(da.moments_hist(dpar, ddata, planes=hp_n, nbins=hist_bins, bits=16)), "k_hist")
        f_ms, f_counted = timed(reg_fused, "k_signal")
        res.append(f_ms / (s_ms + h_ms))
        print("round %d: (s) %d signals %.3f ms; (h) k_moments_hist, %d bins x 16 bit on %d planes %.3f ms (%.0f counted pixels); (f) the fused "
              "signal-histogram launch %.3f ms (%.0f counted pixels) = %.3f of (s) + (h) = %.3f ms"
              % (r + 1, len(specs), s_ms, hist_bins, len(hp_n), h_ms, h_counted, f_ms, f_counted, f_ms / (s_ms + h_ms), s_ms + h_ms))
    print("(f) / ((s) + (h)): median %.3f (spread %.3f .. %.3f); must not exceed 1" % (float(np.median(res)), min(res), max(res)))
    print("records: %d B x %d pixels x %d signals = %.2f GB at %d bins x 16 bit" % (hist_bins * 2, npx, len(specs), hist_bins * 2.0 * npx * len(specs) * 1e-9, hist_bins))
    da.moments_begin(dpar, ddata, sel=sel)

if "--signals" in sys.argv and not hist_bins:
    npx = meta["npix"]
    ratios = []
    for r in range(rounds):
        a_ms = launches("plain")[0]
        a_bw = 5 * 8 * planes * npx / a_ms * 1e-9
        s_ms, m_ms, specs = signal_launches()
        traffic = 8.0 * signal_planes(specs) * npx
        s_bw = traffic / s_ms * 1e-9
        ratios.append(s_bw / a_bw)
        print("round %d: (a) plain %.3f ms -> %.2f TB/s; (s) %d signals %.3f ms, %.2f GB algorithmic -> %.2f TB/s = %.3f of (a); k_moments "
              "beside it %.3f ms" % (r + 1, a_ms, a_bw, len(specs), s_ms, traffic * 1e-9, s_bw, s_bw / a_bw, m_ms))
    print("(s) / (a): median %.3f (spread %.3f .. %.3f); target >= 0.9" % (float(np.median(ratios)), min(ratios), max(ratios)))
    print("accumulators: 16 B x %d pixels x %d signals = %.2f GB" % (npx, len(specs), 16.0 * npx * len(specs) * 1e-9))
    da.moments_begin(dpar, ddata, sel=sel)   # drops the accumulators
