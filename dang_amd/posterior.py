"""Posterior summaries accumulated on the device (dangx_moments_* / dangx_chains_*, include/dangx.h), host side.

Registration over the contexts of a process (moments_begin, moments_pairs, moments_hist, moments_signals, moments_batches and their
default_* planners), the thin several-chain read-outs (chains_get*), and the functions that assemble {key: maps} over shards.
Those are ONE builder (_build) driven by two descriptions:

  a source   what a *_maps call reads its chains through: one chain of this process (_OneChain), several (_LocalChains), or
             the chains of every rank of a process group (DistChains); all with shards, counts, fetch, batches_info, finish, here
  a family   what is read (FAMILIES: planes, pair, hist, rank, batches, signal, angle, fit): its registration, how an item becomes a key,
             which sections it owns, which statistics are available, its two thin getters and the checks each form makes

Chains of other processes (dist_chains) and save / restore (moments_save, moments_load) are thin layers over the sections of the
accumulator state and take their section lists from the same families.  Engine stays in api.py; this module imports api."""
import os
import struct
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

from . import _lib as L
from . import api as _api
from . import dist as _dist
from .api import DangxError, Engine, _code, _ctx_array, _engines_of, _hist_stat_args, _is_range_maps, _is_torch, _readout_dest, _registration

__all__ = ["GLOBAL_TYPES", "BATCH_STATS", "default_moment_selection", "default_moment_pairs", "default_hist_planes", "default_signal_specs",
           "moments_begin", "moments_accumulate", "moments_pairs", "moments_hist", "moments_signals", "moments_batches",
           "posterior_maps", "posterior_pair_maps", "posterior_quantile_maps", "posterior_batch_maps", "posterior_signal_maps",
           "chains_posterior_maps", "chains_pair_maps", "chains_quantile_maps", "chains_rank_maps", "chains_batch_maps", "chains_signal_maps",
           "chains_get", "chains_get_template", "chains_get_signal", "chains_get_pair", "chains_hist_stat", "chains_hist_rank",
           "chains_batches_get", "open_chain", "DistChains", "dist_chains", "head_unpack", "head_diff", "dist_verdict",
           "moments_save", "moments_load"]

# --------------------------------------------------------------------------- posterior moments
# The reference writes every sample (write_maps every iter_out iterations, src/dang.f90:119-121) and averages the files afterwards
# (scripts/make_mean_maps.py: return_mean_map, return_std_map = np.std).  Here the moments accumulate on the device and are read once.

_FLAG_PLANES = ((L.FLAG_T, 1), (L.FLAG_Q, 2), (L.FLAG_U, 4), (L.FLAG_QU, 6))   # poltype bit -> plane bits T=1, Q=2, U=4
GLOBAL_TYPES = ("template", "monopole", "hi_fit")


def _flag_planes(flag):
    return sum(bits for f, bits in _FLAG_PLANES if flag & f) & 7


def default_moment_selection(dpar, component_list):
    """Selection words (include/dangx.h, dangx_moments_begin) of what a run samples: amplitude plane k of component l when
    c.sample_amplitude holds and a CG group with c's cg_group has a pol_flag covering k; index plane k of index j when
    c.sample_index[j] holds and a flag of c.pol_flag[j] covers k.  Pure Python: needs no device."""
    sel = np.zeros(len(component_list), dtype=np.int32)
    for l, c in enumerate(component_list):
        if c.sample_amplitude:
            for g in dpar.cg_groups:
                if g.cg_group == c.cg_group:
                    for f in g.pol_flag:
                        sel[l] |= _flag_planes(f)
        for j in range(c.nindices):
            if j < len(c.sample_index) and c.sample_index[j]:
                for f in (c.pol_flag[j] if j < len(c.pol_flag) else []):
                    sel[l] |= _flag_planes(f) << (3 + 3 * j)
    return sel


def moments_begin(dpar, ddata, sel=None, engines=None):
    """dangx_moments_begin on every context of this process; sel=None: default_moment_selection(dpar, ...).  Returns the selection."""
    engs = _engines_of(ddata, engines)
    if sel is None:
        sel = default_moment_selection(dpar, engs[0].component_list)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    for e in engs:
        e.moments_begin(sel)
    return sel


def moments_accumulate(ddata, engines=None):
    """One sample of the current state on every context (asynchronous on each context's stream)."""
    for e in _engines_of(ddata, engines):
        e.moments_accumulate()


def _mask_fill(m, mask, value):
    """Pixels whose mask (plane 1, as the reference tests it; make_mean_maps.py's mask[i] == 0) is 0 get `value` on every plane."""
    mask1 = np.asarray(mask.cpu().numpy() if _is_torch(mask) else mask)[0]
    out = np.array(m, dtype=np.float64, copy=True)
    out[..., mask1 == 0] = value
    return out


def posterior_maps(ddata, ddof=0, masked_value=None, engines=None):
    """{(label, 'amplitude' | ind_label): {'mean', 'std', 'n'}} of what moments_begin selected, as host arrays ([nmaps][npix]; template
    / monopole / hi_fit amplitudes [nmaps][nbands]).  Several contexts of this process (shard order): their shards side by side.
    masked_value (e.g. MISSVAL, healpy's UNSEEN, as make_mean_maps.py writes): pixels masked in ddata.masks plane 1 get it.
    With several ranks each rank returns its shard: dist.gather_maps(..., bounds) assembles the sky, as for the state."""
    return _build(PLANES, "posterior_maps", _OneChain(ddata, engines), ddof=ddof, masked_value=masked_value)


def _plane_name(c, what):
    return "amplitude" if what == 0 else (c.ind_label[what - 1] if what - 1 < len(c.ind_label) else "index%d" % what)


def _int_tuple(p):
    return tuple(int(v) for v in p)


def _register(method, dpar, ddata, engines, items, planner, tidy, **kw):
    """Engine.<method>(items, **kw) on every context of this process; items=None: planner(dpar, the components, the selection
    moments_begin made).  Returns the items."""
    engs = _engines_of(ddata, engines)
    if items is None:
        items = planner(dpar, engs[0].component_list, _registration(engs[0], "sel", method, "moments_begin"))
    items = [tidy(it) for it in items]
    for e in engs:
        getattr(e, method)(items, **kw)
    return items


def default_moment_pairs(dpar, component_list, sel):
    """The degeneracies of a pixel's own parameters, as [((l, what, plane), (l, what, plane)), ...] for moments_pairs: per component
    and plane k, (amplitude, index j) for every sampled index j whose plane k and the amplitude's plane k are both in `sel`, then
    (index 0, index 1) when both are sampled on plane k.  Component order, then plane, then that pair order.  Pure Python."""
    pairs = []
    for l, c in enumerate(component_list):
        if c.type in GLOBAL_TYPES:
            continue
        w = int(sel[l])
        for k in range(3):
            ind = [j for j in range(c.nindices) if (w >> (3 + 3 * j + k)) & 1]
            if (w >> k) & 1:
                pairs += [((l, 0, k), (l, 1 + j, k)) for j in ind]
            if 0 in ind and 1 in ind:
                pairs.append(((l, 1, k), (l, 2, k)))
    return pairs


def moments_pairs(dpar, ddata, pairs=None, lag1=True, engines=None):
    """dangx_moments_pairs on every context of this process, after moments_begin and before the first moments_accumulate;
    pairs=None: default_moment_pairs of the selection moments_begin made.  Returns the pair list."""
    return _register("moments_pairs", dpar, ddata, engines, pairs, default_moment_pairs, lambda p: (tuple(p[0]), tuple(p[1])), lag1=lag1)


def posterior_pair_maps(ddata, stat="corr", ddof=0, masked_value=None, engines=None):
    """{((label_a, name_a, plane_a), (label_b, name_b, plane_b)): [npix]} of the pairs moments_pairs registered: their correlation
    ('corr') or covariance ('cov', with ddof) maps; names as posterior_maps' keys, planes 0-based.  Several contexts of this
    process: their shards side by side.  masked_value: as in posterior_maps."""
    return _build(PAIR, "posterior_pair_maps", _OneChain(ddata, engines), stat=stat, ddof=ddof, masked_value=masked_value)


def default_hist_planes(dpar, component_list, sel):
    """[(l, what, plane), ...] for moments_hist: every plane in `sel` of every index the run samples (c.sample_index[j], the flag
    default_moment_selection follows), in component / index / plane order.  Their default range is the index's uni_prior, which
    the chain never leaves.  Pure Python."""
    planes = []
    for l, c in enumerate(component_list):
        if c.type in GLOBAL_TYPES:
            continue
        for j in range(c.nindices):
            if j < len(c.sample_index) and c.sample_index[j]:
                planes += [(l, 1 + j, k) for k in range(3) if (int(sel[l]) >> (3 + 3 * j + k)) & 1]
    return planes


def moments_hist(dpar, ddata, planes=None, ranges=None, nbins=64, bits=16, engines=None):
    """dangx_moments_hist on every context of this process, after moments_begin and before the first moments_accumulate;
    planes=None: default_hist_planes of the selection moments_begin made.  Returns the plane list.  A ranges[r] may be a pair of maps
    (lo, hi) -- a per-pixel range, Engine.moments_hist -- over the whole pixel range of this process (the contexts' shards side by
    side, as hist_ranges_from_moments returns them): every context is handed its slice by (pix0, npix).  Give every chain the same
    maps: the read-outs over several chains refuse chains whose maps differ."""
    engs = _engines_of(ddata, engines)
    if ranges is None or not any(_is_range_maps(r) for r in ranges):
        return _register("moments_hist", dpar, ddata, engs, planes, default_hist_planes, _hist_plane, ranges=ranges, nbins=nbins, bits=bits)
    if planes is None:
        planes = default_hist_planes(dpar, engs[0].component_list, _registration(engs[0], "sel", "moments_hist", "moments_begin"))
    planes = [_hist_plane(p) for p in planes]
    total = sum(e.npix for e in engs)
    for e in engs:
        e.moments_hist(planes, ranges=_slice_ranges(ranges, e.pix0 - engs[0].pix0, e.npix, total), nbins=nbins, bits=bits)
    return planes


def _hist_plane(p):
    """a histogram's source as the library takes it: (l, what, plane), or ("signal", s) -> (s, HIST_SIGNAL, 0)"""
    if isinstance(p[0], str) and p[0] == "signal":
        return (int(p[1]), L.HIST_SIGNAL, 0)
    return _int_tuple(p)


def _slice_ranges(ranges, off, npix, total):
    """ranges with every pair of maps over `total` pixels cut down to the `npix` pixels from `off` on; the rest as it is"""
    out = []
    for r in ranges:
        if _is_range_maps(r):
            if any(tuple(m.shape) != (total,) for m in r):
                raise DangxError("moments_hist: a per-pixel range is a pair of maps over this process's %d pixels, not of shape %s and %s"
                                 % (total, tuple(r[0].shape), tuple(r[1].shape)))
            r = (r[0][off:off + npix], r[1][off:off + npix])
        out.append(r)
    return out


def _ranges_from_mean_std(mean, std, nsigma, clip0=False):
    """(mean - nsigma std, mean + nsigma std); NaN where std is 0 or not finite (a pixel that never moved: a masked one).  clip0
    (a polarised intensity P, which is never negative): the lower bound is not below 0.  numpy arrays or torch tensors."""
    xp = __import__("torch") if _is_torch(mean) else np
    bad = ~(xp.isfinite(std) & (std > 0))
    nan = xp.full_like(mean, float("nan"))
    lo = mean - nsigma * std
    if clip0:
        lo = xp.where(lo < 0, xp.zeros_like(lo), lo)
    return xp.where(bad, nan, lo), xp.where(bad, nan, mean + nsigma * std)


def hist_ranges_from_moments(ddata, planes, nsigma=5.0, engines=None):
    """Per-pixel histogram ranges from the accumulators a pilot stretch left behind: for every plane (l, what, plane) or signal
    ("signal", s) of `planes` (the lower bound of a P signal clipped at 0)
    the pair (mean - nsigma std, mean + nsigma std) as device tensors over this process's pixels (the contexts' shards side by
    side), NaN where the standard deviation is 0 or not finite -- such a pixel counts nothing.  The planes must be selected in
    the pilot's moments_begin.  Intended use: a pilot of some iterations with moments_begin / moments_accumulate, this call,
    moments_begin again, then moments_hist(planes, ranges=these) -- with the same maps on every chain."""
    import torch
    engs = _engines_of(ddata, engines)
    out, cache = [], {}
    for l, what, k in (_hist_plane(p) for p in planes):
        if what == L.HIST_SIGNAL:                        # ("signal", s): the signal's own moments; P is clipped at 0
            mean = torch.cat([e.moments_get_signal(l, "mean", device=True) for e in engs])
            std = torch.cat([e.moments_get_signal(l, "std", device=True) for e in engs])
            out.append(_ranges_from_mean_std(mean, std, float(nsigma), clip0=_registration(engs[0], "signals", "hist_ranges_from_moments",
                                                                                          "moments_signals")[l][2] == 3))
            continue
        if (l, what) not in cache:
            cache[(l, what)] = [(e.moments_get(l, what, "mean", device=True), e.moments_get(l, what, "std", device=True)) for e in engs]
        mean = torch.cat([m[k] for m, _ in cache[(l, what)]])
        std = torch.cat([s[k] for _, s in cache[(l, what)]])
        out.append(_ranges_from_mean_std(mean, std, float(nsigma)))
    return out


def posterior_quantile_maps(ddata, q=(0.16, 0.5, 0.84), masked_value=None, engines=None):
    """{(label, name, plane): {'q': [nq][npix], 'mode': [npix], 'n': [npix], 'range': (lo, hi), 'nbins'}} of the histograms
    moments_hist registered; names as posterior_maps' keys, planes 0-based.  Several contexts of this process: their shards side by
    side.  For a per-pixel range, 'range' is the pair of maps (lo, hi), [npix] each, shards side by side.  masked_value: as in posterior_maps.  Raises when the contexts differ in sample count or registration."""
    return _build(HIST, "posterior_quantile_maps", _OneChain(ddata, engines), q=q, masked_value=masked_value)


BATCH_STATS = ("mean", "std", "mcse", "ess_bm", "split_rhat")


def moments_batches(dpar, ddata, planes=None, nbatch=16, batch_len=1, engines=None):
    """dangx_moments_batches on every context of this process, after moments_begin and before the first moments_accumulate;
    planes=None: default_hist_planes of the selection moments_begin made (every sampled index).  Returns the plane list."""
    return _register("moments_batches", dpar, ddata, engines, planes, default_hist_planes, _int_tuple, nbatch=nbatch, batch_len=batch_len)


def _batch_stats(info, first):
    """The statistics a chain with these batches carries after `first` are discarded: MCSE, ESS and split R-hat need two full
    batches, split R-hat two samples per half."""
    B = info["nfull"] - first
    out = ("mean", "std")
    if B >= 2:
        out += ("mcse", "ess_bm")
        if (B // 2) * info["batch_len"] >= 2:
            out += ("split_rhat",)
    return out


def _batch_first_check(who, info, first):
    """`first` leading batches can be discarded when they exist and a sample is left behind them"""
    if not 0 <= first <= info["nfull"]:
        raise DangxError("%s: first must be 0 .. %d full batches, not %d" % (who, info["nfull"], first))
    if first == info["nfull"] and info["partial"] == 0:
        raise DangxError("%s: first = %d discards every sample held (%d full batches, none in the open one)" % (who, first, info["nfull"]))


def posterior_batch_maps(ddata, first=0, ddof=0, masked_value=None, engines=None):
    """{(label, name, plane): {'mean', 'std', 'mcse', 'ess_bm', 'split_rhat', 'n', 'batch_len', 'nfull', 'partial', 'first'}} of
    the planes moments_batches registered, the first `first` batches discarded as burn-in; keys as posterior_quantile_maps'.  A
    statistic the batches held cannot give yet (fewer than two full ones after `first`) is left out.  Several contexts of this
    process: their shards side by side.  masked_value: as in posterior_maps."""
    return _build(BATCHES, "posterior_batch_maps", _OneChain(ddata, engines), first=first, ddof=ddof, masked_value=masked_value)


def default_signal_specs(dpar, component_list, bands):
    """[(l, band, kind), ...] for moments_signals: for every non-global component whose amplitude is sampled and that has at least
    one sampled index (without one its signal is a constant multiple of its amplitude), the signal at the band whose nu_c is
    nearest the component's nu_ref (the lowest band on ties) on every plane default_moment_selection selects for its amplitude,
    plus P (kind 3) when both Q and U are.  Component order, then kind.  Pure Python."""
    sel = default_moment_selection(dpar, component_list)
    specs = []
    for l, c in enumerate(component_list):
        if c.type in GLOBAL_TYPES or not c.sample_amplitude:
            continue
        if not any(j < len(c.sample_index) and c.sample_index[j] for j in range(c.nindices)):
            continue
        w = int(sel[l]) & 7
        if not w:
            continue
        ref = float(c.nu_ref) * (1e9 if float(c.nu_ref) < 1e7 else 1.0)       # Hz, the library's own rules (dangx_set_band / _set_component)
        dist = [abs(float(b.nu_c) * (1e9 if float(b.nu_c) < 1e9 else 1.0) - ref) for b in bands]
        band = dist.index(min(dist))
        kinds = [k for k in range(3) if (w >> k) & 1]
        if (w & 6) == 6:
            kinds.append(3)
        specs += [(l, band, k) for k in kinds]
    return specs


def moments_signals(dpar, ddata, specs=None, engines=None):
    """dangx_moments_signals on every context of this process, after moments_begin and before the first moments_accumulate;
    specs=None: default_signal_specs of the run.  Returns the spec list [(l, band, kind), ...]."""
    engs = _engines_of(ddata, engines)
    if specs is None:
        specs = default_signal_specs(dpar, engs[0].component_list, engs[0].bands)
    specs = [(int(l), int(j), L.SIGNAL_KINDS.index(k) if isinstance(k, str) else int(k)) for l, j, k in specs]
    for e in engs:
        e.moments_signals(specs)
    return specs


def posterior_signal_maps(ddata, ddof=0, masked_value=None, engines=None):
    """{(component label, band label, 'T' | 'Q' | 'U' | 'P'): {'mean', 'std', 'n'}} of the signals moments_signals registered, as
    host arrays [npix].  Several contexts of this process: their shards side by side.  masked_value: as in posterior_maps."""
    return _build(SIGNAL, "posterior_signal_maps", _OneChain(ddata, engines), ddof=ddof, masked_value=masked_value)


def default_angle_specs(dpar, component_list, bands):
    """[(l, band), ...] for moments_angles: one angle for every polarised intensity (l, band, P) of default_signal_specs -- the
    components whose Q and U amplitudes are both sampled and that have a sampled index, at the band nearest their nu_ref.
    Pure Python."""
    return [(l, band) for l, band, kind in default_signal_specs(dpar, component_list, bands) if kind == 3]


def moments_angles(dpar, ddata, specs=None, engines=None):
    """dangx_moments_angles on every context of this process, after moments_begin and before the first moments_accumulate;
    specs=None: default_angle_specs of the run.  Returns the spec list [(l, band), ...]."""
    engs = _engines_of(ddata, engines)
    if specs is None:
        specs = default_angle_specs(dpar, engs[0].component_list, engs[0].bands)
    specs = [(int(l), int(j)) for l, j in specs]
    for e in engs:
        e.moments_angles(specs)
    return specs


def posterior_angle_maps(ddata, masked_value=None, engines=None):
    """{(component label, band label): {'n', 'psi', 'psi_std', 'R'}} of the angles moments_angles registered, as host arrays
    [npix]: the circular mean of the polarisation angle psi = atan2(U, Q) / 2 in [-pi/2, pi/2] (the model's own Q, U: no sign
    convention is applied), its circular standard deviation in radians and the mean resultant length.  Several contexts of this
    process: their shards side by side.  masked_value: as in posterior_maps."""
    return _build(ANGLE, "posterior_angle_maps", _OneChain(ddata, engines), masked_value=masked_value)


def default_fit_specs(dpar, component_list, bands, nmaps=3):
    """[(what, band, plane), ...] for moments_fit: for every plane below `nmaps` named by a pol_flag of a CG group that samples a
    component (a group some component with sample_amplitude belongs to), the chi^2 map of the plane (1, -1, plane) and then the
    residual of every band (0, band, plane), bands ascending; planes ascending.  16 bytes per pixel and item: at full resolution
    register fewer.  Pure Python."""
    planes = 0
    for g in dpar.cg_groups:
        if any(c.sample_amplitude and c.cg_group == g.cg_group for c in component_list):
            for f in g.pol_flag:
                planes |= _flag_planes(f)
    specs = []
    for k in range(min(3, int(nmaps))):            # a flag that names a plane the model lacks adds nothing, as posterior_fit_gpu's loop over nmaps
        if (planes >> k) & 1:
            specs.append((1, -1, k))
            specs += [(0, j, k) for j in range(len(bands))]
    return specs


def moments_fit(dpar, ddata, specs=None, engines=None):
    """dangx_moments_fit on every context of this process, after moments_begin and before the first moments_accumulate;
    specs=None: default_fit_specs of the run.  'residual' / 'chisq' and 'T' / 'Q' / 'U' are accepted in specs.  Returns the spec
    list [(what, band, plane), ...]."""
    engs = _engines_of(ddata, engines)
    if specs is None:
        specs = default_fit_specs(dpar, engs[0].component_list, engs[0].bands, nmaps=engs[0].nmaps)
    specs = [_api.fit_spec(s) for s in specs]
    for e in engs:
        e.moments_fit(specs)
    return specs


def posterior_fit_maps(ddata, ddof=0, masked_value=None, engines=None):
    """{('residual', band label, 'T' | 'Q' | 'U') or ('chisq', 'T' | 'Q' | 'U'): {'mean', 'std', 'n'}} of the items moments_fit
    registered, as host arrays [npix] in the model's units (the residual of a band not divided by its unit conversion; a chi^2 map
    reads 0 at masked pixels).  Several contexts of this process: their shards side by side.  masked_value: as in posterior_maps.
    The std of the sky model at a band is the residual's std, its mean the (calibrated) data minus the residual's mean."""
    return _build(FIT, "posterior_fit_maps", _OneChain(ddata, engines), ddof=ddof, masked_value=masked_value)


# --------------------------------------------------------------------------- several chains: R-hat and pooled summaries
# dangx_chains_* (include/dangx.h): the accumulators of K chains of one device are combined on the device and only the map asked
# for is written.  `engines` below is one Engine per chain (the same shard of each); a "chain" of the map functions is a ddata
# or the list of that chain's shard engines in shard order.

def _chains_call(engines, fn, *args):
    engines = list(engines)
    arr, n = _ctx_array(engines)
    if getattr(engines[0].lib, fn)(arr, n, *args) != 0:
        raise DangxError(engines[0].lib.dangx_last_error(engines[0].h).decode())


def _chains_readout(engines, stem, shape, lead, device=False, out=None):
    """Engine._readout over the chains `engines`: `stem` or `stem`_dev with the leading arguments and the destination last.  The
    device form is asynchronous on the first chain's stream."""
    out, ptr = _readout_dest(engines[0], shape, device, out)
    _chains_call(engines, stem + "_dev" if device else stem, *lead, ptr)
    return out


def chains_get(engines, l, what, stat, ddof=0, device=False, out=None):
    """Over the chains `engines`: 'mean' / 0 = pooled mean, 'std' / 1 = pooled standard deviation sqrt(M / (N - ddof)), 'rhat' / 2 =
    Gelman-Rubin R-hat, 'W' / 3 = within-chain variance, 'B' / 4 = B/n, the variance of the chain means, 'ess' / 5 = the sum of the
    chains' AR(1) effective sample sizes, of component l's amplitude (what 0) or index j (what 1 + j) as [nmaps][npix].  R-hat, W
    and B need equal sample counts >= 2; NaN R-hat where no chain ever moved (a masked pixel).  device=True: a torch cuda tensor,
    written asynchronously on the first chain's stream (synchronize that engine, or use that stream, before reading it)."""
    e = engines[0]
    return _chains_readout(engines, "dangx_chains_get", (e.nmaps, e.npix), (int(l), int(what), _code(L.CHAINS_STAT_CODES, stat), int(ddof)), device, out)


def chains_get_template(engines, l, stat, ddof=0, out=None):
    """chains_get's statistics of the rows of c%template_amplitudes of a template / monopole / hi_fit member, [nmaps][nbands]."""
    e = engines[0]
    return _chains_readout(engines, "dangx_chains_get_template", (e.nmaps, e.nbands), (int(l), _code(L.CHAINS_STAT_CODES, stat), int(ddof)), out=out)


def chains_get_signal(engines, s, stat, ddof=0, device=False, out=None):
    """chains_get's statistics 'mean', 'std', 'rhat', 'W', 'B' of registered signal s (the same registration in every chain), [npix]."""
    return _chains_readout(engines, "dangx_chains_get_signal", (engines[0].npix,), (int(s), _code(L.CHAINS_STAT_CODES, stat), int(ddof)), device, out)


def chains_get_fit(engines, i, stat, ddof=0, device=False, out=None):
    """chains_get's statistics 'mean', 'std', 'rhat', 'W', 'B' of registered fit item i (the same registration in every chain), [npix]."""
    return _chains_readout(engines, "dangx_chains_get_fit", (engines[0].npix,), (int(i), _code(L.CHAINS_STAT_CODES, stat), int(ddof)), device, out)


def chains_get_angle(engines, a, stat, device=False, out=None):
    """Engine.moments_get_angle's statistics of registered angle a (the same registration in every chain) on the chains' (Cbar,
    Sbar) pooled by their sample counts -- unequal counts allowed -- and 'between' / 5: the circular standard deviation of the
    chains' mean directions, to set beside 'psi_std' (there is no standard circular R-hat); [npix]."""
    return _chains_readout(engines, "dangx_chains_get_angle", (engines[0].npix,), (int(a), _code(L.ANGLE_STAT_CODES, stat)), device, out)


def chains_get_pair(engines, p, stat, ddof=0, device=False, out=None):
    """Pooled covariance ('cov' / 0: C / (N - ddof)) or correlation ('corr' / 1) of registered pair p over the chains, [npix]."""
    return _chains_readout(engines, "dangx_chains_get_pair", (engines[0].npix,), (int(p), _code(L.PAIR_STAT_CODES, stat), int(ddof)), device, out)


def chains_hist_stat(engines, reg, stat, q=None, device=False, out=None):
    """Engine.moments_hist_stat on the bins of all chains summed: 'quantile' / 0 -> [nq][npix], 'mode' / 1, 'n' / 2 -> [npix]."""
    shape, lead = _hist_stat_args("chains_hist_stat", engines[0].npix, reg, stat, q)
    return _chains_readout(engines, "dangx_chains_hist_stat", shape, lead, device, out)


def chains_hist_rank(engines, reg, stat, device=False, out=None):
    """Rank-normalised R-hat (Vehtari et al. 2021) of histogram registration reg over the chains `engines`, read from their
    records: 'bulk' / 0 = rank-normalised, 'folded' / 1 = of the fold around the pooled median bin (chains that differ in spread),
    'max' / 2 = the larger of the two, the number to report; [npix].  The samples of a bin are ties, so this is the statistic of
    the binned trace.  NaN where the chains hold different numbers of counted samples in a pixel, fewer than 2, or one bin only.
    Not split: drift inside a chain is 'split_rhat' of moments_batches."""
    return _chains_readout(engines, "dangx_chains_hist_rank", (engines[0].npix,), (int(reg), _code(L.RANK_STAT_CODES, stat)), device, out)


def open_chain(dpar, ddata, seed, stream=None, tcmb=None):
    """A further chain over the same data: (dpar_k, ddata_k).  dpar_k is a copy of dpar with its own seed.  ddata_k shares ddata's
    sig_map / rms_map / masks objects -- for device tensors its Engine adopts the same HBM, host arrays are uploaded once more --
    and carries a new Engine (ddata_k.engine) on the same pix0 / npix_global / device that owns deep copies of the component state
    as ddata.engine's component_list holds it.  Starting values are the caller's: put them into ddata_k.engine afterwards
    (put_amplitude / put_indices), dispersed for R-hat to mean something."""
    import copy
    import dataclasses
    src = ddata.engine
    if src is None:
        raise DangxError("open_chain: ddata has no engine (call initialize first)")
    dpar_k = copy.copy(dpar)
    dpar_k.seed = int(seed)
    ddata_k = dataclasses.replace(ddata, engine=None, sky_model=None, res_map=None, chi_map=None,
                                  gain=None if ddata.gain is None else np.array(ddata.gain, dtype=np.float64),
                                  offset=None if ddata.offset is None else np.array(ddata.offset, dtype=np.float64))
    comps = copy.deepcopy(src.component_list)
    ddata_k.engine = Engine(src.bands, comps, ddata_k, npix_global=src.npix_global, pix0=src.pix0, device=src._device, stream=stream,
                            tcmb=tcmb)
    return dpar_k, ddata_k


def _chain_engines(chain):
    return [chain.engine] if hasattr(chain, "engine") else list(chain)


def _chains_shards(chains, who):
    """[[chain 0's engine of shard s, chain 1's, ...] for every shard s] and the per-chain sample counts."""
    chs = [_chain_engines(c) for c in chains]
    if not 2 <= len(chs) <= L.MAX_CHAINS:
        raise DangxError("%s: takes 2 to %d chains, not %d" % (who, L.MAX_CHAINS, len(chs)))
    if len({len(c) for c in chs}) != 1:
        raise DangxError("%s: the chains hold different numbers of shards %s" % (who, [len(c) for c in chs]))
    counts = []
    for k, c in enumerate(chs):
        ns = {e.moments_count() for e in c}
        if len(ns) != 1:
            raise DangxError("%s: the contexts of chain %d hold different sample counts %s" % (who, k, sorted(ns)))
        counts.append(ns.pop())
    return [list(col) for col in zip(*chs)], counts


# --------------------------------------------------------------------------- sources, families and the one map builder

class _Here:
    """A source whose chains all live in this process: nothing to fetch, the maps are made here."""
    here = True

    def fetch(self, sections):
        pass

    def batches_info(self):
        return self.shards[0][0].moments_batches_info()

    def finish(self, out):
        return out


class _OneChain(_Here):
    """One chain of this process as the posterior_*_maps read it: its shard engines, one to a column.  `counts` is set by the
    count check of the families that make one (_build)."""
    pooled = False

    def __init__(self, ddata, engines=None):
        self.shards, self.counts = [[e] for e in _engines_of(ddata, engines)], None


class _LocalChains(_Here):
    """The chains of this process as the chains_*_maps read them."""
    pooled = True

    def __init__(self, chains, who):
        self.shards, self.counts = _chains_shards(chains, who)


def _source(chains, who):
    """what a *_maps call reads its chains through: one chain, a list of chains of this process, or dist_chains' object"""
    if isinstance(chains, _OneChain):
        return chains
    if isinstance(chains, DistChains):
        chains.begin(who)
        return chains
    return _LocalChains(chains, who)


@dataclass(frozen=True)
class _Family:
    """One kind of summary, for its single-chain (posterior_*_maps) and several-chain (chains_*_maps) form."""
    reg: str                        # the registration it reads: mirror attribute _moment_<reg> (api.MOMENT_ATTRS)
    call: str                       # ... and the call that makes it, named in "<call> was not called"
    noun: Optional[str]             # "the contexts hold different <noun> registrations"
    single: Optional[str]           # the thin getter of one chain: an Engine method, called on the shard's engine
    chains: str                     # ... of several: a chains_* function, looked up as an attribute of dang_amd.api when called
    checks: Tuple[tuple, tuple]     # the checks of the single-chain and of the several-chain form, in their order (_build)
    items: Callable                 # (first engine, registration) -> the registered items
    key: Callable                   # (first engine, item) -> the item's key in the result
    sections: Callable              # (item, statistics) -> [(family, a, b, with lag-1 parts), ...] the read-outs need, its own first
    stats: Callable                 # (source, options) -> [(name in the entry, statistic), ...] available
    args: Callable                  # (item, statistic, options) -> the getters' arguments after the engine(s)
    head: Callable                  # (source, registration, item, options) -> the entry before its maps; None: the entry IS the one map
    rows: Callable = lambda e0, item: False     # the item is a template's [nmaps][nbands] rows: <getter>_template without `what`
    own: Optional[Callable] = None              # item -> the sections the item owns; None: the first of `sections`


def _named(stats):
    return [(s, s) for s in stats]


def _plane_key(e0, l, what, *plane):
    return (e0.component_list[l].label, _plane_name(e0.component_list[l], what)) + plane


def _count_head(src, *_):
    if not src.pooled:
        return {"n": src.counts[0]}
    return {"n": src.counts[0] if len(set(src.counts)) == 1 else list(src.counts), "nchains": len(src.counts)}


def _plane_stats(src, o):
    if not src.pooled:
        return _named(("mean", "std") + (("rho1", "ess") if _registration(src.shards[0][0], "lag1") else ()))
    return _named(_chains_stats(src.counts, all(_registration(e, "lag1") for col in src.shards for e in col)))


def _hist_kind(reg, r):
    """'global' or 'pixel': the range kind of registration r in the mirror `reg` (a mirror without kinds: global ranges)"""
    kinds = reg.get("kinds")
    return kinds[r] if kinds else "global"


def _hist_range(src, reg, r, fetched):
    """a registration's 'range': its two numbers, or for a per-pixel range the pair of maps, shards side by side -- read from the
    first chain of each shard that has accumulators of its own (every chain holds the same maps).  A shard whose chains are all
    holders: its first holder, when the family's statistics had HIST_RANGE fetched into it (`fetched`); otherwise nobody on this
    side holds the maps -- the rank R-hat needs none and moves none -- and 'range' is None."""
    if _hist_kind(reg, r) != "pixel":
        return reg["ranges"][r]
    owners = [next((e for e in col if not getattr(e, "_moment_holder", False)), col[0] if fetched else None) for col in src.shards]
    if any(e is None for e in owners):
        return None
    parts = [e.moments_hist_range_get(r) for e in owners]
    return tuple(np.concatenate([p[i] for p in parts]) for i in (0, 1))


def _hist_key(e0, it):
    """a state plane as posterior_maps names it plus the plane; a signal source as posterior_signal_maps keys it"""
    l, what, k = it[1]
    if what == L.HIST_SIGNAL:
        c, band, kind = _registration(e0, "signals", "a histogram of a signal", "moments_signals")[l]
        return (e0.component_list[c].label, e0.bands[band].label, L.SIGNAL_KINDS[kind])
    return _plane_key(e0, l, what, k)


_RANGE_STATS = ("quantile", "mode")      # the histogram statistics that need range values; N and the rank R-hat do not


def _hist_sections(it, stats):
    """HIST, and for a per-pixel range HIST_RANGE where a statistic needs its values (no statistics named: every section owned)"""
    secs = [(L.SEC_HIST, it[0], 0, False)]
    if it[2] == "pixel" and (not stats or any(s in _RANGE_STATS for s in stats)):
        secs.append((L.SEC_HIST_RANGE, it[0], 0, False))
    return secs


def _hist_family(chains, checks, stats, args, ranged):
    return _Family("hist", "moments_hist", "histogram", "moments_hist_stat", chains, checks,
                   items=lambda e0, reg: [(r, p, _hist_kind(reg, r)) for r, p in enumerate(reg["planes"])], key=_hist_key,
                   sections=_hist_sections, stats=lambda src, o: stats, args=args,
                   head=lambda src, reg, it, o: {"range": _hist_range(src, reg, it[0], ranged), "nbins": reg["nbins"]},
                   own=lambda it: _hist_sections(it, ()))


_REGISTERED, _SAME = ("registered",), ("registered", "same")
PLANES = _Family("sel", "moments_begin", None, "moments_get", "chains_get", (("counts", "registered"), _REGISTERED),
                 items=lambda e0, sel: [(l, what) for l, c in enumerate(e0.component_list) for what in range(1 + c.nindices)
                                        if (int(sel[l]) >> (0 if what == 0 else 3 + 3 * (what - 1))) & 7],
                 key=lambda e0, it: _plane_key(e0, *it), sections=lambda it, stats: [(L.SEC_PLANES, it[0], it[1], "ess" in stats)],
                 stats=_plane_stats, args=lambda it, stat, o: (it[0], it[1], stat, o["ddof"]), head=_count_head,
                 rows=lambda e0, it: it[1] == 0 and e0.component_list[it[0]].type in GLOBAL_TYPES)
PAIR = _Family("pairs", "moments_pairs", None, "moments_get_pair", "chains_get_pair", (_REGISTERED, _REGISTERED),
               items=lambda e0, pairs: list(enumerate(pairs)), key=lambda e0, it: tuple(_plane_key(e0, *plane) for plane in it[1]),
               sections=lambda it, stats: [(L.SEC_PAIR, it[0], 0, False)] + sorted({(L.SEC_PLANES, l, what, False) for l, what, _ in it[1]}),
               stats=lambda src, o: [(None, o["stat"])], args=lambda it, stat, o: (it[0], stat, o["ddof"]), head=lambda *_: None)
HIST = _hist_family("chains_hist_stat", (_SAME + ("counts",), _SAME), [("q", "quantile"), ("mode", "mode"), ("n", "n")],
                    lambda it, stat, o: (it[0], stat, o["q"] if stat == "quantile" else None), ranged=True)
RANK = _hist_family("chains_hist_rank", ((), _SAME), [("rhat_rank", "bulk"), ("rhat_folded", "folded"), ("rhat_max", "max")],
                    lambda it, stat, o: (it[0], stat), ranged=False)
BATCHES = _Family("batches", "moments_batches", "batch", "moments_batches_get", "chains_batches_get",
                  (_SAME + ("counts", "first"), _SAME + ("equal", "first")),
                  items=lambda e0, reg: list(enumerate(reg["planes"])), key=lambda e0, it: _plane_key(e0, *it[1]),
                  sections=lambda it, stats: [(L.SEC_BATCHES, it[0], 0, False)], stats=lambda src, o: _named(_batch_stats(o["info"], o["first"])),
                  args=lambda it, stat, o: (it[0], stat, o["first"], o["ddof"]),
                  head=lambda src, reg, it, o: dict(o["info"], **_count_head(src), first=int(o["first"])))
SIGNAL = _Family("signals", "moments_signals", "signal", "moments_get_signal", "chains_get_signal", (_SAME + ("counts",), _SAME),
                 items=lambda e0, specs: list(enumerate(specs)),
                 key=lambda e0, it: (e0.component_list[it[1][0]].label, e0.bands[it[1][1]].label, L.SIGNAL_KINDS[it[1][2]]),
                 sections=lambda it, stats: [(L.SEC_SIGNAL, it[0], 0, False)],
                 stats=lambda src, o: _named(_chains_stats(src.counts, False) if src.pooled else ("mean", "std")),
                 args=lambda it, stat, o: (it[0], stat, o["ddof"]), head=_count_head)
ANGLE = _Family("angles", "moments_angles", "angle", "moments_get_angle", "chains_get_angle", (_SAME + ("counts",), _SAME),
                items=lambda e0, specs: list(enumerate(specs)),
                key=lambda e0, it: (e0.component_list[it[1][0]].label, e0.bands[it[1][1]].label),
                sections=lambda it, stats: [(L.SEC_ANGLE, it[0], 0, False)],
                stats=lambda src, o: _named(("psi", "psi_std", "R") + (("between",) if src.pooled else ())),
                args=lambda it, stat, o: (it[0], stat), head=_count_head)
def _fit_key(e0, it):
    what, band, plane = it[1]
    if what == 1:
        return ("chisq", L.SIGNAL_KINDS[plane])
    return ("residual", e0.bands[band].label, L.SIGNAL_KINDS[plane])


FIT = _Family("fit", "moments_fit", "fit", "moments_get_fit", "chains_get_fit", (_SAME + ("counts",), _SAME),
              items=lambda e0, specs: list(enumerate(specs)), key=_fit_key,
              sections=lambda it, stats: [(L.SEC_FIT, it[0], 0, False)],
              stats=lambda src, o: _named(_chains_stats(src.counts, False) if src.pooled else ("mean", "std")),
              args=lambda it, stat, o: (it[0], stat, o["ddof"]), head=_count_head)
FAMILIES = {"planes": PLANES, "pair": PAIR, "hist": HIST, "rank": RANK, "batches": BATCHES, "signal": SIGNAL, "angle": ANGLE, "fit": FIT}


def own_sections(e):
    """Engine.moments_sections: the section every registered item of engine e owns, in the order moments_save writes them"""
    out = []
    for fam in (PLANES, PAIR, HIST, SIGNAL, BATCHES, ANGLE, FIT):
        reg = _registration(e, fam.reg, None, fam.call if fam is PLANES else None)
        if reg is not None:
            for item in fam.items(e, reg):
                out += [s[:3] for s in (fam.own(item) if fam.own else fam.sections(item, ())[:1])]
    return out


def _build(fam, who, chains, masked_value=None, **o):
    """{key: entry} of every registered item of family `fam` for the public function `who`: its checks, then per item the
    sections fetched into the source, and (where the maps are made) per statistic the shards side by side, the pixels masked in
    a shard's ddata.masks plane 1 set to masked_value.  `o`: the options the family's getters take (ddof, stat, q, first)."""
    src = _source(chains, who)
    e0, everyone, reg = src.shards[0][0], [e for col in src.shards for e in col], None
    for check in fam.checks[src.pooled]:
        if check == "registered":
            reg = _registration(e0, fam.reg, who, fam.call)
        elif check == "same" and any(_registration(e, fam.reg) != reg for e in everyone):
            raise DangxError("%s: the contexts hold different %s registrations" % (who, fam.noun))
        elif check == "counts":                          # of one chain: its contexts hold the same number of samples
            ns = {e.moments_count() for e in everyone}
            if len(ns) != 1:
                raise DangxError("%s: the contexts hold different sample counts %s" % (who, sorted(ns)))
            src.counts = [ns.pop()]
        elif check == "equal" and len(set(src.counts)) != 1:
            raise DangxError("%s: the chains hold different sample counts %s" % (who, list(src.counts)))
        elif check == "first":
            o["info"] = src.batches_info()
            _batch_first_check(who, o["info"], o["first"])
    if src.pooled:
        # through dang_amd.api, where these names have always been replaced by stand-ins; it hands back this module's own otherwise
        # (a name outside __all__, which api does not carry, is taken here)
        get = lambda col, suffix, args: (getattr(_api, fam.chains + suffix, None) or globals()[fam.chains + suffix])(col, *args)
    else:
        get = lambda col, suffix, args: getattr(col[0], fam.single + suffix)(*args)
    stats = fam.stats(src, o)
    out = {}
    for item in fam.items(e0, reg):
        key = fam.key(e0, item)
        src.fetch(fam.sections(item, [stat for _, stat in stats]))
        if not src.here:
            continue
        entry = fam.head(src, reg, item, o)
        for name, stat in stats:
            args = fam.args(item, stat, o)
            if fam.rows(e0, item):                       # the first shard's: the rows are the same in all, and no pixels to fill
                m = get(src.shards[0], "_template", args[:1] + args[2:])
            else:
                parts = []
                for col in src.shards:
                    part = get(col, "", args)
                    parts.append(_mask_fill(part, col[0].ddata.masks, masked_value) if masked_value is not None else part)
                m = np.concatenate(parts, axis=-1) if len(parts) > 1 else parts[0]
            if entry is None:
                entry = m
            else:
                entry[name] = m
        out[key] = entry
    return src.finish(out)


def _chains_stats(counts, lag1):
    """The statistics a set of chains with these counts carries: R-hat, W and B only for equal counts >= 2."""
    equal = len(set(counts)) == 1 and counts[0] >= 2
    return ("mean", "std") + (("rhat", "W", "B") if equal else ()) + (("ess",) if lag1 else ())


def chains_posterior_maps(chains, ddof=0, masked_value=None):
    """posterior_maps over several chains (each a ddata, or the list of that chain's shard engines in shard order): the same keys,
    every entry {'n', 'nchains', 'mean', 'std', 'rhat', 'W', 'B'} (+ 'ess' when every chain tracks lag-1) with the pooled mean and
    standard deviation, R-hat, the within-chain variance and B/n of chains_get.  'n' is the samples per chain -- a list, and no
    'rhat' / 'W' / 'B', when the chains hold different counts.  Shards side by side; masked_value as in posterior_maps."""
    return _build(PLANES, "chains_posterior_maps", chains, ddof=ddof, masked_value=masked_value)


def chains_pair_maps(chains, stat="corr", ddof=0, masked_value=None):
    """posterior_pair_maps over several chains: the pooled correlation ('corr') or covariance ('cov', with ddof) of every pair."""
    return _build(PAIR, "chains_pair_maps", chains, stat=stat, ddof=ddof, masked_value=masked_value)


def chains_quantile_maps(chains, q=(0.16, 0.5, 0.84), masked_value=None):
    """posterior_quantile_maps over several chains: 'q', 'mode' and 'n' of the bins of all chains summed (+ 'range', 'nbins')."""
    return _build(HIST, "chains_quantile_maps", chains, q=q, masked_value=masked_value)


def chains_rank_maps(chains, masked_value=None):
    """The rank-normalised R-hat of every registered histogram plane over several chains: {'rhat_rank', 'rhat_folded', 'rhat_max',
    'range', 'nbins'} per plane (chains_hist_rank's 'bulk', 'folded' and 'max').  Shards side by side; masked_value as in
    posterior_maps.  The statistic needs no range values, so a per-pixel range's maps are not moved for it: 'range' is then the
    pair of maps where a chain with accumulators of its own is at hand in every shard, and None where all are holders."""
    return _build(RANK, "chains_rank_maps", chains, masked_value=masked_value)


def chains_batches_get(engines, reg, stat, first=0, ddof=0, device=False, out=None):
    """Engine.moments_batches_get over the chains `engines` (the same registration, batch length and count in each): 'mean' /
    'std' pooled over chains and batches first.., 'mcse' = sqrt(sum MCSE_k^2) / K, 'ess_bm' = sum ESS_k, 'split_rhat' over the 2K
    half-chains, as [npix].  device=True: written asynchronously on the first chain's stream."""
    return _chains_readout(engines, "dangx_chains_batches_get", (engines[0].npix,), (int(reg), _code(L.BATCH_STAT_CODES, stat), int(first), int(ddof)),
                           device, out)


def chains_batch_maps(chains, first=0, ddof=0, masked_value=None):
    """posterior_batch_maps over several chains: the same keys, every entry with chains_batches_get's statistics + 'n' (samples per
    chain), 'nchains', 'batch_len', 'nfull', 'partial', 'first'.  Every chain must hold the same registration and batch state."""
    return _build(BATCHES, "chains_batch_maps", chains, first=first, ddof=ddof, masked_value=masked_value)


def chains_angle_maps(chains, masked_value=None):
    """posterior_angle_maps over several chains (or dist_chains' object): {'n', 'nchains', 'psi', 'psi_std', 'R', 'between'} per
    registered angle -- the first three of the pooled (Cbar, Sbar), 'between' the circular std of the chains' mean directions."""
    return _build(ANGLE, "chains_angle_maps", chains, masked_value=masked_value)


def chains_fit_maps(chains, ddof=0, masked_value=None):
    """posterior_fit_maps over several chains (or dist_chains' object): {'n', 'nchains', 'mean', 'std', 'rhat', 'W', 'B'} per
    registered fit item."""
    return _build(FIT, "chains_fit_maps", chains, ddof=ddof, masked_value=masked_value)


def chains_signal_maps(chains, ddof=0, masked_value=None):
    """posterior_signal_maps over several chains: {'n', 'nchains', 'mean', 'std', 'rhat', 'W', 'B'} per registered signal."""
    return _build(SIGNAL, "chains_signal_maps", chains, ddof=ddof, masked_value=masked_value)


# --------------------------------------------------------------------------- chains in other processes, save / restore
# Both are thin layers over the sections of the accumulator state (Engine.moments_section_*, include/dangx.h): a chain that ran in
# another process reaches the chains_* read-outs as a HOLDER on this device (Engine.moments_begin_like) given the few sections a
# read-out needs, so the read-outs stay the one implementation they are and give bit for bit what the same chains give inside
# one process; a saved run is HEAD plus every section, streamed one at a time.

_HEAD_STRUCT = struct.Struct("<IIqiiqiiqQ6Q")
_HEAD_GROUPS = ("the shard (npix, pix0 or nmaps)", "the selection (selection words, type or nindices of a selected component)",
                "the pair list", "the histogram registrations (planes, lo / hi range, nbins or bits)", "the fit items, signal or angle registrations",
                "the batch registrations (planes)")


def head_unpack(raw):
    """The fields of a HEAD section (include/dangx.h) as a dict; `raw`: its DANGX_SECTION_HEAD_BYTES bytes."""
    raw = bytes(raw)
    if len(raw) != L.SECTION_HEAD_BYTES:
        raise DangxError("a HEAD section is %d bytes, not %d (truncated or foreign)" % (L.SECTION_HEAD_BYTES, len(raw)))
    v = _HEAD_STRUCT.unpack(raw)
    if v[0] != 0x48535844:
        raise DangxError("not a HEAD section (foreign bytes: the magic word is missing)")
    return {"version": v[1], "count": v[2], "lag1": v[3], "nbatch": v[4], "batch_len": v[5], "nfull": v[6], "partial": v[8],
            "fingerprint": v[9], "groups": tuple(v[10:16])}


def head_diff(got, own):
    """'' when two unpacked HEADs describe the same registration, else what differs (dx_section_head_diff's words)"""
    why = []
    if got["lag1"] != own["lag1"]:
        why.append("lag-1 is tracked there and missing here" if got["lag1"] else "lag-1 is missing there and tracked here")
    if got["nbatch"] != own["nbatch"]:
        why.append("nbatch is %d there and %d here" % (got["nbatch"], own["nbatch"]))
    for i, name in enumerate(_HEAD_GROUPS):
        if got["groups"][i] == own["groups"][i] or (i == 2 and got["lag1"] != own["lag1"]) or (i == 5 and got["nbatch"] != own["nbatch"]):
            continue
        why.append(name + " differ")
    if not why and got["fingerprint"] != own["fingerprint"]:
        why.append("the fingerprints differ")
    return "; ".join(why)


def dist_verdict(metas):
    """What every rank concludes from the gathered metadata of dist_chains, metas[r] = {'error': str or None, 'heads': [chain]
    [shard] HEAD bytes, 'shape': [chain][shard] (pix0, npix)} of rank r: (error message or None, the chains in global order as
    (rank, local index), their sample counts).  A pure function of its argument: every rank reaches the same verdict."""
    for r, m in enumerate(metas):
        if m.get("error"):
            return "rank %d: %s" % (r, m["error"]), [], []
    order = [(r, i) for r, m in enumerate(metas) for i in range(len(m["heads"]))]
    if not 2 <= len(order) <= L.MAX_CHAINS:
        return "takes 2 to %d chains in all, not %d" % (L.MAX_CHAINS, len(order)), [], []
    nsh = {len(metas[r]["heads"][i]) for r, i in order}
    if len(nsh) != 1:
        return "the chains hold different numbers of shards %s" % sorted(nsh), [], []
    r0, i0 = order[0]
    counts = []
    for r, i in order:
        who = "rank %d chain %d" % (r, i)
        heads = [head_unpack(h) for h in metas[r]["heads"][i]]
        for s, h in enumerate(heads):
            if tuple(metas[r]["shape"][i][s]) != tuple(metas[r0]["shape"][i0][s]):
                return "%s shard %d holds pixels %s, the first chain %s: the ranks of one group must hold the same pixel range" % (
                    who, s, tuple(metas[r]["shape"][i][s]), tuple(metas[r0]["shape"][i0][s])), [], []
            why = head_diff(h, head_unpack(metas[r0]["heads"][i0][s]))
            if why:
                return "%s shard %d is registered differently from the first chain: %s" % (who, s, why), [], []
        ns = {h["count"] for h in heads}
        if len(ns) != 1:
            return "the contexts of %s hold different sample counts %s" % (who, sorted(ns)), [], []
        if heads[0]["count"] == 0:
            return "%s: no sample accumulated" % who, [], []
        counts.append(heads[0]["count"])
    return None, order, counts


class DistChains:
    """dist_chains' object: the chains of every rank of a process group, which the chains_*_maps take in place of a list."""
    pooled = True

    def __init__(self, chains, group=None, dst=0):
        import torch.distributed as td
        if not (td.is_available() and td.is_initialized()):
            raise DangxError("dist_chains: torch.distributed is not initialised")
        self.local = [_chain_engines(c) for c in chains]          # [local chain][shard]
        self.group, self.dst = group, dst
        self.rank, self.nranks = td.get_rank(group), td.get_world_size(group)
        if dst is not None and not 0 <= int(dst) < self.nranks:
            raise DangxError("dist_chains: dst must be a rank of the group (0..%d) or None" % (self.nranks - 1))
        self.here = dst is None or self.rank == int(dst)
        self._holders = {}                                       # (rank, local index) -> [holder Engine per shard]
        self.peak_held = 0                                       # most device bytes the holders held at once during the last call
        self.fetched = []                                        # the sections the last call moved, in order
        self.begin("dist_chains")

    def _meta(self):
        try:
            return {"error": None,
                    "heads": [[bytes(e.moments_section_get(L.SEC_HEAD)) for e in ch] for ch in self.local],
                    "shape": [[(e.pix0, e.npix) for e in ch] for ch in self.local]}
        except (DangxError, AssertionError) as ex:
            return {"error": str(ex) or type(ex).__name__, "heads": [], "shape": []}

    def begin(self, who):
        """The one all_gather of metadata in front of every call: shard ranges, HEADs (fingerprint, counts, batch state) and the
        number of local chains.  Every rank reaches the same verdict, so a mismatch raises on every rank before a section moves."""
        import torch.distributed as td
        metas = [None] * self.nranks
        td.all_gather_object(metas, self._meta(), group=self.group)
        err, self.order, self.counts = dist_verdict(metas)
        if err:
            raise DangxError("%s: %s" % (who, err))
        self.heads = {(r, i): metas[r]["heads"][i] for r, i in self.order}
        self.nlocal = [len(m["heads"]) for m in metas]
        self.peak_held, self.fetched = 0, []
        nsh = len(self.local[0]) if self.local else len(next(iter(self.heads.values())))
        if self.here and not self.local:
            raise DangxError("%s: the rank that makes the maps must hold a chain of its own (the model of the holders is taken from it)" % who)
        cols = []
        for s in range(nsh):
            col = []
            for r, i in (self.order if self.here else [(self.rank, j) for j in range(len(self.local))]):
                if r == self.rank:
                    col.append(self.local[i][s])
                else:
                    hs = self._holders.setdefault((r, i), [])
                    while len(hs) <= s:                           # a holder from its first moment: it carries the registration
                        hs.append(_api._holder_engine(self.local[0][len(hs)]))      # through the module: tests replace it there
                        hs[-1].moments_begin_like(self.local[0][len(hs) - 1])
                    col.append(hs[s])
            cols.append(col)
        self.shards = cols
        if not self.here:
            self.counts = list(self.counts)

    def batches_info(self):
        h = head_unpack(self.heads[self.order[0]][0])
        if h["nbatch"] == 0:
            raise DangxError("no batches are registered (moments_batches was not called)")
        return {"batch_len": h["batch_len"], "nfull": h["nfull"], "partial": h["partial"]}

    def _payload(self, e, f, a, b, lag):
        """this rank's bytes of a section: a device tensor under nccl, a host tensor under gloo (staged through the host form)"""
        import torch
        import torch.distributed as td
        if td.get_backend(self.group) == "nccl":
            t = e.moments_section_get(f, a, b, device=True)
            e.synchronize()
        else:
            t = torch.from_numpy(e.moments_section_get(f, a, b))
        pixel_planes = f == L.SEC_PLANES and not (b == 0 and e.component_list[a].type in GLOBAL_TYPES)
        if pixel_planes and _registration(e, "lag1") and not lag:
            t = t[:t.numel() * L.PLANES_MOMENT_PARTS // L.PLANES_LAG1_PARTS]      # mean and m2 come first
        return t

    def fetch(self, sections):
        """Collective: the sections [(family, a, b, with lag-1 parts), ...] of every chain reach the holders on the ranks that make
        the maps.  What the holders held before is dropped first: they never hold more than one call's sections."""
        import torch
        import torch.distributed as td
        nccl = td.get_backend(self.group) == "nccl"
        rows = max(self.nlocal)
        remote = [(r, i) for r, i in self.order if r != self.rank]
        for s in range(len(self.shards)):
            if self.here:
                for key in remote:
                    h = self._holders[key][s]
                    h.moments_begin_like(self.local[0][s])
                    h.moments_section_put(L.SEC_HEAD, 0, 0, np.frombuffer(self.heads[key][s], dtype=np.uint8).copy())
            keep = []
            for f, a, b, lag in sections:
                mine = [self._payload(ch[s], f, a, b, lag) for ch in self.local]
                send = torch.stack(mine + [torch.zeros_like(mine[0])] * (rows - len(mine))).contiguous()
                parts = _dist.gather_equal(send, self.group, self.dst)
                self.fetched.append((s, f, a, b, bool(lag)))
                if not self.here:
                    continue
                if nccl:
                    torch.cuda.current_stream().synchronize()     # the gathered bytes exist before a holder's stream copies them
                for r, i in remote:
                    self._holders[(r, i)][s].moments_section_put(f, a, b, parts[r][i] if nccl else parts[r][i].numpy())
                keep.append(parts)
            if self.here:
                for key in remote:
                    self._holders[key][s].synchronize()           # the copies out of `keep` are over
                held = sum(h.moments_held_bytes() for hs in self._holders.values() for h in hs)
                self.peak_held = max(self.peak_held, held)

    def finish(self, out):
        for key, hs in self._holders.items():                    # nothing stays held between calls
            for s, h in enumerate(hs):
                h.moments_begin_like(self.local[0][s])
        return out if self.here else None


def dist_chains(chains, group=None, dst=0):
    """The chains of every rank of `group` (None: the default process group) as ONE set: every rank passes its local chain or
    chains (each a ddata, or the list of that chain's shard engines), and the object returned is accepted by chains_posterior_maps,
    chains_pair_maps, chains_quantile_maps, chains_rank_maps, chains_batch_maps, chains_signal_maps and chains_angle_maps in place of the list.  Those
    calls are then collective -- every rank of the group makes the same call -- and return the maps on rank `dst` of the group and
    None elsewhere; dst=None: on every rank.  The chain order is rank order, and list order within a rank; 2 to 8 chains in all.
    The ranks of one group hold the same pixel range (a sharded run makes one group per shard).  A rank whose registration, shard
    or chain count does not fit raises DangxError on EVERY rank before anything moves.  For each map only the sections it needs
    travel (mean and m2 of a plane; the lag-1 parts for 'ess' only; one histogram or batch registration at a time), as device
    tensors under nccl and through the host under gloo, into holders (Engine.moments_begin_like) beside the local chains."""
    return DistChains(chains, group=group, dst=dst)


_SAVE_MAGIC = b"DANGXSEC"
_SAVE_HEAD = struct.Struct("<8sIIqq")            # magic, format version, number of sections, pix0, npix
_SAVE_ENTRY = struct.Struct("<iiiiqq")           # family, a, b, reserved, offset of the payload in the file, its bytes


def _save_paths(path, engines):
    return [path] if len(engines) == 1 else ["%s.%d" % (path, s) for s in range(len(engines))]


def moments_save(ddata, path, engines=None):
    """Write the accumulator state of every shard engine to `path` (several shards: path.0, path.1, ...): one self-describing file
    per shard -- a fixed header, an index of (family, a, b, offset, bytes), then the raw section payloads (include/dangx.h), HEAD
    first.  Sections are streamed one at a time: host memory is one section.  Together with the chain state this resumes a run:

        # save                                             # restore, in a fresh process
        state = ddata.engine.pull_state()                  initialize(...); moments_begin / _pairs / _hist / _signals / _batches as before
        np.savez(p + ".chain", it=it, **state arrays)      put_amplitude / put_indices / put_template_amplitudes of the saved state
        da.moments_save(ddata, p + ".moments")             da.moments_load(ddata, p + ".moments"); continue at iteration it + 1

    (the random streams are keyed by seed, iteration and global pixel, so the resumed chain is the uninterrupted one)."""
    engines = _engines_of(ddata, engines)
    for e, fn in zip(engines, _save_paths(path, engines)):
        secs = [(L.SEC_HEAD, 0, 0)] + e.moments_sections()
        sizes = [e.moments_section_bytes(*s) for s in secs]
        off = _SAVE_HEAD.size + _SAVE_ENTRY.size * len(secs)
        tmp = fn + ".tmp"
        with open(tmp, "wb") as f:
            f.write(_SAVE_HEAD.pack(_SAVE_MAGIC, 1, len(secs), e.pix0, e.npix))
            for (fam, a, b), n in zip(secs, sizes):
                f.write(_SAVE_ENTRY.pack(fam, a, b, 0, off, n))
                off += n
            for (fam, a, b), n in zip(secs, sizes):
                f.write(memoryview(np.ascontiguousarray(e.moments_section_get(fam, a, b))).cast("B"))
        os.replace(tmp, fn)


def moments_load(ddata, path, engines=None):
    """Read what moments_save wrote into engines on which the same registrations were made first: HEAD decides (its fingerprint
    must be that of the engine's registration; the error names what differs) before any accumulator is written.  A file that is
    truncated, foreign or of another shard is refused whole.  The next moments_accumulate continues the saved run."""
    engines = _engines_of(ddata, engines)
    for e, fn in zip(engines, _save_paths(path, engines)):
        size = os.path.getsize(fn)
        with open(fn, "rb") as f:
            raw = f.read(_SAVE_HEAD.size)
            if len(raw) != _SAVE_HEAD.size or raw[:8] != _SAVE_MAGIC:
                raise DangxError("moments_load: %s is not a file of moments_save" % fn)
            _, ver, nsec, pix0, npix = _SAVE_HEAD.unpack(raw)
            if ver != 1:
                raise DangxError("moments_load: %s has format version %d, this library reads version 1" % (fn, ver))
            if (pix0, npix) != (e.pix0, e.npix):
                raise DangxError("moments_load: %s holds pixels (%d, %d), the engine (%d, %d)" % (fn, pix0, npix, e.pix0, e.npix))
            raw = f.read(_SAVE_ENTRY.size * nsec) if 0 < nsec < 1 << 20 else b""
            if nsec < 1 or len(raw) != _SAVE_ENTRY.size * nsec:
                raise DangxError("moments_load: %s is truncated (its index is incomplete)" % fn)
            index = [_SAVE_ENTRY.unpack_from(raw, _SAVE_ENTRY.size * i) for i in range(nsec)]
            end = _SAVE_HEAD.size + _SAVE_ENTRY.size * nsec
            for fam, a, b, _, off, n in index:
                if off != end or n < 0:
                    raise DangxError("moments_load: %s is damaged (its index does not describe consecutive payloads)" % fn)
                end += n
            if end != size:
                raise DangxError("moments_load: %s is truncated (%d bytes, its index describes %d)" % (fn, size, end))
            if index[0][0] != L.SEC_HEAD:
                raise DangxError("moments_load: %s does not begin with a HEAD section" % fn)
            f.seek(index[0][4])
            head = np.frombuffer(f.read(index[0][5]), dtype=np.uint8).copy()
            why = head_diff(head_unpack(head), head_unpack(e.moments_section_get(L.SEC_HEAD)))
            if why:
                raise DangxError("moments_load: %s does not fit the engine's registration: %s" % (fn, why))
            want = e.moments_sections()
            if [tuple(t[:3]) for t in index[1:]] != want:
                raise DangxError("moments_load: %s holds other sections than the engine's registration has" % fn)
            for fam, a, b, _, off, n in index[1:]:
                if n != e.moments_section_bytes(fam, a, b):
                    raise DangxError("moments_load: %s: section %s(%d, %d) is %d bytes, the engine's %d" % (
                        fn, L.SECTION_NAMES_ALL[fam], a, b, n, e.moments_section_bytes(fam, a, b)))
            e.moments_section_put(L.SEC_HEAD, 0, 0, head)        # the library checks the fingerprint once more
            for fam, a, b, _, off, n in index[1:]:
                f.seek(off)
                e.moments_section_put(fam, a, b, np.frombuffer(f.read(n), dtype=np.uint8).copy())

