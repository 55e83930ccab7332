"""Posterior mean and standard deviation of component signals at a band, accumulated on the device (dangx_moments_signals).

Definitions (include/dangx.h, dang_amd/csrc/dx_signal_host.h): one sample of signal (comp, band, kind), kind T / Q / U, at a pixel
is the float64 product amplitude * sed, rounded as a product, with sed what dangx_eval_sed(comp, band, plane) returns; kind P is
sqrt(sQ * sQ + sU * sU) of those two rounded samples.  The host restates both with the same float64 operations, so after ONE
accumulation the mean must agree bit for bit (T / Q / U) or within the rounding of the square root's argument (P).  Over a chain
the tolerances are those derived in test_gpu_moments.py::_check_moments for Welford's update against np.mean / np.std:
8 n eps max|x| for the mean and 16 n eps (s + max|x|) for the standard deviation; for P the host's per-sample value may differ
from the device's by the rounding of two products, a sum and a square root (<= 4 eps |x|), which adds 4 eps max|x| to the mean's
tolerance and 8 eps max|x| to the standard deviation's."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import synth
from dang_amd.api import comp_desc

import oracle_ffi as O
from util import TOL_SED, make_case, shard_engines

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
T, Q, U, P = 0, 1, 2, 3

# C2: 0 cmb, 1 synch, 2 dust (T); 3 cmb_P, 4 synch_P, 5 dust_P (Q+U).  The power law, both indices of the mbb, the constant SED of
# the cmb, T and Q / U / P, two bands of one component (a segment with more than one band), a band that wants P alone, one that
# wants U alone, and an all-zero amplitude plane (synch on Q: 0 * sed is evaluated like any other sample).
C2_SPECS = [(0, 2, T), (1, 0, T), (1, 3, T), (2, 4, T), (2, 1, T), (1, 0, Q),
            (3, 2, Q), (3, 2, U), (3, 2, P), (4, 0, Q), (4, 0, U), (4, 0, P), (4, 3, P),
            (5, 4, Q), (5, 4, U), (5, 4, P), (5, 2, U)]


def _engine(case):
    dpar, ddata, bands, comps, meta = case
    return da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)


def _host_samples(eng, specs):
    """{spec: [npix]} of the current state, restated on the host: amplitude * eval_sed in float64, P from those"""
    amps, seds, out = {}, {}, {}
    for l, j, kind in specs:
        for k in ((Q, U) if kind == P else (kind,)):
            if l not in amps:
                amps[l] = eng.get_amplitude(l)
            if (l, j, k) not in seds:
                seds[(l, j, k)] = eng.eval_sed(l, j, k + 1)
    plane = lambda l, j, k: amps[l][k] * seds[(l, j, k)]
    with np.errstate(invalid="ignore"):
        for l, j, kind in specs:
            if kind == P:
                sq, su = plane(l, j, Q), plane(l, j, U)
                out[(l, j, kind)] = np.sqrt(sq * sq + su * su)
            else:
                out[(l, j, kind)] = plane(l, j, kind)
    return out


def _same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def _check_one_accumulation(eng, specs, what):
    """n = 1: the mean IS the sample -- bit-equal for T / Q / U, within 4 eps P for P; the std exactly 0 where the sample is finite"""
    assert eng.moments_count() == 1
    ref = _host_samples(eng, specs)
    for s, spec in enumerate(specs):
        mean, std = eng.moments_get_signal(s, "mean"), eng.moments_get_signal(s, "std")
        x = ref[spec]
        assert np.array_equal(np.isnan(mean), np.isnan(x)), (what, spec, "NaN positions")
        fin = np.isfinite(x)
        if spec[2] == P:
            err = np.abs(mean[fin] - x[fin])
            print("%s %s P: worst error / (4 eps P) %.3g" % (what, spec, float((err / (4 * EPS * x[fin] + 1e-300)).max()) if fin.any() else 0.0))
            assert (err <= 4 * EPS * x[fin]).all(), (what, spec)
        else:
            assert _same_bits(mean, x), (what, spec, "mean is not amplitude * eval_sed")
        assert (std[fin] == 0.0).all() and np.array_equal(np.isnan(std), np.isnan(x)), (what, spec, "std")
    return ref


def test_meaning_pinned_to_eval_signal(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    da.moments_begin(dpar, ddata)
    assert da.moments_signals(dpar, ddata, specs=C2_SPECS) == C2_SPECS
    da.gibbs_iteration(dpar, ddata, 1)
    da.moments_accumulate(ddata)
    ref = _check_one_accumulation(eng, C2_SPECS, "C2")
    assert any(np.isnan(v).any() for v in ref.values())           # masked pixels of a swept index map hold 0: NaN samples exist
    assert any(np.isfinite(v).all() for v in ref.values())
    assert (ref[(1, 0, Q)][np.isfinite(ref[(1, 0, Q)])] == 0.0).all()   # the all-zero plane: 0 * sed
    # the oracle's eval_signal on the same state, unmasked pixels
    cs = copy.deepcopy(comps)
    for l, c in enumerate(cs):
        c.amplitude = eng.get_amplitude(l)
        c.indices = eng.get_indices(l) if c.nindices else None
    orc = O.Oracle(bands, cs, ddata)
    unmasked = np.flatnonzero(np.asarray(ddata.masks)[0] != 0)
    for s, (l, j, kind) in enumerate(C2_SPECS):
        if kind == P:
            continue
        mean = eng.moments_get_signal(s, "mean")
        o = np.array([orc.L.dgo_eval_signal(orc.c, l, j, int(i), kind + 1, None) for i in unmasked])
        rel = np.abs(mean[unmasked] - o) / np.maximum(np.abs(o), 1e-300)
        print("signal %s against the oracle: worst relative error %.3g" % ((l, j, kind), float(rel[o != 0].max()) if (o != 0).any() else 0.0))
        assert (np.abs(mean[unmasked] - o) <= TOL_SED * np.abs(o)).all(), (l, j, kind)
    # the maps by name: component label, band label, kind
    pm = da.posterior_signal_maps(ddata)
    assert list(pm) == [(comps[l].label, bands[j].label, "TQUP"[k]) for l, j, k in C2_SPECS]
    assert pm[("synch_P", bands[3].label, "P")]["n"] == 1
    assert _same_bits(pm[("dust", bands[4].label, "T")]["mean"], eng.moments_get_signal(3, "mean"))
    filled = da.posterior_signal_maps(ddata, masked_value=-1.6375e30)
    m = np.asarray(ddata.masks)[0] == 0
    assert (filled[("dust", bands[4].label, "T")]["mean"][m] == -1.6375e30).all()


def test_a_real_chain(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    da.moments_begin(dpar, ddata)
    da.moments_signals(dpar, ddata, specs=C2_SPECS)
    series = {spec: [] for spec in C2_SPECS}
    n = 9
    for it in range(1, n + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        for spec, x in _host_samples(eng, C2_SPECS).items():
            series[spec].append(x)
    assert eng.moments_count() == n
    for s, spec in enumerate(C2_SPECS):
        xs = np.stack(series[spec])
        bad = np.isnan(xs).any(axis=0)
        fin = ~bad
        with np.errstate(invalid="ignore"):
            big = np.abs(xs).max(axis=0)
            ref_m = np.mean(xs, axis=0)
        extra_m, extra_s = (4 * EPS * big, 8 * EPS * big) if spec[2] == P else (0.0, 0.0)
        mean = eng.moments_get_signal(s, "mean")
        assert np.array_equal(np.isnan(mean), bad), (spec, "NaN exactly where the host series has one")
        err = np.abs(mean - ref_m)[fin]
        tol = (8 * n * EPS * big + extra_m + 1e-300)[fin]
        print("%-14s mean: worst error / tolerance %.3g" % (spec, float((err / tol).max())))
        assert (err <= tol).all(), (spec, float((err / tol).max()))
        moved = False
        for ddof in (0, 1):
            with np.errstate(invalid="ignore"):
                ref_s = np.std(xs, axis=0, ddof=ddof)
            std = eng.moments_get_signal(s, "std", ddof)
            assert np.array_equal(np.isnan(std), bad), (spec, ddof)
            err = np.abs(std - ref_s)[fin]
            tol = (16 * n * EPS * (ref_s + big) + extra_s + 1e-300)[fin]
            print("%-14s std ddof %d: worst error / tolerance %.3g" % (spec, ddof, float((err / tol).max())))
            assert (err <= tol).all(), (spec, ddof, float((err / tol).max()))
            moved = moved or (std[fin] > 0).any()
        if spec != (1, 0, Q):            # every series but the all-zero plane's moves
            assert moved, spec


def _specs_of(comps, nbands, band_of):
    """T of two bands for the T components; Q, U, P of one band and P alone of another for the Q+U components"""
    specs = []
    for l, c in enumerate(comps):
        ja, jb = band_of(l) % nbands, (band_of(l) + 3) % nbands
        if c.label.endswith("_P"):
            specs += [(l, ja, Q), (l, ja, U), (l, ja, P), (l, jb, P)]
        else:
            specs += [(l, ja, T), (l, jb, T)]
    return specs


def _bandpass_tweak(dpar, ddata, bands, comps):
    rng = np.random.default_rng(4)
    for b in bands[1::2]:                  # every second band integrated, one empty row (test_gpu_round4.py)
        nu = b.nu_c * 1e9 * np.linspace(0.9, 1.1, 9)
        tau = rng.uniform(0.2, 1.0, nu.size)
        nu[3] = 0.0
        b.id, b.nu0, b.tau0 = "bp", nu, tau / tau.sum()


@pytest.mark.parametrize("which", ["c5_six_bands", "bandpass", "calibration"])
def test_types_and_bands(built, which):
    """Free-free with a constant T_e, the log-normal and an mbb with constant indices (csed rows); integrated bandpasses; band
    calibration: one accumulation each, bit-equal to amplitude * eval_sed."""
    if which == "c5_six_bands":
        case = make_case("C5", nside=4, nbands=6, start="truth")
    elif which == "bandpass":
        case = make_case("C2", nside=4, start="truth", tweak=_bandpass_tweak)
    else:
        nb = 5
        case = make_case("C2", nside=4, start="truth", gain=[1.0 + 0.01 * ((j % 3) - 1) for j in range(nb)],
                         offset=[0.5 * ((j % 4) - 1.5) for j in range(nb)])
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    specs = _specs_of(comps, meta["nbands"], lambda l: l)
    assert len(specs) <= L.MAX_SIGNALS
    if which == "c5_six_bands":
        assert {c.type for c in comps} == {"cmb", "power-law", "mbb", "freefree", "lognormal"} and meta["nbands"] == 6
    if which == "bandpass":
        assert any(bands[j].id != "delta" for l, j, k in specs) and any(bands[j].id == "delta" for l, j, k in specs)
    eng.moments_begin(np.zeros(len(comps), dtype=np.int32))      # an empty selection plus signals is a valid run
    eng.moments_signals(specs)
    eng.profile(True)
    eng.moments_accumulate()
    prof, marked = eng.profile_get(), eng.profile_get(by_planes=True)
    eng.profile(False)
    # segments whose bands are all delta: one launch; segments with an integrated band: a second one, marked 2 in the profile
    mixed = which == "bandpass"
    assert set(prof) == {"k_signal"} and prof["k_signal"]["launches"] == (2 if mixed else 1), prof
    assert (("k_signal", 2) in marked) == mixed and (not mixed or marked[("k_signal", 2)]["launches"] == 1), marked
    ref = _check_one_accumulation(eng, specs, which)
    assert all(np.isfinite(v).all() for v in ref.values()) and any((v != 0).any() for v in ref.values())


def _states(case, n):
    """n states about the case's truth: {l: (amplitude, indices or None)} per sample"""
    dpar, ddata, bands, comps, meta = case
    rng = np.random.default_rng(17)
    out = []
    for t in range(n):
        st = {}
        for l, c in enumerate(comps):
            a = np.asarray(c.amplitude) * (1.0 + 0.05 * rng.standard_normal(np.asarray(c.amplitude).shape))
            x = None
            if c.nindices:
                x = np.asarray(c.indices) * (1.0 + 0.01 * rng.standard_normal(np.asarray(c.indices).shape))
            st[l] = (a, x)
        out.append(st)
    return out


def _all_maps(eng, nsig, n):
    out = {}
    for s in range(nsig):
        out[(s, "mean")] = eng.moments_get_signal(s, "mean")
        for ddof in ((0, 1) if n > 1 else (0,)):
            out[(s, "std", ddof)] = eng.moments_get_signal(s, "std", ddof)
    return out


def test_shards_equal_one_context(built):
    case = make_case("C2", nside=4, start="truth")
    dpar, ddata, bands, comps, meta = case
    whole = _engine(case)
    b3 = [0, 63, 130, meta["npix_global"]]               # odd lengths: the element-by-element path; the whole sky: pairs
    shards = shard_engines(case, 3, bounds=b3)
    n = 3
    states = _states(case, n)
    for engs, bounds in (([whole], [0, meta["npix"]]), (shards, b3)):
        for e in engs:
            e.moments_begin(None)
            e.moments_signals(C2_SPECS)
        for t in range(n):
            for l, (a, x) in states[t].items():
                for e, (b0, b1) in zip(engs, zip(bounds[:-1], bounds[1:])):
                    e.put_amplitude(l, np.ascontiguousarray(a[:, b0:b1]))
                    if x is not None:
                        e.put_indices(l, np.ascontiguousarray(x[:, :, b0:b1]))
            for e in engs:
                e.moments_accumulate()
    mw = _all_maps(whole, len(C2_SPECS), n)
    ms = [_all_maps(e, len(C2_SPECS), n) for e in shards]
    assert all(np.isfinite(v).all() for v in mw.values()) and any((v > 0).all() for k, v in mw.items() if k[1] == "std")
    for k, v in mw.items():
        assert _same_bits(v, np.concatenate([m[k] for m in ms])), ("three shards", k)
    pw, ps = da.posterior_signal_maps(ddata, ddof=1, engines=[whole]), da.posterior_signal_maps(ddata, ddof=1, engines=shards)
    assert list(pw) == list(ps)
    for s, k in enumerate(pw):
        assert _same_bits(pw[k]["mean"], ps[k]["mean"]) and _same_bits(pw[k]["std"], ps[k]["std"]) and pw[k]["n"] == n
        assert _same_bits(pw[k]["std"], mw[(s, "std", 1)])


def _move_off_the_grid(eng, comps, meta, dev, keep):
    """every component's maps into new caller buffers one double off the 16-byte grid"""
    npix, nmaps = meta["npix"], meta["nmaps"]
    for l, c in enumerate(comps):
        amp_old, idx_old = eng._adopted[l]
        abuf = torch.empty(nmaps * npix + 1, dtype=torch.float64, device=dev)
        amp_new = abuf[1:].view(nmaps, npix)
        amp_new.copy_(amp_old)
        idx_new, iptr = None, None
        if c.nindices:
            ibuf = torch.empty(c.nindices * nmaps * npix + 1, dtype=torch.float64, device=dev)
            idx_new = ibuf[1:].view(c.nindices, nmaps, npix)
            idx_new.copy_(idx_old)
            iptr = ctypes.c_void_p(idx_new.data_ptr())
            assert idx_new.data_ptr() % 16 == 8
        assert amp_new.data_ptr() % 16 == 8
        torch.cuda.synchronize()
        eng._chk(eng.lib.dangx_adopt_device_state(eng.h, l, ctypes.c_void_p(amp_new.data_ptr()), iptr))
        eng._adopted[l] = (amp_new, idx_new)
        c.amplitude, c.indices = amp_new, idx_new
        keep.append((abuf, amp_old, idx_old))


def test_adopted_buffers_moved_off_the_grid(built):
    """Three identical runs on caller-owned device buffers.  One moves every component's maps to new buffers one double off the
    16-byte grid after the first sample: the accumulators stay where they were and the segments go element by element.  One moves
    them BEFORE the registration (npix is even): planes and accumulators share the odd phase, so the head element goes alone and
    the pairs start at pixel 1.  Accumulation follows the buffers and gives the same bits in all three."""
    dev = torch.device("cuda", 0)
    runs = []
    for move in ("never", "after the first sample", "before the registration"):
        dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
        assert meta["npix"] % 2 == 0
        eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
        assert eng._adopted
        keep = []
        if move == "before the registration":
            _move_off_the_grid(eng, comps, meta, dev, keep)
        da.moments_begin(dpar, ddata)
        da.moments_signals(dpar, ddata, specs=C2_SPECS)
        for it in range(1, 4):
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
            if move == "after the first sample" and it == 1:
                _move_off_the_grid(eng, comps, meta, dev, keep)
        runs.append((_all_maps(eng, len(C2_SPECS), 3), [eng.get_amplitude(l) for l in range(len(comps))]))
    (ma, sa) = runs[0]
    assert any((v[np.isfinite(v)] > 0).any() for k, v in ma.items() if k[1] == "std")
    for what, (mb, sb) in zip(("moved after the first sample", "moved before the registration"), runs[1:]):
        for a, b in zip(sa, sb):
            assert np.array_equal(a, b), what                 # the chains themselves are the same
        for k in ma:
            assert _same_bits(ma[k], mb[k]), (what, k)


def _snapshot(eng):
    return {l: (eng.get_amplitude(l), eng.get_indices(l) if c.nindices else None) for l, c in enumerate(eng.component_list)}


def _run(nit, signals):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    eng.profile(True)
    da.moments_begin(dpar, ddata)
    if signals == "first":
        da.moments_signals(dpar, ddata)
    da.moments_pairs(dpar, ddata)
    da.moments_hist(dpar, ddata)
    if signals == "last":
        da.moments_signals(dpar, ddata)
    for it in range(1, nit + 1):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    return (eng, _snapshot(eng), ddata.chisq, da.posterior_maps(ddata), da.posterior_pair_maps(ddata),
            da.posterior_quantile_maps(ddata), ddata)


def test_nothing_else_moves(built):
    """Five iterations with pairs, lag-1 and histograms registered, with and without signals (registered before or after the
    others): the chain, chi^2 and every other summary bit-identical; one k_signal launch per accumulation, none without."""
    e0, s0, chi0, p0, c0, q0, d0 = _run(5, None)
    assert getattr(e0, "_moment_signals", None) is None
    sig = {}
    for order in ("first", "last"):
        e, s, chi, p, c, q, d = _run(5, order)
        assert chi == chi0
        for l in s0:
            assert np.array_equal(s[l][0], s0[l][0]) and (s0[l][1] is None or np.array_equal(s[l][1], s0[l][1]))
        assert p.keys() == p0.keys() and c.keys() == c0.keys() and q.keys() == q0.keys() and len(c0) == 12 and len(q0) == 9
        for k in p0:
            for stat in ("mean", "std", "rho1", "ess"):
                assert np.array_equal(p[k][stat], p0[k][stat], equal_nan=True), (k, stat)
        for k in c0:
            assert np.array_equal(c[k], c0[k], equal_nan=True), k
        for k in q0:
            for name in ("q", "mode", "n"):
                assert np.array_equal(q[k][name], q0[k][name], equal_nan=True), (k, name)
        prof0, prof = e0.profile_get(), e.profile_get()
        assert "k_signal" not in prof0
        assert prof["k_signal"]["launches"] == 5 and prof["k_signal"]["total_ms"] > 0
        assert prof["k_moments"]["launches"] == prof0["k_moments"]["launches"] == 10
        assert prof["k_hist"]["launches"] == prof0["k_hist"]["launches"] == 5
        assert {k: v["launches"] for k, v in prof0.items()} == {k: v["launches"] for k, v in prof.items() if k != "k_signal"}
        sig[order] = da.posterior_signal_maps(d)
        specs = e._moment_signals
        assert specs == [(1, 0, T), (2, 3, T), (4, 0, Q), (4, 0, U), (4, 0, P), (5, 3, Q), (5, 3, U), (5, 3, P)]
    for k in sig["first"]:                                  # the order of the registrations does not matter to the signals either
        assert sig["first"][k]["n"] == 5
        for stat in ("mean", "std"):
            assert _same_bits(sig["first"][k][stat], sig["last"][k][stat]), (k, stat)


def test_errors_and_the_begin_drops_it_rule(built):
    """Every error of dangx_moments_signals / _get_signal except a failed allocation, which cannot be produced on a shared device
    without exhausting its memory (that path frees what it allocated and leaves the registration as it was, as the others do)."""
    case = make_case("C2", nside=4, start="truth")
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    good = [(1, 0, T), (4, 0, P)]
    with pytest.raises(da.DangxError, match="begin"):
        eng.moments_signals(good)
    none = np.zeros(len(comps), dtype=np.int32)
    eng.moments_begin(none)
    eng.moments_signals(good)
    with pytest.raises(da.DangxError, match="no sample accumulated"):
        eng.moments_get_signal(0, "mean")
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="before the first"):
        eng.moments_signals(good)
    eng.moments_begin(none)
    first = [(1, 0, "T"), (4, 0, "Q"), (4, 0, "P"), (5, 4, U)]
    eng.moments_signals(first)
    first = [(1, 0, T), (4, 0, Q), (4, 0, P), (5, 4, U)]
    assert eng._moment_signals == first
    bad = [
        ("component index", [(len(comps), 0, T)]),
        ("component index", [(-1, 0, T)]),
        ("band index", [(1, meta["nbands"], T)]),
        ("band index", [(1, -1, T)]),
        ("kind must be", [(1, 0, 4)]),
        ("kind must be", [(1, 0, -1)]),
        ("the same signal twice", [(1, 0, T), (4, 0, P), (1, 0, T)]),
        ("DANGX_MAX_SIGNALS", [(l, j, k) for l in range(6) for j in range(5) for k in range(4)][:65]),
    ]
    for match, specs in bad:
        with pytest.raises(da.DangxError, match=match):
            eng.moments_signals(specs)
        assert eng._moment_signals == first                    # nothing changed
    eng.moments_signals([(l, j, k) for l in range(6) for j in range(5) for k in range(4)][:64])     # the limit itself is fine
    eng.moments_signals(first)
    # a registered component changes its shape: accumulation refuses, as it does for a selected one
    d = comp_desc(comps[4])
    d.type = L.FREEFREE                                      # a power law becomes free-free: one index either way
    eng._chk(eng.lib.dangx_set_component(eng.h, 4, ctypes.byref(d)))
    with pytest.raises(da.DangxError, match="component 4 changed type or nindices since dangx_moments_signals"):
        eng.moments_accumulate()
    eng._chk(eng.lib.dangx_set_component(eng.h, 4, ctypes.byref(comp_desc(comps[4]))))
    assert eng.moments_count() == 0
    eng.moments_accumulate()
    eng.moments_accumulate()
    ref = _host_samples(eng, first)
    for s, spec in enumerate(first):                            # the earlier registration is what accumulated, twice the same state
        mean = eng.moments_get_signal(s, "mean")
        if spec[2] != P:
            assert _same_bits(mean, ref[spec]), spec
        assert (eng.moments_get_signal(s, "std") == 0).all()
        dm = eng.moments_get_signal(s, "mean", device=True)
        ds = eng.moments_get_signal(s, "std", ddof=1, device=True)
        assert dm.is_cuda and dm.dtype == torch.float64 and np.array_equal(dm.cpu().numpy(), mean)
        assert np.array_equal(ds.cpu().numpy(), eng.moments_get_signal(s, "std", ddof=1))
    for s in (len(first), -1):
        with pytest.raises(da.DangxError, match="signal index out of range"):
            eng.moments_get_signal(s, "mean")
        with pytest.raises(da.DangxError, match="signal index out of range"):
            eng.moments_get_signal(s, "mean", device=True)
    with pytest.raises(da.DangxError, match="stat of a signal"):
        eng.moments_get_signal(0, 2)
    for ddof in (2, 3, -1):
        with pytest.raises(da.DangxError, match="ddof"):
            eng.moments_get_signal(0, "std", ddof)
    # the amplitude plane of a signal need not be selected: nothing else is readable here
    with pytest.raises(da.DangxError, match="nothing selected"):
        eng.moments_get(1, 0, "mean")
    # a second call replaces the first; nsig = 0: none; pairs and histograms stay
    sel = da.default_moment_selection(dpar, comps)
    eng.moments_begin(sel)
    eng.moments_pairs([((1, 0, 0), (1, 1, 0))], lag1=True)
    eng.moments_hist([(1, 1, 0)], nbins=8)
    eng.moments_signals(first)
    eng.moments_signals(good)
    eng.moments_accumulate()
    assert eng.moments_get_signal(1, "mean").shape == (meta["npix"],)
    with pytest.raises(da.DangxError, match="out of range .2 signals registered"):
        eng.moments_get_signal(2, "mean")
    assert eng.moments_get_pair(0, "cov").shape == (meta["npix"],) and eng.moments_hist_get(0).shape == (meta["npix"], 8)
    eng.moments_begin(sel)
    eng.moments_signals(good)
    eng.moments_signals([])
    eng.profile(True)
    eng.moments_accumulate()
    assert "k_signal" not in eng.profile_get()
    with pytest.raises(da.DangxError, match="out of range .0 signals registered"):
        eng.moments_get_signal(0, "mean")
    # begin drops a registration
    eng.moments_begin(sel)
    eng.moments_signals(good)
    eng.moments_begin(sel)
    assert eng._moment_signals is None
    eng.moments_accumulate()
    assert "k_signal" not in eng.profile_get()
    with pytest.raises(da.DangxError, match="out of range .0 signals registered"):
        eng.moments_get_signal(0, "mean")
    with pytest.raises(da.DangxError, match="moments_signals was not called"):
        da.posterior_signal_maps(ddata)
    eng.moments_end()
    with pytest.raises(da.DangxError, match="begin"):
        eng.moments_signals(good)


def test_kinds_the_model_does_not_have_and_global_members(built):
    """nmaps = 1: no Q, U or P.  A template / monopole member: refused by the name of the call that reads its amplitude."""
    case = make_case("C1", nside=4, start="truth")
    dpar, ddata, bands, comps, meta = case
    eng = _engine(case)
    eng.moments_begin(None)
    eng.moments_signals([(0, 1, T)])
    for kind, match in ((Q, "a plane the model does not have"), (U, "a plane the model does not have"), (P, "P needs nmaps == 3")):
        with pytest.raises(da.DangxError, match=match):
            eng.moments_signals([(0, 1, kind)])
    eng.moments_accumulate()
    assert _same_bits(eng.moments_get_signal(0, "mean"), eng.get_amplitude(0)[0] * eng.eval_sed(0, 1, 1))
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 3, 4), amplitudes=(3.0, -2.0, 5.0))
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    da.moments_begin(dpar, ddata)
    lt, lm = len(comps) - 2, len(comps) - 1
    specs = da.moments_signals(dpar, ddata)                   # the defaults leave them out
    assert len(specs) == 8 and all(l < lt for l, j, k in specs)
    for spec in ((lt, 2, Q), (lt, 2, P), (lm, 0, T)):
        with pytest.raises(da.DangxError, match="dangx_moments_get_template"):
            eng.moments_signals([(1, 0, T), spec])
    assert eng._moment_signals == specs
    da.gibbs_iteration(dpar, ddata, 1)
    da.moments_accumulate(ddata)
    _check_one_accumulation(eng, specs, "with global members")
