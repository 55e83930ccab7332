"""Posterior polarisation angle of a component's signal at a band, accumulated on the device (dangx_moments_angles).

Definitions (include/dangx.h, dang_amd/csrc/dx_angle_host.h): one sample of angle (comp, band) at a pixel is the pair
c = sQ / P, s = sU / P with sQ, sU the rounded samples amplitude * sed of signal kinds Q and U and P = sqrt(sQ * sQ + sU * sU); the
accumulators are the running means Cbar, Sbar (stats 3 and 4).  The host restates the sample with the same float64 operations,
so after ONE accumulation stats 3 and 4 must agree bit for bit.  Over a chain of n samples the means are checked against
np.longdouble: |c|, |s| <= 1 and the update m = fma(x - m, 1/n, m) rounds twice (the difference, the fma), so the error is at most
4 n 2^-52 absolute.  The read-outs psi = atan2(Sbar, Cbar) / 2, R = min(1, sqrt(Cbar^2 + Sbar^2)) and the circular std
sqrt(-2 log R) / 2 are checked against numpy on the device's own Cbar, Sbar: psi to 16 * 2^-52 rad (a 6-ulp atan2 at |result| <=
pi, halved, plus numpy's own rounding), the std as its square to 8 * 2^-52 * (1 + ref) (a 3-ulp log plus the conditioning of R
near 1; the exact 0 the library returns for R >= 1 - 5 * 2^-53 differs from the expression by at most 1.25 * 2^-52 there), R bit
for bit."""
import ctypes

import numpy as np
import pytest
import torch

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import api, synth

import test_gpu_chains as tc
import test_gpu_moments_signal as tsig
import test_gpu_sections as tsec
from util import make_case, shard_engines

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
NPIX = 192
# C2: 3 cmb_P, 4 synch_P, 5 dust_P (Q+U): every polarised diffuse component at two bands
C2_ANGLES = [(3, 2), (3, 0), (4, 0), (4, 3), (5, 4), (5, 2)]
STATS = ("psi", "psi_std", "R", "C", "S")


def _same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def _host_cs(eng, specs):
    """{spec: (c, s)} of the current state, restated on the host with the definition's float64 operations"""
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for l, j in specs:
            amp = eng.get_amplitude(l)
            sq, su = amp[1] * eng.eval_sed(l, j, 2), amp[2] * eng.eval_sed(l, j, 3)
            p = np.sqrt(sq * sq + su * su)
            out[(l, j)] = (sq / p, su / p)
    return out


def _pull(eng, a):
    return {st: eng.moments_get_angle(a, st) for st in STATS}


def _check_readouts(got, what):
    """stats 0-2 against numpy on the device's own stats 3 and 4; prints each worst figure as a fraction of its bound"""
    C, S = got["C"], got["S"]
    with np.errstate(invalid="ignore", divide="ignore"):
        R = np.minimum(1, np.sqrt(C * C + S * S))
        psi = 0.5 * np.arctan2(S, C)
        std = 0.5 * np.sqrt(-2 * np.log(R))
    assert _same_bits(got["R"], R), (what, "R is not min(1, sqrt(C*C + S*S))")
    nan = np.isnan(C) | np.isnan(S)
    for st in ("psi", "psi_std"):
        assert np.array_equal(np.isnan(got[st]), nan), (what, st, "NaN positions")
    fin = ~nan
    e_psi = np.abs(got["psi"][fin] - psi[fin])
    print("%s psi: worst error / (16 * 2^-52) = %.3g" % (what, float(e_psi.max() / (16 * U52)) if fin.any() else 0.0))
    assert (e_psi <= 16 * U52).all(), what
    inf = fin & np.isinf(std)
    assert np.array_equal(np.isinf(got["psi_std"]) & fin, inf), (what, "R = 0 gives +inf")
    ok = fin & ~inf
    sq_got, sq_ref = got["psi_std"][ok] ** 2, std[ok] ** 2
    e_std = np.abs(sq_got - sq_ref) / (8 * U52 * (1 + sq_ref))
    print("%s psi_std^2: worst error / (8 * 2^-52 (1 + ref)) = %.3g" % (what, float(e_std.max()) if ok.any() else 0.0))
    assert (e_std <= 1.0).all(), what
    assert (np.abs(got["psi"][fin]) <= np.pi / 2).all()


def _check_one_accumulation(eng, specs, what):
    """n = 1: Cbar, Sbar ARE the sample, bit for bit; then the read-outs on them"""
    assert eng.moments_count() == 1
    ref = _host_cs(eng, specs)
    for a, spec in enumerate(specs):
        got = _pull(eng, a)
        assert _same_bits(got["C"], ref[spec][0]), (what, spec, "Cbar is not sQ / P")
        assert _same_bits(got["S"], ref[spec][1]), (what, spec, "Sbar is not sU / P")
        _check_readouts(got, "%s %s" % (what, spec))
    return ref


# ---- 1. meaning

def test_meaning_pinned_to_the_signals(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = tsig._engine(case)
    da.moments_begin(dpar, ddata)
    assert da.moments_angles(dpar, ddata, specs=C2_ANGLES) == C2_ANGLES and eng._moment_angles == C2_ANGLES
    da.gibbs_iteration(dpar, ddata, 1)
    da.moments_accumulate(ddata)
    ref = _check_one_accumulation(eng, C2_ANGLES, "C2")
    assert any(np.isnan(c).any() for c, s in ref.values()) and any(np.isfinite(c).sum() > NPIX // 2 for c, s in ref.values())
    pm = da.posterior_angle_maps(ddata)
    assert list(pm) == [(comps[l].label, bands[j].label) for l, j in C2_ANGLES]
    e = pm[("dust_P", bands[4].label)]
    assert set(e) == {"n", "psi", "psi_std", "R"} and e["n"] == 1
    assert _same_bits(e["psi"], eng.moments_get_angle(4, "psi")) and _same_bits(e["R"], eng.moments_get_angle(4, 2))
    filled = da.posterior_angle_maps(ddata, masked_value=-1.6375e30)
    m = np.asarray(ddata.masks)[0] == 0
    assert m.any() and (filled[("dust_P", bands[4].label)]["psi"][m] == -1.6375e30).all()
    # the device form gives the same bits
    dev = eng.moments_get_angle(2, "psi_std", device=True)
    assert _same_bits(dev.cpu().numpy(), eng.moments_get_angle(2, "psi_std"))
    # the default list: one angle per default P signal
    assert da.default_angle_specs(dpar, comps, bands) == [(l, j) for l, j, k in da.default_signal_specs(dpar, comps, bands) if k == 3]


# ---- 2. and 3. a real chain, and the read-outs on it

@pytest.fixture(scope="module")
def chain9(built):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = tsig._engine(case)
    da.moments_begin(dpar, ddata)
    da.moments_angles(dpar, ddata, specs=C2_ANGLES)
    series = {spec: [] for spec in C2_ANGLES}
    for it in range(1, 10):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
        for spec, cs in _host_cs(eng, C2_ANGLES).items():
            series[spec].append(cs)
    return {"eng": eng, "series": series, "got": [_pull(eng, a) for a in range(len(C2_ANGLES))]}


def test_a_real_chain(chain9):
    """Worst measured error of Cbar, Sbar against the long-double mean of the restated samples, as a fraction of the bound
    4 n 2^-52: printed per angle (DESIGN.md records it)."""
    n = 9
    assert chain9["eng"].moments_count() == n
    worst, moved = 0.0, False
    for a, spec in enumerate(C2_ANGLES):
        for i, st in enumerate(("C", "S")):
            xs = np.stack([cs[i] for cs in chain9["series"][spec]]).astype(np.longdouble)
            bad = np.isnan(xs).any(axis=0)
            with np.errstate(invalid="ignore"):
                ref = xs.sum(axis=0) / n
            got = chain9["got"][a][st]
            assert np.array_equal(np.isnan(got), bad), (spec, st, "NaN exactly where the host series has one")
            err = np.abs(got.astype(np.longdouble) - ref)[~bad]
            frac = float(err.max() / (4 * n * U52))
            print("%s %s: worst error / (4 n 2^-52) = %.3g" % (spec, st, frac))
            worst = max(worst, frac)
            assert (err <= 4 * n * U52).all(), (spec, st, frac)
            moved = moved or (np.ptp(np.asarray(xs[:, ~bad], dtype=np.float64), axis=0) > 0).any()
    print("worst of all: %.3g of the bound" % worst)
    assert moved


def test_readouts_of_the_chain(chain9):
    some_spread = False
    for a, spec in enumerate(C2_ANGLES):
        got = chain9["got"][a]
        _check_readouts(got, "chain %s" % (spec,))
        fin = np.isfinite(got["psi_std"])
        some_spread = some_spread or (got["psi_std"][fin] > 0).any()
        assert ((got["R"][np.isfinite(got["R"])] >= 0) & (got["R"][np.isfinite(got["R"])] <= 1)).all()
    assert some_spread


# ---- 4. and 5. planted angles, zero pixels

def _planted_run(zero_pixel=None):
    """synch_P's Q, U written by hand into the adopted amplitude tensor before each of 4 accumulations: psi = +85 / -85 degrees in
    turn in the first half of the pixels, 20 degrees in the rest, |P| = 1; the Q and U index planes made equal, so that the SED
    scales both alike and leaves the angle as written"""
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    l = [c.label for c in comps].index("synch_P")
    amp, idx = eng._adopted[l]
    idx[:, 2, :] = idx[:, 1, :]
    eng.moments_begin(np.zeros(len(comps), dtype=np.int32))
    eng.moments_angles([(l, 0), (l, 3)])
    half = NPIX // 2
    for t in range(4):
        psi = np.full(NPIX, np.deg2rad(20.0))
        psi[:half] = np.deg2rad(85.0) * (1 if t % 2 == 0 else -1)
        q, u = np.cos(2 * psi), np.sin(2 * psi)
        if t % 2 == 1:
            u[:half] = -np.sin(2 * np.deg2rad(85.0))        # exactly the negative of the even samples' U
        if zero_pixel is not None:
            q[zero_pixel] = u[zero_pixel] = 0.0
        amp[1].copy_(torch.from_numpy(q).to(dev))
        amp[2].copy_(torch.from_numpy(u).to(dev))
        torch.cuda.synchronize()
        eng.moments_accumulate()
    return eng, half


def test_planted_angles(built):
    eng, half = _planted_run()
    for a in (0, 1):
        got = _pull(eng, a)
        assert all(np.isfinite(v).all() for v in got.values())
        # the wrap: the arithmetic mean of +85 and -85 degrees is 0, the circular mean is +-90 degrees
        e = np.abs(np.abs(got["psi"][:half]) - np.pi / 2)
        print("angle %d: | |psi| - pi/2 | worst / (16 * 2^-52) = %.3g" % (a, float(e.max() / (16 * U52))))
        assert (e <= 16 * U52).all()
        e = np.abs(got["psi"][half:] - np.deg2rad(20.0))
        print("angle %d: | psi - 20 deg | worst / (16 * 2^-52) = %.3g" % (a, float(e.max() / (16 * U52))))
        assert (e <= 16 * U52).all()
        # R: the samples' c = cos 170 deg carries the rounding of cos, a product, P (two products, a sum, a square root) and a
        # division, each at most 2^-53 relative on values <= 1: 16 * 2^-52 leaves room for all of them
        e = np.abs(got["R"][:half] - np.cos(np.deg2rad(10.0)))
        print("angle %d: | R - cos 10 deg | worst / (16 * 2^-52) = %.3g" % (a, float(e.max() / (16 * U52))))
        assert (e <= 16 * U52).all()
        # the fixed pixels: every sample is the same unit vector, so Cbar, Sbar are that vector and R its rounded length
        e = np.abs(got["R"][half:] - 1.0)
        print("angle %d: fixed pixels | R - 1 | worst / (16 * 2^-52) = %.3g" % (a, float(e.max() / (16 * U52))))
        assert (e <= 16 * U52).all() and (got["R"][half:] <= 1.0).all()
        assert (got["psi_std"][:half] > 0.08).all() and (got["psi_std"][:half] < 0.09).all()     # sqrt(-2 log cos 10 deg) / 2 = 0.0875


def test_planted_fixed_pixels_have_a_std_of_exactly_zero(built):
    """The pixels whose angle never moves read a circular std of exactly 0.  The sample (c, s) = (sQ, sU) / P is a unit vector only
    to rounding: where c * c + s * s rounds below 1 the clamp R = min(1, .) has nothing to cut and R reads 1 - 2^-53 (measured: 41
    of the 96 fixed pixels at Nside 4), for which 0.5 sqrt(-2 log R) is 7.45e-9 rad.  dx_angle_spread therefore returns 0 for every
    R within the rounding of a unit vector's length of 1, R >= 1 - 5 * 2^-53 (the derivation stands in dx_angle_host.h); R itself
    (stat 2) stays the stated expression, bit for bit."""
    eng, half = _planted_run()
    for a in (0, 1):
        got = _pull(eng, a)
        print("angle %d: fixed pixels: R - 1 in [%.3g, %.3g], std in [%.3g, %.3g], %d of %d pixels with a std of 0" % (
            a, float((got["R"][half:] - 1).min()), float((got["R"][half:] - 1).max()), float(got["psi_std"][half:].min()),
            float(got["psi_std"][half:].max()), int((got["psi_std"][half:] == 0).sum()), NPIX - half))
        assert not np.isnan(got["psi_std"][half:]).any()
        assert (got["psi_std"][half:] == 0.0).all()
        assert (got["R"][half:] >= 1 - 5 * 2.0 ** -53).all() and (got["R"][half:] <= 1).all()


def test_zero_pixels(built):
    """Q = U = 0 in pixel 10 of every sample: NaN in stats 0-4 there, and its neighbour in the same 16-byte pair (pixel 11), like
    every other pixel, holds what it holds in the run without the zero"""
    ref, _ = _planted_run()
    eng, _ = _planted_run(zero_pixel=10)
    for a in (0, 1):
        got, want = _pull(eng, a), _pull(ref, a)
        for st in STATS:
            assert np.isnan(got[st][10]), st
            keep = np.arange(NPIX) != 10
            assert np.isfinite(got[st][keep]).all() and np.array_equal(got[st][keep], want[st][keep]), st


# ---- 6. forms

def _qu_index_tweak(eng, comps):
    for l, c in enumerate(comps):
        if c.nindices and c.label.endswith("_P"):
            x = eng.get_indices(l)
            x[:, 2, :] *= 1.0 + 0.01 * (1 + np.arange(x.shape[2]) % 3)
            eng.put_indices(l, x)


@pytest.mark.parametrize("which", ["c5_six_bands", "bandpass", "calibration", "qu_index_maps_differ"])
def test_forms(built, which):
    """Free-free with a constant T_e, the log-normal, an mbb with constant indices (csed rows); integrated bandpasses through the
    BP form; band calibration; index maps that differ between Q and U: one accumulation each, stats 3 and 4 bit-equal to the
    restated sample.  The profile: one launch, two where a segment has an integrated band, and nothing else."""
    if which == "c5_six_bands":
        case = make_case("C5", nside=4, nbands=6, start="truth")
    elif which == "bandpass":
        case = make_case("C2", nside=4, start="truth", tweak=tsig._bandpass_tweak)
    elif which == "calibration":
        case = make_case("C2", nside=4, start="truth", gain=[1.0 + 0.01 * ((j % 3) - 1) for j in range(5)],
                         offset=[0.5 * ((j % 4) - 1.5) for j in range(5)])
    else:
        case = make_case("C2", nside=4, start="truth")
    dpar, ddata, bands, comps, meta = case
    eng = tsig._engine(case)
    nb = meta["nbands"]
    specs = [(l, j % nb) for l, c in enumerate(comps) if c.label.endswith("_P") for j in (l, l + 3)]
    if which == "c5_six_bands":
        assert {c.type for c in comps} == {"cmb", "power-law", "mbb", "freefree", "lognormal"} and nb == 6
    if which == "bandpass":
        assert any(bands[j].id != "delta" for l, j in specs) and any(bands[j].id == "delta" for l, j in specs)
    if which == "qu_index_maps_differ":
        _qu_index_tweak(eng, comps)
        x = eng.get_indices(4)
        assert (x[0, 1] != x[0, 2]).all()
    eng.moments_begin(np.zeros(len(comps), dtype=np.int32))      # an empty selection plus angles is a valid run
    eng.moments_angles(specs)
    eng.profile(True)
    eng.moments_accumulate()
    prof, marked = eng.profile_get(), eng.profile_get(by_planes=True)
    eng.profile(False)
    mixed = which == "bandpass"
    assert set(prof) == {"k_angle"} and prof["k_angle"]["launches"] == (2 if mixed else 1), prof
    assert (("k_angle", 2) in marked) == mixed and (not mixed or marked[("k_angle", 2)]["launches"] == 1), marked
    ref = _check_one_accumulation(eng, specs, which)
    assert all(np.isfinite(c).all() and np.isfinite(s).all() for c, s in ref.values())


def _all_maps(eng, nang):
    return {(a, st): eng.moments_get_angle(a, st) for a in range(nang) for st in STATS}


def test_odd_shards_equal_one_context(built):
    """192 = 95 + 97: both shards go element by element (the U plane of an odd-length shard is off the Q plane's 16-byte phase),
    the whole sky in pairs: the same bits"""
    case = make_case("C2", nside=4, start="truth")
    dpar, ddata, bands, comps, meta = case
    whole = tsig._engine(case)
    b2 = [0, 95, meta["npix_global"]]
    shards = shard_engines(case, 2, bounds=b2)
    assert [e.npix for e in shards] == [95, 97]
    n = 3
    states = tsig._states(case, n)
    for engs, bounds in (([whole], [0, meta["npix"]]), (shards, b2)):
        for e in engs:
            e.moments_begin(None)
            e.moments_angles(C2_ANGLES)
        for t in range(n):
            for l, (a, x) in states[t].items():
                for e, (b0, b1) in zip(engs, zip(bounds[:-1], bounds[1:])):
                    e.put_amplitude(l, np.ascontiguousarray(a[:, b0:b1]))
                    if x is not None:
                        e.put_indices(l, np.ascontiguousarray(x[:, :, b0:b1]))
            for e in engs:
                e.moments_accumulate()
    mw = _all_maps(whole, len(C2_ANGLES))
    ms = [_all_maps(e, len(C2_ANGLES)) for e in shards]
    assert all(np.isfinite(v).all() for v in mw.values()) and any((v > 0).all() for k, v in mw.items() if k[1] == "psi_std")
    for k, v in mw.items():
        assert _same_bits(v, np.concatenate([m[k] for m in ms])), ("two odd shards", k)
    pw, ps = da.posterior_angle_maps(ddata, engines=[whole]), da.posterior_angle_maps(ddata, engines=shards)
    assert list(pw) == list(ps)
    for k in pw:
        assert all(_same_bits(pw[k][st], ps[k][st]) for st in ("psi", "psi_std", "R")) and pw[k]["n"] == ps[k]["n"] == n


def test_adopted_buffers_moved_off_the_grid(built):
    """Three identical runs on caller-owned device buffers: never moved (pairs at phase 0); moved one double off the 16-byte
    grid after the first sample (the accumulators stay: element by element); moved before the registration (planes and
    accumulators share the odd phase: the head element alone, pairs from pixel 1, the last element alone).  The same bits."""
    dev = torch.device("cuda", 0)
    runs = []
    for move in ("never", "after the first sample", "before the registration"):
        dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
        eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
        keep = []
        if move == "before the registration":
            tsig._move_off_the_grid(eng, comps, meta, dev, keep)
        da.moments_begin(dpar, ddata)
        da.moments_angles(dpar, ddata, specs=C2_ANGLES)
        for it in range(1, 4):
            da.gibbs_iteration(dpar, ddata, it)
            da.moments_accumulate(ddata)
            if move == "after the first sample" and it == 1:
                tsig._move_off_the_grid(eng, comps, meta, dev, keep)
        runs.append((_all_maps(eng, len(C2_ANGLES)), [eng.get_amplitude(l) for l in range(len(comps))]))
    (ma, sa) = runs[0]
    assert any((v[np.isfinite(v)] > 0).any() for k, v in ma.items() if k[1] == "psi_std")
    for what, (mb, sb) in zip(("moved after the first sample", "moved before the registration"), runs[1:]):
        for a, b in zip(sa, sb):
            assert np.array_equal(a, b), what                 # the chains themselves are the same
        for k in ma:
            assert _same_bits(ma[k], mb[k]), (what, k)


# ---- 7. nothing else moves

def _launch_counts(angles):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    eng = tsig._engine(case)
    da.moments_begin(dpar, ddata)
    da.moments_pairs(dpar, ddata)
    da.moments_hist(dpar, ddata)
    da.moments_signals(dpar, ddata)
    if angles:
        assert len(da.moments_angles(dpar, ddata)) == 2
    eng.profile(True)
    for it in (1, 2):
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    eng.synchronize()
    counts = {k: v["launches"] for k, v in eng.profile_get().items()}
    state = [eng.get_amplitude(l) for l in range(len(comps))]
    sig = [eng.moments_get_signal(s, "mean") for s in range(len(eng._moment_signals))]
    return counts, state, sig


def test_nothing_else_moves(built):
    c0, s0, g0 = _launch_counts(False)
    c1, s1, g1 = _launch_counts(True)
    assert "k_angle" not in c0 and c0["k_signal"] == 2 and c0["k_moments"] >= 2
    assert c1.pop("k_angle") == 2                         # one launch per accumulation
    assert c1 == c0
    assert all(np.array_equal(a, b) for a, b in zip(s0, s1)) and all(_same_bits(a, b) for a, b in zip(g0, g1))


# ---- 8. errors

def test_errors(built):
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    eng = da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    lt = len(comps) - 1
    with pytest.raises(da.DangxError, match="dangx_moments_begin was not called"):
        eng.moments_angles([(4, 0)])
    da.moments_begin(dpar, ddata)
    for specs, match in (([(len(comps), 0)], "angle 0: component index out of range"), ([(4, 0), (4, 5)], "angle 1: band index out of range"),
                         ([(4, -1)], "band index out of range"), ([(lt, 2)], "template / monopole / hi_fit"),
                         ([(4, 0), (5, 1), (4, 0)], "angle 2: the same angle twice"),
                         ([(3 + k % 3, (k // 3) % 5) for k in range(65)], "DANGX_MAX_ANGLES")):
        with pytest.raises(da.DangxError, match="dangx_moments_angles: .*" + match):
            eng.moments_angles(specs)
        assert eng._moment_angles is None
    eng.moments_angles([(4, 0), (5, 4)])
    with pytest.raises(da.DangxError, match="no sample accumulated"):
        eng.moments_get_angle(0, "psi")
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match="dangx_moments_angles is legal only before the first dangx_moments_accumulate"):
        eng.moments_angles([(4, 1)])
    assert eng._moment_angles == [(4, 0), (5, 4)]
    with pytest.raises(da.DangxError, match=r"angle index out of range \(2 angles registered\)"):
        eng.moments_get_angle(2, "psi")
    with pytest.raises(da.DangxError, match="angle index out of range"):
        eng.moments_get_angle(-1, "psi")
    with pytest.raises(da.DangxError, match="the stat of an angle must be"):
        eng.moments_get_angle(0, 6)
    with pytest.raises(da.DangxError, match="stat 5 .* needs several chains"):
        eng.moments_get_angle(0, "between")
    assert eng.moments_section_bytes("ANGLE", 1) == 2 * NPIX * 8
    with pytest.raises(da.DangxError, match=r"angle index out of range \(2 registered\)"):
        eng.moments_section_bytes("ANGLE", 2)
    assert ("ANGLE" in [L.SECTION_NAMES[f] for f, a, b in eng.moments_sections()]) and eng.moments_sections()[-2:] == [(L.SEC_ANGLE, 0, 0), (L.SEC_ANGLE, 1, 0)]
    # a holder takes the registration over and refuses the single-chain read-out
    H = api._holder_engine(eng)
    H.moments_begin_like(eng)
    assert H._moment_angles == [(4, 0), (5, 4)]
    with pytest.raises(da.DangxError, match="holder"):
        H.moments_get_angle(0, "psi")
    # moments_begin drops the registration, in the library and in the mirror
    da.moments_begin(dpar, ddata)
    assert eng._moment_angles is None and eng.moments_sections() and L.SEC_ANGLE not in [f for f, a, b in eng.moments_sections()]
    eng.moments_accumulate()
    with pytest.raises(da.DangxError, match=r"angle index out of range \(0 angles registered\)"):
        eng.moments_get_angle(0, "psi")
    with pytest.raises(da.DangxError, match="moments_angles was not called"):
        da.posterior_angle_maps(ddata)
    # an nmaps = 1 model has no Q, U
    c1 = make_case("C1", nside=4)
    e1 = tsig._engine(c1)
    e1.moments_begin(None)
    with pytest.raises(da.DangxError, match="nmaps == 3"):
        e1.moments_angles([(0, 0)])


# ---- 9. several chains, holders

def _host_chains(Ck, Sk, counts, stat):
    """the definitions over K chains on the per-chain Cbar, Sbar in numpy: the pooled pair in list order, every product and sum
    rounded; 'between' from the chains' unit vectors"""
    N = float(sum(counts))
    w = [float(n) / N for n in counts]
    with np.errstate(invalid="ignore", divide="ignore"):
        if stat == "between":
            cb = sb = None
            for C, S in zip(Ck, Sk):
                r = np.sqrt(C * C + S * S)
                cb, sb = (C / r, S / r) if cb is None else (cb + C / r, sb + S / r)
            cb, sb = cb / float(len(Ck)), sb / float(len(Ck))
            return 0.5 * np.sqrt(-2 * np.log(np.minimum(1, np.sqrt(cb * cb + sb * sb))))
        C, S = w[0] * Ck[0], w[0] * Sk[0]
        for k in range(1, len(Ck)):
            C, S = C + w[k] * Ck[k], S + w[k] * Sk[k]
    return C, S


def _three_chains(counts):
    case = make_case("C2", nside=4)
    dpar, ddata, bands, comps, meta = case
    tsig._engine(case)
    runs = [(dpar, ddata)] + [da.open_chain(dpar, ddata, 7000 + k) for k in (1, 2)]
    for sign, (p, d) in zip((0, 1, -1), runs):
        if sign:
            tc._disperse(d.engine, sign)
        da.moments_begin(p, d)
        da.moments_angles(p, d, specs=C2_ANGLES)
    for it in range(1, max(counts) + 1):
        for n, (p, d) in zip(counts, runs):
            da.gibbs_iteration(p, d, it)
            if it <= n:
                da.moments_accumulate(d)
    return [d.engine for _, d in runs], [d for _, d in runs]


@pytest.mark.parametrize("counts", [(5, 5, 5), (6, 3, 4)])
def test_several_chains(built, counts):
    engs, chains = _three_chains(counts)
    assert [e.moments_count() for e in engs] == list(counts)
    between_seen = False
    for a, spec in enumerate(C2_ANGLES):
        Ck, Sk = [e.moments_get_angle(a, "C") for e in engs], [e.moments_get_angle(a, "S") for e in engs]
        C, S = _host_chains(Ck, Sk, counts, "pooled")
        got = {st: da.chains_get_angle(engs, a, st) for st in STATS + ("between",)}
        assert _same_bits(got["C"], C) and _same_bits(got["S"], S), (spec, "the pooled pair is not the list-order expression")
        _check_readouts(got, "chains %s %s" % (counts, spec))
        ref = _host_chains(Ck, Sk, counts, "between")
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got["between"]), nan), spec
        sq_got, sq_ref = got["between"][~nan] ** 2, ref[~nan] ** 2
        e = np.abs(sq_got - sq_ref) / (8 * U52 * (1 + sq_ref))
        print("chains %s %s between^2: worst error / (8 * 2^-52 (1 + ref)) = %.3g" % (counts, spec, float(e.max())))
        assert (e <= 1.0).all(), spec
        between_seen = between_seen or (got["between"][~nan] > 0).any()
        dv = da.chains_get_angle(engs, a, "between", device=True)
        engs[0].synchronize()
        assert _same_bits(dv.cpu().numpy(), got["between"])
    assert between_seen
    # the maps
    cm = da.chains_angle_maps(chains)
    assert list(cm) == [(engs[0].component_list[l].label, engs[0].bands[j].label) for l, j in C2_ANGLES]
    e = cm[list(cm)[2]]
    assert set(e) == {"n", "nchains", "psi", "psi_std", "R", "between"} and e["nchains"] == 3
    assert e["n"] == (counts[0] if len(set(counts)) == 1 else list(counts))
    assert _same_bits(e["between"], da.chains_get_angle(engs, 2, 5)) and _same_bits(e["psi"], da.chains_get_angle(engs, 2, 0))
    # a holder filled through the sections of family ANGLE gives the same bits; one that lacks the section is refused by name
    H = api._holder_engine(engs[1])
    H.moments_begin_like(engs[1])
    H.moments_section_put("HEAD", 0, 0, engs[1].moments_section_get("HEAD"))
    for a in range(len(C2_ANGLES) - 1):
        buf = engs[1].moments_section_get("ANGLE", a, 0, device=(a % 2 == 0))
        assert (buf.numel() if a % 2 == 0 else buf.size) == 2 * NPIX * 8
        engs[1].synchronize()
        H.moments_section_put("ANGLE", a, 0, buf)
        H.synchronize()
    assert H.moments_held_bytes() == (len(C2_ANGLES) - 1) * 2 * NPIX * 8
    held = [engs[0], H, engs[2]]
    for a in range(len(C2_ANGLES) - 1):
        for st in STATS + ("between",):
            assert _same_bits(da.chains_get_angle(held, a, st), da.chains_get_angle(engs, a, st)), (a, st)
    out = np.full(NPIX, 7.0)
    with pytest.raises(da.DangxError, match=r"chain 1: section ANGLE\(%d\) was not put into this holder" % (len(C2_ANGLES) - 1)):
        da.chains_get_angle(held, len(C2_ANGLES) - 1, "psi", out=out)
    assert (out == 7.0).all()
    with pytest.raises(da.DangxError, match="the stat of an angle must be"):
        da.chains_get_angle(engs, 0, 6)
    with pytest.raises(da.DangxError, match="chain 0: angle index out of range"):
        da.chains_get_angle(engs, len(C2_ANGLES), "psi")
    engs[2].moments_begin(None)
    engs[2].moments_angles(C2_ANGLES[1:])
    engs[2].moments_accumulate()
    with pytest.raises(da.DangxError, match="chain 2: angle 0 is not the registration of chain 0"):
        da.chains_get_angle(engs, 0, "psi")


# ---- 10. save / restore

def _saved_run():
    dev = torch.device("cuda", 0)
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device=dev, as_numpy=False)
    da.initialize(bands, comps, ddata, npix_global=meta["npix_global"], device=0)
    da.moments_begin(dpar, ddata)
    da.moments_signals(dpar, ddata)
    return dpar, ddata


def test_save_restore(built, tmp_path):
    dpar, A = _saved_run()
    da.moments_angles(dpar, A)
    for it in range(1, 6):
        da.gibbs_iteration(dpar, A, it)
        da.moments_accumulate(A)
    want = _all_maps(A.engine, 2)
    dpar, B = _saved_run()
    da.moments_angles(dpar, B)
    for it in range(1, 4):
        da.gibbs_iteration(dpar, B, it)
        da.moments_accumulate(B)
    path = str(tmp_path / "run.moments")
    da.moments_save(B, path)
    e = B.engine
    state = [(e.get_amplitude(l), e.get_indices(l) if c.nindices else None) for l, c in enumerate(e.component_list)]
    e.moments_end()
    dpar, R = _saved_run()
    da.moments_angles(dpar, R)
    for l, (a, x) in enumerate(state):
        R.engine.put_amplitude(l, a)
        if x is not None:
            R.engine.put_indices(l, x)
    da.moments_load(R, path)
    assert R.engine.moments_count() == 3
    for it in range(4, 6):
        da.gibbs_iteration(dpar, R, it)
        da.moments_accumulate(R)
    got = _all_maps(R.engine, 2)
    assert got.keys() == want.keys() and any((v[np.isfinite(v)] > 0).any() for k, v in want.items() if k[1] == "psi_std")
    for k in want:
        assert _same_bits(got[k], want[k]), k
    # an engine registered without the angles refuses the file, naming the group
    dpar, D = _saved_run()
    da.moments_accumulate(D)
    with pytest.raises(da.DangxError, match="signal or angle registrations differ"):
        da.moments_load(D, path)
    assert D.engine.moments_count() == 1
    # and a run without angles saves what it always saved: no ANGLE section, the HEAD's groups those of the same registration
    da.moments_save(D, path + ".plain")
    assert L.SEC_ANGLE not in [f for f, a, b in D.engine.moments_sections()]


# ---- 11. chains in two processes (gloo, one device): the launcher of test_gpu_sections.py, imported as it is

def _dist_worker(rank, world, port, out):
    import datetime
    import os
    import sys
    import torch.distributed as td
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    eng = _dist_chain(rank)
    td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    dc = da.dist_chains([[eng]], dst=0)
    m = da.chains_angle_maps(dc)
    assert (m is None) == (rank != 0)
    res = {"fetched": np.array([f for s, f, a, b, lag in dc.fetched])}
    if m is not None:
        res.update({repr((k, s)): v for k, e in m.items() for s, v in e.items() if isinstance(v, np.ndarray)})
    np.savez(out + ".%d.npz" % rank, **res)
    td.barrier()
    td.destroy_process_group()


def _dist_chain(k):
    case = make_case("C2", nside=4)
    dpar, ddata = case[0], case[1]
    dpar.seed = 8100 + k
    eng = tsig._engine(case)
    if k:
        tc._disperse(eng, 1)
    da.moments_begin(dpar, ddata)
    da.moments_angles(dpar, ddata)
    for it in range(1, 4 + k):                            # unequal counts: 3 and 4 samples
        da.gibbs_iteration(dpar, ddata, it)
        da.moments_accumulate(ddata)
    return eng


def test_two_processes(built, tmp_path):
    out = str(tmp_path / "res")
    tsec._spawn(_dist_worker, (2, tsec._free_port(), out), 2, 120)
    r0, r1 = (np.load(out + ".%d.npz" % r) for r in (0, 1))
    want = da.chains_angle_maps([[_dist_chain(0)], [_dist_chain(1)]])
    flat = {repr((k, s)): v for k, e in want.items() for s, v in e.items() if isinstance(v, np.ndarray)}
    assert len(flat) == 2 * 4 and sorted(k for k in r0.files if k != "fetched") == sorted(flat)
    for k, v in flat.items():
        assert _same_bits(r0[k], v), k
    assert r1.files == ["fetched"] and list(r0["fetched"]) == [L.SEC_ANGLE, L.SEC_ANGLE]      # one section per angle moved, nothing else
