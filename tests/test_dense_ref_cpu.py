"""The dense reference of tests/dense_ref.py and its checker are sound -- shown on the CPU before any kernel is judged by them
(tests/test_gpu_schur_values.py): the oracle's per-pixel direct solve lies within the bound of the dense solve on groups without
global members; on the template-group models the reference's own uncertainty is three orders below the bound and a plain float64
LAPACK solve stays under it; three errors a kernel or the host solve could make push the answer over the bound; schur_pivots
places the threshold pair on either side of device_schur's minpiv >= 1e-3 switch."""
import copy

import numpy as np
import pytest

from dang_amd import _lib as L

import dense_ref as D
import oracle_ffi as O
from test_oracle_templates_cpu import add_globals
from test_schur_host_cpu import host_solve, schur_exe  # noqa: F401  (schur_exe: the fixture that builds the stand-alone program)
from util import make_case

GLOBAL_TYPES = ("template", "monopole", "hi_fit")
SEED, STREAM = 8, 9

# name -> (config, members, group, flag, add_globals keywords as a function of the number of bands)
MODELS = {
    "a-C2": ("C2", ("template",), 2, L.FLAG_QU, lambda nb: dict(fit_bands=[nb - 2, nb - 1])),
    "a-C3": ("C3", ("template",), 2, L.FLAG_QU, lambda nb: dict(fit_bands=[nb - 2, nb - 1])),
    "b": ("C2", ("template",), 2, L.FLAG_QU, lambda nb: dict()),                     # 4 of 5 bands: ill-posed by design
    "c": ("C2", ("monopole",), 1, L.FLAG_T, lambda nb: dict(fit_bands=[0, nb - 2, nb - 1])),
    "d": ("C2", ("hi_fit",), 1, L.FLAG_T, lambda nb: dict(skip_band0=True)),
    "e": ("C2", ("monopole", "hi_fit"), 1, L.FLAG_T, lambda nb: dict(skip_band0=True)),
}
WELL_POSED = ("a-C2", "a-C3", "c", "d")    # the componentwise backward error of the GPU's x is asserted on these

# The threshold pair: model (a) on C2 whose template is alpha * (truth amplitude map of the polarised dust member, unit variance)
# + (1 - alpha) * noise.  The smallest pivot of the equilibrated Schur system is the part of a global row that the diffuse
# members do NOT absorb, a weighted mean over the pixels of a per-pixel figure that the bands' SED geometry and noise weights
# set: the blend moves it between 1.4e-2 (alpha = 1) and 1.7e-2 (alpha = 0) only.  What moves it across the switch is the weight
# of the fitted bands (a band of low noise is absorbed almost entirely by the pixel's own members), so the pair also scales the
# Q/U noise of the two fitted bands by `noise` -- rms map and the noise in the data alike.  Both figures were chosen with
# schur_pivots on the CPU; test_schur_pivots_of_the_threshold_pair holds them in place.
THRESHOLD_PAIR = {"skipped": dict(alpha=0.5, noise=0.15), "taken": dict(alpha=0.5, noise=0.02)}


def schur_case(name, nside=4):
    config, which, group, flag, kw = MODELS[name]

    def tweak(dpar, ddata, bands, comps):
        add_globals(dpar, ddata, bands, comps, which, group, **kw(ddata.sig_map.shape[0]))
    return make_case(config, nside=nside, start="truth", tweak=tweak), group, flag


def blend_case(alpha, noise, nside=4):
    def tweak(dpar, ddata, bands, comps):
        nb = ddata.sig_map.shape[0]
        fit = [nb - 2, nb - 1]
        dust = [c for c in comps if c.type == "mbb" and c.cg_group == 2][0]
        truth = np.array(dust.amplitude, dtype=np.float64, copy=True)
        _, res = O.Oracle(bands, comps, ddata).sky_model()          # data - sky model at the truth: the noise realisation
        for j in fit:
            ddata.sig_map[j, 1:, :] -= (1.0 - noise) * res[j, 1:, :]
            ddata.rms_map[j, 1:, :] *= noise
        add_globals(dpar, ddata, bands, comps, ("template",), 2, fit_bands=fit)
        c = comps[-1]
        old = c.template.copy()
        for k in (1, 2):
            c.template[k] = alpha * truth[k] / truth[k].std() + (1.0 - alpha) * old[k]
            ddata.sig_map[:, k, :] += c.truth_ta[k][:, None] * (c.template[k] - old[k])[None, :]
    return make_case("C2", nside=nside, start="truth", tweak=tweak), 2, L.FLAG_QU


def rows_case(nrows, nside=4):
    """A Q+U template group with `nrows` global rows: one template on the last `nrows` bands of C3 up to 8 rows (the models of
    tests/test_gpu_round4.py).  One template on 9 of C3's 10 bands beside four diffuse members is singular (smallest pivot 1e-15
    from schur_pivots), so 9 rows are two templates on the last 5 and 4 bands; 32 rows, the most one group holds, are four
    templates on the last eight bands of a 13-band C2."""
    split = {9: [5, 4], 32: [8, 8, 8, 8]}.get(nrows, [nrows])

    def tweak(dpar, ddata, bands, comps):
        nb = ddata.sig_map.shape[0]
        rng = np.random.default_rng(23)
        for t, nfit in enumerate(split):
            add_globals(dpar, ddata, bands, comps, ("template",), 2, fit_bands=list(range(nb - nfit, nb)))
            if len(split) > 1:
                c = comps[-1]                       # add_globals draws the same template every time: give each its own map
                new = c.template.copy()
                new[1], new[2] = rng.normal(0, 1, new.shape[1]), rng.normal(0, 1, new.shape[1])
                for k in (1, 2):
                    ddata.sig_map[:, k, :] += c.truth_ta[k][:, None] * (new[k] - c.template[k])[None, :]
                c.template, c.label = new, "tmpl%d" % t
    # 32 rows: pass 1 keeps (fitted bands x (members + 2) + rows) doubles per thread in LDS and refuses more than 150 KB per block
    # of 256 -- 8 x 6 + 32 = 80 > 75 beside C3's four members, 8 x 5 + 32 = 72 beside C2's three
    if nrows > 9:
        return make_case("C2", nside=nside, start="truth", tweak=tweak, nbands=13), 2, L.FLAG_QU
    return make_case("C3", nside=nside, start="truth", tweak=tweak), 2, L.FLAG_QU


def nglobal(comps, group):
    return sum(c.nfit for c in comps if c.type in GLOBAL_TYPES and c.cg_group == group)


_SYS, _REF = {}, {}


def reference(base, case, group, flag, ml_mode, ddata=None, tag=None, seed=SEED, stream=STREAM):
    """dict(A, b, live, x, last, bound, nrows) of the live sub-system of model `base` in one ml_mode; the matrix is built and
    inverted once per model, everything is computed once, shared by the tests and never modified.  ddata: other data than the
    case's (the perturbed data of the textbook fluctuation term), kept apart under `tag`."""
    key = (base, tag or ml_mode)
    if key not in _REF:
        dpar, dd, bands, comps, meta = case
        orc = O.Oracle(bands, copy.deepcopy(comps), dd if ddata is None else ddata)
        if (base, tag) not in _SYS:
            A = D.dense_matrix(orc, group, flag)
            live = np.flatnonzero(np.abs(A).sum(axis=1) > 0)
            A = np.ascontiguousarray(A[np.ix_(live, live)])
            _SYS.clear()                            # the inverse of the last model only: its modes are asked for together
            _SYS[(base, tag)] = (A, live, D.equilibrated_inverse(A))
        A, live, fact = _SYS[(base, tag)]
        b = D.dense_rhs(orc, group, flag, ml_mode, seed, stream)[live]
        x, last = D.solve_extended(A, b, fact=fact)
        r = dict(A=A, b=b, live=live, x=x, last=last, bound=D.forward_bound(A, x, b, D.EPS, fact=fact), nrows=nglobal(comps, group))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def worst_ratio(x, ref):
    """max over the live entries of |x - x_ref| / forward_bound"""
    return float((np.abs(np.asarray(x).astype(D.LD) - ref["x"]) / ref["bound"]).max())


# --------------------------------------------------------------------------- the reference against the oracle's direct solve

@pytest.mark.parametrize("ml_mode", ["optimize", "sample"])
@pytest.mark.parametrize("group,flag", [(1, L.FLAG_T), (2, L.FLAG_QU)])
def test_oracle_direct_solve_of_diffuse_groups_lies_within_the_bound(group, flag, ml_mode):
    case = make_case("C2", nside=4, start="truth")
    dpar, ddata, bands, comps, meta = case
    ref = reference(("diffuse", group), case, group, flag, ml_mode)
    orc = O.Oracle(bands, copy.deepcopy(comps), ddata)
    assert orc.amp_sample_direct(group, flag, ml_mode, SEED, STREAM, "reference") == 0
    x = D.packed_state((orc.amplitude, orc.template_amplitudes), comps, group, flag, meta["nbands"])[ref["live"]]
    w = worst_ratio(x, ref)
    print("oracle direct solve, group %d %s: worst error / bound %.2e" % (group, ml_mode, w))
    assert w <= 1.0


# --------------------------------------------------------------------------- the reference on the template-group models

@pytest.mark.parametrize("ml_mode", ["optimize", "sample"])
@pytest.mark.parametrize("name", list(MODELS))
def test_reference_uncertainty_is_far_below_the_bound(name, ml_mode):
    case, group, flag = schur_case(name)
    ref = reference(name, case, group, flag, ml_mode)
    own = float((ref["last"] / ref["bound"]).max())
    s, As = D._equilibrated(ref["A"])
    x64 = s * np.linalg.solve(As, s * ref["b"])
    w64 = worst_ratio(x64, ref)
    print("%s %s: n = %d, last correction / bound %.2e (%.1e of |x|), float64 solve error / bound %.2e, bound / |x| %.1e .. %.1e"
          % (name, ml_mode, ref["A"].shape[0], own, float((ref["last"] / np.abs(ref["x"])).max()), w64,
             float((ref["bound"] / np.abs(ref["x"])).min()), float((ref["bound"] / np.abs(ref["x"])).max())))
    assert own <= 1e-3
    assert w64 <= 1.0


# --------------------------------------------------------------------------- the checker notices what a wrong kernel would do

def _well_posed(ml_mode):
    case, group, flag = schur_case("a-C2")
    return case, group, flag, reference("a-C2", case, group, flag, ml_mode)


def test_checker_sees_one_band_of_one_pixel_block_scaled_by_1e_8():
    """A band tile applied with a factor 1 + 1e-8 to ONE (pixel, plane) block of the diffuse members."""
    case, group, flag, ref = _well_posed("optimize")
    dpar, ddata, bands, comps, meta = case
    npix, nb = meta["npix"], meta["nbands"]
    members = [c for c in comps if c.cg_group == group and c.type not in GLOBAL_TYPES]
    pix = int(np.flatnonzero(np.asarray(ddata.masks)[1] != 0)[7])
    band, plane = nb - 1, 1                                                          # Q of the last band
    full = np.array([m * 2 * npix + pix for m in range(len(members))])               # the block's unknowns, full layout
    idx = np.searchsorted(ref["live"], full)
    assert np.array_equal(ref["live"][idx], full)
    # the band's contribution to the block: the block minus the block without that band (its noise made infinite there)
    dd = copy.copy(ddata)
    dd.rms_map = np.array(ddata.rms_map, dtype=np.float64, copy=True)
    dd.rms_map[band, plane, pix] = 1e150
    without = O.Oracle(bands, copy.deepcopy(comps), dd)
    n = without.group_size(group, flag)
    part = np.zeros((len(full), len(full)))
    for q, k in enumerate(full):
        e = np.zeros(n)
        e[k] = 1.0
        part[:, q] = ref["A"][idx, idx[q]] - without.compute_Ax(group, flag, e)[full]
    assert np.abs(part).max() > 1e-3 * np.abs(ref["A"][np.ix_(idx, idx)]).max()      # the band does weigh in this block
    A = np.array(ref["A"])
    A[np.ix_(idx, idx)] += 1e-8 * part
    x, _ = D.solve_extended(A, ref["b"])
    w = worst_ratio(x, ref)
    print("one band of one block * (1 + 1e-8): worst error / bound %.2e" % w)
    assert w > 1.0


def test_checker_sees_a_fluctuation_term_on_the_neighbouring_global_row():
    case, group, flag, ref = _well_posed("sample")
    dpar, ddata, bands, comps, meta = case
    orc = O.Oracle(bands, copy.deepcopy(comps), ddata)
    v = orc.compute_sample_vector(group, flag, orc.draw_eta(flag, SEED, STREAM))[ref["live"]]
    n, R = ref["b"].size, ref["nrows"]
    assert R == 2 and v[n - R] != 0.0
    b = np.array(ref["b"])
    b[n - R] -= v[n - R]
    b[n - R + 1] += v[n - R]
    x, _ = D.solve_extended(ref["A"], b)
    w = worst_ratio(x, ref)
    print("fluctuation term of row 0 on row 1: worst error / bound %.2e" % w)
    assert w > 1.0


def host_lu(S, t, g0, diag, unscaled_row=None):
    """The generator of the mutant below, not the code under test: the host solve of device_schur (dang_amd/csrc/dx_schur_host.h,
    which tests/test_schur_host_cpu.py and the "whole" leg below run as it is) restated so that one step of it can be left out --
    the correction to g0 from the system equilibrated by the global block's diagonal, LU with complete pivoting, pivots below 1e-10
    left alone.  unscaled_row: that row of S misses its 1/sqrt(diag) -- the equilibration half applied.  Returns (g, rank)."""
    R = len(t)
    S = np.array(S, dtype=np.float64)
    sc = 1.0 / np.sqrt(np.abs(np.asarray(diag, dtype=np.float64)))
    res = np.asarray(t, dtype=np.float64) - S @ g0
    for r in range(R):
        S[r, :] *= (1.0 if r == unscaled_row else sc[r]) * sc
    rp, cp, rank = list(range(R)), list(range(R)), 0
    for c in range(R):
        sub = np.abs(S[c:, c:])
        pr, pc = np.unravel_index(int(np.argmax(sub)), sub.shape)
        if not sub[pr, pc] > 1e-10:
            break
        pr, pc = pr + c, pc + c
        S[[c, pr], :] = S[[pr, c], :]
        rp[c], rp[pr] = rp[pr], rp[c]
        S[:, [c, pc]] = S[:, [pc, c]]
        cp[c], cp[pc] = cp[pc], cp[c]
        for r in range(c + 1, R):
            f = S[r, c] / S[c, c]
            S[r, c] = f
            S[r, c + 1:] -= f * S[c, c + 1:]
        rank += 1
    y = np.array([res[rp[r]] * sc[rp[r]] for r in range(R)])
    for r in range(R):
        for k in range(min(r, rank)):
            y[r] -= S[r, k] * y[k]
    z = np.zeros(R)
    for r in range(rank - 1, -1, -1):
        z[r] = (y[r] - S[r, r + 1:rank] @ z[r + 1:rank]) / S[r, r]
    d = np.zeros(R)
    for r in range(rank):
        d[cp[r]] = z[r] * sc[cp[r]]
    return g0 + d, rank


def test_checker_sees_a_half_applied_equilibration_of_the_host_solve(schur_exe):
    """The host LU of dx_schur_host.h (the real code, in its stand-alone program) on the float64 Schur system, followed by the
    back-substitution, is within the bound; the restated solve with the equilibration of one row dropped from the matrix (but not
    from the right-hand side) is not.  The restated solve without the mutation is the real one to within the bound's share of
    every global row."""
    case, group, flag, ref = _well_posed("optimize")
    A, b, R = ref["A"], ref["b"], ref["nrows"]
    m = A.shape[0] - R
    X, _ = D.solve_extended(A[:m, :m], np.column_stack([A[:m, m:], b[:m]]))          # A11^-1 [A12 | b1]
    S = (A[m:, m:] - A[m:, :m].astype(D.LD) @ X[:, :R]).astype(np.float64)
    t = (b[m:] - A[m:, :m].astype(D.LD) @ X[:, R]).astype(np.float64)
    out = {}
    real, real_rank, _ = host_solve(schur_exe, S, t, np.zeros(R), np.diag(A)[m:])
    restated, restated_rank = host_lu(S, t, np.zeros(R), np.diag(A)[m:])
    assert restated_rank == real_rank
    assert (np.abs(restated - real) <= ref["bound"][m:].astype(np.float64)).all(), (restated, real)
    for which, (g, rank) in (("whole", (real, real_rank)), ("half", host_lu(S, t, np.zeros(R), np.diag(A)[m:], unscaled_row=1))):
        assert rank == R
        x = np.concatenate([(X[:, R] - X[:, :R] @ g.astype(D.LD)), g.astype(D.LD)])
        out[which] = worst_ratio(x, ref)
    print("host LU: worst error / bound %.2e; with row 1 unscaled in the matrix %.2e" % (out["whole"], out["half"]))
    assert out["whole"] <= 1.0
    assert out["half"] > 1.0


# --------------------------------------------------------------------------- the minpiv switch, seen from the CPU

def test_schur_pivots_of_the_threshold_pair():
    lo = {"skipped": (2e-3, 5e-3), "taken": (2e-4, 5e-4)}
    for which, kw in THRESHOLD_PAIR.items():
        case, group, flag = blend_case(**kw)
        ref = reference(("blend", which), case, group, flag, "optimize")
        piv = D.schur_pivots(ref["A"], ref["nrows"])
        print("threshold pair, %s: pivots %s" % (which, piv))
        assert lo[which][0] <= piv.min() <= lo[which][1]


def test_schur_pivots_against_a_hand_made_system():
    """A 2 x 2 diffuse block and two global rows whose pivots can be worked out by hand."""
    A = np.array([[2.0, 0.0, 1.0, 0.0], [0.0, 4.0, 0.0, 2.0], [1.0, 0.0, 1.0, 0.0], [0.0, 2.0, 0.0, 4.0]])
    # S = [[1 - 1/2, 0], [0, 4 - 1]] scaled by diag(1, 4): pivots 3/4 and 1/2
    assert np.allclose(D.schur_pivots(A, 2), [0.75, 0.5], rtol=1e-15, atol=0)
    x = np.array([1.0, -2.0, 3.0, 0.5])
    assert D.componentwise_backward_error(A, x, A @ x) == 0.0
    xs, last = D.solve_extended(A, A @ x)
    assert np.abs(xs - x).max() <= 1e-18 and last.max() <= 1e-15
    assert np.allclose(D.forward_bound(A, x, A @ x, 1e-10), 1e-10 * (np.abs(np.linalg.inv(A)) @ (np.abs(A) @ np.abs(x) + np.abs(A @ x))))
