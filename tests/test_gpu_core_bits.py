"""What dang_amd/csrc/dangx_core.hip and dangx_solve.hip answer outside the sweeps, against a record of the commit before the
solvers moved into their own translation unit and the bandpass sum, the solvers' prologue, the row read-back and the host scans
of the state setters were each written once: unit conversions, the host-evaluated SEDs of constant index maps, amp_residual,
the index and gain sums, schur_info and what the setters derive from the maps they are given must be the recorded BITS
(tests/golden/core_parent_bits.npz, written by record() below on the same device family).  The Schur and CG routes through the
sampling entry points are held by tests/test_gpu_entry_routes.py."""
import copy
import os

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L

from test_gpu_entry_routes import _bandpass, _monopole, _template
from test_oracle_templates_cpu import add_globals
from util import make_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "core_parent_bits.npz")
SEED = 11


def _engine(case):
    dpar, ddata, bands, comps, meta = case
    return da.Engine(bands, copy.deepcopy(comps), ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)


def _state(e, out, tag):
    for l, c in enumerate(e.component_list):
        out["%s_amp%d" % (tag, l)] = e.get_amplitude(l)
        if c.type in ("template", "monopole", "hi_fit"):
            out["%s_tamp%d" % (tag, l)] = e.get_template_amplitudes(l)


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


@case
def unit_conversions():
    """C3 with every second band bandpass-integrated, one of its samples at nu0 == 0: delta and bandpass bands, all selectors"""
    c = make_case("C3", nside=2, start="truth", tweak=_bandpass)
    assert any(b.id == "bp" and (np.asarray(b.nu0) == 0.0).any() for b in c[2]) and any(b.id != "bp" for b in c[2])
    e = _engine(c)
    return {w: np.array([e.unit_conversion(j, w) for j in range(e.nbands)]) for w in ("a2t", "a2f", "f2t")}


@case
def constant_index_seds():
    """the same model after put_indices with spatially constant maps: sync_model evaluates every SED on the host (csed), the
    tau0-weighted sum on the bandpass bands -- cmb, power-law, mbb and free-free"""
    c = make_case("C3", nside=2, start="truth", tweak=_bandpass)
    e = _engine(c)
    out = {}
    assert {cc.type for cc in e.component_list} >= {"cmb", "power-law", "mbb", "freefree"}
    for l, cc in enumerate(e.component_list):
        if cc.nindices:
            x = np.array(e.get_indices(l))
            for q in range(cc.nindices):
                for k in range(e.nmaps):
                    x[q, k, :] = x[q, k, 0] * (1.0 + 0.01 * (k + 1) + 0.003 * q)
            e.put_indices(l, x)
        out["sed%d" % l] = np.array([[e.eval_sed(l, j, k) for k in range(1, e.nmaps + 1)] for j in range(e.nbands)])
    return out


def _residuals(c, group, flag, info=False):
    out = {}
    for mode in ("sample", "optimize"):
        e = _engine(c)
        before = e.amp_residual(group, flag, mode, SEED, 5)
        ret = e.amp_sample(group, flag, mode, SEED, 5)
        after = e.amp_residual(group, flag, mode, SEED, 5)
        out[mode] = np.array(list(before) + list(after) + [float(v) for v in ret] + [float(e.group_size(group, flag))])
        if info:
            (rb, rw), n = e.schur_info()
            out[mode + "_info"] = np.array([rb, rw, float(n)])
        _state(e, out, mode)
    return out


@case
def residual_diffuse():
    """C2 from the prior, the T and the Q+U group: amp_residual before and after a solve, both modes"""
    c = make_case("C2", nside=2, start="prior")
    out = {}
    for group, flag in ((1, L.FLAG_T), (2, L.FLAG_QU)):
        out.update({"g%d_%s" % (group, k): v for k, v in _residuals(c, group, flag).items()})
    return out


@case
def residual_template():
    """C2 + Q/U template at nside 4 (more than one block): the mixed operators in amp_residual, schur_info after the solve; the T
    group beside the template's zero T plane"""
    c = make_case("C2", nside=4, start="truth", tweak=_template)
    out = _residuals(c, 2, L.FLAG_QU, info=True)
    out.update({"T_" + k: v for k, v in _residuals(c, 1, L.FLAG_T).items()})
    return out


@case
def residual_monopole():
    """C2 + monopole in the T group: the measured residual of the global rows (no a-priori bound for a monopole), schur_info"""
    return _residuals(make_case("C2", nside=2, start="truth", tweak=_monopole), 1, L.FLAG_T, info=True)


@case
def residual_monopole_hi_fit():
    """C2 + monopole and hi_fit in the T group (eight global rows of very different sizes), from the prior: the equilibration, and the
    refinement loop from a state far from the solution"""
    def both(dpar, ddata, bands, comps):
        add_globals(dpar, ddata, bands, comps, ("monopole", "hi_fit"), 1, skip_band0=True)
    return _residuals(make_case("C2", nside=2, start="prior", tweak=both), 1, L.FLAG_T, info=True)


@case
def masked_sums():
    """C3 at nside 4 (192 pixels, the masked band inside): index_masked_sum, index_plain_sum and gain_sums"""
    c = make_case("C3", nside=4, start="truth")
    assert (np.asarray(c[1].masks)[0] == 0).any()
    e = _engine(c)
    ms, ps = [], []
    for l, cc in enumerate(e.component_list):
        for q in range(cc.nindices):
            for k in range(1, e.nmaps + 1):
                ms += [float(v) for v in e.index_masked_sum(l, q, k)]
                ps += list(e.index_plain_sum(l, q, k))
    return {"masked": np.array(ms), "plain": np.array(ps), "gain": np.array([e.gain_sums(j) for j in range(e.nbands)])}


@case
def derived_plane_bits():
    """what the setters derive from their maps, through its effect: the T solve beside polarised members whose T plane is all zero
    (skipped) and then holds one non-zero pixel (part of the model); a Q+U solve after put_indices with the Q plane constant and
    the U plane not; a template with a signal on T beside the T group"""
    c = make_case("C2", nside=2, start="truth")
    e = _engine(c)
    out = {"size": np.array([float(e.group_size(1, L.FLAG_T)), float(e.group_size(2, L.FLAG_QU))])}
    e.amp_sample(1, L.FLAG_T, "sample", SEED, 3)
    _state(e, out, "zero")
    a = np.array(e.get_amplitude(4))
    a[0, -1] = 2.5
    e.put_amplitude(4, a)
    e.amp_sample(1, L.FLAG_T, "sample", SEED, 3)
    _state(e, out, "one_pixel")
    x = np.array(e.get_indices(5))
    x[:, 1, :] = x[:, 1, :1]
    x[0, 2, 1] += 0.01
    e.put_indices(5, x)
    out["sed_q"] = np.array([e.eval_sed(5, j, 2) for j in range(e.nbands)])
    out["sed_u"] = np.array([e.eval_sed(5, j, 3) for j in range(e.nbands)])
    e.amp_sample(2, L.FLAG_QU, "sample", SEED, 4)
    _state(e, out, "q_constant")

    def t_signal(dpar, ddata, bands, comps):
        _template(dpar, ddata, bands, comps)
        t = np.array(comps[-1].template)
        t[0] = 0.5 * t[1]
        comps[-1].template = t
        ta = np.array(comps[-1].template_amplitudes if comps[-1].template_amplitudes is not None else np.zeros((3, len(bands))))
        ta[0] = 0.25
        comps[-1].template_amplitudes = ta
    e = _engine(make_case("C2", nside=2, start="truth", tweak=t_signal))
    e.amp_sample(1, L.FLAG_T, "sample", SEED, 3)
    _state(e, out, "template_on_T")
    return out


def run_case(name):
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in CASES[name]().items()}


def record(path):
    """writes the fixture from the build that is loaded (run once, on the parent commit)"""
    arrays = {}
    for name in CASES:
        for k, v in run_case(name).items():
            arrays[name + "/" + k] = v
    np.savez_compressed(path, **arrays)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_has_every_case(golden):
    assert sorted({k.split("/", 1)[0] for k in golden}) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_core_bits_are_the_parents(built, golden, name):
    out = run_case(name)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(name + "/"))
    assert keys == sorted(out), (keys, sorted(out))
    for k in keys:
        want, got = golden[name + "/" + k], out[k]
        assert want.shape == got.shape and want.dtype == got.dtype, (name, k, want.shape, got.shape)
        ne = int(np.count_nonzero(want.view(np.int64) != got.view(np.int64)))
        print("%s/%s: %d of %d values differ in their bits" % (name, k, ne, want.size))
        assert ne == 0, (name, k, ne)
