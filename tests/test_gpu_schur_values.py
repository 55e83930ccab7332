"""VALUES of the direct (Schur complement) solve of CG groups with template / monopole / hi_fit members against the dense,
extended-precision solve of the oracle's system (tests/dense_ref.py; shown sound on the CPU in tests/test_dense_ref_cpu.py).

The assertion is the same on every route: from start="truth", the engine's state packed like initialize_x lies within
forward_bound = EPS * |A^-1| (|A||x| + |b|) of the reference ELEMENTWISE on the live entries, global rows included; no unit was
not positive definite and the nullity is 0.  EPS = 2 * TOL_SED + 64 ulp is derived in dense_ref.py; no tolerance here is tuned.
The componentwise backward error of the GPU's x is printed on every route and held to EPS on the well-posed models.

Routes: amp_sample as built; the run-time-typed passes (DANGX_SCHUR_FAST=0) and the per-plane pass 1 (DANGX_SCHUR_QU=0), both
read once and therefore run in a child process; plane_set_sample with the group's sweeps (deferred back-substitution);
sky_plane_set_sample over three unequal shards; the textbook fluctuation term; 2 to 32 global rows; and both sides of
device_schur's minpiv >= 1e-3 switch.  Nothing is compared with another GPU route."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L

import dense_ref as D
from fluct_helpers import perturbed_data
from test_dense_ref_cpu import (MODELS, SEED, STREAM, THRESHOLD_PAIR, WELL_POSED, blend_case, reference, rows_case, schur_case,
                                worst_ratio)
from util import shard_engines

pytestmark = pytest.mark.gpu

ML_MODES = ("optimize", "sample")
SHARD_BOUNDS = (0, 37, 101, 192)          # Nside 4: three unequal shards, no boundary a multiple of 64
# quoted from device_schur (dang_amd/csrc/dangx_solve.hip): the switch on the smallest pivot, and the residual it promises
MINPIV_SWITCH, SKIP_RESIDUAL = 1e-3, 1e-12


def _sweeps(comps, group, flag, it=2):
    return [(l, j, da.stream_id(it, 1, l, j, flag)) for l, c in enumerate(comps) for j in range(c.nindices)
            if c.cg_group == group and c.sample_index[j] and flag in c.pol_flag[j]]


def _engine(case, ddata=None):
    dpar, dd, bands, comps, meta = case
    return da.Engine(bands, copy.deepcopy(comps), dd if ddata is None else ddata, npix_global=meta["npix_global"], pix0=meta["pix0"],
                     device=0)


def _plane_set(eng, group, flag, ml_mode, sweeps, nsample, seed_index, fluct_mode):
    """Engine.plane_set_sample, with the nullity the entry point reports through cg_iters (the method does not ask for it)."""
    comp = np.ascontiguousarray([s[0] for s in sweeps], dtype=np.int32)
    nind = np.ascontiguousarray([s[1] for s in sweeps], dtype=np.int32)
    strm = np.ascontiguousarray([s[2] for s in sweeps], dtype=np.uint64)
    it, bad, acc = C.c_int(0), C.c_int64(0), np.zeros(max(len(sweeps), 1), dtype=np.int64)
    eng._chk(eng.lib.dangx_plane_set_sample(
        eng.h, group, flag, L.ML_CODES[ml_mode], L.SOLVER_DIRECT, L.FLUCT_REFERENCE if fluct_mode == "reference" else L.FLUCT_CORRECT,
        SEED, STREAM, 100, 1e-8, len(sweeps), comp.ctypes.data, nind.ctypes.data, strm.ctypes.data, nsample, seed_index,
        C.byref(it), C.byref(bad), acc.ctypes.data))
    return it.value, bad.value


def run_route(route, case, group, flag, ml_mode, fluct_mode="reference"):
    """One solve on fresh engines.  dict(xs = packed states (one per context: they share the diffuse maps' concatenation and carry
    their own copy of the global amplitudes), bad, nullity, resid, backward, steps, kernels = the names the profile of each
    context saw)."""
    dpar, ddata, bands, comps, meta = case
    nb = meta["nbands"]
    if route == "sky3":
        assert meta["npix"] == SHARD_BOUNDS[-1]
        engs = shard_engines(case, 3, bounds=SHARD_BOUNDS)
        for e in engs:
            e.profile(True)
        nul, bad, _ = da.sky_plane_set_sample(engs, group, flag, ml_mode, SEED, STREAM, _sweeps(comps, group, flag), dpar.nsample,
                                              dpar.seed, fluct_mode=fluct_mode)
        whole = lambda l: np.concatenate([e.get_amplitude(l) for e in engs], axis=1)
        xs = [D.packed_state((whole, e.get_template_amplitudes), comps, group, flag, nb) for e in engs]
    else:
        engs = [_engine(case)]
        engs[0].profile(True)
        if route == "amp":
            nul, bad = engs[0].amp_sample(group, flag, ml_mode, SEED, STREAM, solver="direct", fluct_mode=fluct_mode)
        else:
            assert route == "plane_set"
            nul, bad = _plane_set(engs[0], group, flag, ml_mode, _sweeps(comps, group, flag), dpar.nsample, dpar.seed, fluct_mode)
        xs = [D.packed_state((engs[0].get_amplitude, engs[0].get_template_amplitudes), comps, group, flag, nb)]
    (resid, backward), steps = engs[0].schur_info()
    kernels = [sorted(e.profile_get()) for e in engs]
    return dict(xs=[x.tolist() for x in xs], bad=int(bad), nullity=int(nul), resid=resid, backward=backward, steps=int(steps),
                kernels=kernels)


def check(what, out, ref, assert_backward):
    """The assertion of this file.  Prints the worst error / bound and the componentwise backward error, returns the former."""
    assert out["bad"] == 0 and out["nullity"] == 0, (what, out["bad"], out["nullity"])
    worst = 0.0
    for q, x in enumerate(out["xs"]):
        x = np.asarray(x, dtype=np.float64)[ref["live"]]
        assert x.size == ref["b"].size and np.isfinite(x).all(), what
        w = worst_ratio(x, ref)
        cbe = D.componentwise_backward_error(ref["A"], x, ref["b"])
        err = np.abs(x.astype(D.LD) - ref["x"]) / ref["bound"]
        R = ref["nrows"]
        print("%s%s: worst error / bound %.3e (global rows %.3e), componentwise backward error %.2e (EPS %.2e), reported residual %.1e, "
              "%d refinement steps" % (what, " context %d" % q if len(out["xs"]) > 1 else "", w, float(err[-R:].max()), cbe, D.EPS,
                                       out["resid"], out["steps"]))
        assert w <= 1.0, (what, q, w, int(np.argmax(err)), x.size)
        if assert_backward:
            assert cbe <= D.EPS, (what, q, cbe)
        worst = max(worst, w)
    print("%s: kernels launched %s" % (what, ", ".join(out["kernels"][0])))
    return worst


def _model(name):
    case, group, flag = schur_case(name)
    return case, group, flag, {ml: reference(name, case, group, flag, ml) for ml in ML_MODES}


# --------------------------------------------------------------------------- routes 1, 3, 4: one process, switches as built

@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("route", ["amp", "plane_set", "sky3"])
def test_schur_solve_values(built, route, name):
    case, group, flag, refs = _model(name)
    for ml in ML_MODES:
        out = run_route(route, case, group, flag, ml)
        check("%s %s %s" % (route, name, ml), out, refs[ml], name in WELL_POSED)
        if route != "amp" and name in ("a-C2", "a-C3"):
            # the route under test here is the DEFERRED back-substitution: the launch that does the sweeps solved the pixel blocks
            # on the data minus the templates' new signal, no stand-alone pass 2 ran (cf. tests/test_gpu_round4.py)
            for k in out["kernels"]:
                assert "k_amp_index" in k and "k_amp_direct" not in k and "k_index_mh" not in k, k


# --------------------------------------------------------------------------- route 2: the switches that are read once

_CHILD = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
          "import test_gpu_schur_values as t\n"
          "case, group, flag = t.schur_case(%r)\n"
          "print('RESULT ' + json.dumps({ml: t.run_route('amp', case, group, flag, ml) for ml in t.ML_MODES}))\n")


@pytest.mark.parametrize("switch,name", [("DANGX_SCHUR_FAST", n) for n in MODELS] + [("DANGX_SCHUR_QU", "a-C2"), ("DANGX_SCHUR_QU", "a-C3")])
def test_schur_solve_values_with_a_switch_off(built, switch, name):
    """DANGX_SCHUR_FAST=0: the run-time-typed passes of dangx_schur.hip; DANGX_SCHUR_QU=0: pass 1 per plane instead of
    k_schur_pass1_qu.  Both are read once per process (diagnostic switches): a fresh child process, whose state comes
    back as JSON (repr round-trips a double) and is judged here against the same reference."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    case, group, flag, refs = _model(name)
    r = subprocess.run([sys.executable, "-c", _CHILD % (root, os.path.join(root, "tests"), name)], env=dict(os.environ, **{switch: "0"}),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and lines, r.stdout[-3000:]
    out = json.loads(lines[-1][7:])
    for ml in ML_MODES:
        check("%s=0 %s %s" % (switch, name, ml), out[ml], refs[ml], name in WELL_POSED)


# --------------------------------------------------------------------------- route 5: the textbook fluctuation term

@pytest.mark.parametrize("name", ["a-C2", "a-C3"])
@pytest.mark.parametrize("route", ["amp", "plane_set", "sky3"])
def test_textbook_fluctuation_term_values(built, route, name):
    """fluct_mode='correct' is the OPTIMIZE solve on d + sigma * eta (fluct_helpers): the reference is the dense system of an
    oracle built on those data."""
    case, group, flag = schur_case(name)
    dpar, ddata, bands, comps, meta = case
    ref = reference(name, case, group, flag, "optimize", ddata=perturbed_data(ddata, [(flag, STREAM)], SEED, meta["pix0"]), tag="correct")
    check("%s %s correct" % (route, name), run_route(route, case, group, flag, "sample", fluct_mode="correct"), ref, True)


def test_textbook_term_stays_refused_on_the_other_models(built):
    for name in ("c", "d", "e"):
        case, group, flag = schur_case(name)
        with pytest.raises(da.DangxError):
            _engine(case).amp_sample(group, flag, "sample", SEED, STREAM, fluct_mode="correct")


# --------------------------------------------------------------------------- route 6: row counts

@pytest.mark.parametrize("nrows", [2, 5, 6, 8, 9, 32])
def test_row_counts_values(built, nrows):
    """2, 5, 6, 8: k_schur_pass1_qu (beyond five rows the row values are reduced row by row); 9: the first count past its limit;
    32: DX_MAX_ROWS, four templates on 13 bands (beside three diffuse members: what pass 1's LDS budget admits)."""
    case, group, flag = rows_case(nrows)
    for ml in ML_MODES:
        ref = reference(("rows", nrows), case, group, flag, ml)
        assert ref["nrows"] == nrows
        check("amp %d rows %s" % (nrows, ml), run_route("amp", case, group, flag, ml), ref, False)


# --------------------------------------------------------------------------- the minpiv switch

@pytest.mark.parametrize("which", list(THRESHOLD_PAIR))
def test_both_sides_of_the_minpiv_switch(built, which, monkeypatch):
    """The pair of tests/test_dense_ref_cpu.py: smallest pivot about 3e-3 (residual pass skipped: the a-priori figure is reported
    as the residual, with 0 steps) and about 3e-4 (pass taken).  The values hold on both sides; on the skipped side a second engine
    under DANGX_SCHUR_CHECK=1 (read at call time) MEASURES a residual no larger than the a-priori figure and than the 1e-12 the
    skip promises, and if it took no refinement step its amplitudes are the first engine's bit for bit."""
    case, group, flag = blend_case(**THRESHOLD_PAIR[which])
    dpar, ddata, bands, comps, meta = case
    monkeypatch.setenv("DANGX_SCHUR_CHECK", "0")
    for ml in ML_MODES:
        ref = reference(("blend", which), case, group, flag, ml)
        minpiv = D.schur_pivots(ref["A"], ref["nrows"]).min()
        out = run_route("amp", case, group, flag, ml)
        print("%s %s: smallest pivot %.3e from the CPU" % (which, ml, minpiv))
        check("amp threshold %s %s" % (which, ml), out, ref, True)
        if which == "skipped":
            assert minpiv >= MINPIV_SWITCH
            assert out["steps"] == 0 and out["resid"] == out["backward"]         # the a-priori figure, reported as both
            monkeypatch.setenv("DANGX_SCHUR_CHECK", "1")
            chk = run_route("amp", case, group, flag, ml)
            monkeypatch.setenv("DANGX_SCHUR_CHECK", "0")
            print("%s %s: a-priori figure %.3e (16 R eps / minpiv of the CPU's pivot: %.3e), measured residual %.3e (%d steps)"
                  % (which, ml, out["resid"], 16.0 * ref["nrows"] * np.finfo(float).eps / minpiv, chk["resid"], chk["steps"]))
            check("amp threshold %s %s, residual measured" % (which, ml), chk, ref, True)
            assert chk["resid"] <= out["resid"] and chk["resid"] <= SKIP_RESIDUAL, (chk["resid"], out["resid"])
            if chk["steps"] == 0:
                assert chk["xs"] == out["xs"]
        else:
            assert minpiv < MINPIV_SWITCH
            assert out["resid"] != out["backward"]      # measured: relative to b and relative to the row's terms, two figures
