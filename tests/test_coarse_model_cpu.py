"""The coarse-model switch (DANGX_COARSE_REFERENCE / DANGX_COARSE_DEGRADED) without a GPU: option validation of
DangComps.coarse_model and the new entry points in every layer (header, ctypes, Fortran module, shared library)."""
import ctypes
import os
import re

import pytest

import dang_amd as da
from dang_amd import _lib as L
from dang_amd.api import coarse_model_codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dangx_set_coarse_model", "dangx_coarse_model_size", "dangx_coarse_model_partials", "dangx_coarse_model_finish")


def _comp(**kw):
    return da.DangComps(label="dust", type="mbb", nu_ref=353.0, nindices=2, **kw)


def test_coarse_model_defaults_to_reference():
    assert coarse_model_codes(_comp()) == [L.COARSE_REFERENCE, L.COARSE_REFERENCE]
    assert coarse_model_codes(_comp(coarse_model=["degraded"])) == [L.COARSE_DEGRADED, L.COARSE_REFERENCE]
    assert coarse_model_codes(_comp(coarse_model=["reference", "degraded"])) == [L.COARSE_REFERENCE, L.COARSE_DEGRADED]
    assert coarse_model_codes(da.DangComps(label="cmb", type="cmb", nu_ref=100.0)) == []


@pytest.mark.parametrize("bad", [["Degraded"], ["fine"], [""], ["degraded", "reference", "degraded"]])
def test_unknown_or_surplus_coarse_models_raise(bad):
    with pytest.raises(da.DangxError):
        coarse_model_codes(_comp(coarse_model=bad))


def test_constants_agree_across_layers():
    h = open(os.path.join(ROOT, "include", "dangx.h")).read()
    assert re.search(r"DANGX_COARSE_REFERENCE\s*=\s*0\s*,\s*DANGX_COARSE_DEGRADED\s*=\s*1", h)
    f90 = open(os.path.join(ROOT, "fortran", "dangx_mod.f90")).read()
    assert re.search(r"DANGX_COARSE_REFERENCE\s*=\s*0\s*,\s*DANGX_COARSE_DEGRADED\s*=\s*1", f90)
    assert (L.COARSE_REFERENCE, L.COARSE_DEGRADED) == (0, 1)
    assert L.COARSE_MODEL_CODES == {"reference": 0, "degraded": 1}


def test_new_entry_points_are_declared_and_bound():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dangx.h")).read(), flags=re.S)
    f90 = open(os.path.join(ROOT, "fortran", "dangx_mod.f90")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, h), n
        assert n in L.SYMBOLS, n
        assert "name='%s'" % n in f90, n
    multi = open(os.path.join(ROOT, "fortran", "dangx_multi_mod.f90")).read()
    assert "dangx_coarse_model_partials" in multi and "dangx_coarse_model_finish" in multi


def test_library_exports_the_new_entry_points(built):
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), n


def test_bench_tool_takes_the_coarse_model_option():
    src = open(os.path.join(ROOT, "tools", "bench_coarse_iter.py")).read()
    assert '"--coarse-model", choices=("reference", "degraded"), default="reference"' in src
