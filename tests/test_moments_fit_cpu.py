"""Posterior goodness-of-fit maps, host side: the default item list of what a run samples, posterior_fit_maps' assembly on host
arrays, the fingerprint of a registration without fit items (unchanged: constants recorded from the section layer as it was
before fit items existed) and dang_amd/csrc/dx_fit_host.h -- the check of an item list, the segment plan and the rounded
expressions of a sample -- as a stand-alone program under the address and undefined-behaviour sanitizers.  No device needed;
nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, CHI = 0, 1


def test_default_items_of_a_c3_shaped_model():
    """C3: a T group and a Q+U group, 10 bands: per plane the chi^2 map, then every band's residual -- 33 items"""
    dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=1)
    specs = da.default_fit_specs(dpar, comps, bands)
    want = [(1, -1, 0), (0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0), (0, 5, 0), (0, 6, 0), (0, 7, 0), (0, 8, 0), (0, 9, 0),
            (1, -1, 1), (0, 0, 1), (0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (0, 5, 1), (0, 6, 1), (0, 7, 1), (0, 8, 1), (0, 9, 1),
            (1, -1, 2), (0, 0, 2), (0, 1, 2), (0, 2, 2), (0, 3, 2), (0, 4, 2), (0, 5, 2), (0, 6, 2), (0, 7, 2), (0, 8, 2), (0, 9, 2)]
    assert specs == want and len(specs) == 33 <= L.MAX_FIT == 128
    dpar.cg_groups[1].pol_flag = [L.FLAG_Q]                              # the Q+U group solves Q alone: no U plane
    assert da.default_fit_specs(dpar, comps, bands) == want[:22]
    for c in comps:
        if c.cg_group == dpar.cg_groups[0].cg_group:
            c.sample_amplitude = False                                   # nothing sampled in the T group: its plane drops out
    assert da.default_fit_specs(dpar, comps, bands) == want[11:22]
    dpar.cg_groups[1].pol_flag = [L.FLAG_U, L.FLAG_Q]
    assert da.default_fit_specs(dpar, comps, bands) == want[11:]
    # a flag that names a plane the model lacks adds nothing: the list is bounded by nmaps, as the Fortran wrapper's is
    assert da.default_fit_specs(dpar, comps, bands, nmaps=2) == want[11:22] and da.default_fit_specs(dpar, comps, bands, nmaps=1) == []


def test_default_items_of_a_c5_shaped_model():
    dpar, ddata, bands, comps, meta = synth.make_sky("C5", nside=1)
    specs = da.default_fit_specs(dpar, comps, bands)
    want = []
    for k in (0, 1, 2):
        want.append((CHI, -1, k))
        want += [(RES, j, k) for j in range(20)]
    assert specs == want and len(specs) == 63 and specs[0] == (1, -1, 0) and specs[21] == (1, -1, 1) and specs[62] == (0, 19, 2)
    assert len({s for s in specs}) == 63


def test_the_python_layer_names_the_new_family_and_codes():
    assert L.SEC_FIT == 8 and L.SECTION_NAMES_ALL[L.SEC_FIT] == "FIT" and L.SECTION_NAMES_ALL[:8] == L.SECTION_NAMES
    assert L.K_FIT == 13 and L.KERNEL_NAMES[L.K_FIT] == "k_fit" and len(L.KERNEL_NAMES) == 14
    assert L.FIT_KINDS == ("residual", "chisq") and L.MAX_FIT == 128
    from dang_amd import api, posterior
    assert "_moment_fit" in api.MOMENT_ATTRS
    assert api._sec_family("FIT") == 8 and api._sec_family("ANGLE") == 7
    for name in ("default_fit_specs", "moments_fit", "posterior_fit_maps", "chains_get_fit", "chains_fit_maps"):
        assert name not in posterior.__all__ and getattr(da, name) is getattr(posterior, name)
    assert posterior.FAMILIES["fit"].reg == "fit" and posterior.FAMILIES["fit"] is posterior.FIT
    assert api.fit_spec(("residual", 3, "Q")) == (0, 3, 1) and api.fit_spec(("chisq", "U")) == (1, -1, 2) and api.fit_spec((1, -1, 0)) == (1, -1, 0)
    for sym in ("dangx_moments_fit", "dangx_moments_get_fit", "dangx_moments_get_fit_dev", "dangx_chains_get_fit", "dangx_chains_get_fit_dev"):
        assert sym in L.SYMBOLS


class _FakeEngine:
    """What posterior_fit_maps and Engine.moments_sections read of an Engine, over host arrays: one shard."""

    def __init__(self, comps, bands, masks, maps, reg, count=5):
        self.component_list, self.bands, self.ddata = comps, bands, da.DangData(sig_map=None, rms_map=None, masks=masks)
        self._maps, self._moment_fit, self._count = maps, reg, count
        self.ddofs = []

    def moments_count(self):
        return self._count

    def moments_get_fit(self, i, stat, ddof):
        self.ddofs.append(ddof)
        return self._maps[stat][i].copy()


def test_posterior_fit_maps_fill_and_assembly_on_host_arrays():
    rng = np.random.default_rng(12)
    comps = [da.DangComps(label="synch", type="power-law", nu_ref=30.0, nindices=1, ind_label=["beta"])]
    bands = [da.BandInfo(label="bp_030", nu_c=30.0), da.BandInfo(label="bp_044", nu_c=44.0)]
    reg = [(RES, 1, 0), (CHI, -1, 2), (RES, 0, 1)]

    def shard(npix, masked):
        masks = np.ones((3, npix))
        masks[0, masked] = 0.0
        maps = {st: [rng.uniform(0, 1, npix) for _ in reg] for st in ("mean", "std")}
        return _FakeEngine(comps, bands, masks, maps, list(reg))
    engs = [shard(5, [1]), shard(4, [0, 3])]
    plain = da.posterior_fit_maps(None, ddof=1, engines=engs)
    keys = [("residual", "bp_044", "T"), ("chisq", "U"), ("residual", "bp_030", "Q")]
    assert list(plain) == keys
    for i, key in enumerate(keys):
        assert set(plain[key]) == {"n", "mean", "std"} and plain[key]["n"] == 5
        for st in ("mean", "std"):
            assert np.array_equal(plain[key][st], np.concatenate([e._maps[st][i] for e in engs]))
    assert set(engs[0].ddofs) == {1}
    filled = da.posterior_fit_maps(None, masked_value=-1.6375e30, engines=engs)
    masked = np.zeros(9, dtype=bool)
    masked[[1, 5, 8]] = True
    for key in keys:
        assert (filled[key]["std"][masked] == -1.6375e30).all() and np.array_equal(filled[key]["std"][~masked], plain[key]["std"][~masked])
    # the sections the items own, behind every other family's; a registration without items owns none
    from dang_amd.posterior import own_sections
    engs[0]._moment_sel = np.zeros(1, dtype=np.int32)
    assert own_sections(engs[0]) == [(L.SEC_FIT, 0, 0), (L.SEC_FIT, 1, 0), (L.SEC_FIT, 2, 0)]
    engs[0]._moment_angles = [(0, 1)]
    assert own_sections(engs[0]) == [(L.SEC_ANGLE, 0, 0), (L.SEC_FIT, 0, 0), (L.SEC_FIT, 1, 0), (L.SEC_FIT, 2, 0)]
    engs[0]._moment_fit = []
    assert own_sections(engs[0]) == [(L.SEC_ANGLE, 0, 0)]
    engs[0]._moment_fit = list(reg)
    engs[1]._moment_fit = reg[:1]
    with pytest.raises(da.DangxError, match="different fit registrations"):
        da.posterior_fit_maps(None, engines=engs)
    engs[1]._moment_fit = list(reg)
    engs[1]._count = 6
    with pytest.raises(da.DangxError, match="different sample counts"):
        da.posterior_fit_maps(None, engines=engs)
    engs[0]._moment_fit = None
    with pytest.raises(da.DangxError, match="moments_fit was not called"):
        da.posterior_fit_maps(None, engines=engs)
    # the words of head_diff for the group the fit items are hashed into
    from dang_amd.posterior import head_diff
    own = {"lag1": 0, "nbatch": 0, "groups": (1, 2, 3, 4, 5, 6), "fingerprint": 7}
    got = dict(own, groups=(1, 2, 3, 4, 9, 6))
    assert head_diff(got, own) == "the fit items, signal or angle registrations differ" and head_diff(own, own) == ""


HOST_MAIN = r"""
#include "dx_fit_host.h"
#include "dx_section_host.h"
#include <cmath>
#include <cstdio>
#include <limits>
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool has(const std::string& s, const char* w) { return s.find(w) != std::string::npos; }

// the registration of tests/test_sections_cpu.py's base case (v = 0), of its variant 14 (another signal spec), with two angles
// (v = 2) and without signals (v = 3)
static DxSecReg reg(int v) {
    DxSecReg r;
    r.npix = 95; r.pix0 = 1; r.nmaps = 3;
    r.sel = {0x1ff, 0, 7}; r.type = {2, 3, 8}; r.nind = {2, 1, 0};
    r.lag1 = 1;
    r.pairs = {0, 0, 0, 0, 1, 1};
    r.hist_planes = {0, 1, 1, 0, 0, 0};
    r.hist_range = {1.0, 2.0, -5.0, 5.0};
    r.nbins = 16; r.bits = 16;
    r.signals = {0, 1, v == 14 ? 1 : 0, 0, 0, 3};
    r.batch_planes = {0, 0, 0};
    r.nbatch = 4;
    if (v == 2) r.angles = {0, 1, 0, 2};
    if (v == 3) r.signals.clear();
    return r;
}

int main() {
    const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
    // ---- the check: 5 bands
    auto chk = [&](const std::vector<int32_t>& sp, int nmaps = 3) { return dx_fit_check((int)(sp.size() / 3), sp.data(), 5, nmaps); };
    CHECK(chk({0, 0, 0, 1, -1, 0, 0, 4, 2, 1, -1, 2}).empty());
    CHECK(dx_fit_check(0, nullptr, 5, 3).empty() && dx_fit_check(0, nullptr, 5, 1).empty());
    CHECK(has(dx_fit_check(1, nullptr, 5, 3), "no fit item list"));
    CHECK(has(dx_fit_check(-1, nullptr, 5, 3), "negative"));
    CHECK(has(chk({2, 0, 0}), "fit item 0: what must be") && has(chk({0, 0, 0, -1, 0, 0}), "fit item 1: what must be"));
    CHECK(has(chk({0, 5, 0}), "fit item 0: band index") && has(chk({0, -1, 0}), "fit item 0: band index"));
    CHECK(has(chk({0, 0, 3}), "plane must be") && has(chk({1, -1, -1}), "plane must be"));
    CHECK(has(chk({1, 0, 0}), "band must be -1") && has(chk({1, 5, 0}), "band must be -1"));
    CHECK(has(chk({0, 0, 1}, 1), "a plane the model does not have") && has(chk({1, -1, 2}, 2), "a plane the model does not have"));
    CHECK(chk({0, 0, 0, 1, -1, 0}, 1).empty());
    CHECK(has(chk({0, 1, 1, 1, -1, 1, 0, 1, 1}), "fit item 2: the same fit item twice"));
    CHECK(has(chk({1, -1, 1, 1, -1, 1}), "fit item 1: the same fit item twice"));
    CHECK(chk({0, 1, 1, 0, 1, 2, 0, 2, 1}).empty());                    // the same band on another plane, another band on the same
    std::vector<int32_t> many;
    for (int i = 0; i < 129; ++i) { many.push_back(0); many.push_back(i % 5); many.push_back(0); }
    CHECK(has(dx_fit_check(129, many.data(), 5, 3), "DANGX_MAX_FIT"));
    CHECK(has(dx_fit_check(128, many.data(), 5, 3), "the same fit item twice"));   // the limit comes first, then the list
    CHECK(DX_FIT_MAX == 128);
    // ---- the plan: a segment per plane with items, planes ascending whatever the list order
    const std::vector<int32_t> sp = {0, 3, 2, 1, -1, 0, 0, 1, 2, 0, 4, 0, 1, -1, 2};
    std::vector<DxFitSeg> plan = dx_fit_plan(5, sp.data(), 5);
    CHECK(plan.size() == 2 && plan[0].plane == 0 && plan[1].plane == 2);
    if (plan.size() == 2) {
        CHECK(plan[0].chi == 1 && plan[0].res.size() == 5 && plan[0].res[4] == 3);
        for (int j = 0; j < 4; ++j) CHECK(plan[0].res[j] == -1);
        CHECK(plan[1].chi == 4 && plan[1].res[3] == 0 && plan[1].res[1] == 2 && plan[1].res[0] == -1 && plan[1].res[2] == -1 && plan[1].res[4] == -1);
    }
    const std::vector<int32_t> q = {0, 2, 1};
    plan = dx_fit_plan(1, q.data(), 5);
    CHECK(plan.size() == 1 && plan[0].plane == 1 && plan[0].chi == -1 && plan[0].res[2] == 0);
    CHECK(dx_fit_plan(0, nullptr, 5).empty());
    const std::vector<int32_t> all3 = {1, -1, 2, 1, -1, 1, 1, -1, 0};
    plan = dx_fit_plan(3, all3.data(), 5);
    CHECK(plan.size() == 3 && plan[0].chi == 2 && plan[1].chi == 1 && plan[2].chi == 0);
    // ---- a sample, by hand.  Two components at one band: x = 3 * 0.5 and -2 * 0.25; sky = (0 + 1.5) + -0.5 = 1
    double sky = 0.0;
    sky = dx_fit_sky_add(sky, dx_fit_product(3.0, 0.5));
    sky = dx_fit_sky_add(sky, dx_fit_product(-2.0, 0.25));
    CHECK(sky == 1.0);
    // T: (sig - offset) / gain - sky = (7 - 1) / 2 - 1 = 2; Q, U ignore the calibration: 7 - 1 = 6
    CHECK(dx_fit_residual(0, 7.0, 1.0, 2.0, sky) == 2.0 && dx_fit_residual(1, 7.0, 1.0, 2.0, sky) == 6.0 && dx_fit_residual(2, 7.0, 1.0, 2.0, sky) == 6.0);
    // chi^2 over two bands: (2 * 2) / (0.5 * 0.5) = 16 and (6 * 6) / (3 * 3) = 4; (16 + 4) / 2 = 10
    double chi = 0.0;
    chi = dx_fit_chi_add(chi, dx_fit_chi_term(2.0, 0.5));
    chi = dx_fit_chi_add(chi, dx_fit_chi_term(6.0, 3.0));
    CHECK(chi == 20.0 && dx_fit_chisq(chi, 2) == 10.0);
    // every product and sum is rounded on its own: 0.1 * 0.1 is not 0.01, and a fused multiply-add would give another sum
    const double p = dx_fit_product(0.1, 0.1);
    CHECK(p == 0.1 * 0.1 && p != 0.01);
    CHECK(dx_fit_sky_add(-0.01, p) == p - 0.01 && dx_fit_sky_add(-0.01, p) != std::fma(0.1, 0.1, -0.01));
    const double third = 1.0 / 3.0;
    CHECK(dx_fit_chi_term(third, 3.0) == (third * third) / 9.0);
    CHECK(dx_fit_residual(0, 1.0, 0.1, 3.0, 0.0) == (1.0 - 0.1) / 3.0);
    // NaN and inf propagate, nothing is skipped: a zero amplitude times an infinite sed is NaN, a zero rms gives inf
    CHECK(std::isnan(dx_fit_product(0.0, INF)) && std::isnan(dx_fit_sky_add(1.0, NaN)) && std::isnan(dx_fit_residual(0, NaN, 0.0, 1.0, 0.0)));
    CHECK(dx_fit_chi_term(1.0, 0.0) == INF && std::isnan(dx_fit_chi_term(0.0, 0.0)) && std::isnan(dx_fit_chisq(NaN, 5)));
    CHECK(dx_fit_residual(0, 1.0, 0.0, 0.0, 0.0) == INF);
    // ---- sections: a registration WITHOUT fit items hashes as it did before fit items existed (constants recorded from the
    // section layer of the parent commit); fit items change the signals' group and only it, apart from an angle list of the same numbers
    uint64_t g0[DX_SEC_GROUPS], g1[DX_SEC_GROUPS], g2[DX_SEC_GROUPS];
    CHECK(dx_section_fingerprint(reg(0)) == 0x3881fd03ae980036ull && dx_section_fingerprint(reg(14)) == 0x6c4235f5e3401aaull);
    CHECK(dx_section_fingerprint(reg(2)) == 0x9bd9e7b99d414c9cull && dx_section_fingerprint(reg(3)) == 0x26483c867bd289d1ull);
    CHECK(dx_section_fingerprint(DxSecReg()) == 0xd50d7e171164e4f3ull);
    dx_section_groups(reg(0), g0);
    CHECK(g0[DX_SEC_G_SIGNALS] == 0x9819c89c69c04b01ull);
    dx_section_groups(reg(14), g1);
    CHECK(g1[DX_SEC_G_SIGNALS] == 0x5f7ced70f6d7f740ull);
    dx_section_groups(reg(2), g1);
    CHECK(g1[DX_SEC_G_SIGNALS] == 0xbab8e1ea4b9eda06ull);
    dx_section_groups(reg(3), g1);
    CHECK(g1[DX_SEC_G_SIGNALS] == 0xa8c7f832281a39c5ull);
    DxSecReg rf = reg(0);
    rf.fit = {0, 1, 0};
    dx_section_groups(rf, g1);
    for (int i = 0; i < DX_SEC_GROUPS; ++i) CHECK((g0[i] != g1[i]) == (i == DX_SEC_G_SIGNALS));
    CHECK(dx_section_fingerprint(rf) != dx_section_fingerprint(reg(0)));
    DxSecReg rg = reg(0);
    rg.fit = {1, -1, 0};
    CHECK(dx_section_fingerprint(rg) != dx_section_fingerprint(rf));
    DxSecReg ra = reg(0), rb = reg(0);                  // an angle list and a fit list of the same numbers are told apart
    ra.angles = {0, 1, 0, 2, 0, 3}; rb.fit = {0, 1, 0, 2, 0, 3};
    dx_section_groups(ra, g1); dx_section_groups(rb, g2);
    CHECK(g1[DX_SEC_G_SIGNALS] != g2[DX_SEC_G_SIGNALS]);
    CHECK(has(dx_section_head_diff(dx_section_head(rf, 3, 4), dx_section_head(reg(0), 3, 4)), "the fit items, signal or angle registrations differ"));
    CHECK(dx_section_head_diff(dx_section_head(rf, 3, 4), dx_section_head(rf, 3, 4)).empty());
    CHECK(DX_SEC_FIT == 8 && std::string(dx_section_family_name(DX_SEC_FIT)) == "FIT" && std::string(dx_section_family_name(9)) == "?");
    CHECK(DX_SEC_VERSION == 1u && DX_SEC_HEAD_BYTES == 104 && DX_SEC_GROUPS == 6);
    CHECK(dx_section_fit_bytes(95) == 2 * 95 * 8);
    std::printf(bad ? "host part: %d checks failed\n" : "host part ok\n", bad);
    return bad ? 1 : 0;
}
"""


def test_fit_header_under_sanitizers(tmp_path):
    """dang_amd/csrc/dx_fit_host.h and dx_section_host.h -- what dangx_moments_fit, the kernel's expressions and the sections call
    -- in a program of its own, compiled with -fsanitize=address,undefined and run once on the CPU as a child process."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "host_main.cpp", tmp_path / "host_main"
    src.write_text(HOST_MAIN)
    # -ffp-contract=off: the header's expressions are stated with every product and sum rounded; the device build says so by
    # pragma, a host compiler that knows no such pragma is told here
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "dang_amd", "csrc"), "-o", str(exe), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip: the same source must then compile without the sanitizers, so that
        # an error of the program's own is never hidden
        plain = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert plain.returncode == 0, r.stdout
        if any(w in r.stdout for w in ("libasan", "libubsan", "clang_rt.asan", "clang_rt.ubsan")):
            pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host part ok" in r.stdout, r.stdout
