"""Posterior moments of component signals, host side: the default signal list of what a run samples (band nearest nu_ref, the
lowest on ties; the planes of the sampled amplitude plus P; nothing for index-less or global-amplitude components),
posterior_signal_maps' assembly on host arrays, and the registration planner (dang_amd/csrc/dx_signal_host.h: the check of a
signal list, the grouping into segments of at most 8 bands, the two rounded expressions of a sample) as a stand-alone program
under the address and undefined-behaviour sanitizers.  No device needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, Q, U, P = 0, 1, 2, 3


def _nearest(bands, nu_ref_ghz):
    d = [abs(b.nu_c - nu_ref_ghz) for b in bands]
    return d.index(min(d))


def test_default_specs_of_a_c3_shaped_model():
    """C3: cmb (no index), synch (beta), dust (beta, T), ff (T_e fixed) on T and on Q+U: synch and dust only, 8 signals."""
    dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=1)
    assert [c.label for c in comps] == ["cmb", "synch", "dust", "ff", "cmb_P", "synch_P", "dust_P", "ff_P"]
    bs, bd = _nearest(bands, 30.0), _nearest(bands, 353.0)
    assert (bs, bd) == (1, 7)               # 20 (857/20)^(j/9) GHz: 30.4 GHz and 371.9 GHz
    specs = da.default_signal_specs(dpar, comps, bands)
    assert specs == [(1, bs, T), (2, bd, T), (5, bs, Q), (5, bs, U), (5, bs, P), (6, bd, Q), (6, bd, U), (6, bd, P)]
    assert len(specs) == 8 <= L.MAX_SIGNALS


def test_default_specs_of_a_c5_shaped_model():
    """C5 adds ame (nu_p sampled, w fixed) and dust2 (both indices fixed): ame joins, dust2 and ff do not."""
    dpar, ddata, bands, comps, meta = synth.make_sky("C5", nside=1)
    lab = [c.label for c in comps]
    bs, bd, ba = _nearest(bands, 30.0), _nearest(bands, 353.0), _nearest(bands, 22.0)
    want = []
    for name, band in (("synch", bs), ("dust", bd), ("ame", ba)):
        want.append((lab.index(name), band, T))
    for name, band in (("synch_P", bs), ("dust_P", bd), ("ame_P", ba)):
        want += [(lab.index(name), band, k) for k in (Q, U, P)]
    specs = da.default_signal_specs(dpar, comps, bands)
    assert specs == sorted(want) == want
    assert not any(comps[l].label.split("_")[0] in ("cmb", "ff", "dust2") for l, j, k in specs)


def test_default_specs_follow_the_flags_and_the_tie_rule():
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=1, device="cpu", as_numpy=False)
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 4))
    specs = da.default_signal_specs(dpar, comps, bands)
    assert {l for l, j, k in specs} == {1, 2, 4, 5}                  # synch, dust on T and on Q+U; no cmb, template or monopole
    # a tie: nu_ref half way between two bands takes the lower one
    bands[1].nu_c, bands[2].nu_c = 25.0, 35.0
    assert [s for s in da.default_signal_specs(dpar, comps, bands) if s[0] == 1] == [(1, 1, T)]
    bands[1].nu_c, bands[0].nu_c = 35.0, 25.0                         # the same two distances in the other order: still the first
    assert [s for s in da.default_signal_specs(dpar, comps, bands) if s[0] == 1] == [(1, 0, T)]
    # frequencies in Hz and in GHz mix: the nearest is found in Hz
    bands[0].nu_c = 29.0e9
    assert [s for s in da.default_signal_specs(dpar, comps, bands) if s[0] == 1] == [(1, 0, T)]
    comps[1].sample_amplitude = False                                 # synch: a fixed amplitude -- no signal
    comps[2].sample_index = [False, False]                            # dust: no sampled index -- a multiple of the amplitude
    dpar.cg_groups[1].pol_flag = [L.FLAG_Q]                           # the Q+U group solves Q alone: no U, no P
    specs = da.default_signal_specs(dpar, comps, bands)
    assert {l for l, j, k in specs} == {4, 5}
    assert [k for l, j, k in specs if l == 4] == [Q] and [k for l, j, k in specs if l == 5] == [Q]


class _FakeEngine:
    """What posterior_signal_maps reads of an Engine, over host arrays: one shard."""

    def __init__(self, comps, bands, masks, maps, reg, count=5):
        self.component_list, self.bands, self.ddata = comps, bands, da.DangData(sig_map=None, rms_map=None, masks=masks)
        self._maps, self._moment_signals, self._count = maps, reg, count

    def moments_count(self):
        return self._count

    def moments_get_signal(self, s, stat, ddof=0):
        return self._maps[stat][s].copy() + ddof


def test_posterior_signal_maps_fill_and_assembly_on_host_arrays():
    rng = np.random.default_rng(7)
    comps = [da.DangComps(label="synch_P", type="power-law", nu_ref=30.0, nindices=1, ind_label=["beta"])]
    bands = [da.BandInfo(label="bp_030", nu_c=30.0), da.BandInfo(label="bp_044", nu_c=44.0)]
    reg = [(0, 0, Q), (0, 0, P), (0, 1, U)]

    def shard(npix, masked, reg=reg, count=5):
        masks = np.ones((3, npix))
        masks[0, masked] = 0.0
        maps = {st: [rng.uniform(1, 2, npix) for _ in reg] for st in ("mean", "std")}
        return _FakeEngine(comps, bands, masks, maps, list(reg), count)
    engs = [shard(5, [1, 4]), shard(4, [0])]
    plain = da.posterior_signal_maps(None, engines=engs)
    keys = [("synch_P", "bp_030", "Q"), ("synch_P", "bp_030", "P"), ("synch_P", "bp_044", "U")]
    assert list(plain) == keys
    for s, key in enumerate(keys):
        assert set(plain[key]) == {"mean", "std", "n"} and plain[key]["n"] == 5
        for st in ("mean", "std"):
            assert np.array_equal(plain[key][st], np.concatenate([e._maps[st][s] for e in engs]))
    assert np.array_equal(da.posterior_signal_maps(None, ddof=1, engines=engs)[keys[0]]["std"], plain[keys[0]]["std"] + 1)
    unseen = -1.6375e30
    filled = da.posterior_signal_maps(None, masked_value=unseen, engines=engs)
    masked = np.zeros(9, dtype=bool)
    masked[[1, 4, 5]] = True
    for key in keys:
        for st in ("mean", "std"):
            assert (filled[key][st][masked] == unseen).all() and np.array_equal(filled[key][st][~masked], plain[key][st][~masked])
    engs[1]._moment_signals = reg[:2]
    with pytest.raises(da.DangxError, match="different signal registrations"):
        da.posterior_signal_maps(None, engines=engs)
    engs[1]._moment_signals = list(reg)
    engs[1]._count = 6
    with pytest.raises(da.DangxError, match="different sample counts"):
        da.posterior_signal_maps(None, engines=engs)
    engs[0]._moment_signals = None
    with pytest.raises(da.DangxError, match="moments_signals was not called"):
        da.posterior_signal_maps(None, engines=engs)


HOST_MAIN = r"""
#include "dx_signal_host.h"
#include <cstdio>
#include <limits>
#include <vector>
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool has(const std::string& s, const char* w) { return s.find(w) != std::string::npos; }
int main() {
    // ---- the check.  three components: 0 = diffuse, 1 = a template, 2 = not set; 20 bands, IQU
    const int set[3] = {1, 1, 0}, global[3] = {0, 1, 0};
    auto chk = [&](const std::vector<int32_t>& sp, int nmaps = 3) {
        return dx_signal_check((int)(sp.size() / 3), sp.data(), 3, 20, nmaps, set, global);
    };
    CHECK(chk({0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 19, 3}).empty());
    CHECK(dx_signal_check(0, nullptr, 3, 20, 3, set, global).empty());
    CHECK(has(dx_signal_check(1, nullptr, 3, 20, 3, set, global), "no signal list"));
    CHECK(has(dx_signal_check(-1, nullptr, 3, 20, 3, set, global), "negative"));
    CHECK(has(chk({3, 0, 0}), "component index") && has(chk({-1, 0, 0}), "component index"));
    CHECK(has(chk({2, 0, 0}), "not set"));
    CHECK(has(chk({0, 20, 0}), "band index") && has(chk({0, -1, 0}), "band index"));
    CHECK(has(chk({0, 0, 4}), "kind must be") && has(chk({0, 0, -1}), "kind must be"));
    CHECK(chk({0, 0, 0}, 1).empty());
    CHECK(has(chk({0, 0, 1}, 1), "a plane the model does not have") && has(chk({0, 0, 2}, 1), "a plane the model does not have"));
    CHECK(has(chk({0, 0, 3}, 1), "P needs nmaps == 3"));
    CHECK(has(chk({1, 0, 1}), "dangx_moments_get_template"));
    // ---- duplicate detection: the same (comp, band, kind) anywhere in the list; a different kind or band is not one
    CHECK(has(chk({0, 3, 1, 0, 4, 1, 0, 3, 1}), "signal 2: the same signal twice"));
    CHECK(chk({0, 3, 1, 0, 4, 1, 0, 3, 2, 0, 3, 3}).empty());
    // ---- the limit
    std::vector<int32_t> many;
    for (int j = 0; j < 20; ++j)
        for (int k = 0; k < 4 && (int)many.size() < 3 * 65; ++k) { many.push_back(0); many.push_back(j); many.push_back(k); }
    CHECK((int)many.size() == 3 * 65);
    CHECK(has(dx_signal_check(65, many.data(), 3, 20, 3, set, global), "DANGX_MAX_SIGNALS"));
    CHECK(dx_signal_check(64, many.data(), 3, 20, 3, set, global).empty());
    // ---- the plan: a 17-band component splits into three segments of 8, 8 and 1 bands, bands ascending, whatever the list order
    std::vector<int32_t> sp;
    for (int j = 16; j >= 0; --j) { sp.push_back(0); sp.push_back(j); sp.push_back(0); }      // T of bands 16 .. 0
    std::vector<DxSigSeg> plan = dx_signal_plan(17, sp.data(), 3, 20);
    CHECK(plan.size() == 3 && plan[0].nb == 8 && plan[1].nb == 8 && plan[2].nb == 1);
    int next = 0;
    for (const DxSigSeg& g : plan) {
        CHECK(g.comp == 0 && g.cls == 0);
        for (int b = 0; b < g.nb; ++b) {
            CHECK(g.b[b].band == next && g.b[b].sig[0] == 16 - next && g.b[b].sig[1] == -1 && g.b[b].sig[2] == -1);
            ++next;
        }
    }
    CHECK(next == 17);
    // exactly 8 and 16 bands: no empty segment behind
    CHECK(dx_signal_plan(8, sp.data(), 3, 20).size() == 1 && dx_signal_plan(16, sp.data(), 3, 20).size() == 2);
    CHECK(dx_signal_plan(0, nullptr, 3, 20).empty());
    // classes and slots: P alone, Q and P of one band, T of another component; components ascending, T before Q+U
    const std::vector<int32_t> mix = {2, 5, 3, 0, 1, 3, 0, 1, 1, 0, 7, 2, 0, 1, 0};
    plan = dx_signal_plan(5, mix.data(), 3, 20);
    CHECK(plan.size() == 3);
    CHECK(plan[0].comp == 0 && plan[0].cls == 0 && plan[0].nb == 1 && plan[0].b[0].band == 1 && plan[0].b[0].sig[0] == 4);
    CHECK(plan[1].comp == 0 && plan[1].cls == 1 && plan[1].nb == 2);
    CHECK(plan[1].b[0].band == 1 && plan[1].b[0].sig[0] == 2 && plan[1].b[0].sig[1] == -1 && plan[1].b[0].sig[2] == 1);
    CHECK(plan[1].b[1].band == 7 && plan[1].b[1].sig[0] == -1 && plan[1].b[1].sig[1] == 3 && plan[1].b[1].sig[2] == -1);
    CHECK(plan[2].comp == 2 && plan[2].cls == 1 && plan[2].nb == 1 && plan[2].b[0].sig[2] == 0);
    // every signal of the 64-signal list lands in exactly one slot
    plan = dx_signal_plan(64, many.data(), 3, 20);
    std::vector<int> seen(64, 0);
    for (const DxSigSeg& g : plan)
        for (int b = 0; b < g.nb; ++b)
            for (int o = 0; o < 3; ++o)
                if (g.b[b].sig[o] >= 0) ++seen[g.b[b].sig[o]];
    for (int s = 0; s < 64; ++s) CHECK(seen[s] == 1);
    CHECK(plan.size() == 4);        // 16 bands of T and of Q+U: two segments each
    // ---- the sample's expressions: the product is rounded (not the exact amp * sed an fma would carry), P from rounded terms
    const double a = 1.0 + std::ldexp(1.0, -30), s = 1.0 + std::ldexp(1.0, -29), p = dx_signal_product(a, s);
    CHECK(p == a * s && std::fma(a, s, -p) != 0.0);
    CHECK(dx_signal_pol(3.0, 4.0) == 5.0 && dx_signal_pol(0.0, 0.0) == 0.0 && dx_signal_pol(-3.0, 0.0) == 3.0);
    CHECK(std::isnan(dx_signal_pol(std::numeric_limits<double>::quiet_NaN(), 1.0)));
    CHECK(dx_signal_class(0) == 0 && dx_signal_class(1) == 1 && dx_signal_class(2) == 1 && dx_signal_class(3) == 1);
    CHECK(dx_signal_slot(0) == 0 && dx_signal_slot(1) == 0 && dx_signal_slot(2) == 1 && dx_signal_slot(3) == 2);
    std::printf(bad ? "host part: %d checks failed\n" : "host part ok\n", bad);
    return bad ? 1 : 0;
}
"""


def test_planner_under_sanitizers(tmp_path):
    """dang_amd/csrc/dx_signal_host.h -- what dangx_moments_signals calls to check and group a list -- in a program of its own,
    compiled with -fsanitize=address,undefined and run once on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "host_main.cpp", tmp_path / "host_main"
    src.write_text(HOST_MAIN)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
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
