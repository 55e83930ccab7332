"""Per-pixel posterior histograms, host side: the default plane list of what a run samples, posterior_quantile_maps' assembly and
masked-pixel fill on host arrays, and the shared definitions (dang_amd/csrc/dx_hist_host.h: bin rule, quantile walk, mode,
registration checks, counter limit -- the functions the kernels call) as a stand-alone program under the address and
undefined-behaviour sanitizers.  No device needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, Q, U = 0, 1, 2      # planes, 0-based

# label -> (planes its indices live on, the sampled indices as `what`).  synth.PHYS: ff T_e, ame w and both dust2 indices are fixed.
EXPECT = {
    "cmb": ((T,), ()), "synch": ((T,), (1,)), "dust": ((T,), (1, 2)), "ff": ((T,), ()), "ame": ((T,), (1,)), "dust2": ((T,), ()),
    "cmb_P": ((Q, U), ()), "synch_P": ((Q, U), (1,)), "dust_P": ((Q, U), (1, 2)), "ff_P": ((Q, U), ()),
    "ame_P": ((Q, U), (1,)), "dust2_P": ((Q, U), ()),
}


def _expected(comps):
    return [(l, w, k) for l, c in enumerate(comps) for w in EXPECT[c.label][1] for k in EXPECT[c.label][0]]


@pytest.mark.parametrize("config", ["C1", "C2", "C3", "C5"])
def test_default_planes_of_the_synthetic_models(config):
    dpar, ddata, bands, comps, meta = synth.make_sky(config, nside=1)
    sel = da.default_moment_selection(dpar, comps)
    planes = da.default_hist_planes(dpar, comps, sel)
    assert planes == _expected(comps)
    assert len(set(planes)) == len(planes) <= L.MAX_HIST
    assert all(w >= 1 for l, w, k in planes)              # index planes only: those have a default range
    if config == "C1":      # synch beta, dust beta and T on T alone
        assert planes == [(0, 1, 0), (1, 1, 0), (1, 2, 0)]
    if config == "C3":      # 3 of the synchrotron, 6 of the dust: the nine planes of the measurement at Nside 1024
        labels = [comps[l].label.split("_")[0] for l, w, k in planes]
        assert len(planes) == 9 and labels.count("synch") == 3 and labels.count("dust") == 6


def test_default_planes_follow_the_flags():
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=1, device="cpu", as_numpy=False)
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 4))
    sel = da.default_moment_selection(dpar, comps)
    assert da.default_hist_planes(dpar, comps, sel) == _expected(comps[:-2])      # the template and the monopole have no index
    comps[1].sample_amplitude = False                          # synch: index only -- still a histogram
    comps[2].sample_index = [True, False]                      # dust: T fixed
    comps[5].pol_flag = [[L.FLAG_Q], [L.FLAG_U]]               # dust_P: beta on Q, T on U
    sel = da.default_moment_selection(dpar, comps)
    planes = da.default_hist_planes(dpar, comps, sel)
    assert [p for p in planes if p[0] == 1] == [(1, 1, T)]
    assert [p for p in planes if p[0] == 2] == [(2, 1, T)]
    assert [p for p in planes if p[0] == 5] == [(5, 1, Q), (5, 2, U)]
    assert [p for p in planes if p[0] == 4] == [(4, 1, Q), (4, 1, U)]             # synch_P as before
    comps[4].sample_index = [False]
    sel = da.default_moment_selection(dpar, comps)
    assert [p for p in da.default_hist_planes(dpar, comps, sel) if p[0] == 4] == []
    # a selection narrower than the flags: only what is selected
    sel = da.default_moment_selection(dpar, comps)
    sel[5] &= ~(1 << (3 + Q))
    assert [p for p in da.default_hist_planes(dpar, comps, sel) if p[0] == 5] == [(5, 2, U)]


class _FakeEngine:
    """What posterior_quantile_maps reads of an Engine, over host arrays: one shard."""

    def __init__(self, comps, masks, qmaps, mode, n, reg, count=7):
        self.component_list, self.ddata = comps, da.DangData(sig_map=None, rms_map=None, masks=masks)
        self._q, self._mode, self._n, self._moment_hist, self._count = qmaps, mode, n, reg, count
        self.npix = masks.shape[1]
        self.asked = []

    def moments_count(self):
        return self._count

    def moments_hist_stat(self, reg, stat, q=None):
        self.asked.append((reg, stat, None if q is None else tuple(q)))
        return {"quantile": self._q, "mode": self._mode, "n": self._n}[stat][reg].copy()


def _shard(rng, npix, masked, reg, nq=3, count=7):
    comps = [da.DangComps(label="dust", type="mbb", nu_ref=353.0, nindices=2, ind_label=["beta", "T"])]
    masks = np.ones((3, npix))
    masks[0, masked] = 0.0
    nreg = len(reg["planes"])
    return _FakeEngine(comps, masks, [rng.uniform(1, 2, (nq, npix)) for _ in range(nreg)], [rng.uniform(1, 2, npix) for _ in range(nreg)],
                       [np.full(npix, 7.0) for _ in range(nreg)], reg, count)


def test_posterior_quantile_maps_fill_and_assembly_on_host_arrays():
    rng = np.random.default_rng(3)
    reg = {"planes": [(0, 1, 0), (0, 2, 0)], "ranges": [(1.0, 2.0), (10.0, 40.0)], "nbins": 32, "bits": 16}
    engs = [_shard(rng, 5, [1, 4], dict(reg)), _shard(rng, 4, [0], dict(reg))]
    keys = [("dust", "beta", 0), ("dust", "T", 0)]
    plain = da.posterior_quantile_maps(None, engines=engs)
    assert list(plain) == keys
    for r, key in enumerate(keys):
        e = plain[key]
        assert set(e) == {"q", "mode", "n", "range", "nbins"} and e["range"] == reg["ranges"][r] and e["nbins"] == 32
        assert e["q"].shape == (3, 9) and np.array_equal(e["q"], np.concatenate([g._q[r] for g in engs], axis=1))
        assert np.array_equal(e["mode"], np.concatenate([g._mode[r] for g in engs]))
        assert np.array_equal(e["n"], np.full(9, 7.0))
    assert (0, "quantile", (0.16, 0.5, 0.84)) in engs[0].asked
    unseen = -1.6375e30
    filled = da.posterior_quantile_maps(None, masked_value=unseen, engines=engs)
    masked = np.zeros(9, dtype=bool)
    masked[[1, 4, 5]] = True
    for key in keys:
        for name in ("q", "mode", "n"):
            assert (filled[key][name][..., masked] == unseen).all()
            assert np.array_equal(filled[key][name][..., ~masked], plain[key][name][..., ~masked])
    one = da.posterior_quantile_maps(None, q=(0.5,), engines=[_shard(rng, 5, [], dict(reg), nq=1)])
    assert one[keys[0]]["q"].shape == (1, 5)
    # contexts that differ in registration or count
    engs[1]._moment_hist = dict(reg, nbins=64)
    with pytest.raises(da.DangxError, match="different histogram registrations"):
        da.posterior_quantile_maps(None, engines=engs)
    engs[1]._moment_hist = dict(reg)
    engs[1]._count = 8
    with pytest.raises(da.DangxError, match="different sample counts"):
        da.posterior_quantile_maps(None, engines=engs)
    engs[0]._moment_hist = None
    with pytest.raises(da.DangxError, match="moments_hist was not called"):
        da.posterior_quantile_maps(None, engines=engs)


HOST_MAIN = r"""
#include "dx_hist_host.h"
#include <algorithm>
#include <cstdio>
#include <limits>
#include <vector>
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool has(const std::string& s, const char* w) { return s.find(w) != std::string::npos; }
static unsigned long long rng_state = 12345;
static double uniform() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}
// a record filled by the rule the kernel runs: load the one word, add, store
static void add(std::vector<uint32_t>& rec, double x, double lo, double hi, int nbins, int bits) {
    if (!dx_hist_counted(x, lo, hi)) return;
    const int b = dx_hist_bin(x, lo, dx_hist_scale(lo, hi, nbins), nbins);
    rec[dx_hist_word_of(b, bits)] += dx_hist_one(b, bits);
}
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- the bin rule on edge values
    for (int nbins : {8, 16, 32, 64}) {
        for (double offs : {0.0, -3.1, 1.0e6}) {
            const double lo = offs - 12.0, hi = offs + 12.0, scale = dx_hist_scale(lo, hi, nbins);
            CHECK(dx_hist_counted(lo, lo, hi) && dx_hist_bin(lo, lo, scale, nbins) == 0);
            CHECK(dx_hist_counted(hi, lo, hi) && dx_hist_bin(hi, lo, scale, nbins) == nbins - 1);      // the last bin is closed
            CHECK(!dx_hist_counted(std::nextafter(lo, -inf), lo, hi) && !dx_hist_counted(std::nextafter(hi, inf), lo, hi));
            CHECK(!dx_hist_counted(nan, lo, hi) && !dx_hist_counted(inf, lo, hi) && !dx_hist_counted(-inf, lo, hi));
            CHECK(dx_hist_bin(std::nextafter(hi, -inf), lo, scale, nbins) == nbins - 1);
            for (int e = 1; e < nbins; ++e) {       // 24 / nbins is a binary fraction: the interior edges are exact here
                const double edge = lo + (hi - lo) * e / nbins;
                CHECK(dx_hist_bin(edge, lo, scale, nbins) == e);                                          // an edge opens its bin
                const int below = dx_hist_bin(std::nextafter(edge, -inf), lo, scale, nbins);
                CHECK(below == e - 1 || below == e);       // one ulp under the edge may round onto it: the rule is the definition
            }
        }
    }
    // ---- records: both widths hold the same counts, 16-bit halves do not disturb each other
    for (int bits : {16, 32}) {
        const int nbins = 8;
        std::vector<uint32_t> rec(dx_hist_words(nbins, bits), 0u);
        CHECK((int)rec.size() * 4 == nbins * bits / 8);
        for (int b = 0; b < nbins; ++b)
            for (int r = 0; r <= b; ++r) add(rec, 0.5 + b, 0.0, 8.0, nbins, bits);
        for (int b = 0; b < nbins; ++b) CHECK(dx_hist_count(rec.data(), b, bits) == (uint32_t)(b + 1));
        CHECK(dx_hist_total(rec.data(), nbins, bits) == 36);
        CHECK(dx_hist_mode(rec.data(), nbins, bits, 0.0, 8.0) == 7.5);
    }
    {   // a 16-bit counter at its limit next to its neighbour
        std::vector<uint32_t> rec(4, 0u);
        for (int r = 0; r < 65535; ++r) add(rec, 0.5, 0.0, 8.0, 8, 16);
        add(rec, 1.5, 0.0, 8.0, 8, 16);
        CHECK(dx_hist_count(rec.data(), 0, 16) == 65535u && dx_hist_count(rec.data(), 1, 16) == 1u && rec[0] == 0x0001ffffu);
    }
    // ---- the quantile walk against the order statistic, on seeded series: unimodal, bimodal with empty bins between, constant,
    // samples on edges, samples outside
    int cases = 0;
    for (int kind = 0; kind < 4; ++kind)
        for (int nbins : {8, 64})
            for (int bits : {16, 32})
                for (int n : {1, 2, 7, 64, 500}) {
                    const double lo = -3.1 - 12.0, hi = -3.1 + 12.0, width = (hi - lo) / nbins, scale = dx_hist_scale(lo, hi, nbins);
                    std::vector<uint32_t> rec(dx_hist_words(nbins, bits), 0u);
                    std::vector<double> in;
                    double v = 0.0;
                    for (int t = 0; t < n; ++t) {
                        double x;
                        if (kind == 0) { if (t % 2 == 0) v = 0.6 * v + 6.0 * (uniform() - 0.5); x = -3.1 + v; }
                        else if (kind == 1) x = (uniform() < 0.4 ? lo + 2.0 : hi - 3.0) + uniform();
                        else if (kind == 2) x = 1.25;
                        else x = lo + width * (int)(uniform() * (nbins + 3) - 1);       // edges, one below lo, some above hi
                        add(rec, x, lo, hi, nbins, bits);
                        if (dx_hist_counted(x, lo, hi)) in.push_back(x);
                    }
                    std::sort(in.begin(), in.end());
                    const unsigned long long N = dx_hist_total(rec.data(), nbins, bits);
                    CHECK(N == in.size());
                    for (double q : {0.025, 0.16, 0.5, 0.84, 0.975}) {
                        const double val = dx_hist_quantile(rec.data(), nbins, bits, lo, hi, q);
                        if (N == 0) { CHECK(std::isnan(val)); continue; }
                        const long long k = (long long)std::ceil(q * (double)N);
                        CHECK(k >= 1 && k <= (long long)N);
                        const int b = dx_hist_bin(in[k - 1], lo, scale, nbins);
                        CHECK(val >= dx_hist_value(lo, width, b) && val <= dx_hist_value(lo, width, b + 1));
                        ++cases;
                    }
                    if (N == 0) CHECK(std::isnan(dx_hist_mode(rec.data(), nbins, bits, lo, hi)));
                    if (kind == 2 && N) {     // a series that never moved: everything in its one bin
                        const int b = dx_hist_bin(1.25, lo, scale, nbins);
                        CHECK(dx_hist_mode(rec.data(), nbins, bits, lo, hi) == dx_hist_value(lo, width, b + 0.5));
                    }
                }
    CHECK(cases > 300);
    {   // the walk by hand: counts 2 0 0 6 in four of eight bins on [0, 8]
        std::vector<uint32_t> rec(4, 0u);
        for (double x : {0.1, 0.9, 3.0, 3.1, 3.2, 3.3, 3.4, 3.5}) add(rec, x, 0.0, 8.0, 8, 16);
        CHECK(dx_hist_quantile(rec.data(), 8, 16, 0.0, 8.0, 0.25) == 1.0);          // target 2 = the first bin's count: its upper edge
        CHECK(dx_hist_quantile(rec.data(), 8, 16, 0.0, 8.0, 0.125) == 0.5);
        CHECK(dx_hist_quantile(rec.data(), 8, 16, 0.0, 8.0, 0.625) == 3.5);         // target 5: 3 + (5 - 2) / 6, the empty bins skipped
        CHECK(dx_hist_mode(rec.data(), 8, 16, 0.0, 8.0) == 3.5);
        std::vector<uint32_t> tie(4, 0u);
        for (double x : {5.5, 2.5, 2.6, 5.6}) add(tie, x, 0.0, 8.0, 8, 16);
        CHECK(dx_hist_mode(tie.data(), 8, 16, 0.0, 8.0) == 2.5);                    // the lowest bin on ties
    }
    // ---- the registration checks.  two components: 0 = mbb with two indices, amplitude and both indices on T selected;
    // 1 = a template with rows Q, U selected
    const int32_t sel[2] = {1 | (1 << 3) | (1 << 6), 6};
    const int nind[2] = {2, 0}, global[2] = {0, 1};
    const std::vector<int32_t> ok = {0, 1, 0, 0, 2, 0, 0, 0, 0};
    const std::vector<double> rg = {1.0, 2.0, 10.0, 40.0, -5.0, 5.0};
    const std::vector<int> has_rg = {1, 1, 1};
    auto chk = [&](int nreg, const std::vector<int32_t>& p, const std::vector<double>& r, const std::vector<int>& h, int nbins, int bits) {
        return dx_hist_check(nreg, p.data(), r.data(), h.data(), nbins, bits, 2, 3, sel, nind, global);
    };
    CHECK(chk(3, ok, rg, has_rg, 64, 16).empty());
    CHECK(chk(3, ok, rg, has_rg, 32, 32).empty());
    CHECK(dx_hist_check(0, nullptr, nullptr, nullptr, 64, 16, 2, 3, sel, nind, global).empty());
    CHECK(has(dx_hist_check(1, nullptr, rg.data(), has_rg.data(), 64, 16, 2, 3, sel, nind, global), "no plane list"));
    for (int nb : {0, 7, 12, 128, -8}) CHECK(has(chk(3, ok, rg, has_rg, nb, 16), "nbins must be"));
    for (int bt : {0, 8, 64}) CHECK(has(chk(3, ok, rg, has_rg, 64, bt), "bits must be"));
    CHECK(has(chk(3, ok, rg, has_rg, 64, 32), "128 bytes"));
    std::vector<int32_t> p = ok;
    p[2] = 1;
    CHECK(has(chk(3, p, rg, has_rg, 64, 16), "not selected"));
    p = ok; p[6] = 1; p[7] = 0; p[8] = 1;
    CHECK(has(chk(3, p, rg, has_rg, 64, 16), "template"));
    p = ok; p[0] = 2;
    CHECK(has(chk(3, p, rg, has_rg, 64, 16), "component index"));
    p = ok; p[1] = 3;
    CHECK(has(chk(3, p, rg, has_rg, 64, 16), "what"));
    p = ok; p[2] = 3;
    CHECK(has(chk(3, p, rg, has_rg, 64, 16), "plane out of range"));
    p = ok; p[3] = 0; p[4] = 1; p[5] = 0;
    CHECK(has(chk(3, p, rg, has_rg, 64, 16), "the same plane twice"));
    std::vector<int> h = has_rg;
    h[2] = 0;
    CHECK(has(chk(3, ok, rg, h, 64, 16), "explicit range"));
    std::vector<double> r = rg;
    r[1] = 1.0;
    CHECK(has(chk(3, ok, r, has_rg, 64, 16), "hi > lo"));
    r = rg; r[3] = 5.0;
    CHECK(has(chk(3, ok, r, has_rg, 64, 16), "hi > lo"));
    r = rg; r[2] = -inf;
    CHECK(has(chk(3, ok, r, has_rg, 64, 16), "non-finite"));
    r = rg; r[5] = nan;
    CHECK(has(chk(3, ok, r, has_rg, 64, 16), "non-finite"));
    r = rg; r[4] = -1.7e308; r[5] = 1.7e308;
    CHECK(has(chk(3, ok, r, has_rg, 64, 16), "non-finite"));
    std::vector<int32_t> many;
    std::vector<double> many_r;
    std::vector<int> many_h;
    for (int i = 0; i < 33; ++i) { many.insert(many.end(), ok.begin(), ok.begin() + 3); many_r.push_back(0.0); many_r.push_back(1.0); many_h.push_back(1); }
    CHECK(has(chk(33, many, many_r, many_h, 64, 16), "DANGX_MAX_HIST"));
    CHECK(has(chk(32, many, many_r, many_h, 64, 16), "the same plane twice"));
    CHECK(has(chk(-1, ok, rg, has_rg, 64, 16), "negative"));
    // ---- the sample limit of both widths
    CHECK(dx_hist_limit(16) == 65535ll && dx_hist_limit(32) == 4294967295ll);
    CHECK(dx_hist_limit_check(65535, 16).empty() && has(dx_hist_limit_check(65536, 16), "65535"));
    CHECK(dx_hist_limit_check(4294967295ll, 32).empty() && has(dx_hist_limit_check(4294967296ll, 32), "4294967295"));
    std::printf(bad ? "host part: %d checks failed\n" : "host part ok\n", bad);
    return bad ? 1 : 0;
}
"""


def test_host_part_under_sanitizers(tmp_path):
    """The definitions of dang_amd/csrc/dx_hist_host.h -- the functions k_moments_hist / k_hist_stat call -- in a program of
    their own, compiled with -fsanitize=address,undefined and run once on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "host_main.cpp", tmp_path / "host_main"
    src.write_text(HOST_MAIN)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "dang_amd", "csrc"), "-o", str(exe), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and ("cannot find" in r.stdout or "unsupported" in r.stdout):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host part ok" in r.stdout, r.stdout
