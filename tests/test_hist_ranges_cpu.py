"""Per-pixel histogram ranges, host side: the shared definitions (dang_amd/csrc/dx_hist_host.h: the per-pixel bin rule, which pixels
are off, the checksum of a pair of range maps, the registration check with a declared per-pixel range; dx_section_host.h: the
fingerprint, which a list of global ranges must leave as it was) as a stand-alone program under the address and
undefined-behaviour sanitizers, and the Python layer on host arrays: the arithmetic of hist_ranges_from_moments, the slicing of
maps over shards, the keys and 'range' of posterior_quantile_maps and the sections a registration owns.  No device needed."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import posterior as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fnv1a_words(values):
    """FNV-1a (64 bit) over the little-endian 64-bit words of the doubles `values`, restated"""
    h = 0xcbf29ce484222325
    for v in values:
        for byte in struct.pack("<d", v):
            h = ((h ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    return h


# The registration list whose fingerprint is pinned below.  FP_HIST_GROUP / FP_ALL are what the header of the commit BEFORE per-pixel
# ranges existed gives for it (computed once from that header): a list of global ranges must hash as it always did, so that saved
# runs keep loading.
FP_HIST_GROUP, FP_ALL = 0x958f19a3533ecc32, 0x0bdc4c5022a9dd7e
KNOWN_LO, KNOWN_HI = (0.0, 1.0, -2.5e-3), (2.0, -0.0, 7.0e300)

HOST_MAIN = r"""
#include "dx_hist_host.h"
#include "dx_section_host.h"
#include <cstdio>
#include <limits>
#include <vector>
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool has(const std::string& s, const char* w) { return s.find(w) != std::string::npos; }
static DxSecReg plain() {
    DxSecReg r;
    r.npix = 192; r.pix0 = 0; r.nmaps = 3;
    r.sel = {9, 73, 0}; r.type = {1, 2, 5}; r.nind = {1, 2, 0};
    r.lag1 = 1; r.pairs = {0, 0, 0, 0, 1, 0};
    r.hist_planes = {0, 1, 0, 1, 1, 0, 1, 2, 0};
    r.hist_range = {-4.5, -1.5, 1.0, 2.0, 10.0, 40.0};
    r.nbins = 64; r.bits = 16;
    r.signals = {0, 1, 0, 1, 3, 3};
    r.batch_planes = {1, 1, 0}; r.nbatch = 8;
    return r;
}
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double big = std::numeric_limits<double>::max(), tiny = std::numeric_limits<double>::denorm_min();
    // ---- the per-pixel bin rule on edge values: the pixel's own bounds land in bins 0 and nbins - 1, one ulp outside is not counted
    for (int nbins : {8, 16, 32, 64})
        for (double offs : {0.0, -3.1, 1.0e6, 4.0e-7}) {
            const double lo = offs - 12.0 * (offs == 4.0e-7 ? 1.0e-8 : 1.0), hi = offs + 12.0 * (offs == 4.0e-7 ? 1.0e-8 : 1.0);
            CHECK(dx_hist_pixel_on(lo, hi, nbins));
            CHECK(dx_hist_pixel_bin(lo, lo, hi, nbins) == 0);
            CHECK(dx_hist_pixel_bin(hi, lo, hi, nbins) == nbins - 1);
            CHECK(dx_hist_pixel_bin(std::nextafter(hi, -inf), lo, hi, nbins) == nbins - 1);
            CHECK(dx_hist_pixel_bin(std::nextafter(lo, -inf), lo, hi, nbins) == -1);
            CHECK(dx_hist_pixel_bin(std::nextafter(hi, inf), lo, hi, nbins) == -1);
            CHECK(dx_hist_pixel_bin(nan, lo, hi, nbins) == -1 && dx_hist_pixel_bin(inf, lo, hi, nbins) == -1 && dx_hist_pixel_bin(-inf, lo, hi, nbins) == -1);
            // the rule IS the global one with this pixel's bounds: scale one division, then dx_hist_bin
            const double scale = (double)nbins / (hi - lo);
            CHECK(scale == dx_hist_pixel_scale(lo, hi, nbins) && scale == dx_hist_scale(lo, hi, nbins));
            for (int t = 0; t <= 1000; ++t) {
                const double x = lo + (hi - lo) * (t / 1000.0);
                if (!dx_hist_counted(x, lo, hi)) { CHECK(dx_hist_pixel_bin(x, lo, hi, nbins) == -1); continue; }
                const int b = dx_hist_pixel_bin(x, lo, hi, nbins);
                CHECK(b == dx_hist_bin(x, lo, scale, nbins) && b >= 0 && b < nbins);
            }
        }
    // ---- every kind of off pixel counts nothing, whatever the sample
    {
        const double off[][2] = {{nan, 1.0}, {0.0, nan}, {nan, nan}, {-inf, 1.0}, {0.0, inf}, {-inf, inf}, {inf, -inf}, {2.0, 2.0}, {3.0, 2.0},
                                 {-big, big}, {0.0, tiny}, {-0.0, 0.0}};
        for (const auto& p : off)
            for (int nbins : {8, 64}) {
                CHECK(!dx_hist_pixel_on(p[0], p[1], nbins));
                for (double x : {0.0, 1.0, 2.0, 2.5, -1.0e300, 1.0e300, tiny, nan, inf, -inf}) CHECK(dx_hist_pixel_bin(x, p[0], p[1], nbins) == -1);
            }
        CHECK(dx_hist_pixel_on(0.0, big, 64) && dx_hist_pixel_on(-big, 0.0, 8));       // wide, and still inside the format
        // an off pixel's record (zeros) reads as N = 0, NaN quantile and mode
        std::vector<uint32_t> rec(dx_hist_words(8, 16), 0u);
        CHECK(dx_hist_total(rec.data(), 8, 16) == 0 && std::isnan(dx_hist_quantile(rec.data(), 8, 16, nan, nan, 0.5)) && std::isnan(dx_hist_mode(rec.data(), 8, 16, nan, nan)));
    }
    // ---- quantile and mode with a pixel's bounds: dx_hist_value(lo[p], (hi[p] - lo[p]) / nbins, t)
    {
        const double lo = 1.0e-6, hi = 9.0e-6;
        std::vector<uint32_t> rec(4, 0u);
        for (double x : {1.1e-6, 1.9e-6, 4.0e-6, 4.1e-6, 4.2e-6, 4.3e-6, 4.4e-6, 4.5e-6}) {
            const int b = dx_hist_pixel_bin(x, lo, hi, 8);
            CHECK(b >= 0);
            rec[dx_hist_word_of(b, 16)] += dx_hist_one(b, 16);
        }
        const double width = (hi - lo) / 8;
        CHECK(dx_hist_quantile(rec.data(), 8, 16, lo, hi, 0.25) == dx_hist_value(lo, width, 1.0));
        CHECK(dx_hist_mode(rec.data(), 8, 16, lo, hi) == dx_hist_value(lo, width, 3.5));
    }
    // ---- the checksum on a known vector (the expected value is restated in Python), and what it depends on
    {
        const double lo[3] = {KNOWN_LO}, hi[3] = {KNOWN_HI};
        CHECK(dx_hist_range_checksum(lo, hi, 3) == KNOWN_SUM);
        CHECK(dx_hist_range_checksum(lo, hi, 0) == 0xcbf29ce484222325ull);
        CHECK(dx_hist_range_checksum(hi, lo, 3) != KNOWN_SUM);                         // lo first, then hi
        double hi2[3] = {KNOWN_HI};
        hi2[1] = 0.0;                                                                  // -0.0 -> 0.0: the bits count, not the value
        CHECK(dx_hist_range_checksum(lo, hi2, 3) != KNOWN_SUM);
        double lo2[3] = {KNOWN_LO};
        lo2[2] = std::nextafter(lo2[2], 0.0);                                          // one pixel, one ulp
        CHECK(dx_hist_range_checksum(lo2, hi, 3) != KNOWN_SUM);
        const double ln[2] = {nan, 1.0}, hn[2] = {nan, 2.0};
        CHECK(dx_hist_range_checksum(ln, hn, 2) == dx_hist_range_checksum(ln, hn, 2));  // NaN maps have a checksum like any other
    }
    // ---- the fingerprint: a list of global ranges hashes as it did before range kinds existed
    {
        uint64_t g[DX_SEC_GROUPS];
        DxSecReg r = plain();
        dx_section_groups(r, g);
        CHECK(g[DX_SEC_G_HIST] == FP_HIST_GROUP && dx_section_fingerprint(r) == FP_ALL);
        r.hist_kind = {0, 0, 0}; r.hist_sum = {0, 0, 0};                                // what a context with global ranges now passes
        dx_section_groups(r, g);
        CHECK(g[DX_SEC_G_HIST] == FP_HIST_GROUP && dx_section_fingerprint(r) == FP_ALL);
        DxSecReg p = r;                                                                 // registration 1 per pixel
        p.hist_range[2] = -inf; p.hist_range[3] = inf; p.hist_kind[1] = DX_HIST_RANGE_PIXEL; p.hist_sum[1] = KNOWN_SUM;
        uint64_t gp[DX_SEC_GROUPS];
        dx_section_groups(p, gp);
        CHECK(gp[DX_SEC_G_HIST] != FP_HIST_GROUP && dx_section_fingerprint(p) != FP_ALL);
        for (int i = 0; i < DX_SEC_GROUPS; ++i) CHECK(i == DX_SEC_G_HIST || gp[i] == g[i]);      // no other group moves
        DxSecReg q = p;
        q.hist_sum[1] = KNOWN_SUM + 1;                                                  // other maps: another histogram group
        uint64_t gq[DX_SEC_GROUPS];
        dx_section_groups(q, gq);
        CHECK(gq[DX_SEC_G_HIST] != gp[DX_SEC_G_HIST]);
        const DxSecHead hp = dx_section_head(p, 5, 0), hq = dx_section_head(q, 5, 0);
        CHECK(dx_section_head_diff(hp, hp).empty() && has(dx_section_head_diff(hq, hp), "the histogram registrations"));
        CHECK(std::string(dx_section_family_name(DX_SEC_HIST_RANGE)) == "HIST_RANGE" && DX_SEC_HIST_RANGE == 6);
        CHECK(dx_section_hist_range_bytes(192) == 2 * 192 * 8);
    }
    // ---- the registration check with declared per-pixel ranges.  component 0 = mbb with two indices, amplitude and both indices on T
    const int32_t sel[2] = {1 | (1 << 3) | (1 << 6), 6};
    const int nind[2] = {2, 0}, global[2] = {0, 1};
    const std::vector<int32_t> planes = {0, 1, 0, 0, 2, 0, 0, 0, 0};
    const std::vector<int> has_rg = {1, 1, 1};
    auto chk = [&](const std::vector<double>& r, const int* kind) {
        return dx_hist_check(3, planes.data(), r.data(), has_rg.data(), 64, 16, 2, 3, sel, nind, global, kind);
    };
    CHECK(dx_hist_range_kind(-inf, inf) == DX_HIST_RANGE_PIXEL);
    CHECK(dx_hist_range_kind(-inf, 2.0) == DX_HIST_RANGE_GLOBAL && dx_hist_range_kind(0.0, inf) == DX_HIST_RANGE_GLOBAL);
    CHECK(dx_hist_range_kind(inf, -inf) == DX_HIST_RANGE_GLOBAL && dx_hist_range_kind(nan, inf) == DX_HIST_RANGE_GLOBAL);
    CHECK(dx_hist_range_kind(1.0, 2.0) == DX_HIST_RANGE_GLOBAL);
    const std::vector<double> rg = {1.0, 2.0, 10.0, 40.0, -inf, inf};
    const int kinds[3] = {DX_HIST_RANGE_GLOBAL, DX_HIST_RANGE_GLOBAL, DX_HIST_RANGE_PIXEL};
    CHECK(chk(rg, kinds).empty());                                     // an amplitude plane with a declared per-pixel range
    CHECK(has(chk(rg, nullptr), "non-finite"));                        // the pair alone, not declared: the error it always was
    const int none[3] = {0, 0, 0};
    CHECK(has(chk(rg, none), "non-finite"));
    std::vector<double> r = rg;
    r[2] = -inf;                                                       // any other non-finite bound stays an error
    CHECK(has(chk(r, kinds), "registration 1: a non-finite bound"));
    r = rg; r[1] = 1.0;
    CHECK(has(chk(r, kinds), "hi > lo"));
    const int all_px[3] = {1, 1, 1};
    CHECK(chk({-inf, inf, -inf, inf, -inf, inf}, all_px).empty());
    std::vector<int32_t> twice = planes;
    twice[6] = 0; twice[7] = 1; twice[8] = 0;                          // the other checks do not depend on the range kind
    CHECK(has(dx_hist_check(3, twice.data(), rg.data(), has_rg.data(), 64, 16, 2, 3, sel, nind, global, kinds), "the same plane twice"));
    // ---- a registered signal as the source: planes[r] = {sig, DX_HIST_SIGNAL, 0}, checked against the number of signals registered
    {
        auto sck = [&](const std::vector<int32_t>& p, const std::vector<double>& r, const std::vector<int>& h, const int* kind, int nsig) {
            return dx_hist_check((int)h.size(), p.data(), r.data(), h.data(), 64, 16, 2, 3, sel, nind, global, kind, nsig);
        };
        CHECK(DX_HIST_SIGNAL == -1);
        const std::vector<int32_t> ps = {0, 1, 0, 2, DX_HIST_SIGNAL, 0, 0, DX_HIST_SIGNAL, 0};      // a plane, signal 2, signal 0
        const std::vector<double> rs = {1.0, 2.0, 0.0, 5.0, -inf, inf};
        const int ks[3] = {0, 0, DX_HIST_RANGE_PIXEL};
        CHECK(sck(ps, rs, {1, 1, 1}, ks, 3).empty());                                       // a global range and maps, beside a plane
        CHECK(has(sck(ps, rs, {1, 1, 1}, ks, 0), "registration 1: a signal source, and no signals are registered"));
        CHECK(has(sck(ps, rs, {1, 1, 1}, ks, 2), "registration 1: signal index out of range (2 signals registered)"));
        std::vector<int32_t> q = ps;
        q[3] = -1;
        CHECK(has(sck(q, rs, {1, 1, 1}, ks, 3), "registration 1: signal index out of range"));
        q = ps; q[6] = 2;
        CHECK(has(sck(q, rs, {1, 1, 1}, ks, 3), "registration 2: the same signal twice"));
        CHECK(has(sck(ps, rs, {1, 0, 1}, ks, 3), "registration 1: a signal source has no default range"));
        q = ps; q[5] = 1;
        CHECK(has(sck(q, rs, {1, 1, 1}, ks, 3), "the third word of a signal source must be 0"));
        std::vector<double> r2 = rs;
        r2[3] = 0.0;                                                                        // the range rules are the planes'
        CHECK(has(sck(ps, r2, {1, 1, 1}, ks, 3), "registration 1: the range needs hi > lo"));
        r2 = rs; r2[2] = nan;
        CHECK(has(sck(ps, r2, {1, 1, 1}, ks, 3), "registration 1: a non-finite bound"));
        // a caller that does not know signal sources (the argument list as it was) sees what it always saw for what = -1
        q = ps; q[3] = 0;                                                                   // (a component that exists, so that `what` is what is named)
        CHECK(has(dx_hist_check(3, q.data(), rs.data(), std::vector<int>{1, 1, 1}.data(), 64, 16, 2, 3, sel, nind, global, ks), "registration 1: what must be 0"));
        // the plane triple of a signal source is in the fingerprint: another signal, another histogram group
        DxSecReg a = plain(), b2 = plain();
        a.hist_planes = {0, 1, 0, 1, DX_HIST_SIGNAL, 0, 1, 2, 0};
        b2.hist_planes = {0, 1, 0, 0, DX_HIST_SIGNAL, 0, 1, 2, 0};
        uint64_t ga[DX_SEC_GROUPS], gb[DX_SEC_GROUPS];
        dx_section_groups(a, ga); dx_section_groups(b2, gb);
        CHECK(ga[DX_SEC_G_HIST] != gb[DX_SEC_G_HIST] && ga[DX_SEC_G_HIST] != FP_HIST_GROUP && ga[DX_SEC_G_SIGNALS] == gb[DX_SEC_G_SIGNALS]);
    }
    std::printf(bad ? "host part: %d checks failed\n" : "host part ok\n", bad);
    return bad ? 1 : 0;
}
"""


def test_host_part_under_sanitizers(tmp_path):
    """The per-pixel definitions of dx_hist_host.h -- the functions k_moments_hist_px / k_hist_stat_px / k_chains_hist_px call --
    and the fingerprint of dx_section_host.h in a program of their own, compiled with -fsanitize=address,undefined and run once."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # asked up front, of a program that cannot fail for any other reason: does this compiler have the sanitizer runtimes?
    probe, probe_exe = tmp_path / "probe.cpp", tmp_path / "probe"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-std=c++17"] + san + ["-o", str(probe_exe), str(probe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    known = _fnv1a_words(KNOWN_LO + KNOWN_HI)
    assert known != _fnv1a_words(KNOWN_HI + KNOWN_LO) and _fnv1a_words(()) == 0xcbf29ce484222325
    src, exe = tmp_path / "host_main.cpp", tmp_path / "host_main"
    src.write_text(HOST_MAIN)
    defs = ["-DKNOWN_LO=" + ",".join(repr(v) for v in KNOWN_LO), "-DKNOWN_HI=" + ",".join(repr(v) for v in KNOWN_HI),
            "-DKNOWN_SUM=0x%016xull" % known, "-DFP_HIST_GROUP=0x%016xull" % FP_HIST_GROUP, "-DFP_ALL=0x%016xull" % FP_ALL]
    cmd = [cxx, "-std=c++17", "-O1", "-g"] + san + ["-I" + os.path.join(ROOT, "dang_amd", "csrc")] + defs + ["-o", str(exe), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout                      # from here on a failure is a failure
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host part ok" in r.stdout, r.stdout


def test_ranges_from_mean_and_std():
    mean = np.array([1.0, -2.0, 3.0, 4.0, 5.0, 6.0])
    std = np.array([0.5, 2.0, 0.0, np.nan, np.inf, 1e-3])
    lo, hi = P._ranges_from_mean_std(mean, std, 5.0)
    assert np.array_equal(lo[[0, 1, 5]], (mean - 5.0 * std)[[0, 1, 5]]) and np.array_equal(hi[[0, 1, 5]], (mean + 5.0 * std)[[0, 1, 5]])
    assert lo[0] == -1.5 and hi[0] == 3.5 and lo[1] == -12.0 and hi[1] == 8.0
    assert np.isnan(lo[2:5]).all() and np.isnan(hi[2:5]).all()            # std 0 (a pixel that never moved), NaN, inf
    cl, ch = P._ranges_from_mean_std(mean, std, 5.0, clip0=True)      # a polarised intensity: the lower bound not below 0
    assert cl[0] == 0.0 and cl[1] == 0.0 and cl[5] == lo[5] > 0 and np.array_equal(ch, hi, equal_nan=True) and np.isnan(cl[2:5]).all()
    lo2, hi2 = P._ranges_from_mean_std(mean, std, 2.0)
    assert lo2[0] == 0.0 and hi2[0] == 2.0 and np.array_equal(np.isnan(lo2), np.isnan(lo))
    torch = pytest.importorskip("torch")
    tl, th = P._ranges_from_mean_std(torch.from_numpy(mean), torch.from_numpy(std), 5.0)
    assert np.array_equal(tl.numpy(), lo, equal_nan=True) and np.array_equal(th.numpy(), hi, equal_nan=True)


def test_maps_are_sliced_over_shards():
    lo, hi = np.arange(10.0), np.arange(10.0) + 100.0
    ranges = [(1.0, 2.0), None, (lo, hi)]
    assert not P._is_range_maps((1.0, 2.0)) and not P._is_range_maps(None) and P._is_range_maps((lo, hi))
    cuts = [P._slice_ranges(ranges, off, n, 10) for off, n in ((0, 3), (3, 1), (4, 6))]
    for (off, n), cut in zip(((0, 3), (3, 1), (4, 6)), cuts):
        assert cut[0] == (1.0, 2.0) and cut[1] is None
        assert np.array_equal(cut[2][0], lo[off:off + n]) and np.array_equal(cut[2][1], hi[off:off + n])
    assert np.array_equal(np.concatenate([c[2][1] for c in cuts]), hi)
    with pytest.raises(da.DangxError, match="over this process's 10 pixels"):
        P._slice_ranges([(lo[:9], hi[:9])], 0, 3, 10)


class _FakeEngine:
    """What posterior_quantile_maps reads of an Engine with a per-pixel registration, over host arrays: one shard."""

    def __init__(self, npix, seed, reg):
        rng = np.random.default_rng(seed)
        self.component_list = [da.DangComps(label="dust", type="mbb", nu_ref=353.0, nindices=2, ind_label=["beta", "T"])]
        self.ddata = da.DangData(sig_map=None, rms_map=None, masks=np.ones((3, npix)))
        self.npix, self._moment_hist = npix, reg
        self.lo, self.hi = rng.uniform(0, 1, npix), rng.uniform(2, 3, npix)
        self.lo[0] = self.hi[0] = np.nan
        self.range_asked = []

    def moments_count(self):
        return 7

    def moments_hist_stat(self, reg, stat, q=None):
        return np.full((3, self.npix) if stat == "quantile" else (self.npix,), float(reg))

    def moments_hist_range_get(self, reg):
        self.range_asked.append(reg)
        return self.lo.copy(), self.hi.copy()


def test_quantile_maps_keys_range_and_sections_of_a_per_pixel_registration():
    reg = {"planes": [(0, 1, 0), (0, 0, 0)], "ranges": [(1.0, 2.0), None], "nbins": 32, "bits": 16, "kinds": ["global", "pixel"]}
    engs = [_FakeEngine(5, 1, dict(reg)), _FakeEngine(4, 2, dict(reg))]
    out = da.posterior_quantile_maps(None, engines=engs)
    assert list(out) == [("dust", "beta", 0), ("dust", "amplitude", 0)]
    assert out[("dust", "beta", 0)]["range"] == (1.0, 2.0)
    lo, hi = out[("dust", "amplitude", 0)]["range"]                   # the pair of maps, shards side by side
    assert np.array_equal(lo, np.concatenate([e.lo for e in engs]), equal_nan=True)
    assert np.array_equal(hi, np.concatenate([e.hi for e in engs]), equal_nan=True)
    assert all(e.range_asked == [1] for e in engs)                    # asked of the per-pixel registration only
    assert out[("dust", "amplitude", 0)]["q"].shape == (3, 9) and out[("dust", "amplitude", 0)]["nbins"] == 32
    # the sections: HIST_RANGE exists for the per-pixel registration alone, is owned (saved and restored), and travels only where
    # a statistic needs range values
    items = P.HIST.items(engs[0], reg)
    assert [it[2] for it in items] == ["global", "pixel"]
    assert P.HIST.sections(items[0], ["quantile", "mode", "n"]) == [(L.SEC_HIST, 0, 0, False)]
    assert P.HIST.sections(items[1], ["quantile", "mode", "n"]) == [(L.SEC_HIST, 1, 0, False), (L.SEC_HIST_RANGE, 1, 0, False)]
    assert P.HIST.sections(items[1], ["n"]) == [(L.SEC_HIST, 1, 0, False)]
    assert P.RANK.sections(P.RANK.items(engs[0], reg)[1], ["bulk", "folded", "max"]) == [(L.SEC_HIST, 1, 0, False)]
    assert [s[:3] for it in items for s in P.HIST.own(it)] == [(L.SEC_HIST, 0, 0), (L.SEC_HIST, 1, 0), (L.SEC_HIST_RANGE, 1, 0)]
    engs[0]._moment_sel = np.zeros(1, dtype=np.int32)                 # nothing selected: the histogram family's sections alone
    assert P.own_sections(engs[0]) == [(L.SEC_HIST, 0, 0), (L.SEC_HIST, 1, 0), (L.SEC_HIST_RANGE, 1, 0)]
    # the rank maps need no range values and move no HIST_RANGE: where every chain of a shard is a holder nobody holds the maps, and
    # 'range' is None instead of a read-out that must fail; one chain with accumulators of its own is enough to give the maps
    class _Src:
        pass

    src = _Src()
    src.shards = [[engs[0]], [engs[1]]]
    for e in engs:
        e._moment_holder = True
        e.range_asked = []
    assert P._hist_range(src, reg, 1, False) is None and all(e.range_asked == [] for e in engs)
    assert P._hist_range(src, reg, 0, False) == (1.0, 2.0)             # a global range is in the mirror
    lo2, hi2 = P._hist_range(src, reg, 1, True)                        # quantile / mode: HIST_RANGE was fetched into the holders
    assert np.array_equal(lo2, lo, equal_nan=True) and np.array_equal(hi2, hi, equal_nan=True)
    engs[1]._moment_holder = False
    assert P._hist_range(src, reg, 1, False) is None                  # shard 0 still has holders only
    engs[0]._moment_holder = False
    assert np.array_equal(P._hist_range(src, reg, 1, False)[0], lo, equal_nan=True)
    # a signal as the source: keyed as posterior_signal_maps keys it, (component label, band label, kind)
    class _Band:
        def __init__(self, label):
            self.label = label

    sreg = {"planes": [(1, L.HIST_SIGNAL, 0), (0, 2, 0), (0, L.HIST_SIGNAL, 0)], "ranges": [(0.0, 5.0), (10.0, 40.0), None], "nbins": 32,
            "bits": 16, "kinds": ["global", "global", "pixel"], "sources": ["signal", "plane", "signal"]}
    for e in engs:
        e._moment_hist, e._moment_signals, e.bands = dict(sreg), [(0, 1, 3), (0, 0, 1)], [_Band("030"), _Band("353")]
        e._moment_holder = False
    out = da.posterior_quantile_maps(None, engines=engs)
    assert list(out) == [("dust", "030", "Q"), ("dust", "T", 0), ("dust", "353", "P")]
    assert out[("dust", "030", "Q")]["range"] == (0.0, 5.0) and len(out[("dust", "353", "P")]["range"]) == 2
    assert P._hist_plane(("signal", 4)) == (4, L.HIST_SIGNAL, 0) and P._hist_plane((1, 0, 2)) == (1, 0, 2)
    # a mirror without kinds (what a caller's stand-in engine may hold) means global ranges
    old = {"planes": [(0, 1, 0)], "ranges": [(1.0, 2.0)], "nbins": 32, "bits": 16}
    assert [it[2] for it in P.HIST.items(engs[0], old)] == ["global"]
    assert L.SECTION_NAMES[L.SEC_HIST_RANGE] == "HIST_RANGE" and L.SEC_HIST_RANGE == 6
