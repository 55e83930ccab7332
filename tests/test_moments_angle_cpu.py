"""Posterior polarisation angle, host side: the default angle list of what a run samples (one angle per default P signal),
posterior_angle_maps' assembly on host arrays, the fingerprint of a registration without angles (unchanged, restated from the
values the section layer gave before angles existed) and dang_amd/csrc/dx_angle_host.h -- the check of an angle list, the
grouping into segments of at most 8 bands, the sample's direction cosines, the read-out of one chain and of several -- as a
stand-alone program under the address and undefined-behaviour sanitizers.  No device needed; nothing is loaded into Python under
a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nearest(bands, nu_ref_ghz):
    d = [abs(b.nu_c - nu_ref_ghz) for b in bands]
    return d.index(min(d))


def test_default_angles_of_a_c3_shaped_model():
    """C3: synch_P at the band nearest 30 GHz and dust_P at the band nearest 353 GHz; nothing on T, nothing for cmb_P or ff_P."""
    dpar, ddata, bands, comps, meta = synth.make_sky("C3", nside=1)
    lab = [c.label for c in comps]
    bs, bd = _nearest(bands, 30.0), _nearest(bands, 353.0)
    specs = da.default_angle_specs(dpar, comps, bands)
    assert specs == [(lab.index("synch_P"), bs), (lab.index("dust_P"), bd)] == [(5, 1), (6, 7)]
    # one angle for every P of default_signal_specs, in its order; that list itself is what it was
    sig = da.default_signal_specs(dpar, comps, bands)
    assert specs == [(l, j) for l, j, k in sig if k == 3] and len(sig) == 8
    assert len(specs) <= L.MAX_ANGLES == 64


def test_default_angles_of_a_c5_shaped_model():
    """C5 adds ame_P (nu_p sampled); dust2_P (both indices fixed) and ff_P do not join."""
    dpar, ddata, bands, comps, meta = synth.make_sky("C5", nside=1)
    lab = [c.label for c in comps]
    want = [(lab.index(n), _nearest(bands, nu)) for n, nu in (("synch_P", 30.0), ("dust_P", 353.0), ("ame_P", 22.0))]
    assert da.default_angle_specs(dpar, comps, bands) == sorted(want) == want
    dpar.cg_groups[1].pol_flag = [L.FLAG_Q]                            # the Q+U group solves Q alone: no P, so no angle
    assert da.default_angle_specs(dpar, comps, bands) == []


class _FakeEngine:
    """What posterior_angle_maps reads of an Engine, over host arrays: one shard."""

    def __init__(self, comps, bands, masks, maps, reg, count=5):
        self.component_list, self.bands, self.ddata = comps, bands, da.DangData(sig_map=None, rms_map=None, masks=masks)
        self._maps, self._moment_angles, self._count = maps, reg, count

    def moments_count(self):
        return self._count

    def moments_get_angle(self, a, stat):
        return self._maps[stat][a].copy()


def test_posterior_angle_maps_fill_and_assembly_on_host_arrays():
    rng = np.random.default_rng(11)
    comps = [da.DangComps(label="synch_P", type="power-law", nu_ref=30.0, nindices=1, ind_label=["beta"])]
    bands = [da.BandInfo(label="bp_030", nu_c=30.0), da.BandInfo(label="bp_044", nu_c=44.0)]
    reg = [(0, 1), (0, 0)]

    def shard(npix, masked):
        masks = np.ones((3, npix))
        masks[0, masked] = 0.0
        maps = {st: [rng.uniform(0, 1, npix) for _ in reg] for st in ("psi", "psi_std", "R")}
        return _FakeEngine(comps, bands, masks, maps, list(reg))
    engs = [shard(5, [1]), shard(4, [0, 3])]
    plain = da.posterior_angle_maps(None, engines=engs)
    keys = [("synch_P", "bp_044"), ("synch_P", "bp_030")]
    assert list(plain) == keys
    for a, key in enumerate(keys):
        assert set(plain[key]) == {"n", "psi", "psi_std", "R"} and plain[key]["n"] == 5
        for st in ("psi", "psi_std", "R"):
            assert np.array_equal(plain[key][st], np.concatenate([e._maps[st][a] for e in engs]))
    filled = da.posterior_angle_maps(None, masked_value=-1.6375e30, engines=engs)
    masked = np.zeros(9, dtype=bool)
    masked[[1, 5, 8]] = True
    for key in keys:
        assert (filled[key]["psi"][masked] == -1.6375e30).all() and np.array_equal(filled[key]["psi"][~masked], plain[key]["psi"][~masked])
    engs[1]._moment_angles = reg[:1]
    with pytest.raises(da.DangxError, match="different angle registrations"):
        da.posterior_angle_maps(None, engines=engs)
    engs[1]._moment_angles = list(reg)
    engs[1]._count = 6
    with pytest.raises(da.DangxError, match="different sample counts"):
        da.posterior_angle_maps(None, engines=engs)
    engs[0]._moment_angles = None
    with pytest.raises(da.DangxError, match="moments_angles was not called"):
        da.posterior_angle_maps(None, engines=engs)


def test_the_python_layer_names_the_new_family_and_codes():
    assert L.SEC_ANGLE == 7 and L.SECTION_NAMES[L.SEC_ANGLE] == "ANGLE" and len(L.SECTION_NAMES) == 8
    assert L.K_ANGLE == 12 and L.KERNEL_NAMES[L.K_ANGLE] == "k_angle"
    assert L.ANGLE_STAT_CODES == {"psi": 0, "psi_std": 1, "R": 2, "C": 3, "S": 4, "between": 5}
    from dang_amd import api, posterior
    assert api.MOMENT_ATTRS[-1] == "_moment_angles"
    assert "posterior_angle_maps" not in posterior.__all__ and da.posterior_angle_maps is posterior.posterior_angle_maps
    assert posterior.FAMILIES["angle"].reg == "angles"


HOST_MAIN = r"""
#include "dx_angle_host.h"
#include "dx_section_host.h"
#include <cfloat>
#include <cstdio>
#include <limits>
#include <vector>
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool has(const std::string& s, const char* w) { return s.find(w) != std::string::npos; }
static double ulps(double got, long double want) { return (double)(std::fabs((long double)got - want) / ((long double)DBL_EPSILON * std::fabs(want))); }

// the registration of tests/test_sections_cpu.py's base case (v = 0) and of its variant 14 (another signal spec)
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
    return r;
}

int main() {
    const double PI = 3.14159265358979323846, NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
    // ---- the check.  four components: 0 = diffuse, 1 = a template, 2 = not set, 3 = T_cmb; 20 bands
    const int set[4] = {1, 1, 0, 1}, global[4] = {0, 1, 0, 0}, tcmb[4] = {0, 0, 0, 1};
    auto chk = [&](const std::vector<int32_t>& sp, int nmaps = 3) {
        return dx_angle_check((int)(sp.size() / 2), sp.data(), 4, 20, nmaps, set, global, tcmb);
    };
    CHECK(chk({0, 0, 0, 19, 0, 7}).empty());
    CHECK(dx_angle_check(0, nullptr, 4, 20, 3, set, global, tcmb).empty());
    CHECK(dx_angle_check(0, nullptr, 4, 20, 1, set, global, tcmb).empty());      // an empty list drops the registration on any model
    CHECK(has(dx_angle_check(1, nullptr, 4, 20, 3, set, global, tcmb), "no angle list"));
    CHECK(has(dx_angle_check(-1, nullptr, 4, 20, 3, set, global, tcmb), "negative"));
    CHECK(has(chk({0, 0}, 1), "nmaps == 3") && has(chk({0, 0}, 2), "nmaps == 3"));
    CHECK(has(chk({4, 0}), "component index") && has(chk({-1, 0}), "component index"));
    CHECK(has(chk({0, 20}), "band index") && has(chk({0, -1}), "band index"));
    CHECK(has(chk({2, 0}), "not set"));
    CHECK(has(chk({1, 0}), "template / monopole / hi_fit"));
    CHECK(has(chk({3, 0}), "T_cmb") && has(chk({3, 0}), "no direction"));
    CHECK(has(chk({0, 3, 0, 4, 0, 3}), "angle 2: the same angle twice"));
    std::vector<int32_t> many;
    for (int a = 0; a < 65; ++a) { many.push_back(0); many.push_back(a % 20); }
    CHECK(has(dx_angle_check(65, many.data(), 4, 20, 3, set, global, tcmb), "DANGX_MAX_ANGLES"));
    CHECK(has(dx_angle_check(64, many.data(), 4, 20, 3, set, global, tcmb), "the same angle twice"));   // the limit comes first, then the list
    // the stat: 0..5, and 5 only over several chains
    CHECK(has(dx_angle_stat_check(6, 3), "the stat of an angle must be") && has(dx_angle_stat_check(-1, 1), "the stat of an angle must be"));
    CHECK(has(dx_angle_stat_check(5, 1), "needs several chains") && dx_angle_stat_check(5, 2).empty());
    for (int st = 0; st < 5; ++st) CHECK(dx_angle_stat_check(st, 1).empty() && dx_angle_stat_check(st, 8).empty());
    // ---- the plan: 9 bands of one component give segments of 8 + 1, whatever the list order; components ascending
    std::vector<int32_t> sp = {3, 5};
    for (int j = 8; j >= 0; --j) { sp.push_back(0); sp.push_back(2 * j); }      // component 0 at bands 16, 14, .. 0
    std::vector<DxAngSeg> plan = dx_angle_plan(10, sp.data(), 4, 20);
    CHECK(plan.size() == 3 && plan[0].comp == 0 && plan[0].nb == 8 && plan[1].comp == 0 && plan[1].nb == 1 && plan[2].comp == 3 && plan[2].nb == 1);
    if (plan.size() == 3) {
        for (int b = 0; b < 8; ++b) CHECK(plan[0].band[b] == 2 * b && plan[0].ang[b] == 9 - b);
        CHECK(plan[1].band[0] == 16 && plan[1].ang[0] == 1 && plan[2].band[0] == 5 && plan[2].ang[0] == 0);
    }
    CHECK(dx_angle_plan(9, sp.data(), 4, 20).size() == 2 && dx_angle_plan(0, nullptr, 4, 20).empty());   // exactly 8 of component 0: no empty segment behind
    // ---- the read-out of one chain at the axes
    CHECK(dx_angle_stat(0, 1.0, 0.0) == 0.0);
    CHECK(dx_angle_stat(0, 0.0, 1.0) == 0.5 * std::atan2(1.0, 0.0) && std::fabs(dx_angle_stat(0, 0.0, 1.0) - PI / 4) <= 1e-16);
    CHECK(dx_angle_stat(0, -1.0, +0.0) == 0.5 * std::atan2(+0.0, -1.0) && dx_angle_stat(0, -1.0, +0.0) > 0 && std::fabs(dx_angle_stat(0, -1.0, +0.0) - PI / 2) <= 2.3e-16);
    CHECK(dx_angle_stat(0, -1.0, -0.0) == -dx_angle_stat(0, -1.0, +0.0));
    CHECK(dx_angle_stat(0, 0.0, -1.0) == -dx_angle_stat(0, 0.0, 1.0));
    CHECK(dx_angle_stat(3, 0.25, -0.5) == 0.25 && dx_angle_stat(4, 0.25, -0.5) == -0.5);
    // the clamp: sqrt(2)/2 rounded up squares to more than 1/2 and the sum of squares to 1 + eps; with a resultant that rounds
    // to more than 1 the std would be sqrt of a negative number, NaN, where the chain never moved
    const double h = 0.70710678118654757, tiny = 3e-8;
    CHECK(h * h + h * h > 1.0 && std::sqrt(1.0 + tiny * tiny) > 1.0);
    CHECK(dx_angle_stat(2, h, h) == 1.0 && dx_angle_stat(1, h, h) == 0.0 && dx_angle_stat(1, 1.0, 0.0) == 0.0);
    CHECK(dx_angle_stat(2, 1.0, tiny) == 1.0 && dx_angle_stat(1, 1.0, tiny) == 0.0 && dx_angle_stat(1, -tiny, -1.0) == 0.0);
    CHECK(dx_angle_stat(2, 0.0, 0.0) == 0.0 && dx_angle_stat(1, 0.0, 0.0) == INF);
    // below 1 the clamp cuts nothing: a unit vector's length comes out as low as 1 - 5u (u = 2^-53, DX_ANG_UNIT_SLACK), and the
    // spread is exactly +0 down to there and the stated expression from the next double on
    const double u = std::ldexp(1.0, -53);
    CHECK(DX_ANG_UNIT_SLACK == 5);
    for (int k = 0; k <= 5; ++k) CHECK(dx_angle_spread(1.0 - k * u) == 0.0 && !std::signbit(dx_angle_spread(1.0 - k * u)));
    CHECK(dx_angle_spread(1.0 - 6 * u) == 0.5 * std::sqrt(-2.0 * std::log(1.0 - 6 * u)) && dx_angle_spread(1.0 - 6 * u) > 1.8e-8);
    CHECK(dx_angle_stat(2, 1.0 - u, 0.0) == 1.0 - u && dx_angle_stat(1, 1.0 - u, 0.0) == 0.0);       // R itself stays what it is
    CHECK(std::isnan(dx_angle_spread(NaN)) && dx_angle_spread(0.0) == INF);
    {   // a unit vector made as a sample is made, at the angle of the issue's fixed pixels and at others: the std is 0 every time
        int below = 0;
        for (int d = 1; d < 180; ++d)
            for (double scale : {1.0, 0.3, 7.5, 1e-3}) {
                double cc, ss;
                dx_angle_cs(scale * std::cos(2.0 * d * PI / 180.0), scale * std::sin(2.0 * d * PI / 180.0), cc, ss);
                if (dx_angle_stat(2, cc, ss) < 1.0) ++below;
                CHECK(dx_angle_stat(2, cc, ss) >= 1.0 - 5 * u && dx_angle_stat(1, cc, ss) == 0.0);
            }
        CHECK(below > 0);          // the case the clamp does not reach does occur
    }
    for (int st = 0; st < 5; ++st) CHECK(std::isnan(dx_angle_stat(st, NaN, NaN)));
    CHECK(std::isnan(dx_angle_stat(0, NaN, 0.5)) && std::isnan(dx_angle_stat(1, 0.5, NaN)) && std::isnan(dx_angle_stat(2, NaN, 0.0)));
    // ---- a sample: two IEEE divisions by the signals' own P; Q = U = 0 gives NaN
    double c, s;
    dx_angle_cs(3.0, -4.0, c, s);
    CHECK(c == 3.0 / 5.0 && s == -4.0 / 5.0);
    dx_angle_cs(0.0, 0.0, c, s);
    CHECK(std::isnan(c) && std::isnan(s));
    dx_angle_cs(-2.5, 0.0, c, s);
    CHECK(c == -1.0 && s == 0.0);
    // ---- the wrap: two samples at psi = +85 and -85 degrees.  Their arithmetic mean is 0; the circular mean is +-90 degrees
    const double p85 = 85.0 * PI / 180.0;
    double C = 0.0, S = 0.0;
    for (int t = 0; t < 2; ++t) {
        const double psi = t == 0 ? p85 : -p85;
        dx_angle_cs(2.0 * std::cos(2.0 * psi), 2.0 * std::sin(2.0 * psi), c, s);
        C = dx_angle_mean(c, C, 1.0 / (t + 1));
        S = dx_angle_mean(s, S, 1.0 / (t + 1));
    }
    CHECK(0.5 * (p85 + -p85) == 0.0);
    CHECK(std::fabs(std::fabs(dx_angle_stat(0, C, S)) - PI / 2) <= 1e-15);
    CHECK(ulps(dx_angle_stat(2, C, S), std::cos(10.0L * 3.14159265358979323846264338327950288L / 180.0L)) <= 4.0);
    {   // its std against long-double arithmetic on the same R
        const long double R = dx_angle_stat(2, C, S);
        CHECK(ulps(dx_angle_stat(1, C, S), 0.5L * std::sqrt(-2.0L * std::log(R))) <= 4.0);
    }
    // ---- three chains with unequal counts: the pooled pair and the between-chain spread against long-double arithmetic
    const long long n[3] = {7, 3, 12};
    const double deg[3] = {10.0, 40.0, 80.0}, len[3] = {0.9, 0.5, 0.75};
    double Ck[DX_ANG_MAX_CHAINS] = {}, Sk[DX_ANG_MAX_CHAINS] = {};
    for (int k = 0; k < 3; ++k) { Ck[k] = len[k] * std::cos(2.0 * deg[k] * PI / 180.0); Sk[k] = len[k] * std::sin(2.0 * deg[k] * PI / 180.0); }
    const DxAngPar par = dx_angle_par(3, n);
    CHECK(par.K == 3 && par.w[0] == 7.0 / 22.0 && par.w[1] == 3.0 / 22.0 && par.w[2] == 12.0 / 22.0 && par.kd == 3.0);
    long double Cp = 0, Sp = 0, Cb = 0, Sb = 0;
    for (int k = 0; k < 3; ++k) {
        Cp += (long double)n[k] / 22.0L * Ck[k];
        Sp += (long double)n[k] / 22.0L * Sk[k];
        const long double r = std::sqrt((long double)Ck[k] * Ck[k] + (long double)Sk[k] * Sk[k]);
        Cb += Ck[k] / r; Sb += Sk[k] / r;
    }
    Cb /= 3; Sb /= 3;
    // the stated list-order expression, every product and sum rounded to f64
    const double c_list = (par.w[0] * Ck[0] + par.w[1] * Ck[1]) + par.w[2] * Ck[2];
    CHECK(dx_angle_chains_stat(3, par, Ck, Sk) == c_list);
    // a sum of three rounded products of magnitude <= 1: three roundings of the products, two of the sums, one of each weight
    CHECK(std::fabs((long double)dx_angle_chains_stat(3, par, Ck, Sk) - Cp) <= 8 * DBL_EPSILON);
    CHECK(std::fabs((long double)dx_angle_chains_stat(4, par, Ck, Sk) - Sp) <= 8 * DBL_EPSILON);
    CHECK(std::fabs((long double)dx_angle_chains_stat(0, par, Ck, Sk) - 0.5L * std::atan2(Sp, Cp)) <= 16 * DBL_EPSILON);
    const long double Rp = std::sqrt(Cp * Cp + Sp * Sp), Rb = std::sqrt(Cb * Cb + Sb * Sb);
    CHECK(std::fabs((long double)dx_angle_chains_stat(2, par, Ck, Sk) - Rp) <= 16 * DBL_EPSILON);
    // R well inside (0, 1): d(std)/dR = -1 / (4 R std) is of order one, so the error stays a few units of R's
    CHECK(std::fabs((long double)dx_angle_chains_stat(1, par, Ck, Sk) - 0.5L * std::sqrt(-2.0L * std::log(Rp))) <= 32 * DBL_EPSILON);
    CHECK(std::fabs((long double)dx_angle_chains_stat(5, par, Ck, Sk) - 0.5L * std::sqrt(-2.0L * std::log(Rb))) <= 32 * DBL_EPSILON);
    CHECK(Rb < 0.9L && dx_angle_chains_stat(5, par, Ck, Sk) > 0.2);          // the chains do sit at different angles
    // chains at ONE direction and different lengths: between is 0 while the pooled spread is not
    double C1[DX_ANG_MAX_CHAINS] = {0.5, 0.25, 1.0}, S1[DX_ANG_MAX_CHAINS] = {0.0, 0.0, 0.0};
    CHECK(dx_angle_chains_stat(5, par, C1, S1) == 0.0 && dx_angle_chains_stat(1, par, C1, S1) > 0.0);
    S1[1] = NaN;
    CHECK(std::isnan(dx_angle_chains_stat(5, par, C1, S1)) && std::isnan(dx_angle_chains_stat(1, par, C1, S1)));
    // ---- sections: a registration without angles hashes as it did before angles existed (values of the base case and of the
    // variant with another signal spec, as the section layer gave them then); an angle changes the signals' group and only it
    uint64_t g0[DX_SEC_GROUPS], g1[DX_SEC_GROUPS];
    CHECK(dx_section_fingerprint(reg(0)) == 0x3881fd03ae980036ull && dx_section_fingerprint(reg(14)) == 0x6c4235f5e3401aaull);
    dx_section_groups(reg(0), g0);
    CHECK(g0[DX_SEC_G_SIGNALS] == 0x9819c89c69c04b01ull && g0[DX_SEC_G_BATCHES] == 0x63878ab3380bce62ull);
    DxSecReg ra = reg(0);
    ra.angles = {0, 1};
    dx_section_groups(ra, g1);
    for (int i = 0; i < DX_SEC_GROUPS; ++i) CHECK((g0[i] != g1[i]) == (i == DX_SEC_G_SIGNALS));
    CHECK(dx_section_fingerprint(ra) != dx_section_fingerprint(reg(0)));
    DxSecReg rb = reg(0);
    rb.angles = {0, 2};
    CHECK(dx_section_fingerprint(rb) != dx_section_fingerprint(ra));
    CHECK(has(dx_section_head_diff(dx_section_head(ra, 3, 4), dx_section_head(reg(0), 3, 4)), "signal or angle registrations differ"));
    CHECK(DX_SEC_FAMILIES == 8 && DX_SEC_ANGLE == 7 && std::string(dx_section_family_name(DX_SEC_ANGLE)) == "ANGLE");
    CHECK(DX_SEC_VERSION == 1u && DX_SEC_HEAD_BYTES == 104 && DX_SEC_GROUPS == 6);
    CHECK(dx_section_angle_bytes(95) == 2 * 95 * 8);
    std::printf(bad ? "host part: %d checks failed\n" : "host part ok\n", bad);
    return bad ? 1 : 0;
}
"""


def test_angle_header_under_sanitizers(tmp_path):
    """dang_amd/csrc/dx_angle_host.h and dx_section_host.h -- what dangx_moments_angles, the read-outs and the sections call -- in
    a program of its own, compiled with -fsanitize=address,undefined and run once on the CPU as a child process."""
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
