"""Posterior pair / lag-1 statistics, host side: the default pair list of what a run samples, posterior_pair_maps' assembly and
masked-pixel fill on host arrays, and the device-free part of the C side (pair validation, the lag-1 update of the template rows)
as a stand-alone program under the address and undefined-behaviour sanitizers.  No device needed."""
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

# label -> (planes its set lives on, pairs of `what` per plane in the order default_moment_pairs gives them): amplitude against
# every sampled index, then index 0 against index 1.  synth.PHYS: ff T_e, ame w and both dust2 indices are fixed.
AB, AT, BT = (0, 1), (0, 2), (1, 2)
EXPECT = {
    "cmb": ((T,), ()), "synch": ((T,), (AB,)), "dust": ((T,), (AB, AT, BT)), "ff": ((T,), ()), "ame": ((T,), (AB,)), "dust2": ((T,), ()),
    "cmb_P": ((Q, U), ()), "synch_P": ((Q, U), (AB,)), "dust_P": ((Q, U), (AB, AT, BT)), "ff_P": ((Q, U), ()),
    "ame_P": ((Q, U), (AB,)), "dust2_P": ((Q, U), ()),
}


def _expected(comps):
    return [((l, wa, k), (l, wb, k)) for l, c in enumerate(comps) for k in EXPECT[c.label][0] for wa, wb in EXPECT[c.label][1]]


@pytest.mark.parametrize("config", ["C1", "C2", "C3", "C5"])
def test_default_pairs_of_the_synthetic_models(config):
    dpar, ddata, bands, comps, meta = synth.make_sky(config, nside=1)
    sel = da.default_moment_selection(dpar, comps)
    pairs = da.default_moment_pairs(dpar, comps, sel)
    assert pairs == _expected(comps)
    assert len(set(pairs)) == len(pairs) <= L.MAX_PAIRS
    if config == "C1":      # synch, dust on T alone
        assert pairs == [((0, 0, 0), (0, 1, 0)), ((1, 0, 0), (1, 1, 0)), ((1, 0, 0), (1, 2, 0)), ((1, 1, 0), (1, 2, 0))]
    if config == "C3":      # 3 of the synchrotron, 9 of the dust
        labels = [comps[a[0]].label.split("_")[0] for a, b in pairs]
        assert len(pairs) == 12 and labels.count("synch") == 3 and labels.count("dust") == 9


def test_default_pairs_follow_the_flags():
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=1, device="cpu", as_numpy=False)
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4))
    synth.add_monopole(ddata, comps, meta, fit_bands=(0, 4))
    sel = da.default_moment_selection(dpar, comps)
    base = da.default_moment_pairs(dpar, comps, sel)
    assert base == _expected(comps[:-2])                       # the template and the monopole take part in no pair
    comps[1].sample_amplitude = False                          # synch: index only
    comps[2].sample_index = [True, False]                      # dust: T fixed
    comps[5].pol_flag = [[L.FLAG_Q], [L.FLAG_U]]               # dust_P: beta on Q, T on U
    dpar.cg_groups[1].pol_flag = [L.FLAG_Q, L.FLAG_U]
    sel = da.default_moment_selection(dpar, comps)
    pairs = da.default_moment_pairs(dpar, comps, sel)
    assert [p for p in pairs if p[0][0] == 1] == []            # no amplitude plane, one index: nothing to pair
    assert [p for p in pairs if p[0][0] == 2] == [((2, 0, T), (2, 1, T))]
    assert [p for p in pairs if p[0][0] == 5] == [((5, 0, Q), (5, 1, Q)), ((5, 0, U), (5, 2, U))]   # never beta against T
    assert [p for p in pairs if p[0][0] == 4] == [((4, 0, Q), (4, 1, Q)), ((4, 0, U), (4, 1, U))]   # synch_P as before
    dpar.cg_groups = [g for g in dpar.cg_groups if g.cg_group != 2]   # no group samples the polarisation amplitudes
    sel = da.default_moment_selection(dpar, comps)
    pairs = da.default_moment_pairs(dpar, comps, sel)
    assert [p for p in pairs if p[0][0] in (4, 5)] == []


class _FakeEngine:
    """What posterior_pair_maps (and posterior_maps with lag-1) reads of an Engine, over host arrays: one shard."""

    def __init__(self, comps, masks, corr, cov, pairs, lag1=True):
        self.component_list, self.ddata = comps, da.DangData(sig_map=None, rms_map=None, masks=masks)
        self._corr, self._cov, self._moment_pairs, self._moment_lag1 = corr, cov, pairs, lag1
        self._moment_sel = np.array([1 | (1 << 3) | (1 << 6)], dtype=np.int32)
        self.npix = masks.shape[1]

    def moments_count(self):
        return 7

    def moments_get_pair(self, p, stat, ddof=0):
        return (self._corr if stat == "corr" else self._cov)[p].copy() * (1.0 if stat == "corr" else 7.0 / (7 - ddof))

    def moments_get(self, l, what, stat, ddof=0):
        return np.full((3, self.npix), {"mean": 1.0, "std": 2.0, "rho1": 0.25, "ess": 4.2}[stat])


def _shard(rng, npix, masked, pairs, lag1=True):
    comps = [da.DangComps(label="dust", type="mbb", nu_ref=353.0, nindices=2, ind_label=["beta", "T"])]
    masks = np.ones((3, npix))
    masks[0, masked] = 0.0
    corr = [rng.uniform(-1, 1, npix) for _ in pairs]
    cov = [rng.standard_normal(npix) for _ in pairs]
    return _FakeEngine(comps, masks, corr, cov, pairs, lag1)


def test_posterior_pair_maps_fill_and_assembly_on_host_arrays():
    rng = np.random.default_rng(2)
    pairs = [((0, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 2, 0))]
    engs = [_shard(rng, 5, [1, 4], pairs), _shard(rng, 4, [0], pairs)]
    keys = [(("dust", "amplitude", 0), ("dust", "beta", 0)), (("dust", "beta", 0), ("dust", "T", 0))]
    plain = da.posterior_pair_maps(None, engines=engs)
    assert list(plain) == keys
    for p, key in enumerate(keys):
        assert np.array_equal(plain[key], np.concatenate([e._corr[p] for e in engs]))
    cov = da.posterior_pair_maps(None, stat="cov", ddof=1, engines=engs)
    for p, key in enumerate(keys):
        assert np.array_equal(cov[key], np.concatenate([e._cov[p] for e in engs]) * (7.0 / 6.0))
    unseen = -1.6375e30
    filled = da.posterior_pair_maps(None, masked_value=unseen, engines=engs)
    masked = np.zeros(9, dtype=bool)
    masked[[1, 4, 5]] = True
    for key in keys:
        assert (filled[key][masked] == unseen).all() and np.array_equal(filled[key][~masked], plain[key][~masked])
    # posterior_maps: rho1 and ess appear exactly when lag-1 is tracked, masked like the others
    pm = da.posterior_maps(None, masked_value=unseen, engines=engs)
    for key in (("dust", "amplitude"), ("dust", "beta"), ("dust", "T")):
        assert set(pm[key]) == {"n", "mean", "std", "rho1", "ess"}
        assert (pm[key]["rho1"][:, masked] == unseen).all() and (pm[key]["ess"][:, ~masked] == 4.2).all()
    for e in engs:
        e._moment_lag1 = False
    assert set(da.posterior_maps(None, engines=engs)[("dust", "beta")]) == {"n", "mean", "std"}
    del engs[0]._moment_pairs
    with pytest.raises(da.DangxError, match="moments_pairs was not called"):
        da.posterior_pair_maps(None, engines=engs)


HOST_MAIN = r"""
#include "dx_moments_host.h"
#include <cstdio>
#include <vector>
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool has(const std::string& s, const char* w) { return s.find(w) != std::string::npos; }
int main() {
    // two components: 0 = mbb with two indices, everything on T selected; 1 = a template with rows Q, U selected
    const int32_t sel[2] = {1 | (1 << 3) | (1 << 6), 6};
    const int nind[2] = {2, 0}, global[2] = {0, 1};
    std::vector<int32_t> ok = {0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 2, 0};
    CHECK(dx_pairs_check(2, ok.data(), 2, 3, sel, nind, global).empty());
    CHECK(dx_pairs_check(0, nullptr, 2, 3, sel, nind, global).empty());
    CHECK(has(dx_pairs_check(1, nullptr, 2, 3, sel, nind, global), "no pair list"));
    std::vector<int32_t> p = ok;
    p[9] = 0; p[10] = 1; p[11] = 0;
    CHECK(has(dx_pairs_check(2, p.data(), 2, 3, sel, nind, global), "a == b"));
    p = ok; p[2] = 1;
    CHECK(has(dx_pairs_check(2, p.data(), 2, 3, sel, nind, global), "not selected"));
    p = ok; p[3] = 1; p[4] = 0; p[5] = 1;
    CHECK(has(dx_pairs_check(2, p.data(), 2, 3, sel, nind, global), "template"));
    p = ok; p[0] = 2;
    CHECK(has(dx_pairs_check(2, p.data(), 2, 3, sel, nind, global), "component index"));
    p = ok; p[4] = 3;
    CHECK(has(dx_pairs_check(2, p.data(), 2, 3, sel, nind, global), "what"));
    p = ok; p[5] = 3;
    CHECK(has(dx_pairs_check(2, p.data(), 2, 3, sel, nind, global), "plane out of range"));
    std::vector<int32_t> many;
    for (int i = 0; i < 65; ++i) many.insert(many.end(), ok.begin(), ok.begin() + 6);
    CHECK(dx_pairs_check(64, many.data(), 2, 3, sel, nind, global).empty());
    CHECK(has(dx_pairs_check(65, many.data(), 2, 3, sel, nind, global), "DANGX_MAX_PAIRS"));
    // the lag-1 update of a template row against the two-pass definition in long double, at an offset 1e6 times the spread
    for (double offs : {0.0, -3.1, 1.0e6}) {
        const int n = 64;
        std::vector<double> x(n);
        unsigned long long s = 12345;
        double v = 0.0;
        for (int t = 0; t < n; ++t) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const double u = (double)(s >> 11) / 9007199254740992.0 - 0.5;
            if (t % 2 == 0) v = 0.6 * v + 3.0 * u;     // every other step held
            x[t] = offs + v;
        }
        double mean = 0.0, m2 = 0.0, prev = 0.0, first = 0.0, P = 0.0;
        for (int t = 0; t < n; ++t) {
            if (t == 0) prev = first = x[t]; else dx_lag_update(x[t], prev, first, P);
            const double d = x[t] - mean;
            mean = std::fma(d, 1.0 / (t + 1), mean);
            m2 = std::fma(d, x[t] - mean, m2);
        }
        long double mu = 0, q = 0, c = 0, big = 0;
        for (double xi : x) { mu += xi; if (std::fabs(xi) > big) big = std::fabs(xi); }
        mu /= n;
        for (int t = 0; t < n; ++t) { q += (x[t] - mu) * (x[t] - mu); if (t) c += (x[t] - mu) * (x[t - 1] - mu); }
        const double rho = dx_lag_rho1(mean, m2, prev, first, P, n), ref = (double)(c / q);
        const double tol = 16.0 * n * 2.220446049250313e-16 * (1.0 + (double)(big / sqrtl(q / n)));
        CHECK(std::fabs(rho - ref) <= tol);
        CHECK(rho > 0.1);
        const double ess = dx_lag_ess(rho, n);
        CHECK(std::fabs(ess - n * (1 - ref) / (1 + ref)) <= 2 * n * tol);
    }
    // a row that never moved, and n = 1: 0/0
    CHECK(std::isnan(dx_lag_rho1(5.0, 0.0, 5.0, 5.0, 0.0, 1.0)) && std::isnan(dx_lag_ess(dx_lag_rho1(5.0, 0.0, 5.0, 5.0, 0.0, 9.0), 9.0)));
    CHECK(dx_lag_ess(-0.5, 10.0) == 10.0);
    CHECK(dx_pair_update(3.0, 4.0, 0.0, 0.0, 0.0, 1.0) == 0.0);      // n = 1: the covariance is exactly 0
    std::printf(bad ? "host part: %d checks failed\n" : "host part ok\n", bad);
    return bad ? 1 : 0;
}
"""


def test_host_part_under_sanitizers(tmp_path):
    """Pair validation and the template rows' lag-1 update (dang_amd/csrc/dx_moments_host.h, what dangx_moments.hip runs on the
    host) in a program of their own, compiled with -fsanitize=address,undefined and run once on the CPU."""
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
