"""Read-outs over several chains, host side: the folds of dang_amd/csrc/dx_chains_host.h (what the kernels, the template rows and
this program share) in a stand-alone program under the address and undefined-behaviour sanitizers against numpy.longdouble, and
the map-assembling functions (chains_posterior_maps, ...) over fake host engines.  No device needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import api

import chains_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# reads: K, ddof, n_0 .. n_{K-1}, then per chain its samples of two series (a_t b_t) as hex floats; accumulates every chain exactly as
# the library does (Welford with fma, dx_lag_update, dx_pair_update) and prints the read-outs of dx_chains_host.h as hex floats
HOST_MAIN = r"""
#include "dx_chains_host.h"
#include <cstdio>
#include <vector>
int main() {
    int K = 0, ddof = 0;
    if (std::scanf("%d %d", &K, &ddof) != 2 || K < 2 || K > DX_CHAINS_MAX) return 2;
    long long n[DX_CHAINS_MAX] = {};
    for (int k = 0; k < K; ++k) if (std::scanf("%lld", &n[k]) != 1 || n[k] < 1) return 2;
    double ma[DX_CHAINS_MAX] = {}, qa[DX_CHAINS_MAX] = {}, mb[DX_CHAINS_MAX] = {}, qb[DX_CHAINS_MAX] = {}, C[DX_CHAINS_MAX] = {};
    double prev[DX_CHAINS_MAX] = {}, first[DX_CHAINS_MAX] = {}, P[DX_CHAINS_MAX] = {};
    for (int k = 0; k < K; ++k) {
        std::vector<double> a((size_t)n[k]), b((size_t)n[k]);   // exactly n_k long: a read past the end is an ASan report
        for (long long t = 0; t < n[k]; ++t) if (std::scanf("%la %la", &a[(size_t)t], &b[(size_t)t]) != 2) return 2;
        for (long long t = 0; t < n[k]; ++t) {
            const double inv_n = 1.0 / (double)(t + 1), x = a[(size_t)t], y = b[(size_t)t];
            C[k] = dx_pair_update(x, y, ma[k], mb[k], C[k], inv_n);      // before the means move, as the launch order has it
            if (t == 0) prev[k] = first[k] = x; else dx_lag_update(x, prev[k], first[k], P[k]);
            double d = x - ma[k]; ma[k] = std::fma(d, inv_n, ma[k]); qa[k] = std::fma(d, x - ma[k], qa[k]);
            d = y - mb[k]; mb[k] = std::fma(d, inv_n, mb[k]); qb[k] = std::fma(d, y - mb[k], qb[k]);
        }
    }
    const std::string why2 = dx_chains_count_check(K, n, DX_CH_RHAT, ddof, false), why1 = dx_chains_count_check(K, n, DX_CH_STD, ddof, false);
    std::printf("equal %d\nstd_ok %d\n", why2.empty() ? 1 : 0, why1.empty() ? 1 : 0);
    if (!why2.empty()) std::printf("why %s\n", why2.c_str());
    const DxChainsPar par = dx_chains_par(K, n, ddof);
    std::printf("mean %a\nstd %a\n", dx_chains_stat(DX_CH_MEAN, par, ma, qa), dx_chains_stat(DX_CH_STD, par, ma, qa));
    std::printf("cov %a\ncorr %a\n", dx_chains_pair(0, par, ma, mb, qa, qb, C), dx_chains_pair(1, par, ma, mb, qa, qb, C));
    if (why2.empty()) {
        std::printf("W %a\nB %a\nrhat %a\n", dx_chains_stat(DX_CH_W, par, ma, qa), dx_chains_stat(DX_CH_BN, par, ma, qa),
                    dx_chains_stat(DX_CH_RHAT, par, ma, qa));
        double ess = 0.0;
        for (int k = 0; k < K; ++k) ess = dx_chains_ess_add(ess, ma[k], qa[k], prev[k], first[k], P[k], par.cnt[k]);
        std::printf("ess %a\n", ess);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("chains_host")
    src, exe = tmp / "host_main.cpp", tmp / "host_main"
    src.write_text(HOST_MAIN)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "dang_amd", "csrc"), "-o", str(exe), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and ("cannot find" in r.stdout or "unsupported" in r.stdout):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stdout
    return str(exe)


def _run(exe, xa, xb, ddof=0):
    lines = ["%d %d" % (len(xa), ddof), " ".join(str(len(x)) for x in xa)]
    for a, b in zip(xa, xb):
        lines += ["%s %s" % (float(u).hex(), float(v).hex()) for u, v in zip(a, b)]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = {}
    for ln in r.stdout.splitlines():
        key, val = ln.split(" ", 1)
        out[key] = val if key == "why" else (int(val) if key in ("equal", "std_ok") else float.fromhex(val))
    return out


def _ar1(rng, n, offset, spread=3.0, coef=0.6, hold=0.5):
    x = np.empty(n)
    v = rng.standard_normal() * spread
    for t in range(n):
        if t and rng.random() >= hold:
            v = coef * v + np.sqrt(1 - coef * coef) * spread * rng.standard_normal()
        x[t] = offset + v
    return x


OFFSETS = (0.0, -3.1, 1.0e6)
COUNTS = [(5, 64, 2), (64, 64, 64), (1, 3, 1, 7, 2, 1, 5, 4), (4,) * 8, (1, 1), (2, 2)]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "n" + "_".join(map(str, c)))
def test_folds_under_sanitizers_against_long_double(host_exe, counts, offset):
    rng = np.random.default_rng(len(counts) * 1000 + sum(counts))
    xa = [_ar1(rng, n, offset + 0.7 * k) for k, n in enumerate(counts)]          # the chains sit in different places
    xb = [_ar1(rng, n, OFFSETS[(OFFSETS.index(offset) + 1) % 3] - 0.4 * k) + 0.5 * (a - offset) for k, (n, a) in enumerate(zip(counts, xa))]
    for ddof in (0, 1):
        got = _run(host_exe, xa, xb, ddof)
        N = sum(counts)
        assert got["std_ok"] == (1 if N - ddof > 0 else 0)
        pm = cr.pooled([x[:, None] for x in xa], ddof) if N - ddof > 0 else None
        if pm:
            cr.compare(np.array([got["mean"]]), *pm["mean"], "pooled mean %s %g" % (counts, offset))
            cr.compare(np.array([got["std"]]), *pm["std"], "pooled std ddof %d %s %g" % (ddof, counts, offset))
            pp = cr.pooled_pair([x[:, None] for x in xa], [x[:, None] for x in xb], ddof)
            cr.compare(np.array([got["corr"]]), *pp["corr"], "pooled corr %s %g" % (counts, offset))
            cr.compare(np.array([got["cov"]]), *pp["cov"], "pooled cov ddof %d %s %g" % (ddof, counts, offset))
        equal = len(set(counts)) == 1 and counts[0] >= 2
        assert got["equal"] == (1 if equal else 0)
        if not equal:
            assert ("equal sample counts" in got["why"] and "chain " in got["why"]) or "at least 2 samples" in got["why"]
            assert "rhat" not in got
            continue
        bw = cr.between([x[:, None] for x in xa])
        cr.compare(np.array([got["W"]]), *bw["W"], "W %s %g" % (counts, offset))
        cr.compare(np.array([got["B"]]), *bw["B"], "B/n %s %g" % (counts, offset))
        cr.compare_rhat(np.array([got["rhat"]]), bw, "R-hat^2 %s %g" % (counts, offset))
        cr.compare(np.array([got["ess"]]), *bw["ess"], "pooled ESS %s %g" % (counts, offset))


def test_closed_forms_and_the_degenerate_elements(host_exe):
    """chain k holds (t + c k) s + off, t = 0..7: W = 6 s^2, B/n = (5/3) c^2 s^2, R-hat^2 = 7/8 + 5 c^2 / 18; a series that
    never moved gives NaN, chains that differ in their means alone +inf"""
    for c in (0, 1, 4):
        for s in (0.25, 1.0, 8.0):
            xa = [(np.arange(8) + c * k) * s for k in range(4)]
            got = _run(host_exe, xa, xa)
            assert got["W"] == 6 * s * s
            assert abs(got["B"] - 5 * c * c * s * s / 3) <= 64 * cr.EPS * 5 * c * c * s * s / 3
            assert abs(got["rhat"] ** 2 - (7 / 8 + 5 * c * c / 18)) <= 64 * cr.EPS * (7 / 8 + 5 * c * c / 18)
            assert got["mean"] == (3.5 + 1.5 * c) * s and got["corr"] == 1.0
    flat = _run(host_exe, [np.full(8, 2.5)] * 4, [np.arange(8.0)] * 4)
    assert flat["W"] == 0 and flat["B"] == 0 and np.isnan(flat["rhat"]) and np.isnan(flat["ess"]) and np.isnan(flat["corr"])
    assert flat["mean"] == 2.5 and flat["std"] == 0 and flat["cov"] == 0
    apart = _run(host_exe, [np.full(8, 2.5 + k) for k in range(4)], [np.arange(8.0)] * 4)
    assert apart["W"] == 0 and apart["B"] == 5 / 3 and apart["rhat"] == np.inf and np.isnan(apart["ess"])


# ---- the map-assembling functions over fake host engines

class _FakeEngine:
    """What the chains_*_maps functions read of an Engine: one shard of one chain.  value: what this chain's accumulators 'hold'."""

    def __init__(self, masks, value, count=7, lag1=True, nbands=2):
        self.component_list = [da.DangComps(label="dust", type="mbb", nu_ref=353.0, nindices=2, ind_label=["beta", "T"]),
                               da.DangComps(label="mono", type="monopole", nu_ref=353.0)]
        self.bands = [da.BandInfo(label="b%d" % j, nu_c=30.0 * (j + 1)) for j in range(nbands)]
        self.ddata = da.DangData(sig_map=None, rms_map=None, masks=masks)
        self._moment_sel = np.array([1 | (6 << 3), 1], dtype=np.int32)     # dust: amplitude T, beta Q+U; the monopole's row T
        self._moment_lag1, self._count, self.value = lag1, count, value
        self._moment_pairs = [((0, 0, 0), (0, 1, 1))]
        self._moment_hist = {"planes": [(0, 1, 1)], "ranges": [(1.0, 2.0)], "nbins": 16, "bits": 16}
        self._moment_signals = [(0, 1, 0), (0, 0, 3)]
        self.npix, self.nmaps, self.nbands = masks.shape[1], 3, nbands

    def moments_count(self):
        return self._count


STAT_VALUE = {"mean": 1.0, "std": 2.0, "rhat": 1.01, "W": 3.0, "B": 0.5, "ess": 11.0}


@pytest.fixture()
def fake_getters(monkeypatch):
    """the thin getters replaced by host functions: sum of the chains' values + a code of the statistic, on the shard's pixels"""
    calls = []

    def base(engs):
        assert len({e.npix for e in engs}) == 1
        return sum(e.value for e in engs) + np.arange(engs[0].npix)

    def get(engs, l, what, stat, ddof=0, device=False, out=None):
        calls.append(("get", l, what, stat, ddof, len(engs)))
        return np.tile(base(engs) + STAT_VALUE[stat], (3, 1))

    def get_template(engs, l, stat, ddof=0, out=None):
        calls.append(("template", l, stat, ddof, len(engs)))
        return np.full((3, engs[0].nbands), STAT_VALUE[stat] + sum(e.value for e in engs))

    def get_signal(engs, s, stat, ddof=0, device=False, out=None):
        return base(engs) + STAT_VALUE[stat] + 100 * s

    def get_pair(engs, p, stat, ddof=0, device=False, out=None):
        return base(engs) + (0.25 if stat == "corr" else 7.0 + ddof)

    def hist_stat(engs, reg, stat, q=None, device=False, out=None):
        return np.stack([base(engs) + v for v in q]) if stat == "quantile" else base(engs) + (0.5 if stat == "mode" else 21.0)

    for name, fn in (("chains_get", get), ("chains_get_template", get_template), ("chains_get_signal", get_signal),
                     ("chains_get_pair", get_pair), ("chains_hist_stat", hist_stat)):
        monkeypatch.setattr(api, name, fn)
    return calls


def _chains(K=3, counts=None, lag1=True):
    """K chains of two shards (5 and 4 pixels; pixels 1, 4 and 5 of the sky masked)"""
    m0, m1 = np.ones((3, 5)), np.ones((3, 4))
    m0[0, [1, 4]] = 0.0
    m1[0, [0]] = 0.0
    counts = counts or [7] * K
    return [[_FakeEngine(m0, 10.0 * (k + 1), counts[k], lag1), _FakeEngine(m1, 10.0 * (k + 1), counts[k], lag1)] for k in range(K)]


MASKED = np.zeros(9, dtype=bool)
MASKED[[1, 4, 5]] = True
SKY = np.concatenate([np.arange(5), np.arange(4)]) + 60.0       # base() of three chains, the two shards side by side


def test_chains_posterior_maps_keys_shards_and_fill(fake_getters):
    chains = _chains()
    pm = api.chains_posterior_maps(chains, ddof=1)
    assert list(pm) == [("dust", "amplitude"), ("dust", "beta"), ("mono", "amplitude")]
    for key in (("dust", "amplitude"), ("dust", "beta")):
        assert set(pm[key]) == {"n", "nchains", "mean", "std", "rhat", "W", "B", "ess"}
        assert pm[key]["n"] == 7 and pm[key]["nchains"] == 3
        for stat, v in STAT_VALUE.items():
            assert pm[key][stat].shape == (3, 9) and np.array_equal(pm[key][stat][1], SKY + v)
    assert pm[("mono", "amplitude")]["rhat"].shape == (3, 2) and (pm[("mono", "amplitude")]["rhat"] == STAT_VALUE["rhat"] + 60.0).all()
    assert ("get", 0, 1, "std", 1, 3) in fake_getters and ("template", 1, "W", 1, 3) in fake_getters
    assert not any(c[0] == "get" and c[2] == 2 for c in fake_getters)            # index T is not selected
    unseen = -1.6375e30
    filled = api.chains_posterior_maps(chains, masked_value=unseen)
    for stat in STAT_VALUE:
        m = filled[("dust", "beta")][stat]
        assert (m[:, MASKED] == unseen).all() and np.array_equal(m[:, ~MASKED], pm[("dust", "beta")][stat][:, ~MASKED])
    assert (filled[("mono", "amplitude")]["mean"] == 61.0).all()                 # rows of a template are no pixels: never filled
    # a ddata stands for a one-shard chain
    whole = [da.DangData(sig_map=None, rms_map=None, masks=c[0].ddata.masks, engine=c[0]) for c in chains]
    assert np.array_equal(api.chains_posterior_maps(whole)[("dust", "beta")]["W"][0], np.arange(5) + 63.0)
    # no lag-1 in one chain: no pooled ESS; unequal counts: the pooled statistics only, n as a list
    assert "ess" not in api.chains_posterior_maps(_chains()[:2] + _chains(1, lag1=False))[("dust", "beta")]
    un = api.chains_posterior_maps(_chains(3, counts=[7, 9, 7]))[("dust", "beta")]
    assert set(un) == {"n", "nchains", "mean", "std", "ess"} and un["n"] == [7, 9, 7]
    assert set(api.chains_posterior_maps(_chains(2, counts=[1, 1]))[("dust", "beta")]) == {"n", "nchains", "mean", "std", "ess"}


def test_chains_maps_of_pairs_quantiles_and_signals(fake_getters):
    chains = _chains()
    unseen = -1.6375e30
    key = (("dust", "amplitude", 0), ("dust", "beta", 1))
    assert np.array_equal(api.chains_pair_maps(chains)[key], SKY + 0.25)
    cov = api.chains_pair_maps(chains, stat="cov", ddof=1, masked_value=unseen)[key]
    assert (cov[MASKED] == unseen).all() and np.array_equal(cov[~MASKED], SKY[~MASKED] + 8.0)
    qm = api.chains_quantile_maps(chains, q=(0.1, 0.9), masked_value=unseen)
    assert list(qm) == [("dust", "beta", 1)]
    e = qm[("dust", "beta", 1)]
    assert e["range"] == (1.0, 2.0) and e["nbins"] == 16 and e["q"].shape == (2, 9)
    assert (e["q"][:, MASKED] == unseen).all() and np.array_equal(e["q"][1, ~MASKED], SKY[~MASKED] + 0.9)
    assert np.array_equal(e["n"][~MASKED], SKY[~MASKED] + 21.0) and np.array_equal(e["mode"][~MASKED], SKY[~MASKED] + 0.5)
    sm = api.chains_signal_maps(chains, ddof=1)
    assert list(sm) == [("dust", "b1", "T"), ("dust", "b0", "P")]
    assert set(sm[("dust", "b0", "P")]) == {"n", "nchains", "mean", "std", "rhat", "W", "B"}
    assert np.array_equal(sm[("dust", "b0", "P")]["rhat"], SKY + STAT_VALUE["rhat"] + 100)


def test_chains_maps_refuse_what_does_not_fit(fake_getters):
    with pytest.raises(da.DangxError, match="2 to 8 chains"):
        api.chains_posterior_maps(_chains(1))
    with pytest.raises(da.DangxError, match="2 to 8 chains"):
        api.chains_pair_maps(_chains(9))
    bad = _chains()
    bad[1][1]._count = 6
    for fn in (api.chains_posterior_maps, api.chains_pair_maps, api.chains_quantile_maps, api.chains_signal_maps):
        with pytest.raises(da.DangxError, match="contexts of chain 1 hold different sample counts"):
            fn(bad)
    short = _chains()
    del short[2][1]
    with pytest.raises(da.DangxError, match="different numbers of shards"):
        api.chains_signal_maps(short)
    other = _chains()
    other[2][0]._moment_hist = dict(other[2][0]._moment_hist, nbins=8)
    with pytest.raises(da.DangxError, match="different histogram registrations"):
        api.chains_quantile_maps(other)
    other[1][1]._moment_signals = [(0, 1, 0)]
    with pytest.raises(da.DangxError, match="different signal registrations"):
        api.chains_signal_maps(other)
    none = _chains()
    del none[0][0]._moment_pairs
    with pytest.raises(da.DangxError, match="moments_pairs was not called"):
        api.chains_pair_maps(none)
