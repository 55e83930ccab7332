"""Batched posterior accumulators, host side: dang_amd/csrc/dx_batches_host.h (what the kernels and this program share) replayed
in a stand-alone program under the address and undefined-behaviour sanitizers -- accumulate, merge in place, every read-out --
against numpy.longdouble (tests/batches_ref.py), closed forms on exact inputs, and the map-assembling functions
(posterior_batch_maps, chains_batch_maps) over fake host engines.  No device needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import api

import batches_ref as br
import chains_ref as cr
import test_chains_cpu as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# reads: K nbatch L0 n first ddof, then per chain its n samples as hex floats; accumulates every chain as the library does
# (Welford with fma into slot c / L, dx_batches_merge in place when every slot is full) and prints the state and every read-out of
# dx_batches_host.h as hex floats, or why it is refused
HOST_MAIN = r"""
#include "dx_batches_host.h"
#include <cstdio>
#include <vector>
int main() {
    int K = 0, nbatch = 0, first = 0, ddof = 0;
    long long L0 = 0, n = 0;
    if (std::scanf("%d %d %lld %lld %d %d", &K, &nbatch, &L0, &n, &first, &ddof) != 6 || K < 1 || K > DX_CHAINS_MAX || n < 1) return 2;
    const int32_t plane[3] = {0, 0, 0}, sel[1] = {1};
    const int nind[1] = {0}, global[1] = {0};
    // a table of two components whose second is a global-amplitude member with its row selected: refused as what it is
    const int32_t row[3] = {1, 0, 0}, sel2[2] = {1, 1};
    const int nind2[2] = {0, 0}, global2[2] = {0, 1};
    std::printf("global_row %s\n", dx_batches_check(1, row, 2, 1, 2, 1, sel2, nind2, global2).c_str());
    const std::string reg = dx_batches_check(1, plane, nbatch, L0, 1, 1, sel, nind, global);
    if (!reg.empty()) { std::printf("refused %s\n", reg.c_str()); return 0; }
    std::vector<std::vector<double>> mean((size_t)K), m2((size_t)K);
    long long L = L0;
    for (int k = 0; k < K; ++k) {
        mean[k].assign((size_t)nbatch, 0.0); m2[k].assign((size_t)nbatch, 0.0);   // exactly nbatch slots: a slot past the end is an ASan report
        std::vector<double> x((size_t)n);
        for (long long t = 0; t < n; ++t) if (std::scanf("%la", &x[(size_t)t]) != 1) return 2;
        L = L0;
        for (long long c = 0; c < n; ++c) {
            if (c / L == nbatch) {
                for (int i = 0; i < nbatch / 2; ++i) {   // ascending, in place: destination i <= 2 i
                    double mu = mean[k][2 * i], M = m2[k][2 * i];
                    dx_batches_merge(mean[k][2 * i + 1], m2[k][2 * i + 1], 0.5 * (double)L, mu, M);
                    mean[k][i] = mu; m2[k][i] = M;
                }
                for (int i = nbatch / 2; i < nbatch; ++i) mean[k][i] = m2[k][i] = 0.0;
                L *= 2;
            }
            const size_t b = (size_t)(c / L);
            const double inv = 1.0 / (double)(c % L + 1), d = x[(size_t)c] - mean[k][b];
            mean[k][b] = std::fma(d, inv, mean[k][b]);
            m2[k][b] = std::fma(d, x[(size_t)c] - mean[k][b], m2[k][b]);
        }
    }
    const DxBatchPos pos = dx_batches_pos(n, L);
    std::printf("L %lld\nnfull %d\npartial %lld\n", pos.L, pos.nfull, pos.partial);
    for (int b = 0; b < nbatch; ++b) std::printf("slot%d %a %a\n", b, mean[0][b], m2[0][b]);
    static const char* const names[5] = {"mean", "std", "mcse", "ess_bm", "split_rhat"};
    for (int stat = 0; stat < 5; ++stat) {
        std::string why = dx_batches_stat_check(stat, first, K == 1 ? ddof : 0, pos.L, pos.nfull, pos.partial);
        if (why.empty() && K > 1 && stat == DX_BT_STD && (ddof < 0 || (long long)K * ((pos.nfull - first) * pos.L + pos.partial) - ddof <= 0)) why = "ddof";
        if (!why.empty()) { std::printf("why_%s %s\n", names[stat], why.c_str()); continue; }
        const DxBatchPar par = dx_batches_par(stat, first, ddof, pos.L, pos.nfull, pos.partial, K);
        double r[1];
        if (K == 1)
            dx_batches_stat<1>(par, [&](int b, bool want, double (&m)[1], double (&q)[1]) { m[0] = mean[0][(size_t)b]; q[0] = want ? m2[0][(size_t)b] : 0.0; }, r);
        else
            dx_chains_batches_stat<1>(par, [&](int k, int b, bool want, double (&m)[1], double (&q)[1]) {
                m[0] = mean[(size_t)k][(size_t)b]; q[0] = want ? m2[(size_t)k][(size_t)b] : 0.0; }, r);
        std::printf("%s %a\n", names[stat], r[0]);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("batches_host")
    src, exe = tmp / "host_main.cpp", tmp / "host_main"
    src.write_text(HOST_MAIN)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "dang_amd", "csrc"), "-o", str(exe), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and ("cannot find" in r.stdout or "unsupported" in r.stdout):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stdout
    return str(exe)


def _run(exe, xs, nbatch, L0, first=0, ddof=0):
    lines = ["%d %d %d %d %d %d" % (len(xs), nbatch, L0, len(xs[0]), first, ddof)]
    for x in xs:
        lines += [float(v).hex() for v in x]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = {}
    for ln in r.stdout.splitlines():
        key, val = ln.split(" ", 1)
        if key.startswith("why_") or key in ("refused", "global_row"):
            out[key] = val
        elif key.startswith("slot"):
            out[key] = tuple(float.fromhex(v) for v in val.split())
        elif key in ("L", "nfull", "partial"):
            out[key] = int(val)
        else:
            out[key] = float.fromhex(val)
    return out


CASES = [(37, 4, 1), (64, 2, 2), (96, 32, 1), (33, 2, 1), (12, 4, 3), (7, 8, 1), (100, 6, 1)]


def _firsts(nfull):
    return sorted({f for f in (0, 1, nfull - 2, nfull) if 0 <= f <= nfull})


@pytest.mark.parametrize("offset", tc.OFFSETS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_nb%d_L%d" % c)
def test_replay_under_sanitizers_against_long_double(host_exe, case, offset):
    n, nbatch, L0 = case
    rng = np.random.default_rng(1000 * n + nbatch)
    x = tc._ar1(rng, n, offset)
    L, nfull, partial = br.replay(n, nbatch, L0)
    for first in _firsts(nfull):
        for ddof in (0, 1):
            got = _run(host_exe, [x], nbatch, L0, first, ddof)
            assert (got["L"], got["nfull"], got["partial"]) == (L, nfull, partial)
            done = br.check(lambda stat: np.array([got[stat]]), x[:, None], L, nfull, partial, first, ddof, "%s off %g" % (case, offset))
            for stat in br.STATS:                                        # refused exactly where the definition needs more
                assert (stat in done) == (stat in got) and (stat in done) != ("why_" + stat in got), (stat, got)
    # the slots themselves: what a long-double run of the scheme holds
    got = _run(host_exe, [x], nbatch, L0)
    _, slots = br.host_batches(x, nbatch, L0)
    for b, s in enumerate(slots):
        mean, m2 = got["slot%d" % b]
        if s is None:
            assert mean == 0.0 and m2 == 0.0
        else:
            pm = cr.pooled([s[:, None]], 0)
            cr.compare(np.array([mean]), *pm["mean"], "slot %d mean %s" % (b, case))
            cr.compare(np.array([np.sqrt(m2 / len(s))]), *pm["std"], "slot %d std %s" % (b, case))


@pytest.mark.parametrize("K", [2, 4, 8])
def test_several_chains_under_sanitizers(host_exe, K):
    n, nbatch, L0 = 48, 4, 1
    rng = np.random.default_rng(77 + K)
    xs = [tc._ar1(rng, n, -3.1 + 0.7 * k) for k in range(K)]
    L, nfull, partial = br.replay(n, nbatch, L0)
    assert (L, nfull, partial) == (16, 3, 0)
    for first in (0, 1):
        got = _run(host_exe, xs, nbatch, L0, first, 1)
        done = br.check(lambda stat: np.array([got[stat]]), None, L, nfull, partial, first, 1, "K %d" % K, chains=[x[:, None] for x in xs])
        assert done == list(br.STATS)


def test_closed_forms_with_exact_inputs(host_exe):
    """x_t = t s with s a power of two and L a power of two: batch b's mean is (b L + (L - 1) / 2) s, an arithmetic progression of
    step L s, so over B' batches  MCSE^2 = (L s)^2 (B' + 1) / 12;  a half of n = h L consecutive samples has M = s^2 n (n^2 - 1) /
    12, so W = s^2 n (n + 1) / 12, the half-means differ by n s, B/n = n^2 s^2 / 2 and  split R-hat^2 = (n - 1) / n + 6 n / (n + 1)."""
    for s in (0.25, 1.0, 8.0):
        for n, nbatch, L0, first in ((64, 8, 2, 0), (64, 8, 2, 3), (96, 32, 1, 0), (32, 4, 8, 0), (40, 8, 1, 1)):
            x = np.arange(n) * s
            got = _run(host_exe, [x], nbatch, L0, first)
            L, nfull, partial = br.replay(n, nbatch, L0)
            assert L & (L - 1) == 0 and (got["L"], got["nfull"], got["partial"]) == (L, nfull, partial)
            for b in range(nfull):
                assert got["slot%d" % b][0] == (b * L + (L - 1) / 2) * s
            Bp = nfull - first
            m2 = (L * s) ** 2 * (Bp + 1) / 12
            assert abs(got["mcse"] ** 2 - m2) <= 64 * cr.EPS * m2
            nh = (Bp // 2) * L
            r2 = (nh - 1) / nh + 6 * nh / (nh + 1)
            assert abs(got["split_rhat"] ** 2 - r2) <= 64 * cr.EPS * r2
            mean = (first * L + n - 1) / 2 * s
            assert abs(got["mean"] - mean) <= 64 * cr.EPS * mean
    flat = _run(host_exe, [np.full(16, 2.5)], 4, 2)
    assert flat["mean"] == 2.5 and flat["std"] == 0 and flat["mcse"] == 0 and np.isnan(flat["ess_bm"]) and np.isnan(flat["split_rhat"])
    apart = _run(host_exe, [np.repeat([1.0, 2.0], 8)], 4, 2)                      # halves that differ in their means alone
    assert apart["split_rhat"] == np.inf and apart["mean"] == 1.5
    odd = _run(host_exe, [np.arange(8.0)], 3, 1)
    assert "nbatch must be even" in odd["refused"]
    assert odd["global_row"] == "registration 0: a template / monopole / hi_fit amplitude is not a pixel plane"


# ---- the map-assembling functions over fake host engines

STAT_VALUE = {"mean": 1.0, "std": 2.0, "mcse": 0.125, "ess_bm": 11.0, "split_rhat": 1.01}


def _with_batches(chains, info, planes=((0, 1, 1), (0, 1, 2))):
    for chain in chains:
        for e in chain:
            e._moment_batches = {"planes": list(planes), "nbatch": 4, "batch_len": 1}
            e.moments_batches_info = lambda info=info: dict(info)
            e.moments_batches_get = (lambda e: lambda r, stat, first=0, ddof=0: e.value + np.arange(e.npix) + STAT_VALUE[stat] + 100 * r + first)(e)
    return chains


INFO = {"batch_len": 2, "nfull": 3, "partial": 1}


def test_posterior_batch_maps_keys_shards_and_fill():
    chain = _with_batches(tc._chains(1), INFO)[0]
    ddata = da.DangData(sig_map=None, rms_map=None, masks=chain[0].ddata.masks)
    pm = api.posterior_batch_maps(ddata, first=1, ddof=1, engines=chain)
    assert list(pm) == [("dust", "beta", 1), ("dust", "beta", 2)]
    e = pm[("dust", "beta", 2)]
    assert set(e) == {"n", "first", "batch_len", "nfull", "partial", "mean", "std", "mcse", "ess_bm", "split_rhat"}
    assert (e["n"], e["first"], e["batch_len"], e["nfull"], e["partial"]) == (7, 1, 2, 3, 1)
    for stat, v in STAT_VALUE.items():
        assert e[stat].shape == (9,) and np.array_equal(e[stat], tc.SKY - 50.0 + v + 100 + 1)
    unseen = -1.6375e30
    filled = api.posterior_batch_maps(ddata, masked_value=unseen, engines=chain)[("dust", "beta", 1)]
    assert (filled["mcse"][tc.MASKED] == unseen).all() and np.array_equal(filled["mcse"][~tc.MASKED], (tc.SKY - 50.0 + 0.125)[~tc.MASKED])
    # too few full batches after `first`: the statistics that need two are left out, not invented
    assert set(api.posterior_batch_maps(ddata, first=2, engines=chain)[("dust", "beta", 1)]) & set(STAT_VALUE) == {"mean", "std"}
    short = _with_batches(tc._chains(1), {"batch_len": 1, "nfull": 3, "partial": 0})[0]
    assert "split_rhat" not in api.posterior_batch_maps(ddata, engines=short)[("dust", "beta", 1)]
    with pytest.raises(da.DangxError, match="first must be 0 .. 3"):
        api.posterior_batch_maps(ddata, first=4, engines=chain)
    assert set(api.posterior_batch_maps(ddata, first=3, engines=chain)[("dust", "beta", 1)]) & set(STAT_VALUE) == {"mean", "std"}   # the open batch alone
    full = _with_batches(tc._chains(1), {"batch_len": 2, "nfull": 3, "partial": 0})[0]
    with pytest.raises(da.DangxError, match="first = 3 discards every sample held"):
        api.posterior_batch_maps(ddata, first=3, engines=full)
    chain[1]._count = 6
    with pytest.raises(da.DangxError, match="different sample counts"):
        api.posterior_batch_maps(ddata, engines=chain)
    chain[1]._count = 7
    chain[1]._moment_batches = dict(chain[1]._moment_batches, nbatch=8)
    with pytest.raises(da.DangxError, match="different batch registrations"):
        api.posterior_batch_maps(ddata, engines=chain)
    with pytest.raises(da.DangxError, match="moments_batches was not called"):
        api.posterior_batch_maps(ddata, engines=tc._chains(1)[0])


def test_chains_batch_maps_keys_shards_and_refusals(monkeypatch):
    calls = []

    def get(engs, reg, stat, first=0, ddof=0, device=False, out=None):
        calls.append((reg, stat, first, ddof, len(engs)))
        return sum(e.value for e in engs) + np.arange(engs[0].npix) + STAT_VALUE[stat] + 100 * reg

    monkeypatch.setattr(api, "chains_batches_get", get)
    chains = _with_batches(tc._chains(), INFO)
    pm = api.chains_batch_maps(chains, first=1, ddof=1)
    assert list(pm) == [("dust", "beta", 1), ("dust", "beta", 2)]
    e = pm[("dust", "beta", 2)]
    assert set(e) == {"n", "nchains", "first", "batch_len", "nfull", "partial", "mean", "std", "mcse", "ess_bm", "split_rhat"}
    assert e["n"] == 7 and e["nchains"] == 3 and e["first"] == 1
    assert np.array_equal(e["split_rhat"], tc.SKY + 1.01 + 100) and (1, "std", 1, 1, 3) in calls
    unseen = -1.6375e30
    filled = api.chains_batch_maps(chains, masked_value=unseen)[("dust", "beta", 1)]["ess_bm"]
    assert (filled[tc.MASKED] == unseen).all() and np.array_equal(filled[~tc.MASKED], (tc.SKY + 11.0)[~tc.MASKED])
    whole = [da.DangData(sig_map=None, rms_map=None, masks=c[0].ddata.masks, engine=c[0]) for c in chains]   # a ddata: a one-shard chain
    assert np.array_equal(api.chains_batch_maps(whole)[("dust", "beta", 1)]["mean"], np.arange(5) + 61.0)
    with pytest.raises(da.DangxError, match="2 to 8 chains"):
        api.chains_batch_maps(_with_batches(tc._chains(1), INFO))
    with pytest.raises(da.DangxError, match="chains hold different sample counts"):
        api.chains_batch_maps(_with_batches(tc._chains(3, counts=[7, 9, 7]), INFO))
    other = _with_batches(tc._chains(), INFO)
    other[2][0]._moment_batches = dict(other[2][0]._moment_batches, batch_len=2)
    with pytest.raises(da.DangxError, match="different batch registrations"):
        api.chains_batch_maps(other)
    with pytest.raises(da.DangxError, match="moments_batches was not called"):
        api.chains_batch_maps(tc._chains())
    with pytest.raises(da.DangxError, match="first must be 0 .. 3"):
        api.chains_batch_maps(chains, first=5)
    with pytest.raises(da.DangxError, match="first = 3 discards every sample held"):
        api.chains_batch_maps(_with_batches(tc._chains(), {"batch_len": 2, "nfull": 3, "partial": 0}), first=3)
