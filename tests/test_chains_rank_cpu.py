"""Rank-normalised and folded R-hat from the histograms of several chains, host side: the definitions of
dang_amd/csrc/dx_rank_host.h (what k_chains_rank, the host checks and this program share) in a stand-alone program under the
address and undefined-behaviour sanitizers against closed forms and against tests/rank_ref.py, and chains_rank_maps over fake
host engines.  No device needed; nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dang_amd as da
from dang_amd import api

import chains_ref as cr
import rank_ref as rr
import test_chains_cpu as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = cr.EPS

# "ppf n" + n hex floats: dx_norm_ppf of each.  "check K nbins bits stat": dx_rank_check's answer.
# "rank K nbins bits npix" + per pixel and chain the 32-bit words of its record: the three stats per pixel, as hex floats
HOST_MAIN = r"""
#include "dx_rank_host.h"
#include <cstdio>
#include <cstring>
#include <memory>
int main() {
    char mode[8] = {};
    if (std::scanf("%7s", mode) != 1) return 2;
    if (!std::strcmp(mode, "ppf")) {
        int n = 0;
        if (std::scanf("%d", &n) != 1) return 2;
        for (int i = 0; i < n; ++i) {
            double p = 0.0;
            if (std::scanf("%la", &p) != 1) return 2;
            std::printf("%a\n", dx_norm_ppf(p));
        }
        return 0;
    }
    int K = 0, nbins = 0, bits = 0, last = 0;
    if (std::scanf("%d %d %d %d", &K, &nbins, &bits, &last) != 4) return 2;
    if (!std::strcmp(mode, "check")) {
        std::printf("%s\n", dx_rank_check(K, nbins, bits, last).c_str());
        return 0;
    }
    if (!dx_rank_check(K, nbins, bits, 0).empty()) return 2;
    const int words = dx_hist_words(nbins, bits);
    for (int i = 0; i < last; ++i) {
        std::unique_ptr<uint32_t[]> rec[DX_CHAINS_MAX];     // exactly `words` long: a read past the end is an ASan report
        const uint32_t* ptr[DX_CHAINS_MAX] = {};
        for (int k = 0; k < K; ++k) {
            rec[k].reset(new uint32_t[(size_t)words]);
            for (int w = 0; w < words; ++w) if (std::scanf("%u", &rec[k][w]) != 1) return 2;
            ptr[k] = rec[k].get();
        }
        std::printf("%a %a %a\n", dx_rank_stat(ptr, K, nbins, bits, DX_RK_BULK), dx_rank_stat(ptr, K, nbins, bits, DX_RK_FOLDED),
                    dx_rank_stat(ptr, K, nbins, bits, DX_RK_MAX));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("rank_host")
    src, exe = tmp / "host_main.cpp", tmp / "host_main"
    src.write_text(HOST_MAIN)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "dang_amd", "csrc"), "-o", str(exe), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and ("cannot find" in r.stdout or "unsupported" in r.stdout):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stdout
    return str(exe)


def _exe(exe, text):
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


def _rank(exe, counts, bits):
    """counts [K][npix][nbins] -> {'bulk', 'folded', 'max'}: [npix] each"""
    counts = np.asarray(counts)
    K, npix, nbins = counts.shape
    words = rr.pack(counts, bits)
    assert np.array_equal(rr.unpack(words, nbins, bits), counts)
    lines = ["rank %d %d %d %d" % (K, nbins, bits, npix)]
    for i in range(npix):
        for k in range(K):
            lines.append(" ".join(str(int(w)) for w in words[k, i]))
    out = np.array([[float.fromhex(v) for v in ln.split()] for ln in _exe(exe, "\n".join(lines) + "\n")])
    assert out.shape == (npix, 3)
    return {"bulk": out[:, 0], "folded": out[:, 1], "max": out[:, 2]}


def _against_ref(exe, counts, bits, what, min_finite=None, weighted=False):
    got = _rank(exe, counts, bits)
    return got, {st: rr.compare(got[st], counts, st, "%s %s" % (what, st), min_finite, weighted) for st in ("bulk", "folded", "max")}


def test_closed_forms(host_exe):
    """(a) identical records: R-hat^2 = (n - 1)/n.  (b) K = 2, bins a < b, chain 0 holds n - 1 samples in a and 1 in b, chain 1
    the mirror image: the scores are +-z, so R-hat^2 = (n - 1)/n + (n - 2)^2 / (2n) whatever z is, for the fold as well (the
    median bin is a).  (c) every chain in one bin: +inf when the bins differ, NaN when they do not."""
    rng = np.random.default_rng(3)
    for nbins, bits in ((8, 16), (64, 16), (32, 32)):
        for K in (2, 3, 8):
            rec = rng.integers(0, 40, (1, 6, nbins))
            rec[0, :, 0] += 2                                          # n >= 2 everywhere
            got = _rank(host_exe, np.repeat(rec, K, axis=0), bits)
            n = rec[0].sum(axis=1)
            for st in got:
                assert (np.abs(got[st] ** 2 - (n - 1) / n) <= 64 * EPS * (n - 1) / n).all(), ("identical records", K, nbins, bits, st)
        for n, r2 in ((2, 0.5), (8, 3.125), (64, 31.015625)):
            assert r2 == (n - 1) / n + (n - 2) ** 2 / (2 * n)
            c = np.zeros((2, 3, nbins), dtype=np.int64)
            for i, (a, b) in enumerate(((0, 1), (2, nbins - 1), (nbins - 2, nbins - 1))):
                c[0, i, a], c[0, i, b], c[1, i, a], c[1, i, b] = n - 1, 1, 1, n - 1
            got = _rank(host_exe, c, bits)
            for st in got:
                assert (np.abs(got[st] ** 2 - r2) <= 64 * EPS * r2).all(), ("two bins", n, nbins, bits, st, got[st])
        c = np.zeros((3, 3, nbins), dtype=np.int64)
        c[0, 0, 1], c[1, 0, 3], c[2, 0, 5] = 9, 9, 9                   # bins 1, 3, 5
        c[0, 1, 2], c[1, 1, 2], c[2, 1, nbins - 1] = 9, 9, 9            # two chains together, one apart
        c[:, 2, 4] = 9                                                  # all in bin 4
        got = _rank(host_exe, c, bits)
        for st in got:
            assert got[st][0] == np.inf and got[st][1] == np.inf and np.isnan(got[st][2]), (nbins, bits, st, got[st])
    # the reference takes the same closed forms
    c = np.zeros((2, 1, 8), dtype=np.int64)
    c[0, 0, 2], c[0, 0, 5], c[1, 0, 2], c[1, 0, 5] = 7, 1, 1, 7
    for st in ("bulk", "folded", "max"):
        ref, tol = rr.rhat2(c, st)
        assert abs(ref[0] - 3.125) <= tol[0] and tol[0] < 1e-9


def test_norm_ppf_within_its_stated_bound(host_exe):
    p = rr.ppf_points(400)
    assert p[0] == rr.PPF_PMIN and p[-1] == 0.5 and 1.7e-11 < p[0] < 1.9e-11
    got = np.array([float.fromhex(v) for v in _exe(host_exe, "ppf %d\n%s\n" % (p.size, "\n".join(float(v).hex() for v in p)))])
    assert got[-1] == 0.0
    ref = rr.ppf_ref(p)
    assert 6.6 < ref[0] < 6.8 and ref[-1] == 0
    err = np.abs(got.astype(rr.LD) - ref)
    print("dx_norm_ppf (host): worst |error| %.3g of the stated %.3g" % (float(err.max()), rr.PPF_BOUND))
    assert (got >= 0).all() and (err <= rr.PPF_BOUND).all()


def _random_counts(rng, K, npix, nbins, n_max, top=None):
    """chains around different bins with different spreads; equal totals per pixel, except in pixel 1 (one chain lacks a sample)"""
    counts = np.zeros((K, npix, nbins), dtype=np.int64)
    for i in range(npix):
        n = int(rng.integers(2, n_max + 1))
        for k in range(K):
            centre, width = rng.uniform(0, nbins), rng.uniform(0.3, nbins / 2)
            b = np.clip(np.rint(rng.normal(centre, width, n)), 0, nbins - 1).astype(int)
            counts[k, i] = np.bincount(b, minlength=nbins)
    if top is not None:
        assert counts.max() <= top
    if npix > 1:
        k = K - 1
        counts[k, 1, np.argmax(counts[k, 1])] -= 1
    return counts


@pytest.mark.parametrize("nbins,bits", [(8, 16), (8, 32), (64, 16), (32, 32)])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_random_records_against_the_reference(host_exe, K, nbins, bits):
    rng = np.random.default_rng(100 * K + nbins + bits)
    counts = _random_counts(rng, K, 24, nbins, 300, top=2 ** bits - 1)
    got, ref = _against_ref(host_exe, counts, bits, "K %d nbins %d bits %d" % (K, nbins, bits), min_finite=0.9)
    assert all(np.isnan(got[st][1]) for st in got)                      # the pixel where one chain holds a sample less
    assert (ref["bulk"][np.isfinite(ref["bulk"])] > 1.0).any()
    # the weighted evaluation of the reference is its expansion (what the largest records below rely on)
    for st in ("bulk", "folded"):
        (re, te), (rw, tw) = rr.rhat2(counts, st), rr.rhat2(counts, st, weighted=True)
        ok = np.isfinite(re)
        assert np.array_equal(np.isnan(re), np.isnan(rw)) and np.array_equal(np.isinf(re), np.isinf(rw))
        assert (np.abs(re[ok] - rw[ok]) <= 1e-15 * re[ok]).all() and (np.abs(te[ok] - tw[ok]) <= 1e-9 * te[ok]).all()
    # every record reflected (bin b -> nbins - 1 - b): the scores change sign, the statistic does not
    refl = _rank(host_exe, counts[:, :, ::-1], bits)
    r, t = rr.rhat2(counts, "bulk")
    cr.compare(refl["bulk"].astype(rr.LD) ** 2, r, t, "reflected K %d nbins %d bits %d" % (K, nbins, bits), 0.9)


def test_a_chain_with_fewer_counted_samples_gives_nan(host_exe):
    c = np.zeros((3, 4, 8), dtype=np.int64)
    c[:, :, 2], c[:, :, 3], c[:, :, 6] = 4, 3, 1
    c[1, 1, 3] -= 1                                                     # chain 1 lost a sample
    c[2, 2, 6] += 1                                                     # chain 2 holds one more
    c[:, 3, :] = 0
    c[:, 3, 4] = 1                                                      # n = 1
    got = _rank(host_exe, c, 16)
    for st in got:
        assert np.isfinite(got[st][0]) and np.isnan(got[st][1:]).all(), (st, got[st])
    none = _rank(host_exe, np.zeros((2, 1, 8), dtype=np.int64), 32)     # S = 0
    assert all(np.isnan(v[0]) for v in none.values())


@pytest.mark.parametrize("nbins,bits", [(8, 16), (64, 16), (32, 32)])
def test_the_median_bin_at_either_end(host_exe, nbins, bits):
    """more than half of the pooled samples in bin 0 (in bin nbins - 1): the fold reaches nbins - 1 with one of its two terms
    outside the record at every distance"""
    rng = np.random.default_rng(nbins + bits)
    K, npix = 3, 6
    counts = np.zeros((K, npix, nbins), dtype=np.int64)
    for i in range(npix):
        for k in range(K):
            rest = np.bincount(rng.integers(1, nbins, 20 + 3 * k), minlength=nbins)
            counts[k, i] = rest
            counts[k, i, 0] = 40 - 3 * k                                # n = 60 in every chain; bin 0 holds 111 of 180
        counts[K - 1, i, nbins - 1] += 1
        counts[K - 1, i, 0] -= 1                                        # the far end is occupied
    assert (rr.median_bin(counts.sum(axis=0)) == 0).all() and (counts.sum(axis=0)[:, nbins - 1] > 0).all()
    _against_ref(host_exe, counts, bits, "median in bin 0, nbins %d" % nbins, min_finite=1.0)
    back = counts[:, :, ::-1]
    assert (rr.median_bin(back.sum(axis=0)) == nbins - 1).all()
    _against_ref(host_exe, back, bits, "median in the last bin, nbins %d" % nbins, min_finite=1.0)


def test_counters_at_their_limits(host_exe):
    """16-bit counters at 65 535, and 32-bit records of 2^32 - 1 samples per chain: S = 8 (2^32 - 1), the smallest p of
    dx_norm_ppf's domain in bin 0"""
    c = np.zeros((3, 2, 8), dtype=np.int64)
    c[0, :, 1], c[1, :, 2], c[2, :, 6] = 65535, 65535, 65535
    c[0, :, 5], c[1, :, 5], c[2, :, 0] = 3, 3, 3
    c[:, 1, 7] = 65535
    _against_ref(host_exe, c, 16, "16-bit counters at 65535", min_finite=1.0)
    top = 2 ** 32 - 1
    rng = np.random.default_rng(8)
    big = np.zeros((8, 3, 32), dtype=np.int64)
    for i in range(3):
        for k in range(8):
            w = rng.dirichlet(np.full(31, 0.5))
            part = np.floor(w * (top - 1000)).astype(np.int64)
            big[k, i, 1:] = part
            big[k, i, 1 + (k + i) % 31] += top - part.sum()
    big[0, :, 0] = 1                                                    # one sample of 8 (2^32 - 1) alone in the lowest bin
    big[0, :, 16] -= 1
    big[:, 2, :] = big[0, 2, :]                                         # identical records: (n - 1) / n
    assert (big.sum(axis=2) == top).all() and big.min() >= 0 and big.max() <= top
    got, ref = _against_ref(host_exe, big, 32, "S = 8 (2^32 - 1)", min_finite=1.0, weighted=True)
    f = (top - 1) / top
    assert all(abs(got[st][2] ** 2 - f) <= 64 * EPS * f for st in got)
    # the two-bin records of closed form (b) at the counter limit.  Not to 64 eps: a bin that holds nearly all of a chain's
    # samples leaves z - mean = d (1 - c / n) after a cancellation, which is what the n in the reference's tolerance pays for
    c2 = np.zeros((2, 1, 8), dtype=np.int64)
    c2[0, 0, 0], c2[0, 0, 7], c2[1, 0, 0], c2[1, 0, 7] = top - 1, 1, 1, top - 1
    r2 = (top - 1) / top + (top - 2) ** 2 / (2 * top)
    _, ref = _against_ref(host_exe, c2, 32, "two bins, n = 2^32 - 1", min_finite=1.0, weighted=True)
    assert all(abs(float(v[0]) - r2) <= 1e-12 * r2 for v in ref.values())


def test_argument_checks_name_the_cause(host_exe):
    def why(K, nbins, bits, stat):
        out = _exe(host_exe, "check %d %d %d %d\n" % (K, nbins, bits, stat))
        return out[0] if out else ""
    assert why(2, 64, 16, 0) == "" and why(8, 32, 32, 2) == ""
    assert "stat" in why(4, 64, 16, 3) and "stat" in why(4, 64, 16, -1)
    assert "2 to 8 chains" in why(1, 64, 16, 0) and "2 to 8 chains" in why(9, 64, 16, 0)
    assert "nbins" in why(2, 12, 16, 0) and "bits" in why(2, 8, 8, 0) and "128 bytes" in why(2, 64, 32, 0)


# ---- chains_rank_maps over fake host engines

@pytest.fixture()
def fake_rank(monkeypatch):
    calls = []
    code = {"bulk": 0.25, "folded": 0.5, "max": 0.75}

    def hist_rank(engs, reg, stat, device=False, out=None):
        calls.append((reg, stat, len(engs)))
        assert len({e.npix for e in engs}) == 1
        return sum(e.value for e in engs) + np.arange(engs[0].npix) + code[stat] + 100 * reg

    monkeypatch.setattr(api, "chains_hist_rank", hist_rank)
    return calls


def test_chains_rank_maps_keys_shards_and_fill(fake_rank):
    assert da.chains_rank_maps is api.chains_rank_maps and da.chains_hist_rank is not None
    chains = tc._chains()
    for c in chains:
        for e in c:
            e._moment_hist = {"planes": [(0, 1, 1), (0, 0, 0)], "ranges": [(1.0, 2.0), (-5.0, 5.0)], "nbins": 16, "bits": 16}
    rm = api.chains_rank_maps(chains)
    assert list(rm) == [("dust", "beta", 1), ("dust", "amplitude", 0)]
    for r, key in enumerate(rm):
        e = rm[key]
        assert set(e) == {"rhat_rank", "rhat_folded", "rhat_max", "range", "nbins"} and e["nbins"] == 16
        assert e["range"] == ((1.0, 2.0), (-5.0, 5.0))[r]
        for name, v in (("rhat_rank", 0.25), ("rhat_folded", 0.5), ("rhat_max", 0.75)):
            assert e[name].shape == (9,) and np.array_equal(e[name], tc.SKY + v + 100 * r)     # the two shards side by side
    assert sorted(set(fake_rank)) == sorted((r, st, 3) for r in (0, 1) for st in ("bulk", "folded", "max"))
    unseen = -1.6375e30
    filled = api.chains_rank_maps(chains, masked_value=unseen)
    for key in rm:
        for name in ("rhat_rank", "rhat_folded", "rhat_max"):
            m = filled[key][name]
            assert (m[tc.MASKED] == unseen).all() and np.array_equal(m[~tc.MASKED], rm[key][name][~tc.MASKED])
    # unequal sample counts between the chains are no refusal: the rule per pixel decides
    assert list(api.chains_rank_maps(tc._chains(3, counts=[7, 9, 7]))) == [("dust", "beta", 1)]
    assert da._lib.RANK_STAT_CODES == {"bulk": 0, "folded": 1, "max": 2}


def test_chains_rank_maps_refuse_what_does_not_fit(fake_rank):
    with pytest.raises(da.DangxError, match="2 to 8 chains"):
        api.chains_rank_maps(tc._chains(1))
    with pytest.raises(da.DangxError, match="2 to 8 chains"):
        api.chains_rank_maps(tc._chains(9))
    other = tc._chains()
    other[2][0]._moment_hist = dict(other[2][0]._moment_hist, nbins=8)
    with pytest.raises(da.DangxError, match="different histogram registrations"):
        api.chains_rank_maps(other)
    none = tc._chains()
    for c in none:
        for e in c:
            del e._moment_hist
    with pytest.raises(da.DangxError, match="moments_hist was not called"):
        api.chains_rank_maps(none)
    short = tc._chains()
    del short[2][1]
    with pytest.raises(da.DangxError, match="different numbers of shards"):
        api.chains_rank_maps(short)
    bad = tc._chains()
    bad[1][1]._count = 6
    with pytest.raises(da.DangxError, match="contexts of chain 1 hold different sample counts"):
        api.chains_rank_maps(bad)
    assert not fake_rank
