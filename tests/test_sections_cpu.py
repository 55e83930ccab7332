"""Sections of the accumulator state, host side: the fingerprint, the HEAD record and the byte counts of
dang_amd/csrc/dx_section_host.h in a stand-alone program under the address and undefined-behaviour sanitizers; the plumbing of
dist_chains over fake engines on two gloo ranks; the file format of moments_save / moments_load over a fake engine.
No device needed; nothing is loaded into Python under a sanitizer."""
import os
import shutil
import socket
import struct
import subprocess

import numpy as np
import pytest
import torch.distributed as td
import torch.multiprocessing as mp

import dang_amd as da
from dang_amd import _lib as L
from dang_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# variant v of one base registration: 0 = the base, 1.. = ONE difference each (VARIANTS below names them)
HOST_MAIN = r"""
#include "dx_section_host.h"
#include <cstdio>
#include <cstring>
#include <memory>
static DxSecReg reg(int v) {
    DxSecReg r;
    r.npix = v == 1 ? 96 : 95; r.pix0 = v == 2 ? 2 : 1; r.nmaps = v == 3 ? 1 : 3;
    r.sel = {v == 4 ? 0x3f : 0x1ff, 0, 7}; r.type = {v == 5 ? 1 : 2, v == 17 ? 4 : 3, 8}; r.nind = {v == 6 ? 1 : 2, 1, 0};
    r.lag1 = v == 8 ? 0 : 1;
    r.pairs = {0, 0, 0, 0, 1, v == 7 ? 2 : 1};
    r.hist_planes = {0, 1, v == 9 ? 0 : 1, 0, 0, 0};
    r.hist_range = {v == 10 ? 1.25 : 1.0, v == 11 ? 2.5 : 2.0, -5.0, 5.0};
    r.nbins = v == 12 ? 8 : 16; r.bits = v == 13 ? 32 : 16;
    r.signals = {0, 1, v == 14 ? 1 : 0, 0, 0, 3};
    r.batch_planes = {0, 0, v == 15 ? 1 : 0};
    r.nbatch = v == 16 ? 6 : 4;
    return r;
}
static void show(const DxSecHead& h) {
    std::printf("%u %lld %d %d %lld %d %lld %llx", h.version, (long long)h.count, h.lag1, h.nbatch, (long long)h.batch_len, h.nfull,
                (long long)h.partial, (unsigned long long)h.fingerprint);
    for (int i = 0; i < DX_SEC_GROUPS; ++i) std::printf(" %llx", (unsigned long long)h.group[i]);
    std::printf("\n");
}
int main() {
    char mode[8] = {};
    int v = 0;
    if (std::scanf("%7s %d", mode, &v) != 2) return 2;
    if (!std::strcmp(mode, "fp")) {
        const DxSecReg a = reg(v), b = reg(v);   // two objects built alike
        std::printf("%d\n", dx_section_fingerprint(a) == dx_section_fingerprint(b) ? 1 : 0);
        show(dx_section_head(a, 11, 4));
        return 0;
    }
    if (!std::strcmp(mode, "diff")) {
        std::printf("%s\n", dx_section_head_diff(dx_section_head(reg(v), 11, 4), dx_section_head(reg(0), 11, 4)).c_str());
        return 0;
    }
    if (!std::strcmp(mode, "head")) {
        // the buffers are exactly as long as what is passed: a read past the end is an ASan report
        const DxSecHead h = dx_section_head(reg(0), 11, 4);
        std::unique_ptr<unsigned char[]> buf(new unsigned char[DX_SEC_HEAD_BYTES]);
        dx_section_head_pack(h, buf.get());
        for (int i = 0; i < DX_SEC_HEAD_BYTES; ++i) std::printf("%02x", buf[i]);
        std::printf("\n");
        DxSecHead g;
        std::printf("[%s]\n", dx_section_head_unpack(buf.get(), DX_SEC_HEAD_BYTES, g).c_str());
        show(g);
        std::unique_ptr<unsigned char[]> cut(new unsigned char[DX_SEC_HEAD_BYTES - 1]);
        std::memcpy(cut.get(), buf.get(), DX_SEC_HEAD_BYTES - 1);
        std::printf("[%s]\n", dx_section_head_unpack(cut.get(), DX_SEC_HEAD_BYTES - 1, g).c_str());
        std::printf("[%s]\n", dx_section_head_unpack(nullptr, 0, g).c_str());
        auto with = [&](int at, unsigned char x) {
            std::unique_ptr<unsigned char[]> c(new unsigned char[DX_SEC_HEAD_BYTES]);
            std::memcpy(c.get(), buf.get(), DX_SEC_HEAD_BYTES);
            c[at] ^= x;
            std::printf("[%s]\n", dx_section_head_unpack(c.get(), DX_SEC_HEAD_BYTES, g).c_str());
        };
        with(0, 0xff);    // the magic word
        with(4, 0x03);    // the layout version
        with(60, 0x01);   // a group value: the fingerprint no longer fits
        with(8, 0x01);    // count 11 -> 10: nfull and partial contradict it
        return 0;
    }
    if (!std::strcmp(mode, "bytes")) {
        for (long long npix : {95LL, 192LL})
            for (int lag = 0; lag < 2; ++lag)
                for (int bits : {16, 32})
                    std::printf("%lld %d %d %lld %lld %lld %lld %lld %lld %lld\n", npix, lag, bits, dx_section_planes_bytes(npix, 3, lag),
                                dx_section_planes_bytes(2, 1, lag), dx_section_pair_bytes(npix), dx_section_hist_bytes(npix, 16, bits),
                                dx_section_signal_bytes(npix), dx_section_batches_bytes(npix, 4), dx_section_round256(dx_section_hist_bytes(npix, 16, bits)));
        return 0;
    }
    return 2;
}
"""

VARIANTS = {1: "npix", 2: "pix0", 3: "nmaps", 4: "a selection word", 5: "type of a selected component", 6: "nindices of a selected component",
            7: "the pair list", 8: "the lag flag", 9: "a histogram plane", 10: "lo", 11: "hi", 12: "nbins", 13: "bits", 14: "a signal spec",
            15: "a batch plane", 16: "nbatch"}
GROUP_OF = {1: 0, 2: 0, 3: 0, 4: 1, 5: 1, 6: 1, 7: 2, 8: 2, 9: 3, 10: 3, 11: 3, 12: 3, 13: 3, 14: 4, 15: 5, 16: 5}


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("section_host")
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


def _fp(exe, v):
    same, head = _exe(exe, "fp %d\n" % v)
    assert same == "1"                                  # equal registrations give equal fingerprints
    f = head.split()
    return int(f[7], 16), [int(x, 16) for x in f[8:14]]


def test_fingerprint_sees_every_single_difference(host_exe):
    base_fp, base_groups = _fp(host_exe, 0)
    seen = {base_fp}
    for v, name in VARIANTS.items():
        fp, groups = _fp(host_exe, v)
        assert fp != base_fp and fp not in seen, name
        seen.add(fp)
        changed = [i for i in range(6) if groups[i] != base_groups[i]]
        assert changed == [GROUP_OF[v]], (name, changed)   # exactly the part that holds the difference
    assert _fp(host_exe, 17) == (base_fp, base_groups)      # the type of a component that is not selected does not count


def test_head_diff_names_what_differs(host_exe):
    def why(v):
        out = _exe(host_exe, "diff %d\n" % v)
        return out[0] if out else ""
    assert why(0) == "" and why(17) == ""
    assert "histogram registrations" in why(10) and "histogram registrations" in why(11) and "histogram registrations" in why(13)
    assert "nbatch is 6 there and 4 here" in why(16) and "lag-1 is missing there and tracked here" in why(8)
    assert "shard" in why(1) and "selection" in why(4) and "pair list" in why(7) and "signal" in why(14) and "batch registrations" in why(15)
    for v in VARIANTS:
        assert why(v), VARIANTS[v]


def test_head_pack_unpack_and_refusals(host_exe):
    out = _exe(host_exe, "head 0\n")
    raw = bytes.fromhex(out[0])
    assert len(raw) == L.SECTION_HEAD_BYTES == 104
    assert out[1] == "[]"
    f = out[2].split()
    assert [int(x) for x in f[:7]] == [1, 11, 1, 4, 4, 2, 3]           # version, count, lag-1, nbatch, batch_len, nfull, partial
    # the bytes are the documented little-endian layout: the Python layer reads the same fields
    h = api.head_unpack(raw)
    assert (h["version"], h["count"], h["lag1"], h["nbatch"], h["batch_len"], h["nfull"], h["partial"]) == (1, 11, 1, 4, 4, 2, 3)
    assert h["fingerprint"] == int(f[7], 16) and list(h["groups"]) == [int(x, 16) for x in f[8:14]]
    assert raw[:4] == b"DXSH" and struct.unpack_from("<q", raw, 8)[0] == 11
    assert "103" in out[3] and "truncated" in out[3] and "truncated" in out[4]
    assert "foreign" in out[5] and "version" in out[6] and "damaged" in out[7] and "contradict" in out[8]
    with pytest.raises(da.DangxError, match="truncated"):
        api.head_unpack(raw[:-1])
    with pytest.raises(da.DangxError, match="foreign"):
        api.head_unpack(b"\0" * 104)
    assert api.head_diff(h, h) == ""
    assert "lag-1 is missing there" in api.head_diff(dict(h, lag1=0), h) and "nbatch is 6 there and 4 here" in api.head_diff(dict(h, nbatch=6), h)
    g = list(h["groups"])
    g[3] ^= 1
    assert "histogram registrations" in api.head_diff(dict(h, groups=tuple(g)), h)


def test_section_byte_counts_match_the_closed_forms(host_exe):
    rows = [[int(x) for x in ln.split()] for ln in _exe(host_exe, "bytes 0\n")]
    assert [(r[0], r[1], r[2]) for r in rows] == [(n, lag, bits) for n in (95, 192) for lag in (0, 1) for bits in (16, 32)]
    for npix, lag, bits, planes, rows_b, pair, hist, sig, batches, rounded in rows:
        parts = 5 if lag else 2
        assert planes == parts * 3 * npix * 8 and rows_b == parts * 1 * 2 * 8
        assert pair == npix * 8 and hist == npix * 16 * bits // 8 and sig == 2 * npix * 8 and batches == 4 * 2 * npix * 8
        assert rounded == -(-hist // 256) * 256


# ---- moments_save / moments_load over a fake engine that serves byte patterns

def _head_bytes(count=11, lag1=1, nbatch=4, batch_len=4, groups=(1, 2, 3, 4, 5, 6), fingerprint=99):
    return struct.pack("<IIqiiqiiqQ6Q", 0x48535844, 1, count, lag1, nbatch, batch_len, count // batch_len, 0, count % batch_len, fingerprint, *groups)


class _FakeStore:
    """What moments_save / moments_load use of an Engine: sections as byte patterns, puts recorded."""

    def __init__(self, pix0=1, npix=95, head=None, sizes=None):
        self.pix0, self.npix = pix0, npix
        self.head = head or _head_bytes()
        self.secs = [(L.SEC_PLANES, 0, 0), (L.SEC_PLANES, 0, 1), (L.SEC_PAIR, 0, 0), (L.SEC_HIST, 0, 0), (L.SEC_HIST, 1, 0),
                     (L.SEC_SIGNAL, 0, 0), (L.SEC_BATCHES, 0, 0)]
        self.sizes = sizes or {s: 8 * (3 + 7 * i) for i, s in enumerate(self.secs)}
        self.put, self.reads = [], []

    def moments_sections(self):
        return list(self.secs)

    def moments_section_bytes(self, f, a=0, b=0):
        return len(self.head) if f == L.SEC_HEAD else self.sizes[(f, a, b)]

    def pattern(self, f, a, b):
        n = self.sizes[(f, a, b)]
        return ((np.arange(n) * 7 + 31 * f + 5 * a + 3 * b) % 251).astype(np.uint8)

    def moments_section_get(self, f, a=0, b=0, device=False, out=None):
        self.reads.append((f, a, b))
        return np.frombuffer(self.head, dtype=np.uint8) if f == L.SEC_HEAD else self.pattern(f, a, b)

    def moments_section_put(self, f, a, b, data):
        self.put.append(((f, a, b), bytes(data)))


def test_save_load_round_trip_and_refusals(tmp_path):
    src = _FakeStore()
    path = str(tmp_path / "run.moments")
    da.moments_save(None, path, engines=[src])
    assert src.reads == [(L.SEC_HEAD, 0, 0)] + src.secs                 # one section at a time, HEAD first
    raw = open(path, "rb").read()
    assert raw[:8] == b"DANGXSEC" and len(raw) == 32 + 32 * 8 + 104 + sum(src.sizes.values())
    assert b"pickle" not in raw and not os.path.exists(path + ".tmp")
    dst = _FakeStore()
    da.moments_load(None, path, engines=[dst])
    assert [k for k, _ in dst.put] == [(L.SEC_HEAD, 0, 0)] + src.secs
    assert dst.put[0][1] == src.head
    for (k, got) in dst.put[1:]:
        assert got == bytes(src.pattern(*k)), k
    # truncated anywhere: refused before anything is put
    for cut in (4, 31, 40, 32 + 32 * 8 - 1, 32 + 32 * 8 + 50, len(raw) - 1):
        bad = str(tmp_path / ("cut%d" % cut))
        open(bad, "wb").write(raw[:cut])
        d = _FakeStore()
        with pytest.raises(da.DangxError, match="truncated|not a file of moments_save"):
            da.moments_load(None, bad, engines=[d])
        assert not d.put
    other = str(tmp_path / "foreign")
    open(other, "wb").write(b"\x80\x04pickle" + raw[10:])
    with pytest.raises(da.DangxError, match="not a file of moments_save"):
        da.moments_load(None, other, engines=[_FakeStore()])
    # another registration, another shard, other sizes: named, nothing put
    d = _FakeStore(head=_head_bytes(groups=(1, 2, 3, 40, 5, 6), fingerprint=98))
    with pytest.raises(da.DangxError, match="histogram registrations"):
        da.moments_load(None, path, engines=[d])
    d2 = _FakeStore(pix0=0)
    with pytest.raises(da.DangxError, match="holds pixels"):
        da.moments_load(None, path, engines=[d2])
    sizes = dict(src.sizes)
    sizes[(L.SEC_HIST, 1, 0)] += 8
    d3 = _FakeStore(sizes=sizes)
    with pytest.raises(da.DangxError, match=r"HIST\(1, 0\)"):
        da.moments_load(None, path, engines=[d3])
    assert not d.put and not d2.put and not d3.put
    # two shards: one file each
    two = [_FakeStore(0, 95), _FakeStore(95, 97)]
    da.moments_save(None, path, engines=two)
    assert os.path.exists(path + ".0") and os.path.exists(path + ".1")
    back = [_FakeStore(0, 95), _FakeStore(95, 97)]
    da.moments_load(None, path, engines=back)
    assert all(len(b.put) == 8 for b in back)


# ---- dist_chains over fake engines on two gloo ranks

class _FakeChain:
    """One shard of one chain as dist_chains and the chains_*_maps read it; value: what its accumulators 'hold'."""

    def __init__(self, value, count=6, hist_hi=2.0, npix=5, pix0=0):
        self.component_list = [da.DangComps(label="dust", type="mbb", nu_ref=353.0, nindices=2, ind_label=["beta", "T"]),
                               da.DangComps(label="mono", type="monopole", nu_ref=353.0)]
        self.bands = [da.BandInfo(label="b%d" % j, nu_c=30.0 * (j + 1)) for j in range(2)]
        self.ddata = da.DangData(sig_map=None, rms_map=None, masks=np.ones((3, npix)))
        self._moment_sel = np.array([1 | (6 << 3), 1], dtype=np.int32)
        self._moment_lag1, self._moment_pairs = True, [((0, 0, 0), (0, 1, 1))]
        self._moment_hist = {"planes": [(0, 1, 1), (0, 0, 0)], "ranges": [(1.0, hist_hi), (-5.0, 5.0)], "nbins": 16, "bits": 16}
        self._moment_signals = [(0, 1, 0)]
        self._moment_batches = {"planes": [(0, 1, 2)], "nbatch": 4, "batch_len": 1}
        self.npix, self.pix0, self.nmaps, self.nbands = npix, pix0, 3, 2
        self.value, self.count, self.hist_hi = float(value), count, hist_hi
        self.held = {}

    def moments_count(self):
        return self.count

    def moments_section_bytes(self, f, a=0, b=0):
        return 104 if f == L.SEC_HEAD else 40

    def moments_section_get(self, f, a=0, b=0, device=False, out=None):
        if f == L.SEC_HEAD:
            hist = 4 if self.hist_hi == 2.0 else 44
            return np.frombuffer(_head_bytes(self.count, 1, 4, 2, (1, 2, 3, hist, 5, 6), 90 + hist), dtype=np.uint8)
        # five parts of 8 bytes, each the chain's value and the section's address
        return np.tile(np.array([self.value, f, a, b, 0, 0, 0, 0], dtype=np.uint8), 5)

    def synchronize(self):
        pass


class _FakeHolder(_FakeChain):
    def __init__(self, src):
        super().__init__(-1.0, npix=src.npix, pix0=src.pix0)
        self.log = []
        for name in [n for n in vars(self) if n.startswith("_moment_")]:      # a fresh Engine knows no registration
            delattr(self, name)

    def moments_begin_like(self, like):
        self.held, self.value = {}, -1.0
        for name in [n for n in vars(like) if n.startswith("_moment_")]:
            setattr(self, name, getattr(like, name))
        self.log.append("begin_like")

    def moments_section_put(self, f, a, b, data):
        data = np.asarray(data)
        self.held[(f, a, b)] = data.size
        if f == L.SEC_HEAD:
            self.count = api.head_unpack(data)["count"]
        else:
            self.value = float(data[0])              # the sender's value travels in the payload
        self.log.append((f, a, b, data.size))

    def moments_held_bytes(self):
        return sum(v for k, v in self.held.items() if k[0] != L.SEC_HEAD)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_api():
    """the thin getters replaced by host functions of the chains' values in list order"""
    def code(engs):
        assert all(e.value >= 0 for e in engs), "a holder was read before its section arrived"
        return float(sum((k + 1) * e.value for k, e in enumerate(engs)))       # depends on the ORDER of the chains

    api._holder_engine = _FakeHolder
    api.chains_get = lambda engs, l, what, stat, ddof=0, device=False, out=None: np.full((3, engs[0].npix), code(engs) + 100 * what)
    api.chains_get_template = lambda engs, l, stat, ddof=0, out=None: np.full((3, 2), code(engs))
    api.chains_get_signal = lambda engs, s, stat, ddof=0, device=False, out=None: np.full(engs[0].npix, code(engs))
    api.chains_get_pair = lambda engs, p, stat, ddof=0, device=False, out=None: np.full(engs[0].npix, code(engs))
    api.chains_hist_stat = lambda engs, reg, stat, q=None, device=False, out=None: np.full((len(q), engs[0].npix) if stat == "quantile" else engs[0].npix, code(engs))
    api.chains_hist_rank = lambda engs, reg, stat, device=False, out=None: np.full(engs[0].npix, code(engs) + reg)
    api.chains_batches_get = lambda engs, reg, stat, first=0, ddof=0, device=False, out=None: np.full(engs[0].npix, code(engs))


def _dist_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    td.init_process_group("gloo", rank=rank, world_size=world)
    _fake_api()
    res = {}
    # rank 0 holds chains of value 1 and 2, rank 1 one chain of value 3: global order 1, 2, 3 -> code 1 + 4 + 9 = 14
    local = [[_FakeChain(1.0)], [_FakeChain(2.0)]] if rank == 0 else [[_FakeChain(3.0)]]
    dc = da.dist_chains(local, dst=0)
    res["order"], res["counts"] = list(dc.order), list(dc.counts)
    sets = {}
    for name, fn in (("posterior", api.chains_posterior_maps), ("pair", api.chains_pair_maps), ("quantile", api.chains_quantile_maps),
                     ("rank", api.chains_rank_maps), ("batch", api.chains_batch_maps), ("signal", api.chains_signal_maps)):
        m = fn(dc)
        sets[name] = None if m is None else {repr(k): float(np.ravel(next(v for v in e.values() if isinstance(v, np.ndarray)) if isinstance(e, dict) else e)[0])
                                             for k, e in m.items()}
        res["fetched_" + name] = list(dc.fetched)
        res["peak_" + name] = dc.peak_held
    res["sets"] = sets
    if rank == 0:
        res["holder_log"] = list(dc._holders[(1, 0)][0].log)
    # dst=None: the maps on every rank, the same order on both
    both = da.dist_chains(local, dst=None)
    res["all_signal"] = {repr(k): float(e["mean"][0]) for k, e in api.chains_signal_maps(both).items()}
    # a rank registered differently: every rank raises, before anything moves and without waiting for the other
    odd = [[_FakeChain(1.0)], [_FakeChain(2.0)]] if rank == 0 else [[_FakeChain(3.0, hist_hi=2.5)]]
    try:
        da.dist_chains(odd, dst=0)
        res["mismatch"] = "no error"
    except da.DangxError as ex:
        res["mismatch"] = str(ex)
    # a mismatch that appears later (the counts of one chain's shards) is seen by the gather in front of the next map call
    try:
        da.dist_chains([[_FakeChain(1.0, npix=5), _FakeChain(1.0, count=7, npix=4, pix0=5)]] if rank == 0 else [[_FakeChain(3.0), _FakeChain(3.0, npix=4, pix0=5)]], dst=0)
        res["counts_mismatch"] = "no error"
    except da.DangxError as ex:
        res["counts_mismatch"] = str(ex)
    try:
        da.dist_chains([[_FakeChain(1.0)]] * (5 if rank == 0 else 4), dst=0)
        res["too_many"] = "no error"
    except da.DangxError as ex:
        res["too_many"] = str(ex)
    np.save(out + ".%d.npy" % rank, np.array([res], dtype=object), allow_pickle=True)
    td.barrier()
    td.destroy_process_group()


def test_dist_chains_order_sections_and_refusals(tmp_path):
    out = str(tmp_path / "res")
    mp.spawn(_dist_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = (np.load(out + ".%d.npy" % r, allow_pickle=True)[0] for r in (0, 1))
    P, PA, H, S, B = L.SEC_PLANES, L.SEC_PAIR, L.SEC_HIST, L.SEC_SIGNAL, L.SEC_BATCHES
    for r in (r0, r1):
        assert r["order"] == [(0, 0), (0, 1), (1, 0)] and r["counts"] == [6, 6, 6]   # rank order, list order within a rank
        # what each map set asks for: (shard, family, a, b, with the lag-1 parts)
        assert r["fetched_posterior"] == [(0, P, 0, 0, True), (0, P, 0, 1, True), (0, P, 1, 0, True)]
        assert r["fetched_pair"] == [(0, PA, 0, 0, False), (0, P, 0, 0, False), (0, P, 0, 1, False)]
        assert r["fetched_quantile"] == [(0, H, 0, 0, False), (0, H, 1, 0, False)] == r["fetched_rank"]   # one registration at a time
        assert r["fetched_batch"] == [(0, B, 0, 0, False)] and r["fetched_signal"] == [(0, S, 0, 0, False)]
        assert "rank 1 chain 0 shard 0 is registered differently" in r["mismatch"] and "histogram registrations" in r["mismatch"]
        assert "different sample counts" in r["counts_mismatch"] and "2 to 8 chains in all, not 9" in r["too_many"]
        assert r["all_signal"] == {repr(("dust", "b1", "T")): 14.0}
    assert all(v is None for v in r1["sets"].values())                    # the maps are on dst
    s0 = r0["sets"]
    assert set(s0["posterior"]) == {repr(("dust", "amplitude")), repr(("dust", "beta")), repr(("mono", "amplitude"))}
    assert s0["posterior"][repr(("dust", "beta"))] == 114.0 and s0["signal"] == {repr(("dust", "b1", "T")): 14.0}
    assert s0["rank"] == {repr(("dust", "beta", 1)): 14.0, repr(("dust", "amplitude", 0)): 15.0}
    assert list(s0["pair"].values()) == [14.0] and list(s0["batch"].values()) == [14.0]
    # the holder of rank 1's chain on rank 0: emptied, given HEAD, then the sections of ONE unit; the payload without the lag-1
    # parts is two fifths
    log = r0["holder_log"]
    i = len(log) - 1 - log[::-1].index((L.SEC_SIGNAL, 0, 0, 40))
    assert log[i - 2:i + 2] == ["begin_like", (L.SEC_HEAD, 0, 0, 104), (L.SEC_SIGNAL, 0, 0, 40), "begin_like"]
    assert (P, 0, 1, 40) in log and (P, 0, 1, 16) in log and (P, 1, 0, 40) in log     # ess: all five parts; the pair: mean and m2
    assert r0["peak_rank"] == 40 and r0["peak_quantile"] == 40 and r0["peak_pair"] == 40 + 16 + 16
    assert r1["peak_rank"] == 0
