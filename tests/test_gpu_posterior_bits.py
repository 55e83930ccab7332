"""The posterior summaries give the BITS they gave before the layer moved into dang_amd/posterior.py (one family table, one map
builder): every *_maps function over one run -- the C2 model at Nside 4 with a fitted Q/U template, three chains, each as two
shards of 95 and 97 pixels with masked pixels in both, every registration made, ten samples (the batches have merged twice) --
against tests/golden/posterior_parent_bits.npz, written by record() below from the parent commit on the same device family.
Keys, key order and non-array entries must be equal, every array equal bit for bit (NaNs by position): nothing here may change a
kernel, a grid or a launch order, so there is no tolerance.

The fixture holds every array whole, packed so that it stays small: the arrays of a variant call (masked_value, ddof, the
restored run) as the XOR of their bits with the same array of the plain call, the bytes of every array transposed so that
the exponents lie together, and an array whose packed bytes were stored before as a reference to that copy."""
import copy
import json
import os
import tempfile

import numpy as np
import pytest

import dang_amd as da
from dang_amd import synth

from util import MAPN, shard_engines

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posterior_parent_bits.npz")
BOUNDS = [0, 95, 192]          # two shards of unequal, odd size; make_sky masks pixels 87..105: eight in the first, eleven in the second
SEEDS = (4321, 4322, 4323)
SAMPLES = 10
UNSEEN = -1.6375e30


def _case():
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=4, device="cpu", as_numpy=False, start="truth")
    synth.add_qu_template(ddata, comps, meta, fit_bands=(2, 3, 4), amplitudes=(2.0, -1.5, 0.7))
    ddata.sig_map, ddata.rms_map, ddata.masks = (t.numpy() for t in (ddata.sig_map, ddata.rms_map, ddata.masks))
    for c in comps:
        c.amplitude = c.amplitude.numpy()
        c.indices = None if c.indices is None else c.indices.numpy()
    return dpar, ddata, bands, comps, meta


def _registered_shards(dpar):
    engs = shard_engines(_case(), 2, bounds=BOUNDS)
    assert [e.npix for e in engs] == [95, 97] and all((e.ddata.masks[0] == 0).any() for e in engs)
    da.moments_begin(dpar, None, engines=engs)
    da.moments_pairs(dpar, None, lag1=True, engines=engs)
    da.moments_hist(dpar, None, nbins=16, engines=engs)
    specs = da.moments_signals(dpar, None, engines=engs)
    assert any(kind == 3 for _, _, kind in specs)
    da.moments_batches(dpar, None, nbatch=4, batch_len=1, engines=engs)
    return engs


def _gibbs(dpar, engs, it):
    """one Gibbs iteration of a chain of several shards: every solve over the shards together, then every sweep on each"""
    for g in dpar.cg_groups:
        for f in g.pol_flag:
            da.sky_amp_sample(engs, g.cg_group, f, dpar.ml_mode, dpar.seed, da.stream_id(it, 0, g.cg_group, 0, f))
    for l, c in enumerate(engs[0].component_list):
        for j in range(c.nindices):
            for f in (c.pol_flag[j] if c.sample_index[j] else ()):
                for e in engs:
                    e.index_sample(l, j, MAPN[f], dpar.nsample, dpar.ml_mode, dpar.seed, da.stream_id(it, 1, l, j, f))


def run():
    """{call: what it returned} in a fixed order: the eleven functions plain, with masked_value, with ddof=1 (where they take it),
    posterior_batch_maps(first=1), and posterior_maps of chain 0 saved and loaded into fresh engines"""
    dpar0 = _case()[0]
    chains = []
    for seed in SEEDS:
        dpar = copy.copy(dpar0)
        dpar.seed = seed
        engs = _registered_shards(dpar)
        for it in range(1, SAMPLES + 1):
            _gibbs(dpar, engs, it)
            da.moments_accumulate(None, engines=engs)
        assert engs[0].moments_batches_info() == {"batch_len": 4, "nfull": 2, "partial": 2}
        chains.append(engs)
    one = chains[0]
    single = {"posterior_maps": da.posterior_maps, "posterior_pair_maps": da.posterior_pair_maps, "posterior_quantile_maps": da.posterior_quantile_maps,
              "posterior_batch_maps": da.posterior_batch_maps, "posterior_signal_maps": da.posterior_signal_maps}
    pooled = {"chains_posterior_maps": da.chains_posterior_maps, "chains_pair_maps": da.chains_pair_maps, "chains_quantile_maps": da.chains_quantile_maps,
              "chains_rank_maps": da.chains_rank_maps, "chains_batch_maps": da.chains_batch_maps, "chains_signal_maps": da.chains_signal_maps}
    no_ddof = ("posterior_quantile_maps", "chains_quantile_maps", "chains_rank_maps")
    out = {}
    for tag, kw in (("", {}), ("|masked", {"masked_value": UNSEEN}), ("|ddof1", {"ddof": 1})):
        for name, fn in single.items():
            if not (kw.get("ddof") and name in no_ddof):
                out[name + tag] = fn(None, engines=one, **kw)
        for name, fn in pooled.items():
            if not (kw.get("ddof") and name in no_ddof):
                out[name + tag] = fn(chains, **kw)
    out["posterior_batch_maps|first1"] = da.posterior_batch_maps(None, first=1, engines=one)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "run.moments")
        da.moments_save(None, path, engines=one)
        fresh = _registered_shards(dpar0)
        da.moments_load(None, path, engines=fresh)
        out["posterior_maps|restored"] = da.posterior_maps(None, engines=fresh)
    return out


def flatten(out):
    """[(call, "call/key/entry", value)] in the order of the dicts: arrays as they are, everything else as JSON gives it back"""
    flat = []
    for call, maps in out.items():
        for key, entry in maps.items():
            for name, v in (entry.items() if isinstance(entry, dict) else [("", entry)]):
                if not isinstance(v, np.ndarray):
                    v = json.loads(json.dumps(v))
                flat.append((call, "%s/%r/%s" % (call, key, name), v))
    return flat


def _pack(a, base):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    bits = a.view(np.uint64).ravel()
    if base is not None:
        bits = bits ^ base.view(np.uint64).ravel()
    return np.ascontiguousarray(bits.view(np.uint8).reshape(-1, 8).T)


def _unpack(packed, shape, base):
    bits = np.ascontiguousarray(packed.T).view(np.uint64).ravel()
    if base is not None:
        bits = bits ^ base.view(np.uint64).ravel()
    return bits.view(np.float64).reshape(shape)


def _base_name(call, name, arrays):
    """the same array of the plain call, when the call is a variant and the plain call has it with this shape"""
    plain = call.split("|")[0]
    other = plain + name[len(call):]
    return other if plain != call and other in arrays else None


def record(path):
    """writes the fixture from the build that is loaded (run once, on the parent commit)"""
    index, members, seen, arrays = [], {}, {}, {}
    for call, name, v in flatten(run()):
        if not isinstance(v, np.ndarray):
            index.append([name, "value", v])
            continue
        base = _base_name(call, name, arrays)
        if base is not None and arrays[base].shape != v.shape:
            base = None
        arrays[name] = v
        packed = _pack(v, arrays[base] if base else None)
        member = seen.setdefault(packed.tobytes(), "a%d" % len(members))
        members.setdefault(member, packed)
        index.append([name, "array", {"member": member, "base": base, "shape": list(v.shape)}])
    np.savez_compressed(path, index=np.array(json.dumps(index)), **members)


def test_posterior_bits_are_the_parents(built):
    with np.load(GOLDEN) as z:
        index = json.loads(str(z["index"]))
        members = {k: z[k] for k in z.files if k != "index"}
    got = flatten(run())
    assert [name for _, name, _ in got] == [name for name, _, _ in index]          # keys and key order, of the maps and of their entries
    assert len({name.split("/")[0] for name, _, _ in index}) == 11 + 11 + 8 + 2
    want, bad = {}, []
    for (_, name, v), (_, kind, w) in zip(got, index):
        if kind == "value":
            assert not isinstance(v, np.ndarray) and v == w, (name, v, w)
            continue
        want[name] = _unpack(members[w["member"]], w["shape"], want[w["base"]] if w["base"] else None)
        assert isinstance(v, np.ndarray) and v.dtype == np.float64 and list(v.shape) == w["shape"], name
        if not np.array_equal(v, want[name], equal_nan=True):
            bad.append((name, int(np.count_nonzero(v.view(np.int64) != want[name].view(np.int64)))))
    assert not bad, "arrays that differ from the parent's (name, values whose bits differ): %s" % bad[:20]
