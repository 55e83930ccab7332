"""The sampling entry points (dang_amd/csrc/dangx_entry.hip) against a record of the commit before their host logic was
rewritten (the deferred solve and the index pair passed as arguments, one place per bookkeeping rule): every return value, the
cached chi^2 of every plane after every call (NaN where the engine answers None -- that is how the validity flags show), the
masked sums of every swept index map and, at the end, every amplitude, index and template-amplitude map must be the recorded
BITS (tests/golden/entry_routes_parent_bits.npz, written by record() below on the same device family).  Each case names the
branch of the file it takes; between them they take every one."""
import copy
import os

import numpy as np
import pytest

import dang_amd as da
from dang_amd import _lib as L

from test_oracle_templates_cpu import add_globals
from util import MAPN, make_case, shard_engines

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_routes_parent_bits.npz")
ITERATIONS = 2
NSIDE = 2           # 48 pixels (5 of them masked): the routes are host decisions, one block shows them
CUT = 21            # two contexts on one device: pixels [0, 21) and [21, 48), both of odd length


def _jeffreys(dpar, ddata, bands, comps):        # 'synch' on T: the register Jeffreys chain; 'synch_P', the dust: the LDS chain
    for c in comps:
        c.prior_type = ["jeffreys"] * c.nindices


def _jeffreys_second(dpar, ddata, bands, comps):  # the dust T only: the beta sweep keeps its register chain, the pair has no form
    for c in comps:
        if c.nindices == 2:
            c.prior_type = [c.prior_type[0], "jeffreys"]


def _bandpass(dpar, ddata, bands, comps):        # every second band bandpass-integrated: a.bp = 1
    rng = np.random.default_rng(4)
    for b in bands[1::2]:
        nu = b.nu_c * 1e9 * np.linspace(0.9, 1.1, 9)
        tau = rng.uniform(0.2, 1.0, nu.size)
        nu[3] = 0.0
        b.id, b.nu0, b.tau0 = "bp", nu, tau / tau.sum()


def _unequal(dpar, ddata, bands, comps):         # Q and U index maps differ: per-plane SED columns in the fused launch
    rng = np.random.default_rng(2)
    for c in comps:
        if c.nindices and c.cg_group == 2:
            c.indices[0, 2] *= 1.0 + 0.02 * rng.standard_normal(c.indices.shape[-1])


def _template(dpar, ddata, bands, comps):        # a Q/U template fitted at the last two bands in the Q+U group
    nb = ddata.sig_map.shape[0]
    add_globals(dpar, ddata, bands, comps, ("template",), 2, fit_bands=[nb - 2, nb - 1])


def _monopole(dpar, ddata, bands, comps):        # a monopole fitted at three bands in the T group
    nb = ddata.sig_map.shape[0]
    add_globals(dpar, ddata, bands, comps, ("monopole",), 1, fit_bands=[0, nb - 2, nb - 1])


def _case(config, tweak=None, start="truth", **kw):
    return make_case(config, nside=NSIDE, start=start, tweak=tweak, **kw)


def _sweeps(comps, group, flag, it):
    return [(l, j, da.stream_id(it, 1, l, j, flag)) for l, c in enumerate(comps) for j in range(c.nindices)
            if c.cg_group == group and c.sample_index[j] and flag in c.pol_flag[j]]


def _planes(flag):
    return {L.FLAG_T: (1,), L.FLAG_Q: (2,), L.FLAG_U: (3,), L.FLAG_QU: (2, 3)}[flag]


class Recorder:
    """what one case leaves behind: `ret` -- per call, whether it raised and the numbers it returned; `chi` -- per call and
    engine, chisq_cached(0|1, k, k) of every plane; `sums` / `counts` -- index_masked_sums of the swept maps"""

    def __init__(self):
        self.engines, self.ret, self.chi, self.sums, self.counts = [], [], [], [], []

    def engine(self, case):
        dpar, ddata, bands, comps, meta = case
        e = da.Engine(bands, copy.deepcopy(comps), ddata, npix_global=meta["npix_global"], pix0=meta["pix0"], device=0)
        self.engines.append(e)
        return e

    def shards(self, case):
        engs = shard_engines(case, 2, [0, CUT, case[4]["npix_global"]])
        self.engines += engs
        return engs

    def _flat(self, r):
        if isinstance(r, (tuple, list)):
            for x in r:
                self._flat(x)
        elif r is not None:
            self.ret.append(float(r))

    def observe(self, engs, flag=None, swept=()):
        for e in engs:
            for which in (0, 1):
                for k in range(1, e.nmaps + 1):
                    v = e.chisq_cached(which, k, k)
                    self.chi.append(np.nan if v is None else v)
            entries = [(s[0], s[1], k) for s in swept for k in _planes(flag)]
            if entries:
                s, n = e.index_masked_sums(entries)
                self.sums += list(s)
                self.counts += list(n)

    def call(self, engs, fn, flag=None, swept=(), observe=True):
        """one entry call on the engine(s): its return values (or that it raised), then what it left observable"""
        try:
            r, raised = fn(), 0
        except da.DangxError:
            r, raised = None, 1
        self.ret.append(float(raised))
        self._flat(r)
        if observe:
            self.observe(engs if isinstance(engs, (list, tuple)) else [engs], flag, swept)

    def arrays(self):
        out = {"ret": np.asarray(self.ret, dtype=np.float64), "chi": np.asarray(self.chi, dtype=np.float64),
               "sums": np.asarray(self.sums, dtype=np.float64), "counts": np.asarray(self.counts, dtype=np.int64)}
        for q, e in enumerate(self.engines):
            for l, c in enumerate(e.component_list):
                out["e%d_amp%d" % (q, l)] = np.ascontiguousarray(e.get_amplitude(l), dtype=np.float64)
                if c.nindices:
                    out["e%d_idx%d" % (q, l)] = np.ascontiguousarray(e.get_indices(l), dtype=np.float64)
                if c.type in ("template", "monopole", "hi_fit"):
                    out["e%d_tamp%d" % (q, l)] = np.ascontiguousarray(e.get_template_amplitudes(l), dtype=np.float64)
        return out


def _loop(case, step):
    """step(it, group, flag, amplitude stream, sweeps of the plane set) for every CG group of ITERATIONS iterations"""
    dpar, comps = case[0], case[3]
    for it in range(1, ITERATIONS + 1):
        for g in dpar.cg_groups:
            f = g.pol_flag[0]
            step(it, g.cg_group, f, da.stream_id(it, 0, g.cg_group, 0, f), _sweeps(comps, g.cg_group, f, it))


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


# ---- 1. dangx_amp_sample alone, on T and on Q+U

def _amp_alone(R, c, current=False, **kw):
    e = R.engine(c)
    ml_mode = kw.pop("ml_mode", "sample")

    def step(it, group, f, sa, sw):
        R.call(e, lambda: e.amp_sample(group, f, ml_mode, 11, sa, **kw), f)
        if current:   # 8. chisq_current after a solve without sweeps
            R.call(e, lambda: e.chisq_current(1, 3))
    _loop(c, step)


@case
def amp_byproduct(R):
    """C3: planeset_group(solve = 1) holds and dx_planeset_lanes != 0 -- the solve is planeset_launch without items, chi^2 of its state
    is cached (both slots valid); chisq_current then reads the cache"""
    _amp_alone(R, _case("C3"), current=True)


@case
def amp_plain(R):
    """C2, 5 bands: no plane-set form -- counters[0] zeroed, dx_launch_amp, the count read back; chi^2 invalid on the planes, so
    chisq_current makes its explicit pass per plane and fills the 'after' slot"""
    _amp_alone(R, _case("C2"), current=True)


@case
def amp_cg(R):
    """C2, DANGX_SOLVER_CG on a diffuse group: device_cg, cg_iters returned"""
    _amp_alone(R, _case("C2", start="prior"), solver="cg", i_max=15, converge=1e-6)


@case
def amp_schur(R):
    """C2 + Q/U template: a.nt > 0 on Q+U -- device_schur on one context, cg_iters = -nullity; the T group is a diffuse solve beside
    a template without a signal on its plane"""
    _amp_alone(R, _case("C2", _template))


@case
def amp_cg_template(R):
    """C2 + Q/U template with the CG solver: a.nt > 0 and solver == CG skips the Schur branch for the mixed operators"""
    _amp_alone(R, _case("C2", _template, start="prior"), solver="cg", i_max=10, converge=1e-6)


@case
def amp_correct(R):
    """C3, DANGX_FLUCT_CORRECT on diffuse groups: the by-product route with the textbook term"""
    _amp_alone(R, _case("C3"), fluct_mode="correct")


@case
def amp_correct_plain(R):
    """C2, DANGX_FLUCT_CORRECT on diffuse groups: dx_launch_amp with the textbook term"""
    _amp_alone(R, _case("C2"), fluct_mode="correct")


@case
def amp_schur_correct(R):
    """C2 + Q/U template, DANGX_FLUCT_CORRECT: textbook_refused is false for a template member, the Schur passes carry the term"""
    _amp_alone(R, _case("C2", _template), fluct_mode="correct")


@case
def amp_refusals(R):
    """C2 + monopole: the textbook term is refused on the T group (Schur branch) and with the CG solver; the solve's bookkeeping
    (chi^2 invalid, plane_nz) has happened before either refusal.  A bad ml_mode fails before anything"""
    c = _case("C2", _monopole)
    e = R.engine(c)
    e.index_sample(1, 0, 1, 2, "sample", 1, 1)
    R.call(e, lambda: e.amp_sample(1, L.FLAG_T, "sample", 5, 7, fluct_mode="correct"), L.FLAG_T)
    e.index_sample(1, 0, 1, 2, "sample", 1, 2)
    R.call(e, lambda: e.amp_sample(1, L.FLAG_T, "sample", 5, 7, solver="cg", fluct_mode="correct"), L.FLAG_T)
    R.call(e, lambda: e.amp_sample(1, L.FLAG_T, "sample", 5, 7), L.FLAG_T)
    R.call(e, lambda: e.lib.dangx_amp_sample(e.h, 1, L.FLAG_T, 99, L.SOLVER_DIRECT, L.FLUCT_REFERENCE, 5, 7, 10, 1e-8, None, None), L.FLAG_T)


@case
def amp_optimize(R):
    """C3, ml_mode optimize: the by-product route without a fluctuation term"""
    _amp_alone(R, _case("C3"), ml_mode="optimize")


@case
def amp_no_counts(R):
    """C2 without counters (cg_iters = n_not_spd = NULL): no memset, no read-back"""
    _amp_alone(R, _case("C2"), want_counts=False)


# ---- 2. dangx_index_sample on T, Q, U and Q+U

def _index_alone(R, c, single_planes=True, ml_mode="sample"):
    e = R.engine(c)
    comps = c[3]

    def step(it, group, f, sa, sw):
        for (l, j, s) in sw:
            R.call(e, lambda: e.index_sample(l, j, MAPN[f], 6, ml_mode, 17, s), f, [(l, j)])
        if f == L.FLAG_QU and single_planes:   # one plane of the pair: qu_equal goes off, the next Q+U sweep stages both planes
            l, j, s = sw[0]
            R.call(e, lambda: e.index_sample(l, j, 2, 6, ml_mode, 17, s + 1), L.FLAG_Q, [(l, j)])
            R.call(e, lambda: e.index_sample(l, j, 3, 6, ml_mode, 17, s + 2, want_counts=False), L.FLAG_U, [(l, j)])
    _loop(c, step)


@case
def index_register(R):
    """C3: delta bands, chisq, gaussian priors -- reg_ok, dx_launch_mh_reg, no solve waiting and no pair"""
    _index_alone(R, _case("C3"))


@case
def index_register_optimize(R):
    """C3, ml_mode optimize on the register chain"""
    _index_alone(R, _case("C3"), single_planes=False, ml_mode="optimize")


@case
def index_jeffreys(R):
    """C3, Jeffreys priors everywhere: 'synch' on T keeps the register chain (a.jeff = 1), 'synch_P' and the dust take the LDS chain"""
    _index_alone(R, _case("C3", _jeffreys))


@case
def index_bandpass(R):
    """C3 with bandpass-integrated bands: a.bp = 1, reg_ok false, the LDS chain in its compile-time modes"""
    _index_alone(R, _case("C3", _bandpass), single_planes=False)


@case
def index_constant_start(R):
    """C3 from the prior: every index map is spatially constant, the first sweep clears its idx_const bits and sets dirty before
    sync_model"""
    _index_alone(R, _case("C3", start="prior"))


@case
def index_rejected(R):
    """C3 from the prior: a sweep rejected for its index number has already marked the maps as varying (idx_const cleared before
    validation); bad map_n and bad ml_mode are rejected after sync_model.  The sweeps that follow see that state"""
    c = _case("C3", start="prior")
    e = R.engine(c)
    R.call(e, lambda: e.index_sample(1, 7, 1, 6, "sample", 17, 3), L.FLAG_T)
    R.call(e, lambda: e.index_sample(2, 0, 5, 6, "sample", 17, 3), L.FLAG_T)
    R.call(e, lambda: e.lib.dangx_index_sample(e.h, 2, 0, 1, 6, 99, 17, 3, None), L.FLAG_T)
    R.call(e, lambda: e.amp_index_sample(1, L.FLAG_T, "sample", 3, 5, 1, 0, 1, 6, 3, 7), L.FLAG_T, [(1, 0)])
    R.call(e, lambda: e.index_sample(2, 0, 1, 6, "sample", 17, 4), L.FLAG_T, [(2, 0)])


# ---- 3. dangx_index_sample_pair

def _pairs(R, c, comps_with=lambda c: c.nindices == 2, want_counts=True):
    e = R.engine(c)
    for it in range(1, ITERATIONS + 1):
        for l, cc in enumerate(c[3]):
            if not comps_with(cc):
                continue
            f = cc.pol_flag[0][0]
            s1, s2 = da.stream_id(it, 1, l, 0, f), da.stream_id(it, 1, l, 1, f)
            R.call(e, lambda: e.index_sample_pair(l, 0, MAPN[f], 6, "sample", 17, s1, s2, want_counts=want_counts), f, [(l, 0), (l, 1)][:cc.nindices])


@case
def pair_fused(R):
    """C3 dust beta -> T on T and on Q+U: dx_launch_mh_pair runs, the wrapper records index nind + 1 and reads counters[2]"""
    _pairs(R, _case("C3"))


@case
def pair_fused_no_counts(R):
    """the same without accepted counts: no memset of counters[1..2], no read-back"""
    _pairs(R, _case("C3"), want_counts=False)


@case
def pair_lane_pairs(R):
    """C5, 20 bands: the T plane takes the pair kernel, on Q+U dx_launch_mh_pair declines (lane-pair chains) and the two sweeps run"""
    _pairs(R, _case("C5"))


@case
def pair_one_index(R):
    """C3 synchrotron (one index): nind + 1 == nindices, the first sweep runs alone and the second call is rejected"""
    _pairs(R, _case("C3"), lambda c: c.type == "power-law")


@case
def pair_jeffreys_powerlaw(R):
    """C3, a power-law with a Jeffreys prior: a.jeff = 1 on 'synch', one index, the fallback as above on the Jeffreys chains"""
    _pairs(R, _case("C3", _jeffreys), lambda c: c.type == "power-law")


@case
def pair_jeffreys_second(R):
    """C3, Jeffreys prior on the dust T only: the beta sweep is reg_ok but ok_b is false -- the two calls, the second on the LDS chain"""
    _pairs(R, _case("C3", _jeffreys_second))


@case
def pair_lds(R):
    """C3, Jeffreys priors on both dust indices: reg_ok false, the pair is not tried"""
    _pairs(R, _case("C3", _jeffreys))


# ---- 4. dangx_amp_index_sample

def _amp_index(R, c, warm=True, **kw):
    e = R.engine(c)
    if warm:   # make the index maps "varying" so that the fused route is the one that is tried
        for l, cc in enumerate(c[3]):
            if cc.nindices and cc.sample_index[0]:
                f = cc.pol_flag[0][0]
                e.index_sample(l, 0, MAPN[f], 2, "sample", 1, 1)

    def step(it, group, f, sa, sw):
        l, j, s = sw[0]
        R.call(e, lambda: e.amp_index_sample(group, f, "sample", 11, sa, l, j, MAPN[f], 6, 11, s, **kw), f, [(l, j)])
        for (l2, j2, s2) in sw[1:]:
            R.call(e, lambda: e.index_sample(l2, j2, MAPN[f], 6, "sample", 11, s2), f, [(l2, j2)])
    _loop(c, step)
    return e


@case
def amp_index_fused(R):
    """C3 after a warm-up sweep: can holds, the solve is handed to the sweep, dx_launch_fused runs both; counters[0] zeroed before
    and read after"""
    _amp_index(R, _case("C3"))


@case
def amp_index_fused_no_counts(R):
    """the same without counters"""
    _amp_index(R, _case("C3"), want_counts=False)


@case
def amp_index_unequal(R):
    """C3 with unequal Q/U index maps: fused, per-plane SED columns"""
    _amp_index(R, _case("C3", _unequal))


@case
def amp_index_c5(R):
    """C5: fused in the lane-pair form on Q+U; on T dx_fused_lanes says 0 -- the handed-over solve is launched by the sweep
    (dx_launch_amp) before its own register chain, and the count is still read from counters[0]"""
    _amp_index(R, _case("C5"))


@case
def amp_index_five_bands(R):
    """C2, 5 bands: dx_fused_supported false -- the two calls"""
    _amp_index(R, _case("C2"))


@case
def amp_index_jeffreys(R):
    """C3, Jeffreys priors: prior_fast false for the dust and 'synch_P' -- the two calls; 'synch' on T is prior_fast, can holds, and
    the fused launch carries the Jeffreys chain or declines"""
    _amp_index(R, _case("C3", _jeffreys))


@case
def amp_index_correct(R):
    """C3, DANGX_FLUCT_CORRECT: can false at the first test -- the two calls"""
    _amp_index(R, _case("C3"), fluct_mode="correct")


@case
def amp_index_cg(R):
    """C2 with the CG solver: can false -- the two calls"""
    _amp_index(R, _case("C2"), solver="cg", i_max=10, converge=1e-6)


@case
def amp_index_constant(R):
    """C3 from the prior without the warm-up: idx_const set on the first iteration -- first sweeps on constant maps go the
    two-call way; the second iteration is fused"""
    _amp_index(R, _case("C3", start="prior"), warm=False)


@case
def amp_index_template(R):
    """C3 + Q/U template: g.nt != 0 on Q+U and g.nuc != 0 on T -- the two calls on both groups"""
    _amp_index(R, _case("C3", _template))


@case
def amp_index_bandpass(R):
    """C3 with bandpass bands: all_delta == 0 -- the two calls"""
    _amp_index(R, _case("C3", _bandpass))


@case
def amp_index_other_planes(R):
    """C3: the sweep's planes are not the solve's (want != map_n), and a sweep of a component outside the group -- the two calls"""
    c = _case("C3")
    e = R.engine(c)
    e.index_sample(1, 0, 1, 2, "sample", 1, 1)
    e.index_sample(5, 0, -1, 2, "sample", 1, 1)
    R.call(e, lambda: e.amp_index_sample(1, L.FLAG_T, "sample", 3, 5, 5, 0, -1, 6, 3, 7), L.FLAG_QU, [(5, 0)])
    R.observe([e], L.FLAG_T)
    R.call(e, lambda: e.amp_index_sample(2, L.FLAG_QU, "sample", 3, 6, 1, 0, 1, 6, 3, 8), L.FLAG_T, [(1, 0)])
    R.call(e, lambda: e.amp_index_sample(2, L.FLAG_QU, "sample", 3, 6, 5, 0, 2, 6, 3, 9), L.FLAG_Q, [(5, 0)])


@case
def amp_index_failing_sweep(R):
    """C3, tests/test_gpu_fused.py::test_a_failing_sweep_still_leaves_the_solve_done: the sweep is rejected (synch has no index 7)
    -- can is false for that index, so this is the two calls, and the solve has happened when the call raises.  Then the fused
    route, and a call whose SOLVE is rejected on the fused route (bad ml_mode: can holds, the preparation fails, nothing is
    handed over and no sweep runs)"""
    c = _case("C3")
    e = R.engine(c)
    e.index_sample(1, 0, 1, 2, "sample", 1, 1)
    R.call(e, lambda: e.amp_index_sample(1, L.FLAG_T, "sample", 3, 5, 1, 7, 1, 6, 3, 7), L.FLAG_T)
    R.call(e, lambda: e.amp_index_sample(1, L.FLAG_T, "sample", 3, 5, 1, 0, 1, 6, 3, 7), L.FLAG_T, [(1, 0)])
    R.call(e, lambda: e.lib.dangx_amp_index_sample(e.h, 1, L.FLAG_T, 99, L.SOLVER_DIRECT, L.FLUCT_REFERENCE, 3, 5, 10, 1e-8, 1, 0, 1, 6, 3, 7,
                                                   None, None, None), L.FLAG_T)
    R.call(e, lambda: e.index_sample(1, 0, 1, 6, "sample", 3, 8), L.FLAG_T, [(1, 0)])


# ---- 5. dangx_plane_set_sample

def _plane_set(R, c, **kw):
    e = R.engine(c)

    def step(it, group, f, sa, sw):
        R.call(e, lambda: e.plane_set_sample(group, f, "sample", 11, sa, sw, 6, 11, **kw), f, sw)
    _loop(c, step)


@case
def plane_set_launch(R):
    """C3: the one launch (planeset_launch with solve = 1 and the sweep items, index sums in the ring entry)"""
    _plane_set(R, _case("C3"))


@case
def plane_set_launch_no_counts(R):
    """the same without counters: no read-back of the sixteen counters"""
    _plane_set(R, _case("C3"), want_counts=False)


@case
def plane_set_correct(R):
    """C3, DANGX_FLUCT_CORRECT: the one launch with SOLVE = 2"""
    _plane_set(R, _case("C3"), fluct_mode="correct")


@case
def plane_set_c5(R):
    """C5: the one launch over 20 bands, four sweeps, the dust pair in one item"""
    _plane_set(R, _case("C5"))


@case
def plane_set_fallback(R):
    """C2: lanes == 0, no global components -- dangx_amp_index_sample for the first sweep, then the sweeps one by one with the dust
    beta -> T through the pair"""
    _plane_set(R, _case("C2"))


@case
def plane_set_constant_start(R):
    """C3 from the prior: planeset_items refuses constant index maps on the first iteration (the fallback chain, its first sweep the
    two calls); the second iteration is the one launch"""
    _plane_set(R, _case("C3", start="prior"))


@case
def plane_set_cg(R):
    """C2 with the CG solver: can false, the fallback chain with the CG solve"""
    _plane_set(R, _case("C2"), solver="cg", i_max=10, converge=1e-6)


@case
def plane_set_template(R):
    """C3 + Q/U template: on Q+U gq.nt != 0 -- the sky form with one context (Schur solve, back-substitution deferred into the launch);
    on T gq.nuc != 0 -- dangx_amp_sample + dangx_plane_sweeps_sample"""
    _plane_set(R, _case("C3", _template))


@case
def plane_set_template_five_bands(R):
    """C2 + Q/U template: the same two routes where no plane-set kernel exists -- the full Schur solve, then the sweeps one by one"""
    _plane_set(R, _case("C2", _template))


@case
def plane_set_template_correct(R):
    """C3 + Q/U template, DANGX_FLUCT_CORRECT: the sky form does not defer"""
    _plane_set(R, _case("C3", _template), fluct_mode="correct")


@case
def plane_set_monopole(R):
    """C2 + monopole in the T group: the sky form on T; the textbook term is refused there"""
    c = _case("C2", _monopole)
    _plane_set(R, c)
    e = R.engines[-1]
    R.call(e, lambda: e.plane_set_sample(1, L.FLAG_T, "sample", 5, 7, [(1, 0, 9)], 3, 5, fluct_mode="correct"), L.FLAG_T, [(1, 0)])
    R.call(e, lambda: e.plane_set_sample(1, L.FLAG_T, "sample", 5, 7, [(1, 3, 9)], 3, 5), L.FLAG_T)      # sweep list out of range
    R.call(e, lambda: e.plane_set_sample(1, 3, "sample", 5, 7, [(1, 0, 9)], 3, 5), L.FLAG_T)             # a compound flag


# ---- 6. dangx_plane_sweeps_sample

def _plane_sweeps(R, c, **kw):
    e = R.engine(c)

    def step(it, group, f, sa, sw):
        R.call(e, lambda: e.amp_sample(group, f, "sample", 11, sa), f)
        R.call(e, lambda: e.plane_sweeps_sample(f, sw, 6, "sample", 11, **kw), f, sw)
        if it == ITERATIONS:   # a second list on the same planes: wb is false now
            R.call(e, lambda: e.plane_sweeps_sample(f, sw[:1], 6, "sample", 12, **kw), f, sw[:1])
    _loop(c, step)
    return e


@case
def plane_sweeps_launch(R):
    """C3: planeset_launch with solve = 0"""
    _plane_sweeps(R, _case("C3"))


@case
def plane_sweeps_one_by_one(R):
    """C2: the sweeps one by one, the dust pair through dangx_index_sample_pair"""
    _plane_sweeps(R, _case("C2"))


@case
def plane_sweeps_no_counts(R):
    """C2 and no accepted array: the loop passes NULL on"""
    _plane_sweeps(R, _case("C2"), want_counts=False)


@case
def plane_sweeps_rejected(R):
    """C3: a compound flag and a list entry out of range are rejected after sync_model; a list over two groups goes one by one"""
    c = _case("C3")
    e = R.engine(c)
    R.call(e, lambda: e.plane_sweeps_sample(3, [(1, 0, 9)], 3, "sample", 5), L.FLAG_T)
    R.call(e, lambda: e.plane_sweeps_sample(L.FLAG_T, [(1, 4, 9)], 3, "sample", 5), L.FLAG_T)
    R.call(e, lambda: e.plane_sweeps_sample(L.FLAG_QU, [(5, 0, 9), (2, 0, 10)], 3, "sample", 5), L.FLAG_QU, [(5, 0), (2, 0)])


# ---- 7. the sky forms with two contexts on one device (unequal shards)

def _sky_amp(R, c, **kw):
    engs = R.shards(c)

    def step(it, group, f, sa, sw):
        R.call(engs, lambda: da.sky_amp_sample(engs, group, f, "sample", 11, sa, **kw), f)
    _loop(c, step)
    return engs


@case
def sky_amp_diffuse(R):
    """C3, diffuse groups: dangx_amp_sample per context with the counters zeroed before and read after every launch; one context alone
    delegates to the single form before any validation"""
    c = _case("C3")
    engs = _sky_amp(R, c)
    R.call(engs[:1], lambda: da.sky_amp_sample(engs[:1], 1, L.FLAG_T, "sample", 11, 3), L.FLAG_T)


@case
def sky_amp_template(R):
    """C2 + Q/U template: the shared Schur rows on Q+U; then the refusals of the sky form (the CG solver, a bad ml_mode)"""
    c = _case("C2", _template)
    engs = _sky_amp(R, c)
    R.call(engs, lambda: da.sky_amp_sample(engs, 2, L.FLAG_QU, "sample", 11, 3, solver="cg"), L.FLAG_QU)
    R.call(engs, lambda: da.sky_amp_sample(engs, 1, L.FLAG_T, "sample", 11, 3, solver="cg"), L.FLAG_T)


@case
def sky_amp_template_correct(R):
    """C2 + Q/U template, DANGX_FLUCT_CORRECT over two contexts"""
    _sky_amp(R, _case("C2", _template), fluct_mode="correct")


@case
def sky_amp_monopole_refused(R):
    """C2 + monopole: the textbook term refused by the sky form before any context is touched"""
    c = _case("C2", _monopole)
    engs = R.shards(c)
    R.call(engs, lambda: da.sky_amp_sample(engs, 1, L.FLAG_T, "sample", 11, 3, fluct_mode="correct"), L.FLAG_T)
    R.call(engs, lambda: da.sky_amp_sample(engs, 1, L.FLAG_T, "sample", 11, 3), L.FLAG_T)


def _sky_plane_set(R, c, **kw):
    engs = R.shards(c)

    def step(it, group, f, sa, sw):
        R.call(engs, lambda: da.sky_plane_set_sample(engs, group, f, "sample", 11, sa, sw, 6, 11, **kw), f, sw)
    _loop(c, step)
    return engs


@case
def sky_plane_set_diffuse(R):
    """C3, diffuse groups: dangx_plane_set_sample on every context, the counts added up"""
    _sky_plane_set(R, _case("C3"))


@case
def sky_plane_set_template(R):
    """C3 + Q/U template: pass 1 and the host solve, then one planeset_launch per context (the deferred back-substitution)"""
    _sky_plane_set(R, _case("C3", _template))


@case
def sky_plane_set_template_no_counts(R):
    """the same without counters"""
    _sky_plane_set(R, _case("C3", _template), want_counts=False)


@case
def sky_plane_set_template_correct(R):
    """C3 + Q/U template, DANGX_FLUCT_CORRECT: not deferred -- the full Schur solve, then dangx_plane_sweeps_sample per context"""
    _sky_plane_set(R, _case("C3", _template), fluct_mode="correct")


@case
def sky_plane_set_refusals(R):
    """C3 + Q/U template: the CG solver over two contexts, a list entry out of range (bubbled from the context that found it)"""
    c = _case("C3", _template)
    engs = R.shards(c)
    R.call(engs, lambda: da.sky_plane_set_sample(engs, 2, L.FLAG_QU, "sample", 11, 3, [(5, 0, 9)], 3, 11, solver="cg"), L.FLAG_QU)
    R.call(engs, lambda: da.sky_plane_set_sample(engs, 2, L.FLAG_QU, "sample", 11, 3, [(5, 3, 9)], 3, 11), L.FLAG_QU)
    R.call(engs, lambda: da.sky_plane_set_sample(engs, 2, L.FLAG_QU, "sample", 11, 3, [(5, 0, 9)], 3, 11), L.FLAG_QU, [(5, 0)])


# ---- 9. dangx_set_calibration between two sweeps: invalidate_chi drops the ring's entries

@case
def calibration_between_sweeps(R):
    """C3: two sweeps with a calibration change in between and nothing asked for -- the first sweep's ring entry is dropped, its
    'before' value with it; then the same around a plane-set launch, whose entry carries index sums"""
    c = _case("C3")
    e = R.engine(c)
    nb = c[4]["nbands"]
    gain, offset = [1.0 + 0.01 * ((j % 3) - 1) for j in range(nb)], [0.5 * ((j % 4) - 1.5) for j in range(nb)]
    R.call(e, lambda: e.amp_sample(1, L.FLAG_T, "sample", 11, 3), observe=False)
    R.call(e, lambda: e.index_sample(1, 0, 1, 6, "sample", 17, 4), observe=False)
    e.set_calibration(gain, offset)
    R.call(e, lambda: e.index_sample(2, 0, 1, 6, "sample", 17, 5), L.FLAG_T, [(1, 0), (2, 0)])
    sw = _sweeps(c[3], 1, L.FLAG_T, 2)
    R.call(e, lambda: e.plane_set_sample(1, L.FLAG_T, "sample", 11, 6, sw, 6, 11), observe=False)
    e.set_calibration(np.ones(nb), np.zeros(nb))
    R.observe([e], L.FLAG_T, sw)
    R.call(e, lambda: e.plane_sweeps_sample(L.FLAG_T, sw, 6, "sample", 11), L.FLAG_T, sw)


def run_case(name):
    """{array name: array} of what the case's entry calls returned and left behind"""
    R = Recorder()
    CASES[name](R)
    return R.arrays()


def record(path):
    """writes the fixture from the build that is loaded (run once, on the parent commit)"""
    arrays = {}
    for name in CASES:
        for k, v in run_case(name).items():
            arrays[name + "/" + k] = v
    np.savez_compressed(path, **arrays)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_has_every_case(golden):
    assert sorted({k.split("/", 1)[0] for k in golden}) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_entry_route_bits_are_the_parents(built, golden, name):
    out = run_case(name)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(name + "/"))
    assert keys == sorted(out), (keys, sorted(out))
    for k in keys:
        want, got = golden[name + "/" + k], out[k]
        assert want.shape == got.shape and want.dtype == got.dtype, (name, k, want.shape, got.shape)
        ne = int(np.count_nonzero(want.view(np.int64) != got.view(np.int64)))
        print("%s/%s: %d of %d values differ in their bits" % (name, k, ne, want.size))
        assert ne == 0, (name, k, ne)
