"""bench.py --gpus N without a launcher starts its own N ranks, and never reports a line for fewer ranks than asked."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    return env


def test_more_gpus_than_visible_is_an_error_not_a_one_gpu_line():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "64", "--steps", "1", "--warmup", "0"], env=_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0
    assert "--gpus 64" in r.stderr and "visible" in r.stderr
    assert r.stdout.strip() == ""            # no JSON line at all


def test_world_size_must_match_gpus():
    env = dict(_env(), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "1", "--warmup", "0"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE (1) != --gpus (8)" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.gpu
def test_self_launched_ranks_report_their_count(built):
    """Two self-spawned ranks (gloo process group, both on cuda:0 -- a rehearsal of the N-rank path on a one-GPU box;
    on a node with N GPUs the same launcher runs N RCCL ranks): the line says n_gpus = 2 and the all-reduced rank
    count agrees; chi^2 equals the one-rank run's (the sky is the same, sharded)."""
    def run(*extra):
        r = subprocess.run([sys.executable, BENCH, "--config", "C2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"] + list(extra),
                           env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    two = run("--gpus", "2", "--backend", "gloo")
    one = run("--gpus", "1")
    assert two["n_gpus"] == 2 and two["ranks_seen"] == 2 and two["backend"] == "gloo"
    assert one["n_gpus"] == 1 and one["ranks_seen"] == 1
    for k in ("chisq_after_amp", "chisq_after_index"):
        assert abs(two["config"][k] - one["config"][k]) <= 1e-12 * abs(one["config"][k])


@pytest.mark.gpu
def test_five_rank_rehearsal_of_the_sharded_path_on_one_gpu(built):
    """The N-rank data path with what one GPU allows (no 8-GPU node has been available to any round; a box admits six
    processes on its card, and the test runner may be one of them): bench.py launches 5 gloo ranks on cuda:0 over the C3 model at Nside 256, each on its RING shard (boundaries by
    unmasked pixel count) with the two-stream form the 8-rank runs take (T chain and Q+U chain on separate HIP streams).  All ranks are seen by the
    all-reduce, and chi^2 equals the one-rank value -- the sky does not depend on how it is sharded.  RCCL itself stays
    unexercised."""
    def run(*extra):
        r = subprocess.run([sys.executable, BENCH, "--config", "C3", "--nside", "256", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                            "--no-fortran-seam"] + list(extra), env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    five = run("--gpus", "5", "--backend", "gloo", "--streams", "2", "--gather")
    one = run("--gpus", "1", "--gather")
    assert five["n_gpus"] == 5 and five["ranks_seen"] == 5 and five["backend"] == "gloo"
    # north_star's "gather for map output" with the run's (work-balanced, unequal) shard boundaries: the maps reassembled on rank 0
    # are the one-rank maps bit for bit
    assert five["gather"]["bounds"] == "work-balanced" and five["gather"]["npix"] == one["gather"]["npix"] == 12 * 256 * 256
    assert five["gather"]["checksum"] == one["gather"]["checksum"], (five["gather"], one["gather"])
    assert "5 rank(s) (contiguous RING ranges of equal unmasked-pixel count), 2 stream(s) per rank" in five["config"]["workload"]
    for k in ("chisq_after_amp", "chisq_after_index"):
        assert abs(five["config"][k] - one["config"][k]) <= 1e-12 * abs(one["config"][k]), k
    # the old split by pixel count: the same sky
    eq = run("--gpus", "2", "--backend", "gloo", "--equal-shards")
    assert "equal pixel count" in eq["config"]["workload"]
    for k in ("chisq_after_amp", "chisq_after_index"):
        assert abs(eq["config"][k] - one["config"][k]) <= 1e-12 * abs(one["config"][k]), k


@pytest.mark.gpu
def test_bench_line_carries_the_template_model_figure(built):
    """The --full line (C3 at full size) with its secondary figure: the same workload with a Q/U template fitted in the Q+U group,
    whole iterations through gibbs_iteration -- the injected amplitudes come back, the Schur solve needed no refinement, and the
    headline keys are what they were."""
    r = subprocess.run([sys.executable, BENCH, "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-fortran-seam"], env=_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] and d["n_gpus"] == 1 and d["roofline"]["frac"] > 0 and "C3" in d["config"]["workload"]
    t = d["template_model"]
    assert "error" not in t, t
    assert t["it_per_s"] > 0 and t["refinements"] == 0 and t["schur_residual_bound"] <= 1e-12
    for got, want in zip(t["template_amplitudes"], (2.0, -1.5, 0.7)):
        assert abs(got - want) < 0.01, t
    m = d["index_modes"]
    assert "error" not in m and m["fullsky"]["it_per_s"] > 0 and m["coarse"]["it_per_s"] > 0, m
    assert np.isfinite(m["fullsky"]["chisq"]) and np.isfinite(m["coarse"]["chisq"])


def test_steps_must_be_at_least_one():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0", "--warmup", "0"], env=_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr
    assert r.stdout.strip() == ""


def _load_bench(monkeypatch):
    import importlib.util
    monkeypatch.setenv("OMP_WAIT_POLICY", os.environ.get("OMP_WAIT_POLICY", "PASSIVE"))   # bench.py sets a default
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_every_map_or_one_seeded_sample_of_it(tmp_path, monkeypatch):
    """--dump-outputs: every component's amplitude and index maps and the chi^2 pair, float64; all pixels when they fit the budget,
    else the same seeded sample of pixels on every call, within the budget."""
    bench = _load_bench(monkeypatch)
    from dang_amd import synth
    dpar, ddata, bands, comps, meta = synth.make_sky("C2", nside=8, as_numpy=False)
    n = meta["npix_global"]
    names = ["chisq"] + ["amplitude_%02d_%s" % (l, c.label) for l, c in enumerate(comps)] + \
            ["indices_%02d_%s" % (l, c.label) for l, c in enumerate(comps) if c.nindices]
    nbytes = bench.dump_outputs(str(tmp_path / "all"), comps, [1.5, 1.25], 0, n, 0, 1, "gloo", "cpu")
    assert sorted(os.listdir(tmp_path / "all")) == sorted(f + ".npy" for f in names)
    assert np.array_equal(np.load(tmp_path / "all" / "chisq.npy"), [1.5, 1.25])
    for l, c in enumerate(comps):
        a = np.load(tmp_path / "all" / ("amplitude_%02d_%s.npy" % (l, c.label)))
        assert a.dtype == np.float64 and np.array_equal(a, c.amplitude.numpy())
        if c.nindices:
            assert np.array_equal(np.load(tmp_path / "all" / ("indices_%02d_%s.npy" % (l, c.label))), c.indices.numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", nbytes // 4)
    for d in ("s1", "s2"):
        assert bench.dump_outputs(str(tmp_path / d), comps, [1.5, 1.25], 0, n, 0, 1, "gloo", "cpu") <= nbytes // 4 + 16
    nsel = np.load(tmp_path / "s1" / "amplitude_00_cmb.npy").shape[-1]
    sel = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, size=nsel, replace=False))
    assert 0 < nsel < n
    for l, c in enumerate(comps):
        f = "amplitude_%02d_%s.npy" % (l, c.label)
        a1, a2 = np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)
        assert np.array_equal(a1, a2) and np.array_equal(a1, c.amplitude.numpy()[:, sel])


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_two_runs_dump_the_same_outputs(built, tmp_path):
    """A plain run times exactly --steps steps, reports ms_per_step and runs none of the --full legs; --dump-outputs writes the last
    timed step's maps (a seeded sample: C2's maps exceed the budget) and the line's chi^2, and two runs write the same arrays."""
    def run(d):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "C2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                           env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    one, two = run(tmp_path / "a"), run(tmp_path / "b")
    for d in (one, two):
        assert d["metric"] == "gibbs_iterations_per_sec" and d["unit"] == "it/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-9 * 1e3
        assert not set(d) & {"cpu_baseline", "fortran_seam", "template_model", "index_modes"}, sorted(d)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "chisq.npy" in files and "amplitude_01_synch.npy" in files
    total = 0
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.array_equal(x, y, equal_nan=True), f
        total += x.nbytes
    assert 0 < total <= 64e6
    assert np.array_equal(np.load(tmp_path / "a" / "chisq.npy"), [one["config"]["chisq_after_amp"], one["config"]["chisq_after_index"]])
    assert np.load(tmp_path / "a" / "amplitude_01_synch.npy").shape[-1] < 12 * 256 * 256
