"""bench.py's contract with the driver (GPU): one JSON line with the required keys, for the plain launch, for the plain
launch with --gpus N (bench.py spawns its own N ranks) and for the one-process-per-GPU launch under a launcher
(`python -m torch.distributed.run ... bench.py --gpus N`).  Two ranks share GPU 0 here (--oversubscribe), which exercises
the rendezvous, the barrier / max-over-ranks timing and the whole-job aggregation."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _line(cmd):
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    lines = [ln for ln in out if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]          # exactly ONE JSON line (rank 0)
    assert len(out) == 1, out[:5]                               # ... and nothing else on stdout (the rendezvous' chatter goes to stderr)
    return json.loads(lines[0])


def _check(d, n_gpus, steps, warmup):
    for k in KEYS:
        assert k in d, k
    assert d["n_gpus"] == n_gpus and d["steps"] == steps and d["warmup"] == warmup
    assert d["unit"] == "Mevents/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert d["value_definition"] == "hbm_resident"               # which definition `value` uses, machine readable
    assert "frac_rocprof" in r and "frac_rocprof" in r["stencil_kernel"] and "frac_rocprof" in r["warp_scatter_kernel"]
    hb = d["config"]["host_budget"]                                # ranks x polling cores against the cores the job may use
    assert hb["ranks"] == n_gpus and hb["host_cores_available"] >= 1 and hb["polling_cores_needed"] > 0
    # value = whole-job events / time: consistent with ms_per_step and the per-step slice count
    ev_per_step = d["config"]["events_per_slice"] * d["config"]["slices_per_step_per_gpu"] * n_gpus
    assert abs(d["value"] - ev_per_step / d["ms_per_step"] / 1e3) < 1e-6 * d["value"]


@pytest.mark.gpu
def test_bench_single_process():
    d = _line([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--cpu-iters", "8", "--cpu-cores", "2",
               "--front-end-slices", "8"])
    _check(d, 1, 3, 1)
    fe = d["front_end"]                  # the command-line front end: file -> last model
    assert "error" not in fe, fe
    assert fe["file_to_last_model"]["slices"] == 8 and fe["steady_state_warm"]["mevents_per_s"] > 100
    assert fe["with_flow_output"]["output_s"] > 0
    assert fe["reference_ring"]["mevents_per_s"] > 5 and fe["reference_ring"]["slices"] > 100   # the reference's compiled-in ring
    assert 0.2 < d["roofline"]["headline_regime"]["frac"] < 1
    # the fractions re-derived from the committed rocprofv3 summary of the same solo run agree with the live hipEvent ones
    for kk in ("stencil_kernel", "warp_scatter_kernel"):
        ko = d["roofline"][kk]
        if ko["rocprof"] is not None:   # (absent only in a checkout without profiles/r6_solo_tail_kernel_stats.csv)
            assert ko["rocprof"]["source"].startswith("profiles/r6_") and 0.7 < ko["frac_rocprof"] / ko["frac"] < 1.3, ko
    assert d["value_host_to_host"] == d["regimes"]["host_to_host"]["cold"]["mevents_per_s"]
    assert d["targets"]["met_by"]["mevents_per_s"] > 1000          # north_star: >= 1 Gevents/s (warm STM, H2D included)
    assert 0 < d["roofline"]["iteration_frac"] < 1
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] == 1 and 0 < c["value"] < d["value"]
    assert set(d["regimes"]) >= {"warm_stm", "capped_max_iter_10", "one_context", "host_to_host"}
    # the top level is the dominant kernel's (the longer average launch of the two loop kernels); both are listed
    r = d["roofline"]
    k1, k3 = r["warp_scatter_kernel"], r["stencil_kernel"]
    dom = r[r["dominant"]]
    assert dom["avg_launch_us"] == max(k1["avg_launch_us"], k3["avg_launch_us"])
    assert r["frac"] == dom["frac"] > 0.1 and r["traffic"] == dom["traffic"] and r["kernel"] == dom["kernel"]
    assert k1["frac"] > 0.2 and k1["traffic"] > k1["algorithmic_bytes_per_launch"] and "regime" in r
    h = d["regimes"]["host_to_host"]     # SURVEY 8(d) as written: H2D included
    for k in ("cold", "warm_stm", "capped_max_iter_10"):
        assert 0 < h[k]["mevents_per_s"] and 0 < h["one_context"][k]["mevents_per_s"]


@pytest.mark.gpu
def test_bench_two_ranks_torchrun():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    d = _line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--oversubscribe", "--steps", "2", "--warmup", "1"])
    _check(d, 2, 2, 1)
    assert d["cpu_baseline"] is None          # timed on rank 0 at N = 1 only


@pytest.mark.gpu
def test_bench_config5_farm_two_ranks():
    """BASELINE config 5 through the farm driver, in small: 2 ranks (both on GPU 0), 4 slices at 1280x720."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    d = _line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--oversubscribe", "--config", "5", "--farm-slices", "4",
               "--events", "150000", "--concurrent", "2"])
    assert d["n_gpus"] == 2 and d["unit"] == "Mevents/s" and d["value"] > 0
    c = d["config"]
    assert c["slices"] == 4 and c["slices_failed"] == 0 and "1280x720" in c["workload"] and c["iterations_per_slice_mean"] > 10


@pytest.mark.gpu
def test_bench_gpus_flag_spawns_its_own_ranks():
    """The driver's command form, `python3 bench.py --gpus N ...` with no launcher around it: N ranks, one JSON line."""
    d = _line([sys.executable, "bench.py", "--gpus", "2", "--oversubscribe", "--steps", "2", "--warmup", "1"])
    _check(d, 2, 2, 1)
    assert "2 GPU(s)" in d["config"]["parallelism"] and d["cpu_baseline"] is None


@pytest.mark.gpu
def test_bench_config5_gpus_flag_spawns_its_own_ranks():
    d = _line([sys.executable, "bench.py", "--gpus", "2", "--oversubscribe", "--config", "5", "--farm-slices", "4",
               "--events", "150000", "--concurrent", "2"])
    assert d["n_gpus"] == 2 and d["config"]["slices"] == 4 and d["config"]["slices_failed"] == 0


@pytest.mark.gpu
def test_bench_four_ranks_on_one_gpu():
    """`bench.py --gpus N` as the driver calls it with more ranks than the two tests above: four ranks, all on GPU 0
    (--oversubscribe), one slice context per rank, two steps of config 2 -- one JSON line, n_gpus 4, the whole-job
    aggregate, the host-core budget in it.  (Four ranks and this process make five processes on the device, within the six
    a shared GPU node allows; world size 8 itself is covered without a device by test_farm_gloo.py.)"""
    d = _line([sys.executable, "bench.py", "--gpus", "4", "--oversubscribe", "--concurrent", "1", "--steps", "2", "--warmup", "1",
               "--slices", "2"])
    _check(d, 4, 2, 1)
    assert "4 GPU(s)" in d["config"]["parallelism"] and d["cpu_baseline"] is None
    assert d["config"]["host_budget"]["ranks"] == 4
    assert abs(d["config"]["events_per_slice"] - 1e6) < 5e4 and d["config"]["iterations_per_slice"] > 400


@pytest.mark.gpu
def test_bench_config5_four_ranks_on_one_gpu():
    """BASELINE config 5's job shape with several ranks: 4 ranks (all on GPU 0) x 1 slice context claim 16 full-size
    1280x720 slices from ONE queue, the slices exchanged through the shared directory; one JSON line with the per-rank
    records."""
    d = _line([sys.executable, "bench.py", "--gpus", "4", "--oversubscribe", "--config", "5", "--farm-slices", "16", "--concurrent", "1"])
    assert d["n_gpus"] == 4 and d["unit"] == "Mevents/s" and d["value"] > 0 and d["value_definition"] == "host_to_host"
    c = d["config"]
    assert c["slices"] == 16 and c["slices_failed"] == 0 and "1280x720" in c["workload"]
    assert len(c["ranks"]["busy_s"]) == 4 and sum(c["ranks"]["slices"]) == 16 and min(c["ranks"]["slices"]) >= 1
    assert sorted(set(c["per_slice"]["rank"])) == list(range(4)) and len(c["per_slice"]["iterations"]) == 16
    assert c["host_budget"]["ranks"] == 4


@pytest.mark.gpu
def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs: the last timed step's model, run info and sampled per-event flow of every slice context, float64,
    under 64 MB, and the same bits from a second run with the same arguments."""
    import numpy as np
    cmd = [sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--concurrent", "2", "--no-cpu-baseline", "--no-front-end",
           "--dump-outputs"]
    runs = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        d = _line(cmd + [str(out)])
        assert d["steps"] == 2
        files = sorted(p.name for p in out.iterdir())
        assert files == ["model.npy", "run_info.npy", "u.npy", "uv_index.npy", "v.npy"], files
        assert sum(p.stat().st_size for p in out.iterdir()) < 64 << 20
        runs.append({f[:-4]: np.load(str(out / f)) for f in files})
    a, b = runs
    for name, arr in a.items():
        assert arr.dtype == np.float64 and np.all(np.isfinite(arr)), name
        assert arr.tobytes() == b[name].tobytes(), name
    assert a["model"].shape[0] == a["run_info"].shape[0] == a["u"].shape[0] == 2
    assert np.all(a["run_info"][:, 0] == 0) and np.all(a["run_info"][:, 1] > 400)       # rc, iterations of each lane's slice
    assert a["u"].shape == a["v"].shape == a["uv_index"].shape and a["u"].shape[1] > 1000
    assert np.any(a["u"] != 0) and np.any(a["v"] != 0)


def test_bench_dump_outputs_files(tmp_path):
    """(CPU) The --dump-outputs writer: float64 arrays, one row per slice context, a seeded sample of the per-event flow
    that is the same for the same inputs."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    models = [{k: float(i + j) for j, k in enumerate(bench.MODEL_FIELDS)} for i in range(2)]
    runs = [{k: float(i) for k in bench.RUN_FIELDS} for i in range(2)]
    rng = np.random.default_rng(0)
    flows = [(rng.standard_normal(5000), rng.standard_normal(5000)) for _ in range(2)]
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), "", models, runs, flows=flows, sample_per_lane=300)
    for name in ("model", "run_info", "uv_index", "u", "v"):
        x, y = np.load(str(tmp_path / "0" / (name + ".npy"))), np.load(str(tmp_path / "1" / (name + ".npy")))
        assert x.dtype == np.float64 and x.tobytes() == y.tobytes(), name
    idx = np.load(str(tmp_path / "0" / "uv_index.npy")).astype(np.int64)
    assert idx.shape == (2, 300) and np.all(np.diff(idx, axis=1) > 0)
    assert np.array_equal(np.load(str(tmp_path / "0" / "u.npy"))[1], flows[1][0][idx[1]])
    assert np.load(str(tmp_path / "0" / "model.npy")).shape == (2, len(bench.MODEL_FIELDS))
    bench.dump_outputs(str(tmp_path / "all"), "", models, runs, flows=flows, sample_per_lane=1 << 20)   # sample > slice: every event
    assert np.array_equal(np.load(str(tmp_path / "all" / "v.npy")), np.array([v for _, v in flows]))


def test_bench_steps_must_be_positive():
    """(CPU) --steps is the number of timed steps: zero is refused, not a division by zero after the fact."""
    r = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode != 0 and b"--steps must be" in r.stderr and b"{" not in r.stdout


def test_bench_refuses_more_ranks_than_host_cores():
    """(CPU) The host-core budget: ranks x polling cores against the cores the job may use -- over budget is an error that says
    so (before any device is touched), not a run that times the host."""
    env = dict(os.environ, WORLD_SIZE="4096", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="1")
    r = subprocess.run([sys.executable, "-c", "import bench, sys; sys.argv = ['bench.py', '--gpus', '4096']; "
                        "import types; bench_main = bench.main\n"
                        "import torch.distributed as dist\n"
                        "dist.init_process_group = lambda **k: None; dist.barrier = lambda: None\n"
                        "from better_flow_amd import accel; accel.device_count = lambda: 4096; accel.bind_thread_to_device_numa = lambda d: -1\n"
                        "bench_main()"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b"host cores for polling" in r.stderr and b"OVER BUDGET" in r.stderr, r.stderr[-2000:]
    assert b"{" not in r.stdout


@pytest.mark.gpu
def test_bench_more_ranks_than_devices_fails_loudly():
    from better_flow_amd import accel
    n = accel.device_count() + 1
    r = subprocess.run([sys.executable, "bench.py", "--gpus", str(n), "--steps", "1", "--warmup", "0"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode != 0 and b"HIP device(s) visible" in r.stderr and b"{" not in r.stdout


def test_bench_world_size_must_match_gpus_flag():
    """(CPU) Under a launcher WORLD_SIZE must equal --gpus: a mismatch is an error, not a silently smaller job."""
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b"must agree" in r.stderr


def test_bench_gpus_flag_spawns_and_fails_without_devices():
    """(CPU) `python bench.py --gpus 2` with no launcher spawns two ranks; on a machine without a HIP device both fail
    loudly (no CPU fallback) and the parent relays the failure instead of printing a line."""
    from better_flow_amd import accel
    try:
        have = accel.device_count() > 0
    except Exception:   # noqa: BLE001
        have = False
    if have:
        pytest.skip("a HIP device is present: the GPU tests cover the spawn path")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and r.stderr.count(b"needs a HIP device") == 2 and b"{" not in r.stdout
