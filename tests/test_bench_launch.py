"""bench.py's launch path on CPU (SURVEY.md §8d / north_star "1/2/4/8-GPU scaling reported"): `python bench.py
--gpus N` must really start N ranks — round 2's bench parsed --gpus and ran one GPU.  --rendezvous-only
stops after the ranks have met over gloo (no GPU, no build)."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "HNY_BENCH_SELF_LAUNCHED"):
        env.pop(k, None)
    return env


def _json_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_gpus_2_self_launches_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rendezvous-only"], capture_output=True, text=True,
                       env=_clean_env(), timeout=300)
    assert r.returncode == 0, r.stderr
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["ranks_seen"] == 2 and j["ranks"] == [0, 1] and j["launcher"] == "self"


def test_gpus_3_self_launches_three_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--rendezvous-only"], capture_output=True, text=True,
                       env=_clean_env(), timeout=300)
    assert r.returncode == 0, r.stderr
    j = _json_line(r.stdout)
    assert j["ranks_seen"] == 3 and j["ranks"] == [0, 1, 2]


def test_under_a_launcher_every_process_is_one_rank():
    """the form the driver uses for N > 1: torch.distributed.run starts the ranks, bench.py must not fork again"""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2",
                        "--rendezvous-only"], capture_output=True, text=True, env=_clean_env(), timeout=600)
    assert r.returncode == 0, r.stderr
    j = _json_line(r.stdout)
    assert j["ranks_seen"] == 2 and j["launcher"] == "torchrun"


def test_launcher_and_flag_must_agree():
    env = dict(_clean_env(), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rendezvous-only"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0 and "disagree" in r.stderr


def test_a_failing_rank_fails_the_run():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("GPU present: the ranks would build")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, env=_clean_env(),
                       timeout=300)
    assert r.returncode != 0 and "exited with code" in r.stderr and not r.stdout.strip()


# ---- the same launch modes with real builds, on the one GPU of the test box (ranks share it) ----
import pytest  # noqa: E402

SMALL = ["--items", "30000", "--dim", "64", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-recall", "--queries", "0"]


@pytest.mark.gpu
def test_gpus_2_native_builds_on_two_replicas_through_the_copy_shim():
    """`bench.py --gpus 2 --native`: the resident multi-builder behind the C ABI (hny_multi.cpp) with two replicas on
    GPU 0, the all-gathers replaced by the copy shim, every replica's export compared inside the library"""
    env = dict(_clean_env(), HNY_MGPU_SHIM="1", HNY_MGPU_VERIFY="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--native"] + SMALL, capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["ranks_seen"] == 2 and j["launcher"] == "native" and j["replicas_identical"] is True
    assert j["n_collectives"] > 0 and j["value"] > 0


@pytest.mark.gpu
def test_gpus_2_self_launched_ranks_build_over_gloo_on_one_gpu():
    """`bench.py --gpus 2 --backend gloo`: two self-launched processes (the torchrun harness, multigpu.py), exchange
    staged through the host; rank 0 compares the replicas' checksums"""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--backend", "gloo"] + SMALL, capture_output=True,
                       text=True, env=_clean_env(), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _json_line(r.stdout)
    assert j["ranks_seen"] == 2 and j["launcher"] == "self" and j["replicas_identical"] is True and j["n_collectives"] > 0


# ---- --full / --dump-outputs ----
def test_extras_without_full_are_refused():
    """a plain run measures the headline figure only: asking it for a --full measurement fails instead of
    silently leaving it out"""
    for extra in (["--alt-data", "overlap"], ["--cpu-full"]):
        r = subprocess.run([sys.executable, BENCH, "--rendezvous-only"] + extra, capture_output=True, text=True,
                           env=_clean_env(), timeout=300)
        assert r.returncode != 0 and "--full" in r.stderr


def _fake_graph(nrec, M0, seed=1):
    import types
    import numpy as np
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, M0 + 1, nrec)
    offsets = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    return types.SimpleNamespace(offsets=offsets, nbrs=rng.integers(0, nrec, int(offsets[-1])).astype(np.uint32),
                                 rec_item=rng.permutation(nrec).astype(np.uint32),
                                 rec_layer=rng.integers(0, 3, nrec).astype(np.uint8),
                                 entry_points=np.array([5, 7], np.uint32), max_level=2)


def _load_dir(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("nrec,M0", [(3000, 32), (1_100_000, 32), (200_000, 1024)])
def test_dump_outputs_is_bounded_exact_and_fixed(tmp_path, nrec, M0):
    """whole graph when it fits 64 MB, else a seeded sample of records whose lists are exact; float64 only"""
    import numpy as np
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    g = _fake_graph(nrec, M0)
    bench.dump_outputs(str(tmp_path / "a"), g, M0)
    bench.dump_outputs(str(tmp_path / "b"), g, M0)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    off = g.offsets.astype(np.int64)
    assert a["graph_counts"].tolist() == [nrec, off[-1]] and a["graph_entry_points"].tolist() == [5, 7]
    if "graph_nbrs" in a:
        assert np.array_equal(a["graph_nbrs"], g.nbrs) and np.array_equal(a["graph_offsets"], off)
        assert np.array_equal(a["graph_rec_item"], g.rec_item)
    else:
        idx = a["graph_sample_records"].astype(np.int64)
        assert len(idx) > 1000 and np.all(np.diff(idx) > 0)
        assert np.array_equal(a["graph_sample_rec_item"], g.rec_item[idx])
        for j in range(0, len(idx), 997):
            r = idx[j]
            lst = a["graph_sample_nbrs"][j]
            n = off[r + 1] - off[r]
            assert np.array_equal(lst[:n], g.nbrs[off[r]:off[r + 1]]) and np.all(lst[n:] == -1)


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_same_graph_twice(tmp_path):
    """`--steps K` timed steps and `ms_per_step`; no --full measurement in a plain line; two runs with the same
    arguments export the same graph"""
    import numpy as np
    args = ["--items", "30000", "--dim", "64", "--steps", "2", "--warmup", "1"]
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH] + args + ["--dump-outputs", str(tmp_path / d)], capture_output=True,
                           text=True, env=_clean_env(), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(_json_line(r.stdout))
    j = lines[0]
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "vectors/s"
    assert abs(j["value"] - 30000 / (j["ms_per_step"] / 1e3)) <= 0.01 * j["value"]
    assert not {"recall_at_10", "search", "cpu_baseline", "value_alt"} & set(j)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert "graph_nbrs" in a and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["graph_counts"][0] >= 30000 and a["graph_counts"][1] == len(a["graph_nbrs"])


@pytest.mark.gpu
def test_full_run_adds_recall_and_cpu_baseline():
    r = subprocess.run([sys.executable, BENCH, "--items", "30000", "--dim", "64", "--steps", "1", "--warmup", "0",
                        "--queries", "200", "--cpu-sample", "5000", "--full"], capture_output=True, text=True,
                       env=_clean_env(), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _json_line(r.stdout)
    assert 0.5 < j["recall_at_10"] <= 1.0 and j["search"]["queries"] == 200
    assert j["cpu_baseline"]["value"] > 0 and j["recall_parity_on_sample"]["n"] == 5000
