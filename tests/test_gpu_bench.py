"""bench.py's measured paths on a small model (GPU): the transfer-inclusive step (extra.h2d,
bench.H2DStep: inputs from pinned host memory, packed results back to pinned host memory) must
produce exactly the resident step's results, and the live stage timing must bracket every stage
of the step it measures."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _small_step():
    import bench
    a = bench.parse(["--model", "llama-2-7b", "--layers", "2", "--hidden", "512", "--inter", "768",
                     "--tokens", "2048", "--no-cpu-baseline"])
    bench._load_runtime(False)
    bench.resolve(a)
    return bench, bench.ModelStep(a, 0, 1, torch.device("cuda", 0), torch.float16)


def test_h2d_step_equals_resident_step():
    bench, ms = _small_step()
    want = ms.step()  # {unit.linear: {T2, alpha, mu, perm, shape}} on the device
    h = bench.H2DStep(ms)
    manifest = h.step()
    got = bench.sharding._unflatten(manifest, h.host_res[:h.d2h_bytes])
    assert sorted(got) == sorted(want) and len(got) == 14
    for k, r in want.items():
        for f in ("T2", "alpha", "mu", "perm"):
            assert torch.equal(got[k][f], r[f].cpu()), (k, f)
    assert h.h2d_bytes > 0 and got[next(iter(got))]["T2"].device.type == "cpu"


def test_stage_busy_brackets_every_stage():
    bench, ms = _small_step()
    ms.step()
    busy = ms.stage_busy()
    for k in ("gram", "inverse", "ssr", "atq", "ef", "setup", "out"):
        assert busy[k] > 0, (k, busy)
    assert busy["records"] > 0
    # one lane: the busy times of the tail phase fit inside its wall
    tails = sum(busy[k] for k in ("setup", "ssr", "atq", "ef", "out"))
    assert tails <= busy["phase_wall_ms"]["tails"] * 1.02 + 0.5
    assert len(ms.gf.pipe.lanes) == 3  # restored after the one-lane measurement


def test_shards_union_equals_whole_step():
    """bench --shard: every rank's LPT shard of a 2-rank step run alone on this GPU (shard_only,
    no gather) gives, linear for linear, exactly the one-GPU step's results, and each non-root
    shard reports the bytes its gather would send."""
    import bench
    a = bench.parse(["--model", "llama-2-7b", "--layers", "2", "--hidden", "512", "--inter", "768",
                     "--tokens", "2048", "--no-cpu-baseline"])
    bench._load_runtime(False)
    bench.resolve(a)
    dev = torch.device("cuda", 0)
    want = bench.ModelStep(a, 0, 1, dev, torch.float16).step()
    got = {}
    for r in range(2):
        ms = bench.ModelStep(a, r, 2, dev, torch.float16, shard_only=True)
        res = ms.step()
        assert (ms.gather_bytes > 0) == (r > 0)
        if r:
            assert ms.gather_bytes == sum(e[4] for e in bench.sharding._manifest(res))
        assert not set(res) & set(got)
        got.update(res)
    assert sorted(got) == sorted(want) and len(got) == 14
    for k, r in want.items():
        for f in ("T2", "alpha", "mu", "perm"):
            assert torch.equal(got[k][f], r[f]), (k, f)


def test_dump_outputs_equals_step_results(tmp_path, monkeypatch):
    """bench.dump_outputs: the four float32 files hold exactly the step's results (codes unpacked
    from the 2-bit packing), linear after linear in sorted name order; with a budget too small for
    every row, the same fixed rows of every linear on each call, and no more bytes than the budget."""
    import numpy as np
    bench, ms = _small_step()
    res = ms.step()
    torch.cuda.synchronize()
    info = bench.dump_outputs(str(tmp_path / "all"), "model", res)
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in ("T", "alpha", "mu", "perm")}
    assert all(v.dtype == np.float32 for v in got.values())
    assert info["linears"] == 14 and info["bytes"] == sum(v.nbytes for v in got.values())
    want = {k: [] for k in got}
    for name in sorted(res):
        e = res[name]
        n, m = e["alpha"].shape[0], e["perm"].numel()
        want["T"].append(bench.pt2q.engine.unpack_ternary(e["T2"], (n, m)).float().cpu().numpy().ravel())
        for k in ("alpha", "mu", "perm"):
            want[k].append(e[k].float().cpu().numpy().ravel())
    for k in got:
        assert np.array_equal(got[k], np.concatenate(want[k])), k
    assert set(np.unique(got["T"])) == {-1.0, 0.0, 1.0}
    # a sampled dump: 1/8 of the whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", info["bytes"] // 8)
    a = bench.dump_outputs(str(tmp_path / "s1"), "model", res)
    b = bench.dump_outputs(str(tmp_path / "s2"), "model", res)
    assert a["bytes"] == b["bytes"] <= info["bytes"] // 8 and a["rows_T"] >= 1
    for k in got:
        s1, s2 = np.load(tmp_path / "s1" / f"{k}.npy"), np.load(tmp_path / "s2" / f"{k}.npy")
        assert np.array_equal(s1, s2), k
    assert np.array_equal(np.load(tmp_path / "s1" / "perm.npy"), got["perm"])
    # the sample's rows are rows of the whole: the first linear's first sampled row of codes
    name = sorted(res)[0]
    n, m = res[name]["alpha"].shape[0], res[name]["perm"].numel()
    row = np.load(tmp_path / "s1" / "T.npy")[:m]
    assert any(np.array_equal(row, r) for r in got["T"][:n * m].reshape(n, m))


def test_dump_outputs_layer_workload(tmp_path):
    """--workload layer: the dump holds the replayed layer's LayerOutput."""
    import numpy as np
    import bench
    a = bench.parse(["--workload", "layer", "--n", "512", "--m", "512", "--tokens", "2048"])
    bench._load_runtime(False)
    bench.resolve(a)
    out = bench.LayerStep(a, 0, 1, torch.device("cuda", 0), torch.float16).step()
    torch.cuda.synchronize()
    bench.dump_outputs(str(tmp_path), "layer", out)
    for k in ("T", "alpha", "mu", "perm"):
        want = getattr(out, k).float().cpu().numpy().ravel()
        assert np.array_equal(np.load(tmp_path / f"{k}.npy"), want) and want.size > 0, k


def _run_bench(args, timeout):
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--layers", "2",
                        "--hidden", "512", "--inter", "768", "--tokens", "2048"] + args,
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), p.stderr


def test_plain_run_line_and_dump(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` run: exactly N timed steps, the headline
    fields, nothing of what --full measures; --dump-outputs writes the same bytes on a second run."""
    import numpy as np
    d, err = _run_bench(["--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")], 120)
    assert d["steps"] == 4 and err.count("[bench] step ") == 4
    assert d["metric"] == "weight-columns quantized/sec (and s/layer) at d=4096" and d["unit"] == "cols/s"
    assert d["higher_is_better"] is True and d["dtype"] == "fp16->f32" and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["weight_columns_per_step"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert "roofline" not in d and "cpu_baseline" not in d and d["extra"] == {}
    assert "cpu baseline" not in err and "h2d" not in err
    d2, _ = _run_bench(["--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path / "b")], 120)
    assert d2["steps"] == 1
    for k in ("T", "alpha", "mu", "perm"):
        x, y = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert x.dtype == np.float32 and x.size > 0 and np.array_equal(x, y), k


def test_full_run_line():
    """`--full` keeps everything the line carried beside the headline: the Gram roofline with the
    live stage rooflines, the single-layer extras, the transfer-inclusive step, the CPU baselines."""
    d, err = _run_bench(["--steps", "1", "--warmup", "1", "--full"], 240)
    assert d["ms_per_step"] > 0 and d["steps"] == 1
    assert d["roofline"]["frac"] > 0 and d["roofline"]["stages"]["dominant"]["busy_s"] > 0
    assert d["extra"]["s_per_layer_d4096"] > 0 and d["extra"]["h2d"]["ms_per_step"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["one_core"]["value"] > 0


def test_shard_mode_line():
    """`bench.py --gpus 2 --shard all` (one process): the whole step, then both shards, one JSON
    line with the projection fields."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--shard", "all",
                        "--layers", "2", "--hidden", "512", "--inter", "768", "--tokens", "2048",
                        "--steps", "1", "--warmup", "1"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["world"] == 2 and len(d["shards"]) == 2
    assert sum(s["linears"] for s in d["shards"]) == 14
    assert d["t1_ms"] > 0 and 0 < d["projected_efficiency"] < 2
    assert set(d["share_ratio"]) == {"gram", "inverse", "tails"}
    assert d["gather_bytes_to_rank0"] == d["shards"][1]["gather_send_bytes"] > 0


@pytest.mark.gpu
def test_two_rank_launch_shared_gpu():
    """`bench.py --gpus 2 --share-gpu` (TEST ONLY: both ranks on cuda:0, gloo gather -- RCCL refuses
    two ranks on one device): the launcher starts its own torch.distributed.run child, each rank
    quantises its LPT shard and rank 0 gathers every linear's device results; the line reports
    both ranks and the whole job's columns."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu",
                        "--layers", "2", "--hidden", "512", "--inter", "768", "--tokens", "2048",
                        "--steps", "1", "--warmup", "1", "--no-extra", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and len(d["ranks"]) == 2
    assert d["gathered_linears"] == 14 and sum(r["linears"] for r in d["ranks"]) == 14
    assert d["value"] > 0
