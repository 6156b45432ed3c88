"""CPU: `python bench.py --gpus N` can never silently be a one-rank run.  The N > 1 path self-launches N
ranks through torch.distributed.run when no launcher environment is present (reference launcher: T/train_bert_base.py:40-50),
reports the world size the ranks actually observed, and refuses a launcher that started a different number of ranks."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return env


def test_gpus2_self_launches_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-check", "--backend", "gloo"], capture_output=True, text=True,
                       timeout=300, env=_clean_env())
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["ranks_joined"] == 2 and out["launch_check"] is True


def test_world_size_mismatch_fails_loudly():
    env = dict(_clean_env(), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-check"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_sweep_needs_full():
    """--sweep widens the data-parallel sweep of a --full run; without --full it is refused, not silently dropped."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--sweep", "--launch-check"], capture_output=True, text=True, timeout=300, env=_clean_env())
    assert r.returncode != 0 and "--full" in r.stderr


import pytest  # noqa: E402


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_two_rank_line_on_one_gpu_carries_the_reduce_trace():
    """The N > 1 code path of bench.py end to end on one MI355X: two gloo ranks sharing cuda:0 (RCCL refuses two ranks on one device),
    pooled negatives, bucketed gradient reduction from the backward callbacks.  The line must say what ran (2 ranks, weak scaling,
    whole-job throughput) and carry the per-bucket issue / join trace a scaling run is read with."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--share-device", "--backend", "gloo", "--bert", "tiny", "--batch", "16", "--steps", "3",
                        "--warmup", "2", "--full", "--no-secondary", "--no-cpu-baseline", "--sweep"], capture_output=True, text=True, timeout=500,
                       env=_clean_env())
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["world_size_observed"] == 2 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 32 and "pooled-negatives" in out["config"]["parallelism"]
    assert abs(out["value"] - 32 * 1e3 / out["ms_per_step"]) < 1e-2 * out["value"]
    tr = out["gradient_reduce_trace"]
    assert "error" not in tr and len(tr["buckets"]) >= 3            # recommender group, encoder layers, closing sweep
    issued = [b["issued_at_ms"] for b in tr["buckets"]]
    assert issued == sorted(issued) and tr["join_begin_ms"] >= issued[-1] and tr["join_end_ms"] >= tr["join_begin_ms"]
    assert out["config"]["gemm8p_reserve_cus"] == 0      # gloo ranks: no RCCL ring kernel to leave CUs for (train_step.TrainStep.reserve_cus)
    assert "exposed_join_ms" in tr and tr["pooled_scoring"]["Nc"] == 2 * 16 * 21          # scored against BOTH ranks' item vectors
    # --sweep (schema: INTEGRATION.md): over gloo on one device the RCCL-communicator leg is reported as skipped, the torch.distributed leg
    # runs with the reduction overlapped and not; every timed configuration carries its own trace
    sw = out["sweep"]
    assert any(c.get("comm") == "rccl" and "skipped" in c for c in sw)
    timed = [c for c in sw if "ms_per_step" in c]
    assert {(c["comm"], c["overlap_reduce"], c["reserve_cus"]) for c in timed} == {("torch.distributed", True, 0), ("torch.distributed", False, 0)}
    for c in timed:
        assert "error" not in c and c["ms_per_step"] > 0 and "error" not in c["trace"] and "exposed_join_ms" in c["trace"]
        assert abs(c["user_seq_per_s"] - 32 * 1e3 / c["ms_per_step"]) < 1e-2 * c["user_seq_per_s"]
    no_overlap = [c for c in timed if not c["overlap_reduce"]][0]["trace"]
    # without overlap nothing is issued from the backward pass: one closing sweep per arena, at the join
    assert len(no_overlap["buckets"]) <= 2 and all("issued_at_ms" in b for b in no_overlap["buckets"])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_watchdog_prints_the_headline_alone():
    """N > 1, --full: when the explanatory passes behind the timed region do not finish in MOREC_BENCH_WATCHDOG_S (here: a limit they cannot meet), rank 0
    prints the measured headline with `post_headline` saying so and every rank exits 0 -- a hang in a first real multi-GPU run must not take
    the measured number with it."""
    env = dict(_clean_env(), MOREC_BENCH_WATCHDOG_S="0.001")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--share-device", "--backend", "gloo", "--bert", "tiny", "--batch", "16", "--steps", "3",
                        "--warmup", "2", "--full", "--no-secondary", "--no-cpu-baseline"], capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world_size_observed"] == 2 and out["value"] > 0 and "watchdog" in out["post_headline"]
    assert abs(out["value"] - 32 * 1e3 / out["ms_per_step"]) < 1e-2 * out["value"]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: after exactly --steps timed steps, the last step's loss and every trained parameter's updated value and gradient
    land in DIR as float .npy files (large tensors as their fixed sample), within the size limit -- and, the headline step running in the
    deterministic mode, a second run with the same arguments writes the same bits.  A plain run stops after the timed steps; a --full run
    steps the model again after the dump and writes the same bits too."""
    import zlib

    import numpy as np

    def run(d, *extra):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--bert", "tiny", "--batch", "16", "--steps", "3", "--warmup", "2", "--no-secondary",
                            "--no-cpu-baseline", "--dump-outputs", str(d), *extra], capture_output=True, text=True, timeout=250,
                           env={k: v for k, v in _clean_env().items() if k != "MOREC_DETERMINISTIC"})
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])

    d = tmp_path / "out"
    out = run(d)
    assert out["config"]["deterministic"] is True
    # a plain run: 2 warm-up + 3 timed steps and nothing after them
    assert out["steps"] == 3 and out["steps_executed"] == 2 + 3 and out["ms_per_step"] > 0
    assert out["full"] is False and out["roofline"] is None
    files = {f.name: np.load(f) for f in d.iterdir()}
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 * 10 ** 6
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())
    # final_loss is the loss of the last TIMED step (a warm-up step's loss would not match it)
    assert files["loss.npy"].shape == (1,) and abs(float(files["loss.npy"][0]) - out["final_loss"]) < 1e-4
    params = {k[len("param."):-len(".npy")] for k in files if k.startswith("param.")}
    assert params and params == {k[len("grad."):-len(".npy")] for k in files if k.startswith("grad.")}
    assert any("bert_model" in k for k in params) and any("user_encoder" in k for k in params)
    for k in params:
        p, g = files[f"param.{k}.npy"], files[f"grad.{k}.npy"]
        assert p.shape == g.shape and p.ndim == 1 and np.isfinite(p).all()      # (an fp16 step may overflow: its gradient need not be finite)
    # real gradients, not an empty buffer: most tensors carry finite, non-zero values
    live = [k for k in params if np.isfinite(files[f"grad.{k}.npy"]).all() and np.abs(files[f"grad.{k}.npy"]).max() > 0]
    assert len(live) >= 0.9 * len(params), sorted(set(params) - set(live))[:5]
    # the word embeddings (vocab x H) are larger than the sample: the fixed, seeded sample of their flat indices
    from idvs.morec_amd.model import BertShape
    shp = BertShape.named("tiny")
    w = "bert_encoder.text_encoders.title.bert_model.embeddings.word_embeddings.weight"
    idx = np.unique(np.random.default_rng(zlib.crc32(w.encode())).integers(0, shp.vocab_size * shp.hidden_size, 16384))
    assert files[f"param.{w}.npy"].shape == idx.shape
    assert files["param.user_encoder.transformer_encoder.layer_norm.weight.npy"].shape == (512,)      # small tensors: whole
    # same arguments, same bits
    d2 = tmp_path / "again"
    run(d2)
    assert sorted(f.name for f in d2.iterdir()) == sorted(files)
    differ = [k for k, v in files.items() if not np.array_equal(np.load(d2 / k), v)]
    assert not differ, differ[:5]
    # --full: 2 warm-up + 3 timed + the instrumented pass after the headline (1 untimed + min(steps, 8) event-timed); the dump is written
    # before that pass and holds the same bits
    d3 = tmp_path / "full"
    out3 = run(d3, "--full")
    assert out3["steps"] == 3 and out3["steps_executed"] == 2 + 3 + 1 + 3 and out3["full"] is True and out3["roofline"]["launches_per_step"] > 0
    assert out3["final_loss"] == out["final_loss"] and sorted(f.name for f in d3.iterdir()) == sorted(files)
    differ = [k for k, v in files.items() if not np.array_equal(np.load(d3 / k), v)]
    assert not differ, differ[:5]
