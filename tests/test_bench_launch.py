"""CPU: `python bench.py --gpus N` without a launcher starts N ranks itself
(torch.distributed.run child, before any GPU call) and prints rank 0's JSON line with
n_gpus = N, the max-over-ranks time and per-rank rates.  Stub replicas (--stub-ms)
replace the engine; the GPU path shares the launcher and the reduction (bench.py)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_arrays_and_samples_past_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: tokens and waveforms concatenated in utterance order with their
    lengths, float32; past the size budget the waveform is a fixed seeded sample whose
    indices are stored beside it, the same from call to call."""
    import torch
    import bench
    sems = [np.arange(5, dtype=np.int64), np.arange(7, dtype=np.int64) + 100]
    wavs = [torch.arange(1280 * 5, dtype=torch.float32), -torch.arange(1280 * 7, dtype=torch.float32)]
    d = tmp_path / "a"
    bench.dump_outputs(str(d), sems, wavs)
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["semantic_lengths", "semantic_tokens", "waveform", "waveform_lengths"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["semantic_tokens"].tolist() == [*range(5), *range(100, 107)]
    assert got["semantic_lengths"].tolist() == [5, 7] and got["waveform_lengths"].tolist() == [6400, 8960]
    full = np.concatenate([w.numpy() for w in wavs])
    np.testing.assert_array_equal(got["waveform"], full)

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", (1 << 16) + 12 * 1000 + 12 * 4 + 8 * 2)
    for sub in ("a", "b"):          # over "a": the sampled dump replaces the full one
        bench.dump_outputs(str(tmp_path / sub), sems, wavs)
    idx = np.load(d / "waveform_index.npy")
    assert idx.dtype == np.float64 and idx.size == 1000 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(d / "waveform.npy"), full[idx.astype(np.int64)])
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "waveform_index.npy"))
    monkeypatch.undo()
    bench.dump_outputs(str(d), sems, wavs)       # a full dump again: no stale index left behind
    assert not (d / "waveform_index.npy").exists()


def test_bench_launches_n_ranks():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4",
                        "--warmup", "1", "--stub-ms", "20"], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout            # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["stub"] and len(d["per_rank_utt_s"]) == 2
    # rank 1 steps 1.5x slower: the job's time is the slowest rank's
    assert d["ms_per_step"] >= 29.0, d
    assert abs(d["value"] - 2 * 4 / (d["ms_per_step"] * 4e-3)) < 1e-6 * d["value"]
    assert d["per_rank_utt_s"][0] > d["per_rank_utt_s"][1]
