"""bench.py's process launch (CPU, gloo): ``--gpus N`` without WORLD_SIZE starts N ranks
itself; the JSON line reports the world size the process group saw and every rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                           "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          env=e, timeout=240, cwd=ROOT)


def _line(p):
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (p.stdout, p.stderr[-2000:])
    return json.loads(lines[0])


def test_launcher_starts_two_ranks():
    p = _run(["--gpus", "2", "--stub", "--steps", "3", "--warmup", "1", "--prewarm-s", "0.05"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = _line(p)
    assert out["n_gpus"] == 2 and out["world_size"] == 2
    assert [r["rank"] for r in out["ranks"]] == [0, 1]
    assert len({r["pid"] for r in out["ranks"]}) == 2  # two processes, not one


def test_single_rank_stub():
    p = _run(["--gpus", "1", "--stub", "--steps", "3", "--warmup", "1", "--prewarm-s", "0.05"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = _line(p)
    assert out["n_gpus"] == 1 and len(out["ranks"]) == 1


def test_world_size_mismatch_fails():
    p = _run(["--gpus", "2", "--stub", "--steps", "1", "--warmup", "0", "--prewarm-s", "0"],
             env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0
    assert "WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_mfma_mode_is_config5_only():
    """--mode mfma names the config-5 matrix-core pass; any other config refuses it before
    touching the GPU (C5's mode="fast" runs the exact kernel)."""
    p = _run(["--mode", "mfma", "--config", "c2", "--stub"])
    assert p.returncode != 0
    assert "--mode mfma" in (p.stderr + p.stdout)


def test_rank_parity_checker_on_host_outputs():
    """bench.rank_parity (each rank's own-shard check on N > 1 lines) against the restatement's
    own outputs: equal -> all_equal; one flipped weight bit -> not (CPU, no GPU)."""
    import types

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle as orc

    offsets, sid, prob, rel, conf, present = bench.make_c2(300, 32, 500, seed=4)
    cpu = orc.consensus_csr(offsets, sid, prob, rel, conf, present)
    res = types.SimpleNamespace(**{k: torch.from_numpy(np.array(v)) for k, v in cpu.items()})
    ok = bench.rank_parity(res, offsets, sid, prob, rel, conf, present, True, 1, m_sample=200)
    assert ok["all_equal"] and ok["markets"] == 200 and ok["signals"] == 6400
    res.weight[3] = float(np.nextafter(res.weight[3].item(), 2.0))
    assert not bench.rank_parity(res, offsets, sid, prob, rel, conf, present, True, 1, m_sample=200)["all_equal"]


def _c2_host_result(M, seed):
    import types

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle as orc

    arrays = bench.make_c2(M, 32, 500, seed=seed)
    cpu = orc.consensus_csr(*arrays)
    return bench, arrays, cpu, types.SimpleNamespace(**{k: torch.from_numpy(np.array(v)) for k, v in cpu.items()})


def _check_dump(d, cpu, offsets, M):
    """The files --dump-outputs wrote against the restatement's outputs `cpu`, bit for bit."""
    import numpy as np

    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    pm = got["markets"].astype(np.int64) if "markets" in got else np.arange(M)
    for k in ("consensus", "confidence", "total_weight", "n_unique", "err_idx"):
        assert np.array_equal(got[k], cpu[k][pm].astype(got[k].dtype), equal_nan=True), k
    mk = got["sample_markets"].astype(np.int64)
    assert len(mk) and got["weight"].shape == (len(mk), 32)
    for i, m in enumerate(mk):
        a, u = int(offsets[m]), int(cpu["n_unique"][m])
        for k in ("usid", "weight", "nweight"):
            assert np.array_equal(got[k][i, :u], cpu[k][a:a + u].astype(np.float64)), (k, m)
            assert not got[k][i, u:].any(), (k, m)
    return got


def test_dump_outputs_layout_and_sampling(tmp_path, monkeypatch):
    """bench.dump_outputs_c2 on the restatement's own outputs (CPU): whole per-market arrays
    below the cap, a seeded sample with its market list above it; the per-unique rows are the
    sampled markets' valid slots, zero past n_unique; the same sample on every call."""
    import numpy as np

    bench, arrays, cpu, res = _c2_host_result(700, seed=5)
    res.weight[arrays[0][1:] - 1] = 123.0  # a market's last slot is stale unless all 32 ids differ
    dup = cpu["n_unique"] < 32
    assert dup.any()
    monkeypatch.setattr(bench, "DUMP_SAMPLE_MARKETS", 64)
    bench.dump_outputs_c2(res, 700, arrays[0], True, str(tmp_path / "a"))
    cpu["weight"][(arrays[0][1:] - 1)[~dup]] = 123.0
    a = _check_dump(str(tmp_path / "a"), cpu, arrays[0], 700)
    assert "markets" not in a and len(a["consensus"]) == 700 and len(a["sample_markets"]) == 64
    monkeypatch.setattr(bench, "DUMP_MARKETS", 300)
    for name in ("b", "c"):
        bench.dump_outputs_c2(res, 700, arrays[0], True, str(tmp_path / name))
    b = _check_dump(str(tmp_path / "b"), cpu, arrays[0], 700)
    c = _check_dump(str(tmp_path / "c"), cpu, arrays[0], 700)
    assert len(b["markets"]) == 300 and len(np.unique(b["markets"])) == 300
    assert sorted(b) == sorted(c) and all(np.array_equal(b[k], c[k], equal_nan=True) for k in b)
    bench.dump_outputs_c2(res, 700, arrays[0], False, str(tmp_path / "d"))  # compact: scalars only
    assert sorted(os.listdir(tmp_path / "d")) == ["confidence.npy", "consensus.npy", "err_idx.npy", "markets.npy",
                                                  "n_unique.npy", "total_weight.npy"]


def test_dump_outputs_is_the_headline_config_only():
    p = _run(["--stub", "--dump-outputs", "unused_dir"])
    assert p.returncode != 0 and "--dump-outputs" in (p.stderr + p.stdout)
    assert not os.path.exists(os.path.join(ROOT, "unused_dir"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_step(tmp_path):
    """A plain run on the GPU (small batch): K timed steps, no CPU baseline / parity / secondary
    lines, and --dump-outputs holds what the last step computed, bit for bit the restatement's."""
    d = str(tmp_path / "out")
    p = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0", "--markets", "3000",
              "--sources", "500", "--dump-outputs", d])
    assert p.returncode == 0, p.stderr[-2000:]
    out = _line(p)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "f64" and out["unit"] == "signals/s"
    assert out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert abs(out["value"] - 3000 * 32 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert out["cpu_baseline"] is None and "secondary" not in out and "parity_vs_oracle" not in out
    _, arrays, cpu, _ = _c2_host_result(3000, seed=2)
    _check_dump(d, cpu, arrays[0], 3000)
