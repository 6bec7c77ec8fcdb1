"""`not gpu`: bench.py's own logic -- the JSON line it assembles -- at world sizes the 1-GPU boxes cannot run.  `--emulated` runs the real kernel
sources on the CPU emulator of tests/hostemu with gloo in place of RCCL; the figures mean nothing, the STRUCTURE of the line is what is tested:
at N > 1 the line must carry a non-null `parity` (every rank's sampled documents against the oracle, reduced), `cpu_baseline` (rank 0's bounded
sample) and `roofline` (the slowest rank's kernels) -- the round-4 review's point: without them a scaling line earns nothing."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, extra, timeout=900, full=True):
    args = ["--emulated", "--gpus", str(world), "--steps", "1", "--warmup", "1", "--pipelined-steps", "0", "--min-len", "20", "--max-len", "300"] + extra
    if full:
        args.append("--full")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    if world == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py")] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]           # ONE JSON line on stdout, from rank 0
    return json.loads(lines[0])


def test_world_2_line_has_parity_cpu_baseline_and_roofline():
    line = _run(2, ["--docs", "240", "--parity-sample-docs", "50", "--cpu-sample-docs", "120"])
    assert line["emulated"] is True and line["data"].startswith("EMULATED")
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["steps"] == 1 and line["warmup"] == 1
    assert line["config"]["job_docs"] == 480 and line["config"]["docs_per_gpu"] == 240
    # parity: both ranks checked the first and the last 50 documents of their own shard
    assert line["parity"].startswith("bit-exact vs oracle on 2 x 100 = 200 sampled docs"), line["parity"]
    # cpu_baseline: rank 0's bounded sample, non-null, with its thread sweep and the one-thread figure
    cpu = line["cpu_baseline"]
    assert cpu and cpu["kind"] == "port" and cpu["value"] > 0 and cpu["value_1_thread"] > 0 and cpu["cores"] >= 1 and "120 documents" in cpu["sample"]
    # roofline: the slowest rank's kernels, priced with that rank's algorithmic bytes
    r = line["roofline"]
    # (the emulator's GB/s round to zero: present and numeric is what is asserted)
    assert r and r["bound"] == "hbm" and r["achieved"] >= 0 and 0 <= r["frac"] < 1 and r["peak"] == 8000.0 and r["rank"] in (0, 1) and r["avg_launch_ms"] > 0
    assert r["algorithmic_bytes_per_launch"] > 0 and set(r["kernels_ms"]) >= {"k_probe", "k_place", "k_pretok"}
    assert line["rank_ms_per_step"]["max"] >= line["rank_ms_per_step"]["min"] > 0
    assert line["value"] > 0 and line["ms_per_step"] == pytest.approx(line["rank_ms_per_step"]["max"], rel=1e-3)


def test_world_2_shard_smaller_than_two_samples_is_checked_whole():
    line = _run(2, ["--docs", "60", "--parity-sample-docs", "50", "--cpu-sample-docs", "60", "--kind", "2"])
    assert line["parity"].startswith("bit-exact vs oracle on 2 x 60 = 120 sampled docs (every document of every rank's shard"), line["parity"]
    assert line["cpu_baseline"] and line["roofline"]


def test_world_1_line_and_real_text_kind(tmp_path):
    # the default shape at N = 1 (full-batch parity) ...
    line = _run(1, ["--docs", "150", "--cpu-sample-docs", "100", "--real-text-mb", "0", "--heldout-steps", "0"])
    assert line["parity"].startswith("bit-exact vs oracle on all 150 docs") and line["cpu_baseline"] and line["roofline"] and line["n_gpus"] == 1
    # ... and kind 6: real files (this repository's sources), every file once, cut at character boundaries; the memo emptied before every step
    line = _run(1, ["--kind", "6", "--real-text-mb", "1", "--real-text-root", ROOT, "--vocab", "gpt2", "--pattern", "1", "--cpu-sample-docs", "500"])
    rt = line["config"]["real_text"]
    assert rt["bytes"] >= 1 << 20 and rt["files"] > 10 and len(rt["sha256"]) == 64 and rt["docs"] == line["config"]["docs_per_gpu"]
    assert line["parity"].startswith("bit-exact vs oracle on all %d docs" % rt["docs"]), line["parity"]
    assert "EMPTIED before every step" in line["config"]["piece_memo"] and line["value_warm_memo"] and line["value_no_memo"]
    assert line["config"]["vocab"] == "gpt2" and line["config"]["pattern"].startswith("pattern 1")


def test_plain_line_and_dumped_outputs(tmp_path):
    # a plain run times the headline steps and nothing else; --dump-outputs writes what its last step computed -- the same arrays as a --full
    # run's, whose parity check holds every document against the oracle
    common = ["--docs", "150", "--cpu-sample-docs", "100", "--real-text-mb", "0", "--heldout-steps", "0"]
    plain = _run(1, common + ["--dump-outputs", str(tmp_path / "plain")], full=False)
    assert plain["steps"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["unit"] == "MB/s" and plain["higher_is_better"] is True
    assert not {"parity", "roofline", "cpu_baseline", "piece_stats", "value_no_memo", "first_call"} & set(plain)
    full = _run(1, common + ["--dump-outputs", str(tmp_path / "full")])
    assert full["parity"].startswith("bit-exact vs oracle on all 150 docs"), full["parity"]
    for name in ("n_tokens", "token_offsets", "ids"):
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    n = plain["config"]["tokens_per_gpu"]
    offs, ids = np.load(tmp_path / "plain" / "token_offsets.npy"), np.load(tmp_path / "plain" / "ids.npy")
    assert np.load(tmp_path / "plain" / "n_tokens.npy").tolist() == [n]
    assert len(offs) == 151 and offs[0] == 0 and offs[-1] == n and (np.diff(offs) > 0).all()
    assert len(ids) == plain["config"]["bytes_per_gpu"] and (ids[:n] >= 0).all() and (ids[n:] == -1).all()


def test_dump_outputs_samples_large_arrays(tmp_path):
    # past its budget an array is sampled at sorted positions of a fixed seed: ids[i] = i shows which, and -1 stands where a position is past the tokens
    import torch
    import bench
    total, ntok, n_docs = 12 << 20, 10 << 20, 3 << 20
    d_ids = torch.arange(total, dtype=torch.int32)
    d_ooffs = torch.arange(n_docs + 1, dtype=torch.int64) * 3
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), d_ids, ntok, d_ooffs, n_docs, total)
    size = 0
    for name in ("n_tokens", "token_offsets", "ids"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert np.array_equal(a, b), name
        size += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert size <= 64 << 20
    ids, offs = np.load(tmp_path / "a" / "ids.npy"), np.load(tmp_path / "a" / "token_offsets.npy")
    assert ids.dtype == np.float32 and offs.dtype == np.float64
    assert len(ids) == 1 << 23 and len(offs) == 1 << 21
    kept = ids[ids >= 0]
    assert (np.diff(kept) > 0).all() and kept[-1] < ntok and (ids[len(kept):] == -1).all() and len(kept) < len(ids)
    assert (offs % 3 == 0).all() and (np.diff(offs) > 0).all() and offs[-1] <= 3 * n_docs
