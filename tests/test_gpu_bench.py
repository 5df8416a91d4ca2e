"""bench.py's multi-rank path on the GPU box: `--gpus 2` starts its own two
ranks (torch.distributed.run, before any GPU call), splits one batch by
bytes, and reports a max-over-ranks time.  With one GPU on the test box the
two ranks share device 0 and talk over gloo (--one-device); the driver's
8-GPU run uses RCCL with one rank per GPU.  And its plain run with
--dump-outputs, checked against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bench_two_ranks_rehearsal():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--dist-backend", "gloo",
           "--one-device", "--strings", "65536", "--steps", "2", "--warmup", "1",
           "--c5-strings", "200000", "--c4-blocks", "2000", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["bit_exact"] is True
    assert rec["config"]["plain_bytes_all"] > rec["config"]["plain_bytes_rank0"]
    ex = rec["extra"]
    assert ex["config5_zipf"]["bit_exact"] is True and ex["config5_zipf"]["shards"] == 2
    assert ex["config4_qpack_blocks"]["bit_exact"] is True
    assert ex["enc_global_offset_rank0"] == 0
    # the north-star path at N > 1: every rank its shard from pinned host
    # memory, timed as the max over ranks, aggregate over all ranks' bytes
    hp = ex["host_path"]
    assert hp["ranks"] == 2 and hp["bit_exact"] is True
    assert hp["plain_bytes_all"] == rec["config"]["plain_bytes_all"]
    assert hp["decode_GiBps_incl_h2d_d2h_all"] > 0 and hp["ms_rank0"] > 0
    assert hp["ms_max_over_ranks"] >= hp["ms_rank0"] - 1e-6


def _valid_checks(bench, valid):
    """The <s>_sums and <s>_sample arrays that bench.dump_outputs documents,
    restated on the CPU for the back-to-back valid bytes of one stream."""
    m = valid.size
    c = bench.DUMP_CHUNK * max(1, -(-m // (bench.DUMP_CHUNK << 16)))
    v = np.concatenate([valid, np.zeros((-m) % c, np.uint8)]).reshape(-1, c).astype(np.int64)
    w = 1 + np.arange(c, dtype=np.int64) % 251
    sums = np.stack([v.sum(1), (v * w).sum(1)], 1).astype(np.float64)
    at = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, m, size=min(m, bench.DUMP_SAMPLE)))
    return sums, valid[at].astype(np.float32)


def test_bench_plain_run_dumps_the_last_steps_outputs(tmp_path):
    """A plain run (no --full): the result line's headline fields, nothing of
    the other legs, and --dump-outputs files that equal what the oracle
    computes for the same seeded batch -- every span and status, the checksum
    of every 4 KiB of encoded and decoded bytes, and the sampled bytes (12,000
    strings: more valid bytes than the sample holds, and no multiple of any
    block or chunk size)."""
    import bench
    import oracle
    from nghttp3_amd import decode_slot_size, synth
    n, steps = 12000, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--strings", str(n), "--dump-outputs", str(tmp_path / "out")]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])

    plain, off, ln = synth.batch(0x5EED0003, n, 8, 256, synth.ALPHABET_A)
    assert rec["metric"] == bench.METRIC and rec["unit"] == "GiB/s" and rec["dtype"] == "u8"
    assert rec["higher_is_better"] is True and rec["full"] is False
    assert rec["steps"] == steps and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["config"]["plain_bytes_all"] == plain.size
    assert rec["ms_per_step"] > 0
    # value and ms_per_step are the same measurement, each rounded on its
    # own: value to 0.01 GiB/s, ms_per_step to 1e-4 ms of a step of >= 0.05 ms
    assert rec["value"] == pytest.approx(plain.size / (rec["ms_per_step"] * 1e-3) / bench.GIB, rel=2e-3, abs=0.006)
    assert rec["extra"] is None and rec["roofline"] is None and rec["cpu_baseline"] is None
    assert rec["bit_exact"] is None

    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == [s + k for s in ("dec", "enc") for k in ("_sample", "_spans", "_status", "_sums")]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")) <= 64_000_000

    enc, eoff, elen = oracle.encode_batch(plain, off, ln)
    slot = decode_slot_size(elen.astype(np.int64))
    want = {"enc": (np.stack([eoff, elen], 1), enc),
            "dec": (np.stack([np.cumsum(slot) - slot, ln], 1), plain)}
    for s, (spans, valid) in want.items():
        assert np.array_equal(got[s + "_spans"], spans.astype(np.float64)), s
        assert np.array_equal(got[s + "_status"], np.zeros(n, np.float32)), s
        sums, sample = _valid_checks(bench, valid)
        assert sample.size == bench.DUMP_SAMPLE < valid.size
        assert np.array_equal(got[s + "_sums"], sums), s
        assert np.array_equal(got[s + "_sample"], sample), s
