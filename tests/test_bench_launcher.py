"""bench.py --gpus N spawns its own N worker processes (RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* set, before any GPU or thesia import) -- the launcher plumbing and the gloo
reductions (barrier, max time, per-rank report), on CPU via --selftest."""
import argparse
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env,
                          capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("n", [2, 3])
def test_launcher_spawns_n_workers(n):
    r = _run("--gpus", str(n), "--selftest")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1  # one JSON line, rank 0's
    d = lines[0]
    assert d["n_ranks"] == n and d["n_gpus"] == n
    assert d["per_rank_frames"] == [1000 * (k + 1) for k in range(n)]
    assert len(set(d["pids"])) == n and os.getpid() not in d["pids"]
    # max over ranks: the slowest rank sleeps 50 ms x n
    assert d["ms_per_step"] >= 50.0 * n
    assert abs(d["value"] - sum(d["per_rank_frames"]) / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


def test_single_process_without_launcher():
    r = _run("--selftest")
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_ranks"] == 1 and d["per_rank_frames"] == [1000]


def test_failing_worker_fails_the_launch():
    r = _run("--gpus", "2", "--selftest", "--selftest-fail-rank", "1")
    assert r.returncode != 0


def test_profile_records_behind_the_bench_line():
    """The default bench line's `roofline.traffic` and `roofline_valu_issue` come from the PMC
    record of exactly its workload (profiles/pmc_traffic.json: every launch parameter equal) and
    say so (`traffic_source` / `valu_insts_source`: stored, not measured in this run); any other
    workload (fewer tracks, another n_mels, another kernel) gets none. The issue roofline is the
    kernel's VALU wave-instructions over the kernel time against 256 CUs x 4 SIMDs x 2.4 GHz / 2."""
    sys.path.insert(0, ROOT)
    import bench
    saved, sys.argv = sys.argv, ["bench.py"]
    try:
        args = bench.parse()
    finally:
        sys.argv = saved
    rec = bench.profile_record(bench.workload_params(args, 5))
    assert rec is not None and rec["hbm_bytes_per_launch"] > 12.96e9  # >= the algorithmic bytes
    src = bench.provenance(rec)
    assert src["measured_in_this_run"] is False and src["profile"].startswith("profiles/r05_close")
    ic = bench.issue_ceiling(rec, 4.0)
    assert ic["bound"] == "valu-issue" and ic["peak"] == 1228.8
    assert abs(ic["achieved"] - ic["valu_insts_per_launch"] / 4e-3 / 1e9) < 1e-9 * ic["achieved"]
    assert abs(ic["frac"] - ic["achieved"] / ic["peak"]) < 1e-12
    assert ic["valu_insts_source"]["measured_in_this_run"] is False
    for change in ({"tracks": 100}, {"n_mels": 64}, {"seconds": 10.0}):
        other = argparse.Namespace(**dict(vars(args), **change))
        assert bench.profile_record(bench.workload_params(other, 5)) is None
    assert bench.profile_record(bench.workload_params(args, 3)) is None
    assert bench.issue_ceiling(None, 4.0) is None


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _parse(*argv):
    bench = _bench_module()
    saved, sys.argv = sys.argv, ["bench.py", *argv]
    try:
        return bench.parse()
    finally:
        sys.argv = saved


def test_full_is_off_by_default_and_gates_the_roofline_options():
    """A plain run measures the timed steps only; the A/B options whose figures are reported
    inside the roofline sections are refused without --full (they would be measured nowhere)."""
    assert _parse().full is False and _parse().dump_outputs is None
    assert _parse("--full").full is True
    assert _parse("--workload", "c5", "--full", "--max-blocks", "0,64").max_blocks == "0,64"
    assert _parse("--max-blocks", "0,64").max_blocks == "0,64"  # c4 / c3: a line of its own
    for argv in (["--workload", "c5", "--max-blocks", "0,64"], ["--workload", "c5", "--render-paths", "0,4"],
                 ["--workload", "c5", "--spec-policies", "0,1"], ["--output", "complex", "--row-stores", "0,1"],
                 ["--workload", "viewer", "--dump-outputs", "x"], ["--steps", "0"]):
        with pytest.raises(SystemExit):
            _parse(*argv)


class _FakeBuffer:
    """DeviceBuffer.read over a host array, counting the bytes it hands out."""

    def __init__(self, a):
        self.a, self.read_elems = a, 0

    def read(self, dtype, count, offset_elems=0):
        self.read_elems += count
        return self.a[offset_elems:offset_elems + count].astype(dtype)


def test_dump_sample_is_fixed_whole_when_small_and_within_budget():
    """--dump-outputs' sampling: the whole buffer when it fits the budget; else whole blocks in
    buffer order with the first and the last (partial) block among them, the same choice on
    every call, never more bytes than the budget."""
    import numpy as np
    bench = _bench_module()
    B = bench.DUMP_BLOCK
    a = np.arange(10 * B + 123, dtype=np.float32)
    whole = bench.sample_device(_FakeBuffer(a), np.float32, a.size, a.size * 4)
    assert whole.dtype == np.float32 and np.array_equal(whole, a)
    budget = 4 * B * 4 + 100  # 4 blocks and a remainder that buys nothing
    f1, f2 = _FakeBuffer(a), _FakeBuffer(a)
    s1 = bench.sample_device(f1, np.float32, a.size, budget)
    s2 = bench.sample_device(f2, np.float32, a.size, budget)
    assert np.array_equal(s1, s2) and s1.dtype == np.float32
    assert s1.nbytes <= budget and s1.size == 3 * B + 123 and f1.read_elems == s1.size
    assert np.all(np.diff(s1) > 0)  # buffer order, no block twice
    assert s1[0] == 0 and s1[-1] == a[-1] and np.array_equal(s1[-123:], a[-123:])
    starts = s1[:3 * B:B]
    assert np.all(starts % B == 0) and np.array_equal(s1[:3 * B].reshape(3, B) - starts[:, None],
                                                      np.tile(np.arange(B, dtype=np.float32), (3, 1)))
    u8 = bench.sample_device(_FakeBuffer((np.arange(3 * B) % 251).astype(np.uint8)), np.uint8, 3 * B, 2 * B * 4)
    assert u8.dtype == np.float32 and u8.size == 2 * B and u8.max() == 250.0


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_output(tmp_path):
    """A plain run of a 3-track C4-shaped shard: the result line holds the headline fields and
    none of --full's sections, and --dump-outputs holds the rows of the last timed step: equal,
    bit for bit, to the same batch on the same generated input run here."""
    import numpy as np
    from thesia import engine
    out = tmp_path / "out"
    r = _run("--gpus", "1", "--steps", "2", "--warmup", "1", "--tracks", "3", "--seconds", "2",
             "--dump-outputs", str(out))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0 and d["metric"]
    n, sr, ch, n_tracks = 96000, 48000, 2, 3
    plan = engine.Plan(2048, 2048, 512, engine.OUT_MEL_AMP_DB, sr=sr, n_mels=128)
    T = engine.Batch.frames_for(plan, [n] * n_tracks)
    assert d["config"]["frames_per_gpu"] == T
    assert abs(d["value"] - T / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    for k in ("roofline", "roofline_window_rfft", "bit_exact", "cpu_baseline", "c1", "end_to_end_pcie"):
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["mel_db.npy"]
    got = np.load(out / "mel_db.npy")
    assert got.dtype == np.float32 and got.shape == (T * 128,)
    din = engine.DeviceBuffer(n_tracks * n * ch * 4)
    engine.synth_pcm_device(din, engine.IN_F32, ch, n_tracks, n, sr, seed=0)
    dout = engine.DeviceBuffer(T * 128 * 4)
    b = engine.Batch(plan, din, np.arange(n_tracks, dtype=np.uint64) * (n * ch), [n] * n_tracks, dout,
                     input_format=engine.IN_F32, channels=ch)
    b.run()
    engine.synchronize()
    want = dout.to_host(np.float32)
    assert np.isfinite(want).all() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
