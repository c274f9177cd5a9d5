"""bench.py's process entry on CPU (no GPU call is made before these checks):
`--gpus N` against the launcher's WORLD_SIZE, and the command that starts
N ranks when no launcher is around (the driver's plain `bench.py --gpus N`).
The GPU half (the ranks actually rendering, one JSON line with n_gpus N and
the N = 1 image hash) is tests/test_boundary_gpu.py::
test_bench_entry_two_ranks_gloo_matches_one."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_world_check():
    assert bench.world_check(1, {}) == 1
    assert bench.world_check(8, {}) is None                  # spawn the 8 ranks
    assert bench.world_check(8, {"WORLD_SIZE": "8"}) == 8
    assert bench.world_check(1, {"WORLD_SIZE": "1"}) == 1
    with pytest.raises(SystemExit) as e:
        bench.world_check(3, {"WORLD_SIZE": "2"})
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        bench.world_check(1, {"WORLD_SIZE": "8"})


def test_launcher_cmd_is_the_drivers_form():
    cmd = bench.launcher_cmd(4, ["--gpus", "4", "--steps", "2"], 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-5:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2"]


def test_dump_outputs_writes_float_arrays(tmp_path, monkeypatch):
    """--dump-outputs' writer: the RGB8 image as f32 rows, the segment count as
    f64; above DUMP_MAX_PIXELS the same seeded rows every time, with their
    indices beside them."""
    import numpy as np
    img = (np.arange(40 * 3) % 251).astype(np.uint8).reshape(40, 3)
    bench.dump_outputs(str(tmp_path / "a"), img, 12345)
    assert sorted(os.listdir(tmp_path / "a")) == ["rgb8.npy", "segments.npy"]
    rgb = np.load(tmp_path / "a" / "rgb8.npy")
    assert rgb.dtype == np.float32 and np.array_equal(rgb, img.astype(np.float32))
    seg = np.load(tmp_path / "a" / "segments.npy")
    assert seg.dtype == np.float64 and seg.tolist() == [12345.0]
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 16)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), img, 1)
    rows = np.load(tmp_path / "b" / "rgb8_rows.npy")
    assert rows.dtype == np.float64 and rows.size == 16 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "rgb8.npy"), img[rows.astype(np.int64)].astype(np.float32))
    for f in ("rgb8.npy", "rgb8_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_run_dumps_the_same_frame(tmp_path):
    """A plain run prints the headline figures only and --dump-outputs writes
    the last timed frame: its rows, put back in frame order, hash to the
    line's img_sha1.  A --full run of the same arguments adds the counting
    frame's work counts and the roofline, and dumps the identical arrays."""
    import hashlib
    import json
    import numpy as np
    from zig_raytracing_contest_amd import native, scenes
    from zig_raytracing_contest_amd import dist as zdist

    def run(extra, d):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cfg2", "--spp", "4",
                            "--steps", "2", "--warmup", "0", "--dump-outputs", str(d)] + extra,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        return json.loads(lines[0])

    j = run([], tmp_path / "plain")
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["unit"] == "Mrays/s" and j["dtype"] == "f32"
    # value = segments per step / ms_per_step (both rounded to 3 decimals in the line)
    rel = 0.0006 / j["ms_per_step"] + 0.0006 / j["value"]
    assert abs(j["value"] - j["config"]["segments_per_step"] / j["ms_per_step"] / 1e3) <= rel * j["value"]
    for k in ("roofline", "work", "cpu_baseline", "wall_clock_ms", "oracle_frame_match"):
        assert k not in j, k
    rgb = np.load(tmp_path / "plain" / "rgb8.npy")
    seg = np.load(tmp_path / "plain" / "segments.npy")
    c = scenes.CONFIGS["cfg2"]
    assert rgb.dtype == np.float32 and rgb.shape == (c["width"] * c["height"], 3)
    assert seg.dtype == np.float64 and int(seg[0]) == j["config"]["segments_per_step"]
    frame = np.zeros(rgb.shape, np.uint8)
    frame[native.tile_pixels(c["width"], c["height"], zdist.TILE)] = rgb.astype(np.uint8)
    assert hashlib.sha1(frame.tobytes()).hexdigest() == j["img_sha1"]

    f = run(["--full", "--no-cpu-baseline", "--no-wall-clock"], tmp_path / "full")
    assert f["img_sha1"] == j["img_sha1"] and f["work"]["segments"] == j["config"]["segments_per_step"]
    assert f["roofline"]["launch_ms"] > 0
    for name in ("rgb8.npy", "segments.npy"):
        assert np.array_equal(np.load(tmp_path / "full" / name), np.load(tmp_path / "plain" / name)), name


def test_mismatched_world_size_exits_nonzero():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
    assert "WORLD_SIZE=2" in p.stderr
    assert '"metric"' not in p.stdout
