"""bench.py's run modes: a plain run switches off every measurement beside the headline figure, --full leaves each to
its own option; --dump-outputs writes float arrays, large ones as the same seeded sample in every run."""
import os

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + list(argv))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return bench.parse()


def test_plain_run_is_lean(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_matrix and not a.tile_projection


def test_full_run_keeps_every_measurement(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not a.no_cpu_baseline and not a.no_matrix and a.tile_projection
    a = _parse(monkeypatch, "--full", "--no-matrix", "--no-cpu-baseline", "--no-tile-projection")
    assert a.full and a.no_cpu_baseline and a.no_matrix and not a.tile_projection


def test_child_runs_are_full(monkeypatch):
    """The matrix's rows and the projection's ranks rely on what --full measures (config 1's CPU baseline, the
    isolated phase): their child runs ask for it, without children of their own."""
    import subprocess
    seen = []

    def fake_run(cmd, **kw):
        seen.append(cmd)
        return subprocess.CompletedProcess(cmd, 1, "", "not run")

    monkeypatch.setattr(subprocess, "run", fake_run)
    bench.run_matrix()
    bench.run_projection(_parse(monkeypatch, "--full"))
    assert len(seen) == len(bench.MATRIX) + 3
    assert all("--full" in c and "--no-matrix" in c for c in seen)


def test_dump_outputs_refuses_partial_pictures(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--gpus", "2", "--dump-outputs", "x")
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--emulate-rank", "4", "--dump-outputs", "x")


def test_output_dump_samples_are_fixed(tmp_path):
    big = np.arange(5 * bench.DUMP_SAMPLE, dtype=np.uint16).reshape(5, -1)
    wide = np.array([2 ** 40 + 1, 3], np.uint64)
    for d in ("a", "b"):
        dump = bench.OutputDump(str(tmp_path / d))
        dump.put("big", big)
        dump.put("whole", big, whole=True)
        dump.put("wide", wide)
    a, b = (np.load(str(tmp_path / d / "big.npy")) for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
    assert len(np.unique(a)) > bench.DUMP_SAMPLE // 2
    w = np.load(str(tmp_path / "a" / "whole.npy"))
    assert w.dtype == np.float32 and np.array_equal(w, big)
    wd = np.load(str(tmp_path / "a" / "wide.npy"))
    assert wd.dtype == np.float64 and np.array_equal(wd.astype(np.uint64), wide)
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["big.npy", "whole.npy", "wide.npy"]


def test_output_dump_budget(tmp_path):
    dump = bench.OutputDump(str(tmp_path))
    dump.bytes = bench.DUMP_BUDGET - 4
    with pytest.raises(SystemExit):
        dump.put("x", np.zeros(2, np.uint8))


@pytest.mark.parametrize("frames", [1, 4, 7, 16])
@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160), (7680, 4320)])
def test_dump_plan_fits_the_budget(frames, size):
    """Whatever the frames in flight, the planned dump stays within the budget and keeps a usable sample."""
    picture = int(1.5 * size[0] * size[1] * 4)
    whole, sample = bench.dump_plan(frames, picture)
    assert 4096 <= sample <= bench.DUMP_SAMPLE or (not whole and sample >= 256)
    total = (picture if whole else 0) + frames * (bench.DUMP_SLOT_FIXED + bench.DUMP_SLOT_SAMPLED * 8 * sample)
    assert total <= bench.DUMP_BUDGET
    assert whole == (picture <= bench.DUMP_WHOLE) or frames > 4


def _bench_run(tmp_path, tag):
    import json
    import subprocess
    import sys
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(bench.__file__)), "bench.py"),
                        "--gpus", "1", "--steps", "2", "--warmup", "1", "--width", "640", "--height", "384",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_run_line_and_repeatable_dump(tmp_path):
    """A plain run times its steps and nothing else, and two runs with the same arguments dump the same outputs."""
    (d1, o1), (d2, o2) = _bench_run(tmp_path, "a"), _bench_run(tmp_path, "b")
    for d in (d1, d2):
        c = d["config"]
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "Mpixels/s"
        assert abs(d["value"] - c["frames_per_step"] * 640 * 384 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
        assert "cpu_baseline" not in d and "matrix" not in c and "next_rows" not in c
        assert c["tile_projection"] is None and c["transfers"]["input_upload_ms"] is None
        assert "main run" in d["roofline"]["condition"] and "contended" not in d["roofline"]
    names = sorted(os.listdir(str(o1)))
    assert names == sorted(os.listdir(str(o2)))
    slots = d1["config"]["frames_in_flight"]
    for k in range(slots):
        for n in ("lr_out_y", "cdef_out_u", "dlf_out_v", "md_sad_sse_var", "dlf_levels", "cdef_params", "lr_units_y",
                  "lr_frame_types", "cdef_mse", "cdef_fb_strength"):
            assert "slot%d_%s.npy" % (k, n) in names
    total = 0
    for n in names:
        a, b = np.load(str(o1 / n)), np.load(str(o2 / n))
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= bench.DUMP_BUDGET
    whole = np.load(str(o1 / "slot0_lr_out_y.npy"))
    assert whole.shape == (384, 640) and whole.min() >= 0 and whole.max() <= 1023 and whole.std() > 0
