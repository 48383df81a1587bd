"""bench.py's plain run and its --dump-outputs: the synthetic inputs are the same whichever way they are built (worker
processes or one by one), the dump holds every field of the last step's detection records as float64 within its size cap,
and on the GPU two plain runs with the same arguments dump the same outputs and print the headline fields only."""
import json
import multiprocessing
import subprocess
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _assert_same_scans(want, got):
    assert len(want) == len(got)
    for a, b in zip(want, got):
        for k in ("x", "y", "z", "intensity", "range", "tf"):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
        assert b.scan.x is b.x and b.scan.range is b.range  # (the scan views its own columns after the trip between processes)


def test_scans_built_in_worker_processes_are_the_serial_ones():
    from vofod_amd import synth

    scene = synth.bench_scene()
    with ProcessPoolExecutor(2, mp_context=multiprocessing.get_context("spawn")) as pool:
        frames = synth.bench_frames(scene, "os1-128", 4, rank=1, pmap=pool.map)
        seq = synth.scan_sequence(scene, "os1-16", 3, seed0=synth.BENCH_WARM_SEED0, pmap=pool.map)
    _assert_same_scans(synth.bench_frames(scene, "os1-128", 4, rank=1), frames)
    _assert_same_scans(synth.scan_sequence(scene, "os1-16", 3, seed0=synth.BENCH_WARM_SEED0), seq)


def test_dump_holds_every_field_as_float64_within_its_cap(tmp_path):
    import bench
    from vofod_amd import capi

    dets = np.zeros(10, dtype=capi.DETECTION)
    dets["id"] = np.arange(100, 110)
    dets["frame"] = np.arange(10) // 4
    dets["n_points"] = 2**40 + np.arange(10)
    dets["confidence"] = np.linspace(0.0, 1.0, 10)
    dets["position"] = np.arange(30).reshape(10, 3) * 0.5
    dets["covariance"][:, 0] = 3.0
    per = np.array([4, 4, 2], dtype=np.uint32)
    bench.dump_outputs(tmp_path / "all", dets, per)
    names = sorted(p.name for p in (tmp_path / "all").iterdir())
    assert names == sorted([f"detections_{k}.npy" for k in capi.DETECTION.names] + ["detections_per_frame.npy"])
    for k in capi.DETECTION.names:
        a = np.load(tmp_path / "all" / f"detections_{k}.npy")
        assert a.dtype == np.float64 and a.shape == (10,) + capi.DETECTION[k].shape
        np.testing.assert_array_equal(a, dets[k].astype(np.float64))
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "detections_per_frame.npy"), [4.0, 4.0, 2.0])
    # a cap that holds the counts and four records: a fixed sample of four, in their order, the same every time
    cap = 8 * len(per) + 4 * 8 * 17  # (17 float64 per record)
    bench.dump_outputs(tmp_path / "a", dets, per, max_bytes=cap)
    bench.dump_outputs(tmp_path / "b", dets, per, max_bytes=cap)
    ids = np.load(tmp_path / "a" / "detections_id.npy")
    assert len(ids) == 4 and np.all(np.diff(ids) > 0) and set(ids) <= set(dets["id"].astype(np.float64))
    np.testing.assert_array_equal(ids, np.load(tmp_path / "b" / "detections_id.npy"))
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= cap + 128 * len(names)  # (+ the .npy headers)


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    d1 = _plain_run(tmp_path / "a")
    d2 = _plain_run(tmp_path / "b")
    for d in (d1, d2):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
        assert d["ms_per_step"] > 0 and abs(d["value"] - d["config"]["frames_per_gpu_per_step"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert not {"roofline", "kernels", "cpu_baseline", "single_stream", "config3_share", "loaded_tail", "host_input"} & set(d)  # (--full only)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names and names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert len(np.load(tmp_path / "a" / "detections_per_frame.npy")) == d1["config"]["frames_per_gpu_per_step"]
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n), err_msg=n)
