"""Two ranks, one map: rank 0 builds a map with a sensor stream, rank 1 starts empty and receives a full snapshot and one
delta through vofod_amd.dist.broadcast_map (torch.distributed over gloo; two fresh child processes share the one GPU).  Both
then run the same read-only batch."""
import hashlib
import json
import multiprocessing as mp
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _rank(rank, port, out_dir):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import vofod_amd
    from test_gpu_stream_route import cycle
    from vofod_amd import capi, dist as vdist, synth
    from vofod_amd.detector import VoFOD, VofodError, default_params

    dist.init_process_group("gloo", rank=rank, world_size=2)
    hip = vofod_amd.library()
    h, w, vfov_deg, _ = synth.SENSORS["os1-128"]
    sp, dp = default_params(hip)
    sp.voxel_size, sp.sensor_hrays, sp.sensor_vrays, sp.max_batch_frames = 0.25, w, h, 4
    sp.sensor_vfov = np.float32(np.deg2rad(vfov_deg))
    det = VoFOD(hip, sp, dp)
    scene = synth.make_scene(21, n_targets=3)
    scans = synth.scan_sequence(scene, "os1-128", 11, seed0=300)
    if rank == 0:
        det.load_apriori(synth.apriori_points(scene, 0.25, n_voxels=1_000_000, solid_ground_to=-1.2))
        for k in range(6):
            cycle(det, scans[k], k)
    n_full = vdist.broadcast_map(det, root=0, maps=capi.MAPS_ALL, full=True)
    if rank == 0:
        cycle(det, scans[6], 6)
    n_delta = vdist.broadcast_map(det, root=0, maps=capi.MAPS_ALL, full=False)
    # the owner exports outside the broadcast (a checkpoint): its chain restarts, so the replica misses a delta.  Every rank
    # sees the replica's DELTA_BASE and takes the documented recovery (a full snapshot) together.
    missed = None
    if rank == 0:
        det.save_map(Path(out_dir) / "checkpoint.vfmd")
        cycle(det, scans[7], 7)
    try:
        vdist.broadcast_map(det, root=0, maps=capi.MAPS_ALL, full=False)
    except VofodError as e:
        missed = e.status
        vdist.broadcast_map(det, root=0, maps=capi.MAPS_ALL, full=True)
    if rank == 0:
        cycle(det, scans[8], 8)
    n_after = vdist.broadcast_map(det, root=0, maps=capi.MAPS_ALL, full=False)  # the new chain carries on
    batch = scans[7:11]
    dets, per = det.process_batch([s.scan for s in batch], np.stack([s.tf for s in batch]))
    digest = hashlib.sha256()
    for m in range(3):
        digest.update(det.read_map(m).tobytes())
    st = det.status()
    res = {"dets": dets.tobytes().hex(), "per": per.tolist(), "map": digest.hexdigest(), "n_full": n_full, "n_delta": n_delta, "missed": missed, "n_after": n_after,
           "status": [st.detection_its, st.last_detection_id, st.background_pts_sufficient, st.sure_background_sufficient, st.raycast_pending]}
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(res))
    det.close()
    dist.destroy_process_group()


def test_two_ranks_full_then_delta_then_same_batch():
    """a full snapshot and a delta; then a delta the replica cannot apply (the owner exported a checkpoint in between), which
    every rank sees and recovers from with a full snapshot; then the next delta; then the same read-only batch on both"""
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        port = 33500 + (os.getpid() % 2000)
        procs = [ctx.Process(target=_rank, args=(r, port, d)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=150)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.kill()
        assert not alive, "a rank did not finish"
        assert [p.exitcode for p in procs] == [0, 0]
        r0, r1 = (json.loads(Path(d, f"rank{r}.json").read_text()) for r in range(2))
    assert r0["n_full"] == r1["n_full"] > 128 and r0["n_delta"] == r1["n_delta"] > 128
    assert r0["missed"] == r1["missed"] == 14  # capi.ERR_DELTA_BASE on both ranks, not only on the replica
    assert r0["n_after"] == r1["n_after"] > 128
    assert r0["map"] == r1["map"]
    assert r0["status"] == r1["status"]
    assert r0["per"] == r1["per"]
    assert r0["dets"] == r1["dets"]
