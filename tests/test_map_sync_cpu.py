"""Map snapshots and deltas without a GPU: the numpy statement of the wire format (vofod_amd/mapsync.py, include/vofod.h) and the
torch.distributed transport of vofod_amd/dist.py (broadcast_map_bytes) over gloo with two ranks."""
import json
import multiprocessing as mp
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from vofod_amd import capi, mapsync

ROOT = Path(__file__).resolve().parent.parent


def _snapshot(maps=mapsync.MAPS_ALL, kind=mapsync.KIND_FULL, seed=0, n=(5, 0, 3), size=(7, 6, 5)):
    rng = np.random.default_rng(seed)
    m_tot = int(np.prod(size))
    recs = {}
    for m in range(3):
        if (maps >> m) & 1:
            idx = np.sort(rng.choice(m_tot, size=n[m], replace=False)).astype(np.uint32)
            recs[m] = (idx, rng.integers(0, 2**32, size=n[m], dtype=np.uint64).astype(np.uint32))
    return mapsync.Snapshot(maps=maps, kind=kind, map_size=size, map_offset=(-20.0, -30.5, -1.25), voxel_size=0.25, score_init=-0.0625,
                            base_gen=0 if kind == mapsync.KIND_FULL else 0x1234_5678_9ABC_DEF0, new_gen=0xFEDC_BA98_7654_3210, detection_its=9,
                            last_detection_id=4_000_000_123, background_pts_sufficient=1, sure_background_sufficient=0, raycast_pending=1,
                            raycast_start_its=8, records=recs)


@pytest.mark.parametrize("maps,kind,n", [(7, 1, (5, 0, 3)), (1, 0, (1, 0, 0)), (6, 0, (0, 4, 2)), (4, 1, (0, 0, 0)), (5, 1, (150, 0, 1))])
def test_encode_decode_round_trip(maps, kind, n):
    s = _snapshot(maps, kind, seed=maps * 10 + kind, n=n)
    buf = mapsync.encode(s)
    assert buf.dtype == np.uint8 and buf.size == mapsync.nbytes(n) == 128 + 8 * sum(n)
    d = mapsync.decode(buf)
    for k in ("maps", "kind", "map_size", "base_gen", "new_gen") + mapsync.STATE_FIELDS:
        assert getattr(d, k) == getattr(s, k), k
    assert d.map_offset == pytest.approx(s.map_offset) and d.voxel_size == 0.25 and d.score_init == -0.0625
    assert sorted(d.records) == sorted(s.records)
    for m, (idx, bits) in s.records.items():
        np.testing.assert_array_equal(d.records[m][0], idx)
        np.testing.assert_array_equal(d.records[m][1], bits)
    assert mapsync.encode(d).tobytes() == buf.tobytes()  # bytes -> snapshot -> the same bytes


def test_header_layout_is_the_documented_one():
    """offsets of include/vofod.h's table, read back with plain struct unpacking"""
    import struct

    s = _snapshot()
    b = mapsync.encode(s).tobytes()
    assert struct.unpack_from("<4I", b, 0) == (0x444D4656, 1, 7, 1)
    assert b[:4] == b"VFMD"
    assert struct.unpack_from("<3i", b, 16) == s.map_size
    assert struct.unpack_from("<3f", b, 28) == pytest.approx(s.map_offset)
    assert struct.unpack_from("<2f", b, 40) == (0.25, -0.0625)
    assert struct.unpack_from("<2Q", b, 48) == (0, 0xFEDC_BA98_7654_3210)
    assert struct.unpack_from("<iIii", b, 64) == (9, 4_000_000_123, 1, 0)
    assert struct.unpack_from("<ii", b, 80) == (1, 8)
    assert struct.unpack_from("<3Q", b, 88) == (5, 0, 3)
    assert b[112:128] == bytes(16)
    idx0 = np.frombuffer(b, dtype="<u4", count=5, offset=128)
    np.testing.assert_array_equal(idx0, s.records[0][0])
    bits2 = np.frombuffer(b, dtype="<u4", count=3, offset=128 + 8 * 5 + 4 * 3)
    np.testing.assert_array_equal(bits2, s.records[2][1])


def test_special_float_values_survive_as_bits():
    vals = np.array([np.inf, -0.0, np.nan, 1e-45, -np.inf], dtype=np.float32)
    bits = vals.view(np.uint32).copy()
    bits[2] = 0x7FC0_1234  # a NaN payload
    s = mapsync.Snapshot(maps=1, kind=1, map_size=(4, 2, 1), map_offset=(0, 0, 0), voxel_size=0.5, score_init=0.0,
                         records={0: (np.array([0, 1, 2, 5, 7], np.uint32), bits)})
    d = mapsync.decode(mapsync.encode(s))
    np.testing.assert_array_equal(d.records[0][1], bits)


def test_diff_records_and_apply_to_follow_the_bits():
    init = mapsync.init_bits(mapsync.MAP_VOXELS, -0.0625)
    cur = np.full(24, -0.0625, np.float32)
    cur[[3, 17]] = [np.inf, -0.0]
    idx, bits = mapsync.diff_records(cur, init)
    np.testing.assert_array_equal(idx, [3, 17])
    zero = np.zeros(24, np.float32)
    idx0, _ = mapsync.diff_records(np.array([-0.0] + [0.0] * 23, np.float32), zero)
    np.testing.assert_array_equal(idx0, [0])  # -0.0 differs from +0.0 as bits
    s = mapsync.Snapshot(maps=1, kind=1, map_size=(4, 3, 2), map_offset=(0, 0, 0), voxel_size=0.5, score_init=-0.0625, records={0: (idx, bits)})
    out = mapsync.apply_to(mapsync.decode(mapsync.encode(s)), {0: np.zeros(24, np.float32)})
    np.testing.assert_array_equal(out[0].view(np.uint32), cur.view(np.uint32))


def test_decode_rejects_bad_buffers():
    good = mapsync.encode(_snapshot())
    bad = good.copy()
    bad[0] ^= 1
    with pytest.raises(ValueError, match="magic"):
        mapsync.decode(bad)
    bad = good.copy()
    bad[4] = 2
    with pytest.raises(ValueError, match="version"):
        mapsync.decode(bad)
    for cut in (0, 64, 127, good.size - 1, good.size - 8):
        with pytest.raises(ValueError):
            mapsync.decode(good[:cut])
    with pytest.raises(ValueError):
        mapsync.decode(np.concatenate([good, np.zeros(8, np.uint8)]))
    # indices not strictly ascending: a repeated index, then a swapped pair
    s = _snapshot()
    idx, bits = s.records[0]
    s.records[0] = (np.concatenate([idx[:2], idx[1:2], idx[3:]]), bits)
    with pytest.raises(ValueError, match="ascending"):
        mapsync.decode(mapsync.encode(s))
    s.records[0] = (idx[[1, 0, 2, 3, 4]], bits)
    with pytest.raises(ValueError, match="ascending"):
        mapsync.decode(mapsync.encode(s))
    s.records[0] = (np.array([0, 1, 2, 3, 7 * 6 * 5], np.uint32), bits)  # == M
    with pytest.raises(ValueError, match="outside"):
        mapsync.decode(mapsync.encode(s))


# ---------------------------------------------------------------- gloo transport


def _payload(n_records):
    s = _snapshot(maps=1, n=(n_records, 0, 0), size=(128, 128, 64))
    return mapsync.encode(s)


def _bcast_worker(rank, world, port, out_dir, cases):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from vofod_amd import capi, dist as vdist
    from vofod_amd.detector import VofodError

    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    for name, n_records, status in cases:
        buf = _payload(n_records) if rank == 0 and status == capi.OK else None
        try:
            got = vdist.broadcast_map_bytes(buf, root=0, status=status)
            res[name] = {"status": 0, "bytes": got.tobytes().hex() if got.size < 4096 else None, "size": int(got.size),
                         "same": bool(got.tobytes() == _payload(n_records).tobytes())}
        except VofodError as e:
            res[name] = {"status": e.status}
    # a rank-local status reaches every rank (the outcome of dist.broadcast_map's apply step)
    res["agree"] = [vdist.agree_status(capi.ERR_DELTA_BASE if rank == 1 else capi.OK), vdist.agree_status(capi.OK)]
    dist.destroy_process_group()
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps(res))


def test_gloo_broadcast_map_bytes_two_ranks():
    """payloads of 0 records, 1 record and ~1 MB reach rank 1 intact; a root-side error status reaches rank 1, which returns
    (raises the status) instead of waiting for a payload"""
    cases = [("empty", 0, capi.OK), ("one", 1, capi.OK), ("error", 0, capi.ERR_DELTA_BASE), ("mb", 131_072, capi.OK), ("after_error", 1, capi.OK)]
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        port = 31500 + (os.getpid() % 2000)
        procs = [ctx.Process(target=_bcast_worker, args=(r, 2, port, d, cases)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=120)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.kill()
        assert not alive, "a rank hung"
        assert [p.exitcode for p in procs] == [0, 0]
        r0, r1 = (json.loads(Path(d, f"rank{r}.json").read_text()) for r in range(2))
    for name, n_records, status in cases:
        if status != capi.OK:
            assert r0[name] == r1[name] == {"status": status}
            continue
        assert r1[name]["status"] == 0 and r1[name]["same"], name
        assert r1[name]["size"] == 128 + 8 * n_records
        assert r0[name] == r1[name]
    assert r1["mb"]["size"] > 1_000_000
    assert r0["agree"] == r1["agree"] == [capi.ERR_DELTA_BASE, capi.OK]
