"""The operation areas of tests/test_gpu_frame_inputs.py and a numpy float32 mirror of fill_ref_lattice (vofod_hip.hip): which areas
and voxel sizes the frame kernel (kernels_frame.h) takes.  No test here: tests/test_properties.py holds the table's CPU test."""
import math
import re
from pathlib import Path

import numpy as np

f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent


def capacities():
    """the frame kernel's capacities, read from the kernel headers: a change there fails the table below"""
    src = (ROOT / "vofod_amd" / "csrc" / "kernels_brick_lds.h").read_text() + (ROOT / "vofod_amd" / "csrc" / "kernels_frame.h").read_text()
    out = {}
    for name in ("LB_BITWORDS", "LB_MAX", "FR_ROWS_MAX", "FR_MAX_NBZ"):
        m = re.search(r"constexpr\s+(?:int|uint32_t)\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert m, name
        out[name] = int(m.group(1))
    return out


def area_bounds(off, size):
    """operation area in float32 as vofod_create / fill_grid_params work it out (the z offset is the bottom)"""
    c = [f32(off[0]), f32(off[1]), f32(off[2]) + f32(size[2]) / f32(2)]
    lo = np.array([c[a] - f32(size[a]) / f32(2) for a in range(3)], dtype=f32)
    hi = np.array([c[a] + f32(size[a]) / f32(2) for a in range(3)], dtype=f32)
    return lo, hi


def ref_lattice(off, size, vs, cap=None):
    """fill_ref_lattice (vofod_hip.hip) in numpy float32: offset, dims, bricks, eps and the six conditions of the frame kernel.
    The grid is aligned to the map's voxel 0 (frames_launch.h: align_center = idxToCoord(0), fill_grid_params: aco)."""
    cap = cap or capacities()
    lo, hi = area_bounds(off, size)
    leaf = f32(vs)
    inv = f32(1) / leaf
    offs, dims = [], []
    cmax = dmax = f32(0)
    for a in range(3):
        centre0 = f32(f32(0.5) * leaf) + lo[a]  # VoxelMap::idxToCoord(0): the map's offset is the area's lower corner
        aco = f32(np.fmod(f32(centre0 - leaf / f32(2)), leaf))
        if aco < 0:
            aco = f32(aco + leaf)
        min_b = int(math.floor(f32(lo[a] * inv)))
        o = f32(f32(f32(min_b) * leaf) - aco)
        d = int(math.floor(f32(f32(hi[a] - o) * inv))) + 2
        offs.append(o)
        dims.append(d)
        cmax = max(cmax, f32(max(abs(lo[a]), abs(hi[a])) + leaf))
        dmax = max(dmax, f32(d))
    u = f32(1.1920929e-7)
    e1 = f32(2) * (f32(2) * cmax) * inv * u
    e2 = f32(2) * cmax * u * inv + dmax * f32(2) * u
    eps = f32(f32(4) * f32(e1 + e2) + f32(1e-4))
    nb = [(d + 3) // 4 for d in dims]
    conds = {"nbx": nb[0] <= 512, "nby": nb[1] <= 512, "nbz": nb[2] <= cap["FR_MAX_NBZ"], "bricks": nb[0] * nb[1] * nb[2] <= cap["LB_BITWORDS"] * 32,
             "rows": nb[1] * nb[2] <= cap["FR_ROWS_MAX"], "eps": bool(eps < f32(0.05))}
    return {"off": np.array(offs, dtype=f32), "dims": dims, "nb": nb, "bricks": nb[0] * nb[1] * nb[2], "rows": nb[1] * nb[2], "eps": float(eps), "inv": inv,
            "conds": conds, "on": all(conds.values())}


# the switches of tools/run_fallback_matrix.sh: under one of them a batch may take other kernels than the route a case names
FALLBACK_SWITCHES = ("VOFOD_CLOSE_FIRST", "VOFOD_DEVICE_TAIL", "VOFOD_SLABS", "VOFOD_SLAB_EMIT", "VOFOD_BRICK_LDS", "VOFOD_DILATE", "VOFOD_CCL", "VOFOD_EXPLORE")

# (the 0.2 m row has 128 cells along z where the table this one was drawn up from had 127: the lowest cell is floor(-1.25 / 0.2) = -7,
# the alignment remainder 0.15 moves the offset to -1.55, and (23.75 + 1.55) / 0.2 = 126.5 gives 126 + 2.  fill_ref_lattice says 128;
# 32 bricks along z and 608 832 bricks either way)
# name: (centre xy + bottom z, size, voxel, dims, bricks, eps to 4 places, the conditions that fail, sensor xy, sensor height or None)
TABLE = {
    "default": ((40, 20, -1.25), (120, 100, 25), 0.25, (482, 402, 102), 317_746, 0.0017, (), (0, 0), None),
    "default_0.2": ((40, 20, -1.25), (120, 100, 25), 0.2, (602, 502, 128), 608_832, 0.0021, ("bricks",), (0, 0), None),
    "x_121": ((40, 20, -1.25), (121, 100, 25), 0.25, (486, 402, 102), 320_372, 0.0017, ("bricks",), (0, 0), None),
    "long_x_508": ((0, 0, -1.25), (508, 24, 12), 0.25, (2034, 98, 50), 165_425, 0.0049, (), (245, 5), None),
    "long_x_520": ((0, 0, -1.25), (520, 24, 12), 0.25, (2082, 98, 50), 169_325, 0.0051, ("nbx",), (250, 5), None),
    "tall_62": ((0, 0, -1.25), (40, 40, 62), 0.25, (162, 162, 250), 105_903, 0.0010, (), (10, 10), 14.0),
    "tall_66": ((0, 0, -1.25), (40, 40, 66), 0.25, (162, 162, 266), 112_627, 0.0011, ("nbz",), (10, 10), 14.0),
    "long_y_rows_8016": ((0, 0, -1.25), (30, 500, 15), 0.25, (122, 2002, 62), 248_496, 0.0049, (), (5, 240), None),
    "long_y_rows_9018": ((0, 0, -1.25), (30, 500, 17), 0.25, (122, 2002, 70), 279_558, 0.0049, ("rows",), (5, 240), None),
    "negative_origin": ((-70, -60, -1.25), (120, 100, 25), 0.25, (482, 402, 102), 317_746, 0.0021, (), (-100, -80), None),
    "far_3000": ((3000, -2000, -1.25), (120, 100, 25), 0.25, (482, 402, 102), 317_746, 0.0356, (), (2960, -2020), None),
    "far_4000": ((4000, -2000, -1.25), (120, 100, 25), 0.25, (482, 402, 102), 317_746, 0.0470, (), (3960, -2020), None),
    "far_5000": ((5000, -2000, -1.25), (120, 100, 25), 0.25, (482, 402, 102), 317_746, 0.0585, ("eps",), (4960, -2020), None),
}
