"""The query calls' staging of host-resident scans (vofod_amd/csrc/scan_stage.h) without a GPU.

scan_stage_check.cpp compiles the header alone with the host compiler under -fsanitize=address,undefined and stages lists of
scans of a 3 x 2 sensor - none, one and three; host strides 4, 5 and 48 from odd addresses; with and without a pose table; host and
device scans in one list; tables, range, points or nothing asked for - holding every staged word and every returned pointer to a
plain indexed reference; the test builds and runs it.  The GPU tests of the three calls (tests/test_gpu_map_render_scans.py,
tests/test_gpu_map_match.py, tests/test_gpu_map_distance.py) hold what the kernels then compute from the block."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vofod_amd" / "csrc"


def test_scan_stage_check_runs_clean_under_the_sanitizers():
    r = subprocess.run(["make", "-C", str(CSRC), "scan_stage_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = subprocess.run([str(CSRC / "scan_stage_check")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands on stderr)
    assert out.stdout.strip() == "scan_stage_check: ok"
