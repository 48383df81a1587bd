#!/usr/bin/env python3
"""Record what every handle-taking entry point answers in every handle state of tests/entry_gate_cases.py into a JSON file.

tests/golden/entry_refusals.json is this tool's output AT THE PARENT of a change to the entry points' admission tests:
tests/test_gpu_entry_gate.py then holds the changed code to the same statuses and error strings.  The tool uses the cases module
and the public API only, so it runs on any commit; it is never run on the code under test to refresh the file.
Usage on the GPU box:  python tools/record_entry_refusals.py [OUT.json]   (default: out/entry_refusals.json)"""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import entry_gate_cases as egc  # noqa: E402
import vofod_amd  # noqa: E402


def main():
    out = Path(sys.argv[1] if len(sys.argv) > 1 else ROOT / "out" / "entry_refusals.json")
    lib = vofod_amd.library()
    inp = egc.Inputs(lib)
    t0 = time.perf_counter()
    try:
        table = egc.table(lib, inp)
    finally:
        inp.close()
    dt = time.perf_counter() - t0
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("RECORDED_AT", "unknown")  # (a tree without its history: the caller names the commit)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"recorded_at": commit, "sensor": [egc.W, egc.H], "voxel_size": egc.VS, "table": table}, indent=1, sort_keys=True) + "\n")
    for state, rows in table.items():
        print(state, {c: r[0] for c, r in rows.items() if r[0]}, flush=True)
    print(f"{out}: {len(table)} states x {len(next(iter(table.values())))} calls in {dt:.2f} s, recorded at {commit}")


if __name__ == "__main__":
    main()
