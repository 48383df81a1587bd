#!/usr/bin/env python3
"""Record which kernels every case of tests/chain_route_cases.py launches, under every setting, into a JSON file.

tests/golden/chain_routes.json is this tool's output AT THE PARENT of a change to the launch path: tests/test_gpu_chain_routes.py
then holds the changed code to the same launches.  The tool uses the cases module and the public API only, so it runs on any
commit; it is never run on the code under test to refresh the file.
Usage on the GPU box:  python tools/record_chain_routes.py [OUT.json]   (default: out/chain_routes.json)"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import chain_route_cases as crc  # noqa: E402
import vofod_amd  # noqa: E402


def main():
    out = Path(sys.argv[1] if len(sys.argv) > 1 else ROOT / "out" / "chain_routes.json")
    outside = crc.outside_switches()
    if outside:
        sys.exit(f"unset {outside} first: the settings are this tool's own")
    lib = vofod_amd.library()
    inp = crc.Inputs()
    routes = {}
    for setting in crc.settings():
        env = crc.setting_env(setting)
        os.environ.update(env)
        try:
            routes[setting] = crc.routes_of_setting(lib, inp)
        finally:
            for k in env:
                del os.environ[k]
        print(setting, {c: sum(r.values()) for c, r in routes[setting].items()}, flush=True)
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("RECORDED_AT", "unknown")  # (a tree without its history: the caller names the commit)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"recorded_at": commit, "sensor": crc.SENSOR, "voxel_size": crc.VS, "routes": routes}, indent=1, sort_keys=True) + "\n")
    print(f"{out}: {len(routes)} settings x {len(next(iter(routes.values())))} calls, recorded at {commit}")


if __name__ == "__main__":
    main()
