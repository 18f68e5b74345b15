#!/usr/bin/env python
"""Record tests/golden/front_end_transcript.json: what the 23 command-line front ends print, call, draw, write and return when
everything below them is a stub (the scenarios and stubs are those of tests/test_front_ends_host.py; CPU, no library).

    python tools/gen_goldens_front_ends.py

The file is recorded ONCE, from a commit whose front-end modules are the ones to be preserved, and names that commit.  It is not
regenerated when the front ends are reorganised: a change to it means their behaviour changed.
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "front_end_transcript.json"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("test_front_ends_host", os.path.join(ROOT, "tests", "test_front_ends_host.py"))
    scenes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scenes)
    front_ends = [os.path.join("self-diagnosing-gan_amd", "diagan", n + ".py")
                  for n in ("cli", "eval_cli", "attr_cli", "feature_cli", "stylegan2_cli")]
    if subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--"] + front_ends).returncode:
        raise SystemExit("the front-end modules differ from HEAD: record from a commit")
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        table = scenes.run_scenarios(Path(tmp) / "runs")
    with open(args.out, "w") as f:
        json.dump({"recorded_at_commit": commit, "scenarios": table}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(table)} scenarios of commit {commit[:12]}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
