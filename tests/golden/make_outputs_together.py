#!/usr/bin/env python3
"""Writes tests/golden/outputs_together.json: the sha256 of every output file of tests/test_gpu_outputs_together.py's run,
per way (bvcf_run_buffer, the CLI on one worker, the CLI on two).  Needs the GPU and a built tree.

The digests in the repository were recorded with the build of the commit before the outputs' shared open / per-batch /
finish path (bvcf_outputs.cpp), so the test holds that path to the bytes the hand-wired drivers wrote.  Record again only
when an output's bytes are meant to change, and say so in the commit."""
import json
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bystro_vcf_amd as bv  # noqa: E402
import test_gpu_outputs_together as t  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        digests = t.run_three_ways(bv, pathlib.Path(d))
    ways = list(digests)
    same = {name: len({digests[w][name] for w in ways}) == 1 for name in digests[ways[0]]}
    path = os.path.join(HERE, "outputs_together.json")
    with open(path, "w") as f:
        json.dump({"digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, {w: len(v) for w, v in digests.items()})
    print("files whose bytes differ between the ways:", [n for n, s in same.items() if not s] or "none")
