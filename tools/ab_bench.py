#!/usr/bin/env python3
"""Same-box A/B of two libbvcf builds (not a test): alternates BVCF_LIB between the given .so files
and prints per-build medians of the dominant kernel and of the chain.
usage: python tools/ab_bench.py libA.so libB.so [libC.so ...] [rounds] [-- extra bench.py args]
       python tools/ab_bench.py --in-flight libA.so libB.so [rounds] [-- extra bench.py args]
--in-flight: the plain bench line instead (`bench.py --gpus 1 --steps 20 --warmup 5`: blocks in flight, the headline's
`value`), the order of the builds turned round every round; prints every run, then per build n / median / min / max and
the later builds' median against the first one's spread (max - min).  A run that fails ends the script."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
in_flight = "--in-flight" in args
args = [x for x in args if x != "--in-flight"]
extra = []
if "--" in args:
    k = args.index("--")
    args, extra = args[:k], args[k + 1:]
libs = [x for x in args if x.endswith(".so")]
rest = [x for x in args if not x.endswith(".so")]
rounds = int(rest[0]) if rest else 4
res = {l: [] for l in libs}
if in_flight:
    for r in range(rounds):
        for l in (libs if r % 2 == 0 else libs[::-1]):
            env = dict(os.environ, BVCF_LIB=os.path.abspath(l))
            out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"] + extra,
                                          env=env, stderr=subprocess.DEVNULL, timeout=240)
            d = json.loads(out.decode().strip().splitlines()[-1])
            res[l].append(d["value"])
            print("round %d %-44s value %.0f  ms_per_step %.4f" % (r + 1, l, d["value"], d["ms_per_step"]), flush=True)
    base = res[libs[0]]
    for l in libs:
        v = res[l]
        print("%-44s n %d  median %.1f M  min %.1f  max %.1f  spread %.1f M  median against %s: %+.2f %% (%+.1f M; its spread %.1f M)" % (
            l, len(v), statistics.median(v) / 1e6, min(v) / 1e6, max(v) / 1e6, (max(v) - min(v)) / 1e6, os.path.basename(os.path.dirname(libs[0])) or libs[0],
            100 * (statistics.median(v) / statistics.median(base) - 1), (statistics.median(v) - statistics.median(base)) / 1e6, (max(base) - min(base)) / 1e6))
    sys.exit(0)
for r in range(rounds):
    for l in libs:
        env = dict(os.environ, BVCF_LIB=os.path.abspath(l))
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "1",
                                       "--no-cpu-baseline", "--no-e2e", "--slots", "1", "--blocks", "4"] + extra, env=env, stderr=subprocess.DEVNULL)
        d = json.loads(out.decode().strip().splitlines()[-1])
        res[l].append((d["roofline"]["mean_launch_ms"], d["roofline"]["chain_ms_one_block_at_a_time"]))
for l in libs:
    k = [x[0] for x in res[l]]
    c = [x[1] for x in res[l]]
    print("%-40s kernel med %.4f ms (min %.4f)  chain med %.4f ms (min %.4f)" % (
        os.path.basename(l), statistics.median(k), min(k), statistics.median(c), min(c)))
