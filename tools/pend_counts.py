#!/usr/bin/env python3
"""Why does k_stream's pending-store log leave?  Flushes by cause and their pieces, with blocks in flight as in the bench
line, and the resident workgroups per CU of the kernels that share a CU.  (not a test; needs an experiments build:
    make -C bystro-vcf_amd/csrc OUT=/tmp/t OBJ=/tmp/t/obj EXTRA="-DBVCF_EXPERIMENTS -DBVCF_EXP_PEND_COUNTS" \
      && BVCF_LIB=/tmp/t/libbvcf.so python tools/pend_counts.py c3 [epoch ticks ...]
The epoch is BVCF_PEND_EPOCH_TICKS, one ctx per value; log size and look period are build knobs, see the Makefile.)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchgen as bg  # noqa: E402
import bystro_vcf_amd as bv  # noqa: E402

ROWS = {"c3": 311_296, "c4": 262_144}
BLOCKS, SLOTS, STEPS = 4, 3, 3
CAUSES = ["epoch", "capacity", "exit", "before a direct store"]
prof = sys.argv[1] if len(sys.argv) > 1 else "c3"
epochs = sys.argv[2:] or [""]
cfg = bg.make_cfg(prof)
rows = ROWS[prof]
blocks = [bg.rows_device(cfg, b * rows, rows, pad=bv.DEVICE_PAD) for b in range(BLOCKS)]
ptrs, sizes = [t.data_ptr() for t, _ in blocks], [n for _, n in blocks]
ns = cfg.n_samples
stride = ((ns + 3) // 4 + 15) & ~15
n_alt = rows * (4 if prof == "c4" else 1) + 1024
occ = (C.c_int * 3)()
if bv.lib.bvcf_debug_occupancy(occ) == 0:
    print("workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor): k_stream %d  k_head_lean %d  k_gt %d" % tuple(occ))
out = (C.c_ulonglong * 8)()
for ep in epochs:
    if ep:
        os.environ["BVCF_PEND_EPOCH_TICKS"] = ep
    ctx = bv.Ctx(bg.n_header_fields(cfg), max_batch_bytes=max(sizes), n_slots=SLOTS, max_lines=rows + 16, max_alleles=n_alt,
                 cmap_bytes=min((n_alt + max(sizes) // (4 * ns + 8) + 16 * 8192) * stride + 4096, 0xFFFFFF00), path=2)
    ctx.bench_device(ptrs, sizes, BLOCKS)
    assert bv.lib.bvcf_debug_pend_counts(out) == 0  # (zeroes them: the warm-up's are dropped)
    ctx.bench_device(ptrs, sizes, STEPS * BLOCKS)
    assert bv.lib.bvcf_debug_pend_counts(out) == 0
    ctx.close()
    n, p = list(out[:4]), list(out[4:])
    print("== %s, epoch %s ticks, %d blocks in flight, %d launches: %d flushes, %.1f pieces each, %.0f per launch" % (
        prof, ep or "default", SLOTS, STEPS * BLOCKS, sum(n), sum(p) / max(sum(n), 1), sum(n) / (STEPS * BLOCKS)))
    for k in range(4):
        print("  %-22s %9d flushes  %5.1f %%   %6.1f pieces each   %5.1f %% of the pieces" % (
            CAUSES[k], n[k], 100.0 * n[k] / max(sum(n), 1), p[k] / max(n[k], 1), 100.0 * p[k] / max(sum(p), 1)))
