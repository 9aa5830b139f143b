#!/usr/bin/env python3
"""The device BGZF compressor (--compressOutput bgzf) measured (not a test): one JSON line.

  kernel    k_deflate + k_crc32 + k_bgzf_scan + k_bgzf_pack with the text resident (BVCF_TIMING=json's compress.kernel_ms
            over compress.text_bytes), on configs[2]-shaped TSV and on the golden 1000 Genomes TSV
  ratio     the compressed size against zlib levels 1 and 6 over the same 65 280-byte pieces (26 bytes of framing each)
  e2e       the CLI on configs[2]-shaped rows from a BGZF file: plain, --compressOutput bgzf, and the plain output then
            compressed on the host by 16 zlib threads at level 1 (zlib releases the GIL)

usage: deflate_bench.py [ROWS]   (configs[2] rows, default 200 000: ~2 GB of VCF text)"""
import concurrent.futures as cf
import gzip
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchgen as bg  # noqa: E402
import bgzf  # noqa: E402

PIECE = 65280
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


def zlib_pieces(text, level, threads=16):
    def one(i):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        return len(c.compress(text[i:i + PIECE]) + c.flush()) + 26
    with cf.ThreadPoolExecutor(threads) as ex:
        return sum(ex.map(one, range(0, len(text), PIECE)))


def timing(stderr):
    for ln in stderr.decode().splitlines():
        if ln.startswith("[bvcf timing-json] "):
            return json.loads(ln[len("[bvcf timing-json] "):])
    return {}


def cli(args, stdin=None, out=None):
    env = dict(os.environ, BVCF_TIMING="json")
    t0 = time.perf_counter()
    with open(out or os.devnull, "wb") as fo:
        p = subprocess.run([EXE] + args, stdin=stdin, stdout=fo, stderr=subprocess.PIPE, env=env, timeout=900)
    dt = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-400:]
    return dt, timing(p.stderr)


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    tmp = os.environ.get("TMPDIR", "/tmp")
    base = os.path.join(tmp, "bvcf_deflate_%d" % rows)
    cfg = bg.make_cfg("c3")
    if not os.path.exists(base + ".bgzf"):
        with open(base + ".bgzf", "wb") as fb:
            fb.write(bgzf.bgzf_compress(bg.header(cfg), eof_marker=False, level=1))
            for first in range(0, rows, 5_000):
                fb.write(bgzf.bgzf_compress(bg.rows_host(cfg, first, min(5_000, rows - first)), eof_marker=False, level=1))
            fb.write(bgzf.bgzf_block(b""))
    res = {"rows": rows, "bgzf_file_MB": os.path.getsize(base + ".bgzf") / 1e6}
    subprocess.run(["cat", base + ".bgzf"], stdout=subprocess.DEVNULL)
    # end to end (the second of two runs each: the first pages the runtime in)
    plain_out, bgzf_out = base + ".tsv", base + ".tsv.gz"
    for _ in range(2):
        t_plain, _ = cli(["--in", base + ".bgzf"], out=plain_out)
    for _ in range(2):
        t_bgzf, tj = cli(["--in", base + ".bgzf", "--compressOutput", "bgzf"], out=bgzf_out)
    text = open(plain_out, "rb").read()
    t0 = time.perf_counter()
    z1 = zlib_pieces(text, 1)
    t_host = time.perf_counter() - t0
    c = tj.get("compress", {})
    ours = os.path.getsize(bgzf_out)
    with gzip.open(bgzf_out, "rb") as f:
        same = f.read() == text
    res["c2"] = {"tsv_MB": len(text) / 1e6, "plain_s": t_plain, "bgzf_s": t_bgzf, "bgzf_over_plain": t_bgzf / t_plain,
                 "host_zlib1_16thr_s": t_host, "plain_then_host_zlib1_s": t_plain + t_host,
                 "kernel_ms": c.get("kernel_ms"), "kernel_GBps": c.get("text_bytes", 0) / max(1e-9, c.get("kernel_ms", 0)) / 1e6,
                 "compressor_busy_s": c.get("busy_s"), "sink_wait_s": c.get("sink_wait_s"), "finish_s": c.get("finish_s"),
                 "formatter_busy_s": tj.get("formatter_busy_s"), "bytes": ours, "zlib1_bytes": z1,
                 "zlib6_bytes": zlib_pieces(text, 6), "ratio_vs_zlib1": ours / z1, "decompresses_to_plain": same}
    res["c2"]["ratio_vs_zlib6"] = ours / res["c2"]["zlib6_bytes"]
    # the golden TSV: through the CLI (its VCF), the kernel time of its compressed run
    with gzip.open(os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz"), "rb") as f:
        gv = f.read()
    gpath = base + ".golden.vcf"
    open(gpath, "wb").write(gv)
    cli(["--in", gpath], out=plain_out)
    _, tg = cli(["--in", gpath, "--compressOutput", "bgzf"], out=bgzf_out)
    gt = open(plain_out, "rb").read()
    g1, g6, gours = zlib_pieces(gt, 1), zlib_pieces(gt, 6), os.path.getsize(bgzf_out) - 28
    cg = tg.get("compress", {})
    res["golden"] = {"tsv_MB": len(gt) / 1e6, "kernel_ms": cg.get("kernel_ms"),
                     "kernel_GBps": cg.get("text_bytes", 0) / max(1e-9, cg.get("kernel_ms", 0)) / 1e6,
                     "bytes": gours, "ratio_vs_zlib1": gours / g1, "ratio_vs_zlib6": gours / g6}
    for p in (plain_out, bgzf_out, gpath):
        os.unlink(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
