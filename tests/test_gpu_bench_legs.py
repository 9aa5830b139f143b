"""bench.py's N > 1 leg -- rank 0's `bystro-vcf --devices 0,..,N-1` run over text and BGZF with the whole output hashed
against the oracle -- cannot run on the one-GPU boxes with N > 1; its code path can, with the one device there is: the file
is written, the BGZF twin built, the CLI run twice over each, the hashes compared.  (A crash in there on the first 8-GPU
node would cost the scaling record.)"""
import argparse
import json

import pytest

pytestmark = pytest.mark.gpu


def test_all_devices_leg_with_the_one_device():
    import torch
    import bench
    import benchgen as bg
    import bystro_vcf_amd as bv
    cfg = bg.make_cfg("c3")
    args = argparse.Namespace(blocks=2, rows=12_000, all_devices_rows=24_000, profile="c3")
    blocks, sizes = [], []
    for first in bench.rank_blocks(0, args.blocks, args.rows):
        t, n = bg.rows_device(cfg, first, args.rows, pad=bv.DEVICE_PAD)
        blocks.append(t)
        sizes.append(n)
    line = {}
    bench.all_devices_leg(line, args, cfg, bg, bv, blocks, sizes, 1, lambda: None)
    assert "host_legs_error" not in line, line
    leg = line["e2e_all_devices"]
    assert leg["devices"] == "0" and leg["full_output_check"]["equal"], leg["full_output_check"]
    for k in ("text", "bgzf"):
        assert leg[k]["rows"] == 24_000 and leg[k]["wall_s"] > 0 and "error" not in leg[k], leg[k]
    # ... and the compact line carries its summaries
    full = {"metric": "variants/sec", "value": 1.0, "unit": "variants/s", "n_gpus": 2, "config": {"workload": "x"}, "e2e_all_devices": leg,
            "ranks_seen": 2, "per_rank_variants_per_s": [1.0, 1.0]}
    out = json.loads(bench.compact_line(full))
    assert out["e2e_all_devices_text"]["sha256_equal"] is True and out["e2e_all_devices_bgzf"]["wall_s"] > 0
    del blocks
    torch.cuda.empty_cache()


def test_bench_main_takes_the_multi_rank_path_with_one_rank():
    """bench.py's main() through every N > 1 branch -- RCCL process group, the gloo group for the host-side wait, the
    reductions, rank 0's all-devices leg, the barrier, the compact line -- with ONE rank (BVCF_BENCH_FORCE_MULTI=1 and the
    launcher's environment): what the driver's torch.distributed.run starts on an 8-GPU node, minus the other seven"""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               BVCF_BENCH_FORCE_MULTI="1")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--blocks", "2",
                        "--rows", "12000", "--all-devices-rows", "24000", "--full"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                       timeout=600, cwd=root)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    last = p.stdout.decode().splitlines()[-1]
    assert len(last) < 3072
    line = json.loads(last)
    assert line["n_gpus"] == 1 and line["ranks_seen"] == 1 and len(line["per_rank_variants_per_s"]) == 1 and line["value"] > 0
    assert line["roofline"]["frac"] > 0 and "cpu_baseline" not in line  # (cpu_baseline: rank 0 at N == 1 only)
    assert line["e2e_all_devices_text"]["sha256_equal"] is True and line["e2e_all_devices_bgzf"]["wall_s"] > 0


def test_plain_run_is_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: the line has the headline and no leg
    that --full adds, `steps` is K, and two runs with the same arguments write the same arrays (float32 / float64, at
    most 64 MB) whose records are the ones the row model makes (configs[2]: biallelic SNPs, an == 2 * samples)"""
    import os
    import subprocess
    import sys
    import numpy as np
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--blocks", "2", "--rows", "12000", "--dump-outputs", str(d)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=600, cwd=root)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        line = json.loads(p.stdout.decode().splitlines()[-1])
        assert line["metric"] == "variants/sec" and line["unit"] == "variants/s" and line["higher_is_better"] is True
        assert line["dtype"] == "u8" and line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert abs(line["value"] - 2 * 12000 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
        for k in ("cpu_baseline", "e2e", "e2e_bgzf", "real_data_frac", "value_at_library_default_slots"):
            assert k not in line, k
        assert line["roofline"]["frac"] is None and line["roofline"]["chain_frac"] > 0
        arrays = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert sum(a.nbytes for a in arrays.values()) <= bench.DUMP_LIMIT_BYTES
        assert all(a.dtype in (np.float32, np.float64) and a.size for a in arrays.values())
        dumps.append(arrays)
    a, b = dumps
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    n = 2 * min(12000, bench.DUMP_LINES_PER_BLOCK)
    assert len(a["line_index"]) == n and len(a["record_pos"]) == n and (a["line_status"] == 0).all()
    assert (a["record_an"] == 2 * 2504).all() and (a["record_ac"] == a["record_n_het"] + 2 * a["record_n_hom"]).all()
    # every row of the step's blocks passes and gives one record; configs[2]'s rows have no errors, so no err_* file
    assert a["block_counts"].tolist() == [[12000, 12000, 12000, 0]] * 2 and not [k for k in a if k.startswith("err_")]
    cls = a["classes"]
    assert cls.shape[1] == 2504 and len(cls) == len(a["classes_record"]) > 0
    rec = a["classes_record"].astype(int)
    assert ((cls == 1).sum(axis=1) == a["record_n_het"][rec]).all() and ((cls == 2).sum(axis=1) == a["record_n_hom"][rec]).all()
    # the dumped records and class codes against the oracle on the dumped lines, regenerated on the host from the same
    # first rows (bench.rank_blocks); configs[2]'s lines give one record each, so the oracle's row j is record j
    import benchgen as bg
    import bystro_vcf_amd as bv
    import oracle_lib as orc
    cfg = bg.make_cfg("c3")
    texts = [bg.rows_host(cfg, first, 12000).split(b"\n") for first in bench.rank_blocks(0, 2, 12000)]
    blk, idx = a["line_block"].astype(int), a["line_index"].astype(int)
    assert (a["record_block"] == a["line_block"]).all() and (a["record_line"] == a["line_index"]).all()
    rc, out, log, n_rows = orc.run(bg.header(cfg) + b"".join(texts[k][i] + b"\n" for k, i in zip(blk, idx)), n_threads=16)
    assert rc == 0 and log == "" and n_rows == n
    rows = [r.decode().split("\t") for r in out.split(b"\n") if r]
    assert len(rows) == n
    hdr = bv.string_header().split("\t")
    col = {k: hdr.index(k) for k in ("pos", "ref", "alt", "trTv", "heterozygotes", "homozygotes", "missingGenos", "ac", "an")}
    names = ["HG%05d" % s for s in range(2504)]

    def listed(r, k):
        return 0 if r[col[k]] == "!" else len(r[col[k]].split(";"))
    for j, r in enumerate(rows):
        assert (int(r[col["ac"]]), int(r[col["an"]]), r[col["ref"]], r[col["alt"]], int(r[col["trTv"]])) == (
            a["record_ac"][j], a["record_an"][j], chr(int(a["record_ref"][j])), chr(int(a["record_alt_base"][j])),
            a["record_trtv"][j]), (j, r[:6])
        # (pos: the output position, unless the record says the line's POS text is printed as it is)
        assert a["record_pos_text"][j] or int(r[col["pos"]]) == a["record_pos"][j], (j, r[:6], a["record_pos"][j])
        assert (listed(r, "heterozygotes"), listed(r, "homozygotes"), listed(r, "missingGenos")) == (
            a["record_n_het"][j], a["record_n_hom"][j], a["record_n_miss"][j]), j
    for c, j in zip(cls, rec):
        for q, k in ((1, "heterozygotes"), (2, "homozygotes"), (3, "missingGenos")):
            assert (";".join(names[s] for s in np.flatnonzero(c == q)) or "!") == rows[j][col[k]], (j, k)
