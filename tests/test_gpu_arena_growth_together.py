"""The three arenas of the row analyses growing in one run: --plinkOutput (the .bed rows), --mendel / --mendelErrors (the trio
events) and --ld / --ldPrune (the pair events) together with --sampleStats and --relatedness, over a file of several
batches of 1 MiB in which one batch outruns all three starting bounds.

bvcf_run_buffer takes the grow path of process_block; the CLI takes the driver's, with batches in flight to drain and to
submit again, on one worker and on two.  Every output must be what the oracle's TSV of the same bytes implies, byte for
byte (plinkbed, mendel, ldpairs, the --sampleStats table, pairtable): the two tables show that the totals carried over the
drain are neither lost nor counted twice."""
import os
import subprocess

import pytest

import ldpairs as lp
import mendel as md
import oracle_lib as orc
import pairtable as pt
import plinkbed as pb
from test_gpu_sample_stats import table_from_tsv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")

NS, N_TRIOS = 39, 6  # rows of 10 bytes
# at a threshold of 0 every pair of varying rows in a window is an event, and a line of the --ld table; the window is short
# because the batch that outruns the arenas has 29 000 rows (87 000 events: five times the arena's starting bound)
WINDOW, R2, T6 = 3, "0", 0
BATCH = 1 << 20
PAD = 1900  # bytes of INFO per cohort line: 1 200 lines are 2.4 MB, the batches hold some 500 of them


def data_lines(vcf):
    return vcf[vcf.index(b"\n", vcf.index(b"#CHROM")) + 1:].split(b"\n")[:-1]


def padded(line, k):
    f = line.split(b"\t")
    f[7] = b"PAD=" + bytes(65 + (k + j) % 26 for j in range(PAD))
    return b"\t".join(f)


def build_input():
    """-> (vcf, fam): 600 pedigree lines and 600 lines with LD between neighbours, their INFO padded so that the file is
    several batches, and in the middle of them 145 lines of 201 ALT rows each (test_gpu_plink's growth case): some 29 000
    rows from 70 KB of text, which land in one batch"""
    ped_vcf, trios = md.pedigree_vcf(NS, N_TRIOS, 600, 9910, flip=0.1, miss=0.03)
    cohort = [padded(x, k) for k, x in enumerate(data_lines(ped_vcf))]
    ld = [padded(x, k) for k, x in enumerate(data_lines(lp.ld_vcf(7610, NS, 600)))]
    alts = data_lines(pb.many_alts_vcf(ns=NS, n_lines=145, seed=8710))
    head = ped_vcf[:ped_vcf.index(b"\n", ped_vcf.index(b"#CHROM")) + 1]
    lines = cohort[:300] + ld[:300] + alts + cohort[300:] + ld[300:]
    vcf = head + b"".join(x + b"\n" for x in lines)
    return vcf, md.fam_of(trios, pt.sample_names(vcf))


def batches_of(vcf):
    """the data lines as bvcf_run_buffer cuts them: whole lines, at most BATCH bytes"""
    at = vcf.index(b"\n", vcf.index(b"#CHROM")) + 1
    head, out = vcf[:at], []
    while at < len(vcf):
        end = min(len(vcf), at + BATCH)
        end = vcf.rindex(b"\n", at, end) + 1
        out.append(head + vcf[at:end])
        at = end
    return out


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def make_case(bv):
    """the input, what every output must be, and -- on the oracle's side, before anything touches the device -- that the run
    is what this test is about: several batches, and each arena outrun by some batch"""
    vcf, fam = build_input()
    names = pt.sample_names(vcf)
    rc, body, log, _ = orc.run(vcf)
    assert rc == 0
    want = {"body": body, "log": log, "plink": pb.expected_from_body(body, names), "mendel": md.expected_from_body(body, names, fam),
            "ld": lp.expected_from_body(body, names, WINDOW, T6), "stats": table_from_tsv(bv, body, names), "pairs": pt.file_text(pt.tables(*pt.matrices(body, names)), names)}
    batches = batches_of(vcf)
    assert len(batches) >= 3
    need_bed, need_trio, need_ld, row0 = [], [], [], 0
    for b in batches:
        rc_b, body_b, _, _ = orc.run(b)
        assert rc_b == 0
        n_rows = body_b.count(b"\n")
        need_bed.append(n_rows * pb.row_bytes(NS))
        need_trio.append(len(md.expected_from_body(body_b, names, fam, with_errors_text=False)["events"]))
        need_ld.append(len(lp.batch_events(want["ld"]["events"], row0, row0 + n_rows)))
        row0 += n_rows
    assert row0 == body.count(b"\n")
    assert max(need_bed) > BATCH // 4, need_bed
    assert max(need_trio) > max(BATCH // 64, 1024), need_trio
    assert max(need_ld) > max(BATCH // 64, 1024), need_ld
    # (not the first batch: the totals of --sampleStats and --relatedness hold earlier batches when the driver drains)
    assert need_bed.index(max(need_bed)) > 0
    return vcf, fam, want


@pytest.fixture(scope="module")
def case(bv):
    return make_case(bv)


def first_diff(g, w):
    n = min(len(g), len(w))
    at = next((i for i in range(n) if g[i] != w[i]), n)
    return "%d vs %d bytes, first difference at byte %d: got %r want %r" % (len(g), len(w), at, g[at:at + 40], w[at:at + 40])


def same(what, got, want):
    assert got == want, what + ": " + first_diff(got, want)


def outputs(d, tag):
    """(the pedigree is TAG.ped: TAG.fam is the fileset's)"""
    return {k: d / ("%s.%s" % (tag, k)) for k in ("ped", "mendel", "errors", "ld", "stats", "pairs")}


def check_files(d, tag, want):
    f = outputs(d, tag)
    got = pb.read_files(d / tag)
    assert not pb.diff(got, want["plink"]), pb.diff(got, want["plink"])
    same("--mendel", f["mendel"].read_bytes(), want["mendel"]["mendel"])
    same("--mendelErrors", f["errors"].read_bytes(), want["mendel"]["errors"])
    same("--ld", f["ld"].read_bytes(), want["ld"]["table"])
    same(".prune.in", (d / (tag + ".prune.in")).read_bytes(), want["ld"]["prune_in"])
    same(".prune.out", (d / (tag + ".prune.out")).read_bytes(), want["ld"]["prune_out"])
    same("--sampleStats", f["stats"].read_bytes(), want["stats"])
    same("--relatedness", f["pairs"].read_bytes(), want["pairs"])


def test_run_buffer(bv, case, tmp_path):
    vcf, fam, want = case
    f = outputs(tmp_path, "b")
    f["ped"].write_bytes(fam)
    cfg = {"plinkOutput": str(tmp_path / "b"), "fam": str(f["ped"]), "mendel": str(f["mendel"]), "mendelErrors": str(f["errors"]),
           "ld": str(f["ld"]), "ldPrune": str(tmp_path / "b"), "ldWindow": WINDOW, "ldR2": R2, "sampleStats": str(f["stats"]),
           "relatedness": str(f["pairs"])}
    rc, out, log, _ = bv.run_buffer(vcf, cfg, max_batch_bytes=BATCH)
    assert rc == 0, log
    same("the TSV", out, want["body"])
    assert log == want["log"]
    check_files(tmp_path, "b", want)


@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_cli(case, tmp_path, devices):
    vcf, fam, want = case
    src = tmp_path / "in.vcf"
    src.write_bytes(vcf)
    f = outputs(tmp_path, "c")
    f["ped"].write_bytes(fam)
    p = subprocess.run([EXE, "--in", str(src), "--batchMB", "1", "--devices", devices, "--plinkOutput", str(tmp_path / "c"),
                        "--fam", str(f["ped"]), "--mendel", str(f["mendel"]), "--mendelErrors", str(f["errors"]), "--ld", str(f["ld"]),
                        "--ldPrune", str(tmp_path / "c"), "--ldWindow", str(WINDOW), "--ldR2", R2, "--sampleStats", str(f["stats"]),
                        "--relatedness", str(f["pairs"])], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-400:]
    same("the TSV", p.stdout.split(b"\n", 1)[1], want["body"])
    check_files(tmp_path, "c", want)
