"""Every side output in one run, three ways: bvcf_run_buffer, the CLI on one worker and the CLI on two, over the input of
test_gpu_arena_growth_together (1 MiB batches, one of which outruns the arenas: the drivers regrow with run tables to carry).

To that test's outputs (--plinkOutput, --mendel / --mendelErrors, --ld / --ldPrune, --sampleStats, --relatedness) this adds
--grm, --pca, --score over a third of the loci, --pheno / --covar / --assoc, --dosageOutput and the three filter reports with
gates that drop rows (--maxMissing, --excludeVariants, --excludeRegions).

What the files hold is the business of each analysis's own suite, which compares it with a model.  This test pins the bytes:
the sha256 of every output file and of the TSV, per way, as golden/make_outputs_together.py recorded them
(golden/outputs_together.json) -- so the one open / per-batch / finish path of the outputs cannot change a byte of any of
them on either driver unnoticed."""
import hashlib
import json
import os
import subprocess

import pytest

import assoc
import assoc_cov as ac
import oracle_lib as orc
import score as sc
import variantlist as vl
from test_gpu_arena_growth_together import BATCH, R2, WINDOW, build_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN = os.path.join(ROOT, "tests", "golden", "outputs_together.json")
WAYS = {"run_buffer": None, "cli_one_worker": "0", "cli_two_workers": "0,0"}


def write_inputs(d):
    """the VCF and the files the analyses read, under d -> (vcf, the options that name them and set the gates)"""
    vcf, fam = build_input()
    rc, body, _, _ = orc.run(vcf)
    assert rc == 0
    loci = vl.loci_of(body)
    chrom, pos = loci[len(loci) // 4].split(b":")[:2]
    files = {"in.vcf": vcf, "ped": fam, "weights": sc.file_text(sc.entries_for(loci, 3, 7710, frac=0.33), [b"a", b"b", b"c"]),
             "pheno": assoc.pheno_for(vcf, 2, 7711), "covar": ac.covar_for(vcf, 2, 7712), "drop.loci": vl.list_text(loci[5::11])}
    for name, data in files.items():
        (d / name).write_bytes(data)
    opts = {"fam": d / "ped", "score": d / "weights", "pheno": d / "pheno", "covar": d / "covar", "excludeVariants": d / "drop.loci",
            "excludeRegions": "%s:%d-%d" % (chrom.decode(), int(pos), int(pos) + 500), "maxMissing": 0.2, "ldWindow": WINDOW, "ldR2": R2}
    return vcf, opts


def outputs_in(d):
    """every output flag, its file (or prefix) in d"""
    files = {"sampleStats": "stats", "relatedness": "pairs", "siteFilterReport": "site.report", "variantFilterReport": "variant.report",
             "regionFilterReport": "region.report", "plinkOutput": "plink", "mendel": "mendel", "mendelErrors": "mendel.errors", "ld": "ld",
             "ldPrune": "ld", "grm": "m", "pca": "m", "pcaReport": "pca.report", "scoreOutput": "scores", "scoreReport": "scores.report",
             "assoc": "scan", "assocReport": "scan.report", "dosageOutput": "dosage"}
    return {k: d / v for k, v in files.items()}


def digests_of(d, tsv):
    out = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(d.iterdir())}
    out["the TSV"] = hashlib.sha256(tsv).hexdigest()
    return out


def run_way(bv, way, vcf, opts, d):
    """one run with every output in the (new) directory d -> {file name: sha256}"""
    d.mkdir()
    cfg = {k: str(v) if isinstance(v, os.PathLike) else v for k, v in list(opts.items()) + list(outputs_in(d).items())}
    if WAYS[way] is None:
        rc, tsv, log, _ = bv.run_buffer(vcf, cfg, max_batch_bytes=BATCH)
        assert rc == 0, log
    else:
        args = [EXE, "--in", cfg.pop("in"), "--batchMB", str(BATCH >> 20), "--devices", WAYS[way]]
        for k, v in cfg.items():
            args += ["--" + k, str(v)]
        p = subprocess.run(args, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-400:]
        tsv = p.stdout.split(b"\n", 1)[1]
    return digests_of(d, tsv)


def run_three_ways(bv, d):
    """-> {way: {file name: sha256}} (the recorder's entry point too)"""
    (d / "inputs").mkdir()
    vcf, opts = write_inputs(d / "inputs")
    got = {}
    for way in WAYS:
        o = dict(opts)
        if WAYS[way] is not None:
            o["in"] = d / "inputs" / "in.vcf"
        got[way] = run_way(bv, way, vcf, o, d / way)
    return got


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    import bystro_vcf_amd as bv
    return run_three_ways(bv, tmp_path_factory.mktemp("together"))


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("way", list(WAYS))
def test_every_output_byte_for_byte(got, want, way):
    assert sorted(got[way]) == sorted(want[way]) and len(want[way]) >= 25  # (24 files of 18 flags, and the TSV)
    differ = [name for name in want[way] if got[way][name] != want[way][name]]
    assert not differ, differ
