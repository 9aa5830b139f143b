"""--pca on the device: bvcf_pca_eigen over every matrix family against numpy.linalg.eigh within the bounds of pca.py (which
come from the numpy model of the algorithm, never from the device's results), the sign rule, repeatability; a poisoned run;
the files through bvcf_run_buffer and the CLI against the oracle's matrix; byte-identity across input kinds, batch sizes and
device lists; no effect on any other output; composition and edge cases."""
import ctypes as C
import gzip
import hashlib
import os
import subprocess

import numpy as np
import pytest

import bgzf
import grm
import oracle_lib as orc
import pairtable as pt
import pca
import samplecut
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
GOLDEN_GZ = os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.vcf.gz")
GRM_SUFFIXES = (".grm.bin", ".grm.N.bin", ".grm.id")
# a file number against its reference: "%.6G" steps by at most 5e-6 relative around a value; room on top
FILE_RTOL, FILE_FLOOR = 1e-5, 1e-3


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def check_pairs(A, vals, vecs, tag):
    """the three bounds, the sign rule, finiteness, unit norm"""
    assert np.isfinite(vals).all() and np.isfinite(vecs).all(), tag
    assert np.all(np.diff(vals) <= 0), tag
    r = pca.ratios(A, vals, vecs)
    print(tag, "residual %.3f eigenvalue %.3f orthonormality %.3f" % r)
    assert r[0] <= pca.BOUND_RES and r[1] <= pca.BOUND_VAL and r[2] <= pca.BOUND_ORTH, (tag, r)
    assert all(pca.sign_rule_holds(v) for v in vecs), tag
    return r


# ---- 1. the solver alone

@pytest.mark.parametrize("n", pca.GPU_SIZES)
@pytest.mark.parametrize("fam", pca.FAMILIES)
def test_eigen_families(bv, fam, n):
    A = pca.family(fam, n)
    lower = pca.lower_f32(A)
    for k in pca.ks_of(n):
        vals, vecs = bv.pca_eigen(lower, n, k)
        check_pairs(A, vals, vecs, "%s n=%d k=%d" % (fam, n, k))
    v2, u2 = bv.pca_eigen(lower, n, k)
    assert vals.tobytes() == v2.tobytes() and vecs.tobytes() == u2.tobytes(), "two calls, two answers"


def test_eigen_zero_matrix_is_finite_and_orthonormal(bv):
    vals, vecs = bv.pca_eigen(np.zeros(10 * 11 // 2, dtype=np.float32), 10, 4)
    assert not vals.any() and np.array_equal(vecs, np.eye(10)[:4])


def test_eigen_two_by_two_with_equal_magnitudes(bv):
    """[[0, 1], [1, 0]]: the vectors are (1, 1) / sqrt 2 and (1, -1) / sqrt 2 up to the sign the rule picks -- the larger
    magnitude positive, the first one where the two are the same number"""
    vals, vecs = bv.pca_eigen(np.array([0.0, 1.0, 0.0], dtype=np.float32), 2, 2)
    assert np.allclose(vals, [1.0, -1.0], atol=4 * pca.EPS)
    assert np.allclose(np.abs(vecs), 0.5 ** 0.5, atol=8 * pca.EPS)
    assert vecs[0][0] > 0 and vecs[0][1] > 0 and vecs[1][0] * vecs[1][1] < 0
    assert all(pca.sign_rule_holds(v) for v in vecs)


def test_eigen_refusals(bv):
    A = pca.family("grm", 100)
    lower = pca.lower_f32(A)
    for k in (0, 101, 65):
        with pytest.raises(bv.BvcfError) as ei:
            bv.pca_eigen(lower, 100, k)
        assert ei.value.rc == bv.E_ARG and "components" in str(ei.value)
    for bad in (np.nan, np.inf, -np.inf):
        x = lower.copy()
        x[777] = bad
        with pytest.raises(bv.BvcfError) as ei:
            bv.pca_eigen(x, 100, 3)
        assert ei.value.rc == bv.E_ARG and "777" in str(ei.value)
    # one sample too many: refused before the matrix is looked at
    fn = bv.lib.bvcf_pca_eigen
    fn.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    err = C.create_string_buffer(256)
    out = np.zeros(16)
    assert fn(0, lower.ctypes.data, bv.PAIR_MAX_SAMPLES + 1, 1, out.ctypes.data, out.ctypes.data, err, len(err)) == bv.E_ARG
    assert b"8193" in err.value
    # no samples: nothing to do
    assert fn(0, None, 0, 0, None, None, err, len(err)) == 0 and err.value == b""
    assert fn(0, None, 0, 5, None, None, None, 0) == 0


# ---- 2. poisoned allocations

def test_poisoned_allocations(bv, monkeypatch):
    """BVCF_POISON: every fresh buffer filled with 0xa5 and held between guards -- nothing is read before it is written
    (the answer is the unpoisoned one), nothing written outside its buffer"""
    A = pca.family("grm", 257)
    lower = pca.lower_f32(A)
    want = bv.pca_eigen(lower, 257, 10)
    monkeypatch.setenv("BVCF_POISON", "a5")
    bv.guard_check()
    got = bv.pca_eigen(lower, 257, 10)
    n, msg = bv.guard_check()
    assert n == 0, "%d buffer(s) written out of bounds, the first: %s" % (n, msg)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    check_pairs(A, got[0], got[1], "poisoned")


# ---- 3. end to end

def cli(args, stdin_bytes=None, timeout=120, env=None):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=timeout, env=env)


def read_pca(prefix):
    out = []
    for sfx in (".eigenvec", ".eigenval"):
        with open(str(prefix) + sfx, "rb") as f:
            out.append(f.read())
    return tuple(out)


def read_grm(prefix):
    return tuple(open(str(prefix) + sfx, "rb").read() for sfx in GRM_SUFFIXES)


def matrix_of_bin(data, ns):
    return pca.from_lower(np.frombuffer(data, dtype="<f4"), ns)


def reference_pairs(A, k):
    """numpy's k largest pairs with the sign rule, after the gap condition: lambda_1 .. lambda_k and lambda_{k+1} pairwise at
    least 0.01 lambda_1 apart, so that a vector moves by at most 4 u / gap, far below the files' print step"""
    assert pca.gap_ratio(A, k) >= 0.01, "the cohort's leading eigenvalues do not stand apart"
    w, v = np.linalg.eigh(A)
    vals = w[::-1][:k]
    vecs = np.array([pca.apply_sign_rule(v[:, -1 - a]) for a in range(k)])
    return vals, vecs


def close(x, ref):
    return np.all(np.abs(np.asarray(x) - np.asarray(ref)) <= FILE_RTOL * np.maximum(np.abs(ref), FILE_FLOOR))


def check_files(files, names, vals, vecs, k):
    head, got_names, table, texts = pca.parse_eigenvec(files[0])
    assert head == "#FID\tIID" + "".join("\tPC%d" % (c + 1) for c in range(k))
    assert got_names == [(nm, nm) for nm in names]
    got_vals, val_texts = pca.parse_eigenval(files[1])
    assert len(got_vals) == k and table.shape == (len(names), k)
    assert close(got_vals, vals), (got_vals, vals)
    assert close(table, vecs.T), float(np.abs(table - vecs.T).max())
    for t in [x for row in texts for x in row] + val_texts:  # "%.6G", a zero as "0"
        assert t == "0" or (float(t) != 0 and t == "%.6G" % float(t)), t


STRUCTURED = [(24, 300), (70, 400), (300, 500)]


@pytest.fixture(scope="module")
def structured():
    """{(ns, lines): (vcf, names, A, TSV body)}: the cohort, its float32 matrix from the oracle's TSV, made once"""
    out = {}
    for ns, n_lines in STRUCTURED:
        vcf = pca.structured_vcf(ns, n_lines, 4, seed=ns)
        (T, MM, N), files, body, _ = grm.expected(orc.run, vcf)
        A = matrix_of_bin(files[0], ns)
        A.setflags(write=False)
        out[(ns, n_lines)] = (vcf, pt.sample_names(vcf), A, body, N, files)
    return out


@pytest.mark.parametrize("shape", STRUCTURED)
def test_end_to_end_ctx_and_cli(bv, structured, tmp_path, shape):
    vcf, names, A, body, n_rows, grm_files = structured[shape]
    vals, vecs = reference_pairs(A, 3)
    # bvcf_run_buffer
    prefix, rep = str(tmp_path / "b"), str(tmp_path / "b.report")
    rc, out, log, _ = bv.run_buffer(vcf, {"pca": prefix, "pcaCount": 3, "pcaReport": rep})
    assert rc == 0, log
    assert out == body
    check_files(read_pca(prefix), names, vals, vecs, 3)
    report = pca.parse_report(open(rep, "rb").read())
    assert list(report) == ["samples", "rows", "components", "trace"]
    assert (report["samples"], report["rows"], report["components"]) == (str(len(names)), str(n_rows), "3")
    trace = 0.0
    for x in np.diag(A):
        trace += float(x)
    assert report["trace"] == "%.6G" % trace
    # the CLI, with the matrix beside it
    p = cli(["--pca", str(tmp_path / "c"), "--pcaCount", "3", "--grm", str(tmp_path / "c")], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout.split(b"\n", 1)[1] == body
    assert read_pca(tmp_path / "c") == read_pca(prefix), "the CLI and bvcf_run_buffer write the same bytes"
    assert read_grm(tmp_path / "c") == grm_files


def test_golden_slice_three_components(bv, tmp_path):
    """the 1000-Genomes slice, 2 504 samples: three PCs of the matrix --grm writes, within the bounds; the files hold them"""
    p = cli(["--in", GOLDEN_GZ, "--noOut", "--grm", str(tmp_path / "g"), "--pca", str(tmp_path / "g"), "--pcaCount", "3"], timeout=300)
    assert p.returncode == 0, p.stderr[-400:]
    data = read_grm(tmp_path / "g")[0]
    ns = 2504
    lower = np.frombuffer(data, dtype="<f4")
    A = pca.from_lower(lower, ns)
    vals, vecs = bv.pca_eigen(lower, ns, 3)
    check_pairs(A, vals, vecs, "golden")
    names = [ln.split("\t")[0] for ln in read_grm(tmp_path / "g")[2].decode().splitlines()]
    check_files(read_pca(tmp_path / "g"), names, vals, vecs, 3)


# ---- 4. byte-identity across run configurations

@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("pca")
    vcf = pca.structured_vcf(300, 3000, 4, seed=5)
    paths = {"text": d / "c.vcf", "gz": d / "c.vcf.gz", "bgzf": d / "c.bgz.vcf.gz"}
    paths["text"].write_bytes(vcf)
    paths["gz"].write_bytes(gzip.compress(vcf, 1))
    paths["bgzf"].write_bytes(bgzf.bgzf_compress(vcf))
    return vcf, paths, d


def test_cli_inputs_devices_and_batches_agree(bv, cohort):
    vcf, paths, d = cohort
    assert len(vcf) > 3 << 20, "--batchMB 1 cuts it into several batches"
    two = "0,1" if bv.lib.bvcf_device_count() >= 2 else "0,0"
    runs = [("text", ["--in", str(paths["text"])], None), ("gzip", ["--in", str(paths["gz"])], None),
            ("bgzf", ["--in", str(paths["bgzf"])], None), ("pipe", [], vcf),
            ("two", ["--in", str(paths["text"]), "--devices", two], None),
            ("batch1", ["--in", str(paths["text"]), "--batchMB", "1"], None),
            ("bgzf-batch1-two", ["--in", str(paths["bgzf"]), "--batchMB", "1", "--devices", two], None)]
    want = None
    for tag, args, stdin in runs:
        p = cli(args + ["--noOut", "--pca", str(d / tag), "--pcaCount", "5", "--pcaReport", str(d / (tag + ".rep"))], stdin)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        got = read_pca(d / tag) + ((d / (tag + ".rep")).read_bytes(),)
        want = want or got
        assert got == want, tag
    head, names, table, _ = pca.parse_eigenvec(want[0])
    assert table.shape == (300, 5) and np.abs(np.linalg.norm(table, axis=0) - 1.0).max() < 1e-4


# ---- 5. no effect on other outputs

def test_cli_other_outputs_unchanged(bv, cohort):
    vcf, paths, d = cohort
    outs = {}
    for tag, extra in (("plain", []), ("pca", ["--pca", str(d / "o"), "--pcaReport", str(d / "o.rep")]), ("count", ["--pcaCount", "7"])):
        tsv, dos, smp, sst, prs = (d / ("%s.%s" % (tag, x)) for x in ("tsv.gz", "arrow", "samples", "stats", "pairs"))
        p = cli(["--in", str(paths["bgzf"]), "--out", str(tsv), "--compressOutput", "bgzf", "--dosageOutput", str(dos),
                 "--sample", str(smp), "--sampleStats", str(sst), "--relatedness", str(prs), "--plinkOutput", str(d / tag),
                 "--grm", str(d / tag)] + extra)
        assert p.returncode == 0, (tag, p.stderr[-400:])
        made = [tsv, dos, smp, sst, prs] + [d / (tag + x) for x in (".bed", ".bim", ".fam") + GRM_SUFFIXES]
        outs[tag] = tuple(hashlib.sha256(f.read_bytes()).hexdigest() for f in made) + (p.stderr,)
    assert outs["plain"] == outs["pca"], "--pca changed another output"
    assert outs["plain"] == outs["count"], "--pcaCount alone does nothing"
    assert not os.path.exists(str(d / "count.eigenvec"))
    assert len(read_pca(d / "o")[1].splitlines()) == 10, "ten components by default"


def test_cli_no_out_pca_only_pass(bv, cohort):
    vcf, paths, d = cohort
    p = cli(["--in", str(paths["text"]), "--out", str(d / "with.tsv"), "--pca", str(d / "with")])
    assert p.returncode == 0, p.stderr[-400:]
    p = cli(["--in", str(paths["text"]), "--noOut", "--pca", str(d / "noout")])
    assert p.returncode == 0, p.stderr[-400:]
    assert p.stdout == b""
    assert read_pca(d / "noout") == read_pca(d / "with")
    assert not os.path.exists(str(d / "noout.grm.bin")), "--pca alone writes no matrix"


# ---- 6. composition and edge cases

def test_keep_samples_composes(bv, structured, tmp_path):
    """the components are those of the kept samples' matrix: the matrix --grm writes under the same selection"""
    vcf, names, _, _, _, _ = structured[(70, 400)]
    idx = [i for i in range(70) if i % 7]
    lst = samplecut.list_file(tmp_path / "keep.txt", vcf[:vcf.index(b"\n", vcf.index(b"#CHROM")) + 1], idx)
    p = cli(["--noOut", "--keepSamples", lst, "--grm", str(tmp_path / "k"), "--pca", str(tmp_path / "k"), "--pcaCount", "3"], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    A = matrix_of_bin(read_grm(tmp_path / "k")[0], len(idx))
    vals, vecs = reference_pairs(A, 3)
    check_files(read_pca(tmp_path / "k"), [names[i] for i in idx], vals, vecs, 3)


def test_count_is_clipped_to_the_samples(bv, structured, tmp_path):
    vcf, names, A, _, _, _ = structured[(24, 300)]
    p = cli(["--noOut", "--pca", str(tmp_path / "m"), "--pcaCount", "64", "--pcaReport", str(tmp_path / "m.rep")], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    files = read_pca(tmp_path / "m")
    head, got_names, table, _ = pca.parse_eigenvec(files[0])
    assert head.split("\t")[-1] == "PC24" and table.shape == (24, 24) and got_names == [(nm, nm) for nm in names]
    got_vals, _ = pca.parse_eigenval(files[1])
    assert close(got_vals, np.linalg.eigvalsh(A)[::-1])
    assert np.abs(table.T @ table - np.eye(24)).max() < 1e-4
    assert pca.parse_report((tmp_path / "m.rep").read_bytes())["components"] == "24"


def test_one_sample(bv, tmp_path):
    vcf = pca.structured_vcf(1, 40, 1, seed=9)
    p = cli(["--noOut", "--grm", str(tmp_path / "s"), "--pca", str(tmp_path / "s"), "--pcaReport", str(tmp_path / "s.rep")], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    a = float(np.frombuffer(read_grm(tmp_path / "s")[0], dtype="<f4")[0])
    vec, val = read_pca(tmp_path / "s")
    one = "0" if a == 0 else "%.6G" % a
    assert vec == b"#FID\tIID\tPC1\nS00000\tS00000\t1\n" and val == (one + "\n").encode()
    rep = pca.parse_report((tmp_path / "s.rep").read_bytes())
    assert (rep["samples"], rep["components"], rep["trace"]) == ("1", "1", one)


def test_no_sample_columns_and_an_unwritable_path(bv, tmp_path):
    vcf = vcfgen.gen_vcf(51, 300, 0, weird=0.02)
    p = cli(["--pca", str(tmp_path / "sites"), "--pcaReport", str(tmp_path / "sites.rep")], vcf)
    assert p.returncode == 0, p.stderr[-400:]
    assert read_pca(tmp_path / "sites") == (b"#FID\tIID\n", b"")
    assert (tmp_path / "sites.rep").read_bytes() == b"samples\t0\nrows\t0\ncomponents\t0\ntrace\t0\n"
    bad = tmp_path / "no_such_dir" / "x"
    p = cli(["--pca", str(bad)], vcf)
    assert p.returncode == 1 and str(bad).encode() in p.stderr and p.stderr.count(b"\n") == 1
    assert p.stdout == b""
    # one sample too many: one message, before anything is allocated
    ns = 8193
    wide = (vcfgen.header(ns) + "\t".join(["chr1", "100", ".", "A", "C", "50", "PASS", ".", "GT"] + ["0|1"] * ns) + "\n").encode()
    p = cli(["--pca", str(tmp_path / "wide")], wide)
    assert p.returncode == 1
    assert p.stderr.count(b"\n") == 1 and p.stderr.startswith(b"pca: 8193 samples") and b"8192" in p.stderr, p.stderr[-400:]
