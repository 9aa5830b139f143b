"""k_deflate / k_crc32 / k_bgzf_pack (bvcf_bgzf_deflate_device) and --compressOutput bgzf: every output must inflate to
its text under zlib, this repo's device inflater and its host reader; the framing is bgzip's; the bytes depend on the
text only; the CLI's compressed stream is its plain output, compressed."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

import bgzf
import vcfgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
PIECE = 65280
HDR = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def _cli(args, data):
    return subprocess.run([EXE] + args, input=data, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def cohort_vcf():
    return vcfgen.gen_vcf(501, 4000, 600, weird=0.01)


@pytest.fixture(scope="module")
def cohort_tsv(cohort_vcf):
    p = _cli([], cohort_vcf)
    assert p.returncode == 0, p.stderr[-300:]
    assert len(p.stdout) > 2 << 20
    return p.stdout


@pytest.fixture(scope="module")
def golden_tsv():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "1kg_chr1_20klines.expected.tsv.gz"), "rb") as f:
        return f.read()


def _members(out):
    """the members of a BGZF stream, by bvcf_bgzf.h's rules: (header, payload, crc, isize, total)"""
    ms, pos = [], 0
    while pos < len(out):
        assert out[pos:pos + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", out, pos + 10)[0]
        assert xlen == 6 and out[pos + 12:pos + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", out, pos + 16)[0]
        total = bsize + 1
        assert total <= 65536 and pos + total <= len(out)
        crc, isize = struct.unpack_from("<II", out, pos + total - 8)
        ms.append((out[pos:pos + 16], out[pos + 18:pos + total - 8], crc, isize, total))
        pos += total
    assert pos == len(out)
    return ms


def _check_round_trip(bv, text, add_eof=True):
    out = bv.bgzf_deflate_device(text, add_eof=add_eof)
    assert len(out) <= bv.bgzf_bound(len(text))
    assert gzip.decompress(out) == text  # zlib is the judge
    if out:
        rc, got, _ = bv.bgzf_inflate_device(out)
        assert rc == 0 and got == text  # this repo's inflater
        rc, got, kind = bv.decompress(out)
        assert rc == 0 and got == text  # the driver's host reader
    ms = _members(out)
    body = ms[:-1] if add_eof else ms
    if add_eof:
        assert out[-28:] == bv.BGZF_EOF and ms[-1][3] == 0
    assert len(body) == (len(text) + PIECE - 1) // PIECE
    for i, (h, pay, crc, isize, total) in enumerate(body):
        assert h == HDR
        assert isize == (PIECE if i + 1 < len(body) else len(text) - PIECE * i)
        assert crc == zlib.crc32(text[i * PIECE:i * PIECE + isize]) & 0xFFFFFFFF
        assert total <= 65311
    return out


def _far_only():
    rng = random.Random(3)
    a = bytes(rng.getrandbits(8) for _ in range(32100))
    return a + bytes(rng.getrandbits(8) for _ in range(600)) + a[:30000]  # matches 32 100 .. 32 700 bytes back


def _de_bruijn4():
    # every 4-byte string over ACGT exactly once: no 4-byte repeat, yet 2 bits a byte under Huffman codes
    a, seq = [0] * 20, []

    def f(t, p):
        if t > 4:
            if 4 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            f(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                f(t + 1, t)
    f(1, 1)
    s = bytes(b"ACGT"[i] for i in seq)
    return s + s[:3]


@pytest.mark.parametrize("name", ["empty", "one", "p65279", "p65280", "p65281", "random", "one_byte_1MiB", "far_only",
                                  "no_repeat", "crlf", "golden_head"])
def test_round_trip(bv, golden_tsv, name):
    text = {
        "empty": lambda: b"",
        "one": lambda: b"x",
        "p65279": lambda: golden_tsv[:65279],
        "p65280": lambda: golden_tsv[:65280],
        "p65281": lambda: golden_tsv[:65281],
        "random": lambda: os.urandom(200000),
        "one_byte_1MiB": lambda: b"\t" * (1 << 20),
        "far_only": _far_only,
        "no_repeat": _de_bruijn4,
        "crlf": lambda: golden_tsv[:300000].replace(b"\n", b"\r\n"),
        "golden_head": lambda: golden_tsv[:3000000],
    }[name]()
    for eof in (True, False):
        out = _check_round_trip(bv, text, eof)
    if name == "random":
        assert len(out) == len(text) + 31 * 4  # four stored members: never beyond the stored size
    if name == "no_repeat":
        assert len(out) < len(text)  # a literal-only dynamic block (the distance tree's two-code corner)


def test_round_trip_cohort_and_golden(bv, cohort_tsv, golden_tsv):
    _check_round_trip(bv, cohort_tsv)
    _check_round_trip(bv, golden_tsv)


def test_deterministic_per_piece(bv, golden_tsv):
    text = golden_tsv[:PIECE * 40 + 1234]
    a = bv.bgzf_deflate_device(text)
    assert bv.bgzf_deflate_device(text) == a
    ma = _members(a)
    # a different concatenation: the same pieces (whole-piece offsets) give the same members
    b = bv.bgzf_deflate_device(golden_tsv[PIECE * 7:PIECE * 19] + golden_tsv[:PIECE * 3], add_eof=False)
    mb = _members(b)
    assert [m[:4] for m in mb[:12]] == [m[:4] for m in ma[7:19]]
    assert [m[:4] for m in mb[12:]] == [m[:4] for m in ma[:3]]


def _zlib_pieces(text, level):
    n = 0
    for i in range(0, len(text), PIECE):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        n += len(c.compress(text[i:i + PIECE]) + c.flush()) + 26
    return n


def test_ratio_against_zlib_level1(bv, cohort_tsv, golden_tsv):
    for text in (golden_tsv, cohort_tsv):
        ours = len(bv.bgzf_deflate_device(text, add_eof=False))
        z1 = _zlib_pieces(text, 1)
        assert ours <= 1.15 * z1, (ours, z1, _zlib_pieces(text, 6))


def _plain_and_bgzf(bv, args, data):
    p = _cli(args, data)
    q = _cli(args + ["--compressOutput", "bgzf"], data)
    assert p.returncode == 0 and q.returncode == 0, (p.stderr[-300:], q.stderr[-300:])
    assert gzip.decompress(q.stdout) == p.stdout
    assert q.stdout == bv.bgzf_deflate_device(p.stdout, add_eof=True)
    assert q.stdout.endswith(bv.BGZF_EOF)
    return q.stdout


def test_cli_golden_1kg(bv, golden_1kg):
    _plain_and_bgzf(bv, [], golden_1kg[0])


def test_cli_same_bytes_for_devices_batches_and_input_kinds(bv, cohort_vcf, tmp_path):
    outs = [_plain_and_bgzf(bv, [], cohort_vcf)]
    outs.append(_plain_and_bgzf(bv, ["--devices", "0"], cohort_vcf))
    outs.append(_plain_and_bgzf(bv, ["--devices", "0,0"], cohort_vcf))
    outs.append(_plain_and_bgzf(bv, ["--batchMB", "1"], cohort_vcf))
    gz = bgzf.bgzf_compress(cohort_vcf)
    outs.append(_plain_and_bgzf(bv, [], gz))  # BGZF through stdin
    f = tmp_path / "in.vcf.gz"
    f.write_bytes(gz)
    outs.append(_plain_and_bgzf(bv, ["--in", str(f)], b""))  # BGZF file: inflated on the device
    assert all(o == outs[0] for o in outs)


def test_cli_sites_only_flags_and_header_only(bv):
    sites = vcfgen.gen_vcf(77, 3000, 0, weird=0.02)
    _plain_and_bgzf(bv, [], sites)  # device-rendered rows
    cohort = vcfgen.gen_vcf(78, 300, 40, weird=0.02)
    _plain_and_bgzf(bv, ["--keepId", "--keepInfo", "--keepPos"], cohort)
    out = _plain_and_bgzf(bv, [], vcfgen.header(5).encode())
    assert len(_members(out)) == 2  # the header line's member + EOF


def test_cli_out_path_and_no_out(bv, cohort_vcf, tmp_path):
    o = tmp_path / "new.tsv.gz"
    p = _cli(["--out", str(o), "--compressOutput", "bgzf"], cohort_vcf)
    assert p.returncode == 0 and p.stdout == b""
    plain = _cli([], cohort_vcf).stdout
    assert o.read_bytes() == bv.bgzf_deflate_device(plain)
    d1, d2 = tmp_path / "a.arrow", tmp_path / "b.arrow"
    p1 = _cli(["--noOut", "--dosageOutput", str(d1)], cohort_vcf)
    p2 = _cli(["--noOut", "--dosageOutput", str(d2), "--compressOutput", "bgzf"], cohort_vcf)
    assert p1.returncode == 0 and p2.returncode == 0
    assert p2.stdout == b"" and d1.read_bytes() == d2.read_bytes()
