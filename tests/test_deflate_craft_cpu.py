"""The crafted DEFLATE members of test_gpu_inflate_craft.py against zlib's inflater alone (no GPU): every valid case
must inflate to the text its tokens mean, every refused and lenient case must be refused, and each case must still hold
the edge it was built for.  So a device test that fails there fails for the decoder's sake, not the case's."""
import math
import random
import struct
import zlib
from fractions import Fraction

import pytest

import deflate_craft as dc
import test_gpu_inflate_craft as craft


def inflate(pay):
    """-> (text, reached the end of the stream, bytes left over), or None if zlib refuses the stream"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(pay)
    except zlib.error:
        return None
    return text, d.eof, d.unused_data


def check_valid(c):
    m = c["member"]
    assert len(m) <= dc.MAX_MEMBER, c["name"]
    assert m[:4] == b"\x1f\x8b\x08\x04" and struct.unpack_from("<H", m, 16)[0] + 1 == len(m), c["name"]
    got = inflate(m[18:-8])
    assert got is not None and got[1], c["name"]
    assert got[0] == c["text"], c["name"]
    if "tokens" in c:
        assert bytes(dc.expand(c["tokens"])) == c["text"], c["name"]
    assert struct.unpack("<II", m[-8:]) == (zlib.crc32(c["text"]), len(c["text"])), c["name"]


def matches(tokens):
    """(pos mod 4, length, distance) of every match"""
    out, pos = [], 0
    for t in tokens:
        if isinstance(t, int):
            pos += 1
        elif isinstance(t, bytes):
            pos += len(t)
        else:
            ls, lx, ds, dx = dc.raw_of(t)
            out.append((pos & 3, dc.LEN_BASE[ls - 257] + lx, dc.DIST_BASE[ds] + dx))
            pos += out[-1][1]
    return out


@pytest.mark.parametrize("W", (0,) + craft.A_WINDOWS)
def test_match_placement_cases(W):
    cases = craft.cases_a(W)
    for c in cases:
        check_valid(c)
        have = matches(c["tokens"])
        assert all(w in have for w in c["want"]), c["name"]
    got = {(c["kind"],) + w for c in cases for w in c["want"]}
    if W == 0:
        want = {("overlap", a, length, dist) for dist in craft.A_OVERLAP_DISTS for length in {max(3, dist + 1), 64, 65, 258} for a in range(4)}
        assert got == want and len(cases) == 41
        return
    # the list is what it says: every length at every alignment, at and around the window's edge
    for length in craft.A_LENS:
        for a in range(4):
            for d in (-1, 0, 1):
                assert ("sum%+d" % d, a, length, W + d - length) in got
                assert W + d > 32768 or ("dist%+d" % d, a, length, W + d) in got
    for s in range(1, 6):
        for length in (4, 65, 258):
            for a in range(4):
                assert W - length + s > 32768 or ("oldest+%d" % s, a, length, W - length + s) in got
    seg = W // 2
    starts = {c["name"].split("pos=")[1].split()[0] for c in cases if c["kind"] == "seg_at"}
    assert starts and all(int(p) % seg == 0 for p in starts)
    for c in cases:
        if c["kind"] == "seg_cross":
            pos = int(c["name"].split("pos=")[1].split()[0])
            _, length, dist = c["want"][0]
            assert pos // seg != (pos + length - 1) // seg and pos % seg and (W == 32768 or dist + length > W), c["name"]
    if W == 32768:
        assert {int(c["name"].split("pos=")[1].split()[0]) - 32768 for c in cases if c["kind"] == "dist32768"} >= {0, 1, 2, 3}
        assert all(c["want"][0][2] == 32768 for c in cases if c["kind"] == "dist32768")
    assert len(cases) == {4096: 286, 16384: 286, 32768: 264}[W]


def test_code_cases():
    cases = craft.cases_b()
    for c in cases:
        check_valid(c)
    by_name = {c["name"]: c for c in cases}
    for v in range(6):  # a code of length 15 that is used
        c = by_name["lit15 v%d" % v]
        assert sorted(l for l in c["lit_lens"] if l) == list(range(1, 15)) + [15, 15]
        assert any(c["lit_lens"][s] == 15 for s in dc.symbols(c["tokens"])[0])
    assert by_name["lit15 v0"]["lit_lens"][256] == 1 and by_name["lit15 v1"]["lit_lens"][256] == 15
    for v in range(4):
        c = by_name["dist15 v%d" % v]
        assert sorted(c["dist_lens"]) == list(range(1, 15)) + [15, 15]
        assert any(c["dist_lens"][s] == 15 for s in dc.symbols(c["tokens"])[1])
    c = by_name["all length symbols"]
    assert len(c["lit_lens"]) == 286 and len(c["dist_lens"]) == 30 and all(c["lit_lens"]) and all(c["dist_lens"])
    seen = {t[1:3] for t in c["tokens"] if isinstance(t, tuple)}
    assert seen == {(ls, lx) for ls in range(257, 286) for lx in (0, (1 << dc.LEN_EXTRA[ls - 257]) - 1)}
    c = by_name["all distance symbols"]
    seen = {dc.raw_of(t)[2:] for t in c["tokens"] if isinstance(t, tuple)}
    assert seen == {(ds, dx) for ds in range(30) for dx in (0, (1 << dc.DIST_EXTRA[ds]) - 1)}
    assert len([c for c in cases if c["name"].startswith("random_code seed")]) == 64


def test_block_and_size_cases():
    for c in craft.cases_c():
        check_valid(c)
    sizes = sorted(len(c["text"]) for c in craft.cases_c())
    assert sizes.count(65535) == 3 and sizes.count(65536) == 3
    c = [c for c in craft.cases_c() if c["name"].startswith("garbage")][0]
    assert inflate(c["member"][18:-8])[2]  # zlib leaves the garbage unused
    sweep = craft.cases_sweep()
    for c in sweep:
        check_valid(c)
    assert [len(c["text"]) for c in sweep] == craft.SWEEP_SIZES and {n % 16 for n in craft.SWEEP_SIZES} == set(range(16))
    assert len(sweep[-1]["member"]) == dc.MAX_MEMBER


def test_random_members():
    for c in craft.cases_random(0, 64):
        check_valid(c)
    texts = [len(c["text"]) for c in craft.cases_random(0, 64)]
    assert max(texts) == dc.MAX_MEMBER and min(texts) < 300


def test_random_code_is_complete():
    rng = random.Random(15)
    deepest = 0
    for n in list(range(2, 40)) + [100, 257, 286] * 5:
        for max_len in (15, 7, max(1, math.ceil(math.log2(n)))):
            if n <= 1 << max_len:
                code = dc.random_code(range(n), rng, max_len)
                assert sorted(code) == list(range(n))
                assert sum(Fraction(1, 1 << l) for l in code.values()) == 1 and max(code.values()) <= max_len
                deepest = max(deepest, max(code.values()))
    assert deepest == 15


def test_refused_cases_are_refused_by_zlib():
    names = [n for n, _ in craft.cases_refuse()]
    assert len(names) == len(set(names)) == 28
    for name, m in craft.cases_refuse():
        assert len(m) <= dc.MAX_MEMBER
        crc, isize = struct.unpack("<II", m[-8:])
        got = inflate(m[18:-8])
        if name.startswith("R17"):  # the stream and ISIZE are right, only the CRC is not
            assert got[1] and len(got[0]) == isize and zlib.crc32(got[0]) != crc
        elif name.startswith(("R4", "R15 literal", "R15 match")):  # a well-formed stream of more text than ISIZE says
            assert got[1] and len(got[0]) > isize
        else:
            assert got is None or not got[1] or len(got[0]) < isize, name


def test_lenient_cases_are_refused_by_zlib():
    cases = craft.cases_lenient()
    assert len(cases) == 3
    for c in cases:
        assert inflate(c["member"][18:-8]) is None, c["name"]
        assert struct.unpack("<II", c["member"][-8:]) == (zlib.crc32(c["text"]), len(c["text"]))
    assert sum(Fraction(1, 1 << l) for l in cases[0]["dist_lens"]) == Fraction(30, 32)
    assert sum(Fraction(1, 1 << l) for l in cases[1]["lit_lens"] if l) == Fraction(3, 4)


def test_libdeflate_fixture_is_self_consistent():
    data, members = craft.fixture_members()
    assert len(members) == 29
    stored_only = 0
    for pay, crc, isize in members:
        text = craft.zlib_inflate(pay)
        assert (zlib.crc32(text), len(text)) == (crc, isize) and isize <= 65280
        stored_only += (pay[0] & 6) == 0
    assert stored_only >= 1  # the level-0 member
    import gzip
    import os
    with open(os.path.join(craft.GOLDEN, "libdeflate_cohort.vcf.gz"), "rb") as f:
        comp = f.read()
    assert gzip.decompress(comp) == craft.cohort_vcf()
    assert len(data) + len(comp) < 512 << 10


def test_pipeline_files_hold_the_cohort():
    vcf = craft.cohort_vcf()
    assert 150_000 < len(vcf) < 400_000
    for name, members in craft.pipeline_files(vcf).items():
        texts = []
        for m in members:
            assert len(m) <= dc.MAX_MEMBER
            texts.append(craft.zlib_inflate(m[18:-8]))
            assert struct.unpack("<II", m[-8:]) == (zlib.crc32(texts[-1]), len(texts[-1])), name
        assert b"".join(texts) == vcf, name
        if name == "member_sizes":
            assert {65536, 1, 0} <= {len(t) for t in texts}
