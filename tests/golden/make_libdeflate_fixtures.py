"""Writes libdeflate_members.bgzf and libdeflate_cohort.vcf.gz: BGZF members whose DEFLATE streams come from libdeflate,
the encoder htslib's bgzip is normally built with (other block splits, near-optimal parses, code lengths up to 15).

Run by hand where libdeflate.so.0 is installed:  python tests/golden/make_libdeflate_fixtures.py
Never run from a test.  The expected texts are not stored: the tests inflate each payload with zlib and hold the
result against the member's own CRC-32 / ISIZE trailer."""
import ctypes as C
import gzip
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import deflate_craft as dc  # noqa: E402
import test_gpu_inflate  # noqa: E402
import test_gpu_inflate_craft as craft  # noqa: E402
import vcfgen  # noqa: E402

lib = C.CDLL("libdeflate.so.0")
lib.libdeflate_alloc_compressor.restype = C.c_void_p
lib.libdeflate_alloc_compressor.argtypes = [C.c_int]
lib.libdeflate_deflate_compress.restype = C.c_size_t
lib.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
lib.libdeflate_free_compressor.argtypes = [C.c_void_p]


def deflate(text, level):
    comp = lib.libdeflate_alloc_compressor(level)
    buf = C.create_string_buffer(65510)  # the most a BGZF member's payload may be
    n = lib.libdeflate_deflate_compress(comp, text, len(text), buf, len(buf))
    lib.libdeflate_free_compressor(comp)
    assert n, "does not fit a BGZF member"
    return buf.raw[:n]


def texts():
    t = test_gpu_inflate._texts()
    with gzip.open(os.path.join(HERE, "1kg_chr1_20klines.expected.tsv.gz"), "rb") as f:
        tsv = f.read(65280)
    gt_dp_gq = vcfgen.gen_vcf(12, 40, 400, fmt_extra=True, weird=0.02)
    # (name, text, levels); both files together stay under 512 KB -- if a text is added, drop levels of those that hardly compress
    return [("vcf", t["vcf"], (1, 6, 9, 12)), ("gt_dp_gq", gt_dp_gq[:65280], (1, 6, 9, 12)), ("tsv", tsv, (1, 6, 9, 12)),
            ("long_lines", t["long_lines"], (0, 1, 6, 9, 12)), ("bytes_all", t["bytes_all"], (1, 6, 9, 12)),
            ("random_small_alphabet", t["random_small_alphabet"], (1, 6, 9, 12)), ("far_refs", t["far_refs"], (1, 6, 9, 12))]


def main():
    members = []
    for name, text, levels in texts():
        assert len(text) <= 65280
        for level in levels:
            members.append(dc.member(deflate(text, level), text))
            print("%-22s level %2d  %6d -> %6d" % (name, level, len(text), len(members[-1])))
    with open(os.path.join(HERE, "libdeflate_members.bgzf"), "wb") as f:
        f.write(b"".join(members))
    vcf = craft.cohort_vcf()
    cohort = [dc.member(deflate(vcf[i:i + 65536], 12), vcf[i:i + 65536]) for i in range(0, len(vcf), 65536)]
    cohort.append(dc.member(deflate(b"", 12), b""))  # the EOF member
    with open(os.path.join(HERE, "libdeflate_cohort.vcf.gz"), "wb") as f:
        f.write(b"".join(cohort))
    for name in ("libdeflate_members.bgzf", "libdeflate_cohort.vcf.gz"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
