"""--plinkOutput without a device: the exported per-row code (bvcf_bed_row, the function k_bed_rows makes every 16 bytes
of a row with), the layout and the markers of the config, the CLI's argument check, and -- with the oracle alone -- that
the inputs of tests/test_gpu_plink.py hold what the cases are about.  The reference recode is plinkbed.py's."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
import pairtable as pt
import plinkbed as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")
SIZES = list(range(1, 71)) + [127, 128, 129, 2504]
CANARY = 0xA5


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def row_with_canaries(bv, cmap, ns, sparse):
    """bvcf_bed_row into the middle of a canary-filled buffer -> the row; nothing on either side may change"""
    rb = pb.row_bytes(ns)
    buf = np.full(64 + rb + 64, CANARY, dtype=np.uint8)
    assert bv.bed_row(cmap, ns, sparse=sparse, out=buf[64:64 + rb]) == rb
    assert (buf[:64] == CANARY).all() and (buf[64 + rb:] == CANARY).all(), "bytes outside the row were written (S = %d)" % ns
    return buf[64:64 + rb].tobytes()


@pytest.mark.parametrize("ns", SIZES)
def test_dense_map_into_row(bv, ns):
    rng = random.Random(100 + ns)
    for pad in (0, 1, 2, 3):  # (the 2-bit slots of samples >= S hold every value in turn: masked)
        classes = [rng.randrange(4) for _ in range(ns)]
        got = row_with_canaries(bv, pb.dense_map(classes, pad_bits=pad), ns, False)
        assert got == pb.row_of_classes(classes), (ns, pad)
    for cls in range(4):  # a row of one class
        assert row_with_canaries(bv, pb.dense_map([cls] * ns, pad_bits=3 - cls), ns, False) == pb.row_of_classes([cls] * ns)


@pytest.mark.parametrize("ns", SIZES)
def test_short_list_into_row(bv, ns):
    rng = random.Random(200 + ns)
    rb = pb.row_bytes(ns)
    for n_entries in (0, 1, 15):
        n = min(n_entries, rb)
        idx = set(rng.sample(range(rb), n))
        if n and rb - 1 not in idx:  # an entry in the row's last byte, with its pad bits set
            idx.discard(next(iter(idx)))
            idx.add(rb - 1)
        entries = [(i, rng.randrange(1, 256)) for i in sorted(idx)]
        classes = [0] * (4 * rb)
        for i, byte in entries:
            for q in range(4):
                classes[4 * i + q] = (byte >> (2 * q)) & 3
        got = row_with_canaries(bv, pb.short_list(entries), ns, True)
        assert got == pb.row_of_classes(classes[:ns]), (ns, n_entries)


def test_short_list_bounds(bv):
    """n is clamped to 15 and an entry past the row is ignored, as k_ss_list and join_class read a list"""
    ns = 300
    entries = [(i, 0x1B) for i in range(15)]
    words = np.frombuffer(pb.short_list(entries), dtype="<u4").copy()
    words[0] = 200
    assert row_with_canaries(bv, words.tobytes(), ns, True) == row_with_canaries(bv, pb.short_list(entries), ns, True)
    past = np.frombuffer(pb.short_list([(3, 0x06)]), dtype="<u4").copy()
    past[0], past[2] = 2, (75 << 8) | 0xFF  # byte 75 of a 75-byte row
    assert row_with_canaries(bv, past.tobytes(), ns, True) == row_with_canaries(bv, pb.short_list([(3, 0x06)]), ns, True)


def test_record_without_a_map_is_all_missing(bv):
    for ns in (1, 5, 64, 299):
        assert row_with_canaries(bv, None, ns, False) == pb.row_of_classes([3] * ns)


def test_reference_recode_by_hand():
    # none, het, hom, missing -> 11, 10, 00, 01 from the low bits up: 0b01_00_10_11
    assert pb.row_of_classes([0, 1, 2, 3]) == bytes([0b01001011])
    assert pb.row_of_classes([1]) == bytes([0b10]) and pb.row_of_classes([0, 0, 0, 0, 2]) == bytes([0xFF, 0x00])
    H = np.array([[0, 1, 0, 0, 0]], dtype=np.uint8)
    O = np.array([[0, 0, 1, 0, 0]], dtype=np.uint8)
    M = np.array([[0, 0, 0, 1, 0]], dtype=np.uint8)
    bed = pb.bed_bytes(H, O, M)
    assert bed == pb.MAGIC + bytes([0b01001011, 0b11])
    for got, want in zip(pb.decode_bed(bed, 5), (H, O, M)):
        assert np.array_equal(got, want)
    for x, (hi, lo) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):  # the issue's bit operations are the same table
        assert pb.CLASS_TO_CODE[x] == ((1 - hi) << 1) | (1 - (hi ^ lo))


def test_header_binding_and_library_agree(bv):
    with open(os.path.join(ROOT, "include", "bvcf.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "bvcf_plan.h")) as f:
        plan = f.read()
    with open(os.path.join(ROOT, "include", "bvcf_bench.h")) as f:
        bench = f.read()
    assert re.search(r"int bvcf_enable_bed_rows\(bvcf_ctx \*ctx\);", h)
    assert re.search(r"int bvcf_reserve_bed_rows\(bvcf_ctx \*ctx, uint64_t bytes\);", h)
    assert re.search(r"int bvcf_bed_rows\(const bvcf_ctx \*ctx, bvcf_bed_rows_info \*out\);", h)
    assert "#define BVCF_CONFIG_MORE_PLINK 2\n" in h and bv.CONFIG_MORE_PLINK == 2 > bv.CONFIG_MORE_GATE
    assert re.search(r"int bvcf_bed_row\(const uint8_t \*cmap_or_list, int sparse, uint32_t S, uint8_t \*out\);", plan)
    assert "bvcf_bench_bed_kernels" in bench
    for name in ("bvcf_enable_bed_rows", "bvcf_reserve_bed_rows", "bvcf_bed_rows", "bvcf_config_plink_defaults"):
        assert name in bv.EXPORTS and hasattr(bv.lib, name)
    assert "bvcf_bed_row" in bv.PLAN_EXPORTS and hasattr(bv.lib, "bvcf_bed_row")
    assert "bvcf_bench_bed_kernels" in bv.BENCH_EXPORTS and hasattr(bv.lib, "bvcf_bench_bed_kernels")
    assert bv.BED_MAGIC == pb.MAGIC and bv.BED_CODE == tuple(pb.CLASS_TO_CODE[c] for c in range(4))
    assert bv.ABI_VERSION == 9 and bv.ABI_VERSION_SUBSET == 10


def test_layout_matches_header(bv, tmp_path):
    src = tmp_path / "lay.c"
    info = ["rows", "n_rows", "row_bytes", "reserved", "need_bytes"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(bvcf_config), sizeof(bvcf_config_more), sizeof(bvcf_params),'
                   "sizeof(bvcf_result), offsetof(bvcf_config_more, pair_stats_path), offsetof(bvcf_config_more, site_gate),"
                   "offsetof(bvcf_config_more, site_filter_path), offsetof(bvcf_config_more, plink_prefix), sizeof(bvcf_bed_rows_info));"
                   + "".join('printf(" %%zu", offsetof(bvcf_bed_rows_info, %s));' % f for f in info)
                   + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M, B = bv.ConfigMore, bv.BedRowsInfo
    assert out == [C.sizeof(bv.Config), C.sizeof(M), C.sizeof(bv.Params), C.sizeof(bv.Result), M.pair_stats_path.offset,
                   M.site_gate.offset, M.site_filter_path.offset, M.plink_prefix.offset, C.sizeof(B)] + [getattr(B, f).offset for f in info]
    # the struct grew at its end only: what came before plink_prefix is where it was
    assert M.plink_prefix.offset == M.site_filter_path.offset + 8 and C.sizeof(M) == M.plink_prefix.offset + 8


def test_older_defaults_write_nothing_new(bv):
    for fn, first_untouched in ((bv.lib.bvcf_config_more_defaults, bv.ConfigMore.site_gate.offset),
                                (bv.lib.bvcf_config_gate_defaults, bv.ConfigMore.plink_prefix.offset)):
        m = bv.ConfigMore()
        C.memset(C.byref(m), 0xFF, C.sizeof(m))
        fn(C.byref(m))
        assert bytes(m)[first_untouched:] == b"\xff" * (C.sizeof(m) - first_untouched), fn
    m = bv.ConfigMore()
    C.memset(C.byref(m), 0xFF, C.sizeof(m))
    bv.lib.bvcf_config_gate_defaults(C.byref(m))
    assert (m.base.reserved[0], m.base.reserved[1]) == (bv.CONFIG_MORE, bv.CONFIG_MORE_GATE)
    bv.lib.bvcf_config_plink_defaults(C.byref(m))
    assert (m.base.reserved[0], m.base.reserved[1]) == (bv.CONFIG_MORE, bv.CONFIG_MORE_PLINK)
    assert m.plink_prefix is None and m.site_filter_path is None and m.pair_stats_path is None
    g = m.site_gate
    assert (g.size, g.min_mac, g.min_maf, g.max_maf, g.max_missing, g.hwe_p) == (40, 0, 0.0, 1.0, 1.0, 0.0)


def test_make_config_markers(bv):
    assert list(bv.make_config({}).reserved) == [0, 0]
    assert list(bv.make_config({"relatedness": "/x"}).reserved) == [bv.CONFIG_MORE, 0]
    assert list(bv.make_config({"minMac": 2}).reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_GATE]
    for cfg in ({"plinkOutput": "/x/p"}, {"plinkOutput": "/x/p", "minMaf": 0.05}):
        c = bv.make_config(cfg)
        assert list(c.reserved) == [bv.CONFIG_MORE, bv.CONFIG_MORE_PLINK]
        more = C.cast(C.byref(c), C.POINTER(bv.ConfigMore)).contents
        assert more.plink_prefix == b"/x/p" and more.site_gate.size == 40 and more.site_gate.min_maf == cfg.get("minMaf", 0.0)
        assert more.site_gate.max_maf == 1.0 and more.site_gate.max_missing == 1.0


SITES = (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
         b"chr1\t100\t.\tA\tC\t50\tPASS\t.\n")


def run_marked(bv, prefix, marker):
    """bvcf_run_buffer over a ConfigMore with plink_prefix set and base.reserved[1] = marker -> the log.  The files of
    --plinkOutput are opened before any device work, so this says which marker reads the field with or without a device"""
    c = bv.make_config({"plinkOutput": str(prefix)})
    c.reserved[1] = marker
    return bv.run_buffer(SITES, c)[2]


def test_three_marker_levels_are_read_as_specified(bv, tmp_path):
    bad = tmp_path / "no_such_dir" / "p"
    # the third marker: the prefix is read, and an unwritable one is one message
    log = run_marked(bv, bad, bv.CONFIG_MORE_PLINK)
    assert ("open %s.bed: " % bad) in log and log.count("\n") == 1, log
    # the second marker and none: nothing behind site_filter_path is read
    for marker in (bv.CONFIG_MORE_GATE, 0):
        assert str(bad) not in run_marked(bv, bad, marker)
    good = tmp_path / "p"
    for marker in (bv.CONFIG_MORE_GATE, 0):
        run_marked(bv, good, marker)
        assert not any(os.path.exists("%s.%s" % (good, e)) for e in ("bed", "bim", "fam"))
    run_marked(bv, good, bv.CONFIG_MORE_PLINK)
    assert all(os.path.exists("%s.%s" % (good, e)) for e in ("bed", "bim", "fam"))
    # a larger value still reaches the gate fields ("at least"): a gate out of range is refused whatever the device
    c = bv.make_config({"plinkOutput": str(good), "minMaf": 0.05})
    more = C.cast(C.byref(c), C.POINTER(bv.ConfigMore)).contents
    assert c.reserved[1] == bv.CONFIG_MORE_PLINK and more.site_gate.min_maf == 0.05


def cli(args, stdin_bytes=b""):
    return subprocess.run([EXE] + args, input=stdin_bytes, capture_output=True, timeout=60)


def test_cli_flag_without_a_value():
    p = cli(["--plinkOutput"])
    assert p.returncode == 2 and b"flag needs an argument: -plinkOutput" in p.stderr
    assert p.stdout == b""


# ---- the inputs of tests/test_gpu_plink.py, with the oracle alone

@pytest.fixture(scope="module")
def seeded():
    return pb.seeded_inputs()


def test_inputs_hold_what_the_cases_are_about(seeded):
    """every seeded input: all four codes; rows with at most 5 carriers (short lists on the streaming path) and rows that
    a quarter of the cohort carries (dense maps); multiallelic rows"""
    assert len(seeded) >= 12
    for name, vcf in seeded.items():
        names = pt.sample_names(vcf)
        rc, body, _, _ = orc.run(vcf)
        assert rc == 0
        H, O, M = pt.matrices(body, names)
        codes = pb.codes_of(H, O, M)
        assert set(np.unique(codes).tolist()) == {0, 1, 2, 3}, name
        carriers = (H + O).sum(axis=1)
        assert (carriers <= 5).any() and (4 * carriers >= len(names)).any(), (name, len(names))
        assert any(r.split(b"\t")[2] == b"MULTIALLELIC" for r in body.split(b"\n") if r), name
        # and the decoder is the inverse of the expected file
        for got, want in zip(pb.decode_bed(pb.bed_bytes(H, O, M), len(names)), (H, O, M)):
            assert np.array_equal(got, want)


def test_sample_counts_cover_every_tail_and_alignment():
    rb = [pb.row_bytes(ns) for ns in pb.GPU_SAMPLE_COUNTS]
    assert {ns % 4 for ns in pb.GPU_SAMPLE_COUNTS} == {0, 1, 2, 3}
    assert any(x % 16 for x in rb) and any(x % 2 for x in rb)
    assert [pb.row_bytes(ns) for ns in pb.ALIGN_SAMPLES] == [1, 1, 1, 1, 2, 2, 2, 4, 4, 5, 16, 16, 17, 33, 75, 75]
    # rows of an odd number of bytes laid back to back start at every alignment mod 16
    for odd in (1, 5, 17, 33, 75):
        assert {(k * odd) % 16 for k in range(16)} == set(range(16))


def test_many_alts_input_overruns_the_starting_arena():
    vcf = pb.many_alts_vcf()
    rc, body, _, _ = orc.run(vcf)
    n_rows = body.count(b"\n")
    assert rc == 0 and len(vcf) < (1 << 20)
    assert n_rows * pb.row_bytes(8) > (1 << 20) // 4  # (--batchMB 1: the arena starts at a quarter of a megabyte)
    assert n_rows > 150 * vcf.count(b"\nchr4")
