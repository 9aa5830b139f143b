"""The plan of a ctx (bvcf_plan_ctx, include/bvcf_plan.h): which kernel chain and which genotype scan bvcf_create picks from
bvcf_params and the BVCF_* variables, and the sizes it derives -- no device involved.  The expectations are written out
from the rules in include/bvcf.h (bvcf_params.path, min_gq / min_dp, sample_keep, packed_sites / render_sites) and README.md's
list of variables; nothing here is computed by the library."""
import pytest

WIDE = 32768    # BVCF_WIDE_SAMPLES
STAGED = 16384  # samples whose dense class map k_stream_gen can stage in LDS (4 * 4 KiB of 2-bit classes)
STREAM, S2_TILES, S2_CHUNKS, CENSUS, SITES_EXP, SITES1_EXP = 0, 1, 2, 3, 4, 5
NONE, PLAIN, WIDE_SCAN, FILTER, SUBSET = 0, 1, 2, 3, 4
E_ARG = -1
VARIABLES = ["BVCF_PATH", "BVCF_WIDE", "BVCF_WIDE_WIN", "BVCF_GEN_STREAM", "BVCF_HEAD_FAST", "BVCF_SITES", "BVCF_S2_CENSUS",
             "BVCF_TILE_KB"]


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def chain(c, s, **more):
    return dict(rc=0, chain=c, scan=s, **more)


# (id, n_header_fields, bvcf_params beyond it, environment, what the plan must say)
CASES = [
    # ---- the file's width, path 0: no samples -> k_sites2 behind the census per tile; few samples -> the census chain;
    # 256 header fields up -> the streaming chain; BVCF_WIDE_SAMPLES samples up -> the census chain with the split scan
    ("fields-8", 8, {}, {}, chain(S2_TILES, NONE, n_samples=0, n_samples_full=0, packed=0, render=0)),
    ("fields-9", 9, {}, {}, chain(S2_TILES, NONE, n_samples=0, n_samples_full=0)),
    ("fields-10", 10, {}, {}, chain(CENSUS, PLAIN, n_samples=1, n_samples_full=1, gen_policy=0, gen_mode=0)),
    ("fields-17", 17, {}, {}, chain(CENSUS, PLAIN, n_samples=8)),
    ("fields-255", 255, {}, {}, chain(CENSUS, PLAIN, n_samples=246)),
    ("fields-256", 256, {}, {}, chain(STREAM, PLAIN, n_samples=247, gen_policy=-1, gen_mode=0, shape_seen=0)),
    ("fields-265", 265, {}, {}, chain(STREAM, PLAIN, n_samples=256, gen_policy=-1)),
    ("fields-wide-minus-1", 9 + WIDE - 1, {}, {}, chain(STREAM, PLAIN, n_samples=WIDE - 1, gen_policy=0, gen_mode=0)),
    ("fields-wide", 9 + WIDE, {}, {}, chain(CENSUS, WIDE_SCAN, n_samples=WIDE, gen_policy=0)),
    # ---- bvcf_params.path
    ("path-0", 17, dict(path=0), {}, chain(CENSUS, PLAIN)),
    ("path-1", 17, dict(path=1), {}, chain(CENSUS, PLAIN, gen_policy=0)),
    ("path-2", 17, dict(path=2), {}, chain(STREAM, PLAIN, gen_policy=-1, gen_mode=0, shape_seen=0)),
    ("path-3", 17, dict(path=3), {}, chain(STREAM, PLAIN, gen_policy=-1, gen_mode=1, shape_seen=1)),
    ("path-1-cohort", 265, dict(path=1), {}, chain(CENSUS, PLAIN, gen_policy=0)),
    ("path-1-wide", 9 + WIDE, dict(path=1), {}, chain(CENSUS, WIDE_SCAN)),
    ("path-2-wide", 9 + WIDE, dict(path=2), {}, chain(STREAM, PLAIN, gen_policy=0, gen_mode=0)),
    ("path-2-no-samples", 9, dict(path=2), {}, chain(S2_TILES, NONE)),
    ("path-3-beyond-staging", 9 + STAGED + 1, dict(path=3), {}, chain(STREAM, PLAIN, gen_policy=0, gen_mode=0, shape_seen=0)),
    # ---- k_stream_gen stages a line's dense class map in LDS: never beyond 4 * kStageBytes samples
    ("gen-staged", 9 + STAGED, dict(path=2), {}, chain(STREAM, PLAIN, gen_policy=-1)),
    ("gen-beyond-staging", 9 + STAGED + 1, dict(path=2), {}, chain(STREAM, PLAIN, gen_policy=0, gen_mode=0)),
    # ---- min_gq / min_dp: the census chain with the masked scan whatever path says; nothing changes without samples
    ("min-gq", 17, dict(path=2, min_gq=20), {}, chain(CENSUS, FILTER, gen_policy=0, gen_mode=0)),
    ("min-dp", 17, dict(path=2, min_dp=5), {}, chain(CENSUS, FILTER)),
    ("min-gq-dp", 17, dict(path=2, min_gq=20, min_dp=5), {}, chain(CENSUS, FILTER)),
    ("min-gq-path-3", 265, dict(path=3, min_gq=1), {}, chain(CENSUS, FILTER, gen_mode=0, shape_seen=0)),
    ("min-gq-wide", 9 + WIDE, dict(min_gq=20), {}, chain(CENSUS, FILTER)),
    ("min-gq-no-samples", 9, dict(min_gq=20, min_dp=5), {}, chain(S2_TILES, NONE)),
    ("min-gq-too-large", 17, dict(min_gq=1000000000), {}, dict(rc=E_ARG)),
    # ---- sample_keep: the census chain with the subset scan (it applies the thresholds too)
    ("subset", 17, dict(sample_keep=[0, 2, 7]), {}, chain(CENSUS, SUBSET, n_samples=3, n_samples_full=8, cmap_stride=16)),
    ("subset-path-2", 265, dict(path=2, sample_keep=range(0, 256, 2)), {},
     chain(CENSUS, SUBSET, n_samples=128, n_samples_full=256, cmap_stride=32, gen_policy=0)),
    ("subset-thresholds", 17, dict(sample_keep=[1], min_gq=20, min_dp=3), {}, chain(CENSUS, SUBSET, n_samples=1)),
    ("subset-wide", 9 + WIDE, dict(sample_keep=[5]), {}, chain(CENSUS, SUBSET, n_samples=1, n_samples_full=WIDE)),
    ("subset-bits-past-the-end", 17, dict(sample_keep=[3, 8, 31]), {}, chain(CENSUS, SUBSET, n_samples=1)),
    ("subset-keeps-nothing", 17, dict(sample_keep=[]), {}, dict(rc=E_ARG)),
    ("subset-keeps-only-past-the-end", 17, dict(sample_keep=[8, 9]), {}, dict(rc=E_ARG)),
    ("subset-no-samples", 9, dict(sample_keep=[]), {}, chain(S2_TILES, NONE, n_samples=0)),
    # ---- the result's form: packed / rendered only on a k_sites2 chain
    ("packed", 8, dict(packed_sites=True), {}, chain(S2_TILES, NONE, packed=1, render=0)),
    ("rendered", 8, dict(packed_sites=True, render_sites=True), {}, chain(S2_TILES, NONE, packed=1, render=1)),
    ("packed-with-samples", 17, dict(packed_sites=True, render_sites=True), {}, chain(CENSUS, PLAIN, packed=0, render=0)),
    ("packed-streaming", 265, dict(packed_sites=True, render_sites=True), {}, chain(STREAM, PLAIN, packed=0, render=0)),
    # ---- the variables
    ("BVCF_PATH-2", 17, {}, {"BVCF_PATH": "2"}, chain(STREAM, PLAIN)),
    ("BVCF_PATH-1", 265, dict(path=2), {"BVCF_PATH": "1"}, chain(CENSUS, PLAIN)),
    ("BVCF_PATH-3", 17, dict(path=1), {"BVCF_PATH": "3"}, chain(STREAM, PLAIN, gen_mode=1, shape_seen=1)),
    ("BVCF_PATH-2-threshold", 17, dict(min_dp=2), {"BVCF_PATH": "2"}, chain(CENSUS, FILTER)),
    ("BVCF_PATH-2-subset", 17, dict(sample_keep=[0]), {"BVCF_PATH": "2"}, chain(CENSUS, SUBSET)),
    ("BVCF_WIDE-1", 17, dict(path=1), {"BVCF_WIDE": "1"}, chain(CENSUS, WIDE_SCAN)),
    ("BVCF_WIDE-0", 9 + WIDE, {}, {"BVCF_WIDE": "0"}, chain(CENSUS, PLAIN)),
    ("BVCF_WIDE-1-streaming", 17, dict(path=2), {"BVCF_WIDE": "1"}, chain(STREAM, PLAIN)),
    ("BVCF_WIDE-1-threshold", 17, dict(min_gq=9), {"BVCF_WIDE": "1"}, chain(CENSUS, FILTER)),
    ("BVCF_WIDE-1-subset", 17, dict(sample_keep=[0]), {"BVCF_WIDE": "1"}, chain(CENSUS, SUBSET)),
    ("BVCF_WIDE-1-no-samples", 9, {}, {"BVCF_WIDE": "1"}, chain(S2_TILES, NONE)),
    ("BVCF_WIDE_WIN", 17, dict(path=1), {"BVCF_WIDE": "1", "BVCF_WIDE_WIN": "64"}, chain(CENSUS, WIDE_SCAN, win_bytes=64)),
    ("BVCF_WIDE_WIN-too-small", 17, {}, {"BVCF_WIDE_WIN": "63"}, chain(CENSUS, PLAIN, win_bytes=65536)),
    ("BVCF_GEN_STREAM-1", 265, {}, {"BVCF_GEN_STREAM": "1"}, chain(STREAM, PLAIN, gen_policy=1, gen_mode=1, shape_seen=0)),
    ("BVCF_GEN_STREAM-0", 265, {}, {"BVCF_GEN_STREAM": "0"}, chain(STREAM, PLAIN, gen_policy=0, gen_mode=0)),
    ("BVCF_GEN_STREAM-0-path-3", 265, dict(path=3), {"BVCF_GEN_STREAM": "0"},
     chain(STREAM, PLAIN, gen_policy=0, gen_mode=0, shape_seen=0)),
    ("BVCF_GEN_STREAM-1-census", 17, {}, {"BVCF_GEN_STREAM": "1"}, chain(CENSUS, PLAIN, gen_policy=0, gen_mode=0)),
    ("BVCF_GEN_STREAM-1-beyond-staging", 9 + WIDE - 1, {}, {"BVCF_GEN_STREAM": "1"}, chain(STREAM, PLAIN, gen_policy=0, gen_mode=0)),
    ("BVCF_HEAD_FAST-unset", 265, {}, {}, chain(STREAM, PLAIN, head_fast=1)),
    ("BVCF_HEAD_FAST-0", 265, {}, {"BVCF_HEAD_FAST": "0"}, chain(STREAM, PLAIN, head_fast=0)),
    ("BVCF_HEAD_FAST-1", 265, {}, {"BVCF_HEAD_FAST": "1"}, chain(STREAM, PLAIN, head_fast=1)),
    ("BVCF_SITES-0", 9, dict(packed_sites=True, render_sites=True), {"BVCF_SITES": "0"}, chain(CENSUS, NONE, packed=0, render=0)),
    ("BVCF_SITES-2", 9, dict(packed_sites=True), {"BVCF_SITES": "2"}, chain(S2_TILES, NONE, packed=1)),
    ("BVCF_SITES-0-with-samples", 17, {}, {"BVCF_SITES": "0"}, chain(CENSUS, PLAIN)),
    ("BVCF_SITES-2-with-samples", 265, {}, {"BVCF_SITES": "2"}, chain(STREAM, PLAIN)),
    ("BVCF_S2_CENSUS-chunk", 9, {}, {"BVCF_S2_CENSUS": "chunk"}, chain(S2_CHUNKS, NONE, packed=0)),
    ("BVCF_S2_CENSUS-chunk-packed", 8, dict(packed_sites=True, render_sites=True), {"BVCF_S2_CENSUS": "chunk"},
     chain(S2_CHUNKS, NONE, packed=1, render=1)),
    ("BVCF_S2_CENSUS-tile", 9, {}, {"BVCF_S2_CENSUS": "tile"}, chain(S2_TILES, NONE)),
    ("BVCF_S2_CENSUS-chunk-BVCF_SITES-0", 9, {}, {"BVCF_S2_CENSUS": "chunk", "BVCF_SITES": "0"}, chain(CENSUS, NONE)),
    ("BVCF_S2_CENSUS-chunk-with-samples", 17, {}, {"BVCF_S2_CENSUS": "chunk"}, chain(CENSUS, PLAIN)),
    # (experiments builds only: k_sites behind the census, k_sites1 without one; neither has a packed form)
    ("BVCF_SITES-1", 9, dict(packed_sites=True), {"BVCF_SITES": "1"}, chain(SITES_EXP, NONE, packed=0, render=0)),
    ("BVCF_SITES-3", 9, dict(packed_sites=True), {"BVCF_SITES": "3", "BVCF_S2_CENSUS": "chunk"}, chain(SITES1_EXP, NONE, packed=0)),
    # ---- the defaults and the derived sizes
    # 8 samples: 2 map bytes, rounded up to 16; 64 MiB / 48 bytes a line + 4096 = 1 402 197 lines; two records a line + 1024;
    # 1.5 maps a line + 1 MiB, rounded up to 64; a passing line has 16 TABs and its terminator: 65536 / 17 + 2 entries a tile
    ("sizes-8-samples", 17, {}, {},
     chain(CENSUS, PLAIN, max_batch_bytes=64 << 20, n_slots=3, eol_byte=10, cmap_stride=16, dosage_stride=0, max_lines=1402197,
           max_alleles=2805418, max_cmap=34701312, tile_bytes=65536, tile_quota=3857, win_bytes=65536, ss_on=0, ss_ns_pad=0)),
    # 2 504 samples: 626 map bytes -> 640; a line is at least 2 * 2513 bytes: 13 352 of them + 4096; 26 172 maps of 640 + 1 MiB
    ("sizes-2504-samples", 2513, dict(want_dosage=True, sample_stats=True, n_slots=2, max_batch_bytes=64 << 20), {},
     chain(STREAM, PLAIN, n_slots=2, cmap_stride=640, dosage_stride=2512, max_lines=17448, max_alleles=35920, max_cmap=17798656,
           tile_quota=28, ss_on=1, ss_ns_pad=2560, ss_stripes=3, ss_max_runs=327)),
    # a million samples: the slack between the records is what 32 MiB of maps can hold, 134 lines; 33 lines of 2 000 018 bytes
    ("sizes-million-samples", 1000009, {}, {}, chain(CENSUS, WIDE_SCAN, cmap_stride=250000, max_lines=167, max_alleles=1358)),
    # no samples, 1 MiB batches, "\r\n": no maps (1 MiB and nothing per line); 65536 / (7 TABs + 2) + 2 entries
    ("sizes-no-samples", 8, dict(max_batch_bytes=1 << 20, eol_chars=2, eol_byte=b"\r", want_dosage=True, sample_stats=True), {},
     chain(S2_TILES, NONE, max_batch_bytes=1 << 20, eol_byte=13, cmap_stride=0, dosage_stride=0, max_lines=25941, max_alleles=52906,
           max_cmap=1 << 20, tile_quota=7283, ss_on=0)),
    # slot i of alleles[] belongs to line i: at least max_lines + 64 of them; the caller's arena, rounded up to 64 / at least 4096
    ("sizes-given", 17, dict(max_lines=1000, max_alleles=1000, cmap_bytes=100001), {},
     chain(CENSUS, PLAIN, max_lines=1000, max_alleles=1064, max_cmap=100032)),
    ("sizes-given-small-arena", 17, dict(max_lines=1000, max_alleles=5000, cmap_bytes=10), {},
     chain(CENSUS, PLAIN, max_alleles=5000, max_cmap=4096)),
    ("sample-stats-8-samples", 17, dict(sample_stats=True), {}, chain(CENSUS, PLAIN, ss_on=1, ss_ns_pad=64, ss_stripes=1, ss_max_runs=4096)),
    ("BVCF_TILE_KB", 265, {}, {"BVCF_TILE_KB": "8"}, chain(STREAM, PLAIN, tile_bytes=8192, tile_quota=32)),  # 8192 / 265 + 2
    # ---- the allow list as dwords: "PASS" and "." little-endian; anything excluded, or a value of five bytes: the general test
    ("filter-default", 9, {}, {}, chain(S2_TILES, NONE, s1_fmode=1, s1_fkey=[0x53534150, 0x2E, 0, 0], s1_flen=[4, 1, 0, 0])),
    ("filter-allow-all", 9, dict(allow="*"), {}, chain(S2_TILES, NONE, s1_fmode=2, s1_flen=[0, 0, 0, 0])),
    ("filter-exclude", 9, dict(exclude="q10"), {}, chain(S2_TILES, NONE, s1_fmode=0, s1_flen=[0, 0, 0, 0])),
    ("filter-long-value", 9, dict(allow="PASS,LowQual"), {}, chain(S2_TILES, NONE, s1_fmode=0, s1_flen=[0, 0, 0, 0])),
    ("filter-five-values", 9, dict(allow="a,b,c,d,e"), {}, chain(S2_TILES, NONE, s1_fmode=0)),
    ("filter-too-many", 9, dict(allow=",".join("f%d" % i for i in range(33))), {}, dict(rc=E_ARG)),
    # ---- arguments bvcf_create refuses
    ("no-header-fields", 0, {}, {}, dict(rc=E_ARG)),
    ("eol-chars-3", 17, dict(eol_chars=3), {}, dict(rc=E_ARG)),
]


@pytest.mark.parametrize("n_header_fields,params,env,want", [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_plan(bv, monkeypatch, n_header_fields, params, env, want):
    if env.get("BVCF_SITES") in ("1", "3") and b"experiments" not in bv.lib.bvcf_version():
        pytest.skip("k_sites and k_sites1 are only in builds with -DBVCF_EXPERIMENTS")
    for name in VARIABLES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    rc, plan = bv.plan_ctx(n_header_fields, **params)
    got = {"rc": rc}
    for key in want:
        if key != "rc":
            v = getattr(plan, key)
            got[key] = v if isinstance(v, int) else list(v)
    assert got == want


def test_render_needs_the_packed_form(bv, monkeypatch):
    for name in VARIABLES:
        monkeypatch.delenv(name, raising=False)
    import ctypes as C
    p = bv.make_params(8, render_sites=True)
    p.packed_sites = 0
    plan = bv.CtxPlan()
    bv.lib.bvcf_plan_ctx.argtypes = [C.POINTER(bv.Params), C.POINTER(bv.CtxPlan)]
    assert bv.lib.bvcf_plan_ctx(C.byref(p), C.byref(plan)) == 0
    assert (plan.chain, plan.packed, plan.render) == (S2_TILES, 0, 0)


def test_bad_abi_version_reads_nothing_behind_min_dp(bv):
    import ctypes as C
    p = bv.make_params(17)
    p.abi_version = bv.ABI_VERSION + 2
    assert bv.lib.bvcf_plan_ctx(C.byref(p), C.byref(bv.CtxPlan())) == E_ARG
    assert b"bad bvcf_params" in bv.lib.bvcf_last_error(None)
    # BVCF_ABI_VERSION: sample_keep is not read, whatever it points at
    p = bv.make_params(17, sample_keep=[0])
    p.abi_version = bv.ABI_VERSION
    plan = bv.CtxPlan()
    assert bv.lib.bvcf_plan_ctx(C.byref(p), C.byref(plan)) == 0
    assert (plan.scan, plan.n_samples) == (PLAIN, 8)


def test_binding_matches_the_header(bv, tmp_path):
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf_plan.h"\nint main(){printf("%zu %zu %zu %d %d\\n",'
                   "sizeof(bvcf_ctx_plan),offsetof(bvcf_ctx_plan,chain),offsetof(bvcf_ctx_plan,eol_byte),"
                   "BVCF_CHAIN_SITES1_EXP,BVCF_SCAN_SUBSET);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(bv.CtxPlan), bv.CtxPlan.chain.offset, bv.CtxPlan.eol_byte.offset, SITES1_EXP, SUBSET]
    assert (bv.CHAIN_STREAM, bv.CHAIN_SITES2_TILES, bv.CHAIN_SITES2_CHUNKS, bv.CHAIN_CENSUS, bv.CHAIN_SITES_EXP,
            bv.CHAIN_SITES1_EXP) == (STREAM, S2_TILES, S2_CHUNKS, CENSUS, SITES_EXP, SITES1_EXP)
    assert (bv.SCAN_NONE, bv.SCAN_PLAIN, bv.SCAN_WIDE, bv.SCAN_FILTER, bv.SCAN_SUBSET) == (NONE, PLAIN, WIDE_SCAN, FILTER, SUBSET)
