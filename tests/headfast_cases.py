"""Crafted data lines on every boundary of k_order's fast lane (csrc/bvcf_headfast.hip.h), and a Python model of what
k_stream hands it.  Test infrastructure only (tests/test_head_fast_cpu.py, tests/test_gpu_head_fast.py)."""
import vcfgen

NS = 300                      # samples: n_header = 309 puts a ctx on the streaming path; a line is > 1 200 bytes
N_HEADER = 9 + NS
GTS = (["0|1", "1|1", "0|0", ".|.", "1|0", "0|0"] * (NS // 6 + 1))[:NS]
HEAD_BYTES = 64               # kHeadFastBytes


def header():
    return vcfgen.header(NS).encode()


def line(chrom="1", pos="12345", vid="rs1", ref="A", alt="G", qual="50", flt="PASS", info="AC=1", gts=None):
    return "\t".join([chrom, pos, vid, ref, alt, qual, flt, info, "GT"] + (gts or GTS)).encode()


def counts(gts=None):
    """ALT #1's {ac, an, n_het, n_hom, n_miss} of diploid single-digit fields, as k_stream's regular scan counts them"""
    het = hom = miss = 0
    for g in gts or GTS:
        a, b = g[0], g[2]
        if a == "." or b == ".":
            miss += 1
        elif a == "1" and b == "1":
            hom += 1
        elif a == "1" or b == "1":
            het += 1
    return [het + 2 * hom, 2 * (len(gts or GTS) - miss), het, hom, miss]


def tab_bits(text, ls):
    """head_window16's bitmap of the line at text[ls:]: the TABs of the 256 bytes from ls & ~3 (nothing before ls), as eight
    words -- or None where k_stream has no bitmap for the line: a terminator in the window, or fewer than nine TABs"""
    base = ls & ~3
    win = text[base:base + 256]
    if len(win) < 256 or b"\n" in win[ls - base:] or b"\r" in win[ls - base:]:
        return None
    words = [0] * 8
    n = 0
    for i in range(ls - base, 256):
        if win[i] == 9:
            words[i >> 5] |= 1 << (i & 31)
            n += 1
    return words if n >= 9 else None


def cases():
    """[(name, line bytes, allow, exclude, expect)]; expect: "pass" / "filter" (the lane must settle the line that way),
    "decline", or None (either: only agreement is asked)"""
    out = []

    def add(name, expect, allow="PASS,.", exclude="", **kw):
        out.append((name, line(**kw), allow, exclude, expect))

    add("plain", "pass")
    for r in "ACGT":
        for a in "ACGT":
            add("snp_%s%s" % (r, a), "pass" if r != a else "decline", ref=r, alt=a)
    for a in ["N", "*", ".", "a", "c", "g", "t", "<", ","]:
        add("alt_%r" % a, "decline", alt=a)
    add("ref_N", "pass", ref="N")
    add("ref_lower", "pass", ref="a", alt="A")
    add("ref_dot", "pass", ref=".", alt="T")
    add("ref2", "decline", ref="AC", alt="A")
    add("alt2", "decline", ref="A", alt="AC")
    add("mnp", "decline", ref="AC", alt="GT")
    add("ref_empty", "decline", ref="", alt="A")
    add("alt_empty", "decline", ref="A", alt="")
    add("multi", "decline", alt="G,T")
    add("comma_tail", "decline", alt="G,")
    add("comma_head", "decline", alt=",G")
    # FILTER: pass / fail / empty allow set / deny set
    add("filter_dot", "pass", flt=".")
    add("filter_fail", "filter", flt="q10")
    add("filter_prefix", "filter", flt="PAS")
    add("filter_longer", "filter", flt="PASSS")
    add("filter_empty_value", "filter", flt="")
    add("filter_empty_value_allowed", "pass", allow="PASS,", flt="")
    add("allow_all_empty", "pass", allow="", flt="q10")
    add("allow_all_star", "pass", allow="*", flt="anything")
    add("deny_hit", "filter", allow="", exclude="q10,s50", flt="s50")
    add("deny_miss", "pass", allow="", exclude="q10,s50", flt="q1")
    add("allow_and_deny", "filter", allow="PASS,q10", exclude="q10", flt="q10")
    add("allow_compound", "pass", allow="LowQual;s50", flt="LowQual;s50")
    add("filter_16", "pass", allow="ABCDEFGHIJKLMNOP", flt="ABCDEFGHIJKLMNOP")
    add("filter_16_differs_last", "filter", allow="ABCDEFGHIJKLMNOP", flt="ABCDEFGHIJKLMNOQ")
    add("filter_17", None, allow="ABCDEFGHIJKLMNOPQ", flt="ABCDEFGHIJKLMNOPQ")
    # TAB #7 (the end of FILTER) across byte 63 / 64, moved by CHROM, by ID, and with a FILTER key that straddles byte 64
    fixed = len("1\t12345\t\tA\tG\t50\tPASS")  # bytes before TAB #7 with an empty ID
    for tab7 in (61, 62, 63, 64, 65, 66):
        add("id_tab7_%d" % tab7, "pass" if tab7 < HEAD_BYTES else "decline", vid="r" * (tab7 - fixed))
        add("chrom_tab7_%d" % tab7, "pass" if tab7 < HEAD_BYTES else "decline", chrom="1" * (tab7 - fixed + 1), vid="")
        add("id_tab7_%d_fail" % tab7, "filter" if tab7 < HEAD_BYTES else "decline", vid="r" * (tab7 - fixed), flt="PASX")
    for start in (51, 52, 56, 62, 63):
        key = "STRADDLES_64"
        pad = start - len("1\t12345\t\tA\tG\t50\t")
        add("key_from_%d" % start, "pass" if start + len(key) < HEAD_BYTES else "decline", allow=key, vid="r" * pad, flt=key)
    # POS is taken as text: leading zeros, non-digits, twelve digits, nothing
    for p in ["000123", "abc", "123456789012", "", "-5", "+7", "1e3", "99999999999999999999"]:
        add("pos_%r" % p, "pass", pos=p)
    # a long INFO pushes TAB #9 out of the head window: no bitmap
    add("long_info", "decline", info="X" * 300)
    add("info_to_window_end", None, info="X" * 200)
    return out


def body(case_list, reps=4):
    """the cases as one block, `reps` times over; a plain line with k more bytes of INFO in front of repetition k moves the
    lines' starts through every ls & 3 (a short or "#" line would do that too, but it also ends k_stream's pipeline: the
    line behind it then has no bitmap and takes no fast lane)"""
    parts = []
    for k in range(reps):
        parts.append(line(info="AC=1" + "X" * k) + b"\n")
        for _, ln, _, _, _ in case_list:
            parts.append(ln + b"\n")
    return b"".join(parts)


def groups():
    """the cases by FILTER configuration: {(allow, exclude): [case, ...]}"""
    g = {}
    for c in cases():
        g.setdefault((c[2], c[3]), []).append(c)
    return g
