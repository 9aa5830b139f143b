"""--keepSamples / --excludeSamples: the one rule of include/bvcf.h applied to VCF text, and the selections the tests share.

The oracle knows nothing of the flags.  What a run with a selection must produce follows from an equivalence instead:

    device run of the ORIGINAL bytes with the selection  ==  oracle run of cut_vcf(bytes, kept indices) without it

cut_vcf cuts the unselected sample columns out of the header line and out of every data line that has the header's field
count, and touches nothing else of those lines."""
import functools
import random

import gtmask


def sample_names(vcf):
    """the sample names of the #CHROM line, as bytes"""
    for ln in vcf.split(b"\n"):
        if ln.startswith(b"#CHROM"):
            return ln.rstrip(b"\r").split(b"\t")[9:]
    return []


def cut_vcf(vcf_bytes, keep_indices):
    """the file with sample columns `keep_indices` (0-based, any order, duplicates harmless) only, in header order.
    Header line and data lines with the header's field count: columns 0-8 and the kept sample columns.  A data line with
    any other field count fails the field-count gate of the original file without a word in the log; it is replaced by
    its first 8 columns, which fail the gate of the cut file the same way (whose header has at least 10 fields).  CRLF is
    kept."""
    keep = sorted(set(int(i) for i in keep_indices))
    lines = vcf_bytes.split(b"\n")
    crlf = len(lines) > 1 and lines[0].endswith(b"\r")
    n_header = None
    for i, ln in enumerate(lines):
        if n_header is None and not ln.startswith(b"#CHROM"):
            continue
        cr = b"\r" if crlf and ln.endswith(b"\r") else b""
        cols = ln[:len(ln) - len(cr)].split(b"\t")
        if n_header is None:  # the header line
            n_header = len(cols)
            assert all(0 <= k < n_header - 9 for k in keep), "selection outside the header's samples"
        if len(cols) == n_header:
            cols = cols[:9] + [cols[9 + k] for k in keep]
        else:
            cols = cols[:8]
        lines[i] = b"\t".join(cols) + cr
    return b"\n".join(lines)


# ---- seeded selections of the inputs of gtmask.SEEDED

KINDS = ["half", "tenth", "one", "allbutone", "ends"]
# one seed per input, fixed here (test_sample_subset_cpu.py checks with the oracle alone that the tenth selection of every
# input of its table keeps a row, drops a row and changes a list; a seed that misses that is replaced, not excused)
SEEDS = {"fuzz17": 1101, "fuzz70crlf": 1102, "fuzz300": 1103, "fuzz2600crlf": 1104, "crafted37": 1105, "crafted5crlf": 1106,
         "crafted130": 1107, "alignment": 1108, "alignment_crlf": 1109, "wide33000": 1110, "cohort": 1111, "stats300": 1112}


@functools.lru_cache(maxsize=None)
def n_samples(name):
    return len(sample_names(gtmask.seeded(name)))


@functools.lru_cache(maxsize=None)
def selection(name, kind):
    """the kept sample indices (sorted tuple) of a seeded input: about half the samples, about a tenth, exactly one, all
    but one, the first and the last column only"""
    ns = n_samples(name)
    rng = random.Random(SEEDS[name] * 16 + KINDS.index(kind))
    if kind == "half":
        k = rng.sample(range(ns), max(1, ns // 2))
    elif kind == "tenth":
        k = rng.sample(range(ns), max(1, (ns + 5) // 10))
    elif kind == "one":
        k = [rng.randrange(ns)]
    elif kind == "allbutone":
        out = rng.randrange(ns)
        k = [s for s in range(ns) if s != out]
    elif kind == "ends":
        k = [0, ns - 1]
    else:
        raise KeyError(kind)
    return tuple(sorted(set(k)))


def complement(name, kept):
    kept = set(kept)
    return tuple(s for s in range(n_samples(name)) if s not in kept)


@functools.lru_cache(maxsize=None)
def cut(name, kind):
    """cut bytes of a seeded input under one of its selections"""
    return cut_vcf(gtmask.seeded(name), selection(name, kind))


def list_file(path, vcf, indices, eol=b"\n"):
    """writes the names of sample columns `indices` of `vcf`, one per line -> str(path)"""
    names = sample_names(vcf)
    with open(str(path), "wb") as f:
        f.write(b"".join(names[i] + eol for i in indices))
    return str(path)
