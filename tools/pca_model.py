#!/usr/bin/env python3
"""Where the bounds of the --pca tests come from  (not a test; needs no device): the numpy restatement of the solver's
algorithm (tests/pca.py) over the GPU test's case list and over every matrix family at sizes 2 .. 40 and every 16th size up
to 300, against numpy.linalg.eigh.  Prints the worst residual, eigenvalue and orthonormality ratio (units: tests/pca.py)
with the case that gave each, and numpy's own worst residual ratio.  tests/pca.py's MODEL_WORST and BOUND_* are these
numbers; run this again when the algorithm or the case list changes.

usage: pca_model.py [PROCESSES]   (default 8; about a minute)"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pca  # noqa: E402


def one(case):
    fam, n, k = case
    A = pca.family(fam, n)
    vals, vecs = pca.model_eigen(A, k)
    w, v = np.linalg.eigh(A)
    u = pca.unit(A)
    own = float(np.abs(A @ v - v * w[None, :]).max()) / u if u > 0 else 0.0
    return case, pca.ratios(A, vals, vecs), own, bool(np.isfinite(vecs).all())


def main():
    sizes = list(range(2, 41)) + list(range(44, 301, 16)) + [300]
    gpu = pca.gpu_cases()
    cases = gpu + [(f, n, k) for f in pca.FAMILIES for n in sizes for k in pca.ks_of(n)]
    with mp.Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 8) as pool:
        out = pool.map(one, cases, chunksize=4)
    for tag, part in (("all %d cases" % len(out), out), ("gpu_cases() alone", out[:len(gpu)])):
        worst, where, own = [0.0] * 3, [None] * 3, 0.0
        for case, r, rn, finite in part:
            assert finite, case
            own = max(own, rn)
            for i in range(3):
                if r[i] > worst[i]:
                    worst[i], where[i] = r[i], case
        print(tag)
        for name, x, c in zip(("residual", "eigenvalue", "orthonormality"), worst, where):
            print("  %-15s %.3f  %s" % (name, x, c))
        print("  numpy's own residual %.3f" % own)


if __name__ == "__main__":
    main()
