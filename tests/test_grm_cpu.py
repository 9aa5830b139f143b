"""--grm without a device: the definition is a GRM, the test inputs reach every case of it, and bvcf_grm_q.h -- the
quantiser the kernels and the host writer share -- agrees with Python's exact definition, in a stand-alone program under
the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import grm
import oracle_lib as orc
import pairtable as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bystro-vcf_amd", "csrc")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
N_MAX = 40


@pytest.fixture(scope="module")
def inputs():
    """{name: (H, O, M)} of every small input, through the oracle"""
    out = {}
    for name, vcf in grm.small_inputs().items():
        rc, body, _, _ = orc.run(vcf)
        assert rc == 0, name
        out[name] = pt.matrices(body, pt.sample_names(vcf))
    return out


def scores_in_use(H, O, M):
    """the q values samples of the GRM rows have"""
    n, a, D = grm.row_counts(H, O, M)
    Q, Mk = grm.score_matrix(H, O, M, grm.row_scores(n, a, D), D)
    return Q[Mk == 0]


def test_definition_rounds_to_nearest_without_ties():
    """over every row shape with n <= 40: q is the integer nearest to z 2^14, and no z 2^14 lies on a half"""
    for n in range(1, N_MAX + 1):
        for a in range(1, 2 * n):
            D = 2 * a * (2 * n - a)
            for g in range(3):
                q = grm.q_exact(n, a, g)
                num = 2 * n * g - 2 * a
                # |q| - 1/2 < |num| 2^14 / sqrt(D) < |q| + 1/2, squared and cleared of fractions; strict: no tie
                if num:
                    assert (2 * abs(q) - 1) ** 2 * D < 4 * num * num * grm.ONE < (2 * abs(q) + 1) ** 2 * D, (n, a, g)
                    assert (q > 0) == (num > 0)
                else:
                    assert q == 0
                assert sum(d << (8 * k) for k, d in enumerate(grm.limbs(q))) == q


def test_score_bounds_of_the_header():
    """|z| <= sqrt(2 (n - 1)) for a score a sample has, at the cap of 8 192 called samples: |q| < 2^21"""
    n = 8192
    assert grm.q_exact(n, 2, 2) == max(abs(grm.q_exact(n, a, 2)) for a in (2, 3, 4, 100, n, 2 * n - 2))
    assert abs(grm.q_exact(n, 2, 2)) < 1 << 21 and abs(grm.q_exact(n, 2 * n - 2, 0)) < 1 << 21
    assert abs(grm.q_exact(n, 1, 2)) < 1 << 22 and abs(grm.q_exact(n, 2 * n - 1, 0)) < 1 << 22  # (scores nobody has)


def test_inputs_reach_every_case(inputs):
    used = np.concatenate([scores_in_use(*m).ravel() for m in inputs.values()])
    assert (used < 0).any() and (used > 0).any()
    three = [q for q in np.unique(used).tolist() if all(grm.limbs(q))]
    assert three and max(abs(q) for q in three) >= 2 << grm.SHIFT, "no score with three non-zero limbs"
    # a singleton hom among 40: z = sqrt(2 * 39) > 8
    assert max(abs(q) for q in scores_in_use(*inputs["singleton"]).ravel().tolist()) > 8 << grm.SHIFT
    # monomorphic rows: of n = 0, a = 0 and a = 2n only the last can be a row at all (a row has ac > 0) -- with every
    # sample called, with missing calls, and haploid
    H, O, M = inputs["monomorphic"]
    n, a, D = grm.row_counts(H, O, M)
    mono = D == 0
    assert (a[mono] == 2 * n[mono]).all() and (n[mono] == H.shape[1]).any() and (n[mono] < H.shape[1]).any()
    all_het = (H.sum(axis=1) == n) & ~mono
    assert all_het.any(), "no all-het row (kept: the score every called sample has is 0)"
    assert not grm.row_scores(n, a, D)[all_het][:, 1].any()
    # no row with both called: N(i,j) = 0, and a half-missing sample
    T, MM, N = grm.tables(*inputs["allmissing"])
    nij = grm.pair_rows(MM, N)
    assert N > 0 and (nij[2] == 0).all() and nij[0, 0] == N and 0 < nij[0, 1] < N
    assert (grm.matrix(T, MM, N)[0][2] == 0).all()
    # a short list at its limit with missing entries
    H, O, M = inputs["limit"]
    full = [r for r in range(H.shape[0]) if (H[r] + O[r] + M[r]).sum() >= 45 and M[r].any()]
    assert full


def test_flush_input_overflows_an_int32_sum():
    gts, v = grm.flush_pattern()
    assert v * grm.FLUSH_ROWS >= 1 << 31, (gts, v)
    assert len(grm.flush_vcf()) > 7 << 20


def test_quantised_matrix_is_a_grm(inputs):
    """|A_quantised - A_double| <= mean over the rows of (|z_i| + |z_j|) 2^-15 + 2^-30 + 1e-12, for every pair: q differs
    from z 2^14 by at most 1/2, so q_i q_j 2^-28 from z_i z_j by at most (|z_i| + |z_j|) 2^-15 + 2^-30"""
    for name, (H, O, M) in inputs.items():
        T, MM, N = grm.tables(H, O, M)
        Aq, nij = grm.matrix(T, MM, N)
        Ad, B, nij_d = grm.double_matrix(H, O, M)
        assert np.array_equal(nij, nij_d.astype(np.int64)), name
        bound = B * 2.0 ** -15 + 2.0 ** -30 + 1e-12
        worst = float((np.abs(Aq - Ad) - bound).max(initial=-1.0))
        assert worst <= 0.0, (name, worst)
        assert np.array_equal(T, T.T) and np.array_equal(MM, MM.T), name


def test_quantiser_header_alone_under_sanitizers(tmp_path):
    """bvcf_grm_q.h in a program of its own: every q over the closed domain against Python's, the 128-bit add across a carry"""
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present: sanitized programs run on the build machine")
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "grm_q_check")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "grm_q_check.cpp"),
                           "-o", exe], timeout=120)
    p = subprocess.run([exe, str(N_MAX)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.endswith("grm_q ok\n"), out[-2000:]
    assert "ERROR" not in out and "runtime error" not in out, out[-2000:]
    lines = out.split("\n")[:-2]
    want = []
    for n in range(1, N_MAX + 1):
        for a in range(1, 2 * n):
            for g in range(3):
                q = grm.q_exact(n, a, g)
                want.append("%d %d %d %d %d %d %d" % ((n, a, g, q) + tuple(grm.limbs(q))))
    assert lines == want
