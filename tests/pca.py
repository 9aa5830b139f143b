"""--pca: the algorithm restated in numpy (the model), the matrix families, a structured cohort, the parsers of the two
files and the sign rule.  Test infrastructure only.

The definition (include/bvcf.h, bvcf_pca_eigen): the input is the symmetric matrix whose lower triangle is the float32
content of PREFIX.grm.bin, promoted to float64; the output its k algebraically largest eigenvalues, descending, and unit
eigenvectors whose component of largest magnitude is positive (ties: the lowest index).

The model follows the library step by step -- Householder tridiagonalisation by dlarfg / dsytd2's formulas over the rows
of the full matrix, Sturm-count bisection until the interval cannot shrink, inverse iteration with modified Gram-Schmidt
inside a cluster, reflectors applied in reverse -- but sums with numpy's own orders, so its digits are not the library's:
it says what accuracy the ALGORITHM reaches, and the bounds of the tests are set from it, never from the device's results.

u(A) = n 2^-52 ||A||_F is the unit of the residual and eigenvalue checks; n 2^-52 that of U^T U - I.  The bounds and the
model's measured ratios they come from stand next to the constants below."""
import math
import random

import numpy as np

import pairtable as pt
import vcfgen

EPS = 2.0 ** -52
# The three bounds in their units: 4 where the model stays at or below 0.5 (an 8x margin), 8x the model's worst where it does
# not.  The model's worst ratios (tools/pca_model.py: gpu_cases(), the case list of tests/test_gpu_pca.py, and every family at
# sizes 2 .. 40 and every 16th size up to 300 -- 1 472 cases): residual 0.47 (indefinite, n = 3), eigenvalue 0.70 (rank-1,
# n = 3), orthonormality 0.53 (indefinite, n = 23, k = 23); over gpu_cases() alone 0.47, 0.70, 0.50.  numpy.linalg.eigh's own
# residual over the same list reaches 0.71.  The large ratios all belong to n <= 4, where u is a handful of roundings.
MODEL_WORST = (0.47, 0.70, 0.53)
BOUND_RES = 4.0
BOUND_VAL = 5.6   # 8 x 0.70
BOUND_ORTH = 4.24  # 8 x 0.53
MAX_K = 64
KITERS = 5


def unit(A):
    n = A.shape[0]
    return n * EPS * float(np.linalg.norm(A))


def ratios(A, vals, vecs):
    """(residual / u, eigenvalue error / u, orthonormality / (n 2^-52)) of k pairs against numpy.linalg.eigh; vecs is (k, n).
    A zero matrix has u = 0: the ratios are then 0 for exact results and inf otherwise"""
    A = np.asarray(A, dtype=np.float64)
    n, k = A.shape[0], len(vals)
    U = np.asarray(vecs, dtype=np.float64).reshape(k, n).T
    u = unit(A)
    ref = np.linalg.eigvalsh(A)[::-1][:k]
    res = float(np.abs(A @ U - U * np.asarray(vals)[None, :]).max())
    ev = float(np.abs(np.asarray(vals) - ref).max())
    orth = float(np.abs(U.T @ U - np.eye(k)).max()) / (n * EPS)

    def over(x):
        return x / u if u > 0 else (0.0 if x == 0 else math.inf)
    return over(res), over(ev), orth


def apply_sign_rule(v):
    """the component of largest magnitude positive, ties to the lowest index"""
    v = np.array(v, dtype=np.float64)
    i = int(np.argmax(np.abs(v)))  # (argmax returns the first of equal maxima)
    return -v if v[i] < 0 else v


def sign_rule_holds(v):
    v = np.asarray(v)
    i = int(np.argmax(np.abs(v)))
    return bool(v[i] > 0) or not np.any(v)


def lower_f32(A):
    """the packed lower triangle with the diagonal, row by row, as float32: what bvcf_pca_eigen takes"""
    i, j = np.tril_indices(A.shape[0])
    return np.ascontiguousarray(np.asarray(A)[i, j], dtype=np.float32)


def from_lower(lower, n):
    A = np.zeros((n, n), dtype=np.float64)
    i, j = np.tril_indices(n)
    A[i, j] = np.asarray(lower, dtype=np.float32).astype(np.float64)
    A[j, i] = A[i, j]
    return A


# ---- the model

def tridiagonalise(A):
    """(d, e, tau, V): dsytd2 over rows.  Step j: x = A[j, j+1:], beta = -sign(alpha) ||x||, tau = (beta - alpha) / beta,
    v = x / (alpha - beta) with v_0 = 1; tau = 0 when ||x[1:]|| = 0.  V[j, j+1:] keeps v_j"""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    d, e, tau = np.zeros(n), np.zeros(max(n - 1, 0)), np.zeros(max(n - 1, 0))
    for j in range(n - 1):
        x = A[j, j + 1:].copy()
        alpha = x[0]
        xn2 = float(x[1:] @ x[1:])
        d[j] = A[j, j]
        if xn2 == 0.0:
            e[j] = alpha
            continue
        beta = -math.copysign(math.sqrt(alpha * alpha + xn2), alpha)
        tau[j] = (beta - alpha) / beta
        v = x / (alpha - beta)
        v[0] = 1.0
        e[j] = beta
        A[j, j + 1:] = v
        B = A[j + 1:, j + 1:]
        p = tau[j] * (B @ v)
        w = p - (tau[j] * float(p @ v) / 2.0) * v
        B -= np.outer(v, w) + np.outer(w, v)
    d[n - 1] = A[n - 1, n - 1]
    return d, e, tau, A


def _count_below(d, e2, x, pivmin):
    """the number of eigenvalues below x (d, e2: lists of floats, e2 the squared off-diagonal)"""
    q = d[0] - x
    if abs(q) < pivmin:
        q = -pivmin
    c = q < 0
    for i in range(1, len(d)):
        q = d[i] - x - e2[i - 1] / q
        if abs(q) < pivmin:
            q = -pivmin
        c += q < 0
    return c


def _rng(a):
    s = (0x5EED * 0x100000001B3 + a) & (2 ** 64 - 1)
    while True:
        s = (s + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        z ^= z >> 31
        yield float((z >> 11) | 1) * 2.0 ** -52 - 1.0


def _guard(p, pm):
    return (-pm if p < 0 else pm) if abs(p) < pm else p


def _factor(d, e, lam, pm):
    n = len(d)
    u0, u1, u2, l, sw = [0.0] * n, [0.0] * n, [0.0] * n, [0.0] * n, [0] * n
    cur_d, cur_u = d[0] - lam, (e[0] if n > 1 else 0.0)
    for i in range(n - 1):
        sub, next_d, next_u = e[i], d[i + 1] - lam, (e[i + 1] if i + 2 < n else 0.0)
        if abs(cur_d) >= abs(sub):
            piv = _guard(cur_d, pm)
            m = sub / piv
            u0[i], u1[i], l[i] = piv, cur_u, m
            cur_d, cur_u = next_d - m * cur_u, next_u
        else:
            piv = _guard(sub, pm)
            m = cur_d / piv
            u0[i], u1[i], u2[i], l[i], sw[i] = piv, next_d, next_u, m, 1
            cur_d, cur_u = cur_u - m * next_d, -(m * next_u)
    u0[n - 1] = _guard(cur_d, pm)
    return u0, u1, u2, l, sw


def _solve(f, x):
    u0, u1, u2, l, sw = f
    n = len(x)
    for i in range(n - 1):
        if sw[i]:
            x[i], x[i + 1] = x[i + 1], x[i]
        x[i + 1] -= l[i] * x[i]
    for i in range(n - 1, -1, -1):
        v = x[i]
        if i + 1 < n:
            v -= u1[i] * x[i + 1]
        if i + 2 < n:
            v -= u2[i] * x[i + 2]
        v /= u0[i]
        x[i] = v
        if abs(v) > 2.0 ** 500:
            x = [t * 2.0 ** -500 for t in x]
    return x


def _normalise(x):
    x = np.asarray(x, dtype=np.float64)
    m = float(np.abs(x).max())
    if not (m > 0) or not math.isfinite(m):
        return None
    x = x / m
    return x / math.sqrt(float(x @ x))


def tridiag_eig(d_in, e_in, k):
    """bvcf_pca_tridiag's algorithm -> (values descending, Z (k, n))"""
    d_in, e_in = np.asarray(d_in, dtype=np.float64), np.asarray(e_in, dtype=np.float64)
    n = len(d_in)
    amax = max(float(np.abs(d_in).max()), float(np.abs(e_in).max()) if n > 1 else 0.0)
    if amax == 0.0:
        return np.zeros(k), np.eye(n)[:k].copy()
    ex = math.frexp(amax)[1]
    d, e = np.ldexp(d_in, 1 - ex), np.ldexp(e_in, 1 - ex)
    r = np.zeros(n)
    if n > 1:
        r[1:] += np.abs(e)
        r[:-1] += np.abs(e)
    gl, gu, norm1 = float((d - r).min()), float((d + r).max()), float((np.abs(d) + r).max())
    pivmin, pivot_min = 2.0 ** -1000, EPS * norm1
    slack = 2.0 * EPS * norm1 * n + 2.0 * pivmin
    gl, gu = gl - slack, gu + slack
    vals = np.zeros(k)
    dl, e2 = d.tolist(), (e * e).tolist()
    for a in range(k):
        m = n - 1 - a
        lo, hi = gl, (min(gu, float(vals[a - 1])) if a else gu)
        hi = max(hi, lo)
        while True:
            mid = lo + (hi - lo) / 2.0
            if not (mid > lo) or not (mid < hi):
                break
            if _count_below(dl, e2, mid, pivmin) <= m:
                lo = mid
            else:
                hi = mid
        vals[a] = hi
    thr = norm1 * max(1e-3, 1.0 / n)
    Z = np.zeros((k, n))
    el = e.tolist()
    for a in range(k):
        first = a
        while first > 0 and vals[first - 1] - vals[first] <= thr:
            first -= 1
        f = _factor(dl, el, float(vals[a]), pivot_min)
        g = _rng(a)
        x = [next(g) for _ in range(n)]
        for _ in range(KITERS):
            y = _normalise(_solve(f, list(x)))
            for _ in range(2):  # (two passes of Gram-Schmidt, as the library makes)
                if y is not None and first < a:
                    for b in range(first, a):
                        y = y - float(Z[b] @ y) * Z[b]
                    y = _normalise(y)
            x = [next(g) for _ in range(n)] if y is None else y.tolist()
        y = _normalise(x)
        Z[a] = y if y is not None else np.eye(n)[a]
    return np.ldexp(vals, ex - 1), Z


def back_transform(V, tau, Z):
    """U = H_0 H_1 ... H_{n-2} Z: the reflectors applied in reverse order to every row of Z; normalised, sign rule"""
    k, n = Z.shape
    U = np.array(Z)
    for j in range(n - 2, -1, -1):
        if tau[j] == 0.0:
            continue
        v = V[j, j + 1:]
        U[:, j + 1:] -= np.outer(tau[j] * (U[:, j + 1:] @ v), v)
    out = np.zeros_like(U)
    for a in range(k):
        y = _normalise(U[a])
        out[a] = apply_sign_rule(y if y is not None else U[a])
    return out


def model_eigen(A, k):
    """(values, vectors (k, n)) of the float64 matrix A by the library's algorithm"""
    d, e, tau, V = tridiagonalise(A)
    vals, Z = tridiag_eig(d, e, k)
    return vals, back_transform(V, tau, Z)


# ---- matrix families (all rounded through float32: the solver's input is float32)

FAMILIES = ["grm", "identity", "zero", "rank1", "indefinite", "clustered", "diagonal", "blocks"]


def family(name, n, seed=0, markers=None):
    rng = np.random.default_rng(1000 + 7919 * seed + 31 * n + FAMILIES.index(name))
    if name == "grm":  # standardised genotypes with planted groups: Z Z^T / m
        m, groups = markers or 4 * n + 16, 1 + min(3, n // 2)
        grp = np.arange(n) % groups
        base = rng.uniform(0.1, 0.9, m)
        shift = rng.normal(0.0, 0.12, (groups, m))
        p = np.clip(base[None, :] + shift[grp], 0.02, 0.98)
        g = rng.binomial(2, p).astype(np.float64)
        f = np.clip(g.mean(axis=0) / 2.0, 0.01, 0.99)
        z = (g - 2.0 * f) / np.sqrt(2.0 * f * (1.0 - f))
        A = z @ z.T / m
    elif name == "identity":
        A = np.eye(n)
    elif name == "zero":
        A = np.zeros((n, n))
    elif name == "rank1":
        x = rng.normal(size=n)
        A = np.outer(x, x)
    elif name == "indefinite":
        B = rng.normal(size=(n, n))
        A = (B + B.T) / 2.0
    elif name == "clustered":  # two 5-fold eigenvalues on top of a spread rest (fewer when n is small)
        q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        lam = np.concatenate([np.full(5, 3.0), np.full(5, 2.0), rng.uniform(-1.0, 1.0, max(n - 10, 0))])[:n]
        A = (q * lam[None, :]) @ q.T
    elif name == "diagonal":
        A = np.diag(rng.normal(size=n))
    elif name == "blocks":  # two blocks without a coupling: the reflector of the seam's row has nothing to do, e = 0 there
        h = max(n // 2, 1)
        A = np.zeros((n, n))
        for lo, hi in ((0, h), (h, n)):
            B = rng.normal(size=(hi - lo, hi - lo))
            A[lo:hi, lo:hi] = (B + B.T) / 2.0
    else:
        raise ValueError(name)
    A = (A + A.T) / 2.0
    return from_lower(lower_f32(A), n)


GPU_SIZES = [1, 2, 3, 4, 63, 64, 65, 257, 1000]


def ks_of(n):
    return sorted({1, min(10, n), min(MAX_K, n)})


def gpu_cases():
    """(family, n, k) of tests/test_gpu_pca.py's first test"""
    return [(f, n, k) for f in FAMILIES for n in GPU_SIZES for k in ks_of(n)]


def within_bounds(r):
    return r[0] <= BOUND_RES and r[1] <= BOUND_VAL and r[2] <= BOUND_ORTH


def measure_model(cases):
    """the worst three ratios of the model over cases, and numpy's own worst residual ratio"""
    worst, worst_np = [0.0, 0.0, 0.0], 0.0
    for fam, n, k in cases:
        A = family(fam, n)
        vals, vecs = model_eigen(A, k)
        r = ratios(A, vals, vecs)
        worst = [max(a, b) for a, b in zip(worst, r)]
        w, v = np.linalg.eigh(A)
        if unit(A) > 0:
            worst_np = max(worst_np, float(np.abs(A @ v - v * w[None, :]).max()) / unit(A))
    return worst, worst_np


# ---- a cohort with structure, and the files

def structured_vcf(ns, n_lines, groups, seed):
    """samples of `groups` groups (sample s is in group s % groups) whose allele frequencies are shifted per group and line:
    vcfgen plants no structure, and a cohort without any has no leading components to compare"""
    rng = random.Random(77000 + seed)
    out = [vcfgen.header(ns)]
    for k in range(n_lines):
        base = rng.uniform(0.15, 0.85)
        fr = [min(0.97, max(0.03, base + rng.gauss(0.0, 0.22))) for _ in range(groups)]
        gts = []
        for s in range(ns):
            f = fr[s % groups]
            if rng.random() < 0.01:
                gts.append(".|.")
            else:
                gts.append("%d|%d" % (rng.random() < f, rng.random() < f))
        if all(g in ("0|0", ".|.") for g in gts):
            gts[rng.randrange(ns)] = "0|1"
        out.append(pt.snp_line(100 + 11 * k, gts))
    return "".join(out).encode()


def gap_ratio(A, k):
    """the smallest distance between two of lambda_1 .. lambda_{k+1}, over lambda_1 (numpy's values)"""
    w = np.linalg.eigvalsh(A)[::-1][:k + 1]
    return float(np.min(-np.diff(w))) / float(w[0])


def parse_eigenvec(data):
    """PREFIX.eigenvec -> (header line, names [(fid, iid)], array (samples, k) of the printed numbers, their texts)"""
    lines = data.decode().split("\n")
    assert lines[-1] == "", "the file ends with a newline"
    head, rows = lines[0], [ln.split("\t") for ln in lines[1:-1]]
    names = [(r[0], r[1]) for r in rows]
    texts = [r[2:] for r in rows]
    k = len(head.split("\t")) - 2
    assert all(len(t) == k for t in texts)
    return head, names, np.array([[float(x) for x in t] for t in texts], dtype=np.float64).reshape(len(rows), k), texts


def parse_eigenval(data):
    lines = data.decode().split("\n")
    assert lines[-1] == ""
    return np.array([float(x) for x in lines[:-1]], dtype=np.float64), lines[:-1]


def parse_report(data):
    return dict(ln.split("\t") for ln in data.decode().splitlines())
