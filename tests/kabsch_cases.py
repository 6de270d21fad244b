"""Cases and the independent references of the Kabsch rotation tests (tests/test_kabsch_cpu.py, tests/test_gpu_kabsch.py):
NumPy and plain torch on the CPU, nothing of the op layer.

The function under test: H (3,3) = U diag(s) V^T  ->  R = V diag(1, 1, d) U^T, d = sign det(V U^T) (= sign det H at full
rank).  With the SIGNED spectrum (s_1, s_2, d s_3) R is analytic wherever s_i + e_ij s_j > 0 for all i < j, e_ij = d_i d_j:
at d = +1 everywhere down to rank 2, at d = -1 wherever s_3 stays below s_2.  Coinciding singular values as such are no
poles of R, only of its factors.

Every case is built in float64 as Qa diag(s) Qb^T from seeded proper rotations (det < 0: one column of Qa negated) and
rounded to float32; every reference starts from the rounded float32 values, so the rounding of the input is part of no
error.

References
  ref_rotation   float64 numpy.linalg.svd and the determinant fix.  R is well conditioned where the factors are not (a
                 rotation inside a cluster's plane acts on U and V alike and cancels in V U^T).
  ref_singular_values  the same singular values with s_3 from the exact determinant: accurate relatively, not only
                 to 2^-53 s_1, which a comparison of a tiny s_3 at rtol 2^-23 needs.
  ref_gradient   float64 central differences of ref_rotation, 18 evaluations a matrix, step STEP times the largest
                 singular value.  No autograd, no formula of an SVD's derivative.
  polar_gradient float64 autograd through Newton's iteration X <- (X + X^-T) / 2 for the orthogonal polar factor (R is its
                 transpose where det H > 0): no SVD in it.  It exists to cross-check ref_gradient and needs rank 3.

The reference's own error.  On the accuracy cases with det > 0 and rank 3 (tests/test_kabsch_cpu.py asserts this on every
run) ref_gradient and polar_gradient agree to 7.1e-10 of the gradient's largest entry at STEP = 1e-5; 3e-6 gives
2.4e-9 and 1e-6 4.9e-9 (cancellation, eps / step), 3e-5 gives 1.1e-9 and 1e-4 1.2e-8 (truncation, step^2).  Per sample
the difference is at most 0.047 of a hundredth of the bound below: the reference's own error sits 2000 times under it.

The bound of a float32 gradient, absolute, per sample:

    bound = 32 * 2^-24 * max|g| / conditioning(H)

(the adjoint is four chained 3x3 products of at most 3 roundings each, three rounded factors enter twice each, the
divisions add two: about 20 roundings, taken as 32; 1 / conditioning is the gradient's own magnification of max|g|)."""
import itertools

import numpy as np
import torch

EPS = 2.0 ** -24
GAPS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 0.0)
STEP = 1e-5
ROTATIONS_PER_SPECTRUM = 4


def proper_rotations(rng, n):
    """n proper rotations (float64) from QR factors of normal matrices."""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.einsum("bii->bi", r))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return q


def spectra():
    """-> list of (family, gap or scale, (s1, s2, s3))."""
    out = [("separated", None, (1.0, 0.6, 0.3))]
    out += [("top", g, (1.0 + g, 1.0, 0.4)) for g in GAPS]
    out += [("bottom", g, (1.0, 0.4 + g, 0.4)) for g in GAPS]
    out += [("equal", c, (c, c, c)) for c in (0.5, 1.0, 4.0)]
    out += [("rank2", None, (1.0, 0.5, 0.0))]
    return out


def _is_pole(family, sign):
    return sign < 0 and family in ("bottom", "equal")


def build(s, sign, rng, n=ROTATIONS_PER_SPECTRUM):
    """n matrices Qa diag(s) Qb^T rounded to float32; sign < 0 negates the first column of Qa."""
    qa, qb = proper_rotations(rng, n), proper_rotations(rng, n)
    if sign < 0:
        qa[:, :, 0] = -qa[:, :, 0]
    return np.einsum("bij,j,bkj->bik", qa, np.asarray(s, np.float64), qb).astype(np.float32)


def _collect(want_pole):
    rng = np.random.default_rng(20240)
    mats, labels = [], []
    for (family, param, s), sign in itertools.product(spectra(), (1, -1)):
        H = build(s, sign, rng)                       # always drawn: both lists see the same stream of rotations
        if _is_pole(family, sign) == want_pole:
            mats.append(H)
            labels += [(family, param, sign)] * len(H)
    return np.concatenate(mats), labels


def accuracy_cases():
    """-> H (n,3,3) float32, labels [(family, gap or scale, sign)]: every spectrum and sign at which R is smooth."""
    return _collect(False)


def poison_cases():
    """-> H (m,3,3) float32: the true poles of R -- bottom cluster and all-equal spectra with det < 0 (gap 0 included: an
    exact pole), rank 1 and the zero matrix.  Their own gradients may be anything, inf and NaN included."""
    H, _ = _collect(True)
    rng = np.random.default_rng(20241)
    a, b = rng.standard_normal((4, 3, 1)), rng.standard_normal((4, 1, 3))
    exact = np.diag([1.0, 0.5, -0.5]).astype(np.float32)[None]       # s_2 = s_3 exactly, det < 0
    return np.concatenate([H, (a @ b).astype(np.float32), exact, np.zeros((1, 3, 3), np.float32)])


def signed_permutations():
    """The 24 signed permutation matrices with det +1 (float32), the identity first."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            m[np.arange(3), perm] = signs
            if np.linalg.det(m) > 0:
                out.append(m)
    out.sort(key=lambda m: not np.array_equal(m, np.eye(3)))
    return np.stack(out).astype(np.float32)


def upstream(n, seed=7):
    """(n,3,3) float32 upstream gradients g = dL/dR."""
    return np.random.default_rng(seed).standard_normal((n, 3, 3)).astype(np.float32)


def ref_rotation(H):
    """H (n,3,3) -> R (n,3,3) float64, flipped (n) bool, S (n,3) float64."""
    u, s, vt = np.linalg.svd(np.asarray(H, np.float64))
    v = np.swapaxes(vt, 1, 2)
    flipped = np.linalg.det(v @ np.swapaxes(u, 1, 2)) < 0
    d = np.ones_like(s)
    d[:, 2] = np.where(flipped, -1.0, 1.0)
    return (v * d[:, None, :]) @ np.swapaxes(u, 1, 2), flipped, s


def ref_singular_values(H):
    """(n,3) float64 singular values with a RELATIVE error of a few 2^-53 each, for H whose s_2 is of s_1's order.
    LAPACK's are accurate to 2^-53 s_1 absolutely: nothing for the s_3 ~ 1e-11 that rounding Qa diag(1, .5, 0) Qb^T to
    float32 leaves (the Jacobi kernel, accurate relatively, was seen 4.9e-6 of s_3 = 5e-17 away from LAPACK's).  So s_3
    is taken from |det H| = s_1 s_2 s_3, the determinant in exact rational arithmetic on the float32 entries."""
    from fractions import Fraction
    s = np.linalg.svd(np.asarray(H, np.float64), compute_uv=False)
    for i, h in enumerate(np.asarray(H, np.float64)):
        (a, b, c), (d, e, f), (g, k, l) = [[Fraction(float(x)) for x in row] for row in h]
        det = a * (e * l - f * k) - b * (d * l - f * g) + c * (d * k - e * g)
        s[i, 2] = float(abs(det) / (Fraction(s[i, 0]) * Fraction(s[i, 1])))
    return s


def ref_gradient(H, g, step=STEP):
    """d sum(R * g) / dH, (n,3,3) float64: central differences of ref_rotation."""
    H = np.asarray(H, np.float64)
    g = np.asarray(g, np.float64)
    h = step * np.linalg.svd(H, compute_uv=False)[:, 0]
    out = np.empty_like(H)
    for i, j in itertools.product(range(3), range(3)):
        e = np.zeros_like(H)
        e[:, i, j] = h
        out[:, i, j] = ((ref_rotation(H + e)[0] - ref_rotation(H - e)[0]) * g).sum(axis=(1, 2)) / (2 * h)
    return out


def polar_gradient(H, g, iterations=40):
    """The same gradient for det H > 0 (rank 3) by float64 autograd through Newton's polar iteration."""
    H = torch.as_tensor(np.asarray(H, np.float64)).requires_grad_(True)
    X = H
    for _ in range(iterations):
        X = 0.5 * (X + torch.linalg.inv(X).transpose(1, 2))
    (grad,) = torch.autograd.grad((X.transpose(1, 2) * torch.as_tensor(np.asarray(g, np.float64))).sum(), H)
    return grad.numpy()


def conditioning(H):
    """min over i < j of s_i + e_ij s_j (e_ij = d_i d_j, d = (1, 1, sign det)) from the float64 singular values: the
    smallest denominator of the gradient, (n) float64.  0 at a pole of R."""
    _, flipped, s = ref_rotation(H)
    d3 = np.where(flipped, -1.0, 1.0)
    return np.minimum(s[:, 0] + s[:, 1], np.minimum(s[:, 0] + d3 * s[:, 2], s[:, 1] + d3 * s[:, 2]))


def gradient_bound(H, g):
    """(n) float64: 32 * 2^-24 * max|g| / conditioning(H), absolute, per sample."""
    return 32 * EPS * np.abs(np.asarray(g, np.float64)).max(axis=(1, 2)) / conditioning(H)
