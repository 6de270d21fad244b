"""svd3_kabsch_backward (mvp_benchmark_amd/registration.py) on clustered singular values, on the CPU: the adjoint is fed
float64 factors from torch.linalg.svd -- as they are, and rounded to float32, which is what mvp_kabsch_svd3 hands it on
the device -- and compared with float64 central differences of the rotation itself (tests/kabsch_cases.py: cases,
references, the bound and its derivation).  No test here differentiates through an SVD.

Observed (printed on every run):
  reference against the Newton polar autograd, det > 0 and rank 3:   7.1e-10 of the gradient's largest entry,
                                                                      0.047 of bound / 100
  float64 adjoint against the reference, all accuracy cases:          1.6e-9 of the gradient's largest entry
  float32 adjoint, error / bound, all accuracy cases:                 0.19 (gap 0 included; all-equal spectrum)
The general SVD adjoint this one replaced gave, on the same cases and under the same bound: 0.37 at gap 1e-1, 4.4 at
1e-2, 68 at 1e-3, 4.6e2 at 1e-4, 2.5e3 at 1e-5, 3.6e4 at 1e-6, 4.1e5 at 1e-7, NaN at 0."""
import numpy as np
import pytest
import torch

import kabsch_cases as cases


@pytest.fixture(scope="module")
def accuracy():
    """H, labels, g, the reference gradient and the bound of the accuracy cases, computed once."""
    H, labels = cases.accuracy_cases()
    g = cases.upstream(len(H))
    return {"H": H, "labels": labels, "g": g, "ref": cases.ref_gradient(H, g), "bound": cases.gradient_bound(H, g)}


def _factors(H, dtype):
    """float64 torch.linalg.svd of H (float32 values) -> U, S, V, flipped, the factors rounded to `dtype`."""
    U, S, Vh = torch.linalg.svd(torch.as_tensor(H).double())
    V = Vh.transpose(1, 2)
    flipped = (torch.linalg.det(V @ U.transpose(1, 2)) < 0).int()
    return U.to(dtype), S.to(dtype), V.to(dtype), flipped


def _adjoint(H, g, dtype):
    from mvp_benchmark_amd.registration import svd3_kabsch_backward
    U, S, V, flipped = _factors(H, dtype)
    return svd3_kabsch_backward(U, S, V, flipped, torch.as_tensor(g).to(dtype)).double().numpy()


def _per_sample(x):
    return np.abs(x).max(axis=(1, 2))


def test_cases_cover_what_they_claim():
    H, labels = cases.accuracy_cases()
    s = np.linalg.svd(H.astype(np.float64), compute_uv=False)
    cond = cases.conditioning(H)
    assert len(H) == 31 * cases.ROTATIONS_PER_SPECTRUM and H.dtype == np.float32
    assert cond.min() > 0.299 and (s[:, 0] / cond).max() < 3.4
    dets = np.linalg.det(H.astype(np.float64))
    full = np.array([fam != "rank2" for fam, _, _ in labels])
    assert (np.sign(dets[full]) == np.array([sign for _, _, sign in labels])[full]).all()
    assert (np.abs(dets[~full]) < 1e-7).all()
    # the exact clusters survive the rounding to float32 as clusters: gaps of a few ulps, far below every other gap
    top0 = np.array([fam == "top" and p == 0.0 for fam, p, _ in labels])
    equal = np.array([fam == "equal" for fam, _, _ in labels])
    assert top0.sum() == 8 and (s[top0, 0] - s[top0, 1] < 4e-7).all()
    assert ((s[equal, 0] - s[equal, 2]) / s[equal, 0] < 4e-7).all()
    # the poison samples are poles: the denominator vanishes (to rounding) or, along the bottom family, shrinks to it
    P = cases.poison_cases()
    pc = cases.conditioning(P)
    assert len(P) == 11 * cases.ROTATIONS_PER_SPECTRUM + 6
    assert (pc < 0.11).all() and (pc[-6:] < 1e-6).all() and (pc[-2:] == 0).all()
    # the relatively accurate singular values are LAPACK's to LAPACK's own (absolute) error: s_3 inherits s_1's and s_2's
    assert (np.abs(cases.ref_singular_values(H) - s) <= 16 * 2.0 ** -53 * s[:, :1]).all()
    perms = cases.signed_permutations()
    assert perms.shape == (24, 3, 3) and np.array_equal(perms[0], np.eye(3, dtype=np.float32))
    assert len({p.tobytes() for p in perms}) == 24 and np.allclose(np.linalg.det(perms), 1.0)


def test_reference_gradient_agrees_with_polar_autograd(accuracy):
    """Where both exist (det > 0, rank 3) the central differences and the autograd through Newton's polar iteration
    differ by less than a hundredth of the bound: the reference's own error."""
    sel = np.array([sign > 0 and fam != "rank2" for fam, _, sign in accuracy["labels"]])
    assert sel.sum() == 20 * cases.ROTATIONS_PER_SPECTRUM
    polar = cases.polar_gradient(accuracy["H"][sel], accuracy["g"][sel])
    diff = _per_sample(accuracy["ref"][sel] - polar)
    print("reference vs polar autograd: %.3g of the gradient's largest entry, %.3g of bound / 100"
          % ((diff / _per_sample(polar)).max(), (100 * diff / accuracy["bound"][sel]).max()))
    assert (diff <= accuracy["bound"][sel] / 100).all()


def test_adjoint_float64_matches_central_differences(accuracy):
    """Every accuracy case, det < 0 and rank 2 included: 1e-8 of the gradient's largest entry, ten times what the
    reference was seen to agree with the polar autograd and still below a fiftieth of the float32 bound."""
    got = _adjoint(accuracy["H"], accuracy["g"], torch.float64)
    rel = _per_sample(got - accuracy["ref"]) / _per_sample(accuracy["ref"])
    print("float64 adjoint vs reference: %.3g of the gradient's largest entry" % rel.max())
    assert np.isfinite(got).all()
    assert (rel <= 1e-8).all(), rel.max()
    assert (1e-8 * _per_sample(accuracy["ref"]) <= accuracy["bound"] / 50).all()


def test_adjoint_float32_within_the_bound(accuracy):
    """Factors rounded to float32: every sample within 32 * 2^-24 * max|g| / conditioning, exact clusters included."""
    got = _adjoint(accuracy["H"], accuracy["g"], torch.float32)
    ratio = _per_sample(got - accuracy["ref"]) / accuracy["bound"]
    worst = {}
    for (fam, p, _), r in zip(accuracy["labels"], ratio):
        worst[(fam, p)] = r if np.isnan(r) else max(worst.get((fam, p), 0.0), r)
    print("float32 adjoint, error / bound: max %.3g" % np.nanmax(ratio))
    print("  " + ", ".join("%s %s: %.2g" % (fam, p, r) for (fam, p), r in worst.items()))
    assert np.isfinite(got).all(), sorted({(fam, p) for (fam, p), r in worst.items() if np.isnan(r)})
    assert (ratio <= 1.0).all(), {k: r for k, r in worst.items() if r > 1.0}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_poles_stay_in_their_own_sample(accuracy, dtype):
    """The poison samples appended to the batch: every other gradient bit-equal, and the exact poles show as inf / NaN
    (IEEE division, nothing masked, no epsilon)."""
    P = cases.poison_cases()
    H = np.concatenate([accuracy["H"], P])
    g = np.concatenate([accuracy["g"], cases.upstream(len(P), seed=8)])
    alone = _adjoint(accuracy["H"], accuracy["g"], dtype)
    mixed = _adjoint(H, g, dtype)
    n = len(accuracy["H"])
    assert np.array_equal(mixed[:n], alone)
    assert not np.isfinite(mixed[-2:]).all(axis=(1, 2)).any()        # diag(1, .5, -.5) and the zero matrix
