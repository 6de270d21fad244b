"""mvp_kabsch_svd3 (csrc/svd3.hip) and its adjoint (registration.svd3_kabsch_backward, through kabsch_rotation) on the
device, on clustered singular values, structured matrices and the edges of the launch; then the two consumers on clouds
with a symmetry axis.  Cases, references, the gradient's bound and their derivations: tests/kabsch_cases.py.  No test
here differentiates through an SVD: gradients are compared with float64 central differences of float64 forwards.

Observed on an MI355X (every figure is printed on every run):
  forward, accuracy cases        max |R - ref| 2.98e-8 = 2^-25 (bound 2^-23); R(H^T) against R(H)^T: 0
  subnormal inputs               max |R - ref| 2.98e-8; S within 0.48 subnormal ulps: the kernel sees the subnormals
  backward, accuracy cases       max error / bound 0.18
  test_kabsch_rotation_gradient  (tests/test_registration.py, 64 randn matrices) max error / bound 0.18
  procrustes, g_src_corr         max error / bound 0.038 (noise 0: 0.038, 1e-6: 0.024, 1e-4: 0.026, 1e-2: 0.029)
  gmm_register, g_mu_t           max error / bound 0.097 (noise 0: 0.037, 1e-6: 0.097, 1e-4: 0.070, 1e-2: 0.026)
With the general SVD adjoint these tests replaced (division by s_j^2 - s_i^2) the same runs gave error / bound 4.1e5 on
the accuracy cases (NaN at the exact clusters), 1.6e5 for procrustes and 6.3e4 for gmm_register."""
import itertools

import numpy as np
import pytest
import torch

import kabsch_cases as cases

DEV = "cuda:0"
gpu = pytest.mark.gpu
SENTINEL = -777.25


@pytest.fixture(scope="module")
def accuracy():
    H, labels = cases.accuracy_cases()
    g = cases.upstream(len(H))
    R, flipped, S = cases.ref_rotation(H)
    return {"H": H, "labels": labels, "g": g, "R": R, "flipped": flipped, "S": S, "grad": cases.ref_gradient(H, g),
            "bound": cases.gradient_bound(H, g)}


@pytest.fixture(scope="module")
def pool():
    """130 matrices for the launch-shape tests: the accuracy cases and six true poles."""
    return np.concatenate([cases.accuracy_cases()[0], cases.poison_cases()[-6:]])


def run_abi(H, outputs="USVF"):
    """mvp_kabsch_svd3 through the C ABI on buffers one matrix longer than the batch, pre-filled with a sentinel; the
    outputs not named in `outputs` are passed as NULL.  -> dict of numpy arrays (the batch's part), after asserting
    that every sentinel behind the batch survived."""
    from mvp_benchmark_amd import _lib
    H = np.ascontiguousarray(H, np.float32).reshape(-1, 3, 3)
    b = len(H)
    Hd = torch.full((b + 1, 3, 3), SENTINEL, device=DEV)
    Hd[:b] = torch.as_tensor(H)
    buf = {"R": torch.full((b + 1, 3, 3), SENTINEL, device=DEV)}
    for name, shape in (("U", (b + 1, 3, 3)), ("S", (b + 1, 3)), ("V", (b + 1, 3, 3))):
        buf[name] = torch.full(shape, SENTINEL, device=DEV) if name in outputs else None
    buf["F"] = torch.full((b + 1,), -77, device=DEV, dtype=torch.int32) if "F" in outputs else None
    _lib.call("mvp_kabsch_svd3", DEV, b, Hd, buf["R"], buf["U"], buf["S"], buf["V"], buf["F"])
    torch.cuda.synchronize()
    out = {}
    for name, t in buf.items():
        if t is None:
            continue
        t = t.cpu().numpy()
        assert (t[b] == (-77 if name == "F" else np.float32(SENTINEL))).all(), "%s written past the batch" % name
        out[name] = t[:b]
    return out


def _rotation_defect(R):
    R = R.astype(np.float64)
    return max(np.abs(np.einsum("bji,bjk->bik", R, R) - np.eye(3)).max(), np.abs(np.linalg.det(R) - 1.0).max())


# ---------------------------------------------------------------------------------------------------------- forward

@gpu
def test_forward_on_clustered_spectra(accuracy):
    """Every accuracy case: flipped equals the reference's, |R - ref| <= 2^-23 (one ulp at 1.0; a correctly rounded
    float64-accurate entry errs by at most 2^-25), S descending and at rtol 2^-23, U diag(S) V^T = H at 2e-6 of its
    scale, U and V orthogonal at 2^-22.

    S, weakened by an absolute term: |S - ref| <= 2^-23 ref + 16 * 2^-53 s_1.  Reason (svd3.hip): the kernel applies its
    plane rotations in float64 to the columns of H itself (`A[r][q] = sn * ap + cs * aq`, no preconditioning), so each
    column carries an absolute error of a few 2^-53 of the LARGEST column norm, and the norm of a column 1e-11 times
    smaller than its neighbours is known to that absolute error only, as with any float64 SVD of these entries.  The one
    value this concerns is the s_3 = 1.03e-11 that rounding Qa diag(1, .5, 0) Qb^T to float32 leaves in one rank-2 case:
    the kernel is 1.8e-18 = 1.7e-7 s_3 = 0.016 * 2^-53 s_1 away from the exact value (LAPACK: 5.0e-17); every other
    singular value of the accuracy cases is above 4e-10 s_1 and meets the relative bound alone (asserted).  The
    reference is kabsch_cases.ref_singular_values (s_3 from the exact determinant), so that its own error is not part
    of this."""
    H = accuracy["H"]
    out = run_abi(H)
    err = np.abs(out["R"].astype(np.float64) - accuracy["R"]).max()
    print("forward, accuracy cases: max |R - ref| = %.3g (bound %.3g)" % (err, 2.0 ** -23))
    np.testing.assert_array_equal(out["F"].astype(bool), accuracy["flipped"])
    assert err <= 2.0 ** -23
    S = out["S"]
    assert (S[:, 0] >= S[:, 1]).all() and (S[:, 1] >= S[:, 2]).all() and (S >= 0).all()
    ref_S = cases.ref_singular_values(H)
    dev = np.abs(S.astype(np.float64) - ref_S)
    print("forward, accuracy cases: max |S - ref| / ref = %.3g; in units of 2^-53 s_1 where above 2^-23 ref: %.3g"
          % ((dev / ref_S).max(), np.where(dev > 2.0 ** -23 * ref_S, dev / (2.0 ** -53 * ref_S[:, :1]), 0.0).max()))
    assert (dev <= 2.0 ** -23 * ref_S + 16 * 2.0 ** -53 * ref_S[:, :1]).all()
    assert (dev <= 2.0 ** -23 * ref_S)[ref_S > 1e-10 * ref_S[:, :1]].all()
    assert (ref_S <= 1e-10 * ref_S[:, :1]).sum() == 1
    U, V = out["U"].astype(np.float64), out["V"].astype(np.float64)
    scale = np.abs(H).max(axis=(1, 2), keepdims=True).astype(np.float64)
    rec = np.einsum("bij,bj,bkj->bik", U, S.astype(np.float64), V)
    assert (np.abs(rec - H) / scale).max() <= 2e-6
    eye = np.eye(3)
    assert np.abs(np.einsum("bji,bjk->bik", U, U) - eye).max() <= 2.0 ** -22
    assert np.abs(np.einsum("bji,bjk->bik", V, V) - eye).max() <= 2.0 ** -22


@gpu
def test_forward_on_exact_matrices():
    """Signed permutations with det +1 (the identity among them): no rotation is applied, every column norm is 1, and
    R == H^T bit for bit.  diag(3,2,1): R == I, S == (3,2,1).  diag(1,1,-1) and diag(1,.5,-.5) are poles of R (two
    equal singular values behind the reflection): only a finite proper rotation and flipped == 1 are asserted."""
    perms = cases.signed_permutations()
    out = run_abi(perms)
    assert np.array_equal(out["R"], np.swapaxes(perms, 1, 2))
    assert (out["F"] == 0).all() and (out["S"] == 1.0).all()
    special = np.stack([np.diag([3.0, 2.0, 1.0]), np.diag([1.0, 1.0, -1.0]), np.diag([1.0, 0.5, -0.5])])
    out = run_abi(special)
    assert np.array_equal(out["R"][0], np.eye(3, dtype=np.float32)) and np.array_equal(out["S"][0], [3.0, 2.0, 1.0])
    assert list(out["F"]) == [0, 1, 1]
    assert np.isfinite(out["R"]).all() and _rotation_defect(out["R"][1:]) <= 2.0 ** -22


@gpu
def test_forward_transpose_property(accuracy):
    """R(H^T) = R(H)^T (U and V change places), at 2^-22: two results of 2^-24 each, with margin."""
    H = accuracy["H"]
    a = run_abi(H, "")["R"]
    b = run_abi(np.swapaxes(H, 1, 2), "")["R"]
    err = np.abs(a.astype(np.float64) - np.swapaxes(b, 1, 2)).max()
    print("transpose property: max |R(H^T) - R(H)^T| = %.3g" % err)
    assert err <= 2.0 ** -22


@gpu
def test_forward_power_of_two_scaling():
    """Entries in [2^-10, 1], scaled by 2^k: every threshold of the kernel is relative (the rotation test against
    sqrt(alpha beta), the rank tolerance against s_1) and no float64 intermediate leaves its range, so R and flipped
    are bit-equal to k = 0 and S is scaled exactly."""
    rng = np.random.default_rng(11)
    H = np.exp2(rng.uniform(-10.0, 0.0, (128, 3, 3))).astype(np.float32)
    base = run_abi(H)
    assert 16 < base["F"].sum() < 112
    for k in (-100, -50, 50, 100):
        scaled = run_abi(H * np.float32(2.0) ** k)
        assert np.array_equal(scaled["R"], base["R"]) and np.array_equal(scaled["F"], base["F"]), k
        assert np.array_equal(scaled["S"], base["S"] * np.float32(2.0) ** k), k
        assert np.array_equal(scaled["U"], base["U"]) and np.array_equal(scaled["V"], base["V"]), k


@gpu
def test_forward_subnormal_inputs():
    """Entries m * 2^-149 with |m| < 2^12 (all float32 subnormals).  The kernel sees the subnormals, not zeros: the
    loads convert to float64 exactly, and R equals the float64 reference of the same bits at 2^-23 (a kernel reading
    zeros would return the identity).  S, itself subnormal in float32, is the reference's to one subnormal ulp."""
    rng = np.random.default_rng(12)
    m = rng.integers(-4095, 4096, (64, 3, 3))
    H = (m * 2.0 ** -149).astype(np.float32)
    assert np.array_equal(H.astype(np.float64), m * 2.0 ** -149) and (np.abs(H) < np.finfo(np.float32).tiny).all()
    want, flipped, S = cases.ref_rotation(H)
    out = run_abi(H)
    err = np.abs(out["R"].astype(np.float64) - want).max()
    print("subnormal inputs: max |R - ref| = %.3g, S max error %.3g subnormal ulps"
          % (err, np.abs(out["S"].astype(np.float64) - S).max() / 2.0 ** -149))
    np.testing.assert_array_equal(out["F"].astype(bool), flipped)
    assert err <= 2.0 ** -23
    assert np.abs(out["S"].astype(np.float64) - S).max() <= 2.0 ** -149


@gpu
def test_forward_batch_sizes_and_optional_outputs(pool):
    """Batches of 1, 63, 64, 65, 129 and 0 matrices (a block is 64 lanes) with every combination of U, S, V and flipped
    passed as NULL: R, and every output that is asked for, bit-equal to the full run's rows; nothing is written behind
    the batch (run_abi's sentinels)."""
    full = run_abi(pool[:129])
    for b in (1, 63, 64, 65, 129, 0):
        for r in range(5):
            for outputs in itertools.combinations("USVF", r):
                out = run_abi(pool[:b], "".join(outputs))
                assert set(out) == {"R", *outputs}
                for name, t in out.items():
                    assert t.shape == full[name][:b].shape
                    assert np.array_equal(t, full[name][:b], equal_nan=True), (b, outputs, name)


@gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_forward_non_finite_inputs(pool, bad):
    """One matrix among 130 carries a NaN (an Inf); then one matrix for each of the nine positions.  The call returns,
    every other matrix is bit-equal to the clean run, and the poisoned R is NaN throughout rather than a plausible
    rotation (mvpops.h states it; S carries the NaN / Inf of the column's norm)."""
    clean = run_abi(pool)
    H = pool.copy()
    H[64, 1, 2] = bad
    many = pool.copy()
    where = 3 + 14 * np.arange(9)
    many[where, np.arange(9) // 3, np.arange(9) % 3] = bad
    for H, hit in ((H, np.array([64])), (many, where)):
        out = run_abi(H)
        others = np.setdiff1d(np.arange(len(pool)), hit)
        for name in "RUSVF":
            assert np.array_equal(out[name][others], clean[name][others], equal_nan=True), name
        assert np.isnan(out["R"][hit]).all()
        assert not np.isfinite(out["S"][hit]).all(axis=1).any()


# --------------------------------------------------------------------------------------------------------- backward

def _device_gradient(H, g):
    from mvp_benchmark_amd.registration import kabsch_rotation
    Hd = torch.as_tensor(H).to(DEV).requires_grad_(True)
    R = kabsch_rotation(Hd)
    (grad,) = torch.autograd.grad((R * torch.as_tensor(g).to(DEV)).sum(), Hd)
    return R.detach().cpu().numpy(), grad.cpu().numpy()


@gpu
def test_backward_on_clustered_spectra(accuracy):
    """kabsch_rotation's gradient on every accuracy case, exact clusters included, within
    32 * 2^-24 * max|g| / conditioning of the central differences."""
    R, grad = _device_gradient(accuracy["H"], accuracy["g"])
    assert np.abs(R.astype(np.float64) - accuracy["R"]).max() <= 2.0 ** -23
    ratio = np.abs(grad - accuracy["grad"]).max(axis=(1, 2)) / accuracy["bound"]
    print("backward, accuracy cases: max error / bound = %.3g" % np.nanmax(ratio))
    assert np.isfinite(grad).all()
    assert (ratio <= 1.0).all(), sorted({lab for lab, r in zip(accuracy["labels"], ratio) if not r <= 1.0})


@gpu
def test_backward_is_reproducible_and_poles_stay_in_their_sample(accuracy):
    """Two runs are bit-equal; with the poison samples (true poles of R) appended to the batch the gradients of all
    other samples are bit-equal too, and the exact poles show as inf / NaN in their own sample."""
    _, first = _device_gradient(accuracy["H"], accuracy["g"])
    _, second = _device_gradient(accuracy["H"], accuracy["g"])
    assert np.array_equal(first, second)
    P = cases.poison_cases()
    _, mixed = _device_gradient(np.concatenate([accuracy["H"], P]),
                                np.concatenate([accuracy["g"], cases.upstream(len(P), seed=8)]))
    assert np.array_equal(mixed[:len(first)], first)
    assert not np.isfinite(mixed[-2:]).all(axis=(1, 2)).any()        # diag(1, .5, -.5) and the zero matrix


# -------------------------------------------------------------------------------------------------------- consumers

N_PTS = 64
NOISE = (0.0, 1e-6, 1e-4, 1e-2)


def _ring_cloud(rng, stretch):
    """64 points on four rings of 16 about a common axis (radii and heights differ, heights times `stretch`): the
    second-moment matrix about the centroid is diag(a, a, b) in the rings' frame for any weights that are constant on a
    ring.  -> (64, 3) float64 in a randomly rotated frame, and the ring of every point."""
    ang = 2 * np.pi * np.arange(16) / 16
    pts, ring = [], []
    for i, (rad, z) in enumerate(zip((1.0, 0.8, 0.5, 0.3), (-0.6, -0.1, 0.4, 0.9))):
        pts.append(np.stack([rad * np.cos(ang + 0.1 * i), rad * np.sin(ang + 0.1 * i), np.full(16, stretch * z)], axis=1))
        ring += [i] * 16
    return np.concatenate(pts) @ cases.proper_rotations(rng, 1)[0].T, np.array(ring)


def _moved_copies(rng):
    """Per noise level a tall cloud (b > a: the two SMALLEST singular values coincide) and a flat one (b < a: the two
    largest): src (B,64,3), its rotated and translated copy with noise (B,64,3), rings (64)."""
    src, dst = [], []
    for stretch, noise in itertools.product((2.0, 0.3), NOISE):
        pts, ring = _ring_cloud(rng, stretch)
        R0, t0 = cases.proper_rotations(rng, 1)[0], rng.standard_normal(3)
        src.append(pts)
        dst.append(pts @ R0.T + t0 + noise * rng.standard_normal(pts.shape))
    return np.stack(src).astype(np.float32), np.stack(dst).astype(np.float32), ring


def _central_differences(loss, x, step=1e-5):
    """loss: (M, ...) float64 tensor -> (M) losses, one per row; x (B, ...) float64, row i of the result depends on row i
    of x only.  -> d loss_i / d x_i, shape of x: all 2 * D perturbed copies of the batch go through `loss` at once, with
    `reps` = 2 * D telling it how often to repeat its other arguments."""
    B = x.shape[0]
    D = x[0].numel()
    pert = step * torch.eye(D, dtype=torch.float64).reshape(D, 1, *x.shape[1:])
    both = torch.cat([x.unsqueeze(0) + pert, x.unsqueeze(0) - pert]).reshape(2 * D * B, *x.shape[1:])
    vals = loss(both, 2 * D).reshape(2, D, B)
    return ((vals[0] - vals[1]) / (2 * step)).t().reshape(x.shape)


def _assert_clustered(sv):
    """sv (B,3): the tall clouds (first half) have s_2 = s_3, the flat ones s_1 = s_2, to the noise level."""
    half = len(NOISE)
    gap = np.concatenate([sv[:half, 1] - sv[:half, 2], sv[half:, 0] - sv[half:, 1]]) / sv[:, 0]
    print("relative gap of the cluster per cloud: " + ", ".join("%.2g" % x for x in gap))
    assert (gap < 0.02).all() and (gap[[0, 1, half, half + 1]] < 1e-5).all()
    other = np.concatenate([sv[:half, 0] - sv[:half, 1], sv[half:, 1] - sv[half:, 2]]) / sv[:, 0]
    assert (other > 0.1).all()


def _report(name, got, want, bound):
    ratio = np.abs(got - want) / bound
    print("%s: max error / bound = %.3g (per noise level %s)"
          % (name, np.nanmax(ratio), ", ".join("%g: %.2g" % (n, r) for n, r in
                                               zip(NOISE, np.nanmax(ratio.reshape(2, len(NOISE), -1), axis=(0, 2))))))
    assert np.isfinite(got).all()
    assert (ratio <= 1.0).all()


def _reg_model_utils():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("registration_model_utils_kabsch",
                                                  os.path.join(ROOT, "registration", "model_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@gpu
def test_procrustes_gradient_on_a_cloud_with_a_symmetry_axis():
    """procrustes(src, src_corr) on the device, src on rings (H has the spectrum (a, a, b) up to the noise: 0, 1e-6,
    1e-4, 1e-2), loss = <R, w_R> + <t, w_t>, gradient with respect to src_corr against float64 central differences of
    the float64 forward.  Bound: H = src_c corr_c^T is linear in src_corr, so the bound of g_H,
    bH = 32 * 2^-24 * max|g_R| / conditioning(H) with g_R = w_R - w_t src_mean^T, reaches point n as
    bH * (|src_c[:, n]|_1 + mean_m |src_c[:, m]|_1) (the second term: the centring of src_corr)."""
    mu = _reg_model_utils()
    rng = np.random.default_rng(31)
    src, dst, _ = _moved_copies(rng)
    B = len(src)
    w_R, w_t = rng.standard_normal((B, 3, 3)).astype(np.float32), rng.standard_normal((B, 3)).astype(np.float32)
    src_t, dst_t = torch.as_tensor(src).transpose(1, 2), torch.as_tensor(dst).transpose(1, 2)      # (B,3,N)

    def loss64(corr, reps):
        R, t = mu.procrustes(src_t.double().repeat(reps, 1, 1), corr)
        return (R * torch.as_tensor(w_R).double().repeat(reps, 1, 1)).sum(dim=(1, 2)) \
            + (t * torch.as_tensor(w_t).double().repeat(reps, 1)).sum(dim=1)

    want = _central_differences(loss64, dst_t.double().contiguous()).numpy()
    corr = dst_t.contiguous().to(DEV).requires_grad_(True)
    R, t = mu.procrustes(src_t.contiguous().to(DEV), corr)
    assert R.is_cuda and R.dtype == torch.float32
    (got,) = torch.autograd.grad((R * torch.as_tensor(w_R).to(DEV)).sum() + (t * torch.as_tensor(w_t).to(DEV)).sum(), corr)
    s64, d64 = src.astype(np.float64), dst.astype(np.float64)
    sc, dc = s64 - s64.mean(axis=1, keepdims=True), d64 - d64.mean(axis=1, keepdims=True)
    H = np.einsum("bni,bnj->bij", sc, dc)
    sv = np.linalg.svd(H, compute_uv=False)
    _assert_clustered(sv)
    g_R = w_R.astype(np.float64) - np.einsum("bi,bj->bij", w_t.astype(np.float64), s64.mean(axis=1))
    bH = 32 * cases.EPS * np.abs(g_R).max(axis=(1, 2)) / cases.conditioning(H)
    l1 = np.abs(sc).sum(axis=2)                                                # (B,N)
    bound = bH[:, None] * (l1 + l1.mean(axis=1, keepdims=True))
    _report("procrustes g_src_corr", got.cpu().numpy(), want, np.broadcast_to(bound[:, None, :], want.shape))


@gpu
def test_gmm_register_gradient_on_a_mixture_with_a_symmetry_axis():
    """gmm_register on the device with the ring cloud as component means, weights and variances constant on each ring
    (the registration matrix Ms = A^T (mu_t - c_t), A = pi (mu_s - c_s) / sigma, keeps the spectrum (a, a, b)),
    loss = <T, w>, gradient with respect to mu_t against float64 central differences of the float64 forward.  Bound:
    bH = 32 * 2^-24 * max|g_R| / conditioning(Ms) with g_R = w[:3,:3] - w[:3,3] c_s^T reaches component j as
    bH * (|A[j]|_1 + pi_j sum_l |A[l]|_1) (the second term: c_t = pi mu_t)."""
    from mvp_benchmark_amd.registration import gmm_register
    rng = np.random.default_rng(32)
    mu_s, mu_t, ring = _moved_copies(rng)
    B = len(mu_s)
    pi = rng.uniform(0.7, 1.3, (B, 4))[:, ring]
    pi = (pi / pi.sum(axis=1, keepdims=True)).astype(np.float32)
    sigma = rng.uniform(0.5, 1.0, (B, 4))[:, ring].astype(np.float32)
    w = rng.standard_normal((B, 4, 4)).astype(np.float32)
    w[:, 3] = 0.0
    ten = lambda a: torch.as_tensor(a)

    def loss64(m_t, reps):
        T = gmm_register(ten(pi).double().repeat(reps, 1), ten(mu_s).double().repeat(reps, 1, 1), m_t,
                         ten(sigma).double().repeat(reps, 1))
        return (T * ten(w).double().repeat(reps, 1, 1)).sum(dim=(1, 2))

    want = _central_differences(loss64, ten(mu_t).double()).numpy()
    m_t = ten(mu_t).to(DEV).requires_grad_(True)
    T = gmm_register(ten(pi).to(DEV), ten(mu_s).to(DEV), m_t, ten(sigma).to(DEV))
    assert T.is_cuda and T.dtype == torch.float32
    (got,) = torch.autograd.grad((T * ten(w).to(DEV)).sum(), m_t)
    p64, s64, t64, v64 = (a.astype(np.float64) for a in (pi, mu_s, mu_t, sigma))
    c_s, c_t = np.einsum("bj,bjk->bk", p64, s64), np.einsum("bj,bjk->bk", p64, t64)
    A = p64[:, :, None] * (s64 - c_s[:, None]) / v64[:, :, None]                # (B,J,3)
    Ms = np.einsum("bji,bjk->bik", A, t64 - c_t[:, None])
    sv = np.linalg.svd(Ms, compute_uv=False)
    _assert_clustered(sv)
    g_R = w[:, :3, :3].astype(np.float64) - np.einsum("bi,bj->bij", w[:, :3, 3].astype(np.float64), c_s)
    bH = 32 * cases.EPS * np.abs(g_R).max(axis=(1, 2)) / cases.conditioning(Ms)
    l1 = np.abs(A).sum(axis=2)                                                 # (B,J)
    bound = bH[:, None] * (l1 + p64 * l1.sum(axis=1, keepdims=True))
    _report("gmm_register g_mu_t", got.cpu().numpy(), want, np.broadcast_to(bound[:, :, None], want.shape))
