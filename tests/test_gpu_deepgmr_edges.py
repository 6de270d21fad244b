"""DeepGMR kernels (mvp_rri_features, mvp_gmm_params, mvp_gmm_params_backward) at the shapes and inputs where kernels
go wrong, and the gradient path of the model.

GPU, through the C entry points: every output lies inside a larger buffer whose margins and interior hold a sentinel
NaN (a payload no arithmetic produces), so a store past either end and an element left unwritten are both seen.
Shapes below one workgroup, at and around tile multiples, the cfg batch; bit-exact invariances (batch, permutation,
zero upstream gradient); float64 as judge for the softmax range, an off-centre cloud, empty components; hand-built
neighbour lists with points at the origin.  Wrappers: gmm_register on the device, non-contiguous inputs, a side stream.
Model: parameter gradients of float32 (CPU and GPU) against the float64 model for the three variants, and the eval
forward of the two variants without RRI against the reference's fixture.

The CPU tests here calibrate the GPU ones: they show that the float32 torch formulations meet the same bounds (so a
bound is the format's, not the kernel's) and that a nearly right formulation (one-pass variance) does not."""
import math

import numpy as np
import pytest
import torch

from test_deepgmr import DEV, _check_rri, _gmm_inputs, _golden, _model

EPS = 2.0 ** -24          # float32 unit roundoff
SENTINEL = 0x7FC5A5A5     # a quiet NaN with a payload: arithmetic yields 0x7FC00000 / 0xFFC00000 or an input's payload
MARGIN = 1024             # floats on each side; keeps the interior 256-byte aligned like a fresh allocation


# ------------------------------------------------------------------------------------------------- guarded outputs

class _Guarded:
    """A float32 output of `shape` inside a sentinel-filled buffer."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.raw = torch.full((self.n + 2 * MARGIN,), SENTINEL, dtype=torch.int32, device=DEV)
        self.t = self.raw[MARGIN:MARGIN + self.n].view(torch.float32).view(*shape)

    def check(self, what):
        raw = self.raw.cpu()
        assert (raw[:MARGIN] == SENTINEL).all(), "%s: store in front of the output" % what
        assert (raw[MARGIN + self.n:] == SENTINEL).all(), "%s: store past the end of the output" % what
        missed = (raw[MARGIN:MARGIN + self.n] == SENTINEL).nonzero().flatten()
        assert missed.numel() == 0, "%s: %d elements never written, first %s" % (what, missed.numel(), missed[:4].tolist())
        return self.t.clone()


def _rri(xyz, idx):
    from mvp_benchmark_amd._lib import call
    B, N, k = idx.shape
    out = _Guarded(B, 4 * k, N)
    call("mvp_rri_features", DEV, B, N, k, xyz, idx, out.t)
    torch.cuda.synchronize()
    return out.check("rri feat")


def _gmm_forward(logits, xyz):
    from mvp_benchmark_amd._lib import call
    B, J, N = logits.shape
    outs = [_Guarded(B, N, J), _Guarded(B, J), _Guarded(B, J, 3), _Guarded(B, J)]
    call("mvp_gmm_params", DEV, B, N, J, logits, xyz, *[o.t for o in outs])
    torch.cuda.synchronize()
    return [o.check(name) for o, name in zip(outs, ("gamma", "pi", "mu", "sigma"))]


def _gmm_backward(gamma, xyz, pi, mu, sigma, g_pi, g_mu, g_sigma):
    from mvp_benchmark_amd._lib import call
    B, N, J = gamma.shape
    out = _Guarded(B, J, N)
    call("mvp_gmm_params_backward", DEV, B, N, J, gamma, xyz, pi, mu, sigma, g_pi, g_mu, g_sigma, out.t)
    torch.cuda.synchronize()
    return out.check("g_logits")


def _gmm_float64(logits, xyz, grads):
    """-> (gamma, pi, mu, sigma), g_logits of the float64 reference formulation under autograd."""
    from mvp_benchmark_amd.registration import _gmm_params_reference
    l64 = logits.double().cpu().requires_grad_(True)
    want = _gmm_params_reference(l64, xyz.double().cpu())
    g_pi, g_mu, g_sigma = (g.double().cpu() for g in grads)
    (g_lg,) = torch.autograd.grad((want[1] * g_pi).sum() + (want[2] * g_mu).sum() + (want[3] * g_sigma).sum(), l64)
    return [w.detach() for w in want], g_lg


# tolerances of test_gmm_params_forward_backward_match_float64
GMM_RTOL, GMM_ATOL = 1e-4, (2e-7, 1e-6, 1e-5, 1e-5)


def _assert_gmm_forward(got, want, atol=GMM_ATOL):
    for name, g, w, tol in zip(("gamma", "pi", "mu", "sigma"), got, want, atol):
        torch.testing.assert_close(g.double().cpu(), w, rtol=GMM_RTOL, atol=tol, msg=lambda m, name=name: name + ": " + m)


def _assert_gmm_backward(g_lg, want):
    scale = want.abs().max()
    assert (g_lg.double().cpu() - want).abs().max() <= 1e-4 * scale


# ------------------------------------------------------------------------------------------ 1. shapes and bounds

# (B, N, J): N in {1, 2, 63, 64, 65, 255, 256, 257, 2048, 16384}, J in {1, 2, 15, 16, 17, 63, 64}, B in {1, 32}
GMM_SHAPES = [(1, 1, 1), (32, 1, 64), (1, 2, 16), (32, 2, 2), (1, 63, 15), (32, 64, 16), (1, 65, 17), (1, 255, 63),
              (32, 256, 64), (1, 257, 16), (32, 257, 1), (32, 2048, 16), (1, 2048, 2), (1, 16384, 64), (1, 16384, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,J", GMM_SHAPES)
def test_gmm_kernels_match_float64_at_edge_shapes(B, N, J):
    logits, xyz, grads = _gmm_inputs(B, J, N, 100 + N + J)
    want, w_lg = _gmm_float64(logits, xyz, grads)
    got = _gmm_forward(logits.to(DEV), xyz.to(DEV))
    _assert_gmm_forward(got, want)
    g_lg = _gmm_backward(got[0], xyz.to(DEV), *got[1:], *[g.to(DEV) for g in grads])
    _assert_gmm_backward(g_lg, w_lg)
    if N == 1:
        # one point: mu_j = (gamma_j p) / gamma_j and sigma_j = gamma_j |p - mu_j|^2 / gamma_j.  Exact where gamma = 1
        # (J = 1).  Else the product and the quotient round once each, so mu is within (1 + EPS)^2 of p, 1 ulp, and
        # sigma at most 3 (2 EPS |p|_max)^2, up to its own roundings (factor 2)
        p = xyz.expand(B, J, 3)
        mu, sigma = got[2].cpu(), got[3].cpu()
        if J == 1:
            assert torch.equal(mu, p) and (sigma == 0).all()
        assert ((mu - p).abs() <= 2 * EPS * p.abs()).all()
        assert (sigma <= 2 * 3 * (2 * EPS * p.abs().amax(dim=2)) ** 2).all() and (sigma >= 0).all()


# (B, N, k): k in {2, 3, 4, 5, 7, 20, 63, 64}; N = k + 1 upwards, 63, 64, 65, 128, 2048; the cfg shape last
RRI_SHAPES = [(1, 3, 2), (2, 4, 3), (1, 5, 4), (2, 6, 5), (1, 8, 7), (1, 21, 20), (1, 64, 63), (1, 65, 64),
              (2, 63, 5), (2, 64, 7), (2, 65, 20), (1, 128, 64), (2, 128, 3), (1, 2048, 63), (2, 2048, 4),
              (32, 2048, 20)]


def _rri_case(B, N, k):
    """Clouds in the centred unit cube and the float32 reference's own neighbours (topk of the expanded distance, self
    column dropped), computed on the CPU so that the CPU calibration and the kernel see the same lists."""
    from mvp_benchmark_amd.registration import _knn_reference
    gen = torch.Generator().manual_seed(1000 * k + N)
    xyz = torch.rand(B, N, 3, generator=gen) - 0.5
    idx = torch.cat([_knn_reference(xyz[b:b + 1], k + 1)[:, :, 1:] for b in range(B)]).int()
    return xyz, idx


def _check_rri_in_chunks(feat, xyz, idx):
    """_check_rri four clouds at a time (its (B,N,k,k,3) float64 temporaries), ties added up."""
    return sum(_check_rri(feat[b:b + 4], xyz[b:b + 4], idx[b:b + 4]) for b in range(0, xyz.shape[0], 4))


def _tie_cap(B, N, k):
    return 3 * B * N * k // 1000       # 3 per 1000 slots


@pytest.mark.parametrize("B,N,k", RRI_SHAPES)
def test_rri_cases_stay_inside_the_tie_cap_in_float32_torch(B, N, k):
    """Without the kernel: the float32 torch formulation on the seeds of RRI_SHAPES passes _check_rri with at most
    the capped number of verified ties, so a kernel that exceeds the cap there is wrong, not unlucky."""
    from mvp_benchmark_amd.registration import _rri_reference
    xyz, idx = _rri_case(B, N, k)
    ties = _check_rri_in_chunks(_rri_reference(xyz, idx.long()), xyz, idx)
    print("float32 torch phi ties at", (B, N, k), ":", ties, "cap", _tie_cap(B, N, k))
    assert ties <= _tie_cap(B, N, k)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,k", RRI_SHAPES)
def test_rri_kernel_matches_float64_at_edge_shapes(B, N, k):
    xyz, idx = _rri_case(B, N, k)
    feat = _rri(xyz.to(DEV), idx.to(DEV))
    ties = _check_rri_in_chunks(feat, xyz, idx)
    print("kernel phi ties at", (B, N, k), ":", ties, "cap", _tie_cap(B, N, k))
    assert ties <= _tie_cap(B, N, k)


# ------------------------------------------------------------------------------------------- 1. exact invariances

@pytest.mark.gpu
def test_deepgmr_kernels_cloud_of_a_batch_equals_the_cloud_alone():
    xyz, idx = _rri_case(3, 200, 20)
    feat = _rri(xyz.to(DEV), idx.to(DEV))
    logits, pts, grads = _gmm_inputs(3, 16, 777, 31)
    fwd = _gmm_forward(logits.to(DEV), pts.to(DEV))
    bwd = _gmm_backward(fwd[0], pts.to(DEV), *fwd[1:], *[g.to(DEV) for g in grads])
    for b in range(3):
        s = slice(b, b + 1)
        assert torch.equal(_rri(xyz[s].to(DEV), idx[s].to(DEV)), feat[s])
        alone = _gmm_forward(logits[s].to(DEV), pts[s].to(DEV))
        for a, f in zip(alone, fwd):
            assert torch.equal(a, f[s])
        assert torch.equal(_gmm_backward(alone[0], pts[s].to(DEV), *alone[1:], *[g[s].to(DEV) for g in grads]), bwd[s])


@pytest.mark.gpu
def test_deepgmr_kernels_commute_with_a_permutation_of_the_points():
    gen = torch.Generator().manual_seed(77)
    # RRI: point perm[i] moves to place i, the lists name the new places
    B, N, k = 2, 333, 20
    xyz, idx = _rri_case(B, N, k)
    perm = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)])
    inv = torch.empty_like(perm)
    for b in range(B):
        inv[b, perm[b]] = torch.arange(N)
    xyz_p = torch.stack([xyz[b, perm[b]] for b in range(B)])
    idx_p = torch.stack([inv[b][idx[b, perm[b]].long()] for b in range(B)]).int()
    feat, feat_p = _rri(xyz.to(DEV), idx.to(DEV)).cpu(), _rri(xyz_p.to(DEV), idx_p.to(DEV)).cpu()
    for b in range(B):
        assert torch.equal(feat_p[b], feat[b][:, perm[b]])
    # GMM: gamma and the backward are per point (bit-equal); pi, mu, sigma sum in another order (float64 judges)
    B, J, N = 2, 16, 1500
    logits, pts, grads = _gmm_inputs(B, J, N, 32)
    perm = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)])
    logits_p = torch.stack([logits[b][:, perm[b]] for b in range(B)])
    pts_p = torch.stack([pts[b, perm[b]] for b in range(B)])
    fwd, fwd_p = _gmm_forward(logits.to(DEV), pts.to(DEV)), _gmm_forward(logits_p.to(DEV), pts_p.to(DEV))
    for b in range(B):
        assert torch.equal(fwd_p[0][b].cpu(), fwd[0][b].cpu()[perm[b]])
    want, _ = _gmm_float64(logits, pts, grads)
    _assert_gmm_forward(fwd_p[1:], want[1:], GMM_ATOL[1:])
    # the backward reads pi, mu, sigma as arguments: the same ones for both orders
    dgrads = [g.to(DEV) for g in grads]
    bwd = _gmm_backward(fwd[0], pts.to(DEV), *fwd[1:], *dgrads).cpu()
    bwd_p = _gmm_backward(fwd_p[0], pts_p.to(DEV), *fwd[1:], *dgrads).cpu()
    for b in range(B):
        assert torch.equal(bwd_p[b], bwd[b][:, perm[b]])


@pytest.mark.gpu
def test_gmm_backward_zero_and_single_upstream_gradients():
    """All three upstream gradients zero: exactly zero.  Each alone: float64 autograd.  sum_j g_logits = 0 at every
    point up to the rounding of that sum."""
    from mvp_benchmark_amd.registration import gmm_params_backward_reference
    B, J, N = 2, 16, 2048
    # logits of unit spread: no gamma of a point is within rounding of 1.  (Where one is, every g_logits of the point
    # cancels towards 0 while the rounding of sum_j gamma_j g_gamma_j does not, and no bound in terms of
    # max_j |g_logits| holds, for the float32 torch closed form either.)
    gen = torch.Generator().manual_seed(6)
    logits = torch.randn(B, J, N, generator=gen)
    xyz = torch.rand(B, N, 3, generator=gen) - 0.5
    grads = [torch.randn(*s, generator=gen) for s in ((B, J), (B, J, 3), (B, J))]
    fwd = _gmm_forward(logits.to(DEV), xyz.to(DEV))
    zeros = [torch.zeros_like(g) for g in grads]
    out = _gmm_backward(fwd[0], xyz.to(DEV), *fwd[1:], *[z.to(DEV) for z in zeros])
    assert (out == 0).all()
    for which in range(3):
        only = [g if i == which else z for i, (g, z) in enumerate(zip(grads, zeros))]
        _, want = _gmm_float64(logits, xyz, only)
        got = _gmm_backward(fwd[0], xyz.to(DEV), *fwd[1:], *[g.to(DEV) for g in only]).cpu()
        _assert_gmm_backward(got, want)
        # |sum_j g_logits| <= C J EPS max_j |g_logits| per point, C = 8.  The float32 torch closed form on these
        # inputs reaches C = 2.0 (g_pi alone; 0.9 and 1.1 for g_mu and g_sigma; up to 3.0 with another host's
        # vectorisation); the kernel adds in another order and gets 4 times the 2.0.  (The first-order worst case, every rounding aligned, is (2 kappa + 1) with kappa =
        # sum_j gamma_j |g_gamma_j| / max_j |g_logits_j| <= 20 on these inputs: far above either.)
        cpu = gmm_params_backward_reference(*[t.cpu() for t in fwd[:1]], xyz, *[t.cpu() for t in fwd[1:]], *only)
        ratios = [(t.double().sum(dim=1).abs() / (J * EPS * t.abs().amax(dim=1).double())).max().item()
                  for t in (got, cpu)]
        print("sum_j g_logits / (J EPS max_j |g_logits|), gradient %d alone: kernel %.2f, float32 torch %.2f"
              % (which, *ratios))
        assert ratios[0] <= 8.0


# ------------------------------------------------------------------------------------------------- 2. numerics

def _wide_logits(B, J, N, seed):
    """Per-point maximum near +90 (even points) and -90 (odd points), spread over 104 = ln(2^150): expf of a raw
    logit overflows (> 88.7) or underflows, and the lowest gammas of a point are exactly 0 in float32."""
    gen = torch.Generator().manual_seed(seed)
    logits = -120.0 * torch.rand(B, J, N, generator=gen)
    top = torch.randint(0, J, (B, 1, N), generator=gen)
    logits.scatter_(1, top, 0.0)
    logits[:, :, 0::2] += 90.0
    logits[:, :, 1::2] -= 90.0
    return logits


@pytest.mark.gpu
def test_gmm_softmax_survives_logits_beyond_the_range_of_expf():
    B, J, N = 2, 16, 2048
    logits = _wide_logits(B, J, N, 41)
    gen = torch.Generator().manual_seed(42)
    xyz = torch.rand(B, N, 3, generator=gen) - 0.5
    grads = [torch.randn(*s, generator=gen) for s in ((B, J), (B, J, 3), (B, J))]
    top = logits.amax(dim=1)
    assert (top[:, 0::2] == 90.0).all() and (top[:, 1::2] == -90.0).all()
    assert ((top - logits.amin(dim=1)) > 104.0).float().mean() > 0.5
    want, w_lg = _gmm_float64(logits, xyz, grads)
    got = _gmm_forward(logits.to(DEV), xyz.to(DEV))
    for t in got:
        assert torch.isfinite(t).all()
    assert (got[0] == 0).any()
    _assert_gmm_forward(got, want)
    g_lg = _gmm_backward(got[0], xyz.to(DEV), *got[1:], *[g.to(DEV) for g in grads])
    _assert_gmm_backward(g_lg, w_lg)


SHIFT = (100.0, -50.0, 25.0)
# mu of the shifted cloud: sum_n gamma p / sum_n gamma, every p within 0.5 of the shift s.  The stored p carries no
# error (float64 runs on the same float32 inputs); each product gamma p rounds once and the two sums are trees of depth
# ~ N / 256 + 12 in the kernel, blocked in torch, whose rounding errors largely cancel in the quotient because all
# terms of one coordinate have one sign.  What remains is a few roundings of a number of size |s|: tolerance 8 ulp of
# the largest shift, ulp(100) = 2^-17, 6.1e-5.  Measured for the float32 torch formulation: 2.4e-5 (3.2 ulp).
MU_ATOL_SHIFTED = 8 * 2.0 ** -17


def _shifted_case():
    gen = torch.Generator().manual_seed(21)
    B, J, N = 2, 16, 2048
    logits = 3.0 * torch.randn(B, J, N, generator=gen)
    xyz = torch.rand(B, N, 3, generator=gen) - 0.5 + torch.tensor(SHIFT)
    return logits, xyz


def test_off_centre_cloud_separates_two_pass_from_one_pass_variance_in_float32():
    """Calibration on the CPU: on the shifted cloud the float32 two-pass formulation meets the mu and sigma bounds
    against float64 and a one-pass E[|p|^2] - |mu|^2 in float32 misses sigma's (3e-2 against rtol 1e-4)."""
    from mvp_benchmark_amd.registration import _gmm_params_reference
    logits, xyz = _shifted_case()
    g32 = _gmm_params_reference(logits, xyz)
    g64 = _gmm_params_reference(logits.double(), xyz.double())
    assert (g32[2].double() - g64[2]).abs().max() <= MU_ATOL_SHIFTED
    torch.testing.assert_close(g32[3].double(), g64[3], rtol=GMM_RTOL, atol=0)     # measured 1.5e-7
    npi = g32[1] * xyz.shape[1]
    one_pass = (g32[0].transpose(1, 2) @ (xyz * xyz).sum(dim=2, keepdim=True)).squeeze(2) / npi - (g32[2] ** 2).sum(dim=2)
    assert ((one_pass.double() - g64[3]).abs() / g64[3]).max() > 100 * GMM_RTOL    # measured 3.2e-2


@pytest.mark.gpu
def test_gmm_variance_of_an_off_centre_cloud():
    from mvp_benchmark_amd.registration import _gmm_params_reference
    logits, xyz = _shifted_case()
    want = _gmm_params_reference(logits.double(), xyz.double())
    got = _gmm_forward(logits.to(DEV), xyz.to(DEV))
    print("shifted cloud: mu error %.3g (bound %.3g), sigma relative error %.3g"
          % ((got[2].double().cpu() - want[2]).abs().max(), MU_ATOL_SHIFTED,
             ((got[3].double().cpu() - want[3]).abs() / want[3]).max()))
    _assert_gmm_forward(got[:2], want[:2])
    assert (got[2].double().cpu() - want[2]).abs().max() <= MU_ATOL_SHIFTED
    torch.testing.assert_close(got[3].double().cpu(), want[3], rtol=GMM_RTOL, atol=0)


def _sparse_case():
    """Cloud 0: component 2 has gamma exactly 0 at every point (float32), component 4 has pi ~ 1e-21, component 6 owns
    point 17 alone.  Cloud 1: the same without the empty component."""
    gen = torch.Generator().manual_seed(22)
    B, J, N = 2, 8, 300
    logits = torch.randn(B, J, N, generator=gen)
    xyz = torch.rand(B, N, 3, generator=gen) - 0.5
    logits[0, 2, :] = -200.0
    logits[:, 4, :] = -46.0
    logits[:, 6, :] = -200.0
    logits[:, 6, 17] = 30.0
    grads = [torch.randn(*s, generator=gen) for s in ((B, J), (B, J, 3), (B, J))]
    return logits, xyz, grads


def test_empty_component_nan_pattern_of_the_references():
    """What the references give for an empty component, without the kernel.  Forward, float32: pi = 0, mu and sigma of
    that component alone NaN (0 / 0).  Backward, float32 closed form and float32 autograd alike: every g_logits of
    that cloud is NaN (the softmax backward's sum over j meets 0 * NaN), while float64 autograd is finite everywhere
    (its pi is 2e-88, not 0).  The two disagree; the kernel follows the closed form."""
    from mvp_benchmark_amd.registration import _gmm_params_reference, gmm_params_backward_reference
    logits, xyz, grads = _sparse_case()
    gamma, pi, mu, sigma = _gmm_params_reference(logits, xyz)
    assert (gamma[0, :, 2] == 0).all() and pi[0, 2] == 0 and 0 < pi[0, 4] < 1e-20 and 0 < pi[1, 4] < 1e-20
    assert torch.equal(mu[:, 6], xyz[:, 17]) and (sigma[:, 6] == 0).all()
    nan_mu = torch.zeros(2, 8, dtype=torch.bool)
    nan_mu[0, 2] = True
    assert torch.equal(torch.isnan(mu), nan_mu.unsqueeze(2).expand(2, 8, 3)) and torch.equal(torch.isnan(sigma), nan_mu)
    closed = gmm_params_backward_reference(gamma, xyz, pi, mu, sigma, *grads)
    assert torch.isnan(closed[0]).all() and torch.isfinite(closed[1]).all()
    _, auto64 = _gmm_float64(logits, xyz, grads)
    assert torch.isfinite(auto64).all()


@pytest.mark.gpu
def test_gmm_empty_and_nearly_empty_components():
    from mvp_benchmark_amd.registration import _gmm_params_reference, gmm_params_backward_reference
    logits, xyz, grads = _sparse_case()
    ref32 = _gmm_params_reference(logits, xyz)
    want, w_lg = _gmm_float64(logits, xyz, grads)
    got = _gmm_forward(logits.to(DEV), xyz.to(DEV))
    for name, g, r, w, tol in zip(("gamma", "pi", "mu", "sigma"), got, ref32, want, GMM_ATOL):
        g = g.cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(r)), name
        keep = ~torch.isnan(r)
        torch.testing.assert_close(g.double()[keep], w[keep], rtol=GMM_RTOL, atol=tol)
    assert got[1][0, 2] == 0 and (got[0][0, :, 2] == 0).all()
    assert torch.equal(got[2][:, 6].cpu(), xyz[:, 17]) and (got[3][:, 6] == 0).all()
    # backward: the closed form's NaN pattern (all of cloud 0, none of cloud 1), float64 autograd where finite
    closed = gmm_params_backward_reference(*ref32[:1], xyz, *ref32[1:], *grads)
    g_lg = _gmm_backward(got[0], xyz.to(DEV), *got[1:], *[g.to(DEV) for g in grads]).cpu()
    assert torch.equal(torch.isnan(g_lg), torch.isnan(closed))
    assert torch.isnan(g_lg[0]).all() and torch.isfinite(g_lg[1]).all()
    _assert_gmm_backward(g_lg[1], w_lg[1])


@pytest.mark.gpu
def test_gmm_params_kernel_matches_reference_fixture():
    """The fixture's logits and cloud: the reference's own gamma, pi, mu, sigma, at the CPU fallback test's tolerance."""
    from mvp_benchmark_amd.registration import gmm_params
    g = _golden()
    got = _gmm_forward(torch.tensor(g["logits"], device=DEV), torch.tensor(g["pts1"], device=DEV))
    wrapped = gmm_params(torch.tensor(g["logits"], device=DEV), torch.tensor(g["pts1"], device=DEV))
    for name, t, w in zip(("gamma", "pi", "mu", "sigma"), got, wrapped):
        np.testing.assert_allclose(t.cpu().numpy(), g[name], rtol=1e-5, atol=1e-7)
        assert torch.equal(t, w)


def _hand_built_rri_case():
    """70 points (one full tile and a tail), k = 4, lists drawn from the other points 1..69, then: point 0 at the
    origin; point 5 repeats a slot; point 6 names itself; points 7 and 69 (in the tail) list the origin point."""
    gen = torch.Generator().manual_seed(9)
    N, k = 70, 4
    xyz = torch.rand(1, N, 3, generator=gen) - 0.5
    xyz[0, 0] = 0.0
    idx = torch.empty(1, N, k, dtype=torch.int32)
    for i in range(N):
        others = torch.tensor([j for j in range(1, N) if j != i])
        idx[0, i] = others[torch.randperm(others.numel(), generator=gen)[:k]].int()
    idx[0, 5, 2] = idx[0, 5, 0]
    idx[0, 6, 1] = 6
    idx[0, 7, 3] = 0
    idx[0, 69, 0] = 0
    return xyz, idx


def _expected_rri_nan_mask(N, k):
    """(1, N, k, 4) [rp, rq, theta, phi]: theta and phi of every slot of the origin point and of exactly the slot
    that lists it; rp and rq are always finite."""
    nan = torch.zeros(1, N, k, 4, dtype=torch.bool)
    nan[0, 0, :, 2:] = True
    nan[0, 7, 3, 2:] = True
    nan[0, 69, 0, 2:] = True
    return nan


def test_rri_reference_nan_mask_for_points_at_the_origin():
    from mvp_benchmark_amd.registration import _rri_reference
    xyz, idx = _hand_built_rri_case()
    N, k = idx.shape[1:]
    feat = _rri_reference(xyz, idx.long())
    assert torch.equal(torch.isnan(feat).view(1, k, 4, N).permute(0, 3, 1, 2), _expected_rri_nan_mask(N, k))
    assert not torch.isinf(feat).any()
    _check_rri(feat, xyz, idx)


@pytest.mark.gpu
def test_rri_kernel_hand_built_lists_and_points_at_the_origin():
    """The NaN mask of the float32 torch reference, exactly: a bad cloud shows as NaN, never as pi or inf."""
    from mvp_benchmark_amd.registration import _rri_reference
    xyz, idx = _hand_built_rri_case()
    feat = _rri(xyz.to(DEV), idx.to(DEV)).cpu()
    assert torch.equal(torch.isnan(feat), torch.isnan(_rri_reference(xyz, idx.long())))
    assert not torch.isinf(feat).any()
    _check_rri(feat, xyz, idx)
    # a repeated slot has the features of the slot it repeats; a slot that names the point itself has theta = 0
    f = feat.view(1, 4, 4, 70)
    assert torch.equal(f[0, 2, :, 5], f[0, 0, :, 5])
    assert f[0, 1, 0, 6] == f[0, 1, 1, 6] and f[0, 1, 2, 6] <= 4e-4      # acos(1 - 2^-24 ...) at most
    # k = 2 with one undefined tangent leaves a single finite psi in the other row: NaN there too
    xyz2 = xyz[:, :8].clone()
    idx2 = torch.tensor([[[1, 2], [2, 3], [3, 4], [0, 4], [5, 6], [6, 7], [7, 1], [1, 2]]], dtype=torch.int32)
    feat2 = _rri(xyz2.to(DEV), idx2.to(DEV)).cpu()
    assert torch.equal(torch.isnan(feat2), torch.isnan(_rri_reference(xyz2, idx2.long())))
    assert torch.isnan(feat2.view(1, 2, 4, 8)[0, :, 3, 3]).all() and not torch.isinf(feat2).any()


# -------------------------------------------------------------------------------------------------- 3. wrappers

def _register_case():
    """Mixtures whose registration matrix has separated singular values (both gaps above 0.05, the rule of
    test_kabsch_rotation_gradient: away from the adjoint's poles; test_gmm_register_separated_singular_values), a known
    rigid motion between them, and a noisy target for the gradients."""
    gen = torch.Generator().manual_seed(2)
    B, J = 8, 8
    pi = torch.softmax(torch.randn(B, J, generator=gen), dim=1)
    mu = torch.randn(B, J, 3, generator=gen) * torch.tensor([1.5, 1.0, 0.5])
    sigma = 0.1 + torch.rand(B, J, generator=gen)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen))[0]
    R = R * torch.linalg.det(R).view(B, 1, 1)
    t = torch.randn(B, 3, generator=gen)
    noise = 0.05 * torch.randn(B, J, 3, generator=gen)
    w = torch.randn(B, 4, 4, generator=gen)
    return pi, mu, sigma, R, t, noise, w


def _register_and_grads(pi, mu_s, mu_t, sigma, w):
    from mvp_benchmark_amd.registration import gmm_register
    leaves = [x.clone().requires_grad_(True) for x in (pi, mu_s, mu_t, sigma)]
    T = gmm_register(*leaves)
    return T.detach(), torch.autograd.grad((T * w).sum(), leaves)


def _register_errors(dtype_dev):
    """-> per-tensor max abs errors of gmm_register run as `dtype_dev` against float64: T of the exact copy, T and the
    four gradients of the noisy pair, each relative to the float64 tensor's largest entry."""
    pi, mu, sigma, R, t, noise, w = _register_case()
    conv = (lambda x: x.double()) if dtype_dev == "float64" else (lambda x: x.to(dtype_dev))
    exact_t = mu @ R.transpose(1, 2) + t.unsqueeze(1)
    out = {}
    runs = {}
    for name, c in (("got", conv), ("want", lambda x: x.double())):
        T0, _ = _register_and_grads(c(pi), c(mu), c(exact_t), c(sigma), c(w))
        T1, grads = _register_and_grads(c(pi), c(mu), c(exact_t + noise), c(sigma), c(w))
        runs[name] = [T0, T1, *grads]
    for name, g, x in zip(("T_exact", "T", "g_pi_s", "g_mu_s", "g_mu_t", "g_sigma_t"), runs["got"], runs["want"]):
        out[name] = ((g.double().cpu() - x).abs().max() / x.abs().max()).item()
    return out, runs["want"][0], R, t


def test_gmm_register_separated_singular_values():
    """The precondition of the GPU test: the registration matrices of _register_case are away from the adjoint's poles."""
    pi, mu, sigma, R, t, noise, w = _register_case()
    pi, mu, sigma, R, t, noise = (x.double() for x in (pi, mu, sigma, R, t, noise))
    mu_t = mu @ R.transpose(1, 2) + t.unsqueeze(1) + noise
    c_s, c_t = pi.unsqueeze(1) @ mu, pi.unsqueeze(1) @ mu_t
    Ms = ((pi.unsqueeze(2) * (mu - c_s)) / sigma.unsqueeze(2)).transpose(1, 2) @ (mu_t - c_t)
    S = torch.linalg.svdvals(Ms)
    assert ((S[:, 0] - S[:, 1] > 0.05) & (S[:, 1] - S[:, 2] > 0.05)).all(), S


@pytest.mark.gpu
def test_gmm_register_on_the_device_recovers_a_motion_and_its_gradients():
    """float32 CUDA (mvp_kabsch_svd3 and its adjoint) against float64 autograd through _kabsch_reference.  Bound per
    tensor: 4 times the error of the float32 CPU path of the same function on the same inputs (another summation
    order, the same formula) plus a floor of 1e-6 relative (16 EPS, for a tensor the CPU path happens to hit within
    an ulp).  Measured for the float32 CPU path, relative to each tensor's largest entry: T_exact 1.6e-7, T 1.3e-7,
    g_pi_s 1.3e-6, g_mu_s 3.3e-7, g_mu_t 5.4e-7, g_sigma_t 4.7e-6 (printed on every run)."""
    cpu, _, _, _ = _register_errors(torch.float32)
    pi, mu, sigma, R, t, noise, w = _register_case()
    dev = lambda x: x.to(DEV)
    exact_t = mu @ R.transpose(1, 2) + t.unsqueeze(1)
    T0, _ = _register_and_grads(dev(pi), dev(mu), dev(exact_t), dev(sigma), dev(w))
    assert T0.is_cuda and T0.dtype == torch.float32
    torch.testing.assert_close(T0[:, :3, :3].cpu(), R, rtol=0, atol=1e-5)
    torch.testing.assert_close(T0[:, :3, 3].cpu(), t, rtol=0, atol=2e-5)
    gpu, _, _, _ = _register_errors(DEV)
    for name in cpu:
        print("gmm_register %-9s float32 CPU %.3g, device %.3g" % (name, cpu[name], gpu[name]))
    for name in cpu:
        assert gpu[name] <= 4 * cpu[name] + 1e-6, (name, gpu[name], cpu[name])


@pytest.mark.gpu
def test_deepgmr_wrappers_take_views_and_a_side_stream():
    """A transposed view as logits, a batch slice as xyz, a non-default stream: bit-equal to the contiguous call on
    the default stream (forward and backward)."""
    from mvp_benchmark_amd.registration import gmm_params, rri_features
    B, J, N = 3, 16, 1000
    logits, xyz, grads = _gmm_inputs(B, J, N, 51)
    grads = [g.to(DEV) for g in grads]
    big = torch.rand(2 * B, N, 3, generator=torch.Generator().manual_seed(52)) - 0.5
    big[0::2] = xyz
    big = big.to(DEV)
    view_xyz = big[0::2]                                         # batch slice, stride 2 N 3
    view_logits = logits.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)     # (B,J,N) view of (B,N,J) storage
    assert not view_xyz.is_contiguous() and not view_logits.is_contiguous()

    def run(lg, pts):
        lg = lg.detach().requires_grad_(True)
        out = gmm_params(lg, pts)
        (g,) = torch.autograd.grad((out[1] * grads[0]).sum() + (out[2] * grads[1]).sum() + (out[3] * grads[2]).sum(), lg)
        return [rri_features(pts, 20)] + [t.detach() for t in out] + [g]

    base = run(logits.to(DEV), xyz.to(DEV))
    torch.cuda.synchronize()
    views = run(view_logits, view_xyz)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = run(view_logits, view_xyz)
    s.synchronize()
    for a, b, c in zip(base, views, side):
        assert torch.equal(a, b) and torch.equal(a, c)


# --------------------------------------------------------------------------------- 4. the model's gradient path

VARIANTS = [{}, {"use_rri": False}, {"use_rri": False, "use_tnet": True}]
VARIANT_IDS = ["rri", "xyz", "xyz-tnet"]


def _pairs(B, N, seed=8):
    gen = torch.Generator().manual_seed(seed)
    pts1 = torch.rand(B, N, 3, generator=gen) - 0.5
    ang = 2 * math.pi * torch.rand(B, generator=gen)
    c, s, z, o = torch.cos(ang), torch.sin(ang), torch.zeros(B), torch.ones(B)
    R = torch.stack([c, -s, z, s, c, z, z, z, o], dim=1).view(B, 3, 3)
    t = 0.5 * (torch.rand(B, 3, generator=gen) - 0.5)
    pts2 = pts1 @ R.transpose(1, 2) + t.unsqueeze(1)
    T_gt = torch.eye(4).repeat(B, 1, 1)
    T_gt[:, :3, :3], T_gt[:, :3, 3] = R, t
    return pts1, pts2, T_gt


class _FollowedReLU(torch.nn.Module):
    """ReLU of the float64 judge.  A network of ReLUs is piecewise linear, and where a pre-activation lies within
    rounding of zero a float32 run may take the other piece: its gradient is then the exact gradient of that piece and
    differs from the float64 model's by a whole element, not by rounding.  One such element in a layer moves the
    relative L2 error of every gradient below it by ~2e-3, whichever float32 implementation it happens to: measured
    at the last ReLU of the `xyz` variant, 1 flip on the CPU (1.3e-3), 2 with the device's library BatchNorm (4.7e-3),
    0 with its native one (4.9e-6).  So the judge differentiates the piece the judged run is on: it takes that run's
    mask.  That the run is on a piece next to the judge's own, and not somewhere else, is a statement about its
    forward pass and is checked as one: the relative L2 error of every ReLU's input is recorded (`forward_errors`)
    and bounded by the callers, together with the largest |float64 input| at which the two masks differ."""

    def __init__(self, judged, forward_errors):
        super().__init__()
        self.judged, self.forward_errors = judged, forward_errors

    def forward(self, x):
        theirs = next(self.judged).to(x.device, x.dtype)
        mine = x.detach()
        differ = (theirs > 0) != (mine > 0)
        self.forward_errors.append((((theirs - mine).norm() / mine.norm()).item(),
                                    mine[differ].abs().max().item() if differ.any() else 0.0))
        return x * (theirs > 0).to(x.dtype)


def _train_step(over, conv, pts, feats=None, follow=None):
    """One train-mode forward + backward of the model run as `conv` (a dtype / device conversion).  feats: the RRI
    features of the two clouds to hand to the model in place of its own (in call order); else the model's own are
    recorded.  follow: the ReLU inputs of the run to be judged (its fourth result), for the float64 judge
    (_FollowedReLU); the fourth result is then [(relative L2 error, largest |input| at a differing mask)] per ReLU.
    -> loss, {name: grad}, [features], [ReLU inputs in call order].  Besides the parameters, the
    gradients that the op layer hands to the backbone and passes inside itself are kept as
    "op.cloud<c>.g_{logits,pi,mu,sigma}": the part of the chain (loss -> gmm_register -> Kabsch adjoint ->
    GmmParams.backward) that runs on this project's kernels."""
    net = conv(_model(**over).train())
    mod = type(net)._mixture.__globals__                 # the model module's namespace (_model loads it privately)
    real, seen = mod["rri_features"], []
    real_gmm, mixtures = mod["gmm_params"], []
    inputs, forward_errors = [], []
    relus = [(parent, name) for parent in net.modules() for name, m in parent.named_children()
             if isinstance(m, torch.nn.ReLU)]
    assert relus
    if follow is not None:
        replay = iter(follow)
        for parent, name in relus:
            setattr(parent, name, _FollowedReLU(replay, forward_errors))
    else:
        for parent, name in relus:
            getattr(parent, name).register_forward_pre_hook(lambda m, i: inputs.append(i[0].detach().cpu()))
    if feats is not None:
        it = iter(feats)
        mod["rri_features"] = lambda p, k: conv(next(it))
    else:
        def recording(p, k):
            seen.append(real(p, k))
            return seen[-1]
        mod["rri_features"] = recording

    def keeping(logits, xyz):
        logits.retain_grad()
        out = real_gmm(logits, xyz)
        for t in out[1:]:
            t.retain_grad()
        mixtures.append((logits,) + tuple(out[1:]))
        return out
    mod["gmm_params"] = keeping
    try:
        loss = net(*[conv(p) for p in pts])[0]
        loss.backward()
    finally:
        mod["rri_features"], mod["gmm_params"] = real, real_gmm
    if follow is not None:
        assert next(replay, None) is None                 # every ReLU of the judged run met its counterpart
    grads = {n: p.grad.detach().double().cpu() for n, p in net.named_parameters()}
    for c, kept in enumerate(mixtures):
        for name, t in zip(("logits", "pi", "mu", "sigma"), kept):
            grads["op.cloud%d.g_%s" % (c, name)] = t.grad.detach().double().cpu()
    return loss.item(), grads, seen, (inputs if follow is None else forward_errors)


def _split(grads):
    """-> parameter gradients, op-layer gradients"""
    return ({n: g for n, g in grads.items() if not n.startswith("op.")},
            {n: g for n, g in grads.items() if n.startswith("op.")})


def _grad_errors(grads, want):
    """Relative L2 error of every parameter gradient whose float64 norm is above 1e-9 of the largest; the rest (true
    gradient zero, seen at norm ~1e-14) are returned as skipped."""
    top = max(g.norm().item() for g in want.values())
    errs, skipped = {}, []
    for name, w in want.items():
        if w.norm().item() <= 1e-9 * top:
            skipped.append(name)
        else:
            errs[name] = ((grads[name] - w).norm() / w.norm()).item()
    return errs, skipped


def _bias_in_front_of_a_batchnorm(net, name):
    """A bias whose true gradient is zero because a train-mode BatchNorm removes every per-channel constant behind it:
    the bias of a convolution / linear layer of a block that normalises right after (Conv1DBNReLU, FCBNReLU; the
    model builds them without one), and the T-net's last encoder bias: where the channel's maximum over the points is
    positive it passes ReLU and the max as a constant, the bias-free linear layer maps it to a constant per output
    channel, and the decoder's first BatchNorm subtracts it (float64 norm 2.5e-14)."""
    if not name.endswith(".bias"):
        return False
    if name == "backbone.tnet.encoder.2.bn.bias":
        return True
    parent = net.get_submodule(name.rsplit(".", 2)[0])
    return name.rsplit(".", 2)[1] in ("conv", "linear") and hasattr(parent, "bn")


def _assert_only_dead_biases_skipped(over, skipped, grads, want):
    """The norm rule may skip biases in front of a BatchNorm only, and what was computed for them is as good as zero."""
    net = _model(**over)
    assert all(_bias_in_front_of_a_batchnorm(net, n) for n in skipped), skipped
    top = max(g.norm().item() for g in want.values())
    for n in skipped:
        assert grads[n].norm().item() <= 1e-4 * top, (n, grads[n].norm().item(), top)


# float32 CPU model against the float64 model on the same features, B = 4, N = 512, measured: loss relative 2e-6 / 7e-8 /
# 1e-5 for the three variants; the bound is 10 times that (the loss is one number, its error is not an average).
# Worst parameter-gradient relative L2: 2.0e-3 / 1.9e-3 / 5.3e-3 against the plain float64 model, all of it ReLU
# flips; 9.7e-6 / 9.3e-6 / 1.35e-4 against the judge that follows the run at the kinks (_FollowedReLU), which is what
# is asserted.  That is the error of the op layer's gradients handed down, so it gets their bound (next lines).
CPU_LOSS_RTOL = {"rri": 2e-5, "xyz": 2e-5, "xyz-tnet": 1e-4}
# gradients with respect to the logits, pi, mu, sigma of both clouds (what the op layer hands on): measured 1.5e-5 /
# 5.5e-6 / 1.3e-4 at worst, and 1.3e-4 / 6.4e-6 / 3.0e-4 on a second host whose BLAS blocks differently (it moves with
# the conditioning of the Kabsch adjoint, not with the variant's formulas): one bound, 4 times the largest
CPU_OP_GRAD_RTOL = 1.2e-3
# largest |float64 ReLU input| at which the float32 run's mask differs from the float64 model's own (how far from a kink
# a run may be and still land on the other side): measured 3.1e-6 / 1.4e-6 / 8.8e-5, and 1.8e-4 for `xyz-tnet` on a second
# host (the T-net normalises over a batch of 4, which amplifies rounding a hundredfold); bound 4 times the largest
CPU_KINK = 1e-3


@pytest.mark.parametrize("over", VARIANTS, ids=VARIANT_IDS)
def test_deepgmr_float32_gradients_match_float64_model_cpu(over, request):
    vid = request.node.callspec.id
    pts = _pairs(4, 512)
    loss32, g32, feats, masks = _train_step(over, lambda x: x.float(), pts)
    assert len(feats) == (0 if over.get("use_rri") is False else 2)
    loss64, g64, _, fwd = _train_step(over, lambda x: x.double(), pts, feats or None, follow=masks)
    print("%s: ReLU inputs, worst relative L2 error %.3g, masks differ up to |x| = %.3g"
          % (vid, max(e for e, _ in fwd), max(k for _, k in fwd)))
    assert max(k for _, k in fwd) <= CPU_KINK
    (p32, o32), (p64, o64) = _split(g32), _split(g64)
    errs, skipped = _grad_errors(p32, p64)
    op_errs, _ = _grad_errors(o32, o64)
    print("%s: loss relative %.3g, worst gradient relative L2 %.3g (%s), op layer %.3g (%s), skipped %s"
          % (vid, abs(loss32 - loss64) / abs(loss64), max(errs.values()), max(errs, key=errs.get),
             max(op_errs.values()), max(op_errs, key=op_errs.get), skipped))
    assert abs(loss32 - loss64) <= CPU_LOSS_RTOL[vid] * abs(loss64)
    assert max(errs.values()) <= CPU_OP_GRAD_RTOL, max(errs, key=errs.get)
    assert len(op_errs) == 8 and max(op_errs.values()) <= CPU_OP_GRAD_RTOL, op_errs
    _assert_only_dead_biases_skipped(over, skipped, p32, p64)
    assert all(torch.isfinite(g).all() for g in g32.values())


_DEVICE_RUNS = {}


def _device_runs(vid):
    """The device model, the float64 CPU model and the float32 CPU model on the same pairs and, with RRI, on the
    device model's own features; once per variant for the two tests below."""
    if vid not in _DEVICE_RUNS:
        over = VARIANTS[VARIANT_IDS.index(vid)]
        pts = _pairs(4, 512)
        loss_d, g_d, feats, masks_d = _train_step(over, lambda x: x.to(DEV), pts)     # masks_*: the ReLU inputs
        feats = [f.cpu() for f in feats] or None
        loss32, g32, _, masks32 = _train_step(over, lambda x: x.float(), pts, feats)
        # the float64 judge once per judged run: each follows its own run at the ReLU kinks (_FollowedReLU)
        judge_d = _train_step(over, lambda x: x.double(), pts, feats, follow=[m.cpu() for m in masks_d])
        judge32 = _train_step(over, lambda x: x.double(), pts, feats, follow=masks32)
        _DEVICE_RUNS[vid] = ((loss_d, g_d), judge_d[:2], (loss32, g32), judge32[:2],
                             (max(k for _, k in judge_d[3]), max(k for _, k in judge32[3])))
    return _DEVICE_RUNS[vid]


@pytest.mark.gpu
@pytest.mark.parametrize("over", VARIANTS, ids=VARIANT_IDS)
def test_deepgmr_op_layer_gradients_match_float64_model_gpu(over, request):
    """Loss -> gmm_register -> Kabsch adjoint (mvp_kabsch_svd3's) -> GmmParams.backward (mvp_gmm_params_backward) on
    the device, inside the model's training step, against the float64 CPU model: the loss, and the gradients with
    respect to pi, mu, sigma and the logits of both clouds, which is everything the backbone receives.  Bound per
    tensor: 4 times the relative L2 error of the float32 CPU model in the same test (another summation order, the
    same formulas), with a floor of 1e-5: the float32 CPU errors are 3e-6 to 3e-4 (the Kabsch adjoint's conditioning
    times EPS) and the floor keeps a tensor the CPU happens to hit well from setting a bound below that range."""
    vid = request.node.callspec.id
    (loss_d, g_d), (loss64, g64), (loss32, g32), (loss64_32, g64_32), _ = _device_runs(vid)
    e_d, _ = _grad_errors(_split(g_d)[1], _split(g64)[1])
    e_32, _ = _grad_errors(_split(g32)[1], _split(g64_32)[1])
    assert len(e_d) == 8
    for name in e_d:
        print("%s %-22s device %.3g / float32 CPU %.3g" % (vid, name, e_d[name], e_32[name]))
    assert abs(loss_d - loss64) <= max(4 * abs(loss32 - loss64_32), 1e-4 * abs(loss64))
    for name in e_d:
        assert e_d[name] <= max(4 * e_32[name], 1e-5), (name, e_d[name], e_32[name])


@pytest.mark.gpu
@pytest.mark.parametrize("over", VARIANTS, ids=VARIANT_IDS)
def test_deepgmr_gradients_match_float64_model_gpu(over, request):
    """The whole chain down to the parameters: each parameter gradient's relative L2 error against the float64 CPU
    model (handed the device model's own RRI features) may be 4 times that of the float32 CPU model, run here on the
    same features and judged the same way, with a floor of 1e-4.  The float64 judge follows the judged run at the
    ReLU kinks (_FollowedReLU): without that, both errors are the count of activations that rounding put on the other
    side of zero, 0 to 2 per layer at ~2e-3 each, and the comparison is a coin toss (first measured so on an MI355X:
    `xyz` at 2.2e-3 to 3.7e-3 on the device against 3.4e-4 to 1.9e-3 on the CPU, with the op layer's g_logits at
    7.3e-6 against 4.1e-6).  With it the float32 CPU model is at 1e-5 (`rri`, `xyz`) and 1.4e-4 (`xyz-tnet`), so the
    device is held to 1e-4 to 1e-3, several times closer than before."""
    vid = request.node.callspec.id
    (loss_d, g_d), (loss64, g64), (loss32, g32), (_, g64_32), (kink_d, kink32) = _device_runs(vid)
    (p_d, _), (p64, _), (p32, _), (p64_32, _) = _split(g_d), _split(g64), _split(g32), _split(g64_32)
    e_d, skipped = _grad_errors(p_d, p64)
    e_32, _ = _grad_errors(p32, p64_32)
    assert set(e_d) == set(e_32)
    worst = max(e_d, key=lambda n: e_d[n] / max(4 * e_32[n], 1e-4))
    print("%s: loss relative device %.3g / float32 CPU %.3g; worst gradient %s device %.3g / float32 CPU %.3g; skipped %s"
          % (vid, abs(loss_d - loss64) / abs(loss64), abs(loss32 - loss64) / abs(loss64), worst, e_d[worst],
             e_32[worst], skipped))
    print("%s: masks differ from the float64 model's up to |x| = %.3g on the device, %.3g on the CPU" % (vid, kink_d, kink32))
    _assert_only_dead_biases_skipped(over, skipped, p_d, p64)
    assert all(torch.isfinite(g).all() for g in g_d.values())
    # the device run lies on a piece next to the float64 model's own: same rule as for the gradients
    assert kink_d <= max(4 * kink32, 1e-4), (kink_d, kink32)
    for name in e_d:
        assert e_d[name] <= max(4 * e_32[name], 1e-4), (name, e_d[name], e_32[name])


def _eval_outputs(net, conv):
    g = _golden()
    pts1, pts2, T_gt = (conv(torch.tensor(g[k])) for k in ("pts1", "pts2", "T_gt"))
    with torch.no_grad():
        return net(pts1, pts2, prefix="test").cpu().numpy(), [t.cpu().numpy() for t in net(pts1, pts2, T_gt, prefix="val")]


@pytest.mark.parametrize("key,over", [("norri_", VARIANTS[1]), ("norri_tnet_", VARIANTS[2])], ids=VARIANT_IDS[1:])
def test_deepgmr_variants_without_rri_match_reference_fixture_cpu(key, over):
    """Tolerances of test_deepgmr_fallback_matches_reference_fixture."""
    g = _golden()
    T_12, out = _eval_outputs(_model(**over), lambda x: x)
    np.testing.assert_allclose(T_12, g[key + "T_12"], rtol=0, atol=2e-4)
    for name, t, tol in zip(("loss", "r_err", "t_err", "rmse", "mse"), out, (1e-4, 2e-2, 1e-5, 1e-4, 1e-4)):
        np.testing.assert_allclose(t, g[key + name], rtol=0, atol=tol)


@pytest.mark.gpu
@pytest.mark.parametrize("key,over", [("norri_", VARIANTS[1]), ("norri_tnet_", VARIANTS[2])], ids=VARIANT_IDS[1:])
def test_deepgmr_variants_without_rri_match_reference_fixture_gpu(key, over):
    """Tolerances of test_deepgmr_forward_matches_reference_fixture."""
    g = _golden()
    T_12, out = _eval_outputs(_model(**over).to(DEV), lambda x: x.to(DEV))
    np.testing.assert_allclose(T_12, g[key + "T_12"], rtol=0, atol=1e-3)
    for name, t, tol in zip(("loss", "r_err", "t_err", "rmse", "mse"), out, (1e-3, 0.1, 1e-4, 1e-3, 1e-3)):
        np.testing.assert_allclose(t, g[key + name], rtol=0, atol=tol)
