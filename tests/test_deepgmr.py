"""SURVEY 8(f) row N3, second model: DeepGMR (registration/models/deepgmr.py) -- RRI features and GMM moments as
HIP kernels (mvp_rri_features, mvp_gmm_params, mvp_gmm_params_backward), registration through mvp_kabsch_svd3.

CPU tests: parameter layout and cfg against the fixture generated from the imported reference
(tests/golden/make_deepgmr_golden.py), the torch fallback formulations against the fixture, the closed-form GMM
backward against autograd (gradcheck, float64).  GPU tests: the kernels against float64 recomputations and the
fixture, determinism, argument errors, the model against the fixture and a training step at the cfg shape."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

REG = os.path.join(ROOT, "registration")
GOLD = os.path.join(ROOT, "tests", "golden")
if GOLD not in sys.path:
    sys.path.insert(0, GOLD)

DEV = "cuda:0"
CFG = dict(use_rri=True, rri_size=20, num_groups=16, use_tnet=False)


def _golden():
    return np.load(os.path.join(GOLD, "deepgmr_golden.npz"))


def _model(**over):
    spec = importlib.util.spec_from_file_location("registration_deepgmr", os.path.join(REG, "models", "deepgmr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from make_dcp_golden import fill_parameters
    net = mod.Model(types.SimpleNamespace(**dict(CFG, **over)))
    fill_parameters(net)
    return net.eval()


# ------------------------------------------------------------------------------------------------------------ CPU

def test_deepgmr_state_dict_layout_and_cfg_match_reference():
    """Names and shapes of every parameter / buffer equal the reference model's, with and without the T-net:
    checkpoints interchange.  The cfg carries the reference's key set and values."""
    g = _golden()
    for prefix, over in (("", {}), ("tnet_", {"use_tnet": True})):
        mine = {k: str(list(v.shape)) for k, v in _model(**over).state_dict().items()}
        assert mine == dict(zip(g[prefix + "names"].tolist(), g[prefix + "shapes"].tolist()))
    assert sum(p.numel() for p in _model().parameters()) == 1527440
    import yaml
    cfg = yaml.safe_load(open(os.path.join(REG, "cfgs", "deepgmr.yaml")))
    assert cfg == {
        'batch_size': 32, 'workers': 0, 'nepoch': 100, 'model_name': 'deepgmr', 'load_model': None, 'start_epoch': 0,
        'work_dir': 'log/', 'flag': 'debug', 'manual_seed': None, 'step_interval_to_print': 30,
        'step_interval_to_plot': 250, 'epoch_interval_to_save': 10, 'epoch_interval_to_val': 1, 'lr': 0.001,
        'lr_decay': True, 'lr_decay_rate': 0.5, 'lr_clip': 1e-6, 'optimizer': 'Adam', 'weight_decay': 0,
        'betas': '0.9, 0.999', 'use_rri': True, 'rri_size': 20, 'num_groups': 16, 'num_points': 2048,
        'use_tnet': False, 'use_fpfh': False, 'use_ppf': False, 'descriptor_size': 1024, 'max_angle': 180,
        'max_trans': 0.5, 'category': None, 'benchmark': 'mvp', 'num_rot_levels': 2, 'num_corr_levels': 2}


def test_deepgmr_fallback_matches_reference_fixture():
    """The CPU formulations (topk kNN + torch RRI, softmax + moments, torch SVD registration) reproduce the
    reference's features, moments and eval-mode outputs."""
    from mvp_benchmark_amd.registration import gmm_params, rri_features
    g = _golden()
    pts1, pts2, T_gt = (torch.tensor(g[k]) for k in ("pts1", "pts2", "T_gt"))
    for k in (20, 5):
        np.testing.assert_allclose(rri_features(pts1, k).numpy(), g["rri_k%d" % k], rtol=0, atol=1e-5)
    gamma, pi, mu, sigma = gmm_params(torch.tensor(g["logits"]), pts1)
    for name, t in (("gamma", gamma), ("pi", pi), ("mu", mu), ("sigma", sigma)):
        np.testing.assert_allclose(t.numpy(), g[name], rtol=1e-5, atol=1e-7)
    net = _model()
    with torch.no_grad():
        np.testing.assert_allclose(net(pts1, pts2, prefix="test").numpy(), g["T_12"], rtol=0, atol=2e-4)
        out = net(pts1, pts2, T_gt, prefix="val")
    assert net.sigma1.shape == (2, 16, 3, 3) and net.gamma1.shape == (2, 256, 16)
    for name, t, tol in zip(("loss", "r_err", "t_err", "rmse", "mse"), out, (1e-4, 2e-2, 1e-5, 1e-4, 1e-4)):
        np.testing.assert_allclose(t.numpy(), g[name], rtol=0, atol=tol)


def test_gmm_backward_closed_form_matches_autograd():
    """The closed form of mvp_gmm_params_backward (in torch) against autograd of the reference formulation, and
    GmmParams as a whole (its CPU path runs that closed form) under gradcheck, float64."""
    from mvp_benchmark_amd.registration import (GmmParams, _gmm_params_reference,
                                                gmm_params_backward_reference)
    gen = torch.Generator().manual_seed(5)
    B, J, N = 2, 5, 11
    logits = torch.randn(B, J, N, generator=gen, dtype=torch.float64, requires_grad=True)
    xyz = torch.rand(B, N, 3, generator=gen, dtype=torch.float64)
    g_pi, g_mu, g_sigma = (torch.randn(*s, generator=gen, dtype=torch.float64) for s in ((B, J), (B, J, 3), (B, J)))
    gamma, pi, mu, sigma = _gmm_params_reference(logits, xyz)
    want, = torch.autograd.grad((pi * g_pi).sum() + (mu * g_mu).sum() + (sigma * g_sigma).sum(), logits)
    got = gmm_params_backward_reference(gamma.detach(), xyz, pi.detach(), mu.detach(), sigma.detach(),
                                        g_pi, g_mu, g_sigma)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-12)
    assert torch.autograd.gradcheck(lambda lg: GmmParams.apply(lg, xyz)[1:], (logits,))


def test_rri_and_register_fallback_edge_cases():
    """k < 2 has no second-smallest psi (the reference's argpartition fails): an exception.  gmm_register of a
    mixture onto its own rigidly moved copy recovers the motion."""
    from mvp_benchmark_amd.registration import gmm_register, rri_features
    with pytest.raises(ValueError):
        rri_features(torch.rand(2, 16, 3), 1)
    gen = torch.Generator().manual_seed(2)
    pi = torch.softmax(torch.randn(3, 8, generator=gen, dtype=torch.float64), dim=1)
    mu = torch.randn(3, 8, 3, generator=gen, dtype=torch.float64)
    sigma = 0.1 + torch.rand(3, 8, generator=gen, dtype=torch.float64)
    R = torch.linalg.qr(torch.randn(3, 3, 3, generator=gen, dtype=torch.float64))[0]
    R = R * torch.linalg.det(R).view(3, 1, 1)                       # proper rotations
    t = torch.randn(3, 3, generator=gen, dtype=torch.float64)
    T = gmm_register(pi, mu, mu @ R.transpose(1, 2) + t.unsqueeze(1), sigma)
    torch.testing.assert_close(T[:, :3, :3], R)
    torch.testing.assert_close(T[:, :3, 3], t)


# ------------------------------------------------------------------------------------------------------------ GPU

def _knn_idx(xyz, k):
    from mvp_benchmark_amd.mm3d_pn2 import knn
    return knn(k + 1, xyz)[:, 1:, :].transpose(1, 2).contiguous()


def _rri_kernel(xyz, idx):
    from mvp_benchmark_amd._lib import call
    B, N, k = idx.shape
    feat = torch.empty(B, 4 * k, N, device=xyz.device)
    call("mvp_rri_features", xyz.device, B, N, k, xyz, idx, feat)
    return feat


def _check_rri(feat, xyz, idx):
    """feat (B,4k,N) from the kernel against a float64 recomputation on the same neighbours.  theta is compared as
    cos(theta) where |d| > 0.99 (acos is ill-conditioned there).  phi may differ from the float64 selection only
    where that is a tie: some psi of the row within rounding of 0 / 2 pi (it wraps), or the selected psi itself
    within rounding (nearly parallel tangents).  Returns the number of such ties, each verified.  Entries whose float64
    expectation is not finite (a point or a neighbour at the origin) are left out here; the caller pins their NaN
    pattern.  With finite expectations nothing is left out."""
    x = xyz.double().cpu()
    ix = idx.long().cpu()
    B, N, k = ix.shape
    f = feat.double().cpu().view(B, k, 4, N).permute(0, 3, 1, 2)          # (B,N,k,4)
    p = x.unsqueeze(2).expand(B, N, k, 3)
    q = torch.stack([x[b][ix[b]] for b in range(B)])
    rp, rq = p.norm(dim=-1), q.norm(dim=-1)
    pn = p / rp.unsqueeze(-1)
    d = (pn * q).sum(-1) / rq
    torch.testing.assert_close(f[..., 0], rp, rtol=1e-6, atol=0)
    torch.testing.assert_close(f[..., 1], rq, rtol=1e-6, atol=0)
    steep = d.abs() > 0.99
    flat = torch.isfinite(d) & ~steep
    if flat.any():
        assert (f[..., 2] - torch.acos(d.clamp(-1, 1)))[flat].abs().max() < 2e-5
    if steep.any():
        assert (torch.cos(f[..., 2]) - d.clamp(-1, 1))[steep].abs().max() < 2e-6
    T = q - d.unsqueeze(-1) * p                                            # (B,N,k,3)
    Tb, Ta = T.unsqueeze(2), T.unsqueeze(3)                                # [.., a, b]
    sin = (torch.linalg.cross(Tb.expand(-1, -1, k, -1, -1), Ta.expand(-1, -1, -1, k, -1), dim=-1)
           * pn[:, :, :1].unsqueeze(2)).sum(-1)
    cos = (Tb * Ta).sum(-1)
    psi = torch.remainder(torch.atan2(sin, cos), 2 * math.pi)
    eye = torch.eye(k, dtype=torch.bool)
    psi[:, :, eye] = 0.0
    phi64 = psi.sort(dim=-1).values[..., 1]                                # NaN sorts last
    known = torch.isfinite(phi64)
    # rounding of one psi in float32: the tangents carry an absolute error ~ eps (|p| + |q|), so the angle one of
    # ~ eps (|p| + |q_a|) / |T_a| + eps (|p| + |q_b|) / |T_b| (generously scaled)
    tn = T.norm(dim=-1)
    cond = torch.nan_to_num((rp + rq) / tn, nan=0.0)                       # an undefined tangent takes no part
    delta = 256 * 2.0 ** -24 * (cond.unsqueeze(-1) + cond.unsqueeze(-2)) + 1e-6
    wrap = (torch.minimum(psi, 2 * math.pi - psi) <= delta) & ~eye
    assert torch.isfinite(f[..., 3][known]).all()
    err = (f[..., 3] - phi64).abs()
    bad = (err > 1e-4) & known
    tie = wrap.any(-1) | (err <= delta.max(-1).values)
    assert not (bad & ~tie).any(), "phi differs without a tie at %s" % (bad & ~tie).nonzero()[:5].tolist()
    assert (err[~bad & known] <= 1e-4).all()
    return int(bad.sum())


@pytest.mark.gpu
def test_rri_kernel_matches_float64_and_counts_ties():
    gen = torch.Generator().manual_seed(17)
    xyz = (torch.rand(3, 1000, 3, generator=gen) - 0.5).to(DEV)
    ties = {}
    for k in (2, 5, 20, 64):
        idx = _knn_idx(xyz, k)
        ties[k] = _check_rri(_rri_kernel(xyz, idx), xyz, idx)
        assert ties[k] <= 3 * 1000 * k // 1000, ties          # rare: a few per thousand slots at most
    print("phi ties vs float64:", ties)


@pytest.mark.gpu
def test_rri_features_match_reference_fixture():
    """rri_features (knn operator + kernel) on the fixture's clouds against the reference's own features."""
    from mvp_benchmark_amd.registration import rri_features
    g = _golden()
    xyz = torch.tensor(g["pts1"], device=DEV)
    for k in (20, 5):
        feat = rri_features(xyz, k)
        assert feat.shape == (2, 4 * k, 256) and not feat.requires_grad
        ref = torch.tensor(g["rri_k%d" % k])
        idx = _knn_idx(xyz, k)
        _check_rri(feat, xyz, idx)                      # kernel vs float64 on the same neighbours
        # ... and the reference's float32 features: rp, rq exact up to rounding, phi except at verified ties
        f, r = feat.cpu().view(2, k, 4, 256), ref.view(2, k, 4, 256)
        torch.testing.assert_close(f[:, :, :2], r[:, :, :2], rtol=1e-6, atol=0)
        torch.testing.assert_close(torch.cos(f[:, :, 2]), torch.cos(r[:, :, 2]), rtol=0, atol=2e-6)
        assert ((f[:, :, 3] - r[:, :, 3]).abs() > 1e-4).sum() <= 2


@pytest.mark.gpu
def test_rri_duplicate_points_give_identical_features():
    """Self and a duplicate are interchangeable: whichever the kNN lists first is dropped, the features agree."""
    from mvp_benchmark_amd.registration import rri_features
    gen = torch.Generator().manual_seed(4)
    xyz = torch.rand(2, 300, 3, generator=gen) - 0.5
    xyz[:, 9] = xyz[:, 5]
    xyz[1, 200] = xyz[1, 17]
    feat = rri_features(xyz.to(DEV), 20).cpu()
    assert torch.equal(feat[:, :, 5], feat[:, :, 9])
    assert torch.equal(feat[1, :, 17], feat[1, :, 200])
    assert torch.isfinite(feat).all()


def _gmm_inputs(B, J, N, seed):
    gen = torch.Generator().manual_seed(seed)
    logits = 3.0 * torch.randn(B, J, N, generator=gen)
    xyz = torch.rand(B, N, 3, generator=gen) - 0.5
    grads = tuple(torch.randn(*s, generator=gen) for s in ((B, J), (B, J, 3), (B, J)))
    return logits, xyz, grads


@pytest.mark.gpu
@pytest.mark.parametrize("J", [1, 16, 33, 64])
def test_gmm_params_forward_backward_match_float64(J):
    from mvp_benchmark_amd.registration import _gmm_params_reference, gmm_params
    B, N = 3, 1000
    logits, xyz, (g_pi, g_mu, g_sigma) = _gmm_inputs(B, J, N, J)
    lg = logits.to(DEV).requires_grad_(True)
    gamma, pi, mu, sigma = gmm_params(lg, xyz.to(DEV))
    (g_lg,) = torch.autograd.grad((pi * g_pi.to(DEV)).sum() + (mu * g_mu.to(DEV)).sum()
                                  + (sigma * g_sigma.to(DEV)).sum(), lg)
    l64 = logits.double().requires_grad_(True)
    want = _gmm_params_reference(l64, xyz.double())
    (w_lg,) = torch.autograd.grad((want[1] * g_pi.double()).sum() + (want[2] * g_mu.double()).sum()
                                  + (want[3] * g_sigma.double()).sum(), l64)
    for got, ref, tol in zip((gamma, pi, mu, sigma), want, (2e-7, 1e-6, 1e-5, 1e-5)):
        torch.testing.assert_close(got.double().cpu(), ref.detach(), rtol=1e-4, atol=tol)
    scale = w_lg.abs().max()
    assert (g_lg.double().cpu() - w_lg).abs().max() <= 1e-4 * scale


@pytest.mark.gpu
def test_deepgmr_kernels_are_deterministic():
    from mvp_benchmark_amd.registration import gmm_params, rri_features
    logits, xyz, (g_pi, g_mu, g_sigma) = _gmm_inputs(4, 16, 2048, 1)
    xyz = xyz.to(DEV)
    assert torch.equal(rri_features(xyz, 20), rri_features(xyz, 20))
    runs = []
    for _ in range(2):
        lg = logits.to(DEV).requires_grad_(True)
        out = gmm_params(lg, xyz)
        (g,) = torch.autograd.grad((out[1] * g_pi.to(DEV)).sum() + (out[2] * g_mu.to(DEV)).sum()
                                   + (out[3] * g_sigma.to(DEV)).sum(), lg)
        runs.append([t.detach() for t in out] + [g])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_deepgmr_kernels_reject_bad_sizes():
    from mvp_benchmark_amd._lib import MvpOpsError, call
    from mvp_benchmark_amd.registration import gmm_params, rri_features
    xyz = torch.rand(2, 128, 3, device=DEV)
    for k in (1, 65):
        with pytest.raises(MvpOpsError):
            rri_features(xyz, k)
    with pytest.raises(MvpOpsError):
        gmm_params(torch.randn(2, 65, 128, device=DEV), xyz)
    buf = torch.zeros(2 * 128 * 4, device=DEV)
    with pytest.raises(MvpOpsError):
        call("mvp_gmm_params", DEV, 2, 128, 0, buf, xyz, buf, buf, buf, buf)
    with pytest.raises(MvpOpsError):
        call("mvp_gmm_params_backward", DEV, 2, 128, 65, buf, xyz, buf, buf, buf, buf, buf, buf, buf)


@pytest.mark.gpu
def test_deepgmr_forward_matches_reference_fixture():
    g = _golden()
    pts1, pts2, T_gt = (torch.tensor(g[k], device=DEV) for k in ("pts1", "pts2", "T_gt"))
    net = _model().to(DEV)
    with torch.no_grad():
        T_12 = net(pts1, pts2, prefix="test")
        out = net(pts1, pts2, T_gt, prefix="val")
    np.testing.assert_allclose(T_12.cpu().numpy(), g["T_12"], rtol=0, atol=1e-3)
    for name, t, tol in zip(("loss", "r_err", "t_err", "rmse", "mse"), out, (1e-3, 0.1, 1e-4, 1e-3, 1e-3)):
        np.testing.assert_allclose(t.cpu().numpy(), g[name], rtol=0, atol=tol)


@pytest.mark.gpu
def test_deepgmr_training_step_at_cfg_shape():
    """B = 32 pairs of 2048 points, k = 20, 16 components, train mode: the loss agrees with the float64 CPU model on
    the same inputs and parameters, and every parameter gradient is finite."""
    gen = torch.Generator().manual_seed(8)
    B, N = 32, 2048
    pts1 = torch.rand(B, N, 3, generator=gen) - 0.5
    ang = 2 * math.pi * torch.rand(B, generator=gen)
    c, s, z, o = torch.cos(ang), torch.sin(ang), torch.zeros(B), torch.ones(B)
    R = torch.stack([c, -s, z, s, c, z, z, z, o], dim=1).view(B, 3, 3)
    t = 0.5 * (torch.rand(B, 3, generator=gen) - 0.5)
    pts2 = pts1 @ R.transpose(1, 2) + t.unsqueeze(1)
    T_gt = torch.eye(4).repeat(B, 1, 1)
    T_gt[:, :3, :3], T_gt[:, :3, 3] = R, t
    net = _model().train()
    ref = _model().train().double()
    with torch.no_grad():
        loss64 = ref(pts1.double(), pts2.double(), T_gt.double())[0].item()
    net = net.to(DEV)
    loss = net(pts1.to(DEV), pts2.to(DEV), T_gt.to(DEV))[0]
    loss.backward()
    assert math.isfinite(loss.item())
    assert abs(loss.item() - loss64) <= 2e-3 * abs(loss64), (loss.item(), loss64)
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert net.backbone.decoder[3].weight.grad.abs().sum() > 0
