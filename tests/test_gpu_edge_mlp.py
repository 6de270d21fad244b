"""The fused edge MLP (csrc/edge_mlp.hip, registration.edge_mlp_max, DGCNN's opt-in inference route) against an independent
float64 reference: plain torch on the CPU with an explicit gather, nothing of the op layer (tests/edge_mlp_cases.py, where
the bound is derived).  Every case runs through the C ABI on a NaN-filled output (an element no lane writes stays NaN) and
through the wrapper.

Two kinds of input, two kinds of assertion, no tuned tolerance:

  exact    small integers stored as float32 (x and shift in [-2, 2], scale in {-1, 1, 2}, weights in {-1, 0, 1} with three
           non-zeros a row).  The test asserts on the float64 run that `mag` stays below 2^24: then every intermediate is
           an integer float32 holds, no order of additions and no FMA can change a bit, and out must EQUAL the reference.
           Ties over k and negative scales are frequent in these inputs.
  random   randn inputs, weights scaled by 1 / sqrt(K): |got - ref| <= t * 2^-24 * mag elementwise.

Indices always lie in [0, N)."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch
from conftest import ROOT

import edge_mlp_cases as cases
from dcp_util import abi_call_names, load_dcp

DEV = "cuda:0"
gpu = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def run_abi(case):
    """mvp_edge_mlp_max on a NaN-filled output -> CPU tensor."""
    from mvp_benchmark_amd import _lib
    x, idx = case["x"].to(DEV), case["idx"].to(DEV)
    B, c, N = x.shape
    k = idx.shape[1]
    widths = [W.shape[0] for W in case["weights"]]
    w = torch.cat([W.reshape(-1) for W in case["weights"]]).to(DEV)
    scale, shift = torch.cat(case["scales"]).to(DEV), torch.cat(case["shifts"]).to(DEV)
    out = torch.full((B, sum(widths), N), float("nan"), device=DEV)
    _lib.call("mvp_edge_mlp_max", DEV, B, c, N, k, len(widths), *(widths + [0] * (4 - len(widths))), x, idx, w, scale,
              shift, out)
    torch.cuda.synchronize()
    return out.cpu()


def run_wrapper(case):
    from mvp_benchmark_amd.registration import edge_mlp_max
    on_dev = lambda ts: [t.to(DEV) for t in ts]
    with torch.no_grad():
        out = edge_mlp_max(case["x"].to(DEV), case["idx"].to(DEV), on_dev(case["weights"]), on_dev(case["scales"]),
                           on_dev(case["shifts"]))
    return out.cpu()


@gpu
@pytest.mark.parametrize("pattern", cases.PATTERNS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_exact(shape, pattern):
    case = cases.make_case(shape, pattern, "exact")
    ref = cases.reference(**case)
    assert float(ref["mag"].max()) < 2.0 ** 24
    want = ref["out"].float()
    for name, got in (("abi", run_abi(case)), ("wrapper", run_wrapper(case))):
        bad = (got != want) | torch.isnan(got)
        assert not bool(bad.any()), "%s: %d of %d differ, first at %s" % (
            name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())


@gpu
@pytest.mark.parametrize("pattern", cases.PATTERNS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_random_within_the_rounding_bound(shape, pattern):
    case = cases.make_case(shape, pattern, "random")
    ref = cases.reference(**case)
    for name, got in (("abi", run_abi(case)), ("wrapper", run_wrapper(case))):
        assert not bool(torch.isnan(got).any()), name
        share = cases.bound_share(got, ref)
        print("%s %s %s: %.3f of the bound" % (name, shape, pattern, share))
        assert share <= 1.0, name


@gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_coordinate(value):
    """One non-finite coordinate in one point: where the output is NaN is what the float32 PyTorch composition on the GPU
    yields (ReLU keeps a NaN, the maximum is NaN if a member is), the finite entries stay within the bound and an
    infinite entry of the reference is the same infinity."""
    case = cases.make_case(cases.SHAPES[1], "random", "random")
    case["x"][1, 2, 17] = value
    ref = cases.reference(**case)
    on_dev = lambda ts: [t.to(DEV) for t in ts]
    torch_nan = torch.isnan(cases.compose(case["x"].to(DEV), case["idx"].to(DEV), on_dev(case["weights"]),
                                          on_dev(case["scales"]), on_dev(case["shifts"]))).cpu()
    assert bool(torch_nan.any()) or value == float("inf")
    for name, got in (("abi", run_abi(case)), ("wrapper", run_wrapper(case))):
        assert torch.equal(torch.isnan(got), torch_nan), name
        assert torch.equal(torch.isnan(got), torch.isnan(ref["out"])), name
        inf = torch.isinf(ref["out"])
        assert torch.equal(got[inf].double(), ref["out"][inf]), name
        fin = torch.isfinite(ref["out"]) & torch.isfinite(ref["mag"])
        err = (got.double() - ref["out"]).abs()
        assert bool((err[fin] <= (ref["t"] * cases.U * ref["mag"])[fin]).all()), name
        assert bool(torch.isfinite(got[torch.isfinite(ref["out"])]).all()), name
    assert bool(torch.isfinite(ref["out"][0]).all())             # the other cloud is untouched


@gpu
def test_two_runs_give_the_same_bits():
    case = cases.make_case(cases.SHAPES[1], "random", "random")
    first = run_abi(case)
    for _ in range(2):
        assert torch.equal(run_abi(case), first)
    assert torch.equal(run_wrapper(case), first)


# ---------------------------------------------------------------------------------------------- the module and the model

def _randomised_dgcnn(dcp):
    """A DGCNN whose BatchNorm layers carry random running statistics and affine parameters, some weights negative."""
    torch.manual_seed(11)
    net = dcp.DGCNN()
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for i in range(1, 6):
            bn = getattr(net, "bn%d" % i)
            bn.weight.copy_(torch.randn(bn.num_features, generator=gen))
            bn.bias.copy_(torch.randn(bn.num_features, generator=gen) * 0.5)
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=gen) * 0.5)
            bn.running_var.copy_(torch.rand(bn.num_features, generator=gen) + 0.5)
        assert int((net.bn1.weight < 0).sum()) > 0
    return net.eval()


def _module_reference(net64, x, graph):
    """DGCNN in eval mode as the edge MLP's reference plus stage 5, in float64, with the bound of the FUSED route.
    scale = weight / sqrt(var + eps) is three rounded operations (add, sqrt, divide) and shift = bias - mean * scale two
    more on top of scale's (multiply, subtract), so a stage's t grows by 5 extra roundings -- 3 on the scale's term, at
    most 5 on the shift's, whose magnitude is taken as |bias| + |mean * scale| >= |shift|.  Stage 5 fits the same count:
    its weight diag(scale_5) W_5 carries scale's 3 roundings and the product's 1 (<= 5), then K = 512 multiply-adds and
    the bias."""
    bns = [getattr(net64, "bn%d" % i) for i in range(1, 6)]
    scales = [bn.weight / torch.sqrt(bn.running_var + bn.eps) for bn in bns]
    shifts = [bn.bias - bn.running_mean * s for bn, s in zip(bns, scales)]
    shift_mags = [bn.bias.abs() + (bn.running_mean * s).abs() for bn, s in zip(bns, scales)]
    weights = [getattr(net64, "conv%d" % i).weight.flatten(1) for i in range(1, 6)]
    idx = graph.transpose(1, 2)
    r = cases.reference(x, idx, weights[:4], scales[:4], shifts[:4], extra=5, shift_mags=shift_mags[:4])
    t5 = r["t"].max() + 512 + 2 + 5
    pre = torch.einsum("oc,bcn->bon", weights[4].detach(), r["out"])
    out = torch.relu(scales[4].view(1, -1, 1) * pre + shifts[4].view(1, -1, 1)).detach()
    mag = (scales[4].abs().view(1, -1, 1) * torch.einsum("oc,bcn->bon", weights[4].abs(), r["mag"])
           + shift_mags[4].view(1, -1, 1)).detach()
    return {"out": out, "mag": mag, "t": torch.full((1, 512, 1), float(t5), dtype=torch.float64)}


def _golden_clouds():
    g = np.load(os.path.join(GOLD, "dcp_golden.npz"))
    return torch.tensor(g["src"]).transpose(1, 2).contiguous()              # (2, 3, 64)


@gpu
@pytest.mark.parametrize("which", ["golden", "300"])
def test_dgcnn_module_against_its_float64_copy(which, monkeypatch):
    """DGCNN in eval mode on the GPU with the switch on (mvp_edge_mlp_max + one MFMA GEMM) and off (the composed route)
    against a float64 CPU copy of the module on the same neighbour graph (taken from the float64 copy's knn and injected,
    so the test is about the op, not about kNN ties).  The fused route must stay within the rounding bound
    (_module_reference counts the roundings of scale and shift); both routes' largest errors are printed (-s)."""
    from mvp_benchmark_amd.registration import routes
    dcp = load_dcp("edge_mlp_gpu")
    net = _randomised_dgcnn(dcp)
    x = _golden_clouds() if which == "golden" else torch.randn(2, 3, 300, generator=torch.Generator().manual_seed(13))
    net64 = copy.deepcopy(net).double()
    graph = dcp._mu.knn(x.double(), 20)                                     # (B, N, k)
    monkeypatch.setattr(dcp._mu, "knn", lambda feats, kk: graph.to(feats.device))
    with torch.no_grad():
        want = net64(x.double())
    ref = _module_reference(net64, x.double(), graph)
    assert float((ref["out"] - want).abs().max()) <= 1e-9 * float(want.abs().max())      # two float64 formulations
    netd, xd = copy.deepcopy(net).to(DEV), x.to(DEV)
    outs = {}
    for on in (True, False):
        with routes(edge_mlp=on), abi_call_names() as names, torch.no_grad():
            outs[on] = netd(xd).cpu()
        assert ("mvp_edge_mlp_max" in names) == on and ("mvp_group_points" in names) == (not on), names
        if on:
            assert names.count("mvp_edge_mlp_max") == 1 and names.count("mvp_pointwise_mfma_ex") == 1
    assert outs[True].shape == want.shape
    share = cases.bound_share(outs[True], ref)
    print("DGCNN %s: fused %.3e of the bound, largest error fused %.3e composed %.3e (largest value %.3e)" % (
        which, share, float((outs[True].double() - want).abs().max()), float((outs[False].double() - want).abs().max()),
        float(want.abs().max())))
    assert share <= 1.0
    # train() mode: batch statistics, so the op is not called and the switch changes nothing, bit for bit
    trained = {}
    for on in (True, False):
        nett = copy.deepcopy(net).to(DEV).train()
        with routes(edge_mlp=on), abi_call_names() as names, torch.no_grad():
            trained[on] = nett(xd).cpu()
        assert "mvp_edge_mlp_max" not in names and "mvp_group_points" in names
    assert torch.equal(trained[True], trained[False])


@gpu
def test_dcp_model_matches_the_reference_fixture_on_the_fused_route():
    """Model's forward with the switch on against tests/golden/dcp_golden.npz (generated from the imported reference):
    the tolerances of the composed route's fixture test, restated."""
    if GOLD not in sys.path:
        sys.path.insert(0, GOLD)
    from make_dcp_golden import fill_parameters
    from mvp_benchmark_amd.registration import routes
    dcp = load_dcp("edge_mlp_gpu")
    g = np.load(os.path.join(GOLD, "dcp_golden.npz"))
    net = dcp.Model(types.SimpleNamespace())
    fill_parameters(net)
    net = net.eval().to(DEV)
    src, tgt, T_gt = (torch.tensor(g[k], device=DEV) for k in ("src", "tgt", "T_gt"))
    with routes(edge_mlp=True), abi_call_names() as names, torch.no_grad():
        T_12 = net(src, tgt)
        loss, r_err, t_err, rmse, rt_mse = net(src, tgt, T_gt)
    assert names.count("mvp_edge_mlp_max") == 4 and "mvp_group_points" not in names
    np.testing.assert_allclose(T_12.cpu().numpy(), g["T_12"], atol=2e-4)
    np.testing.assert_allclose(loss.cpu().numpy(), g["loss"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(r_err.cpu().numpy(), g["r_err"], rtol=1e-3, atol=2e-2)
    np.testing.assert_allclose(t_err.cpu().numpy(), g["t_err"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(rmse.cpu().numpy(), g["rmse"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(rt_mse.cpu().numpy(), g["rt_mse"], rtol=1e-3, atol=5e-4)
