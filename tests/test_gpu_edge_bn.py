"""The fused BatchNorm + ReLU + max over the neighbours (csrc/edge_bn.hip, registration.bn_relu_max, DGCNN's opt-in training
route) against the float64 reference and the bounds of tests/edge_bn_cases.py.  Every shape runs through the C ABI on
NaN-filled outputs (an element no lane writes stays NaN) and through the wrapper.

Model level, measured on an MI355X (test_dgcnn_against_its_float64_copy prints them; profiles/dcp_edge_bn.txt keeps them): the
worst tensor's max |difference| / max |reference| on the golden clouds is 2.514e-06 on the fused route against 2.547e-06 on
the composed one, on the random (2, 3, 68) input 1.398e-06 against 1.712e-06; the fused route's may be at most 4 times the
composed route's.  The kernels use at most 0.42 of any bound of tests/edge_bn_cases.py."""
import copy
import os
import types

import numpy as np
import pytest
import torch
from conftest import ROOT

import edge_bn_cases as cases
from dcp_util import abi_call_names, load_dcp, rel_err

DEV = "cuda:0"
gpu = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
EBADSHAPE, EBADARG = "MVP_EBADSHAPE", "MVP_EBADARG"
GRADS = ("g_r", "g_pool", "both")


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def cpu(t):
    return None if t is None else t.cpu()


def abi_stats(z, eps=cases.EPS):
    """mvp_edge_bn_stats on NaN-filled outputs -> (stats (C,2), var (C)), CPU tensors."""
    from mvp_benchmark_amd import _lib
    B, C, k, N = z.shape
    stats, var = nan_like(C, 2), nan_like(C)
    nbytes = _lib.edge_bn_scratch_bytes(B, C)
    scratch = torch.full((nbytes,), 255, device=DEV, dtype=torch.uint8)
    _lib.call("mvp_edge_bn_stats", DEV, B, C, k, N, z.to(DEV), eps, stats, var, scratch, nbytes)
    torch.cuda.synchronize()
    return stats.cpu(), var.cpu()


def running_stats(case, eps=cases.EPS):
    """{running_mean, 1 / sqrt(running_var + eps)} as the wrapper forms them: the root in double, rounded once."""
    return torch.stack((case["running_mean"], (1 / torch.sqrt(case["running_var"].double() + eps)).float()), dim=1).contiguous()


def abi_forward(z, stats, gamma, beta, want_r=True):
    """mvp_edge_bn_relu_max on NaN-filled outputs -> (r or None, pooled, arg), CPU tensors."""
    from mvp_benchmark_amd import _lib
    B, C, k, N = z.shape
    r = nan_like(B, C, k, N) if want_r else None
    pooled = nan_like(B, C, N)
    arg = torch.full((B, C, N), 255, device=DEV, dtype=torch.uint8)
    _lib.call("mvp_edge_bn_relu_max", DEV, B, C, k, N, z.to(DEV), stats.to(DEV), gamma.to(DEV), beta.to(DEV), r, pooled, arg)
    torch.cuda.synchronize()
    return cpu(r), pooled.cpu(), arg.cpu()


def abi_backward(z, stats, gamma, beta, arg, g_r, g_pool, batch, sums=True):
    """mvp_edge_bn_relu_max_backward on NaN-filled outputs -> (gz, ggamma, gbeta) CPU tensors (the sums None without `sums`)."""
    from mvp_benchmark_amd import _lib
    B, C, k, N = z.shape
    gz = nan_like(B, C, k, N)
    ggamma, gbeta = (nan_like(C), nan_like(C)) if sums else (None, None)
    need = sums or batch
    nbytes = _lib.edge_bn_scratch_bytes(B, C) if need else 0
    scratch = torch.full((nbytes,), 255, device=DEV, dtype=torch.uint8) if need else None
    dev = lambda t: None if t is None else t.to(DEV)
    _lib.call("mvp_edge_bn_relu_max_backward", DEV, B, C, k, N, int(batch), z.to(DEV), stats.to(DEV), gamma.to(DEV),
              beta.to(DEV), arg.to(DEV), dev(g_r), dev(g_pool), gz, ggamma, gbeta, scratch, nbytes)
    torch.cuda.synchronize()
    return gz.cpu(), cpu(ggamma), cpu(gbeta)


def pick(case, grads):
    return (case["g_r"] if grads != "g_pool" else None), (case["g_pool"] if grads != "g_r" else None)


def wrapper_run(case, training, grads, want_r=True, z=None):
    """bn_relu_max and its backward on the GPU -> dict of CPU tensors (running statistics after the call included)."""
    from mvp_benchmark_amd.registration import bn_relu_max
    leaf = lambda t: t.to(DEV).requires_grad_()
    zd, gd, bd = leaf(case["z"] if z is None else z), leaf(case["gamma"]), leaf(case["beta"])
    rm, rv = case["running_mean"].to(DEV), case["running_var"].to(DEV)
    r, pooled = bn_relu_max(zd, gd, bd, rm, rv, training, cases.MOMENTUM, cases.EPS, want_r)
    g_r, g_pool = pick(case, grads)
    outs, gs = zip(*[(o, g.to(DEV)) for o, g in ((r, g_r), (pooled, g_pool)) if g is not None and o is not None])
    torch.autograd.backward(outs, gs)
    return {"r": None if r is None else r.detach().cpu(), "pooled": pooled.detach().cpu(), "gz": zd.grad.cpu(),
            "ggamma": gd.grad.cpu(), "gbeta": bd.grad.cpu(), "running_mean": rm.cpu(), "running_var": rv.cpu()}


def within(tag, name, got, want, mag, t):
    assert not bool(torch.isnan(got).any()), (tag, name)
    s = cases.share(got, want, mag, t)
    print("%s %s: %.3f of the bound (t = %d)" % (tag, name, s, t))
    assert s <= 1.0, (tag, name, s)


def check_arg(tag, r, pooled, arg, k):
    """arg points at a maximal element of the kernel's own r, and at the lowest such neighbour."""
    assert int(arg.max()) < k, tag
    at = r.gather(2, arg.long().unsqueeze(2)).squeeze(2)
    assert torch.equal(at, pooled) and torch.equal(pooled, r.max(dim=2)[0]), tag
    lowest = (r == pooled.unsqueeze(2)).int().argmax(dim=2)
    assert torch.equal(arg.long(), lowest), tag


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@gpu
@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_bounds_and_exact_relations(shape):
    B, C, k, N = shape
    for family in cases.FAMILIES:
        case = cases.make_case(shape, family)
        z, gamma, beta = case["z"], case["gamma"], case["beta"]
        for batch in (True, False):
            tag = "%s %s %s" % (shape, family, "batch" if batch else "running")
            ref = cases.reference(z, gamma, beta, running=None if batch else (case["running_mean"], case["running_var"]))
            if batch:
                stats, var = abi_stats(z)
                within(tag, "mean", stats[:, 0], ref["mean"], ref["mag_mean"], cases.T_Y)
                within(tag, "invstd", stats[:, 1], ref["invstd"], ref["mag_invstd"], cases.T_Y)
                within(tag, "var", var, ref["var"], ref["mag_var"], cases.T_Y)
            else:
                stats = running_stats(case)
            # ---- forward: arg first, then r and pooled
            r, pooled, arg = abi_forward(z, stats, gamma, beta)
            check_arg(tag, r, pooled, arg, k)
            within(tag, "r", r, ref["r"], ref["mag_y"], cases.T_Y)
            within(tag, "pooled", pooled, ref["pooled"], ref["mag_pooled"], cases.T_Y)
            none, pooled_n, arg_n = abi_forward(z, stats, gamma, beta, want_r=False)
            assert none is None and torch.equal(pooled_n, pooled) and torch.equal(arg_n, arg), tag
            # ---- backward, the reference's mask and arg taken from the kernel's forward
            for grads in GRADS:
                g_r, g_pool = pick(case, grads)
                back = cases.reference_backward(ref, r > 0, arg, g_r, g_pool)
                gz, ggamma, gbeta = abi_backward(z, stats, gamma, beta, arg, g_r, g_pool, batch)
                t2 = "%s %s" % (tag, grads)
                within(t2, "gz", gz, back["gz"], back["mag_gz"], cases.T_GZ)
                within(t2, "ggamma", ggamma, back["ggamma"], back["mag_ggamma"], cases.T_GGAMMA)
                within(t2, "gbeta", gbeta, back["gbeta"], back["mag_gbeta"], cases.T_GBETA)
                gz_n, none_a, none_b = abi_backward(z, stats, gamma, beta, arg, g_r, g_pool, batch, sums=False)
                assert torch.equal(gz_n, gz) and none_a is None and none_b is None, t2
                # ---- the wrapper: the same kernels, the same bits; want_r=False changes none of them
                w = wrapper_run(case, batch, grads)
                assert torch.equal(w["r"], r) and torch.equal(w["pooled"], pooled) and torch.equal(w["gz"], gz), t2
                assert torch.equal(w["ggamma"], ggamma) and torch.equal(w["gbeta"], gbeta), t2
                if grads == "g_pool":
                    wn = wrapper_run(case, batch, grads, want_r=False)
                    assert wn["r"] is None and torch.equal(wn["pooled"], pooled) and torch.equal(wn["gz"], gz), t2
                    assert torch.equal(wn["ggamma"], ggamma) and torch.equal(wn["gbeta"], gbeta), t2
            # ---- the running statistics: moved as nn.BatchNorm2d moves them in training, untouched otherwise
            if batch and B * k * N > 1:
                M = ref["M"]
                want_mean = (1 - cases.MOMENTUM) * case["running_mean"].double() + cases.MOMENTUM * ref["mean"]
                want_var = (1 - cases.MOMENTUM) * case["running_var"].double() + cases.MOMENTUM * ref["var"] * M / (M - 1)
                within(tag, "running_mean", w["running_mean"], want_mean, case["running_mean"].double().abs() + ref["mag_mean"], 4)
                within(tag, "running_var", w["running_var"], want_var, case["running_var"].double() + ref["mag_var"] * M / (M - 1), 4)
            elif not batch:
                assert torch.equal(w["running_mean"], case["running_mean"]) and torch.equal(w["running_var"], case["running_var"])


@gpu
def test_two_runs_give_the_same_bits():
    for shape in ((2, 64, 20, 260), (1, 2, 64, 1028), (3, 5, 7, 68)):
        case = cases.make_case(shape, cases.FAMILIES[1])
        z, gamma, beta = case["z"], case["gamma"], case["beta"]
        stats, var = abi_stats(z)
        r, pooled, arg = abi_forward(z, stats, gamma, beta)
        first = {batch: abi_backward(z, stats, gamma, beta, arg, case["g_r"], case["g_pool"], batch) for batch in (True, False)}
        for _ in range(2):
            s2, v2 = abi_stats(z)
            assert torch.equal(s2, stats) and torch.equal(v2, var)
            assert all(torch.equal(u, v) for u, v in zip(abi_forward(z, stats, gamma, beta), (r, pooled, arg)))
            for batch in (True, False):
                again = abi_backward(z, stats, gamma, beta, arg, case["g_r"], case["g_pool"], batch)
                assert all(torch.equal(u, v) for u, v in zip(again, first[batch]))


@gpu
@pytest.mark.parametrize("batch", [True, False], ids=["batch", "running"])
def test_dead_channels_are_exact(batch):
    """gamma = 0 with beta < 0, and a beta far below every gamma xhat: every y <= 0, so r = pooled = 0, arg = 0, gz = 0 and
    ggamma = gbeta = 0 exactly; the live channel between them is within its bounds."""
    shape = (2, 3, 20, 68)
    case = cases.make_case(shape, cases.FAMILIES[1])
    z, gamma, beta = case["z"], case["gamma"].clone(), case["beta"].clone()
    gamma[0], beta[0] = 0.0, -1.0
    beta[2] = -100.0
    stats = abi_stats(z)[0] if batch else running_stats(case)
    r, pooled, arg = abi_forward(z, stats, gamma, beta)
    gz, ggamma, gbeta = abi_backward(z, stats, gamma, beta, arg, case["g_r"], case["g_pool"], batch)
    zero = lambda t: bool((t == 0).all())
    for ch in (0, 2):
        assert zero(r[:, ch]) and zero(pooled[:, ch]) and zero(arg[:, ch]) and zero(gz[:, ch]), ch
        assert float(ggamma[ch]) == 0.0 and float(gbeta[ch]) == 0.0, ch
    ref = cases.reference(z, gamma, beta, running=None if batch else (case["running_mean"], case["running_var"]))
    back = cases.reference_backward(ref, r > 0, arg, case["g_r"], case["g_pool"])
    assert bool((back["mag_gz"][:, 0] == 0).all()) and bool((r[:, 1] > 0).any())
    within("dead", "r", r, ref["r"], ref["mag_y"], cases.T_Y)
    within("dead", "gz", gz, back["gz"], back["mag_gz"], cases.T_GZ)          # a bound of 0 asks for exactness
    within("dead", "ggamma", ggamma, back["ggamma"], back["mag_ggamma"], cases.T_GGAMMA)
    w = wrapper_run(dict(case, gamma=gamma, beta=beta), batch, "both")
    assert torch.equal(w["r"], r) and torch.equal(w["gz"], gz) and torch.equal(w["gbeta"], gbeta)


@gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=str)
def test_non_finite_values_with_batch_statistics(bad):
    """One non-finite z makes its channel's statistics, r, pooled and gz NaN; the other channels keep every bit."""
    shape = (3, 4, 7, 68)
    case = cases.make_case(shape, cases.FAMILIES[1])
    z, gamma, beta = case["z"], case["gamma"].clone(), case["beta"]
    gamma[1] = 0.0                                                    # 0 * NaN: the scale must not hide the channel
    def run(zz):
        stats, var = abi_stats(zz)
        r, pooled, arg = abi_forward(zz, stats, gamma, beta)
        return (stats, var, r, pooled, arg) + abi_backward(zz, stats, gamma, beta, arg, case["g_r"], case["g_pool"], True)
    clean = run(z)
    zb = z.clone()
    zb[1, 1, 3, 67] = bad
    zb[2, 3, 0, 0] = bad
    stats, var, r, pooled, arg, gz, ggamma, gbeta = run(zb)
    keep = [0, 2]
    for ch in (1, 3):
        assert bool(torch.isnan(stats[ch]).all()) and bool(torch.isnan(var[ch])), ch
        assert bool(torch.isnan(r[:, ch]).all()) and bool(torch.isnan(pooled[:, ch]).all()) and bool(torch.isnan(gz[:, ch]).all()), ch
        assert bool(torch.isnan(ggamma[ch])), ch
    for got, want in zip((stats, var), clean[:2]):
        assert same_bits(got[keep], want[keep])
    for got, want in zip((r, pooled, gz), (clean[2], clean[3], clean[5])):
        assert same_bits(got[:, keep], want[:, keep])
    assert torch.equal(arg[:, keep], clean[4][:, keep])
    assert same_bits(ggamma[keep], clean[6][keep]) and same_bits(gbeta[keep], clean[7][keep])
    w = wrapper_run(dict(case, gamma=gamma), True, "both", z=zb)
    assert torch.equal(torch.isnan(w["r"]), torch.isnan(r)) and same_bits(w["r"][:, keep], r[:, keep])
    assert torch.equal(torch.isnan(w["gz"]), torch.isnan(gz)) and same_bits(w["gz"][:, keep], gz[:, keep])
    assert bool(torch.isnan(w["running_mean"][[1, 3]]).all()) and not bool(torch.isnan(w["running_mean"][keep]).any())


@gpu
def test_non_finite_values_with_running_statistics():
    """The map is elementwise: a NaN z makes its own r and its column's pooled NaN (arg = its neighbour) and nothing else; an
    Inf gives y = +-Inf.  Every other element of r, pooled, arg and gz keeps its bits; the NaN element's gz is 0."""
    shape = (3, 4, 7, 68)
    case = cases.make_case(shape, cases.FAMILIES[1])
    z, gamma, beta = case["z"], case["gamma"], case["beta"]
    stats = running_stats(case)
    r0, pooled0, arg0 = abi_forward(z, stats, gamma, beta)
    gz0, ggamma0, gbeta0 = abi_backward(z, stats, gamma, beta, arg0, case["g_r"], case["g_pool"], False)
    zb = z.clone()
    zb[1, 1, 3, 67] = float("nan")
    zb[1, 1, 5, 67] = float("nan")                                   # a second NaN in the column: the lowest neighbour is named
    zb[2, 3, 2, 0] = float("inf") * (1 if float(gamma[3]) > 0 else -1)          # y = +Inf
    r, pooled, arg = abi_forward(zb, stats, gamma, beta)
    gz, ggamma, gbeta = abi_backward(zb, stats, gamma, beta, arg, case["g_r"], case["g_pool"], False)
    assert bool(torch.isnan(r[1, 1, 3, 67])) and bool(torch.isnan(r[1, 1, 5, 67])) and bool(torch.isnan(pooled[1, 1, 67]))
    assert int(arg[1, 1, 67]) == 3 and float(gz[1, 1, 3, 67]) == 0.0
    assert float(r[2, 3, 2, 0]) == float("inf") and float(pooled[2, 3, 0]) == float("inf") and int(arg[2, 3, 0]) == 2
    assert int(torch.isnan(r).sum()) == 2 and int(torch.isnan(pooled).sum()) == 1 and not bool(torch.isnan(gz).any())
    touched = torch.zeros(shape, dtype=torch.bool)
    touched[1, 1, :, 67] = True
    touched[2, 3, :, 0] = True                                       # the two columns whose arg moved
    assert same_bits(r[~touched], r0[~touched]) and same_bits(gz[~touched], gz0[~touched])
    cols = touched.any(dim=2)
    assert same_bits(pooled[~cols], pooled0[~cols]) and torch.equal(arg[~cols], arg0[~cols])
    assert same_bits(ggamma[[0, 2]], ggamma0[[0, 2]]) and same_bits(gbeta[[0, 2]], gbeta0[[0, 2]])


@gpu
def test_ties_go_to_the_lowest_neighbour():
    """Duplicated neighbours (a cloud with duplicated points): arg is the lowest of the equal maxima and the pooled gradient
    goes there only.  With running statistics gz = gamma invstd g_y is elementwise, so every other neighbour's gz is 0."""
    shape = (2, 3, 8, 68)
    case = cases.make_case(shape, cases.FAMILIES[0])
    z = case["z"].clone()
    z[:, :, 5], z[:, :, 6], z[:, :, 7], z[:, :, 4] = z[:, :, 1], z[:, :, 1], z[:, :, 2], z[:, :, 0]
    stats = running_stats(case)
    r, pooled, arg = abi_forward(z, stats, case["gamma"], case["beta"])
    check_arg("ties", r, pooled, arg, 8)
    assert int(arg.max()) <= 3 and int((r == pooled.unsqueeze(2)).sum(dim=2).max()) >= 3
    gz, _, _ = abi_backward(z, stats, case["gamma"], case["beta"], arg, None, case["g_pool"], False)
    hit = torch.zeros(shape, dtype=torch.bool).scatter_(2, arg.long().unsqueeze(2), True)
    assert bool((gz[~hit] == 0).all())
    want = (case["gamma"] * stats[:, 1]).view(1, -1, 1) * case["g_pool"] * (pooled > 0)
    assert torch.equal(gz.sum(dim=2), want)                          # one non-zero term per column: the sum is that term
    w = wrapper_run(dict(case), False, "g_pool", z=z)
    assert torch.equal(w["gz"], gz)
    # batch statistics through the wrapper against the composition's CPU rule
    wb = wrapper_run(dict(case), True, "g_pool", z=z)
    lowest = (wb["r"] == wb["pooled"].unsqueeze(2)).int().argmax(dim=2)
    assert int(lowest.max()) <= 3
    ref = cases.reference(z, case["gamma"], case["beta"])
    back = cases.reference_backward(ref, wb["r"] > 0, lowest, None, case["g_pool"])
    within("ties batch", "gz", wb["gz"], back["gz"], back["mag_gz"], cases.T_GZ)


@gpu
def test_refusals_and_the_composed_route():
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd.registration import bn_relu_max
    case = cases.make_case((2, 3, 5, 8), cases.FAMILIES[0])
    d = {k: v.to(DEV) for k, v in case.items()}
    stats, pooled = nan_like(3, 2), nan_like(2, 3, 8)
    arg = torch.zeros(2, 3, 8, device=DEV, dtype=torch.uint8)
    for n in (6, 2):
        with pytest.raises(_lib.MvpOpsError, match=EBADSHAPE):
            _lib.call("mvp_edge_bn_relu_max", DEV, 2, 3, 5, n, d["z"], stats, d["gamma"], d["beta"], None, pooled, arg)
    with pytest.raises(_lib.MvpOpsError, match=EBADSHAPE):
        _lib.call("mvp_edge_bn_relu_max", DEV, 2, 3, 65, 8, d["z"], stats, d["gamma"], d["beta"], None, pooled, arg)
    with pytest.raises(_lib.MvpOpsError, match=EBADARG):
        _lib.call("mvp_edge_bn_relu_max_backward", DEV, 2, 3, 5, 8, 0, d["z"], stats, d["gamma"], d["beta"], arg, None, None,
                  d["g_r"], None, None, None, 0)
    assert bool(torch.isnan(pooled).all())                            # nothing ran
    # the wrapper keeps what the kernels refuse away from them: N % 4 != 0, an unaligned view, a non-contiguous one, k > 64
    big = torch.randn(2 * 3 * 5 * 8 + 4, device=DEV)
    odd = big[1:241].view(2, 3, 5, 8)
    assert odd.data_ptr() % 16 == 4
    inputs = {"N = 6": torch.randn(2, 3, 5, 6, device=DEV), "unaligned": odd,
              "non-contiguous": torch.randn(2, 3, 8, 5, device=DEV).transpose(2, 3), "k = 65": torch.randn(1, 3, 65, 4, device=DEV)}
    for name, zz in inputs.items():
        for training in (True, False):
            za, zb = zz.detach().requires_grad_(), zz.detach().requires_grad_()      # two leaves on the view itself
            ga, ba, gb, bb = (d[n].clone().requires_grad_() for n in ("gamma", "beta", "gamma", "beta"))
            rm_a, rv_a, rm_b, rv_b = d["running_mean"].clone(), d["running_var"].clone(), d["running_mean"].clone(), d["running_var"].clone()
            with abi_call_names() as names:
                r, pooled_w = bn_relu_max(za, ga, ba, rm_a, rv_a, training, cases.MOMENTUM, cases.EPS)
                (r.sum() + 2 * pooled_w.sum()).backward()
            assert names == [], (name, names)
            rc, pc, _ = cases.compose(zb, gb, bb, rm_b, rv_b, training)
            (rc.sum() + 2 * pc.sum()).backward()
            assert torch.equal(r, rc) and torch.equal(pooled_w, pc) and torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b), name
            assert torch.equal(za.grad, zb.grad) and torch.equal(ga.grad, gb.grad) and torch.equal(ba.grad, bb.grad), name
    # ... and what they take reaches them
    with abi_call_names() as names:
        r, pooled_w = bn_relu_max(d["z"], d["gamma"], d["beta"], d["running_mean"].clone(), d["running_var"].clone(), True, cases.MOMENTUM, cases.EPS)
    assert names == ["mvp_edge_bn_stats", "mvp_edge_bn_relu_max"]


# ---------------------------------------------------------------------------------------------- the module and the model

@gpu
@pytest.mark.parametrize("which", ["golden", "random68"])
def test_dgcnn_against_its_float64_copy(which):
    """DGCNN in train mode on the GPU in float32, fused route and composed route, each against a float64 CPU copy run on the
    SAME neighbour graph (the GPU's: a float64 kNN may order two nearly equidistant neighbours differently, which is no
    rounding error of these stages).  A tensor's error = max |difference| / max |reference|, over the output, the input's
    gradient, every parameter gradient and every running statistic; a ROUTE's error is its worst tensor's.  The fused route's
    may be at most 4 times the composed route's: both carry the convolutions' rounding, which dominates."""
    from mvp_benchmark_amd.registration import routes
    dcp = load_dcp("edge_bn_gpu")
    torch.manual_seed(31)
    net = dcp.DGCNN().train()
    with torch.no_grad():                                       # BatchNorms away from gamma = 1, beta = 0
        for name, p in net.named_parameters():
            if name.startswith("bn"):
                p.add_(0.3 * torch.randn_like(p))
    if which == "golden":
        x = torch.tensor(np.load(os.path.join(GOLD, "dcp_golden.npz"))["src"]).transpose(1, 2).contiguous()      # (2, 3, 64)
    else:
        x = torch.randn(2, 3, 68, generator=torch.Generator().manual_seed(32))
    w = torch.randn(2, dcp.EMB_DIMS, x.shape[2], generator=torch.Generator().manual_seed(33)).double()
    with torch.no_grad():
        graph = dcp._mu.knn(x.to(DEV), 20).cpu()

    def run(model, xin, weight):
        model.zero_grad(set_to_none=True)
        xin = xin.clone().requires_grad_()
        out = model(xin)
        (out * weight).sum().backward()
        tensors = {"output": out.detach(), "grad input": xin.grad}
        tensors.update({"grad " + k: p.grad for k, p in model.named_parameters()})
        tensors.update({k: v for k, v in model.state_dict().items() if "running_" in k})
        return tensors, {k: int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")}

    net64 = copy.deepcopy(net).double()
    real_knn = dcp._mu.knn
    dcp._mu.knn = lambda t, k: graph if not t.is_cuda else real_knn(t, k)
    try:
        want, want_count = run(net64, x.double(), w)
    finally:
        dcp._mu.knn = real_knn
    errs = {}
    for on in (True, False):
        netd = copy.deepcopy(net).to(DEV)
        with routes(edge_bn=on), abi_call_names() as names:
            got, count = run(netd, x.to(DEV), w.float().to(DEV))
        assert names.count("mvp_edge_bn_stats") == (4 if on else 0), names
        assert names.count("mvp_edge_bn_relu_max") == names.count("mvp_edge_bn_relu_max_backward") == (4 if on else 0), names
        assert count == want_count and all(v == 1 for v in count.values()) and len(count) == 5
        assert got.keys() == want.keys() and all(bool(torch.isfinite(v).all()) for v in got.values())
        errs[on] = {k: rel_err(got[k], want[k]) for k in want}
    for k in errs[True]:
        print("DGCNN %s %-28s fused %.3e composed %.3e" % (which, k, errs[True][k], errs[False][k]))
    worst = {on: max(errs[on].values()) for on in (True, False)}
    print("DGCNN %s: worst tensor fused %.3e (%s) composed %.3e (%s)" % (
        which, worst[True], max(errs[True], key=errs[True].get), worst[False], max(errs[False], key=errs[False].get)))
    assert worst[True] <= 4 * worst[False], worst


@gpu
def test_dcp_training_step_on_the_fused_route():
    """One Model training step with T_gt and the switch on: a finite loss, a gradient on every parameter, the module tree of
    the switched-off model (and the golden fixture's parameter names), num_batches_tracked counted once per cloud."""
    from mvp_benchmark_amd.registration import routes
    dcp = load_dcp("edge_bn_gpu")
    g = np.load(os.path.join(GOLD, "dcp_golden.npz"))
    torch.manual_seed(34)
    net = dcp.Model(types.SimpleNamespace())
    keys = list(net.state_dict())
    assert set(str(n) for n in g["names"]) <= set(keys)
    net = net.train().to(DEV)
    src, tgt, T_gt = (torch.tensor(g[k], device=DEV) for k in ("src", "tgt", "T_gt"))
    with routes(edge_bn=True), abi_call_names() as names:
        loss = net(src, tgt, T_gt)[0].mean()
        loss.backward()
    assert names.count("mvp_edge_bn_stats") == 8 and names.count("mvp_edge_bn_relu_max_backward") == 8, names
    assert bool(torch.isfinite(loss))
    grads = {k: p.grad for k, p in net.named_parameters() if p.requires_grad}
    bad = [k for k, v in grads.items() if v is None or not bool(torch.isfinite(v).all())]
    assert not bad and len(grads) > 60, bad
    assert list(net.state_dict()) == keys
    assert all(int(getattr(net.emb_nn, "bn%d" % i).num_batches_tracked) == 2 for i in range(1, 6))
    # eval without gradients stays on the composed route
    net.eval()
    with routes(edge_bn=True), abi_call_names() as names, torch.no_grad():
        net(src, tgt)
    assert not any(n.startswith("mvp_edge_bn") for n in names), names
    import mvp_benchmark_amd.registration as R_
    assert R_.EDGE_BN is False
