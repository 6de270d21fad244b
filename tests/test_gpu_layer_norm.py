"""The fused LayerNorm + residual sum (csrc/layer_norm.hip, registration.ref_layer_norm, the transformer's opt-in route) against
the float64 reference and the bounds of tests/layer_norm_cases.py.  Every shape runs through the C ABI on NaN-filled
outputs (an element no lane writes stays NaN) and through the wrapper."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch
from conftest import ROOT

import layer_norm_cases as cases
from dcp_util import abi_call_names, load_dcp, rel_err

DEV = "cuda:0"
gpu = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
EBADSHAPE, EBADARG = "MVP_EBADSHAPE", "MVP_EBADARG"

# The grid is min(ceil(rows / 4), 2048) workgroups of four rows: with 4 * 2048 + 5 rows the first workgroups take a second
# trip of their grid-stride loop, two of them with a partial set of waves (test_grid_formula reads it off the scratch size).
LOOPING = (4 * 2048 + 5, 4)
SHAPES = [(rows, d) for rows in cases.ROWS for d in cases.DIMS] + [LOOPING]


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def abi_forward(x, a, b, delta=None, eps=cases.EPS, want_stats=True):
    """mvp_ref_layernorm on NaN-filled outputs -> (sum or None, y, stats or None), CPU tensors."""
    from mvp_benchmark_amd import _lib
    rows, d = x.shape
    xd, ad, bd = x.to(DEV), a.to(DEV), b.to(DEV)
    dd = None if delta is None else delta.to(DEV)
    total = None if delta is None else nan_like(rows, d)
    y, stats = nan_like(rows, d), (nan_like(rows, 2) if want_stats else None)
    _lib.call("mvp_ref_layernorm", DEV, rows, d, xd, dd, ad, bd, eps, total, y, stats)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()
    return cpu(total), cpu(y), cpu(stats)


def abi_backward(z, a, gy, stats, gres=None, cols=True, eps=cases.EPS):
    """mvp_ref_layernorm_backward on NaN-filled outputs -> (gz, ga, gb) CPU tensors (ga, gb None without cols)."""
    from mvp_benchmark_amd import _lib
    rows, d = z.shape
    gz = nan_like(rows, d)
    ga, gb = (nan_like(d), nan_like(d)) if cols else (None, None)
    nbytes = _lib.ref_layernorm_backward_scratch_bytes(rows, d) if cols else 0
    scratch = torch.full((nbytes // 4,), float("nan"), device=DEV) if cols else None
    _lib.call("mvp_ref_layernorm_backward", DEV, rows, d, z.to(DEV), a.to(DEV), gy.to(DEV),
              None if gres is None else gres.to(DEV), stats.to(DEV), eps, gz, ga, gb, scratch, nbytes)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()
    return cpu(gz), cpu(ga), cpu(gb)


def wrapper_run(x, a, b, gy, delta=None, gres=None):
    """ref_layer_norm and its backward on the GPU -> dict of CPU tensors."""
    from mvp_benchmark_amd.registration import ref_layer_norm
    leaf = lambda t: None if t is None else t.to(DEV).requires_grad_()
    xd, ad, bd, dd = leaf(x), leaf(a), leaf(b), leaf(delta)
    if delta is None:
        y = ref_layer_norm(xd, ad, bd, cases.EPS)
        y.backward(gy.to(DEV))
        total = None
    else:
        total, y = ref_layer_norm(xd, ad, bd, cases.EPS, dd)
        outs, grads = ([y], [gy.to(DEV)]) if gres is None else ([y, total], [gy.to(DEV), gres.to(DEV)])
        torch.autograd.backward(outs, grads)
        assert torch.equal(dd.grad.view(torch.int32), xd.grad.view(torch.int32))     # the same bits, NaN rows included
    return {"sum": None if total is None else total.detach().cpu(), "y": y.detach().cpu(), "gz": xd.grad.cpu(),
            "ga": ad.grad.cpu(), "gb": bd.grad.cpu()}


def check_bounds(tag, ref, rows, y=None, gz=None, ga=None, gb=None):
    for name, got, mag, t in (("y", y, "mag_y", cases.T_ROW), ("gz", gz, "mag_gz", cases.T_ROW),
                              ("ga", ga, "mag_ga", cases.t_cols(rows)), ("gb", gb, "mag_gb", cases.t_cols(rows))):
        if got is None:
            continue
        assert not bool(torch.isnan(got).any()), (tag, name)
        s = cases.share(got, ref[name], ref[mag], t)
        print("%s %s: %.3f of the bound (t = %d)" % (tag, name, s, t))
        assert s <= 1.0, (tag, name, s)


@gpu
def test_grid_formula():
    from mvp_benchmark_amd import _lib
    rows, d = LOOPING
    grid = _lib.ref_layernorm_backward_scratch_bytes(rows, d) // (2 * d * 4)
    assert grid == 2048 and rows > 4 * grid
    assert _lib.ref_layernorm_backward_scratch_bytes(257, 512) // (2 * 512 * 4) == 65


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bounds_and_exact_relations(shape):
    rows, d = shape
    for family in cases.FAMILIES:
        case = cases.make_case(rows, d, family)
        x, delta, a, b, gy, gres = (case[k] for k in ("x", "delta", "a", "b", "gy", "gres"))
        tag = "%s %s" % (shape, family)
        # ---- without delta
        _, y0, st0 = abi_forward(x, a, b)
        ref0 = cases.reference(x, a, b, gy)
        gz0, ga0, gb0 = abi_backward(x, a, gy, st0)
        check_bounds(tag + " plain", ref0, rows, y0, gz0, ga0, gb0)
        assert torch.equal(abi_forward(x, a, b, want_stats=False)[1], y0)
        gz0n, none_a, none_b = abi_backward(x, a, gy, st0, cols=False)             # ga / gb NULL: no scratch
        assert torch.equal(gz0n, gz0) and none_a is None and none_b is None
        # ---- with delta: sum == x + delta, y == the y of a second call on that sum, bit for bit
        z = x + delta
        total, y1, st1 = abi_forward(x, a, b, delta)
        assert torch.equal(total, z)
        _, y1b, st1b = abi_forward(z, a, b)
        assert torch.equal(y1, y1b) and torch.equal(st1, st1b)
        ref1 = cases.reference(z, a, b, gy)
        check_bounds(tag + " delta", ref1, rows, y1)
        # the statistics are the reference's to a few roundings of their own chains
        assert cases.share(st1[:, :1], ref1["mean"], z.double().abs().mean(-1, keepdim=True), cases.T_ROW) <= 1.0
        # ---- backward with gres: fl(gz_without + gres), bit for bit; within the bound on its own account too
        gz1, ga1, gb1 = abi_backward(z, a, gy, st1)
        gz1r, ga1r, gb1r = abi_backward(z, a, gy, st1, gres)
        assert torch.equal(gz1r, gz1 + gres) and torch.equal(ga1r, ga1) and torch.equal(gb1r, gb1)
        check_bounds(tag + " delta", ref1, rows, None, gz1, ga1, gb1)
        check_bounds(tag + " gres", cases.reference(z, a, b, gy, gres), rows, None, gz1r)
        assert torch.equal(abi_backward(z, a, gy, st1, gres, cols=False)[0], gz1r)
        # ---- the wrapper: the same kernels, the same bits
        w = wrapper_run(x, a, b, gy, delta, gres)
        assert torch.equal(w["sum"], z) and torch.equal(w["y"], y1) and torch.equal(w["gz"], gz1r)
        assert torch.equal(w["ga"], ga1) and torch.equal(w["gb"], gb1)
        w0 = wrapper_run(x, a, b, gy)
        assert torch.equal(w0["y"], y0) and torch.equal(w0["gz"], gz0) and torch.equal(w0["ga"], ga0)
        wn = wrapper_run(x, a, b, gy, delta)                                        # the sum's gradient is None
        assert torch.equal(wn["gz"], gz1) and torch.equal(wn["gb"], gb1)


@gpu
@pytest.mark.parametrize("d", [4, 64, 512])
def test_constant_rows(d):
    """All-zero rows and rows of 3.0 (every sum over z exact): y == b exactly, gz = U (gh - mean gh) within the bound, no NaN;
    the random rows between them are untouched by their neighbours."""
    case = cases.make_case(6, d, cases.FAMILIES[0])
    x, a, b, gy = case["x"], case["a"], case["b"], case["gy"]
    x[1], x[3], x[4] = 0.0, 3.0, 0.0
    for delta in (None, torch.zeros_like(x)):
        _, y, stats = abi_forward(x, a, b, delta)
        for r in (1, 3, 4):
            assert torch.equal(y[r], b), r
            assert float(stats[r, 1]) == 0.0 and float(stats[r, 0]) == float(x[r, 0])
        ref = cases.reference(x, a, b, gy)
        gz, ga, gb = abi_backward(x, a, gy, stats)
        check_bounds("constant rows d=%d" % d, ref, 6, y, gz, ga, gb)
        gh = (gy * a).double()
        first = (gh - gh.mean(-1, keepdim=True)) / cases.EPS
        for r in (1, 3, 4):
            assert cases.share(gz[r], first[r], ref["mag_gz"][r], cases.T_ROW) <= 1.0
    w = wrapper_run(x, a, b, gy)
    assert torch.equal(w["y"], y) and torch.equal(w["gz"], gz)


@gpu
@pytest.mark.parametrize("d", [8, 512, 1024])
def test_non_finite_rows(d):
    """A row with a NaN and a row with +Inf are NaN in all their entries of y and gz; every other row keeps its bits; the
    columns of ga / gb are NaN, a contributing row is."""
    case = cases.make_case(9, d, cases.FAMILIES[1])
    x, delta, a, b, gy, gres = (case[k] for k in ("x", "delta", "a", "b", "gy", "gres"))
    a[0] = 0.0                                                      # 0 * NaN: the scale must not hide the row
    _, y_clean, st_clean = abi_forward(x, a, b, delta)
    gz_clean, _, _ = abi_backward(x + delta, a, gy, st_clean, gres)
    bad = x.clone()
    bad[2, d - 1] = float("nan")
    bad[7, 0] = float("inf")
    total, y, stats = abi_forward(bad, a, b, delta)
    gz, ga, gb = abi_backward(total, a, gy, stats, gres)
    keep = [r for r in range(9) if r not in (2, 7)]
    for r in (2, 7):
        assert bool(torch.isnan(y[r]).all()) and bool(torch.isnan(gz[r]).all()), r
    assert torch.equal(y[keep], y_clean[keep]) and torch.equal(gz[keep], gz_clean[keep])
    assert torch.equal(stats[keep], st_clean[keep])
    assert bool(torch.isnan(ga).all())
    assert not bool(torch.isnan(gb).any())                          # gb sums gy alone, and gy is finite
    w = wrapper_run(bad, a, b, gy, delta, gres)
    assert torch.equal(torch.isnan(w["y"]), torch.isnan(y)) and torch.equal(w["y"][keep], y[keep])
    assert torch.equal(torch.isnan(w["gz"]), torch.isnan(gz)) and torch.equal(w["gz"][keep], gz[keep])
    # a NaN in the gradient of one row reaches that row and its columns only
    gyn = gy.clone()
    gyn[5, 3] = float("nan")
    gzn, gan, gbn = abi_backward(x + delta, a, gyn, st_clean, gres)
    others = [r for r in range(9) if r != 5]
    assert bool(torch.isnan(gzn[5]).all()) and torch.equal(gzn[others], gz_clean[others])
    assert bool(torch.isnan(gbn[3])) and int(torch.isnan(gbn).sum()) == 1 and bool(torch.isnan(gan[3]))


@gpu
def test_two_runs_give_the_same_bits():
    for rows, d in ((257, 512), LOOPING, (5, 60)):
        case = cases.make_case(rows, d, cases.FAMILIES[1])
        x, delta, a, b, gy, gres = (case[k] for k in ("x", "delta", "a", "b", "gy", "gres"))
        total, y, stats = abi_forward(x, a, b, delta)
        first = abi_backward(total, a, gy, stats, gres)
        for _ in range(2):
            t2, y2, s2 = abi_forward(x, a, b, delta)
            assert torch.equal(t2, total) and torch.equal(y2, y) and torch.equal(s2, stats)
            assert all(torch.equal(u, v) for u, v in zip(abi_backward(total, a, gy, stats, gres), first))


@gpu
def test_refusals():
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd.registration import ref_layer_norm
    for d in (2, 6, 1028):
        case = cases.make_case(5, d, cases.FAMILIES[0])
        x, a, b, gy = (case[k].to(DEV) for k in ("x", "a", "b", "gy"))
        y, stats, gz = nan_like(5, d), nan_like(5, 2), nan_like(5, d)
        with pytest.raises(_lib.MvpOpsError, match=EBADSHAPE):
            _lib.call("mvp_ref_layernorm", DEV, 5, d, x, None, a, b, cases.EPS, None, y, stats)
        with pytest.raises(_lib.MvpOpsError, match=EBADSHAPE):
            _lib.call("mvp_ref_layernorm_backward", DEV, 5, d, x, a, gy, None, stats, cases.EPS, gz, None, None, None, 0)
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(gz).all())              # nothing ran
        # ... and the wrapper still answers, through the composed route
        xr, ar, br = (t.clone().requires_grad_() for t in (x, a, b))
        out = ref_layer_norm(xr, ar, br, cases.EPS)
        out.backward(gy)
        ref = cases.reference(case["x"], case["a"], case["b"], case["gy"])
        assert cases.share(out, ref["y"], ref["mag_y"], cases.T_ROW) <= 1.0
        assert cases.share(xr.grad, ref["gz"], ref["mag_gz"], cases.T_ROW) <= 1.0
        total, out2 = ref_layer_norm(x, a, b, cases.EPS, gy)
        assert torch.equal(total, x + gy) and torch.equal(out2, cases.compose(x + gy, a, b))
    case = cases.make_case(5, 8, cases.FAMILIES[0])
    x, a, b, gy = (case[k].to(DEV) for k in ("x", "a", "b", "gy"))
    y, stats = nan_like(5, 8), nan_like(5, 2)
    for eps in (-1e-6, float("nan"), float("inf")):
        with pytest.raises(_lib.MvpOpsError, match=EBADARG):
            _lib.call("mvp_ref_layernorm", DEV, 5, 8, x, None, a, b, eps, None, y, stats)
        with pytest.raises(_lib.MvpOpsError, match=EBADARG):
            _lib.call("mvp_ref_layernorm_backward", DEV, 5, 8, x, a, gy, None, stats, eps, y, None, None, None, 0)
    # a pointer off the 16-byte grid: one float into a larger buffer
    big = torch.zeros(5 * 8 + 4, device=DEV)
    off = big[1:41].view(5, 8)
    assert off.data_ptr() % 16 == 4
    for args in ((off, None, a, b, cases.EPS, None, y, stats), (x, off, a, b, cases.EPS, y, y, stats),
                 (x, gy, a, b, cases.EPS, off, y, stats), (x, None, a, b, cases.EPS, None, off, stats)):
        with pytest.raises(_lib.MvpOpsError, match=EBADARG):
            _lib.call("mvp_ref_layernorm", DEV, 5, 8, *args)
    for args in ((off, a, gy, None, stats, cases.EPS, y), (x, a, off, None, stats, cases.EPS, y),
                 (x, a, gy, off, stats, cases.EPS, y), (x, a, gy, None, stats, cases.EPS, off)):
        with pytest.raises(_lib.MvpOpsError, match=EBADARG):
            _lib.call("mvp_ref_layernorm_backward", DEV, 5, 8, *args, None, None, None, 0)
    assert bool(torch.isnan(y).all())
    # ... which the wrapper keeps away from the kernel (the composed route)
    assert torch.equal(ref_layer_norm(off, a, b, cases.EPS), cases.compose(off, a, b))
    # rows == 0 is accepted, by the entry points and by the wrapper
    empty = torch.empty(0, 8, device=DEV)
    _lib.call("mvp_ref_layernorm", DEV, 0, 8, empty, None, a, b, cases.EPS, None, empty, None)
    _lib.call("mvp_ref_layernorm_backward", DEV, 0, 8, empty, a, empty, None, empty, cases.EPS, empty, None, None, None, 0)
    e = empty.clone().requires_grad_()
    ar = a.clone().requires_grad_()
    out = ref_layer_norm(e, ar, b, cases.EPS)
    out.sum().backward()
    assert out.shape == (0, 8) and e.grad.shape == (0, 8) and torch.equal(ar.grad, torch.zeros_like(ar))
    # a non-contiguous input takes the composed formula
    xt = torch.randn(8, 5, device=DEV).t()
    assert torch.equal(ref_layer_norm(xt, a, b, cases.EPS), cases.compose(xt, a, b))


# ---------------------------------------------------------------------------------------------- the module and the model

def _transformer_inputs(dcp, which):
    if which == "golden":                                       # the golden clouds' embeddings, (2, 512, 64) each
        g = np.load(os.path.join(GOLD, "dcp_golden.npz"))
        torch.manual_seed(21)
        emb = dcp.DGCNN().eval()
        with torch.no_grad():
            return tuple(emb(torch.tensor(g[k]).transpose(1, 2).contiguous()) for k in ("src", "tgt"))
    gen = torch.Generator().manual_seed(22)
    return torch.randn(2, 512, 68, generator=gen), torch.randn(2, 512, 68, generator=gen)


@gpu
@pytest.mark.parametrize("which", ["golden", "random68"])
def test_transformer_module_against_its_float64_copy(which):
    """Transformer on the GPU in float32 with the switch on and off against its float64 CPU copy: outputs and parameter
    gradients under one fixed scalar loss.  A tensor's error = max |difference| / max |reference|; a ROUTE's error, one for the
    outputs and one for the gradients, is its worst tensor's.  Only the norms' summation order differs between the routes,
    the GEMMs' rounding is the same on both and dominates: the fused route's error may not exceed twice the composed route's.
    The comparison is per route, not per tensor: both routes carry the same kind of rounding noise in two realisations, and a
    single tensor's ratio scatters (measured on the golden embeddings: 0.6 .. 2.07 over the 47 tensors, 2.07 on
    decoder.layers.0.src_attn.linears.0.bias at errors of 1.9e-6 against 9.2e-7; the routes' worst tensors 2.4e-6 against
    2.0e-6).  The four key projections' biases have no relative error: softmax does not see a shift common to all keys, their
    gradient is 0 in exact arithmetic (1e-16 of their weights' in float64), what float32 leaves there is noise on both
    routes; they are held to 1e-4 of their weight gradient's largest entry instead (noise of u sqrt(rows) size is 1e-6)."""
    from mvp_benchmark_amd.registration import routes
    dcp = load_dcp("layer_norm_gpu")
    torch.manual_seed(23)
    net = dcp.Transformer(types.SimpleNamespace())
    with torch.no_grad():                                       # norms away from a = 1, b = 0
        for name, p in net.named_parameters():
            if name.endswith("a_2"):
                p.add_(0.3 * torch.randn_like(p))
            elif name.endswith("b_2"):
                p.add_(0.3 * torch.randn_like(p))
    src, tgt = _transformer_inputs(dcp, which)
    gen = torch.Generator().manual_seed(24)
    w_src, w_tgt = torch.randn(src.shape, generator=gen).double(), torch.randn(tgt.shape, generator=gen).double()

    def run(model, s, t, ws, wt):
        model.zero_grad(set_to_none=True)
        o_src, o_tgt = model(s, t)
        ((o_src * ws).sum() + (o_tgt * wt).sum()).backward()
        return [o_src, o_tgt], {k: p.grad for k, p in model.named_parameters()}

    net64 = copy.deepcopy(net).double()
    want_out, want_grad = run(net64, src.double(), tgt.double(), w_src, w_tgt)
    netd = copy.deepcopy(net).to(DEV)
    errs = {}
    for on in (True, False):
        with routes(layer_norm=on), abi_call_names() as names:
            outs, grads = run(netd, src.to(DEV), tgt.to(DEV), w_src.float().to(DEV), w_tgt.float().to(DEV))
        # 2 * (3 + 4) norms each way when on, none when off
        assert names.count("mvp_ref_layernorm") == (14 if on else 0), names
        assert names.count("mvp_ref_layernorm_backward") == (14 if on else 0), names
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
        zero = [k for k in want_grad if k.endswith("linears.1.bias")]
        assert len(zero) == 3
        for k in zero:                                          # 0 in exact arithmetic
            scale = float(want_grad[k.replace("bias", "weight")].abs().max())
            assert float(want_grad[k].abs().max()) <= 1e-12 * scale and float(grads[k].abs().max()) <= 1e-4 * scale, k
        errs[on] = {"out%d" % i: rel_err(o, w) for i, (o, w) in enumerate(zip(outs, want_out))}
        errs[on].update({k: rel_err(grads[k], want_grad[k]) for k in want_grad if k not in zero})
    for k in errs[True]:
        print("Transformer %s %-55s fused %.3e composed %.3e" % (which, k, errs[True][k], errs[False][k]))
    route = {on: (max(v for k, v in errs[on].items() if k.startswith("out")),
                  max(v for k, v in errs[on].items() if not k.startswith("out"))) for on in (True, False)}
    print("Transformer %s: outputs fused %.3e composed %.3e; parameter gradients fused %.3e composed %.3e" % (
        which, route[True][0], route[False][0], route[True][1], route[False][1]))
    assert route[True][0] <= 2 * route[False][0] and route[True][1] <= 2 * route[False][1], route


@gpu
def test_dcp_model_on_the_fused_route():
    """Model's forward with the switch on against tests/golden/dcp_golden.npz under the tolerances of the composed route's
    fixture test; then one training-mode forward + backward on the golden clouds: every parameter gradient finite."""
    if GOLD not in sys.path:
        sys.path.insert(0, GOLD)
    from make_dcp_golden import fill_parameters
    from mvp_benchmark_amd.registration import routes
    dcp = load_dcp("layer_norm_gpu")
    g = np.load(os.path.join(GOLD, "dcp_golden.npz"))
    net = dcp.Model(types.SimpleNamespace())
    fill_parameters(net)
    keys = list(net.state_dict())
    net = net.eval().to(DEV)
    src, tgt, T_gt = (torch.tensor(g[k], device=DEV) for k in ("src", "tgt", "T_gt"))
    with routes(layer_norm=True), abi_call_names() as names, torch.no_grad():
        T_12 = net(src, tgt)
        loss, r_err, t_err, rmse, rt_mse = net(src, tgt, T_gt)
    assert names.count("mvp_ref_layernorm") == 28 and "mvp_ref_layernorm_backward" not in names
    np.testing.assert_allclose(T_12.cpu().numpy(), g["T_12"], atol=2e-4)
    np.testing.assert_allclose(loss.cpu().numpy(), g["loss"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(r_err.cpu().numpy(), g["r_err"], rtol=1e-3, atol=2e-2)
    np.testing.assert_allclose(t_err.cpu().numpy(), g["t_err"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(rmse.cpu().numpy(), g["rmse"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(rt_mse.cpu().numpy(), g["rt_mse"], rtol=1e-3, atol=5e-4)
    net.train()
    with routes(layer_norm=True), abi_call_names() as names:
        net(src, tgt, T_gt)[0].mean().backward()
    assert names.count("mvp_ref_layernorm") == 14 and names.count("mvp_ref_layernorm_backward") == 14
    grads = {k: p.grad for k, p in net.named_parameters() if p.requires_grad}
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values()), [k for k, v in grads.items() if v is None or not bool(torch.isfinite(v).all())]
    assert list(net.state_dict()) == keys                       # the module tree is the composed route's
    import mvp_benchmark_amd.registration as R_
    assert R_.LAYER_NORM is False
