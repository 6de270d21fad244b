"""Host side of the fused LayerNorm (no GPU): the wrapper's composed route on CPU / float64 tensors, the closed-form backward
against autograd, the model switch falling back on the CPU, the entry points' guards through the loaded library, and the
bounds of tests/layer_norm_cases.py checked on the float32 torch composition (met with room) and on wrong variants
(missed by far), so the GPU tests' bound is neither vacuous nor out of reach."""
import copy
import ctypes
import types

import pytest
import torch

import layer_norm_cases as cases
from dcp_util import load_dcp

OK, EBADSHAPE, EBADARG = 0, -1, -2


def _inputs(rows, d, seed=0, dtype=torch.float64, shape=None):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=dtype)
    lead = (rows,) if shape is None else shape
    return r(*lead, d) + 0.5, r(d), r(d), r(*lead, d)


def test_binding_lists_the_entry_points():
    from mvp_benchmark_amd import _lib
    assert _lib.ABI_VERSION >= 23
    assert _lib.SIGNATURES["mvp_ref_layernorm"] == "iippppfppp"
    assert _lib.SIGNATURES["mvp_ref_layernorm_backward"] == "iipppppfppppq"
    assert "mvp_ref_layernorm_backward_scratch_bytes" in _lib.exported_symbols()


def test_switch_defaults_to_off():
    from mvp_benchmark_amd import registration
    assert registration.LAYER_NORM is False


@pytest.mark.parametrize("with_residual", [False, True])
def test_wrapper_on_float64_cpu_equals_the_composed_module(with_residual):
    from mvp_benchmark_amd.registration import ref_layer_norm
    dcp = load_dcp("layer_norm_cpu")
    x, a, b, res = _inputs(5, 60, shape=(2, 5))
    norm = dcp.LayerNorm(60).double()
    with torch.no_grad():
        norm.a_2.copy_(a)
        norm.b_2.copy_(b)
        if with_residual:
            total, y = ref_layer_norm(x, a, b, norm.eps, res)
            assert torch.equal(total, x + res) and torch.equal(y, norm(x + res))
        else:
            assert torch.equal(ref_layer_norm(x, a, b, norm.eps), norm(x))
        # float32 on the CPU and a row length the kernel refuses: the same route
        x32 = x.float()
        assert torch.equal(ref_layer_norm(x32, a.float(), b.float()), cases.compose(x32, a.float(), b.float()))
        x6, a6, b6, _ = _inputs(3, 6)
        assert torch.equal(ref_layer_norm(x6, a6, b6), cases.compose(x6, a6, b6))


@pytest.mark.parametrize("with_residual", [False, True])
def test_gradcheck(with_residual):
    from mvp_benchmark_amd.registration import ref_layer_norm
    x, a, b, res = (t.requires_grad_() for t in _inputs(3, 8, seed=1))
    if with_residual:
        assert torch.autograd.gradcheck(lambda x, a, b, r: ref_layer_norm(x, a, b, 1e-6, r), (x, a, b, res))
    else:
        assert torch.autograd.gradcheck(lambda x, a, b: ref_layer_norm(x, a, b, 1e-6), (x, a, b))


@pytest.mark.parametrize("d", [2, 4, 60, 512])
@pytest.mark.parametrize("with_gres", [False, True])
def test_closed_form_backward_matches_autograd(d, with_gres):
    from mvp_benchmark_amd.registration import ref_layer_norm_backward_reference
    z, a, b, gy = _inputs(7, d, seed=2 + d)
    gres = torch.randn(7, d, dtype=torch.float64, generator=torch.Generator().manual_seed(9)) if with_gres else None
    z.requires_grad_(), a.requires_grad_(), b.requires_grad_()
    y = cases.compose(z, a, b)
    outs, grads = ((y, z), (gy, gres)) if with_gres else ((y,), (gy,))
    want = torch.autograd.grad(outs, (z, a, b), grads)
    got = ref_layer_norm_backward_reference(z.detach(), a.detach(), gy, cases.EPS, gres)
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max()))
    ref = cases.reference(z, a, b, gy, gres)                          # ... and the tests' own reference
    for g, name in zip(got, ("gz", "ga", "gb")):
        assert float((g - ref[name]).abs().max()) <= 1e-12 * max(1.0, float(ref[name].abs().max()))


@pytest.mark.parametrize("d", [4, 64, 512])
def test_closed_form_backward_on_a_constant_row(d):
    """std == 0: autograd's std backward masks it, the second term is 0 and nothing is NaN."""
    from mvp_benchmark_amd.registration import ref_layer_norm_backward_reference
    _, a, b, gy = _inputs(3, d, seed=4)
    z = torch.full((3, d), 3.0, dtype=torch.float64)
    z[1] = 0.0
    z[2] = torch.randn(d, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    z.requires_grad_()
    y = cases.compose(z, a, b)
    assert torch.equal(y[:2], b.expand(2, d))
    (want,) = torch.autograd.grad(y, z, gy)
    gz, _, _ = ref_layer_norm_backward_reference(z.detach(), a, gy, cases.EPS)
    assert bool(torch.isfinite(gz).all()) and float((gz - want).abs().max()) <= 1e-12 * float(want.abs().max())
    gh = gy * a
    first = ((gh - gh.mean(-1, keepdim=True)) / cases.EPS)[:2]                     # U = 1 / eps, the first term alone
    assert float((gz[:2] - first).abs().max()) <= 1e-12 * float(first.abs().max())
    assert float((cases.reference(z, a, b, gy)["gz"] - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_cpu_model_with_the_switch_on_equals_the_switch_off(monkeypatch):
    """The fused route is float32 CUDA only: on the CPU the switch re-orders nothing, outputs and gradients are the same bits."""
    dcp = load_dcp("layer_norm_cpu")
    from mvp_benchmark_amd import registration
    torch.manual_seed(6)
    proto = dcp.Model(types.SimpleNamespace()).train()
    gen = torch.Generator().manual_seed(7)
    src, tgt = torch.rand(2, 32, 3, generator=gen), torch.rand(2, 32, 3, generator=gen)
    runs = {}
    for on in (False, True):
        monkeypatch.setattr(registration, "LAYER_NORM", on)
        net = copy.deepcopy(proto)            # BatchNorm's running statistics move with every training-mode forward
        f_src, f_tgt = net.emb_nn(src.transpose(1, 2)), net.emb_nn(tgt.transpose(1, 2))
        p_src, p_tgt = net.pointer(f_src, f_tgt)
        (p_src.square().mean() + p_tgt.sum()).backward()
        runs[on] = ([p_src.detach(), p_tgt.detach()], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
        with torch.no_grad():
            runs[on][0].append(net.eval()(src, tgt))
            net.train()
    assert all(torch.equal(u, v) for u, v in zip(runs[True][0], runs[False][0]))
    assert runs[True][1].keys() == runs[False][1].keys() and len(runs[True][1]) > 40
    assert all(torch.equal(runs[True][1][k], runs[False][1][k]) for k in runs[True][1])
    # a single layer called on its own adds its last branch itself
    layer = net.pointer.model.decoder.layers[0]
    x, mem = torch.randn(2, 32, 512, generator=gen), torch.randn(2, 32, 512, generator=gen)
    with torch.no_grad():
        on = layer(x, mem)
        monkeypatch.setattr(registration, "LAYER_NORM", False)
        assert torch.equal(on, layer(x, mem))


def test_guards_need_no_gpu():
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    null, dummy, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    eps = ctypes.c_float(1e-6)
    fwd = lambda rows, d, p=null, e=eps, **kw: lib.mvp_ref_layernorm(
        rows, d, kw.get("x", p), kw.get("delta", p), p, p, e, kw.get("sum", p), kw.get("y", p), p, null)
    bwd = lambda rows, d, p=null, e=eps, **kw: lib.mvp_ref_layernorm_backward(
        rows, d, kw.get("z", p), p, kw.get("gy", p), kw.get("gres", p), p, e, kw.get("gz", p), kw.get("ga", p),
        kw.get("gb", p), kw.get("scratch", p), kw.get("nbytes", 0), null)
    for fn in (fwd, bwd):
        for d in (2, 6, 1028, 0, -4, 3):
            assert fn(5, d) == EBADSHAPE and fn(5, d, dummy) == EBADSHAPE and fn(0, d) == EBADSHAPE, d
        assert fn(-1, 512) == EBADSHAPE
        assert fn(2 ** 22, 512) == EBADSHAPE and fn(2 ** 22 - 1, 512) == EBADARG        # rows * d < 2^31
        for d in (4, 8, 60, 512, 1024):
            assert fn(5, d) == EBADARG                                                   # covered: the null buffers
            assert fn(0, d) == OK and fn(0, d, dummy) == OK                              # nothing to do
        for bad in (-1e-6, float("nan"), float("inf")):
            assert fn(5, 512, dummy, ctypes.c_float(bad)) == EBADARG
            assert fn(0, 512, null, ctypes.c_float(bad)) == EBADARG                      # ... before the empty batch
        assert fn(0, 512, null, ctypes.c_float(0.0)) == OK                               # eps = 0 is allowed
    for name in ("x", "delta", "sum", "y"):
        assert fwd(0, 512, dummy, **{name: odd}) == EBADARG, name
    for name in ("z", "gy", "gres", "gz"):
        assert bwd(0, 512, dummy, **{name: odd}) == EBADARG, name
    assert fwd(5, 512, dummy, delta=dummy, sum=null) == EBADARG                          # a delta needs its sum
    # the column sums need their scratch; without ga and gb none is asked for
    need = _lib.ref_layernorm_backward_scratch_bytes(5, 512)
    assert need == 2 * 2 * 512 * 4 and _lib.ref_layernorm_backward_scratch_bytes(8197, 4) == 2048 * 2 * 4 * 4
    assert _lib.ref_layernorm_backward_scratch_bytes(9, 6) == 0 and _lib.ref_layernorm_backward_scratch_bytes(0, 8) == 0
    assert bwd(5, 512, dummy, nbytes=need - 1) == EBADARG and bwd(5, 512, dummy, scratch=null, nbytes=need) == EBADARG


@pytest.mark.parametrize("d", [4, 8, 60, 512])
@pytest.mark.parametrize("family", cases.FAMILIES, ids=str)
def test_float32_composition_meets_the_bound_and_wrong_variants_miss_it(d, family):
    case = cases.make_case(33, d, family)
    z = case["x"] + case["delta"]
    ref = cases.reference(z, case["a"], case["b"], case["gy"])
    got = cases.compose(z, case["a"], case["b"])
    s = cases.share(got, ref["y"], ref["mag_y"], 1)
    zz = z.clone().requires_grad_()
    a, b = case["a"].clone().requires_grad_(), case["b"].clone().requires_grad_()
    gz, ga, gb = torch.autograd.grad(cases.compose(zz, a, b), (zz, a, b), case["gy"])
    sg = cases.share(gz, ref["gz"], ref["mag_gz"], 1)
    print("float32 composition d=%d %s: y %.2f, gz %.2f of u * mag" % (d, family, s, sg))
    assert s <= 2.0 and sg <= 2.0
    assert cases.share(ga, ref["ga"], ref["mag_ga"], cases.t_cols(33)) <= 1.0
    assert cases.share(gb, ref["gb"], ref["mag_gb"], cases.t_cols(33)) <= 1.0


def test_wrong_variants_exceed_the_bound():
    """Each in the family that exposes it (float64 arithmetic, so only the formula differs)."""
    worst = {}
    for family in cases.FAMILIES:
        for d in (8, 60, 512):
            case = cases.make_case(33, d, family)
            z, a, b = (case["x"] + case["delta"]).double(), case["a"].double(), case["b"].double()
            ref = cases.reference(z, a, b, case["gy"])
            c = z - z.mean(-1, keepdim=True)
            variants = {
                "biased std": a * c / (z.std(-1, keepdim=True, unbiased=False) + cases.EPS) + b,
                "eps inside the sqrt": a * c / torch.sqrt(z.var(-1, keepdim=True) + cases.EPS) + b,
                "one-pass variance": a * c / (torch.sqrt((((z.float() ** 2).mean(-1, keepdim=True) - z.float().mean(-1, keepdim=True) ** 2)
                                                          * d / (d - 1)).clamp_min(0)).double() + cases.EPS) + b,
            }
            for name, got in variants.items():
                worst[name] = max(worst.get(name, 0.0), cases.share(got, ref["y"], ref["mag_y"], 1))
    print(worst)
    assert all(v > 10 * cases.T_ROW for v in worst.values()), worst
