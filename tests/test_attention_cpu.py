"""Fused attention without a GPU: the binding, the operator's composed route against the module's formula bit for bit, the
float64 reference and its bound on the float32 composition (and that the bound tells a wrong result from a right one), the two
exact families, registration.routes(fused_attention=), MultiHeadedAttention._route over everything it reads, and the
transformer's bits with the switch off."""
import itertools
import math
import types

import pytest
import torch
import torch.nn.functional as F

import attention_cases as ac
from dcp_util import OpLayerTensor, load_dcp


def test_binding_knows_the_entry_point():
    from mvp_benchmark_amd import _lib
    assert _lib.ABI_VERSION >= 25
    assert "mvp_attention_forward" in _lib.SIGNATURES
    assert _lib.SIGNATURES["mvp_attention_forward"] == "iiiiipppfp"
    assert _lib.load().mvp_abi_version() == _lib.ABI_VERSION


def module_formula(q, k, v, heads):
    """MultiHeadedAttention.forward between its projections, line for line (registration/models/dcp.py)."""
    b, d_k = q.size(0), q.size(2) // heads
    split = lambda t: t.view(b, -1, heads, d_k).transpose(1, 2)
    q, k, v = split(q), split(k), split(v)
    weights = F.softmax(q @ k.transpose(-2, -1) / math.sqrt(d_k), dim=-1)
    return (weights @ v).transpose(1, 2).reshape(b, -1, heads * d_k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("shape", [(2, 4, 64, 64, 128), (1, 2, 33, 70, 32), (2, 3, 7, 9, 20)], ids=ac.shape_id)
def test_operator_on_the_cpu_is_the_module_formula(shape, dtype):
    from mvp_benchmark_amd.registration import fused_attention
    q, k, v = (ac.packed(t).to(dtype) for t in ac.inputs(shape, "random"))
    heads = shape[1]
    want = module_formula(q, k, v, heads)
    assert torch.equal(fused_attention(q, k, v, heads), want)
    assert fused_attention(q, k, v, heads).dtype == dtype and want.shape == q.shape
    # a scale of one's own: the same composition with that divisor
    got = fused_attention(q, k, v, heads, scale=0.25)
    assert torch.equal(ac.by_head(got, heads), ac.composed(*(ac.by_head(t, heads) for t in (q, k, v)), 0.25))
    # a strided view takes the same route
    wide = torch.cat((q, q), dim=2)
    assert torch.equal(fused_attention(wide[:, :, :q.shape[2]], k, v, heads), want)


def test_operator_has_no_backward():
    from mvp_benchmark_amd.registration import fused_attention
    q, k, v = (ac.packed(t) for t in ac.inputs((1, 2, 5, 6, 32), "random"))
    with pytest.raises(AssertionError):
        fused_attention(q.requires_grad_(), k, v, 2)
    with torch.no_grad():
        fused_attention(q, k, v, 2)


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_float32_composition_is_under_the_bound(shape, family):
    """The float32 composition, and a 32-key online softmax in torch float32, against the float64 reference: under the bound
    (they use a few per cent of it: the bound is first order and worst case, the errors add like a random walk)."""
    scale = ac.default_scale(shape)
    q, k, v = ac.inputs(shape, family)
    ref, bound = ac.reference(q, k, v, scale)
    shares = ac.share(ac.composed(q, k, v, scale), ref, bound), ac.share(ac.tiled(q, k, v, scale), ref, bound)
    print("share of bound %s %s: composed %.4f, 32-key online softmax %.4f" % (ac.shape_id(shape), family, *shares))
    assert max(shares) <= 1, shares


def test_the_bound_tells_a_wrong_result():
    """At (2, 4, 64, 64, 128) random: the last key dropped lands at about 2890 x the bound, a scale off by 2^-8 at about 45 x."""
    shape = (2, 4, 64, 64, 128)
    scale = ac.default_scale(shape)
    q, k, v = ac.inputs(shape, "random")
    ref, bound = ac.reference(q, k, v, scale)
    assert ac.share(ac.tiled(q, k, v, scale), ref, bound) <= 1
    dropped = ac.share(ac.tiled(q, k, v, scale, drop_last_key=True), ref, bound)
    rescaled = ac.share(ac.tiled(q, k, v, scale * (1 + 2.0 ** -8)), ref, bound)
    print("share of bound: last key dropped %.0f, scale (1 + 2^-8) %.1f" % (dropped, rescaled))
    assert dropped > 1000 and rescaled > 10
    assert ac.share(ac.composed(q, k[..., :-1, :], v[..., :-1, :], scale), ref, bound) > 1000
    assert ac.share(ac.composed(q, k, v, scale * (1 + 2.0 ** -8)), ref, bound) > 10


@pytest.mark.parametrize("family", ac.EXACT_FAMILIES)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_exact_families(shape, family):
    """The exact results hold on the 32-key online softmax at every shape, and on the composition: one_hot at every shape,
    flat where Nk is a power of two -- the composition multiplies by the ROUNDED weight 1 / Nk before it sums, which is
    exact only there (at Nk = 70 a column whose values cancel comes out as 9e-8 instead of 0); a scheme that sums first and
    divides once, as the kernel does, has no such term."""
    scale = ac.default_scale(shape)
    q, k, v, want = ac.exact_inputs(shape, family)
    ac.assert_exact(ac.tiled(q, k, v, scale), want, family)
    nk = shape[3]
    if family == "one_hot" or nk & (nk - 1) == 0:
        ac.assert_exact(ac.composed(q, k, v, scale), want, family)
    # the packed layout round-trips
    assert torch.equal(ac.by_head(ac.packed(q), shape[1]), q)


def test_routes_sets_the_switch_and_puts_it_back():
    from mvp_benchmark_amd import registration as reg
    state = lambda: (reg.EDGE_MLP, reg.LAYER_NORM, reg.EDGE_BN, reg.FUSED_ATTENTION)
    assert state() == (False, False, False, False)
    with reg.routes(fused_attention=True):
        assert state() == (False, False, False, True)
        with reg.routes(fused_attention=False, layer_norm=True):        # nests; False is a value, None is not
            assert state() == (False, True, False, False)
            with reg.routes(fused_attention=None, edge_mlp=True):
                assert state() == (True, True, False, False)
        assert state() == (False, False, False, True)
    assert state() == (False, False, False, False)
    with pytest.raises(ZeroDivisionError):                              # restores when the block raises
        with reg.routes(edge_mlp=True, layer_norm=True, edge_bn=True, fused_attention=True):
            assert state() == (True, True, True, True)
            1 / 0
    assert all(s is False for s in state())
    with pytest.raises(TypeError):
        reg.routes(attention=True)


def _input(kind, shape, wants_grad):
    if kind == "cpu":
        return torch.zeros(*shape, requires_grad=wants_grad)
    t = OpLayerTensor(*shape, dtype=torch.float32 if kind == "cuda float32" else torch.float64)
    t.requires_grad = wants_grad
    return t


def test_route_table(monkeypatch):
    """Everything _route reads: the switch, grad mode, who requires grad (nothing, either input, the parameters), device and
    dtype, 3-D or not, d_k in and out of the coverage.  "fused" exactly where the switch is on, both inputs are float32 CUDA
    and 3-D, d_k is covered and nothing asks for a gradient."""
    dcp = load_dcp("attention_cpu")
    from mvp_benchmark_amd import registration
    blocks = {128: dcp.MultiHeadedAttention(4, 512), 96: dcp.MultiHeadedAttention(2, 192), 32: dcp.MultiHeadedAttention(2, 64),
              16: dcp.MultiHeadedAttention(4, 64), 160: dcp.MultiHeadedAttention(1, 160)}
    seen = {"fused": 0, "composed": 0}
    for on, grad_mode, wants, kind, d_k, three_d in itertools.product(
            (False, True), (False, True), ("nothing", "query", "memory", "parameters"),
            ("cuda float32", "cpu", "cuda float64"), blocks, (True, False)):
        monkeypatch.setattr(registration, "FUSED_ATTENTION", on)
        block = blocks[d_k]
        width = block.h * block.d_k
        for p in block.parameters():
            p.requires_grad_(wants == "parameters")
        shape = (2, 9, width) if three_d else (9, width)
        query, memory = _input(kind, shape, wants == "query"), _input(kind, (2, 11, width) if three_d else (11, width), wants == "memory")
        with torch.set_grad_enabled(grad_mode):
            got = block._route(query, memory)
        want_fused = (on and kind == "cuda float32" and three_d and d_k in (32, 64, 96, 128)
                      and not (grad_mode and wants != "nothing"))
        assert got == ("fused" if want_fused else "composed"), (on, grad_mode, wants, kind, d_k, three_d, got)
        seen[got] += 1
    assert seen["fused"] == 3 * (4 + 1) and sum(seen.values()) == 2 * 2 * 4 * 3 * 5 * 2, seen
    # one input on the op layer, the other not: composed
    monkeypatch.setattr(registration, "FUSED_ATTENTION", True)
    block = blocks[128]
    with torch.no_grad():
        assert block._route(OpLayerTensor(2, 9, 512), torch.zeros(2, 11, 512)) == "composed"
        assert block._route(OpLayerTensor(2, 9, 512), OpLayerTensor(2, 11, 512, dtype=torch.float64)) == "composed"
        assert block._route(OpLayerTensor(2, 9, 512), OpLayerTensor(2, 11, 512)) == "fused"


# ------------------------------------------------------------------------------------------------ the transformer's bits

def textbook_layer(layer, x, memory=None):
    """The plain pre-norm layer on the module's own submodules, attention written out as the five steps (no module call)."""
    def attention(block, query, mem):
        lin = block.linears
        return lin[3](module_formula(lin[0](query), lin[1](mem), lin[2](mem), block.h))
    h = layer.sublayer[0].norm(x)
    x = x + attention(layer.self_attn, h, h)
    last = 1
    if memory is not None:
        x = x + attention(layer.src_attn, layer.sublayer[1].norm(x), memory)
        last = 2
    return x + layer.feed_forward(layer.sublayer[last].norm(x))


def textbook_transformer(net, src, tgt):
    def stack(s, x, memory=None):
        for layer in s.layers:
            x = textbook_layer(layer, x, memory)
        return s.norm(x)
    src, tgt = src.transpose(2, 1).contiguous(), tgt.transpose(2, 1).contiguous()
    pointer = lambda a, b: stack(net.model.decoder, b, stack(net.model.encoder, a))
    tgt_embedding = pointer(src, tgt).transpose(2, 1).contiguous()
    return pointer(tgt, src).transpose(2, 1).contiguous(), tgt_embedding


def test_transformer_keeps_its_bits():
    """Transformer.forward against the textbook formula with the attention's five steps written out here: the same bits with
    the switch off, and with it on (on the CPU the route is "composed"), outputs and parameter gradients."""
    dcp = load_dcp("attention_cpu")
    from mvp_benchmark_amd import registration
    torch.manual_seed(29)
    net = dcp.Transformer(types.SimpleNamespace())
    gen = torch.Generator().manual_seed(28)
    src, tgt = torch.randn(2, 512, 40, generator=gen), torch.randn(2, 512, 40, generator=gen)

    def run(forward):
        net.zero_grad(set_to_none=True)
        a, b = forward(src, tgt)
        (a.sum() + 2 * b.sum()).backward()
        return (a.detach(), b.detach()), {name: p.grad.clone() for name, p in net.named_parameters()}

    want = run(lambda s, t: textbook_transformer(net, s, t))
    assert len(want[1]) == 46 and sorted(net.state_dict()) == sorted(want[1])     # no parameter or buffer came or went
    for on in (False, True):
        with registration.routes(fused_attention=on):
            outs, grads = run(net)
        assert all(torch.equal(g, w) for g, w in zip(outs, want[0]))
        assert all(torch.equal(grads[name], want[1][name]) for name in want[1])
    assert registration.FUSED_ATTENTION is False
