"""Fused multi-head attention (csrc/attention.hip, registration.fused_attention, the transformer's opt-in inference route)
against the float64 reference and the bound of tests/attention_cases.py, and on the two families whose result is known
exactly.  Every shape runs through the C ABI on NaN-filled outputs: an element no lane writes stays NaN."""
import copy
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
from conftest import ROOT

import attention_cases as ac
from dcp_util import abi_call_names, load_dcp, rel_err

DEV = "cuda:0"
gpu = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
EBADARG = "MVP_EBADARG"


def run_entry(shape, q, k, v, scale, out=None):
    """mvp_attention_forward on by-head CPU tensors -> the output by head on the CPU; `out`: a packed device tensor to write."""
    from mvp_benchmark_amd import _lib
    B, H, Nq, Nk, D = shape
    qd, kd, vd = (ac.packed(t).to(DEV) for t in (q, k, v))
    if out is None:
        out = torch.full((B, Nq, H * D), float("nan"), device=DEV)
    _lib.call("mvp_attention_forward", DEV, B, H, Nq, Nk, D, qd, kd, vd, scale, out)
    return ac.by_head(out.cpu(), H)


@functools.lru_cache(maxsize=None)
def case(shape, family):
    """(q, k, v, reference, bound) of one shape and random family, made once and left unchanged."""
    q, k, v = ac.inputs(shape, family)
    return (q, k, v) + ac.reference(q, k, v, ac.default_scale(shape))


@gpu
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_entry_point_within_the_bound(shape, family):
    q, k, v, ref, bound = case(shape, family)
    got = run_entry(shape, q, k, v, ac.default_scale(shape))
    share = ac.share(got, ref, bound)
    print("share of bound %s %s: %.4f" % (ac.shape_id(shape), family, share))
    assert share <= 1, share


@gpu
def test_scale_of_ones_own_and_its_sign():
    """The scale is applied to the score, whatever its sign: a negative one turns the order of the keys around."""
    shape = (1, 2, 33, 70, 32)
    q, k, v = ac.inputs(shape, "random")
    for scale in (0.7, -0.4):
        ref, bound = ac.reference(q, k, v, scale)
        assert ac.share(run_entry(shape, q, k, v, scale), ref, bound) <= 1


@gpu
@pytest.mark.parametrize("family", ac.EXACT_FAMILIES)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_exact_families(shape, family):
    """flat within 2 ulp of the mean, one_hot equal to the bit -- where the bound is blind (a dropped key of low weight at
    Nk = 1024 stays under it).  Nk = 70, 200, 96 end in a partial tile."""
    q, k, v, want = ac.exact_inputs(shape, family)
    got = run_entry(shape, q, k, v, ac.default_scale(shape))
    if family == "flat":
        print("flat %s: %.3f ulp" % (ac.shape_id(shape), ac.ulps_off(got, want)))
    ac.assert_exact(got, want, family)


@gpu
def test_same_bits_on_every_run_and_for_a_row_on_its_own():
    """Two runs give the same bits, and the first 5 query rows computed alone have the bits they have in the full call."""
    for shape in ((1, 2, 33, 70, 32), (1, 1, 257, 96, 64), (1, 1, 40, 1024, 128)):
        q, k, v, _, _ = case(shape, "peaked")
        scale = ac.default_scale(shape)
        first = run_entry(shape, q, k, v, scale)
        assert torch.equal(run_entry(shape, q, k, v, scale), first)
        B, H, Nq, Nk, D = shape
        alone = run_entry((B, H, 5, Nk, D), q[:, :, :5].contiguous(), k, v, scale)
        assert torch.equal(alone, first[:, :, :5])


@gpu
def test_nan_contract():
    """A NaN in query row i: output row i of that head NaN, no other row.  A NaN in key j or in value j (its whole row): every
    row of that (cloud, head).  No other (cloud, head) changes by a bit."""
    shape = (2, 4, 64, 64, 128)
    q, k, v, _, _ = case(shape, "random")
    scale = ac.default_scale(shape)
    clean = run_entry(shape, q, k, v, scale)
    assert bool(torch.isfinite(clean).all())
    cloud, head, at = 1, 2, 37
    others = torch.ones(2, 4, dtype=torch.bool)
    others[cloud, head] = False
    for which in ("query", "key", "value"):
        qn, kn, vn = q.clone(), k.clone(), v.clone()
        if which == "query":
            qn[cloud, head, at, 5] = float("nan")
        elif which == "key":
            kn[cloud, head, at, 5] = float("nan")
        else:
            vn[cloud, head, at, :] = float("nan")
        got = run_entry(shape, qn, kn, vn, scale)
        assert torch.equal(got[others], clean[others]), which
        hit = torch.isnan(got[cloud, head])
        if which == "query":
            rows = torch.arange(64) != at
            assert bool(hit[at].all()) and torch.equal(got[cloud, head][rows], clean[cloud, head][rows])
        else:
            assert bool(hit.all()), which
    # one column of a value: that column of every row, and nothing else
    vn = v.clone()
    vn[cloud, head, at, 9] = float("nan")
    got = run_entry(shape, q, k, vn, scale)
    cols = torch.arange(128) != 9
    assert bool(torch.isnan(got[cloud, head][:, 9]).all()) and torch.equal(got[cloud, head][:, cols], clean[cloud, head][:, cols])
    assert torch.equal(got[others], clean[others])


@gpu
def test_bad_arguments_are_refused_and_nothing_is_written():
    from mvp_benchmark_amd import _lib
    B, H, Nq, Nk, D = 1, 2, 8, 12, 32
    gen = torch.Generator().manual_seed(7)
    q = torch.randn(B, Nq, H * D, generator=gen).to(DEV)
    k, v = torch.randn(B, Nk, H * D, generator=gen).to(DEV), torch.randn(B, Nk, H * D, generator=gen).to(DEV)
    out = torch.full((B, Nq, H * D), 77.0, device=DEV)
    big = torch.zeros(B * Nk * H * D + 4, device=DEV)
    off = big[1:1 + B * Nk * H * D].view(B, Nk, H * D)
    off_q = big[1:1 + B * Nq * H * D].view(B, Nq, H * D)
    assert off.data_ptr() % 16 == 4
    refused = [
        (B, H, Nq, 0, D, q, k, v, out),                         # no keys
        (B, H, Nq, Nk, 16, q, k, v, out), (B, H, Nq, Nk, 48, q, k, v, out), (B, H, Nq, Nk, 160, q, k, v, out),   # another d
        (B, 0, Nq, Nk, D, q, k, v, out), (-1, H, Nq, Nk, D, q, k, v, out), (B, H, -1, Nk, D, q, k, v, out),
        (B, H, Nq, -1, D, q, k, v, out),
        (B, H, Nq, Nk, D, None, k, v, out), (B, H, Nq, Nk, D, q, None, v, out), (B, H, Nq, Nk, D, q, k, None, out),
        (B, H, Nq, Nk, D, q, k, v, None),
        (B, H, Nq, Nk, D, off_q, k, v, out), (B, H, Nq, Nk, D, q, off, v, out), (B, H, Nq, Nk, D, q, k, off, out),
        (B, H, Nq, Nk, D, q, k, v, off_q),
        (65536, 64, 1024, Nk, D, q, k, v, out),                 # 2^32 elements of q
    ]
    for args in refused:
        with pytest.raises(_lib.MvpOpsError, match=EBADARG):
            _lib.call("mvp_attention_forward", DEV, *args[:8], 0.5, args[8])
    torch.cuda.synchronize()
    assert bool((out == 77.0).all()) and bool((big == 0).all())
    # empty shapes launch nothing and are accepted, whatever else is passed
    _lib.call("mvp_attention_forward", DEV, 0, H, Nq, Nk, D, None, None, None, 0.5, None)
    _lib.call("mvp_attention_forward", DEV, B, H, 0, Nk, D, q, k, v, 0.5, out)
    _lib.call("mvp_attention_forward", DEV, B, H, 0, 0, D, None, None, None, 0.5, None)
    torch.cuda.synchronize()
    assert bool((out == 77.0).all())


@gpu
def test_operator_routes():
    """The operator: the kernel for what it covers (same bits as the entry point), the composition for a non-contiguous or
    misaligned view, another d, float64 and Nk == 0; empty batches and query sets come back empty."""
    from mvp_benchmark_amd.registration import _attention_reference, fused_attention
    shape = (1, 2, 33, 70, 32)
    B, H, Nq, Nk, D = shape
    q, k, v, ref, bound = case(shape, "random")
    scale = ac.default_scale(shape)
    qd, kd, vd = (ac.packed(t).to(DEV) for t in (q, k, v))
    with abi_call_names() as names:
        got = fused_attention(qd, kd, vd, H)
    assert names == ["mvp_attention_forward"]
    assert torch.equal(ac.by_head(got.cpu(), H), run_entry(shape, q, k, v, scale))
    composed = _attention_reference(qd, kd, vd, H, D ** 0.5)
    assert ac.share(ac.by_head(composed.cpu(), H), ref, bound) <= 1
    # a strided view and a view off the 16-byte grid
    wide = torch.cat((qd, qd), dim=2)[:, :, :H * D]
    big = torch.zeros(kd.numel() + 4, device=DEV)
    big[1:1 + kd.numel()] = kd.reshape(-1)
    off = big[1:1 + kd.numel()].view(kd.shape)
    assert not wide.is_contiguous() and off.data_ptr() % 16 == 4
    with abi_call_names() as names:
        assert torch.equal(fused_attention(wide, kd, vd, H), composed)
        assert torch.equal(fused_attention(qd, off, vd, H), composed)
        assert torch.equal(fused_attention(qd, kd, vd, 4), _attention_reference(qd, kd, vd, 4, 4.0))        # d = 16
        out64 = fused_attention(qd.double(), kd.double(), vd.double(), H)
        none = fused_attention(qd, kd[:, :0], vd[:, :0], H)                                                # softmax over nothing
        assert fused_attention(qd.cpu(), kd.cpu(), vd.cpu(), H).device.type == "cpu"
    assert names == []
    assert out64.dtype == torch.float64 and rel_err(out64, ac.packed(ref)) < 1e-12
    assert none.shape == qd.shape
    with abi_call_names() as names:
        assert fused_attention(qd[:0], kd[:0], vd[:0], H).shape == (0, Nq, H * D)
        assert fused_attention(qd[:, :0], kd, vd, H).shape == (B, 0, H * D)
    assert names == ["mvp_attention_forward"] * 2                  # accepted by the entry point, nothing launched
    with pytest.raises(AssertionError):
        fused_attention(qd.clone().requires_grad_(), kd, vd, H)


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
    """Transformer in eval, float32 on the GPU, on both routes against its float64 CPU copy.  A tensor's error = max |difference|
    / max |reference|; the fused route's may be at most 4 x the composed route's on the same tensor: two realisations of the
    same rounding scatter 0.6 .. 2.07 x on single tensors (profiles/dcp_layer_norm.txt), 4 x is twice that spread.
    Measured (profiles/dcp_attention.txt): see the printed pairs."""
    from mvp_benchmark_amd.registration import routes
    dcp = load_dcp("attention_gpu")
    torch.manual_seed(23)
    net = dcp.Transformer(types.SimpleNamespace()).eval()
    with torch.no_grad():                                       # norms away from a = 1, b = 0
        for name, p in net.named_parameters():
            if name.endswith("a_2") or name.endswith("b_2"):
                p.add_(0.3 * torch.randn_like(p))
    src, tgt = _transformer_inputs(dcp, which)
    with torch.no_grad():
        want = copy.deepcopy(net).double()(src.double(), tgt.double())
        netd = copy.deepcopy(net).to(DEV)
        errs = {}
        for on in (False, True):
            with routes(fused_attention=on), abi_call_names() as names:
                outs = netd(src.to(DEV), tgt.to(DEV))
            assert names.count("mvp_attention_forward") == (6 if on else 0), names
            errs[on] = [rel_err(o, w) for o, w in zip(outs, want)]
    for name, composed, fused in zip(("src_embedding", "tgt_embedding"), errs[False], errs[True]):
        print("transformer %s %s: composed %.3e  fused %.3e  ratio %.2f" % (which, name, composed, fused, fused / composed))
        assert fused <= 4 * composed, (name, composed, fused)


@gpu
def test_dcp_model_with_the_four_switches_on():
    """Model on the golden clouds with every switch on: an eval forward under no_grad reaches mvp_attention_forward six times
    and lands on the fixture's T_12; a training step reaches it never and has finite gradients; the switches are off afterwards."""
    from mvp_benchmark_amd import registration
    if GOLD not in sys.path:
        sys.path.insert(0, GOLD)
    from make_dcp_golden import fill_parameters
    dcp = load_dcp("attention_gpu_model")
    g = np.load(os.path.join(GOLD, "dcp_golden.npz"))
    net = dcp.Model(types.SimpleNamespace())
    fill_parameters(net)
    keys = list(net.state_dict())
    net = net.eval().to(DEV)
    src, tgt, T_gt = (torch.tensor(g[k], device=DEV) for k in ("src", "tgt", "T_gt"))
    everything = dict(edge_mlp=True, layer_norm=True, edge_bn=True, fused_attention=True)
    with registration.routes(**everything), abi_call_names() as names, torch.no_grad():
        T_12 = net(src, tgt)
    assert names.count("mvp_attention_forward") == 6, names
    assert names.count("mvp_edge_mlp_max") == 2 and names.count("mvp_ref_layernorm") == 14, names
    np.testing.assert_allclose(T_12.cpu().numpy(), g["T_12"], atol=2e-4)
    with registration.routes(fused_attention=True), abi_call_names() as names, torch.no_grad():      # the switch on its own
        np.testing.assert_allclose(net(src, tgt).cpu().numpy(), g["T_12"], atol=2e-4)
    assert names.count("mvp_attention_forward") == 6 and "mvp_ref_layernorm" not in names, names
    net.train()
    with registration.routes(**everything), abi_call_names() as names:
        net(src, tgt, T_gt)[0].mean().backward()
    assert names.count("mvp_attention_forward") == 0, names
    assert names.count("mvp_ref_layernorm") == 14 and names.count("mvp_ref_layernorm_backward") == 14, names
    grads = {k: p.grad for k, p in net.named_parameters() if p.requires_grad}
    bad = [k for k, v in grads.items() if v is None or not bool(torch.isfinite(v).all())]
    assert not bad and len(grads) > 60, bad
    assert list(net.state_dict()) == keys
    assert not (registration.EDGE_MLP or registration.LAYER_NORM or registration.EDGE_BN or registration.FUSED_ATTENTION)
