"""The 1x1-convolution gradient kernels off the MFMA path -- mvp_pointwise_max_backward (csrc/pointwise_max.hip),
mvp_pointwise_wgrad and mvp_pointwise_dgrad (csrc/pointwise.hip) -- through the C ABI against the float64 references of
tests/conv_gradient_cases.py: EQUAL on the integer family, within gamma_t * mag on randn, element by element.  Every output
buffer is NaN before the call: an element nobody writes stays NaN and fails either check."""
import functools

import pytest
import torch

import conv_gradient_cases as cg

DEV = "cuda:0"
gpu = pytest.mark.gpu
NAN = float("nan")

MAX_SHAPES = [shape for shape, _ in cg.MAX_SHAPES]
STAGED_SHAPES = [shape for shape in MAX_SHAPES if cg.takes_gx(shape)]
DIRECT_ONLY = (2, 5, 4096, 16384)


def nan_tensor(*size):
    return torch.full(size, NAN, device=DEV)


@functools.lru_cache(maxsize=4)
def on_device(shape, pattern, family):
    case = cg.max_case(shape, pattern, family)
    return tuple(t.to(DEV) for t in (case.x, case.w, case.g, case.idx))


def max_backward(shape, pattern, family, want=("gx", "gw", "gb"), staged=True, scratch_fill=NAN):
    """One call of mvp_pointwise_max_backward -> {"gx", "gw", "gb"} on the CPU.  All three buffers exist and start as NaN;
    the entry point gets the ones in `want`, NULL for the others.  staged: with the scratch the entry point asks for
    (filled with `scratch_fill`), else without any."""
    from mvp_benchmark_amd import _lib
    b, cin, cout, length = shape
    x, w, g, idx = on_device(shape, pattern, family)
    out = {"gx": nan_tensor(b, cin, length), "gw": nan_tensor(cout, cin), "gb": nan_tensor(cout)}
    nbytes = _lib.pointwise_max_backward_scratch_bytes(*shape) if staged else 0
    scratch = torch.full((nbytes // 4,), scratch_fill, device=DEV) if nbytes else None
    _lib.call("mvp_pointwise_max_backward", DEV, b, cin, cout, length, x, w, g, idx,
              *(out[k] if k in want else None for k in ("gx", "gw", "gb")), scratch, nbytes)
    return {k: v.cpu() for k, v in out.items()}


def outputs_of(shape):
    return ("gx", "gw", "gb") if cg.takes_gx(shape) else ("gw", "gb")


def same_bits(a, b):
    """Equal as bit patterns (NaN equal to NaN)."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# --------------------------------------------------------------------------------------------- conv -> max over the positions

@gpu
@pytest.mark.parametrize("shape,pattern", cg.max_cases(), ids=cg.max_case_id)
def test_max_backward_equals_the_reference_on_integers(shape, pattern):
    ref = cg.max_case(shape, pattern, "exact").ref
    want = outputs_of(shape)
    got = max_backward(shape, pattern, "exact", want)
    for name in want:
        cg.assert_equal(got[name], ref[name], "%s %s %s" % (name, cg.shape_id(shape), pattern))
    if "gx" in want:
        nobody = (ref["count"] == 0).unsqueeze(1).expand_as(got["gx"])
        assert bool((got["gx"][nobody] == 0).all())
    else:
        assert bool(torch.isnan(got["gx"]).all())


@gpu
@pytest.mark.parametrize("shape,pattern", cg.max_cases(), ids=cg.max_case_id)
def test_max_backward_within_the_bound_on_randn(shape, pattern):
    """t = b for gw (an fmaf chain over the clouds), b - 1 for gb (additions), count[b, l] for gx (an fmaf chain over a
    position's winners: nothing to add where nobody won, the bound is 0 there)."""
    ref = cg.max_case(shape, pattern, "random").ref
    want = outputs_of(shape)
    got = max_backward(shape, pattern, "random", want)
    b = shape[0]
    tag = "%s %s" % (cg.shape_id(shape), pattern)
    cg.assert_within(got["gw"], ref["gw"], ref["gw_mag"], b, "gw " + tag)
    cg.assert_within(got["gb"], ref["gb"], ref["gb_mag"], b - 1, "gb " + tag)
    if "gx" in want:
        cg.assert_within(got["gx"], ref["gx"], ref["gx_mag"], ref["count"].unsqueeze(1), "gx " + tag)


@gpu
def test_gx_is_refused_outside_the_lds_budget_and_nothing_is_written():
    from mvp_benchmark_amd import _lib
    with pytest.raises(_lib.MvpOpsError, match="MVP_EBADSHAPE"):
        max_backward(DIRECT_ONLY, "random", "random", ("gx", "gw", "gb"))
    b, cin, cout, length = DIRECT_ONLY
    x, w, g, idx = on_device(DIRECT_ONLY, "random", "random")
    gx, gw, gb = nan_tensor(b, cin, length), nan_tensor(cout, cin), nan_tensor(cout)
    with pytest.raises(_lib.MvpOpsError, match="MVP_EBADSHAPE"):
        _lib.call("mvp_pointwise_max_backward", DEV, b, cin, cout, length, x, w, g, idx, gx, gw, gb, None, 0)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (gx, gw, gb))
    assert _lib.pointwise_max_backward_scratch_bytes(*DIRECT_ONLY) == 0


@gpu
@pytest.mark.parametrize("family", cg.FAMILIES)
@pytest.mark.parametrize("shape", STAGED_SHAPES, ids=cg.shape_id)
def test_both_weight_gradient_routes_give_the_same_bits(shape, family):
    """Staged columns (with scratch) and the direct gather (scratch = NULL): both are fmaf chains over the clouds in ascending
    order.  The direct route is held to the reference as well -- nothing else in the suite runs it at these shapes."""
    from mvp_benchmark_amd import _lib
    assert _lib.pointwise_max_backward_scratch_bytes(*shape) > 0
    for pattern in ("random", cg.patterns_for(shape)[-1]):
        staged = max_backward(shape, pattern, family, ("gw", "gb"), staged=True)
        direct = max_backward(shape, pattern, family, ("gw", "gb"), staged=False)
        assert torch.equal(staged["gw"], direct["gw"]) and torch.equal(staged["gb"], direct["gb"]), pattern
        ref = cg.max_case(shape, pattern, family).ref
        if family == "exact":
            cg.assert_equal(direct["gw"], ref["gw"], "direct gw")
            cg.assert_equal(direct["gb"], ref["gb"], "direct gb")
        else:
            cg.assert_within(direct["gw"], ref["gw"], ref["gw_mag"], shape[0], "direct gw %s %s" % (cg.shape_id(shape), pattern))
            cg.assert_within(direct["gb"], ref["gb"], ref["gb_mag"], shape[0] - 1, "direct gb")
    # a scratch one byte short is no scratch: the direct route, the same bits
    b, cin, cout, length = shape
    x, w, g, idx = on_device(shape, "random", family)
    nbytes = _lib.pointwise_max_backward_scratch_bytes(*shape)
    gw, scratch = nan_tensor(cout, cin), torch.full((nbytes // 4,), 7.0, device=DEV)
    _lib.call("mvp_pointwise_max_backward", DEV, b, cin, cout, length, x, w, g, idx, None, gw, None, scratch, nbytes - 1)
    assert torch.equal(gw.cpu(), max_backward(shape, "random", family, ("gw",), staged=False)["gw"])
    assert bool((scratch == 7.0).all())


@gpu
@pytest.mark.parametrize("want", [("gx",), ("gw",), ("gb",), ("gw", "gb")], ids="+".join)
def test_each_output_on_its_own(want):
    """gx, gw and gb may each be NULL (include/mvpops.h): what is asked for has the bits it has in the call for all three,
    with and without scratch, and a buffer that is not asked for is not touched."""
    for shape in ((3, 5, 2, 33), (11, 65, 33, 20), (9, 300, 200, 257)):
        for staged in (True, False):
            full = max_backward(shape, "random", "random", staged=staged)
            assert not any(bool(torch.isnan(t).any()) for t in full.values())
            got = max_backward(shape, "random", "random", want, staged=staged)
            for name in ("gx", "gw", "gb"):
                if name in want:
                    assert torch.equal(got[name], full[name]), (shape, staged, name)
                else:
                    assert bool(torch.isnan(got[name]).all()), (shape, staged, name)
    # the shape without a data gradient
    if "gx" not in want:
        full = max_backward(DIRECT_ONLY, "random", "random", ("gw", "gb"))
        got = max_backward(DIRECT_ONLY, "random", "random", want)
        for name in ("gw", "gb"):
            assert torch.equal(got[name], full[name]) if name in want else bool(torch.isnan(got[name]).all()), name


@gpu
def test_max_backward_same_bits_on_every_run_whatever_the_scratch_holds():
    for shape, pattern in (((11, 65, 33, 20), "runs_9_17"), ((9, 300, 200, 257), "random"), ((2, 7, 2049, 1353), "tile_edges")):
        first = max_backward(shape, pattern, "random")
        again = max_backward(shape, pattern, "random")
        zeros = max_backward(shape, pattern, "random", scratch_fill=0.0)
        for name in ("gx", "gw", "gb"):
            assert same_bits(first[name], again[name]) and same_bits(first[name], zeros[name]), (shape, name)
            assert not bool(torch.isnan(first[name]).any())


@gpu
@pytest.mark.parametrize("length", [200, 201], ids=["fused_forward", "library_forward"])
def test_through_the_wrapper_the_forward_positions_reach_the_backward(length):
    """PointwiseConv1d.max_over_positions on integers, x built so that channel co wins at a chosen position: column p_k of x
    is 64 e_k (+ small entries in the rows behind the targets), channel co has weight 4 on its target's row and <= 0 on the
    other targets' rows, so y[co] is >= 256 - 32 there and <= 32 everywhere else.  Every target column stands a second time
    at a later position: the maximum is attained twice and the first occurrence must win (what torch.max reports).  The
    gradients EQUAL the reference at the chosen positions -- a forward that reported the second occurrence would put gx
    there."""
    from mvp_benchmark_amd.pointwise import PointwiseConv1d
    b, cin, cout = 3, 12, 40
    targets = (0, 31, 32, 64, length - 9)
    copies = (5, 33, 150, 65, length - 1)                      # each after its target
    gen = torch.Generator().manual_seed(8)
    x = torch.randint(-1, 2, (b, cin, length), generator=gen).float()
    x[:, :len(targets)] = 0
    for k, (p, q) in enumerate(zip(targets, copies)):
        x[:, :, p] = torch.randint(-1, 2, (b, cin), generator=gen).float()
        x[:, :len(targets), p] = 0
        x[:, k, p] = 64
        x[:, :, q] = x[:, :, p]
    weight = torch.randint(-4, 5, (cout, cin), generator=gen).float()
    owner = torch.randint(0, len(targets), (cout,), generator=gen)
    weight[:, :len(targets)] = -weight[:, :len(targets)].abs()
    weight[torch.arange(cout), owner] = 4
    bias = torch.randint(-4, 5, (cout,), generator=gen).float()
    g = torch.randint(-4, 5, (b, cout), generator=gen).float()
    idx = torch.tensor(targets)[owner].expand(b, cout).int().contiguous()
    y = torch.einsum("oi,bil->bol", weight.double(), x.double()) + bias.double()[None, :, None]
    value = y.max(2)[0]
    attained = torch.where(y == value.unsqueeze(2), torch.arange(length), length)
    second = torch.tensor(copies)[owner].expand(b, cout)
    assert torch.equal(attained.min(2)[0].int(), idx) and bool((attained.gather(2, second.unsqueeze(2)).squeeze(2) == second).all())
    ref = cg.ref_max_backward(x, weight, g, idx)
    cg.assert_exactly_representable(ref)

    layer = PointwiseConv1d(cin, cout).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(weight.unsqueeze(2))
        layer.bias.copy_(bias)
    xd = x.to(DEV).requires_grad_()
    got = layer.max_over_positions(xd)
    assert torch.equal(got.cpu().double(), value)
    gx, gw, gb = torch.autograd.grad(got, (xd, layer.weight, layer.bias), g.to(DEV))
    cg.assert_equal(gx.cpu(), ref["gx"], "gx through the wrapper")
    cg.assert_equal(gw.cpu().squeeze(2), ref["gw"], "gw through the wrapper")
    cg.assert_equal(gb.cpu(), ref["gb"], "gb through the wrapper")
    # the bias alone: no weight gradient is computed for it
    layer.weight.requires_grad_(False)
    gb_alone, = torch.autograd.grad(layer.max_over_positions(x.to(DEV)), (layer.bias,), g.to(DEV))
    assert torch.equal(gb_alone, gb)


# -------------------------------------------------------------------------------------------- few channels: weight gradient

def small_wgrad(shape, family, with_bias=True):
    from mvp_benchmark_amd import _lib
    b, cin, cout, length = shape
    case = cg.wgrad_case(shape, family)
    gw, gb = nan_tensor(cout, cin), nan_tensor(cout)
    nbytes = _lib.pointwise_wgrad_scratch_bytes(*shape)
    assert nbytes > 0
    scratch = torch.full((nbytes // 4,), NAN, device=DEV)
    _lib.call("mvp_pointwise_wgrad", DEV, b, cin, cout, length, case.x.to(DEV), case.gy.to(DEV), gw, gb if with_bias else None,
              scratch, nbytes)
    return gw.cpu(), gb.cpu()


@gpu
@pytest.mark.parametrize("family", cg.FAMILIES)
@pytest.mark.parametrize("shape", [s for s, _, _ in cg.WGRAD_SHAPES], ids=cg.shape_id)
def test_small_weight_gradient(shape, family):
    """t = b len products for gw, b len - 1 additions for gb; without gb, gw keeps its bits and gb stays untouched."""
    ref = cg.wgrad_case(shape, family).ref
    gw, gb = small_wgrad(shape, family)
    terms = shape[0] * shape[3]
    if family == "exact":
        cg.assert_equal(gw, ref["gw"], "gw " + cg.shape_id(shape))
        cg.assert_equal(gb, ref["gb"], "gb " + cg.shape_id(shape))
    else:
        cg.assert_within(gw, ref["gw"], ref["gw_mag"], terms, "gw " + cg.shape_id(shape))
        cg.assert_within(gb, ref["gb"], ref["gb_mag"], terms - 1, "gb " + cg.shape_id(shape))
    gw_alone, gb_untouched = small_wgrad(shape, family, with_bias=False)
    assert torch.equal(gw_alone, gw) and bool(torch.isnan(gb_untouched).all())


# ---------------------------------------------------------------------------------------------- few channels: data gradient

@gpu
@pytest.mark.parametrize("family", cg.FAMILIES)
@pytest.mark.parametrize("shape", cg.DGRAD_SHAPES, ids=cg.shape_id)
def test_small_data_gradient(shape, family):
    """t = cout: an fmaf chain over the output channels."""
    from mvp_benchmark_amd import _lib
    b, cin, cout, length = shape
    case = cg.dgrad_case(shape, family)
    gx = nan_tensor(b, cin, length)
    _lib.call("mvp_pointwise_dgrad", DEV, b, cin, cout, length, case.w.to(DEV), case.gy.to(DEV), gx)
    if family == "exact":
        cg.assert_equal(gx.cpu(), case.ref["gx"], "gx " + cg.shape_id(shape))
    else:
        cg.assert_within(gx.cpu(), case.ref["gx"], case.ref["gx_mag"], cout, "gx " + cg.shape_id(shape))
