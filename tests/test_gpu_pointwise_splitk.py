"""mvp_pointwise_mfma_splitk (csrc/pointwise_mfma.hip, ABI 20): the 1x1 convolution's forward / data-gradient GEMM with the
reduction split over workgroups, and the routes of mvp_benchmark_amd/pointwise.py that use it under MFMA_SPLIT_K.

The header's arithmetic contract makes the main check exact: chunk s is what mvp_pointwise_mfma_ex -- the entry point that
already exists -- yields on the K-slice [s k_chunk, ...) of x (xmask) and w with the same prologue and no epilogue; the
output is the ascending float32 sum of the chunks followed by the epilogue steps.  `exact` builds that on the GPU from
contiguous copies of the slices and torch float32 operations; the kernel must give the same bits (NaNs compared as NaNs).
The float64 check holds both to one plain statement of the operation at the bound tools/fuzz_pointwise.py uses for these
inputs (seeded randn): 1e-5 sqrt(K) 4.

Shapes (B, cin, cout, L, k_chunk, w_kmajor): the smallest at which each part can go wrong, see SHAPES."""
import importlib.util
import itertools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SPLITK = "mvp_pointwise_mfma_splitk"
tb = torch.ops.aten.threshold_backward

SHAPES = [
    (1, 32, 8, 4, 16, False),        # two one-slab chunks, one tile mostly empty
    (3, 50, 70, 132, 32, False),     # last chunk of 18: a float4 group straddles K, cin % 4 != 0; M edge of a 128-row tile, N
                                     # edge past one column tile, the cloud stride of the partial buffer
    (2, 40, 64, 64, 16, False),      # chunks of 16 / 16 / 8, a 64-row tile exactly full, the 64-column tile
    (2, 40, 65, 60, 16, False),      # one row into the 128-row tile, a partial 64-column tile
    (1, 512, 32, 8, 16, False),      # 32 chunks, the maximum
    (2, 48, 72, 132, 16, True),      # the data-gradient form (the weight read as W^T), cout % 4 == 0
]
EPILOGUES = [dict(), dict(relu=True), dict(relu_after=True), dict(residual=True), dict(residual=True, relu_after=True),
             dict(residual=True, res_is_mask=True), dict(residual=True, res_is_mask=True, relu_after=True)]
PROLOGUES = ["none", "xmask", "x_relu"]


def tol(k):
    return 1e-5 * math.sqrt(k) * 4


def same(a, b):
    """Bit-level agreement as torch.equal sees it, a NaN matching a NaN."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


_INPUTS = {}


def inputs(shape):
    """Seeded randn operands of a shape, made once and never written: x, xmask, w ((cout, cin), or (cin, cout) with
    w_kmajor), bias (cout), cloud_bias (B, cout), residual."""
    if shape not in _INPUTS:
        b, cin, cout, length, _, kmajor = shape
        g = torch.Generator().manual_seed(1000 + SHAPES.index(shape) if shape in SHAPES else 999)
        r = lambda *s: torch.randn(*s, generator=g).to(DEV)
        _INPUTS[shape] = dict(x=r(b, cin, length), xmask=r(b, cin, length), w=r(cin, cout) if kmajor else r(cout, cin),
                              bias=r(cout), cloud_bias=r(b, cout), residual=r(b, cout, length))
    return _INPUTS[shape]


def chunk_sum(x, w, k_chunk, kmajor, xmask=None, x_relu=False):
    """((p0 + p1) + p2) + ... with p_s = mvp_pointwise_mfma_ex on contiguous copies of the K-slice s, no bias, no epilogue."""
    from mvp_benchmark_amd.pointwise import mfma_linear
    cin = x.size(1)
    acc = None
    for ks in range(0, cin, k_chunk):
        ke = min(ks + k_chunk, cin)
        ws = (w[ks:ke] if kmajor else w[:, ks:ke]).clone().contiguous()
        ms = None if xmask is None else xmask[:, ks:ke].clone().contiguous()
        p = mfma_linear(x[:, ks:ke].clone().contiguous(), ws, w_kmajor=kmajor, xmask=ms, x_relu=x_relu)
        acc = p if acc is None else acc + p
    return acc


def epilogue(acc, bias=None, bias_per_cloud=False, relu=False, residual=None, res_is_mask=False, relu_after=False):
    """The reduce kernel's steps as torch float32 operations."""
    y = acc
    if bias is not None:
        y = y + (bias.view(y.size(0), y.size(1), 1) if bias_per_cloud else bias.view(1, -1, 1))
    if relu:
        y = torch.relu(y)
    if residual is not None:
        y = tb(y, residual, 0) if res_is_mask else y + residual
    if relu_after:
        y = torch.relu(y)
    return y


def splitk_raw(x, w, k_chunk, kmajor=False, xmask=None, bias=None, bias_per_cloud=False, residual=None, flags=0, ldw=0,
               scratch="auto"):
    """The entry point itself: w as it lies (dense rows unless ldw says otherwise), scratch the caller's."""
    from mvp_benchmark_amd import _lib
    b, cin, length = x.shape
    cout = w.size(1) if kmajor else w.size(0)
    nbytes = _lib.pointwise_mfma_splitk_scratch_bytes(b, cin, cout, length, k_chunk)
    if isinstance(scratch, str):
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    y = torch.empty(b, cout, length, device=x.device)
    _lib.call(SPLITK, x.device, b, cin, cout, length, x, xmask, w, ldw, int(kmajor), bias, int(bias_per_cloud), residual,
              flags, y, k_chunk, scratch, nbytes if scratch is not None else 0)
    return y


def float64_fwd(t, kmajor, xmask=None, x_relu=False, bias=None):
    x, w = t["x"].double().cpu(), t["w"].double().cpu()
    if xmask is not None:
        x = tb(x, xmask.double().cpu(), 0)
    if x_relu:
        x = torch.relu(x)
    y = torch.einsum("oc,bcl->bol", w.t() if kmajor else w, x)
    return y if bias is None else y + bias.double().cpu().view(1, -1, 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d_k%d%s" % (s[:5] + ("T" if s[5] else "",)))
def test_chunks_sum_to_the_output_bit_for_bit_and_match_float64(shape):
    from mvp_benchmark_amd.pointwise import mfma_linear
    b, cin, cout, length, k_chunk, kmajor = shape
    t = inputs(shape)
    assert -(-cin // k_chunk) >= 2
    for pro in PROLOGUES:
        kw = dict(xmask=t["xmask"] if pro == "xmask" else None, x_relu=pro == "x_relu")
        acc = chunk_sum(t["x"], t["w"], k_chunk, kmajor, **kw)
        want = epilogue(acc, t["bias"])
        got = mfma_linear(t["x"], t["w"], t["bias"], w_kmajor=kmajor, k_chunk=k_chunk, **kw)
        assert torch.equal(got, want), (shape, pro, (got - want).abs().max().item())
        ref = float64_fwd(t, kmajor, bias=t["bias"], **kw)
        err = (got.double().cpu() - ref).abs().max().item()
        assert err <= tol(cin), (shape, pro, err, tol(cin))
        if not kmajor:
            # through the ABI with the weight's rows dense: cin % 4 != 0 takes the scalar loads along k (mfma_linear pads
            # such rows to a multiple of 4 floats and takes the 16-byte ones)
            raw = splitk_raw(t["x"], t["w"], k_chunk, xmask=kw["xmask"], bias=t["bias"], flags=8 if kw["x_relu"] else 0)
            assert torch.equal(raw, want), (shape, pro, "dense rows")


@pytest.mark.parametrize("pro", PROLOGUES)
def test_every_epilogue_on_every_bias_form(pro):
    from mvp_benchmark_amd.pointwise import mfma_linear
    shape = SHAPES[1]
    b, cin, cout, length, k_chunk, kmajor = shape
    t = inputs(shape)
    kw = dict(xmask=t["xmask"] if pro == "xmask" else None, x_relu=pro == "x_relu")
    acc = chunk_sum(t["x"], t["w"], k_chunk, kmajor, **kw)            # the chunks once; the 21 epilogues from them
    ref64 = float64_fwd(t, kmajor, **kw)
    for (bias, per_cloud), ep in itertools.product(((None, False), (t["bias"], False), (t["cloud_bias"], True)), EPILOGUES):
        ep = dict(ep)
        res = t["residual"] if ep.pop("residual", False) else None
        want = epilogue(acc, bias, per_cloud, residual=res, **ep)
        got = mfma_linear(t["x"], t["w"], bias, residual=res, bias_per_cloud=per_cloud, k_chunk=k_chunk, **kw, **ep)
        assert torch.equal(got, want), (pro, per_cloud, bias is not None, ep)
        ref = epilogue(ref64, None if bias is None else bias.double().cpu(), per_cloud,
                       residual=None if res is None else res.double().cpu(), **ep)
        # (ReLU and the select by the residual are 1-Lipschitz in the value: the GEMM's error passes through, never grows)
        assert (got.double().cpu() - ref).abs().max().item() <= tol(cin), (pro, per_cloud, ep)
    assert not torch.equal(epilogue(acc, t["bias"], relu=True), epilogue(acc, t["bias"]))        # (the flags do something here)


def test_one_chunk_is_the_plain_entry_point():
    from mvp_benchmark_amd.pointwise import mfma_linear
    for shape in (SHAPES[1], SHAPES[5]):
        b, cin, cout, length, _, kmajor = shape
        t = inputs(shape)
        plain = mfma_linear(t["x"], t["w"], t["bias"], relu=True, residual=t["residual"], relu_after=True, xmask=t["xmask"],
                            w_kmajor=kmajor)
        for k_chunk in (-(-cin // 16) * 16, 4096):
            got = mfma_linear(t["x"], t["w"], t["bias"], relu=True, residual=t["residual"], relu_after=True, xmask=t["xmask"],
                              w_kmajor=kmajor, k_chunk=k_chunk)
            assert torch.equal(got, plain)
        if not kmajor:
            w4 = torch.nn.functional.pad(t["w"], (0, -cin % 4)).contiguous()
            raw = splitk_raw(t["x"], w4, 64, xmask=t["xmask"], bias=t["bias"], residual=t["residual"], flags=1 | 2, ldw=w4.size(1),
                             scratch=None)
            assert torch.equal(raw, plain)


def test_scratch_is_written_before_it_is_read_and_nowhere_else():
    from mvp_benchmark_amd import _lib
    for shape in (SHAPES[1], SHAPES[3], SHAPES[5]):
        b, cin, cout, length, k_chunk, kmajor = shape
        t = inputs(shape)
        need = _lib.pointwise_mfma_splitk_scratch_bytes(b, cin, cout, length, k_chunk)
        assert need == -(-cin // k_chunk) * b * cout * length * 4
        slack = 4096
        scratch = torch.full((need + slack,), 0xFF, dtype=torch.uint8, device=DEV)       # every float a NaN
        assert scratch.data_ptr() % 16 == 0
        w = t["w"]
        ldw = 0
        if not kmajor and cin % 4:
            w = torch.nn.functional.pad(w, (0, -cin % 4)).contiguous()
            ldw = w.size(1)
        first = splitk_raw(t["x"], w, k_chunk, kmajor, bias=t["bias"], ldw=ldw, scratch=scratch[:need])
        assert bool(torch.isfinite(first).all()), shape            # every partial element that was read had been written
        assert bool((scratch[need:] == 0xFF).all()), shape         # nothing past the stated size
        assert bool(torch.isfinite(scratch[:need].view(torch.float32)).all()), shape      # and all of it is partial sums
        again = splitk_raw(t["x"], w, k_chunk, kmajor, bias=t["bias"], ldw=ldw, scratch=scratch[:need])
        assert torch.equal(first, again)
        assert torch.equal(first, epilogue(chunk_sum(t["x"], t["w"], k_chunk, kmajor), t["bias"]))


def test_non_finite_values_go_where_the_unsplit_kernel_sends_them():
    """tests/test_gpu_pointwise_nonfinite.py's contract, chunk by chunk: a NaN and a +Inf of x inside ONE chunk's range reach
    exactly the outputs they reach through the unsplit kernel; an Inf under a closed xmask is dropped, a NaN in the mask lets
    the value through; both ReLUs keep a NaN; a NaN in a residual used as a mask lets the value through."""
    from mvp_benchmark_amd.pointwise import mfma_linear
    shape = SHAPES[1]
    b, cin, cout, length, k_chunk, kmajor = shape
    t = inputs(shape)
    nan, inf = float("nan"), float("inf")
    x = t["x"].clone()
    x[1, 35, 7] = nan            # both in the second chunk [32, 50), different columns
    x[2, 40, 129] = inf
    clean = mfma_linear(t["x"], t["w"], t["bias"], k_chunk=k_chunk)
    got = mfma_linear(x, t["w"], t["bias"], k_chunk=k_chunk)
    plain = mfma_linear(x, t["w"], t["bias"])
    assert same(got, epilogue(chunk_sum(x, t["w"], k_chunk, kmajor), t["bias"]))
    assert torch.equal(got.isnan(), plain.isnan()) and torch.equal(got == inf, plain == inf) and torch.equal(got == -inf, plain == -inf)
    hit = torch.zeros_like(got, dtype=torch.bool)
    hit[1, :, 7] = True
    hit[2, :, 129] = True
    assert bool(got[1, :, 7].isnan().all()) and bool(got[2, :, 129].isinf().all()) and bool(torch.isfinite(got[~hit]).all())
    assert torch.equal(got[~hit], clean[~hit])                     # bit for bit everywhere else
    # both ReLUs keep the NaN (and turn the -Inf column entries into 0)
    for ep in (dict(relu=True), dict(relu_after=True), dict(relu=True, residual=t["residual"], relu_after=True)):
        y = mfma_linear(x, t["w"], t["bias"], k_chunk=k_chunk, **ep)
        assert bool(y[1, :, 7].isnan().all()) and int(y.isnan().sum()) == cout
        assert same(y, epilogue(chunk_sum(x, t["w"], k_chunk, kmajor), t["bias"], **ep))
    # an Inf / NaN of x under a closed mask is dropped; a NaN in the mask passes the value
    mask = t["xmask"].clone()
    mask[1, 35, 7] = -1.0
    mask[2, 40, 129] = 0.0
    mask[0, 33, 5] = nan
    open_there = mask.clone()
    open_there[0, 33, 5] = 1.0
    zeroed = x.clone()
    zeroed[1, 35, 7] = 0.0
    zeroed[2, 40, 129] = 0.0
    y = mfma_linear(x, t["w"], t["bias"], xmask=mask, k_chunk=k_chunk)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, mfma_linear(zeroed, t["w"], t["bias"], xmask=open_there, k_chunk=k_chunk))
    assert torch.equal(y, epilogue(chunk_sum(x, t["w"], k_chunk, kmajor, xmask=mask), t["bias"]))
    closed_there = mask.clone()
    closed_there[0, 33, 5] = -1.0
    assert not torch.equal(y, mfma_linear(x, t["w"], t["bias"], xmask=closed_there, k_chunk=k_chunk))    # (the value did pass)
    # the ReLU of x on load keeps the NaN, drops nothing of the +Inf
    y = mfma_linear(x, t["w"], t["bias"], x_relu=True, k_chunk=k_chunk)
    assert bool(y[1, :, 7].isnan().all()) and bool(y[2, :, 129].isinf().all()) and int((~torch.isfinite(y)).sum()) == 2 * cout
    # the residual as a mask: a NaN there passes the value, a closed one drops an Inf
    res = t["residual"].clone()
    res[0, 3, 9] = nan
    res[2, 5, 129] = -1.0
    y = mfma_linear(x, t["w"], t["bias"], residual=res, res_is_mask=True, k_chunk=k_chunk)
    assert y[0, 3, 9].item() == got[0, 3, 9].item() != 0.0 and y[2, 5, 129].item() == 0.0
    assert same(y, epilogue(chunk_sum(x, t["w"], k_chunk, kmajor), t["bias"], residual=res, res_is_mask=True))


UNALIGNED = (2, 515, 40, 68, 128, False)     # a 515-long reduction in chunks of 128: four whole ones and one of 3


@pytest.mark.parametrize("flags,with_residual", [(0, False), (2, True), (4, True)], ids=["plain", "residual_relu_after", "residual_mask"])
def test_unaligned_y_and_residual_take_the_reduce_kernels_scalar_branch(flags, with_residual):
    """y and / or the residual a view one float into its storage (4 bytes past a 16-byte boundary): the reduce kernel loads
    and stores them one float at a time (vec_io = 0).  The bits are those of the aligned call (themselves the chunk sum and
    the torch epilogue), and the float before and the float after the view of y keep what they held."""
    from mvp_benchmark_amd import _lib
    b, cin, cout, length, k_chunk, kmajor = UNALIGNED
    t = inputs(UNALIGNED)
    n = b * cout * length
    nbytes = _lib.pointwise_mfma_splitk_scratch_bytes(b, cin, cout, length, k_chunk)
    assert nbytes == 5 * n * 4
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    guard = 12345.5

    def view_one_float_in(values=None):
        buf = torch.full((n + 2,), guard, device=DEV)
        if values is not None:
            buf[1:n + 1] = values.flatten()
        v = buf[1:n + 1].view(b, cout, length)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return buf, v

    def call(y, residual):
        _lib.call(SPLITK, DEV, b, cin, cout, length, t["x"], None, t["w"], 0, 0, t["bias"], 0, residual, flags, y, k_chunk,
                  scratch, nbytes)

    aligned_res = t["residual"] if with_residual else None
    assert aligned_res is None or aligned_res.data_ptr() % 16 == 0
    want = torch.full((b, cout, length), guard, device=DEV)
    assert want.data_ptr() % 16 == 0
    call(want, aligned_res)
    assert torch.equal(want, epilogue(chunk_sum(t["x"], t["w"], k_chunk, kmajor), t["bias"], residual=aligned_res,
                                      res_is_mask=bool(flags & 4), relu_after=bool(flags & 2)))
    placements = [(True, False)] + ([(False, True), (True, True)] if with_residual else [])
    for y_off, res_off in placements:
        buf, y = view_one_float_in() if y_off else (None, torch.full((b, cout, length), guard, device=DEV))
        res = aligned_res
        if res_off:
            _, res = view_one_float_in(aligned_res)
        call(y, res)
        assert torch.equal(y, want), (y_off, res_off, int((y != want).sum()))
        if y_off:
            assert buf[0].item() == guard and buf[n + 1].item() == guard


# ------------------------------------------------------------------------------------------------ through autograd
_spec = importlib.util.spec_from_file_location("make_pointwise_routes", os.path.join(HERE, "golden", "make_pointwise_routes.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

AUTOGRAD_SHAPES = [(2, 520, 520, 64), (2, 1864, 768, 64)]
AUTOGRAD_ENTRIES = [("conv", {}), ("conv", dict(relu=1)), ("fused", dict(relu_in=1, residual=1, relu_after=1))]


def float64_autograd(c, t, grad_out):
    """The entry point composed of PyTorch operators, float64, on the CPU -> (y, gradients in the order of t's inputs)."""
    fl = c["flags"]
    leaves = {k: v.detach().double().cpu().requires_grad_(v.requires_grad) for k, v in t.items() if v is not None}
    x = torch.relu(leaves["x"]) if fl.get("relu_in") else leaves["x"]
    y = torch.einsum("oc,bcl->bol", leaves["w"].flatten(1), x) + leaves["b"].view(1, -1, 1)
    if fl.get("relu"):
        y = torch.relu(y)
    if fl.get("residual"):
        y = y + leaves["res"]
    if fl.get("relu_after"):
        y = torch.relu(y)
    wanted = [leaves[k] for k, v in t.items() if v is not None and v.requires_grad]
    return y.detach(), torch.autograd.grad(y, wanted, grad_out.double().cpu())


@pytest.mark.parametrize("entry,flags", AUTOGRAD_ENTRIES, ids=["conv", "conv_relu", "fused"])
@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_autograd_through_the_split_routes(shape, entry, flags):
    from mvp_benchmark_amd import pointwise as pw
    b, cin, cout, length = shape
    # LIBRARY_IS_GEMM: no MIOpen solver search; the fused entry point wants the MFMA weight gradient, which 128 positions are
    # too few for by default
    sel = {"LIBRARY_IS_GEMM": True}
    if entry == "fused":
        sel["MFMA_WGRAD_MIN_POSITIONS"] = 0
    c = rec.case("iii", entry, b, cin, cout, (length,), flags=flags, grad="xwb" + ("r" if flags.get("residual") else ""), sel=sel)
    saved = pw.MFMA_SPLIT_K, pw.LIBRARY_IS_GEMM
    try:
        pw.MFMA_SPLIT_K = True
        t = rec.build_inputs(c)
        trace, outs, grads = rec.run_case(c, t)
        assert "error" not in trace, trace
        # forward and data gradient both on the split kernel, no plain MFMA GEMM
        assert trace["calls"].count(SPLITK) == 2 and "mvp_pointwise_mfma_ex" not in trace["calls"], trace
        assert trace["calls"][0] == SPLITK
        assert trace["fn"] == ["_PointwiseConvFusedBackward" if entry == "fused" else "_PointwiseConvBackward"], trace
        if entry == "fused":
            assert "mvp_pointwise_wgrad_mfma_ex" in trace["calls"], trace
        y64, grads64 = float64_autograd(rec.full(c), t, rec.grad_outs(c, outs)[0])
        names = [k for k, v in t.items() if v is not None and v.requires_grad]
        assert names[:3] == ["x", "w", "b"] and len(grads) == len(names)
        assert (outs[0].detach().double().cpu() - y64).abs().max().item() <= tol(cin)
        reduction = {"x": cout, "w": b * length, "b": b * length, "res": 1}
        for name, got, want in zip(names, grads, grads64):
            err = (got.double().cpu() - want.view_as(got)).abs().max().item()
            assert err <= tol(reduction[name]), (name, err, tol(reduction[name]))

        pw.MFMA_SPLIT_K = False
        off, outs_off, _ = rec.run_case(c, t)
        assert SPLITK not in off["calls"], off
        assert (outs_off[0].detach().double().cpu() - y64).abs().max().item() <= tol(cin)
    finally:
        pw.MFMA_SPLIT_K, pw.LIBRARY_IS_GEMM = saved


def test_inference_takes_the_split_route_too():
    from mvp_benchmark_amd import pointwise as pw
    b, cin, cout, length = AUTOGRAD_SHAPES[0]
    c = rec.case("iii", "conv", b, cin, cout, (length,), flags=dict(relu=1), sel={"LIBRARY_IS_GEMM": True})
    saved = pw.MFMA_SPLIT_K
    try:
        pw.MFMA_SPLIT_K = True
        t = rec.build_inputs(c)
        trace, outs, _ = rec.run_case(c, t)
        assert trace["calls"] == [SPLITK] and trace["ops"] == [], trace
        k_chunk = pw._split_k(b, cout, cin, length)
        assert k_chunk > 0
        want = epilogue(chunk_sum(t["x"], t["w"].view(cout, cin), k_chunk, False), t["b"], relu=True)
        assert torch.equal(outs[0], want)
    finally:
        pw.MFMA_SPLIT_K = saved
