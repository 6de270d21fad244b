"""Shared-weight aggregation (csrc/pn2_aggregate.hip) against an independent float64 reference.

    share_weighted_sum   out[b, s*Cw+m, p] = sum_k w[b,m,k,p] * vals[b, s*Cw+m, k, p]
    share_gather_sum     out[b, s*Cw+m, p] = sum_k w[b,m,k,p] * v[b, s*Cw+m, idx[b,k,p]]

The reference below is plain torch on the CPU in float64 (gather / index_add, nothing of the op layer).  Two kinds of
input, two kinds of assertion, no tuned tolerance:

  exact    w, v, grad_out are integers in [-8, 8] stored as float32 and k <= 64: every product and every partial sum
           is an integer far below 2^24, so neither the order of the additions nor an FMA contraction can change a
           bit.  got.double() must EQUAL the float64 reference, for out, grad_w, grad_v and (C ABI) grad_vals.
  random   randn inputs.  |got - ref| <= t * 2^-24 * mag elementwise, mag the same sum over absolute values and t the
           number of terms (out: k; grad_w: share; grad_v[b,c,j]: 1 + the occurrences of j in idx[b]) -- the first-
           order gamma_t bound of a float32 sum of t rounded products, whatever the order, FMA or not.  grad_vals (and
           the plain operator's grad_v) are one rounded product each: bit-equal to (w.double() * g.double()).float().

No assertion masks or samples elements; the only mask is the one the non-finite test is about (finite where the
reference is finite, and there the bound).  Indices always lie in [0, n_src): anything else is outside the contract."""
import contextlib
import os
import sys

import pytest
import torch
from conftest import ROOT

DEV = "cuda:0"
gpu = pytest.mark.gpu
COMPLETION = os.path.join(ROOT, "completion")
U = 2.0 ** -24                      # unit roundoff of float32
LDS_FLOATS = 96 * 1024 // 4         # the fused kernel stages share * n_src floats


# ------------------------------------------------------------------------------------------------- the reference

def ref_share_weighted(w, vals, share, grad_out=None):
    """w (B,Cw,k,N), vals (B,share*Cw,k,N) [, grad_out (B,share*Cw,N)] float32 -> dict of float64 tensors: out, mag
    (the same sum over absolute values) and, with grad_out, grad_w, grad_w_mag, grad_vals."""
    w64, x64 = w.detach().cpu().double(), vals.detach().cpu().double()
    B, Cw, k, N = w64.shape
    C = share * Cw
    assert x64.shape == (B, C, k, N)
    x5 = x64.reshape(B, share, Cw, k, N)                     # channel c = s * Cw + m
    prod = w64.unsqueeze(1) * x5
    r = {"out": prod.sum(3).reshape(B, C, N), "mag": prod.abs().sum(3).reshape(B, C, N)}
    if grad_out is not None:
        g5 = grad_out.detach().cpu().double().reshape(B, share, Cw, 1, N)
        gx = g5 * x5
        r["grad_w"], r["grad_w_mag"] = gx.sum(1), gx.abs().sum(1)
        r["grad_vals"] = (w64.unsqueeze(1) * g5).reshape(B, C, k, N)
    return r


def ref_share_gather(w, v, idx, share, grad_out=None):
    """w (B,Cw,k,N), v (B,share*Cw,n_src), idx (B,k,N) int32 [, grad_out (B,share*Cw,N)] -> the dict of
    ref_share_weighted on the gathered values plus, with grad_out, grad_v (B,C,n_src) = the sum of grad_vals over every
    (k,p) with idx == j, grad_v_mag, and count (B,n_src) = how often idx[b] names j."""
    v64 = v.detach().cpu().double()
    B, C, n_src = v64.shape
    ii = idx.detach().cpu().long()
    k, N = ii.shape[1:]
    assert ii.shape[0] == B and (ii.numel() == 0 or (int(ii.min()) >= 0 and int(ii.max()) < n_src))
    vals = torch.gather(v64, 2, ii.reshape(B, 1, k * N).expand(B, C, k * N)).reshape(B, C, k, N)
    r = ref_share_weighted(w, vals, share, grad_out)
    if grad_out is not None:
        gv, gvm, count = torch.zeros(B, C, n_src, dtype=torch.float64), torch.zeros(B, C, n_src, dtype=torch.float64), \
            torch.zeros(B, n_src, dtype=torch.float64)
        for b in range(B):
            j = ii[b].reshape(-1)
            terms = r["grad_vals"][b].reshape(C, k * N)
            gv[b].index_add_(1, j, terms)
            gvm[b].index_add_(1, j, terms.abs())
            count[b].index_add_(0, j, torch.ones(k * N, dtype=torch.float64))
        r.update(grad_v=gv, grad_v_mag=gvm, count=count)
    return r


def gs_chunk(b, cw, n):
    """Positions per workgroup of the fused kernel (csrc/pn2_aggregate.hip: gs_chunk) -> (chunk, parts, last chunk)."""
    parts = 1
    while b * cw * parts < 512 and n // (parts * 2) >= 256:
        parts *= 2
    chunk = (n + parts - 1) // parts
    grid = (n + chunk - 1) // chunk
    return chunk, grid, n - (grid - 1) * chunk


# ------------------------------------------------------------------------------------------------- inputs, checks

def make_inputs(shape, seed, exact, idx=None, vals=False):
    """shape = (B, share, Cw, k, n_src, N) -> w, v (vals: the un-gathered (B,C,k,N) tensor instead), idx, grad_out."""
    B, share, Cw, k, n_src, N = shape
    g = torch.Generator().manual_seed(seed)
    C = share * Cw
    if exact:
        assert k <= 64
        draw = lambda *s: torch.randint(-8, 9, s, generator=g).float()
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
    w, v, go = draw(B, Cw, k, N), (draw(B, C, k, N) if vals else draw(B, C, n_src)), draw(B, C, N)
    if idx is None and not vals:
        idx = torch.randint(0, n_src, (B, k, N), generator=g, dtype=torch.int32)
    return w, v, idx, go


def assert_exact(got, want, what):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first])))


def assert_bound(got, want, mag, t, what, where=None):
    """|got - want| <= t * 2^-24 * mag on every element (`where`: the non-finite test's finite positions)."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, bound = (got - want).abs(), t * U * mag
    ok = err <= bound                                          # a NaN in got compares false
    if where is not None:
        ok = ok | ~where
        err, bound = err[where], bound[where]
    used = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: largest share of the bound used %.3f" % (what, used))
    if not bool(ok.all()):
        first = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside t * 2^-24 * mag, first at %s: got %r, want %r"
                             % (what, int((~ok).sum()), ok.numel(), first, float(got[first]), float(want[first])))


def rounded_product(w, go, share):
    """(w.double() * g.double()).float(): the correctly rounded float32 product, (B, share*Cw, k, N)."""
    B, Cw, k, N = w.shape
    g5 = go.double().reshape(B, share, Cw, 1, N)
    return (w.double().unsqueeze(1) * g5).reshape(B, share * Cw, k, N).float()


def compare(got, ref, shape, exact, tag, where=None):
    """got: dict of GPU results under the reference's names."""
    B, share, Cw, k, n_src, N = shape
    terms = {"out": ("mag", k), "grad_w": ("grad_w_mag", share)}
    if "grad_v" in got:
        assert got["grad_v"].shape == (B, share * Cw, n_src), (tag, got["grad_v"].shape)
        terms["grad_v"] = ("grad_v_mag", 1 + ref["count"].unsqueeze(1))
    for name in got:
        if exact:
            assert_exact(got[name], ref[name], "%s %s" % (tag, name))
        elif name == "grad_vals":
            assert torch.equal(got[name].cpu(), ref["grad_vals_f32"]), "%s grad_vals is not the rounded product" % tag
        else:
            mag, t = terms[name]
            assert_bound(got[name], ref[name], ref[mag], t, "%s %s" % (tag, name),
                         None if where is None else where[name])
    if "grad_v" in got:                                        # rows nobody names: exactly 0 (part of the above, said aloud)
        unused = (ref["count"] == 0).unsqueeze(1).expand(B, share * Cw, n_src)
        assert bool((got["grad_v"].detach().cpu()[unused] == 0).all()), "%s grad_v of an unreferenced row" % tag


def run_wrapper(w, v, idx, go, w_grad=True, v_grad=True):
    from mvp_benchmark_amd.mm3d_pn2.functional import share_gather_sum
    wd, vd = w.to(DEV).requires_grad_(w_grad), v.to(DEV).requires_grad_(v_grad)
    out = share_gather_sum(wd, vd, idx.to(DEV))
    got = {"out": out.detach()}
    names = [n for n, on in (("grad_w", w_grad), ("grad_v", v_grad)) if on]
    grads = torch.autograd.grad(out, [t for t, on in ((wd, w_grad), (vd, v_grad)) if on], go.to(DEV))
    got.update(zip(names, grads))
    return got


def run_abi(w, v, idx, go, share):
    """The two C entry points on NaN-filled outputs: a position no workgroup writes stays NaN."""
    from mvp_benchmark_amd import _lib
    B, Cw, k, N = w.shape
    C, n_src = v.shape[1:]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    got = {"out": nan(B, C, N), "grad_w": nan(B, Cw, k, N), "grad_vals": nan(B, C, k, N)}
    wd, vd, idd, god = w.to(DEV), v.to(DEV), idx.to(DEV), go.to(DEV)
    _lib.call("mvp_share_gather_sum", DEV, B, share, Cw, k, n_src, N, wd, vd, idd, got["out"])
    _lib.call("mvp_share_gather_sum_grad", DEV, B, share, Cw, k, n_src, N, wd, vd, idd, god, got["grad_w"], got["grad_vals"])
    torch.cuda.synchronize()
    return got


def check_gather(shape, seed, exact, idx=None, routes=("wrapper", "abi")):
    w, v, idx, go = make_inputs(shape, seed, exact, idx)
    ref = ref_share_gather(w, v, idx, shape[1], go)
    ref["grad_vals_f32"] = rounded_product(w, go, shape[1])
    tag = "%s %s" % (shape, "exact" if exact else "randn")
    if "wrapper" in routes:
        compare(run_wrapper(w, v, idx, go), ref, shape, exact, tag + " share_gather_sum")
    if "abi" in routes:
        compare(run_abi(w, v, idx, go, shape[1]), ref, shape, exact, tag + " C ABI")
    return w, v, idx, go, ref


@contextlib.contextmanager
def abi_call_names():
    """Names of the C-ABI entry points the op layer calls inside the block."""
    from mvp_benchmark_amd.mm3d_pn2 import functional
    real, names = functional.call, []

    def spy(name, device, *args):
        names.append(name)
        real(name, device, *args)

    functional.call = spy
    try:
        yield names
    finally:
        functional.call = real


# ------------------------------------------------------------------------------------------------- CPU: the reference

NAIVE_SHAPES = [(2, 8, 3, 20, 300, 513), (2, 4, 2, 5, 513, 77), (1, 16, 1, 3, 1, 130), (3, 1, 5, 7, 33, 40)]


@pytest.mark.parametrize("shape", NAIVE_SHAPES)
@pytest.mark.parametrize("exact", [True, False])
def test_reference_equals_float64_autograd_of_the_naive_formulation(shape, exact):
    """repeat, product, sum over k (vrcnet.py:52-55) on values gathered by advanced indexing, differentiated by autograd
    in float64: equal on integer inputs, within float64 rounding (t + 1 terms at 2^-52) on randn."""
    B, share, Cw, k, n_src, N = shape
    w, v, idx, go = make_inputs(shape, 5, exact)
    ref = ref_share_gather(w, v, idx, share, go)
    w64, v64 = w.double().requires_grad_(), v.double().requires_grad_()
    bi = torch.arange(B).view(B, 1, 1, 1)
    ci = torch.arange(share * Cw).view(1, -1, 1, 1)
    vals = v64[bi, ci, idx.long().unsqueeze(1)]                          # (B, C, k, N)
    vals.retain_grad()
    out = (w64.repeat(1, share, 1, 1) * vals).sum(dim=2)
    out.backward(go.double())
    mag = (w64.abs().repeat(1, share, 1, 1) * vals.abs()).sum(dim=2).detach()
    plain = ref_share_weighted(w, vals.detach().float(), share, go)
    for name, want, m, t in (("out", out.detach(), ref["mag"], k), ("grad_w", w64.grad, ref["grad_w_mag"], share),
                             ("grad_vals", vals.grad, ref["grad_vals"].abs(), 1),
                             ("grad_v", v64.grad, ref["grad_v_mag"], 1 + ref["count"].unsqueeze(1))):
        if exact:
            assert torch.equal(ref[name], want), name
        else:
            assert bool(((ref[name] - want).abs() <= (t + 1) * 2.0 ** -52 * m).all()), name
        if name in plain:                                                # the un-gathered reference: the same numbers
            assert torch.equal(plain[name], ref[name]), name
    assert torch.equal(ref["mag"], mag) if exact else torch.allclose(ref["mag"], mag, rtol=1e-14, atol=0)
    assert torch.equal(ref["count"].sum(1), torch.full((B,), float(k * N), dtype=torch.float64))


def test_reference_ignores_padding_of_the_source_rows():
    """n_src == N against the same v with 37 more source rows nobody names: the same numbers, zero gradient there."""
    shape = (2, 4, 3, 6, 90, 90)
    w, v, idx, go = make_inputs(shape, 8, False)
    pad = torch.cat([v, torch.randn(2, 12, 37, generator=torch.Generator().manual_seed(9))], dim=2)
    a, b = ref_share_gather(w, v, idx, 4, go), ref_share_gather(w, pad, idx, 4, go)
    for name in ("out", "mag", "grad_w", "grad_w_mag", "grad_vals"):
        assert torch.equal(a[name], b[name]), name
    for name in ("grad_v", "grad_v_mag"):
        assert b[name].shape == (2, 12, 127) and torch.equal(a[name], b[name][:, :, :90]), name
        assert bool((b[name][:, :, 90:] == 0).all())
    assert torch.equal(a["count"], b["count"][:, :90]) and bool((b["count"][:, 90:] == 0).all())


def test_exact_inputs_leave_float32_no_rounding():
    """The claim the exact cases rest on: integers in [-8, 8], k <= 64 -- float32 evaluates every sum exactly."""
    shape = (2, 8, 3, 20, 300, 513)
    w, v, idx, go = make_inputs(shape, 1, True)
    ref = ref_share_gather(w, v, idx, 8, go)
    vals = torch.gather(v, 2, idx.long().reshape(2, 1, -1).expand(2, 24, -1)).reshape(2, 24, 20, 513)
    out32 = torch.zeros(2, 24, 513)
    for kk in range(20):                                                 # sequential float32, k ascending
        out32 = out32 + w.repeat(1, 8, 1, 1)[:, :, kk] * vals[:, :, kk]
    assert out32.dtype == torch.float32 and torch.equal(out32.double(), ref["out"])
    for name in ("mag", "grad_w_mag", "grad_v_mag"):
        assert float(ref[name].max()) < 2 ** 24, name
    assert 100 < float(ref["out"].abs().max()) <= 64 * 20


# the issue's table: (B, Cw, N) -> chunk, workgroups along the positions, length of the last chunk
SEAMS = [((1, 1, 5000), (313, 16, 305)), ((2, 2, 1027), (257, 4, 256)), ((1, 3, 513), (257, 2, 256)),
         ((1, 2, 4103), (257, 16, 248)), ((128, 1, 4103), (1026, 4, 1025)), ((4, 128, 1029), (1029, 1, 1029))]


def test_seam_cases_are_the_ragged_ones():
    for (b, cw, n), want in SEAMS:
        assert gs_chunk(b, cw, n) == want, (b, cw, n)


# ------------------------------------------------------------------------------------------------- GPU: n_src != N

# (B, share, Cw, k, n_src, N)
NSRC_CASES = [(2, 8, 3, 20, 300, 513), (2, 4, 2, 5, 513, 77), (1, 16, 1, 3, 1, 130), (1, 2, 7, 1, 64, 1),
              (3, 1, 5, 64, 33, 257)]


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "randn"])
@pytest.mark.parametrize("shape", NSRC_CASES, ids=lambda s: "-".join(map(str, s)))
def test_gather_sum_with_n_src_unequal_n(shape, exact):
    """n_src is the stride of v, of the staged rows and of grad_v; N that of w, idx, grad_out, out, grad_w, grad_vals.
    Both ways round, through the autograd function and through the C ABI.  (n_src = 1: every index is 0.)"""
    check_gather(shape, 100 + shape[5], exact)


# ------------------------------------------------------------------------------------------------- GPU: chunk seams

@gpu
@pytest.mark.parametrize("bcn,share,k,n_src", [
    ((1, 1, 5000), 2, 3, 97),      # chunk 313, 16 parts, last chunk 305 (chunk no multiple of 64)
    ((2, 2, 1027), 2, 2, 300),     # chunk 257, 4 parts, last chunk 256
    ((1, 3, 513), 1, 3, 64),       # chunk 257, 2 parts, last chunk 256
    ((1, 2, 4103), 2, 3, 129),     # chunk 257, 16 parts, last chunk 248
    ((128, 1, 4103), 2, 2, 50),    # chunk 1026, 4 parts, last chunk 1025: lanes 0 and 1 take two positions
    ((4, 128, 1029), 2, 2, 40),    # chunk 1029, 1 part: the whole row in one workgroup, lanes 0 to 4 take two positions
], ids=lambda a: "-".join(map(str, a)) if isinstance(a, tuple) else str(a))
def test_gather_sum_at_the_chunk_seams(bcn, share, k, n_src):
    """Exact inputs, NaN-filled outputs through the C ABI: a position two neighbouring chunks both compute is harmless,
    one that is missed or shifted is not."""
    assert dict(SEAMS)[bcn] == gs_chunk(*bcn)
    B, Cw, N = bcn
    check_gather((B, share, Cw, k, n_src, N), 200 + N, True)


# ------------------------------------------------------------------------------------------------- GPU: the LDS limit

def lds_limit_case(share, n_src, seed):
    shape = (1, share, 2, 4, n_src, 65)
    idx = torch.randint(0, n_src, (1, 4, 65), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    idx[0, 0, 0], idx[0, 1, 0], idx[0, 2, 0], idx[0, 3, 64] = 0, n_src - 1, max(n_src - 2, 0), n_src - 1
    return shape, idx


@gpu
@pytest.mark.parametrize("share", [1, 2, 4, 8, 16])
def test_gather_sum_at_the_lds_limit(share):
    """share * n_src * 4 = 96 KiB exactly: the highest staged rows (n_src - 1, n_src - 2) and row 0 are read."""
    from mvp_benchmark_amd.mm3d_pn2.functional import ShareGatherSum
    n_src = LDS_FLOATS // share
    assert ShareGatherSum.covers(share, n_src) and not ShareGatherSum.covers(share, n_src + 1)
    shape, idx = lds_limit_case(share, n_src, share)
    *_, ref = check_gather(shape, 300 + share, True, idx)
    assert ref["count"][0, 0] >= 1 and ref["count"][0, n_src - 1] >= 2 and ref["count"][0, n_src - 2] >= 1
    check_gather(shape, 310 + share, False, idx, routes=("wrapper",))


@gpu
@pytest.mark.parametrize("share", [1, 2, 4, 8, 16])
def test_one_row_above_the_lds_limit_takes_the_two_step_route(share):
    """aggregate_shared_gathered where the fused kernel does not cover: grouping operator + plain weighted sum, and the
    numbers are still the reference's."""
    sys.path.insert(0, COMPLETION)
    import model_utils as mu
    n_src = LDS_FLOATS // share + 1
    shape, idx_t = lds_limit_case(share, n_src, 20 + share)
    w, v, _, go = make_inputs(shape, 320 + share, True, idx_t)
    ref = ref_share_gather(w, v, idx_t, share, go)
    idx = idx_t.transpose(1, 2).contiguous().long().to(DEV)               # (B, N, k), as the models hold it
    wd, vd = w.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    with abi_call_names() as names:
        out = mu.aggregate_shared_gathered(wd, vd, idx, share)
        gw, gv = torch.autograd.grad(out, (wd, vd), go.to(DEV))
    assert "mvp_share_weighted_sum" in names and "mvp_group_points" in names, names
    assert not any(n.startswith("mvp_share_gather_sum") for n in names), names
    compare({"out": out, "grad_w": gw, "grad_v": gv}, ref, shape, True, "two-step route share %d" % share)


# ------------------------------------------------------------------------------------------------- GPU: index patterns

PATTERN_SHAPE = (2, 8, 2, 16, 200, 300)


def pattern_idx(kind):
    B, share, Cw, k, n_src, N = PATTERN_SHAPE
    g = torch.Generator().manual_seed(40)
    idx = torch.randint(0, n_src, (B, k, N), generator=g, dtype=torch.int32)
    shape = PATTERN_SHAPE
    if kind == "repeated":        # even positions: one neighbour k times (ball-query padding); odd: slots 0, 1 and 5 equal
        idx[:, :, 0::2] = idx[:, :1, 0::2]
        idx[:, 1, 1::2] = idx[:, 0, 1::2]
        idx[:, 5, 1::2] = idx[:, 0, 1::2]
    elif kind == "hub":           # every list holds source row 17 (and the last row, in another slot)
        idx[:, 3, :] = 17
        idx[1, 9, :] = n_src - 1
    elif kind == "identity":      # slot 0 is the point itself (kNN with self), n_src = N
        shape = (B, share, Cw, k, N, N)
        idx = torch.randint(0, N, (B, k, N), generator=g, dtype=torch.int32)
        idx[:, 0, :] = torch.arange(N, dtype=torch.int32)
    elif kind == "upper_half":    # rows 0 .. n_src/2 - 1 are never named
        idx = torch.randint(n_src // 2, n_src, (B, k, N), generator=g, dtype=torch.int32)
    return shape, idx


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "randn"])
@pytest.mark.parametrize("kind", ["repeated", "hub", "identity", "upper_half"])
def test_gather_sum_index_patterns(kind, exact):
    shape, idx = pattern_idx(kind)
    *_, ref = check_gather(shape, 400, exact, idx)
    count = ref["count"]
    if kind == "hub":
        assert float(count[:, 17].min()) >= shape[5]
    if kind == "upper_half":
        assert bool((count[:, :shape[4] // 2] == 0).all()) and float(count.sum()) == 2 * 16 * 300
    if kind == "repeated":
        assert float(count.max()) >= 16


# ------------------------------------------------------------------------------------------------- GPU: non-finite values

def check_nonfinite(w, v, idx, go, shape, expect_out):
    share = shape[1]
    ref = ref_share_gather(w, v, idx, share, go)
    ref["grad_vals_f32"] = rounded_product(w, go, share)
    assert torch.equal(~torch.isfinite(ref["out"]), expect_out)          # the reference marks what the formula says
    for tag, got in (("share_gather_sum", run_wrapper(w, v, idx, go)), ("C ABI", run_abi(w, v, idx, go, share))):
        got.pop("grad_vals", None)                                       # (a rounded product: covered elsewhere)
        where = {}
        for name in got:
            where[name] = torch.isfinite(ref[name])
            assert torch.equal(torch.isfinite(got[name].detach().cpu()), where[name]), \
                "%s %s: non-finite values not where the reference has them" % (tag, name)
        compare(got, ref, shape, False, "non-finite " + tag, where)


@gpu
def test_gather_sum_contains_non_finite_values():
    """A NaN and a +Inf in two source rows reach exactly the outputs of that channel whose list names the row; one Inf
    weight reaches that position's `share` channels.  Everything else meets the bound."""
    shape = (2, 4, 3, 6, 50, 130)
    B, share, Cw, k, n_src, N = shape
    w, v, idx, go = make_inputs(shape, 500, False)
    v2 = v.clone()
    v2[0, 5, 7], v2[1, 2, 31] = float("nan"), float("inf")
    expect = torch.zeros(B, share * Cw, N, dtype=torch.bool)
    expect[0, 5] = (idx[0] == 7).any(0)
    expect[1, 2] = (idx[1] == 31).any(0)
    assert 0 < int(expect[0, 5].sum()) < N and 0 < int(expect[1, 2].sum()) < N
    check_nonfinite(w, v2, idx, go, shape, expect)
    w2 = w.clone()
    w2[1, 2, 3, 100] = float("inf")
    expect = torch.zeros(B, share * Cw, N, dtype=torch.bool)
    expect[1, 2::Cw, 100] = True
    check_nonfinite(w2, v, idx, go, shape, expect)


# ------------------------------------------------------------------------------------------------- GPU: wrapper branches

BRANCH_SHAPE = (2, 4, 3, 5, 90, 150)


@gpu
def test_frozen_values_skip_the_scatter_pass():
    w, v, idx, go = make_inputs(BRANCH_SHAPE, 600, True)
    ref = ref_share_gather(w, v, idx, 4, go)
    from mvp_benchmark_amd.mm3d_pn2.functional import share_gather_sum
    wd, vd = w.to(DEV).requires_grad_(), v.to(DEV)
    with abi_call_names() as names:
        out = share_gather_sum(wd, vd, idx.to(DEV))
        out.backward(go.to(DEV))
    assert names == ["mvp_share_gather_sum", "mvp_share_gather_sum_grad"], names
    assert vd.grad is None
    compare({"out": out, "grad_w": wd.grad}, ref, BRANCH_SHAPE, True, "frozen v")


@gpu
def test_frozen_weights_still_give_the_values_gradient():
    w, v, idx, go = make_inputs(BRANCH_SHAPE, 601, True)
    ref = ref_share_gather(w, v, idx, 4, go)
    compare(run_wrapper(w, v, idx, go, w_grad=False), ref, BRANCH_SHAPE, True, "frozen w")
    w, v, idx, go = make_inputs(BRANCH_SHAPE, 602, False)
    ref = ref_share_gather(w, v, idx, 4, go)
    got = run_wrapper(w, v, idx, go, w_grad=False)
    assert sorted(got) == ["grad_v", "out"]
    compare(got, ref, BRANCH_SHAPE, False, "frozen w")


@gpu
def test_empty_neighbour_lists():
    """k == 0: the output is all zeros, both gradients have their shapes, grad_v is zero."""
    from mvp_benchmark_amd.mm3d_pn2.functional import share_weighted_sum
    B, share, Cw, k, n_src, N = shape = (2, 4, 3, 0, 90, 150)
    w, v, idx, go = make_inputs(shape, 603, False)
    assert w.shape == (B, Cw, 0, N) and idx.shape == (B, 0, N)
    got = run_wrapper(w, v, idx, go)
    assert got["out"].shape == (B, share * Cw, N) and bool((got["out"] == 0).all())
    assert got["grad_w"].shape == (B, Cw, 0, N)
    assert got["grad_v"].shape == (B, share * Cw, n_src) and bool((got["grad_v"] == 0).all())
    wd = w.to(DEV).requires_grad_()
    xd = torch.zeros(B, share * Cw, 0, N, device=DEV, requires_grad=True)
    out = share_weighted_sum(wd, xd)
    gw, gx = torch.autograd.grad(out, (wd, xd), go.to(DEV))
    assert out.shape == (B, share * Cw, N) and bool((out == 0).all())
    assert gw.shape == wd.shape and gx.shape == xd.shape


@gpu
def test_aggregate_shared_gathered_entry_point(monkeypatch):
    """The models' entry point: v (B, C, 1, n_src), idx (B, N, k) int64; k-major lists derived or handed in; the fused
    kernel or (OPS.gather_sum off) the two-step route -- the same bits every way, and the reference's numbers."""
    sys.path.insert(0, COMPLETION)
    import model_utils as mu
    import op_config
    for exact in (True, False):
        w, v, idx_t, go = make_inputs(BRANCH_SHAPE, 610, exact)
        ref = ref_share_gather(w, v, idx_t, 4, go)
        idx = idx_t.transpose(1, 2).contiguous().long().to(DEV)
        given = mu.neighbour_lists_k_major(idx)
        assert given.dtype == torch.int32 and torch.equal(given.cpu(), idx_t)
        results = []
        for fused, lists in ((True, None), (True, given), (False, None), (False, given)):
            monkeypatch.setattr(op_config.OPS, "gather_sum", fused)
            wd, vd = w.to(DEV).requires_grad_(), v.unsqueeze(2).to(DEV).requires_grad_()
            with abi_call_names() as names:
                out = mu.aggregate_shared_gathered(wd, vd, idx, 4, lists)
                gw, gv = torch.autograd.grad(out, (wd, vd), go.to(DEV))
            assert ("mvp_share_gather_sum" in names) == fused and ("mvp_share_weighted_sum" in names) == (not fused), names
            assert gv.shape == vd.shape
            results.append({"out": out.detach(), "grad_w": gw, "grad_v": gv.squeeze(2)})
            compare(results[-1], ref, BRANCH_SHAPE, exact, "aggregate_shared_gathered fused=%s idx_t=%s" % (fused, lists is not None))
        # (grad_v on randn inputs: the scatter adds a row's terms in the order of its inverted list, which every call
        # with freshly derived lists builds anew and which is not fixed -- bits compared where no order can change them)
        for other in results[1:]:
            for name in other:
                if exact or name != "grad_v":
                    assert torch.equal(results[0][name], other[name]), name


@gpu
@pytest.mark.parametrize("shape", [(2, 8, 3, 20, 300, 513), (2, 2, 2, 3, 300, 1027), (1, 2, 2, 3, 129, 4103)],
                         ids=lambda s: "-".join(map(str, s)))
def test_fused_route_is_bit_identical_to_the_two_step_route(shape):
    """The header's claim (same arithmetic, same order) where it is not the easiest: n_src != N, ragged chunks."""
    from mvp_benchmark_amd.mm3d_pn2.functional import grouping_operation, share_gather_sum, share_weighted_sum
    w, v, idx, go = (t.to(DEV) for t in make_inputs(shape, 700, False))
    w.requires_grad_(), v.requires_grad_()
    got = share_gather_sum(w, v, idx)
    two = share_weighted_sum(w, grouping_operation(v, idx))
    assert torch.equal(got, two)
    for a, b in zip(torch.autograd.grad(got, (w, v), go), torch.autograd.grad(two, (w, v), go)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- GPU: the plain operator

# (B, share, Cw, k, N): the six shapes of test_share_weighted_sum_matches_torch, k = 64 at one position, N = 4 * 256 + 1
PLAIN_SHAPES = [(2, 8, 2, 16, 3072), (3, 8, 16, 10, 384), (1, 4, 3, 5, 77), (2, 1, 5, 3, 300), (2, 16, 1, 20, 257),
                (1, 2, 7, 1, 64), (1, 16, 1, 64, 1), (2, 2, 3, 1, 1025)]


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "randn"])
@pytest.mark.parametrize("shape", PLAIN_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_weighted_sum_against_float64(shape, exact):
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd.mm3d_pn2.functional import share_weighted_sum
    B, share, Cw, k, N = shape
    full = (B, share, Cw, k, 0, N)
    w, x, _, go = make_inputs(full, 800 + N, exact, vals=True)
    ref = ref_share_weighted(w, x, share, go)
    product = rounded_product(w, go, share)
    wd, xd = w.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    out = share_weighted_sum(wd, xd)
    gw, gx = torch.autograd.grad(out, (wd, xd), go.to(DEV))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    abi = {"out": nan(B, share * Cw, N), "grad_w": nan(B, Cw, k, N), "grad_vals": nan(B, share * Cw, k, N)}
    _lib.call("mvp_share_weighted_sum", DEV, B, share, Cw, k, N, wd.detach(), xd.detach(), abi["out"])
    _lib.call("mvp_share_weighted_sum_grad", DEV, B, share, Cw, k, N, wd.detach(), xd.detach(), go.to(DEV), abi["grad_w"], abi["grad_vals"])
    for tag, got in (("share_weighted_sum", {"out": out, "grad_w": gw, "grad_vals": gx}), ("C ABI", abi)):
        assert torch.equal(got["grad_vals"].cpu(), product), "%s grad_v is not the rounded product" % tag
        ref["grad_vals_f32"] = product
        compare(got, ref, full, exact, "%s %s" % (shape, tag))
