"""Every route of csrc/pn2_gather.hip's gather / scatter operators against an independent float64 reference.

    forward    out[b,c,p]  = sum_r w[b,p,r] * points[b,c, idx[b,p,r]]           (one index: r = 1, w = 1)
    backward   grad_points[b,c,j] += sum over (p,r) with idx[b,p,r] == j of w[b,p,r] * grad_out[b,c,p]

The reference below is plain torch on the CPU in float64 (gather / index_add_, nothing of the op layer).  Features,
grad_out and pre-filled destinations are integers in [-8, 8] stored as float32, weights integers in [-4, 4] divided by
4: every product is a multiple of 1/4 of magnitude <= 8 and every partial sum stays far below 2^24 quarters, so neither
the order of the additions (global atomics, LDS atomics, the counting sort's fill order) nor an FMA can change a bit.
Every assertion is torch.equal(got.double(), ref): no tolerance, no element masked or sampled.  Indices always lie in
[0, n_src).  The C ABI is called through `_lib.call`, so the ROUTE is chosen by the shape (see `forward_route` /
`backward_route`, the host logic restated) and not by a wrapper; every case runs for the one-index family
(mvp_gather_points*) and the three-index family (mvp_three_interpolate*)."""
import functools

import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu
FAMILIES = ("one", "three")
PATTERNS = ("hub", "permutation", "uniform")
OVERWRITE, INDEX_READY = 1, 2          # include/mvpops.h: MVP_SCATTER_OVERWRITE, MVP_SCATTER_INDEX_READY
LDS_FLOATS = 24576                     # kScFloats: floats of rows one workgroup stages
TR_MAX_DST = 8192                      # kTrMaxDst


# ------------------------------------------------------------------------------------------------- the host logic, restated

def lds_channels(c, n_row):
    """scatter_channels: rows per workgroup of the LDS kernels; 0 = rows too long."""
    return min(LDS_FLOATS // n_row, c, 16)


def forward_route(c, n_src, m_out):
    return "lds" if lds_channels(c, n_src) > 0 and 2 * m_out >= n_src else "direct"


def backward_route(c, n_dst, ws):
    if ws and n_dst <= TR_MAX_DST:
        return "transposed"
    return "lds" if lds_channels(c, n_dst) > 0 else "atomics"


def tr_plan(n_dst):
    """D (destinations per thread), CH (rows per strip), CHUNK (columns per step) of the transposed reduce."""
    return (1, 8, 1536) if n_dst <= 1024 else (2, 8, 1536) if n_dst <= 2048 else (4, 4, 3072) if n_dst <= 4096 else (8, 4, 3072)


# ------------------------------------------------------------------------------------------------- inputs, the reference

def ints(g, bound, *shape):
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


def make_taps(family, pattern, b, count, n_row, g):
    """idx (b, count) / (b, count, 3) int32 and weight (None / (b, count, 3)) naming rows of [0, n_row)."""
    r = 1 if family == "one" else 3
    e = torch.arange(count * r)
    if pattern == "hub":               # three destinations take everything: the first row, a middle one, the last
        flat = torch.tensor([0, n_row // 2, n_row - 1])[e % 3].expand(b, -1)
    elif pattern == "permutation":     # entry e -> perm[e mod n_row]: one entry per destination while they last
        flat = torch.stack([torch.randperm(n_row, generator=g)[e % n_row] for _ in range(b)])
    else:
        flat = torch.randint(0, n_row, (b, count * r), generator=g)
        flat[:, 0], flat[:, -1] = 0, n_row - 1
    idx = flat.to(torch.int32).reshape((b, count) if r == 1 else (b, count, 3)).contiguous()
    assert int(idx.min()) >= 0 and int(idx.max()) < n_row
    return idx, (None if r == 1 else ints(g, 4, b, count, 3) / 4)


def ref_forward(points, idx, weight):
    p64 = points.double()
    b, c, _ = p64.shape
    ii = idx.long().reshape(b, 1, -1).expand(b, c, -1)
    vals = torch.gather(p64, 2, ii)
    if weight is None:
        return vals
    return (vals.reshape(b, c, idx.shape[1], 3) * weight.double().unsqueeze(1)).sum(3)


def ref_backward(grad_out, idx, weight, n_dst):
    """-> (sum (b, c, n_dst) float64, entries per destination (b, n_dst))."""
    g64 = grad_out.double()
    b, c, m = g64.shape
    terms = g64.unsqueeze(3) * (1.0 if weight is None else weight.double().unsqueeze(1))
    terms = terms.reshape(b, c, -1)
    out, count = torch.zeros(b, c, n_dst, dtype=torch.float64), torch.zeros(b, n_dst, dtype=torch.float64)
    for i in range(b):
        j = idx[i].long().reshape(-1)
        out[i].index_add_(1, j, terms[i])
        count[i].index_add_(0, j, torch.ones(j.numel(), dtype=torch.float64))
    return out, count


@functools.lru_cache(maxsize=None)
def backward_case(family, pattern, shape):
    """shape = (b, c, n_dst, m_src) -> inputs on the CPU, the float64 sum and a pre-filled destination."""
    b, c, n_dst, m_src = shape
    g = torch.Generator().manual_seed(1000 + n_dst + m_src + 7 * len(family) + len(pattern))
    idx, weight = make_taps(family, pattern, b, m_src, n_dst, g)
    grad_out, before = ints(g, 8, b, c, m_src), ints(g, 8, b, c, n_dst)
    ref, count = ref_backward(grad_out, idx, weight, n_dst)
    assert float(ref.abs().max()) * 4 < 2 ** 24
    r = 1 if family == "one" else 3
    if pattern == "hub":               # lists far longer than the 1 + 4 the reduce kernel takes per step; per chunk of
        # 1536 / 3072 columns they hold 66, 67, 200, 512, 1024, 1536 or 3072 entries (and 1 in a second chunk): no 1 + 4k
        assert int((count > 0).sum()) == 3 * b and float(count.max()) > 60
    elif pattern == "permutation":
        assert float(count.max()) == -(-m_src * r // n_dst) and (m_src * r != n_dst or float(count.min()) == 1)
    else:
        assert float(count.min()) == 0 or m_src * r > 4 * n_dst
    return grad_out, idx, weight, before, ref


def assert_exact(got, want, what):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first])))


def dev(t):
    return None if t is None else t.to(DEV)


def call_forward(family, points, idx, weight):
    """NaN-filled output: a position no thread writes stays NaN."""
    from mvp_benchmark_amd import _lib
    b, c, n_src = points.shape
    m_out = idx.shape[1]
    out = torch.full((b, c, m_out), float("nan"), device=DEV)
    if family == "one":
        _lib.call("mvp_gather_points", DEV, b, c, n_src, m_out, dev(points), dev(idx), out)
    else:
        _lib.call("mvp_three_interpolate", DEV, b, c, n_src, m_out, dev(points), dev(idx), dev(weight), out)
    return out


def call_backward(family, grad_out, idx, weight, dst, ws=None):
    """ws = (scratch, nbytes, mode): the _grad_ws entry; None: the plain _grad entry.  `dst` is accumulated into / written."""
    from mvp_benchmark_amd import _lib
    b, c, m_src = grad_out.shape
    n_dst = dst.shape[2]
    name = ("mvp_gather_points" if family == "one" else "mvp_three_interpolate") + ("_grad" if ws is None else "_grad_ws")
    dims = (b, c, n_dst, m_src) if family == "one" else (b, c, m_src, n_dst)     # three_interpolate_grad: (b, c, n, m)
    tensors = [grad_out, idx] + ([] if family == "one" else [weight]) + [dst]
    _lib.call(name, DEV, *dims, *tensors, *(() if ws is None else ws))
    return dst


# ------------------------------------------------------------------------------------------------- CPU: the tables name their routes

# (b, c, n_src, m_out)
FORWARD_DIRECT = [(2, 13, 100, 7), (1, 2, 101, 50), (1, 9, 24577, 40)]
FORWARD_LDS = [(2, 17, 64, 70), (1, 3, 33, 1100), (1, 2, 24576, 12288)]
# (b, c, n_dst, m_src)
BACKWARD_ATOMICS = (1, 9, 24577, 300)
BACKWARD_LDS = (2, 21, 50, 300)
BACKWARD_LDS_FROM_WS = (1, 3, 8193, 200)
TRANSPOSED_DST = (1000, 1024, 1025, 2048, 2049, 4096, 4097, 8192)


def transposed_shapes():
    for n_dst in TRANSPOSED_DST:
        _, ch, chunk = tr_plan(n_dst)
        for m_src in (200, chunk + 1):        # one partial chunk; two chunks, the second holding one column
            yield (2, 11 if ch == 8 else 6, n_dst, m_src)      # strips 8 + 3 / 4 + 2


def test_the_cases_take_the_routes_they_are_listed_under():
    for b, c, n, m in FORWARD_DIRECT:
        assert forward_route(c, n, m) == "direct"
    for b, c, n, m in FORWARD_LDS:
        assert forward_route(c, n, m) == "lds"
    assert 2 * 50 == 101 - 1 and 2 * 12288 == 24576                       # one below / exactly at the 2 * m_out >= n_src rule
    assert lds_channels(9, 24577) == 0 and lds_channels(2, 24576) == 1 and lds_channels(17, 64) == 16
    assert backward_route(9, 24577, False) == "atomics" and backward_route(21, 50, False) == "lds"
    assert lds_channels(21, 50) == 16                                      # strips 16 + 5
    assert backward_route(3, 8193, True) == "lds"
    plans = [tr_plan(n)[0] for n in TRANSPOSED_DST]
    assert plans == [1, 1, 2, 2, 4, 4, 8, 8]
    for shape in transposed_shapes():
        assert backward_route(shape[1], shape[2], True) == "transposed"
        assert shape[1] % tr_plan(shape[2])[1] != 0 and shape[1] > tr_plan(shape[2])[1]


def test_reference_equals_float64_autograd_of_advanced_indexing():
    g = torch.Generator().manual_seed(3)
    for family in FAMILIES:
        idx, weight = make_taps(family, "uniform", 2, 40, 17, g)
        points = ints(g, 8, 2, 5, 17).double().requires_grad_()
        grad_out = ints(g, 8, 2, 5, 40)
        bi, ci = torch.arange(2).view(2, 1, 1), torch.arange(5).view(1, 5, 1)
        if family == "one":
            out = points[bi, ci, idx.long().unsqueeze(1)]
        else:
            out = sum(weight.double()[:, :, r].unsqueeze(1) * points[bi, ci, idx.long()[:, :, r].unsqueeze(1)] for r in range(3))
        out.backward(grad_out.double())
        assert torch.equal(ref_forward(points.detach().float(), idx, weight), out.detach())
        assert torch.equal(ref_backward(grad_out, idx, weight, 17)[0], points.grad)


# ------------------------------------------------------------------------------------------------- GPU: forward

@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", FORWARD_DIRECT + FORWARD_LDS, ids=lambda s: "-".join(map(str, s)))
def test_forward_routes(shape, family):
    """direct: a full strip of 8 and a ragged one of 5, 2 * m_out == n_src - 1, rows too long for LDS (strips 8 + 1).
    LDS: ch 16 with a ragged strip of 1, more outputs than threads, ch == 1 at exactly 2 * m_out == n_src."""
    b, c, n_src, m_out = shape
    g = torch.Generator().manual_seed(n_src + m_out)
    idx, weight = make_taps(family, "uniform", b, m_out, n_src, g)
    points = ints(g, 8, b, c, n_src)
    assert_exact(call_forward(family, points, idx, weight), ref_forward(points, idx, weight), "%s forward %s" % (family, shape))


# ------------------------------------------------------------------------------------------------- GPU: backward, plain entries

@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", [BACKWARD_ATOMICS, BACKWARD_LDS], ids=["atomics", "lds"])
def test_backward_plain_entries(shape, pattern, family):
    """Global atomics (rows longer than 24576) and the LDS scatter (strip of 16: the 4-way unrolled loop; strip of 5: one
    unrolled step plus the tail).  Both accumulate onto the destination."""
    grad_out, idx, weight, before, ref = backward_case(family, pattern, shape)
    got = call_backward(family, dev(grad_out), dev(idx), dev(weight), dev(before))
    assert_exact(got, before.double() + ref, "%s %s _grad %s" % (family, pattern, shape))


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_backward_lds_scatter_reached_from_ws(pattern, family):
    """More than 8192 destinations: no scratch size, so _grad_ws runs the plain LDS scatter -- accumulating (mode 0), or
    onto its own zero fill (OVERWRITE, destination pre-filled with 7)."""
    from mvp_benchmark_amd import _lib
    b, c, n_dst, m_src = shape = BACKWARD_LDS_FROM_WS
    assert _lib.scatter_scratch_bytes(b, n_dst, m_src, 1 if family == "one" else 3) == 0
    grad_out, idx, weight, before, ref = backward_case(family, pattern, shape)
    scratch = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    got = call_backward(family, dev(grad_out), dev(idx), dev(weight), dev(before), (scratch, 4096, 0))
    assert_exact(got, before.double() + ref, "%s %s _grad_ws mode 0 %s" % (family, pattern, shape))
    dirty = torch.full((b, c, n_dst), 7.0, device=DEV)
    got = call_backward(family, dev(grad_out), dev(idx), dev(weight), dirty, (scratch, 4096, OVERWRITE))
    assert_exact(got, ref, "%s %s _grad_ws OVERWRITE %s" % (family, pattern, shape))


# ------------------------------------------------------------------------------------------------- GPU: backward, transposed

@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", list(transposed_shapes()), ids=lambda s: "-".join(map(str, s)))
def test_backward_transposed_route(shape, pattern, family):
    """D = 1 / 2 / 4 / 8 destinations per thread on both sides of every threshold, ragged channel strips, one partial
    chunk and two chunks; the four modes of mvpops.h on one scratch."""
    from mvp_benchmark_amd import _lib
    b, c, n_dst, m_src = shape
    nbytes = _lib.scatter_scratch_bytes(b, n_dst, m_src, 1 if family == "one" else 3)
    assert nbytes > 0
    grad_out, idx, weight, before, ref = backward_case(family, pattern, shape)
    go, ii, ww = dev(grad_out), dev(idx), dev(weight)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    tag = "%s %s _grad_ws %s " % (family, pattern, shape)
    dirty = lambda: torch.full((b, c, n_dst), 7.0, device=DEV)
    added = before.double() + ref
    assert_exact(call_backward(family, go, ii, ww, dev(before), (scratch, nbytes, 0)), added, tag + "mode 0")
    assert_exact(call_backward(family, go, ii, ww, dirty(), (scratch, nbytes, OVERWRITE)), ref, tag + "OVERWRITE")
    assert_exact(call_backward(family, go, ii, ww, dev(before), (scratch, nbytes, INDEX_READY)), added, tag + "INDEX_READY")
    assert_exact(call_backward(family, go, ii, ww, dirty(), (scratch, nbytes, OVERWRITE | INDEX_READY)), ref,
                 tag + "OVERWRITE | INDEX_READY")
