"""Non-finite contract and tile edges of the pointwise MFMA kernels (csrc/pointwise_mfma.hip, pointwise.py,
mvp_pointwise_mfma* / mvp_pointwise_wgrad_mfma*).

The contract is what the float32 PyTorch formulation of each operation yields: torch.relu keeps a NaN, torch.max
propagates it (and reports the first one), ReLU' is aten.threshold_backward's select (0 where the mask is <= 0, the
gradient elsewhere -- also where the mask is NaN).  Every check compares the kernel with ONE plain float64 statement of the
operation, run on the CPU from the same float32 inputs and composed of einsum, torch.relu, +, torch.max(dim) and
aten.threshold_backward:
  (a) the output's isnan mask and its +Inf / -Inf masks equal the reference's exactly;
  (b) on the elements the float64 reference itself leaves finite, the error is inside the summation-order bound the
      plain tests of the entry point use (tests/test_gpu_harness.py): 4e-6 sqrt(K) 4 forward / data gradient,
      3e-6 sqrt(B L) 4 weight gradient.
The inputs are randn with exact NaNs (both sign bits), +Inf and -Inf injected so that the reference's pattern does not
depend on the summation order: an Inf meets finite non-zero partners only, a sum holds two infinities only where NaN is
the intended answer (mixed-sign weight rows; row 0 of every weight has one sign, there the Inf stays an Inf).

A non-finite value is also the one input that shows "0 x whatever lies past the tile": a finite neighbour contributes
exactly 0 through a zero-padded operand, an Inf or NaN does not.  The isolation tests poison ONE element at every tile
edge and demand bit equality with the clean call everywhere else.

Shapes: B = 3 clouds (slab runs and the work-item mapping cross cloud boundaries); forward / data-gradient tiles are 64
(cout <= 64) or 128 rows x 128 positions x 16 of K, weight-gradient tiles 64 or 128 on both channel axes x slabs of 32
positions numbered across the clouds, at least 4 slabs per split -- the shapes below are the smallest that reach every
edge.  test_reference_patterns_are_order_free_and_not_vacuous (CPU) walks the same case table as the GPU tests."""
import itertools
import math

import pytest
import torch

DEV = "cuda:0"
B = 3
SHAPES = [(5, 33, 4), (40, 33, 132), (68, 130, 260), (16, 64, 128), (129, 128, 388)]      # (cin, cout, L)
WGRAD_SHAPES = SHAPES + [(64, 65, 36)]
# with the weight layout: (cout, cin) always; (cin, cout) read as W^T -- the data gradient, whose output rows are the
# layer's cin -- where the kernel takes it (16-byte loads along the rows: cin % 4 == 0)
FWD_PARAMS = [(cin, cout, length, kmajor) for cin, cout, length in SHAPES for kmajor in ((False, True) if cin % 4 == 0 else (False,))]
BITS = {"nan": 0x7FC00000, "-nan": 0xFFC00000 - (1 << 32), "inf": 0x7F800000, "-inf": 0xFF800000 - (1 << 32)}
VALUES = ("nan", "-nan", "inf", "-inf")
tb = torch.ops.aten.threshold_backward


def fwd_tol(k):
    return 4e-6 * math.sqrt(k) * 4


def wgrad_tol(positions):
    return 3e-6 * math.sqrt(positions) * 4


def poison(t, site, value):
    """A copy of t with the exact bit pattern of `value` at `site`."""
    t = t.clone()
    t.view(torch.int32)[site] = BITS[value]
    return t


def rand(gen, *shape):
    return torch.randn(*shape, generator=gen)


# ----------------------------------------------------------------- the operations, stated once in PyTorch (CPU)

def compose_fwd(t, kw, dtype):
    """mvp_pointwise_mfma_ex.  t: x (B, K, L), w (M, K) -- (K, M) with w_kmajor --, bias (M) / (B, M), residual, xmask."""
    c = lambda a: None if a is None else a.to(dtype)
    x, w = c(t["x"]), c(t["w"])
    w = w.t() if kw.get("w_kmajor") else w
    nb, m = x.size(0), w.size(0)
    if t.get("xmask") is not None:
        x = tb(x, c(t["xmask"]), 0)
    if kw.get("x_relu"):
        x = torch.relu(x)
    y = torch.einsum("oc,bcl->bol", w, x)
    if t.get("bias") is not None:
        y = y + (c(t["bias"]).view(nb, m, 1) if kw.get("bias_per_cloud") else c(t["bias"]).view(1, m, 1))
    if kw.get("relu"):
        y = torch.relu(y)
    group = kw.get("group", 1)
    if group > 1:
        y = torch.max(y.view(nb, m, -1, group), dim=3)[0]
    if t.get("residual") is not None:
        y = tb(y, c(t["residual"]), 0) if kw.get("res_is_mask") else y + c(t["residual"])
    if kw.get("relu_after"):
        y = torch.relu(y)
    ms = kw.get("m_split", 0)
    return (y[:, :ms], y[:, ms:]) if ms else (y,)


def compose_wgrad(t, kw, dtype):
    """mvp_pointwise_wgrad_mfma_ex: (gw (cout, cin), gb (cout))."""
    x, g = t["x"].to(dtype), t["gy"].to(dtype)
    if t.get("gymask") is not None:
        g = tb(g, t["gymask"].to(dtype), 0)
    if kw.get("x_relu"):
        x = torch.relu(x)
    return torch.einsum("bol,bil->oi", g, x), g.sum((0, 2))


def compose_rowmax(t, kw, dtype):
    """mvp_pointwise_mfma_max: (val, idx) of [relu](W x + bias).max over the positions."""
    (y,) = compose_fwd(t, dict(relu=kw["relu"]), dtype)
    return torch.max(y, dim=2)


COMPOSE = {"fwd": compose_fwd, "wgrad": compose_wgrad, "rowmax": compose_rowmax}


# ----------------------------------------------------------------- the same calls on the GPU

def gpu_fwd(t, kw):
    from mvp_benchmark_amd.pointwise import mfma_linear
    d = lambda a: None if a is None else a.to(DEV)
    flags = {k: bool(kw.get(k)) for k in ("relu", "w_kmajor", "x_relu", "relu_after", "res_is_mask", "bias_per_cloud")}
    out = mfma_linear(d(t["x"]), d(t["w"]), d(t.get("bias")), residual=d(t.get("residual")), xmask=d(t.get("xmask")),
                      group=kw.get("group", 1), m_split=kw.get("m_split", 0), **flags)
    return tuple(o.cpu() for o in (out if isinstance(out, tuple) else (out,)))


def gpu_wgrad(t, kw):
    from mvp_benchmark_amd.pointwise import mfma_wgrad
    d = lambda a: None if a is None else a.to(DEV)
    cout, cin = t["gy"].size(1), t["x"].size(1)
    gw, gb = mfma_wgrad(d(t["x"]), d(t["gy"]), cout, cin, True, gymask=d(t.get("gymask")), x_relu=bool(kw.get("x_relu")))
    return gw.cpu(), gb.cpu()


def gpu_rowmax(t, kw):
    from mvp_benchmark_amd import _lib
    x, w, bias = t["x"].to(DEV), t["w"], t["bias"].to(DEV)
    nb, cin, length = x.shape
    cout, ldw = w.size(0), 0
    if cin % 4:
        w = torch.nn.functional.pad(w, (0, -cin % 4)).contiguous()
        ldw = w.size(1)
    w = w.to(DEV)
    val = torch.empty(nb, cout, device=DEV)
    idx = torch.empty(nb, cout, dtype=torch.int32, device=DEV)
    keys = torch.empty(nb * cout, dtype=torch.int64, device=DEV)
    _lib.call("mvp_pointwise_mfma_max", DEV, nb, cin, cout, length, x, w, ldw, bias, int(kw["relu"]), val, idx, keys,
              keys.numel() * 8)
    return val.cpu(), idx.cpu()


# ----------------------------------------------------------------- the checks

def masks_of(a):
    return torch.isnan(a), a == float("inf"), a == float("-inf")


def same_masks(got, ref):
    return all(torch.equal(g, r) for g, r in zip(masks_of(got), masks_of(ref)))


def assert_matches(got, ref, tol, what):
    """(a) NaN, +Inf and -Inf masks equal the reference's; (b) the bound on everything the reference leaves finite."""
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (what, i, g.shape, r.shape)
        for name, gm, rm in zip(("nan", "+inf", "-inf"), masks_of(g), masks_of(r)):
            assert torch.equal(gm, rm), "%s output %d: %s mask differs at %d elements (kernel %d, reference %d)" % (
                what, i, name, int((gm != rm).sum()), int(gm.sum()), int(rm.sum()))
        fin = torch.isfinite(r)
        err = (g.double() - r)[fin].abs().max().item() if fin.any() else 0.0
        assert err < tol, "%s output %d: error %.3g, bound %.3g" % (what, i, err, tol)


def assert_isolated(got, clean, ref, what):
    """Outside the elements the reference marks non-finite, bit equality with the same call on the clean input."""
    for i, (g, c, r) in enumerate(zip(got, clean, ref)):
        keep = torch.isfinite(r)
        assert torch.equal(g[keep], c[keep]), "%s output %d: %d elements outside the poisoned ones changed" % (
            what, i, int((g[keep] != c[keep]).sum()))


# ----------------------------------------------------------------- the case table
# A case: id, kind (fwd / wgrad / rowmax), t (tensors), kw (options), tol; then for the isolation cases
#   clean  the tensors without the poison (bit equality outside the non-finite elements), and `inside`, a function that
#          marks in each output where a non-finite value may appear at all;
#   same_as  a poisoned MASK has no non-finite output: tensors with the finite mask value that the contract makes it
#          equivalent to (NaN and +Inf pass, -Inf drops); bit equality everywhere.

def edge_positions(length, tile):
    """First and last position, the last column of the first full tile and the first of the last (ragged) tile."""
    ps = {0, length - 1}
    if length > tile:
        ps |= {tile - 1, tile * ((length - 1) // tile)}
    return sorted(ps)


def edge_channels(c, tile):
    cs = {0, c - 1}
    if c > tile:
        cs |= {tile - 1, tile}
    return sorted(cs)


def sites3(nb, c, length, tile_c, tile_l, extra=()):
    """(b, channel, position) sites: every edge position in the first and the last cloud, the edge channels dealt over
    them in turn, the last channel (last k of a ragged K / last row of a ragged M) at both ends, the very last element."""
    cs = edge_channels(c, tile_c)
    pos = [(b, l) for b in (0, nb - 1) for l in edge_positions(length, tile_l)] + list(extra)
    out = [(b, cs[i % len(cs)], l) for i, (b, l) in enumerate(pos)]
    out += [(0, c - 1, 0), (1, c - 1, length // 2), (nb - 1, c - 1, length - 1)]
    return list(dict.fromkeys(out))


def one_sign_row0(w, kmajor):
    """Row 0 of W of a single sign (an Inf stays an Inf there); all other rows mixed."""
    if kmajor:
        w[:, 0] = w[:, 0].abs()
    else:
        w[0] = w[0].abs()
    return w


def fwd_base(cin, cout, length, kmajor, seed):
    """Tensors of one forward-kernel problem: K = reduction, M = output rows."""
    k, m = (cout, cin) if kmajor else (cin, cout)
    gen = torch.Generator().manual_seed(seed)
    w = one_sign_row0(rand(gen, k, m) if kmajor else rand(gen, m, k), kmajor)
    return k, m, dict(x=rand(gen, B, k, length), w=w, bias=rand(gen, m), residual=rand(gen, B, m, length),
                      xmask=rand(gen, B, k, length), cbias=rand(gen, B, m))


def pick(base, *names, **renamed):
    t = {n: base[n] for n in names}
    t.update({n: base[src] for n, src in renamed.items()})
    return t


def isolation_fwd_cases(cin, cout, length, kmajor):
    k, m, base = fwd_base(cin, cout, length, kmajor, 1000 + cin * 7 + cout)
    bm = 64 if m <= 64 else 128
    kw0 = dict(w_kmajor=kmajor)
    values = itertools.cycle(VALUES)
    col = lambda b, l: (lambda outs: [_mark(o, (b, slice(None), l)) for o in outs])
    row = lambda r: (lambda outs: [_mark(o, (slice(None), r, slice(None))) for o in outs])
    for (b, c, l) in sites3(B, k, length, 16, 128):
        clean = pick(base, "x", "w", "bias")
        yield dict(id="x[%d,%d,%d]" % (b, c, l), kind="fwd", kw=kw0, tol=fwd_tol(k), clean=clean, inside=col(b, l),
                   t=dict(clean, x=poison(base["x"], (b, c, l), next(values))))
        clean = pick(base, "x", "w", xmask="xmask")
        clean["xmask"] = clean["xmask"].clone()
        clean["xmask"][b, c, l] = -1.0                          # dropped on the clean input
        v = next(values)
        same = dict(clean, xmask=clean["xmask"].clone())
        same["xmask"][b, c, l] = -1.0 if v == "-inf" else 1.0
        yield dict(id="xmask[%d,%d,%d]" % (b, c, l), kind="fwd", kw=kw0, tol=fwd_tol(k), clean=clean, inside=col(b, l),
                   same_as=same, t=dict(clean, xmask=poison(clean["xmask"], (b, c, l), v)))
    for r, c in itertools.product(edge_channels(m, bm), (0, k - 1)):
        clean = pick(base, "x", "w", "bias")
        yield dict(id="w[%d,%d]" % (r, c), kind="fwd", kw=kw0, tol=fwd_tol(k), clean=clean, inside=row(r),
                   t=dict(clean, w=poison(base["w"], (c, r) if kmajor else (r, c), next(values))))
    for r in edge_channels(m, bm):
        clean = pick(base, "x", "w", "bias")
        yield dict(id="bias[%d]" % r, kind="fwd", kw=kw0, tol=fwd_tol(k), clean=clean, inside=row(r),
                   t=dict(clean, bias=poison(base["bias"], (r,), next(values))))
        clean = pick(base, "x", "w", bias="cbias")
        for b in (0, B - 1):
            yield dict(id="cloud_bias[%d,%d]" % (b, r), kind="fwd", kw=dict(kw0, bias_per_cloud=True), tol=fwd_tol(k),
                       clean=clean, inside=(lambda b, r: lambda outs: [_mark(o, (b, r, slice(None))) for o in outs])(b, r),
                       t=dict(clean, bias=poison(base["cbias"], (b, r), next(values))))
    for (b, r, l) in sites3(B, m, length, bm, 128):
        clean = pick(base, "x", "w", "bias", "residual")
        yield dict(id="residual[%d,%d,%d]" % (b, r, l), kind="fwd", kw=kw0, tol=fwd_tol(k), clean=clean,
                   inside=(lambda s: lambda outs: [_mark(o, s) for o in outs])((b, r, l)),
                   t=dict(clean, residual=poison(base["residual"], (b, r, l), next(values))))


def _mark(out, index):
    m = torch.zeros(out.shape, dtype=torch.bool)
    m[index] = True
    return m


def wgrad_positions(length):
    """(cloud, position) at the slab edges: slabs of 32 positions numbered across the clouds; at these sizes a split is
    exactly 4 slabs, so global slabs 3 | 4 are the first split boundary."""
    spc = (length + 31) // 32
    out = []
    for gs in (3, 4, B * spc - 1):
        if 0 <= gs < B * spc:
            b, l0 = gs // spc, (gs % spc) * 32
            out += [(b, l0), (b, min(l0 + 31, length - 1))]
    return out


def isolation_wgrad_cases(cin, cout, length):
    gen = torch.Generator().manual_seed(2000 + cin + cout + length)
    base = dict(x=rand(gen, B, cin, length), gy=rand(gen, B, cout, length), gymask=rand(gen, B, cout, length))
    tol = wgrad_tol(B * length)
    values = itertools.cycle(VALUES)
    for (b, co, l) in sites3(B, cout, length, 64 if cout <= 64 else 128, 32, wgrad_positions(length)):
        clean = pick(base, "x", "gy")
        yield dict(id="gy[%d,%d,%d]" % (b, co, l), kind="wgrad", kw={}, tol=tol, clean=clean,
                   inside=(lambda co: lambda outs: [_mark(outs[0], (co, slice(None))), _mark(outs[1], (co,))])(co),
                   t=dict(clean, gy=poison(base["gy"], (b, co, l), next(values))))
        clean = pick(base, "x", "gy", "gymask")
        clean["gymask"] = clean["gymask"].clone()
        clean["gymask"][b, co, l] = -1.0
        v = next(values)
        same = dict(clean, gymask=clean["gymask"].clone())
        same["gymask"][b, co, l] = -1.0 if v == "-inf" else 1.0
        yield dict(id="gymask[%d,%d,%d]" % (b, co, l), kind="wgrad", kw={}, tol=tol, clean=clean, same_as=same,
                   inside=(lambda co: lambda outs: [_mark(outs[0], (co, slice(None))), _mark(outs[1], (co,))])(co),
                   t=dict(clean, gymask=poison(clean["gymask"], (b, co, l), v)))
    for (b, ci, l) in sites3(B, cin, length, 64 if cin <= 64 else 128, 32, wgrad_positions(length)):
        clean = pick(base, "x", "gy")
        yield dict(id="x[%d,%d,%d]" % (b, ci, l), kind="wgrad", kw={}, tol=tol, clean=clean,
                   inside=(lambda ci: lambda outs: [_mark(outs[0], (slice(None), ci)), torch.zeros_like(outs[1], dtype=torch.bool)])(ci),
                   t=dict(clean, x=poison(base["x"], (b, ci, l), next(values))))


ACTIVATIONS = [dict(relu=True), dict(relu_after=True), dict(x_relu=True), dict(relu=True, residual=True, relu_after=True),
               dict(relu=True, bias_per_cloud=True), dict(x_relu=True, residual=True, relu_after=True, bias_per_cloud=True)]


def activation_cases(cin, cout, length, kmajor):
    """A NaN (and an Inf) through the product, the bias and the residual of every activation pattern, one and two outputs."""
    k, m, base = fwd_base(cin, cout, length, kmajor, 3000 + cin * 5 + cout)
    combos = list(ACTIVATIONS)
    if m > 32:
        top = (m - 1) // 32 * 32                               # the largest split below m
        combos += [dict(m_split=32, x_relu=True, relu=True), dict(m_split=top, relu_after=True, bias_per_cloud=True),
                   dict(m_split=top, relu=True, relu_after=True)]
    values = itertools.cycle(VALUES)
    soft = itertools.cycle(("nan", "-nan", "inf"))              # where -Inf would leave nothing non-finite behind a ReLU
    l_mid = 128 * ((length - 1) // 128)                        # first column of the last tile
    for combo in combos:
        kw = dict(combo, w_kmajor=kmajor)
        with_res = kw.pop("residual", False)
        clean = pick(base, "x", "w", bias="cbias" if kw.get("bias_per_cloud") else "bias")
        if with_res:
            clean["residual"] = base["residual"]
        ms = kw.get("m_split", 0)
        name = ",".join(sorted(k_ for k_ in combo))
        mk = lambda src, t: dict(id="%s<-%s" % (name, src), kind="fwd", kw=kw, tol=fwd_tol(k), t=t)
        v = next(soft) if kw.get("x_relu") else next(values)
        yield mk("x:" + v, dict(clean, x=poison(base["x"], (1, k - 1, length - 1), v)))
        yield mk("x:" + "nan", dict(clean, x=poison(base["x"], (B - 1, 0, l_mid), "nan")))
        rows = (ms - 1, ms) if ms else (m - 1,)                # both outputs of a split
        for r in rows:
            v = next(soft)
            site = (B - 1, r) if kw.get("bias_per_cloud") else (r,)
            yield mk("bias[%d]:%s" % (r, v), dict(clean, bias=poison(clean["bias"], site, v)))
        if with_res:
            v = next(soft)
            yield mk("residual:" + v, dict(clean, residual=poison(base["residual"], (0, m - 1, length - 1), v)))
        x2 = poison(poison(base["x"], (0, 0, 0), "inf"), (0, k - 1, 0), "inf")      # two +Inf in one column: Inf in the
        yield mk("x:two inf", dict(clean, x=x2))                                     # one-sign row, NaN where the signs mix


GROUP_P = {2: 66, 4: 35, 32: 5}                                # P * group = 132, 140, 160: a ragged second tile of positions
GROUP_COMBOS = [dict(), dict(relu=True), dict(relu=True, residual=True), dict(relu=True, residual=True, res_is_mask=True),
                dict(relu=True, residual=True, relu_after=True), dict(relu=True, bias_per_cloud=True),
                dict(residual=True, res_is_mask=True, relu_after=True, bias_per_cloud=True)]


def group_cases(group, cout, kmajor=False):
    """Clean inputs, then a NaN as the first, middle and last member of a group (in the first, the last and the two groups
    either side of the position-tile edge).  kmajor: the reduction has `cin` = 40 either way."""
    cin, p = 40, GROUP_P[group]
    length = p * group
    gen = torch.Generator().manual_seed(4000 + group * 10 + cout)
    w = one_sign_row0(rand(gen, cin, cout) if kmajor else rand(gen, cout, cin), kmajor)
    base = dict(x=rand(gen, B, cin, length), w=w, bias=rand(gen, cout), cbias=rand(gen, B, cout), residual=rand(gen, B, cout, p))
    groups = sorted({0, p - 1, 127 // group, min(p - 1, 128 // group)})
    members = sorted({0, group // 2, group - 1})
    for combo in GROUP_COMBOS:
        kw = dict(combo, group=group, w_kmajor=kmajor)
        with_res = kw.pop("residual", False)
        clean = pick(base, "x", "w", bias="cbias" if kw.get("bias_per_cloud") else "bias")
        if with_res:
            clean["residual"] = base["residual"]
        name = ",".join(sorted(combo)) or "plain"
        yield dict(id=name + " clean", kind="fwd", kw=kw, tol=fwd_tol(cin), t=clean, finite=True)
        for i, (q, mem) in enumerate(itertools.product(groups, members)):
            b = i % B
            inside = (lambda b, q: lambda outs: [_mark(outs[0], (b, slice(None), q))])(b, q)
            yield dict(id="%s nan member %d of group %d" % (name, mem, q), kind="fwd", kw=kw, tol=fwd_tol(cin), clean=clean,
                       inside=inside, t=dict(clean, x=poison(base["x"], (b, (i * 7) % cin, q * group + mem), VALUES[i % 2])))


def rowmax_cases(cin, cout, length):
    """Cloud 0 holds two NaN columns of opposite sign bits (every row: NaN at the first); one weight row is NaN (NaN at
    position 0 in every cloud); one row's every product is -Inf (-Inf at position 0; 0 behind the ReLU)."""
    gen = torch.Generator().manual_seed(5000 + cin + cout)
    for relu, (first, second) in itertools.product((1, 0), (("-nan", "nan"), ("nan", "-nan"))):
        x, w, bias = rand(gen, B, cin, length), rand(gen, cout, cin), rand(gen, cout)
        l1, l2 = min(length - 2, 129), length - 1
        for c in range(cin):
            x = poison(poison(x, (0, c, l1), first), (0, c, l2), second)
        x[:, 0] = x[:, 0].abs() + 0.1                           # (keeps the NaNs of cloud 0: abs only clears the sign bit)
        w = poison(poison(w, (cout - 1, cin - 1), first), (cout // 2, 0), "-inf")
        yield dict(id="relu=%d %s first" % (relu, first), kind="rowmax", kw=dict(relu=relu), tol=fwd_tol(cin),
                   t=dict(x=x, w=w, bias=bias), l1=l1)


def all_cases():
    for cin, cout, length, kmajor in FWD_PARAMS:
        yield from isolation_fwd_cases(cin, cout, length, kmajor)
        yield from activation_cases(cin, cout, length, kmajor)
    for cin, cout, length in SHAPES:
        yield from rowmax_cases(cin, cout, length)
    for shape in WGRAD_SHAPES:
        yield from isolation_wgrad_cases(*shape)
    for group, cout in itertools.product((2, 4, 32), (33, 130)):
        yield from group_cases(group, cout)
    yield from group_cases(4, 68, kmajor=True)
    yield from relu_prime_entry_cases()


# ----------------------------------------------------------------- ReLU' (case table of the C entries; modules below)

def relu_prime_tensors(cin, cout, length, seed, passing=True, relu_in=False):
    """A layer y = relu(W x + b) whose input holds one NaN (so y holds a NaN column), and a grad_out with +-Inf where
    y <= 0 by a margin (dropped by ReLU') and, with `passing`, +Inf on the NaN column (passed: threshold_backward compares
    y <= 0).  Not `passing` where the layer takes relu(x) (`relu_in`): the Inf that passes would meet relu(x)'s zeros."""
    gen = torch.Generator().manual_seed(seed)
    x, w, bias = rand(gen, B, cin, length), rand(gen, cout, cin, 1), rand(gen, cout)
    go = rand(gen, B, cout, length)
    pre = torch.nn.functional.conv1d(torch.relu(x.double()) if relu_in else x.double(), w.double(), bias.double())
    bn, ln = 1, length - 1
    pre[bn, :, ln] = 0.0                                        # (not on the NaN column)
    dead = (pre < -0.5).nonzero()                               # far from 0: no float32 route disagrees about y <= 0 there
    assert len(dead) >= 4
    for i, j in enumerate((0, len(dead) // 3, 2 * len(dead) // 3, len(dead) - 1)):
        go = poison(go, tuple(dead[j].tolist()), ("inf", "-inf")[i % 2])
    x = poison(x, (bn, cin - 1, ln), "nan")
    if passing:
        go = poison(go, (bn, 0, ln), "inf")
    return x, w, bias, go


def relu_prime_entry_cases():
    """ReLU' at the three mask sites of the C entries: xmask and the residual-as-mask of the data gradient, gymask of the
    weight gradient -- masks and gradients handed over explicitly, so values are compared at the bound too."""
    for cin, cout, length in ((68, 130, 260), (16, 64, 128), (40, 33, 132)):
        x, w, bias, go = relu_prime_tensors(cin, cout, length, 6000 + cin)
        y = torch.relu(torch.nn.functional.conv1d(x, w, bias))  # holds the NaN column
        w2 = w.view(cout, cin).contiguous()
        yield dict(id="dgrad xmask (%d,%d,%d)" % (cin, cout, length), kind="fwd", kw=dict(w_kmajor=True), tol=fwd_tol(cout),
                   t=dict(x=go, w=w2, xmask=y))
        yield dict(id="dgrad xmask + input mask (%d,%d,%d)" % (cin, cout, length), kind="fwd", tol=fwd_tol(cout),
                   kw=dict(w_kmajor=True, res_is_mask=True), t=dict(x=go, w=w2, xmask=y, residual=x))
        yield dict(id="wgrad gymask (%d,%d,%d)" % (cin, cout, length), kind="wgrad", kw={}, tol=wgrad_tol(B * length),
                   t=dict(x=x, gy=go, gymask=y))
        go = relu_prime_tensors(cin, cout, length, 6000 + cin, passing=False)[3]
        yield dict(id="wgrad gymask x_relu (%d,%d,%d)" % (cin, cout, length), kind="wgrad", kw=dict(x_relu=True),
                   tol=wgrad_tol(B * length), t=dict(x=x, gy=go, gymask=y))


def composed_layer(x, w, bias, kw, res=None, cb=None):
    """The float32 function a pointwise layer stands for, for plain autograd."""
    a = torch.relu(x) if kw.get("relu_in") else x
    h = torch.nn.functional.conv1d(a, w, bias)
    if cb is not None:
        h = h + cb.unsqueeze(2)
    h = torch.relu(h) if kw.get("relu") else h
    h = h + res if res is not None else h
    return torch.relu(h) if kw.get("relu_after") else h


FUSED_COMBOS = [dict(relu=True), dict(relu_in=True, relu=True), dict(residual=True, relu_after=True),
                dict(relu=True, cloud_bias=True), dict(relu_in=True, residual=True, relu_after=True)]


def module_cases():
    """(id, tensors, options) of the autograd cases: _PointwiseConv (options None) and _PointwiseConvFused."""
    for cin, cout, length in ((68, 130, 260), (16, 64, 128), (40, 33, 132), (129, 128, 388)):
        x, w, bias, go = relu_prime_tensors(cin, cout, length, 7000 + cin)
        yield "conv+relu (%d,%d,%d)" % (cin, cout, length), dict(x=x, w=w, bias=bias, go=go), None
        if cin % 4:
            continue
        gen = torch.Generator().manual_seed(7100 + cin)
        # (a residual / per-cloud vector of small scale: the layer's dead outputs stay dead, by the margin above)
        res, cb = 0.1 * rand(gen, B, cout, length), 0.1 * rand(gen, B, cout)
        go_in = relu_prime_tensors(cin, cout, length, 7000 + cin, passing=False, relu_in=True)[3]
        for combo in FUSED_COMBOS:
            t = dict(x=x, w=w, bias=bias, go=go_in if combo.get("relu_in") else go)
            if combo.get("residual"):
                t["res"] = res
            if combo.get("cloud_bias"):
                t["cb"] = cb
            yield "fused %s (%d,%d,%d)" % (",".join(sorted(combo)), cin, cout, length), t, combo


def autograd_reference(t, kw, dtype):
    """(y, gx, gw, gb[, gres][, gcb]) by plain autograd of the composed function on the CPU."""
    leaves = {k: v.to(dtype).requires_grad_() for k, v in t.items() if k != "go"}
    y = composed_layer(leaves["x"], leaves["w"], leaves["bias"], kw or dict(relu=True), leaves.get("res"), leaves.get("cb"))
    order = [k for k in ("x", "w", "bias", "res", "cb") if k in leaves]
    return (y.detach(),) + torch.autograd.grad(y, [leaves[k] for k in order], t["go"].to(dtype))


# ----------------------------------------------------------------- CPU: the table itself

def test_reference_patterns_are_order_free_and_not_vacuous():
    """The float64 reference and the float32 CPU composition agree on the NaN / +Inf / -Inf masks of EVERY case of the
    table (so the pattern is a property of the inputs, not of a summation order), and every case's outputs are at least
    80 % finite with at least one non-finite value -- none passes vacuously or on a tensor that is all NaN.  (The clean
    group-maximum cases are finite by design.  A poisoned MASK has no non-finite output under the contract -- NaN and +Inf
    pass the gradient, -Inf drops it: those cases must instead differ from the clean call exactly inside the mask's column,
    and equal the call with the equivalent finite mask.)  Row max: the reported position is the first NaN."""
    n = 0
    for case in all_cases():
        f = COMPOSE[case["kind"]]
        r64, r32 = f(case["t"], case["kw"], torch.float64), f(case["t"], case["kw"], torch.float32)
        what = "%s %s %s" % (case["kind"], case["kw"], case["id"])
        for a, b in zip(r64, r32):
            if a.dtype.is_floating_point:
                assert same_masks(a.double(), b.double()), what
            else:                                                                       # (positions of the row max)
                bad = ~torch.isfinite(r64[0])
                assert torch.equal(a[bad], b[bad]), what
        flat = torch.cat([a.double().flatten() for a in r64])
        finite = torch.isfinite(flat).double().mean().item()
        assert finite >= 0.8, (what, finite)
        if case.get("finite"):
            assert finite == 1.0, what
        elif "same_as" in case:
            assert finite == 1.0, what
            same, clean = f(case["same_as"], case["kw"], torch.float64), f(case["clean"], case["kw"], torch.float64)
            changed = [a != c for a, c in zip(r64, clean)]
            assert all(torch.equal(a, s) for a, s in zip(r64, same)), what
            assert all(not (ch & ~ins).any() for ch, ins in zip(changed, case["inside"](r64))), what
            if not torch.equal(case["same_as"][_mask_name(case)], case["clean"][_mask_name(case)]):
                assert any(ch.any() for ch in changed), what
        else:
            assert finite < 1.0, what
        if "inside" in case and "same_as" not in case:                                  # non-finite only where it may be
            for a, ins in zip(r64, case["inside"](r64)):
                assert not (~torch.isfinite(a) & ~ins).any(), what
        if case["kind"] == "rowmax":
            val, idx = r64
            assert torch.isnan(val[0]).all() and (idx[0, :-1] == case["l1"]).all() and idx[0, -1] == 0, what
            assert torch.isnan(val[:, -1]).all() and (idx[:, -1] == 0).all(), what
            half = val.size(1) // 2
            assert (val[1:, half] == (0.0 if case["kw"]["relu"] else float("-inf"))).all() and (idx[1:, half] == 0).all(), what
        n += 1
    assert n > 1000, n
    for name, t, kw in module_cases():
        r64, r32 = autograd_reference(t, kw, torch.float64), autograd_reference(t, kw, torch.float32)
        assert all(same_masks(a.double(), b.double()) for a, b in zip(r64, r32)), name
        for a in r32:
            assert torch.isfinite(a).double().mean().item() >= 0.8, name
        assert not torch.isfinite(r32[0]).all() and not torch.isfinite(r32[2]).all(), name      # y, grad w
        # the Inf of grad_out at the dead outputs is dropped: the bias gradient holds the one +Inf that passed, no NaN
        passed = 0 if kw and kw.get("relu_in") else 1
        assert not torch.isnan(r32[3]).any() and (r32[3] == float("inf")).sum() == passed, name
        assert torch.isfinite(r32[1]).all() == (passed == 0), name                            # grad x


def _mask_name(case):
    return "xmask" if "xmask" in case["t"] else "gymask"


# ----------------------------------------------------------------- GPU

GPU = {"fwd": gpu_fwd, "wgrad": gpu_wgrad, "rowmax": gpu_rowmax}


def run_cases(cases):
    """Every case against the float64 reference; the isolation cases also against the clean call (computed once per set
    of clean tensors)."""
    clean_runs = {}
    failures = []
    n = 0
    for case in cases:
        what = "%s %s %s" % (case["kind"], case["kw"], case["id"])
        ref = COMPOSE[case["kind"]](case["t"], case["kw"], torch.float64)
        got = GPU[case["kind"]](case["t"], case["kw"])
        n += 1
        try:
            if case["kind"] == "rowmax":
                check_rowmax(got, ref, case, what)
                continue
            assert_matches(got, ref, case["tol"], what)
            if "same_as" in case:
                same = GPU[case["kind"]](case["same_as"], case["kw"])
                assert all(torch.equal(g, s) for g, s in zip(got, same)), what + ": differs from the equivalent finite mask"
            if "clean" in case:
                key = (case["kind"], str(case["kw"])) + tuple(sorted((k, id(v)) for k, v in case["clean"].items()))
                if "same_as" in case or key not in clean_runs:
                    clean = GPU[case["kind"]](case["clean"], case["kw"])
                    if "same_as" not in case:
                        clean_runs[key] = (clean, case["clean"])          # (the tensors stay alive: ids stay unique)
                else:
                    clean = clean_runs[key][0]
                if "same_as" in case:                                     # only the mask's own column may change
                    for g, c, ins in zip(got, clean, case["inside"](got)):
                        assert torch.equal(g[~ins], c[~ins]), what + ": changed outside the mask's column"
                else:
                    assert_isolated(got, clean, ref, what)
        except AssertionError as e:
            failures.append(str(e))
    assert n > 0
    assert not failures, "%d of %d cases fail:\n%s" % (len(failures), n, "\n".join(failures[:40]))


def check_rowmax(got, ref, case, what):
    val, idx = got
    rval, ridx = ref
    assert_matches((val,), (rval,), case["tol"], what)
    bad = ~torch.isfinite(rval)
    assert torch.equal(idx.long()[bad], ridx[bad]), what + ": position of a non-finite maximum is not torch.max's"
    # finite rows: float32 may pick another of two near-equal maxima than float64 -- the reference's value AT the reported
    # position is within the bound of its maximum
    (y,) = compose_fwd(case["t"], dict(relu=case["kw"]["relu"]), torch.float64)
    assert (idx >= 0).all() and (idx < y.size(2)).all(), what
    at = y.gather(2, idx.long().unsqueeze(2)).squeeze(2)
    assert ((rval - at)[~bad].abs() < 2 * case["tol"]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,length,kmajor", FWD_PARAMS)
def test_forward_one_poisoned_element_stays_in_its_column_or_row(cin, cout, length, kmajor):
    """One NaN / -NaN / +Inf / -Inf in x, w, the bias, the per-cloud bias, the residual or xmask of mvp_pointwise_mfma_ex,
    at every tile edge: non-finite exactly where the reference says, bit-identical to the clean call elsewhere."""
    run_cases(isolation_fwd_cases(cin, cout, length, kmajor))


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,length", WGRAD_SHAPES)
def test_wgrad_one_poisoned_element_stays_in_its_row_or_column(cin, cout, length):
    """mvp_pointwise_wgrad_mfma_ex: a poisoned gy[b, co, l] touches gw[co, :] and gb[co] only, a poisoned x[b, ci, l]
    gw[:, ci] only, a poisoned gymask nothing beyond what the equivalent finite mask does."""
    run_cases(isolation_wgrad_cases(cin, cout, length))


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,length,kmajor", FWD_PARAMS)
def test_activations_keep_nan_like_torch_relu(cin, cout, length, kmajor):
    """relu, relu_after, x_relu, relu -> + residual -> relu_after, one and two outputs (m_split), with and without a bias
    per cloud: a NaN through the product, the bias or the residual comes out as torch.relu's composition leaves it."""
    run_cases(activation_cases(cin, cout, length, kmajor))


@pytest.mark.gpu
@pytest.mark.parametrize("cout", [33, 130])
@pytest.mark.parametrize("group", [2, 4, 32])
def test_group_maximum_matches_float64_and_propagates_nan(group, cout):
    """The group > 1 epilogue with and without residual, res_is_mask, relu_after and a bias per cloud: clean inputs at the
    forward bound, then a NaN as the first, middle and last member -- that group NaN (where the reference says), every
    other output bit-identical."""
    run_cases(group_cases(group, cout))


@pytest.mark.gpu
def test_group_maximum_with_the_transposed_weight():
    run_cases(group_cases(4, 68, kmajor=True))


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,length", SHAPES)
def test_row_maximum_reports_the_first_nan_with_and_without_relu(cin, cout, length):
    """mvp_pointwise_mfma_max, relu = 1 and 0: a NaN of either sign bit in a row -> NaN at the first NaN; a row whose
    every product is -Inf -> -Inf (0 behind the ReLU) at position 0."""
    run_cases(rowmax_cases(cin, cout, length))


@pytest.mark.gpu
def test_relu_prime_at_the_mask_sites_of_the_c_entries():
    """xmask, the residual as a mask and gymask are aten.threshold_backward's select: grad_out passes where the saved
    output is NaN, an Inf of grad_out where the output is <= 0 is dropped (not multiplied by 0)."""
    run_cases(relu_prime_entry_cases())


@pytest.mark.gpu
def test_relu_prime_is_one_convention_on_every_backward_route():
    """_PointwiseConv on every route of its backward pass (the switches test_pointwise_conv_autograd_through_mfma toggles)
    and _PointwiseConvFused: output and every gradient carry the NaN / +Inf / -Inf masks that plain autograd of the
    composed float32 function gives on the CPU -- hence the same masks on all routes."""
    from mvp_benchmark_amd import pointwise as pw
    saved = (pw.MFMA_DGRAD, pw.MFMA_WGRAD_MIN_CIN, pw.MFMA_TRAIN, pw.MFMA_WGRAD_MIN_POSITIONS)
    failures = []
    try:
        pw.MFMA_TRAIN, pw.MFMA_WGRAD_MIN_POSITIONS = True, 0
        for name, t, kw in module_cases():
            ref = autograd_reference(t, kw, torch.float32)
            routes = ((True, 1), (True, 1 << 30), (False, 1), (False, 1 << 30)) if kw is None else ((True, 1),)
            for dgrad, wmin in routes:
                pw.MFMA_DGRAD, pw.MFMA_WGRAD_MIN_CIN = dgrad, wmin
                leaves = {k: v.to(DEV).requires_grad_() for k, v in t.items() if k != "go"}
                order = [k for k in ("x", "w", "bias", "res", "cb") if k in leaves]
                if kw is None:
                    y = pw.pointwise_conv(leaves["x"], leaves["w"], leaves["bias"], relu=True)
                else:
                    assert pw._fused_routes(leaves["x"], leaves["w"], True), name
                    y = pw.pointwise_conv_fused(leaves["x"], leaves["w"], leaves["bias"], relu_in=bool(kw.get("relu_in")),
                                                relu=bool(kw.get("relu")), residual=leaves.get("res"),
                                                relu_after=bool(kw.get("relu_after")), cloud_bias=leaves.get("cb"))
                got = (y.detach(),) + torch.autograd.grad(y, [leaves[k] for k in order], t["go"].to(DEV))
                for what, g, r in zip(["y"] + ["grad " + k for k in order], got, ref):
                    for mname, gm, rm in zip(("nan", "+inf", "-inf"), masks_of(g.cpu()), masks_of(r)):
                        if not torch.equal(gm, rm):
                            failures.append("%s dgrad=%s wgrad_min_cin=%d: %s %s mask: %d against %d" % (
                                name, dgrad, wmin, what, mname, int(gm.sum()), int(rm.sum())))
    finally:
        pw.MFMA_DGRAD, pw.MFMA_WGRAD_MIN_CIN, pw.MFMA_TRAIN, pw.MFMA_WGRAD_MIN_POSITIONS = saved
    assert not failures, "\n".join(failures[:20])
