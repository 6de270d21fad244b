"""What the 1x1-convolution gradient tests share (tests/test_conv_gradients_cpu.py, tests/test_gpu_conv_gradients.py): the
shapes with the edge each one is there for, the two input families, the winner patterns of the conv -> max backward, and the
float64 references of the three entry points off the MFMA path
    mvp_pointwise_max_backward (csrc/pointwise_max.hip), mvp_pointwise_wgrad, mvp_pointwise_dgrad (csrc/pointwise.hip).
Plain torch on the CPU, nothing of the op layer.

Every reference returns, beside a sum, the same sum over absolute values (its `mag`).  Two checks follow from it:
    exact    integers in [-4, 4] stored as float32.  While mag < 2^24 every partial sum of every order is an integer below
             2^24, which float32 holds: neither the order nor a fused multiply-add changes a bit, the result EQUALS the
             reference.
    random   randn.  A float32 sum of t rounded products, in any order and with any mix of fmaf and multiply-then-add, is
             within gamma_t * mag of the exact sum, gamma_t = t u / (1 - t u), u = 2^-24 (Higham, Accuracy and Stability of
             Numerical Algorithms, sec. 3.1); a sum of t + 1 numbers (additions only) takes t roundings.  A product of two
             float32 is exact in float64, so the reference's own error is that of its float64 additions, 2^-29 of the bound."""
import functools
from collections import namedtuple

import torch

U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 24
FAMILIES = ("exact", "random")


def gamma(t):
    """t u / (1 - t u), elementwise; t a number or a tensor of term counts."""
    t = torch.as_tensor(t, dtype=torch.float64)
    return t * U / (1 - t * U)


def shape_id(shape):
    return "x".join(map(str, shape))


def values(size, family, gen):
    if family == "exact":
        return torch.randint(-4, 5, size, generator=gen).float()
    assert family == "random", family
    return torch.randn(size, generator=gen)


def assert_exactly_representable(ref):
    """Every mag of an `exact` case is below 2^24 (and so is every partial sum of every summation order)."""
    for name, value in ref.items():
        if name.endswith("_mag"):
            assert float(value.max()) < EXACT_LIMIT, (name, float(value.max()))


# ------------------------------------------------------------------------------------------- conv -> max over the positions

# (b, cin, cout, len) -> the edge it is there for
MAX_SHAPES = (
    ((1, 1, 1, 1), "smallest possible shape; cout_p2 = 1, an empty sorting network"),
    ((3, 5, 2, 33), "33 positions leave a 1-position partial tile"),
    ((11, 65, 33, 20), "b = 8 + 3: the unrolled loop and its tail; cin = 65: a ragged second block of 64 channels; "
                       "cout one above a power of two"),
    ((2, 64, 64, 64), "one winner per position"),
    ((9, 300, 200, 257), "cin > 256: the strided ci loop; len = 257: two positions per thread in the scan"),
    ((2, 7, 2048, 1356), "exactly on the LDS guard: 3 * 2048 + 1356 = 7500 words"),
    ((2, 7, 2049, 1353), "on the guard with cout_p2 = 4096"),
    ((2, 5, 4096, 16384), "both maxima of the header; gw / gb only, by the direct gather; gx is refused"),
)
MAX_LDS_BYTES = 30000        # (3 cout + len) * 4 must not exceed it where gx is wanted or the columns are staged


def max_lds_bytes(shape):
    return (3 * shape[2] + shape[3]) * 4


def takes_gx(shape):
    """The data gradient (and the staged weight gradient) covers the shape: the sort of a cloud's winners fits its LDS."""
    return max_lds_bytes(shape) <= MAX_LDS_BYTES


def cout_p2(cout):
    p = 1
    while p < cout:
        p <<= 1
    return p


def _run_lengths(cout):
    """9, 17, 9, 17, ... summing to cout (the last one cut short)."""
    runs, left = [], cout
    while left > 0:
        runs.append(min(left, 17 if len(runs) % 2 else 9))
        left -= runs[-1]
    return runs


def one_positions(length):
    """0, 31, 32 and len - 1, clipped to the shape, each once."""
    return sorted({min(p, length - 1) for p in (0, 31, 32, length - 1)})


def tile_edge_positions(length):
    return sorted({p for p in (31, 32, 63, 64, length - 1) if p < length})


def patterns_for(shape):
    """The winner patterns that fit a shape, by name."""
    b, cin, cout, length = shape
    names = ["random"] + ["one_position_%d" % p for p in one_positions(length)]
    if cout == length:
        names.append("one_each")
    if length >= 33:
        names.append("tile_edges")
    if cout >= 9 and len(_run_lengths(cout)) <= length:
        names.append("runs_9_17")
    if cout >= 2:
        names.append("descending")
    return names


def winners(shape, pattern, gen):
    """idx (b, cout) int32 in [0, len):
      random            uniform
      one_position_P    every channel of every cloud wins position P
      one_each          cout == len, a permutation per cloud
      tile_edges        only positions 31, 32, 63, 64 and len - 1
      runs_9_17         the channels dealt in runs of 9 and 17 onto ascending positions (cloud 0 in channel order, the
                        other clouds through a permutation of the channels: a position keeps its 9 or 17 winners)
      descending        channel c -> a position decreasing in c"""
    b, cin, cout, length = shape
    assert pattern in patterns_for(shape), (shape, pattern)
    if pattern == "random":
        idx = torch.randint(0, length, (b, cout), generator=gen)
    elif pattern.startswith("one_position_"):
        idx = torch.full((b, cout), int(pattern.rsplit("_", 1)[1]))
    elif pattern == "one_each":
        idx = torch.stack([torch.randperm(length, generator=gen) for _ in range(b)])
    elif pattern == "tile_edges":
        allowed = torch.tensor(tile_edge_positions(length))
        idx = allowed[torch.randint(0, len(allowed), (b, cout), generator=gen)]
    elif pattern == "runs_9_17":
        runs = _run_lengths(cout)
        at = torch.tensor([r * length // len(runs) for r in range(len(runs))])
        dealt = torch.repeat_interleave(at, torch.tensor(runs))
        rows = [dealt]
        for _ in range(1, b):
            row = torch.empty_like(dealt)
            row[torch.randperm(cout, generator=gen)] = dealt
            rows.append(row)
        idx = torch.stack(rows)
    else:
        assert pattern == "descending", pattern
        idx = ((cout - 1 - torch.arange(cout)) * length // cout).expand(b, cout)
    assert idx.shape == (b, cout) and int(idx.min()) >= 0 and int(idx.max()) < length
    return idx.to(torch.int32).contiguous()


def ref_max_backward(x, w, g, idx):
    """x (b, cin, len), w (cout, cin), g (b, cout), idx (b, cout) -> dict of float64 tensors
      gw[co, ci]   = sum_b g[b, co] x[b, ci, idx[b, co]]                gw_mag: the same over absolute values
      gb[co]       = sum_b g[b, co]                                     gb_mag
      gx[b, ci, l] = sum_{co: idx[b, co] = l} g[b, co] w[co, ci]        gx_mag
      count[b, l]  = the number of winners at l (int64)"""
    b, cin, length = x.shape
    cout = w.shape[0]
    xd, wd, gd = x.double(), w.double(), g.double()
    at = idx.long()
    where = at.unsqueeze(1).expand(b, cin, cout)                 # [b, ci, co] -> the position (b, co) won
    cols = torch.gather(xd, 2, where)                            # [b, ci, co] = x[b, ci, idx[b, co]]
    terms = gd.unsqueeze(1) * wd.t().unsqueeze(0)                # [b, ci, co] = g[b, co] w[co, ci]
    return {
        "gw": torch.einsum("bo,bio->oi", gd, cols),
        "gw_mag": torch.einsum("bo,bio->oi", gd.abs(), cols.abs()),
        "gb": gd.sum(0),
        "gb_mag": gd.abs().sum(0),
        "gx": torch.zeros(b, cin, length, dtype=torch.float64).scatter_add_(2, where, terms),
        "gx_mag": torch.zeros(b, cin, length, dtype=torch.float64).scatter_add_(2, where, terms.abs()),
        "count": torch.zeros(b, length, dtype=torch.int64).scatter_add_(1, at, torch.ones_like(at)),
    }


MaxCase = namedtuple("MaxCase", "shape x w g idx ref")


@functools.lru_cache(maxsize=8)
def max_case(shape, pattern, family):
    """Inputs and reference of one (shape, pattern, family), made once and left unchanged."""
    b, cin, cout, length = shape
    gen = torch.Generator().manual_seed(5)
    x = values((b, cin, length), family, gen)
    w = values((cout, cin), family, gen)
    g = values((b, cout), family, gen)
    idx = winners(shape, pattern, gen)
    ref = ref_max_backward(x, w, g, idx)
    if family == "exact":
        assert_exactly_representable(ref)
    return MaxCase(shape, x, w, g, idx, ref)


def max_cases():
    """Every (shape, pattern) of the conv -> max backward."""
    return [(shape, pattern) for shape, _ in MAX_SHAPES for pattern in patterns_for(shape)]


def max_case_id(value):
    return shape_id(value) if isinstance(value, tuple) else str(value)


# ------------------------------------------------------------------------------------------------ few channels: weight gradient

Plan = namedtuple("Plan", "cog cig pg chunks")     # co-groups, ci-groups, position groups, blocks of input channels


def pw_plan(cin, cout):
    """csrc/pointwise.hip: pw_plan, line for line."""
    threads, tile, max_rows = 256, 64, 224
    cog = (cout + 3) // 4
    cig = min((cin + 3) // 4, threads // cog, max_rows // 4 - cog)
    pg = min(threads // (cog * cig), tile // 4)
    return Plan(cog, cig, pg, (cin + 4 * cig - 1) // (4 * cig))


WGRAD_TILE, WGRAD_RUN = 64, 1024                   # positions per LDS tile, per workgroup
WGRAD_MAX_POSITIONS = 2 ** 20                      # b * len of the case list: the exact family's mags stay below 2^24

# (b, cin, cout, len), the plan the kernel makes for it, the edge
WGRAD_SHAPES = tuple(((2, 5, 5, length), Plan(2, 2, 16, 1), edge) for length, edge in (
    (4, "one float4 per row"),
    (60, "the tile's last float4 is past the end"),
    (64, "exactly one tile"),
    (68, "one float4 into the second tile"),
    (1020, "the run's last float4 is past the end"),
    (1024, "exactly one run of 16 tiles"),
    (1028, "one float4 into a second workgroup"),
    (2052, "three workgroups per cloud"),
)) + (
    ((3, 1, 1, 64), Plan(1, 1, 16, 1), "PG = 16 from the cap of one group per float4"),
    ((2, 28, 9, 128), Plan(3, 7, 12, 1), "cog cig = 21: PG = 12 does not divide the 16 float4 of a tile"),
    ((2, 130, 33, 68), Plan(9, 28, 1, 2), "252 active threads, 4 idle"),
    ((2, 65, 64, 64), Plan(16, 16, 1, 2), "two channel blocks, the second of one channel; the bias from block 0 only"),
    ((1, 221, 4, 8), Plan(1, 55, 4, 2), "two channel blocks at cog = 1"),
    ((2, 17, 49, 132), Plan(13, 5, 3, 1), "a general ragged shape"),
)


def ref_small_wgrad(x, gy):
    """x (b, cin, len), gy (b, cout, len) -> gw[co, ci] = sum_{b, l} gy[b, co, l] x[b, ci, l], gb[co] = sum_{b, l} gy[b, co, l]
    and their mags, float64."""
    xd, gd = x.double(), gy.double()
    return {
        "gw": torch.einsum("bol,bil->oi", gd, xd),
        "gw_mag": torch.einsum("bol,bil->oi", gd.abs(), xd.abs()),
        "gb": gd.sum((0, 2)),
        "gb_mag": gd.abs().sum((0, 2)),
    }


WgradCase = namedtuple("WgradCase", "shape x gy ref")


@functools.lru_cache(maxsize=8)
def wgrad_case(shape, family):
    b, cin, cout, length = shape
    assert b * length <= WGRAD_MAX_POSITIONS
    gen = torch.Generator().manual_seed(6)
    x = values((b, cin, length), family, gen)
    gy = values((b, cout, length), family, gen)
    ref = ref_small_wgrad(x, gy)
    if family == "exact":
        assert_exactly_representable(ref)
    return WgradCase(shape, x, gy, ref)


# -------------------------------------------------------------------------------------------------- few channels: data gradient

DGRAD_CINS = (1, 8, 9, 16, 17, 24, 25, 48, 49, 50, 63, 64)
DGRAD_LENS = (4, 508, 512, 516)                    # a workgroup owns 512 positions


def dgrad_accumulators(cin):
    """The CI of the pointwise_dgrad_kernel instantiation mvp_pointwise_dgrad launches; 32 runs two passes over gy."""
    return 8 if cin <= 8 else 16 if cin <= 16 else 24 if cin <= 24 else 48 if cin <= 48 else 32


def _dgrad_shapes():
    """Every cin with cout = 64 and with cout <= 2, the lengths and b in {1, 3} dealt round: every length meets both."""
    shapes = []
    for i, cin in enumerate(DGRAD_CINS):
        shapes.append(((1, 3)[i % 2], cin, 64, DGRAD_LENS[i % 4]))
        shapes.append(((3, 1)[i % 2], cin, (1, 2)[(i // 2) % 2], DGRAD_LENS[(i + 1) % 4]))
    return tuple(shapes)


DGRAD_SHAPES = _dgrad_shapes()                     # (b, cin, cout, len)


def ref_small_dgrad(w, gy):
    """w (cout, cin), gy (b, cout, len) -> gx[b, ci, l] = sum_co w[co, ci] gy[b, co, l] and its mag, float64."""
    wd, gd = w.double(), gy.double()
    return {"gx": torch.einsum("oi,bol->bil", wd, gd), "gx_mag": torch.einsum("oi,bol->bil", wd.abs(), gd.abs())}


DgradCase = namedtuple("DgradCase", "shape w gy ref")


@functools.lru_cache(maxsize=8)
def dgrad_case(shape, family):
    b, cin, cout, length = shape
    gen = torch.Generator().manual_seed(7)
    w = values((cout, cin), family, gen)
    gy = values((b, cout, length), family, gen)
    ref = ref_small_dgrad(w, gy)
    if family == "exact":
        assert_exactly_representable(ref)
    return DgradCase(shape, w, gy, ref)


# ---------------------------------------------------------------------------------------------------------------- the two checks

def assert_equal(got, want, what):
    """Bit for bit on the values: got.double() EQUALS the float64 reference (a NaN left in `got` fails)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not bool(torch.isnan(got).any()), "%s: %d entries left unwritten" % (what, int(torch.isnan(got).sum()))
    wrong = got.double() != want
    assert not bool(wrong.any()), "%s: %d of %d entries differ, the first at %s, by at most %g" % (
        what, int(wrong.sum()), wrong.numel(), tuple(wrong.nonzero()[0].tolist()), float((got.double() - want).abs().max()))


def assert_within(got, want, mag, terms, what):
    """Every element: |got - want| <= gamma_terms * mag; `terms` a number or a tensor that broadcasts.  Prints the largest
    share of the bound in use.  Where the bound is 0 (no term, or one number and no addition) the result must be equal."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not bool(torch.isnan(got).any()), "%s: %d entries left unwritten" % (what, int(torch.isnan(got).sum()))
    err = (got.double() - want).abs()
    bound = gamma(terms) * mag
    share = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    print("share of bound %s: %.4f" % (what, float(share.max()) if share.numel() else 0.0))
    over = err > bound
    assert not bool(over.any()), "%s: %d of %d entries over the bound, the first at %s: error %g, bound %g" % (
        what, int(over.sum()), over.numel(), tuple(over.nonzero()[0].tolist()), float(err[over][0]), float(bound[over][0]))
