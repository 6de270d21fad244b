"""The 1x1-convolution gradient kernels off the MFMA path, without a GPU: the references of tests/conv_gradient_cases.py
against float64 autograd of the functions they describe, the case lists against the edges they claim (the exact family's
range, the patterns' fit, the weight gradient's launch plan, the data gradient's instantiations), and the host guards of
mvp_pointwise_max_backward, its _scratch_bytes and mvp_pointwise_dgrad."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_gradient_cases as cg

OK, EBADSHAPE, EBADARG = 0, -1, -2


# ------------------------------------------------------------------------------------------- the references are the gradients

def autograd_max_backward(x, w, g, idx, chunk=256):
    """Gradients of sum(g * v), v[b, co] = (conv1d(x, w) + bias)[b, co, idx[b, co]]: conv(x).max(2) with the gradient routed
    to the given positions.  The output channels go through in chunks (the (b, cout, len) tensor of the largest shape is
    1 GiB in float64)."""
    xd, wd, gd = x.double().requires_grad_(), w.double().requires_grad_(), g.double()
    bias = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    for c0 in range(0, w.shape[0], chunk):
        y = F.conv1d(xd, wd[c0:c0 + chunk].unsqueeze(2), bias[c0:c0 + chunk])
        v = y.gather(2, idx[:, c0:c0 + chunk].long().unsqueeze(2)).squeeze(2)
        (v * gd[:, c0:c0 + chunk]).sum().backward()
    return xd.grad, wd.grad, bias.grad


@pytest.mark.parametrize("family", cg.FAMILIES)
def test_max_backward_reference_is_the_gradient(family):
    """Every shape and pattern: equal for the integers, at float64 rounding for randn."""
    for shape, pattern in cg.max_cases():
        case = cg.max_case(shape, pattern, family)
        gx, gw, gb = autograd_max_backward(case.x, case.w, case.g, case.idx)
        for name, got in (("gx", gx), ("gw", gw), ("gb", gb)):
            want = case.ref[name]
            if family == "exact":
                assert torch.equal(got, want), (shape, pattern, name)
            else:
                assert bool(((got - want).abs() <= 1e-13 * case.ref[name + "_mag"]).all()), (shape, pattern, name)
        b, cin, cout, length = shape
        count = case.ref["count"]
        assert count.shape == (b, length) and bool((count.sum(1) == cout).all())
        assert bool((case.ref["gx_mag"][count.unsqueeze(1).expand(b, cin, length) == 0] == 0).all())


def test_max_backward_reference_on_a_real_maximum():
    """With idx what torch.max reports, the reference is the gradient of conv(x).max(2)[0] itself."""
    gen = torch.Generator().manual_seed(1)
    x, w, g = torch.randn(3, 5, 33, generator=gen), torch.randn(7, 5, generator=gen), torch.randn(3, 7, generator=gen)
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    v, idx = F.conv1d(xd, wd.unsqueeze(2)).max(2)
    gx, gw = torch.autograd.grad(v, (xd, wd), g.double())
    ref = cg.ref_max_backward(x, w, g, idx.int())
    assert bool(((gx - ref["gx"]).abs() <= 1e-13 * ref["gx_mag"]).all())
    assert bool(((gw - ref["gw"]).abs() <= 1e-13 * ref["gw_mag"]).all())


@pytest.mark.parametrize("family", cg.FAMILIES)
def test_small_references_are_the_gradients_of_conv1d(family):
    tol = 0.0 if family == "exact" else 1e-13
    for shape, _, _ in cg.WGRAD_SHAPES:
        case = cg.wgrad_case(shape, family)
        cout, cin = shape[2], shape[1]
        xd = case.x.double()
        wd = torch.zeros(cout, cin, 1, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        gw, gb = torch.autograd.grad(F.conv1d(xd, wd, bias), (wd, bias), case.gy.double())
        assert bool(((gw.squeeze(2) - case.ref["gw"]).abs() <= tol * case.ref["gw_mag"]).all()), shape
        assert bool(((gb - case.ref["gb"]).abs() <= tol * case.ref["gb_mag"]).all()), shape
    for shape in cg.DGRAD_SHAPES:
        case = cg.dgrad_case(shape, family)
        b, cin, cout, length = shape
        xd = torch.zeros(b, cin, length, dtype=torch.float64, requires_grad=True)
        gx, = torch.autograd.grad(F.conv1d(xd, case.w.double().unsqueeze(2)), (xd,), case.gy.double())
        assert bool(((gx - case.ref["gx"]).abs() <= tol * case.ref["gx_mag"]).all()), shape


def test_the_bound_tells_a_dropped_term():
    """What the old tolerance (1e-4 of the largest entry) let through: the weight gradient of (2, 5, 5, 1028) without its last
    float4 of positions is over gamma_t * mag, and, in the exact family, not equal."""
    shape = (2, 5, 5, 1028)
    for family in cg.FAMILIES:
        case = cg.wgrad_case(shape, family)
        short = cg.ref_small_wgrad(case.x[..., :-4], case.gy[..., :-4])
        bound = cg.gamma(shape[0] * shape[3]) * case.ref["gw_mag"]
        err = (short["gw"] - case.ref["gw"]).abs()
        if family == "random":
            assert int((err > bound).sum()) > err.numel() // 2
        else:
            assert not torch.equal(short["gw"], case.ref["gw"])


# --------------------------------------------------------------------------------------------- the case lists hit their edges

def test_exact_family_stays_below_2_to_24():
    """The generators assert it; here every exact case is generated.  The worst case by the shapes alone: 16 per term."""
    for shape, pattern in cg.max_cases():
        ref = cg.max_case(shape, pattern, "exact").ref
        assert max(float(ref[k].max()) for k in ("gw_mag", "gb_mag", "gx_mag")) < cg.EXACT_LIMIT
        assert 16 * max(shape[0], shape[2]) < cg.EXACT_LIMIT
    for shape, _, _ in cg.WGRAD_SHAPES:
        assert shape[0] * shape[3] <= cg.WGRAD_MAX_POSITIONS
        ref = cg.wgrad_case(shape, "exact").ref
        assert max(float(ref["gw_mag"].max()), float(ref["gb_mag"].max())) < cg.EXACT_LIMIT
    for shape in cg.DGRAD_SHAPES:
        assert float(cg.dgrad_case(shape, "exact").ref["gx_mag"].max()) < cg.EXACT_LIMIT
    with pytest.raises(AssertionError):
        cg.assert_exactly_representable({"gw_mag": torch.tensor([2.0 ** 24])})


def test_patterns_fit_their_shapes():
    seen = set()
    for shape, pattern in cg.max_cases():
        b, cin, cout, length = shape
        idx = cg.max_case(shape, pattern, "exact").idx
        assert idx.dtype == torch.int32 and idx.shape == (b, cout)
        assert 0 <= int(idx.min()) and int(idx.max()) < length
        count = cg.max_case(shape, pattern, "exact").ref["count"]
        kind = "one_position" if pattern.startswith("one_position_") else pattern
        seen.add(kind)
        if kind == "one_position":
            p = int(pattern.rsplit("_", 1)[1])
            assert p in (0, min(31, length - 1), min(32, length - 1), length - 1)
            assert bool((count[:, p] == cout).all())
        elif kind == "one_each":
            assert cout == length and bool((count == 1).all())
        elif kind == "tile_edges":
            allowed = torch.zeros(length, dtype=torch.bool)
            allowed[cg.tile_edge_positions(length)] = True
            assert bool((count[:, ~allowed] == 0).all())
            assert cout < 64 or bool((count[:, allowed] > 0).all())   # with channels enough, every edge in every cloud
        elif kind == "runs_9_17":
            runs = cg._run_lengths(cout)
            assert runs[:2] == [9, 17] and sum(runs) == cout           # 8 k + 1 channels: the tail of the 8-wide loop
            for row in count:                                         # every cloud: the runs, in the order of their positions
                assert row[row > 0].tolist() == runs
            assert torch.equal(idx[0].sort()[0], idx[0])              # cloud 0: dealt in channel order
        elif kind == "descending":
            assert bool((idx[:, 1:] <= idx[:, :-1]).all()) and int(idx[0, 0]) > int(idx[0, -1])
    assert seen == {"random", "one_position", "one_each", "tile_edges", "runs_9_17", "descending"}
    # the positions the issue names, wherever the shape has them
    assert cg.one_positions(257) == [0, 31, 32, 256] and cg.one_positions(20) == [0, 19] and cg.one_positions(1) == [0]
    assert cg.patterns_for((2, 64, 64, 64)).count("one_each") == 1
    assert "one_each" not in cg.patterns_for((3, 5, 2, 33))


def test_max_shapes_sit_on_the_edges_they_name():
    shapes = [s for s, _ in cg.MAX_SHAPES]
    assert len(shapes) == 8 and len(set(shapes)) == 8
    assert cg.max_lds_bytes((2, 7, 2048, 1356)) == 30000 and cg.max_lds_bytes((2, 7, 2049, 1353)) == 30000
    assert cg.cout_p2(2048) == 2048 and cg.cout_p2(2049) == 4096 and cg.cout_p2(1) == 1 and cg.cout_p2(33) == 64
    assert [cg.takes_gx(s) for s in shapes] == [True] * 7 + [False]
    assert shapes[-1][2:] == (4096, 16384)                                        # the header's maxima
    assert any(b > 8 and b % 8 for b, _, _, _ in shapes)                          # the 8-wide loop over the clouds and its tail
    assert any(cin > 256 for _, cin, _, _ in shapes) and any(64 < cin < 128 for _, cin, _, _ in shapes)
    assert any(256 < length <= 512 for _, _, _, length in shapes)                 # two positions per thread in the scan
    assert any(length % 32 == 1 for _, _, _, length in shapes)


def test_wgrad_shapes_have_the_plans_they_record():
    plans = {}
    for shape, plan, edge in cg.WGRAD_SHAPES:
        b, cin, cout, length = shape
        assert cg.pw_plan(cin, cout) == plan, (shape, cg.pw_plan(cin, cout))
        assert length % 4 == 0 and cout <= 64 and edge
        assert plan.cog * plan.cig * plan.pg <= 256 and 4 * (plan.cog + plan.cig) <= 224
        plans[shape] = plan
    lengths = sorted(s[3] for s in plans if s[:3] == (2, 5, 5))
    assert lengths == [4, 60, 64, 68, 1020, 1024, 1028, 2052]
    assert plans[(3, 1, 1, 64)].pg == 16 and 256 // (1 * 1) > 16                  # the cap, not the thread count
    p = plans[(2, 28, 9, 128)]
    assert p.cog * p.cig == 21 and p.pg == 12 and 16 % p.pg != 0
    p = plans[(2, 130, 33, 68)]
    assert p.cog * p.cig * p.pg == 252
    p = plans[(2, 65, 64, 64)]
    assert p.chunks == 2 and 65 - 4 * p.cig == 1
    p = plans[(1, 221, 4, 8)]
    assert p.chunks == 2 and p.cog == 1 and p.cig == 224 // 4 - 1                  # the LDS rows cap the channel block
    assert cg.pw_plan(24, 24) == cg.Plan(6, 6, 7, 1) and cg.pw_plan(64, 64) == cg.Plan(16, 16, 1, 1)


def test_dgrad_shapes_cover_every_width_and_length():
    shapes = cg.DGRAD_SHAPES
    assert len(set(shapes)) == len(shapes) == 2 * len(cg.DGRAD_CINS)
    for wide in (True, False):
        part = [s for s in shapes if (s[2] == 64) == wide]
        assert sorted(s[1] for s in part) == list(cg.DGRAD_CINS)
        assert {s[3] for s in part} == set(cg.DGRAD_LENS)
        assert {s[0] for s in part} == {1, 3}
        assert all(s[2] in ((64,) if wide else (1, 2)) for s in part)
    assert {s[2] for s in shapes} == {1, 2, 64}
    assert {cg.dgrad_accumulators(c) for c in cg.DGRAD_CINS} == {8, 16, 24, 48, 32}
    for below, above in ((8, 9), (16, 17), (24, 25), (48, 49)):                   # both sides of every dispatch edge
        assert cg.dgrad_accumulators(below) != cg.dgrad_accumulators(above)
    assert [c for c in cg.DGRAD_CINS if cg.dgrad_accumulators(c) == 32 and c % 32] == [49, 50, 63]   # a ragged second pass


# --------------------------------------------------------------------------------------------------------------- host guards

def test_guards_of_the_max_backward_entry_point():
    """Every row returns before a launch: a shape guard refuses, or an argument guard behind it."""
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)

    def run(shape, x=some, w=some, g=some, idx=some, gx=null, gw=null, gb=null, scratch=null, nbytes=0):
        return lib.mvp_pointwise_max_backward(*shape, x, w, g, idx, gx, gw, gb, scratch, nbytes, null)

    # a dimension that is not positive, whatever the pointers are
    for shape in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, 4, 4, -1)):
        assert run(shape, gx=some, gw=some, gb=some) == EBADSHAPE, shape
        assert run(shape, g=null, idx=null) == EBADSHAPE, shape
    # the limits: the shape is accepted (the missing g is what is wrong) up to them, refused one above -- first of all
    for at, above in (((1, 1, 1, 16384), (1, 1, 1, 16385)), ((1, 1, 4096, 1), (1, 1, 4097, 1)), ((65535, 1, 1, 1), (65536, 1, 1, 1))):
        assert run(at, g=null, gw=some) == EBADARG, at
        assert run(above, g=null, gw=some) == EBADSHAPE, above
        assert run(above, gw=some) == EBADSHAPE, above
    # the sort's LDS: (3 cout + len) * 4 <= 30000 where gx is wanted, no limit where it is not
    for at, above in (((2, 7, 2048, 1356), (2, 7, 2048, 1357)), ((2, 7, 2049, 1353), (2, 7, 2049, 1354)),
                      ((2, 7, 1, 7497), (2, 7, 1, 7498)), ((2, 7, 2499, 3), (2, 7, 2500, 1))):
        assert cg.max_lds_bytes(at) == 30000 and cg.max_lds_bytes(above) > 30000
        assert run(at, gx=some, g=null) == EBADARG, at
        assert run(above, gx=some, g=null) == EBADSHAPE, above
        assert run(above, gx=some, gw=some, gb=some) == EBADSHAPE, above
        assert run(above, gw=some, gb=some, g=null) == EBADARG, above               # without gx: accepted
    assert run((2, 5, 4096, 16384), gx=some) == EBADSHAPE
    assert run((2, 5, 4096, 16384), gw=some, idx=null) == EBADARG
    # the arguments, on an accepted shape: g and idx always, x for gw, w for gx -- and nothing else
    shape = (2, 3, 4, 5)
    for out in ("gx", "gw", "gb"):
        assert run(shape, g=null, **{out: some}) == EBADARG, out
        assert run(shape, idx=null, **{out: some}) == EBADARG, out
    assert run(shape, x=null, gw=some) == EBADARG and run(shape, x=null, gw=some, gx=some, gb=some) == EBADARG
    assert run(shape, w=null, gx=some) == EBADARG and run(shape, w=null, gx=some, gw=some, gb=some) == EBADARG


def test_scratch_bytes_of_the_max_backward():
    from mvp_benchmark_amd import _lib
    need = _lib.pointwise_max_backward_scratch_bytes
    assert need(2, 3, 4, 5) == 2 * 4 * 3 * 4 and need(1, 1, 1, 1) == 4
    for shape, _ in cg.MAX_SHAPES:
        b, cin, cout, length = shape
        assert need(*shape) == (b * cout * cin * 4 if cg.takes_gx(shape) else 0), shape
    assert need(2, 7, 2048, 1356) == 2 * 2048 * 7 * 4 and need(2, 7, 2048, 1357) == 0      # both sides of the LDS guard
    assert need(2, 7, 2049, 1353) > 0 and need(2, 7, 2049, 1354) == 0
    assert need(1, 1, 1, 7497) == 4 and need(1, 1, 1, 7498) == 0
    for shape in ((0, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (2, 3, 4, 0), (-1, 3, 4, 5), (1, 1, 1, 16385), (1, 1, 4097, 1)):
        assert need(*shape) == 0, shape
    assert need(65535, 1, 1, 1) == 65535 * 4
    assert need(65535, 512, 1024, 2048) == 65535 * 1024 * 512 * 4                        # above 2^31 bytes: not truncated


def test_guards_of_the_small_data_gradient():
    """mvp_pointwise_dgrad: cin, cout <= 64, len % 4 == 0, b <= 65535 (shape, answered first); every pointer given, gy and gx
    on the 16-byte grid (arguments)."""
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    null, some, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    def run(shape, w=some, gy=some, gx=some):
        return lib.mvp_pointwise_dgrad(*shape, w, gy, gx, null)

    for shape in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -4),
                  (1, 65, 4, 4), (1, 4, 65, 4), (1, 4, 4, 5), (1, 4, 4, 6), (1, 4, 4, 7), (65536, 4, 4, 4)):
        assert run(shape) == EBADSHAPE, shape
        assert run(shape, null, null, null) == EBADSHAPE, shape                  # the shape is answered first
    for shape in ((1, 64, 64, 4), (65535, 1, 1, 4), (3, 49, 2, 516)):                # at the limits: the arguments are what is wrong
        assert run(shape, w=null) == EBADARG and run(shape, gy=null) == EBADARG and run(shape, gx=null) == EBADARG, shape
        assert run(shape, gy=odd) == EBADARG and run(shape, gx=odd) == EBADARG, shape
        assert run(shape, null, odd, odd) == EBADARG, shape
