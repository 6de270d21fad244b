"""Host side of the fused edge MLP (no GPU): mvp_edge_mlp_max's guards through the loaded library with null pointers, the
binding, the switch, DGCNN's routing function, the torch composition of the wrapper against a case worked by hand, and the
rounding bound of the GPU tests checked on the float32 torch composition (so the bound is one the reference formulation
itself meets, with room, and is not vacuous)."""
import ctypes

import pytest
import torch

import edge_mlp_cases as cases
from dcp_util import OpLayerTensor, load_dcp

OK, EBADSHAPE, EBADARG = 0, -1, -2


def _entry():
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    # (b, c, n, k, stages, w1..w4), x .. out, stream
    return lambda b, c, n, k, stages, *w, ptr=null: lib.mvp_edge_mlp_max(b, c, n, k, stages, *w, *([ptr] * 6), null)


def test_shape_guards_and_null_buffers():
    fn = _entry()
    dummy = ctypes.c_void_p(4096)
    good = (2, 3, 50, 20, 4, 64, 64, 128, 256)
    assert fn(*good) == EBADARG                                  # covered: the null buffers are what is wrong
    for bad_w in (48, 288, 0, -32):                              # a used width
        for slot in range(4):
            w = list(good[5:])
            w[slot] = bad_w
            assert fn(*good[:5], *w) == EBADSHAPE, (bad_w, slot)
            assert fn(*good[:5], *w, ptr=dummy) == EBADSHAPE      # shape refusals come first
    assert fn(2, 3, 50, 20, 2, 64, 64, 32, 0) == EBADSHAPE       # non-zero in an unused slot
    assert fn(2, 3, 50, 20, 1, 64, 0, 0, 32) == EBADSHAPE
    assert fn(2, 3, 50, 20, 0, 0, 0, 0, 0) == EBADSHAPE          # stages
    assert fn(2, 3, 50, 20, 5, 64, 64, 64, 64) == EBADSHAPE
    assert fn(2, 0, 50, 20, 1, 64, 0, 0, 0) == EBADSHAPE         # c
    assert fn(2, 5, 50, 20, 1, 64, 0, 0, 0) == EBADSHAPE
    assert fn(2, 3, 50, 0, 1, 64, 0, 0, 0) == EBADSHAPE          # k
    assert fn(2, 3, 50, 65, 1, 64, 0, 0, 0) == EBADSHAPE
    assert fn(-1, 3, 50, 20, 1, 64, 0, 0, 0) == EBADSHAPE and fn(2, 3, -1, 20, 1, 64, 0, 0, 0) == EBADSHAPE
    assert fn(0, 3, 50, 65, 1, 64, 0, 0, 0) == EBADSHAPE         # ... also in front of the empty batch
    for stages in (1, 2, 3, 4):
        for wd in (32, 96, 256):
            for c in (1, 4):
                for k in (1, 64):
                    w = [wd] * stages + [0] * (4 - stages)
                    assert fn(2, c, 300, k, stages, *w) == EBADARG
                    assert fn(0, c, 300, k, stages, *w) == OK and fn(2, c, 0, k, stages, *w) == OK   # nothing to do
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    ptrs = [dummy] * 6
    for missing in range(6):                                     # each buffer on its own
        p = [ctypes.c_void_p(0) if i == missing else dummy for i in range(6)]
        assert lib.mvp_edge_mlp_max(*good, *p, ctypes.c_void_p(0)) == EBADARG, missing
    ptrs[2] = ctypes.c_void_p(4100)                              # the weights are read 16 bytes at a time
    assert lib.mvp_edge_mlp_max(*good, *ptrs, ctypes.c_void_p(0)) == EBADARG


def test_binding_lists_the_entry_point():
    from mvp_benchmark_amd import _lib
    assert _lib.ABI_VERSION >= 22
    assert len(_lib.SIGNATURES["mvp_edge_mlp_max"]) == 15 and _lib.SIGNATURES["mvp_edge_mlp_max"] == "i" * 9 + "p" * 6
    assert "mvp_edge_mlp_max" in _lib.exported_symbols()


def test_switch_defaults_to_off():
    from mvp_benchmark_amd import registration
    assert registration.EDGE_MLP is False


def test_routing_function(monkeypatch):
    dcp = load_dcp("edge_mlp_cpu")
    from mvp_benchmark_amd import registration
    net = dcp.DGCNN().eval()
    x_gpu, x_cpu = OpLayerTensor(2, 3, 64), torch.zeros(2, 3, 64)
    with torch.no_grad():
        assert net._route(x_gpu) == "composed"                        # the switch is off
    monkeypatch.setattr(registration, "EDGE_MLP", True)
    with torch.no_grad():
        assert net._route(x_gpu) == "edge_mlp"
        assert net._route(x_cpu) == "composed"                        # CPU
        assert net.double()._route(x_cpu.double()) == "composed"      # float64
        net.float()
        assert net._route(OpLayerTensor(2, 3, 66)) == "composed"     # rows that are no whole 16-byte groups (conv5's GEMM)
        assert net._route(OpLayerTensor(2, 5, 64)) == "composed"     # more channels than the kernel gathers
        net.train()
        assert net._route(x_gpu) == "composed"                        # batch statistics
        net.eval()
    assert net._route(x_gpu) == "composed"                            # grad mode and the parameters require grad
    wants = OpLayerTensor(2, 3, 64)
    wants.requires_grad = True
    for p in net.parameters():
        p.requires_grad_(False)
    assert net._route(x_gpu) == "edge_mlp" and net._route(wants) == "composed"
    with torch.no_grad():
        assert net._route(wants) == "edge_mlp"


def test_cpu_and_float64_take_the_composed_route_whatever_the_switch(monkeypatch):
    dcp = load_dcp("edge_mlp_cpu")
    from mvp_benchmark_amd import registration
    torch.manual_seed(3)
    net = dcp.DGCNN().double().eval()
    x = torch.randn(2, 3, 32, dtype=torch.float64)
    with torch.no_grad():
        off = net(x)
        monkeypatch.setattr(registration, "EDGE_MLP", True)
        on = net(x)
    assert torch.equal(on, off)


def test_reference_route_on_a_case_worked_by_hand():
    """One cloud of two points x = (1, -2), c = 1, two slots, one stage of 32 channels of which channel 0 is live:
    W[0] = (1, 1) (neighbour + centre), scale[0] = -1, shift[0] = 0.5; the other rows are 0 with scale 1, shift 0.
      point 0 (centre 1), slots (1, 0): neighbours -2, 1 -> sums -1, 2 -> -1 * s + 0.5 = 1.5, -1.5 -> ReLU 1.5, 0 -> max 1.5
      point 1 (centre -2), slots (0, 0): neighbours 1, 1 -> sums -1, -1 -> 1.5, 1.5: a tie over k                -> max 1.5
    (the negative scale turns the smaller sum into the maximum)."""
    from mvp_benchmark_amd.registration import edge_mlp_max
    for dtype in (torch.float64, torch.float32):
        x = torch.tensor([[[1.0, -2.0]]], dtype=dtype)
        idx = torch.tensor([[[1, 0], [0, 0]]], dtype=torch.int32)          # (B, k, N): slot 0 = (1, 0), slot 1 = (0, 0)
        W = torch.zeros(32, 2, dtype=dtype)
        W[0] = 1.0
        scale, shift = torch.ones(32, dtype=dtype), torch.zeros(32, dtype=dtype)
        scale[0], shift[0] = -1.0, 0.5
        out = edge_mlp_max(x, idx, [W], [scale], [shift])
        want = torch.zeros(1, 32, 2, dtype=dtype)
        want[0, 0] = 1.5
        assert out.dtype == dtype and torch.equal(out, want)
        assert torch.equal(cases.reference(x, idx, [W], [scale], [shift])["out"], want.double())
        assert torch.equal(edge_mlp_max(x, idx, [W.view(32, 2, 1, 1)], [scale], [shift]), want)   # a convolution's weight
    # forward only
    with pytest.raises(AssertionError):
        edge_mlp_max(x, idx, [W.requires_grad_()], [scale], [shift])
    with torch.no_grad():
        assert torch.equal(edge_mlp_max(x, idx, [W], [scale], [shift]), want)
    with pytest.raises(AssertionError):                                     # widths that do not chain
        edge_mlp_max(x, idx, [W.detach(), torch.zeros(32, 64)], [scale] * 2, [shift] * 2)


@pytest.mark.parametrize("pattern", cases.PATTERNS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_float32_composition_stays_inside_the_bound(shape, pattern):
    """The bound the GPU tests hold the kernel to, asserted on the float32 torch composition on the CPU."""
    from mvp_benchmark_amd.registration import edge_mlp_max
    case = cases.make_case(shape, pattern, "random")
    ref = cases.reference(**case)
    assert float(ref["mag"].max()) < float("inf")
    share = cases.bound_share(cases.compose(**case), ref)
    print("float32 composition %s %s: %.3f of the bound" % (shape, pattern, share))
    assert share <= 1.0
    with torch.no_grad():
        assert cases.bound_share(edge_mlp_max(**case), ref) <= 1.0          # the wrapper's CPU route


@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_exact_cases_stay_below_2_to_24(shape):
    """The premise of the exact GPU cases: every intermediate is an integer that float32 holds."""
    for pattern in cases.PATTERNS:
        case = cases.make_case(shape, pattern, "exact")
        ref = cases.reference(**case)
        assert float(ref["mag"].max()) < 2.0 ** 24
        assert torch.equal(ref["out"], ref["out"].round())
        assert torch.equal(cases.compose(**case).double(), ref["out"])     # so float32 must reproduce it bit for bit
