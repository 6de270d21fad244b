"""Host side of the split-K route of the pointwise MFMA kernels (mvp_pointwise_mfma_splitk*, ABI 20; the selector
MFMA_SPLIT_K and the planners of mvp_benchmark_amd/pointwise.py).  No GPU: the plan and the scratch query are pure host
functions, the entry point refuses bad arguments before it launches anything, the planners work on hand-built Layers."""
import ctypes
import itertools

import pytest

EBADSHAPE, EBADARG = -1, -2
# (B, cin, cout, L) of ECG's bottleneck layers: the GEMMs _gemm_fits refuses (tests/test_host.py)
ECG_BOTTLENECKS = [(32, 2824, 1024, 64), (32, 1800, 1024, 64), (32, 1864, 768, 256)]


def _splits(cin, chunk):
    return -(-cin // chunk)


def test_plan_gives_a_chunk_of_whole_slabs_or_none():
    from mvp_benchmark_amd import _lib
    plan = _lib.pointwise_mfma_splitk_plan
    nonzero = 0
    for b, cin, cout, length in itertools.product((1, 2, 8, 32, 64, 600), (1, 64, 512, 513, 520, 640, 1029, 1864, 2824, 8192, 100000),
                                                  (1, 16, 64, 65, 520, 768, 1024), (4, 60, 64, 68, 128, 132, 256, 2048)):
        chunk = plan(b, cin, cout, length)
        assert chunk >= 0 and chunk % 16 == 0, (b, cin, cout, length, chunk)
        if cin <= 512:
            assert chunk == 0, (b, cin, cout, length, chunk)
        if chunk:
            nonzero += 1
            assert 2 <= _splits(cin, chunk) <= 32, (b, cin, cout, length, chunk)
            assert chunk >= 128, (b, cin, cout, length, chunk)          # (cin / 128 chunks at the most)
    assert nonzero > 100
    # bad shapes: nothing to split
    assert plan(0, 1864, 768, 256) == 0 and plan(32, 1864, 768, 254) == 0 and plan(32, 1864, 0, 256) == 0
    assert plan(65536, 1864, 8, 4) == 0


def test_plan_leaves_what_the_plain_kernel_fits_and_splits_the_bottlenecks():
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd import pointwise as pw
    plan = _lib.pointwise_mfma_splitk_plan
    for b, cin, cout, length in ((32, 1029, 512, 16384), (64, 512, 512, 384)):
        assert pw._gemm_fits(b, cout, cin, length) and plan(b, cin, cout, length) == 0
    for b, cin, cout, length in ECG_BOTTLENECKS:
        assert not pw._gemm_fits(b, cout, cin, length)
        chunk = plan(b, cin, cout, length)
        assert chunk > 0 and chunk % 16 == 0 and 2 <= _splits(cin, chunk) <= 32, (b, cin, cout, length, chunk)
    # the heuristic, by hand: 8 x 1 x 32 = 256 tiles of 128 x 64 -> 2 chunks of ceil(2824 / 2) = 1412 -> 1424;
    # 6 x 2 x 32 = 384 tiles -> 2 chunks of 932 -> 944; 5 tiles x 2 clouds -> min(52, 520 / 128 = 4, 16) chunks of 130 -> 144
    assert plan(32, 2824, 1024, 64) == 1424 and plan(32, 1864, 768, 256) == 944 and plan(2, 520, 520, 64) == 144
    assert plan(1, 8192, 64, 64) == 512                                   # the cap of 16 chunks


def test_scratch_bytes_is_the_formula_and_zero_for_a_refused_call():
    from mvp_benchmark_amd import _lib
    nbytes = _lib.pointwise_mfma_splitk_scratch_bytes
    for b, cin, cout, length, chunk in ((32, 1864, 768, 256, 944), (3, 50, 70, 132, 32), (1, 512, 32, 8, 16), (2, 40, 64, 64, 16),
                                        (7, 513, 1, 4, 32), (2, 48, 72, 132, 64)):
        assert nbytes(b, cin, cout, length, chunk) == _splits(cin, chunk) * b * cout * length * 4
    assert nbytes(65535, 4096, 1024, 1024, 128) == 32 * 65535 * 1024 * 1024 * 4       # (64-bit: 8.8e12)
    assert nbytes(3, 50, 70, 132, 24) == 0 and nbytes(3, 50, 70, 132, 0) == 0 and nbytes(3, 50, 70, 132, -16) == 0
    assert nbytes(1, 513, 32, 8, 16) == 0                                  # 33 chunks
    assert nbytes(3, 50, 70, 130, 32) == 0 and nbytes(0, 50, 70, 132, 32) == 0 and nbytes(65536, 50, 70, 132, 32) == 0


def test_entry_point_refuses_before_it_launches():
    """Null / made-up pointers throughout: every call must come back with its error code from the argument checks."""
    from mvp_benchmark_amd import _lib
    fn = _lib.load().mvp_pointwise_mfma_splitk
    null = None
    fake = ctypes.c_void_p(1 << 20)                 # never dereferenced: the calls below are refused before any launch

    def call(b=3, cin=50, cout=70, length=132, x=null, xmask=null, w=null, flags=0, y=null, k_chunk=32, scratch=null, nbytes=0,
             residual=null, bias=null, per_cloud=0):
        return fn(b, cin, cout, length, x, xmask, w, 0, 0, bias, per_cloud, residual, flags, y, k_chunk, scratch, nbytes, null)

    assert call(k_chunk=24) == EBADARG and call(k_chunk=0) == EBADARG and call(k_chunk=-16) == EBADARG
    assert call(k_chunk=24, x=fake, w=fake, y=fake, scratch=fake, nbytes=1 << 40) == EBADARG
    assert call(cin=513, k_chunk=16) == EBADSHAPE                          # 33 chunks
    assert call(cin=513, k_chunk=16, x=fake, w=fake, y=fake, scratch=fake, nbytes=1 << 40) == EBADSHAPE
    assert call(length=130) == EBADSHAPE
    assert call(flags=16) == EBADARG                                       # unknown flag
    assert call(flags=8, xmask=fake) == EBADARG                            # MVP_PW_X_RELU with an xmask
    assert call(flags=4) == EBADARG                                        # MVP_PW_RES_IS_MASK without a residual
    assert call(per_cloud=1) == EBADARG                                    # a bias per cloud without a bias
    assert call(b=65536) == EBADSHAPE and call(cout=0) == EBADSHAPE
    # two chunks: scratch null / misaligned / too small
    need = _lib.pointwise_mfma_splitk_scratch_bytes(3, 50, 70, 132, 32)
    assert need == 2 * 3 * 70 * 132 * 4
    assert call(x=fake, w=fake, y=fake, scratch=null, nbytes=need) == EBADARG
    assert call(x=fake, w=fake, y=fake, scratch=ctypes.c_void_p((1 << 20) + 4), nbytes=need) == EBADARG
    assert call(x=fake, w=fake, y=fake, scratch=fake, nbytes=need - 1) == EBADARG
    # the plain call's pointer refusals
    assert call(scratch=fake, nbytes=need) == EBADARG                      # x, w, y null
    assert call(x=ctypes.c_void_p((1 << 20) + 4), w=fake, y=fake, scratch=fake, nbytes=need) == EBADARG
    # one chunk is the plain entry point: its refusals, and an empty batch is a no-op
    assert call(k_chunk=64, length=130) == EBADSHAPE and call(k_chunk=64) == EBADARG
    assert call(b=0) == 0 and call(b=0, k_chunk=64) == 0


def _layer(pw, b, cin, cout, length, **kw):
    d = pw.Layer(cuda=True, f32=True, dim=3, B=b, cin=cin, cout=cout, L=length, x_dense=True, w_dense=True, x_aligned=True,
                 w_aligned=True, nonempty=True)
    return d._replace(**kw)


SELECTORS = ("MFMA_SPLIT_K", "MFMA_WGRAD_MIN_POSITIONS", "LIBRARY_IS_GEMM", "USE_MFMA", "MFMA_DGRAD", "MFMA_TRAIN")


def _plans(pw):
    """Every planner on the layers of this file -> a comparable record."""
    out = {}
    layers = ECG_BOTTLENECKS + [(2, 520, 520, 64), (8, 544, 16, 384), (2, 1864, 768, 64), (64, 512, 512, 384), (32, 1029, 512, 16384)]
    for b, cin, cout, length in layers:
        d = _layer(pw, b, cin, cout, length)
        for grad in (False, True):
            plan = pw._plan_conv(d, grad)
            out[(b, cin, cout, length, "conv", grad)] = (plan.via, plan.fwd)
        for relu in (False, True):
            out[(b, cin, cout, length, "back", relu)] = tuple(pw._plan_conv_backward(d, relu, True, True, True, True))
        for need_x in (False, True):
            out[(b, cin, cout, length, "fused", need_x)] = pw._plan_fused(d, need_x)
        out[(b, cin, cout, length, "dual")] = pw._plan_dual(d, d._replace(cout=64), True)
        out[(b, cin, cout, length, "max")] = tuple(pw._plan_max(d, True))[:2]
        out[(b, cin, cout, length, "split")] = (pw._split_k(b, cout, cin, length), pw._split_k(b, cin, cout, length))
    return out


def test_planners_route_the_refused_gemms_to_the_split_kernel_only_with_the_selector():
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd import pointwise as pw
    saved = {k: getattr(pw, k) for k in SELECTORS}
    assert saved["MFMA_SPLIT_K"] is False                                   # the default of this route
    try:
        off = _plans(pw)
        # ---- off: today's routes
        for b, cin, cout, length in ECG_BOTTLENECKS:
            assert off[(b, cin, cout, length, "conv", True)] == ("function", "library")
            assert off[(b, cin, cout, length, "conv", False)] == ("none", "library")
            # (the data gradient reduces over cout into cin rows: 15 x 2 x 32 = 960 tiles at 256 points fit the plain kernel)
            assert off[(b, cin, cout, length, "back", True)][0] == ("gemm" if length == 64 else "mfma")
            assert off[(b, cin, cout, length, "split")] == (0, 0)
        assert off[(2, 520, 520, 64, "back", False)][0] == "gemm" and off[(2, 520, 520, 64, "conv", True)] == ("function", "library")
        assert all(v == "composed" for k, v in off.items() if k[4] == "fused" and k[:4] not in ((64, 512, 512, 384), (32, 1029, 512, 16384)))

        pw.MFMA_SPLIT_K = True
        on = _plans(pw)
        for b, cin, cout, length in ECG_BOTTLENECKS:
            d = _layer(pw, b, cin, cout, length)
            assert pw._plan_conv(d, True) == pw.ConvPlan("function", "splitk", d)
            assert pw._plan_conv(d, False) == pw.ConvPlan("none", "splitk", d)
            assert pw._split_k(b, cout, cin, length) == _lib.pointwise_mfma_splitk_plan(b, cin, cout, length) > 0
        # 2824 -> 1024 at 64 points: the data gradient reduces over 1024 into 2824 rows -- 23 x 1 x 32 = 736 tiles, nothing to
        # split, and _gemm_fits refuses it (64 positions): the library's GEMM as today
        d = _layer(pw, 32, 2824, 1024, 64)
        assert not pw._gemm_fits(32, 2824, 1024, 64) and pw._split_k(32, 2824, 1024, 64) == 0
        assert pw._plan_conv_backward(d, True, True, True, True, True).dgrad == "gemm" == off[(32, 2824, 1024, 64, "back", True)][0]
        # 1864 -> 768 at 256 points: 15 x 2 x 32 = 960 tiles for the data gradient: as today too
        assert on[(32, 1864, 768, 256, "back", True)] == off[(32, 1864, 768, 256, "back", True)]
        # 520 -> 520 at 64 points, 2 clouds: both passes split
        d = _layer(pw, 2, 520, 520, 64)
        assert pw._plan_conv(d, True).fwd == "splitk"
        back = pw._plan_conv_backward(d, True, True, True, True, True)
        assert back.dgrad == "splitk" and back.wgrad in ("miopen", "gemm") and back.premask
        assert pw._plan_conv_backward(d._replace(cin=522), False, True, True, True, True).dgrad == "gemm"     # cin % 4
        pw.MFMA_DGRAD = False
        assert pw._plan_conv_backward(d, True, True, True, True, True).dgrad == "gemm"
        pw.MFMA_DGRAD = True
        # the fused entry point needs the MFMA weight gradient as well: not at 128 positions in all ...
        assert pw._plan_fused(d, True) == "composed"
        pw.MFMA_WGRAD_MIN_POSITIONS = 0
        assert pw._plan_fused(d, True) == "fused" and pw._plan_fused(d, False) == "fused"       # ... but where its conditions hold
        assert pw._plan_fused(d._replace(cin=522), True) == "composed" and pw._plan_fused(d._replace(cin=522), False) == "fused"
        assert pw._plan_fused(d, True, relu=True, residual=True) == "composed"
        assert pw._plan_dual(d._replace(cout=512), d._replace(cout=64), True) == "separate"     # no stacked split kernel
        pw.MFMA_SPLIT_K = False
        assert pw._plan_fused(d, True) == "composed"
        pw.MFMA_SPLIT_K = True
        pw.MFMA_WGRAD_MIN_POSITIONS = saved["MFMA_WGRAD_MIN_POSITIONS"]
        # the skinny rule keeps applying: 544 -> 16 stays on the library although its plan would split
        d = _layer(pw, 8, 544, 16, 384)
        assert _lib.pointwise_mfma_splitk_plan(8, 544, 16, 384) > 0 and not pw._gemm_fits(8, 16, 544, 384)
        assert pw._plan_conv(d, True).fwd == "library" and pw._plan_conv(d, False).fwd == "library"
        # tensors the kernels do not take, and the other selectors
        d = _layer(pw, 32, 1864, 768, 256)
        assert pw._plan_conv(d._replace(w_aligned=False), False).fwd == "library"
        assert pw._plan_conv(d._replace(x_dense=False), False).fwd == "library"
        assert pw._plan_conv(d._replace(L=254), False).fwd == "library"
        pw.MFMA_TRAIN = False
        assert pw._plan_conv(d, True).fwd == "library"
        pw.MFMA_TRAIN = True
        pw.USE_MFMA = False
        assert pw._plan_conv(d, False) == pw.ConvPlan("autograd", "library", d)
        pw.USE_MFMA = True
        # what fits is untouched by the selector
        for key, value in on.items():
            if key[:4] in ((64, 512, 512, 384), (32, 1029, 512, 16384)):
                assert value == off[key], key

        # ---- off again: exactly the first record
        pw.MFMA_SPLIT_K = False
        assert _plans(pw) == off
    finally:
        for k, v in saved.items():
            setattr(pw, k, v)


def test_mfma_linear_refuses_a_chunk_with_groups_or_two_outputs():
    import torch
    from mvp_benchmark_amd.pointwise import mfma_linear
    x, w = torch.zeros(1, 32, 8), torch.zeros(64, 32)
    with pytest.raises(ValueError):
        mfma_linear(x, w, group=2, k_chunk=16)
    with pytest.raises(ValueError):
        mfma_linear(x, w, m_split=32, k_chunk=16)
