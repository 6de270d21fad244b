"""CPU tests of the host side: the C-ABI library loads and exports every
symbol include/mvpops.h declares (no compute without a GPU), the Python
operator surface mirrors the reference's names, the product path refuses to
run on CPU tensors (no fallback), and the pure-PyTorch counterparts
(fscore, distChamfer, calc_cd formulas) match the reference-generated golden
vectors bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from conftest import ROOT


def test_library_exports_every_declared_symbol():
    from mvp_benchmark_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvpops.h")).read()
    declared = set(re.findall(r"\b(mvp_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 18
    assert declared == set(_lib.exported_symbols())
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mvp_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define MVP_ABI_VERSION (\d+)", header).group(1))
    # per cloud: state 132 B/pt + bound broadcast buffers + cell offsets + barrier granules (3 x 256 B), the bid areas of
    # the gathered-bid rounds (2 parities x (256 bids x 16 B + 8 member words)), hand-over record (96 B), statistics (16 B)
    assert lib.mvp_emd_scratch_bytes(64, 16384) == 64 * (16384 * 132 + 8 * 2048 * 8 + 1732 * 4 + 768 + 2 * (2 * 256 + 8) * 8 + 96 + 16)
    assert lib.mvp_emd_scratch_bytes(2, 32768) == 2 * (32768 * 132 + 8 * 2048 * 8 + 1732 * 4 + 768 + 2 * (2 * 256 + 8) * 8 + 96 + 16)
    # the knobs are process-wide: restore what is touched
    try:
        assert lib.mvp_emd_configure(-1, -1, 0, -1) == 0
        assert lib.mvp_emd_configure(3, -1, -1, -1) == -2           # MVP_EBADARG: cluster width
        assert lib.mvp_emd_configure(-1, -1, -1, 0) == -2           # MVP_EBADARG: resident cap 1..64
        assert lib.mvp_emd_configure(-1, -1, -1, 65) == -2
        assert lib.mvp_emd_configure(-1, -1, -1, 8) == 0
    finally:
        assert lib.mvp_emd_configure(0, -1, _lib.EMD_DEFAULT_SPLIT, 16) == 0


def test_binding_tables_match_every_prototype_of_the_header():
    """Every prototype of include/mvpops.h against the binding's two tables: the return type and, parameter by parameter,
    the kind ctypes converts to (* -> p, long long -> q, float -> f, int -> i).  A launching entry point returns int and
    ends in the stream pointer, which SIGNATURES leaves out; a host-only one is in HOST_SIGNATURES with its return kind."""
    from mvp_benchmark_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvpops.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    protos = re.findall(r"(?m)^(int|long long|const char \*)\s*(mvp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header)
    assert len(protos) == len(set(p[1] for p in protos)) == len(re.findall(r"\bmvp_[a-z0-9_]+\s*\(", header))

    def kind(param):
        param = " ".join(param.split())
        if "*" in param:
            return "p"
        for text, k in (("long long ", "q"), ("float ", "f"), ("int ", "i")):
            if param.startswith(text):
                return k
        raise AssertionError("parameter %r" % param)

    ret_kind = {"int": "i", "long long": "q", "const char *": "s"}
    seen = {}
    for ret, name, params in protos:
        params = [] if params.strip() in ("", "void") else params.split(",")
        seen[name] = (ret_kind[ret], "".join(kind(p) for p in params), params)
    assert not set(_lib.SIGNATURES) & set(_lib.HOST_SIGNATURES)
    assert set(seen) == set(_lib.SIGNATURES) | set(_lib.HOST_SIGNATURES)
    for name, (ret, kinds, params) in seen.items():
        if name in _lib.SIGNATURES:
            assert ret == "i" and params[-1].split() == ["void", "*stream"], name
            assert kinds == _lib.SIGNATURES[name] + "p", name
        else:
            assert (ret, kinds) == _lib.HOST_SIGNATURES[name], name
    assert len(_lib.HOST_SIGNATURES) >= 18 and len(_lib.SIGNATURES) >= 51       # the parser did not come back empty
    # what load() hands ctypes is the tables, nothing else
    lib = _lib.load()
    for name, (ret, kinds, _) in seen.items():
        fn = getattr(lib, name)
        assert fn.restype is _lib._CT[ret] and list(fn.argtypes) == [_lib._CT[k] for k in kinds], name


def test_argument_guards_need_no_gpu():
    """Shape guards return error codes before anything is launched."""
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    # emd: n % 1024 != 0, b > 512 (emd_cuda.cu:236-249) -> MVP_EBADSHAPE
    assert lib.mvp_emd_forward(1, 1000, null, null, null, null, 0.005, 50, null, 0, null) == -1
    assert lib.mvp_emd_forward(513, 1024, null, null, null, null, 0.005, 50, null, 0, null) == -1
    assert lib.mvp_emd_forward(1, 1024, null, null, null, null, 0.005, 0, null, 0, null) == -1
    assert lib.mvp_emd_forward(1, 1024, null, null, null, null, 0.0, 50, null, 0, null) == -2     # eps must be > 0
    # null buffers -> MVP_EBADARG
    assert lib.mvp_emd_forward(1, 1024, null, null, null, null, 0.005, 50, null, 0, null) == -2
    assert lib.mvp_chamfer_forward(1, 8, 8, null, null, null, null, null, null, null) == -2
    assert lib.mvp_knn(1, 8, 8, 101, null, null, null, null, null) == -1
    assert lib.mvp_knn(1, 8, 8, 0, null, null, null, null, null) == -1
    # empty batch is a successful no-op
    assert lib.mvp_chamfer_forward(0, 8, 8, null, null, null, null, null, null, null) == 0
    assert lib.mvp_gather_points(0, 3, 8, 8, null, null, null, null) == 0


def test_guards_and_scratch_sizes_of_the_widened_entry_points():
    """Host logic of the entry points beyond the reference's operator set: shape
    guards, scratch formulas, no launch."""
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    # transposed scatter gradients: chunk 1536 up to 2048 destinations, 3072 above; not covered beyond 8192
    # per (cloud, chunk): u16 offsets padded to 8 bytes + u16 entries (weighted: {column, weight} pairs of 8 bytes)
    up8 = lambda v: (v + 7) // 8 * 8
    assert _lib.scatter_scratch_bytes(2, 1024, 3000, 1) == 2 * 2 * up8(up8((1024 + 1) * 2) + 1536 * 2)
    assert _lib.scatter_scratch_bytes(1, 3072, 49152, 1) == 16 * up8(up8((3072 + 1) * 2) + 3072 * 2)
    assert _lib.scatter_scratch_bytes(1, 1024, 3072, 3) == 2 * up8(up8((1024 + 1) * 2) + 1536 * 3 * 8)
    assert _lib.scatter_scratch_bytes(1, 8193, 100, 1) == 0 and _lib.scatter_scratch_bytes(1, 100, 100, 2) == 0
    # ... and the _ws entry points fall back to the plain ones (which accept the empty batch)
    assert lib.mvp_gather_points_grad_ws(0, 3, 8, 8, null, null, null, null, 0, 0, null) == 0
    assert lib.mvp_three_interpolate_grad_ws(1, 3, 8, 0, null, null, null, null, null, 0, 0, null) == -1    # m == 0
    # Gram top-k
    assert lib.mvp_topk_gram(1, 8, 9, null, null, null, null) == -1        # k > n
    assert lib.mvp_topk_gram(1, 8, 0, null, null, null, null) == -1
    assert lib.mvp_topk_gram(1, 8, 4, null, null, null, null) == -2
    assert lib.mvp_topk_gram(0, 8, 4, null, null, null, null) == 0
    # shared-weight aggregation: share in {1,2,4,8,16}
    assert lib.mvp_share_weighted_sum(1, 3, 2, 4, 8, null, null, null, null) == -1
    assert lib.mvp_share_weighted_sum(1, 8, 2, 4, 8, null, null, null, null) == -2
    assert lib.mvp_share_weighted_sum(0, 8, 2, 4, 8, null, null, null, null) == 0
    assert lib.mvp_share_weighted_sum_grad(1, 8, 2, 4, 8, null, null, null, null, null, null) == -2
    # ... with the gather fused in: (b, share, cw, k, n_src, n); the `share` staged rows fit 96 KiB of LDS
    gather = lambda *dims: lib.mvp_share_gather_sum(*dims, null, null, null, null, null)
    gather_grad = lambda *dims: lib.mvp_share_gather_sum_grad(*dims, null, null, null, null, null, null, null)
    for fn in (gather, gather_grad):
        assert fn(1, 3, 2, 4, 8, 8) == -1                                # share
        assert fn(1, 8, 2, 4, 0, 8) == -1 and fn(1, 8, 2, 4, -1, 8) == -1   # n_src <= 0
        assert fn(0, 8, 2, 4, 0, 8) == -1                                # ... also in front of the empty batch
        assert fn(1, 8, 2, 4, 8, -1) == -1 and fn(1, 8, 2, -1, 8, 8) == -1 and fn(65536, 8, 2, 4, 8, 8) == -1
        for share in (1, 2, 4, 8, 16):
            n_src = 24576 // share
            assert lib.mvp_share_gather_sum_lds_bytes(share, n_src) == 96 * 1024
            assert lib.mvp_share_gather_sum_lds_bytes(share, n_src + 1) == 96 * 1024 + 4 * share
            assert fn(1, share, 2, 4, n_src, 65) == -2                   # covered: the null buffers are what is wrong
            assert fn(1, share, 2, 4, n_src + 1, 65) == -1               # one row above the limit
        assert fn(0, 8, 2, 4, 8, 8) == 0 and fn(1, 8, 0, 4, 8, 8) == 0 and fn(1, 8, 2, 4, 8, 0) == 0   # nothing to do
    assert gather_grad(1, 8, 2, 0, 8, 8) == 0                            # k == 0: no gradient to write
    assert gather(1, 8, 2, 0, 8, 8) == -2                                # ... but an output to zero
    # pointwise weight gradient: cout <= 64, positions a multiple of 4; one partial per run of 1024 positions
    assert _lib.pointwise_wgrad_scratch_bytes(2, 24, 24, 4096) == 2 * 4 * (24 * 24 + 24) * 4
    assert _lib.pointwise_wgrad_scratch_bytes(1, 24, 65, 4096) == 0
    assert _lib.pointwise_wgrad_scratch_bytes(1, 24, 24, 4094) == 0
    assert lib.mvp_pointwise_wgrad(1, 24, 24, 4094, null, null, null, null, null, 0, null) == -1
    assert lib.mvp_pointwise_wgrad(1, 24, 24, 4096, null, null, null, null, null, 0, null) == -2
    # chamfer / fps scratch
    assert _lib.fps_scratch_bytes(3, 16384) == 3 * 16384 * 16
    assert lib.mvp_furthest_point_sampling_sorted(1, 0, 4, null, null, null, null, 0, null) == -1


def test_return_codes_of_the_sorted_geometry_entry_points():
    """mvp_knn_sorted, mvp_chamfer_forward_sorted and mvp_furthest_point_sampling_sorted: the scratch and pointer guards
    of the sorted route, and the edges of the rule that hands a call to the plain entry point.  Every row returns before
    a launch: a guard refuses, or the batch is empty."""
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    OK, EBADSHAPE, EBADARG = 0, -1, -2
    null, dummy, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4097)
    # name -> (dimensions of a sorted-route shape, device pointers, scratch size of (b, dims), has a b > 65535 guard)
    entries = {
        "mvp_knn_sorted": ((4096, 1024, 8), 4, lambda b, n, m, k: _lib.knn_scratch_bytes(b, n, m), True),
        "mvp_chamfer_forward_sorted": ((4096, 4096), 6, _lib.chamfer_scratch_bytes, True),
        "mvp_furthest_point_sampling_sorted": ((4097, 4), 3, lambda b, n, m: _lib.fps_scratch_bytes(b, n), False),
    }

    def run(name, b, dims, ptrs, scratch, nbytes):
        nptr = entries[name][1]
        ptrs = list(ptrs) if isinstance(ptrs, (list, tuple)) else [ptrs] * nptr
        return getattr(lib, name)(b, *dims, *ptrs, scratch, nbytes, null)

    for name, (dims, nptr, need_of, guards_b) in entries.items():
        need = need_of(1, *dims)
        assert need > 0, name
        assert run(name, 1, dims, dummy, null, need) == EBADARG, name           # no scratch
        assert run(name, 1, dims, dummy, null, 0) == EBADARG, name
        assert run(name, 1, dims, dummy, dummy, need - 1) == EBADARG, name      # one byte short
        assert run(name, 1, dims, dummy, odd, need + 16) == EBADARG, name       # misaligned
        for missing in range(nptr):                                            # each input / output on its own
            ptrs = [null if i == missing else dummy for i in range(nptr)]
            assert run(name, 1, dims, ptrs, dummy, need) == EBADARG, (name, missing)
        if guards_b:
            # more clouds than a grid dimension holds, with scratch that passes: the shape is what is wrong ...
            assert run(name, 65536, dims, dummy, dummy, need_of(65536, *dims)) == EBADSHAPE, name
            # ... and without scratch the scratch is refused first
            assert run(name, 65536, dims, dummy, null, 0) == EBADARG, name
        assert run(name, 0, dims, null, null, 0) == OK, name                    # the empty batch needs nothing

    # One below each threshold of the sorted route the call is the plain entry point's, which wants no scratch: its code,
    # not EBADARG.  The empty batch returns MVP_OK before a pointer is read; where the plain entry point has a guard the
    # sorted route answers differently (b = 65536 without scratch: EBADSHAPE there, EBADARG here), that one names the
    # side of the threshold a shape is on without a launch.
    below = {
        "mvp_knn_sorted": [(4095, 1024, 8), (2047, 2048, 8), (4096, 1023, 8), (4096, 1024, 33)],
        "mvp_chamfer_forward_sorted": [(2047, 16384), (16384, 2047), (4095, 4097)],     # 4095 * 4097 = 2^24 - 1
        "mvp_furthest_point_sampling_sorted": [(4096, 4), (16385, 4), (4097, 1)],
    }
    at = {
        "mvp_knn_sorted": [(4096, 1024, 8), (2048, 2048, 8), (4096, 1024, 32)],
        "mvp_chamfer_forward_sorted": [(2048, 8192), (8192, 2048), (4096, 4096)],
        "mvp_furthest_point_sampling_sorted": [(4097, 4), (16384, 2)],
    }
    for name, (_, _, _, guards_b) in entries.items():
        for dims in below[name]:
            assert run(name, 0, dims, dummy, null, 0) == OK, (name, dims)
            if guards_b:
                assert run(name, 65536, dims, dummy, null, 0) == EBADSHAPE, (name, dims)
        for dims in at[name]:
            assert run(name, 1, dims, dummy, null, 0) == EBADARG, (name, dims)
            if guards_b:
                assert run(name, 65536, dims, dummy, null, 0) == EBADARG, (name, dims)
    # the plain entry points' own shape guards come through the fall-back
    assert run("mvp_knn_sorted", 1, (4096, 1024, 101), dummy, null, 0) == EBADSHAPE
    assert run("mvp_chamfer_forward_sorted", 1, (0, 4096), dummy, null, 0) == EBADSHAPE
    assert run("mvp_furthest_point_sampling_sorted", 1, (0, 4), dummy, null, 0) == EBADSHAPE


def test_return_codes_of_the_gather_and_scatter_entry_points():
    """The nine entry points of csrc/pn2_gather.hip that share one body: which guard answers, and in which order.  Every
    row returns before a launch (null pointers, or dummy ones behind a guard that refuses first).  Dimensions are given
    as (b, c, row, count): `row` the length of a feature row (source of a gather, destination of a scatter), `count` the
    number of outputs / of grad_out columns."""
    from mvp_benchmark_amd import _lib
    lib = _lib.load()
    OK, EBADSHAPE, EBADARG = 0, -1, -2
    null, dummy = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    same = lambda b, c, row, count: (b, c, row, count)
    grouped = lambda b, c, row, count: (b, c, row, count, 1)
    # name -> (argument order of the dimensions, device pointers, taps per entry of its scratch size or None)
    entries = {
        "mvp_gather_points": (same, 3, None), "mvp_gather_points_grad": (same, 3, None),
        "mvp_group_points": (grouped, 3, None), "mvp_group_points_grad": (grouped, 3, None),
        "mvp_three_interpolate": (same, 4, None),
        "mvp_three_interpolate_grad": (lambda b, c, row, count: (b, c, count, row), 4, None),
        "mvp_gather_points_grad_ws": (same, 3, 1), "mvp_group_points_grad_ws": (grouped, 3, 1),
        "mvp_three_interpolate_grad_ws": (lambda b, c, row, count: (b, c, count, row), 4, 3),
    }
    assert all(name in _lib.SIGNATURES for name in entries)
    # (b, c, row, count), pointers, code.  "dummy" rows pass every argument guard and are refused by the grid check.
    table = [
        ((-1, 3, 8, 8), null, EBADSHAPE), ((1, -1, 8, 8), null, EBADSHAPE), ((1, 3, -1, 8), null, EBADSHAPE),
        ((1, 3, 8, -1), null, EBADSHAPE),
        ((-1, 0, 8, 8), null, EBADSHAPE), ((0, 3, 8, -1), null, EBADSHAPE),          # the sign guard comes first
        ((0, 3, 8, 8), null, OK), ((1, 0, 8, 8), null, OK), ((1, 3, 8, 0), null, OK),  # nothing to do
        ((1, 3, 0, 0), null, OK), ((0, 0, 0, 0), null, OK),                           # ... also with an empty source
        ((1, 3, 0, 8), null, EBADSHAPE), ((1, 3, 0, 8), dummy, EBADSHAPE),            # an empty source with work to do
        ((1, 3, 8, 8), null, EBADARG), ((1, 3, 24577, 8), null, EBADARG), ((65536, 3, 8, 8), null, EBADARG),
        ((65536, 1, 8, 8), dummy, EBADSHAPE),         # b == 65536 on the LDS routes ...
        ((65536, 1, 8, 1), dummy, EBADSHAPE),         # ... the direct gather (2 * count < row) ...
        ((65536, 1, 24577, 1), dummy, EBADSHAPE),     # ... and with rows too long for LDS
    ]

    def run(name, dims, ptrs, ws=()):
        order, nptr, _ = entries[name]
        ptrs = list(ptrs) if isinstance(ptrs, (list, tuple)) else [ptrs] * nptr
        return getattr(lib, name)(*order(*dims), *ptrs, *ws, null)

    def scratch_need(name, dims):
        b, _, row, count = dims
        return _lib.scatter_scratch_bytes(b, row, count, entries[name][2]) if min(dims) >= 0 else 0

    for name, (_, nptr, taps) in entries.items():
        for dims, ptrs, code in table:
            if taps is None:
                assert run(name, dims, ptrs) == code, (name, dims)
                continue
            # _ws with no scratch, or with fewer bytes than needed: the plain entry's code
            plain = run(name[:-3], dims, ptrs)
            need = scratch_need(name, dims)
            assert plain == code and run(name, dims, ptrs, (null, 0, 0)) == code, (name, dims)
            assert run(name, dims, ptrs, (dummy, max(need - 1, 0), 0)) == code, (name, dims, need)
            if ptrs is null:                                   # ... and with enough of it, the same guards (null buffers)
                assert run(name, dims, ptrs, (dummy, need, 0)) == code, (name, dims, need)
        for missing in range(nptr):                            # each required pointer on its own
            ptrs = [null if i == missing else dummy for i in range(nptr)]
            if taps is None:
                assert run(name, (1, 3, 8, 8), ptrs) == EBADARG, (name, missing)
            else:
                need = scratch_need(name, (1, 3, 8, 8))
                assert need > 0
                assert run(name, (1, 3, 8, 8), ptrs, (null, 0, 0)) == EBADARG, (name, missing)
                assert run(name, (1, 3, 8, 8), ptrs, (dummy, need, 0)) == EBADARG, (name, missing)
    # the flattened group: npoint * nsample has to fit an int, whatever else is asked
    for name in ("mvp_group_points", "mvp_group_points_grad", "mvp_group_points_grad_ws"):
        ws = (null, 0, 0) if name.endswith("_ws") else ()
        fn = getattr(lib, name)
        assert fn(1, 3, 8, 65536, 32768, null, null, null, *ws, null) == EBADSHAPE          # 2^31
        assert fn(0, 3, 8, 65536, 32768, null, null, null, *ws, null) == EBADSHAPE          # ... in front of the empty batch
        assert fn(0, 3, 8, 65536, 32767, null, null, null, *ws, null) == OK                 # 2^31 - 32768
        assert fn(1, 3, 8, 65536, 32767, null, null, null, *ws, null) == EBADARG
        assert fn(1, 3, 8, 8, -1, null, null, null, *ws, null) == EBADSHAPE
        assert fn(0, 3, 8, -1, -1, null, null, null, *ws, null) == EBADSHAPE                # (a positive product)
        assert fn(1, 3, 8, 8, 0, null, null, null, *ws, null) == OK
    # OVERWRITE has a destination to zero or to write, scratch or not
    for name, (_, nptr, taps) in entries.items():
        if taps is not None:
            ptrs = [dummy] * (nptr - 1) + [null]
            need = scratch_need(name, (1, 3, 8, 8))
            for ws in ((null, 0, 1), (dummy, need - 1, 1), (dummy, need, 1), (dummy, need, 3)):
                assert run(name, (1, 3, 8, 8), ptrs, ws) == EBADARG, (name, ws)
            assert run(name, (1, 3, 24577, 8), ptrs, (dummy, 1 << 20, 1)) == EBADARG, name   # no scratch size: the fall-back
            assert run(name, (1, 0, 8, 8), null, (null, 0, 1)) == OK, name                   # nothing to zero


def test_operator_surface_matches_reference_names():
    import mvp_benchmark_amd.metrics as metrics
    import mvp_benchmark_amd.mm3d_pn2 as pn2
    assert metrics.__all__ == ['cd', 'fscore', 'emd']
    for name in ['ball_query', 'knn', 'furthest_point_sample',
                 'furthest_point_sample_with_dist', 'three_interpolate',
                 'three_nn', 'gather_points', 'grouping_operation',
                 'group_points', 'GroupAll', 'QueryAndGroup', 'Points_Sampler',
                 'NaiveSyncBatchNorm1d', 'NaiveSyncBatchNorm2d']:
        assert hasattr(pn2, name), name
    # `group_points` resolves to the submodule, as in the reference
    assert pn2.group_points.__name__.endswith("group_points.group_points")
    assert isinstance(metrics.cd(), torch.nn.Module)
    assert isinstance(metrics.emd(), torch.nn.Module)


def test_drop_in_utils_shims_import():
    """`sys.path.append("../utils"); from metrics import cd, fscore, emd`
    (completion/model_utils.py:19-21) keeps working against utils/."""
    import subprocess
    import sys
    code = ("import sys; sys.path.append(%r); "
            "from metrics import cd, fscore, emd; "
            "from mm3d_pn2 import furthest_point_sample, gather_points, "
            "grouping_operation, ball_query, three_nn; print('ok')"
            % os.path.join(ROOT, "utils"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                         cwd=os.path.join(ROOT, "completion"))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_no_cpu_fallback():
    from mvp_benchmark_amd._lib import MvpOpsError
    from mvp_benchmark_amd.metrics import cd, emd
    from mvp_benchmark_amd.mm3d_pn2 import furthest_point_sample, gather_points
    a = torch.rand(1, 16, 3)
    with pytest.raises((MvpOpsError, AssertionError, RuntimeError)):
        cd()(a, a)
    with pytest.raises((MvpOpsError, AssertionError, RuntimeError)):
        emd()(torch.rand(1, 1024, 3), torch.rand(1, 1024, 3), 0.005, 5)
    with pytest.raises((MvpOpsError, AssertionError, RuntimeError)):
        furthest_point_sample(a, 4)
    with pytest.raises((MvpOpsError, AssertionError, RuntimeError)):
        gather_points(torch.rand(1, 3, 16), torch.zeros(1, 4, dtype=torch.int32))


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under mvp_benchmark_amd/,
    utils/ or completion/ may reference it."""
    bad = []
    for top in ("mvp_benchmark_amd", "utils", "completion"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".cpp", ".h")):
                    txt = open(os.path.join(dirpath, f)).read()
                    if re.search(r"^\s*(import|from)\s+oracle\b", txt, re.M) or "libmvp_oracle" in txt:
                        bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_python_counterparts_match_reference_golden(chamfer_golden):
    """fscore (fscore.py:3-16), distChamfer (chamfer_python.py:18-39) and the
    calc_cd reductions (model_utils.py:67-77): bit-for-bit on this torch."""
    from mvp_benchmark_amd.metrics import fscore
    from mvp_benchmark_amd.metrics.CD.chamfer_python import distChamfer
    for name, c in chamfer_golden.items():
        a, b = torch.tensor(c["a"]), torch.tensor(c["b"])
        for chunk in (None, 1):
            d1, d2, i1, i2 = distChamfer(a, b, chunk=chunk)
            np.testing.assert_array_equal(d1.numpy(), c["dist1"], err_msg=name)
            np.testing.assert_array_equal(d2.numpy(), c["dist2"], err_msg=name)
            np.testing.assert_array_equal(i1.numpy(), c["idx1"], err_msg=name)
            np.testing.assert_array_equal(i2.numpy(), c["idx2"], err_msg=name)
        f, p1, p2 = fscore(d1, d2)
        np.testing.assert_array_equal(f.numpy(), c["f"])
        np.testing.assert_array_equal(p1.numpy(), c["p1"])
        np.testing.assert_array_equal(p2.numpy(), c["p2"])
        np.testing.assert_array_equal(fscore(d1, d2, 0.01)[0].numpy(), c["f_loose"])
        cd_p = (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2
        cd_t = d1.mean(1) + d2.mean(1)
        np.testing.assert_array_equal(cd_p.numpy(), c["cd_p"])
        np.testing.assert_array_equal(cd_t.numpy(), c["cd_t"])


def test_emd_lazy_status_check_raises_one_call_late():
    """emd_module files every call's status words (async copy to pinned memory) and examines them
    at the next forward / at check(): a negative word (abandoned cluster wait, internal check) is
    an MvpOpsError, never a silent NaN.  Exercised here with hand-made pending entries."""
    import torch
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd.metrics.EMD import emd_module

    class Done:
        def query(self):
            return True

        def synchronize(self):
            pass

    class NotYet(Done):
        def query(self):
            return False

    emd_module._PENDING.clear()
    emd_module._PENDING.append((Done(), torch.tensor([3000, 3000]), "ok call"))
    emd_module._PENDING.append((NotYet(), torch.tensor([3000, -2]), "failed call, still in flight"))
    emd_module.check(block=False)                 # the finished one is fine, the other stays filed
    assert len(emd_module._PENDING) == 1
    with pytest.raises(_lib.MvpOpsError, match="failed call"):
        emd_module.check(block=True)
    assert not emd_module._PENDING
    emd_module.check()                            # nothing pending: no-op


def test_emd_records_reads_the_scratch_tail():
    """_lib.emd_records: per-cloud hand-over records (20 ints) + statistics (2 int64) at the END of the scratch
    buffer, whatever its size -- the layout csrc/emd_common.h writes (no GPU needed: a synthetic buffer)."""
    import numpy as np
    import torch
    from mvp_benchmark_amd import _lib
    b, nbytes = 3, 4096
    buf = np.zeros(nbytes, np.uint8)
    stats = np.array([[3000, 111], [2999, 222], [-2, 0]], np.int64)
    rec = np.zeros((b, _lib.EMD_RECORD_INTS), np.int32)
    rec[:, 0] = [0, 0, 300]; rec[:, 1] = [150, 90, 201]; rec[:, 18] = [70, 0, 101]; rec[:, 19] = [2 * 16 + 8, 0, 1 * 16 + 4]
    buf[nbytes - b * 16:] = stats.view(np.uint8).ravel()
    buf[nbytes - b * 16 - rec.nbytes: nbytes - b * 16] = rec.view(np.uint8).ravel()
    got = _lib.emd_records(torch.from_numpy(buf), nbytes, b)
    assert got["rounds"].tolist() == [3000, 2999, -2] and got["bids"].tolist() == [111, 222, 0]
    assert got["next_round"].tolist() == [0, 0, 300] and got["unassigned"].tolist() == [150, 90, 201]
    assert got["first_handover"].tolist() == [70, 0, 101]
    assert got["final_width"].tolist() == [8, 0, 4] and got["final_launch"].tolist() == [2, 0, 1]


def test_pointwise_routing_rules():
    """mvp_benchmark_amd/pointwise.py: which per-cloud GEMMs go to the MFMA kernels (host logic, no GPU):
    short reductions always; long ones only with a chip's worth of 128 x 128 output tiles and full column tiles."""
    from mvp_benchmark_amd import pointwise as pw
    assert pw.MFMA_TRAIN and pw.MFMA_DGRAD and pw.MFMA_MIN_CH == 1
    fits = pw._gemm_fits
    assert fits(64, 1024, 512, 2048) and fits(64, 512, 1536, 384)          # VRCNet's widest layers
    assert fits(32, 48, 240, 1024)                                         # few workgroups but a short reduction
    assert not fits(32, 1024, 2824, 64) and not fits(32, 1024, 1800, 64)   # ECG, 64-point level: half-empty column tiles
    assert not fits(32, 768, 1864, 256)                                    # 6 x 2 x 32 = 384 workgroups < 512
    # round 6: a reduction of exactly 512 stays on the MFMA kernel even with one row of tiles -- as the data gradient of
    # (64, 128 -> 512, 384) it takes 0.050 ms against the library's 0.108, (64, 512 -> 512, 384) forward 0.127 against 0.145
    # (tools/bench_conv_passes.py); only (64, 512 -> 192, 384) forward loses 0.015 ms
    assert fits(64, 128, 512, 384) and fits(64, 32, 512, 384) and not fits(64, 128, 516, 384)
    assert fits(64, 512, 128, 384)                                         # the same layers' data gradients


def test_bench_settle_and_model_level_note():
    """bench.py's untimed pre-warm-up of the model-level steps stops once three consecutive steps agree (and gives up at its
    bound); the note that travels in the bench line formats (a '%' in it once cost the line its model-level figures)."""
    import importlib
    import time
    import types
    bench = importlib.import_module("bench")
    durations = iter([0.05, 0.04, 0.03, 0.03, 0.003, 0.003, 0.003, 0.003, 0.003, 0.003])
    calls = []

    def step():
        calls.append(1)
        time.sleep(next(durations, 0.003))

    n = bench.settle(step, max_steps=10)
    assert 7 <= n <= 10 and len(calls) == n
    jitter = iter([0.002, 0.02] * 10)
    assert bench.settle(lambda: time.sleep(next(jitter)), max_steps=8) == 8
    note = bench.model_level_note(types.SimpleNamespace(points=16384, eps=0.004, iters=3000))
    assert "5 %" in note and "16384" in note and "0.004 x 3000" in note


def test_bench_dump_outputs_budget_and_sample(tmp_path):
    """bench.py --dump-outputs: float32 (float64 kept), one .npy per output; an array past the 64 MB budget becomes a fixed
    seeded sample of its elements, the same on every call."""
    import importlib
    bench = importlib.import_module("bench")
    small = torch.arange(6, dtype=torch.float16).view(2, 3)
    wide = torch.arange(5, dtype=torch.float64)
    big = torch.arange(bench.DUMP_BUDGET_BYTES // 4 + 1000, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "wide": wide, "big": big})
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("small", "wide", "big")}
    assert a["small"].dtype == np.float32 and np.array_equal(a["small"], small.float().numpy())
    assert a["wide"].dtype == np.float64 and np.array_equal(a["wide"], wide.numpy())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET_BYTES
    assert a["big"].size == (bench.DUMP_BUDGET_BYTES - a["small"].nbytes - a["wide"].nbytes) // 4
    assert np.all(np.diff(a["big"]) > 0) and np.all(np.isin(a["big"], big.numpy()))
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
