#!/usr/bin/env python3
"""Same-process timing of the geometry query entry points: kNN, Gram top-k, Chamfer forward, furthest point sampling.

usage: ab_geometry.py [OTHER_LIB] [--reps N] [--only TEXT]
    OTHER_LIB  a second build of libmvpops.so (say the parent commit's): both are loaded into this process and every
               case is timed on them in turn, N >= 7 alternations -- the comparison a refactor is judged by
    --only T   only the cases whose "operator dimensions kind" contains T

Prints median [min .. max] in ms per call; with two libraries whether they wrote the same outputs and where the tree's
median lies in the other build's own range; with one, whether the plain and the sorted entry point wrote the same."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mvp_benchmark_amd import _lib

BOTH = ("plain", "sorted")
# (operator, input kind, entry points timed, shapes).  kNN: (b, n candidates, m queries, k); Gram top-k: (b, n, k);
# Chamfer: (b, n, m); FPS: (b, n, m samples).  "lattice": every distance is tied, so every query of the sorted kNN goes
# through knn_fix_kernel.  kNN shapes below the sorted route's thresholds time what mvp_knn_sorted hands to mvp_knn.
CASES = [
    ("knn", "uniform", BOTH, [(64, 16384, 16384, 16), (64, 8192, 8192, 16), (64, 4096, 4096, 16), (64, 16384, 16384, 8),
                              (64, 16384, 16384, 32), (64, 3072, 3072, 10), (64, 3072, 3072, 20), (64, 3072, 1536, 16),
                              (64, 1536, 1536, 20), (64, 2048, 2048, 16), (64, 768, 768, 20), (32, 2048, 2048, 16)]),
    ("knn", "uniform", ("plain",), [(128, 1024, 1024, 20), (64, 2048, 2048, 40)]),   # DCP's graph; knn_kernel<64>: k > 32
    ("knn", "lattice", BOTH, [(64, 4096, 4096, 16)]),                  # 16^3
    ("topk_gram", "uniform", ("gram",), [(1, 16640, 20)]),             # above 16384 columns: the tile kernel
    ("chamfer", "uniform", BOTH, [(64, 16384, 16384), (32, 16384, 16384), (64, 8192, 8192), (64, 4096, 4096),
                                  (64, 2048, 16384), (64, 8192, 16384), (64, 2048, 2048)]),
    ("fps", "uniform", BOTH, [(64, 16384, 2048), (64, 8192, 1024), (64, 6144, 1024), (32, 16384, 2048)]),
    ("fps", "uniform", ("plain",), [(64, 2048, 2048), (64, 768, 384)]),
]


def cloud(kind, b, n, gen, dev):
    """(b, n, 3) points: uniform in the unit cube, or the side^3 = n lattice in a random order per cloud."""
    if kind == "uniform":
        return torch.rand(b, n, 3, generator=gen).to(dev)
    side = round(n ** (1 / 3))
    assert side ** 3 == n, "a lattice needs a cube number of points"
    axis = torch.arange(side, dtype=torch.float32) / side
    grid = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(n, 3)
    return torch.stack([grid[torch.randperm(n, generator=gen)] for _ in range(b)]).to(dev)


def variants(op, dims, kind, gen, dev):
    """label -> (entry point, its arguments without the stream, the output tensors that are compared)."""
    new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
    b, n, m = dims[:3]
    if op == "topk_gram":
        feat = torch.rand(b, 64, n, generator=gen).to(dev)
        idx = new(b, n, m, dtype=torch.int32)
        return {"gram": ("mvp_topk_gram", (b, n, m, torch.bmm(feat.transpose(1, 2), feat), (feat * feat).sum(1), idx), (idx,))}
    x = cloud(kind, b, n, gen, dev)
    if op == "knn":
        idx = new(b, m, dims[3], dtype=torch.int32)
        args, outs = dims + (x, x[:, :m].contiguous(), idx, new(b, m, dims[3])), (idx,)
        names, nbytes = ("mvp_knn", "mvp_knn_sorted"), _lib.knn_scratch_bytes(b, n, m)
    elif op == "chamfer":
        outs = (new(b, n), new(b, m), new(b, n, dtype=torch.int32), new(b, m, dtype=torch.int32))
        args = dims + (x, cloud(kind, b, m, gen, dev)) + outs
        names, nbytes = ("mvp_chamfer_forward", "mvp_chamfer_forward_sorted"), _lib.chamfer_scratch_bytes(b, n, m)
    else:
        idx = new(b, m, dtype=torch.int32)
        args, outs = dims + (x, new(b, n), idx), (idx,)
        names, nbytes = ("mvp_furthest_point_sampling", "mvp_furthest_point_sampling_sorted"), _lib.fps_scratch_bytes(b, n)
    return {"plain": (names[0], args, outs), "sorted": (names[1], args + (new(max(nbytes, 16), dtype=torch.uint8), nbytes), outs)}


def bind(path):
    """One build of the library: name -> ctypes function, typed from the binding's table."""
    handle = ctypes.CDLL(path)
    assert handle.mvp_abi_version() == _lib.ABI_VERSION, "%s: another ABI" % path
    fns = {name: getattr(handle, name) for name in _lib.SIGNATURES}
    for name, fn in fns.items():
        fn.restype = ctypes.c_int
        fn.argtypes = [_lib._CT[k] for k in _lib.SIGNATURES[name]] + [ctypes.c_void_p]
    return fns


def time_ms(fns, name, args, calls=3):
    """ms per call: `calls` calls between two device events (every return code checked)."""
    cargs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    codes = [fns[name](*cargs, torch.cuda.current_stream().cuda_stream) for _ in range(calls)]
    e1.record()
    e1.synchronize()
    assert not any(codes), "%s returned %s" % (name, codes)
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("other", nargs="?", help="a second build of libmvpops.so")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    opt = ap.parse_args()
    if opt.reps < 7:
        ap.error("--reps: at least 7 alternations")
    libs = {"tree": bind(_lib.LIB_PATH)}
    if opt.other:
        libs["other"] = bind(os.path.abspath(opt.other))
    dev, gen = torch.device("cuda:0"), torch.Generator().manual_seed(0)
    equal = lambda xs, ys: all(torch.equal(x, y) for x, y in zip(xs, ys))
    print("%s; tree = the tree's library%s; %d alternations, ms per call: median [min .. max]"
          % (torch.cuda.get_device_name(0), ", other = " + opt.other if opt.other else "", opt.reps), flush=True)
    for op, kind, labels, shapes in CASES:
        for dims in shapes:
            title = "%s %s %s" % (op, dims, kind)
            if opt.only not in title:
                continue
            var, wrote = variants(op, dims, kind, gen, dev), {}
            for label in labels:
                name, args, outs = var[label]
                for lib, fns in libs.items():       # warm-up, and what each build writes
                    time_ms(fns, name, args, calls=1)
                    wrote[lib, label] = [o.clone() for o in outs]
                times = {lib: [] for lib in libs}
                for _ in range(opt.reps):
                    for lib, fns in libs.items():
                        times[lib].append(time_ms(fns, name, args))
                cols = ["%s %.3f [%.3f .. %.3f]" % (lib, statistics.median(t), min(t), max(t)) for lib, t in times.items()]
                if opt.other:
                    med, lo, hi = statistics.median(times["tree"]), min(times["other"]), max(times["other"])
                    cols += ["outputs equal: %s" % equal(wrote["tree", label], wrote["other", label]),
                             "tree's median %s other's range" % ("below" if med < lo else "ABOVE" if med > hi else "inside")]
                print("%-34s %-7s %s" % (title, label, "  ".join(cols)), flush=True)
            if not opt.other and labels == BOTH:
                print("%-34s plain and sorted outputs equal: %s" % ("", equal(wrote["tree", "plain"], wrote["tree", "sorted"])), flush=True)


if __name__ == "__main__":
    main()
