"""The forward and data-gradient GEMMs of one training step of PCN / ECG / VRCNet that _gemm_fits refuses (a reduction > 512
with too few output tiles: mvp_benchmark_amd/pointwise.py), each under every route it could take, in ONE process, the routes
alternating: the library's convolution, the library's batched GEMM (the parent's route with LIBRARY_IS_GEMM, and for every
data gradient), the plain MFMA kernel, and mvp_pointwise_mfma_splitk at the plan's chunk, half of it and double.
    python tools/bench_splitk.py [pcn ecg vrcnet]        MVP_SPLITK_ROUNDS / MVP_SPLITK_WINDOW_MS: alternations, ms per window
Shapes are recorded the way tools/bench_conv_passes.py records them (one step through the library route, F.conv1d / conv2d
wrapped).  A row: forward = relu(W x + b); data gradient = W^T (gy masked by ReLU'), reduction over cout -- as a
convolution it is the FORWARD convolution with the transposed weight (never MIOpen's backward-data kernels:
profiles/r6_miopen_igemm_bwd_fault.txt).  Times: device events around `reps` back-to-back calls, reps chosen per route so
that a window lasts about WINDOW_MS; per route the median over the rounds and min..max, in ms per call.  `err`: largest
difference of the split kernel's output from the batched GEMM's (summation order only)."""
import collections
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "completion"))
import torch
import torch.nn.functional as F
from mvp_benchmark_amd import _lib
from mvp_benchmark_amd import pointwise as pw

dev = "cuda:0"
ROUNDS = int(os.environ.get("MVP_SPLITK_ROUNDS", "7"))
WINDOW_MS = float(os.environ.get("MVP_SPLITK_WINDOW_MS", "60"))
tb = torch.ops.aten.threshold_backward


def record_shapes(name):
    """(B, Cin, L, Cout) -> count of the 1x1 convolutions of one training step (batch 32, 2048 points)."""
    import train
    args = train.load_config(os.path.join(ROOT, "completion", "cfgs", name + ".yaml"))
    args.load_model = None
    net = importlib.import_module("models." + name).Model(args).to(dev).train()
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(32, 2048, 3, generator=g).to(dev)
    shapes = collections.Counter()
    o1, o2 = F.conv1d, F.conv2d

    def rec(orig):
        def f(x, w, b=None, *a, **k):
            if w.shape[2:].numel() == 1:
                shapes[(x.shape[0], x.shape[1], x[0, 0].numel(), w.shape[0])] += 1
            return orig(x, w, b, *a, **k)
        return f
    saved = pw.MFMA_TRAIN, pw.USE_MFMA
    pw.MFMA_TRAIN = pw.USE_MFMA = False                   # through the library route: every layer passes F.conv*
    F.conv1d, F.conv2d = rec(o1), rec(o2)
    try:
        net(gt.transpose(2, 1).contiguous(), gt, alpha=0.5)
    finally:
        F.conv1d, F.conv2d = o1, o2
        pw.MFMA_TRAIN, pw.USE_MFMA = saved
    torch.cuda.synchronize()
    del net
    torch.cuda.empty_cache()
    return shapes


def refused_gemms(shapes):
    """[(pass, B, rows m, reduction k, L, count)] of the layers' forward and data-gradient GEMMs _gemm_fits refuses."""
    out = []
    for (B, cin, L, cout), n in sorted(shapes.items()):
        if L % 4 or L == 0:
            continue
        if not pw._gemm_fits(B, cout, cin, L):
            out.append(("fwd", B, cout, cin, L, n))
        if not pw._gemm_fits(B, cin, cout, L):
            out.append(("dgrad", B, cin, cout, L, n))
    return out


def chunks_of(B, m, k, L):
    """The plan's chunk, half and double (multiples of 16, 2..32 chunks); without a plan: 2 and 4 chunks."""
    plan = _lib.pointwise_mfma_splitk_plan(B, k, m, L)
    r16 = lambda v: max(16, -(-int(v) // 16) * 16)
    cand = [plan, r16(plan / 2), r16(plan * 2)] if plan else [r16(-(-k // 2)), r16(-(-k // 4))]
    out = []
    for c in cand:
        if c not in out and 2 <= -(-k // c) <= 32:
            out.append(c)
    return plan, out


def bench(routes):
    """routes: [(label, fn)] -> {label: [ms per call, one per round]}, the routes alternating inside every round."""
    reps = {}
    for label, fn in routes:                               # warm-up (code objects, the library's algorithm choice) + calibration
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        reps[label] = max(10, int(WINDOW_MS / max(e0.elapsed_time(e1) / 10, 1e-3)))
    times = {label: [] for label, _ in routes}
    for _ in range(ROUNDS):
        for label, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[label]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) / reps[label])
    return times, reps


def routes_of(kind, B, m, k, L, chunks):
    """The callables of one GEMM.  fwd: x (B, k, L), w (m, k); dgrad: gy, y (B, k, L), w (k, m) = the layer's (cout, cin)."""
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    if kind == "fwd":
        x, w, b = r(B, k, L), r(m, k), r(m)
        w3, wb = w.unsqueeze(2).contiguous(), w.unsqueeze(0).expand(B, m, k)
        routes = [("conv1d", lambda: torch.relu_(F.conv1d(x, w3, b))),
                  ("bmm", lambda: torch.relu_(torch.baddbmm(b.view(1, m, 1), wb, x))),
                  ("mfma", lambda: pw.mfma_linear(x, w, b, relu=True))]
        routes += [("split %d" % c, lambda c=c: pw.mfma_linear(x, w, b, relu=True, k_chunk=c)) for c in chunks]
    else:
        gy, y, w = r(B, k, L), r(B, k, L), r(k, m)
        wt3, wt = w.t().unsqueeze(2).contiguous(), w.t()
        routes = [("conv1d", lambda: F.conv1d(tb(gy, y, 0), wt3)),
                  ("bmm", lambda: torch.matmul(wt, tb(gy, y, 0)))]
        if m % 4 == 0:                                   # (the kernels read W^T with 16-byte loads along the rows)
            routes += [("mfma", lambda: pw.mfma_linear(gy, w, w_kmajor=True, xmask=y))]
            routes += [("split %d" % c, lambda c=c: pw.mfma_linear(gy, w, w_kmajor=True, xmask=y, k_chunk=c)) for c in chunks]
    return routes


def main():
    names = sys.argv[1:] or ["pcn", "ecg", "vrcnet"]
    assert torch.cuda.is_available(), "bench_splitk needs the GPU"
    print("# split-K MFMA route against the library and the plain MFMA kernel; %d alternations, ~%.0f ms per window; %s; torch %s"
          % (ROUNDS, WINDOW_MS, torch.cuda.get_device_name(0), torch.__version__))
    print("# ms per call: median [min..max]; flops = 2 B m k L")
    done = {}
    for name in names:
        gemms = refused_gemms(record_shapes(name))
        print("\n## %s: %d refused GEMMs in one training step" % (name, len(gemms)), flush=True)
        for kind, B, m, k, L, n in gemms:
            key = (kind, B, m, k, L)
            if key in done:
                print("%-5s B %d, %d rows x %d reduction x %d positions, %d per step: see %s" % (kind, B, m, k, L, n, done[key]))
                continue
            done[key] = name
            plan, chunks = chunks_of(B, m, k, L)
            routes = routes_of(kind, B, m, k, L, chunks)
            outs = {label: fn() for label, fn in routes}
            torch.cuda.synchronize()
            err = max([(outs[label] - outs["bmm"]).abs().max().item() for label in outs if label.startswith("split")] or [float("nan")])
            del outs
            times, reps = bench(routes)
            print("%-5s B %d, %d rows x %d reduction x %d positions, %d per step; plan chunk %d (%s chunks); err %.2e"
                  % (kind, B, m, k, L, n, plan, -(-k // plan) if plan else "no", err))
            for label, _ in routes:
                ts = times[label]
                med = statistics.median(ts)
                print("    %-12s %8.4f [%.4f..%.4f]  %6.1f TFLOP/s  x%d" % (label, med, min(ts), max(ts), 2.0 * B * m * k * L / med / 1e9,
                                                                         reps[label]), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
