"""BASELINE cfg 5: DCP registration, 128 pairs of 1024 points, one MI355X -- forward (eval) and forward +
backward (training step without the optimizer) timings, with the op-layer split from the torch profiler
(kNN graph, neighbour gather / its gradient, the 3x3 Kabsch SVD launch); then the same-process A/B of the fused edge MLP
(mvp_benchmark_amd.registration.EDGE_MLP) on the eval forward, on emb_nn alone and on the edge stages alone; then the same for
the transformer's fused LayerNorm + residual sums (mvp_benchmark_amd.registration.LAYER_NORM): eval forward, forward + backward,
the transformer alone, the training step's peak memory per route, and the two kernels alone with their bytes/s; then DGCNN's
BatchNorm + ReLU + max over the neighbours as kernels in training (mvp_benchmark_amd.registration.EDGE_BN): emb_nn forward +
backward, the whole step, peak memory per route, and the three entry points alone at the four stage shapes; then multi-head
attention as one kernel in inference (mvp_benchmark_amd.registration.FUSED_ATTENTION): eval forward, the transformer alone, one
attention block alone, the eval forward's peak memory per route, and the kernel alone in TFLOP/s.
   python tools/bench_dcp.py            (MVP_BENCH_REPS: timed repetitions, MVP_BENCH_AB_ROUNDS: alternations, at least 5;
                                         MVP_LIB=<other libmvpops.so> for an A/B of two builds;
                                         MVP_BENCH_ONLY=attention: the attention block alone)"""
import os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = os.path.join(ROOT, "registration")
sys.path.insert(0, ROOT); sys.path.insert(0, REG); sys.path.insert(0, os.path.join(REG, "models"))
import torch
import dcp
import train_utils as tu

from mvp_benchmark_amd import _lib
if os.environ.get("MVP_LIB"):          # A/B: another build of the library
    _lib.LIB_PATH = os.path.abspath(os.environ["MVP_LIB"])
import mvp_benchmark_amd.registration as reg_ops

REPS = int(os.environ.get("MVP_BENCH_REPS", "10"))
ROUNDS = max(5, int(os.environ.get("MVP_BENCH_AB_ROUNDS", "5")))
HBM_SPEC, HBM_COPY = 8.0, 6.29                           # TB/s: MI355X spec, measured float4 copy
dev = "cuda:0"
B, N = 128, 1024
torch.manual_seed(0)
net = dcp.Model(types.SimpleNamespace()).to(dev)
g = torch.Generator().manual_seed(5)
src = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev)
q = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=1).to(dev)
Rg = tu.quat2mat(q)
tg = (torch.rand(B, 3, generator=g) - 0.5).to(dev)
tgt = src @ Rg.transpose(1, 2) + tg.unsqueeze(1)
T_gt = tu.rt_to_transformation(Rg, tg.unsqueeze(2))


def timed(fn, reps=REPS):
    fn(); fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def alternate(switch, cases, width, tail):
    """The A/B of one switch of mvp_benchmark_amd.registration (`switch`: routes()' keyword for it), every other switch off: per
    case (name, fn, training, after) ROUNDS alternations of composed / fused, REPS repetitions each, one printed line -- the
    medians with [min .. max], then `tail` filled from ratio, diff and faster -- and after(med), where given, for a line of
    the case's own.  -> {name: fused faster than composed in every alternation}."""
    faster = {}
    for name, fn, training, after in cases:
        net.train(training)
        ms = {False: [], True: []}
        for _ in range(ROUNDS):
            for on in (False, True):
                with reg_ops.routes(**{switch: on}):
                    ms[on].append(timed(fn))
        med = {on: sorted(v)[len(v) // 2] for on, v in ms.items()}
        faster[name] = all(f < c for f, c in zip(ms[True], ms[False]))
        print("  %-*s composed %7.2f [%7.2f .. %7.2f]   fused %7.2f [%7.2f .. %7.2f]   " % (
            width, name, med[False], min(ms[False]), max(ms[False]), med[True], min(ms[True]), max(ms[True])) + tail % {
                "ratio": med[False] / med[True], "diff": med[False] - med[True], "faster": "yes" if faster[name] else "NO"},
            flush=True)
        if after is not None:
            after(med)
    return faster


def peak_memory(switch):
    """The training step's torch.cuda.max_memory_allocated per route of one switch, in GB -> {on: GB}."""
    net.train()
    peak = {}
    for on in (False, True):
        with reg_ops.routes(**{switch: on}):
            fwd_bwd(); torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            fwd_bwd(); torch.cuda.synchronize()
            peak[on] = torch.cuda.max_memory_allocated() / 1e9
        print("  training step, %s route: torch.cuda.max_memory_allocated %.2f GB" % ("fused" if on else "composed", peak[on]), flush=True)
    return peak


def kernels_alone(entries, tensor_bytes, reps, lead):
    """Entry points on their own: per (name, passes over a tensor of tensor_bytes, fn) the median of five timings of `reps`
    calls and the bytes/s of the algorithmic bytes beside the HBM rates; `lead` formats the name."""
    for name, passes, fn in entries:
        t = sorted(timed(fn, reps) for _ in range(5))[2]
        rate = passes * tensor_bytes / t / 1e9                                  # TB/s: bytes / ms / 1e9
        print(lead % name + " %7.3f ms  %5.2f TB/s = %4.1f %% of spec, %4.1f %% of the copy rate" % (
            t, rate, rate / HBM_SPEC * 100, rate / HBM_COPY * 100), flush=True)


def fwd():
    with torch.no_grad():
        return net(src, tgt, T_gt)


def fwd_bwd():
    net.zero_grad(set_to_none=True)
    loss = net(src, tgt, T_gt)[0]
    loss.mean().backward()


def attention_block():
    """The A/B of mvp_benchmark_amd.registration.FUSED_ATTENTION (default off), every other switch off, both routes in this one
    process: the eval forward, the transformer alone, one attention block alone at cfg 5's shape (the five composed steps
    against the one kernel, projections left out), the eval forward's peak memory per route, and the kernel alone in TFLOP/s."""
    import math
    H, D, PEAK_F32 = dcp.HEADS, dcp.EMB_DIMS // dcp.HEADS, 157.3
    net.eval()
    with torch.no_grad():
        f_a, f_b = (net.emb_nn(c.transpose(1, 2).contiguous()) for c in (src, tgt))
    ga = torch.Generator().manual_seed(8)
    qa, ka, va = (torch.randn(B, N, H * D, generator=ga).to(dev) for _ in range(3))
    oa = torch.empty_like(qa)
    flop = 4.0 * B * H * N * N * D

    def pointer_alone():
        with torch.no_grad():
            return net.pointer(f_a, f_b)

    def block_alone():
        with torch.no_grad():
            if reg_ops.FUSED_ATTENTION:
                return reg_ops.fused_attention(qa, ka, va, H)
            return reg_ops._attention_reference(qa, ka, va, H, math.sqrt(D))

    print("# fused attention A/B: %s; torch %s; %d alternations x %d repetitions, median ms [min .. max]; 6 attention blocks per "
          "forward over (%d, %d, %d, %d, %d); one block = %.0f GFLOP, float32 MFMA peak %.1f TFLOP/s = %.2f ms" % (
              torch.cuda.get_device_name(0), torch.__version__, ROUNDS, REPS, B, H, N, N, D, flop / 1e9, PEAK_F32,
              flop / PEAK_F32 / 1e9), flush=True)
    faster = alternate("fused_attention", (("eval forward", fwd, False, None),
                                           ("transformer alone, eval forward", pointer_alone, False, None),
                                           ("one attention block alone (%d, %d, %d, %d, %d)" % (B, H, N, N, D), block_alone, False, None)),
                       48, "composed / fused %(ratio).3f   composed - fused %(diff)6.2f ms   fused faster in every alternation: %(faster)s")
    print("  criterion (fused faster than composed in every alternation of the eval forward): %s" % (
        "met" if faster["eval forward"] else "NOT met -- the switch stays off either way"), flush=True)
    for on in (False, True):
        with reg_ops.routes(fused_attention=on):
            fwd(); torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            fwd(); torch.cuda.synchronize()
            print("  eval forward, %s route: torch.cuda.max_memory_allocated %.2f GB" % (
                "fused" if on else "composed", torch.cuda.max_memory_allocated() / 1e9), flush=True)
    t = sorted(timed(lambda: _lib.call("mvp_attention_forward", dev, B, H, N, N, D, qa, ka, va, 1 / math.sqrt(D), oa), 20)
               for _ in range(5))[2]
    print("  mvp_attention_forward alone at (%d, %d, %d, %d, %d): %7.3f ms  %6.1f TFLOP/s = %4.1f %% of the float32 MFMA peak "
          "(FLOP = 4 b h nq nk d)" % (B, H, N, N, D, t, flop / t / 1e9, flop / t / 1e9 / PEAK_F32 * 100), flush=True)


if os.environ.get("MVP_BENCH_ONLY") == "attention":      # this block alone (the whole tool takes minutes)
    attention_block()
    sys.exit(0)

net.eval()
ms_f = timed(fwd)
net.train()
ms_fb = timed(fwd_bwd)
print("cfg 5 DCP (%d pairs x %d points, k = 20 graph, 5.57 M parameters): forward %.2f ms (%.0f pairs/s), "
      "forward + backward %.2f ms (%.0f pairs/s)" % (B, N, ms_f, B / ms_f * 1e3, ms_fb, B / ms_fb * 1e3), flush=True)

from torch.profiler import profile, ProfilerActivity
for name, fn in (("forward", fwd), ("forward + backward", fwd_bwd)):
    (net.eval() if name == "forward" else net.train())
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    # kernel rows only (operator rows carry their kernels' time a second time)
    rows = [(e.key, e.self_device_time_total / 3e3, e.count // 3) for e in prof.key_averages()
            if e.self_device_time_total > 0 and str(e.device_type).endswith("CUDA")]
    total = sum(r[1] for r in rows)
    def share(*subs):
        return sum(r[1] for r in rows if any(s in r[0] for s in subs))
    knn = share("knn_kernel")
    gather = share("gather_lds_kernel", "gather_direct_kernel", "group_points")
    scatter = share("scatter_lds_kernel", "scatter_atomic_kernel", "transposed_reduce_kernel", "transpose_index_kernel", "_grad_kernel")
    svd = share("svd3")
    print("  %s: GPU time %.2f ms per step = kNN graph %.2f + neighbour gather %.2f + gather gradient %.2f + "
          "Kabsch SVD3 %.3f + everything else (library GEMMs / attention / elementwise) %.2f" % (
              name, total, knn, gather, scatter, svd, total - knn - gather - scatter - svd), flush=True)
    for r in sorted(rows, key=lambda r: -r[1])[:8]:
        print("      %-90s %8.3f ms x%d" % (r[0][:90], r[1], r[2]), flush=True)

# ---- the fused edge MLP of DGCNN (mvp_benchmark_amd.registration.EDGE_MLP, default off): the two routes in this one process,
# alternated (MVP_BENCH_AB_ROUNDS alternations, REPS repetitions each): the eval forward, emb_nn alone on both clouds, and
# the edge stages alone (mvp_edge_mlp_max against the composed gather / conv / BatchNorm / ReLU / max chain).
K_GRAPH, MAC_PER_COLUMN, PEAK = 20, 45440, 157.3         # 6*64 + 64*64 + 64*128 + 128*256 multiply-adds per edge; f32 MFMA TFLOP/s
columns = 2 * B * N * K_GRAPH
tflop = 2.0 * MAC_PER_COLUMN * columns / 1e12
net.eval()
clouds = (src.transpose(1, 2).contiguous(), tgt.transpose(1, 2).contiguous())
emb = net.emb_nn


def emb_both():
    with torch.no_grad():
        return [emb(c) for c in clouds]


def edge_stages():
    """Stages 1-4 and their maxima on both clouds, the graph given: the composed chain or the one kernel."""
    with torch.no_grad():
        for c, idx in zip(clouds, graphs):
            if reg_ops.EDGE_MLP:
                bns = [getattr(emb, "bn%d" % i) for i in range(1, 5)]
                scales = [bn.weight / torch.sqrt(bn.running_var + bn.eps) for bn in bns]
                shifts = [bn.bias - bn.running_mean * s for bn, s in zip(bns, scales)]
                reg_ops.edge_mlp_max(c, idx, [getattr(emb, "conv%d" % i).weight for i in range(1, 5)], scales, shifts)
            else:
                nbr = dcp._mu.grouping_operation(c, idx)
                edge = torch.cat((nbr, c.unsqueeze(2).expand(-1, -1, K_GRAPH, -1)), dim=1)
                for i in range(1, 5):
                    edge = emb._stage(i, edge)
                    edge.max(dim=2, keepdim=True)


with torch.no_grad():
    graphs = [dcp._mu.knn(c, K_GRAPH).int().transpose(1, 2).contiguous() for c in clouds]
print("# fused edge MLP A/B: %s; torch %s; %d alternations x %d repetitions, median ms [min .. max]; "
      "edge stages = %d MAC x %.2f M columns = %.0f GFLOP, float32 MFMA peak %.1f TFLOP/s" % (
          torch.cuda.get_device_name(0), torch.__version__, ROUNDS, REPS, MAC_PER_COLUMN, columns / 1e6, tflop * 1e3, PEAK),
      flush=True)
def arithmetic(note):
    return lambda med: print("  %-48s composed %6.1f TFLOP/s (%4.1f %% of peak)   fused %6.1f TFLOP/s (%4.1f %% of peak)%s" % (
        "  the edge stages' arithmetic over that time:", tflop / med[False] * 1e3, tflop / med[False] * 1e5 / PEAK,
        tflop / med[True] * 1e3, tflop / med[True] * 1e5 / PEAK, note), flush=True)


alternate("edge_mlp", (("eval forward", fwd, False, None),
                       ("emb_nn (kNN + edge stages + conv5), both clouds", emb_both, False, arithmetic("   (kNN and conv5 inside the time)")),
                       ("edge stages alone, both clouds", edge_stages, False, arithmetic(""))),
          48, "composed / fused %(ratio).2f")

# ---- the transformer's LayerNorm + residual sums as kernels (mvp_benchmark_amd.registration.LAYER_NORM, default off): the two
# routes in this one process, alternated like the block above: the eval forward, the training step (forward + backward), the
# transformer alone both ways; the training step's peak memory per route; then the two kernels alone at cfg 5's row count.
def pointer_eval():
    with torch.no_grad():
        return net.pointer(f_src, f_tgt)


def pointer_train():
    net.pointer.zero_grad(set_to_none=True)
    p_src, p_tgt = net.pointer(f_src, f_tgt)
    (p_src.sum() + p_tgt.sum()).backward()


net.eval()
with torch.no_grad():
    f_src, f_tgt = net.emb_nn(clouds[0]), net.emb_nn(clouds[1])
print("# fused LayerNorm + residual A/B: %d alternations x %d repetitions, median ms [min .. max]; 14 norms and 10 residual "
      "sums per forward over (%d, %d) rows" % (ROUNDS, REPS, B * N, dcp.EMB_DIMS), flush=True)
faster = alternate("layer_norm", (("eval forward", fwd, False, None), ("forward + backward", fwd_bwd, True, None),
                                  ("transformer alone, eval forward", pointer_eval, False, None),
                                  ("transformer alone, forward + backward", pointer_train, True, None)),
                   40, "composed / fused %(ratio).3f   fused faster in every alternation: %(faster)s")
print("  criterion (fused faster than composed in every alternation, eval forward and forward + backward): %s" % (
    "met" if faster["eval forward"] and faster["forward + backward"] else "NOT met -- the switch stays off either way"), flush=True)
peak_memory("layer_norm")
net.zero_grad(set_to_none=True)

ROWS_LN, D_LN = B * N, dcp.EMB_DIMS
gl = torch.Generator().manual_seed(6)
xs, ds_, gys, grs = ((torch.randn(ROWS_LN, D_LN, generator=gl) + 0.5).to(dev) for _ in range(4))
al, bl = torch.randn(D_LN, generator=gl).to(dev), torch.randn(D_LN, generator=gl).to(dev)
zs, ys, gzs = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
st = torch.empty(ROWS_LN, 2, device=dev)
gal, gbl = torch.empty_like(al), torch.empty_like(al)
nb = _lib.ref_layernorm_backward_scratch_bytes(ROWS_LN, D_LN)
scr = torch.empty(nb, device=dev, dtype=torch.uint8)
tensor_bytes = ROWS_LN * D_LN * 4
kernels = (
    ("mvp_ref_layernorm, residual (2 reads + 2 writes)", 4,
     lambda: _lib.call("mvp_ref_layernorm", dev, ROWS_LN, D_LN, xs, ds_, al, bl, 1e-6, zs, ys, st)),
    ("mvp_ref_layernorm, no residual (1 read + 1 write)", 2,
     lambda: _lib.call("mvp_ref_layernorm", dev, ROWS_LN, D_LN, xs, None, al, bl, 1e-6, None, ys, st)),
    ("mvp_ref_layernorm_backward, gres, ga / gb (3 reads + 1 write)", 4,
     lambda: _lib.call("mvp_ref_layernorm_backward", dev, ROWS_LN, D_LN, zs, al, gys, grs, st, 1e-6, gzs, gal, gbl, scr, nb)),
    ("mvp_ref_layernorm_backward, no gres, ga / gb (2 reads + 1 write)", 3,
     lambda: _lib.call("mvp_ref_layernorm_backward", dev, ROWS_LN, D_LN, zs, al, gys, None, st, 1e-6, gzs, gal, gbl, scr, nb)),
    ("mvp_ref_layernorm_backward, no gres, no ga / gb (2 reads + 1 write)", 3,
     lambda: _lib.call("mvp_ref_layernorm_backward", dev, ROWS_LN, D_LN, zs, al, gys, None, st, 1e-6, gzs, None, None, None, 0)),
)
print("# the kernels alone at (%d, %d) float32, %.0f MB a tensor; bytes/s from the algorithmic bytes; HBM %.1f TB/s spec, "
      "%.2f TB/s measured float4 copy" % (ROWS_LN, D_LN, tensor_bytes / 1e6, HBM_SPEC, HBM_COPY), flush=True)
kernels_alone(kernels, tensor_bytes, 20, "  %-70s")

# ---- DGCNN's BatchNorm + ReLU + max over k as kernels in training (mvp_benchmark_amd.registration.EDGE_BN, default off): the
# two routes in this one process, alternated like the blocks above, every other switch off: emb_nn forward + backward on both
# clouds, the whole training step; the step's peak memory per route; then the three entry points alone at cfg 5's four stage
# shapes, bytes/s from the algorithmic bytes (T = one (B, C, k, N) tensor; pooled, arg and the statistics are under T / 16).
del xs, ds_, gys, grs, zs, ys, gzs, scr
torch.cuda.empty_cache()


def emb_train():
    emb.zero_grad(set_to_none=True)
    (emb(clouds[0]).sum() + emb(clouds[1]).sum()).backward()


net.train()
print("# fused BatchNorm + ReLU + max A/B (training): %d alternations x %d repetitions, median ms [min .. max]; 4 stages x 2 "
      "clouds over (%d, C, %d, %d), C = 64, 64, 128, 256" % (ROUNDS, REPS, B, K_GRAPH, N), flush=True)
faster = alternate("edge_bn", (("emb_nn forward + backward, both clouds", emb_train, True, None), ("forward + backward", fwd_bwd, True, None)),
                   40, "composed - fused %(diff)6.2f ms   composed / fused %(ratio).3f   fused faster in every alternation: %(faster)s")
peak = peak_memory("edge_bn")
print("  criterion (fused faster than composed in every alternation of forward + backward, and a lower peak): %s" % (
    "met" if faster["forward + backward"] and peak[True] < peak[False] else "NOT met -- the switch stays off either way"), flush=True)
net.zero_grad(set_to_none=True)
torch.cuda.empty_cache()

print("# the entry points alone at (%d, C, %d, %d) float32; bytes/s from the algorithmic bytes; HBM %.1f TB/s spec, %.2f TB/s "
      "measured float4 copy" % (B, K_GRAPH, N, HBM_SPEC, HBM_COPY), flush=True)
ge = torch.Generator().manual_seed(7)
for C, which in ((64, "stages 1 and 2"), (128, "stage 3"), (256, "stage 4")):
    ze = (torch.randn(B, C, K_GRAPH, N, generator=ge) + 0.5).to(dev)
    gre = torch.randn(B, C, K_GRAPH, N, generator=ge).to(dev)
    gpe = torch.randn(B, C, N, generator=ge).to(dev)
    gam, bet = torch.randn(C, generator=ge).to(dev), torch.randn(C, generator=ge).to(dev)
    re_, gze = torch.empty_like(ze), torch.empty_like(ze)
    pe, ae = torch.empty(B, C, N, device=dev), torch.empty(B, C, N, device=dev, dtype=torch.uint8)
    ste, vae = torch.empty(C, 2, device=dev), torch.empty(C, device=dev)
    gga, gbe = torch.empty(C, device=dev), torch.empty(C, device=dev)
    nbe = _lib.edge_bn_scratch_bytes(B, C)
    sce = torch.empty(nbe, device=dev, dtype=torch.uint8)
    dims = (B, C, K_GRAPH, N)
    T = ze.numel() * 4
    _lib.call("mvp_edge_bn_stats", dev, *dims, ze, 1e-5, ste, vae, sce, nbe)
    _lib.call("mvp_edge_bn_relu_max", dev, *dims, ze, ste, gam, bet, None, pe, ae)
    entries = (
        ("mvp_edge_bn_stats (1 read)", 1, lambda: _lib.call("mvp_edge_bn_stats", dev, *dims, ze, 1e-5, ste, vae, sce, nbe)),
        ("mvp_edge_bn_relu_max, r written (1 read + 1 write)", 2,
         lambda: _lib.call("mvp_edge_bn_relu_max", dev, *dims, ze, ste, gam, bet, re_, pe, ae)),
        ("mvp_edge_bn_relu_max, no r (1 read)", 1,
         lambda: _lib.call("mvp_edge_bn_relu_max", dev, *dims, ze, ste, gam, bet, None, pe, ae)),
        ("mvp_edge_bn_relu_max_backward, g_r + g_pool, batch (4 reads + 1 write)", 5,
         lambda: _lib.call("mvp_edge_bn_relu_max_backward", dev, *dims, 1, ze, ste, gam, bet, ae, gre, gpe, gze, gga, gbe, sce, nbe)),
        ("mvp_edge_bn_relu_max_backward, g_pool only, batch (2 reads + 1 write)", 3,
         lambda: _lib.call("mvp_edge_bn_relu_max_backward", dev, *dims, 1, ze, ste, gam, bet, ae, None, gpe, gze, gga, gbe, sce, nbe)),
    )
    print("  C = %d (%s), T = %.0f MB" % (C, which, T / 1e6), flush=True)
    kernels_alone(entries, T, 10, "    %-74s")
    del ze, gre, gpe, re_, gze
    torch.cuda.empty_cache()

# ---- multi-head attention as one kernel in inference (mvp_benchmark_amd.registration.FUSED_ATTENTION, default off)
attention_block()
