"""Same-process A/B of the op-layer switch `dense_edge_conv` (completion/op_config.py): ECG's Dense_conv with its
per-edge work in one kernel each way (mvp_dense_edge_conv) against the composed route.

  * Dense_conv forward and forward + backward at the four level shapes of EF_encoder at the default cfg
    (B = 32; (C, N) = (24, 3072), (48, 1024), (48, 256), (48, 64); growth 24, dense_n 3, k 16)
  * the ECG training step (batch 32, 2048 input points)

ONE module / network per item, the two settings alternated ROUNDS times (>= 5), REPS timed runs each after two untimed
ones: per-round times, medians, spread (max - min over the rounds), launches per step and peak memory, both ways.
The switch-off leg is the code of the parent commit.

    python tools/bench_dense_edge_conv.py [rounds] [ecg warm-up steps] > profiles/dense_edge_conv.txt"""
import importlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "completion"))
import torch
import train
import op_config
from models.edge_unet import Dense_conv

ROUNDS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 6
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 150
REPS = int(os.environ.get("MVP_BENCH_REPS", "10"))
dev = "cuda:0"
gen = torch.Generator().manual_seed(0)


def timed(fn, fused):
    op_config.OPS.reset(); op_config.configure(dense_edge_conv=fused)
    fn(); fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e3


def launches(fn, fused):
    from torch.profiler import profile, ProfilerActivity
    op_config.OPS.reset(); op_config.configure(dense_edge_conv=fused)
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(); torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))


def peak_mb(fn, fused):
    op_config.OPS.reset(); op_config.configure(dense_edge_conv=fused)
    fn(); torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn(); torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def ab(title, fn):
    off, on = [], []
    for _ in range(ROUNDS):
        off.append(timed(fn, False)); on.append(timed(fn, True))
    m_off, m_on = statistics.median(off), statistics.median(on)
    print(title)
    print("  off  %s  median %.3f ms  spread %.3f" % (" ".join("%.3f" % t for t in off), m_off, max(off) - min(off)))
    print("  on   %s  median %.3f ms  spread %.3f" % (" ".join("%.3f" % t for t in on), m_on, max(on) - min(on)))
    print("  on - off: %+.3f ms (%+.1f %%)" % (m_on - m_off, 100 * (m_on / m_off - 1)))
    try:
        print("  launches: off %d, on %d" % (launches(fn, False), launches(fn, True)))
    except Exception as e:      # (the profiler is optional)
        print("  launch count unavailable:", e)
    print("  peak memory: off %.0f MiB, on %.0f MiB" % (peak_mb(fn, False), peak_mb(fn, True)), flush=True)
    return m_off, m_on, max(max(off) - min(off), max(on) - min(on))


print("dense_edge_conv A/B on %s: %d alternations x %d runs" % (torch.cuda.get_device_name(0), ROUNDS, REPS))
for C, N in ((24, 3072), (48, 1024), (48, 256), (48, 64)):
    dc = Dense_conv(C, growth_rate=24, dense_n=3, k=16).to(dev)
    x = torch.randn(32, C, N, generator=gen).to(dev).requires_grad_(True)
    go = torch.randn(32, C + 72, N, generator=gen).to(dev)

    def fwd():
        with torch.no_grad():
            dc(x)

    def fwd_bwd():
        dc.zero_grad(set_to_none=True); x.grad = None
        dc(x).backward(go)

    ab("Dense_conv(%d, 24, 3, 16) on (32, %d, %d) forward" % (C, C, N), fwd)
    ab("Dense_conv(%d, 24, 3, 16) on (32, %d, %d) forward + backward" % (C, C, N), fwd_bwd)
    del dc, x, go

args = train.load_config(os.path.join(ROOT, "completion", "cfgs", "ecg.yaml")); args.load_model = None
net = importlib.import_module("models.ecg").Model(args).to(dev).train()
opt = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True)
gt = torch.rand(32, 2048, 3, generator=gen).to(dev); partial = gt.transpose(2, 1).contiguous()


def step():
    opt.zero_grad(); _, _, loss = net(partial, gt, alpha=0.5); loss.backward(); opt.step()


for fused in (False, True):     # ECG settles late (tools/bench_models.py): the same long warm-up for both settings
    op_config.OPS.reset(); op_config.configure(dense_edge_conv=fused)
    for _ in range(WARMUP):
        step()
m_off, m_on, spread = ab("ECG training step (batch 32, 2048 points), %d warm-up steps per setting" % WARMUP, step)
print("verdict: the step is %s with the switch on (%.3f -> %.3f ms; the run's own spread is %.3f ms)"
      % ("faster by more than the spread" if m_off - m_on > spread else
         "slower by more than the spread" if m_on - m_off > spread else "within the spread", m_off, m_on, spread))
op_config.OPS.reset()
