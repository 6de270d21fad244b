"""DeepGMR registration at its cfg (registration/cfgs/deepgmr.yaml): 32 pairs of 2048 points, RRI features of
k = 20 neighbours, 16 mixture components, one MI355X -- forward (eval) and forward + backward (training step without
the optimizer) timings, with the op-layer split from the torch profiler (kNN, RRI, GMM forward / backward, Kabsch
SVD3).  Same-box comparison: this repository's torch restatement of the reference's RRI (the CPU fallback of
mvp_benchmark_amd.registration.rri_features, one cloud at a time) timed on the host, on the same clouds and
neighbours -- the reference itself computes that part with NumPy on the host.
   python tools/bench_deepgmr.py            (MVP_BENCH_REPS: timed repetitions)"""
import math, os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = os.path.join(ROOT, "registration")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(REG, "models"))
import torch
import deepgmr
from mvp_benchmark_amd.registration import _rri_reference, rri_features

REPS = int(os.environ.get("MVP_BENCH_REPS", "10"))
dev = "cuda:0"
B, N, K, J = 32, 2048, 20, 16
torch.manual_seed(0)
net = deepgmr.Model(types.SimpleNamespace(use_rri=True, rri_size=K, num_groups=J, use_tnet=False)).to(dev)
g = torch.Generator().manual_seed(5)
pts1 = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev)
q = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=1).to(dev)
Rg = deepgmr.metrics.quat2mat(q)
tg = (torch.rand(B, 3, generator=g) - 0.5).to(dev)
pts2 = pts1 @ Rg.transpose(1, 2) + tg.unsqueeze(1)
T_gt = deepgmr.metrics.rt_to_transformation(Rg, tg.unsqueeze(2))


def timed(fn, reps=REPS):
    fn(); fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def fwd():
    with torch.no_grad():
        return net(pts1, pts2, prefix="test")


def fwd_bwd():
    net.zero_grad(set_to_none=True)
    net(pts1, pts2, T_gt)[0].backward()


net.eval()
ms_f = timed(fwd)
net.train()
ms_fb = timed(fwd_bwd)
ms_rri = timed(lambda: rri_features(pts1, K))
print("DeepGMR cfg (%d pairs x %d points, k = %d RRI, %d components, %.2f M parameters): forward %.2f ms "
      "(%.0f pairs/s), forward + backward %.2f ms (%.0f pairs/s); rri_features alone (kNN + kernel, one cloud "
      "batch) %.3f ms" % (B, N, K, J, sum(p.numel() for p in net.parameters()) / 1e6, ms_f, B / ms_f * 1e3, ms_fb,
                          B / ms_fb * 1e3, ms_rri), flush=True)

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
    knn = share("knn_kernel", "knn_sorted")
    rri = share("rri_features_kernel")
    gmm_f = share("gmm_softmax_kernel", "gmm_moments_kernel")
    gmm_b = share("gmm_backward_kernel")
    svd = share("svd3")
    print("  %s: GPU time %.2f ms per step = kNN %.3f + RRI %.3f + GMM forward %.3f + GMM backward %.3f + "
          "Kabsch SVD3 %.3f + everything else (library GEMMs / BatchNorm / elementwise) %.2f" % (
              name, total, knn, rri, gmm_f, gmm_b, svd, total - knn - rri - gmm_f - gmm_b - svd), flush=True)
    for r in sorted(rows, key=lambda r: -r[1])[:8]:
        print("      %-90s %8.3f ms x%d" % (r[0][:90], r[1], r[2]), flush=True)

# the host-side comparison: this repository's torch restatement of the reference's RRI, float32, on the CPU
from mvp_benchmark_amd.mm3d_pn2 import knn
idx = knn(K + 1, pts1)[:, 1:, :].transpose(1, 2).contiguous().long().cpu()
x = pts1.cpu()
torch.set_num_threads(min(16, torch.get_num_threads()))
t0 = time.perf_counter()
host = _rri_reference(x, idx)
ms_host = (time.perf_counter() - t0) * 1e3
dev_feat = rri_features(pts1, K).cpu()
print("  RRI of one cloud batch (%d x %d, k = %d): GPU kernel + kNN %.3f ms; this repository's torch restatement of "
      "the reference's RRI on the host (%d threads, same neighbours) %.0f ms (%.0fx); rp/rq/theta max |diff| %.1e" % (
          B, N, K, ms_rri, torch.get_num_threads(), ms_host, ms_host / ms_rri,
          (host.view(B, K, 4, N)[:, :, :3] - dev_feat.view(B, K, 4, N)[:, :, :3]).abs().max().item()), flush=True)
