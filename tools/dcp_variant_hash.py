"""Digest of DCP's norm, edge and attention kernels of one library build on fixed seeded inputs:
   python tools/dcp_variant_hash.py [lib.so]
One line per case, a sha1 over the raw bytes of every output of mvp_edge_bn_stats, mvp_edge_bn_relu_max (with and without
r), mvp_edge_bn_relu_max_backward (batch and running statistics; g_r / g_pool each absent once), mvp_ref_layernorm (with and
without delta), mvp_ref_layernorm_backward (with and without gres, with and without ga / gb), mvp_edge_mlp_max and
mvp_attention_forward (every shape of tests/attention_cases.py, the four random families and the two exact ones).  Two
builds whose kernels compute the same bits print the same lines (the -m gpu tests hold the default library to its bounds)."""
import sys, os, hashlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from mvp_benchmark_amd import _lib
if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
import attention_cases, edge_bn_cases, edge_mlp_cases, layer_norm_cases

dev = torch.device("cuda:0")
LOOPING = (4 * 2048 + 5, 4)                      # tests/test_gpu_layer_norm.py: more rows than the grid has waves
EDGE_D = (252, 260, 768, 772)                    # either side of NV = 1 | 2 and of the backward kernel's kHold (NV = 3 | 4)


class Digest:
    def __init__(self):
        self.h = hashlib.sha1()

    def add(self, *tensors):
        torch.cuda.synchronize()
        for t in tensors:
            self.h.update(t.cpu().contiguous().numpy().tobytes())

    def line(self, name):
        print("%-44s %s" % (name, self.h.hexdigest()[:16]), flush=True)


def nan(*shape):
    return torch.full(shape, float("nan"), device=dev)


def edge_bn(shape):
    B, C, k, N = shape
    dg = Digest()
    nbytes = _lib.edge_bn_scratch_bytes(B, C)
    scratch = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    for family in edge_bn_cases.FAMILIES:
        c = {key: v.to(dev) for key, v in edge_bn_cases.make_case(shape, family).items()}
        stats, var = nan(C, 2), nan(C)
        _lib.call("mvp_edge_bn_stats", dev, B, C, k, N, c["z"], edge_bn_cases.EPS, stats, var, scratch, nbytes)
        dg.add(stats, var)
        running = torch.stack((c["running_mean"], (1 / torch.sqrt(c["running_var"].double() + edge_bn_cases.EPS)).float()), dim=1).contiguous()
        for batch, st in ((1, stats), (0, running)):
            r, pooled = nan(B, C, k, N), nan(B, C, N)
            arg = torch.full((B, C, N), 255, device=dev, dtype=torch.uint8)
            _lib.call("mvp_edge_bn_relu_max", dev, B, C, k, N, c["z"], st, c["gamma"], c["beta"], r, pooled, arg)
            dg.add(r, pooled, arg)
            pooled_n, arg_n = nan(B, C, N), torch.full_like(arg, 255)
            _lib.call("mvp_edge_bn_relu_max", dev, B, C, k, N, c["z"], st, c["gamma"], c["beta"], None, pooled_n, arg_n)
            dg.add(pooled_n, arg_n)
            for g_r, g_pool in ((c["g_r"], c["g_pool"]), (None, c["g_pool"]), (c["g_r"], None)):
                gz, ggamma, gbeta = nan(B, C, k, N), nan(C), nan(C)
                _lib.call("mvp_edge_bn_relu_max_backward", dev, B, C, k, N, batch, c["z"], st, c["gamma"], c["beta"], arg,
                          g_r, g_pool, gz, ggamma, gbeta, scratch, nbytes)
                dg.add(gz, ggamma, gbeta)
    dg.line("edge_bn %s" % (shape,))


def layer_norm(rows, d):
    dg = Digest()
    nbytes = _lib.ref_layernorm_backward_scratch_bytes(rows, d)
    scratch = torch.zeros(max(nbytes, 16), device=dev, dtype=torch.uint8)
    for family in layer_norm_cases.FAMILIES:
        c = {key: v.to(dev) for key, v in layer_norm_cases.make_case(rows, d, family).items()}
        for delta in (c["delta"], None):
            total = None if delta is None else nan(rows, d)
            y, stats = nan(rows, d), nan(rows, 2)
            _lib.call("mvp_ref_layernorm", dev, rows, d, c["x"], delta, c["a"], c["b"], layer_norm_cases.EPS, total, y, stats)
            dg.add(y, stats, *(() if total is None else (total,)))
            z = c["x"] if total is None else total
            for gres in (c["gres"], None):
                for cols in (True, False):
                    gz = nan(rows, d)
                    ga, gb = (nan(d), nan(d)) if cols else (None, None)
                    _lib.call("mvp_ref_layernorm_backward", dev, rows, d, z, c["a"], c["gy"], gres, stats, layer_norm_cases.EPS,
                              gz, ga, gb, scratch if cols else None, nbytes if cols else 0)
                    dg.add(gz, *((ga, gb) if cols else ()))
    dg.line("layer_norm (%d, %d)" % (rows, d))


def edge_mlp(shape, pattern):
    case = edge_mlp_cases.make_case(shape, pattern, "random")
    x, idx = case["x"].to(dev), case["idx"].to(dev)
    B, c, N = x.shape
    widths = [W.shape[0] for W in case["weights"]]
    w = torch.cat([W.reshape(-1) for W in case["weights"]]).to(dev)
    scale, shift = torch.cat(case["scales"]).to(dev), torch.cat(case["shifts"]).to(dev)
    out = nan(B, sum(widths), N)
    _lib.call("mvp_edge_mlp_max", dev, B, c, N, idx.shape[1], len(widths), *(widths + [0] * (4 - len(widths))), x, idx, w,
              scale, shift, out)
    dg = Digest()
    dg.add(out)
    dg.line("edge_mlp %s %s" % (shape, pattern))


def attention(shape):
    B, H, Nq, Nk, D = shape
    dg = Digest()
    cases = [attention_cases.inputs(shape, family) for family in attention_cases.FAMILIES]
    cases += [attention_cases.exact_inputs(shape, family)[:3] for family in attention_cases.EXACT_FAMILIES]
    for q, k, v in cases:
        q, k, v = (attention_cases.packed(t).to(dev) for t in (q, k, v))
        out = nan(B, Nq, H * D)
        _lib.call("mvp_attention_forward", dev, B, H, Nq, Nk, D, q, k, v, attention_cases.default_scale(shape), out)
        dg.add(out)
    dg.line("attention %s" % (shape,))


for shape in edge_bn_cases.SHAPES:
    edge_bn(shape)
for rows, d in [(rows, d) for rows in layer_norm_cases.ROWS for d in layer_norm_cases.DIMS] + [(257, d) for d in EDGE_D] + [LOOPING]:
    layer_norm(rows, d)
edge_mlp(edge_mlp_cases.SHAPES[1], "random")
for shape in attention_cases.SHAPES:
    attention(shape)
