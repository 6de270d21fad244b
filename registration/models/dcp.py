"""Deep Closest Point -- counterpart of the reference's registration/models/dcp.py
(DGCNN :286-318, Transformer :321-345 built from the annotated-transformer
blocks :24-252, SVDHead :348-376, Model :379-429).  BASELINE cfg 5.

The module tree reproduces the reference's parameter names (checkpoints
interchange; tests/golden/dcp_golden.npz pins the layout and a forward pass
generated from the imported reference), the code does not: the transformer is
one generic pre-norm layer class used for both stacks, the edge-convolution
stages are a loop.  On the op layer: DGCNN's k = 20 coordinate kNN and
neighbour gather (knn + grouping operators instead of a (B,N,N) matrix, topk and
advanced indexing) and the SVD head (one mvp_kabsch_svd3 launch instead of B
torch.svd / torch.det calls with a host synchronisation each).  Attention and
the 1x1 convolutions are library GEMMs -- except on DGCNN's opt-in inference route
(mvp_benchmark_amd.registration.EDGE_MLP), which runs the four edge stages and their
maxima as one kernel and conv5 as one MFMA GEMM.  The transformer's LayerNorm and residual sums have an opt-in route of
their own (mvp_benchmark_amd.registration.LAYER_NORM): every `x + f(...)` followed by a norm is one kernel, each way.
DGCNN in training has a third (mvp_benchmark_amd.registration.EDGE_BN): BatchNorm, ReLU and the max over the neighbours of
stages 1-4 as kernels, forward and backward.  Attention in inference has a fourth (mvp_benchmark_amd.registration.FUSED_ATTENTION):
softmax(q k^T / sqrt(d_k)) v for all heads as one kernel between the projections, no score tensor and no head transpose.  Each
module has ONE dataflow: the switches are read in three places, DGCNN._route, LayerNorm.forward and
MultiHeadedAttention._route (mvp_benchmark_amd.registration.routes sets them for a block).
"""
import copy
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sibling(name):
    """registration/<name>.py under the private module name `registration_<name>`: completion/ has
    files of the same names, and a process that already imported those (one test session, a tool
    that touches both trees) must not get them here -- the reference imports them by bare name
    after a sys.path edit (dcp.py:14-19), which only works in a process of its own."""
    import importlib.util
    full = "registration_" + name
    if full in sys.modules:
        return sys.modules[full]
    spec = importlib.util.spec_from_file_location(full, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[full] = mod
    spec.loader.exec_module(mod)
    return mod


_mu = _sibling("model_utils")
get_graph_feature, procrustes = _mu.get_graph_feature, _mu.procrustes
metrics = _sibling("train_utils")
from mvp_benchmark_amd import pointwise as _pw, registration as _reg  # noqa: E402  (model_utils put the root on sys.path)

EMB_DIMS, FF_DIMS, HEADS, STACK_DEPTH = 512, 1024, 4, 1


class LayerNorm(nn.Module):
    """a_2 * (x - mean) / (std + eps) + b_2 with the UNBIASED std and eps added
    to the std -- the reference's own normalisation (:139-149), not nn.LayerNorm."""

    def __init__(self, features, eps=1e-6):
        super().__init__()
        self.a_2 = nn.Parameter(torch.ones(features))
        self.b_2 = nn.Parameter(torch.zeros(features))
        self.eps = eps

    def forward(self, x, residual=None):
        """The norm of z = x (+ residual): y, or (z, y) when a residual is given -- z is the residual stream's next value, so
        `x = x + f(...); h = norm(x)` is one call, whatever the route.  The switch on: ref_layer_norm, one kernel for float32
        CUDA tensors and this formula for every other; off: this formula, no kernel."""
        if _reg.LAYER_NORM:
            return _reg.ref_layer_norm(x, self.a_2, self.b_2, self.eps, residual)
        z = x if residual is None else x + residual
        centred = z - z.mean(-1, keepdim=True)
        y = self.a_2 * centred / (z.std(-1, keepdim=True) + self.eps) + self.b_2
        return y if residual is None else (z, y)


class SublayerConnection(nn.Module):
    """Holder of a pre-norm residual branch's LayerNorm (`norm`)."""

    def __init__(self, size):
        super().__init__()
        self.norm = LayerNorm(size)


class MultiHeadedAttention(nn.Module):
    """Four d x d projections (`linears`: query, key, value, output), HEADS heads."""

    def __init__(self, heads, d_model):
        super().__init__()
        assert d_model % heads == 0
        self.h, self.d_k = heads, d_model // heads
        # the reference builds `clones(nn.Linear(d_model, d_model), 4)` (dcp.py:52-54,167): four deep copies
        # of ONE layer, so the four projections of a block start from identical weights
        proto = nn.Linear(d_model, d_model)
        self.linears = nn.ModuleList([copy.deepcopy(proto) for _ in range(4)])

    def _route(self, query, memory):
        """forward(query, memory)'s route, decided once and launching nothing: a pure function of the switch, grad mode and who
        requires grad (the two inputs, the module's parameters), the inputs' device, dtype and shape.
          "fused"     the three projections, softmax(q k^T / sqrt(d_k)) v for all heads as one kernel
                      (mvp_benchmark_amd.registration.fused_attention), the output projection: FUSED_ATTENTION is on, both
                      inputs are float32 CUDA and 3-D, d_k is a width the kernel covers and nothing asks for a gradient (the
                      route has no backward).
          "composed"  everything else: the switch off, training with gradients, CPU, float64."""
        if not _reg.FUSED_ATTENTION or self.d_k not in _reg.ATTENTION_WIDTHS:
            return "composed"
        if not all(t.dim() == 3 and t.is_cuda and t.dtype == torch.float32 for t in (query, memory)):
            return "composed"
        wanted = torch.is_grad_enabled() and (query.requires_grad or memory.requires_grad
                                              or any(p.requires_grad for p in self.parameters()))
        return "composed" if wanted else "fused"

    def forward(self, query, memory):
        if self._route(query, memory) == "fused":
            q, k, v = self.linears[0](query), self.linears[1](memory), self.linears[2](memory)
            return self.linears[3](_reg.fused_attention(q, k, v, self.h))
        b = query.size(0)
        split = lambda t: t.view(b, -1, self.h, self.d_k).transpose(1, 2)
        q = split(self.linears[0](query))
        k = split(self.linears[1](memory))
        v = split(self.linears[2](memory))
        weights = F.softmax(q @ k.transpose(-2, -1) / math.sqrt(self.d_k), dim=-1)
        mixed = (weights @ v).transpose(1, 2).reshape(b, -1, self.h * self.d_k)
        return self.linears[3](mixed)


class PositionwiseFeedForward(nn.Module):
    def __init__(self, d_model, d_ff):
        super().__init__()
        self.w_1 = nn.Linear(d_model, d_ff)
        self.norm = nn.Sequential()          # empty in the reference as well (no parameters)
        self.w_2 = nn.Linear(d_ff, d_model)

    def forward(self, x):
        return self.w_2(F.relu(self.w_1(x)))


class TransformerLayer(nn.Module):
    """Pre-norm layer: self-attention, (decoder only) attention over the other
    cloud's encoding, feed-forward; every branch is x + f(norm(x))."""

    def __init__(self, size, self_attn, feed_forward, src_attn=None):
        super().__init__()
        self.size = size
        self.self_attn = self_attn
        if src_attn is not None:
            self.src_attn = src_attn
        self.feed_forward = feed_forward
        self.sublayer = nn.ModuleList([SublayerConnection(size) for _ in range(2 if src_attn is None else 3)])

    def forward(self, x, memory=None):
        x, last = self.branches(x, memory)
        return x + last

    def branches(self, x, memory=None, pending=None):
        """The layer's one body: every branch's output is the `residual` of the NEXT norm, which adds it to the stream and
        normalises the sum (one kernel on the fused route).  `pending`: the previous layer's last branch, not yet added to x.
        -> (x, last): the layer's output is x + last, left to whoever normalises it next (LayerStack) or to forward."""
        norm = lambda i, x, branch: (x, self.sublayer[i].norm(x)) if branch is None else self.sublayer[i].norm(x, branch)
        x, h = norm(0, x, pending)
        branch = self.self_attn(h, h)
        i = 1
        if memory is not None:
            x, h = norm(1, x, branch)
            branch = self.src_attn(h, memory)
            i = 2
        x, h = norm(i, x, branch)
        return x, self.feed_forward(h)


class LayerStack(nn.Module):
    def __init__(self, layer, depth):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(depth)])
        self.norm = LayerNorm(layer.size)

    def forward(self, x, memory=None):
        pending = None                    # a layer's last sum joins the next layer's first norm, or the final one
        for layer in self.layers:
            x, pending = layer.branches(x, memory, pending)
        return self.norm(x) if pending is None else self.norm(x, pending)[1]


class EncoderDecoder(nn.Module):
    """decoder(tgt | encoder(src)); the embedding / generator slots of the
    annotated transformer exist (empty) so that the module tree matches."""

    def __init__(self, encoder, decoder):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.src_embed = nn.Sequential()
        self.tgt_embed = nn.Sequential()
        self.generator = nn.Sequential()

    def forward(self, src, tgt):
        return self.decoder(tgt, self.encoder(src))


class DGCNN(nn.Module):
    """Four edge-convolution stages over the k = 20 coordinate neighbourhood
    (6 -> 64 -> 64 -> 128 -> 256 channels, BatchNorm + ReLU, max over the
    neighbours after each), their maxima concatenated and mapped to emb_dims."""

    WIDTHS = (6, 64, 64, 128, 256)

    def __init__(self, emb_dims=EMB_DIMS):
        super().__init__()
        stages = list(zip(self.WIDTHS[:-1], self.WIDTHS[1:])) + [(sum(self.WIDTHS[1:]), emb_dims)]
        for i, (c_in, c_out) in enumerate(stages, start=1):       # parameters conv1..5 first, then bn1..5
            setattr(self, "conv%d" % i, nn.Conv2d(c_in, c_out, kernel_size=1, bias=False))
        for i, (_, c_out) in enumerate(stages, start=1):
            setattr(self, "bn%d" % i, nn.BatchNorm2d(c_out))

    def _stage(self, i, x):
        return F.relu(getattr(self, "bn%d" % i)(getattr(self, "conv%d" % i)(x)))

    def _route(self, x):
        """forward(x)'s route, decided once and launching nothing: a pure function of the two switches, self.training, grad
        mode and who requires grad, x's device, dtype and shape, and the BatchNorm configuration.
          "edge_mlp"  stages 1-4 and their maxima as one kernel (mvp_benchmark_amd.registration.edge_mlp_max), then conv5 as one
                      MFMA GEMM: EDGE_MLP is on, BatchNorm uses its running statistics (eval) and nothing asks for a gradient
                      (the route has no backward); x has at most 4 channels and rows of whole 16-byte groups.
          "edge_bn"   BatchNorm, ReLU and the max of stages 1-4 as kernels (mvp_benchmark_amd.registration.bn_relu_max): EDGE_BN
                      is on, the module trains or some gradient is needed, and bn1..bn4 track their running statistics with a
                      float momentum.
          "composed"  everything else: both switches off, CPU, float64.
        "edge_mlp" needs eval AND no gradient wanted, "edge_bn" training OR a gradient wanted: never both, whatever the switches."""
        if not (_reg.EDGE_MLP or _reg.EDGE_BN) or x.dim() != 3 or not (x.is_cuda and x.dtype == torch.float32):
            return "composed"
        wanted = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not (self.training or wanted):
            return "edge_mlp" if _reg.EDGE_MLP and x.size(1) <= 4 and x.size(2) % 4 == 0 else "composed"
        bns = [getattr(self, "bn%d" % i) for i in range(1, 5)]
        tracked = all(bn.track_running_stats and bn.running_mean is not None and isinstance(bn.momentum, float) for bn in bns)
        return "edge_bn" if _reg.EDGE_BN and tracked else "composed"

    def _forward_fused(self, x):
        """BatchNorm in eval mode is the per-channel map scale * t + shift; stages 1-4 and their maxima are one kernel, the
        scale of stage 5 goes into conv5's weight and its shift is the GEMM's bias.  Nothing is kept between calls."""
        bns = [getattr(self, "bn%d" % i) for i in range(1, 6)]
        widths = [bn.num_features for bn in bns]
        assert all(bn.eps == bns[0].eps for bn in bns)
        scale = torch.cat([bn.weight for bn in bns]) / torch.sqrt(torch.cat([bn.running_var for bn in bns]) + bns[0].eps)
        shift = torch.cat([bn.bias for bn in bns]) - torch.cat([bn.running_mean for bn in bns]) * scale
        scales, shifts = scale.split(widths), shift.split(widths)
        idx = _mu.knn(x, 20).transpose(1, 2)                          # (B, k, N)
        pooled = _reg.edge_mlp_max(x, idx, [getattr(self, "conv%d" % i).weight for i in range(1, 5)], scales[:4], shifts[:4])
        w5 = self.conv5.weight.view(widths[4], -1) * scales[4].unsqueeze(1)
        return _pw.mfma_linear(pooled, w5.contiguous(), bias=shifts[4].contiguous(), relu=True)

    def _stage_edge_bn(self, i, edge, want_r):
        """conv_i, then BatchNorm + ReLU + max over k in one operator -> (relu(bn(conv(edge))) or None, its maximum (B,C,N));
        num_batches_tracked counts as nn.BatchNorm2d counts it."""
        bn = getattr(self, "bn%d" % i)
        z = getattr(self, "conv%d" % i)(edge)
        if bn.training:
            bn.num_batches_tracked.add_(1)
        return _reg.bn_relu_max(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, bn.momentum, bn.eps, want_r)

    def forward(self, x):
        route = self._route(x)
        if route == "edge_mlp":
            return self._forward_fused(x.detach())
        batch_size, _, num_points = x.size()
        # (B, 6, 20, N): knn + grouping operators; neighbours on the SLOW spatial axis (the stages are
        # 1x1 convolutions + per-channel BatchNorm: layout-agnostic; the reference keeps (B, 6, N, 20))
        edge = get_graph_feature(x, k_major=True)
        pooled = []
        for i in range(1, 5):
            if route == "edge_bn":                                    # stage 4's activations feed only their maximum
                edge, top = self._stage_edge_bn(i, edge, want_r=i < 4)
                pooled.append(top.unsqueeze(2))
            else:
                edge = self._stage(i, edge)
                pooled.append(edge.max(dim=2, keepdim=True)[0])       # (B, C, 1, N)
        return self._stage(5, torch.cat(pooled, dim=1)).view(batch_size, -1, num_points)


class Transformer(nn.Module):
    """The "pointer": each cloud's embedding attends to the other's."""

    def __init__(self, args):
        super().__init__()
        self.emb_dims, self.N, self.dropout, self.ff_dims, self.n_heads = EMB_DIMS, STACK_DEPTH, 0.0, FF_DIMS, HEADS
        # one prototype of each block, deep-copied into place: all attention blocks start from the
        # same weights, as in the reference (:331-337)
        attn = MultiHeadedAttention(HEADS, EMB_DIMS)
        ff = PositionwiseFeedForward(EMB_DIMS, FF_DIMS)
        dup = copy.deepcopy
        self.model = EncoderDecoder(
            LayerStack(TransformerLayer(EMB_DIMS, dup(attn), dup(ff)), STACK_DEPTH),
            LayerStack(TransformerLayer(EMB_DIMS, dup(attn), dup(ff), src_attn=dup(attn)), STACK_DEPTH))

    def forward(self, src, tgt):
        src, tgt = src.transpose(2, 1).contiguous(), tgt.transpose(2, 1).contiguous()
        tgt_embedding = self.model(src, tgt).transpose(2, 1).contiguous()
        src_embedding = self.model(tgt, src).transpose(2, 1).contiguous()
        return src_embedding, tgt_embedding


class SVDHead(nn.Module):
    """Soft correspondences (softmax of the embedding products), then the rigid
    motion that carries src onto them: one batched 3x3 SVD launch."""

    def __init__(self, args):
        super().__init__()
        self.emb_dims = EMB_DIMS
        reflect = torch.eye(3)
        reflect[2, 2] = -1
        self.reflect = nn.Parameter(reflect, requires_grad=False)   # unused here, kept: part of the checkpoint

    def forward(self, src_embedding, tgt_embedding, src, tgt):
        logits = src_embedding.transpose(2, 1) @ tgt_embedding / math.sqrt(src_embedding.size(1))
        src_corr = tgt @ torch.softmax(logits, dim=2).transpose(2, 1)
        return procrustes(src, src_corr)


class Model(nn.Module):
    """forward(src (B,N,3), tgt (B,N,3)[, T_gt (B,4,4)]) -> T_12 (B,4,4); with
    T_gt: (loss, r_err, t_err, rmse, rt_mse) as the reference (:391-429)."""

    def __init__(self, args):
        super().__init__()
        self.emb_dims = EMB_DIMS
        self.cycle = False
        self.emb_nn = DGCNN(emb_dims=EMB_DIMS)
        self.pointer = Transformer(args=args)
        self.head = SVDHead(args=args)

    def forward(self, src, tgt, T_gt=None, prefix="train"):
        cloud_src = src
        src = src.transpose(1, 2).contiguous()
        tgt = tgt.transpose(1, 2).contiguous()
        f_src, f_tgt = self.emb_nn(src), self.emb_nn(tgt)
        p_src, p_tgt = self.pointer(f_src, f_tgt)
        rotation, translation = self.head(f_src + p_src, f_tgt + p_tgt, src, tgt)
        T_12 = metrics.rt_to_transformation(rotation, translation.unsqueeze(2))
        if T_gt is None:
            return T_12
        R, t, R_gt, t_gt = T_12[:, :3, :3], T_12[:, :3, 3], T_gt[:, :3, :3], T_gt[:, :3, 3]
        t_err = metrics.translation_error(t, t_gt)
        identity = torch.eye(4, device=T_gt.device).expand_as(T_gt)
        loss = F.mse_loss(T_12 @ torch.inverse(T_gt), identity)
        return (loss, metrics.rotation_error(R, R_gt), t_err, metrics.rmse_loss(cloud_src, T_12, T_gt),
                metrics.rotation_geodesic_error(R, R_gt) + t_err)
