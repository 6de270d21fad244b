"""The registration models' op layer: what registration/models/{dcp,deepgmr}.py run on HIP kernels, each with the same
composition written in torch for CPU / float64 tensors (the float64 equivalence tests run on it).  In file order:

  Kabsch rotation      kabsch_rotation, svd3, svd3_kabsch_backward             mvp_kabsch_svd3
  DeepGMR              rri_features, gmm_params, gmm_register                  mvp_rri_features, mvp_gmm_params[_backward]
  DCP's switches       EDGE_MLP, LAYER_NORM, EDGE_BN, FUSED_ATTENTION (all off) and routes(), the one way to flip them for a block
  DGCNN, inference     edge_mlp_max                                            mvp_edge_mlp_max
  the transformer      ref_layer_norm (LayerNorm + the residual sum)           mvp_ref_layernorm[_backward]
  DGCNN, training      bn_relu_max (BatchNorm + ReLU + max over k)             mvp_edge_bn_stats, mvp_edge_bn_relu_max[_backward]
  attention, inference fused_attention (softmax(q k^T scale) v, all heads)     mvp_attention_forward

`kabsch_rotation(H)` replaces the per-sample loop of the reference's SVDHead
(registration/models/dcp.py:360-373, registration/model_utils.py:229-240):

    for i in range(B):
        u, s, v = torch.svd(H[i]); r = v @ u.T
        if det(r) < 0: v = v @ diag(1, 1, -1); r = v @ u.T

B tiny LAPACK-style calls with a host synchronisation each become ONE launch of
mvp_kabsch_svd3 (one lane per matrix, float64 one-sided Jacobi).  Differentiable:
the backward pass is a closed-form adjoint on (B,3,3) tensors (batched
elementwise / 3x3 matmul PyTorch ops, device-agnostic, no loop, no sync) -- the
gradient torch.svd's autograd produces for R = V D U^T with the reflection D held
fixed, in a form without that autograd's removable poles.

Domain of the gradient: R is smooth, and svd3_kabsch_backward finite and accurate
(32 * 2^-24 * max|grad_R| / min(s_i + e_ij s_j) in float32), wherever the two
smallest singular values do not cancel: every H with det H > 0 down to rank 2,
coinciding singular values included, and every H with det H < 0 whose s_3 stays
below s_2.  s_2 = s_3 with det H < 0 and rank <= 1 are poles of R itself: that
sample's gradient is inf / NaN, the rest of the batch is unaffected.
"""
import contextlib
import math

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import call, edge_bn_scratch_bytes, ref_layernorm_backward_scratch_bytes


def svd3_kabsch_backward(U, S, V, flipped, grad_R):
    """Adjoint of H -> R = V diag(1,1,d) U^T  (H = U diag(S) V^T, d = -1 where
    `flipped`) for batches of 3x3 matrices: returns grad_H (B,3,3).

    With dU = U Wu, dV = V Wv (Wu, Wv skew):
        P = U^T dH V = Wu S - S Wv + dS,      W = V^T dR U = Wv D - D Wu.
    For a != b the pair (P_ab, P_ba) determines (Wu_ab, Wv_ab) through a 2x2 system of determinant s_b^2 - s_a^2;
    in W_ab = d_b Wv_ab - d_a Wu_ab one factor of that determinant cancels (e_ab = d_a d_b):
        W_ab = d_b (P_ba / (s_b + e_ab s_a) - P_ab / (s_a + e_ab s_b)),      W_aa = 0,
    so with Q = V^T gR U and <gR, dR> = <Q, W> = <G, P>:
        G_ab = (d_a Q_ba - d_b Q_ab) / (s_a + e_ab s_b)   (a != b),   G_aa = 0,      gH = U G V^T.
    The denominators are s_a + s_b between unflipped directions and s_a - s_3 against a flipped third one: the
    formula is singular exactly where R is -- s_2 = s_3 (or s_1 = s_3) with det H < 0, and rank <= 1 -- and nowhere
    else; s_1 = s_2, and s_2 = s_3 with det H > 0, are ordinary points (the general SVD adjoint, which divides by
    s_b^2 - s_a^2, has removable poles there: NaN at an exact coincidence, float32 noise of 6e-8 / gap near one).
    At a true pole the sample's own gradient is inf or NaN (IEEE division, nothing masked); no other sample of the
    batch is touched.  float32 error on clustered spectra: tests/test_kabsch_cpu.py."""
    d = torch.ones_like(S)
    d[:, 2] = torch.where(flipped.bool(), -torch.ones_like(S[:, 2]), torch.ones_like(S[:, 2]))
    Q = V.transpose(1, 2) @ grad_R @ U
    off = 1 - torch.eye(3, dtype=S.dtype, device=S.device)
    den = S.unsqueeze(2) + (d.unsqueeze(2) * d.unsqueeze(1)) * S.unsqueeze(1)     # s_a + e_ab s_b
    num = d.unsqueeze(2) * Q.transpose(1, 2) - d.unsqueeze(1) * Q
    G = torch.where(off.bool(), num / den, torch.zeros_like(num))                 # G_aa = 0 (0 / 0 at s_a = 0)
    return U @ G @ V.transpose(1, 2)


def _svd3_launch(H):
    """One mvp_kabsch_svd3 launch on H (B,3,3) -> (U, S, V, R, flipped), float32 (flipped int32)."""
    H = H.contiguous().float()
    b = H.shape[0]
    R, U, V = torch.empty_like(H), torch.empty_like(H), torch.empty_like(H)
    S = torch.empty(b, 3, device=H.device, dtype=torch.float32)
    flipped = torch.empty(b, device=H.device, dtype=torch.int32)
    call("mvp_kabsch_svd3", H.device, b, H, R, U, S, V, flipped)
    return U, S, V, R, flipped


class KabschSVD(Function):
    """H (B,3,3) float32 CUDA -> R (B,3,3): mvp_kabsch_svd3."""

    @staticmethod
    def forward(ctx, H):
        assert H.dim() == 3 and H.shape[1:] == (3, 3)
        U, S, V, R, flipped = _svd3_launch(H)
        ctx.save_for_backward(U, S, V, flipped)
        return R

    @staticmethod
    def backward(ctx, grad_R):
        U, S, V, flipped = ctx.saved_tensors
        return svd3_kabsch_backward(U, S, V, flipped, grad_R.contiguous())


kabsch_rotation = KabschSVD.apply


def svd3(H):
    """(U, S, V, R, flipped) of a batch of 3x3 matrices (no autograd): the
    factors torch.svd would return plus the Kabsch rotation."""
    return _svd3_launch(H)


# ---------------------------------------------------------------------------------------------------- DeepGMR
# registration/models/deepgmr.py's two op-layer pieces: the RRI features of every point and the moments of the soft
# Gaussian mixture (mvp_rri_features, mvp_gmm_params[_backward]); gmm_register closes the loop with kabsch_rotation.
# float32 CUDA tensors run the kernels; CPU / float64 tensors take the reference's formulation written in torch (the
# float64 equivalence tests run on it).

def _on_op_layer(t):
    return t.is_cuda and t.dtype == torch.float32


def _kernel_reads(tensors, aligned):
    """Whether a kernel takes these tensors as they are: float32 CUDA, contiguous, all on one device, and those of `aligned`
    on 16-byte addresses (the kernels load them four floats at a time)."""
    return (all(_on_op_layer(t) and t.is_contiguous() and t.device == tensors[0].device for t in tensors)
            and all(t.data_ptr() % 16 == 0 for t in aligned))


def _scratch(nbytes, device):
    """A kernel's (scratch, nbytes) argument pair: a fresh byte buffer, None where it asks for none."""
    return (torch.empty(nbytes, device=device, dtype=torch.uint8) if nbytes else None), nbytes


def _knn_reference(xyz, k):
    """(B,N,3) -> (B,N,k) int64: topk of the negated expanded squared distance (deepgmr.py:10-15), self included."""
    inner = -2 * xyz @ xyz.transpose(1, 2)
    xx = (xyz * xyz).sum(dim=2, keepdim=True)
    return (-xx - inner - xx.transpose(1, 2)).topk(k=k, dim=-1)[1]


def _rri_reference(xyz, idx):
    """get_rri_cluster (deepgmr.py:54-96) in torch, one cloud at a time so the (N,k,k,3) temporaries stay per cloud:
    xyz (B,N,3), idx (B,N,k) -> (B,4k,N).  phi = the second smallest psi of each row (np.argpartition(psi, 1))."""
    B, N, k = idx.shape
    out = []
    for b in range(B):
        p = xyz[b].unsqueeze(1).expand(N, k, 3)
        q = xyz[b][idx[b]]                                        # (N,k,3)
        rp = torch.norm(p, dim=-1, keepdim=True)
        rq = torch.norm(q, dim=-1, keepdim=True)
        pn = p / rp
        dot = (pn * (q / rq)).sum(dim=-1, keepdim=True)
        theta = torch.acos(dot.clamp(-1, 1))
        T = q - dot * p
        # [i, a, b]: sin = (T_b x T_a) . p^, cos = T_b . T_a (np.cross(T_q[:, :, None], T_q[:, :, :, None]))
        # (the cross product spelled out like np.cross: torch.linalg.cross may contract into fmas, and then
        # T_a x T_a is not exactly 0 and psi[a, a] leaves the multiset's bottom)
        Tb, Ta = T.unsqueeze(1), T.unsqueeze(2)
        cross = torch.stack([Tb[..., 1] * Ta[..., 2] - Tb[..., 2] * Ta[..., 1],
                             Tb[..., 2] * Ta[..., 0] - Tb[..., 0] * Ta[..., 2],
                             Tb[..., 0] * Ta[..., 1] - Tb[..., 1] * Ta[..., 0]], dim=-1)
        sin_psi = (cross * pn.unsqueeze(1)).sum(dim=-1)
        cos_psi = (Tb * Ta).sum(dim=-1)
        psi = torch.remainder(torch.atan2(sin_psi, cos_psi), 2 * math.pi)
        phi = psi.sort(dim=-1).values[:, :, 1:2]
        out.append(torch.cat([rp, rq, theta, phi], dim=-1).reshape(N, 4 * k).t())
    return torch.stack(out)


def rri_features(xyz, k):
    """Rotation-reference-invariant features of every point (get_rri_cluster, deepgmr.py:54-96, with one cluster):
    xyz (B,N,3) -> (B,4k,N), channel 4a+f = {rp, rq, theta, phi}[f] of neighbour slot a.  Returned detached: the
    reference's phi goes through NumPy, so no gradient ever reaches the points.

    Neighbours: the knn operator with k+1, first slot dropped.  It stands in for the reference's topk of the expanded
    distance (deepgmr.py:10-15); the two agree except where rounding ties two distances, exactly as for DCP's graph.
    With duplicate points, self and its duplicate are interchangeable (same coordinates): the features come out the
    same whichever of the two is dropped."""
    xyz = xyz.detach()
    if _on_op_layer(xyz):
        from .mm3d_pn2 import knn
        xyz = xyz.contiguous()
        B, N, _ = xyz.shape
        idx = knn(k + 1, xyz)[:, 1:, :].transpose(1, 2).contiguous()     # (B,k+1,N) -> (B,N,k) int32
        feat = torch.empty(B, 4 * k, N, device=xyz.device, dtype=torch.float32)
        call("mvp_rri_features", xyz.device, B, N, k, xyz, idx, feat)
        return feat
    if k < 2:
        raise ValueError("rri_features needs k >= 2 (got %d)" % k)
    return _rri_reference(xyz, _knn_reference(xyz, k + 1)[:, :, 1:])


def _gmm_params_reference(logits, xyz):
    """gamma = softmax over the components, then gmm_params (deepgmr.py:98-121) with the isotropic variance kept as
    (B,J) (the reference's (B,J,3,3) is sigma * I)."""
    gamma = torch.softmax(logits.transpose(1, 2), dim=2)         # (B,N,J)
    pi = gamma.mean(dim=1)
    npi = pi * gamma.shape[1]
    mu = gamma.transpose(1, 2) @ xyz / npi.unsqueeze(2)
    diff = xyz.unsqueeze(2) - mu.unsqueeze(1)                    # (B,N,J,3)
    sigma = ((diff * diff).sum(dim=3) * gamma).sum(dim=1) / npi
    return gamma, pi, mu, sigma


def gmm_params_backward_reference(gamma, xyz, pi, mu, sigma, g_pi, g_mu, g_sigma):
    """The closed form mvp_gmm_params_backward computes, in torch: -> g_logits (B,J,N)."""
    n = gamma.shape[1]
    npi = (pi * n).unsqueeze(1)                                  # (B,1,J)
    diff = xyz.unsqueeze(2) - mu.unsqueeze(1)                    # (B,N,J,3)
    g_gamma = (g_pi.unsqueeze(1) / n + (diff * g_mu.unsqueeze(1)).sum(dim=3) / npi
               + g_sigma.unsqueeze(1) * ((diff * diff).sum(dim=3) - sigma.unsqueeze(1)) / npi)
    g_logits = gamma * (g_gamma - (gamma * g_gamma).sum(dim=2, keepdim=True))
    return g_logits.transpose(1, 2)


class GmmParams(Function):
    """(logits (B,J,N), xyz (B,N,3)) -> gamma (B,N,J), pi (B,J), mu (B,J,3), sigma (B,J).  Gradient to the logits
    only (through pi, mu and sigma; gamma itself is returned without a gradient path, none of the model's losses
    reads it); none to xyz, whose coordinates never require grad in the reference."""

    @staticmethod
    def forward(ctx, logits, xyz):
        assert logits.dim() == 3 and xyz.dim() == 3 and xyz.shape[2] == 3
        assert logits.shape[0] == xyz.shape[0] and logits.shape[2] == xyz.shape[1]
        if _on_op_layer(logits):
            logits, xyz = logits.contiguous(), xyz.detach().float().contiguous()
            B, J, N = logits.shape
            gamma = torch.empty(B, N, J, device=logits.device, dtype=torch.float32)
            pi = torch.empty(B, J, device=logits.device, dtype=torch.float32)
            mu = torch.empty(B, J, 3, device=logits.device, dtype=torch.float32)
            sigma = torch.empty(B, J, device=logits.device, dtype=torch.float32)
            call("mvp_gmm_params", logits.device, B, N, J, logits, xyz, gamma, pi, mu, sigma)
        else:
            xyz = xyz.detach().to(logits.dtype)
            gamma, pi, mu, sigma = _gmm_params_reference(logits, xyz)
        ctx.save_for_backward(gamma, xyz, pi, mu, sigma)
        ctx.mark_non_differentiable(gamma)
        return gamma, pi, mu, sigma

    @staticmethod
    def backward(ctx, _g_gamma, g_pi, g_mu, g_sigma):
        gamma, xyz, pi, mu, sigma = ctx.saved_tensors
        if not _on_op_layer(gamma):
            return gmm_params_backward_reference(gamma, xyz, pi, mu, sigma, g_pi, g_mu, g_sigma), None
        B, N, J = gamma.shape
        g_logits = torch.empty(B, J, N, device=gamma.device, dtype=torch.float32)
        call("mvp_gmm_params_backward", gamma.device, B, N, J, gamma, xyz, pi, mu, sigma,
             g_pi.float().contiguous(), g_mu.float().contiguous(), g_sigma.float().contiguous(), g_logits)
        return g_logits, None


def gmm_params(logits, xyz):
    """Soft assignment and mixture moments of one cloud batch (DeepGMR's softmax + gmm_params): see GmmParams."""
    return GmmParams.apply(logits, xyz)


def _kabsch_reference(H):
    """R = V diag(1, 1, det(V U^T)) U^T of H = U S V^T in torch (gmm_register's torch.svd + determinant).  Its gradient
    is the reference's: torch.linalg.svd's autograd, which divides by s_j^2 - s_i^2 and is singular at EVERY coincidence
    of two singular values (NaN at an exact one, error ~ eps / gap near one), where the device path's adjoint
    (svd3_kabsch_backward) is not.  No reference for a gradient near a cluster."""
    U, _, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    d = torch.ones(H.shape[0], 3, dtype=H.dtype, device=H.device)
    d[:, 2] = torch.where(torch.linalg.det(V @ U.transpose(1, 2)) < 0, -1.0, 1.0).to(H.dtype)
    return (V * d.unsqueeze(1)) @ U.transpose(1, 2)


def gmm_register(pi_s, mu_s, mu_t, sigma_t):
    """Closed-form rigid motion between two mixtures (gmm_register, deepgmr.py:123-144): pi_s (B,J), mu_s / mu_t
    (B,J,3), sigma_t (B,J) isotropic variances -> T (B,4,4) taking the source onto the target.
      c_s = pi_s mu_s, c_t = pi_s mu_t, Ms = sum_j pi_j (mu_s_j - c_s)(mu_t_j - c_t)^T / sigma_t_j
    (sigma_t is sigma * I: no 3x3 inverse), R = kabsch_rotation(Ms) (one mvp_kabsch_svd3 launch in place of a
    host-side torch.svd and a determinant), t = c_t - R c_s."""
    c_s = pi_s.unsqueeze(1) @ mu_s                               # (B,1,3)
    c_t = pi_s.unsqueeze(1) @ mu_t
    Ms = ((pi_s.unsqueeze(2) * (mu_s - c_s)) / sigma_t.unsqueeze(2)).transpose(1, 2) @ (mu_t - c_t)
    R = kabsch_rotation(Ms) if _on_op_layer(Ms) else _kabsch_reference(Ms)
    t = c_t.transpose(1, 2) - R @ c_s.transpose(1, 2)
    bottom = R.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(R.shape[0], 1, 4)
    return torch.cat([torch.cat([R, t], dim=2), bottom], dim=1)


# ----------------------------------------------------------------------------------------------- DCP's switches
# registration/models/dcp.py reads these where it chooses a route (DGCNN._route, LayerNorm.forward,
# MultiHeadedAttention._route).  Plain module attributes, all off: a route changes a summation order, and a default flips in a
# change of its own.

EDGE_MLP = False           # True: DGCNN.forward takes the fused route in eval mode (float32 CUDA, nothing requires grad)
LAYER_NORM = False         # True: LayerNorm.forward and the transformer's residual sums take ref_layer_norm
EDGE_BN = False            # True: DGCNN.forward runs stages 1-4 through bn_relu_max when training or a gradient is needed
FUSED_ATTENTION = False    # True: MultiHeadedAttention.forward takes fused_attention where nothing asks for a gradient (float32 CUDA)


@contextlib.contextmanager
def routes(*, edge_mlp=None, layer_norm=None, edge_bn=None, fused_attention=None):
    """Set the named switches (EDGE_MLP, LAYER_NORM, EDGE_BN, FUSED_ATTENTION) for the length of a `with` block: None leaves a
    switch as it is, and every switch named gets back the value it had on the way in, also when the block raises.  Blocks nest.
        with registration.routes(edge_mlp=True, layer_norm=True, edge_bn=True): ...
    The switches are module attributes, so this is process-global and not thread-safe: every model in the process sees them,
    and two threads inside blocks of their own restore each other's values."""
    asked = {"EDGE_MLP": edge_mlp, "LAYER_NORM": layer_norm, "EDGE_BN": edge_bn, "FUSED_ATTENTION": fused_attention}
    module = globals()
    before = {name: module[name] for name, on in asked.items() if on is not None}
    module.update({name: bool(asked[name]) for name in before})
    try:
        yield
    finally:
        module.update(before)


# ------------------------------------------------------------------------------------------- DGCNN's edge MLP (DCP)
# registration/models/dcp.py: DGCNN in inference -- the neighbourhood gather, the 1x1 convolutions with BatchNorm's affine
# map and ReLU, and the max over the k neighbours after each, as one kernel (mvp_edge_mlp_max, csrc/edge_mlp.hip).

def _edge_mlp_reference(x, idx, weights, scales, shifts):
    """The composition mvp_edge_mlp_max computes, in torch: an explicit gather, then per stage the product with W_i, the
    affine map, ReLU and the max over k."""
    B, c, N = x.shape
    k = idx.shape[1]
    flat = idx.long().reshape(B, 1, k * N).expand(B, c, k * N)
    edge = torch.cat((torch.gather(x, 2, flat).reshape(B, c, k, N), x.unsqueeze(2).expand(-1, -1, k, -1)), dim=1)
    pooled = []
    for W, sc, sh in zip(weights, scales, shifts):
        edge = torch.relu(torch.einsum("oc,bckn->bokn", W, edge) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
        pooled.append(edge.max(dim=2)[0])
    return torch.cat(pooled, dim=1)


def edge_mlp_max(x, idx, weights, scales, shifts):
    """x (B,c,N) point features, idx (B,k,N) neighbour lists (the knn operator's layout, values in [0,N)), per stage i a
    weight (w_i, K_i) with K_1 = 2c and K_i = w_{i-1} (a 1x1 convolution's 4-D weight is taken as its matrix), a scale
    and a shift (w_i) -> (B, w_1 + .. + w_s, N):
        e_0 = [x[:, idx] ; x],  e_i = relu(scale_i * (W_i e_{i-1}) + shift_i),  out_i = max over k of e_i.
    float32 CUDA tensors run mvp_edge_mlp_max (1..4 stages, widths multiples of 32 up to 256, c <= 4, k <= 64); CPU /
    float64 tensors take the same composition written in torch.  ReLU keeps a NaN, the maximum is NaN if a member is.
    Forward only: no input may require grad while grad mode is on."""
    weights = [W.reshape(W.shape[0], -1) for W in weights]
    tensors = [x] + weights + list(scales) + list(shifts)
    assert not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)), "edge_mlp_max has no backward"
    assert x.dim() == 3 and idx.dim() == 3 and idx.shape[0] == x.shape[0] and idx.shape[2] == x.shape[2]
    assert len(weights) == len(scales) == len(shifts) >= 1
    fan_in = 2 * x.shape[1]
    for W, sc, sh in zip(weights, scales, shifts):
        assert W.shape[1] == fan_in and sc.shape == sh.shape == (W.shape[0],), "stage shapes do not chain"
        fan_in = W.shape[0]
    if not _on_op_layer(x):
        return _edge_mlp_reference(x, idx, weights, scales, shifts)
    assert len(weights) <= 4, "mvp_edge_mlp_max takes at most four stages"
    B, c, N = x.shape
    k = idx.shape[1]
    widths = [W.shape[0] for W in weights] + [0] * (4 - len(weights))
    w = torch.cat([W.detach().reshape(-1) for W in weights]).float().contiguous()
    scale = torch.cat([s.detach() for s in scales]).float().contiguous()
    shift = torch.cat([s.detach() for s in shifts]).float().contiguous()
    out = torch.empty(B, sum(widths), N, device=x.device, dtype=torch.float32)
    call("mvp_edge_mlp_max", x.device, B, c, N, k, len(weights), *widths, x.detach().contiguous(),
         idx.int().contiguous(), w, scale, shift, out)
    return out


# ------------------------------------------------------------------------ the transformer's LayerNorm + residual sums (DCP)
# registration/models/dcp.py: LayerNorm -- a_2 * (x - mean) / (std + eps) + b_2 with the unbiased std and eps added to the
# std -- and the residual addition in front of it, as one kernel each way (mvp_ref_layernorm[_backward],
# csrc/layer_norm.hip).

def _layer_norm_reference(z, a, b, eps):
    """The module's own formula, op for op (registration/models/dcp.py: LayerNorm.forward)."""
    centred = z - z.mean(-1, keepdim=True)
    return a * centred / (z.std(-1, keepdim=True) + eps) + b


def ref_layer_norm_backward_reference(z, a, gy, eps, gres=None):
    """The closed form mvp_ref_layernorm_backward computes, in torch: z (..., d) what was normalised, gy the gradient of y,
    gres the gradient reaching z directly -> (gz, ga, gb).  U = 1 / (std + eps), gh = gy * a:
        gz = U (gh - mean gh) - c (sum gh c) U^2 / ((d - 1) std)  [+ gres],   ga = sum_r gy c U,   gb = sum_r gy,
    the second term 0 where std == 0 (torch's std backward masks a zero std)."""
    d = z.shape[-1]
    c = z - z.mean(-1, keepdim=True)
    std = torch.sqrt((c * c).sum(-1, keepdim=True) / (d - 1))
    U = 1 / (std + eps)
    gh = gy * a
    coef = torch.where(std == 0, torch.zeros_like(std), (gh * c).sum(-1, keepdim=True) * U * U / ((d - 1) * std))
    gz = U * (gh - gh.mean(-1, keepdim=True)) - c * coef
    if gres is not None:
        gz = gz + gres
    return gz, (gy * c * U).reshape(-1, d).sum(0), gy.reshape(-1, d).sum(0)


def _layer_norm_fits(x, a, b, residual):
    """Whether mvp_ref_layernorm takes these tensors as they are: float32 CUDA, contiguous, rows on 16-byte addresses, a row
    length the kernel covers."""
    d = x.shape[-1] if x.dim() >= 1 else 0
    if not (d % 4 == 0 and 4 <= d <= 1024 and x.numel() < 2 ** 31 and a.shape == b.shape == (d,)):
        return False
    rows = (x,) if residual is None else (x, residual)
    return _kernel_reads(rows + (a, b), aligned=rows) and (residual is None or residual.shape == x.shape)


def _aligned_rows(g):
    """A gradient as the kernel reads it: float32, contiguous, on a 16-byte address (autograd may hand over a view)."""
    g = g.float().contiguous()
    return g if g.data_ptr() % 16 == 0 else g.clone()


class RefLayerNorm(Function):
    """(x (..., d), a (d), b (d), eps, residual (..., d) or None) -> y, or (x + residual, y): mvp_ref_layernorm, float32
    CUDA only (ref_layer_norm decides).  Saves z (the sum, or x), a and the (rows, 2) row statistics, nothing else."""

    @staticmethod
    def forward(ctx, x, a, b, eps, residual):
        d = x.shape[-1]
        rows = x.numel() // d
        y = torch.empty_like(x)
        total = torch.empty_like(x) if residual is not None else None
        wants = any(ctx.needs_input_grad)
        stats = torch.empty(rows, 2, device=x.device, dtype=torch.float32) if wants else None
        call("mvp_ref_layernorm", x.device, rows, d, x, residual, a, b, eps, total, y, stats)
        ctx.eps, ctx.with_residual = eps, residual is not None
        ctx.set_materialize_grads(False)
        if wants:
            ctx.save_for_backward(x if total is None else total, a, stats)
        return y if total is None else (total, y)

    @staticmethod
    def backward(ctx, *grads):
        z, a, stats = ctx.saved_tensors
        gres, gy = grads if ctx.with_residual else (None, grads[0])
        need_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[4]
        need_a, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        d = z.shape[-1]
        rows = z.numel() // d
        if gy is None:                                          # y was not used: only the residual stream passes through
            gz, ga, gb = gres, (torch.zeros_like(a) if need_a else None), (torch.zeros_like(a) if need_b else None)
        else:
            gy, gres = _aligned_rows(gy), (None if gres is None else _aligned_rows(gres))
            gz = torch.empty_like(z)
            ga = torch.empty_like(a) if need_a else None
            gb = torch.empty_like(a) if need_b else None
            scratch, nbytes = _scratch(ref_layernorm_backward_scratch_bytes(rows, d) if need_a or need_b else 0, z.device)
            if rows == 0:                                       # nothing is launched, nothing written
                ga, gb = (None if ga is None else ga.zero_()), (None if gb is None else gb.zero_())
            call("mvp_ref_layernorm_backward", z.device, rows, d, z, a, gy, gres, stats, ctx.eps, gz, ga, gb, scratch, nbytes)
        if not need_x:
            gz = None
        return (gz if ctx.needs_input_grad[0] else None, ga, gb, None, gz if ctx.needs_input_grad[4] else None)


def ref_layer_norm(x, a, b, eps=1e-6, residual=None):
    """The transformer's normalisation of z = x (+ residual) over the last axis: a * (z - mean) / (std + eps) + b, std
    unbiased.  Returns y, or (x + residual, y) when a residual is given -- the sum is the residual stream's next value, so
    `x = x + f(...); h = norm(x)` is one call.  float32 CUDA contiguous tensors with d % 4 == 0, 4 <= d <= 1024 run
    mvp_ref_layernorm (backward: mvp_ref_layernorm_backward; gradients for x, a, b and the residual, whose gradient equals
    x's); CPU tensors, float64, any other d and non-contiguous input take the module's formula composed in torch."""
    if _layer_norm_fits(x, a, b, residual):
        return RefLayerNorm.apply(x, a, b, float(eps), residual)
    if residual is None:
        return _layer_norm_reference(x, a, b, eps)
    z = x + residual
    return z, _layer_norm_reference(z, a, b, eps)


# ------------------------------------------------------- DGCNN's BatchNorm + ReLU + max over the neighbours, both ways (DCP)
# registration/models/dcp.py: DGCNN in training -- after each edge stage's 1x1 convolution, BatchNorm2d (batch or running
# statistics), ReLU and the max over the k neighbours as kernels (mvp_edge_bn_stats, mvp_edge_bn_relu_max[_backward],
# csrc/edge_bn.hip).  Saved for backward: z, two statistics per channel and one byte per pooled value; never r.

def _bn_relu_max_reference(z, weight, bias, running_mean, running_var, training, momentum, eps, want_r=True):
    """The composition in torch: F.batch_norm, relu, max(dim=2).  momentum None leaves the running statistics alone (a
    cumulative average needs the caller's batch count)."""
    y = F.batch_norm(z, running_mean, running_var, weight, bias, training, 0.0 if momentum is None else momentum, eps)
    r = torch.relu(y)
    return (r if want_r else None), r.max(dim=2)[0]


def bn_relu_max_backward_reference(z, weight, bias, mean, invstd, arg, g_r, g_pool, batch_stats):
    """The closed form mvp_edge_bn_relu_max_backward computes, in torch: z (B,C,k,N), mean / invstd (C), arg (B,C,N) the
    neighbour each pooled value came from, g_r (B,C,k,N) or None, g_pool (B,C,N) or None -> (gz, ggamma, gbeta).
        g_y = (g_r + [j == arg] g_pool) (y > 0),  gbeta = sum g_y,  ggamma = sum g_y xhat,  xhat = (z - mean) invstd
        gz = gamma invstd (g_y - gbeta / M - xhat ggamma / M)   (running statistics: gamma invstd g_y)"""
    v = lambda t: t.view(1, -1, 1, 1)
    xhat = (z - v(mean)) * v(invstd)
    y = xhat * v(weight) + v(bias)
    g = torch.zeros_like(z) if g_r is None else g_r.clone()
    if g_pool is not None:
        g.scatter_add_(2, arg.long().unsqueeze(2), g_pool.unsqueeze(2))
    g_y = torch.where(y > 0, g, torch.zeros_like(g))
    gbeta, ggamma = g_y.sum(dim=(0, 2, 3)), (g_y * xhat).sum(dim=(0, 2, 3))
    if not batch_stats:
        return v(weight * invstd) * g_y, ggamma, gbeta
    m = z.numel() // z.shape[1]
    return v(weight * invstd) * (g_y - v(gbeta) / m - xhat * v(ggamma) / m), ggamma, gbeta


def _bn_relu_max_fits(z, weight, bias, running_mean, running_var, training, momentum):
    """Whether the kernels take these tensors as they are: float32 CUDA, contiguous, on 16-byte addresses, a shape the entry
    points cover, and a way to the statistics (a batch of more than one value, or running statistics to read)."""
    if z.dim() != 4 or weight is None or bias is None or not isinstance(momentum, float):
        return False
    b, c, k, n = z.shape
    if not (b >= 1 and c >= 1 and 1 <= k <= 64 and n >= 4 and n % 4 == 0 and k * n < 2 ** 31 and b * c < 2 ** 31):
        return False
    running = (running_mean, running_var)
    if any(t is None for t in running) and not (training and all(t is None for t in running)):
        return False
    if training and b * k * n < 2:
        return False
    tensors = [z, weight, bias] + [t for t in running if t is not None]
    return _kernel_reads(tensors, aligned=(z,)) and all(t.shape == (c,) for t in tensors[1:])


class BnReluMax(Function):
    """(z (B,C,k,N), weight (C), bias (C), stats (C,2) = {mean, invstd} or None for batch statistics, eps, want_r) ->
    (r or None, pooled (B,C,N), stats, var (C) biased or None): float32 CUDA only (bn_relu_max decides).  Saves z, weight,
    bias, stats and arg (uint8), never r."""

    @staticmethod
    def forward(ctx, z, weight, bias, stats, eps, want_r):
        b, c, k, n = z.shape
        batch = stats is None
        var = None
        if batch:
            stats = torch.empty(c, 2, device=z.device, dtype=torch.float32)
            var = torch.empty(c, device=z.device, dtype=torch.float32)
            scratch, nbytes = _scratch(edge_bn_scratch_bytes(b, c), z.device)
            call("mvp_edge_bn_stats", z.device, b, c, k, n, z, eps, stats, var, scratch, nbytes)
        r = torch.empty_like(z) if want_r else None
        pooled = torch.empty(b, c, n, device=z.device, dtype=torch.float32)
        arg = torch.empty(b, c, n, device=z.device, dtype=torch.uint8)
        call("mvp_edge_bn_relu_max", z.device, b, c, k, n, z, stats, weight, bias, r, pooled, arg)
        ctx.batch = batch
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(z, weight, bias, stats, arg)
        if batch:
            ctx.mark_non_differentiable(stats, var)
        return r, pooled, (stats if batch else None), var

    @staticmethod
    @once_differentiable
    def backward(ctx, g_r, g_pool, _g_stats, _g_var):
        z, weight, bias, stats, arg = ctx.saved_tensors
        if g_r is None and g_pool is None:
            return None, None, None, None, None, None
        b, c, k, n = z.shape
        g_r, g_pool = (None if g_r is None else _aligned_rows(g_r)), (None if g_pool is None else _aligned_rows(g_pool))
        gz = torch.empty_like(z)
        ggamma = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        gbeta = torch.empty_like(bias) if ctx.needs_input_grad[2] else None
        sums = ctx.batch or ggamma is not None or gbeta is not None
        scratch, nbytes = _scratch(edge_bn_scratch_bytes(b, c) if sums else 0, z.device)
        call("mvp_edge_bn_relu_max_backward", z.device, b, c, k, n, int(ctx.batch), z, stats, weight, bias, arg, g_r, g_pool,
             gz, ggamma, gbeta, scratch, nbytes)
        return (gz if ctx.needs_input_grad[0] else None), ggamma, gbeta, None, None, None


def bn_relu_max(z, weight, bias, running_mean, running_var, training, momentum, eps, want_r=True):
    """BatchNorm2d -> ReLU -> max over the neighbour axis of z (B,C,k,N): returns (r or None, pooled), r = relu(bn(z))
    (B,C,k,N) -- None with want_r=False, and then nothing of z's size is written -- and pooled = r.max(dim=2) (B,C,N).
    training: batch statistics (biased variance from centred values), and running_mean / running_var, where given, move as
    nn.BatchNorm2d moves them: running = (1 - momentum) running + momentum {mean, var M / (M - 1)}, under no_grad; the
    caller increments num_batches_tracked.  Otherwise the running statistics normalise.  ReLU keeps a NaN, the maximum is
    NaN if a member is; of equal maxima the lowest neighbour takes the gradient.
    float32 CUDA contiguous tensors with N % 4 == 0, k <= 64 and a float momentum run mvp_edge_bn_stats,
    mvp_edge_bn_relu_max and, for gradients to z, weight and bias, mvp_edge_bn_relu_max_backward; CPU tensors, float64,
    momentum None, any other shape or an unaligned view take the composition written in torch."""
    if not _bn_relu_max_fits(z, weight, bias, running_mean, running_var, training, momentum):
        return _bn_relu_max_reference(z, weight, bias, running_mean, running_var, training, momentum, eps, want_r)
    eps = float(eps)
    if training:
        r, pooled, stats, var = BnReluMax.apply(z, weight, bias, None, eps, want_r)
        if running_mean is not None:
            m = z.numel() // z.shape[1]
            with torch.no_grad():
                running_mean.mul_(1 - momentum).add_(stats[:, 0], alpha=momentum)
                running_var.mul_(1 - momentum).add_(var, alpha=momentum * m / (m - 1))
        return r, pooled
    with torch.no_grad():
        stats = torch.stack((running_mean, (1 / torch.sqrt(running_var.double() + eps)).float()), dim=1).contiguous()
    r, pooled, _, _ = BnReluMax.apply(z, weight, bias, stats, eps, want_r)
    return r, pooled


# ------------------------------------------------------------------------------ multi-head attention in inference (DCP)
# registration/models/dcp.py: MultiHeadedAttention between its projections -- q k^T, the scale, the softmax and the product
# with v for all heads as one kernel (mvp_attention_forward, csrc/attention.hip), on the projections' own (B, N, heads * d)
# layout: no score tensor, no head transpose.

ATTENTION_WIDTHS = (32, 64, 96, 128)     # the head widths mvp_attention_forward covers


def _attention_reference(q, k, v, heads, divisor):
    """The composition MultiHeadedAttention.forward runs, op for op: split into heads, softmax(q k^T / divisor) v, the heads
    back side by side (the module divides by sqrt(d_k))."""
    b, d = q.size(0), q.size(2) // heads
    split = lambda t: t.reshape(b, -1, heads, d).transpose(1, 2)
    q, k, v = split(q), split(k), split(v)
    weights = F.softmax(q @ k.transpose(-2, -1) / divisor, dim=-1)
    return (weights @ v).transpose(1, 2).reshape(b, -1, heads * d)


def fused_attention(q, k, v, heads, scale=None):
    """q (B, Nq, heads * d), k and v (B, Nk, heads * d), head t in the columns t d .. t d + d (what the module's projections
    produce) -> (B, Nq, heads * d): per (cloud, head, query row i)
        s_ij = scale * <q_i, k_j>,   out_i = sum_j softmax_j(s_ij) v_j,        scale = 1 / sqrt(d) unless given.
    float32 CUDA contiguous tensors on 16-byte addresses with d in {32, 64, 96, 128}, Nk >= 1 and fewer than 2^31 elements run
    mvp_attention_forward (flash-style on v_mfma_f32_32x32x2_f32: no (B, heads, Nq, Nk) tensor exists); CPU tensors, float64,
    any other d, a non-contiguous or misaligned view and Nk == 0 take the module's composition written in torch.
    Forward only: no input may require grad while grad mode is on."""
    assert not (torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))), "fused_attention has no backward"
    assert q.dim() == k.dim() == v.dim() == 3 and k.shape == v.shape and q.shape[0] == k.shape[0] and q.shape[2] == k.shape[2]
    assert heads >= 1 and q.shape[2] % heads == 0
    d = q.shape[2] // heads
    divisor = math.sqrt(d) if scale is None else 1.0 / scale      # the composition divides, as the module does
    scale = 1.0 / divisor if scale is None else scale
    B, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    fits = d in ATTENTION_WIDTHS and nk >= 1 and max(q.numel(), k.numel()) < 2 ** 31
    if not (fits and _kernel_reads((q, k, v), aligned=(q, k, v))):
        return _attention_reference(q, k, v, heads, divisor)
    out = torch.empty_like(q)
    call("mvp_attention_forward", q.device, B, heads, nq, nk, d, q.detach(), k.detach(), v.detach(), scale, out)
    return out
