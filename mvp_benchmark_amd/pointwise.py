"""Per-point / per-edge linear maps (1x1 convolutions) of the completion
networks.  Same parameters and state_dict layout as nn.Conv1d /
nn.Conv2d(kernel_size=1); the reference builds these layers with nn.Conv1d /
nn.Conv2d directly (completion/models/pcn.py, ecg.py, vrcnet.py).

Routing.  Every entry point describes its layer (`_describe` -> `Layer`: device, dtype, shape, layout of x and the
weight -- no tensors) and a pure planner turns the description, what needs a gradient and the route selectors below into
named routes; the autograd Functions branch on the names.  "ours" = float32 CUDA, 3-d / 4-d, positions L > 0 a multiple
of 4, at most 65535 clouds; "small" = ours with <= 64 x 64 channels; "mfma" = ours, USE_MFMA, >= MFMA_MIN_CH channels, x
and the weight dense and 16-byte aligned; "fits" = _gemm_fits.

  pass                 route     rule                                                                    runs
  pointwise_conv       function  a gradient is wanted and: dense and (mfma or small) and (MFMA_TRAIN or  _PointwiseConv
    (_plan_conv)                 small) -- or USE_MFMA, float32 CUDA, x not empty (any layout: the
                                 backward pass below never calls the library's backward-data kernels)
                       autograd  a gradient is wanted otherwise                                          conv1d / conv2d
                       none      no gradient wanted                                                      the forward alone
    forward            mfma      mfma and fits(cout x cin) and (cout >= 32 or cin <=                     mvp_pointwise_mfma_ex
                                 MFMA_SKINNY_FWD_MAX_CIN); under `function` also MFMA_TRAIN or small,
                                 on the contiguous copies; under `none` only from dense tensors
                       splitk    MFMA_SPLIT_K: as `mfma`, but fits fails and _split_k gives a chunk      mvp_pointwise_mfma_splitk
                       library   otherwise                                                               _library_conv
  data gradient        small     small                                                                   mvp_pointwise_dgrad
    (_plan_conv_       mfma      MFMA_DGRAD, mfma but for x's layout, cin % 4 == 0, fits(cin x cout)     mvp_pointwise_mfma_ex (W^T)
     backward)         splitk    MFMA_SPLIT_K: as `mfma`, but fits fails and _split_k gives a chunk      mvp_pointwise_mfma_splitk (W^T)
                       gemm      otherwise                                                               torch.matmul
  weight gradient      mfma      mfma, not small, cin >= MFMA_WGRAD_MIN_CIN, B * L >=                    mvp_pointwise_wgrad_mfma_ex
                                 MFMA_WGRAD_MIN_POSITIONS, the kernel's scratch query > 0
                       small     small, x 16-byte aligned (the kernel refuses a view at an odd offset)   mvp_pointwise_wgrad
                       gemm      LIBRARY_IS_GEMM or L % 4 != 0                                           torch.einsum
                       miopen    otherwise                                                               aten.convolution_backward
    premask                      ReLU and a wanted gradient whose route is not mfma (those mask on load) aten.threshold_backward
  pointwise_conv_fused fused     dense, mfma, fits forward, (x needs a gradient: cin % 4 == 0 and fits   one GEMM
    (_plan_fused)                the data gradient), the weight-gradient conditions (also for
                                 inference), float32 residual / cloud_bias, not relu with a residual;
                                 with MFMA_SPLIT_K "fits" also where _split_k gives a chunk (that GEMM
                                 then runs on mvp_pointwise_mfma_splitk)
                       composed  otherwise                                                               pointwise_conv + elementwise
  pointwise_conv_dual  stacked   cout1 % 32 == 0, both layers `fused`, the stacked forward `mfma`        one GEMM, two outputs
    (_plan_dual)       separate  otherwise                                                               two pointwise_conv
  pointwise_conv_max   function  a gradient is wanted and: not CUDA, or the sparse kernel's shapes       _PointwiseConvMax
    (_plan_max)        autograd  a gradient is wanted otherwise                                          pointwise_conv, max
    forward            fused     float32 CUDA, not empty, dense weight, forward `mfma`                   mvp_pointwise_mfma_max
                       conv_max  otherwise                                                               pointwise_conv, max
    backward           sparse    the kernel's shapes ((3 cout + L) * 4 <= 30000), x and weight dense     mvp_pointwise_max_backward
     (_plan_max_backward) torch  otherwise (host tensors, other dtypes)                                  scatter_add_ / gather
"""
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from ._lib import (call, pointwise_max_backward_scratch_bytes, pointwise_mfma_splitk_plan, pointwise_mfma_splitk_scratch_bytes,
                   pointwise_wgrad_mfma_scratch_bytes, pointwise_wgrad_scratch_bytes)

# The route selectors stay module globals under these names (not completion/op_config.py): bench.py, the tools and
# several tests assign them, and the planners read them at call time.
MAX_COUT = 64   # mvp_pointwise_wgrad's limit
MAX_CIN = 64
# Channel minimum of the MFMA route.  Rounds 2-3: 32 (below it a 32-wide MFMA block is mostly padding).  Round 4: 1 -- the
# skinny layers (attention-weight MLPs 544 / 272 / 136 / 68 -> 16 / 8 / 4 / 2, the 3- and 8-channel inputs) move bytes, not
# flops, and the library needs 25-200 us per pass for them where one read of the activations takes 7-25
# (profiles/r4_conv_passes_vrcnet_skinny.txt: 3.60 -> 1.97 ms per step over the 16 shapes).
MFMA_MIN_CH = 1
MFMA_SKINNY_FWD_MAX_CIN = 136   # forward with < 32 output channels: the library's GEMV-like kernel wins from ~256 input channels
# Round 4 (tools/bench_conv_passes.py, profiles/r4_conv_passes_*.txt): on the 20 routed shapes of a VRCNet step the
# three passes cost 3.99 / 3.93 / 5.38 ms on these kernels against 5.34 / 5.54 / 6.29 ms on the library (whose
# weight gradient is an NHWC implicit GEMM wrapped in layout transposes), every shape at least a tie: every routed layer
# trains and infers on the MFMA kernels.  What is left below are ROUTE SELECTORS, not experiments: the parity tests drive
# every branch of the backward pass through them (tests/test_gpu_harness.py) and the reference-formulation report and the
# per-pass bench record the library route beside ours (tests/report_reference_model_step.py, tools/bench_conv_passes.py).
# (Round 6 removed the superseded ones: MFMA_WGRAD_TRAIN / _MIN_CIN -- weight gradients only --, MFMA_FWD_MAX_CIN.)
USE_MFMA = True            # False: nothing is routed to the MFMA kernels (the library's convolution everywhere)
MFMA_TRAIN = True          # under autograd the routed layers go through _PointwiseConv
MFMA_DGRAD = True          # data gradient on mvp_pointwise_mfma (W^T, ReLU' on load)
MFMA_WGRAD_MIN_CIN = 1     # weight gradient on mvp_pointwise_wgrad_mfma from this many input channels
MFMA_WGRAD_MIN_POSITIONS = 16384   # B * L below this: too few slabs of positions to deal out (ECG's 64- and 256-point levels)
# Round 6: what "the library" is for a float32 CUDA layer our kernels leave to it -- batched GEMMs (rocBLAS / hipBLASLt
# through torch.matmul), not MIOpen's convolutions: a 1x1 convolution IS a GEMM per cloud; MIOpen wraps it in NHWC
# transposes, starts every process on its naive reference kernels (5.4 ms per weight gradient of ECG's bottleneck layers for
# the first ~150 steps) until its solver search settles on a different kernel from run to run, and its implicit-GEMM
# backward-data kernel reads out of bounds on odd shapes (profiles/r6_miopen_igemm_bwd_fault.txt; that one is avoided either
# way: the `gemm` data gradient).  Measured (tools/ab_flag.py, 12 alternations, ECG -- the model with library-routed layers):
# first alternation 23.9 -> 18.5 ms (no naive-kernel phase), steady state 16.94 = 16.93 ms in rounds 3-6 but 17.2 -> 17.55 in
# rounds 8-12; VRCNet 18.39 -> 18.45.  Not faster, so the default stays MIOpen for the forward and the weight gradient of
# those layers; True = no MIOpen call at all in the training path.
LIBRARY_IS_GEMM = False
# The GEMMs _gemm_fits refuses (a reduction > 512 with too few output tiles: ECG's bottleneck layers and their data gradients)
# on mvp_pointwise_mfma_splitk -- partial tiles per chunk of the reduction, then a fixed-order sum with the epilogue -- instead
# of the library.  Off: whether it pays is decided from profiles/pointwise_splitk.txt and profiles/pointwise_splitk_ecg_ab.txt
# (tools/bench_splitk.py, tools/ab_flag.py); with it off every planner returns what it returned before the route existed.
MFMA_SPLIT_K = False

_WGRAD_SCRATCH = {}   # (device, stream) -> one growing workspace for the partial tiles (no allocator churn)


def _wgrad_scratch(device, nbytes):
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _WGRAD_SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _WGRAD_SCRATCH[key] = buf
    return buf


# ---- the layer's description: every dtype, layout and alignment test of this module is in the next three functions --------------------
Layer = namedtuple("Layer", "cuda f32 dim B cin cout L x_dense w_dense x_aligned w_aligned nonempty")


def _describe(x, weight):
    """What the planners need to know about y = W x: device, dtypes (x and the weight float32), x.dim(), clouds, channels,
    positions per cloud, x / the weight contiguous, x / the weight 16-byte aligned (the kernels' vector loads), x not empty."""
    nonempty = x.numel() > 0
    return Layer(x.is_cuda, x.dtype == torch.float32 and weight.dtype == torch.float32, x.dim(), x.size(0), weight.size(1),
                 weight.size(0), x[0, 0].numel() if nonempty else 0, x.is_contiguous(), weight.is_contiguous(),
                 x.data_ptr() % 16 == 0, weight.data_ptr() % 16 == 0, nonempty)


def _float32(*tensors):
    """The optional operands of the fused epilogue (residual, cloud_bias) are ones the kernel takes?"""
    return all(t is None or t.dtype == torch.float32 for t in tensors)


def _dense_grad(g):
    """grad_out as every backward route reads it: contiguous and 16-byte aligned -- a clone where it is a view at an odd
    offset (allocator blocks are aligned)."""
    g = g.contiguous()
    return g if g.data_ptr() % 16 == 0 else g.clone()


def _densified(d):
    """The description of (x.contiguous(), weight.contiguous()): a copy is a fresh, aligned block."""
    return d._replace(x_dense=True, w_dense=True, x_aligned=d.x_aligned or not d.x_dense, w_aligned=d.w_aligned or not d.w_dense)


# ---- the planners: pure functions of a Layer, what needs a gradient and the selectors above ------------------------------------
def _gemm_fits(batch, m, k, length):
    """Per-cloud GEMM (m x k) (k x length) worth running on mvp_pointwise_mfma?  Not with a long
    reduction and fewer workgroups (128 x 128 tiles of the output) than the chip holds at once, or a
    column tile that is half empty: the library splits K there (ECG's bottleneck layers: 1864 -> 768 at
    256 points 0.28 against 0.21 ms, 2824 -> 1024 at 64 points 0.25 against 0.10;
    profiles/r4_conv_passes_ecg.txt)."""
    if k <= 512:   # (round 6: 512 included -- (64, 512 -> 512, 384) 0.127 against the library's 0.145 ms, the data gradient of
        return True   # (64, 128 -> 512, 384) 0.050 against 0.108: tools/bench_conv_passes.py)
    if length < 128:
        return False
    bm = 128 if m > 64 else 64
    return -(-m // bm) * -(-length // 128) * batch >= 512


def _split_k(batch, m, k, length):
    """The chunk of the reduction for mvp_pointwise_mfma_splitk where the per-cloud GEMM (m x k) (k x length) is one
    _gemm_fits refuses and the library's plan splits it; 0 = not split (always, with MFMA_SPLIT_K off).  Pure; the planners
    and the Functions both ask here, so a plan and its call cannot disagree."""
    if not MFMA_SPLIT_K or _gemm_fits(batch, m, k, length):
        return 0
    return pointwise_mfma_splitk_plan(batch, k, m, length)


def _ours(d):
    return d.cuda and d.f32 and d.dim in (3, 4) and d.L > 0 and d.L % 4 == 0 and d.B <= 65535


def _small(d):
    """mvp_pointwise_wgrad / mvp_pointwise_dgrad take the layer's shape (the layout of x is the weight gradient's business)."""
    return _ours(d) and 0 < d.cin <= MAX_CIN and 0 < d.cout <= MAX_COUT


def _mfma(d, x_too=True):
    """The MFMA kernels take the layer (16-byte loads: a parameter that is a view at an odd offset of a flattened /
    bucketed storage goes to the library instead of failing with MVP_EBADARG).  x_too=False: the operand is not x (the
    data gradient reads grad_out, which _dense_grad has made dense)."""
    return USE_MFMA and _ours(d) and d.w_dense and d.w_aligned and d.cin >= MFMA_MIN_CH and d.cout >= MFMA_MIN_CH \
        and (not x_too or (d.x_dense and d.x_aligned))


def _mfma_fwd(d):
    return _mfma(d) and _gemm_fits(d.B, d.cout, d.cin, d.L) and (d.cout >= 32 or d.cin <= MFMA_SKINNY_FWD_MAX_CIN)


def _fwd_route(d):
    """Forward route of a layer whose tensors the kernels take: `mfma`, `splitk` (everything of _mfma_fwd holds but
    _gemm_fits, and _split_k gives a chunk) or `library`."""
    if _mfma_fwd(d):
        return "mfma"
    if _mfma(d) and (d.cout >= 32 or d.cin <= MFMA_SKINNY_FWD_MAX_CIN) and _split_k(d.B, d.cout, d.cin, d.L) > 0:
        return "splitk"
    return "library"


ConvPlan = namedtuple("ConvPlan", "via fwd layer")     # layer: what _PointwiseConv saves for its backward plan
BackwardPlan = namedtuple("BackwardPlan", "dgrad wgrad premask wgrad_bytes")
MaxPlan = namedtuple("MaxPlan", "via fwd layer")


def _plan_conv(d, wants_grad):
    """pointwise_conv: via `function` (_PointwiseConv), `autograd` (the library's convolution, differentiated by PyTorch) or
    `none` (no gradient wanted); forward `mfma`, `splitk` or `library`."""
    routed = d.cuda and d.f32 and d.x_dense and d.w_dense and d.nonempty and (_mfma(d) or _small(d))
    if wants_grad and ((routed and (MFMA_TRAIN or _small(d))) or (not routed and USE_MFMA and d.cuda and d.f32 and d.nonempty)):
        # (not routed: shapes no kernel of ours covers -- positions not a multiple of 4, strided tensors: the library's forward,
        # but STILL _PointwiseConv's backward: its data gradient is a batched GEMM, never MIOpen's implicit-GEMM backward-data
        # kernel, which reads out of bounds on such shapes)
        d = _densified(d)
        return ConvPlan("function", _fwd_route(d) if MFMA_TRAIN or _small(d) else "library", d)
    if wants_grad or not USE_MFMA:
        return ConvPlan("autograd", "library", d)
    return ConvPlan("none", _fwd_route(d) if routed else "library", d)


def _plan_conv_backward(d, relu, has_bias, need_x, need_w, need_b):
    """_PointwiseConv.backward from the Layer saved at forward time: data gradient `small` / `mfma` / `splitk` / `gemm`, weight (+ bias)
    gradient `mfma` / `small` / `gemm` / `miopen` (None: not needed), whether grad_out is masked by ReLU' up front for the
    routes that do not mask on load, and the MFMA weight gradient's scratch size (queried once, here)."""
    dgrad = wgrad = None
    nbytes = 0
    if need_x:
        # <= 64 x 64 channels: mvp_pointwise_dgrad (11-26 us, at or below the MFMA kernel)
        kernel = MFMA_DGRAD and _mfma(d, x_too=False) and d.cin % 4 == 0
        dgrad = "small" if _small(d) else "mfma" if kernel and _gemm_fits(d.B, d.cin, d.cout, d.L) else \
            "splitk" if kernel and _split_k(d.B, d.cin, d.cout, d.L) > 0 else "gemm"
    if need_w or need_b:
        if d.cin >= MFMA_WGRAD_MIN_CIN and _mfma(d) and not _small(d) and d.B * d.L >= MFMA_WGRAD_MIN_POSITIONS:
            nbytes = pointwise_wgrad_mfma_scratch_bytes(d.B, d.cin, d.cout, d.L, has_bias)
        # (the library = GEMMs, see LIBRARY_IS_GEMM; MIOpen's weight-gradient kernels only with the switch off)
        wgrad = "mfma" if nbytes > 0 else "small" if _small(d) and d.x_aligned else "gemm" if LIBRARY_IS_GEMM or d.L % 4 != 0 else "miopen"
    premask = relu and (dgrad in ("small", "gemm") or wgrad in ("small", "gemm", "miopen"))
    return BackwardPlan(dgrad, wgrad, premask, nbytes)


def _plan_fused(d, need_x, relu=False, residual=False, float32_operands=True, split_k=True):
    """pointwise_conv_fused: `fused` -- all three passes of the layer on the MFMA kernels (the fused prologues / epilogues live
    there only), one GEMM -- or `composed`.  relu with a residual is composed: the fused backward masks by the final output,
    which is not the inner ReLU's mask there.  A GEMM _gemm_fits refuses also counts where _split_k gives it a chunk
    (split_k=False: not for this caller -- the stacked form has no split kernel)."""
    # (the skinny-forward rule of _mfma_fwd is not applied: 544 -> 16 at 384 points costs 0.031 ms here against the
    # library's 0.024, the passes over the 53 MB input that the fused prologue saves cost 0.06)
    def fits(m, k):
        return _gemm_fits(d.B, m, k, d.L) or (split_k and _split_k(d.B, m, k, d.L) > 0)
    ok = _mfma(d) and not (relu and residual) and float32_operands and fits(d.cout, d.cin) \
        and (not need_x or (d.cin % 4 == 0 and fits(d.cin, d.cout))) \
        and d.B * d.L >= MFMA_WGRAD_MIN_POSITIONS and pointwise_wgrad_mfma_scratch_bytes(d.B, d.cin, d.cout, d.L, True) > 0
    return "fused" if ok else "composed"


def _fused_routes(x, weight, need_x):
    """All three passes of a layer on the MFMA kernels?  (_plan_fused on tensors.)"""
    return _plan_fused(_describe(x, weight), need_x) == "fused"


def _plan_dual(d1, d2, need_x):
    """pointwise_conv_dual: `stacked` (one GEMM over both weights, two outputs) or `separate`."""
    ok = d1.cout % 32 == 0 and _plan_fused(d1, need_x, split_k=False) == "fused" and _plan_fused(d2, need_x, split_k=False) == "fused" \
        and _mfma_fwd(d1._replace(cout=d1.cout + d2.cout))
    return "stacked" if ok else "separate"


def _max_kernel_covers(d):
    """Shapes mvp_pointwise_max_backward takes: its per-cloud sort of the winners lives in LDS ((3 Cout + L) * 4 <= 30000
    bytes: L <= 4428 positions at Cout = 1024)."""
    return d.cuda and d.f32 and d.L <= 16384 and d.cout <= 4096 and (3 * d.cout + d.L) * 4 <= 30000 and d.B <= 65535


def _plan_max(d, wants_grad):
    """pointwise_conv_max: via `function` (_PointwiseConvMax: the sparse backward pass), `autograd` (conv + max, dense) or
    `none`; forward `fused` (the max inside the GEMM's epilogue) or `conv_max`."""
    via = "none" if not wants_grad else "function" if not d.cuda or _max_kernel_covers(d) else "autograd"
    fused = via != "autograd" and d.cuda and d.f32 and d.w_dense and d.nonempty and _mfma_fwd(d)
    return MaxPlan(via, "fused" if fused else "conv_max", d)


def _plan_max_backward(d):
    """_PointwiseConvMax.backward, d describing the flattened operands: the `sparse` kernel or the same two index passes in
    `torch` (host tensors / other dtypes -- the CPU tests; CUDA float32 shapes the kernel does not cover never get here:
    this formulation's expanded index tensors would cost more than the dense GEMMs)."""
    return "sparse" if _max_kernel_covers(d) and d.x_dense and d.w_dense else "torch"


# ---- the kernels behind the routes ----------------------------------------------------------------------------------------------
PW_RELU, PW_RELU_AFTER, PW_RES_IS_MASK, PW_X_RELU = 1, 2, 4, 8     # include/mvpops.h MVP_PW_*


def _rows_of_4(w2d, cin):
    """(w2d, ldw): rows padded to a multiple of 4 floats where cin is none -- the kernel reads the weight with 16-byte loads
    (PCN's 1029 -> 512 folding layer at 16384 points: 5.49 -> 4.7 ms; the copy is 2 MB)."""
    if cin % 4:
        w2d = F.pad(w2d, (0, -cin % 4))
    return w2d, w2d.size(1) if cin % 4 else 0


def _one_bias(bias, cloud_bias):
    """The epilogue's one addend per output: cloud_bias (B, Cout) (+ bias), else the bias."""
    if cloud_bias is None:
        return bias
    return cloud_bias if bias is None else cloud_bias + bias          # (B, Cout): tiny


def mfma_linear(x, w2d, bias=None, relu=False, residual=None, group=1, w_kmajor=False, xmask=None, x_relu=False,
                relu_after=False, res_is_mask=False, bias_per_cloud=False, m_split=0, k_chunk=0):
    """y = epilogue(W x) for x (B, Cin, ...) contiguous float32 CUDA, W = w2d (Cout, Cin) -- or its
    transpose (Cin, Cout) with w_kmajor; with xmask, x counts as 0 where xmask <= 0 (aten.threshold_backward's select:
    x passes where xmask is NaN, an Inf of x is dropped, not multiplied); with x_relu, x counts as relu(x) (a NaN stays
    a NaN).  Epilogue (mvp_pointwise_mfma_ex): + bias (one per cloud with bias_per_cloud: (B, Cout)), ReLU,
    max over groups of `group` consecutive positions of the flattened trailing dimensions, + residual (or, with
    res_is_mask, zero where residual <= 0 and unchanged elsewhere, also where residual is NaN), ReLU again with
    relu_after.  Every ReLU keeps a NaN like torch.relu, the group maximum is NaN if a member is (torch.max).
    m_split > 0: two outputs, the rows below m_split and the others -> (y, y2).
    k_chunk > 0 (a multiple of 16; group == 1, no m_split): mvp_pointwise_mfma_splitk -- the reduction in chunks of k_chunk
    over separate workgroups, summed in ascending order before the epilogue.  No autograd."""
    if k_chunk and (group != 1 or m_split):
        raise ValueError("k_chunk: the split-K kernel has neither the group maximum nor two outputs")
    B = x.size(0)
    cin = x.size(1)
    cout = w2d.size(1) if w_kmajor else w2d.size(0)
    length = x[0, 0].numel()
    y2 = None
    if m_split:
        y = torch.empty((B, m_split) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        y2 = torch.empty((B, cout - m_split) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    elif group == 1:
        y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty(B, cout, length // group, dtype=torch.float32, device=x.device)
    w2d, ldw = (w2d, 0) if w_kmajor else _rows_of_4(w2d, cin)
    flags = (PW_RELU if relu else 0) | (PW_RELU_AFTER if relu_after else 0) | (PW_RES_IS_MASK if res_is_mask else 0) \
        | (PW_X_RELU if x_relu else 0)
    if k_chunk:
        scratch, nbytes = None, 0
        if k_chunk < cin:          # (one chunk is the plain kernel: no scratch)
            nbytes = pointwise_mfma_splitk_scratch_bytes(B, cin, cout, length, k_chunk)
            # stream-ordered reuse: the reduce kernel has read it before the next call on this stream writes
            scratch = _wgrad_scratch(x.device, nbytes) if nbytes else None
        call("mvp_pointwise_mfma_splitk", x.device, B, cin, cout, length, x, xmask, w2d, ldw, int(w_kmajor), bias,
             int(bias_per_cloud), residual, flags, y, int(k_chunk), scratch, nbytes)
        return y
    call("mvp_pointwise_mfma_ex", x.device, B, cin, cout, length, x, xmask, w2d, ldw, int(w_kmajor), bias, int(bias_per_cloud),
         residual, flags, int(group), y, int(m_split), y2)
    return (y, y2) if m_split else y


def mfma_wgrad(x, gy, cout, cin, with_bias, gymask=None, x_relu=False, nbytes=None):
    """(gw (Cout, Cin), gb (Cout) | None) of y = W x + b from x (B, Cin, ...) and gy (B, Cout, ...);
    with gymask, gy counts as 0 where gymask <= 0 (aten.threshold_backward's select: gy passes where gymask is NaN); with
    x_relu, x counts as relu(x), a NaN staying a NaN (mvp_pointwise_wgrad_mfma_ex).  nbytes: the kernel's scratch size
    where the caller's plan has queried it already."""
    B = x.size(0)
    length = x[0, 0].numel()
    if nbytes is None:
        nbytes = pointwise_wgrad_mfma_scratch_bytes(B, cin, cout, length, with_bias)
    scratch = _wgrad_scratch(x.device, nbytes)     # stream-ordered reuse: the reduce kernel has read it before the next call writes
    gw = torch.empty(cout, cin, dtype=torch.float32, device=x.device)
    gb = torch.empty(cout, dtype=torch.float32, device=x.device) if with_bias else None
    call("mvp_pointwise_wgrad_mfma_ex", x.device, B, cin, cout, length, x, int(x_relu), gy, gymask, gw, gb, scratch, nbytes)
    return gw, gb


def _library_conv(x, weight, bias, d):
    """The layer on the library, no autograd: conv1d / conv2d (MIOpen) or, with LIBRARY_IS_GEMM on float32 CUDA tensors, one
    batched GEMM W x[b] (+ bias through baddbmm's addend)."""
    if LIBRARY_IS_GEMM and d.cuda and d.f32:
        x3 = x.flatten(2)
        w3 = weight.reshape(1, d.cout, d.cin).expand(d.B, d.cout, d.cin)
        y = torch.bmm(w3, x3) if bias is None else torch.baddbmm(bias.view(1, d.cout, 1), w3, x3)
        return y.view((d.B, d.cout) + tuple(x.shape[2:]))
    return (F.conv1d if d.dim == 3 else F.conv2d)(x, weight, bias)


class _PointwiseConv(Function):
    """y = [relu](W x + bias) on the routes of a ConvPlan (forward) and of _plan_conv_backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, plan):
        d = ctx.layer = plan.layer
        ctx.has_bias = bias is not None
        ctx.relu = relu
        x, weight = x.contiguous(), weight.contiguous()     # (a permuted view: the kernels of the backward pass take dense tensors)
        if plan.fwd in ("mfma", "splitk"):
            y = mfma_linear(x, weight.view(d.cout, d.cin), bias, relu=relu,
                            k_chunk=_split_k(d.B, d.cout, d.cin, d.L) if plan.fwd == "splitk" else 0)
        else:
            y = _library_conv(x, weight, bias, d)
            if relu:
                y = torch.relu_(y)
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, y = ctx.saved_tensors
        d = ctx.layer
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        plan = _plan_conv_backward(d, ctx.relu, ctx.has_bias, need_x, need_w, need_b)
        gy = _dense_grad(grad_out)
        # ReLU'(.): the MFMA kernels mask grad_out by the saved output on load; the other routes get
        # the masked tensor.  Every route takes threshold_backward's convention (0 where y <= 0, grad_out elsewhere -- what
        # autograd of torch.relu does): never a multiply, which would turn an Inf of grad_out at y <= 0 into NaN
        mask = y if ctx.relu else None
        gy_masked = torch.ops.aten.threshold_backward(gy, y, 0) if plan.premask else gy
        gx = gw = gb = None
        if plan.dgrad in ("mfma", "splitk"):
            gx = mfma_linear(gy, weight.view(d.cout, d.cin), w_kmajor=True, xmask=mask,       # W^T (gy . relu')
                             k_chunk=_split_k(d.B, d.cin, d.cout, d.L) if plan.dgrad == "splitk" else 0)
        elif plan.dgrad == "small":
            # few channels: W^T gy in one pass over gy (mvp_pointwise_dgrad) -- not the library's implicit-GEMM
            # kernel, one variant of which reads out of bounds on these shapes (csrc/pointwise.hip)
            gx = torch.empty_like(x)
            call("mvp_pointwise_dgrad", x.device, d.B, d.cin, d.cout, d.L, weight, gy_masked, gx)
        elif plan.dgrad == "gemm":
            # W^T gy per cloud as a batched library GEMM -- NOT aten.convolution_backward: MIOpen's implicit-GEMM
            # backward-data kernel (igemm_bwd_gtcx35_nhwc_fp32) reads past its operands on some of these shapes (37- and
            # 50-point layers of the golden tests: a GPU memory fault whenever the neighbouring page happens to be
            # unmapped -- rocgdb trace in profiles/NOTES_r6.md section 11); a 1x1 convolution's data gradient is a GEMM
            gx = torch.matmul(weight.reshape(d.cout, d.cin).t(), gy_masked.flatten(2)).view_as(x)
        if plan.wgrad == "mfma":
            gw, gb = mfma_wgrad(x, gy, d.cout, d.cin, ctx.has_bias, gymask=mask, nbytes=plan.wgrad_bytes)
            gw = gw.view_as(weight)
        elif plan.wgrad == "small":
            nbytes = pointwise_wgrad_scratch_bytes(d.B, d.cin, d.cout, d.L)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            gw = torch.empty_like(weight)
            gb = torch.empty(d.cout, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            call("mvp_pointwise_wgrad", x.device, d.B, d.cin, d.cout, d.L, x, gy_masked, gw, gb, scratch, nbytes)
        elif plan.wgrad == "gemm":
            gw = torch.einsum("bol,bil->oi", gy_masked.flatten(2), x.flatten(2)).view_as(weight) if need_w else None
            gb = gy_masked.flatten(2).sum((0, 2)) if need_b else None
        elif plan.wgrad == "miopen":
            nd = d.dim - 2
            _, gw, gb = torch.ops.aten.convolution_backward(
                gy_masked, x, weight, [d.cout] if ctx.has_bias else None, [1] * nd, [0] * nd, [1] * nd, False, [0] * nd, 1,
                [False, need_w, need_b])
        return gx, gw, gb, None, None


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def pointwise_conv(x, weight, bias=None, relu=False):
    """y = W x + bias (then ReLU if `relu`) over the channel dimension of x
    (B,Cin,N) / (B,Cin,H,W); weight (Cout,Cin,1[,1])."""
    d = _describe(x, weight)
    plan = _plan_conv(d, _wants_grad(weight, x, bias))
    if plan.via == "function":
        return _PointwiseConv.apply(x, weight, bias, relu, plan)
    if plan.fwd in ("mfma", "splitk"):     # inference
        return mfma_linear(x, weight.view(d.cout, d.cin), bias, relu=relu,
                           k_chunk=_split_k(d.B, d.cout, d.cin, d.L) if plan.fwd == "splitk" else 0)
    if plan.via == "autograd":
        y = (F.conv1d if d.dim == 3 else F.conv2d)(x, weight, bias)
    else:
        y = _library_conv(x, weight, bias, d)
    return torch.relu(y) if relu else y


class _PointwiseConvFused(Function):
    """y = act2(act1(W in(x) + bias + cloud_bias[b]) + residual) with in = ReLU if relu_in, act1 = ReLU if relu, act2 = ReLU
    if relu_after, in ONE GEMM (mvp_pointwise_mfma_ex): the pre-activation ReLUs, residual sums and per-cloud vectors of the
    relational encoder (vrcnet.py:34-57, 151, 172, 283-296) cost no elementwise pass forward.  Backward: ONE pass masks
    grad_out by the output where a residual or a per-cloud bias needs the masked tensor itself (otherwise the GEMMs mask on
    load), the data gradient zeroes its output where x <= 0 in its epilogue (threshold_backward's convention like every
    ReLU' here: it passes where x is NaN), the weight gradient takes relu(x) on load.  (relu together with a residual never
    gets here: _plan_fused.)"""

    @staticmethod
    def forward(ctx, x, weight, bias, cloud_bias, residual, relu_in, relu, relu_after):
        y = _fused_forward(x, weight, bias, cloud_bias, residual, relu_in, relu, relu_after)
        ctx.has_bias, ctx.has_cloud_bias, ctx.has_residual = bias is not None, cloud_bias is not None, residual is not None
        ctx.relu_in, ctx.relu_out = relu_in, relu or relu_after
        ctx.save_for_backward(x, weight, y if ctx.relu_out else None)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, y = ctx.saved_tensors
        cout, cin = weight.shape[:2]
        gy = _dense_grad(grad_out)
        mask = None
        if ctx.relu_out:
            if ctx.has_residual or ctx.has_cloud_bias:
                gy = torch.ops.aten.threshold_backward(gy, y, 0)          # the masked tensor itself is an output
            else:
                mask = y
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = gcb = None
        if need_x:
            gx = mfma_linear(gy, weight.view(cout, cin), w_kmajor=True, xmask=mask,
                             residual=x if ctx.relu_in else None, res_is_mask=ctx.relu_in,
                             k_chunk=_split_k(x.size(0), cin, cout, x[0, 0].numel()))     # (0 where the GEMM fits: _plan_fused)
        if need_w or need_b:
            gw, gb = mfma_wgrad(x, gy, cout, cin, ctx.has_bias, gymask=mask, x_relu=ctx.relu_in)
            gw = gw.view_as(weight)
        if ctx.has_cloud_bias and ctx.needs_input_grad[3]:
            gcb = gy.flatten(2).sum(2)
        gres = gy if ctx.has_residual and ctx.needs_input_grad[4] else None
        return gx, gw, gb, gcb, gres, None, None, None


def _fused_forward(x, weight, bias, cloud_bias, residual, relu_in, relu, relu_after):
    cout, cin = weight.shape[:2]
    return mfma_linear(x, weight.view(cout, cin), _one_bias(bias, cloud_bias), relu=relu, residual=residual, x_relu=relu_in,
                       relu_after=relu_after, bias_per_cloud=cloud_bias is not None,
                       k_chunk=_split_k(x.size(0), cout, cin, x[0, 0].numel()))           # (0 where the GEMM fits: _plan_fused)


def pointwise_conv_fused(x, weight, bias=None, relu_in=False, relu=False, residual=None, relu_after=False, cloud_bias=None):
    """act2(act1(W in(x) + bias + cloud_bias[b]) + residual): in = ReLU if relu_in, act1 = ReLU if relu, act2 = ReLU if
    relu_after; cloud_bias (B, Cout) (summed with the bias first: one addend per output), residual like the output.  One GEMM where all passes of the layer are on the MFMA
    kernels, the same function composed of pointwise_conv and elementwise passes elsewhere (host tensors, other dtypes,
    shapes the routing rules give to the library)."""
    wants_grad = _wants_grad(x, weight, bias, residual, cloud_bias)
    route = _plan_fused(_describe(x, weight), x.requires_grad and wants_grad, relu, residual is not None,
                        _float32(residual, cloud_bias))
    if route == "fused":
        residual = None if residual is None else residual.contiguous()
        cloud_bias = None if cloud_bias is None else cloud_bias.contiguous()
        if wants_grad:
            return _PointwiseConvFused.apply(x, weight, bias, cloud_bias, residual, relu_in, relu, relu_after)
        return _fused_forward(x, weight, bias, cloud_bias, residual, relu_in, relu, relu_after)
    if cloud_bias is not None:
        cb = _one_bias(bias, cloud_bias)
        h = pointwise_conv(torch.relu(x) if relu_in else x, weight, None) + cb.view(cb.shape + (1,) * (x.dim() - 2))
        h = torch.relu_(h) if relu else h
    else:
        h = pointwise_conv(torch.relu(x) if relu_in else x, weight, bias, relu=relu)
    if residual is not None:
        h = h + residual
    return torch.relu(h) if relu_after else h


def _stacked_forward(x, w1, w2):
    c1, c2, cin = w1.size(0), w2.size(0), w1.size(1)
    return mfma_linear(x, torch.cat((w1.view(c1, cin), w2.view(c2, cin)), 0), m_split=c1)


class _PointwiseConvDual(Function):
    """(W1 x, W2 x) of ONE input as one GEMM with two contiguous outputs (mvp_pointwise_mfma_ex, m_split): a residual unit's
    conv1 / conv_res (vrcnet.py:160-172).  The stacked convolution of round 4 handed out torch.split views -- a copy for the
    consumer that needs a contiguous tensor forward, a concatenation of the two gradients backward."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        ctx.save_for_backward(x, w1, w2)
        return _stacked_forward(x, w1, w2)

    @staticmethod
    def backward(ctx, g1, g2):
        x, w1, w2 = ctx.saved_tensors
        c1, c2, cin = w1.size(0), w2.size(0), w1.size(1)
        g1, g2 = _dense_grad(g1), _dense_grad(g2)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = mfma_linear(g1, w1.view(c1, cin), w_kmajor=True)
            gx = mfma_linear(g2, w2.view(c2, cin), w_kmajor=True, residual=gx)       # W1^T g1 + W2^T g2
        gw1 = mfma_wgrad(x, g1, c1, cin, False)[0].view_as(w1) if ctx.needs_input_grad[1] else None
        gw2 = mfma_wgrad(x, g2, c2, cin, False)[0].view_as(w2) if ctx.needs_input_grad[2] else None
        return gx, gw1, gw2


def pointwise_conv_dual(x, w1, w2):
    """(conv(x, w1), conv(x, w2)), bias-free, both contiguous; one pass over x where the MFMA kernels cover the layer."""
    if _plan_dual(_describe(x, w1), _describe(x, w2), torch.is_grad_enabled() and x.requires_grad) == "separate":
        return pointwise_conv(x, w1), pointwise_conv(x, w2)
    if _wants_grad(x, w1, w2):
        return _PointwiseConvDual.apply(x, w1, w2)
    return _stacked_forward(x, w1, w2)


class _PointwiseConvMax(Function):
    """max over the positions of y = W x + bias -> (B, Cout), with the backward pass the max makes possible:
    grad_y is zero except at the B * Cout winning positions, so the weight gradient is a gather of those
    columns of x and the data gradient a scatter of scaled weight rows -- 2 * B * Cout * Cin multiply-adds
    each instead of two dense GEMMs over all B * L positions on a tensor of zeros (the PointNet stage of
    PCN / VRCNet, 64 x (512 -> 1024) x 2048: 1.16 + 1.40 ms of GEMMs -> the two index passes below).  Values and
    gradients are those of `conv(x).max(dim=-1)[0]` under autograd (the gradient goes to the position torch.max
    reports); tests/test_harness_cpu.py::test_pointwise_conv_max_matches_autograd."""

    @staticmethod
    def forward(ctx, x, weight, bias, plan):
        with torch.no_grad():
            val, idx = _conv_max_forward(x, weight, bias, plan)
        ctx.save_for_backward(x, weight, idx)
        ctx.has_bias = bias is not None
        return val

    @staticmethod
    def backward(ctx, g):
        x, weight, idx = ctx.saved_tensors
        B, cin = x.shape[:2]
        cout = weight.size(0)
        x3 = x.reshape(B, cin, -1)
        w2 = weight.reshape(cout, cin)
        g = _dense_grad(g)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        length = x3.size(2)
        gx = gw = gb = None
        if _plan_max_backward(_describe(x3, w2)) == "sparse":
            gx = torch.empty_like(x3) if need_x else None
            gw = torch.empty_like(w2) if need_w else None
            gb = torch.empty(cout, dtype=torch.float32, device=x.device) if need_b else None
            nbytes = pointwise_max_backward_scratch_bytes(B, cin, cout, length) if gw is not None else 0
            scratch = _wgrad_scratch(x.device, nbytes) if nbytes else None     # the winning columns of x, staged
            call("mvp_pointwise_max_backward", x.device, B, cin, cout, length, x3, w2, g, idx.int(), gx, gw, gb, scratch,
                 nbytes)
            return (gx.view_as(x) if need_x else None, gw.view_as(weight) if need_w else None, gb, None)
        where = idx.unsqueeze(1).expand(B, cin, cout)                  # [b, ci, co] -> winning position of (b, co)
        if need_x:
            gx = torch.zeros_like(x3).scatter_add_(2, where, g.unsqueeze(1) * w2.t().unsqueeze(0)).view_as(x)
        if need_w:
            gw = torch.einsum("bo,bio->oi", g, torch.gather(x3, 2, where)).view_as(weight)
        if need_b:
            gb = g.sum(0)
        return gx, gw, gb, None


def _mfma_max(x, weight, bias, d):
    w2d, ldw = _rows_of_4(weight.reshape(d.cout, d.cin), d.cin)
    val = torch.empty(d.B, d.cout, dtype=torch.float32, device=x.device)
    idx = torch.empty(d.B, d.cout, dtype=torch.int32, device=x.device)
    keys = torch.empty(d.B * d.cout, dtype=torch.int64, device=x.device)
    call("mvp_pointwise_mfma_max", x.device, d.B, d.cin, d.cout, d.L, x, w2d, ldw, bias, 0, val, idx, keys, keys.numel() * 8)
    return val, idx


def mfma_conv_max(x, weight, bias=None):
    """(values (B, Cout), positions (B, Cout) int32) of (W x + bias).max over the positions inside the GEMM's epilogue
    (mvp_pointwise_mfma_max: the (B, Cout, L) tensor is never written), or None where the forward GEMM is not routed to
    the MFMA kernel.  No autograd."""
    plan = _plan_max(_describe(x, weight), False)
    return _mfma_max(x, weight, bias, plan.layer) if plan.fwd == "fused" else None


def _conv_max_forward(x, weight, bias, plan):
    """(values, positions) on the forward route of a MaxPlan."""
    if plan.fwd == "fused":
        return _mfma_max(x, weight, bias, plan.layer)
    return pointwise_conv(x, weight, bias).flatten(2).max(dim=2)


_conv_max_uncovered_seen = set()


def pointwise_conv_max(x, weight, bias=None):
    """(W x + bias).max over the positions: x (B,Cin,N) / (B,Cin,H,W), weight (Cout,Cin,1[,1]) -> (B, Cout)."""
    d = _describe(x, weight)
    plan = _plan_max(d, _wants_grad(x, weight, bias))
    if plan.via == "function":
        return _PointwiseConvMax.apply(x, weight, bias, plan)
    if plan.via == "autograd":
        shape = (d.cout, d.L)
        if shape not in _conv_max_uncovered_seen:          # (once per shape)
            _conv_max_uncovered_seen.add(shape)
            import logging
            logging.getLogger(__name__).info("conv -> max over %d positions x %d channels: outside the sparse backward kernel's "
                                             "LDS budget, dense autograd route", shape[1], shape[0])
    return _conv_max_forward(x, weight, bias, plan)[0]      # (plain autograd, or no gradient wanted: the forward alone)


class PointwiseConv1d(nn.Conv1d):
    """nn.Conv1d(kernel_size=1); `layer(x, relu=True)` = relu(layer(x)) with the
    activation fused into the GEMM's epilogue."""

    def __init__(self, c_in, c_out, bias=True):
        super().__init__(c_in, c_out, kernel_size=1, bias=bias)

    def forward(self, x, relu=False):
        return pointwise_conv(x, self.weight, self.bias, relu=relu)

    def max_over_positions(self, x):
        """self(x).max(dim=2)[0] with the sparse backward pass of _PointwiseConvMax."""
        return pointwise_conv_max(x, self.weight, self.bias)


class PointwiseConv2d(nn.Conv2d):
    def __init__(self, c_in, c_out, bias=True):
        super().__init__(c_in, c_out, kernel_size=1, bias=bias)

    def forward(self, x, relu=False):
        return pointwise_conv(x, self.weight, self.bias, relu=relu)

    def max_over_positions(self, x):
        """self(x).flatten(2).max(dim=2)[0] with the sparse backward pass of _PointwiseConvMax."""
        return pointwise_conv_max(x, self.weight, self.bias)
