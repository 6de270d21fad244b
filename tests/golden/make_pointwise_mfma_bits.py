"""Record the output BITS of every instance of the MFMA GEMM kernels (csrc/pointwise_mfma.hip) as
tests/golden/pointwise_mfma_bits.json: a SHA-256 of the output bytes per case.

Needs the GPU:
    python tests/golden/make_pointwise_mfma_bits.py [OUT.json]
    MVP_LIB=path/to/libmvpops.so python tests/golden/make_pointwise_mfma_bits.py OUT.json      (another build of the library)
The other pointwise tests hold the kernels to float64 within a tolerance, or the split-K kernel to the plain one; a
reduction reordered in the code they share passes all of them.  The committed digests are what the commit BEFORE the three
kernels' K loops were merged computed; tests/test_gpu_pointwise_mfma_bits.py recomputes them through this module.

Inputs come from no RNG: an integer LCG with an xor-shift, evaluated per element in torch.int64 operations on the CPU,
mapped to (h % 4001 - 2000) / 997 -- non-dyadic floats in about [-2, 2], so that the order of a summation shows in the
bits.  A mask is such a tensor with every tenth element (by a second hash) <= 0 and the others > 0.

Cases: B = 3 and the smallest ragged shapes that select every template instance --
  fwd     the 12 forward / data-gradient instances: 64- / 128-row tile x weight row-major / k-major x plain / xmask / x_relu.
          Row-major with cin = 515: unaligned rows (scalar loads along k, a_vec = 0, straight through the ABI: mfma_linear
          would pad them) and a partial last k-group; cin = 40 once with rows padded to 44 floats; k-major with cin = 40.
          One case each for the residual, the residual as a mask, two outputs, the group maximum and a bias per cloud.
  max     the 2 row-maximum instances; values and positions.
  splitk  the 24 split-K instances: the same matrix x a 64- / 128-column tile (L = 20 / 388); cin = 515 in chunks of 128 is
          five chunks, the last one three long.
  wgrad   the 16 weight-gradient instances: (cout, cin) in {33, 130} x {40, 515} x gymask x x_relu, L = 388 (a ragged last
          slab of positions), each with and without the bias gradient.
"""
import hashlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "pointwise_mfma_bits.json")
DEV = "cuda:0"
B, L = 3, 388
PROLOGUES = ("plain", "xmask", "x_relu")
PW_RELU, PW_RELU_AFTER, PW_RES_IS_MASK, PW_X_RELU = 1, 2, 4, 8      # include/mvpops.h MVP_PW_*


def _hash(n, seed):
    """n integers in [0, 2^31): three rounds of s = (1103515245 s + 12345) mod 2^31, s ^= s >> 13 on s = i + 7919 seed."""
    s = (torch.arange(n, dtype=torch.int64) + 7919 * seed) % 2147483648
    for _ in range(3):
        s = (s * 1103515245 + 12345) % 2147483648           # (< 2^62: no overflow)
        s = s ^ (s >> 13)
    return s


def values(shape, seed):
    n = 1
    for d in shape:
        n *= d
    v = ((_hash(n, seed) >> 4) % 4001 - 2000).to(torch.float64) / 997.0
    return v.to(torch.float32).view(shape).to(DEV)


def mask(shape, seed):
    n = 1
    for d in shape:
        n *= d
    closed = ((_hash(n, seed + 1) >> 4) % 10 == 0).view(shape).to(DEV)
    v = values(shape, seed).abs()
    return torch.where(closed, -v, v + 0.125)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def cases():
    """[(id, dict)]: kind, cout, cin, L and the kind's options."""
    out = []

    def add(kind, cout, cin, length, **kw):
        name = "%s-%dx%d-L%d" % (kind, cout, cin, length) + "".join("-%s" % (k if v is True else "%s%s" % (k, v))
                                                                    for k, v in kw.items() if v not in (False, "plain"))
        out.append((name, dict(kind=kind, cout=cout, cin=cin, L=length, **kw)))

    weights = [(33, 515, False), (130, 515, False), (36, 40, True), (132, 40, True)]       # (cout, cin, w_kmajor)
    for (cout, cin, kmajor), pro in itertools.product(weights, PROLOGUES):
        add("fwd", cout, cin, L, kmajor=kmajor, pro=pro)
    add("fwd", 33, 40, L, ldw=44)
    for extra in (dict(residual=True, relu=True, relu_after=True), dict(residual=True, res_is_mask=True), dict(m_split=32),
                  dict(group=4, relu=True), dict(cloud_bias=True)):
        add("fwd", 130, 40, L, **extra)
    for cout in (33, 130):
        add("max", cout, 40, L)
    for (cout, _, kmajor), pro, length in itertools.product(weights, PROLOGUES, (20, L)):
        add("splitk", cout, 515, length, kmajor=kmajor, pro=pro, k_chunk=128)
    for cout, cin, gymask, x_relu, bias in itertools.product((33, 130), (40, 515), (False, True), (False, True), (True, False)):
        add("wgrad", cout, cin, L, gymask=gymask, x_relu=x_relu, bias=bias)
    return out


def run(c):
    """The case's output digest."""
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd.pointwise import mfma_linear, mfma_wgrad
    kind, cout, cin, length = c["kind"], c["cout"], c["cin"], c["L"]
    x = values((B, cin, length), 1)
    if kind == "wgrad":
        gy = values((B, cout, length), 2)
        gw, gb = mfma_wgrad(x, gy, cout, cin, c["bias"], gymask=mask((B, cout, length), 3) if c["gymask"] else None,
                            x_relu=c["x_relu"])
        return digest(gw, gb) if c["bias"] else digest(gw)
    bias = values((cout,), 4)
    if kind == "max":
        w = values((cout, cin), 5)
        val = torch.empty(B, cout, device=DEV)
        idx = torch.empty(B, cout, dtype=torch.int32, device=DEV)
        keys = torch.empty(B * cout, dtype=torch.int64, device=DEV)
        _lib.call("mvp_pointwise_mfma_max", DEV, B, cin, cout, length, x, w, 0, bias, 0, val, idx, keys, keys.numel() * 8)
        return digest(val, idx)
    kmajor, pro, ldw = c.get("kmajor", False), c.get("pro", "plain"), c.get("ldw", 0)
    w = values((cin, cout) if kmajor else (cout, ldw or cin), 5)
    xmask = mask((B, cin, length), 6) if pro == "xmask" else None
    if c.get("cloud_bias"):
        bias = values((B, cout), 7)
    residual = values((B, cout, length), 8) if c.get("residual") else None
    flags = (PW_RELU if c.get("relu") else 0) | (PW_RELU_AFTER if c.get("relu_after") else 0) \
        | (PW_RES_IS_MASK if c.get("res_is_mask") else 0) | (PW_X_RELU if pro == "x_relu" else 0)
    if kmajor or (cin % 4 == 0 and not ldw):               # the wrapper leaves such a weight as it lies
        y = mfma_linear(x, w, bias, relu=bool(c.get("relu")), residual=residual, group=c.get("group", 1), w_kmajor=kmajor,
                        xmask=xmask, x_relu=pro == "x_relu", relu_after=bool(c.get("relu_after")),
                        res_is_mask=bool(c.get("res_is_mask")), bias_per_cloud=bool(c.get("cloud_bias")),
                        m_split=c.get("m_split", 0), k_chunk=c.get("k_chunk", 0))
        return digest(*y) if isinstance(y, tuple) else digest(y)
    y = torch.empty(B, cout, length, device=DEV)
    if kind == "splitk":
        nbytes = _lib.pointwise_mfma_splitk_scratch_bytes(B, cin, cout, length, c["k_chunk"])
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.call("mvp_pointwise_mfma_splitk", DEV, B, cin, cout, length, x, xmask, w, ldw, 0, bias, 0, residual, flags, y,
                  c["k_chunk"], scratch, nbytes)
    else:
        _lib.call("mvp_pointwise_mfma_ex", DEV, B, cin, cout, length, x, xmask, w, ldw, 0, bias, 0, residual, flags, 1, y, 0, None)
    return digest(y)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def main(argv):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from mvp_benchmark_amd import _lib
    if os.environ.get("MVP_LIB"):
        _lib.LIB_PATH = os.path.abspath(os.environ["MVP_LIB"])
    assert torch.cuda.is_available(), "the recorder needs the GPU"
    out = {}
    for name, c in cases():
        out[name] = run(c)
        print(name, out[name], flush=True)
    assert len(out) == len(cases())
    path = argv[0] if argv else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d digests; library %s; torch %s" % (path, len(out), _lib.LIB_PATH, torch.__version__))


if __name__ == "__main__":
    main(sys.argv[1:])
