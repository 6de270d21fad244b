"""DCP with ALL THREE switches of mvp_benchmark_amd.registration on at once -- what a user who wants the speed sets -- on the
golden clouds of tests/golden/dcp_golden.npz (2 pairs x 64 points): which entry points an eval forward and a training step
reach, the fixture's T_12, finite gradients, the module tree, and the switches back off afterwards."""
import os
import sys
import types

import numpy as np
import pytest
import torch
from conftest import ROOT

from dcp_util import abi_call_names, load_dcp

DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.gpu
def test_dcp_model_with_every_switch_on():
    from mvp_benchmark_amd import registration
    if GOLD not in sys.path:
        sys.path.insert(0, GOLD)
    from make_dcp_golden import fill_parameters
    dcp = load_dcp("routes_gpu")
    g = np.load(os.path.join(GOLD, "dcp_golden.npz"))
    net = dcp.Model(types.SimpleNamespace())
    fill_parameters(net)
    keys = list(net.state_dict())
    net = net.eval().to(DEV)
    src, tgt, T_gt = (torch.tensor(g[k], device=DEV) for k in ("src", "tgt", "T_gt"))
    everything = dict(edge_mlp=True, layer_norm=True, edge_bn=True)
    # ---- one eval forward without gradients: the inference kernel per cloud, 2 * (3 + 4) norms, nothing of training
    with registration.routes(**everything), abi_call_names() as names, torch.no_grad():
        T_12 = net(src, tgt)
    assert names.count("mvp_edge_mlp_max") == 2 and names.count("mvp_ref_layernorm") == 14, names
    assert not any(n.startswith("mvp_edge_bn") or n.endswith("_backward") for n in names), names
    np.testing.assert_allclose(T_12.cpu().numpy(), g["T_12"], atol=2e-4)
    # ---- one training step: 4 stages x 2 clouds of BatchNorm kernels and 14 norms, each way, and no inference kernel
    net.train()
    with registration.routes(**everything), abi_call_names() as names:
        net(src, tgt, T_gt)[0].mean().backward()
    assert names.count("mvp_edge_bn_stats") == 8 and names.count("mvp_edge_bn_relu_max_backward") == 8, names
    assert names.count("mvp_ref_layernorm") == 14 and names.count("mvp_ref_layernorm_backward") == 14, names
    assert "mvp_edge_mlp_max" not in names, names
    grads = {k: p.grad for k, p in net.named_parameters() if p.requires_grad}
    bad = [k for k, v in grads.items() if v is None or not bool(torch.isfinite(v).all())]
    assert not bad and len(grads) > 60, bad
    assert list(net.state_dict()) == keys
    assert all(int(getattr(net.emb_nn, "bn%d" % i).num_batches_tracked) == 2 for i in range(1, 6))
    assert registration.EDGE_MLP is False and registration.LAYER_NORM is False and registration.EDGE_BN is False
