"""Generates tests/golden/deepgmr_golden.npz from the REFERENCE DeepGMR model, imported
unmodified from /root/reference/registration (runs in the build container only;
the reference never travels to the GPU box).

Stored: parameter names + shapes of registration/models/deepgmr.py:Model at the cfg
(use_rri, rri_size 20, num_groups 16) and with use_tnet; a small pair of clouds
(2, 256, 3) and T_gt; the reference's RRI features of the first cloud batch for
k = 20 and k = 5 (get_rri_cluster, one cluster); softmax + gmm_params for fixed
logits (sigma as its isotropic diagonal); and the model's outputs in eval mode on
CPU: T_12 and (loss, r_err, t_err, rmse, mse); the same six outputs of the two
variants without RRI (raw centred coordinates into the backbone), `norri_*` for
use_rri=False and `norri_tnet_*` for use_rri=False + use_tnet=True (the T-net takes
3 channels, so it excludes RRI).  Parameters are filled with
make_dcp_golden.fill_parameters on both sides.  B = 2: the reference's `.squeeze()`
in gmm_params drops a batch of one.

Shims (as make_dcp_golden.py; none changes the arithmetic): stub `h5py` and
`visu_utils` modules; `torch.arange` inside deepgmr.py ignores its device='cuda'
argument (get_edge_features); `Tensor.cuda()` is the identity (gmm_register).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/registration"
OUT = os.path.join(HERE, "deepgmr_golden.npz")
sys.path.insert(0, HERE)

from make_dcp_golden import fill_parameters  # noqa: E402

ARGS = dict(use_rri=True, rri_size=20, num_groups=16, use_tnet=False)


def make_inputs():
    g = torch.Generator().manual_seed(11)
    pts1 = torch.rand(2, 256, 3, generator=g) - 0.5
    ang = torch.tensor([0.7, -1.3])
    c, s = torch.cos(ang), torch.sin(ang)
    zero, one = torch.zeros(2), torch.ones(2)
    R = torch.stack([c, zero, s, zero, one, zero, -s, zero, c], dim=1).view(2, 3, 3)
    t = torch.tensor([[0.2, -0.1, 0.05], [-0.05, 0.15, -0.2]])
    pts2 = pts1 @ R.transpose(1, 2) + t.unsqueeze(1)
    T = torch.eye(4).repeat(2, 1, 1)
    T[:, :3, :3] = R
    T[:, :3, 3] = t
    logits = 2.0 * torch.randn(2, 16, 256, generator=g)
    return pts1, pts2, T, logits


def main():
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    visu = types.ModuleType("visu_utils")
    visu.visualize = None
    sys.modules["visu_utils"] = visu
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "models"))
    import deepgmr  # the reference, unmodified

    class _TorchOnCpu:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def arange(*a, **k):
            k.pop("device", None)
            return torch.arange(*a, **k)

    deepgmr.torch = _TorchOnCpu()
    torch.Tensor.cuda = lambda self, *a, **k: self

    pts1, pts2, T_gt, logits = make_inputs()
    out = dict(pts1=pts1.numpy(), pts2=pts2.numpy(), T_gt=T_gt.numpy(), logits=logits.numpy())
    for use_tnet in (False, True):
        net = deepgmr.Model(types.SimpleNamespace(**dict(ARGS, use_tnet=use_tnet)))
        names = sorted(net.state_dict())
        key = "tnet_" if use_tnet else ""
        out[key + "names"] = np.array(names)
        out[key + "shapes"] = np.array([str(list(net.state_dict()[n].shape)) for n in names])
    net = deepgmr.Model(types.SimpleNamespace(**ARGS))
    fill_parameters(net)
    net.eval()
    with torch.no_grad():
        for k in (20, 5):
            out["rri_k%d" % k] = deepgmr.get_rri_cluster(pts1.transpose(1, 2).unsqueeze(-1), k).squeeze(-1).numpy()
        gamma = torch.softmax(logits.transpose(1, 2), dim=2)
        pi, mu, sigma = deepgmr.gmm_params(gamma, pts1)
        out.update(gamma=gamma.numpy(), pi=pi.numpy(), mu=mu.numpy(), sigma=sigma[:, :, 0, 0].numpy())
        out["T_12"] = net(pts1, pts2, prefix="test").numpy()
        loss, r_err, t_err, rmse, mse = net(pts1, pts2, T_gt, prefix="val")
    out.update(loss=loss.numpy(), r_err=r_err.numpy(), t_err=t_err.numpy(), rmse=rmse.numpy(), mse=mse.numpy())
    with torch.no_grad():
        for key, over in (("norri_", dict(use_rri=False)), ("norri_tnet_", dict(use_rri=False, use_tnet=True))):
            var = deepgmr.Model(types.SimpleNamespace(**dict(ARGS, **over)))
            fill_parameters(var)
            var.eval()
            out[key + "T_12"] = var(pts1, pts2, prefix="test").numpy()
            vals = var(pts1, pts2, T_gt, prefix="val")
            for name, v in zip(("loss", "r_err", "t_err", "rmse", "mse"), vals):
                out[key + name] = v.numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; params", sum(p.numel() for p in net.parameters()))
    print("T_12[0]", out["T_12"][0], "loss", loss, "r_err", r_err, "t_err", t_err)


if __name__ == "__main__":
    main()
