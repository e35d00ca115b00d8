"""Generates tests/golden/g21_mvs_cnn.npz and tests/golden/mvs_cnn_keys.txt from the reference's own FeatureNet and CostRegNet
(network/mvs_models.py:309-443).

Run where the reference tree is present:  python tests/golden/make_golden_mvs_cnn.py
Data only: the state dicts of two small seeded modules in eval(), one input each and the reference's outputs in float32; and the key names and
shapes of the default-size modules (a list of names).
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

ref = _ref_import.load()
torch.set_num_threads(1)


def quiet(make):
    with contextlib.redirect_stdout(io.StringIO()):                      # (FeatureNet's constructor prints its arch mode)
        return make()


def randomise(module, g):
    """Seeded weights of unit scale per fan-in and batch-norm parameters and statistics away from 1 / 0 (running_var in [0.5, 2])."""
    with torch.no_grad():
        for name, t in sorted(list(module.named_parameters()) + list(module.named_buffers())):
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                t.copy_(0.5 + 1.5 * torch.rand(t.shape, generator=g))
            elif name.endswith("running_mean"):
                t.copy_(0.3 * torch.randn(t.shape, generator=g))
            elif ".bn." in name and name.endswith("weight"):
                t.copy_(0.6 + 0.8 * torch.rand(t.shape, generator=g))
            elif name.endswith("bias"):
                t.copy_(0.2 * torch.randn(t.shape, generator=g))
            else:
                fan = t.numel() // max(t.shape[0], t.shape[1])           # (a convolution weight: the smaller of fan-in and fan-out)
                t.copy_(torch.randn(t.shape, generator=g) * (2.0 / fan) ** 0.5)
    return module.eval()


def main():
    g = torch.Generator().manual_seed(2121)
    feat = randomise(quiet(lambda: ref.mvs.FeatureNet(base_channels=2)), g)
    reg = randomise(ref.mvs.CostRegNet(in_channels=4, base_channels=2), g)
    image = torch.rand(1, 3, 16, 24, generator=g)
    volume = torch.rand(1, 4, 8, 8, 16, generator=g)
    with torch.no_grad():
        stages = feat(image)
        cost, prob = reg(volume)
    out = {"image": image, "volume": volume, "cost": cost, "prob": prob}
    out.update({"stage%d" % k: stages["stage%d" % k] for k in (1, 2, 3)})
    out.update({"feature." + k: v for k, v in feat.state_dict().items()})
    out.update({"reg." + k: v for k, v in reg.state_dict().items()})
    arrs = {k: v.detach().cpu().numpy() for k, v in out.items()}
    assert all(a.dtype in (np.float32, np.int64) for a in arrs.values())
    path = os.path.join(HERE, "g21_mvs_cnn.npz")
    np.savez_compressed(path, **arrs)
    print("g21_mvs_cnn %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(arrs)))

    lines = []
    for title, module in (("FeatureNet(8)", quiet(lambda: ref.mvs.FeatureNet(base_channels=8))), ("CostRegNet(32,8)", ref.mvs.CostRegNet(32, 8)),
                          ("CostRegNet(16,8)", ref.mvs.CostRegNet(16, 8)), ("CostRegNet(8,8)", ref.mvs.CostRegNet(8, 8))):
        lines.append("# " + title)
        lines += ["%s %s" % (k, ",".join(str(s) for s in v.shape) or "-") for k, v in module.state_dict().items()]
    with open(os.path.join(HERE, "mvs_cnn_keys.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("mvs_cnn_keys %d lines" % len(lines))


if __name__ == "__main__":
    main()
