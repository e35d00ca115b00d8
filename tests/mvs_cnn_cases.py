"""Shared cases of the MVS CNN tests and the restatement the modules and kernels are measured against.

The restatement is torch on the CPU, written from the formulas of the two networks (convolution, eval-mode batch-norm
y = (x - mean) / sqrt(var + eps) * gamma + beta, ReLU, nearest x 2 upsampling, the skip additions) over a STATE DICT with the reference's key
names, in the dtype it is asked for: float64 is the yardstick, float32 the scale the device's error is held against.  It shares no code with
uc_nerf_amd.network.mvs_models."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-5                                                               # nn.BatchNorm's default, which the reference leaves alone


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(HERE, "golden", "g21_mvs_cnn.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def golden_state(prefix):
    """The recorded state dict of the reference's module: prefix "feature." or "reg."."""
    return {k[len(prefix):]: v for k, v in golden().items() if k.startswith(prefix)}


def recorded_keys():
    """{title: [(key, shape tuple)]} of tests/golden/mvs_cnn_keys.txt."""
    out, cur = {}, None
    with open(os.path.join(HERE, "golden", "mvs_cnn_keys.txt")) as f:
        for line in f.read().splitlines():
            if line.startswith("# "):
                cur = out.setdefault(line[2:], [])
            elif line:
                k, s = line.split()
                cur.append((k, () if s == "-" else tuple(int(v) for v in s.split(","))))
    return out


def randomise(module, seed):
    """Seeded He-scaled weights and batch-norm parameters / statistics away from 1 / 0 (running_var in [0.5, 2]), in place; -> module.eval()."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in sorted(list(module.named_parameters()) + list(module.named_buffers())):
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                v = 0.5 + 1.5 * torch.rand(t.shape, generator=g)
            elif name.endswith("running_mean"):
                v = 0.3 * torch.randn(t.shape, generator=g)
            elif name.endswith("bn.weight"):
                v = 0.6 + 0.8 * torch.rand(t.shape, generator=g)
            elif name.endswith("bias"):
                v = 0.2 * torch.randn(t.shape, generator=g)
            else:
                v = torch.randn(t.shape, generator=g) * (2.0 / (t.numel() // max(t.shape[0], t.shape[1]))) ** 0.5
            t.copy_(v.to(t.device))
    return module.eval()


def _bn(x, sd, name, dtype):
    shape = (1, -1) + (1,) * (x.dim() - 2)
    g, b, m, v = (sd[name + "." + k].to(dtype).view(shape) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / torch.sqrt(v + EPS) * g + b


def _block2d(x, sd, name, dtype, stride, pad):
    return F.relu(_bn(F.conv2d(x, sd[name + ".conv.weight"].to(dtype), None, stride=stride, padding=pad), sd, name + ".bn", dtype))


def feature_net(x, sd, dtype):
    """FeatureNet ("fpn", three stages) of a state dict -> {"stage1", "stage2", "stage3"}."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    h = x.detach().cpu().to(dtype)
    conv0 = _block2d(_block2d(h, sd, "conv0.0", dtype, 1, 1), sd, "conv0.1", dtype, 1, 1)
    conv1 = _block2d(_block2d(_block2d(conv0, sd, "conv1.0", dtype, 2, 2), sd, "conv1.1", dtype, 1, 1), sd, "conv1.2", dtype, 1, 1)
    conv2 = _block2d(_block2d(_block2d(conv1, sd, "conv2.0", dtype, 2, 2), sd, "conv2.1", dtype, 1, 1), sd, "conv2.2", dtype, 1, 1)
    w = lambda k: sd[k].to(dtype)                                       # noqa: E731
    up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)    # noqa: E731  (nearest x 2)
    out = {"stage1": F.conv2d(conv2, w("out1.weight"))}
    intra = up(conv2) + F.conv2d(conv1, w("inner1.weight"), w("inner1.bias"))
    out["stage2"] = F.conv2d(intra, w("out2.weight"), padding=1)
    intra = up(intra) + F.conv2d(conv0, w("inner2.weight"), w("inner2.bias"))
    out["stage3"] = F.conv2d(intra, w("out3.weight"), padding=1)
    return out


def cost_reg_net(x, sd, dtype):
    """CostRegNet of a state dict -> (cost, prob)."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    h = x.detach().cpu().to(dtype)

    def down(t, name, stride):
        return F.relu(_bn(F.conv3d(t, sd[name + ".conv.weight"].to(dtype), None, stride=stride, padding=1), sd, name + ".bn", dtype))

    def up(t, name):
        y = F.conv_transpose3d(t, sd[name + ".conv.weight"].to(dtype), None, stride=2, padding=1, output_padding=1)
        return F.relu(_bn(y, sd, name + ".bn", dtype))

    conv0 = down(h, "conv0", 1)
    conv2 = down(down(conv0, "conv1", 2), "conv2", 1)
    conv4 = down(down(conv2, "conv3", 2), "conv4", 1)
    t = down(down(conv4, "conv5", 2), "conv6", 1)
    t = conv4 + up(t, "conv7")
    t = conv2 + up(t, "conv9")
    cost = conv0 + up(t, "conv11")
    return cost, F.conv3d(cost, sd["prob.weight"].to(dtype), None, padding=1)


def spacing(v):
    """One float32 spacing at magnitude v."""
    return 2.0 ** (math.floor(math.log2(max(float(v), 1e-30))) - 23)


def chain_bar(ref64, cpu32):
    """The project's chain rule (test_hip_lpips.py): 4 x the float32 restatement's largest distance from float64, at least one float32 spacing of
    the largest value.  -> (bar, the float32 error)."""
    err32 = float((cpu32.double() - ref64).abs().max())
    return max(4.0 * err32, spacing(ref64.abs().max())), err32


def lattice(shape, bound, seed):
    """Integer-valued float32 tensor with |v| <= bound."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).to(torch.float32)
