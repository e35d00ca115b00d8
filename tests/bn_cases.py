"""Shared cases of the batch-statistic batch-norm tests and the restatement the op and the modules are measured against.

The restatement is torch on the CPU, written from the formulas of train-mode batch-norm -- per channel mean = sum y / N, the biased variance
var = sum (y - mean)^2 / N, out = act((y - mean) / sqrt(var + eps) * gamma + beta) (+ skip), running_mean = (1 - m) running_mean + m mean,
running_var = (1 - m) running_var + m var N / (N - 1) -- in the dtype it is asked for: float64 is the yardstick, float32 the scale the device's
error is held against.  The two networks are restated in train mode over a STATE DICT with the reference's key names, as mvs_cnn_cases.py
restates them in eval mode; both return the state dict the forward leaves behind.  It shares no code with the package."""
import torch
import torch.nn.functional as F

from mvs_cnn_cases import EPS, chain_bar, randomise, spacing   # noqa: F401  (re-used by the tests through this module)

MOMENTUM = 0.1                                                      # nn.BatchNorm's default, which the reference leaves alone

# the op's shapes: N = 4 at 64 channels; one slice; odd sizes and two images (the walk crosses the image boundary, no 16-byte accesses); 2-D
OP_SHAPES = ((1, 64, 1, 2, 2), (1, 8, 8, 16, 24), (2, 16, 3, 5, 7), (1, 8, 16, 24))


def ragged_shape(partials):
    """[2, 3, S] whose channels span at least three partial slots with a shorter last slice, chosen with the library's own size query
    `partials(n, S)`: the smallest S of the form 4 k + 1 that does (odd, so the two images do not start on a 16-byte boundary either)."""
    S = 5
    while partials(2, S) < 3:
        S += 4
    return (2, 3, S)


def bn_train(y, gamma, beta, dtype, relu=True, skip=None, eps=EPS):
    """-> (out, mean, biased variance) of train-mode batch-norm over y [n,C,*spatial], everything in `dtype` on the CPU."""
    y = y.detach().cpu().to(dtype)
    dims = (0,) + tuple(range(2, y.dim()))
    shape = (1, -1) + (1,) * (y.dim() - 2)
    mean = y.mean(dims)
    var = ((y - mean.view(shape)) ** 2).mean(dims)
    out = (y - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * gamma.detach().cpu().to(dtype).view(shape) + beta.detach().cpu().to(dtype).view(shape)
    if relu:
        out = F.relu(out)
    if skip is not None:
        out = out + skip.detach().cpu().to(dtype)
    return out, mean, var


def running_update(running_mean, running_var, mean, var, count, dtype, momentum=MOMENTUM):
    """-> (running_mean, running_var) after one training forward whose channels had `count` values each."""
    rm, rv = running_mean.detach().cpu().to(dtype), running_var.detach().cpu().to(dtype)
    return (1 - momentum) * rm + momentum * mean.to(dtype), (1 - momentum) * rv + momentum * var.to(dtype) * count / (count - 1)


def _bn_layer(y, sd, new, name, dtype, skip=None):
    out, mean, var = bn_train(y, sd[name + ".weight"], sd[name + ".bias"], dtype, relu=True, skip=skip)
    count = y.numel() // y.shape[1]
    new[name + ".running_mean"], new[name + ".running_var"] = running_update(sd[name + ".running_mean"], sd[name + ".running_var"], mean, var, count, dtype)
    new[name + ".num_batches_tracked"] = sd[name + ".num_batches_tracked"] + 1
    return out


def cost_reg_net(x, sd, dtype):
    """CostRegNet of a state dict in TRAIN mode -> (cost, prob, the state dict after the forward, in `dtype` but for the counters)."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    new = dict(sd)
    h = x.detach().cpu().to(dtype)

    def down(t, name, stride):
        return _bn_layer(F.conv3d(t, sd[name + ".conv.weight"].to(dtype), None, stride=stride, padding=1), sd, new, name + ".bn", dtype)

    def up(t, name, skip):
        y = F.conv_transpose3d(t, sd[name + ".conv.weight"].to(dtype), None, stride=2, padding=1, output_padding=1)
        return _bn_layer(y, sd, new, name + ".bn", dtype, skip=skip)

    conv0 = down(h, "conv0", 1)
    conv2 = down(down(conv0, "conv1", 2), "conv2", 1)
    conv4 = down(down(conv2, "conv3", 2), "conv4", 1)
    t = down(down(conv4, "conv5", 2), "conv6", 1)
    t = up(t, "conv7", conv4)
    t = up(t, "conv9", conv2)
    cost = up(t, "conv11", conv0)
    return cost, F.conv3d(cost, sd["prob.weight"].to(dtype), None, padding=1), new


def feature_net(x, sd, dtype):
    """FeatureNet ("fpn", three stages) of a state dict in TRAIN mode -> ({"stage1", "stage2", "stage3"}, the state dict after the forward)."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    new = dict(sd)
    h = x.detach().cpu().to(dtype)

    def block(t, name, stride, pad):
        return _bn_layer(F.conv2d(t, sd[name + ".conv.weight"].to(dtype), None, stride=stride, padding=pad), sd, new, name + ".bn", dtype)

    conv0 = block(block(h, "conv0.0", 1, 1), "conv0.1", 1, 1)
    conv1 = block(block(block(conv0, "conv1.0", 2, 2), "conv1.1", 1, 1), "conv1.2", 1, 1)
    conv2 = block(block(block(conv1, "conv2.0", 2, 2), "conv2.1", 1, 1), "conv2.2", 1, 1)
    w = lambda k: sd[k].to(dtype)                                       # noqa: E731
    up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)    # noqa: E731  (nearest x 2)
    out = {"stage1": F.conv2d(conv2, w("out1.weight"))}
    intra = up(conv2) + F.conv2d(conv1, w("inner1.weight"), w("inner1.bias"))
    out["stage2"] = F.conv2d(intra, w("out2.weight"), padding=1)
    intra = up(intra) + F.conv2d(conv0, w("inner2.weight"), w("inner2.bias"))
    out["stage3"] = F.conv2d(intra, w("out3.weight"), padding=1)
    return out, new


def randomise_train(module, seed):
    """`randomise` (seeded weights, batch-norm parameters and statistics away from 1 / 0), left in training mode."""
    return randomise(module, seed).train()
