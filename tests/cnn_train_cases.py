"""Shared cases of the CostRegNet training-route tests and the DIFFERENTIABLE restatement the layer and the module are measured against.

The restatement is torch on the CPU at a chosen dtype, written from the formulas -- convolution, train-mode batch-norm with the batch's own mean
and biased variance, ReLU, the skip additions -- over a STATE DICT with the reference's key names; gradients come from torch's autograd through
these plain expressions.  float64 is the yardstick, float32 the scale the device's error is held against.  It shares no code with the package and
does not import it."""
import torch
import torch.nn.functional as F

from mvs_cnn_cases import EPS, chain_bar, lattice, spacing   # noqa: F401  (re-used by the tests through this module)

ORDER = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11")
STRIDES = {"conv0": 1, "conv1": 2, "conv2": 1, "conv3": 2, "conv4": 1, "conv5": 2, "conv6": 1}

# (in_channels, base_channels, input shape, seed of the weights, seed of the input and the projections): what the GPU module tests run.  The seeds
# are ones at which no ReLU's pre-activation lies within the forward chain bar of zero (test_cnn_train_host.py asserts it), so that a ReLU cannot
# take another side on the device than in float64 and hide or fake a failure.
MODULE_CASES = ((8, 8, (1, 8, 8, 16, 16), 611, 612), (32, 8, (1, 32, 8, 16, 16), 1621, 1622))

# wgrad / dgrad lattice shapes (n, cin, cout, stride, D, H, W) at K 3, pad 1, and the transposed ones (cin, cout, D, H, W) at n = 2
WGRAD_SHAPES = ((1, 8, 8, 1, 4, 5, 7), (1, 8, 16, 2, 8, 8, 8), (1, 4, 8, 2, 5, 7, 9), (1, 16, 1, 1, 3, 4, 5), (1, 1, 8, 1, 3, 4, 5), (1, 33, 65, 1, 3, 3, 3),
                (2, 8, 8, 1, 5, 7, 11))
WGRAD_TRANSPOSED = ((8, 4, 1, 1, 1), (16, 8, 2, 3, 5), (33, 17, 3, 2, 2))
# chunks longer than one 32-voxel round of the kernel: one tile and 18 432 voxels (288 chunks of 64), and conv6 at stage 3 (16 tiles, 20 chunks of 64)
WGRAD_LONG_CHUNKS = ((1, 8, 8, 1, 8, 48, 48), (1, 64, 64, 1, 4, 16, 20))


def conv(x, w, stride, transposed):
    if transposed:
        return F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)
    return F.conv3d(x, w, None, stride=stride, padding=1)


def bn_relu(y, gamma, beta, relu=True, skip=None, eps=EPS):
    """-> (out, z): train-mode batch-norm of y, z its value before the ReLU."""
    dims = (0, 2, 3, 4)
    shape = (1, -1, 1, 1, 1)
    mean = y.mean(dims)
    var = ((y - mean.view(shape)) ** 2).mean(dims)
    z = (y - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * gamma.view(shape) + beta.view(shape)
    out = F.relu(z) if relu else z
    return (out if skip is None else out + skip), z


def leaf(t, dtype):
    return t.detach().cpu().to(dtype).clone().requires_grad_(True)


def layer_grads(x, w, gamma, beta, grad_out, dtype, stride=1, transposed=False, relu=True, skip=None):
    """One layer act(bn(conv(x, w))) (+ skip) and its gradients for the output gradient `grad_out`, everything in `dtype` on the CPU.
    -> dict(out, z, x, w, gamma, beta, skip): the output, the pre-activation values and the five gradients (skip's None without one)."""
    X, W, G, B = leaf(x, dtype), leaf(w, dtype), leaf(gamma, dtype), leaf(beta, dtype)
    S = leaf(skip, dtype) if skip is not None else None
    out, z = bn_relu(conv(X, W, stride, transposed), G, B, relu, S)
    out.backward(grad_out.detach().cpu().to(dtype))
    return dict(out=out.detach(), z=z.detach(), x=X.grad, w=W.grad, gamma=G.grad, beta=B.grad, skip=None if S is None else S.grad)


def cost_reg_net(x, sd, dtype, R1=None, R2=None):
    """CostRegNet of a state dict in TRAIN mode, differentiable: -> dict(cost, prob, z = {layer: pre-activation values}, and with the
    projections R1, R2 given, loss = sum cost R1 + sum prob R2 backpropagated: grad_x and grads = {parameter key: gradient})."""
    P = {k: leaf(v, dtype) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    X = leaf(x, dtype)
    z = {}

    def block(t, name, skip=None):
        y = conv(t, P[name + ".conv.weight"], STRIDES.get(name, 2), name not in STRIDES)
        out, z[name] = bn_relu(y, P[name + ".bn.weight"], P[name + ".bn.bias"], True, skip)
        return out

    conv0 = block(X, "conv0")
    conv2 = block(block(conv0, "conv1"), "conv2")
    conv4 = block(block(conv2, "conv3"), "conv4")
    t = block(block(conv4, "conv5"), "conv6")
    t = block(t, "conv7", conv4)
    t = block(t, "conv9", conv2)
    cost = block(t, "conv11", conv0)
    prob = F.conv3d(cost, P["prob.weight"], None, padding=1)
    out = dict(cost=cost.detach(), prob=prob.detach(), z={k: v.detach() for k, v in z.items()})
    if R1 is not None:
        ((cost * R1.to(dtype)).sum() + (prob * R2.to(dtype)).sum()).backward()
        out["grad_x"], out["grads"] = X.grad, {k: v.grad for k, v in P.items()}
    return out


def module_inputs(case):
    """-> (x, R1, R2) of a MODULE_CASES entry: the input in [0, 1) and the two fixed random projections of the loss."""
    cin, c, shape, _, seed = case
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    return x, torch.randn((shape[0], c) + tuple(shape[2:]), generator=g), torch.randn((shape[0], 1) + tuple(shape[2:]), generator=g)


def relu_offenders(r64, r32, sd):
    """The ReLU-side condition of one module case: [(layer, flat index, z64, bar)] over every pre-activation value whose |z| in float64 is not
    above its layer's forward chain bar, or whose float32 restatement takes the other side."""
    bad = []
    for name in ORDER:
        z64, z32 = r64["z"][name], r32["z"][name]
        bar, _ = chain_bar(z64, z32)
        off = (z64.abs() <= bar) | ((z64 > 0) != (z32 > 0))
        for i in off.flatten().nonzero().flatten().tolist():
            bad.append((name, i, float(z64.flatten()[i]), bar))
    return bad
