"""Shared cases of the FeatureNet training-route tests and the DIFFERENTIABLE restatement the layers and the module are measured against.

The restatement is torch on the CPU at a chosen dtype, written from the formulas -- 2-D convolution, train-mode batch-norm with the batch's own
mean and biased variance, ReLU, nearest x 2 upsampling, the pyramid's additions -- over a STATE DICT with the reference's key names; gradients
come from torch's autograd through these plain expressions.  float64 is the yardstick, float32 the scale the device's error is held against.
It shares no code with the package and does not import it."""
import torch
import torch.nn.functional as F

from mvs_cnn_cases import EPS, chain_bar, lattice, spacing   # noqa: F401  (re-used by the tests through this module)

# the eight batch-normed layers (name, stride, pad) in forward order, and the five bare ones (name, pad)
BLOCKS = (("conv0.0", 1, 1), ("conv0.1", 1, 1), ("conv1.0", 2, 2), ("conv1.1", 1, 1), ("conv1.2", 1, 1), ("conv2.0", 2, 2), ("conv2.1", 1, 1), ("conv2.2", 1, 1))
BARE = (("out1", 0), ("inner1", 0), ("inner2", 0), ("out2", 1), ("out3", 1))

# (input shape, seed of the weights, seed of the input and the projections): what the GPU module tests run.  The seeds are ones at which no ReLU's
# pre-activation lies within the forward chain bar of zero and the float32 restatement takes no other side (test_feature_train_host.py asserts
# it), so that a ReLU cannot take another side on the device than in float64 and hide or fake a failure.
MODULE_CASES = (((1, 3, 16, 24), 2103, 2104), ((2, 3, 8, 12), 2201, 2202))

# wgrad lattice shapes (n, cin, cout, K, stride, H, W), pad (K - 1) / 2: the 3-channel side, both stride-2 layers' kinds, 1 x 1, a one-channel side
# either way, tile edges (33 columns past two 16-column tiles and one group, 17 rows past a 16-row tile), more than one round per chunk
WGRAD_SHAPES = ((1, 3, 8, 3, 1, 5, 7), (1, 8, 8, 3, 1, 4, 6), (2, 8, 16, 5, 2, 8, 12), (1, 16, 32, 5, 2, 6, 10), (1, 32, 32, 1, 1, 3, 5), (1, 1, 8, 3, 1, 4, 5),
                (1, 8, 1, 3, 1, 4, 5), (1, 33, 17, 3, 1, 3, 3), (1, 8, 8, 3, 1, 48, 48))
# a row longer than one 128-pixel segment (two segments, the second shorter and no multiple of 4); rounds of 32 rows, one of them cut at the
# boundary between two images; chunks of two rounds (520 rows over 512 chunks at most)
WGRAD_MORE = ((1, 4, 8, 3, 1, 3, 150), (1, 4, 8, 5, 2, 4, 268), (2, 4, 8, 3, 1, 70, 4), (1, 4, 8, 3, 1, 520, 66))
# stride-2 input gradient (n, cin, cout, H, W) at K 5
DGRAD_S2_SHAPES = ((1, 8, 16, 8, 12), (2, 16, 32, 4, 6), (1, 3, 5, 6, 6))


def out_hw(H, W, K, stride):
    pad = (K - 1) // 2
    return (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1


def documented_chunks(n, cin, cout, K, stride, H, W):
    """(chunks, rows per chunk, rows per round) of ucnerf_conv2d_wgrad as include/ucnerf_hip.h states them."""
    OH, OW = out_hw(H, W, K, stride)
    OW4 = 4 * -(-OW // 4)
    SW = min(OW4, 128)
    WP = stride * (SW - 1) + K
    CG0 = min(cin, 256 // (K * K))
    RR = 1
    if OW4 <= 128:
        for r in range(128 // OW4, 1, -1):
            if CG0 * ((r - 1) * stride + K) * WP <= 11264:
                RR = r
                break
    CG = min(CG0, 11264 // (((RR - 1) * stride + K) * WP))
    tiles = -(-cout // 32) * -(-cin // CG)
    G = n * OH
    C0 = max(1, min(-(-G // RR), -(-512 // tiles)))
    RC = RR * -(-G // (RR * C0))
    return -(-G // RC), RC, RR


def leaf(t, dtype):
    return t.detach().cpu().to(dtype).clone().requires_grad_(True)


def bn_relu(y, gamma, beta, relu=True, eps=EPS):
    """-> (out, z): train-mode batch-norm of y [n,C,H,W], z its value before the ReLU."""
    mean = y.mean((0, 2, 3))
    var = ((y - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    z = (y - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return (F.relu(z) if relu else z), z


def layer_grads(x, w, gamma, beta, grad_out, dtype, stride, relu=True):
    """One layer act(bn(conv(x, w))) with pad (K - 1) / 2 and its gradients for the output gradient `grad_out`, everything in `dtype` on the CPU.
    -> dict(out, z, x, w, gamma, beta)."""
    X, W, G, B = leaf(x, dtype), leaf(w, dtype), leaf(gamma, dtype), leaf(beta, dtype)
    out, z = bn_relu(F.conv2d(X, W, None, stride=stride, padding=(w.shape[2] - 1) // 2), G, B, relu)
    out.backward(grad_out.detach().cpu().to(dtype))
    return dict(out=out.detach(), z=z.detach(), x=X.grad, w=W.grad, gamma=G.grad, beta=B.grad)


def bare_grads(x, w, b, grad_out, dtype):
    """A bare convolution (stride 1, pad (K - 1) / 2) with or without bias -> dict(out, x, w, b)."""
    X, W, B = leaf(x, dtype), leaf(w, dtype), (leaf(b, dtype) if b is not None else None)
    out = F.conv2d(X, W, B, padding=(w.shape[2] - 1) // 2)
    out.backward(grad_out.detach().cpu().to(dtype))
    return dict(out=out.detach(), x=X.grad, w=W.grad, b=None if B is None else B.grad)


def feature_net(x, sd, dtype, R=None):
    """FeatureNet ("fpn", three stages) of a state dict in TRAIN mode, differentiable: -> dict(out = {"stage1", "stage2", "stage3"}, z = {layer:
    pre-activation values}, and with the projections R = {stage: tensor} given, loss = sum over the stages of sum out R backpropagated: grad_x and
    grads = {parameter key: gradient})."""
    P = {k: leaf(v, dtype) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    X = leaf(x, dtype)
    z = {}

    def block(t, name, stride, pad):
        y = F.conv2d(t, P[name + ".conv.weight"], None, stride=stride, padding=pad)
        out, z[name] = bn_relu(y, P[name + ".bn.weight"], P[name + ".bn.bias"])
        return out

    t, stages = X, []
    for name, stride, pad in BLOCKS:
        t = block(t, name, stride, pad)
        if name in ("conv0.1", "conv1.2", "conv2.2"):
            stages.append(t)
    conv0, conv1, conv2 = stages
    up = lambda v: v.repeat_interleave(2, 2).repeat_interleave(2, 3)    # noqa: E731  (nearest x 2)
    outs = {"stage1": F.conv2d(conv2, P["out1.weight"])}
    intra = up(conv2) + F.conv2d(conv1, P["inner1.weight"], P["inner1.bias"])
    outs["stage2"] = F.conv2d(intra, P["out2.weight"], padding=1)
    intra = up(intra) + F.conv2d(conv0, P["inner2.weight"], P["inner2.bias"])
    outs["stage3"] = F.conv2d(intra, P["out3.weight"], padding=1)
    res = dict(out={k: v.detach() for k, v in outs.items()}, z={k: v.detach() for k, v in z.items()})
    if R is not None:
        sum((outs[k] * R[k].to(dtype)).sum() for k in ("stage1", "stage2", "stage3")).backward()
        res["grad_x"], res["grads"] = X.grad, {k: v.grad for k, v in P.items()}
    return res


def module_inputs(case, c=8):
    """-> (x, R) of a MODULE_CASES entry: the image in [0, 1) and the fixed random projections of the loss, one per stage."""
    shape, _, seed = case
    g = torch.Generator().manual_seed(seed)
    n, _, H, W = shape
    x = torch.rand(shape, generator=g)
    R = {"stage1": torch.randn((n, 4 * c, H // 4, W // 4), generator=g), "stage2": torch.randn((n, 2 * c, H // 2, W // 2), generator=g),
         "stage3": torch.randn((n, c, H, W), generator=g)}
    return x, R


def relu_offenders(r64, r32):
    """The ReLU-side condition of one module case: [(layer, flat index, z64, bar)] over every pre-activation value whose |z| in float64 is not
    above its layer's forward chain bar, or whose float32 restatement takes the other side."""
    bad = []
    for name, _, _ in BLOCKS:
        z64, z32 = r64["z"][name], r32["z"][name]
        bar, _ = chain_bar(z64, z32)
        off = (z64.abs() <= bar) | ((z64 > 0) != (z32 > 0))
        for i in off.flatten().nonzero().flatten().tolist():
            bad.append((name, i, float(z64.flatten()[i]), bar))
    return bad
