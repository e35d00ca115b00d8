"""Shared cases of the LPIPS tests and the restatement of the chain they are measured against.

The restatement is torch on the CPU, written from the formulas of the chain (scaling, AlexNet's five convolutions with ReLU and two 3 x 3 / 2
max pools, per-pixel channel normalisation, the weighted squared difference, the mean over the pixels, the sum over the five levels), in the
dtype of the weights it is given: float64 is the yardstick, float32 the scale the device's error is held against.  The weights are seeded
random tensors of the real shapes -- nothing is committed, 2.5 M floats take milliseconds.  Neither `lpips` nor `torchvision` is involved."""
import functools

import torch
import torch.nn.functional as F

# (index inside torchvision's `features`, cin, cout, K, stride, pad)
CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIDE = 31
# the whole-chain cases: (H, W); n = 3 pairs each, pair 1 identical
CHAIN_SHAPES = ((31, 31), (35, 47), (64, 80))
CHAIN_N = 3


@functools.lru_cache(maxsize=None)
def weights(seed=7):
    """(alexnet_state, lin_state) in the packages' key spelling, float32, He-scaled so that the activations keep their size down the stack."""
    g = torch.Generator().manual_seed(seed)
    alex, lin = {}, {}
    for l, (idx, cin, cout, K, _, _) in enumerate(CONVS):
        alex["features.%d.weight" % idx] = torch.randn(cout, cin, K, K, generator=g) * (2.0 / (cin * K * K)) ** 0.5
        alex["features.%d.bias" % idx] = torch.randn(cout, generator=g) * 0.1
        lin["lin%d.model.1.weight" % l] = torch.rand(1, cout, 1, 1, generator=g) * (2.0 / cout)
    alex["classifier.1.weight"] = torch.zeros(2, 2)                     # a key a real checkpoint has and the metric does not use
    return alex, lin


@functools.lru_cache(maxsize=None)
def images(H, W, n=CHAIN_N, seed=11):
    """Two [n,3,H,W] float32 batches in [-1, 1]; b is a perturbed a, pair 1 is identical."""
    g = torch.Generator().manual_seed(seed * 1000 + H * 31 + W)
    a = torch.rand(n, 3, H, W, generator=g) * 2 - 1
    b = (a + 0.3 * torch.randn(n, 3, H, W, generator=g)).clamp(-1, 1)
    if n > 1:
        b[1] = a[1]
    return a, b


def features(x, alex, dtype):
    """The five feature levels of x [n,3,H,W]."""
    x = x.to(dtype)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    h = (x - shift) / scale
    levels = []
    for l, (idx, _, _, _, stride, pad) in enumerate(CONVS):
        if l in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        h = F.relu(F.conv2d(h, alex["features.%d.weight" % idx].to(dtype), alex["features.%d.bias" % idx].to(dtype), stride=stride, padding=pad))
        levels.append(h)
    return levels


def layer_distance(f0, f1, lin):
    """One level: [n,C,h,w] x 2, lin [C] -> [n]."""
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    d = (lin.view(1, -1, 1, 1) * (n0 - n1).pow(2)).sum(1)
    return d.mean((1, 2))


def lpips(a, b, alex, lin, dtype):
    """The whole chain in `dtype` -> [n]."""
    fa, fb = features(a, alex, dtype), features(b, alex, dtype)
    total = None
    for l in range(5):
        d = layer_distance(fa[l], fb[l], lin["lin%d.model.1.weight" % l].to(dtype).reshape(-1))
        total = d if total is None else total + d
    return total


@functools.lru_cache(maxsize=None)
def chain_reference(H, W):
    """(float64 result, float32-CPU result) of the case, computed once and shared."""
    alex, lin = weights()
    a, b = images(H, W)
    return lpips(a, b, alex, lin, torch.float64), lpips(a, b, alex, lin, torch.float32)


def lattice(shape, bound, seed):
    """Integer-valued float32 tensor with |v| <= bound."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).to(torch.float32)
