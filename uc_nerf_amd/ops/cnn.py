"""The 3-D convolutions of the MVS cost regularisation on the device (csrc/conv3d.hip) and the batch-statistic batch-norm of both CNNs (csrc/bn.hip)."""
import torch

from .. import _lib as L
from ._core import _f32, _launch, _ptr


class PackedConv3d:
    """A convolution weight [cout,cin,K,K,K] (transposed: [cin,cout,3,3,3]) in the order `conv3d`'s kernel walks it (made once by `conv3d_pack`)."""
    __slots__ = ("packed", "cin", "cout", "K", "transposed")

    def __init__(self, packed, cin, cout, K, transposed):
        self.packed, self.cin, self.cout, self.K, self.transposed = packed, cin, cout, K, transposed


def conv3d_pack(weight, transposed=False):
    """Packs a float32 device weight for `conv3d`: [cout,cin,K,K,K] with K 1 or 3, or with `transposed` a ConvTranspose3d weight [cin,cout,3,3,3]
    (the transposition is part of the packing).  One launch, nothing read back."""
    weight = _f32(weight.detach(), "weight")
    transposed = bool(transposed)
    if weight.dim() != 5 or not (weight.shape[2] == weight.shape[3] == weight.shape[4]) or 0 in weight.shape:
        raise RuntimeError("uc_nerf_amd.conv3d_pack: weight must be [cout,cin,K,K,K] ([cin,cout,3,3,3] transposed), got %s" % (tuple(weight.shape),))
    K = weight.shape[2]
    cin, cout = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
    floats = L.lib().ucnerf_conv3d_packed_floats(cin, cout, K, int(transposed))
    if floats < 0:
        raise RuntimeError("uc_nerf_amd.conv3d_pack: %s" % L.lib().ucnerf_last_error().decode())
    packed = torch.empty(floats, device=weight.device)
    p = L.Conv3dPackParams()
    p.cin, p.cout, p.K, p.transposed, p.weight, p.packed = cin, cout, K, int(transposed), _ptr(weight), _ptr(packed)
    _launch("ucnerf_conv3d_pack", p, weight.device)
    return PackedConv3d(packed, cin, cout, K, transposed)


def conv3d(x, weight, bias, stride=1, pad=0, relu=True, skip=None, transposed=False):
    """act(conv3d(x, weight, stride, zero padding `pad`) + bias) (+ skip), forward only, exact float32 on the matrix cores (csrc/conv3d.hip: the
    order of the sums is fixed, two calls give the same bits).  x [n,cin,D,H,W]; weight a `PackedConv3d` or a raw weight tensor (packed on the
    spot); bias [cout]; act is ReLU with `relu`, the identity without; `skip`, a tensor of the result's shape, is added AFTER the activation.
    Forward form: cubic K of 1 or 3, stride 1 or 2.  `transposed`: conv_transpose3d with K 3, stride 2, padding 1, output_padding 1 (pass
    stride=2, pad=1), the result is [n,cout,2D,2H,2W].  No autograd: inputs that require grad are used detached."""
    x = _f32(x.detach(), "x")
    w = weight if isinstance(weight, PackedConv3d) else conv3d_pack(weight, transposed)
    bias = _f32(bias.detach(), "bias")
    transposed = bool(transposed)
    if w.transposed != transposed:
        raise RuntimeError("uc_nerf_amd.conv3d: the weight was packed with transposed=%s, the call says %s" % (w.transposed, transposed))
    if x.dim() != 5 or x.shape[1] != w.cin or bias.numel() != w.cout or bias.device != x.device or w.packed.device != x.device:
        raise RuntimeError("uc_nerf_amd.conv3d: x must be [n,%d,D,H,W] and bias [%d] on the weight's device, got %s and %s"
                           % (w.cin, w.cout, tuple(x.shape), tuple(bias.shape)))
    n, _, D, H, W = x.shape
    stride, pad = int(stride), int(pad)
    if transposed:
        if (w.K, stride, pad) != (3, 2, 1):
            raise RuntimeError("uc_nerf_amd.conv3d: the transposed form is K=3, stride=2, pad=1 (output_padding 1), got K=%d stride=%d pad=%d" % (w.K, stride, pad))
        out = (2 * D, 2 * H, 2 * W)
    else:
        if stride not in (1, 2) or pad < 0 or min(D, H, W) + 2 * pad < w.K:
            raise RuntimeError("uc_nerf_amd.conv3d: stride=%d pad=%d on a %d x %d x %d input with a kernel of %d" % (stride, pad, D, H, W, w.K))
        out = tuple((s + 2 * pad - w.K) // stride + 1 for s in (D, H, W))
    if skip is not None:
        skip = _f32(skip.detach(), "skip")
        if tuple(skip.shape) != (n, w.cout) + out or skip.device != x.device:
            raise RuntimeError("uc_nerf_amd.conv3d: skip must be %s on x's device, got %s" % ((n, w.cout) + out, tuple(skip.shape)))
    y = torch.empty((n, w.cout) + out, device=x.device)
    p = L.Conv3dParams()
    p.n, p.cin, p.D, p.H, p.W, p.cout, p.K, p.stride, p.pad = n, w.cin, D, H, W, w.cout, w.K, stride, pad
    p.relu, p.transposed, p.packed_floats = int(bool(relu)), int(transposed), w.packed.numel()
    p.x, p.packed, p.bias, p.skip, p.y = _ptr(x), _ptr(w.packed), _ptr(bias), _ptr(skip), _ptr(y)
    _launch("ucnerf_conv3d", p, x.device)
    return y


def batch_norm_train(y, weight, bias, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5, relu=True, skip=None, out=None,
                     return_stats=False):
    """Train-mode batch-norm of y [n,C,*spatial] (float32, contiguous, on the device) with the statistics of the batch itself, forward only
    (csrc/bn.hip: `ucnerf_bn_stats` then `ucnerf_bn_apply`, the order of every sum fixed, nothing read back): out = act((y - mean) / sqrt(var +
    eps) * weight + bias) (+ skip), var the biased variance, act ReLU with `relu`, `skip` added AFTER the activation.  `running_mean`,
    `running_var` (float32 [C]) and `num_batches_tracked` (one int64) move in place as nn.BatchNorm moves them (the unbiased variance, momentum a
    float in (0, 1]); their version counters are bumped, since the kernels write through raw pointers.  `out`: a tensor like y to write into, y
    itself for in place.  -> out, or (out, saved_mean, saved_var) with `return_stats`.  No autograd: inputs that require grad are used detached."""
    if torch.is_tensor(y) and y.dim() >= 2 and 0 < y.numel() == y.shape[1]:     # n S == 1: torch's own refusal, before anything else is looked at
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(y.size()))
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() >= 2 and y.is_contiguous() and y.numel() > 0):
        raise RuntimeError("uc_nerf_amd.batch_norm_train: y must be a non-empty contiguous float32 [n,C,*spatial] tensor on a ROCm device, got %s"
                           % ("%s %s on %s" % (tuple(y.shape), y.dtype, y.device) if torch.is_tensor(y) else type(y)))
    given, y = out, y.detach()
    n, C = y.shape[0], y.shape[1]
    S = y.numel() // (n * C)
    if momentum is None or not 0.0 < float(momentum) <= 1.0 or not float(eps) > 0.0:
        raise RuntimeError("uc_nerf_amd.batch_norm_train: momentum=%r eps=%r (a float momentum in (0, 1], a positive eps)" % (momentum, eps))
    per_channel = []
    for t, name in ((weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == y.device and tuple(t.shape) == (C,) and t.is_contiguous()):
            raise RuntimeError("uc_nerf_amd.batch_norm_train: %s must be a contiguous float32 [%d] tensor on y's device" % (name, C))
        per_channel.append(t.detach())
    weight, bias = per_channel[0], per_channel[1]
    nbt = num_batches_tracked
    if not (torch.is_tensor(nbt) and nbt.dtype == torch.int64 and nbt.numel() == 1 and nbt.device == y.device):
        raise RuntimeError("uc_nerf_amd.batch_norm_train: num_batches_tracked must be one int64 element on y's device")
    for t, name in ((skip, "skip"), (out, "out")):
        if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == y.device and t.shape == y.shape and t.is_contiguous()):
            raise RuntimeError("uc_nerf_amd.batch_norm_train: %s must be a contiguous float32 tensor of y's shape %s on its device" % (name, tuple(y.shape)))
    if skip is not None:
        skip = skip.detach()
    out = torch.empty_like(y) if out is None else out.detach()
    P = L.lib().ucnerf_bn_partials(n, S)
    if P < 0:
        raise RuntimeError("uc_nerf_amd.batch_norm_train: y %s is outside what the kernels take (at least 2 and below 2^31 - 2^20 values per channel)"
                           % (tuple(y.shape),))
    workspace = torch.empty((C, P, 3), dtype=torch.float64, device=y.device)
    saved = torch.empty((2, C), device=y.device)
    s = L.BnStatsParams()
    s.n, s.C, s.S, s.workspace_triples, s.y, s.workspace = n, C, S, C * P, _ptr(y), _ptr(workspace)
    _launch("ucnerf_bn_stats", s, y.device)
    a = L.BnApplyParams()
    a.n, a.C, a.S, a.workspace_triples, a.eps, a.momentum, a.relu = n, C, S, C * P, float(eps), float(momentum), int(bool(relu))
    a.y, a.workspace, a.weight, a.bias, a.skip, a.out = _ptr(y), _ptr(workspace), _ptr(weight), _ptr(bias), _ptr(skip), _ptr(out)
    a.saved_mean, a.saved_var, a.running_mean, a.running_var = _ptr(saved[0]), _ptr(saved[1]), _ptr(running_mean), _ptr(running_var)
    a.num_batches_tracked = _ptr(nbt)
    _launch("ucnerf_bn_apply", a, y.device)
    for t in (running_mean, running_var, nbt):
        torch.autograd.graph.increment_version(t)
    if given is not None:
        out = given                                        # the caller's own tensor (y itself for in place), not the detached alias
    return (out, saved[0], saved[1]) if return_stats else out
