"""The 3-D convolutions of the MVS cost regularisation on the device (csrc/conv3d.hip), the batch-statistic batch-norm of both CNNs (csrc/bn.hip), and
their backward: the weight gradient (csrc/conv3d_bwd.hip), the input gradient on the forward kernel, the batch-norm backward with the ReLU mask,
and the differentiable layer CostRegNet's training route is made of.  The same for FeatureNet's 2-D layers: the weight, stride-2 input and bias
gradients of csrc/conv2d_bwd.hip and the two differentiable layer functions of its training route.  `groups=` on the batch-norm functions keeps
the statistics per group of images (the same kernels and entry points: `groups=1` is their G = 1): FeatureNet over all the views of a sample in one
pass."""
import torch

from .. import _lib as L
from ._core import _dev, _f32, _launch, _ptr
from .metrics import conv2d_bias_relu, conv2d_pack


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


BN_MAX_GROUPS = 64                                         # csrc/bn.hip: BN_MAX_GROUPS


def _bn_groups(groups, y, who):
    """`groups` of the batch-norm functions -> G, checked against the first dimension of y (before anything else is: no device is needed to be told)."""
    if isinstance(groups, bool) or not isinstance(groups, int) or not 1 <= groups <= BN_MAX_GROUPS:
        raise RuntimeError("uc_nerf_amd.%s: groups=%r (an integer from 1 to %d)" % (who, groups, BN_MAX_GROUPS))
    if groups > 1 and torch.is_tensor(y) and y.dim() >= 1 and y.shape[0] % groups:
        raise RuntimeError("uc_nerf_amd.%s: groups=%d does not divide the first dimension of %s" % (who, groups, tuple(y.shape)))
    return groups


def _bn_args(who, y, shape, *named):
    """Arguments of the batch-norm functions, (tensor, name) each: contiguous float32 tensors on y's device, of `shape` or (None) of y's own
    -> them, detached, in the order given (one call for several: the small layers are bound by the host's time per launch)."""
    want, dev, out = y.shape if shape is None else shape, y.device, []
    for t, name in named:
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == dev and t.shape == want and t.is_contiguous()):
            raise RuntimeError("uc_nerf_amd.%s: %s must be a contiguous float32 %s" % (who, name, "tensor of y's shape %s on its device" % (tuple(y.shape),)
                                                                                     if shape is None else "%s tensor on y's device" % (list(shape),)))
        out.append(t.detach())
    return out


def batch_norm_train(y, weight, bias, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5, relu=True, skip=None, out=None,
                     return_stats=False, groups=1):
    """Train-mode batch-norm of y [n,C,*spatial] (float32, contiguous, on the device) with the statistics of the batch itself, forward only
    (csrc/bn.hip: `ucnerf_bn_stats_groups` then `ucnerf_bn_apply_groups`, the order of every sum fixed, nothing read back): out = act((y - mean) / sqrt(var +
    eps) * weight + bias) (+ skip), var the biased variance, act ReLU with `relu`, `skip` added AFTER the activation.  `running_mean`,
    `running_var` (float32 [C]) and `num_batches_tracked` (one int64) move in place as nn.BatchNorm moves them (the unbiased variance, momentum a
    float in (0, 1]); their version counters are bumped, since the kernels write through raw pointers.  `out`: a tensor like y to write into, y
    itself for in place.  -> out, or (out, saved_mean, saved_var) with `return_stats`.  No autograd: inputs that require grad are used detached.
    `groups` = G > 1 (the same two launches; `groups=1` is their G = 1): the first dimension is G groups of n / G consecutive images, each normalised
    with its OWN statistics, bit for bit what G calls on the G slabs give, the running statistics moved G times in ascending group order;
    saved_mean and saved_var then are [G,C]."""
    if torch.is_tensor(y) and y.dim() >= 2 and 0 < y.numel() == y.shape[1]:     # n S == 1: torch's own refusal, before anything else is looked at
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(y.size()))
    G = _bn_groups(groups, y, "batch_norm_train")
    if G > 1 and torch.is_tensor(y) and y.dim() >= 2 and 0 < y.numel() == G * y.shape[1]:      # ... and the one each of the G calls would meet
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(torch.Size((y.shape[0] // G,) + tuple(y.shape[1:]))))
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() >= 2 and y.is_contiguous() and y.numel() > 0):
        raise RuntimeError("uc_nerf_amd.batch_norm_train: y must be a non-empty contiguous float32 [n,C,*spatial] tensor on a ROCm device, got %s"
                           % ("%s %s on %s" % (tuple(y.shape), y.dtype, y.device) if torch.is_tensor(y) else type(y)))
    given, y = out, y.detach()
    n, C = y.shape[0] // G, y.shape[1]
    S = y.numel() // (G * n * C)
    if momentum is None or not 0.0 < float(momentum) <= 1.0 or not float(eps) > 0.0:
        raise RuntimeError("uc_nerf_amd.batch_norm_train: momentum=%r eps=%r (a float momentum in (0, 1], a positive eps)" % (momentum, eps))
    weight, bias, _, _ = _bn_args("batch_norm_train", y, (C,), (weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var"))
    nbt = num_batches_tracked
    if not (torch.is_tensor(nbt) and nbt.dtype == torch.int64 and nbt.numel() == 1 and nbt.device == y.device):
        raise RuntimeError("uc_nerf_amd.batch_norm_train: num_batches_tracked must be one int64 element on y's device")
    if skip is not None:
        skip, = _bn_args("batch_norm_train", y, None, (skip, "skip"))
    out = torch.empty_like(y) if out is None else _bn_args("batch_norm_train", y, None, (out, "out"))[0]
    P = L.lib().ucnerf_bn_partials(n, S)
    if P < 0:
        raise RuntimeError("uc_nerf_amd.batch_norm_train: y %s is outside what the kernels take (at least 2 and below 2^31 - 2^20 values per channel)"
                           % (tuple(y.shape),))
    workspace = torch.empty((G, C, P, 3), dtype=torch.float64, device=y.device)
    saved = torch.empty((2, G, C) if G > 1 else (2, C), device=y.device)
    s, a = L.BnStatsGroupsParams(), L.BnApplyGroupsParams()
    s.G, s.n, s.C, s.S, s.workspace_triples, s.y, s.workspace = G, n, C, S, G * C * P, _ptr(y), _ptr(workspace)
    _launch("ucnerf_bn_stats_groups", s, y.device)
    a.G, a.n, a.C, a.S, a.workspace_triples, a.eps, a.momentum, a.relu = G, n, C, S, G * C * P, float(eps), float(momentum), int(bool(relu))
    a.y, a.workspace, a.weight, a.bias, a.skip, a.out = _ptr(y), _ptr(workspace), _ptr(weight), _ptr(bias), _ptr(skip), _ptr(out)
    a.saved_mean, a.saved_var, a.running_mean, a.running_var = _ptr(saved[0]), _ptr(saved[1]), _ptr(running_mean), _ptr(running_var)
    a.num_batches_tracked = _ptr(nbt)
    _launch("ucnerf_bn_apply_groups", a, y.device)
    for t in (running_mean, running_var, nbt):
        torch.autograd.graph.increment_version(t)
    if given is not None:
        out = given                                        # the caller's own tensor (y itself for in place), not the detached alias
    return (out, saved[0], saved[1]) if return_stats else out


def _conv_out(size, stride, pad):
    return tuple((s + 2 * pad - 3) // stride + 1 for s in size)


def conv3d_wgrad(x, grad_y, stride=1, pad=1, transposed=False):
    """The weight gradient of `conv3d` with a K = 3 kernel (csrc/conv3d_bwd.hip: exact float32 on the matrix cores, split over chunks of the
    voxels and folded in ascending chunk order, no atomics, two calls give the same bits).  x [n,cin,D,H,W] the layer's input, grad_y the
    gradient of its output ([n,cout,OD,OH,OW]; transposed: [n,cout,2D,2H,2W]) -> [cout,cin,3,3,3] (transposed: [cin,cout,3,3,3])."""
    x, grad_y = _f32(x.detach(), "x"), _f32(grad_y.detach(), "grad_y")
    transposed, stride, pad = bool(transposed), int(stride), int(pad)
    if x.dim() != 5 or grad_y.dim() != 5 or x.device != grad_y.device or x.shape[0] != grad_y.shape[0] or 0 in x.shape[1:] or 0 in grad_y.shape[1:]:
        raise RuntimeError("uc_nerf_amd.conv3d_wgrad: x [n,cin,D,H,W] and grad_y [n,cout,...] on one device, got %s and %s" % (tuple(x.shape), tuple(grad_y.shape)))
    n, cin, D, H, W = x.shape
    cout = grad_y.shape[1]
    floats = L.lib().ucnerf_conv3d_wgrad_workspace_floats(n, cin, cout, D, H, W, 3, stride, pad, int(transposed))
    if floats < 0:
        raise RuntimeError("uc_nerf_amd.conv3d_wgrad: %s" % L.lib().ucnerf_last_error().decode())
    want = tuple(2 * s for s in (D, H, W)) if transposed else _conv_out((D, H, W), stride, pad)
    if tuple(grad_y.shape[2:]) != want:
        raise RuntimeError("uc_nerf_amd.conv3d_wgrad: grad_y must be [%d,%d,%d,%d,%d] for x %s with stride=%d pad=%d transposed=%s, got %s"
                           % ((n, cout) + want + (tuple(x.shape), stride, pad, transposed, tuple(grad_y.shape))))
    grad_w = torch.empty((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), device=x.device)
    workspace = torch.empty(floats, device=x.device)
    p = L.Conv3dWgradParams()
    p.n, p.cin, p.D, p.H, p.W, p.cout, p.K, p.stride, p.pad, p.transposed = n, cin, D, H, W, cout, 3, stride, pad, int(transposed)
    p.workspace_floats, p.x, p.grad_y, p.workspace, p.grad_weight = floats, _ptr(x), _ptr(grad_y), _ptr(workspace), _ptr(grad_w)
    _launch("ucnerf_conv3d_wgrad", p, x.device)
    return grad_w


def conv3d_dgrad_pack(weight, stride=1, pad=1, transposed=False):
    """The K = 3 weight of a layer packed for `conv3d_dgrad` (a copy: the layer's weight may change afterwards).  Stride 1 (pad 1): the
    transposed, flipped weight for the forward form; stride 2 (pad 1): the same tensor read as a transposed convolution's [cin' = cout,
    cout' = cin,3,3,3]; a transposed layer: its weight read as a forward one's [cout' = cin, cin' = cout,3,3,3]."""
    transposed, stride, pad = bool(transposed), int(stride), int(pad)
    if not torch.is_tensor(weight) or weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise RuntimeError("uc_nerf_amd.conv3d_dgrad: the weight must be [cout,cin,3,3,3] ([cin,cout,3,3,3] transposed)")
    if transposed:
        if (stride, pad) != (2, 1):
            raise RuntimeError("uc_nerf_amd.conv3d_dgrad: the transposed form is stride=2 pad=1 (output_padding 1), got stride=%d pad=%d" % (stride, pad))
        return conv3d_pack(weight, transposed=False)
    if pad != 1 or stride not in (1, 2):
        raise RuntimeError("uc_nerf_amd.conv3d_dgrad: stride 1 or 2 with pad 1 is built, got stride=%d pad=%d" % (stride, pad))
    if stride == 2:
        return conv3d_pack(weight, transposed=True)
    return conv3d_pack(_f32(weight.detach(), "weight").transpose(0, 1).flip(2, 3, 4).contiguous(), transposed=False)


def conv3d_dgrad(grad_y, weight, x_shape, stride=1, pad=1, transposed=False):
    """The input gradient of `conv3d` with a K = 3 kernel, on `conv3d` itself (zero bias, no ReLU, no skip): `weight` the layer's raw weight or
    what `conv3d_dgrad_pack` made of it, `x_shape` the layer input's [n,cin,D,H,W].  A stride-2 layer needs even D, H and W (an odd size would
    need output_padding 0, which is not built): RuntimeError otherwise."""
    transposed, stride, pad = bool(transposed), int(stride), int(pad)
    x_shape = tuple(int(v) for v in x_shape)
    if len(x_shape) != 5 or not torch.is_tensor(grad_y) or grad_y.dim() != 5 or min(x_shape) < 1:
        raise RuntimeError("uc_nerf_amd.conv3d_dgrad: grad_y must be [n,cout,...] and x_shape [n,cin,D,H,W], got %s and %s"
                           % (tuple(grad_y.shape) if torch.is_tensor(grad_y) else type(grad_y), x_shape))
    if transposed:
        if (stride, pad) != (2, 1):
            raise RuntimeError("uc_nerf_amd.conv3d_dgrad: the transposed form is stride=2 pad=1 (output_padding 1), got stride=%d pad=%d" % (stride, pad))
        want, route = tuple(2 * s for s in x_shape[2:]), dict(stride=2, pad=1, transposed=False)
    elif stride == 2:
        if pad != 1 or any(s % 2 for s in x_shape[2:]):
            raise RuntimeError("uc_nerf_amd.conv3d_dgrad: a stride-2 layer needs pad 1 and even D, H, W (an odd size needs output_padding 0, which is "
                               "not built), got x_shape %s pad=%d" % (x_shape, pad))
        want, route = tuple(s // 2 for s in x_shape[2:]), dict(stride=2, pad=1, transposed=True)
    else:
        if stride != 1 or pad != 1:
            raise RuntimeError("uc_nerf_amd.conv3d_dgrad: stride 1 or 2 with pad 1 is built, got stride=%d pad=%d" % (stride, pad))
        want, route = x_shape[2:], dict(stride=1, pad=1, transposed=False)
    if tuple(grad_y.shape[2:]) != want or grad_y.shape[0] != x_shape[0]:
        raise RuntimeError("uc_nerf_amd.conv3d_dgrad: grad_y must be [%d,cout,%d,%d,%d] for x_shape %s, got %s" % ((x_shape[0],) + want + (x_shape, tuple(grad_y.shape))))
    grad_y = _f32(grad_y.detach(), "grad_y")
    w = weight if isinstance(weight, PackedConv3d) else conv3d_dgrad_pack(weight, stride, pad, transposed)
    if w.cout != x_shape[1] or w.cin != grad_y.shape[1] or w.K != 3 or w.transposed != route["transposed"]:
        raise RuntimeError("uc_nerf_amd.conv3d_dgrad: grad_y %s and x_shape %s do not fit the weight (the layer's cin=%d cout=%d, packed transposed=%s)"
                           % (tuple(grad_y.shape), x_shape, w.cout, w.cin, w.transposed))
    zero = torch.zeros(w.cout, device=grad_y.device)
    return conv3d(grad_y, w, zero, relu=False, skip=None, **route)


def batch_norm_train_bwd(grad_out, y, saved_mean, saved_var, weight, bias, eps=1e-5, relu=True, out=None, groups=1):
    """The backward of `batch_norm_train` (csrc/bn.hip: `ucnerf_bn_bwd_reduce_groups` then `ucnerf_bn_bwd_apply_groups`, float64 sums in a fixed order, nothing
    read back): grad_out the gradient of act(bn(y)), y the tensor the forward normalised, saved_mean / saved_var what it returned with
    `return_stats`; the ReLU's mask is recomputed from y bit for bit.  `out`: a tensor like y for grad_y, grad_out itself for in place.
    -> (grad_y, grad_weight, grad_bias).  The skip's gradient is grad_out itself.
    `groups` = G > 1, as in the forward: saved_mean / saved_var are its [G,C]; grad_y is, group by group, the ungrouped
    backward's bit for bit; grad_weight and grad_bias [C] are the sums over the groups, added in float64 and rounded once."""
    G = _bn_groups(groups, y, "batch_norm_train_bwd")
    for t, name in ((grad_out, "grad_out"), (y, "y")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 2 and t.is_contiguous() and t.numel() > 0):
            raise RuntimeError("uc_nerf_amd.batch_norm_train_bwd: %s must be a non-empty contiguous float32 [n,C,*spatial] tensor on a ROCm device" % name)
    if grad_out.shape != y.shape or grad_out.device != y.device:
        raise RuntimeError("uc_nerf_amd.batch_norm_train_bwd: grad_out %s and y %s differ" % (tuple(grad_out.shape), tuple(y.shape)))
    grad_out, y = grad_out.detach(), y.detach()
    n, C = y.shape[0] // G, y.shape[1]
    S = y.numel() // (G * n * C)
    if not float(eps) > 0.0:
        raise RuntimeError("uc_nerf_amd.batch_norm_train_bwd: eps=%r (a positive float)" % (eps,))
    per_channel = (_bn_args("batch_norm_train_bwd", y, (G, C) if G > 1 else (C,), (saved_mean, "saved_mean"), (saved_var, "saved_var"))
                   + _bn_args("batch_norm_train_bwd", y, (C,), (weight, "weight"), (bias, "bias")))
    if out is not None:
        _bn_args("batch_norm_train_bwd", y, None, (out, "out"))
    P = L.lib().ucnerf_bn_partials(n, S)
    if P < 0:
        raise RuntimeError("uc_nerf_amd.batch_norm_train_bwd: y %s is outside what the kernels take (at least 2 and below 2^31 - 2^20 values per channel)"
                           % (tuple(y.shape),))
    grad_y = torch.empty_like(y) if out is None else out.detach()
    workspace = torch.empty((G, C, P, 2), dtype=torch.float64, device=y.device)
    grads = torch.empty((2, C), device=y.device)
    r, a = L.BnBwdReduceGroupsParams(), L.BnBwdApplyGroupsParams()
    for q in (r, a):
        q.G, q.n, q.C, q.S, q.workspace_pairs, q.eps, q.relu = G, n, C, S, G * C * P, float(eps), int(bool(relu))
        q.g, q.y, q.workspace = _ptr(grad_out), _ptr(y), _ptr(workspace)
        q.saved_mean, q.saved_var, q.weight, q.bias = (_ptr(t) for t in per_channel)
    a.grad_y, a.grad_weight, a.grad_bias = _ptr(grad_y), _ptr(grads[0]), _ptr(grads[1])
    _launch("ucnerf_bn_bwd_reduce_groups", r, y.device)
    _launch("ucnerf_bn_bwd_apply_groups", a, y.device)
    return (grad_y if out is None else out), grads[0], grads[1]


class _Conv3dBnTrain(torch.autograd.Function):
    """One CostRegNet layer in training mode: conv3d with the raw weight, then batch_norm_train out of place (the raw output survives for the
    backward).  The dgrad weight is packed in the forward, so the backward uses the weight's values as of the forward."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, skip, buffers, momentum, eps, stride, pad, relu, transposed, packed, packed_dgrad):
        running_mean, running_var, nbt = buffers
        w = packed if packed is not None else conv3d_pack(weight, transposed)
        y = conv3d(x, w, torch.zeros(w.cout, device=x.device), stride=stride, pad=pad, relu=False, skip=None, transposed=transposed)
        out, mean, var = batch_norm_train(y, gamma, beta, running_mean, running_var, nbt, momentum=momentum, eps=eps, relu=relu, skip=skip, out=None,
                                          return_stats=True)
        ctx.layer = (stride, pad, bool(relu), bool(transposed), float(eps), tuple(x.shape))
        ctx.packed_dgrad = None
        if ctx.needs_input_grad[0]:
            ctx.packed_dgrad = packed_dgrad if packed_dgrad is not None else conv3d_dgrad_pack(weight, stride, pad, transposed)
        ctx.save_for_backward(x.detach(), y, mean, var, gamma, beta)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, y, mean, var, gamma, beta = ctx.saved_tensors
        stride, pad, relu, transposed, eps, x_shape = ctx.layer
        grad_out = grad_out.contiguous()
        grad_skip = grad_out if ctx.needs_input_grad[4] else None
        grad_y, grad_gamma, grad_beta = batch_norm_train_bwd(grad_out, y, mean, var, gamma, beta, eps=eps, relu=relu)
        grad_w = conv3d_wgrad(x, grad_y, stride, pad, transposed) if ctx.needs_input_grad[1] else None
        grad_x = conv3d_dgrad(grad_y, ctx.packed_dgrad, x_shape, stride, pad, transposed) if ctx.needs_input_grad[0] else None
        return (grad_x, grad_w, grad_gamma if ctx.needs_input_grad[2] else None, grad_beta if ctx.needs_input_grad[3] else None, grad_skip) + (None,) * 9


class _Conv3dTrain(torch.autograd.Function):
    """A bare K = 3 convolution without bias (CostRegNet's `prob`) with its backward on the device."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad, packed, packed_dgrad):
        w = packed if packed is not None else conv3d_pack(weight, False)
        y = conv3d(x, w, torch.zeros(w.cout, device=x.device), stride=stride, pad=pad, relu=False, skip=None, transposed=False)
        ctx.layer = (stride, pad, tuple(x.shape))
        ctx.packed_dgrad = None
        if ctx.needs_input_grad[0]:
            ctx.packed_dgrad = packed_dgrad if packed_dgrad is not None else conv3d_dgrad_pack(weight, stride, pad, False)
        ctx.save_for_backward(x.detach())
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, = ctx.saved_tensors
        stride, pad, x_shape = ctx.layer
        grad_y = grad_y.contiguous()
        grad_w = conv3d_wgrad(x, grad_y, stride, pad, False) if ctx.needs_input_grad[1] else None
        grad_x = conv3d_dgrad(grad_y, ctx.packed_dgrad, x_shape, stride, pad, False) if ctx.needs_input_grad[0] else None
        return grad_x, grad_w, None, None, None, None


def _train_weight(weight, who):
    if not (torch.is_tensor(weight) and weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 5 and tuple(weight.shape[2:]) == (3, 3, 3)):
        raise RuntimeError("uc_nerf_amd.%s: the weight must be a float32 [cout,cin,3,3,3] ([cin,cout,3,3,3] transposed) tensor on a ROCm device" % who)


def conv3d_bn_train(x, weight, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5, stride=1, pad=1, relu=True,
                    skip=None, transposed=False, packed=None, packed_dgrad=None):
    """act(batch_norm(conv3d(x, weight))) (+ skip) with the batch's own statistics, DIFFERENTIABLE (once) in x, weight, bn_weight, bn_bias and
    skip, forward and backward on the device: `conv3d` and `batch_norm_train` (the running statistics move exactly as there), then
    `batch_norm_train_bwd`, `conv3d_wgrad` (only if the weight needs a gradient) and `conv3d_dgrad` (only if x does).  K = 3, pad 1, stride 1 or 2
    (even sizes), or the transposed form.  `packed` / `packed_dgrad`: what `conv3d_pack(weight, transposed)` / `conv3d_dgrad_pack(weight, ...)`
    made of the weight AS IT IS NOW (a module's cache); without them the weight is packed here.  Either way the backward uses the weight's
    values as of this call, whatever happens to the tensor afterwards."""
    _dev(x)
    _train_weight(weight, "conv3d_bn_train")
    return _Conv3dBnTrain.apply(x, weight, bn_weight, bn_bias, skip, (running_mean, running_var, num_batches_tracked), momentum, float(eps), int(stride),
                                int(pad), bool(relu), bool(transposed), packed, packed_dgrad)


def conv3d_train(x, weight, stride=1, pad=1, packed=None, packed_dgrad=None):
    """conv3d(x, weight) with a bias-free K = 3 kernel, differentiable (once) in x and weight on the device (`conv3d`, `conv3d_wgrad`,
    `conv3d_dgrad`); `packed` / `packed_dgrad` as in `conv3d_bn_train`."""
    _dev(x)
    _train_weight(weight, "conv3d_train")
    return _Conv3dTrain.apply(x, weight, int(stride), int(pad), packed, packed_dgrad)


def _same_pad(K, pad):
    return (int(K) - 1) // 2 if pad is None else int(pad)


def conv2d_wgrad(x, grad_y, K, stride=1, pad=None):
    """The weight gradient of `conv2d_bias_relu` (csrc/conv2d_bwd.hip: exact float32 on the matrix cores, split over chunks of whole output rows
    and folded in ascending chunk order, no atomics, two calls give the same bits).  x [n,cin,H,W] the layer's input, grad_y [n,cout,OH,OW] the
    gradient of its output; K 1, 3 or 5 with pad (K - 1) / 2 (the default), stride 1, or 2 with K 3 or 5 -> [cout,cin,K,K]."""
    x, grad_y = _f32(x.detach(), "x"), _f32(grad_y.detach(), "grad_y")
    K, stride, pad = int(K), int(stride), _same_pad(K, pad)
    if x.dim() != 4 or grad_y.dim() != 4 or x.device != grad_y.device or x.shape[0] != grad_y.shape[0] or 0 in x.shape[1:] or 0 in grad_y.shape[1:]:
        raise RuntimeError("uc_nerf_amd.conv2d_wgrad: x [n,cin,H,W] and grad_y [n,cout,OH,OW] on one device, got %s and %s" % (tuple(x.shape), tuple(grad_y.shape)))
    n, cin, H, W = x.shape
    cout = grad_y.shape[1]
    floats = L.lib().ucnerf_conv2d_wgrad_workspace_floats(n, cin, cout, H, W, K, stride, pad)
    if floats < 0:
        raise RuntimeError("uc_nerf_amd.conv2d_wgrad: %s" % L.lib().ucnerf_last_error().decode())
    want = tuple((s + 2 * pad - K) // stride + 1 for s in (H, W))
    if tuple(grad_y.shape[2:]) != want:
        raise RuntimeError("uc_nerf_amd.conv2d_wgrad: grad_y must be [%d,%d,%d,%d] for x %s with K=%d stride=%d pad=%d, got %s"
                           % ((n, cout) + want + (tuple(x.shape), K, stride, pad, tuple(grad_y.shape))))
    grad_w = torch.empty((cout, cin, K, K), device=x.device)
    workspace = torch.empty(floats, device=x.device)
    p = L.Conv2dWgradParams()
    p.n, p.cin, p.H, p.W, p.cout, p.K, p.stride, p.pad, p.workspace_floats = n, cin, H, W, cout, K, stride, pad, floats
    p.x, p.grad_y, p.workspace, p.grad_weight = _ptr(x), _ptr(grad_y), _ptr(workspace), _ptr(grad_w)
    _launch("ucnerf_conv2d_wgrad", p, x.device)
    return grad_w


class PackedDgrad2d:
    """A layer's weight [cout,cin,K,K] as `conv2d_dgrad` reads it (made by `conv2d_dgrad_pack`): stride 1, the transposed, flipped weight packed
    for `conv2d_bias_relu`; stride 2, a copy of the raw weight, which `ucnerf_conv2d_dgrad_s2` takes as it is."""
    __slots__ = ("weight", "cin", "cout", "K", "stride")

    def __init__(self, weight, cin, cout, K, stride):
        self.weight, self.cin, self.cout, self.K, self.stride = weight, cin, cout, K, stride


def conv2d_dgrad_pack(weight, stride=1, pad=None):
    """The weight of a layer prepared for `conv2d_dgrad` (a copy: the layer's weight may change afterwards).  K odd with pad (K - 1) / 2; stride
    1, or 2 with K 3 or 5."""
    if not torch.is_tensor(weight) or weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] % 2 == 0 or 0 in weight.shape:
        raise RuntimeError("uc_nerf_amd.conv2d_dgrad: the weight must be [cout,cin,K,K] with K odd")
    cout, cin, K, _ = weight.shape
    stride, pad = int(stride), _same_pad(K, pad)
    if pad != (K - 1) // 2 or stride not in (1, 2) or (stride == 2 and K not in (3, 5)):
        raise RuntimeError("uc_nerf_amd.conv2d_dgrad: stride 1, or 2 with K 3 or 5, and pad (K - 1) / 2 are built, got K=%d stride=%d pad=%d" % (K, stride, pad))
    w = _f32(weight.detach(), "weight")
    if stride == 2:
        return PackedDgrad2d(w.clone(), cin, cout, K, 2)
    return PackedDgrad2d(conv2d_pack(w.transpose(0, 1).flip(2, 3).contiguous()), cin, cout, K, 1)


def conv2d_dgrad(grad_y, weight, x_shape, stride=1, pad=None):
    """The input gradient of `conv2d_bias_relu` for a layer with pad (K - 1) / 2: stride 1 on `conv2d_bias_relu` itself (the weight transposed
    and flipped, zero bias, no ReLU), stride 2 (K 3 or 5) on `ucnerf_conv2d_dgrad_s2`, which works by parity class of the input pixel.  `weight`
    the layer's raw [cout,cin,K,K] weight or what `conv2d_dgrad_pack` made of it, `x_shape` the layer input's [n,cin,H,W].  A stride-2 layer needs
    even H and W (an odd size would need output_padding 0, which is not built): RuntimeError otherwise."""
    stride = int(stride)
    x_shape = tuple(int(v) for v in x_shape)
    if len(x_shape) != 4 or not torch.is_tensor(grad_y) or grad_y.dim() != 4 or min(x_shape) < 1:
        raise RuntimeError("uc_nerf_amd.conv2d_dgrad: grad_y must be [n,cout,OH,OW] and x_shape [n,cin,H,W], got %s and %s"
                           % (tuple(grad_y.shape) if torch.is_tensor(grad_y) else type(grad_y), x_shape))
    if stride == 2 and (x_shape[2] % 2 or x_shape[3] % 2):
        raise RuntimeError("uc_nerf_amd.conv2d_dgrad: a stride-2 layer needs even H, W (an odd size needs output_padding 0, which is not built), "
                           "got x_shape %s" % (x_shape,))
    w = weight if isinstance(weight, PackedDgrad2d) else conv2d_dgrad_pack(weight, stride, pad)
    if pad is not None and int(pad) != (w.K - 1) // 2 or stride != w.stride:
        raise RuntimeError("uc_nerf_amd.conv2d_dgrad: stride=%d pad=%r do not fit the weight (K=%d, prepared for stride %d, pad %d)"
                           % (stride, pad, w.K, w.stride, (w.K - 1) // 2))
    n, cin, H, W = x_shape
    want = (n, w.cout, H // stride, W // stride)
    if tuple(grad_y.shape) != want or cin != w.cin:
        raise RuntimeError("uc_nerf_amd.conv2d_dgrad: grad_y must be %s for x_shape %s and a weight with cin=%d, got %s" % (want, x_shape, w.cin, tuple(grad_y.shape)))
    grad_y = _f32(grad_y.detach(), "grad_y")
    if stride == 1:
        return conv2d_bias_relu(grad_y, w.weight, torch.zeros(cin, device=grad_y.device), stride=1, pad=(w.K - 1) // 2, relu=False)
    if w.weight.device != grad_y.device:
        raise RuntimeError("uc_nerf_amd.conv2d_dgrad: grad_y and the weight are on different devices")
    grad_x = torch.empty(x_shape, device=grad_y.device)
    p = L.Conv2dDgradS2Params()
    p.n, p.cin, p.H, p.W, p.cout, p.K = n, cin, H, W, w.cout, w.K
    p.grad_y, p.weight, p.grad_x = _ptr(grad_y), _ptr(w.weight), _ptr(grad_x)
    _launch("ucnerf_conv2d_dgrad_s2", p, grad_y.device)
    return grad_x


def conv2d_bias_grad(grad_y):
    """The bias gradient of a convolution: grad_y [n,cout,OH,OW] -> [cout], summed in float64 in a fixed order and rounded once."""
    grad_y = _f32(grad_y.detach(), "grad_y")
    if grad_y.dim() != 4 or 0 in grad_y.shape[1:]:
        raise RuntimeError("uc_nerf_amd.conv2d_bias_grad: grad_y must be [n,cout,OH,OW], got %s" % (tuple(grad_y.shape),))
    n, cout, OH, OW = grad_y.shape
    out = torch.zeros(cout, device=grad_y.device) if n == 0 else torch.empty(cout, device=grad_y.device)
    p = L.Conv2dBiasGradParams()
    p.n, p.cout, p.OH, p.OW, p.grad_y, p.grad_bias = n, cout, OH, OW, _ptr(grad_y), _ptr(out)
    _launch("ucnerf_conv2d_bias_grad", p, grad_y.device)
    return out


class _Conv2dBnTrain(torch.autograd.Function):
    """One batch-normed FeatureNet layer in training mode: conv2d_bias_relu with the raw weight, zero bias and no ReLU, then batch_norm_train out
    of place (the raw output survives for the backward).  The dgrad weight is prepared in the forward, so the backward uses the weight's values
    as of the forward."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, buffers, momentum, eps, stride, pad, relu, packed, packed_dgrad, groups):
        running_mean, running_var, nbt = buffers
        w = packed if packed is not None else conv2d_pack(weight)
        y = conv2d_bias_relu(x, w, torch.zeros(w.cout, device=x.device), stride=stride, pad=pad, relu=False)
        out, mean, var = batch_norm_train(y, gamma, beta, running_mean, running_var, nbt, momentum=momentum, eps=eps, relu=relu, skip=None, out=None,
                                          return_stats=True, groups=groups)
        ctx.layer = (w.K, stride, pad, bool(relu), float(eps), tuple(x.shape), groups)
        ctx.packed_dgrad = None
        if ctx.needs_input_grad[0]:
            ctx.packed_dgrad = packed_dgrad if packed_dgrad is not None else conv2d_dgrad_pack(weight, stride, pad)
        ctx.save_for_backward(x.detach(), y, mean, var, gamma, beta)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, y, mean, var, gamma, beta = ctx.saved_tensors
        K, stride, pad, relu, eps, x_shape, groups = ctx.layer
        grad_y, grad_gamma, grad_beta = batch_norm_train_bwd(grad_out.contiguous(), y, mean, var, gamma, beta, eps=eps, relu=relu, groups=groups)
        grad_w = conv2d_wgrad(x, grad_y, K, stride, pad) if ctx.needs_input_grad[1] else None
        grad_x = conv2d_dgrad(grad_y, ctx.packed_dgrad, x_shape, stride, pad) if ctx.needs_input_grad[0] else None
        return (grad_x, grad_w, grad_gamma if ctx.needs_input_grad[2] else None, grad_beta if ctx.needs_input_grad[3] else None) + (None,) * 9


class _Conv2dTrain(torch.autograd.Function):
    """A bare convolution, with or without bias (FeatureNet's out1, inner1, inner2, out2, out3), with its backward on the device."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, packed, packed_dgrad):
        w = packed if packed is not None else conv2d_pack(weight)
        y = conv2d_bias_relu(x, w, bias if bias is not None else torch.zeros(w.cout, device=x.device), stride=stride, pad=pad, relu=False)
        ctx.layer = (w.K, stride, pad, tuple(x.shape))
        ctx.packed_dgrad = None
        if ctx.needs_input_grad[0]:
            ctx.packed_dgrad = packed_dgrad if packed_dgrad is not None else conv2d_dgrad_pack(weight, stride, pad)
        ctx.save_for_backward(x.detach())
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, = ctx.saved_tensors
        K, stride, pad, x_shape = ctx.layer
        grad_y = grad_y.contiguous()
        grad_w = conv2d_wgrad(x, grad_y, K, stride, pad) if ctx.needs_input_grad[1] else None
        grad_b = conv2d_bias_grad(grad_y) if ctx.needs_input_grad[2] else None
        grad_x = conv2d_dgrad(grad_y, ctx.packed_dgrad, x_shape, stride, pad) if ctx.needs_input_grad[0] else None
        return grad_x, grad_w, grad_b, None, None, None, None


def _train_weight2d(weight, stride, pad, who):
    if not (torch.is_tensor(weight) and weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4 and weight.shape[2] == weight.shape[3]
            and weight.shape[2] in (1, 3, 5)):
        raise RuntimeError("uc_nerf_amd.%s: the weight must be a float32 [cout,cin,K,K] tensor with K 1, 3 or 5 on a ROCm device" % who)
    K = weight.shape[2]
    if pad != (K - 1) // 2 or stride not in (1, 2) or (stride == 2 and K == 1):
        raise RuntimeError("uc_nerf_amd.%s: stride 1, or 2 with K 3 or 5, and pad (K - 1) / 2 are built, got K=%d stride=%d pad=%d" % (who, K, stride, pad))


def conv2d_bn_train(x, weight, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5, stride=1, pad=1, relu=True,
                    packed=None, packed_dgrad=None, groups=1):
    """act(batch_norm(conv2d(x, weight))) with the batch's own statistics, DIFFERENTIABLE (once) in x, weight, bn_weight and bn_bias, forward and
    backward on the device: `conv2d_bias_relu` and `batch_norm_train` (the running statistics move exactly as there), then
    `batch_norm_train_bwd`, `conv2d_wgrad` (only if the weight needs a gradient) and `conv2d_dgrad` (only if x does).  K 1, 3 or 5 with pad
    (K - 1) / 2, stride 1, or 2 with K 3 or 5 (even sizes).  `packed` / `packed_dgrad`: what `conv2d_pack(weight)` / `conv2d_dgrad_pack(weight,
    stride, pad)` made of the weight AS IT IS NOW (a module's cache); without them the weight is prepared here.  Either way the backward uses the
    weight's values as of this call, whatever happens to the tensor afterwards.  `groups` = G > 1: x is G groups of n / G consecutive images and the
    batch-norm keeps its statistics per group (`batch_norm_train`'s `groups`); the convolution and its gradients are per image anyway."""
    groups = _bn_groups(groups, x, "conv2d_bn_train")
    _dev(x)
    _train_weight2d(weight, int(stride), int(pad), "conv2d_bn_train")
    return _Conv2dBnTrain.apply(x, weight, bn_weight, bn_bias, (running_mean, running_var, num_batches_tracked), momentum, float(eps), int(stride), int(pad),
                                bool(relu), packed, packed_dgrad, groups)


def conv2d_train(x, weight, bias=None, stride=1, pad=0, packed=None, packed_dgrad=None):
    """conv2d(x, weight) + bias, differentiable (once) in x, weight and bias on the device (`conv2d_bias_relu`, `conv2d_wgrad`, `conv2d_dgrad`,
    `conv2d_bias_grad`; the bias gradient is computed only when the bias requires one); shapes and `packed` / `packed_dgrad` as in
    `conv2d_bn_train`."""
    _dev(x)
    _train_weight2d(weight, int(stride), int(pad), "conv2d_train")
    return _Conv2dTrain.apply(x, weight, bias, int(stride), int(pad), packed, packed_dgrad)
