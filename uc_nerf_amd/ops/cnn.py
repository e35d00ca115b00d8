"""The 3-D convolutions of the MVS cost regularisation on the device (csrc/conv3d.hip)."""
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
