"""Evaluation on the device: depth and image metrics, the LPIPS kernels and the validation-image ops."""
import ctypes as C

import torch

from .. import _lib as L
from ._core import _dev, _f32, _launch, _on, _ptr, _stream


def _eval_workspace(n, H, W, dev):
    floats = L.lib().ucnerf_eval_workspace_floats(n, H, W)
    if floats < 0:
        raise RuntimeError("uc_nerf_amd: eval workspace: %s" % L.lib().ucnerf_last_error().decode())
    return torch.empty(floats, device=dev)


def depth_eval(gt, pred, mask=None, min_depth=1e-4, max_depth=100., raw=False):
    """Median-scaled depth errors of utils/evaluation.py:29-74 on the device.  gt, pred [n,H,W] float32, mask [n,H,W] uint8 or None (at the ground
    truth's resolution).  Returns device tensors, nothing is read back and nothing synchronises:
      ratio [1] (NaN when no pixel is valid), medians [2] (gt, pred), empty [1] int32 (1: no valid pixel in any image),
      counts [n,4] int32 (valid, a1, a2, a3), errors [n,7] float32 (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3),
      flags [n] int32 (1: the image has no valid pixel -- the reference leaves it out of its mean), packed [4 + 12 n]: all of it in one tensor.
    raw=True: compute_errors (:8-26) on the values as given -- every pixel valid, no scaling, no clamping."""
    gt, pred = _f32(gt, "gt"), _f32(pred, "pred")
    if gt.dim() != 3 or pred.shape != gt.shape or pred.device != gt.device:
        raise RuntimeError("uc_nerf_amd.depth_eval: gt and pred must be [n,H,W] on one device, got %s and %s" % (tuple(gt.shape), tuple(pred.shape)))
    if mask is not None:
        _dev(mask)
        if mask.dtype != torch.uint8 or mask.shape != gt.shape or mask.device != gt.device:
            raise RuntimeError("uc_nerf_amd.depth_eval: mask must be uint8 of gt's shape on gt's device, got %s %s" % (mask.dtype, tuple(mask.shape)))
        mask = mask.contiguous()
    n, H, W = gt.shape
    dev = gt.device
    p = L.DepthEvalParams()
    p.n, p.H, p.W, p.raw, p.min_depth, p.max_depth = n, H, W, int(raw), float(min_depth), float(max_depth)
    ws = _eval_workspace(n, H, W, dev)
    out = torch.empty(4 + 12 * n, device=dev)
    p.gt, p.pred, p.mask, p.workspace, p.out = _ptr(gt), _ptr(pred), _ptr(mask), _ptr(ws), _ptr(out)
    _launch("ucnerf_depth_eval", p, dev)
    words, rows = out.view(torch.int32), out[4:].view(n, 12)
    return dict(ratio=out[0:1], empty=words[1:2], medians=out[2:4], counts=rows[:, 0:4].view(torch.int32), errors=rows[:, 4:11],
                flags=rows[:, 11].view(torch.int32), packed=out)


def image_eval(gt, pred, ssim=True):
    """Per-image mse, psnr and ssim of utils/evaluation.py:82-83, :89-96 on the device.  gt, pred [n,3,H,W] float32, H, W >= 7 (ssim=False: the image error alone, any size, ssim = NaN).  Returns device
    tensors (no read-back, no synchronisation): mse [n], psnr [n], ssim [n], gt_max [n], packed [n,4]."""
    gt, pred = _f32(gt, "gt"), _f32(pred, "pred")
    if gt.dim() != 4 or gt.shape[1] != 3 or pred.shape != gt.shape or pred.device != gt.device:
        raise RuntimeError("uc_nerf_amd.image_eval: gt and pred must be [n,3,H,W] on one device, got %s and %s" % (tuple(gt.shape), tuple(pred.shape)))
    n, _, H, W = gt.shape
    dev = gt.device
    p = L.ImageEvalParams()
    p.n, p.H, p.W, p.no_ssim = n, H, W, int(not ssim)
    ws = _eval_workspace(n, H, W, dev)
    out = torch.empty(n, 4, device=dev)
    p.gt, p.pred, p.workspace, p.out = _ptr(gt), _ptr(pred), _ptr(ws), _ptr(out)
    _launch("ucnerf_image_eval", p, dev)
    return dict(mse=out[:, 0], psnr=out[:, 1], ssim=out[:, 2], gt_max=out[:, 3], packed=out)


class PackedConv:
    """A convolution weight [cout,cin,K,K] in the order `conv2d_bias_relu`'s kernel walks it (made once by `conv2d_pack`)."""
    __slots__ = ("packed", "cin", "cout", "K")

    def __init__(self, packed, cin, cout, K):
        self.packed, self.cin, self.cout, self.K = packed, cin, cout, K


def conv2d_pack(weight):
    """Packs a [cout,cin,K,K] float32 device weight (K <= 11) for `conv2d_bias_relu`: one launch, nothing read back."""
    weight = _f32(weight.detach(), "weight")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or 0 in weight.shape:
        raise RuntimeError("uc_nerf_amd.conv2d_pack: weight must be [cout,cin,K,K], got %s" % (tuple(weight.shape),))
    cout, cin, K, _ = weight.shape
    floats = L.lib().ucnerf_conv2d_packed_floats(cin, cout, K)
    if floats < 0:
        raise RuntimeError("uc_nerf_amd.conv2d_pack: %s" % L.lib().ucnerf_last_error().decode())
    packed = torch.empty(floats, device=weight.device)
    p = L.Conv2dPackParams()
    p.cin, p.cout, p.K, p.weight, p.packed = cin, cout, K, _ptr(weight), _ptr(packed)
    _launch("ucnerf_conv2d_pack", p, weight.device)
    return PackedConv(packed, cin, cout, K)


def conv2d_bias_relu(x, weight, bias, stride=1, pad=0, relu=True, shift=None, scale=None):
    """relu(conv2d(x, weight, bias, stride, zero padding `pad`)), forward only, exact float32 on the matrix cores (csrc/lpips.hip: the order of
    the sums is fixed, two calls give the same bits).  x [n,cin,H,W]; weight a `PackedConv` or a [cout,cin,K,K] tensor (packed on the spot);
    bias [cout].  shift / scale [cin]: the input is read as (x - shift[c]) / scale[c] inside the image, the padding stays zero.  No autograd:
    inputs that require grad are used detached."""
    x = _f32(x.detach(), "x")
    w = weight if isinstance(weight, PackedConv) else conv2d_pack(weight)
    bias = _f32(bias.detach(), "bias")
    if x.dim() != 4 or x.shape[1] != w.cin or bias.numel() != w.cout or bias.device != x.device or w.packed.device != x.device:
        raise RuntimeError("uc_nerf_amd.conv2d_bias_relu: x must be [n,%d,H,W] and bias [%d] on the weight's device, got %s and %s"
                           % (w.cin, w.cout, tuple(x.shape), tuple(bias.shape)))
    if (shift is None) != (scale is None):
        raise RuntimeError("uc_nerf_amd.conv2d_bias_relu: shift and scale go together")
    if shift is not None:
        shift, scale = _f32(shift.detach(), "shift"), _f32(scale.detach(), "scale")
        if shift.numel() != w.cin or scale.numel() != w.cin or shift.device != x.device or scale.device != x.device:
            raise RuntimeError("uc_nerf_amd.conv2d_bias_relu: shift and scale must be [%d] on x's device" % w.cin)
    n, _, H, W = x.shape
    stride, pad = int(stride), int(pad)
    if stride < 1 or pad < 0 or H + 2 * pad < w.K or W + 2 * pad < w.K:
        raise RuntimeError("uc_nerf_amd.conv2d_bias_relu: stride=%d pad=%d on a %d x %d input with a %d x %d kernel" % (stride, pad, H, W, w.K, w.K))
    OH, OW = (H + 2 * pad - w.K) // stride + 1, (W + 2 * pad - w.K) // stride + 1
    y = torch.empty(n, w.cout, OH, OW, device=x.device)
    p = L.Conv2dParams()
    p.n, p.cin, p.H, p.W, p.cout, p.K, p.stride, p.pad, p.relu = n, w.cin, H, W, w.cout, w.K, stride, pad, int(bool(relu))
    p.x, p.packed, p.bias, p.shift, p.scale, p.y = _ptr(x), _ptr(w.packed), _ptr(bias), _ptr(shift), _ptr(scale), _ptr(y)
    _launch("ucnerf_conv2d_bias_relu", p, x.device)
    return y


def maxpool2d(x):
    """max_pool2d(x, 3, 2) (no padding, floor mode) of [n,C,H,W] float32, H, W >= 3; any values, -inf included.  No autograd."""
    x = _f32(x.detach(), "x")
    if x.dim() != 4 or x.shape[2] < 3 or x.shape[3] < 3:
        raise RuntimeError("uc_nerf_amd.maxpool2d: x must be [n,C,H,W] with H, W >= 3, got %s" % (tuple(x.shape),))
    n, C, H, W = x.shape
    y = torch.empty(n, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1, device=x.device)
    p = L.Maxpool2dParams()
    p.planes, p.H, p.W, p.x, p.y = n * C, H, W, _ptr(x), _ptr(y)
    _launch("ucnerf_maxpool2d", p, x.device)
    return y


def lpips_layer(f0, f1, lin, out=None):
    """One feature level of LPIPS in one launch: per pixel n = f / (sqrt(sum_c f^2) + 1e-10) for both maps, d = sum_c lin[c] (n0 - n1)^2, and
    the mean of d over the pixels -> [n].  f0, f1 [n,C,h,w], lin [C].  With `out` ([n] float32) the mean is ADDED to it in place (the levels
    of a network in the caller's order) and `out` is returned.  The normalised maps are never stored.  No autograd."""
    f0, f1, lin = _f32(f0.detach(), "f0"), _f32(f1.detach(), "f1"), _f32(lin.detach(), "lin")
    if f0.dim() != 4 or f1.shape != f0.shape or f1.device != f0.device or lin.device != f0.device or lin.numel() != f0.shape[1] or 0 in f0.shape[1:]:
        raise RuntimeError("uc_nerf_amd.lpips_layer: f0, f1 [n,C,h,w] and lin [C] on one device, got %s, %s and %s"
                           % (tuple(f0.shape), tuple(f1.shape), tuple(lin.shape)))
    n, C, h, w = f0.shape
    p = L.LpipsLayerParams()
    p.accumulate = int(out is not None)
    if out is None:
        out = torch.empty(n, device=f0.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == (n,) and out.is_contiguous() and out.device == f0.device):
        raise RuntimeError("uc_nerf_amd.lpips_layer: out must be a contiguous float32 [%d] tensor on f0's device" % n)
    p.n, p.C, p.h, p.w = n, C, h, w
    p.f0, p.f1, p.lin, p.out = _ptr(f0), _ptr(f1), _ptr(lin), _ptr(out)
    _launch("ucnerf_lpips_layer", p, f0.device)
    return out


def lpips_workspace_floats(n, H, W):
    floats = L.lib().ucnerf_lpips_workspace_floats(n, H, W)
    if floats < 0:
        raise RuntimeError("uc_nerf_amd: lpips workspace: %s" % L.lib().ucnerf_last_error().decode())
    return int(floats)


def lpips_alex(a, b, convs, biases, lins, shift, scale, workspace=None):
    """The whole LPIPS(net='alex') chain for n pairs a, b [n,3,H,W] float32 in [-1, 1] (H, W >= 31) -> [n] on the device, nothing read back.
    convs: five `PackedConv` (conv1 .. conv5 of AlexNet's features); biases, lins: five vectors each; shift, scale [3].  `workspace`: a float32
    tensor of at least lpips_workspace_floats(n, H, W) elements (allocated when None); its contents do not matter.  No autograd."""
    a, b = _f32(a.detach(), "a"), _f32(b.detach(), "b")
    if a.dim() != 4 or a.shape[1] != 3 or b.shape != a.shape or b.device != a.device:
        raise RuntimeError("uc_nerf_amd.lpips_alex: a and b must be [n,3,H,W] on one device, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    geometry = ((3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3))
    if len(convs) != 5 or len(biases) != 5 or len(lins) != 5:
        raise RuntimeError("uc_nerf_amd.lpips_alex: five convolutions, biases and lin vectors")
    dev = a.device
    n, _, H, W = a.shape
    p = L.LpipsAlexParams()
    keep = []
    for l, (cin, cout, K) in enumerate(geometry):
        c = convs[l]
        if not isinstance(c, PackedConv) or (c.cin, c.cout, c.K) != (cin, cout, K) or c.packed.device != dev:
            raise RuntimeError("uc_nerf_amd.lpips_alex: convolution %d must be a PackedConv of %d -> %d, %d x %d on the images' device" % (l + 1, cin, cout, K, K))
        bl, ll = _f32(biases[l].detach(), "bias"), _f32(lins[l].detach(), "lin")
        if bl.numel() != cout or ll.numel() != cout or bl.device != dev or ll.device != dev:
            raise RuntimeError("uc_nerf_amd.lpips_alex: bias and lin of level %d must be [%d] on the images' device" % (l, cout))
        keep += [bl, ll]
        p.packed[l], p.bias[l], p.lin[l] = _ptr(c.packed), _ptr(bl), _ptr(ll)
    shift, scale = _f32(shift.detach(), "shift"), _f32(scale.detach(), "scale")
    if shift.numel() != 3 or scale.numel() != 3 or shift.device != dev or scale.device != dev:
        raise RuntimeError("uc_nerf_amd.lpips_alex: shift and scale must be [3] on the images' device")
    floats = lpips_workspace_floats(n, H, W)
    if workspace is None:
        workspace = torch.empty(floats, device=dev)
    elif not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous()
              and workspace.device == dev and workspace.numel() >= floats):
        raise RuntimeError("uc_nerf_amd.lpips_alex: workspace must be a contiguous float32 tensor of at least %d elements on the images' device" % floats)
    out = torch.empty(n, device=dev)
    p.n, p.H, p.W = n, H, W
    p.a, p.b, p.shift, p.scale, p.workspace, p.out = _ptr(a), _ptr(b), _ptr(shift), _ptr(scale), _ptr(workspace), _ptr(out)
    _launch("ucnerf_lpips_alex", p, dev)
    return out


def image_group_pixels():
    """Pixels one workgroup of the image kernels covers (and folds into one atomicMin / atomicMax)."""
    return int(L.lib().ucnerf_image_group_pixels())


def _is_cell(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.numel() == 2 and t.is_contiguous()


def minmax_reset(cell=None, device=None):
    """Empties a range cell (a new one on `device` when none is given) and returns it: an int32 [2] device tensor holding the order keys of the
    smallest and largest nan_to_num(depth) folded in so far.  `minmax_value` decodes it; an empty cell decodes to (NaN, NaN)."""
    if cell is None:
        if device is None:
            raise RuntimeError("uc_nerf_amd.minmax_reset: a cell or a device")
        cell = torch.empty(2, dtype=torch.int32, device=device)
    if not _is_cell(cell):
        raise RuntimeError("uc_nerf_amd: a range cell is a contiguous int32 [2] tensor on a ROCm device (minmax_reset makes one)")
    with _on(cell.device):
        L.check(L.lib().ucnerf_minmax_reset(_ptr(cell), C.c_void_p(_stream())), "ucnerf_minmax_reset")
    return cell


def minmax_value(cell):
    """The cell's range as a float32 [2] device tensor (min, max); one tiny launch, nothing is read back."""
    if not _is_cell(cell):
        raise RuntimeError("uc_nerf_amd: a range cell is a contiguous int32 [2] tensor on a ROCm device (minmax_reset makes one)")
    out = torch.empty(2, device=cell.device)
    with _on(cell.device):
        L.check(L.lib().ucnerf_minmax_read(_ptr(cell), _ptr(out), C.c_void_p(_stream())), "ucnerf_minmax_read")
    return out


def image_put(rgb, depth, first_pixel, rgb_chw, depth_hw, cell=None):
    """One rendered chunk into the image planes, in place: rgb [n,3], depth [n] -> rgb_chw [3,H,W] (clamped to [0,1] as torch.clamp does: NaN and
    -0.0 stay) and depth_hw [H,W] at pixels first_pixel .. first_pixel + n - 1 of the flattened grid; with `cell` the chunk's depth range is folded
    into it in the same launch.  An overrun of the image raises."""
    rgb, depth = _f32(rgb, "rgb"), _f32(depth, "depth")
    dev = rgb.device
    n = depth.numel()
    if rgb.numel() != 3 * n or rgb.shape[-1] != 3:
        raise RuntimeError("uc_nerf_amd.image_put: rgb must be [n,3] and depth [n], got %s and %s" % (tuple(rgb.shape), tuple(depth.shape)))
    for t, name in ((rgb_chw, "rgb_chw"), (depth_hw, "depth_hw")):
        _dev(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or depth.device != dev:
            raise RuntimeError("uc_nerf_amd.image_put: %s must be a contiguous float32 tensor on the chunk's device" % name)
    pixels = depth_hw.numel()
    if rgb_chw.numel() != 3 * pixels or rgb_chw.shape[0] != 3:
        raise RuntimeError("uc_nerf_amd.image_put: rgb_chw must be [3,H,W] for depth_hw [H,W], got %s and %s" % (tuple(rgb_chw.shape), tuple(depth_hw.shape)))
    if cell is not None and not (_is_cell(cell) and cell.device == dev):
        raise RuntimeError("uc_nerf_amd.image_put: cell must be a range cell on the chunk's device")
    p = L.ImagePutParams()
    p.n, p.first_pixel, p.pixels = n, int(first_pixel), pixels
    p.rgb, p.depth, p.rgb_chw, p.depth_hw, p.minmax = _ptr(rgb), _ptr(depth), _ptr(rgb_chw), _ptr(depth_hw), _ptr(cell)
    _launch("ucnerf_image_put", p, dev)


def depth_minmax(depth, cell=None):
    """min and max of nan_to_num(depth) as a float32 [2] device tensor.  With `cell` the map is folded into that cell (not reset first) and the
    cell's range so far is returned."""
    depth = _f32(depth, "depth")
    dev = depth.device
    if cell is None:
        cell = minmax_reset(device=dev)
    elif not (_is_cell(cell) and cell.device == dev):
        raise RuntimeError("uc_nerf_amd.depth_minmax: cell must be a range cell on the map's device")
    p = L.DepthMinmaxParams()
    p.count, p.depth, p.minmax = depth.numel(), _ptr(depth), _ptr(cell)
    _launch("ucnerf_depth_minmax", p, dev)
    return minmax_value(cell)


def colormap_table(table, device):
    """A 256 x 3 uint8 colour table (numpy array or tensor) as a contiguous device tensor."""
    t = table if torch.is_tensor(table) else torch.as_tensor(table)
    if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
        raise RuntimeError("uc_nerf_amd: a colour table is 256 x 3 uint8, got %s %s" % (t.dtype, tuple(t.shape)))
    return t.to(device).contiguous()


def depth_colormap(depth, table=None, minmax=None, want_index=True, want_color=True):
    """visualize_depth's arithmetic (utils/utils.py:65-76) on the device: depth (any shape, float32) -> (index uint8 of depth's shape or None,
    color float32 [3, *depth.shape] or None).  `minmax`: None -- the map's own range (one more launch); a range cell; or a pair of Python
    floats (the reference's minmax= argument).  `table`: 256 x 3 uint8 on the device (colormap_table), needed for the colour image.
    The uint8 conversion is defined where numpy's is not: NaN -> 0, below 0 -> 0, above 255 -> 255."""
    depth = _f32(depth, "depth")
    dev = depth.device
    p = L.DepthColormapParams()
    p.count, p.depth = depth.numel(), _ptr(depth)
    cell = None
    if minmax is None:
        cell = minmax_reset(device=dev)
        q = L.DepthMinmaxParams()
        q.count, q.depth, q.minmax = depth.numel(), _ptr(depth), _ptr(cell)
        _launch("ucnerf_depth_minmax", q, dev)
    elif torch.is_tensor(minmax):
        if not (_is_cell(minmax) and minmax.device == dev):
            raise RuntimeError("uc_nerf_amd.depth_colormap: a tensor minmax must be a range cell on the map's device (a pair of floats otherwise)")
        cell = minmax
    else:
        p.range_host[0], p.range_host[1] = float(minmax[0]), float(minmax[1])
    p.minmax = _ptr(cell)
    if want_color:
        if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.uint8 and tuple(table.shape) == (256, 3)
                and table.is_contiguous() and table.device == dev):
            raise RuntimeError("uc_nerf_amd.depth_colormap: table must be a contiguous 256 x 3 uint8 tensor on the map's device (colormap_table)")
        p.table = _ptr(table)
    index = torch.empty(depth.shape, dtype=torch.uint8, device=dev) if want_index else None
    color = torch.empty((3,) + tuple(depth.shape), device=dev) if want_color else None
    p.index, p.color = _ptr(index), _ptr(color)
    _launch("ucnerf_depth_colormap", p, dev)
    return index, color
