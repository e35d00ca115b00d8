"""Mirror of the reference's utils/evaluation.py (compute_errors, depth_evaluation, rgb_evaluation) on the device.

Same names, argument orders and return shapes; the arithmetic runs in `ucnerf_depth_eval` / `ucnerf_image_eval` (csrc/metrics.hip).  Inputs may
be numpy arrays (moved to the device) or device tensors (used where they are, as a validation step that keeps `rgb` and `depth` on the device
hands them over); they are not modified -- the reference scales its masked COPIES in place, never its arguments.  Each function reads ONE small
vector back: no cv2, skimage or lpips is needed to finish a validation epoch.

Differences, all deliberate:
  * values are taken as float32 (what the reference's callers pass); a float64 numpy input is rounded first;
  * `pred_masks` at another resolution than the ground truth raises NotImplementedError (the reference resizes them with cv2.resize);
  * LPIPS needs a network's weights, which are in no tree: `rgb_evaluation` returns float('nan') for it unless the caller passes `lpips_fn`.
    `LPIPS` below is such a function on the device: the caller brings the two state dicts, the arithmetic (AlexNet's feature stack and the
    distance, csrc/lpips.hip) is the library's, so neither `lpips` nor `torchvision` has to be installed;
  * SSIM is skimage's documented default restated (7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, 3-pixel crop), see DESIGN.md.
"""
import os

import numpy as np
import torch

from .. import ops


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("uc_nerf_amd.utils.evaluation: no ROCm device (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(x, dev=None):
    """numpy array or tensor -> contiguous float32 device tensor (a device float32 tensor is used in place)."""
    if torch.is_tensor(x):
        t = x.detach()
        if not t.is_cuda:
            t = t.to(dev or _device())
    else:
        t = torch.from_numpy(np.ascontiguousarray(x)).to(dev or _device())
    return t.to(torch.float32).contiguous()


def compute_errors(gt, pred):
    """utils/evaluation.py:8-26.  gt, pred 1-D -> (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3)."""
    g = _to_device(gt)
    q = _to_device(pred, g.device)
    if g.dim() != 1 or q.shape != g.shape:
        raise ValueError("compute_errors takes two 1-D arrays of one length, got %s and %s" % (tuple(g.shape), tuple(q.shape)))
    if g.numel() == 0:
        nan = float("nan")                                  # (numpy: the mean of an empty array, with a warning)
        return (np.float32(nan),) * 4 + (nan,) * 3
    out = ops.depth_eval(g.view(1, 1, -1), q.view(1, 1, -1), raw=True)["packed"].cpu().numpy()      # the one copy
    c = out[4:8].view(np.int32).astype(np.float64)
    e = out[8:12]
    return e[0], e[1], e[2], e[3], c[1] / c[0], c[2] / c[0], c[3] / c[0]


def depth_evaluation(gt_depths, pred_depths, savedir=None, pred_masks=None, min_depth=0.0001, max_depth=100):
    """utils/evaluation.py:29-74.  [n,H,W] ground truth and predictions -> float64 np.ndarray[7], the mean over the images that have a valid
    pixel of (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3) after scaling the predictions by median(gt) / median(pred)."""
    assert gt_depths.shape[0] == pred_depths.shape[0]
    g = _to_device(gt_depths)
    q = _to_device(pred_depths, g.device)
    if g.dim() != 3 or q.shape != g.shape:
        raise ValueError("depth_evaluation takes [n,H,W] depths of one shape, got %s and %s" % (tuple(g.shape), tuple(q.shape)))
    m = None
    if pred_masks is not None:
        if tuple(pred_masks.shape) != tuple(g.shape):
            raise NotImplementedError("pred_masks of shape %s for depths of shape %s: the reference resizes them with cv2.resize, which this "
                                      "mirror does not do -- pass masks at the ground truth's resolution" % (tuple(pred_masks.shape), tuple(g.shape)))
        m = pred_masks.detach() if torch.is_tensor(pred_masks) else torch.from_numpy(np.ascontiguousarray(pred_masks))
        m = m.to(g.device).to(torch.uint8).contiguous()                  # .astype(np.uint8) ... > 0.5 (:44)
    if g.numel() == 0:
        raise ValueError("need at least one array to concatenate")
    out = ops.depth_eval(g, q, m, min_depth, max_depth)["packed"].cpu().numpy()      # the one copy
    if out[1:2].view(np.int32)[0]:
        raise ValueError("depth_evaluation: no image has a valid pixel (need at least one array to concatenate)")
    rows = out[4:].reshape(-1, 12)
    counts = rows[:, 0:4].view(np.int32).astype(np.float64)
    keep = rows[:, 11].view(np.int32) == 0                               # `continue` (:47-48)
    errors = np.concatenate([rows[keep, 4:8].astype(np.float64), counts[keep, 1:4] / counts[keep, 0:1]], axis=1)      # bool.mean(): float64
    mean_errors = errors.mean(0)

    print("\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
    print(("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
    print("\n-> Done!")
    return mean_errors


def rgb_evaluation(gts, predicts, savedir, lpips_fn=None):
    """utils/evaluation.py:76-101.  [n,3,H,W] images in [0,1] -> (psnr, ssim, lpips).  lpips is float('nan') unless `lpips_fn` is given: it is
    called as the reference calls its metric, lpips_fn(2 gts - 1, 2 predicts - 1) on float32 tensors, and the mean of what it returns is used."""
    g = _to_device(gts)
    q = _to_device(predicts, g.device)
    if g.dim() != 4 or g.shape[1] != 3 or q.shape != g.shape:
        raise ValueError("rgb_evaluation takes [n,3,H,W] images of one shape, got %s and %s" % (tuple(g.shape), tuple(q.shape)))
    out = ops.image_eval(g, q)["packed"].cpu().numpy()                   # the one copy: [n,4] = mse, psnr, ssim, max(gt)
    assert out[:, 3].max() <= 1
    psnr = out[:, 1].mean()
    ssim = out[:, 2].astype(np.float64).mean()
    lpips_ = float("nan")
    if lpips_fn is not None:
        lpips_ = lpips_fn(2 * g - 1, 2 * q - 1)
        if hasattr(lpips_, "mean"):
            lpips_ = lpips_.mean()
    result = 'psnr: {0}, ssim: {1}, lpips: {2}'.format(psnr, ssim, lpips_)
    if savedir is not None:
        with open(os.path.join(savedir, 'rgb_evaluation.txt'), 'w'):     # (the reference opens the file and writes nothing into it)
            pass
    print(result)
    return psnr, ssim, lpips_


# AlexNet's five convolutions as torchvision numbers them inside `features`, with (cin, cout, K); the lpips package's scaling layer
_ALEX_CONVS = ((0, 3, 64, 11), (3, 64, 192, 5), (6, 192, 384, 3), (8, 384, 256, 3), (10, 256, 256, 3))
_LPIPS_SHIFT = (-0.030, -0.088, -0.188)
_LPIPS_SCALE = (0.458, 0.448, 0.450)


class LPIPS:
    """LPIPS(net='alex') of the `lpips` package (v0.1) on the device, as a function for `rgb_evaluation(..., lpips_fn=...)`.

    LPIPS(alexnet_state, lin_state, device=None):
      alexnet_state  torchvision's AlexNet state dict: `features.{0,3,6,8,10}.{weight,bias}` (the same keys without `features.` are taken too;
                     other keys, such as the classifier's, are ignored);
      lin_state      the lpips package's linear layers: `lin{0..4}.model.1.weight`, each [1,C,1,1] -- or a list of five [C] vectors.
    THE KEY NAMES ARE WRITTEN FROM KNOWLEDGE OF THE TWO PACKAGES AND ARE NOT VERIFIED AGAINST THEM: neither is installed where this was built.
    The arithmetic is checked against a float64 restatement of the chain (tests/lpips_cases.py), with random weights of the real shapes.

    A wrong shape, a missing key or a negative lin weight raises a ValueError that names the offender (the lpips package trains its lin
    layers under a non-negativity clamp: a negative one means the wrong file).  The weights are packed once, here.
    __call__(a, b): two [n,3,H,W] float32 tensors in [-1, 1] (H, W >= 31) -> a device tensor [n]; nothing is read back, no autograd.

    Long batches run in chunks of `max_pairs` pairs, so that the workspace stays bounded: by default the largest count whose workspace
    (`ops.lpips_workspace_floats`, about 7.5 MB a pair at 256 x 320) fits WORKSPACE_BYTES = 64 MiB, at least 1 -- 8 pairs at 256 x 320.  A pair's
    result does not depend on the chunk it is in (every output element has one fixed summation order)."""

    WORKSPACE_BYTES = 64 << 20

    def __init__(self, alexnet_state, lin_state, device=None, max_pairs=None):
        dev = torch.device(device) if device is not None else _device()
        if dev.type != "cuda":
            raise RuntimeError("uc_nerf_amd.utils.evaluation.LPIPS: device %s is not a ROCm device (there is no CPU fallback)" % dev)
        if max_pairs is not None and int(max_pairs) < 1:
            raise ValueError("LPIPS: max_pairs = %r, need at least 1" % (max_pairs,))
        self.device, self.max_pairs = dev, None if max_pairs is None else int(max_pairs)
        weights, biases, lins = self.parse(alexnet_state, lin_state)
        self.convs = [ops.conv2d_pack(w.to(dev)) for w in weights]
        self.biases = [b.to(dev) for b in biases]
        self.lins = [v.to(dev) for v in lins]
        self.shift = torch.tensor(_LPIPS_SHIFT, dtype=torch.float32, device=dev)
        self.scale = torch.tensor(_LPIPS_SCALE, dtype=torch.float32, device=dev)
        self._workspace = None

    @staticmethod
    def parse(alexnet_state, lin_state):
        """The two state dicts -> (five weights, five biases, five lin vectors) as contiguous float32 CPU-or-wherever tensors, checked."""
        if not hasattr(alexnet_state, "keys"):
            raise ValueError("LPIPS: alexnet_state must be a state dict, got %s" % type(alexnet_state).__name__)
        weights, biases, lins = [], [], []
        for idx, cin, cout, K in _ALEX_CONVS:
            for kind, shape, dst in (("weight", (cout, cin, K, K), weights), ("bias", (cout,), biases)):
                names = ("features.%d.%s" % (idx, kind), "%d.%s" % (idx, kind))
                name = next((k for k in names if k in alexnet_state), None)
                if name is None:
                    raise ValueError("LPIPS: alexnet_state has no key %r (nor %r)" % names)
                t = torch.as_tensor(alexnet_state[name])
                if tuple(t.shape) != shape:
                    raise ValueError("LPIPS: alexnet_state[%r] has shape %s, expected %s" % (name, tuple(t.shape), shape))
                dst.append(t.detach().to(torch.float32).contiguous())
        listed = isinstance(lin_state, (list, tuple))
        if listed and len(lin_state) != 5:
            raise ValueError("LPIPS: lin_state as a list must hold five vectors, got %d" % len(lin_state))
        if not listed and not hasattr(lin_state, "keys"):
            raise ValueError("LPIPS: lin_state must be a state dict or a list of five vectors, got %s" % type(lin_state).__name__)
        for l, (_, _, cout, _) in enumerate(_ALEX_CONVS):
            name = "lin_state[%d]" % l if listed else "lin%d.model.1.weight" % l
            if listed:
                t = torch.as_tensor(lin_state[l])
            elif name in lin_state:
                t = torch.as_tensor(lin_state[name])
            else:
                raise ValueError("LPIPS: lin_state has no key %r" % name)
            if tuple(t.shape) not in ((cout,), (1, cout, 1, 1)):
                raise ValueError("LPIPS: %s has shape %s, expected %s or %s" % (name, tuple(t.shape), (1, cout, 1, 1), (cout,)))
            t = t.detach().to(torch.float32).reshape(cout).contiguous()
            if bool((t < 0).any()):
                raise ValueError("LPIPS: %s has a negative weight (%g): not an lpips linear layer" % (name, float(t.min())))
            lins.append(t)
        return weights, biases, lins

    @classmethod
    def from_files(cls, alexnet_path, lin_path, device=None, max_pairs=None):
        """The two checkpoints as the packages ship them (torchvision's alexnet-*.pth, lpips' weights/v0.1/alex.pth)."""
        alex = torch.load(alexnet_path, map_location="cpu", weights_only=True)
        lin = torch.load(lin_path, map_location="cpu", weights_only=True)
        return cls(alex, lin, device=device, max_pairs=max_pairs)

    def pairs_per_call(self, H, W):
        if self.max_pairs is not None:
            return self.max_pairs
        return max(1, self.WORKSPACE_BYTES // (4 * ops.lpips_workspace_floats(1, H, W)))

    def __call__(self, a, b):
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            raise RuntimeError("uc_nerf_amd.utils.evaluation.LPIPS: two device tensors, got %s and %s" % (type(a).__name__, type(b).__name__))
        if a.dim() != 4 or a.shape[1] != 3 or b.shape != a.shape:
            raise ValueError("LPIPS takes two [n,3,H,W] tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
        n, _, H, W = a.shape
        step = self.pairs_per_call(H, W)
        floats = ops.lpips_workspace_floats(min(n, step), H, W)       # (raises below the minimum side)
        if n == 0:
            return ops.lpips_alex(a, b, self.convs, self.biases, self.lins, self.shift, self.scale)
        if self._workspace is None or self._workspace.numel() < floats:
            self._workspace = torch.empty(floats, device=self.device)
        outs = [ops.lpips_alex(a[i:i + step], b[i:i + step], self.convs, self.biases, self.lins, self.shift, self.scale, self._workspace)
                for i in range(0, n, step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)
