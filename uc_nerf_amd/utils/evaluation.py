"""Mirror of the reference's utils/evaluation.py (compute_errors, depth_evaluation, rgb_evaluation) on the device.

Same names, argument orders and return shapes; the arithmetic runs in `ucnerf_depth_eval` / `ucnerf_image_eval` (csrc/metrics.hip).  Inputs may
be numpy arrays (moved to the device) or device tensors (used where they are, as a validation step that keeps `rgb` and `depth` on the device
hands them over); they are not modified -- the reference scales its masked COPIES in place, never its arguments.  Each function reads ONE small
vector back: no cv2, skimage or lpips is needed to finish a validation epoch.

Differences, all deliberate:
  * values are taken as float32 (what the reference's callers pass); a float64 numpy input is rounded first;
  * `pred_masks` at another resolution than the ground truth raises NotImplementedError (the reference resizes them with cv2.resize);
  * LPIPS needs a network and its weights: `rgb_evaluation` returns float('nan') for it unless the caller passes `lpips_fn`;
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
