"""Generates tests/golden/g20_depth_eval.npz: the reference's utils/evaluation.py depth_evaluation on three seeded 12 x 16 depth maps (one with a
band of zeros, one all zeros: skipped by the reference), and lines 82-83 of rgb_evaluation restated (rgb_evaluation itself needs lpips).

Run where the reference tree is present:  python tests/golden/make_golden_eval.py
utils/evaluation.py is loaded by path with inert stand-ins for cv2, lpips and skimage (none of them is touched by depth_evaluation without
masks).  Data only: inputs, the reference's return value, and what it computed on the way (the two medians through a recording wrapper around
np.median, the arrays handed to compute_errors through a wrapper around it).
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF  # noqa: E402  (where the reference tree lies; UCNERF_REFERENCE overrides it)


def load_reference():
    for name in ("cv2", "lpips", "skimage"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    spec = importlib.util.spec_from_file_location("ref_evaluation", os.path.join(REF, "utils", "evaluation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    rng = np.random.default_rng(2020)
    n, H, W = 3, 12, 16
    gt = rng.uniform(0.8, 9.0, (n, H, W)).astype(np.float32)
    pred = (gt * rng.uniform(0.55, 1.8, (n, H, W)) * 0.41).astype(np.float32)
    gt[0, 4:6] = 0.0                                  # a band without ground truth
    gt[1] = 0.0                                       # an image without any: the reference's `continue`
    pred[0, 0, :3] = 1e-7                             # the clamps bite
    pred[2, 11, 13:] = 1e4
    gt_in, pred_in = gt.copy(), pred.copy()

    medians, handed = [], []
    real_median, real_errors = np.median, ref.compute_errors

    def median(a, *args, **kw):
        medians.append(real_median(a, *args, **kw))
        return medians[-1]

    def compute_errors(g, p):
        handed.append((g.copy(), p.copy()))
        return real_errors(g, p)

    ref.np.median, ref.compute_errors = median, compute_errors
    try:
        with contextlib.redirect_stdout(io.StringIO()) as printed:
            mean_errors = ref.depth_evaluation(gt, pred)
    finally:
        ref.np.median, ref.compute_errors = real_median, real_errors
    assert mean_errors.dtype == np.float64 and mean_errors.shape == (7,) and len(medians) == 2 and len(handed) == 2
    assert np.array_equal(gt, gt_in) and np.array_equal(pred, pred_in)      # the reference scales masked copies, not its arguments
    assert medians[0].dtype == np.float32 and handed[0][1].dtype == np.float32
    errors = np.array([real_errors(g, p) for g, p in handed])
    counts = np.array([[g.size] + [int((np.maximum(g / p, p / g) < t).sum()) for t in (1.25, 1.25 ** 2, 1.25 ** 3)] for g, p in handed])
    out = dict(gt_depths=gt_in, pred_depths=pred_in, mean_errors=mean_errors, median_gt=medians[0], median_pred=medians[1],
               ratio=medians[0] / medians[1], kept=np.array([0, 2]), errors=errors.astype(np.float64), counts=counts,
               printed=np.array(printed.getvalue()))

    # rgb_evaluation lines 82-83 restated on a seeded pair (the function itself constructs lpips.LPIPS)
    gts = rng.random((2, 3, 9, 11)).astype(np.float32)
    predicts = np.clip(gts + rng.normal(0, 0.05, gts.shape), 0, 1).astype(np.float32)
    mse = ((gts - predicts) ** 2).mean(-1).mean(-1).mean(-1)
    psnr = (-10 * np.log10(mse)).mean()
    out.update(gts=gts, predicts=predicts, mse=mse, psnr=psnr)

    path = os.path.join(HERE, "g20_depth_eval.npz")
    np.savez_compressed(path, **out)
    print("g20_depth_eval %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(out)))


if __name__ == "__main__":
    main()
