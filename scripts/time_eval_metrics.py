"""Evaluation metrics of ten 256 x 320 views: the device route (uc_nerf_amd.utils.evaluation from device tensors: depth_evaluation +
rgb_evaluation, one small copy each) against the reference-style route (.cpu().numpy() of the four tensors, then the float32 numpy restatement
of utils/evaluation.py from tests/eval_cases.py -- which leaves skimage's SSIM to a plain-numpy sliding window, so the host figure is a floor
for nothing: it is what this tree can run).  Wall time per validation epoch, median and minimum of --rounds rounds after warm-up; prints one
JSON line.  Under `rocprofv3 --kernel-trace --stats -- python3 scripts/time_eval_metrics.py --rounds 3` the kernel times come from the
profiler's own table (collect no counters in that run)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--host", type=int, default=1, help="0: skip the reference-style route (profiler runs)")
    a = ap.parse_args()
    import eval_cases as E
    from uc_nerf_amd.utils import evaluation as M
    dev = torch.device("cuda:0")
    n, H, W = a.views, 256, 320
    g = torch.Generator().manual_seed(5)
    gt_d = (0.5 + 11.5 * torch.rand(n, H, W, generator=g)).to(dev)
    pred_d = (gt_d.cpu() * (0.6 + 1.3 * torch.rand(n, H, W, generator=g)) * 0.37).to(dev)
    gt_c = torch.rand(n, 3, H, W, generator=g).to(dev)
    pred_c = (gt_c.cpu() + 0.02 * torch.randn(n, 3, H, W, generator=g)).clamp(0, 1).to(dev)
    quiet = io.StringIO()

    def device_route():
        with contextlib.redirect_stdout(quiet):
            d = M.depth_evaluation(gt_d, pred_d)
            r = M.rgb_evaluation(gt_c, pred_c, None)
        return d, r

    def host_route():
        gd, pd, gc, pc = (t.cpu().numpy() for t in (gt_d, pred_d, gt_c, pred_c))
        d = E.depth_reference(gd, pd, dtype=np.float32)["mean"]
        r = E.image_reference(gc, pc, np.float32)
        return d, (r["psnr"].mean(), r["ssim"].mean())

    def timed(fn, rounds):
        ts = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return out, ts

    device_route()
    device_route()
    (d_dev, r_dev), t_dev = timed(device_route, a.rounds)
    res = dict(views=n, H=H, W=W, rounds=a.rounds, device_ms_median=statistics.median(t_dev), device_ms_min=min(t_dev))
    if a.host:
        host_route()
        (d_host, r_host), t_host = timed(host_route, max(3, a.rounds // 4))
        res.update(host_ms_median=statistics.median(t_host), host_ms_min=min(t_host),
                   max_abs_diff_depth=float(np.abs(d_dev - d_host).max()), psnr_diff=abs(float(r_dev[0]) - float(r_host[0])),
                   ssim_diff=abs(float(r_dev[1]) - float(r_host[1])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
