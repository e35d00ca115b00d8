"""Times the link between two cascade stages at the real shapes (256 x 320 image; D = 48 / 32 / 8 at scales 4 / 2 / 1; pad 0 -- the benchmark's --
and pad 2): the reference's chain of torch ops (network/mvs_models.py:536-573, 720-746, the replicate pad of :598), restated with torch ops on
the device, against ucnerf_depth_hypotheses.  HIP events after warm-up; the two are timed alternately, several rounds each, the median round is
reported (launch-bound work: the figure is the per-call cost in a back-to-back stream, host enqueue included where it is the longer).
Also prints the largest difference between the two outputs.   python scripts/time_cascade_glue.py [--out FILE.md]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uc_nerf_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this markdown file")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()

dev = torch.device("cuda:0")
H, W = 256, 320
NEAR, FAR = 1.0, 4.0
near_far = torch.tensor([NEAR, FAR], device=dev)
STAGES = [(1, 48, 4, 4), (2, 32, 2, 2), (3, 8, 1, 1)]            # stage, D, scale, interval ratio


def chain(stage, D, scale, ratio, prev, pad):
    """What CascadeMVSNet.forward + DepthNet do per stage, op for op (near / far stay device values, as in the reference)."""
    near, far = near_far[0], near_far[1]
    interval = (far - near) / 48
    if prev is None:
        t = torch.linspace(0., 1., steps=48, device=dev)
        row = (near * (1. - t) + far * t).unsqueeze(0)
        step = (row[:, -1] - row[:, 0]) / (D - 1)
        samples = row[:, 0].unsqueeze(1) + torch.arange(0, D, device=dev, dtype=torch.float32).reshape(1, -1) * step.unsqueeze(1)
        samples = samples.unsqueeze(-1).unsqueeze(-1).repeat(1, 1, H, W)
    else:
        cur = F.interpolate(prev.unsqueeze(1), [H, W], mode="bilinear", align_corners=False).squeeze(1)
        lo = (cur - D / 2 * (ratio * interval)).clamp(min=near)
        hi = (cur + D / 2 * (ratio * interval)).clamp(max=far)
        step = (hi - lo) / (D - 1)
        samples = lo.unsqueeze(1) + torch.arange(0, D, device=dev, dtype=torch.float32).reshape(1, -1, 1, 1) * step.unsqueeze(1)
    out = F.interpolate(samples.unsqueeze(1), [D, H // scale, W // scale], mode="trilinear", align_corners=False).squeeze(1)
    if pad > 0:
        out = F.pad(out, (pad, pad, pad, pad), "replicate")
    return out


def kernel(stage, D, scale, ratio, prev, pad):
    if prev is None:
        return ops.depth_hypotheses(D, (H // scale, W // scale), row=near_far, pad=pad)
    return ops.depth_hypotheses(D, (H // scale, W // scale), cur_depth=prev[0], near_far=near_far, k=ratio / 48.0, full_hw=(H, W), pad=pad)


def timed(fn, iters):
    a, b = ops.Event(), ops.Event()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_ms(b) / iters * 1e3                                    # us per call


lines = ["| stage | D | output | pad | torch op chain (us) | ucnerf_depth_hypotheses (us) | chain / kernel | output MB | max abs difference |",
         "|---|---|---|---|---|---|---|---|---|"]
sums = {}
gen = torch.Generator().manual_seed(0)
for pad in (0, 2):
    for stage, D, scale, ratio in STAGES:
        stage_pad = pad if stage == 3 else 0                                  # mvs_models.py:735-740
        if pad and not stage_pad:
            continue                                                          # (stages 1 and 2 do not depend on pad)
        prev = None if stage == 1 else (NEAR + (FAR - NEAR) * torch.rand(1, H // (2 * scale), W // (2 * scale), generator=gen)).to(dev)
        run_chain = lambda: chain(stage, D, scale, ratio, prev, stage_pad)    # noqa: E731
        run_kernel = lambda: kernel(stage, D, scale, ratio, prev, stage_pad)  # noqa: E731
        for _ in range(10):
            want, got = run_chain(), run_kernel()
        torch.cuda.synchronize()
        diff = (got - want[0]).abs().max().item()
        t_chain, t_kernel = [], []
        for _ in range(args.rounds):
            t_chain.append(timed(run_chain, args.iters))
            t_kernel.append(timed(run_kernel, args.iters))
        tc, tk = statistics.median(t_chain), statistics.median(t_kernel)
        sums.setdefault(pad, [0.0, 0.0])
        lines.append("| %d | %d | %d x %d | %d | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.1f | %.2f | %.2e (%.2f * 2^-23 * far) |" % (
            stage, D, got.shape[1], got.shape[2], stage_pad, tc, min(t_chain), max(t_chain), tk, min(t_kernel), max(t_kernel), tc / tk,
            got.numel() * 4 / 1e6, diff, diff / (2.0 ** -23 * FAR)))
        for p in ((0, 2) if stage != 3 else (pad,)):
            sums.setdefault(p, [0.0, 0.0])
            sums[p][0] += tc
            sums[p][1] += tk
for pad, (tc, tk) in sorted(sums.items()):
    lines.append("| per step, pad %d | | | | %.1f | %.1f | %.1f | | |" % (pad, tc, tk, tc / tk))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
