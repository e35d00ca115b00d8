"""Times the two routes of utils.build_rays -- the composed one (a ray_gen launch per pixel segment, torch indexing, sample_cascade, ndc_project) and
the one-launch one (ucnerf_build_rays_train) -- at the reference's training shape: 256 x 320 image, patch_num 50, patch_size 6, N_rays 2000,
N_samples 90, a few hundred sparse-depth coordinates, hypothesis volumes of 48 / 32 / 8 planes.  The routes alternate call by call in one process;
every call is bracketed by HIP events and by a host clock (stream drained before the call; the clock is read when the call returns and again
when the stream has drained behind it).  Reported: the median over the calls after warm-up, with the 10th and 90th percentile.
python scripts/time_build_rays.py [--calls 300] [--out FILE.md]"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uc_nerf_amd import ops  # noqa: E402
from uc_nerf_amd.utils import utils as U  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this markdown file")
ap.add_argument("--calls", type=int, default=300, help="timed calls per route (at least 200)")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--coords", type=int, default=300)
a = ap.parse_args()
if a.calls < 200:
    ap.error("--calls must be at least 200")

dev = torch.device("cuda:0")
H, W, V, S, N_RAYS = 256, 320, 4, 90, 2000
args = types.SimpleNamespace(patch_num=50, patch_size=6)
gen = torch.Generator().manual_seed(0)
imgs = torch.rand(1, V, 3, H, W, generator=gen).to(dev)
conf = torch.rand(H, W, generator=gen).clamp(1e-3, 1 - 1e-3).to(dev)
coords = torch.stack([torch.randint(0, H, (a.coords,), generator=gen), torch.randint(0, W, (a.coords,), generator=gen)], -1).float().to(dev)
outputs = {}
for k, (D, div) in enumerate(((48, 4), (32, 2), (8, 1))):
    lo = 1.0 + torch.rand(1, 1, H // div, W // div, generator=gen)
    outputs["stage%d" % (k + 1)] = {"depth_values": torch.cat([lo + 0.5 * i / (D - 1) + 0.3 * k for i in range(D)], 1).to(dev)}
K = torch.tensor([[300., 0, W / 2], [0, 300., H / 2], [0, 0, 1]]).to(dev)
eye = torch.eye(4).to(dev)
pose_ref = {"w2cs": eye.repeat(V, 1, 1), "intrinsics": K.repeat(V, 1, 1), "near_fars": torch.tensor([[1.0, 4.0]] * V).to(dev)}
c2ws, Ks = eye.repeat(V, 1, 1), K.repeat(V, 1, 1)


def call():
    return U.build_rays(args, imgs, conf, None, coords, pose_ref, c2ws, c2ws, Ks, N_RAYS, S, with_depth=True, outputs=outputs)


ROUTES = (("composed", False), ("one launch", True))
times = {name: {"ret": [], "done": [], "gpu": []} for name, _ in ROUTES}
prev = U.set_build_rays_fused(False)
torch.manual_seed(0)
np.random.seed(0)
out_bytes = 0
for it in range(a.warmup + a.calls):
    for name, on in ROUTES:
        U.set_build_rays_fused(on)
        e0, e1 = ops.Event(), ops.Event()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = call()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= a.warmup:
            t = times[name]
            t["ret"].append((t1 - t0) * 1e6); t["done"].append((t2 - t0) * 1e6); t["gpu"].append(e0.elapsed_ms(e1) * 1e3)
        if on and not out_bytes:
            pts, rays_d, colors, ndc, z, _, _, _, pix = out
            out_bytes = sum(t.numel() * t.element_size() for t in (pts, rays_d, colors, z, pix, *ndc.values())) + 12
U.set_build_rays_fused(prev)


def row(v):
    q = statistics.quantiles(v, n=10)
    return "%.0f (%.0f .. %.0f)" % (statistics.median(v), q[0], q[-1])


R = pix.shape[1]
lines = ["`utils.build_rays` at %d x %d, patch_num %d, patch_size %d, N_rays %d, N_samples %d, %d sparse-depth coordinates (%d rays); %s; "
         "%d calls per route after %d warm-up calls, routes alternating; microseconds per call, median (10th .. 90th percentile)."
         % (H, W, args.patch_num, args.patch_size, N_RAYS, S, a.coords, R, torch.cuda.get_device_name(0), a.calls, a.warmup), "",
         "| route | host wall time until the call returns | host wall time until the stream has drained | GPU time (HIP events around the call) |",
         "|---|---|---|---|"]
for name, _ in ROUTES:
    t = times[name]
    lines.append("| %s | %s | %s | %s |" % (name, row(t["ret"]), row(t["done"]), row(t["gpu"])))
med = {name: statistics.median(times[name]["done"]) for name, _ in ROUTES}
lines += ["", "Composed / one launch, wall time until drained: %.2f.  The one launch writes %.2f MB (%.1f us at 6.3 TB/s)."
          % (med["composed"] / med["one launch"], out_bytes / 1e6, out_bytes / 6.3e12 * 1e6)]
text = "\n".join(lines)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
