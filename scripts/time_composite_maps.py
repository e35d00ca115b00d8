"""Times the gradient fold of the compositing's extra maps: ucnerf_composite_fold_grads alone at 4096 x 192 and at 250 x 90 (all three extra
gradients and all three upstream ones given, g_u written: its largest traffic), and one training step through CoarseFineRenderer.render_train
at the shapes of scripts/time_render_train.py -- without the `maps` argument, with maps=False, with maps=True under the same loss (the fold is
skipped: no gradient arrives on var / disp) and with maps=True under that loss plus a term on var and disp of both passes (two fold launches).
The routes are timed in turn, round after round, so that drift of the box lands on all of them.  Exact-f32 precision, the synthetic scene at the
benchmark's size.  Every call is bracketed by HIP events (stream drained before it); reported: the median over the calls after warm-up with
the 10th and 90th percentile; the fold in microseconds per launch (events around 50 back-to-back launches), steps in milliseconds.
python scripts/time_composite_maps.py [--calls 30] [--warmup 5] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uc_nerf_amd import ops  # noqa: E402
from uc_nerf_amd.pipeline import CoarseFineRenderer, flat_params_of  # noqa: E402
from uc_nerf_amd.synthetic import init_ucnerf_state_dict, make_scene, random_pixels, scene_to  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the tables to this markdown file")
ap.add_argument("--calls", type=int, default=30, help="timed calls per shape and route")
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()

dev = torch.device("cuda:0")
NC, NF, BURST = 64, 128, 50


def timed(fn):
    e0, e1 = ops.Event(), ops.Event()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_ms(e1)


def row(v, unit=1.0):
    q = statistics.quantiles(v, n=10)
    return "%.2f (%.2f .. %.2f)" % (statistics.median(v) * unit, q[0] * unit, q[-1] * unit)


lines = ["%s; %d calls per entry after %d warm-up calls, median (10th .. 90th percentile)." % (torch.cuda.get_device_name(0), a.calls, a.warmup), "",
         "`ucnerf_composite_fold_grads`, microseconds per launch (%d launches between two HIP events), and the bytes it moves:" % BURST, "",
         "| rays x samples | us per launch | MB read + written |", "|---|---|---|"]
for n, S in ((4096, 192), (250, 90)):
    g = torch.Generator().manual_seed(S)
    w, u, gw = (torch.rand(n, S, generator=g).to(dev) for _ in range(3))
    depth, acc, gv, gd, gwu, gdep, gacc = (torch.rand(n, generator=g).to(dev) + 0.5 for _ in range(7))
    out = (torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, S, device=dev), torch.empty(n, S, device=dev))

    def burst():
        for _ in range(BURST):
            ops.composite_fold_grads(w, depth, acc, u, gv, gd, gwu, gdep, gacc, gw, out=out)

    ts = [timed(burst) / BURST for _ in range(a.warmup + a.calls)][a.warmup:]
    lines.append("| %d x %d | %s | %.2f |" % (n, S, row(ts, 1e3), (5 * n * S + 9 * n) * 4 / 1e6))

scene = scene_to(make_scene(seed=0), dev)
leaves = scene["vols"] + [scene["img_feat"], scene["confidence"]]
for t in leaves:
    t.requires_grad_(True)
flat = flat_params_of(init_ucnerf_state_dict(seed=0, sigma_scale=0.05, sigma_bias=0.05)).to(dev).requires_grad_(True)
r = CoarseFineRenderer(scene, flat.detach(), NC, NF, precision="f32")
lines += ["", "`CoarseFineRenderer.render_train` forward + loss + backward at %d + %d samples per ray, precision \"f32\", synthetic scene %d x %d with %d "
          "source views; milliseconds per step:" % (NC, NF, scene["H"], scene["W"], scene["w2cs"].shape[0] - 1), "",
          "| rays | no `maps` argument | maps=False | maps=True, same loss | maps=True, loss + var and disp terms |", "|---|---|---|---|---|"]
for n in (4096, 512):
    xs, ys = random_pixels(n, scene["H"], scene["W"], seed=n)
    xs, ys = xs.to(dev), ys.to(dev)
    g = torch.Generator().manual_seed(n)
    noise, u, target = torch.rand(n, NC, generator=g).to(dev), torch.rand(n, NF, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
    kw = dict(perturb=1.0, noise=noise, u=u)

    def step(extra, reg):
        flat.grad = None
        for t in leaves:
            t.grad = None
        out = r.render_train(xs, ys, flat, **kw, **extra)
        loss = ((out["coarse"]["rgb"] - target) ** 2).mean() + ((out["rgb"] - target) ** 2).mean() + 0.1 * out["depth"].mean()
        if reg:
            loss = loss + out["var"].mean() + out["coarse"]["var"].mean() + 0.01 * out["disp"].mean() + 0.01 * out["coarse"]["disp"].mean()
        loss.backward()

    routes = (("default", {}, False), ("off", dict(maps=False), False), ("on", dict(maps=True), False), ("reg", dict(maps=True), True))
    ts = {name: [] for name, _, _ in routes}
    for _ in range(a.warmup + a.calls):
        for name, extra, reg in routes:
            ts[name].append(timed(lambda: step(extra, reg)))
    lines.append("| %d | %s |" % (n, " | ".join(row(ts[name][a.warmup:]) for name, _, _ in routes)))
text = "\n".join(lines)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
