"""Times one training step through the hierarchical renderer -- CoarseFineRenderer.render_train forward, a loss on the coarse and fine colours and
the fine depth, backward to the flat parameters and the gather sources -- at 4096 rays x 64 + 128 and at 512 rays x 64 + 128 (the benchmark's
shape and a data-parallel shard of it), next to the inference render() of the same renderer in the same run.  Exact-f32 precision, the synthetic
scene at the benchmark's size.  Every call is bracketed by HIP events (stream drained before it); reported: the median over the calls after
warm-up, with the 10th and 90th percentile, in milliseconds.
python scripts/time_render_train.py [--calls 30] [--warmup 5] [--out FILE.md]"""
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
ap.add_argument("--out", default=None, help="also write the table to this markdown file")
ap.add_argument("--calls", type=int, default=30, help="timed calls per shape and route")
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()

dev = torch.device("cuda:0")
NC, NF = 64, 128
scene = scene_to(make_scene(seed=0), dev)
for t in scene["vols"] + [scene["img_feat"], scene["confidence"]]:
    t.requires_grad_(True)
leaves = scene["vols"] + [scene["img_feat"], scene["confidence"]]
flat = flat_params_of(init_ucnerf_state_dict(seed=0, sigma_scale=0.05, sigma_bias=0.05)).to(dev).requires_grad_(True)
r = CoarseFineRenderer(scene, flat.detach(), NC, NF, precision="f32")


def timed(fn):
    e0, e1 = ops.Event(), ops.Event()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_ms(e1)


def row(v):
    q = statistics.quantiles(v, n=10)
    return "%.2f (%.2f .. %.2f)" % (statistics.median(v), q[0], q[-1])


lines = ["`CoarseFineRenderer` at %d + %d samples per ray, precision \"f32\", synthetic scene %d x %d with %d source views; %s; %d calls per entry "
         "after %d warm-up calls; milliseconds per call between HIP events, median (10th .. 90th percentile)."
         % (NC, NF, scene["H"], scene["W"], scene["w2cs"].shape[0] - 1, torch.cuda.get_device_name(0), a.calls, a.warmup), "",
         "| rays | render() (inference, channel-last gather) | render_train forward | render_train forward + loss + backward |", "|---|---|---|---|"]
for n in (4096, 512):
    xs, ys = random_pixels(n, scene["H"], scene["W"], seed=n)
    xs, ys = xs.to(dev), ys.to(dev)
    g = torch.Generator().manual_seed(n)
    noise, u, target = torch.rand(n, NC, generator=g).to(dev), torch.rand(n, NF, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
    kw = dict(perturb=1.0, noise=noise, u=u)

    def infer():
        with torch.no_grad():
            r.render(xs, ys, repack=False, **kw)

    def forward():
        return r.render_train(xs, ys, flat, **kw)

    def step():
        flat.grad = None
        for t in leaves:
            t.grad = None
        out = forward()
        loss = ((out["coarse"]["rgb"] - target) ** 2).mean() + ((out["rgb"] - target) ** 2).mean() + 0.1 * out["depth"].mean()
        loss.backward()

    r.pass_.repack_sources()
    res = {}
    for name, fn in (("infer", infer), ("forward", forward), ("step", step)):
        ts = [timed(fn) for _ in range(a.warmup + a.calls)][a.warmup:]
        res[name] = row(ts)
    lines.append("| %d | %s | %s | %s |" % (n, res["infer"], res["forward"], res["step"]))
text = "\n".join(lines)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
