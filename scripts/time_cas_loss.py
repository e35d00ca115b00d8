"""Times forward + backward of the cascade depth loss at the reference's stage sizes of a 256 x 320 image (64 x 80, 128 x 160, 256 x 320; about
30 % of the pixels valid, G15's generator): the device route (utils.loss.cas_mvsnet_loss_device: one launch each way, nothing read back) against
the torch expression (utils.loss.cas_mvsnet_loss on the same device tensors: boolean-mask indexing, which reads the element counts back).
HIP events after warm-up; the two are timed alternately, several rounds each, the median round is reported.  The device route is also timed as
one graph replay (train_step.GraphedStep) -- its GPU time without the host's enqueue -- which the torch expression cannot be (capture refuses its read-back).  Host
synchronisations per call are counted with torch's sync debug mode.   python scripts/time_cas_loss.py [--out FILE.md]"""
import argparse
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uc_nerf_amd import ops  # noqa: E402
from uc_nerf_amd.train_step import GraphedStep  # noqa: E402
from uc_nerf_amd.utils import loss as UL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this markdown file")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--valid", type=float, default=0.3)
args = ap.parse_args()

dev = torch.device("cuda:0")
gen = torch.Generator().manual_seed(15)
keys = ("stage1", "stage2", "stage3")
inputs, gt, w = {}, {}, {}
for k, (h, ww) in zip(keys, ((64, 80), (128, 160), (256, 320))):
    inputs[k] = {"depth": (1.0 + 3.0 * torch.rand(1, h, ww, generator=gen)).to(dev).requires_grad_(True)}
    m = torch.rand(1, h, ww, generator=gen) < args.valid
    gt[k] = torch.where(m, 1.0 + 3.0 * torch.rand(1, h, ww, generator=gen), torch.zeros(1, h, ww)).to(dev)
    w[k] = torch.where(m, 0.1 + 1.9 * torch.rand(1, h, ww, generator=gen), torch.zeros(1, h, ww)).to(dev)
# the captured route has estimates of its own, first used on the capture's stream: train_step.GraphedStep asks for that (gradient accumulators made
# on another stream would have autograd bridge two streams inside the capture)
graph_inputs = {k: {"depth": inputs[k]["depth"].detach().clone().requires_grad_(True)} for k in keys}


def run(fn, ins):
    for k in keys:
        ins[k]["depth"].grad = None
    total, _ = fn(ins, gt, w)
    (total * 0.05).backward()
    return total


graph = GraphedStep(lambda: run(UL.cas_mvsnet_loss_device, graph_inputs), warmup=3)
run_device = lambda: run(UL.cas_mvsnet_loss_device, inputs)      # noqa: E731
run_torch = lambda: run(UL.cas_mvsnet_loss, inputs)              # noqa: E731


def timed(fn, iters):
    a, b = ops.Event(), ops.Event()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_ms(b) / iters * 1e3                  # us per call


def syncs(fn):
    """Host synchronisations of one call, as torch's sync debug mode reports them (None where the build does not offer it)."""
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:
        return None
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(x.message).lower() for x in seen)
    finally:
        torch.cuda.set_sync_debug_mode("default")


for _ in range(10):
    a, b = run_device(), run_torch()
torch.cuda.synchronize()
rel = abs(a.item() - b.item()) / abs(b.item())
n_sync = {"device": syncs(run_device), "torch": syncs(run_torch)}

t_dev, t_torch, t_graph = [], [], []
for _ in range(args.rounds):
    t_dev.append(timed(run_device, args.iters))
    t_torch.append(timed(run_torch, args.iters))
    t_graph.append(timed(graph.replay, args.iters))
assert ops.loss_status() == 0
fmt = lambda t: "%.1f (%.1f .. %.1f)" % (statistics.median(t), min(t), max(t))      # noqa: E731
n_valid = [int((gt[k] > 0).sum()) for k in keys]
lines = ["Forward + backward of the cascade depth loss, stages 64 x 80, 128 x 160, 256 x 320 (valid: %s of %s), us per call: median (min .. max) of %d rounds"
         " of %d calls." % (n_valid, [gt[k].numel() for k in keys], args.rounds, args.iters), "",
         "| route | us per call, eager | us per call, one graph replay | launches | host synchronisations per call |",
         "|---|---|---|---|---|",
         "| device: cas_mvsnet_loss_device | %s | %s | 1 forward + 1 backward (+ the scaling by 0.05) | %s |" % (fmt(t_dev), fmt(t_graph), n_sync["device"]),
         "| torch: cas_mvsnet_loss on the same device tensors | %s | cannot be captured | the op chain of three stages | %s |" % (fmt(t_torch), n_sync["torch"]),
         "", "Relative difference of the two totals: %.2e." % rel]
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
