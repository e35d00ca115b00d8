"""Times forward + backward of CostRegNet under train() + grad enabled: training="device" (ops.conv3d_bn_train: the HIP forward kernels, then
csrc/bn.hip's backward pair, csrc/conv3d_bwd.hip's weight gradient and the input gradient on the forward kernel) against training="torch"
(torch's layers and autograd) of the SAME module, in the same process, alternating; and the backward of the device route split by kernel family
and layer.

    python scripts/time_cnn_train.py [--reps 20] [--out FILE]

The stage shapes of scripts/time_mvs_cnns.py at pad 0 (ndepths 48 / 32 / 8, 256 x 320 images).  The loss is a fixed random projection of both
outputs, sum cost R1 + sum prob R2; the input requires a gradient, as the variance volume does in the training step.  Event-timed on the current
stream, warm (3 untimed calls per route first), the median of --reps repetitions with min .. max.  Random weights (the time does not depend on
the values).  The split times every backward launch group of one device-route step with its own event pair, so its sum exceeds the step's time
by the events' own cost.  The numbers in profiles/cnn_train.md are this script's output."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_mvs_cnns import VOLUMES, alternate      # noqa: E402

BACKWARD_ORDER = ("prob", "conv11", "conv9", "conv7", "conv6", "conv5", "conv4", "conv3", "conv2", "conv1", "conv0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mvs_cnn_cases as MC
    from uc_nerf_amd.network.mvs_models import CostRegNet
    from uc_nerf_amd.ops import cnn
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(5)
    res = {"device": torch.cuda.get_device_name(dev), "modules": [], "split": []}
    for i, (title, shape) in enumerate(VOLUMES[:3]):
        module = MC.randomise(CostRegNet(shape[1], 8, training="device"), 20 + i).to(dev).train()
        x = torch.rand(shape, generator=g).to(dev).requires_grad_(True)
        R1, R2 = torch.randn((1, 8) + shape[2:], generator=g).to(dev), torch.randn((1, 1) + shape[2:], generator=g).to(dev)

        def step(name, backward=True):
            def fn():
                module.training_route = name
                x.grad = None
                for p in module.parameters():
                    p.grad = None
                cost, prob = module(x)
                if backward:
                    ((cost * R1).sum() + (prob * R2).sum()).backward()
                return cost, prob
            return fn

        fns = {"device": step("device"), "torch": step("torch"), "device forward": step("device", False), "torch forward": step("torch", False)}
        row = {"case": title, "shape": list(shape), "routes": alternate(fns, args.reps)}
        row["torch_over_device"] = row["routes"]["torch"]["median_us"] / row["routes"]["device"]["median_us"]
        grads = {}
        for name in ("device", "torch"):
            fns[name]()
            grads[name] = [x.grad.clone()] + [p.grad.clone() for p in module.parameters()]
        row["largest_gradient_difference"] = max(float((a - b).abs().max()) for a, b in zip(grads["device"], grads["torch"]))
        row["largest_gradient"] = max(float(b.abs().max()) for b in grads["torch"])
        # which route is nearer the truth: the same module through torch's layers in float64 (its running statistics are not compared)
        try:
            m64 = copy.deepcopy(module).double()
            m64.training_route = "torch"
            x64 = x.detach().double().requires_grad_(True)
            c64, p64 = m64(x64)
            ((c64 * R1.double()).sum() + (p64 * R2.double()).sum()).backward()
            ref = [x64.grad] + [p.grad for p in m64.parameters()]
            for name in ("device", "torch"):
                row[name + "_gradient_error_against_float64"] = max(float((a.double() - b).abs().max()) for a, b in zip(grads[name], ref))
            del m64, x64, c64, p64, ref
        except RuntimeError as e:
            row["float64_reference_failed"] = str(e)[:200]
        res["modules"].append(row)
        print(json.dumps(row), flush=True)

        # ---- the backward of the device route by kernel family and layer
        real = {k: getattr(cnn, k) for k in ("batch_norm_train_bwd", "conv3d_wgrad", "conv3d_dgrad")}
        events = []

        def timed(kind):
            def f(*a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = real[kind](*a, **k)
                e1.record()
                events.append((kind, e0, e1))
                return out
            return f

        per = {}
        try:
            for kind in real:
                setattr(cnn, kind, timed(kind))
            for _ in range(args.reps):
                events.clear()
                fns["device"]()
                torch.cuda.synchronize()
                seen = {}
                for kind, e0, e1 in events:
                    layer = BACKWARD_ORDER[seen.get(kind, 0) + (1 if kind == "batch_norm_train_bwd" else 0)]
                    seen[kind] = seen.get(kind, 0) + 1
                    per.setdefault((layer, kind), []).append(e0.elapsed_time(e1) * 1e3)
        finally:
            for kind, f in real.items():
                setattr(cnn, kind, f)
        split = {"case": title, "layers": {}, "kinds": {}}
        for (layer, kind), us in per.items():
            split["layers"].setdefault(layer, {})[kind] = statistics.median(us)
            split["kinds"][kind] = split["kinds"].get(kind, 0.0) + statistics.median(us)
        res["split"].append(split)
        print(json.dumps(split), flush=True)
        del module, x, R1, R2, grads
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
