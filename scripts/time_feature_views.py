"""Times FeatureNet over the V views of one sample: the device loop (one call per view, as CascadeMVSNet's feature_views="loop" runs it), the device
batched pass (FeatureNet.forward_views: one pass over [V,3,H,W], every batch-norm keeping its statistics per view through the group dimension of csrc/bn.hip) and
torch's loop (torch's layers, one call per view), of the SAME module, in the same process, alternating.

    python scripts/time_feature_views.py [--reps 20] [--out profiles/feature_views.md]

FeatureNet(8) at 256 x 320 with V = 3 and V = 6.  Two things are timed: the forward under train() + no_grad (batch_stats="device" against "torch")
and forward + backward under grad (training="device" against "torch"; the loss is a fixed random projection of the outputs, the image requires no
gradient, as in the training step).  Event-timed on the current stream, warm (3 untimed calls per route first), the median of --reps repetitions
with min .. max.  Random weights (the time does not depend on the values).  Launches are counted at the library's one call path (_lib.call) in
an untimed step of their own.  The measured part of profiles/feature_views.md is this script's output."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_mvs_cnns import alternate      # noqa: E402

H, W = 256, 320
VIEWS = (3, 6)
STAGES = (("stage1", 32, 4), ("stage2", 16, 2), ("stage3", 8, 1))
ROUTES = ("device loop", "device batched", "torch loop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mvs_cnn_cases as MC
    from uc_nerf_amd import _lib
    from uc_nerf_amd.network.mvs_models import FeatureNet
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(5)
    module = MC.randomise(FeatureNet(8, batch_stats="device", training="device"), 31).to(dev).train()
    res = {"device": torch.cuda.get_device_name(dev), "size": [H, W], "views": {}}
    for V in VIEWS:
        imgs = torch.rand((1, V, 3, H, W), generator=g).to(dev)
        R = {k: torch.randn((V, c, H // s, W // s), generator=g).to(dev) for k, c, s in STAGES}

        def step(route, backward):
            def fn():
                device, batched = route != "torch loop", route == "device batched"
                module.batch_stats, module.training_route = ("device", "device") if device else ("torch", "torch")
                for p in module.parameters():
                    p.grad = None
                with torch.set_grad_enabled(backward):
                    if batched:
                        outs = module.forward_views(imgs)
                    else:
                        per_view = [module(imgs[:, i]) for i in range(V)]
                        # (the loop's consumer stacks the views once more; the time of that copy is part of the loop, as in DepthNet)
                        outs = {k: torch.cat([o[k] for o in per_view]) for k, _, _ in STAGES}
                    if backward:
                        sum((outs[k] * R[k]).sum() for k in R).backward()
                return outs
            return fn

        fns = {"%s, %s" % (route, what): step(route, backward) for backward, what in ((False, "forward under no_grad"), (True, "forward + backward"))
               for route in ROUTES}
        entry = {"routes": alternate(fns, args.reps), "launches": {}}
        real, counted = _lib.call, []
        _lib.call = lambda name, params, stream: counted.append(name) or real(name, params, stream)
        try:
            for name, fn in fns.items():
                counted.clear()
                fn()
                torch.cuda.synchronize()
                entry["launches"][name] = len(counted)
        finally:
            _lib.call = real
        # the batched pass computes the loop's outputs
        module.batch_stats, module.training_route = "device", "device"
        with torch.no_grad():
            state = {k: v.clone() for k, v in module.state_dict().items()}
            a = fns["device batched, forward under no_grad"]()
            after = {k: v.clone() for k, v in module.state_dict().items()}
            module.load_state_dict(state)
            b = fns["device loop, forward under no_grad"]()
        entry["outputs_and_buffers_bit_equal"] = bool(all(torch.equal(a[k], b[k]) for k in a)
                                                      and all(torch.equal(v, module.state_dict()[k]) for k, v in after.items()))
        res["views"][str(V)] = entry
    print(json.dumps(res), flush=True)
    if args.out:
        fmt = lambda v: "%.0f (%.0f .. %.0f)" % (v["median_us"], v["min_us"], v["max_us"])     # noqa: E731
        lines = ["## Measured (scripts/time_feature_views.py, %s, FeatureNet(8) at %d x %d, %d repetitions, microseconds: median (min .. max))"
                 % (res["device"], H, W, args.reps), ""]
        for V in VIEWS:
            e = res["views"][str(V)]
            lines += ["### V = %d" % V, "", "| | " + " | ".join(ROUTES) + " |", "|---|" + "---|" * len(ROUTES)]
            for what in ("forward under no_grad", "forward + backward"):
                lines.append("| %s | " % what + " | ".join(fmt(e["routes"]["%s, %s" % (r, what)]) for r in ROUTES) + " |")
                lines.append("| library launches, %s | " % what + " | ".join(str(e["launches"]["%s, %s" % (r, what)]) for r in ROUTES) + " |")
            lines += ["", "Outputs and batch-norm buffers of the batched forward equal the loop's bit for bit: %s." % ("yes" if e["outputs_and_buffers_bit_equal"] else "NO"), ""]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
