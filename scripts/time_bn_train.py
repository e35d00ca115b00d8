"""Times CascadeMVSNet's CNNs under train() + no_grad, the way the reference's validation_step runs them: batch_stats="device" (the convolution
kernels with raw weights, then csrc/bn.hip's two launches per batch-normed layer) against batch_stats="torch" (torch's layers in training mode) of
the SAME module, in the same process, alternating; and the two batch-norm launches of every layer on their own with the bytes they move per second.

    python scripts/time_bn_train.py [--reps 20] [--out FILE]

CostRegNet at the stage shapes of scripts/time_mvs_cnns.py (ndepths 48 / 32 / 8, 256 x 320 images, stage 3 with pad 0 and pad 24), FeatureNet on
[1,3,256,320].  Event-timed on the current stream, warm (3 untimed calls per route first), the median of --reps repetitions.  Random weights (the
time does not depend on the values).  Every forward moves the running statistics; neither route's time depends on them.  Bytes of a layer: stats
reads |y|, apply reads |y| (+ |skip|) and writes |y|.  The numbers in profiles/bn_train.md are this script's output."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_mvs_cnns import IMAGE, VOLUMES, alternate, reg_layers      # noqa: E402


def bn_layers(cin, c, D, H, W):
    """(name, channels, output dims, has skip) of CostRegNet's ten batch-normed layers."""
    rows = []
    for name, _, co, dims, stride, transposed, _ in reg_layers(cin, c, D, H, W):
        if name == "prob":
            continue
        out = tuple(2 * s for s in dims) if transposed else tuple(s // stride for s in dims)
        rows.append((name, co, out, transposed))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mvs_cnn_cases as MC
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd import ops
    from uc_nerf_amd.network.mvs_models import CostRegNet, FeatureNet
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(3)
    res = {"device": torch.cuda.get_device_name(dev), "modules": [], "layers": []}

    def route(module, x, name):
        def fn():
            module.batch_stats = name
            with torch.no_grad():
                return module(x)
        return fn

    cases = [(title, CostRegNet(shape[1], 8), shape) for title, shape in VOLUMES] + [("feature", FeatureNet(8), IMAGE)]
    for i, (title, module, shape) in enumerate(cases):
        module = MC.randomise(module, 10 + i).to(dev).train()
        x = torch.rand(shape, generator=g).to(dev)
        fns = {name: route(module, x, name) for name in ("device", "torch")}
        row = {"case": title, "shape": list(shape), "routes": alternate(fns, args.reps)}
        a, b = fns["device"](), fns["torch"]()
        a, b = (list(t.values()) if isinstance(t, dict) else list(t) for t in (a, b))
        row["largest_difference"] = max(float((u - v).abs().max()) for u, v in zip(a, b))
        row["largest_value"] = max(float(v.abs().max()) for v in b)
        res["modules"].append(row)
        print(json.dumps(row), flush=True)
        del module, x
        torch.cuda.empty_cache()

    stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
    for title, shape in VOLUMES:
        for name, C, dims, has_skip in bn_layers(shape[1], 8, *shape[2:]):
            y = torch.randn((1, C) + dims, generator=g).to(dev)
            skip = torch.randn((1, C) + dims, generator=g).to(dev) if has_skip else None
            S = y[0, 0].numel()
            P = L.lib().ucnerf_bn_partials(1, S)
            ws = torch.empty((C, P, 3), dtype=torch.float64, device=dev)
            vec = {k: torch.ones(C, device=dev) for k in ("weight", "bias", "saved_mean", "saved_var", "running_mean", "running_var")}
            nbt = torch.zeros((), dtype=torch.int64, device=dev)
            s = L.BnStatsParams()
            s.n, s.C, s.S, s.workspace_triples, s.y, s.workspace = 1, C, S, C * P, y.data_ptr(), ws.data_ptr()
            a = L.BnApplyParams()
            a.n, a.C, a.S, a.workspace_triples, a.eps, a.momentum, a.relu = 1, C, S, C * P, 1e-5, 0.1, 1
            a.y, a.workspace, a.out, a.skip = y.data_ptr(), ws.data_ptr(), y.data_ptr(), 0 if skip is None else skip.data_ptr()
            for k, t in vec.items():
                setattr(a, k, t.data_ptr())
            a.num_batches_tracked = nbt.data_ptr()
            # (apply in place on y, as the modules run it: the values drift towards the normalised ones, the time does not depend on them)
            t = alternate({"stats": lambda: L.call("ucnerf_bn_stats", s, stream()), "apply": lambda: L.call("ucnerf_bn_apply", a, stream()),
                           "both": lambda: ops.batch_norm_train(y, vec["weight"], vec["bias"], vec["running_mean"], vec["running_var"], nbt, skip=skip, out=y)},
                          args.reps)
            nbytes = 4 * y.numel()
            row = {"case": title, "layer": name, "C": C, "out": list(dims), "partials": P, "skip": has_skip, "mbytes": nbytes / 1e6,
                   "stats_us": t["stats"]["median_us"], "stats_min_us": t["stats"]["min_us"], "apply_us": t["apply"]["median_us"],
                   "apply_min_us": t["apply"]["min_us"], "wrapper_us": t["both"]["median_us"],
                   "stats_gbps": nbytes / (t["stats"]["median_us"] * 1e-6) / 1e9,
                   "apply_gbps": (3 if has_skip else 2) * nbytes / (t["apply"]["median_us"] * 1e-6) / 1e9}
            res["layers"].append(row)
            print(json.dumps(row), flush=True)
            del y, skip, ws
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
