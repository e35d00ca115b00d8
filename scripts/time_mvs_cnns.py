"""Times CascadeMVSNet's CNNs under eval() + no_grad: the device route (csrc/conv3d.hip / conv2d with the batch-norms folded in) against the
torch route of the SAME module, in the same process, alternating; and every conv3d layer of the device route on its own with its useful FLOPs
over the fp32-MFMA peak.

    python scripts/time_mvs_cnns.py [--reps 20] [--out FILE]
    python scripts/time_mvs_cnns.py --only device|torch --reps 5      # a run for rocprofv3 --kernel-trace --stats: one route, nothing else

CostRegNet at the three stage shapes of the reference's configuration (ndepths 48 / 32 / 8, the 256 x 320 images of data/scared.py and
data/hamlyn.py, feature channels 32 / 16 / 8): stage 3 is [1,8,8,256,320] with opt.py's default pad = 0 and [1,8,8,304,368] with pad = 24.
FeatureNet on [1,3,256,320].  Event-timed on the current stream, warm (3 untimed calls per route first), the median of --reps repetitions.
Random weights (the time does not depend on the values).  The numbers in profiles/mvs_cnns.md are this script's output."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

PEAK_TFLOPS = 157.3      # fp32 MFMA, MI355X spec
VOLUMES = (("stage1", (1, 32, 48, 64, 80)), ("stage2", (1, 16, 32, 128, 160)), ("stage3 pad 0", (1, 8, 8, 256, 320)), ("stage3 pad 24", (1, 8, 8, 304, 368)))
IMAGE = (1, 3, 256, 320)


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(us):
    us = sorted(us)
    return {"median_us": statistics.median(us), "min_us": us[0], "max_us": us[-1], "reps": len(us)}


def alternate(fns, reps, warm=3):
    """{name: summary} of several functions timed in turn, so that a drift of the machine falls on all of them alike."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            us[k].append(event_us(fn))
    return {k: summary(v) for k, v in us.items()}


def reg_layers(cin, c, D, H, W):
    """(name, cin, cout, input dims, stride, transposed, useful MACs) of CostRegNet's eleven convolutions."""
    rows, d = [], (D, H, W)
    half = lambda t: tuple(s // 2 for s in t)            # noqa: E731
    vox = lambda t: t[0] * t[1] * t[2]                   # noqa: E731
    plan = (("conv0", cin, c, 0, 1), ("conv1", c, 2 * c, 0, 2), ("conv2", 2 * c, 2 * c, 1, 1), ("conv3", 2 * c, 4 * c, 1, 2), ("conv4", 4 * c, 4 * c, 2, 1),
            ("conv5", 4 * c, 8 * c, 2, 2), ("conv6", 8 * c, 8 * c, 3, 1))
    levels = [d, half(d), half(half(d)), half(half(half(d)))]
    for name, ci, co, lvl, stride in plan:
        out = levels[lvl] if stride == 1 else levels[lvl + 1]
        rows.append((name, ci, co, levels[lvl], stride, False, 27 * ci * co * vox(out)))
    for name, ci, co, lvl in (("conv7", 8 * c, 4 * c, 3), ("conv9", 4 * c, 2 * c, 2), ("conv11", 2 * c, c, 1)):
        rows.append((name, ci, co, levels[lvl], 2, True, 27 * ci * co * vox(levels[lvl])))       # every input voxel meets every tap once
    rows.append(("prob", c, 1, d, 1, False, 27 * c * vox(d)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("device", "torch"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mvs_cnn_cases as MC
    from uc_nerf_amd import ops
    from uc_nerf_amd.network.mvs_models import CostRegNet, FeatureNet
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(3)
    res = {"device": torch.cuda.get_device_name(dev), "peak_tflops": PEAK_TFLOPS, "modules": [], "layers": []}

    def route(module, x, name):
        def fn():
            module.inference = name
            with torch.no_grad():
                return module(x)
        return fn

    cases = [(title, CostRegNet(shape[1], 8), shape) for title, shape in VOLUMES] + [("feature", FeatureNet(8), IMAGE)]
    for i, (title, module, shape) in enumerate(cases):
        module = MC.randomise(module, 10 + i).to(dev)
        x = torch.rand(shape, generator=g).to(dev)
        fns = {name: route(module, x, name) for name in ("device", "torch") if args.only in (None, name)}
        row = {"case": title, "shape": list(shape), "routes": alternate(fns, args.reps)}
        if args.only is None:
            a, b = fns["device"](), fns["torch"]()
            a, b = (list(t.values()) if isinstance(t, dict) else list(t) for t in (a, b))
            row["largest_difference"] = max(float((u - v).abs().max()) for u, v in zip(a, b))
            row["largest_value"] = max(float(v.abs().max()) for v in b)
            if title != "feature":
                macs = sum(r[-1] for r in reg_layers(shape[1], 8, *shape[2:]))
                row["useful_gflop"] = 2e-9 * macs
                row["device_fraction_of_peak"] = 2 * macs / (row["routes"]["device"]["median_us"] * 1e-6) / (PEAK_TFLOPS * 1e12)
        res["modules"].append(row)
        print(json.dumps(row), flush=True)
        del module, x
        torch.cuda.empty_cache()

    if args.only is None:
        for title, shape in VOLUMES:
            for name, ci, co, dims, stride, transposed, macs in reg_layers(shape[1], 8, *shape[2:]):
                w = torch.randn((ci, co, 3, 3, 3) if transposed else (co, ci, 3, 3, 3), generator=g).to(dev)
                packed, bias = ops.conv3d_pack(w, transposed=transposed), torch.zeros(co, device=dev)
                x = torch.rand((1, ci) + dims, generator=g).to(dev)
                t = alternate({"conv3d": lambda: ops.conv3d(x, packed, bias, stride=stride, pad=1, transposed=transposed)}, args.reps)["conv3d"]
                row = {"case": title, "layer": name, "cin": ci, "cout": co, "in": list(dims), "stride": stride, "transposed": transposed, "useful_gflop": 2e-9 * macs,
                       "median_us": t["median_us"], "min_us": t["min_us"], "tflops": 2 * macs / (t["median_us"] * 1e-6) / 1e12}
                row["fraction_of_peak"] = row["tflops"] / PEAK_TFLOPS
                res["layers"].append(row)
                print(json.dumps(row), flush=True)
                del w, packed, x
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
