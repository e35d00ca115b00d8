"""Times LPIPS on the device (utils.evaluation.LPIPS over csrc/lpips.hip) per 256 x 320 pair and per 10-view epoch, next to the same chain
through torch's own device convolutions, and each kernel of the chain on its own with its FLOPs over the fp32-MFMA peak.

    python scripts/time_lpips.py [--reps 30] [--out FILE]

Event-timed on the current stream, warm (5 untimed calls first), the median and the spread of --reps repetitions.  Random weights of the
real shapes (the time does not depend on the values).  The numbers in profiles/lpips.md are this script's output."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

PEAK_TFLOPS = 157.3      # fp32 MFMA, MI355X spec


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) * 1e3)
    ms.sort()
    return {"median_us": statistics.median(ms), "min_us": ms[0], "p90_us": ms[int(0.9 * (len(ms) - 1))], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import lpips_cases as LC
    from uc_nerf_amd import ops
    from uc_nerf_amd.utils.evaluation import LPIPS
    dev = torch.device("cuda", torch.cuda.current_device())
    alex, lin = LC.weights()
    metric = LPIPS(alex, lin, device=dev)
    H, W = 256, 320
    res = {"device": torch.cuda.get_device_name(dev), "H": H, "W": W, "peak_tflops": PEAK_TFLOPS, "chain": {}, "kernels": []}
    wd = {k: v.to(dev) for k, v in alex.items()}
    ld = [lin["lin%d.model.1.weight" % l].reshape(-1).to(dev) for l in range(5)]

    # the same chain through torch's device kernels (tests/lpips_cases.py's restatement with its constants on the device)
    shift = torch.tensor(LC.SHIFT, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(LC.SCALE, device=dev).view(1, 3, 1, 1)

    def torch_features(x):
        h = (x - shift) / scale
        out = []
        for l, (idx, _, _, _, stride, pad) in enumerate(LC.CONVS):
            if l in (1, 2):
                h = F.max_pool2d(h, 3, 2)
            h = F.relu(F.conv2d(h, wd["features.%d.weight" % idx], wd["features.%d.bias" % idx], stride=stride, padding=pad))
            out.append(h)
        return out

    def torch_chain(a, b):
        fa, fb = torch_features(a), torch_features(b)
        return sum(LC.layer_distance(fa[l], fb[l], ld[l]) for l in range(5))

    for n, label in ((1, "pair"), (10, "epoch_10_views")):
        g = torch.Generator().manual_seed(n)
        a = (torch.rand(n, 3, H, W, generator=g) * 2 - 1).to(dev)
        b = (torch.rand(n, 3, H, W, generator=g) * 2 - 1).to(dev)
        entry = {"n": n, "ours": timed(lambda: metric(a, b), args.reps)}
        try:
            with torch.no_grad():
                entry["torch"] = timed(lambda: torch_chain(a, b), args.reps)
                entry["max_abs_diff_ours_torch"] = float((metric(a, b) - torch_chain(a, b)).abs().max())
        except Exception as e:                                          # (torch's device convolutions may be unavailable on a box)
            entry["torch"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        res["chain"][label] = entry

    # each kernel of the chain on its own, at the batch of one pair (2 images) and of an epoch (20 images)
    for m in (2, 20):
        x = torch.rand(m, 3, H, W, device=dev) * 2 - 1
        for l, (idx, cin, cout, K, stride, pad) in enumerate(LC.CONVS):
            if l in (1, 2):
                res["kernels"].append(dict(name="pool%d" % l, images=m, **timed(lambda: ops.maxpool2d(x), args.reps)))
                x = ops.maxpool2d(x)
            bias = wd["features.%d.bias" % idx]
            extra = dict(shift=metric.shift, scale=metric.scale) if l == 0 else {}
            t = timed(lambda: ops.conv2d_bias_relu(x, metric.convs[l], bias, stride=stride, pad=pad, **extra), args.reps)
            y = ops.conv2d_bias_relu(x, metric.convs[l], bias, stride=stride, pad=pad, **extra)
            flop = 2.0 * m * cout * y.shape[2] * y.shape[3] * cin * K * K
            t.update(name="conv%d" % (l + 1), images=m, gflop=flop / 1e9, tflops=flop / t["median_us"] / 1e6,
                     of_peak=flop / t["median_us"] / 1e6 / PEAK_TFLOPS, blocks=-(-m * y.shape[2] * y.shape[3] // 64) * -(-cout // 64))
            res["kernels"].append(t)
            half = m // 2
            tl = timed(lambda: ops.lpips_layer(y[:half], y[half:], ld[l]), args.reps)
            tl.update(name="layer%d" % l, images=m, mbytes=2 * y.numel() * 4 / 1e6)
            res["kernels"].append(tl)
            x = y
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
