"""Times the colour frames' resize, 32 synthetic frames of 1024 x 1280 -> (320, 256):
  (a) ucnerf_resize_bilinear_u8 (ops.resize_bilinear_u8 into a padded destination): device events around `--iters` launches, warm, per launch and
      per frame.  The launches rotate over `--buffers` source batches (4 x 126 MB by default, more than the 256 MB Infinity Cache holds), so that
      the frames are read from HBM as they are after an upload, not from a cache a previous launch filled;
  (b) the upload of one such batch from pageable and from pinned host memory (a host clock that ends in a device synchronise);
  (c) Pillow's `Image.fromarray(frame).resize((320, 256), Image.BILINEAR)` on the host, per frame, for the same frames (where PIL imports), and the
      kernel's output is compared with it byte for byte.
Each figure is the median (min .. max) over `--rounds` rounds.  Achieved read bandwidth = 3 N Hin Win bytes over the launch time, against the HBM
figures of the MI355X (8.0 TB/s spec, about 6.3 TB/s achievable by a streaming copy).  The GPU work runs in a child process under its own time limit.
    python scripts/time_resize.py [--out profiles/resize.md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the figures to this markdown file (the resource section below a marker line is kept)")
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--buffers", type=int, default=4)
ap.add_argument("--limit", type=int, default=300, help="time limit of the measuring child, seconds")
ap.add_argument("--measure", action="store_true", help="(internal) run the measurement in this process and print one JSON line")
args = ap.parse_args()

HIN, WIN, W, H = 1024, 1280, 320, 256
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def measure():
    import numpy as np
    import torch

    from uc_nerf_amd import ops
    from uc_nerf_amd.ops._core import Event

    dev = torch.device("cuda:0")
    N = args.frames
    rs = np.random.RandomState(0)
    host = [rs.randint(0, 256, (N, HIN, WIN, 3), dtype=np.uint8) for _ in range(args.buffers)]
    srcs = [torch.from_numpy(h).to(dev) for h in host]
    stride = (3 * H * W + 3) // 4 * 4
    out = torch.zeros((N, stride), dtype=torch.uint8, device=dev)
    for s in srcs:                                            # warm: code object, coefficient tables
        ops.resize_bilinear_u8(s, (W, H), out=out)
    torch.cuda.synchronize()
    res = {"frames": N, "iters": args.iters, "rounds": args.rounds, "buffers": args.buffers, "device": torch.cuda.get_device_name(0)}
    launch = []
    for _ in range(args.rounds):
        a, b = Event(), Event()
        a.record()
        for i in range(args.iters):
            ops.resize_bilinear_u8(srcs[i % len(srcs)], (W, H), out=out)
        b.record()
        torch.cuda.synchronize()
        launch.append(a.elapsed_ms(b) * 1e3 / args.iters)     # microseconds per launch
    res["launch_us"] = med(launch)
    # upload of one batch
    pinned = torch.from_numpy(host[0]).pin_memory()
    for name, h in (("upload_pageable_us", torch.from_numpy(host[0])), ("upload_pinned_us", pinned)):
        ts = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            h.to(dev, non_blocking=True)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e6)
        res[name] = med(ts)
    # Pillow on the host, the same frames; and the bits
    try:
        from PIL import Image
        import PIL
    except ImportError:
        res["pillow_us_per_frame"] = None
    else:
        got = ops.resize_bilinear_u8(srcs[0], (W, H)).cpu().numpy()
        ts, same = [], True
        for r in range(min(args.rounds, 3)):
            t = time.perf_counter()
            ref = [np.asarray(Image.fromarray(host[0][f]).resize((W, H), Image.BILINEAR)) for f in range(N)]
            ts.append((time.perf_counter() - t) * 1e6 / N)
            same = same and all(np.array_equal(ref[f], got[f]) for f in range(N))
        res["pillow_us_per_frame"], res["pillow_version"], res["equal_to_pillow"] = med(ts), PIL.__version__, bool(same)
    print("RESULT " + json.dumps(res), flush=True)


def fmt(m, div=1.0, unit="us"):
    return "%.1f %s (%.1f .. %.1f)" % (m["median"] / div, unit, m["min"] / div, m["max"] / div)


def main():
    if args.measure:
        return measure()
    cmd = [sys.executable, os.path.abspath(__file__), "--measure"] + [a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("time_resize: the measuring child failed (%d)" % r.returncode)
    res = json.loads(line[-1][7:])
    N = res["frames"]
    us = res["launch_us"]["median"]
    in_bytes, out_bytes = 3 * N * HIN * WIN, 3 * N * H * W
    bw = in_bytes / (us * 1e-6)
    rows = ["| figure | value |", "|---|---|",
            "| device | %s |" % res["device"],
            "| workload | %d frames, %d x %d -> (%d, %d); %.1f MB read, %.1f MB written per launch |" % (N, HIN, WIN, W, H, in_bytes / 1e6, out_bytes / 1e6),
            "| resize launch (device events, %d launches a round, %d rounds, %d source batches in rotation) | %s |" % (res["iters"], res["rounds"], res["buffers"], fmt(res["launch_us"])),
            "| ... per frame | %s |" % fmt(res["launch_us"], N),
            "| achieved read bandwidth | %.2f TB/s = %.0f %% of the 6.3 TB/s a streaming copy reaches, %.0f %% of the 8.0 TB/s spec |" % (bw / 1e12, 100 * bw / HBM_COPY, 100 * bw / HBM_SPEC),
            "| upload of the %d frames, pageable host memory | %s; per frame %s |" % (N, fmt(res["upload_pageable_us"], 1e3, "ms"), fmt(res["upload_pageable_us"], N)),
            "| upload of the %d frames, pinned host memory | %s; per frame %s |" % (N, fmt(res["upload_pinned_us"], 1e3, "ms"), fmt(res["upload_pinned_us"], N))]
    if res.get("pillow_us_per_frame"):
        rows.append("| Pillow %s on this host's CPU, per frame, same frames | %s |" % (res["pillow_version"], fmt(res["pillow_us_per_frame"])))
        rows.append("| kernel output equal to Pillow's, byte for byte, all %d frames | %s |" % (N, "yes" if res["equal_to_pillow"] else "NO"))
    else:
        rows.append("| Pillow on the host | PIL does not import here: not measured |")
    table = "\n".join(rows)
    print(table)
    print(json.dumps(res))
    if args.out:
        marker = "<!-- measured figures above this line are rewritten by scripts/time_resize.py -->"
        tail = ""
        if os.path.exists(args.out):
            text = open(args.out).read()
            if marker in text:
                tail = text.split(marker, 1)[1]
        with open(args.out, "w") as f:
            f.write("# Colour frames' resize on the device (`scripts/time_resize.py`)\n\n" + table + "\n\n" + marker + tail)


if __name__ == "__main__":
    main()
