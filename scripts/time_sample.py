"""Times the assembly of one training sample at 256 x 320, V = 5, about 1000 keypoints on the target, in three ways:
  (a) the host restatement of the reference's __getitem__ on already decoded arrays (tests/sample_cases.py: reference_sample) plus pinned
      host-to-device copies of its outputs -- what the reference's loader costs AFTER decoding and resizing, so a floor for it;
  (b) the same sample composed from torch expressions on the scene's resident device arrays;
  (c) DeviceScene.sample: one launch (ucnerf_sample_assemble), with and without images_unpre.
(b) and (c) draw their keypoint permutation on the device inside the timed call, (a) shuffles on the host as the reference does.  Each figure is a
host clock around `--iters` calls that ends in a device synchronise, per call; the three are timed alternately, `--rounds` rounds, median
(min .. max).  The GPU work runs in a child process under its own time limit; this process never opens the device.
    python scripts/time_sample.py [--out profiles/sample_assembly.md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this markdown file")
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--views", type=int, default=5)
ap.add_argument("--keypoints", type=int, default=1000)
ap.add_argument("--limit", type=int, default=420, help="time limit of the measuring child, seconds")
ap.add_argument("--measure", action="store_true", help="(internal) run the measurement in this process and print one JSON line")
args = ap.parse_args()

H, W = 256, 320


def measure():
    import numpy as np
    import torch

    import sample_cases as SC
    from uc_nerf_amd.data import DeviceScene

    dev = torch.device("cuda:0")
    sc = SC.make_scene(H, W, (args.keypoints,) * args.frames, seed=21)
    ds = DeviceScene.from_arrays(sc["poses"], sc["focal"], sc["bounds"], sc["sparse"], sc["frames"], sc["dpt"], sc["depths_h"], sc["img_wh"], device=dev)
    target, src = 1, [(2 + k) % args.frames for k in range(args.views - 1)]
    ids = torch.tensor([target] + src, device=dev)
    mean = torch.tensor(ds.mean, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(ds.std, device=dev).view(1, 3, 1, 1)
    frames = ds.frames[:, :3 * H * W].reshape(-1, H, W, 3)
    r1, c1, r2, c2 = ds.row1.long(), ds.col1.long(), ds.row2.long(), ds.col2.long()
    a0, a1 = ds.offsets[target], ds.offsets[target + 1]
    near_fars = torch.tensor(ds.near_far, device=dev).expand(1, 1, args.views, 2)
    rs = np.random.RandomState(0)

    def flat(d):
        for v in d.values():
            if isinstance(v, dict):
                yield from v.values()
            else:
                yield v

    def host():
        out = SC.reference_sample(sc, target, src, perm=rs.permutation(a1 - a0))
        return [t.pin_memory().to(dev, non_blocking=True) for t in flat(out)]

    def torch_route():
        x = frames[ids].permute(0, 3, 1, 2).to(torch.float32).div(255.0)
        images = ((x - mean) / std)[None]
        d, w = ds.depth_img[target], ds.weight_img[target]
        ms = {"stage1": d[r1][:, c1][None], "stage2": d[r2][:, c2][None], "stage3": d[None]}
        wms = {"stage1": w[r1][:, c1][None], "stage2": w[r2][:, c2][None], "stage3": w[None]}
        perm = torch.randperm(a1 - a0, device=dev)[:1024] + a0
        coord = ds.kp_coord[perm].to(torch.float32)
        rows = torch.stack([ds.kp_depth[perm][:, None].expand(-1, 3), ds.kp_weight[perm][:, None].expand(-1, 3),
                            torch.cat([coord, torch.ones_like(coord[:, :1])], 1)], 1)[None]
        proj = (ds.affine[ids][:, 2] @ ds.ref_proj_inv[target])[:, :3].clone()
        proj[0] = torch.eye(4, device=dev)[:3]
        return {"images": images, "sparse_depths_ms": ms, "weight_ms": wms, "rays_depth": rows, "proj_mats": proj[None], "c2ws": ds.c2w[ids][None],
                "w2cs": ds.w2c[ids][None], "intrinsics": ds.intrinsic[ids][None], "affine_mat": ds.affine[ids][None], "affine_mat_inv": ds.affine_inv[ids][None],
                "near_fars": near_fars, "view_ids": ids[None], "dpt": ds.dpt[target][None], "depths_h": ds.depths_h[target][None],
                "sparse_depths": d[None], "sparse_depths_weight": w[None], "scan": ds.scan}

    routes = {"host": host, "torch": torch_route, "launch": lambda: ds.sample(target, src), "launch_unpre": lambda: ds.sample(target, src, unpreprocess=True)}

    def timed(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    # the torch route and the launch agree where both make the reference's roundings
    a, b = torch_route(), ds.sample(target, src)
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k]))) for k in ("images", "c2ws", "affine_mat_inv", "sparse_depths")}
    same["stage1"] = bool(torch.equal(a["sparse_depths_ms"]["stage1"], b["sparse_depths_ms"]["stage1"]))
    for fn in routes.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(timed(fn, max(1, args.iters // 10) if k == "host" else args.iters))
    print(json.dumps({"times": times, "same": same, "n_kp": a1 - a0, "device": torch.cuda.get_device_name(0)}))


if args.measure:
    measure()
    sys.exit(0)

cmd = [sys.executable, os.path.abspath(__file__), "--measure", "--iters", str(args.iters), "--rounds", str(args.rounds), "--frames", str(args.frames),
       "--views", str(args.views), "--keypoints", str(args.keypoints)]
r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
if r.returncode != 0:
    sys.exit("the measuring process failed (exit %d):\n%s" % (r.returncode, r.stderr[-3000:]))
res = json.loads(r.stdout.strip().splitlines()[-1])
fmt = lambda t: "%.1f (%.1f .. %.1f)" % (statistics.median(t), min(t), max(t))      # noqa: E731
t = res["times"]
lines = ["One sample at %d x %d, V = %d, %d keypoints on the target, %d resident frames, on %s.  Microseconds per sample: a host clock around %d calls"
         " (host route: %d) ending in a device synchronise, median (min .. max) of %d alternating rounds."
         % (H, W, args.views, res["n_kp"], args.frames, res["device"], args.iters, max(1, args.iters // 10), args.rounds), "",
         "| route | us per sample |", "|---|---|",
         "| (a) host restatement of the reference's `__getitem__` on decoded arrays + pinned host-to-device copies | %s |" % fmt(t["host"]),
         "| (b) torch expressions on the resident device arrays | %s |" % fmt(t["torch"]),
         "| (c) `DeviceScene.sample`: one launch | %s |" % fmt(t["launch"]),
         "| (c) with `unpreprocess=True` (images_unpre from the same launch) | %s |" % fmt(t["launch_unpre"]), "",
         "(b) and (c) bit-equal on images, gathered matrices and maps: %s." % res["same"]]
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
