"""Times multi-view depth fusion at 256 x 320, S = 4, with N = 10 and N = 40 views of the two-plane scene of tests/fusion_cases.py:
  * `ops.depth_consistency` (one launch) and `ops.points_compact` (three kernels, one ABI call), device events around `--iters` calls each;
  * a torch-composed route of the same computation on the same device, written here: per source slot a batched pinhole projection,
    `grid_sample` (bilinear, align_corners=True, zero border) on the depth maps, the back-projection and the two tests; then a boolean-mask
    gather for the compaction (`fused[mask]`, which synchronises to learn the count).  It does NOT reproduce the kernel's tap rules (a zero
    border instead of refusing invalid taps), so the two masks are compared and the fraction that differs is reported, not asserted;
  * the consistency launch's achieved bytes/s, counted as what it must stream (4 bytes in and 6 out per pixel; the gathered taps hit the
    caches or not, they are not counted), against the 6.3 TB/s a streaming copy reaches on this board (the figure the other profiles use).
Each N runs in a child process under its own time limit; after one that failed or ran out of time nothing more is started.  The figures
include the wrapper's allocations and the launch: at N = 10 they are partly the rate at which the host issues launches, so the bytes/s row is a
lower bound there.  Nothing here is a pass bar.  Prints one JSON line (--json FILE keeps it): profiles/fusion.md is written from it.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, S = 256, 320, 4
COPY_TBS = 6.3
LIMITS = {10: 120, 40: 200}         # seconds per section (the scene is built in float64 numpy on the host first)
THRESH = dict(pix_thresh=1.0, rel_thresh=0.01, min_views=3)


def events(fn, iters, rounds=5):
    import torch
    fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def torch_consistency(depth, K, c2w, w2c, src, pix_thresh, rel_thresh, min_views):
    """The same computation composed from torch ops (float32, one batch of N views per source slot)."""
    import torch
    import torch.nn.functional as F
    N, Hh, Ww = depth.shape
    ys, xs = torch.meshgrid(torch.arange(Hh, device=depth.device, dtype=torch.float32), torch.arange(Ww, device=depth.device, dtype=torch.float32), indexing="ij")

    def back(Kb, x, y, d):
        return torch.stack([(x - Kb[:, 0, 2, None, None]) / Kb[:, 0, 0, None, None] * d, (y - Kb[:, 1, 2, None, None]) / Kb[:, 1, 1, None, None] * d, d], -1)

    def apply(M, P):
        return torch.einsum("nij,nhwj->nhwi", M[:, :3, :3], P) + M[:, None, None, :3, 3]

    def proj(Kb, Q):
        return (Kb[:, 0, 0, None, None] * Q[..., 0] / Q[..., 2] + Kb[:, 0, 2, None, None], Kb[:, 1, 1, None, None] * Q[..., 1] / Q[..., 2] + Kb[:, 1, 2, None, None])

    valid = torch.isfinite(depth) & (depth > 0)
    X = apply(c2w, back(K, xs, ys, depth))
    count = torch.zeros_like(depth, dtype=torch.int32)
    total = depth.clone()
    for j in range(src.shape[1]):
        s = src[:, j].long()
        Q = apply(w2c[s], X)
        u, v = proj(K[s], Q)
        ok = valid & (Q[..., 2] > 0) & (u >= 0) & (u <= Ww - 1) & (v >= 0) & (v <= Hh - 1)
        grid = torch.stack([2 * u / (Ww - 1) - 1, 2 * v / (Hh - 1) - 1], -1)
        ds = F.grid_sample(depth[s][:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
        Qr = apply(w2c, apply(c2w[s], back(K[s], u, v, ds)))
        xr, yr = proj(K, Qr)
        dp = Qr[..., 2]
        ok = ok & (ds > 0) & (dp > 0) & (torch.hypot(xr - xs, yr - ys) < pix_thresh) & ((dp - depth).abs() / depth < rel_thresh)
        count += ok
        total = total + torch.where(ok, dp, torch.zeros_like(dp))
    fused = torch.where(valid, total / (count + 1), torch.zeros_like(total))
    return valid & (count >= min_views), fused, count


def torch_compact(fused, mask, rgb, K, c2w):
    import torch
    N, Hh, Ww = fused.shape
    ys, xs = torch.meshgrid(torch.arange(Hh, device=fused.device, dtype=torch.float32), torch.arange(Ww, device=fused.device, dtype=torch.float32), indexing="ij")
    P = torch.stack([(xs - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None] * fused, (ys - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None] * fused, fused], -1)
    Xw = torch.einsum("nij,nhwj->nhwi", c2w[:, :3, :3], P) + c2w[:, None, None, :3, 3]
    cols = (rgb.permute(0, 2, 3, 1).nan_to_num(0.0).clamp(0, 1) * 255 + 0.5).to(torch.uint8)
    return Xw[mask], cols[mask]                                                       # boolean-mask gather: synchronises for the count


def run(N, iters):
    import numpy as np
    import torch
    import fusion_cases as FC
    from uc_nerf_amd import ops
    dev = torch.device("cuda")
    case = FC.diff_case("two-plane", H, W, 7, True, N=N, S=S)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in case.items() if v is not None}
    args = (t["depth"], t["intrinsics"], t["c2ws"], t["src_ids"])
    res = {"N": N, "pixels": N * H * W}
    res["depth_consistency"] = events(lambda: ops.depth_consistency(*args, w2cs=t["w2cs"], **THRESH), iters)
    res["depth_consistency_rigid"] = events(lambda: ops.depth_consistency(*args, **THRESH), iters)
    mask, fused, count = ops.depth_consistency(*args, w2cs=t["w2cs"], **THRESH)
    res["masked_fraction"] = float(mask.float().mean())
    res["points_compact"] = events(lambda: ops.points_compact(fused, mask, t["rgb"], t["intrinsics"], t["c2ws"]), iters)
    res["torch_consistency"] = events(lambda: torch_consistency(*args[:3], t["w2cs"], t["src_ids"], **THRESH), max(iters // 10, 2))
    res["torch_compact"] = events(lambda: torch_compact(fused, mask, t["rgb"], t["intrinsics"], t["c2ws"]), max(iters // 10, 2))
    tm, tf, tc = torch_consistency(*args[:3], t["w2cs"], t["src_ids"], **THRESH)
    res["torch_mask_differs_fraction"] = float((tm != mask).float().mean())
    both = tm & mask
    res["torch_fused_max_rel_diff_on_common_mask"] = float(((tf - fused).abs() / fused)[both].max()) if bool(both.any()) else None
    streamed = N * H * W * (4 + 6)
    res["consistency_streamed_bytes"] = streamed
    res["consistency_TBps"] = streamed / (res["depth_consistency"]["median_us"] * 1e-6) / 1e12
    res["consistency_fraction_of_copy"] = res["consistency_TBps"] / COPY_TBS
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", type=int, default=None, help="(internal) run one N in this process")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.section is not None:
        print("RESULT " + json.dumps(run(a.section, a.iters)))
        sys.exit(0)
    result = {"image": [H, W], "S": S, "copy_TBps": COPY_TBS, "runs": []}
    for N, limit in LIMITS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--section", str(N), "--iters", str(a.iters)],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        result["runs"].append(json.loads(line[-1][7:]) if r.returncode == 0 and line else {"N": N, "failed": r.returncode, "stderr": r.stderr[-1500:]})
        if r.returncode != 0:
            break                                                                    # a section that failed or ran out of time: nothing more is started
    print(json.dumps(result))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
