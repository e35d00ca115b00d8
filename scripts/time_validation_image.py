"""One 256 x 320 validation image on the synthetic scene, at --chunk 1024 and --chunk 81920: the loop as the reference writes it (train.py:251-288
through the drop-in modules: build_rays_test -> rendering -> rgb.cpu(), depth.cpu() per chunk, host cat / clamp / permute, the two depth pictures
through visualize_depth's numpy path) against uc_nerf_amd.validate.render_validation_image (chunks written into the image planes by
ucnerf_image_put, the depth pictures by ucnerf_depth_colormap, nothing read back).

Wall time per image on the host clock, every window closed by torch.cuda.synchronize(); median, minimum and maximum of --rounds images after
warm-up.  The routes alternate inside every round (baseline, device, baseline again, device + metrics, baseline + metrics), so the two baseline
columns show the run-to-run spread the difference has to beat.  "+ metrics" adds rgb_evaluation and depth_evaluation of the one image, i.e. it
ends in the metrics' own small read.  The new kernels' own time is taken with device events around the 80 (or 1) image_put launches and the
two colour-map launches of one image.  Both routes are first checked to give the same bits.  Writes a markdown note (--out) and prints one
JSON line.  Needs a GPU: there is no fallback."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(dev, H, W):
    import uc_nerf_amd
    uc_nerf_amd.install_dropin()
    import network.models as models
    from uc_nerf_amd.synthetic import cascade_outputs, init_ucnerf_state_dict, make_scene, scene_to
    scene = scene_to(make_scene(seed=0, H=H, W=W), dev)
    a = types.SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=6, netwidth=128, feat_dim=97, net_type="v2", view_num=7, netchunk=1024,
                              perturb=1.0, N_samples=90, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0, ckpt=None, device=str(dev),
                              img_downscale=1.0, use_color_volume=False, chunk=1024, pad=0)
    kw, _, _, _ = models.create_ucnerf(a, dir_embedder=True, pts_embedder=True)
    kw["network_fn"].load_state_dict(init_ucnerf_state_dict(seed=0, n_src=6, sigma_scale=0.05, sigma_bias=0.05))
    outputs = cascade_outputs(scene)
    outputs["stage3"]["img_feats"] = scene["img_feat"]
    near_fars = torch.tensor([[scene["near"], scene["far"]]] * 7, device=dev)
    g = torch.Generator().manual_seed(9)
    depth_gt = 1.0 + 3.0 * torch.rand(H, W, generator=g)
    depth_gt[:8] = 0.0
    return dict(scene=scene, args=a, kw=kw, outputs=outputs, near_fars=near_fars, depth_gt=depth_gt, gt_rgb=torch.rand(3, H, W, generator=g), H=H, W=W)


def pose(scene):
    return {"w2cs": scene["w2cs"].clone(), "intrinsics": scene["intrinsics"].clone(), "c2ws": scene["c2w"].unsqueeze(0).clone()}


def baseline(s, chunk):
    """train.py:249-288 as the parent commit serves it."""
    import network.renderer as renderer
    import utils.utils as U
    H, W, scene, a, kw, outputs, near_fars = s["H"], s["W"], s["scene"], s["args"], s["kw"], s["outputs"], s["near_fars"]
    pose_ref = pose(scene)
    world_to_ref, tgt_to_world, intrinsic = pose_ref["w2cs"][0], pose_ref["c2ws"][0], pose_ref["intrinsics"][0]
    rgbs, depth_preds = [], []
    with torch.no_grad():
        for chunk_idx in range(H * W // chunk + int(H * W % chunk > 0)):
            rays_pts, rays_dir, rays_NDC, depth_candidates, rays_o, ndc_parameters = U.build_rays_test(
                H, W, tgt_to_world, world_to_ref, intrinsic, near_fars, near_fars[-1], a.N_samples, pad=a.pad, chunk=chunk, idx=chunk_idx, outputs=outputs)
            rgb, depth_pred = renderer.rendering(a, pose_ref, rays_pts, rays_NDC, depth_candidates, rays_dir, outputs, scene["imgs"], near_fars=near_fars[0],
                                                 img_feat=outputs["stage3"]["img_feats"], confidence=scene["confidence"], ndc_parameters=ndc_parameters, **kw)
            rgbs.append(rgb.cpu())
            depth_preds.append(depth_pred.cpu())
        render_rgb = torch.clamp(torch.cat(rgbs).reshape(H, W, 3).permute(2, 0, 1), 0, 1)
        render_depth = torch.cat(depth_preds).reshape(H, W)
        depth_gt = s["depth_gt"]
        log = {"pred_rgb": render_rgb, "pred_depth": render_depth, "gt_rgb": s["gt_rgb"], "gt_depth": depth_gt, "mask": depth_gt > 0,
               "gt_depth_vis": U.visualize_depth(depth_gt), "pred_depth_vis": U.visualize_depth(render_depth),
               "uncertainty": kw["network_fn"].forward_uncertainty(scene["confidence"].reshape(1, -1, 1)).reshape(H, W)}
    return log


def device_route(s, chunk):
    from uc_nerf_amd.validate import render_validation_image
    a = types.SimpleNamespace(**dict(vars(s["args"]), chunk=chunk))
    return render_validation_image(a, pose(s["scene"]), s["outputs"], s["scene"]["imgs"], s["scene"]["confidence"], s["H"], s["W"], s["near_fars"], s["kw"],
                                   depth_gt=s["depth_gt_dev"], gt_rgb=s["gt_rgb_dev"])


def metrics(log):
    from uc_nerf_amd.utils import evaluation as M
    with contextlib.redirect_stdout(io.StringIO()):
        return M.rgb_evaluation(log["gt_rgb"][None], log["pred_rgb"][None], None), M.depth_evaluation(log["gt_depth"][None], log["pred_depth"][None])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def kernel_ms(s, chunk, rounds):
    """Device-event time of the new launches of one image: the image_put calls, and the two colour maps with the ground truth's range fold."""
    from uc_nerf_amd import ops
    from uc_nerf_amd.utils.utils import _device_table
    H, W = s["H"], s["W"]
    dev = s["near_fars"].device
    n = H * W
    rgb, depth = torch.rand(n, 3, device=dev), 1 + torch.rand(n, device=dev)
    img, dep = torch.empty(3, H, W, device=dev), torch.empty(H, W, device=dev)
    table = _device_table(None, dev)
    pieces = [(f, min(chunk, n - f)) for f in range(0, n, chunk)]
    chunks = [(rgb[f:f + m].contiguous(), depth[f:f + m].contiguous(), f) for f, m in pieces]
    put, vis = [], []
    for _ in range(rounds + 2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        cell = ops.minmax_reset(device=dev)
        e[0].record()
        for r, d, f in chunks:
            ops.image_put(r, d, f, img, dep, cell)
        e[1].record()
        ops.depth_colormap(dep, table, minmax=cell, want_index=False)
        ops.depth_colormap(s["depth_gt_dev"], table, want_index=False)
        e[2].record()
        torch.cuda.synchronize()
        put.append(e[0].elapsed_time(e[1]))
        vis.append(e[1].elapsed_time(e[2]))
    return statistics.median(put[2:]), statistics.median(vis[2:]), len(chunks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1024, 81920])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_image.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_validation_image: no GPU (there is no fallback)")
    dev = torch.device("cuda:0")
    H, W = 256, 320
    s = setup(dev, H, W)
    s["depth_gt_dev"], s["gt_rgb_dev"] = s["depth_gt"].to(dev), s["gt_rgb"].to(dev)
    routes = ("baseline", "device", "baseline_again", "device_metrics", "baseline_metrics")
    result = {"image": [H, W], "samples_per_ray": s["args"].N_samples, "rounds": a.rounds, "chunks": {}}
    for chunk in a.chunks:
        fns = {"baseline": lambda: baseline(s, chunk), "device": lambda: device_route(s, chunk), "baseline_again": lambda: baseline(s, chunk),
               "device_metrics": lambda: metrics(device_route(s, chunk)), "baseline_metrics": lambda: metrics(baseline(s, chunk))}
        # same bits first (and the warm-up of every shape the timed windows use)
        torch.manual_seed(3)
        b = baseline(s, chunk)
        torch.manual_seed(3)
        d = device_route(s, chunk)
        same = {k: bool(torch.equal(b[k].to(dev), d[k])) for k in ("pred_rgb", "pred_depth", "pred_depth_vis", "gt_depth_vis", "uncertainty", "mask")}
        for fn in fns.values():
            fn()
        ts = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k in routes:
                ts[k].append(wall(fns[k]))
        put_ms, vis_ms, n_chunks = kernel_ms(s, chunk, a.rounds)
        result["chunks"][str(chunk)] = {"n_chunks": n_chunks, "same_bits": same, "image_put_launches_ms": put_ms, "colormap_launches_ms": vis_ms,
                                        "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ts.items()}}
    lines = ["# A whole validation image on the device", "",
             "`python scripts/time_validation_image.py` on an MI355X: one %d x %d image of the synthetic scene, %d samples per ray, wall time per image in ms" % (H, W, s["args"].N_samples),
             "(host clock, every window closed by a device synchronise; median [min .. max] of %d images after warm-up, the routes alternating inside" % a.rounds,
             "every round).  *baseline* is the reference's loop through the drop-in modules as the parent commit serves it: `.cpu()` twice per chunk, host",
             "cat / clamp / permute, both depth pictures through `visualize_depth`'s numpy path.  *device* is `render_validation_image`.  *+ metrics* adds",
             "`rgb_evaluation` and `depth_evaluation` of the image, so it ends in the metrics' own read.  The baseline is timed twice per round: the",
             "distance between its two columns is the spread a difference has to beat.", ""]
    fmt = lambda m: "%.2f [%.2f .. %.2f]" % (m["median"], m["min"], m["max"])      # noqa: E731
    lines += ["| chunk | chunks | baseline | baseline again | device | baseline + metrics | device + metrics |", "|---|---|---|---|---|---|---|"]
    for chunk, r in result["chunks"].items():
        m = r["ms"]
        lines.append("| %s | %d | %s | %s | %s | %s | %s |" % (chunk, r["n_chunks"], fmt(m["baseline"]), fmt(m["baseline_again"]), fmt(m["device"]),
                                                              fmt(m["baseline_metrics"]), fmt(m["device_metrics"])))
    lines += ["", "The new launches on their own (device events, median): "]
    for chunk, r in result["chunks"].items():
        lines.append("- chunk %s: the %d `image_put` launches of one image %.3f ms; the two colour maps with the ground truth's range fold %.3f ms." % (
            chunk, r["n_chunks"], r["image_put_launches_ms"], r["colormap_launches_ms"]))
    lines += [""]
    for chunk, r in result["chunks"].items():
        m = r["ms"]
        spread = abs(m["baseline"]["median"] - m["baseline_again"]["median"])
        gain = min(m["baseline"]["median"], m["baseline_again"]["median"]) - m["device"]["median"]
        verdict = "faster than the baseline beyond its spread" if gain > spread else "NOT faster than the baseline beyond its spread"
        lines.append("- chunk %s: device route %s (gain %.2f ms against a spread of %.2f ms between the two baseline columns); same bits as the baseline: %s." % (
            chunk, verdict, gain, spread, ", ".join("%s %s" % (k, "yes" if v else "NO") for k, v in r["same_bits"].items())))
    lines += ["", "`utils.colormaps.jet_lut()` is built from the published definition of OpenCV's Jet and is **not verified against OpenCV** (cv2 is not",
              "installed where this was developed or measured); `cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET).reshape(256, 3)` gives",
              "the authoritative table, which every `cmap=` argument accepts.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
