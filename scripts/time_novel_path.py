"""Times free-camera rendering on the synthetic scene of tests/sample_cases.make_scene at 256 x 320, V = 7, 14 resident frames:
  (a) the batch of one novel pose: `DeviceScene.sample_pose` (one launch, ucnerf_novel_assemble) against the host-composed route it replaces --
      `frame_matrices` (four LAPACK inverses), `formats.get_nearest_pose_ids`, one packed upload of the matrices, `sample()`'s image gather for
      the chosen sources, the target's matrices copied into slot 0 and the proj_mats product.  Microseconds per frame: a host clock around
      `--iters` calls closed by a synchronise, and device events around the same loop (what the device itself spends, launch gaps included);
  (b) `UCNeRFSystem.render_path` over 30 poses against 30 frames composed on the host (that route's batch, then `render_novel_view`).
      Milliseconds per frame, host clock closed by a synchronise.
Each section runs in a child process under its own time limit; nothing here is a pass bar.  Prints one JSON line (--json FILE keeps it):
profiles/novel_path.md is written from it.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, V, N_FRAMES, KP, PATH = 256, 320, 7, 14, 16, 30
LIMITS = {"a": 150, "b": 400}


def build_scene():
    import torch
    import sample_cases as SC
    from uc_nerf_amd.data.scene import DeviceScene
    s = SC.make_scene(H, W, (KP,) * N_FRAMES, seed=5)
    scene = DeviceScene.from_arrays(s["poses"], s["focal"], s["bounds"], s["sparse"], s["frames"], s["dpt"], s["depths_h"] + 0.5, device=torch.device("cuda"))
    return s, scene


def path_poses(s, n):
    from uc_nerf_amd.data.paths import interp_path
    return interp_path(s["poses"][[0, 4, 8, 12]], n)


def host_batch(s, scene, pose64, train):
    """The route `sample_pose` replaces, for one pose: host matrices, host selection, one upload, the image gather, slot 0 patched on the device."""
    import numpy as np
    import torch
    from uc_nerf_amd.data.formats import get_nearest_pose_ids
    from uc_nerf_amd.data.scene import frame_matrices
    c2w, w2c, K, aff, aff_inv, ref_proj_inv = frame_matrices(pose64, s["focal"], s["img_wh"])
    src = train[get_nearest_pose_ids(pose64, s["poses"][train], V - 1)].tolist()
    packed = torch.from_numpy(np.concatenate([c2w.ravel(), w2c.ravel(), aff.ravel(), aff_inv.ravel(), ref_proj_inv.ravel()])).to(scene.device)
    b = scene.sample(src[0], src[1:] + src[:1], unpreprocess=True)                   # V views: slot 0 is overwritten below, slots 1.. are the sources
    b = {k: v for k, v in b.items() if torch.is_tensor(v)}                           # (the two per-stage dicts of a training sample: a free pose has none)
    ids = torch.tensor(src[1:] + src[:1], device=scene.device)
    b["c2ws"][0, 0], b["w2cs"][0, 0] = packed[:16].view(4, 4), packed[16:32].view(4, 4)
    b["affine_mat"][0, 0], b["affine_mat_inv"][0, 0] = packed[32:80].view(3, 4, 4), packed[80:128].view(3, 4, 4)
    b["proj_mats"][0, 1:] = (scene.affine[ids][:, 2] @ packed[128:144].view(4, 4))[:, :3]
    return b


def wall(fn, rounds, warm=1):
    import torch
    ts = []
    for i in range(rounds + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(time.perf_counter() - t0)
    return ts


def stat(ts, scale):
    return {"median": scale * statistics.median(ts), "min": scale * min(ts), "max": scale * max(ts)}


def section_a(rounds, iters):
    import numpy as np
    import torch
    s, scene = build_scene()
    poses = path_poses(s, iters)
    poses_d = torch.from_numpy(poses.astype(np.float32)).to(scene.device)
    train = np.arange(N_FRAMES)[1::2]
    routes = {"sample_pose": lambda i: scene.sample_pose(poses_d, i, V, unpreprocess=True), "host": lambda i: host_batch(s, scene, poses[i], train)}
    res = {"iters": iters, "candidates": len(train)}
    for name, fn in routes.items():
        loop = lambda: [fn(i) for i in range(iters)]                                 # noqa: E731
        res[name + "_host_us"] = stat(wall(loop, rounds), 1e6 / iters)
        ev = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            loop()
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b) * 1e-3)
        res[name + "_event_us"] = stat(ev, 1e6 / iters)
    # one launch alone between two events (the kernel and its launch, nothing else on the stream)
    one = []
    for i in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        scene.sample_pose(poses_d, i % iters, V, unpreprocess=True)
        b.record()
        torch.cuda.synchronize()
        one.append(a.elapsed_time(b) * 1e-3)
    res["sample_pose_single_event_us"] = stat(one[5:], 1e6)
    got, want = scene.sample_pose(poses_d, 3, V, unpreprocess=True), host_batch(s, scene, poses[3], train)
    res["same_sources"] = sorted(got["view_ids"][0, 1:].tolist()) == sorted(want["view_ids"][0, 1:].tolist()) or got["view_ids"][0, 1:].tolist()
    res["max_abs_diff_affine_mat_inv_slot0"] = float((got["affine_mat_inv"][0, 0] - want["affine_mat_inv"][0, 0]).abs().max())
    return res


def section_b(rounds):
    import numpy as np
    import torch
    from uc_nerf_amd.network.mvs_models import CascadeMVSNet
    from uc_nerf_amd.system import UCNeRFSystem
    from uc_nerf_amd.validate import render_novel_view
    s, scene = build_scene()
    args = types.SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=6, netwidth=128, net_type="v2", view_num=V, netchunk=1024, perturb=1.0,
                                 N_samples=90, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0, ckpt=None, device="cuda", img_downscale=1.0,
                                 use_color_volume=False, chunk=4096, pad=0, batch_size=1024, patch_num=4, patch_size=8, lrate=5e-4, num_epochs=4,
                                 finetune=None, log=False, basedir=".", expname="timing", num_train_samples=8, pts_dim=3, dir_dim=3)
    torch.manual_seed(0)
    system = UCNeRFSystem(args, [scene], network_mvs=CascadeMVSNet.with_cnns(view_num=V))
    poses = path_poses(s, PATH)
    poses_d = torch.from_numpy(poses.astype(np.float32)).to(scene.frames.device)
    train = np.arange(N_FRAMES)[1::2]
    net = system.Consist_Learner

    def composed():
        net.train()
        return [render_novel_view(args, host_batch(s, scene, poses[j], train), net, system.render_kwargs_train) for j in range(PATH)]

    res = {"poses": PATH, "chunk": args.chunk}
    res["render_path_ms"] = stat(wall(lambda: system.render_path(scene, poses_d), rounds), 1e3 / PATH)
    res["host_composed_ms"] = stat(wall(composed, rounds), 1e3 / PATH)
    res["render_path_again_ms"] = stat(wall(lambda: system.render_path(scene, poses_d), rounds), 1e3 / PATH)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default=None, help="(internal) run one section in this process")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.section:
        out = section_a(a.rounds, a.iters) if a.section == "a" else section_b(a.rounds)
        print("RESULT " + json.dumps(out))
        sys.exit(0)
    result = {"image": [H, W], "views": V, "frames": N_FRAMES, "rounds": a.rounds}
    for section, limit in LIMITS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--section", section, "--rounds", str(a.rounds),
                            "--iters", str(a.iters)], capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        result[section] = json.loads(line[-1][7:]) if r.returncode == 0 and line else {"failed": r.returncode, "stderr": r.stderr[-1500:]}
        if r.returncode != 0:
            break                                                                    # a section that failed or ran out of time: nothing more is started
    print(json.dumps(result))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
