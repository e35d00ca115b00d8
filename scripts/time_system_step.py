"""Times of `uc_nerf_amd.system.UCNeRFSystem` on one synthetic scene at 256 x 320, V = 7, batch_size 1024, 4 patches of 8 x 8, --pad 0:
  (a) ops.step_targets against the torch indexing it replaces (train.py:166-176), same tensors, same process: device-event medians over
      batches of 50 calls (torch's route is timed before and after, so that its two columns show the spread), and the library launches the
      op issues, counted at _lib.call (torch's own launches are NOT counted: that needs a profiler run);
  (b) one whole training step (sample, training_step, backward, Adam) for training="torch" and training="device" CNNs, host clock per step
      ending in a synchronise, and its stages timed the same way one after the other (each stage closed by a synchronise, so the stages
      add up to more than the step);
  (c) one validation_step.
Each section runs in a child process under its own time limit.  Prints one JSON line (--json FILE keeps it): profiles/system_step.md is
written from it.  Needs a GPU: there is no fallback."""
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

H, W, V, N_FRAMES, KP = 256, 320, 7, 14, 1024
LIMITS = {"a": 120, "b_torch": 300, "b_device": 300, "c": 200}


def build(training):
    import torch
    import sample_cases as SC
    from uc_nerf_amd.data.scene import DeviceScene
    from uc_nerf_amd.network.mvs_models import CascadeMVSNet
    from uc_nerf_amd.system import UCNeRFSystem
    dev = torch.device("cuda")
    s = SC.make_scene(H, W, (KP,) * N_FRAMES, seed=5)
    scene = DeviceScene.from_arrays(s["poses"], s["focal"], s["bounds"], s["sparse"], s["frames"], s["dpt"], s["depths_h"] + 0.5, device=dev)
    args = types.SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=6, netwidth=128, net_type="v2", view_num=V, netchunk=1024, perturb=1.0,
                                 N_samples=90, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0, ckpt=None, device="cuda", img_downscale=1.0,
                                 use_color_volume=False, chunk=4096, pad=0, batch_size=1024, patch_num=4, patch_size=8, lrate=5e-4, num_epochs=4,
                                 finetune=None, log=False, basedir=".", expname="timing", num_train_samples=8, pts_dim=3, dir_dim=3)
    kw = {} if training == "torch" else dict(training="device", feature_training="device", batch_stats="device")
    torch.manual_seed(0)
    system = UCNeRFSystem(args, [scene], network_mvs=CascadeMVSNet.with_cnns(view_num=V, **kw))
    system.configure_optimizers()
    return system, scene


def wall(fn, rounds, warm=2):
    import torch
    ts = []
    for i in range(rounds + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}, out


def section_a(rounds):
    import torch
    from uc_nerf_amd import _lib, ops
    system, scene = build("torch")
    b = scene.sample(1, [3, 5, 7, 9, 11, 13])
    sd, sw, dpt = b["sparse_depths"], b["sparse_depths_weight"], b["dpt"]
    g = torch.Generator().manual_seed(1)
    n_rays, patch_num, ps = 1024, 4, 8
    n_total = n_rays + KP
    pix = torch.stack([torch.randint(0, H, (n_total,), generator=g), torch.randint(0, W, (n_total,), generator=g)]).cuda()
    P = patch_num * ps * ps

    def torch_route():
        return (sd[:, pix[0, n_rays:], pix[1, n_rays:]], sw[:, pix[0, n_rays:], pix[1, n_rays:]], dpt[:, pix[0, :P], pix[1, :P]].reshape(-1, ps, ps, 1))

    def device_route():
        return ops.step_targets(sd, sw, dpt, pix, n_rays, patch_num, ps)

    same = all(torch.equal(a, c) for a, c in zip(torch_route(), device_route()))
    counted = []
    real = _lib.call
    _lib.call = lambda name, params, stream: counted.append(name) or real(name, params, stream)
    device_route()
    _lib.call = real
    res = {"same_bits": bool(same), "library_launches": counted, "calls_per_batch": 50}
    for name, fn in (("torch", torch_route), ("step_targets", device_route), ("torch_again", torch_route)):
        per = []
        for i in range(rounds + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                per.append(1e3 * e0.elapsed_time(e1) / 50)                   # us per call, launch-to-launch on the stream
        res[name + "_us"] = {"median": statistics.median(per), "min": min(per), "max": max(per)}
    return res


def section_b(training, rounds):
    import numpy as np
    import torch
    system, scene = build(training)
    metas = system.train_metas(np.random.default_rng(0))
    k = [0]

    def step():
        k[0] += 1
        return system._train_visit(metas[k[0] % len(metas)], k[0])

    res = {"step_ms": wall(step, rounds, warm=3)[0]}
    # the stages, each closed by a synchronise: the step's own code cut at its seams
    from uc_nerf_amd import ops
    from uc_nerf_amd.network.renderer import rendering
    from uc_nerf_amd.utils.loss import training_loss
    a = system.args
    st = {n: [] for n in ("sample", "cascade", "build_rays", "rendering", "targets_loss", "backward", "optimizer")}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        st[name].append(1e3 * (time.perf_counter() - t0))
        return out

    for i in range(rounds + 2):
        _, target, src = metas[i % len(metas)]
        batch = timed("sample", lambda: scene.sample(target, src, unpreprocess=True))
        system.optimizer.zero_grad(set_to_none=True)
        bb = dict(batch)
        ms, wm = bb.pop("sparse_depths_ms"), bb.pop("weight_ms")
        bb.pop("scan")
        d, pose = system.decode_batch(bb)
        nf = pose["near_fars"]
        _, conf, _, outputs = timed("cascade", lambda: system.Consist_Learner(d["images"][:, 1:], d["affine_mat"][0], d["affine_mat_inv"][0], nf[0], pad=a.pad))
        imgs = d["images_unpre"]
        coord = torch.transpose(d["rays_depth"].squeeze(0), 0, 1)[2, :, 0:2]
        r = timed("build_rays", lambda: system._build_rays(a, imgs, conf, d["sparse_depths"], coord, pose, pose["w2cs"], pose["c2ws"], pose["intrinsics"],
                                                           a.batch_size, a.N_samples, pad=a.pad, with_depth=True, outputs=outputs))
        rgb, depth = timed("rendering", lambda: rendering(a, pose, r[0], r[3], r[4], r[1], outputs, imgs[:, 1:], near_fars=nf[0],
                                                          img_feat=outputs["stage3"]["img_feats"], confidence=conf, ndc_parameters=r[7],
                                                          **system.render_kwargs_train))

        def targets_loss():
            td, tw, pd = ops.step_targets(d["sparse_depths"], d["sparse_depths_weight"], d["dpt"], r[8], a.batch_size, a.patch_num, a.patch_size)
            return training_loss(rgb, depth, r[2], td, tw, pd, outputs, ms, wm, n_rays=a.batch_size, patch_num=a.patch_num, patch_size=a.patch_size,
                                 mvs_on_device=True)[0]
        loss = timed("targets_loss", targets_loss)
        timed("backward", loss.backward)
        timed("optimizer", system.optimizer.step)
    res["stages_ms"] = {n: statistics.median(v[2:]) for n, v in st.items()}
    res["loss"] = float(loss.detach())
    res["step_targets_status"] = ops.step_targets_status()
    return res


def section_c(rounds):
    system, scene = build("torch")
    metas = system.val_metas()
    batch = scene.sample(metas[0][1], metas[0][2], unpreprocess=True)

    def val():
        system.validation_step_outputs = []
        return system.validation_step(batch, 0)

    t, log = wall(val, rounds, warm=1)
    return {"validation_step_ms": t, "chunk": system.args.chunk, "chunks": -(-H * W // system.args.chunk)}


def child(section, rounds):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_system_step: no GPU (there is no fallback)")
    res = {"a": lambda: section_a(rounds), "b_torch": lambda: section_b("torch", rounds), "b_device": lambda: section_b("device", rounds),
           "c": lambda: section_c(max(3, rounds // 3))}[section]()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--section", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.section:
        return child(a.section, a.rounds)
    result = {"image": [H, W], "views": V, "batch_size": 1024, "patches": "4 x 8 x 8", "rounds": a.rounds}
    for section, limit in LIMITS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--section", section, "--rounds", str(a.rounds)],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        result[section] = json.loads(line[-1][7:]) if r.returncode == 0 and line else {"failed": r.returncode, "stderr": r.stderr[-1500:]}
        if r.returncode in (124, 134, 137, 139, -6, -11):                                    # a fault or a time limit: nothing more is started on the device
            break
    print(json.dumps(result))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
