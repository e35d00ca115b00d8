"""`uc_nerf_amd.system.UCNeRFSystem` on the device, on the tiny scene of tests/system_cases.py (32 x 32, V = 3, ndepths [48, 32, 8], batch_size 32 =
two 4 x 4 patches, 12 samples a ray, chunk 300): the training step against the same step composed by hand from the public mirrors (torch
indexing for train.py:166-176), two optimiser steps, a validation image against a direct `render_validation_image`, the validation epoch's
end against direct calls of the metric mirrors, `fit`'s results, and the step under torch's synchronisation check.

The system runs `build_rays` on its one-launch route; the hand composition selects the same route through the public switch
(`set_build_rays_fused(True)`), so both sides issue the same launches on the same inputs.

Bars.  Forward values (the loss and its five parts, the validation images) are compared bit for bit.  Gradients cannot be: the gather's
backward and the dense weight gradient accumulate with float32 atomics whose order is not fixed from run to run (profiles/mlp_scale.md,
"Same call twice"), and with torch's CNN routes torch's own convolution backward is in the chain.  What the two compositions may differ by
is therefore the re-ordering of the same float32 terms.  A gradient element is a sum of at most N terms with N about 1e4 here (332 rays x 12
samples for an MLP weight; at most 32 x 32 x 8 = 8192 output voxels for a convolution weight), two orders of one such sum differ by at most
2 (N - 1) u sum|t| with u = 2^-24, and that error passes linearly through the rest of the backward chain: 2 * 1e4 * 6e-8 = 1.2e-3 relative
to the terms' magnitude.  The bar is max |g_a - g_b| <= 1e-3 max |g| per tensor (the terms' magnitude taken as the tensor's largest gradient;
a typical random re-ordering error, sqrt(N) u, is two orders below it).  A composition that gathered other targets, weighted a loss part
otherwise or dropped one changes gradients by a fraction of their size, not by a thousandth.  A second step's loss follows parameters that
went through an Adam step on such gradients: the bar tests/test_hip_round4.py::test_graphed_training_step_follows_the_eager_one uses for an
eager step against an eager step, 1e-4 max(1, |loss|)."""
import numpy as np
import pytest
import torch

import system_cases as YC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PARTS = ("img_loss", "loss_nerf_depth", "loss_mvs", "smooth_loss", "loss_scaleinvariant")
_scene = {}


def scene():
    if "s" not in _scene:
        _scene["s"] = YC.tiny_scene(DEV)
    return _scene["s"]


def make_system(seed=0, mvs=None, scenes=None, build_rays_fused=True, **over):
    from uc_nerf_amd.system import UCNeRFSystem
    torch.manual_seed(seed)
    return UCNeRFSystem(YC.tiny_args(DEV, **over), scenes or [scene()], network_mvs=YC.tiny_mvs(**(mvs or {})), build_rays_fused=build_rays_fused)


def reseed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def sample(target=1, src=(3, 5), seed=11):
    n = scene().n_keypoints(target)
    perm = torch.from_numpy(np.random.RandomState(seed).permutation(n).astype(np.int32)).to(DEV)
    return scene().sample(target, list(src), perm=perm, unpreprocess=True)


def hand_step(system, batch):
    """train.py:110-188 from the public mirrors: the cascade, build_rays, rendering, torch indexing for lines 166-176, training_loss."""
    from uc_nerf_amd.network.renderer import rendering
    from uc_nerf_amd.utils.loss import training_loss
    from uc_nerf_amd.utils.utils import build_rays, set_build_rays_fused
    args = system.args
    batch = dict(batch)
    depth_sparse_ms, weight_ms = batch.pop("sparse_depths_ms"), batch.pop("weight_ms")
    batch.pop("scan")
    data = {k: v.float() for k, v in batch.items()}
    pose_ref = {k: data[k].squeeze() for k in ("w2cs", "intrinsics", "c2ws", "near_fars")}
    near_fars = pose_ref["near_fars"]
    depth_coord = torch.transpose(data["rays_depth"].squeeze(0), 0, 1)[2, :, 0:2]
    _, conf, _, outputs = system.Consist_Learner(data["images"][:, 1:], data["affine_mat"][0], data["affine_mat_inv"][0], near_fars[0], pad=args.pad)
    imgs = system.unpreprocess(data["images"])                                            # the reference's own un-normalisation, not the sample's
    assert torch.equal(imgs, data["images_unpre"])
    N_rays = args.batch_size
    prev = set_build_rays_fused(True)                                                     # the route the system takes, through the public switch
    try:
        pts, dirs, target_s, ndc, z, _, _, ndc_par, pix = build_rays(args, imgs, conf, data["sparse_depths"], depth_coord, pose_ref, pose_ref["w2cs"],
                                                                     pose_ref["c2ws"], pose_ref["intrinsics"], N_rays, args.N_samples, pad=args.pad,
                                                                     with_depth=True, outputs=outputs)
    finally:
        set_build_rays_fused(prev)
    rgb, depth_pred = rendering(args, pose_ref, pts, ndc, z, dirs, outputs, imgs[:, 1:], near_fars=near_fars[0], img_feat=outputs["stage3"]["img_feats"],
                                confidence=conf, ndc_parameters=ndc_par, **system.render_kwargs_train)
    patch_pts = args.patch_num * args.patch_size ** 2
    pix = pix.long()
    target_depths = data["sparse_depths"][:, pix[0, N_rays:], pix[1, N_rays:]]
    target_weights = data["sparse_depths_weight"][:, pix[0, N_rays:], pix[1, N_rays:]]
    patch_dpt = data["dpt"][:, pix[0, :patch_pts], pix[1, :patch_pts]].reshape(-1, args.patch_size, args.patch_size, 1)
    return training_loss(rgb, depth_pred, target_s, target_depths, target_weights, patch_dpt, outputs, depth_sparse_ms, weight_ms, n_rays=N_rays,
                         patch_num=args.patch_num, patch_size=args.patch_size, mvs_on_device=True)


def grads_of(system):
    return [None if p.grad is None else p.grad.detach().clone() for p in system.grad_vars]


# ------------------------------------------------------------------------------------------------ 1. composition
def test_training_step_is_the_hand_composed_step():
    system = make_system()
    batch = sample()
    reseed(21)
    out = system.training_step(batch, 0)
    assert set(out) == {"loss", "psnr"} | set(PARTS) and all(torch.is_tensor(v) and v.is_cuda for v in out.values())
    out["loss"].backward()
    got = grads_of(system)
    for p in system.grad_vars:
        p.grad = None
    reseed(21)
    loss, parts = hand_step(system, batch)
    loss.backward()
    want = grads_of(system)
    print("loss %r hand %r" % (float(out["loss"]), float(loss)))
    assert torch.isfinite(loss) and torch.equal(out["loss"], loss)
    for k in PARTS:
        assert torch.equal(out[k], parts[k]), k
    assert float(out["psnr"]) == pytest.approx(-10.0 * np.log10(float(parts["img_loss"])), rel=1e-5)
    assert [g is None for g in got] == [w is None for w in want] and sum(g is not None for g in got) > 20
    unequal = sum(1 for g, w in zip(got, want) if g is not None and not torch.equal(g, w))
    print("gradients that are not bit-equal between the two compositions: %d of %d" % (unequal, sum(g is not None for g in got)))
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        scale, diff = float(torch.maximum(g.abs().max(), w.abs().max())), float((g - w).abs().max())
        worst = max(worst, diff / scale if scale else 0.0)
        assert diff <= 1e-3 * scale, (k, tuple(g.shape), diff, scale)
    print("largest max|g_a - g_b| / max|g| over the tensors: %.3g" % worst)
    from uc_nerf_amd import ops
    assert ops.step_targets_status() == 0 and ops.loss_status() == 0


# ------------------------------------------------------------------------------------------------ 2. two steps
@pytest.mark.parametrize("finetune", [None, True], ids=["all", "finetune"])
def test_two_steps_move_the_parameters_and_follow_the_hand_composition(finetune):
    system, twin = make_system(finetune=finetune), make_system(finetune=finetune)
    for (k, a), (_, b) in zip(system.Consist_Learner.state_dict().items(), twin.Consist_Learner.state_dict().items()):
        assert torch.equal(a, b), k
    for s in (system, twin):
        s.configure_optimizers()
    metas = [(0, 1, [3, 5]), (0, 3, [5, 1])]
    before = [p.detach().clone() for p in system.grad_vars]
    mvs_before = [p.detach().clone() for p in system.Consist_Learner.parameters()]
    losses = {"system": [], "hand": []}
    for step, (_, target, src) in enumerate(metas):
        batch = sample(target, src, seed=30 + step)
        reseed(40 + step)
        system.optimizer.zero_grad(set_to_none=True)                                        # fit's inner loop (`_train_visit`) on a fixed sample
        out = system.training_step(batch, step)
        out["loss"].backward()
        system.optimizer.step()
        system.global_step += 1
        losses["system"].append(float(out["loss"]))
        reseed(40 + step)
        twin.optimizer.zero_grad(set_to_none=True)
        loss, _ = hand_step(twin, batch)
        loss.backward()
        twin.optimizer.step()
        losses["hand"].append(float(loss))
        if step == 0:
            # every tensor with a gradient has changed -- except one whose gradient is zero in every element (a bias in front of a batch-norm, the
            # MLP's three parameters kept for checkpoint compatibility): Adam without weight decay cannot move it, and it must not have moved
            with_grad = [(p, b) for p, b in zip(system.grad_vars, before) if p.grad is not None]
            live = [(p, b) for p, b in with_grad if bool((p.grad != 0).any())]
            print("tensors with a gradient: %d, of them with a non-zero one: %d" % (len(with_grad), len(live)))
            assert len(live) > 20 and all(not torch.equal(p.detach(), b) for p, b in live)
            assert len(with_grad) - len(live) <= 3, [tuple(p.shape) for p, _ in with_grad if not bool((p.grad != 0).any())]      # (no room to hide a dead branch)
            assert all(torch.equal(p.detach(), b) for p, b in with_grad if not bool((p.grad != 0).any()))
            mvs_moved = [not torch.equal(p.detach(), b) for p, b in zip(system.Consist_Learner.parameters(), mvs_before)]
            assert not any(mvs_moved) if finetune else any(mvs_moved)
    print("losses", losses)
    assert losses["system"][0] == losses["hand"][0]
    assert abs(losses["system"][1] - losses["hand"][1]) < 1e-4 * max(1.0, abs(losses["hand"][1]))
    assert system.global_step == 2


# ------------------------------------------------------------------------------------------------ 3. validation
def test_validation_step_is_render_validation_image_and_leaves_the_cascade_training():
    from uc_nerf_amd.validate import render_validation_image
    system = make_system()
    assert (YC.H * YC.W) % system.args.chunk != 0                                           # a partial last chunk
    batch = scene().sample(0, [1, 3], unpreprocess=True)
    net = system.Consist_Learner.eval()
    name, running = next((n, b) for n, b in net.named_buffers() if n.endswith("running_mean"))
    was = running.clone()
    reseed(5)
    log = system.validation_step(batch, 0)
    assert net.training and not torch.equal(running, was), name                             # train() and never back: the running mean moved
    assert system.validation_step_outputs == [log] and system.idx == 1
    b = dict(batch)
    for k in ("scan", "sparse_depths_ms", "weight_ms"):
        b.pop(k)
    data, pose_ref = system.decode_batch(b)
    near_fars = pose_ref["near_fars"]
    reseed(5)
    with torch.no_grad():
        _, conf, _, outputs = net(data["images"][:, 1:], data["affine_mat"][0], data["affine_mat_inv"][0], near_fars[0], pad=system.args.pad)
    imgs = data["images_unpre"]
    want = render_validation_image(system.args, pose_ref, outputs, imgs[:, 1:], conf, YC.H, YC.W, near_fars, system.render_kwargs_train,
                                   depth_gt=data["depths_h"][0], gt_rgb=imgs[0, 0])
    for k in ("pred_rgb", "pred_depth", "mask", "pred_depth_vis", "uncertainty", "gt_rgb", "gt_depth"):
        assert torch.equal(log[k], want[k]), k
    assert log["pred_rgb"].shape == (3, YC.H, YC.W) and bool(log["mask"].all())


# ------------------------------------------------------------------------------------------------ 4. the epoch's end
def test_validation_epoch_end_single_image_and_grouped_by_scan():
    from uc_nerf_amd.utils.evaluation import depth_evaluation, rgb_evaluation
    system = make_system(scenes=[scene(), scene()])
    reseed(6)
    log = system.validation_step(scene().sample(2, [1, 3], unpreprocess=True), 0)
    result = system.on_validation_epoch_end()
    assert set(result) == {"val/PSNR", "val/SSIM", "val/LPIPS", "val/abs_rel", "val/sq_rel", "val/rmse", "val/rmse_log", "val/a1", "val/a2", "val/a3"}
    assert np.isnan(result["val/LPIPS"]) and all(np.isfinite(v) for k, v in result.items() if k != "val/LPIPS")
    assert system.validation_step_outputs == []
    # 12 images over two scans: ten in the first group, two in the second
    g = torch.Generator().manual_seed(8)
    logs = []
    for i in range(12):
        noise = torch.rand(log["pred_rgb"].shape, generator=g).to(DEV)
        logs.append(dict(log, pred_rgb=(log["pred_rgb"] * 0.5 + 0.5 * noise), pred_depth=log["pred_depth"] * (1.0 + 0.05 * i) + 0.01 * noise[0]))
    system.validation_step_outputs = list(logs)
    result = system.on_validation_epoch_end()
    stack = lambda k, sl: torch.stack([x[k] for x in logs[sl]])                              # noqa: E731
    rgb, depth = [], []
    for sl in (slice(0, 10), slice(10, 20)):
        rgb.append([float(v) for v in rgb_evaluation(stack("gt_rgb", sl), stack("pred_rgb", sl), None)])
        depth.append(depth_evaluation(stack("gt_depth", sl), stack("pred_depth", sl), pred_masks=stack("mask", sl)))
    want = list(np.stack(rgb).mean(0)) + list(np.stack(depth).mean(0))
    got = [result[k] for k in ("val/PSNR", "val/SSIM", "val/LPIPS", "val/abs_rel", "val/sq_rel", "val/rmse", "val/rmse_log", "val/a1", "val/a2", "val/a3")]
    assert np.isnan(got[2]) and [a for i, a in enumerate(got) if i != 2] == [float(b) for i, b in enumerate(want) if i != 2]
    assert rgb[0] != rgb[1] and system.validation_step_outputs == []


# ------------------------------------------------------------------------------------------------ 5. fit
def test_fit_two_epochs_validates_once_and_steps_the_schedule():
    from uc_nerf_amd import ops
    system = make_system(num_train_samples=3, num_epochs=4)
    one = system.val_metas()[:1]
    system.val_metas = lambda: one
    ops.step_targets_status_clear()
    reseed(9)
    results = system.fit(max_epochs=2, seed=4)
    assert len(results) == 1 and np.isfinite(results[0]["val/PSNR"]) and system.global_step == 6 and system.current_epoch == 1
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([{"params": [p], "lr": system.args.lrate}], betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4, eta_min=1e-7)
    for _ in range(2):
        opt.step(), sched.step()
    assert system.optimizer.param_groups[0]["lr"] == opt.param_groups[0]["lr"] < system.args.lrate
    assert ops.step_targets_status() == 0


# ------------------------------------------------------------------------------------------------ 6. no host read
def test_training_step_reads_nothing_back():
    """One whole step as `fit` runs it -- training_step, backward, optimizer.step() -- under torch.cuda.set_sync_debug_mode("error"), with
    log_fn=None, on the system as it is constructed by default: nothing raises.  (A system built with build_rays_fused=False goes through the
    composed `build_rays` and does read back; the last lines show that the check sees it.)"""
    system = make_system()
    assert system.log_fn is None and system.build_rays_fused
    system.configure_optimizers()
    batch = sample()
    for _ in range(2):                                                                     # warm: caches, packed weights, Adam's state
        reseed(3)
        system.optimizer.zero_grad(set_to_none=True)
        system.training_step(batch, 0)["loss"].backward()
        system.optimizer.step()
    system.optimizer.zero_grad(set_to_none=True)
    reseed(3)
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        out = system.training_step(batch, 1)
        out["loss"].backward()
        system.optimizer.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.isfinite(out["loss"])
    composed = make_system(build_rays_fused=False)
    composed.training_step(batch, 0)
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError, match="synchronizing"):
            composed.training_step(batch, 1)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
