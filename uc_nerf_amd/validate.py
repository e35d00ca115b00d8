"""One whole validation image on the device: the body of the reference's validation_step (train.py:249-289) without its host round trips.

The reference renders an image in chunks, pulls every chunk to the host, concatenates, clamps and permutes there, and colours two depth maps
with cv2 + PIL.  Here a chunk goes from `rendering()` straight into the image planes (ucnerf_image_put: clamp, transpose and the depth range in
one launch), the depth pictures are one launch each (ucnerf_depth_colormap), and everything returned is a device tensor that
`utils.evaluation.rgb_evaluation` / `depth_evaluation` take as it is -- a validation image costs the one small read those make.
Nothing in this module reads the device back.

All three metrics of a validation epoch from the images this module returns (LPIPS needs the two checkpoints, nothing else):
    lpips_fn = uc_nerf_amd.utils.evaluation.LPIPS.from_files(alexnet_path, lpips_alex_lin_path)      # once; packs the weights
    psnr, ssim, lpips = rgb_evaluation(torch.stack(gt_rgbs), torch.stack(pred_rgbs), savedir, lpips_fn=lpips_fn)
"""
import torch

from . import ops
from .network.renderer import rendering
from .utils.utils import _device_table, build_rays_test, visualize_depth


def render_validation_image(args, pose_ref, outputs, imgs_input, photo_confidence, H, W, near_fars, render_kwargs, network_fn=None, depth_gt=None,
                            gt_rgb=None, cmap=None):
    """train.py:249-289.  The reference's chunk loop -- H W // args.chunk chunks and a partial last one, `build_rays_test` then `rendering` with
    its arguments (img_feat = outputs["stage3"]["img_feats"], confidence = photo_confidence, **render_kwargs), including rendering's in-place
    trim of `pose_ref` -- under torch.no_grad().  -> the reference's log dict, every value a device tensor:
        pred_rgb [3,H,W] clamped to [0, 1], pred_depth [H,W];  with gt_rgb: gt_rgb;  with depth_gt [H,W]: gt_depth, mask = gt_depth > 0;
    and three more keys: pred_depth_vis [3,H,W] (visualize_depth of pred_depth, its range taken from the cell the chunks were folded into),
    gt_depth_vis (with depth_gt), uncertainty [H,W] = network_fn.forward_uncertainty(photo_confidence) (network_fn defaults to
    render_kwargs["network_fn"]).  `cmap`: a 256 x 3 uint8 table, default utils.colormaps.jet_lut()."""
    H, W = int(H), int(W)
    net = network_fn if network_fn is not None else render_kwargs["network_fn"]
    log = {}
    with torch.no_grad():
        world_to_ref = pose_ref['w2cs'][0]
        tgt_to_world, intrinsic = pose_ref['c2ws'][0], pose_ref['intrinsics'][0]
        dev = tgt_to_world.device
        render_rgb = torch.empty(3, H, W, device=dev)
        render_depth = torch.empty(H, W, device=dev)
        cell = ops.minmax_reset(device=dev)
        for chunk_idx in range(H * W // args.chunk + int(H * W % args.chunk > 0)):
            rays_pts, rays_dir, rays_NDC, depth_candidates, rays_o, ndc_parameters = build_rays_test(
                H, W, tgt_to_world, world_to_ref, intrinsic, near_fars, near_fars[-1], args.N_samples, pad=args.pad, chunk=args.chunk,
                idx=chunk_idx, outputs=outputs)
            rgb, depth_pred = rendering(args, pose_ref, rays_pts, rays_NDC, depth_candidates, rays_dir, outputs, imgs_input,
                                        near_fars=near_fars[0], img_feat=outputs["stage3"]['img_feats'], confidence=photo_confidence,
                                        ndc_parameters=ndc_parameters, **render_kwargs)
            ops.image_put(rgb, depth_pred, chunk_idx * args.chunk, render_rgb, render_depth, cell)
        table = _device_table(cmap, dev)
        log['pred_depth'] = render_depth
        log['pred_rgb'] = render_rgb
        if gt_rgb is not None:
            log['gt_rgb'] = gt_rgb.to(dev)
        if depth_gt is not None:
            depth_gt = depth_gt.to(dev)
            log['gt_depth'] = depth_gt
            log['mask'] = depth_gt > 0
            log['gt_depth_vis'] = visualize_depth(depth_gt, cmap=table)
        log['pred_depth_vis'] = ops.depth_colormap(render_depth, table, minmax=cell, want_index=False)[1]
        log['uncertainty'] = net.forward_uncertainty(photo_confidence.reshape(1, -1, 1)).reshape(H, W)
    return log


def render_novel_view(args, batch, network_mvs, render_kwargs, network_fn=None, cmap=None):
    """One image of a FREE camera pose: `batch` is `DeviceScene.sample_pose(...)`'s (slot 0 the pose, slots 1.. the source views picked on the
    device).  The cascade `network_mvs` runs on batch["images"][:, 1:] with slot 0's stage matrices as validation_step runs it (train.py:233-237;
    the module's mode is the caller's: `UCNeRFSystem.render_path` sets the one validation uses), then `render_validation_image`'s chunk loop on
    the un-normalised source images (batch["images_unpre"] when the batch carries it, train.py:61-70 applied here otherwise).  No gt_rgb, no
    depth_gt: a free pose has neither.  -> (pred_rgb [3,H,W] clamped to [0, 1], pred_depth [H,W], pred_depth_vis [3,H,W]), device tensors;
    nothing is read back."""
    with torch.no_grad():
        data = {k: v.float() for k, v in batch.items() if k != "scan"}
        pose_ref = {k: data[k].squeeze() for k in ("w2cs", "intrinsics", "c2ws", "near_fars")}
        near_fars = pose_ref["near_fars"]
        imgs = data["images"]
        H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
        _, photo_confidence, _, outputs = network_mvs(imgs[:, 1:], data["affine_mat"][0], data["affine_mat_inv"][0], near_fars[0], pad=args.pad)
        if "images_unpre" in data:
            imgs = data["images_unpre"]
        else:
            dev = imgs.device
            mean = torch.tensor([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]).view(1, 1, 3, 1, 1).to(dev)
            std = torch.tensor([1 / 0.229, 1 / 0.224, 1 / 0.225]).view(1, 1, 3, 1, 1).to(dev)
            imgs = (imgs - mean) / std
        log = render_validation_image(args, pose_ref, outputs, imgs[:, 1:], photo_confidence, H, W, near_fars, render_kwargs, network_fn=network_fn,
                                      cmap=cmap)
    return log["pred_rgb"], log["pred_depth"], log["pred_depth_vis"]
