"""`UCNeRFSystem`: the reference's train / validate loop (train.py:26-414) as a plain class over this package's mirrors, without Lightning.

The method names and bodies are the reference's; what differs is listed here, once:
  * the data comes from `DeviceScene`s (one launch per sample) instead of a `DataLoader`;
  * the step's three target gathers (train.py:166-176) are one launch, `ops.step_targets`: a pixel coordinate outside the image gives NaN and
    a bit of a sticky status word (`ops.step_targets_status()`) where torch's indexing raises a device-side assert;
  * the loss is `training_loss(..., mvs_on_device=True)`: the cascade term keeps its counts on the device;
  * `training_step` returns device tensors and reproduces none of the reference's `.item()` calls; `log_fn`, when given, is called every
    `log_every` steps and may read back -- the only read in training that this module asks for;
  * `build_rays` runs on its one-launch route (`utils.utils._build_rays_fused`: the reference's draws, then ucnerf_build_rays_train; the
    same 9-tuple bit for bit) wherever that route takes the shapes, whatever the module-wide switch `set_build_rays_fused` says: on it a
    whole step -- training_step, backward, optimizer.step() -- passes torch's synchronisation check in "error" mode.  With
    `build_rays_fused=False`, or with shapes that route does not take (patch_size larger than half the image, N_samples no multiple of 3 or
    above 768), the step goes through the composed `build_rays`, which reads the device back about twenty times a step (each patch's cell
    through int(), the camera matrices through `.cpu()`: profiles/system_step.md);
  * a validation image is `render_validation_image` (nothing pulled to the host per chunk); the matplotlib figure is written only with
    `savefig=True`;
  * the metrics are the device mirrors; LPIPS is NaN unless an `lpips_fn` is given (`utils.evaluation.LPIPS`);
  * `fit` / `validate` stand for Lightning's `Trainer` as train.py:434-447 configures it.
Nothing here captures or replays a HIP graph.  Importing this module needs no GPU.
"""
import os

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR

from . import ops
from .network.models import create_ucnerf
from .network.mvs_models import CascadeMVSNet
from .network.renderer import rendering
from .utils.evaluation import depth_evaluation, rgb_evaluation
from .utils.loss import EdgePreservingSmoothnessLoss, GradientLoss, training_loss
from .utils.utils import _build_rays_fused, _fused_takes, build_rays, filter_keys, sub_selete_data
from .validate import render_validation_image

VAL_KEYS = ('val/PSNR', 'val/SSIM', 'val/LPIPS', 'val/abs_rel', 'val/sq_rel', 'val/rmse', 'val/rmse_log', 'val/a1', 'val/a2', 'val/a3')


class UCNeRFSystem:
    """train.py:26-414.  args: the opt.py namespace (`args.device`, when present, is where the modules are created); train_scenes / val_scenes:
    lists of `DeviceScene` (val_scenes defaults to the training scenes, as the reference's two datasets read the same scans); network_mvs: the
    consistency learner, default `CascadeMVSNet.with_cnns(view_num=args.view_num)` -- pass one built with training="device" etc. for those
    routes; lpips_fn: handed to `rgb_evaluation`; log_fn(name, value, step): the logger, called every `log_every` training steps, and at a
    validation epoch's end when `args.log` is set (as the reference logs there); build_rays_fused: see the module's list of differences."""

    def __init__(self, args, train_scenes, val_scenes=None, network_mvs=None, lpips_fn=None, log_fn=None, log_every=100, build_rays_fused=True):
        self.args = args
        self.args.feat_dim = 24 + (args.view_num - 1) * (4 + 8) + 1
        self.learning_rate = args.lrate
        self.idx = 0
        self.global_step = 0
        self.current_epoch = 0
        self.validation_step_outputs = []
        self.train_scenes = list(train_scenes)
        self.val_scenes = list(val_scenes) if val_scenes is not None else self.train_scenes
        self.lpips_fn, self.log_fn, self.log_every = lpips_fn, log_fn, int(log_every)
        self.build_rays_fused = bool(build_rays_fused)
        self.device = torch.device(getattr(args, "device", None) or (self.train_scenes[0].device if self.train_scenes else "cuda"))
        if network_mvs is None:
            network_mvs = CascadeMVSNet.with_cnns(view_num=args.view_num)
        self.args.network_mvs = network_mvs.to(self.device)
        # Create ucnerf model
        self.render_kwargs_train, self.render_kwargs_test, start, self.grad_vars = create_ucnerf(args, dir_embedder=True, pts_embedder=True)
        # Create Consistency Learner
        self.Consist_Learner = self.render_kwargs_train['network_mvs']
        filter_keys(self.render_kwargs_train)
        self.smooth_loss = EdgePreservingSmoothnessLoss()
        self.edge_loss = GradientLoss()
        self.render_kwargs_train.pop('network_mvs')
        self.render_kwargs_train['NDC_local'] = False
        self.eval_metric = [0.01, 0.05, 0.1]
        self.optimizer = self.scheduler = None

    # ------------------------------------------------------------------------------------------------ train.py:49-92
    def decode_batch(self, batch, idx=list(torch.arange(4))):
        data_mvs = sub_selete_data(batch, self.device, idx, filtKey=[])
        pose_ref = {'w2cs': data_mvs['w2cs'].squeeze(), 'intrinsics': data_mvs['intrinsics'].squeeze(), 'c2ws': data_mvs['c2ws'].squeeze(),
                    'near_fars': data_mvs['near_fars'].squeeze()}
        return data_mvs, pose_ref

    def unpreprocess(self, data, shape=(1, 1, 3, 1, 1)):
        # to unnormalize image for visualization
        # data N V C H W
        device = data.device
        mean = torch.tensor([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]).view(*shape).to(device)
        std = torch.tensor([1 / 0.229, 1 / 0.224, 1 / 0.225]).view(*shape).to(device)
        return (data - mean) / std

    def _unpreprocessed(self, data_mvs):
        """train.py:142 / :245.  A `DeviceScene.sample(..., unpreprocess=True)` batch carries these very values from the sample's own launch
        (the same subtraction and IEEE division per element): they are used as they are, and `unpreprocess` is not applied on top of them."""
        if 'images_unpre' in data_mvs:
            return data_mvs['images_unpre']
        return self.unpreprocess(data_mvs['images'])

    def forward(self):
        return

    def configure_optimizers(self):
        eps = 1e-7
        variable_dict = [{"params": self.grad_vars, "lr": self.learning_rate}]
        self.optimizer = torch.optim.Adam(variable_dict, betas=(0.9, 0.999))
        self.scheduler = CosineAnnealingLR(self.optimizer, T_max=self.args.num_epochs, eta_min=eps)
        return [self.optimizer], [self.scheduler]

    def log(self, name, value, **kwargs):
        if self.log_fn is not None:
            self.log_fn(name, float(value), self.global_step)

    def _build_rays(self, args, imgs, mvs_confidence, sparse_depths, coords, pose_ref, w2cs, c2ws, intrinsics, N_rays, N_samples, pad=0, with_depth=False,
                    outputs=None):
        """`build_rays` (train.py:147-149), on its one-launch route when `build_rays_fused` is set and that route takes the shapes."""
        if self.build_rays_fused and with_depth and _fused_takes(args, imgs, N_samples):
            return _build_rays_fused(args, imgs, mvs_confidence, coords, pose_ref, c2ws, intrinsics, N_rays, N_samples, pad, False, 0, outputs)
        return build_rays(args, imgs, mvs_confidence, sparse_depths, coords, pose_ref, w2cs, c2ws, intrinsics, N_rays, N_samples, pad=pad,
                          with_depth=with_depth, outputs=outputs)

    # ------------------------------------------------------------------------------------------------ train.py:110-211
    def training_step(self, batch, batch_nb):
        """One step's loss.  -> {'loss', 'img_loss', 'psnr', 'loss_nerf_depth', 'loss_mvs', 'smooth_loss', 'loss_scaleinvariant'}, every value
        a device tensor ('loss' carries the graph).  On the one-launch route of `build_rays` (the default here, see the module's list) nothing
        in it reads the device back or blocks on a copy, unless `log_fn` is due or a checkpoint is; on the composed route `build_rays` does."""
        args = self.args
        batch = dict(batch)
        depth_sparse_ms = batch['sparse_depths_ms']
        weight_ms = batch['weight_ms']
        if 'scan' in batch.keys():
            batch.pop('scan')
            batch.pop('sparse_depths_ms')
            batch.pop('weight_ms')
        data_mvs, pose_ref = self.decode_batch(batch)

        imgs = data_mvs['images']
        near_fars = pose_ref['near_fars']
        dpt = data_mvs['dpt']
        sparse_depths = data_mvs['sparse_depths']
        sparse_weights = data_mvs['sparse_depths_weight']
        batch_depth = data_mvs['rays_depth']

        batch_depth = batch_depth.squeeze(0)
        batch_depth = torch.transpose(batch_depth, 0, 1)
        depth_coord = batch_depth[2, :, 0:2]

        affine_mat, affine_mat_inv = data_mvs['affine_mat'][0], data_mvs['affine_mat_inv'][0]
        imgs_input = imgs[:, 1:]
        volume_feature, uncertainty_map, mvs_depth, outputs = self.Consist_Learner(imgs_input, affine_mat, affine_mat_inv, near_fars[0], pad=args.pad)
        imgs = self._unpreprocessed(data_mvs)

        N_rays, N_samples = args.batch_size, args.N_samples
        c2ws, w2cs, intrinsics = pose_ref['c2ws'], pose_ref['w2cs'], pose_ref['intrinsics']
        rays_pts, rays_dir, target_s, rays_NDC, depth_candidates, rays_o, rays_depth, ndc_parameters, pixel_coordinates = \
            self._build_rays(args, imgs, uncertainty_map, sparse_depths, depth_coord, pose_ref, w2cs, c2ws, intrinsics,
                       N_rays, N_samples, pad=args.pad, with_depth=True, outputs=outputs)

        rgb, depth_pred = rendering(args, pose_ref, rays_pts, rays_NDC, depth_candidates, rays_dir, outputs, imgs[:, 1:], near_fars=near_fars[0],
                                    img_feat=outputs['stage3']['img_feats'], confidence=uncertainty_map, ndc_parameters=ndc_parameters,
                                    **self.render_kwargs_train)

        # train.py:166-176 in one launch
        target_depths, target_weights, patch_dpt = ops.step_targets(sparse_depths, sparse_weights, dpt, pixel_coordinates, N_rays, args.patch_num,
                                                                    args.patch_size)
        # train.py:171-188
        loss, parts = training_loss(rgb, depth_pred, target_s, target_depths, target_weights, patch_dpt, outputs, depth_sparse_ms, weight_ms,
                                    n_rays=N_rays, patch_num=args.patch_num, patch_size=args.patch_size, smooth_loss=self.smooth_loss,
                                    edge_loss=self.edge_loss, mvs_on_device=True)
        img_loss = parts['img_loss']
        psnr = -10. * torch.log(img_loss.detach()) / np.log(10.)           # mse2psnr2 on the tensor (the reference: on img_loss.item())

        with torch.no_grad():
            if self.global_step % 5000 == 4999:
                self.save_ckpt(f'{self.global_step}')
            if self.log_fn is not None and self.global_step % self.log_every == 0:
                self.log('train/loss', loss, prog_bar=True)
                self.log('train/img_mse_loss', img_loss, prog_bar=False)
                self.log('train/PSNR', psnr, prog_bar=True)
                self.log('train/depth loss', loss, prog_bar=True)
                self.log('train/smooth loss', parts['smooth_loss'], prog_bar=True)
                self.log('train/loss_scaleinvariant', parts['loss_scaleinvariant'], prog_bar=True)
                self.log('train/depth loss_mvs', parts['loss_mvs'], prog_bar=False)
                self.log('train/depth loss_nerf_depth', parts['loss_nerf_depth'], prog_bar=False)
        out = {'loss': loss, 'psnr': psnr}
        out.update({k: v.detach() for k, v in parts.items()})
        return out

    # ------------------------------------------------------------------------------------------------ train.py:213-324
    def validation_step(self, batch, batch_nb, savefig=False):
        """One validation image through `render_validation_image`.  As in the reference, this calls `self.Consist_Learner.train()` and never
        switches back: the batch-norm layers normalise with the batch statistics and their running statistics MOVE during validation, there as
        here.  -> the reference's log dict (gt_depth, pred_depth, gt_rgb, pred_rgb, mask) plus render_validation_image's pred_depth_vis,
        gt_depth_vis and uncertainty, all device tensors.  savefig=True writes the reference's 2 x 2 matplotlib figure (the one host copy)."""
        args = self.args
        batch = dict(batch)
        if 'scan' in batch.keys():
            batch.pop('scan')
            batch.pop('sparse_depths_ms')
            batch.pop('weight_ms')
        data_mvs, pose_ref = self.decode_batch(batch)
        imgs = data_mvs['images']
        near_fars = pose_ref['near_fars']
        depths_h = data_mvs['depths_h']
        self.Consist_Learner.train()
        H, W = imgs.shape[-2:]
        H, W = int(H), int(W)

        with torch.no_grad():
            imgs_input = imgs[:, 1:]
            affine_mat, affine_mat_inv = data_mvs['affine_mat'][0], data_mvs['affine_mat_inv'][0]
            volume_feature, photo_confidence, mvs_depth, outputs = self.Consist_Learner(imgs_input, affine_mat, affine_mat_inv, near_fars[0],
                                                                                         pad=args.pad)
            imgs = self._unpreprocessed(data_mvs)
            imgs_input = imgs[:, 1:]
            log = render_validation_image(args, pose_ref, outputs, imgs_input, photo_confidence, H, W, near_fars, self.render_kwargs_train,
                                          depth_gt=depths_h[0], gt_rgb=imgs[0, 0])
            if savefig:
                self._save_figure(log)
            self.idx += 1
        self.validation_step_outputs.append(log)
        return log

    def _save_figure(self, log):
        """train.py:291-316."""
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        save_path = f'{self.args.basedir}/{self.args.expname}/test_results'
        os.makedirs(save_path, exist_ok=True)
        fig, axs = plt.subplots(2, 2)
        panels = ((log['gt_rgb'], 'Ground Truth RGB'), (log['pred_rgb'], 'Rendered RGB'), (log['gt_depth_vis'], 'Ground Truth Depth'),
                  (log['pred_depth_vis'], 'Rendered Depth'))
        for ax, (img, title) in zip(axs.reshape(-1), panels):
            ax.imshow(img.permute(1, 2, 0).cpu().numpy())
            ax.set_title(title)
            ax.axis('off')
        plt.tight_layout()
        plt.savefig(f'{save_path}/{self.global_step:08d}_{self.idx:02d}.png')
        plt.close(fig)

    # ------------------------------------------------------------------------------------------------ free-camera rendering (no counterpart)
    def render_path(self, scene, poses, n_views=None, candidates=None, depth_vis=False):
        """Renders the views of a camera path that are no frames of the dataset.  scene: a `DeviceScene`; poses: [P,3,4] camera-to-world (a
        float32 device tensor is used as it is; anything else -- `data.paths.interp_path`'s float64 array -- is uploaded once as float32, one
        blocking copy); n_views: default args.view_num, the pose and its n_views - 1 nearest source frames among `candidates`
        (`DeviceScene.sample_pose`'s: default the scene's training index; a sequence is uploaded once, before the loop).
        -> {'rgb' [P,3,H,W] in [0, 1], 'depth' [P,H,W]} (and 'depth_vis' [P,3,H,W] with depth_vis=True): device tensors, allocated once and
        written frame by frame -- per frame `sample_pose` (one launch) then `validate.render_novel_view`, under no_grad, nothing read back.
        The CNNs run in the mode `validation_step` runs them, train(): batch statistics, so the images agree with what validation measures.
        UNLIKE validation_step this call leaves the model as it found it: every buffer of the consistency learner (the batch-norm running
        statistics and num_batches_tracked) is copied on the device before the loop and copied back after it, and each module's `training`
        flag is restored -- also when a frame raises."""
        from .validate import render_novel_view
        args = self.args
        n_views = int(args.view_num if n_views is None else n_views)
        dev = scene.frames.device
        if not (torch.is_tensor(poses) and poses.device == dev and poses.dtype == torch.float32 and poses.is_contiguous()):
            poses = torch.as_tensor(np.ascontiguousarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float32)).to(dev)
        if candidates is not None and not torch.is_tensor(candidates):
            candidates = torch.from_numpy(np.ascontiguousarray(np.asarray(candidates), dtype=np.int32)).to(dev)
        P, H, W = int(poses.shape[0]), scene.H, scene.W
        out = {'rgb': torch.empty(P, 3, H, W, device=dev), 'depth': torch.empty(P, H, W, device=dev)}
        if depth_vis:
            out['depth_vis'] = torch.empty(P, 3, H, W, device=dev)
        net = self.Consist_Learner
        flags = [(m, m.training) for n in (net, self.render_kwargs_train['network_fn']) for m in n.modules()]
        with torch.no_grad():
            saved = [(b, b.clone()) for b in net.buffers()]
            try:
                net.train()
                for j in range(P):
                    batch = scene.sample_pose(poses, j, n_views, candidates=candidates, unpreprocess=True)
                    rgb, depth, vis = render_novel_view(args, batch, net, self.render_kwargs_train)
                    out['rgb'][j].copy_(rgb)
                    out['depth'][j].copy_(depth)
                    if depth_vis:
                        out['depth_vis'][j].copy_(vis)
            finally:
                for b, was in saved:
                    b.copy_(was)
                for m, was in flags:
                    m.training = was
        return out

    # ------------------------------------------------------------------------------------------------ reconstruction (no counterpart)
    def _frame_maps(self, batch, depth_source):
        """validation_step's steps on one sample (train.py:213-289; the caller holds no_grad and has set the CNNs' mode): the consistency learner,
        then `render_validation_image`.  -> (depth [H,W], rgb [3,H,W], conf [H,W] or None) by `depth_source`."""
        args = self.args
        batch = {k: v for k, v in batch.items() if k not in ('scan', 'sparse_depths_ms', 'weight_ms')}
        data_mvs, pose_ref = self.decode_batch(batch)
        imgs = data_mvs['images']
        near_fars = pose_ref['near_fars']
        H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
        affine_mat, affine_mat_inv = data_mvs['affine_mat'][0], data_mvs['affine_mat_inv'][0]
        _, photo_confidence, mvs_depth, outputs = self.Consist_Learner(imgs[:, 1:], affine_mat, affine_mat_inv, near_fars[0], pad=args.pad)
        imgs = self._unpreprocessed(data_mvs)
        log = render_validation_image(args, pose_ref, outputs, imgs[:, 1:], photo_confidence, H, W, near_fars, self.render_kwargs_train,
                                      gt_rgb=imgs[0, 0])
        if depth_source == "render":
            return log['pred_depth'], log['pred_rgb'], None
        # (stage 3's depth and confidence are [1,H,W] whatever args.pad is: ops.depth_regress drops the border itself)
        return mvs_depth[0], log['gt_rgb'], photo_confidence[0]

    def reconstruct(self, scene, frames=None, depth_source="render", n_src=4, **thresholds):
        """A coloured point cloud of the scene from the depth maps of `frames` (default: every frame), fused on the device
        (`uc_nerf_amd.fusion.fuse_views`: consistency filter, then compaction).  Per frame, validation's steps: `scene.sample(frame, its
        view_num - 1 nearest training frames, unpreprocess=True)`, the consistency learner, `render_validation_image`.
        depth_source="render": the rendered depth and colour (pred_depth, pred_rgb); "mvs": the cascade's stage-3 depth with its photometric
        confidence as `conf` (so `conf_thresh` applies) and the frame's own colours (gt_rgb); not exercised with args.pad > 0.  n_src: source views per frame for the filter, the
        nearest among `frames` themselves; **thresholds: pix_thresh, rel_thresh, conf_thresh, min_views.  The cameras are the scene's resident
        c2w / w2c / intrinsic.  -> `fusion.PointCloud`, everything on the device: after a first call with the same frames (which uploads their
        source table once: `DeviceScene.fusion_sources` keeps the last one) nothing is read back or synchronised until `PointCloud.trim()`.
        Like `render_path` the CNNs run in train() as validation runs them, and the model is left as found: every buffer of the consistency
        learner and every module's `training` flag is restored, also when a frame raises."""
        from .fusion import fuse_views
        if depth_source not in ("render", "mvs"):
            raise ValueError("UCNeRFSystem.reconstruct: depth_source must be 'render' or 'mvs', got %r" % (depth_source,))
        frames = list(range(scene.N)) if frames is None else [int(f) for f in frames]
        if not frames or min(frames) < 0 or max(frames) >= scene.N:
            raise IndexError("UCNeRFSystem.reconstruct: frames %r outside 0..%d (or empty)" % (frames, scene.N - 1))
        n_views, n_src = int(self.args.view_num), int(n_src)
        dev, P, H, W = scene.frames.device, len(frames), scene.H, scene.W
        depth, rgb = torch.empty(P, H, W, device=dev), torch.empty(P, 3, H, W, device=dev)
        conf = torch.empty(P, H, W, device=dev) if depth_source == "mvs" else None
        net = self.Consist_Learner
        flags = [(m, m.training) for n in (net, self.render_kwargs_train['network_fn']) for m in n.modules()]
        with torch.no_grad():
            saved = [(b, b.clone()) for b in net.buffers()]
            try:
                net.train()
                for j, f in enumerate(frames):
                    batch = scene.sample(f, scene.nearest_train_views(f, n_views), unpreprocess=True)
                    d, c, q = self._frame_maps(batch, depth_source)
                    depth[j].copy_(d)
                    rgb[j].copy_(c)
                    if conf is not None:
                        conf[j].copy_(q)
            finally:
                for b, was in saved:
                    b.copy_(was)
                for m, was in flags:
                    m.training = was
            c2ws, w2cs = torch.stack([scene.c2w[f] for f in frames]), torch.stack([scene.w2c[f] for f in frames])
            K = torch.stack([scene.intrinsic[f] for f in frames])
            return fuse_views(depth, rgb, K, c2ws, src_ids=scene.fusion_sources(frames, n_src), w2cs=w2cs, conf=conf, **thresholds)

    # ------------------------------------------------------------------------------------------------ train.py:326-402
    def on_validation_epoch_end(self):
        """-> {'val/PSNR', 'val/SSIM', 'val/LPIPS', 'val/abs_rel', 'val/sq_rel', 'val/rmse', 'val/rmse_log', 'val/a1', 'val/a2', 'val/a3'}; with
        more than one logged image the images are grouped by scan, `test_num` = 10 to a scan, and the groups' numbers averaged."""
        outs = self.validation_step_outputs
        pred_rgb = torch.stack([x['pred_rgb'] for x in outs])
        pred_depth = torch.stack([x['pred_depth'] for x in outs])
        gt_rgb = torch.stack([x['gt_rgb'] for x in outs])
        gt_depth = torch.stack([x['gt_depth'] for x in outs])
        mask = torch.stack([x['mask'] for x in outs])
        test_num = 10
        savedir = None
        all_rgb_errors = []
        all_depth_errors = []
        if pred_rgb.shape[0] > 1:
            groups = [slice(i * test_num, (i + 1) * test_num) for i in range(len(self.val_scenes))]
        else:
            groups = [slice(None)]
        for g in groups:
            psnr, ssim, lpips = rgb_evaluation(gt_rgb[g], pred_rgb[g], savedir, lpips_fn=self.lpips_fn)
            depth_errors = depth_evaluation(gt_depth[g], pred_depth[g], pred_masks=mask[g], savedir=savedir)
            all_rgb_errors.append([float(psnr), float(ssim), float(lpips)])
            all_depth_errors.append(depth_errors)
        all_rgb_errors = np.stack(all_rgb_errors).mean(axis=0)
        all_depth_errors = np.stack(all_depth_errors).mean(axis=0)
        result = dict(zip(VAL_KEYS, [float(v) for v in all_rgb_errors] + [float(v) for v in all_depth_errors]))
        if getattr(self.args, 'log', False):
            for k, v in result.items():
                self.log(k, v, prog_bar=False)
        print('psnr: {0}, ssim: {1}, lpips: {2}'.format(*all_rgb_errors))
        print('abs_rel: {0}, sq_rel: {1}, rmse: {2}, rmse_log: {3}, a1: {4}, a2: {5}, a3: {6}'.format(*all_depth_errors))
        self.validation_step_outputs = []
        return result

    # ------------------------------------------------------------------------------------------------ train.py:404-414
    def save_ckpt(self, name='latest'):
        save_dir = f'{self.args.basedir}/{self.args.expname}/ckpts/'
        os.makedirs(save_dir, exist_ok=True)
        path = f'{save_dir}/{name}.tar'
        ckpt = {'network_fn_state_dict': self.render_kwargs_train['network_fn'].state_dict(),
                'network_mvs_state_dict': self.Consist_Learner.state_dict()}
        torch.save(ckpt, path)
        print('Saved checkpoints at', path)
        return path

    # ------------------------------------------------------------------------------------------------ the Trainer of train.py:434-447
    def train_metas(self, rng):
        """[(scene index, target, src_views)] of the training split over all training scenes: `DeviceScene.metas('train', view_num)` drawn
        from `rng` (`args.num_train_samples` entries a scene, default the reference's 200)."""
        n = int(getattr(self.args, 'num_train_samples', 200))
        return [(s, t, src) for s, scene in enumerate(self.train_scenes) for t, src in scene.metas('train', self.args.view_num, num_samples=n, rng=rng)]

    def val_metas(self):
        return [(s, t, src) for s, scene in enumerate(self.val_scenes) for t, src in scene.metas('val', self.args.view_num)]

    @staticmethod
    def epoch_order(metas, rng):
        """One epoch's visiting order: every meta once, shuffled by `rng` (a numpy Generator), as the reference's shuffle=True loader does."""
        return [metas[i] for i in rng.permutation(len(metas))]

    def _train_visit(self, meta, batch_nb):
        s, target, src_views = meta
        batch = self.train_scenes[s].sample(target, src_views, unpreprocess=True)
        self.optimizer.zero_grad(set_to_none=True)
        out = self.training_step(batch, batch_nb)
        out['loss'].backward()
        self.optimizer.step()
        self.global_step += 1
        return out

    def _val_visit(self, meta, batch_nb):
        s, target, src_views = meta
        return self.validation_step(self.val_scenes[s].sample(target, src_views, unpreprocess=True), batch_nb)

    def _validate(self, metas):
        self.validation_step_outputs = []
        for k, meta in enumerate(metas):
            self._val_visit(meta, k)
        return self.on_validation_epoch_end()

    def validate(self):
        """`trainer.validate(system)`: every validation meta once, then the epoch end.  -> its result."""
        return self._validate(self.val_metas())

    def fit(self, max_epochs=None, check_val_every_n_epoch=2, num_sanity_val_steps=1, seed=None):
        """`trainer.fit(system)` as train.py:434-447 configures it: `num_sanity_val_steps` validation steps first, their epoch-end result
        discarded; then `max_epochs` (default args.num_epochs) epochs, each visiting every training meta once in an order drawn from
        `np.random.default_rng(seed)` -- sample -> zero_grad(set_to_none=True) -> training_step -> backward -> optimizer.step() -- then one
        scheduler step, then, every `check_val_every_n_epoch`-th epoch, a validation epoch.  -> the list of validation results."""
        rng = np.random.default_rng(seed)
        if self.optimizer is None:
            self.configure_optimizers()
        max_epochs = self.args.num_epochs if max_epochs is None else int(max_epochs)
        metas, val_metas = self.train_metas(rng), self.val_metas()
        if num_sanity_val_steps and val_metas:
            self._validate(val_metas[:num_sanity_val_steps])
        results = []
        for epoch in range(max_epochs):
            self.current_epoch = epoch
            for k, meta in enumerate(self.epoch_order(metas, rng)):
                self._train_visit(meta, k)
            self.scheduler.step()
            if check_val_every_n_epoch and (epoch + 1) % check_val_every_n_epoch == 0 and val_metas:
                results.append(self._validate(val_metas))
        return results
