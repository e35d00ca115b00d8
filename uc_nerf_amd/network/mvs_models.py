"""Drop-in for the part of the reference's `network/mvs_models.py` that sits directly in front of the ray-marching
path: `DepthNet` (mvs_models.py:585-646), the depth-hypothesis helpers `get_depth_range_samples` /
`get_cur_depth_range_samples` (:536-573) and the three-stage loop `CascadeMVSNet` (:648-762).  Same call signatures and
result keys; the cost-volume assembly (`homo_warp` + mask count + variance), the depth regression and the link between
two stages (previous depth -> next stage's hypothesis volume) run as the HIP kernels `ucnerf_cost_volume` /
`ucnerf_depth_regress` / `ucnerf_depth_hypotheses`; the CNNs -- the feature pyramid and the 3D regularisation networks --
stay the caller's modules (MIOpen territory).

The cost volume and the regression have backward kernels behind `torch.autograd.Function`s, so the feature network
trains through the variance volume and the regularisation network through depth and photometric confidence, as in the
reference.  The chain depth regression -> depth_values -> depth hypotheses -> previous depth has backward kernels too
(`ucnerf_depth_regress_bwd_values`, `ucnerf_depth_hypotheses_bwd`): with `grad_method="detach"` (the reference's
default) the depth is detached between stages and the hypothesis volume carries no gradient; with `"undetach"` it
stays in the graph, as the reference's other branch keeps it, and a loss on a later stage's depth reaches the earlier
stages' regularisers.
`features` may be a list of [1,C,H,W] maps (as the reference passes) or a stacked tensor.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


def mvs_depth_regression(p, depth_values):                 # mvs_models.py:574-579
    if depth_values.dim() <= 2:
        depth_values = depth_values.view(*depth_values.shape, 1, 1)
    return torch.sum(p * depth_values, 1)


class DepthNet(nn.Module):
    def forward(self, features, affine_mat_stage, affine_mat_inv_stage, depth_values, num_depth, cost_regularization, imgs,
                pad=0, prob_volume_init=None, *, depth_values_padded=False):
        """`depth_values_padded` (CascadeMVSNet, whose hypothesis kernel writes the replicate border itself): depth_values already is
        [1,D,H+2pad,W+2pad] and is not padded again."""
        features = torch.stack(list(features)) if not torch.is_tensor(features) else features      # [V,B,C,H,W]
        V, B, C, H, W = features.shape
        if B != 1:
            raise RuntimeError("uc_nerf_amd DepthNet: batch size 1 (as the reference's datasets provide)")
        if pad > 0 and not depth_values_padded:
            depth_values = F.pad(depth_values, (pad, pad, pad, pad), "replicate")
        # (src_proj @ ref_proj_inv)[:3] per source view (mvs_models.py:612); entry 0 of the stage matrices is the target view
        proj = (affine_mat_stage[1:V + 1] @ affine_mat_inv_stage[0:1])[:, :3].contiguous()
        variance = ops.cost_volume(features[:, 0], proj, depth_values[0], pad=pad)
        cost_feat_no_ref, prob = cost_regularization(variance.unsqueeze(0))
        prob_pre = prob.squeeze(1)
        prob_volume, depth, conf = ops.depth_regress(prob_pre[0], depth_values[0],
                                                     None if prob_volume_init is None else prob_volume_init[0], pad=pad)
        return {"depth": depth.unsqueeze(0), "photometric_confidence": conf.unsqueeze(0),
                "volume_feature_no_ref": cost_feat_no_ref, "depth_values": depth_values, "img_feats": features,
                "prob_volume": prob_volume.unsqueeze(0)}


def _dev_scalar(v, device):
    """A near / far / interval handed over as a tensor (wherever it lives) or a number -> one float32 element on `device`; a device value
    is never read back."""
    if torch.is_tensor(v):
        return v.detach().to(device=device, dtype=torch.float32).reshape(1)
    return torch.tensor([float(v)], dtype=torch.float32, device=device)


def _batch_one(t, what):
    if t.shape[0] != 1:
        raise RuntimeError("uc_nerf_amd %s: batch size 1 (as the reference's datasets provide)" % what)
    return t[0]


def get_cur_depth_range_samples(cur_depth, ndepth, depth_inteval_pixel, shape, max_depth=192.0, min_depth=0.0):
    """mvs_models.py:536-551.  cur_depth [1,H,W] -> [1,D,H,W]: `ucnerf_depth_hypotheses` with the output at the map's own resolution.
    Differentiable with respect to cur_depth, as the reference's torch expressions are (the bounds and the interval get no gradient)."""
    if tuple(cur_depth.shape) != tuple(shape):
        raise AssertionError("cur_depth:{}, input shape:{}".format(cur_depth.shape, shape))
    c = _batch_one(cur_depth, "get_cur_depth_range_samples")
    dev = c.device
    near_far = torch.cat([_dev_scalar(min_depth, dev), _dev_scalar(max_depth, dev)])
    out = ops.depth_hypotheses(ndepth, c.shape, cur_depth=c, near_far=near_far, k=1.0, interval=_dev_scalar(depth_inteval_pixel, dev))
    return out.unsqueeze(0)


def get_depth_range_samples(cur_depth, ndepth, depth_inteval_pixel, device, dtype, shape, max_depth=192.0, min_depth=0.0):
    """mvs_models.py:554-573.  cur_depth [1,H,W] (a depth map) or [1,D_in] (a hypothesis row: the band row[0] .. row[-1] for every pixel)
    -> [1,D,H,W], float32 on cur_depth's device."""
    if cur_depth.dim() == 2:
        row = _batch_one(cur_depth, "get_depth_range_samples")
        return ops.depth_hypotheses(ndepth, (shape[1], shape[2]), row=row).unsqueeze(0)
    return get_cur_depth_range_samples(cur_depth, ndepth, depth_inteval_pixel, shape, max_depth, min_depth)


class CascadeMVSNet(nn.Module):
    """mvs_models.py:648-762: the three-stage loop around the caller's CNNs.  `feature` (the reference's FeatureNet: image [1,3,H,W] ->
    {"stage1": [1,C1,H/4,W/4], "stage2": ..., "stage3": ...}) and `cost_regularization` (its CostRegNets: variance volume [1,C,D,h,w] ->
    (volume feature, logits [1,1,D,h,w]); an nn.ModuleList / sequence with one per stage, or ONE module with share_cr) are handed in --
    they are registered under the reference's attribute names, so a reference checkpoint's `feature.*` / `cost_regularization.*` keys load.
    Per stage: `ucnerf_depth_hypotheses` (one launch, replicate border included) -> `DepthNet` (cost volume, the caller's regulariser,
    depth regression).  grad_method "detach": the previous stage's depth is detached before the next stage's hypotheses are built; "undetach"
    (the other branch of :716-719): it is not, and the hypotheses, the regressed depth and so the earlier stages carry its gradient.  The reference
    takes ANY other string for that branch; here a value that is neither of the two is refused, so that a misspelt "detach" does not silently
    change what trains."""

    GRAD_METHODS = ("detach", "undetach")

    def __init__(self, view_num=11, ndepths=[48, 32, 8], depth_interals_ratio=[4, 2, 1], share_cr=False, grad_method="detach",
                 arch_mode="fpn", cr_base_chs=[8, 8, 8], *, feature=None, cost_regularization=None):
        super().__init__()
        if grad_method not in self.GRAD_METHODS:
            raise NotImplementedError("uc_nerf_amd CascadeMVSNet: grad_method=%r -- \"detach\" (the reference's default: the depth is detached between "
                                      "stages) or \"undetach\" (it stays in the graph)" % (grad_method,))
        missing = [n for n, m in (("feature", feature), ("cost_regularization", cost_regularization)) if m is None]
        if missing:
            raise ValueError("uc_nerf_amd CascadeMVSNet: the CNNs are the caller's modules -- pass %s=... (the reference's FeatureNet / "
                             "CostRegNets, see INTEGRATION.md)" % "=..., ".join(missing))
        if len(ndepths) != len(depth_interals_ratio):
            raise AssertionError("ndepths and depth_interals_ratio differ in length")
        self.share_cr, self.ndepths, self.depth_interals_ratio = share_cr, list(ndepths), list(depth_interals_ratio)
        self.grad_method, self.arch_mode, self.cr_base_chs = grad_method, arch_mode, cr_base_chs
        self.view_num = view_num
        self.num_stage = len(ndepths)
        self.refine = False
        self.stage_infos = {"stage1": {"scale": 4.0}, "stage2": {"scale": 2.0}, "stage3": {"scale": 1.0}}
        if self.num_stage > len(self.stage_infos):
            raise ValueError("uc_nerf_amd CascadeMVSNet: at most %d stages" % len(self.stage_infos))
        self.feature = feature
        per_stage = isinstance(cost_regularization, (list, tuple, nn.ModuleList))
        if share_cr:
            if per_stage:
                raise ValueError("uc_nerf_amd CascadeMVSNet: share_cr=True takes ONE cost_regularization module")
        else:
            if not per_stage or len(cost_regularization) != self.num_stage:
                raise ValueError("uc_nerf_amd CascadeMVSNet: cost_regularization must hold one module per stage (%d)" % self.num_stage)
            if not isinstance(cost_regularization, nn.ModuleList) and all(isinstance(m, nn.Module) for m in cost_regularization):
                cost_regularization = nn.ModuleList(cost_regularization)
        self.cost_regularization = cost_regularization
        self.DepthNet = DepthNet()

    def forward(self, imgs, affine_mat, affine_mat_inv, near_far, pad):
        if imgs.shape[0] != 1:
            raise RuntimeError("uc_nerf_amd CascadeMVSNet: batch size 1 (as the reference's datasets provide)")
        dev = imgs.device
        H, W = imgs.shape[3], imgs.shape[4]
        # (near, far) on the device: read there by the kernel.  The stage-1 row of the reference, near * (1 - t) + far * t over 48 steps
        # (:694-699), is only ever read at its two ends -- near and far themselves -- so the pair stands for it.
        near_far = torch.cat([_dev_scalar(near_far[0], dev), _dev_scalar(near_far[1], dev)])
        features = [self.feature(imgs[:, i]) for i in range(imgs.size(1))]
        outputs = {}
        depth = None
        for stage_idx in range(self.num_stage):
            key = "stage{}".format(stage_idx + 1)
            features_stage = [feat[key] for feat in features]
            scale = int(self.stage_infos[key]["scale"])
            stage_pad = pad if stage_idx == 2 else 0                                     # :735-740
            D = self.ndepths[stage_idx]
            if depth is None:
                depth_value = ops.depth_hypotheses(D, (H // scale, W // scale), row=near_far, pad=stage_pad)
            else:
                cur_depth = depth.detach() if self.grad_method == "detach" else depth                # :716-719
                # depth_inteval_pixel = ratio * (far - near) / 48: the reference divides by the literal 48 (:694,698), not by ndepths[0]
                depth_value = ops.depth_hypotheses(D, (H // scale, W // scale), cur_depth=cur_depth[0], near_far=near_far,
                                                   k=self.depth_interals_ratio[stage_idx] / 48.0, full_hw=(H, W), pad=stage_pad)
            cr = self.cost_regularization if self.share_cr else self.cost_regularization[stage_idx]
            outputs_stage = self.DepthNet(features_stage, affine_mat[:, stage_idx], affine_mat_inv[:, stage_idx], depth_values=depth_value.unsqueeze(0),
                                          num_depth=D, cost_regularization=cr, imgs=imgs, pad=stage_pad, depth_values_padded=True)
            depth = outputs_stage["depth"]
            outputs[key] = outputs_stage
            outputs.update(outputs_stage)
        return outputs["stage3"]["volume_feature_no_ref"], outputs["stage3"]["photometric_confidence"], outputs["stage3"]["depth"], outputs
