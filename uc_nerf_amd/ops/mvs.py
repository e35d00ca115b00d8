"""The MVS stage ops (cost volume, depth regression, depth hypotheses; forward and backward) and the cascade depth loss."""
import ctypes as C

import torch

from .. import _lib as L
from ._core import _cur_dev, _f32, _launch, _ptr


def _cost_volume_params(feats, proj, depth_values, pad):
    V, Cc, H, W = feats.shape
    D, Hp, Wp = depth_values.shape
    if tuple(proj.shape) != (V, 3, 4) or Hp != H + 2 * pad or Wp != W + 2 * pad:
        raise RuntimeError("uc_nerf_amd.cost_volume: shape mismatch")
    p = L.CostVolumeParams()
    p.V, p.C, p.H, p.W, p.D, p.pad = V, Cc, H, W, D, int(pad)
    p.feats, p.proj, p.depth_values = _ptr(feats), _ptr(proj), _ptr(depth_values)
    return p


def _cost_volume_fwd(feats, proj, depth_values, pad, want_count):
    p = _cost_volume_params(feats, proj, depth_values, pad)
    D, Hp, Wp = depth_values.shape
    var = torch.empty(feats.shape[1], D, Hp, Wp, device=feats.device)
    cnt = torch.empty(D, Hp, Wp, device=feats.device) if want_count else None
    p.variance, p.count = _ptr(var), _ptr(cnt)
    _launch("ucnerf_cost_volume", p, feats.device)
    return var, cnt


class _CostVolumeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, proj, depth_values, pad):
        ctx.save_for_backward(feats, proj, depth_values)
        ctx.pad = pad
        return _cost_volume_fwd(feats, proj, depth_values, pad, False)[0]

    @staticmethod
    def backward(ctx, g_var):
        feats, proj, depth_values = ctx.saved_tensors
        bp = L.CostVolumeBwdParams()
        bp.fwd = _cost_volume_params(feats, proj, depth_values, ctx.pad)
        g_var = _f32(g_var, "g_variance")
        g_feats = torch.zeros_like(feats)
        bp.g_variance, bp.g_feats = _ptr(g_var), _ptr(g_feats)
        _launch("ucnerf_cost_volume_bwd", bp, feats.device)
        return g_feats, None, None, None


def cost_volume(feats, proj, depth_values, pad=0, want_count=False):
    """Variance cost volume of one cascade stage (network/mvs_models.py:609-626 with utils/utils.py:1105-1172 inside).
    feats [V,C,H,W] source-view feature maps, proj [V,3,4] = (src_proj @ ref_proj_inv)[:3], depth_values
    [D,H+2pad,W+2pad].  Returns variance [C,D,H+2pad,W+2pad] (and count [D,Hp,Wp] if asked).  Differentiable with
    respect to `feats` (as in the reference: nearest-neighbour lookup, the grid and the mask count carry no gradient)."""
    feats, proj, depth_values = _f32(feats, "feats"), _f32(proj, "proj"), _f32(depth_values, "depth_values")
    if want_count:
        return _cost_volume_fwd(feats.detach(), proj, depth_values, pad, True)
    return _CostVolumeFn.apply(feats, proj.detach(), depth_values.detach(), int(pad))


def _depth_regress_params(prob_pre, prob_init, depth_values, pad):
    D, Hp, Wp = prob_pre.shape
    if tuple(depth_values.shape) != (D, Hp, Wp) or (prob_init is not None and tuple(prob_init.shape) != (D, Hp, Wp)):
        raise RuntimeError("uc_nerf_amd.depth_regress: shape mismatch")
    p = L.DepthRegressParams()
    p.D, p.Hp, p.Wp, p.pad = D, Hp, Wp, int(pad)
    p.prob_pre, p.prob_init, p.depth_values = _ptr(prob_pre), _ptr(prob_init), _ptr(depth_values)
    return p


class _DepthRegressFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob_pre, depth_values, prob_init, pad):
        D, Hp, Wp = prob_pre.shape
        dev = prob_pre.device
        p = _depth_regress_params(prob_pre, prob_init, depth_values, pad)
        prob = torch.empty(D, Hp, Wp, device=dev)
        depth = torch.empty(Hp - 2 * pad, Wp - 2 * pad, device=dev)
        conf = torch.empty_like(depth)
        p.prob_volume, p.depth, p.confidence = _ptr(prob), _ptr(depth), _ptr(conf)
        _launch("ucnerf_depth_regress", p, dev)
        ctx.save_for_backward(prob, depth_values)
        ctx.pad, ctx.has_init = pad, prob_init is not None
        ctx.mark_non_differentiable(prob)                 # the reference returns prob_volume.detach() (mvs_models.py:646)
        return prob, depth, conf

    @staticmethod
    def backward(ctx, _g_prob, g_depth, g_conf):
        prob, depth_values = ctx.saved_tensors
        g_depth = _f32(g_depth, "g_depth") if g_depth is not None else None
        g_conf = _f32(g_conf, "g_confidence") if g_conf is not None else None
        g_x = g_dv = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            bp = L.DepthRegressBwdParams()
            bp.fwd = _depth_regress_params(prob, None, depth_values, ctx.pad)
            bp.fwd.prob_volume = _ptr(prob)
            g_x = torch.empty_like(prob)
            bp.g_depth, bp.g_confidence, bp.g_prob_pre = _ptr(g_depth), _ptr(g_conf), _ptr(g_x)
            _launch("ucnerf_depth_regress_bwd", bp, prob.device)
        if ctx.needs_input_grad[1]:                       # depth = sum_d p_d * depth_values_d: the hypotheses' own gradient
            g_dv = _depth_regress_bwd_values(prob, g_depth, ctx.pad)
        return g_x, g_dv, (g_x if ctx.has_init else None), None


def _depth_regress_bwd_values(prob, g_depth, pad):
    """g_depth_values [D,Hp,Wp] = prob * g_depth inside the crop, 0 on the border of `pad` pixels (`ucnerf_depth_regress_bwd_values`)."""
    D, Hp, Wp = prob.shape
    g_dv = torch.empty_like(prob)
    if g_depth is None:
        return g_dv.zero_()
    if tuple(g_depth.shape) != (Hp - 2 * pad, Wp - 2 * pad):
        raise RuntimeError("uc_nerf_amd.depth_regress: g_depth %s for a volume %s cropped by %d" % (tuple(g_depth.shape), tuple(prob.shape), pad))
    p = L.DepthRegressBwdValuesParams()
    p.D, p.Hp, p.Wp, p.pad = D, Hp, Wp, int(pad)
    p.prob_volume, p.g_depth, p.g_depth_values = _ptr(prob), _ptr(g_depth), _ptr(g_dv)
    _launch("ucnerf_depth_regress_bwd_values", p, prob.device)
    return g_dv


def depth_regress(prob_pre, depth_values, prob_init=None, pad=0):
    """softmax over depth, expected depth and 4-tap photometric confidence (network/mvs_models.py:629-646).
    prob_pre, depth_values (and prob_init) [D,Hp,Wp] -> (prob_volume [D,Hp,Wp] (detached, as in the reference), depth
    [H,W], confidence [H,W]); depth and confidence are differentiable with respect to the logits, and depth with respect to depth_values
    (depth = sum_d p_d * depth_values_d, as the reference's torch expression is; the confidence does not depend on them)."""
    prob_pre, depth_values = _f32(prob_pre, "prob_pre"), _f32(depth_values, "depth_values")
    prob_init = _f32(prob_init, "prob_init") if prob_init is not None else None
    return _DepthRegressFn.apply(prob_pre, depth_values, prob_init, int(pad))


def _depth_hypotheses_map_params(cur_depth, near_far, interval, sizes):
    p = L.DepthHypothesesParams()
    p.D, p.h, p.w, p.pad, p.H, p.W, p.k = sizes
    p.h0, p.w0 = cur_depth.shape
    p.cur_depth, p.near_far, p.interval = _ptr(cur_depth), _ptr(near_far), _ptr(interval)
    return p


class _DepthHypothesesFn(torch.autograd.Function):
    """Map mode of `depth_hypotheses` under autograd: differentiable in cur_depth; near_far and interval get no gradient."""

    @staticmethod
    def forward(ctx, cur_depth, near_far, interval, sizes):
        D, h, w, pad = sizes[:4]
        p = _depth_hypotheses_map_params(cur_depth, near_far, interval, sizes)
        out = torch.empty(max(D, 0), max(h + 2 * pad, 0), max(w + 2 * pad, 0), device=cur_depth.device)
        p.out = _ptr(out)
        _launch("ucnerf_depth_hypotheses", p, cur_depth.device)
        ctx.save_for_backward(cur_depth, near_far, *(() if interval is None else (interval,)))
        ctx.sizes = sizes
        return out

    @staticmethod
    def backward(ctx, g_out):
        cur_depth, near_far = ctx.saved_tensors[:2]
        interval = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        return depth_hypotheses_bwd(_f32(g_out, "g_out"), cur_depth, near_far, interval, ctx.sizes), None, None, None


def depth_hypotheses_bwd(g_out, cur_depth, near_far, interval, sizes):
    """`ucnerf_depth_hypotheses_bwd`: g_out [D, h + 2 pad, w + 2 pad] -> g_cur_depth [h0,w0] for the map-mode call with sizes =
    (D, h, w, pad, H, W, k).  Three gather launches through a scratch of 2 h w + H W floats from torch's allocator (on the current stream, so
    a capture stays a plain stream capture); no atomics, the same bits from every call.  What autograd runs behind `depth_hypotheses`."""
    dev = cur_depth.device
    D, h, w, pad = sizes[:4]
    if tuple(g_out.shape) != (max(D, 0), max(h + 2 * pad, 0), max(w + 2 * pad, 0)):
        raise RuntimeError("uc_nerf_amd.depth_hypotheses_bwd: g_out %s for sizes %s" % (tuple(g_out.shape), tuple(sizes)))
    bp = L.DepthHypothesesBwdParams()
    bp.fwd = _depth_hypotheses_map_params(cur_depth, near_far, interval, sizes)
    n = L.lib().ucnerf_depth_hypotheses_bwd_scratch_floats(C.addressof(bp.fwd))
    if n < 0:
        raise RuntimeError("uc_nerf_amd.depth_hypotheses_bwd: " + L.lib().ucnerf_last_error().decode())
    scratch = torch.empty(n, device=dev)
    g_cur = torch.empty_like(cur_depth)
    bp.g_out, bp.scratch, bp.g_cur_depth = _ptr(g_out), _ptr(scratch), _ptr(g_cur)
    _launch("ucnerf_depth_hypotheses_bwd", bp, dev)
    return g_cur


def depth_hypotheses(ndepth, out_hw, cur_depth=None, row=None, near_far=None, k=0.0, full_hw=None, pad=0, interval=None):
    """The depth hypotheses of one cascade stage in one launch (network/mvs_models.py:536-573 as CascadeMVSNet.forward uses them, :693-762):
    -> depth_values [ndepth, h + 2 pad, w + 2 pad], (h, w) = out_hw, the border of `pad` pixels repeating the edge (DepthNet's replicate pad).
    Map mode: cur_depth [h0,w0] = the previous stage's depth, near_far a DEVICE tensor (near, far), interval_pixel = k * (far - near) -- or
    k * interval for a one-element device tensor `interval` --, full_hw the resolution the reference up-samples to before it interpolates back down (default: out_hw).  Row mode: row [D_in], the band
    row[0] .. row[-1] for every pixel.  Differentiable with respect to cur_depth (map mode, when it requires grad and grad mode is on:
    `ucnerf_depth_hypotheses_bwd`, ties of the two clamps pass as torch's clamp does); near_far, interval and row are taken detached."""
    if (cur_depth is None) == (row is None):
        raise RuntimeError("uc_nerf_amd.depth_hypotheses: exactly one of cur_depth (map mode) and row (row mode)")
    h, w = int(out_hw[0]), int(out_hw[1])
    H, W = (h, w) if full_hw is None else (int(full_hw[0]), int(full_hw[1]))
    p = L.DepthHypothesesParams()
    p.D, p.h, p.w, p.pad, p.H, p.W, p.k = int(ndepth), h, w, int(pad), H, W, float(k)
    if cur_depth is not None:
        cur_in = cur_depth
        cur_depth = _f32(cur_depth.detach(), "cur_depth")
        if cur_depth.dim() != 2 or near_far is None:
            raise RuntimeError("uc_nerf_amd.depth_hypotheses: map mode takes cur_depth [h0,w0] and near_far")
        near_far = _f32(near_far.detach(), "near_far")
        if near_far.numel() != 2 or near_far.device != cur_depth.device:
            raise RuntimeError("uc_nerf_amd.depth_hypotheses: near_far must hold (near, far) on cur_depth's device")
        p.h0, p.w0 = cur_depth.shape
        p.cur_depth, p.near_far = _ptr(cur_depth), _ptr(near_far)
        if interval is not None:
            interval = _f32(interval.detach(), "interval")
            if interval.numel() != 1 or interval.device != cur_depth.device:
                raise RuntimeError("uc_nerf_amd.depth_hypotheses: interval must hold one value on cur_depth's device")
            p.interval = _ptr(interval)
        if cur_in.requires_grad and torch.is_grad_enabled():
            return _DepthHypothesesFn.apply(_f32(cur_in, "cur_depth"), near_far, interval, (p.D, h, w, p.pad, H, W, p.k))
        dev = cur_depth.device
    else:
        row = _f32(row.detach(), "row")
        if row.dim() != 1:
            raise RuntimeError("uc_nerf_amd.depth_hypotheses: row mode takes row [D_in]")
        p.D_in, p.row = row.shape[0], _ptr(row)
        dev = row.device
    out = torch.empty(max(p.D, 0), max(h + 2 * p.pad, 0), max(w + 2 * p.pad, 0), device=dev)
    p.out = _ptr(out)
    _launch("ucnerf_depth_hypotheses", p, dev)
    return out


# one sticky status word per device (bit s: stage s of a cas_loss call had a valid count different from its positive-weight count), allocated
# once and kept for the life of the process: captured graphs hold its address
_loss_words = {}


def _loss_word(device=None):
    idx = _cur_dev() if device is None or torch.device(device).index is None else torch.device(device).index
    w = _loss_words.get(idx)
    if w is None:
        w = _loss_words[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return w


def loss_status(clear=False, device=None):
    """The cascade loss's status word of `device` (default: the current one) as an int: bit s set = stage s of some `cas_loss` call since the last
    clear had a number of valid depths different from its number of positive weights (its loss was NaN).  SYNCHRONISES (reads the word back);
    clear=True also zeroes it afterwards."""
    w = _loss_word(device)
    v = int(w.item())
    if clear:
        w.zero_()
    return v


def loss_status_clear(device=None):
    """Enqueues a clear of the status word on the current stream (no synchronisation)."""
    _loss_word(device).zero_()


class _CasLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stage_weights, with_weight, status, n_stages, *tensors):
        ests, gts, ws = tensors[:n_stages], tensors[n_stages:2 * n_stages], tensors[2 * n_stages:]
        dev = ests[0].device
        sizes = [e.numel() for e in ests]
        p = L.CasLossParams()
        p.n_stages, p.with_weight = n_stages, int(with_weight)
        head = torch.empty(1 + n_stages, device=dev)                      # total | stage losses
        count = torch.empty(n_stages, dtype=torch.int32, device=dev)
        wpair = torch.empty(sum(sizes), device=dev)
        work = torch.empty(sum(sizes), device=dev) if with_weight else None
        at = 0
        for s in range(n_stages):
            p.n[s], p.stage_w[s] = sizes[s], float(stage_weights[s])
            p.est[s], p.gt[s], p.w[s] = _ptr(ests[s]), _ptr(gts[s]), _ptr(ws[s]) if with_weight else 0
            p.wpair[s] = wpair.data_ptr() + 4 * at
            at += sizes[s]
        p.workspace, p.total, p.stage_loss, p.count, p.status = _ptr(work), head.data_ptr(), head.data_ptr() + 4, _ptr(count), _ptr(status)
        _launch("ucnerf_cas_loss_fwd", p, dev)
        ctx.save_for_backward(wpair, count, *ests, *gts)
        ctx.n_stages, ctx.n_inputs, ctx.stage_weights = n_stages, len(tensors), tuple(float(x) for x in stage_weights)
        total, stage_loss = head[0], head[1:]
        ctx.mark_non_differentiable(count)
        ctx.set_materialize_grads(False)                                  # (an unused output's gradient arrives as None, not as a zero fill)
        return total, stage_loss, count

    @staticmethod
    def backward(ctx, g_total, g_stage, _g_count):
        n = ctx.n_stages
        wpair, count = ctx.saved_tensors[:2]
        ests, gts = ctx.saved_tensors[2:2 + n], ctx.saved_tensors[2 + n:]
        dev = wpair.device
        g_total = _f32(g_total, "g_total") if g_total is not None else torch.zeros(1, device=dev)
        g_stage = _f32(g_stage, "g_stage_loss") if g_stage is not None else None
        p = L.CasLossBwdParams()
        p.n_stages = n
        g_all = torch.empty_like(wpair)
        grads, at = [], 0
        for s in range(n):
            k = ests[s].numel()
            p.n[s], p.stage_w[s] = k, ctx.stage_weights[s]
            p.est[s], p.gt[s], p.wpair[s], p.g_est[s] = _ptr(ests[s]), _ptr(gts[s]), wpair.data_ptr() + 4 * at, g_all.data_ptr() + 4 * at
            grads.append(g_all[at:at + k].view(ests[s].shape))
            at += k
        p.count, p.g_total, p.g_stage = _ptr(count), _ptr(g_total), _ptr(g_stage)
        _launch("ucnerf_cas_loss_bwd", p, dev)
        return (None, None, None, None) + tuple(grads) + (None,) * (ctx.n_inputs - n)


def cas_loss(ests, gts, ws, stage_weights, with_weight=True, status=None):
    """The cascade depth loss (network/mvs_models.py:512-529) of up to three stages in ONE launch, nothing read back: per stage the smooth-L1 term
    of the k-th valid depth (gt > 0, row-major order) times the k-th positive weight (w > 0, row-major order), summed and divided by the valid
    count; total = sum of stage_weights[s] * stage loss.  ests / gts / ws: per stage, float32 tensors of one size each on one device.
    Returns (total 0-d, stage_loss [n_stages], count [n_stages] int32) on the device; the backward is one launch and gives gradients for the
    `ests` only.  A stage without a valid element is NaN (torch's mean of nothing).  A stage whose valid count differs from its positive-weight
    count is NaN and sets bit s of `status` (a one-element int32 device tensor; default: the device's own word, see `loss_status`) -- torch
    raises there, or broadcasts where one of the counts is 1: that broadcast is NOT reproduced, it counts as a mismatch.
    with_weight=False: the weights are ignored (`ws` may be None)."""
    n = len(ests)
    if not 1 <= n <= 3 or len(gts) != n or (with_weight and (ws is None or len(ws) != n)) or len(stage_weights) != n:
        raise RuntimeError("uc_nerf_amd.cas_loss: 1 to 3 stages, each with est, gt%s and a stage weight" % (", w" if with_weight else ""))
    ests = [_f32(e, "est") for e in ests]
    dev = ests[0].device
    gts = [_f32(g.detach(), "gt") for g in gts]
    ws = [_f32(w.detach(), "w") for w in ws] if with_weight else []
    for s in range(n):
        others = [gts[s]] + ([ws[s]] if with_weight else [])
        if ests[s].numel() == 0 or any(t.numel() != ests[s].numel() or t.device != dev for t in others + [ests[s]]):
            raise RuntimeError("uc_nerf_amd.cas_loss: stage %d: est, gt and w must hold the same (non-zero) number of elements on one device" % s)
    if status is None:
        status = _loss_word(dev)
    elif not (torch.is_tensor(status) and status.is_cuda and status.dtype == torch.int32 and status.numel() == 1 and status.device == dev):
        raise RuntimeError("uc_nerf_amd.cas_loss: status must be a one-element int32 tensor on the estimates' device")
    return _CasLoss.apply(tuple(stage_weights), bool(with_weight), status, n, *ests, *gts, *ws)
