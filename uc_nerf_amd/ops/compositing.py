"""Compositing (plain, merged, every-map-differentiable), the gradient fold, sample_pdf and merge_rows."""
import torch

from .. import _lib as L
from ._core import _f32, _launch, _opt, _ptr


def _alloc_maps(p, n, S, dev, var):
    """The output dict of a compositing forward (plain or merged), its maps bound to `p`."""
    out = dict(rgb=torch.empty(n, 3, device=dev), depth=torch.empty(n, device=dev), acc=torch.empty(n, device=dev),
               disp=torch.empty(n, device=dev), weights=torch.empty(n, S, device=dev))
    if var:
        out["var"] = torch.empty(n, device=dev)
    p.rgb_map, p.depth_map, p.acc_map, p.disp_map = _ptr(out["rgb"]), _ptr(out["depth"]), _ptr(out["acc"]), _ptr(out["disp"])
    p.weights, p.var = _ptr(out["weights"]), _ptr(out.get("var"))
    return out


def _bind_wu(who, p, out, u):
    """With a per-sample uncertainty u [n,S]: binds it and adds out["wu"] [n]; returns the tensor bound, for the caller to hold until its
    launch.  Apart from _alloc_maps: composite_fwd converts rays_d and noise between the two, and the order of its allocations stays."""
    if u is not None:
        u = _f32(u, "u")
        n, S = out["weights"].shape
        if tuple(u.shape) != (n, S):
            raise RuntimeError("uc_nerf_amd.%s: u must be [n,S]" % who)
        out["wu"] = torch.empty(n, device=out["weights"].device)
        p.u, p.wu = _ptr(u), _ptr(out["wu"])
    return u


def composite_fwd(raw, z, variant=0, white_bkgd=False, rays_d=None, noise=None, want_var=True, u=None):
    """u: optional [n,S] per-sample uncertainty -> out["wu"] [n] = sum_i w_i u_i (composited uncertainty)."""
    raw, z = _f32(raw, "raw"), _f32(z, "z")
    n, S = z.shape
    dev = z.device
    p = L.CompositeParams()
    p.n, p.S, p.variant, p.white_bkgd = n, S, variant, int(white_bkgd)
    out = _alloc_maps(p, n, S, dev, variant == 0 and want_var and S >= 2)
    rays_d = _f32(rays_d) if rays_d is not None else None
    noise = _f32(noise) if noise is not None else None
    p.raw, p.z, p.rays_d, p.noise = _ptr(raw), _ptr(z), _ptr(rays_d), _ptr(noise)
    u = _bind_wu("composite_fwd", p, out, u)
    _launch("ucnerf_composite_fwd", p, dev)
    return out


def composite_bwd(raw, z, g_rgb=None, g_depth=None, g_acc=None, g_weights=None, white_bkgd=False):
    raw, z = _f32(raw), _f32(z)
    n, S = z.shape
    bp = L.CompositeBwdParams()
    bp.fwd.n, bp.fwd.S, bp.fwd.variant, bp.fwd.white_bkgd = n, S, 0, int(white_bkgd)
    bp.fwd.raw, bp.fwd.z = _ptr(raw), _ptr(z)
    gs = [_opt(g) for g in (g_rgb, g_depth, g_acc, g_weights)]
    bp.g_rgb, bp.g_depth, bp.g_acc, bp.g_weights = (_ptr(g) for g in gs)
    g_raw = torch.empty_like(raw)
    bp.g_raw = _ptr(g_raw)
    _launch("ucnerf_composite_bwd", bp, z.device)
    return g_raw


class _Composite(torch.autograd.Function):
    """raw2outputs (live variant): differentiable w.r.t. raw through rgb_map, depth_map, acc_map and weights."""

    @staticmethod
    def forward(ctx, raw, z, white_bkgd):
        out = composite_fwd(raw, z, 0, white_bkgd)
        ctx.save_for_backward(raw, z)
        ctx.white_bkgd = white_bkgd
        var = out.get("var", torch.zeros_like(out["acc"]))
        ctx.mark_non_differentiable(out["disp"], var)
        return out["rgb"], out["depth"], out["acc"], out["weights"], out["disp"], var

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_acc, g_weights, _g_disp, _g_var):
        raw, z = ctx.saved_tensors
        g_raw = composite_bwd(raw, z, g_rgb, g_depth, g_acc, g_weights, ctx.white_bkgd)
        return g_raw, None, None


def composite(raw, z, white_bkgd=False):
    return _Composite.apply(raw, z, bool(white_bkgd))


def _u_stride(u, n, M, what):
    """Row stride of the draws u for n rays of M samples: [n,M], or [M] = one shared row (e.g. linspace)."""
    if u.numel() == n * M:
        return M
    if u.numel() == M:
        return 0
    raise RuntimeError("uc_nerf_amd.%s must be [n, M] or [M]" % what)


def sample_pdf(bins, weights, u, z_merge=None, want_inds=True, want_cdf=False, from_coarse=False, want_rank=False):
    """Returns dict(samples[n,M], inds[n,M] int64, cdf[n,L] (opt), z_sorted[n,M+n_merge] (when z_merge given)).
    from_coarse: bins=None, weights = coarse weights [n,S], z_merge = coarse depths [n,S] (mid-point bins, w[1:-1]).
    want_rank (with z_merge): merge_rank[n,M+n_merge] int32, the position in z_sorted of each element of
    cat(samples, z_merge) -- feed it to merge_rows."""
    weights, u = _f32(weights, "weights"), _f32(u, "u")
    if from_coarse:
        n, Lb = weights.shape[0], weights.shape[1] - 1
        if z_merge is None or tuple(z_merge.shape) != tuple(weights.shape):
            raise RuntimeError("uc_nerf_amd.sample_pdf: from_coarse needs z_merge with the weights' shape")
    else:
        bins = _f32(bins, "bins")
        n, Lb = bins.shape
        if weights.shape != (n, Lb - 1):
            raise RuntimeError("uc_nerf_amd.sample_pdf: weights must be [n, n_bins-1]")
    M = u.shape[-1]
    dev = weights.device
    p = L.SamplePdfParams()
    p.n, p.n_bins, p.n_samples, p.from_coarse = n, Lb, M, int(from_coarse)
    p.u_stride = _u_stride(u, n, M, "sample_pdf: u")
    out = {"samples": torch.empty(n, M, device=dev)}
    if want_inds:
        out["inds"] = torch.empty(n, M, dtype=torch.int64, device=dev)
    if want_cdf:
        out["cdf"] = torch.empty(n, Lb, device=dev)
    if z_merge is not None:
        z_merge = _f32(z_merge, "z_merge")
        p.n_merge = z_merge.shape[1]
        out["z_sorted"] = torch.empty(n, M + p.n_merge, device=dev)
        if want_rank:
            out["merge_rank"] = torch.empty(n, M + p.n_merge, dtype=torch.int32, device=dev)
            p.merge_rank = _ptr(out["merge_rank"])
    p.bins, p.weights, p.u, p.z_merge = _ptr(None if from_coarse else bins), _ptr(weights), _ptr(u), _ptr(z_merge)
    p.samples, p.inds, p.cdf, p.z_sorted = _ptr(out["samples"]), _ptr(out.get("inds")), _ptr(out.get("cdf")), _ptr(out.get("z_sorted"))
    _launch("ucnerf_sample_pdf", p, dev)
    return out


def merge_rows(a, b, rank):
    """out[r, rank[r, i]] = cat(a[r], b[r])[i] for rows a [n,na,w], b [n,nb,w] and rank [n,na+nb] (int32)."""
    a, b = _f32(a, "a"), _f32(b, "b")
    n, na, w = a.shape
    nb = b.shape[1]
    if rank.dtype != torch.int32 or tuple(rank.shape) != (n, na + nb) or b.shape[0] != n or b.shape[2] != w:
        raise RuntimeError("uc_nerf_amd.merge_rows: shape / dtype mismatch")
    rank = rank.contiguous()
    out = torch.empty(n, na + nb, w, device=a.device)
    p = L.MergeRowsParams()
    p.n, p.na, p.nb, p.width = n, na, nb, w
    p.a, p.b, p.rank, p.out = _ptr(a), _ptr(b), _ptr(rank), _ptr(out)
    _launch("ucnerf_merge_rows", p, a.device)
    return out


def _merged_args(who, raw_a, raw_b, rank, z):
    """The checked arguments of a merged compositing call, contiguous, and its sizes: (raw_a, raw_b, rank, z, n, S, na, nb)."""
    raw_a, raw_b, z = _f32(raw_a, "raw_a"), _f32(raw_b, "raw_b"), _f32(z, "z")
    n, S = z.shape
    na, nb = raw_a.shape[1], raw_b.shape[1]
    if (rank.dtype != torch.int32 or tuple(rank.shape) != (n, S) or tuple(raw_a.shape) != (n, na, 4) or tuple(raw_b.shape) != (n, nb, 4)
            or na + nb != S or rank.device != z.device):
        raise RuntimeError("uc_nerf_amd.%s: shape / dtype mismatch" % who)
    return raw_a, raw_b, rank.contiguous(), z, n, S, na, nb


def composite_merged_fwd(raw_a, raw_b, rank, z, white_bkgd=False, want_var=True, u=None):
    """composite_fwd(merge_rows(raw_a, raw_b, rank), z, 0, white_bkgd, want_var=want_var, u=u) from one launch, bit for bit, with no merged array:
    raw_a [n,na,4], raw_b [n,nb,4], rank [n,na+nb] (int32, a permutation per ray: sample_pdf's merge_rank), z [n,na+nb] sorted."""
    raw_a, raw_b, rank, z, n, S, na, nb = _merged_args("composite_merged_fwd", raw_a, raw_b, rank, z)
    dev = z.device
    p = L.CompositeMergedParams()
    p.n, p.na, p.nb, p.white_bkgd = n, na, nb, int(white_bkgd)
    out = _alloc_maps(p, n, S, dev, want_var and S >= 2)
    p.raw_a, p.raw_b, p.rank, p.z = _ptr(raw_a) if na else None, _ptr(raw_b) if nb else None, _ptr(rank), _ptr(z)
    u = _bind_wu("composite_merged_fwd", p, out, u)
    _launch("ucnerf_composite_merged_fwd", p, dev)
    return out


def composite_merged_bwd(raw_a, raw_b, rank, z, g_rgb=None, g_depth=None, g_acc=None, g_weights=None, white_bkgd=False, out=None):
    """(g_raw_a [n,na,4], g_raw_b [n,nb,4]): composite_bwd(merge_rows(raw_a, raw_b, rank), z, ...) taken back through rank, from one launch, bit for
    bit, with no merged array.  The upstream gradients (each optional) are in merged order.  out: (g_raw_a, g_raw_b) buffers to write into --
    every row is written, whatever they held."""
    raw_a, raw_b, rank, z, n, S, na, nb = _merged_args("composite_merged_bwd", raw_a, raw_b, rank, z)
    gs = [_opt(g) for g in (g_rgb, g_depth, g_acc, g_weights)]
    for g, numel, name in zip(gs, (3 * n, n, n, n * S), ("g_rgb", "g_depth", "g_acc", "g_weights")):
        if g is not None and g.numel() != numel:
            raise RuntimeError("uc_nerf_amd.composite_merged_bwd: %s has %d elements, expected %d" % (name, g.numel(), numel))
    if out is None:
        out = (torch.empty_like(raw_a), torch.empty_like(raw_b))
    g_a, g_b = out
    if (tuple(g_a.shape) != (n, na, 4) or tuple(g_b.shape) != (n, nb, 4) or g_a.dtype != torch.float32 or g_b.dtype != torch.float32
            or not g_a.is_contiguous() or not g_b.is_contiguous() or g_a.device != z.device or g_b.device != z.device):
        raise RuntimeError("uc_nerf_amd.composite_merged_bwd: out must be contiguous float32 (g_raw_a [n,na,4], g_raw_b [n,nb,4]) on the device")
    p = L.CompositeMergedBwdParams()
    p.n, p.na, p.nb, p.white_bkgd = n, na, nb, int(white_bkgd)
    p.raw_a, p.raw_b, p.rank, p.z = _ptr(raw_a) if na else None, _ptr(raw_b) if nb else None, _ptr(rank), _ptr(z)
    p.g_rgb, p.g_depth, p.g_acc, p.g_weights = (_ptr(g) for g in gs)
    p.g_raw_a, p.g_raw_b = _ptr(g_a) if na else None, _ptr(g_b) if nb else None
    _launch("ucnerf_composite_merged_bwd", p, z.device)
    return g_a, g_b


class _CompositeMerged(torch.autograd.Function):
    """raw2outputs (live variant) over the rows of a sorted merge: differentiable w.r.t. raw_a and raw_b through rgb_map, depth_map, acc_map and
    weights.  Upstream gradients autograd leaves out (None) reach the kernel as NULL pointers."""

    @staticmethod
    def forward(ctx, raw_a, raw_b, rank, z, white_bkgd):
        out = composite_merged_fwd(raw_a, raw_b, rank, z, white_bkgd)
        ctx.save_for_backward(raw_a, raw_b, rank, z)
        ctx.white_bkgd = white_bkgd
        ctx.set_materialize_grads(False)
        var = out.get("var", torch.zeros_like(out["acc"]))
        ctx.mark_non_differentiable(out["disp"], var)
        return out["rgb"], out["depth"], out["acc"], out["weights"], out["disp"], var

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_acc, g_weights, _g_disp, _g_var):
        raw_a, raw_b, rank, z = ctx.saved_tensors
        g_a, g_b = composite_merged_bwd(raw_a, raw_b, rank, z, g_rgb, g_depth, g_acc, g_weights, ctx.white_bkgd)
        return g_a, g_b, None, None, None


def composite_merged(raw_a, raw_b, rank, z, white_bkgd=False):
    """(rgb, depth, acc, weights, disp, var) of composite(merge_rows(raw_a, raw_b, rank), z, white_bkgd) with no merged array, forward
    (composite_merged_fwd) and backward (composite_merged_bwd): gradients for raw_a and raw_b, each in its own order."""
    return _CompositeMerged.apply(raw_a, raw_b, rank, z, bool(white_bkgd))


def composite_fold_grads(weights, depth, acc, u=None, g_var=None, g_disp=None, g_wu=None, g_depth=None, g_acc=None, g_weights=None, want_g_u=None,
                         out=None):
    """(g_depth', g_acc', g_weights', g_u): the upstream gradients of the compositing's extra maps -- g_var [n], g_disp [n], g_wu [n] (of
    sum_i w_i u_i), each optional -- folded into those of depth, acc and weights (each optional: None = zero), ready for composite_bwd /
    composite_merged_bwd; g_u [n,S] = g_wu * weights is the gradient of u (None unless want_g_u; default: whenever u is given).
    weights [n,S], depth [n], acc [n]: the forward's outputs (merged order on the merged route); u [n,S]: its per-sample uncertainty.
    out: (g_depth', g_acc', g_weights', g_u or None) buffers to write into -- every element is written, whatever they held."""
    weights, depth, acc = _f32(weights, "weights"), _f32(depth, "depth"), _f32(acc, "acc")
    if weights.dim() != 2:
        raise RuntimeError("uc_nerf_amd.composite_fold_grads: weights must be [n,S]")
    n, S = weights.shape
    dev = weights.device
    u = _opt(u, "u")
    named = dict(depth=(depth, n), acc=(acc, n), u=(u, n * S))
    ups = dict(g_var=(g_var, n), g_disp=(g_disp, n), g_wu=(g_wu, n), g_depth=(g_depth, n), g_acc=(g_acc, n), g_weights=(g_weights, n * S))
    for name, (g, numel) in ups.items():
        named[name] = (_opt(g, name), numel)
    for name, (t, numel) in named.items():
        if t is not None and (t.numel() != numel or t.device != dev):
            raise RuntimeError("uc_nerf_amd.composite_fold_grads: %s has %d elements on %s, expected %d on %s" % (name, t.numel(), t.device, numel, dev))
    if want_g_u is None:
        want_g_u = u is not None
    if out is None:
        out = (torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, S, device=dev), torch.empty(n, S, device=dev) if want_g_u else None)
    o_depth, o_acc, o_w, o_u = out
    for t, numel, name in ((o_depth, n, "g_depth'"), (o_acc, n, "g_acc'"), (o_w, n * S, "g_weights'"), (o_u, n * S, "g_u")):
        if t is None and name == "g_u":
            continue
        if t is None or t.dtype != torch.float32 or t.numel() != numel or not t.is_contiguous() or t.device != dev:
            raise RuntimeError("uc_nerf_amd.composite_fold_grads: out must be contiguous float32 (g_depth' [n], g_acc' [n], g_weights' [n,S], g_u [n,S] or "
                               "None) on the device; %s is not" % name)
    p = L.CompositeFoldParams()
    p.n, p.S = n, S
    p.weights, p.depth, p.acc, p.u = _ptr(weights), _ptr(depth), _ptr(acc), _ptr(u)
    p.g_var, p.g_disp, p.g_wu = (_ptr(named[k][0]) for k in ("g_var", "g_disp", "g_wu"))
    p.g_depth, p.g_acc, p.g_weights = (_ptr(named[k][0]) for k in ("g_depth", "g_acc", "g_weights"))
    p.g_depth_out, p.g_acc_out, p.g_weights_out, p.g_u = _ptr(o_depth), _ptr(o_acc), _ptr(o_w), _ptr(o_u)
    _launch("ucnerf_composite_fold_grads", p, dev)
    return o_depth, o_acc, o_w, o_u


def _maps_outputs(ctx, out):
    """The output tuple of the *_maps functions from a forward's dict: var is differentiable where it exists (S >= 2; zeros without history
    otherwise, as composite() returns them), wu is there when u was given."""
    var = out.get("var")
    if var is None:
        var = torch.zeros_like(out["acc"])
        ctx.mark_non_differentiable(var)
    res = (out["rgb"], out["depth"], out["acc"], out["weights"], out["disp"], var)
    return res + (out["wu"],) if "wu" in out else res


def _maps_fold(ctx, u, weights, depth, acc, g_depth, g_acc, g_weights, g_disp, g_var, g_wu, u_arg):
    """(g_depth, g_acc, g_weights, g_u) for the existing backward launch: the fold launch when a gradient of an extra map arrived, the
    upstream gradients as they are otherwise."""
    if g_var is None and g_disp is None and g_wu is None:
        return g_depth, g_acc, g_weights, None
    return composite_fold_grads(weights, depth, acc, u, g_var, g_disp, g_wu, g_depth, g_acc, g_weights,
                                want_g_u=u is not None and g_wu is not None and ctx.needs_input_grad[u_arg])


class _CompositeMaps(torch.autograd.Function):
    """_Composite with every map differentiable: var, disp and wu hand their gradients to composite_fold_grads, composite_bwd does the rest."""

    @staticmethod
    def forward(ctx, raw, z, white_bkgd, u):
        out = composite_fwd(raw, z, 0, white_bkgd, u=u)
        ctx.save_for_backward(raw, z, u, out["weights"], out["depth"], out["acc"])
        ctx.white_bkgd = white_bkgd
        ctx.set_materialize_grads(False)
        return _maps_outputs(ctx, out)

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_acc, g_weights, g_disp, g_var, g_wu=None):
        raw, z, u, weights, depth, acc = ctx.saved_tensors
        g_depth, g_acc, g_weights, g_u = _maps_fold(ctx, u, weights, depth, acc, g_depth, g_acc, g_weights, g_disp, g_var, g_wu, 3)
        g_raw = composite_bwd(raw, z, g_rgb, g_depth, g_acc, g_weights, ctx.white_bkgd) if ctx.needs_input_grad[0] else None
        return g_raw, None, None, g_u


def composite_maps(raw, z, white_bkgd=False, u=None):
    """(rgb, depth, acc, weights, disp, var[, wu]) of composite(raw, z, white_bkgd) -- the same forward launch -- with EVERY map differentiable
    w.r.t. raw: a loss on var (unbiased variance of the weights), on disp or on wu = sum_i w_i u_i (returned when the per-sample uncertainty
    u [n,S] is given; u receives its gradient too) trains the network.  Backward: one composite_fold_grads launch, then composite_bwd; without
    a gradient on var, disp or wu the fold is skipped and the gradients are composite()'s, bit for bit.  var needs S >= 2 (S = 1: zeros without
    history, as composite() returns them).  disp has no gradient at a ray where the clamp of 1 / max(1e-10, depth / acc) is active."""
    return _CompositeMaps.apply(raw, z, bool(white_bkgd), u)


class _CompositeMergedMaps(torch.autograd.Function):
    """_CompositeMerged with every map differentiable; the fold sees weights, u and gradients in merged order and never raw or rank."""

    @staticmethod
    def forward(ctx, raw_a, raw_b, rank, z, white_bkgd, u):
        out = composite_merged_fwd(raw_a, raw_b, rank, z, white_bkgd, u=u)
        ctx.save_for_backward(raw_a, raw_b, rank, z, u, out["weights"], out["depth"], out["acc"])
        ctx.white_bkgd = white_bkgd
        ctx.set_materialize_grads(False)
        return _maps_outputs(ctx, out)

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_acc, g_weights, g_disp, g_var, g_wu=None):
        raw_a, raw_b, rank, z, u, weights, depth, acc = ctx.saved_tensors
        g_depth, g_acc, g_weights, g_u = _maps_fold(ctx, u, weights, depth, acc, g_depth, g_acc, g_weights, g_disp, g_var, g_wu, 5)
        g_a = g_b = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g_a, g_b = composite_merged_bwd(raw_a, raw_b, rank, z, g_rgb, g_depth, g_acc, g_weights, ctx.white_bkgd)
        return g_a, g_b, None, None, None, g_u


def composite_merged_maps(raw_a, raw_b, rank, z, white_bkgd=False, u=None):
    """composite_maps(merge_rows(raw_a, raw_b, rank), z, white_bkgd, u) with no merged array: composite_merged's forward launch, and in the
    backward one composite_fold_grads launch followed by composite_merged_bwd, bit for bit.  u [n,na+nb] and every map are in merged order."""
    return _CompositeMergedMaps.apply(raw_a, raw_b, rank, z, bool(white_bkgd), u)
