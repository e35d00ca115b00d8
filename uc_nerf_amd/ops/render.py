"""RenderPass: the fused render launch (gather + MLP + compositing) and its backward, bound to one scene."""
import ctypes as C

import torch

from .. import _lib as L
from . import network                                  # (the backward mode is read through the module at call time: a copy here would go stale)
from ._core import _f32, _launch, _mat, _ptr
from .compositing import _u_stride
from .gather import _bind_gather_grads, _gather_scratch
from .network import _launch_split


class RenderPass:
    """Pre-bound arguments of ucnerf_render_fused_fwd for one scene; call it with (rays_d, z).

    rays_o / w2c_ref / K_ref / w2c_dir / near / far describe how the pass derives sample coordinates and the view-direction
    feature itself; a caller that hands both over (`coords=`, `dir_feat=`: the rendering() drop-in) may leave them None."""

    def __init__(self, src, pw, wstream, rays_o=None, w2c_ref=None, K_ref=None, w2c_dir=None, near=0.0, far=1.0, white_bkgd=False,
                 max_blocks=0):
        # pw / wstream may be packed for either precision ("f32" or "bf16x3"); the backward needs "f32"
        eye34, eye33 = torch.eye(3, 4), torch.eye(3)
        self.rays_o = (_f32(rays_o.reshape(-1)[:3].clone(), "rays_o") if rays_o is not None else torch.zeros(3, device=src.device))
        self.p = p = L.RenderParams()
        p.max_blocks = int(max_blocks)
        _mat(p.w2c_ref, w2c_ref if w2c_ref is not None else eye34, 3, 4)
        _mat(p.K_ref, K_ref if K_ref is not None else eye33, 3, 3)
        _mat(p.w2c_dir, w2c_dir if w2c_dir is not None else eye34, 3, 4)
        p.near, p.far = float(near), float(far)
        p.rays_o = _ptr(self.rays_o)
        self.set_sources(src)
        self.set_weights(pw, wstream)
        self.set_white_bkgd(white_bkgd)
        self._ws = None

    def set_sources(self, src):
        """Binds (other) gather sources; the fast gather is used once repack_sources() has run for them."""
        self.src = src
        src.fill(self.p)
        self.use_cl = src.zero_copy                  # (every source IS channel-last: nothing to repack, now or later)
        self._bind_cl(self.p)

    def _bind_cl(self, p):
        """Points a call's parameters at the channel-last sources as they are NOW: all five where this pass reads the copies (built first,
        should the buffer have been dropped under it), the in-place ones alone -- the others' entries NULL -- otherwise."""
        src = self.src
        if self.use_cl and src.cl_all is None:
            src.repack(False)
        p.cl = src.cl_all if self.use_cl else src.cl_inplace

    def set_weights(self, pw, wstream):
        self.pw, self.wstream = pw, wstream
        self.p.cfg = pw.cfg
        self.p.wstream = _ptr(wstream)

    def set_white_bkgd(self, white_bkgd):
        self.p.white_bkgd = int(bool(white_bkgd))

    def repack_sources(self, force=True):
        """Brings the channel-last copies of the sources up to date and makes this pass read them.  The copies belong to the sources object (every
        RenderPass bound to it reads the same ones): GatherSources.repack says what force=True / False / "changed" rebuild."""
        self.src.repack(force)
        self.use_cl = True
        self._bind_cl(self.p)

    @staticmethod
    def _coords(p, coords, m):
        """Coordinates handed over by the caller (dict pts, stage1, stage2, stage3, ndc; each [n,S,3]) instead of derived
        from (rays_d, z) -- what rendering() of the reference receives.  Returns the tensors to keep alive."""
        if coords is None:
            p.pts_in = p.ndc1_in = p.ndc2_in = p.ndc3_in = p.ndc_in = None
            return ()
        keep = [_f32(coords[k], k) for k in ("pts", "stage1", "stage2", "stage3", "ndc")]
        for t in keep:
            if t.numel() != 3 * m:
                raise RuntimeError("uc_nerf_amd.RenderPass: given coordinates must be [n,S,3]")
        p.pts_in, p.ndc1_in, p.ndc2_in, p.ndc3_in, p.ndc_in = (_ptr(t) for t in keep)
        return keep

    def __call__(self, rays_d, z, near_far=None, want=("acc", "weights", "var"), keep=(), events=None, dir_feat=None, coords=None, resample=None, gen=None,
                 w2c_dir_dev=None):
        """want may also name "u" (per-sample uncertainty u = 1 - sampled confidence [n,S], network/models.py:149) and
        "wu" (its composite sum_i w_i u_i [n]) -- the opt-in uncertainty outputs of SURVEY.md 8(a).
        resample: dict(u=draws [n,M] or [M], want_rank=False) -- the pass's compositing launch also draws the NEXT pass's depths from this pass's
        weights (data/ray_utils.py:216-219: mid-point bins, w[1:-1], sorted merge with z): adds out["samples"] [n,M], out["z_sorted"] [n,S+M]
        (and out["merge_rank"]), the results of sample_pdf(None, out["weights"], u, z_merge=z, from_coarse=True) bit for bit, with no launch of its own.
        gen: a RaySampler whose prepare() returned this call's (rays_d, dir_feat, z): the pass generates them itself (gather-fused kernel only) -- the
        values of RaySampler.__call__, bit for bit, with no launch of its own.
        w2c_dir_dev (with dir_feat=None): the rotation of the view-direction feature as a float32 DEVICE tensor ([3,4] or [4,4], contiguous), read by
        the kernels in place of the by-value w2c_dir -- rendering() holds pose_ref['w2cs'][0] on the device; on the tail route the features are
        then made inside the pass's one launch.
        want=None: evaluation only -- the pass ends with the network's outputs in out["raw"] (the only entry) and composites nothing."""
        eval_only = want is None
        if eval_only:
            want, keep = (), ("raw",)
            if resample is not None:
                raise RuntimeError("uc_nerf_amd.RenderPass: an evaluation-only pass (want=None) composites nothing and cannot re-sample")
        rays_d, z = _f32(rays_d, "rays_d"), _f32(z, "z")
        dir_feat = _f32(dir_feat, "dir_feat") if dir_feat is not None else None
        n, S = z.shape
        dev = z.device
        p = self.p
        p.n, p.S = n, S
        self._bind_cl(p)
        need = L.lib().ucnerf_render_workspace_floats(n, S, self.src.V)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=dev)
        near_far = _f32(near_far) if near_far is not None else None
        out = {} if eval_only else {"rgb": torch.empty(n, 3, device=dev), "depth": torch.empty(n, device=dev)}
        if "acc" in want:
            out["acc"] = torch.empty(n, device=dev)
        if "weights" in want:
            out["weights"] = torch.empty(n, S, device=dev)
        if "var" in want and S >= 2:
            out["var"] = torch.empty(n, device=dev)
        if "raw" in keep:
            out["raw"] = torch.empty(n, S, 4, device=dev)
        # training forward (raw + features kept, exact f32 or split-bf16): the features stay in the MLP's tile layout -- the forward reads
        # them as coalesced 128-byte rows (row-major: 4-byte pieces of 388-byte rows, 2x the launch time) and the backward takes them as they are
        training = "raw" in keep and "feats" in keep and self.pw.cfg.precision in (0, 1)
        if "feats" in keep:
            tiled = training and network._backward_mode == 0          # (the layer-by-layer backward reads row-major features)
            out["feats"] = torch.empty((n * S + 31) // 32 * 32 * self.src.F, device=dev) if tiled else torch.empty(n * S, self.src.F, device=dev)
            out["feats_tiled"] = tiled
        p.feats_tiled = int(bool(out.get("feats_tiled", False)))
        if "u" in want or "wu" in want:
            out["u"] = torch.empty(n, S, device=dev)
        if "wu" in want:
            out["wu"] = torch.empty(n, device=dev)
        p.u_sampled, p.wu_map = _ptr(out.get("u")), _ptr(out.get("wu"))
        _alive = self._coords(p, coords, n * S)      # noqa: F841 (kept until the launch is enqueued)
        p.rays_d, p.z, p.near_far, p.workspace = _ptr(rays_d), _ptr(z), _ptr(near_far), _ptr(self._ws)
        p.rgb_map, p.depth_map, p.acc_map = _ptr(out.get("rgb")), _ptr(out.get("depth")), _ptr(out.get("acc"))
        p.weights, p.var, p.raw, p.feats = _ptr(out.get("weights")), _ptr(out.get("var")), _ptr(out.get("raw")), _ptr(out.get("feats"))
        p.ev_mlp_start, p.ev_mlp_stop = events if events is not None else (None, None)
        p.train_workspace = None
        p.dir_feat = _ptr(dir_feat)
        p.w2c_dir_dev = None
        if w2c_dir_dev is not None and dir_feat is None:
            if not (w2c_dir_dev.is_cuda and w2c_dir_dev.dtype == torch.float32 and w2c_dir_dev.dim() == 2 and w2c_dir_dev.shape[0] >= 3
                    and w2c_dir_dev.shape[1] == 4 and w2c_dir_dev.is_contiguous()):
                raise RuntimeError("uc_nerf_amd.RenderPass: w2c_dir_dev must be a contiguous float32 [3,4] or [4,4] tensor on the device")
            p.w2c_dir_dev = _ptr(w2c_dir_dev)
        p.gen_rays = p.gen_depths = None
        if gen is not None:
            if self.pw.cfg.precision != 3 or coords is not None or near_far is not None or dir_feat is None:
                raise RuntimeError("uc_nerf_amd.RenderPass: gen= needs the gather-fused kernel (precision 'bf16x3_fused'), derived coordinates and the sampler's dir_feat")
            p.gen_rays, p.gen_depths = C.addressof(gen.rg), C.addressof(gen.ss)
        p.resample = None
        if resample is not None:
            u = _f32(resample["u"], "u")
            M = u.shape[-1]
            sp = self._resample_p = getattr(self, "_resample_p", None) or L.SamplePdfParams()
            sp.n, sp.n_bins, sp.n_samples, sp.n_merge, sp.from_coarse = n, S - 1, M, S, 1
            sp.u_stride = _u_stride(u, n, M, "RenderPass: resample draws")
            out["samples"] = torch.empty(n, M, device=dev)
            out["z_sorted"] = torch.empty(n, S + M, device=dev)
            sp.merge_rank = None
            if resample.get("want_rank"):
                out["merge_rank"] = torch.empty(n, S + M, dtype=torch.int32, device=dev)
                sp.merge_rank = _ptr(out["merge_rank"])
            sp.u, sp.samples, sp.z_sorted = _ptr(u), _ptr(out["samples"]), _ptr(out["z_sorted"])
            p.resample = C.addressof(sp)
        self._saved_for = None
        if training:
            # training forward (exact f32 or split-bf16): keep the MLP activations in the backward's workspace so that
            # backward() need not repeat the network forward
            need_b = L.lib().ucnerf_render_bwd_workspace_floats(n, S, self.src.V)
            if getattr(self, "_bwd_ws", None) is None or self._bwd_ws.numel() < need_b:
                self._bwd_ws = torch.empty(need_b, device=dev)
            p.train_workspace = _ptr(self._bwd_ws)
            p.train_bwd_mode = network._backward_mode          # (fixes the format the activations are kept in: 24-bit for the chain, fp32 layer by layer)
            self._saved_for = (n, S, out["raw"].data_ptr(), network._backward_mode)
        _launch_split(self.pw, "ucnerf_render_fused_fwd", p, dev)
        return out

    def saved_matches(self, n, S, raw):
        """True when the backward workspace still holds the activations the training forward kept for THIS (n, S, raw) -- no later forward
        overwrote them -- in the format of the current backward mode."""
        return getattr(self, "_saved_for", None) == (n, S, raw.data_ptr(), network._backward_mode)

    def backward(self, rays_d, z, kept, g_rgb, g_depth, flat, near_far=None, need=(True, True, True, True, True), coords=None,
                 dir_feat=None, f32_weights=None, flat_room=0):
        """Backward of the last-style forward call: `kept` = its outputs with keep=("raw", "feats").
        Returns (g_flat, g_vol1, g_vol2, g_vol3, g_conf, g_img_feat).  flat_room > n_params: g_flat is returned with that many floats (the
        rest zero) -- room a gradient bucket uses for its scalars and flags without another buffer (flat.FlatStore.grad_room).  A pass bound to bf16x3 weights runs its backward from
        the activations the training forward kept; should another forward have overwritten them, the network forward is
        repeated in f32 and needs `f32_weights` = (PackedWeights, stream) packed from the same parameters."""
        rays_d, z, flat, g_rgb = _f32(rays_d), _f32(z), _f32(flat), _f32(g_rgb)
        n, S = z.shape
        dev = z.device
        bp = L.RenderBwdParams()
        C.memmove(C.addressof(bp.fwd), C.addressof(self.p), C.sizeof(L.RenderParams))
        p = bp.fwd
        p.n, p.S = n, S
        self._bind_cl(p)
        near_far = _f32(near_far) if near_far is not None else None
        p.rays_d, p.z, p.near_far = _ptr(rays_d), _ptr(z), _ptr(near_far)
        p.raw, p.feats = _ptr(kept["raw"]), _ptr(kept["feats"])
        p.feats_tiled = int(bool(kept.get("feats_tiled", False)))
        if p.feats_tiled and network._backward_mode != 0:
            raise RuntimeError("uc_nerf_amd.RenderPass.backward: features kept in the tile layout need the gradient chain (set_backward_mode('chain'))")
        p.u_sampled = p.wu_map = None
        _alive = self._coords(p, coords, n * S)      # noqa: F841
        dir_feat = _f32(dir_feat, "dir_feat") if dir_feat is not None else None
        p.dir_feat = _ptr(dir_feat)
        p.ev_mlp_start = p.ev_mlp_stop = None
        saved = self.saved_matches(n, S, kept["raw"])
        ws = self._bwd_ws if saved else torch.empty(L.lib().ucnerf_render_bwd_workspace_floats(n, S, self.src.V), device=dev)
        bp.saved_valid = int(saved)
        bp.bwd_mode = network._backward_mode
        if not saved and self.pw.cfg.precision != 0:
            if f32_weights is None:
                raise RuntimeError("uc_nerf_amd.RenderPass.backward: the activations of this bf16x3 training forward were overwritten "
                                   "by a later forward; pass f32_weights=(PackedWeights, stream) to recompute them")
            p.cfg, p.wstream = f32_weights[0].cfg, _ptr(f32_weights[1])
        self._saved_for = None
        # ONE zero fill for all accumulated outputs (six separate torch.zeros were six 5-us launches per step): views of a flat buffer,
        # every segment padded to 16 bytes
        # a source read in place gets its gradient in the SAME layout (channel-last, accumulated straight into it by the gather backward: no scratch,
        # no transposing pass); the pool segment is then viewed with the source's strides -- what autograd's layout contract asks for
        src = self.src
        inp = src.inplace
        shapes = [(max(int(flat_room), self.pw.n_params),)] + \
                 [tuple(v.shape) if need[k] else None for k, v in enumerate(src.vols)] + \
                 [tuple(src.conf.shape) if need[3] else None, tuple(src.img_feat.shape) if need[4] else None]
        sizes = [0 if sh is None else (int(torch.Size(sh).numel()) + 3) // 4 * 4 for sh in shapes]
        pool = torch.zeros(sum(sizes), device=dev)
        segs, off = [], 0
        for sh, sz in zip(shapes, sizes):
            segs.append(None if sh is None else pool[off:off + int(torch.Size(sh).numel())])
            off += sz
        g_flat = segs[0]
        gv = []
        for k in range(3):
            if segs[1 + k] is None:
                gv.append(None)
            elif inp[k]:
                c, d, h, w = src.vols[k].shape
                gv.append(segs[1 + k].view(d, h, w, c).permute(3, 0, 1, 2))
            else:
                gv.append(segs[1 + k].view(shapes[1 + k]))
        gc = None if segs[4] is None else segs[4].view(shapes[4])
        if segs[5] is None:
            gi = None
        elif inp[3]:
            gi = segs[5].view(src.V, src.H, src.W, 8).permute(0, 3, 1, 2)
        else:
            gi = segs[5].view(shapes[5])
        g_depth = _f32(g_depth) if g_depth is not None else None
        bp.g_rgb, bp.g_depth, bp.flat_params, bp.g_flat, bp.workspace = _ptr(g_rgb), _ptr(g_depth), _ptr(flat), _ptr(g_flat), _ptr(ws)
        bp.g_conf = _ptr(gc)
        if _bind_gather_grads(bp, gv, gi, inp[:4]):
            gfwd = L.FeatGatherParams()
            src.fill(gfwd)
            bp.gather_scratch = _ptr(_gather_scratch(src, gfwd, dev))
        _launch("ucnerf_render_fused_bwd", bp, dev)
        return g_flat, gv[0], gv[1], gv[2], gc, gi
