"""The feature gather: its sources (channel-last views, repack) and the forward / backward wrappers."""
import ctypes as C

import torch

from .. import _lib as L
from ._core import _f32, _launch, _on, _opt, _ptr, _stream


def _strides_match(t, want):
    """Strides of `t` equal `want` on every dimension that has more than one element (torch leaves the others arbitrary)."""
    return all(n == 1 or st == w for n, st, w in zip(t.shape, t.stride(), want))


def _cl_ok(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32


def cl_volume_view(v):
    """`v` ([1,8,D,h,w] or [8,D,h,w]) as the [8,D,h,w] view the kernels can read IN PLACE, when its memory is [D,h,w,8] (what torch calls
    channels_last_3d: a Conv3d running in that memory format writes it) and 16-byte aligned; None otherwise."""
    if not _cl_ok(v) or v.dim() not in (4, 5) or (v.dim() == 5 and v.shape[0] != 1):
        return None
    t = v[0] if v.dim() == 5 else v
    c, d, h, w = t.shape
    if c != 8 or t.data_ptr() % 16 or not _strides_match(t, (1, h * w * 8, w * 8, 8)):
        return None
    return t


def cl_img_feat_view(f):
    """`f` ([V,1,8,H,W] or [V,8,H,W]) as the [V,8,H,W] view readable in place: memory [V,H,W,8] (channels_last of [V,8,H,W]), 16-byte aligned."""
    if not _cl_ok(f) or f.dim() not in (4, 5) or (f.dim() == 5 and f.shape[1] != 1):
        return None
    t = f[:, 0] if f.dim() == 5 else f
    V, c, H, W = t.shape
    if c != 8 or t.data_ptr() % 16 or not _strides_match(t, (H * W * 8, 1, W * 8, 8)):
        return None
    return t


def cl_imgs_view(im):
    """`im` ([1,V,3,H,W] or [V,3,H,W]) as ([V,3,H,W] view, values per pixel) when its memory is [V,H,W,3] (channels_last of [V,3,H,W]) or
    [V,H,W,4] (padded pixels, 16-byte aligned); None otherwise."""
    if not _cl_ok(im) or im.dim() not in (4, 5) or (im.dim() == 5 and im.shape[0] != 1):
        return None
    t = im[0] if im.dim() == 5 else im
    V, c, H, W = t.shape
    if c != 3:
        return None
    for px, align in ((3, 4), (4, 16)):
        if t.data_ptr() % align == 0 and _strides_match(t, (H * W * px, 1, W * px, px)):
            return t, px
    return None


class ChannelLastSources:
    """The gather's sources allocated in the layouts the kernels read, as torch tensors in the reference's SHAPES -- a convenience for a producer
    that can write its outputs there (or for sources that stay fixed over many steps); any tensor with these strides is treated the same way,
    wherever it was allocated (e.g. the output of an nn.Conv3d running in channels_last_3d):

        vols[k]   [1, 8, D, h, w]   memory [D,h,w,8] = torch.channels_last_3d                    <- volume_feature_no_ref of stage k + 1
        imgs      [1, V, 3, H, W]   memory [V,H,W,3] = torch.channels_last of [V,3,H,W]          <- imgs[:, 1:]
        img_feat  [V, 1, 8, H, W]   memory [V,H,W,8] = torch.channels_last of [V,8,H,W]          <- img_feat

    Handed to `rendering()` / `GatherSources` (as they are, or `.detach().requires_grad_()` of them), they are recognised by their strides: the
    pass reads them ZERO-COPY -- no per-step repack (25 us, 150 MB of traffic) -- and returns the source gradients with the same strides (no
    transposing pass either).  Every source is recognised on its own: those that do not qualify take the repack route, the others stay in place."""

    def __init__(self, vol_dhw, V, H, W, device):
        self.vol_dhw, self.V, self.H, self.W = [tuple(int(x) for x in t) for t in vol_dhw], int(V), int(H), int(W)
        self.vols = [torch.zeros(1, 8, d, h, w, device=device).contiguous(memory_format=torch.channels_last_3d) for d, h, w in self.vol_dhw]
        self.imgs = torch.zeros(V, 3, H, W, device=device).contiguous(memory_format=torch.channels_last).unsqueeze(0)
        self.img_feat = torch.zeros(V, 8, H, W, device=device).contiguous(memory_format=torch.channels_last).unsqueeze(1)

    @classmethod
    def from_reference_layout(cls, vols, imgs, img_feat):
        """Allocates channel-last tensors for these sources (reference layouts: volumes [1,8,D,h,w], imgs [1,V,3,H,W], img_feat [V,1,8,H,W]) and
        copies them in -- once; afterwards the new tensors ARE the sources."""
        dhw = [tuple(v.shape[-3:]) for v in vols]
        imgs4 = imgs.reshape(-1, 3, *imgs.shape[-2:])
        c = cls(dhw, imgs4.shape[0], imgs.shape[-2], imgs.shape[-1], imgs.device)
        with torch.no_grad():
            for dst, src in zip(c.vols, vols):
                dst.copy_(src.reshape(dst.shape))
            c.imgs.copy_(imgs.reshape(c.imgs.shape))
            c.img_feat.copy_(img_feat.reshape(c.img_feat.shape))
        return c


class GatherSources:
    """The gather's read-only geometry + source tensors, normalised to the layouts the kernels read.
    Any of `vols`, `conf`, `imgs` may be None: the corresponding units are masked out (their feature columns are
    left unwritten), which is how index_point_feature / build_color_volume run on the same kernel."""

    def __init__(self, vols, conf, imgs, img_feat, w2cs, intrinsics, hw=None, cl_bf16=False):
        """cl_bf16: the channel-last copies the fast gather reads (RenderPass.repack_sources) hold bf16 instead of fp32 -- SURVEY.md 8
        configs[4] "fp32 MLP / bf16 features": half the bytes per gather corner, features within bf16 rounding (2^-9 relative) of the
        fp32 sources'; source gradients are still accumulated in fp32 for the fp32 tensors."""
        self.cl_bf16 = bool(cl_bf16)
        self.mask = 0
        dev = None
        self.vols = [None, None, None]
        # PER SOURCE (ABI v5): a tensor whose memory already is the channel-last layout the fast kernels read -- a channels_last_3d volume, a
        # channels_last feature / image stack, each its own allocation -- is read IN PLACE (no repack, ever) and its gradient comes back with the
        # same strides.  Its reference-layout pointer is withheld (fill()): an entry point that reads channel-major sources fails loudly instead
        # of reading the wrong layout.  inplace[k]: 0..2 volumes, 3 img_feat, 4 imgs.
        self.inplace = [False] * 5
        self.rgb_stride = 4
        if vols is not None:
            if any(v is None for v in vols):
                raise RuntimeError("uc_nerf_amd: three cascade volumes or none")
            for k, v in enumerate(vols):
                t = None if cl_bf16 else cl_volume_view(v)
                self.inplace[k] = t is not None
                self.vols[k] = t if t is not None else _f32(v, "volume").reshape(v.shape[-4:])       # [8,D,h,w]
                if self.vols[k].shape[0] != 8:
                    raise RuntimeError("uc_nerf_amd: cascade volumes must have 8 channels")
            self.mask |= 0b111
            dev = self.vols[0].device
        self.conf = None
        if conf is not None:
            hw = tuple(conf.shape[-2:])
            self.conf = _f32(conf, "confidence").reshape(hw)
            self.mask |= 0b1000
            dev = self.conf.device
        self.imgs = self.img_feat = self.w2cs = self.intrinsics = None
        self.V = 1
        if imgs is not None:
            hw = tuple(imgs.shape[-2:])
            t = None if cl_bf16 else cl_imgs_view(imgs)
            if t is not None:
                self.imgs, self.rgb_stride = t
                self.inplace[4] = True
            else:
                self.imgs = _f32(imgs, "imgs").reshape(-1, 3, *hw)                     # [V,3,H,W]
            self.V = self.imgs.shape[0]
            dev = self.imgs.device
            t = None if (cl_bf16 or img_feat is None) else cl_img_feat_view(img_feat)
            if t is not None and t.shape[0] == self.V and tuple(t.shape[2:]) == hw:
                self.img_feat = t
                self.inplace[3] = True
            else:
                self.img_feat = (_f32(img_feat, "img_feat").reshape(self.V, 8, *hw) if img_feat is not None
                                 else torch.zeros(self.V, 8, *hw, device=dev))
            self.w2cs = torch.as_tensor(w2cs, dtype=torch.float32)[:, :3, :4].reshape(-1, 12).to(dev).contiguous()
            self.intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32).reshape(-1, 9).to(dev).contiguous()
            if self.w2cs.shape[0] != self.V or self.intrinsics.shape[0] != self.V:
                raise RuntimeError("uc_nerf_amd: %d source images but %d poses / %d intrinsics"
                                   % (self.V, self.w2cs.shape[0], self.intrinsics.shape[0]))
            self.mask |= ((1 << self.V) - 1) << 4
        if hw is None or self.mask == 0:
            raise RuntimeError("uc_nerf_amd: the gather needs at least one source")
        self.H, self.W = int(hw[0]), int(hw[1])
        self.F = 24 + 12 * self.V + 1
        self.device = dev
        self.full = self.mask == (0b1111 | (((1 << self.V) - 1) << 4))
        self.zero_copy = all(self.inplace)          # every source is read in place: nothing to repack, now or later
        # ucnerf_cl_sources of the in-place sources alone, and of all five once repack() has completed them (shared by every
        # RenderPass bound to these sources); _cl: the buffer the repacked ones live in
        self.cl_inplace = L.ClSources()
        for k in range(3):
            self.cl_inplace.vol[k] = _ptr(self.vols[k]) if self.inplace[k] else None
        self.cl_inplace.img_feat = _ptr(self.img_feat) if self.inplace[3] else None
        self.cl_inplace.imgs = _ptr(self.imgs) if self.inplace[4] else None
        self.cl_inplace.rgb_stride, self.cl_inplace.bf16 = self.rgb_stride, int(self.cl_bf16)
        self.cl_all = self.cl_inplace if self.zero_copy else None
        self._cl = None
        # What the copies in _cl are copies OF, per source (0..2 volumes, 3 img_feat, 4 imgs): the source tensor's version counter at the moment its
        # copy was built (None: not built, or built by a launch that was only recorded into a graph).  This object holds the tensors, so their
        # addresses cannot come back under another tensor while it lives; the counter says whether they were written since.  _cl_gen counts the
        # allocations of _cl (nothing here is keyed on an address); a RenderPass takes cl_all anew at every call and needs no counter.
        self._cl_versions = [None] * 5
        self._cl_gen = 0
        self._repack_p, self._cl_floats = None, None        # repack()'s own parameter struct and the floats _cl must have, made at its first call

    def _cl_tensors(self):
        return self.vols + [self.img_feat, self.imgs]

    def stale_mask(self):
        """Bit k set: source k is repacked (not read in place) and its channel-last copy is not known to hold the tensor's current values -- the
        `source_mask` of ucnerf_gather_repack_masked that brings the copies up to date.  Seen: every write that bumps the tensor's version
        counter (in-place ops, copy_, an optimizer's step).  NOT seen: a write through `.data`, or by another library through the raw pointer --
        RenderPass.repack_sources(force=True) after those."""
        m = 0
        for k, t in enumerate(self._cl_tensors()):
            if t is not None and not self.inplace[k] and self._cl_versions[k] != t._version:
                m |= 1 << k
        return m

    def adopt_copies(self, old):
        """Takes over the channel-last copies of `old`, a GatherSources of the very same volumes, images and image features (same tensors, same
        versions: the caller vouches for that) -- with what is known about them.  Sizes that do not match are found by repack(), which then
        starts over."""
        self._cl, self.cl_all, self._cl_versions, self._cl_gen = old._cl, old.cl_all, list(old._cl_versions), old._cl_gen

    def repack(self, force=True):
        """(Re)builds the channel-last copies of the sources that are not handed over in place, in _cl; cl_all then names all five.
        force=True: all of them.  force=False: existing ones are reused as they are, whatever happened to the tensors since.  force="changed":
        only the sources whose tensor was written since its copy was made (stale_mask: by version counter; see there for what that cannot see);
        no launch and no library call when nothing changed.  All are built when there are no copies yet or the buffer does not fit these sources
        (adopt_copies).  While the stream is being captured "changed" means True: a replay cannot ask the host what changed.
        Of the parameter struct the library reads H, W, vol_d / vol_h / vol_w, vol, img_feat, imgs (fill()), cfg.n_src (V) and cl (cl_inplace): nothing of a pass."""
        if self.zero_copy:                           # (never written: the arrays are the caller's)
            return
        if self._repack_p is None:
            p = self._repack_p = L.RenderParams()
            self.fill(p)
            p.cfg.n_src, p.cl = self.V, self.cl_inplace
            self._cl_floats = L.lib().ucnerf_gather_repack_floats(C.addressof(p))
        capturing = torch.cuda.is_current_stream_capturing() if self.device.type == "cuda" else False
        fresh = self._cl is None or self._cl.numel() != self._cl_floats or self.cl_all is None
        if fresh:
            self._cl = torch.empty(self._cl_floats, device=self.device)
            self.cl_all = L.ClSources()
            self._cl_versions = [None] * 5
            self._cl_gen += 1
        if fresh or (force and (capturing or force != "changed")):
            mask = L.REPACK_ALL
        else:
            mask = self.stale_mask() if force else 0         # (0: the step's usual case)
        if mask:
            with _on(self.device):
                L.check(L.lib().ucnerf_gather_repack_masked(C.addressof(self._repack_p), _ptr(self._cl), C.addressof(self.cl_all), mask, _stream()),
                        "ucnerf_gather_repack_masked")
            if not capturing:                        # (a recorded launch has not run: the copies are what they were)
                for k, t in enumerate(self._cl_tensors()):
                    if mask >> k & 1 and not self.inplace[k]:
                        self._cl_versions[k] = None if t is None else t._version

    def fill(self, p):
        p.V, p.H, p.W = self.V, self.H, self.W
        p.unit_mask = 0 if self.full else self.mask
        for k, v in enumerate(self.vols):
            if v is not None:
                p.vol_d[k], p.vol_h[k], p.vol_w[k] = v.shape[1], v.shape[2], v.shape[3]
            else:
                p.vol_d[k] = p.vol_h[k] = p.vol_w[k] = 1
            p.vol[k] = None if self.inplace[k] else _ptr(v)
        p.conf = _ptr(self.conf)
        p.imgs, p.img_feat = (None if self.inplace[4] else _ptr(self.imgs)), (None if self.inplace[3] else _ptr(self.img_feat))
        p.w2cs, p.intrinsics = _ptr(self.w2cs), _ptr(self.intrinsics)


def feat_gather_fwd(src, pts, ndc1, ndc2, ndc3, tiled=False, u_out=None):
    """u_out: optional [m] float32 tensor receiving the per-sample uncertainty 1 - sampled confidence."""
    pts, ndc1, ndc2, ndc3 = _opt(pts), _opt(ndc1), _opt(ndc2), _opt(ndc3)
    lead = next(t for t in (pts, ndc1, ndc3) if t is not None)
    m = lead.numel() // 3
    p = L.FeatGatherParams()
    src.fill(p)
    p.m, p.out_tiled = m, int(tiled)
    n_out = ((m + 31) // 32) * 32 * src.F if tiled else m * src.F
    feats = torch.empty(n_out, device=lead.device) if src.full else torch.zeros(n_out, device=lead.device)
    p.pts, p.ndc1, p.ndc2, p.ndc3, p.feats = _ptr(pts), _ptr(ndc1), _ptr(ndc2), _ptr(ndc3), _ptr(feats)
    if u_out is not None:
        if u_out.numel() != m or u_out.dtype != torch.float32 or not u_out.is_contiguous() or src.conf is None:
            raise RuntimeError("uc_nerf_amd.feat_gather_fwd: u_out must be a contiguous float32 [m] tensor (and the confidence map given)")
        p.u_out = _ptr(u_out)
    _launch("ucnerf_feat_gather_fwd", p, lead.device)
    return feats if tiled else feats.view(*lead.shape[:-1], src.F)


# route of ucnerf_feat_gather_bwd -> (volumes accumulated channel-last in the caller's arrays, image features likewise)
GATHER_BWD_ROUTES = {"scratch": (False, False), "direct": (False, False), "cl": (True, True), "cl_vols": (True, False), "cl_img_feat": (False, True)}


def feat_gather_bwd(src, pts, ndc1, ndc2, ndc3, g_feats, need=(True, True, True, True, True), route="scratch"):
    """Returns grads (g_vol1, g_vol2, g_vol3, g_conf, g_img_feat); entries not needed are None.
    route: which of the entry point's routes runs (include/ucnerf_hip.h, ucnerf_feat_gather_bwd):
      "scratch"      channel-last accumulation in a scratch buffer, then one transposing add (the default);
      "direct"       no scratch buffer: one atomic per corner and channel, straight into the channel-major arrays;
      "cl"           every source's gradient accumulated in a channel-last array of its own (g_cl), as RenderPass.backward does for sources read
                     in place; the gradients come back in the sources' shapes with channel-last strides.  The only route that serves
                     in-place sources;
      "cl_vols" / "cl_img_feat"   g_cl for the volumes / the image features alone, the other through the scratch buffer."""
    if route not in GATHER_BWD_ROUTES:
        raise ValueError("uc_nerf_amd.feat_gather_bwd: route must be one of %s, got %r" % (sorted(GATHER_BWD_ROUTES), route))
    cl_vol, cl_feat = GATHER_BWD_ROUTES[route]
    if (any(src.inplace[:3]) and not cl_vol) or (src.inplace[3] and not cl_feat):
        raise RuntimeError("uc_nerf_amd.feat_gather_bwd: channel-last sources take their gradients channel-last (route='cl')")

    def cl_zeros(t, perm):          # zeros of t's shape whose memory is channel-last (16-byte aligned: a fresh allocation)
        return torch.zeros([t.shape[i] for i in perm], device=t.device).permute([perm.index(i) for i in range(len(perm))])

    gv = [None if not (need[k] and v is not None) else cl_zeros(v, (1, 2, 3, 0)) if cl_vol else torch.zeros(v.shape, device=v.device)
          for k, v in enumerate(src.vols)]
    gc = torch.zeros_like(src.conf) if (need[3] and src.conf is not None) else None
    gi = None
    if need[4] and src.imgs is not None:
        gi = cl_zeros(src.img_feat, (0, 2, 3, 1)) if cl_feat else torch.zeros(src.img_feat.shape, device=src.img_feat.device)
    _feat_gather_bwd_into(src, pts, ndc1, ndc2, ndc3, g_feats, (gv[0], gv[1], gv[2], gc, gi), route)
    return gv[0], gv[1], gv[2], gc, gi


def _bind_gather_grads(bp, gv, gi, cl):
    """Hands a gather backward its gradient arrays (None: not wanted): the volumes' gv[0..2] and the image features' gi, in g_cl where cl[k] says
    the array is channel-last (k = 3: gi), in g_vol / g_img_feat otherwise.  Returns whether any is channel-major: those go through the scratch buffer."""
    for k in range(3):
        bp.g_vol[k], bp.g_cl.vol[k] = (None, _ptr(gv[k])) if cl[k] else (_ptr(gv[k]), None)
    bp.g_img_feat, bp.g_cl.img_feat = (None, _ptr(gi)) if cl[3] else (_ptr(gi), None)
    return any(g is not None and not c for g, c in zip((*gv, gi), cl))


def _feat_gather_bwd_into(src, pts, ndc1, ndc2, ndc3, g_feats, grads, route):
    """One call of ucnerf_feat_gather_bwd ACCUMULATING into `grads` (what feat_gather_bwd returned for the same sources and route)."""
    pts, ndc1, ndc2, ndc3, g_feats = _opt(pts), _opt(ndc1), _opt(ndc2), _opt(ndc3), _f32(g_feats)
    lead = next(t for t in (pts, ndc1, ndc3) if t is not None)
    cl_vol, cl_feat = GATHER_BWD_ROUTES[route]
    bp = L.FeatGatherBwdParams()
    src.fill(bp.fwd)
    bp.fwd.m = lead.numel() // 3
    bp.fwd.pts, bp.fwd.ndc1, bp.fwd.ndc2, bp.fwd.ndc3 = _ptr(pts), _ptr(ndc1), _ptr(ndc2), _ptr(ndc3)
    bp.g_feats = _ptr(g_feats)
    gv, gc, gi = grads[:3], grads[3], grads[4]
    bp.g_conf = _ptr(gc)
    via_scratch = _bind_gather_grads(bp, gv, gi, (cl_vol, cl_vol, cl_vol, cl_feat))
    bp.scratch = _ptr(_gather_scratch(src, bp.fwd, lead.device)) if (route == "scratch" or (via_scratch and route != "direct")) else None
    _launch("ucnerf_feat_gather_bwd", bp, lead.device)


def _gather_scratch(src, fwd_params, device):
    """Channel-last accumulation buffer of the gather backward, cached on the sources object."""
    n = L.lib().ucnerf_feat_gather_bwd_scratch_floats(C.addressof(fwd_params))
    buf = getattr(src, "_bwd_scratch", None)
    if buf is None or buf.numel() < n or buf.device != device:
        buf = torch.empty(max(int(n), 4), device=device)
        src._bwd_scratch = buf
    return buf


class _FeatGather(torch.autograd.Function):
    """Differentiable w.r.t. the three volumes, confidence and img_feat (never positions: SURVEY 3.2).
    Sources given as None are skipped (see GatherSources)."""

    @staticmethod
    def forward(ctx, vol1, vol2, vol3, conf, img_feat, imgs, w2cs, intrinsics, pts, ndc1, ndc2, ndc3):
        vols = None if vol1 is None else [vol1, vol2, vol3]
        src = GatherSources(vols, conf, imgs, img_feat, w2cs, intrinsics)
        ctx.src = src
        ctx.shapes = tuple(None if t is None else t.shape for t in (vol1, vol2, vol3, conf, img_feat))
        ctx.coords = (pts, ndc1, ndc2, ndc3)
        return feat_gather_fwd(src, pts, ndc1, ndc2, ndc3)

    @staticmethod
    def backward(ctx, g):
        pts, ndc1, ndc2, ndc3 = ctx.coords
        need = ctx.needs_input_grad[:5]
        grads = feat_gather_bwd(ctx.src, pts, ndc1, ndc2, ndc3, g.reshape(-1, ctx.src.F), need)
        out = [x.reshape(s) if (x is not None and s is not None) else None for x, s in zip(grads, ctx.shapes)]
        return tuple(out) + (None,) * 7


def feat_gather(vols, conf, img_feat, imgs, w2cs, intrinsics, pts, ndc1, ndc2, ndc3):
    return _FeatGather.apply(vols[0], vols[1], vols[2], conf, img_feat, imgs, w2cs, intrinsics, pts, ndc1, ndc2, ndc3)
