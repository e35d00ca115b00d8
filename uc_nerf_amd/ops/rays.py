"""The ray front end: ray generation, depth sampling, NDC projection, the one-launch ray builders and the positional embedding."""
import ctypes as C

import torch

from .. import _lib as L
from ._core import _dev_as, _dev_f32, _f32, _launch, _mat, _on, _ptr, _stream


def ray_gen(K, c2w, xs=None, ys=None, H=0, W=0, grid_start=0, n=None, opengl=False, want_origin=False, want_pix=False,
            device=None, w2c_dir=None):
    """Pinhole rays.  Either (xs, ys) pixel lists or a row-major grid range [grid_start, grid_start+n) of an
    HxW image.  Returns (rays_d[n,3], rays_o[n,3] or None, pix[2,n] or None); with `w2c_dir` a fourth element, the
    view-direction feature (d/|d|) @ R_dir^T [n,3] (what `dir_feature(rays_d, w2c_dir)` gives, from the same launch)."""
    p = L.RayGenParams()
    if xs is not None:
        xs, ys = _f32(xs, "xs"), _f32(ys, "ys")
        device, n = xs.device, xs.numel()
        p.xs, p.ys = _ptr(xs), _ptr(ys)
    else:
        if device is None:
            raise RuntimeError("uc_nerf_amd.ray_gen: grid mode needs a device")
        n = H * W - grid_start if n is None else n
    p.n, p.H, p.W, p.grid_start, p.opengl = n, H, W, grid_start, int(opengl)
    if opengl:
        p.K[0] = float(K)
    else:
        _mat(p.K, K, 3, 3)
    _mat(p.c2w, c2w, 3, 4)
    rays_d = torch.empty(n, 3, device=device)
    rays_o = torch.empty(n, 3, device=device) if want_origin else None
    pix = torch.empty(2, n, device=device) if want_pix else None
    p.rays_d, p.rays_o, p.pix = _ptr(rays_d), _ptr(rays_o), _ptr(pix)
    angle = None
    if w2c_dir is not None:
        _mat(p.w2c_dir, w2c_dir, 3, 4)
        angle = torch.empty(n, 3, device=device)
        p.angle = _ptr(angle)
    _launch("ucnerf_ray_gen", p, device)
    return (rays_d, rays_o, pix) if w2c_dir is None else (rays_d, rays_o, pix, angle)


class RaySampler:
    """ray_gen(xs, ys) + sample_stratified(n, S, near, far) from ONE launch, camera matrices bound once (they travel by value in
    the parameter structs: filling them per call costs more host time than the launch).  Call -> (rays_d [n,3], angle [n,3] or
    None, z [n,S])."""

    def __init__(self, K, c2w, S, near, far, w2c_dir=None, lindisp=False):
        self.rg, self.ss = L.RayGenParams(), L.SampleStratifiedParams()
        _mat(self.rg.K, K, 3, 3)
        _mat(self.rg.c2w, c2w, 3, 4)
        self.has_dir = w2c_dir is not None
        if self.has_dir:
            _mat(self.rg.w2c_dir, w2c_dir, 3, 4)
        self.ss.S, self.ss.lindisp, self.ss.near, self.ss.far = int(S), int(lindisp), float(near), float(far)

    def prepare(self, xs, ys, perturb=0.0, noise=None):
        """Binds inputs and freshly allocated outputs WITHOUT launching: (rays_d, angle, z) are filled by whoever runs the bound structs --
        `__call__` (ucnerf_ray_gen_sample) or a render pass handed this sampler as `gen=` (ABI v4: the gather-fused MLP launch of the coarse pass
        generates rays and depths in its own prologue)."""
        xs, ys = _f32(xs, "xs"), _f32(ys, "ys")
        n, device = xs.numel(), xs.device
        rg, ss = self.rg, self.ss
        rays_d = torch.empty(n, 3, device=device)
        angle = torch.empty(n, 3, device=device) if self.has_dir else None
        z = torch.empty(n, ss.S, device=device)
        rg.n, rg.xs, rg.ys, rg.rays_d, rg.angle = n, _ptr(xs), _ptr(ys), _ptr(rays_d), _ptr(angle)
        ss.n, ss.perturb, ss.z = n, float(perturb), _ptr(z)
        if perturb > 0:
            noise = _f32(noise if noise is not None else torch.rand(n, ss.S, device=device), "noise")
        ss.noise = _ptr(noise if perturb > 0 else None)
        self._alive = (xs, ys, noise)              # (until the launch that reads them is enqueued)
        return rays_d, angle, z

    def __call__(self, xs, ys, perturb=0.0, noise=None):
        out = self.prepare(xs, ys, perturb, noise)
        with _on(out[0].device):
            L.check(L.lib().ucnerf_ray_gen_sample(C.addressof(self.rg), C.addressof(self.ss), _stream()), "ucnerf_ray_gen_sample")
        return out


def ray_gen_sample(K, c2w, xs, ys, S, near, far, perturb=0.0, noise=None, lindisp=False, w2c_dir=None):
    return RaySampler(K, c2w, S, near, far, w2c_dir, lindisp)(xs, ys, perturb, noise)


def ndc_rays(H, W, focal_x, focal_y, near, rays_o, rays_d, variant):
    rays_o, rays_d = _f32(rays_o.reshape(-1, 3)), _f32(rays_d.reshape(-1, 3))
    p = L.NdcRaysParams()
    p.n, p.H, p.W, p.variant = rays_o.shape[0], int(H), int(W), variant
    p.focal_x, p.focal_y, p.near = float(focal_x), float(focal_y), float(near)
    out_o, out_d = torch.empty_like(rays_o), torch.empty_like(rays_d)
    p.rays_o, p.rays_d, p.out_o, p.out_d = _ptr(rays_o), _ptr(rays_d), _ptr(out_o), _ptr(out_d)
    _launch("ucnerf_ndc_rays", p, rays_o.device)
    return out_o, out_d


def dir_feature(rays_d, w2c_ref=None):
    """Returns (angle[n,3], cos_angle[n]): normalised direction rotated into the reference camera.  A float32 w2c_ref
    already on the rays' device ([3,4] or [4,4], contiguous) is read by the kernel in place -- no host read-back."""
    rays_d = _f32(rays_d, "rays_d")
    p = L.DirFeatureParams()
    p.n, p.has_ref = rays_d.shape[0], int(w2c_ref is not None)
    if (torch.is_tensor(w2c_ref) and w2c_ref.is_cuda and w2c_ref.dtype == torch.float32 and w2c_ref.device == rays_d.device
            and w2c_ref.dim() == 2 and w2c_ref.shape[0] >= 3 and w2c_ref.shape[1] == 4 and w2c_ref.is_contiguous()):
        p.w2c_ref_dev = _ptr(w2c_ref)
    elif w2c_ref is not None:
        _mat(p.w2c_ref, w2c_ref, 3, 4)
    angle = torch.empty_like(rays_d)
    cos = torch.empty(rays_d.shape[0], device=rays_d.device)
    p.rays_d, p.angle, p.cos_angle = _ptr(rays_d), _ptr(angle), _ptr(cos)
    _launch("ucnerf_dir_feature", p, rays_d.device)
    return angle, cos


def sample_stratified(rays, S, lindisp=False, perturb=0.0, noise=None, want_pts=True, n=None, near=None, far=None,
                      device=None):
    """ray_marcher depths.  Either `rays` [n,8] (per-ray near/far, optional points) or n + scalar near/far."""
    p = L.SampleStratifiedParams()
    if rays is not None:
        rays = _f32(rays, "rays")
        n, device = rays.shape[0], rays.device
    else:
        p.near, p.far, want_pts = float(near), float(far), False
    p.n, p.S, p.lindisp, p.perturb = n, int(S), int(lindisp), float(perturb)
    if perturb > 0:
        if noise is None:
            noise = torch.rand(n, S, device=device)
        noise = _f32(noise, "noise")
    z = torch.empty(n, S, device=device)
    pts = torch.empty(n, S, 3, device=device) if want_pts else None
    p.rays, p.noise, p.z, p.pts = _ptr(rays), _ptr(noise if perturb > 0 else None), _ptr(z), _ptr(pts)
    _launch("ucnerf_sample_stratified", p, device)
    return z, pts


def sample_cascade(near_far, S, t_rand=None, rays_o=None, rays_d=None):
    """near_far [n,6] per-ray cascade ranges -> sorted + stratified depths [n,S] (and points when rays given)."""
    near_far = _f32(near_far, "near_far")
    n = near_far.shape[0]
    p = L.SampleCascadeParams()
    p.n, p.S = n, int(S)
    t_rand = _f32(t_rand) if t_rand is not None else None
    z = torch.empty(n, S, device=near_far.device)
    pts = None
    if rays_d is not None:
        rays_o, rays_d = _f32(rays_o.reshape(-1)[:3]), _f32(rays_d)
        pts = torch.empty(n, S, 3, device=near_far.device)
    p.near_far, p.t_rand, p.rays_o, p.rays_d, p.z, p.pts = (_ptr(near_far), _ptr(t_rand), _ptr(rays_o), _ptr(rays_d),
                                                            _ptr(z), _ptr(pts))
    _launch("ucnerf_sample_cascade", p, near_far.device)
    return z, pts


def ndc_project(pts, w2c, K, inv_scale, near_far=None, sample_2d=False):
    """get_ndc_coordinate.  pts [N,S,3].  near_far: dict with near_1..far_3 ([N,S,1] tensors or scalars) and
    near/far scalars.  Returns dict(stage1, stage2, stage3, ndc) or a single tensor when sample_2d."""
    pts = _f32(pts, "pts")
    shp = pts.shape
    m = pts.numel() // 3
    p = L.NdcProjectParams()
    p.m, p.has_w2c, p.sample_2d = m, int(w2c is not None), int(sample_2d)
    if w2c is not None:
        _mat(p.w2c, w2c, 3, 4)
    _mat(p.K, K, 3, 3)
    s = torch.as_tensor(inv_scale, dtype=torch.float32).detach().cpu().reshape(-1)
    p.inv_scale[0], p.inv_scale[1] = float(s[0]), float(s[1])
    p.pts = _ptr(pts)
    dev = pts.device
    if sample_2d:
        out = torch.empty(shp, device=dev)
        p.out_ndc = _ptr(out)
        _launch("ucnerf_ndc_project", p, dev)
        return out
    keep, strides = [], set()
    for k in ("near_1", "far_1", "near_2", "far_2", "near_3", "far_3"):
        v = near_far[k]
        if torch.is_tensor(v) and v.numel() == m:
            v = _f32(v.to(dev).reshape(-1))
            strides.add(1)
        else:
            v = torch.as_tensor(v, dtype=torch.float32).reshape(-1)[:1].to(dev).contiguous()
            strides.add(0)
        keep.append(v)
        setattr(p, k, _ptr(v))
    if len(strides) != 1:
        raise RuntimeError("uc_nerf_amd.ndc_project: stage near/far must be all per-sample or all scalar")
    p.nf_stride = strides.pop()
    p.near, p.far = float(near_far["near"]), float(near_far["far"])
    outs = {k: torch.empty(shp, device=dev) for k in ("stage1", "stage2", "stage3", "ndc")}
    p.out_stage1, p.out_stage2, p.out_stage3, p.out_ndc = (_ptr(outs["stage1"]), _ptr(outs["stage2"]),
                                                           _ptr(outs["stage3"]), _ptr(outs["ndc"]))
    _launch("ucnerf_ndc_project", p, dev)
    return outs


_BRT_PREPARED = {}       # (ids + data pointers of the camera / hypothesis tensors, image size, S) -> (params struct with the constant fields set, the tensors kept alive)


def build_rays_test(H, W, grid_start, n, S, K, c2w, w2c_ref, K_ref, near_far_ref, depth_values, t_rand=None, want_ranges=False):
    """The evaluation loop's ray builder in ONE launch (utils/utils.py:600-739; ucnerf_build_rays_test): rays through pixels grid_start ..
    grid_start + n - 1 of the HxW grid, cascade ranges from the three depth_values [.., D_k, h_k, w_k], sorted + jittered depths, world points
    and the four normalised copies.  Every matrix is a DEVICE tensor read in place (K [3,3], c2w [4,4] or [3,4], w2c_ref, K_ref, near_far_ref
    [2]): nothing is read back to the host.  Called 80 times per image behind a drained stream, so its host time counts: the argument checks and
    the constant half of the parameter struct are done once per set of input tensors, the five coordinate arrays are one allocation.
    -> dict(rays_o [3], rays_d [n,3], z [n,S], pts / stage1 / stage2 / stage3 / ndc [n,S,3] (+ ranges [n,6]))."""
    dev = c2w.device
    # (keyed by ADDRESS, element type and -- for the hypothesis volumes -- shape: the caller's per-call views of the same memory, e.g.
    #  near_fars[ref_idx], are new objects every time; a key that does not match in full takes the checked route below)
    try:
        key = (int(H), int(W), int(S)) + tuple((t.data_ptr(), t.dtype, t.shape, t.is_contiguous()) for t in (K, c2w, w2c_ref, K_ref, near_far_ref, *depth_values))
    except AttributeError:              # (something that is not a tensor: converted below, not cached)
        key = None
    prep = _BRT_PREPARED.get(key) if key is not None else None
    if prep is None:
        K_, c2w_, w2c_, Kr_ = _dev_f32(K, "K", 9, dev), _dev_f32(c2w, "c2w", 12, dev), _dev_f32(w2c_ref, "w2c_ref", 12, dev), _dev_f32(K_ref, "K_ref", 9, dev)
        nf_ = _dev_f32(near_far_ref, "near_far_ref", 2, dev)
        if c2w_.shape[-1] != 4 or w2c_.shape[-1] != 4:
            raise RuntimeError("uc_nerf_amd.build_rays_test: c2w / w2c_ref must have 4 columns")
        p = L.BuildRaysTestParams()
        p.S, p.H, p.W = int(S), int(H), int(W)
        keep = [K_, c2w_, w2c_, Kr_, nf_]
        for k, dv in enumerate(depth_values):
            dv = _dev_f32(dv, "depth_values")
            keep.append(dv)
            p.dv_d[k], p.dv_h[k], p.dv_w[k] = dv.shape[-3], dv.shape[-2], dv.shape[-1]
            if dv.numel() != dv.shape[-3] * dv.shape[-2] * dv.shape[-1]:
                raise RuntimeError("uc_nerf_amd.build_rays_test: depth_values must be [1,D,h,w] (one batch entry)")
            p.depth_values[k] = dv.data_ptr()
        p.K, p.c2w, p.w2c_ref, p.K_ref, p.near_far_ref = K_.data_ptr(), c2w_.data_ptr(), w2c_.data_ptr(), Kr_.data_ptr(), nf_.data_ptr()
        prep = (p, keep)
        # cached only when every input was usable as it is (the prepared struct then points at the caller's own memory, which the key identifies)
        if key is not None and keep[0] is K and keep[1] is c2w and keep[2] is w2c_ref and keep[3] is K_ref and keep[4] is near_far_ref and all(a is b_ for a, b_ in zip(keep[5:], depth_values)):
            if len(_BRT_PREPARED) >= 8:        # (a handful of scenes at most: the cache must not grow with a caller that builds new tensors per call)
                _BRT_PREPARED.clear()
            _BRT_PREPARED[key] = prep
    p = prep[0]
    n, m = int(n), int(n) * int(S)
    if t_rand is not None:
        t_rand = _f32(t_rand, "t_rand")
        if t_rand.numel() != m:
            raise RuntimeError("uc_nerf_amd.build_rays_test: t_rand must be [n,S]")
    coords = torch.empty(5, n, int(S), 3, device=dev)                  # pts, stage1, stage2, stage3, ndc: one allocation, five views from one call
    pts, s1, s2, s3, ndc = coords.unbind(0)
    z, rays_d, rays_o = torch.empty(n, int(S), device=dev), torch.empty(n, 3, device=dev), torch.empty(3, device=dev)
    ranges = torch.empty(n, 6, device=dev) if want_ranges else None
    p.n, p.grid_start, p.t_rand = n, int(grid_start), _ptr(t_rand)
    p.rays_o, p.rays_d, p.near_far, p.z = rays_o.data_ptr(), rays_d.data_ptr(), _ptr(ranges), z.data_ptr()
    base, step = coords.data_ptr(), 12 * m
    p.pts, p.ndc1, p.ndc2, p.ndc3, p.ndc = base, base + step, base + 2 * step, base + 3 * step, base + 4 * step
    _launch("ucnerf_build_rays_test", p, dev)
    out = {"rays_o": rays_o, "rays_d": rays_d, "z": z, "pts": pts, "stage1": s1, "stage2": s2, "stage3": s3, "ndc": ndc}
    if want_ranges:
        out["ranges"] = ranges
    return out


def build_rays_train(imgs, K, c2w, w2c_ref, K_ref, near_far_ref, depth_values, S, patch_size, sel0=None, sel1=None, shift=None, ux=None, uy=None,
                     coords=None, t_rand=None, want_ranges=False):
    """The training step's ray builder in ONE launch (utils/utils.py:400-597; ucnerf_build_rays_train) behind the caller's draws: the rays of
    P patches of patch_size^2 pixels (sel0 / sel1 [P/2] int64, torch.multinomial's picks from the confidence and the uncertainty map as they are on
    the device; shift [P,2] int32, each patch's (row, col) shift inside its cell), then of the pixels (uy, ux) [n_uniform], then of
    coords [n_coord,2] (row, col); any segment may be left out.  imgs [N,V,3,H,W] is read at [0,0] under its own strides, depth_values are the
    three stages' [.., D_k, h_k, w_k]; every matrix is a DEVICE tensor read in place (K [3,3], c2w [4,4] or [3,4], w2c_ref, K_ref, near_far_ref
    [2]).  Nothing is read back to the host and nothing is uploaded.
    -> dict(rays_o [3], rays_d [R,3], colors [R,3], pix [2,R] int64 (row, col), z [R,S], pts / stage1 / stage2 / stage3 / ndc [R,S,3]
    (+ ranges [R,6])); the five coordinate arrays are one allocation."""
    if not (torch.is_tensor(imgs) and imgs.is_cuda):
        raise RuntimeError("uc_nerf_amd: imgs must live on a ROCm device")
    if imgs.dim() != 5 or imgs.shape[2] != 3 or imgs.dtype != torch.float32:
        raise RuntimeError("uc_nerf_amd.build_rays_train: imgs must be float32 [N,V,3,H,W], got %s %s" % (imgs.dtype, tuple(imgs.shape)))
    dev = imgs.device
    f32, S = torch.float32, int(S)
    K_, c2w_, w2c_, Kr_ = _dev_as(K, "K", f32), _dev_as(c2w, "c2w", f32), _dev_as(w2c_ref, "w2c_ref", f32), _dev_as(K_ref, "K_ref", f32)
    nf_ = _dev_as(near_far_ref, "near_far_ref", f32)
    if K_.numel() < 9 or Kr_.numel() < 9 or nf_.numel() < 2 or c2w_.numel() < 12 or w2c_.numel() < 12 or c2w_.shape[-1] != 4 or w2c_.shape[-1] != 4:
        raise RuntimeError("uc_nerf_amd.build_rays_train: K / K_ref must be [3,3], c2w / w2c_ref [3,4] or [4,4], near_far_ref [2]")
    p = L.BuildRaysTrainParams()
    p.S, p.H, p.W, p.ps = S, imgs.shape[3], imgs.shape[4], int(patch_size)
    p.imgs = imgs.data_ptr()                                             # element [0,0,0,0,0]
    p.img_stride_c, p.img_stride_h, p.img_stride_w = imgs.stride(2), imgs.stride(3), imgs.stride(4)
    keep = [K_, c2w_, w2c_, Kr_, nf_]
    for k, dv in enumerate(depth_values):
        dv = _dev_as(dv, "depth_values", f32)
        keep.append(dv)
        if dv.dim() < 3 or dv.numel() != dv.shape[-3] * dv.shape[-2] * dv.shape[-1]:
            raise RuntimeError("uc_nerf_amd.build_rays_train: depth_values must be [1,D,h,w] (one batch entry)")
        p.dv_d[k], p.dv_h[k], p.dv_w[k] = dv.shape[-3], dv.shape[-2], dv.shape[-1]
        p.depth_values[k] = dv.data_ptr()
    p.K, p.c2w, p.w2c_ref, p.K_ref, p.near_far_ref = K_.data_ptr(), c2w_.data_ptr(), w2c_.data_ptr(), Kr_.data_ptr(), nf_.data_ptr()
    if (sel0 is None) != (sel1 is None) or (sel0 is None) != (shift is None):
        raise RuntimeError("uc_nerf_amd.build_rays_train: sel0, sel1 and shift come together")
    if sel0 is not None:
        sel0, sel1, shift = _dev_as(sel0, "sel0", torch.int64), _dev_as(sel1, "sel1", torch.int64), _dev_as(shift, "shift", torch.int32)
        if sel0.numel() != sel1.numel() or shift.numel() != 4 * sel0.numel():
            raise RuntimeError("uc_nerf_amd.build_rays_train: sel0 / sel1 must be [P/2] and shift [P,2]")
        p.P, p.sel0, p.sel1, p.shift = 2 * sel0.numel(), sel0.data_ptr(), sel1.data_ptr(), shift.data_ptr()
    if (ux is None) != (uy is None):
        raise RuntimeError("uc_nerf_amd.build_rays_train: ux and uy come together")
    if ux is not None:
        ux, uy = _dev_as(ux, "ux", f32), _dev_as(uy, "uy", f32)
        if ux.numel() != uy.numel():
            raise RuntimeError("uc_nerf_amd.build_rays_train: ux and uy must have the same length")
        p.n_uniform, p.ux, p.uy = ux.numel(), ux.data_ptr(), uy.data_ptr()
    if coords is not None:
        if not (torch.is_tensor(coords) and coords.is_cuda):
            raise RuntimeError("uc_nerf_amd: coords must live on a ROCm device")
        if coords.dim() != 2 or coords.shape[1] < 2:
            raise RuntimeError("uc_nerf_amd.build_rays_train: coords must be [n,2] (row, col)")
        if coords.dtype != f32 or (coords.shape[0] > 0 and coords.stride(1) != 1):
            coords = coords.float().contiguous()
        p.n_coord, p.coords, p.coord_stride = coords.shape[0], coords.data_ptr(), coords.stride(0)
    n = p.P * p.ps * p.ps + p.n_uniform + p.n_coord
    m = n * S
    if t_rand is not None:
        t_rand = _dev_as(t_rand, "t_rand", f32)
        if t_rand.numel() != m:
            raise RuntimeError("uc_nerf_amd.build_rays_train: t_rand must be [R,S] = [%d,%d]" % (n, S))
    buf = torch.empty(5, n, S, 3, device=dev)                          # pts, stage1, stage2, stage3, ndc: one allocation, five views from one call
    pts, s1, s2, s3, ndc = buf.unbind(0)
    z, rays_d, rays_o, colors = torch.empty(n, S, device=dev), torch.empty(n, 3, device=dev), torch.empty(3, device=dev), torch.empty(n, 3, device=dev)
    pix = torch.empty(2, n, dtype=torch.int64, device=dev)
    ranges = torch.empty(n, 6, device=dev) if want_ranges else None
    p.t_rand, p.rays_o, p.rays_d, p.colors, p.pix = _ptr(t_rand), rays_o.data_ptr(), rays_d.data_ptr(), colors.data_ptr(), pix.data_ptr()
    p.near_far, p.z = _ptr(ranges), z.data_ptr()
    base, step = buf.data_ptr(), 12 * m
    p.pts, p.ndc1, p.ndc2, p.ndc3, p.ndc = base, base + step, base + 2 * step, base + 3 * step, base + 4 * step
    _launch("ucnerf_build_rays_train", p, dev)
    out = {"rays_o": rays_o, "rays_d": rays_d, "colors": colors, "pix": pix, "z": z, "pts": pts, "stage1": s1, "stage2": s2, "stage3": s3, "ndc": ndc}
    if want_ranges:
        out["ranges"] = ranges
    return out


def embed(x, n_freqs, layout=0):
    x = _f32(x, "x")
    if x.shape[-1] != 3:
        raise RuntimeError("uc_nerf_amd.embed: last dimension must be 3")
    out = torch.empty(*x.shape[:-1], 3 + 6 * n_freqs, device=x.device)
    p = L.EmbedParams()
    p.m, p.n_freqs, p.layout, p.x, p.out = x.numel() // 3, n_freqs, layout, _ptr(x), _ptr(out)
    _launch("ucnerf_embed", p, x.device)
    return out
