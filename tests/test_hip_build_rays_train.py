"""The one-launch training ray builder on the GPU (ucnerf_build_rays_train, ops.build_rays_train, the switch of utils.build_rays): fixture G18 from
its recorded draws, bit-identity with the composition of launches it replaces at the smallest shapes where the kernel can go wrong, the mirror's two
routes under one seed, no host read inside the op, repeatability."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_build_rays_train_host import g18_draws, pixel_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("rays_o", "rays_d", "colors", "pix", "z", "pts", "stage1", "stage2", "stage3", "ndc", "ranges")


def dev(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def close(a, b, atol=1e-5, rtol=1e-5):
    torch.testing.assert_close(a.cpu(), b.cpu(), atol=atol, rtol=rtol, equal_nan=True)


def make_case(H=24, W=32, ps=4, P=4, n_uniform=11, n_coord=5, S=12, pad3=0, D=(5, 4, 3), sel=None, imgs_layout="dense", c2w_rows=4, seed=0):
    """A seeded scene with every input of the op on the device (the draws are taken from a generator of the case's own: nothing here is under test)."""
    gen = torch.Generator().manual_seed(seed)
    V = 2
    if imgs_layout == "dense":
        imgs = torch.rand(1, V, 3, H, W, generator=gen)
    else:                                                                     # channel-last memory behind the same [1,V,3,H,W] shape
        imgs = torch.rand(1, V, H, W, 3, generator=gen).permute(0, 1, 4, 2, 3)
    dvs = []
    for k, div in enumerate((4, 2, 1)):
        h, w = (H - 1) // div + 1, (W - 1) // div + 1
        if k == 2:
            h, w = h + 2 * pad3, w + 2 * pad3
        lo = 1.0 + torch.rand(1, 1, h, w, generator=gen)
        dvs.append(torch.cat([lo + 0.6 * i / (D[k] - 1) + 0.3 * k for i in range(D[k])], 1))     # stages overlap: the sort has work to do
    ang = torch.tensor(0.2)
    c2w = torch.eye(4)
    c2w[:3, :3] = torch.tensor([[torch.cos(ang), 0, torch.sin(ang)], [0, 1, 0], [-torch.sin(ang), 0, torch.cos(ang)]])
    c2w[:3, 3] = torch.tensor([0.1, -0.2, 0.05])
    w2c_ref = torch.eye(4)
    w2c_ref[:3, 3] = torch.tensor([-0.05, 0.1, 0.2])
    K = torch.tensor([[40., 0, W / 2], [0, 42., H / 2], [0, 0, 1]])
    K_ref = torch.tensor([[41., 0, W / 2 - 0.5], [0, 39., H / 2 + 0.5], [0, 0, 1]])
    half = P // 2
    if sel is None:
        sel = torch.randint(0, H * W, (2, half), generator=gen)
    sel = torch.as_tensor(sel, dtype=torch.int64).reshape(2, half)
    shift = torch.randint(0, ps, (P, 2), generator=gen).int()
    ux, uy = torch.randint(0, W, (n_uniform,), generator=gen).float(), torch.randint(0, H, (n_uniform,), generator=gen).float()
    coords = torch.stack([torch.randint(0, H, (n_coord,), generator=gen), torch.randint(0, W, (n_coord,), generator=gen)], -1).float()
    R = P * ps * ps + n_uniform + n_coord
    c = types.SimpleNamespace(H=H, W=W, ps=ps, P=P, S=S, R=R, imgs=dev(imgs), K=dev(K), c2w=dev(c2w[:c2w_rows].contiguous()), w2c_ref=dev(w2c_ref),
                              K_ref=dev(K_ref), near_far_ref=dev(torch.tensor([1.0, 4.0])), dvs=[dev(d) for d in dvs],
                              sel0=dev(sel[0]) if P else None, sel1=dev(sel[1]) if P else None, shift=dev(shift) if P else None,
                              ux=dev(ux) if n_uniform else None, uy=dev(uy) if n_uniform else None, coords=dev(coords) if n_coord else None,
                              t_rand=dev(torch.rand(R, S, generator=gen)))
    c.plan, c.clamped = pixel_plan(H, W, ps, sel[0].numpy(), sel[1].numpy(), shift.numpy(), ux.numpy(), uy.numpy(), coords.numpy())
    return c


def fused(c, **kw):
    from uc_nerf_amd import ops
    return ops.build_rays_train(c.imgs, c.K, c.c2w, c.w2c_ref, c.K_ref, c.near_far_ref, c.dvs, c.S, c.ps, c.sel0, c.sel1, c.shift, c.ux, c.uy,
                                c.coords, c.t_rand, want_ranges=True, **kw)


def composed(c):
    """The launches the op replaces, on the pixels of the restated plan: ray_gen -> torch indexing -> sample_cascade -> ndc_project."""
    from uc_nerf_amd import ops
    from uc_nerf_amd.utils import utils as U
    pix_f = dev(torch.from_numpy(c.plan))
    rays_d, _, _ = ops.ray_gen(c.K, c.c2w, xs=pix_f[1].contiguous(), ys=pix_f[0].contiguous())
    rays_o = c.c2w[:3, -1].clone()
    pix = pix_f.long()
    colors = c.imgs[0, 0, :, pix[0], pix[1]].permute(1, 0)
    ranges = U._stage_ranges({"stage%d" % (k + 1): {"depth_values": c.dvs[k]} for k in range(3)}, pix)
    z, pts = ops.sample_cascade(ranges, c.S, c.t_rand, rays_o, rays_d)
    nd = ops.ndc_project(pts, c.w2c_ref, c.K_ref, torch.tensor([c.W - 1, c.H - 1]), U._near_far_dict(ranges, c.S, c.near_far_ref[0], c.near_far_ref[1]))
    return dict(nd, rays_o=rays_o, rays_d=rays_d, colors=colors, pix=pix, z=z, pts=pts, ranges=ranges)


def test_g18_from_its_recorded_draws():
    from uc_nerf_amd import ops
    g = load_golden("g18_build_rays")
    sel0, sel1, shift, ux, uy, t_rand = g18_draws(g)
    o = ops.build_rays_train(dev(g["imgs"]), dev(g["K"]), dev(g["c2ws"])[0], dev(g["w2cs"])[0], dev(g["K"]), dev(g["near_fars"])[0],
                             [dev(g["stage%d_depth_values" % k]) for k in (1, 2, 3)], int(g["NS"]), int(g["patch_size"]), dev(sel0), dev(sel1),
                             dev(shift), dev(ux.float()), dev(uy.float()), dev(g["coords"]), dev(t_rand))
    R = g["pix"].shape[1]
    assert torch.equal(o["pix"].cpu(), g["pix"])
    assert torch.equal(o["colors"].cpu(), g["colors"])
    close(o["rays_d"], g["rays_d"]); close(o["rays_o"].reshape(1, 3).expand(R, -1), g["rays_o"])
    close(o["z"], g["z"], 1e-6, 1e-6); close(o["pts"], g["pts"], 1e-5, 1e-5)
    for k, name in (("stage1", "ndc1"), ("stage2", "ndc2"), ("stage3", "ndc3"), ("ndc", "ndc")):
        close(o[k], g[name], 2e-5, 2e-5)


CASES = {
    "g18_shape": dict(),
    "one_patch_per_half": dict(P=2),
    "no_patches": dict(P=0),
    "no_uniform": dict(n_uniform=0),
    "no_coords": dict(n_coord=0),
    "S3": dict(S=3),
    "S90": dict(S=90, D=(48, 32, 8)),
    "S96": dict(S=96, D=(48, 32, 8)),
    "odd_image_27x35": dict(H=27, W=35, ps=5, n_uniform=13),
    "stage3_padded_by_2": dict(pad3=2),
    "picks_at_both_ends": dict(P=2, sel=[[0], [24 * 32 - 1]]),
    "imgs_permuted_strides": dict(imgs_layout="channel_last"),
    "c2w_3x4": dict(c2w_rows=3),
    "c2w_4x4": dict(c2w_rows=4),
}


@pytest.mark.parametrize("name", list(CASES))
def test_bit_identical_to_the_composed_launches(name):
    kw = CASES[name]
    c = make_case(seed=len(name), **kw)
    if name == "picks_at_both_ends":
        # pick H W - 1: both of its cells are moved down by the upper clamp; pick 0 sits on the lower one (which no non-negative pick can cross)
        assert c.clamped == 2 and c.plan[:, 0].tolist() == [float(c.shift[0, 0]), float(c.shift[0, 1])]
        assert c.plan[0, c.ps * c.ps] == (c.H // c.ps - 2) * c.ps + int(c.shift[1, 0])
    if name == "stage3_padded_by_2":
        assert c.dvs[2].shape[-1] == c.W + 4
    if name == "imgs_permuted_strides":
        assert c.imgs.stride(2) == 1 and not c.imgs.is_contiguous()
    assert list(c.c2w.shape) == [kw.get("c2w_rows", 4), 4]
    got, want = fused(c), composed(c)
    assert got["pix"].dtype == torch.int64 and tuple(got["pix"].shape) == (2, c.R) and tuple(got["pts"].shape) == (c.R, c.S, 3)
    bad = [k for k in KEYS if not (got[k].shape == want[k].shape and torch.equal(got[k], want[k]))]
    assert not bad, bad
    assert torch.equal(got["pix"].cpu(), torch.from_numpy(c.plan).long())


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


def test_the_mirror_gives_the_same_tuple_on_both_routes():
    from uc_nerf_amd.utils import utils as U
    c = make_case(n_coord=9, seed=5)
    V = c.imgs.shape[1]
    conf = dev(torch.rand(c.H, c.W, generator=torch.Generator().manual_seed(6)).clamp(1e-3, 1 - 1e-3))
    pose_ref = {"w2cs": c.w2c_ref.repeat(V, 1, 1), "intrinsics": c.K_ref.repeat(V, 1, 1), "near_fars": c.near_far_ref.repeat(V, 1)}
    outputs = {"stage%d" % (k + 1): {"depth_values": c.dvs[k]} for k in range(3)}
    args = types.SimpleNamespace(patch_num=6, patch_size=4)
    outs = {}
    prev = U.set_build_rays_fused(False)
    try:
        for on in (True, False):
            U.set_build_rays_fused(on)
            torch.manual_seed(11)
            np.random.seed(11)
            outs[on] = U.build_rays(args, c.imgs, conf, None, c.coords, pose_ref, None, c.c2w.repeat(V, 1, 1), c.K.repeat(V, 1, 1), 120, c.S,
                                    with_depth=True, outputs=outputs)
    finally:
        U.set_build_rays_fused(prev)
    assert len(outs[True]) == len(outs[False]) == 9 and outs[True][0].shape == (120 + 9, c.S, 3)
    bad = [i for i, (a, b) in enumerate(zip(outs[True], outs[False])) if not _same(a, b)]
    assert not bad, bad


def test_the_op_reads_nothing_back_to_the_host():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    c = make_case(seed=7)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = fused(c)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.isfinite(got["pts"]).all()


def test_two_calls_give_equal_outputs():
    c = make_case(S=90, D=(48, 32, 8), seed=8)
    a, b = fused(c), fused(c)
    assert all(torch.equal(a[k], b[k]) for k in KEYS)
