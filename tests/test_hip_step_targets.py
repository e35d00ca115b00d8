"""ucnerf_step_targets through ops.step_targets on the device against torch's advanced indexing on the same device tensors (train.py:166-176):
bit for bit, for int64 and float32 coordinates; NaN plus a sticky status bit for a coordinate outside the image; empty and refused sizes; and
`DeviceScene.sample`'s views read where they are.

No case here provokes a fault.  Read in csrc/step_targets.hip: st_index() is the only place an offset is formed, from two indices st_coord()
returned; st_coord() returns -1 unless the coordinate lies in [-size, size) (for a float: and is a whole number) and wraps a negative one
into 0 .. size - 1; the kernel loads only where st_index() >= 0.  The coordinate load itself is at column n_rays + i < n_total or j <
patch_num * patch_size^2 <= n_total, which the host checks before the launch."""
import numpy as np
import pytest
import torch

import system_cases as YC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
POISON = -1234.5


def bits(t):
    return t.contiguous().view(torch.int32)


def inputs(case, seed=7):
    H, W, n_rays, patch_num, ps, n_total = case
    maps = [torch.from_numpy(m).to(DEV) for m in YC.gather_maps(H, W, seed)]
    pix = torch.from_numpy(YC.gather_coords(H, W, n_total, seed + 1)).to(DEV)
    return maps, pix


def torch_targets(maps, pix, n_rays, patch_num, ps):
    """train.py:166-176 on the device tensors."""
    sd, sw, dpt = maps
    pix = pix.long()
    patch_pts = patch_num * ps * ps
    return (sd[:, pix[0, n_rays:], pix[1, n_rays:]], sw[:, pix[0, n_rays:], pix[1, n_rays:]],
            dpt[:, pix[0, :patch_pts], pix[1, :patch_pts]].reshape(-1, ps, ps, 1))


@pytest.fixture(autouse=True)
def clean_status():
    from uc_nerf_amd import ops
    ops.step_targets_status_clear()
    yield
    assert ops.step_targets_status(clear=True) == 0        # every test leaves the device's own word as it found it


# ------------------------------------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("dtype", [torch.int64, torch.float32], ids=["int64", "float32"])
@pytest.mark.parametrize("case", YC.GATHER_CASES, ids=YC.GATHER_IDS)
def test_bit_equal_to_torch_indexing(case, dtype):
    from uc_nerf_amd import ops
    H, W, n_rays, patch_num, ps, n_total = case
    maps, pix = inputs(case)
    want = torch_targets(maps, pix, n_rays, patch_num, ps)
    assert patch_num == 0 or bool(torch.isinf(want[2]).any())                    # the specials are among what is read: dpt[0, 0] = inf ...
    if n_total == 15:
        assert int(bits(want[0])[0, 8]) == -2 ** 31                              # ... and sparse_depths[0, 0] = -0.0 (column 14 is (0, 0))
    got = ops.step_targets(*maps, pix.to(dtype), n_rays, patch_num, ps)
    n = n_total - n_rays
    assert [tuple(g.shape) for g in got] == [(1, n), (1, n), (patch_num, ps, ps, 1)]
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and not g.requires_grad and torch.equal(bits(g), bits(w))
    ref = YC.step_targets_ref(*[m.cpu().numpy() for m in maps], pix.cpu().numpy(), n_rays, patch_num, ps)
    assert all(np.array_equal(g.cpu().numpy().view(np.int32), r.view(np.int32)) for g, r in zip(got, ref))
    assert ops.step_targets_status() == 0


@pytest.mark.parametrize("case", YC.GATHER_CASES, ids=YC.GATHER_IDS)
def test_entry_point_overwrites_every_output_element_and_nothing_beside_them(case):
    """The C entry point on the test's own buffers: each output sits between two guard bands, all of it pre-filled with a poison pattern.  After
    the launch every output element holds torch's value (none is left poisoned) and every guard element still holds the poison."""
    from uc_nerf_amd import _lib as L
    H, W, n_rays, patch_num, ps, n_total = case
    maps, pix = inputs(case)
    want = [w.reshape(-1) for w in torch_targets(maps, pix, n_rays, patch_num, ps)]
    guard = 8
    bufs = [torch.full((w.numel() + 2 * guard,), POISON, device=DEV) for w in want]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = L.StepTargetsParams()
    p.H, p.W, p.n_total, p.n_rays, p.patch_num, p.patch_size, p.coord_is_float = H, W, n_total, n_rays, patch_num, ps, 0
    p.sparse_depths, p.sparse_weights, p.dpt, p.pixel_coordinates = (t.data_ptr() for t in (*maps, pix))
    p.target_depths, p.target_weights, p.patch_dpt = (b.data_ptr() + 4 * guard for b in bufs)
    p.status = status.data_ptr()
    L.call("ucnerf_step_targets", p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for b, w in zip(bufs, want):
        assert torch.equal(bits(b[guard:guard + w.numel()]), bits(w))
        assert bool((b[:guard] == POISON).all()) and bool((b[guard + w.numel():] == POISON).all())
    assert int(status) == 0


# ------------------------------------------------------------------------------------------------ 2. outside the image
@pytest.mark.parametrize("dtype", [torch.int64, torch.float32], ids=["int64", "float32"])
@pytest.mark.parametrize("where", ["depth", "patch", "both"])
def test_out_of_range_is_nan_in_its_element_and_a_sticky_bit(where, dtype):
    from uc_nerf_amd import ops
    case = YC.GATHER_CASES[2]                                  # 5 x 7, n_rays 6, two patches of 2 x 2, n_total 15
    H, W, n_rays, patch_num, ps, n_total = case
    maps, pix = inputs(case)
    want = [w.clone() for w in torch_targets(maps, pix, n_rays, patch_num, ps)]
    bad = pix.clone()
    depth_col, patch_col = n_rays + 4, 5
    if where in ("depth", "both"):
        bad[0, depth_col] = H                                  # row H: one past the last
    if where in ("patch", "both"):
        bad[1, patch_col] = -W - 1                             # col -W - 1: one before the first wrap
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.step_targets(*maps, bad.to(dtype), n_rays, patch_num, ps, status=status)
    nan_d = torch.zeros(n_total - n_rays, dtype=torch.bool, device=DEV)
    nan_p = torch.zeros(patch_num * ps * ps, dtype=torch.bool, device=DEV)
    nan_d[depth_col - n_rays] = where in ("depth", "both")
    nan_p[patch_col] = where in ("patch", "both")
    for g, w, mask in zip(got, want, (nan_d, nan_d, nan_p)):
        g, w = g.reshape(-1), w.reshape(-1)
        assert torch.isnan(g[mask]).all() and torch.equal(bits(g[~mask]), bits(w[~mask]))       # only those elements; the rest is torch's
    assert int(status) == {"depth": 0b01, "patch": 0b10, "both": 0b11}[where]
    ops.step_targets(*maps, pix.to(dtype), n_rays, patch_num, ps, status=status)                 # a clean call leaves the bits
    assert int(status) == {"depth": 0b01, "patch": 0b10, "both": 0b11}[where]
    assert ops.step_targets_status() == 0                                                        # the device's own word saw none of this


def test_the_device_word_is_sticky_until_cleared_and_a_fraction_is_out_of_range():
    from uc_nerf_amd import ops
    case = YC.GATHER_CASES[2]
    H, W, n_rays, patch_num, ps, n_total = case
    maps, pix = inputs(case)
    want = torch_targets(maps, pix, n_rays, patch_num, ps)
    frac = pix.float()
    frac[0, n_rays + 4] = 2.5                                  # in range as a number, but no pixel (a column past the 8 patch points)
    got = ops.step_targets(*maps, frac, n_rays, patch_num, ps)
    assert torch.isnan(got[0][0, 4]) and torch.isnan(got[1][0, 4]) and torch.equal(bits(got[2]), bits(want[2]))
    keep = torch.arange(n_total - n_rays, device=DEV) != 4
    assert torch.equal(bits(got[0][0, keep]), bits(want[0][0, keep])) and torch.equal(bits(got[1][0, keep]), bits(want[1][0, keep]))
    assert ops.step_targets_status() == 0b01
    clean = ops.step_targets(*maps, pix, n_rays, patch_num, ps)
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(clean, want))
    assert ops.step_targets_status() == 0b01                   # sticky across a clean call
    for value in (float("nan"), float("inf"), -float("inf"), 1e30):
        frac = pix.float()
        frac[1, 2] = value                                     # a patch ray's column
        got = ops.step_targets(*maps, frac, n_rays, patch_num, ps)
        assert torch.isnan(got[2].reshape(-1)[2]) and torch.equal(bits(got[0]), bits(want[0]))
    assert ops.step_targets_status(clear=True) == 0b11 and ops.step_targets_status() == 0
    ops.step_targets(*maps, frac, n_rays, patch_num, ps)
    ops.step_targets_status_clear()
    assert ops.step_targets_status() == 0


# ------------------------------------------------------------------------------------------------ 3. empty and refused sizes
def test_empty_parts_give_empty_tensors_and_leave_the_status():
    from uc_nerf_amd import ops
    maps, pix = inputs(YC.GATHER_CASES[2])
    status = torch.full((1,), 0b10, dtype=torch.int32, device=DEV)
    d, w, patch = ops.step_targets(*maps, pix[:, :6], 6, 1, 2, status=status)                    # n_total == n_rays
    assert d.shape == (1, 0) and w.shape == (1, 0) and patch.shape == (1, 2, 2, 1)
    d, w, patch = ops.step_targets(*maps, pix, 6, 0, 2, status=status)                           # patch_num == 0
    assert d.shape == (1, 9) and patch.shape == (0, 2, 2, 1)
    d, w, patch = ops.step_targets(*maps, pix[:, :6], 6, 0, 2, status=status)                    # both: no grid at all
    assert d.shape == (1, 0) and w.shape == (1, 0) and patch.shape == (0, 2, 2, 1)
    d, w, patch = ops.step_targets(*maps, pix[:, :0], 0, 0, 4, status=status)
    assert d.shape == (1, 0) and patch.shape == (0, 4, 4, 1)
    assert int(status) == 0b10


@pytest.mark.parametrize("n_total,n_rays,patch_num,ps,message", [(15, -1, 2, 2, "negative"), (6, 6, 2, 2, "more than the n_total"),
                                                                 (7, 6, 2, 2, "more than the n_total"), (15, 16, 2, 2, "above n_total"),
                                                                 (15, 6, -1, 2, "negative")])
def test_invalid_sizes_raise_einval(n_total, n_rays, patch_num, ps, message):
    from uc_nerf_amd import ops
    maps, pix = inputs(YC.GATHER_CASES[2])
    with pytest.raises(RuntimeError, match=r"ucnerf_step_targets failed \(-1\).*" + message):
        ops.step_targets(*maps, pix[:, :n_total], n_rays, patch_num, ps)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        ops.step_targets(maps[0], maps[1].double(), maps[2], pix, 6, 2, 2)
    with pytest.raises(RuntimeError, match="int64 or float32"):
        ops.step_targets(*maps, pix.int(), 6, 2, 2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.step_targets(*[m.cpu() for m in maps], pix.cpu(), 6, 2, 2)


# ------------------------------------------------------------------------------------------------ 4. the scene's views, in place
def test_scene_views_are_read_in_place():
    from uc_nerf_amd import ops
    scene = YC.tiny_scene(DEV)
    batch = scene.sample(3, [1, 5])
    sd, sw, dpt = batch["sparse_depths"], batch["sparse_depths_weight"], batch["dpt"]
    assert sd.data_ptr() == scene.depth_img[3].data_ptr() and sw.data_ptr() == scene.weight_img[3].data_ptr() and dpt.data_ptr() == scene.dpt[3].data_ptr()
    assert all(t.is_contiguous() and t.shape == (1, YC.H, YC.W) for t in (sd, sw, dpt))
    kp = scene.kp_coord[scene.offsets[3]:scene.offsets[4]].long()                                # the target's keypoints: (h, w)
    g = torch.Generator().manual_seed(3)
    patch = torch.stack([torch.randint(0, YC.H, (32,), generator=g), torch.randint(0, YC.W, (32,), generator=g)]).to(DEV)
    pix = torch.cat([patch, kp.t()], 1)
    want = torch_targets((sd, sw, dpt), pix, 32, 2, 4)
    assert bool((want[0] > 0).all())                                                             # the keypoints' pixels hold their depths
    decoy = torch.full((3, YC.H, YC.W), POISON, device=DEV)                                      # an unrelated allocation, never handed over
    got = ops.step_targets(sd, sw, dpt, pix, 32, 2, 4)
    decoy.fill_(2 * POISON)
    assert all(torch.equal(bits(g_), bits(w)) for g_, w in zip(got, want))
    # the resident storage is what was read: a value written THERE shows in the next call, and no copy was made on the way
    h, w = int(kp[0, 0]), int(kp[0, 1])
    old = scene.depth_img[3, h, w].clone()
    scene.depth_img[3, h, w] = 77.0
    again = ops.step_targets(sd, sw, dpt, pix, 32, 2, 4)
    scene.depth_img[3, h, w] = old
    hit = (kp[:, 0] == h) & (kp[:, 1] == w)
    assert bool((again[0][0, hit] == 77.0).all()) and torch.equal(bits(again[0][0, ~hit]), bits(want[0][0, ~hit]))
    assert bool((decoy == 2 * POISON).all())
