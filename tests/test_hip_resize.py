"""ucnerf_resize_bilinear_u8 on the device against tests/resize_cases.py's restatement of Pillow's BILINEAR resize (and against Pillow itself where
PIL imports): bit for bit, every case.  Then the padded destination, a dirty destination, another stream, the wrapper's refusals, the ratio bound,
and DeviceScene.from_native against from_arrays fed the restatement's frames."""
import numpy as np
import pytest
import torch

import resize_cases as RC
import sample_cases as SC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("hin,win,wh,n", RC.CASES, ids=RC.CASE_IDS)
def test_resize_equals_the_restatement_bit_for_bit(hin, win, wh, n):
    from uc_nerf_amd import ops
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for kind in RC.KINDS:
        a, ref = RC.reference(kind, n, hin, win, wh)
        got = ops.resize_bilinear_u8(dev(a), wh)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (n, wh[1], wh[0], 3) and got.is_contiguous()
        got = got.cpu()
        assert torch.equal(got, torch.from_numpy(ref.copy())), kind
        if Image is not None:
            for f in range(n):
                assert np.array_equal(got[f].numpy(), np.asarray(Image.fromarray(a[f]).resize(wh, Image.BILINEAR))), (kind, f)


@pytest.mark.parametrize("hin,win,wh", [(37, 53, (16, 12)), (5, 7, (5, 3)), (2, 3, (7, 5)), (40, 150, (70, 9))], ids=lambda v: str(v).replace(" ", ""))
def test_padded_destination_keeps_its_pad_bytes_and_a_dirty_one_gives_the_same_bits(hin, win, wh):
    from uc_nerf_amd import ops
    n = 3
    a, ref = RC.reference("random", n, hin, win, wh)
    frame = 3 * wh[0] * wh[1]
    guard = 64
    for stride in ((frame + 3) // 4 * 4, (frame + 3) // 4 * 4 + 8):
        flat = torch.full((n * stride + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        out = flat[:n * stride].view(n, stride)
        src = dev(a)
        ret = ops.resize_bilinear_u8(src, wh, out=out)
        assert ret is out
        host = flat.cpu()
        rows = host[:n * stride].view(n, stride)
        assert torch.equal(rows[:, :frame].reshape(n, wh[1], wh[0], 3), torch.from_numpy(ref.copy()))
        assert (rows[:, frame:] == 0xA5).all() and (host[n * stride:] == 0xA5).all()           # the pad of every frame; the guard band
        # a second call into the buffer as the first one left it, and one into another pattern: the same bits, the pad still untouched
        ops.resize_bilinear_u8(src, wh, out=out)
        assert torch.equal(flat.cpu(), host)
        flat[:n * stride] = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        before = flat.cpu()
        ops.resize_bilinear_u8(src, wh, out=flat, out_frame_stride=stride)                        # (a flat buffer with the stride given)
        after = flat.cpu()
        assert torch.equal(after[:n * stride].view(n, stride)[:, :frame], rows[:, :frame])
        assert torch.equal(after[:n * stride].view(n, stride)[:, frame:], before[:n * stride].view(n, stride)[:, frame:]) and (after[n * stride:] == 0xA5).all()


def test_on_a_stream_that_is_not_the_default_one():
    from uc_nerf_amd import ops
    hin, win, wh, n = 64, 80, (20, 16), 3
    a, ref = RC.reference("extremes", n, hin, win, wh)
    src = dev(a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = ops.resize_bilinear_u8(src, wh)
    s.synchronize()
    assert torch.equal(got.cpu(), torch.from_numpy(ref.copy()))


def test_empty_batch():
    from uc_nerf_amd import ops
    got = ops.resize_bilinear_u8(torch.empty((0, 9, 9, 3), dtype=torch.uint8, device="cuda"), (4, 3))
    assert got.shape == (0, 3, 4, 3) and got.dtype == torch.uint8


def test_wrapper_refusals():
    from uc_nerf_amd import ops
    good = torch.zeros((2, 8, 12, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.resize_bilinear_u8(good.cpu(), (4, 4))
    with pytest.raises(RuntimeError, match="uint8"):
        ops.resize_bilinear_u8(good.float(), (4, 4))
    with pytest.raises(RuntimeError, match=r"\[N,Hin,Win,3\]"):
        ops.resize_bilinear_u8(torch.zeros((2, 8, 12, 4), dtype=torch.uint8, device="cuda"), (4, 4))
    with pytest.raises(RuntimeError, match=r"\[N,Hin,Win,3\]"):
        ops.resize_bilinear_u8(good[0], (4, 4))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.resize_bilinear_u8(torch.zeros((2, 12, 8, 3), dtype=torch.uint8, device="cuda").transpose(1, 2), (4, 4))
    with pytest.raises(RuntimeError, match="below 1"):
        ops.resize_bilinear_u8(good, (0, 4))
    frame = 3 * 4 * 4
    with pytest.raises(RuntimeError, match="out must be"):
        ops.resize_bilinear_u8(good, (4, 4), out=torch.zeros((2, frame), dtype=torch.uint8))                       # on the host
    with pytest.raises(RuntimeError, match="out must be"):
        ops.resize_bilinear_u8(good, (4, 4), out=torch.zeros((3, frame), dtype=torch.uint8, device="cuda"))        # three rows for two frames
    with pytest.raises(RuntimeError, match="out holds"):
        ops.resize_bilinear_u8(good, (4, 4), out=torch.zeros(2 * frame - 1, dtype=torch.uint8, device="cuda"), out_frame_stride=frame)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.resize_bilinear_u8(good, (5, 3), out=torch.zeros((2, 45), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.resize_bilinear_u8(good, (4, 4), out=torch.zeros((2, frame), dtype=torch.uint8, device="cuda"), out_frame_stride=frame - 4)


def test_ratio_bound_refusal():
    from uc_nerf_amd import ops
    hin, win, wh = RC.REFUSED
    with pytest.raises(RuntimeError, match="ratio 16"):
        ops.resize_bilinear_u8(torch.zeros((1, hin, win, 3), dtype=torch.uint8, device="cuda"), wh)
    a = RC.data("random", 1, 33, 64)                           # 64 -> 4 is the bound itself; 33 -> 2 is beyond it
    assert torch.equal(ops.resize_bilinear_u8(dev(a), (4, 3)).cpu(), torch.from_numpy(RC.resize(a, (4, 3))))
    with pytest.raises(RuntimeError, match="ratio 16"):
        ops.resize_bilinear_u8(dev(a), (4, 2))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def test_from_native_equals_from_arrays_fed_the_restatement():
    """Five native frames of two sizes (so: groups of 2, 1 and 2 at batch=2), img_wh = (14, 10): the resident frame storage equals, byte for
    byte, that of from_arrays fed the restatement's output -- the pad bytes included -- and a sample of each is equal on every key."""
    from uc_nerf_amd.data import DeviceScene
    W, H = 14, 10
    sc = SC.make_scene(H, W, (40, 3, 0, 25, 7), seed=21)
    poses, bounds, sparse, dpt, depths_h = sc["poses"], sc["bounds"], sc["sparse"], sc["dpt"], sc["depths_h"]
    sizes = [(37, 53), (37, 53), (37, 53), (48, 64), (48, 64)]
    native = [RC.data("random", 1, h, w, seed=i)[0] for i, (h, w) in enumerate(sizes)]
    resized = np.concatenate([RC.resize(f[None], (W, H)) for f in native])
    a = DeviceScene.from_native(poses, sc["focal"], bounds, sparse, iter(native), dpt, depths_h, img_wh=(W, H), batch=2, device="cuda", scan=3)
    b = DeviceScene.from_arrays(poses, sc["focal"], bounds, sparse, resized, dpt, depths_h, (W, H), device="cuda", scan=3)
    assert a.frames.shape == b.frames.shape == (5, (3 * H * W + 3) // 4 * 4) and a.frames.dtype == torch.uint8
    assert torch.equal(a.frames, b.frames)
    perm = torch.randperm(a.n_keypoints(3), device="cuda", generator=torch.Generator("cuda").manual_seed(2)).to(torch.int32)
    sa, sb = a.sample(3, [0, 4, 2], perm=perm, unpreprocess=True), b.sample(3, [0, 4, 2], perm=perm, unpreprocess=True)
    assert set(sa) == set(sb)
    for key in sa:
        if isinstance(sa[key], dict):
            assert all(same_bits(sa[key][lvl], sb[key][lvl]) for lvl in sb[key]), key
        else:
            assert same_bits(sa[key], sb[key]), key
    # the records twin, and the refusals that show only once the frames are read
    record = {"poses": poses, "focal": sc["focal"], "bounds": bounds}
    c = DeviceScene.from_native_records(record, sparse, native, dpt, depths_h, img_wh=(W, H), batch=32, device="cuda")
    assert torch.equal(c.frames, b.frames)
    with pytest.raises(ValueError, match="4 frames, 5 poses"):
        DeviceScene.from_native(poses, sc["focal"], bounds, sparse, native[:4], dpt, depths_h, img_wh=(W, H))
    with pytest.raises(ValueError, match="more than the 5 frames"):
        DeviceScene.from_native(poses, sc["focal"], bounds, sparse, native + native[:1], dpt, depths_h, img_wh=(W, H))
    with pytest.raises(ValueError, match="frame 1 must be uint8"):
        DeviceScene.from_native(poses, sc["focal"], bounds, sparse, [native[0], native[1][..., :2]] + native[2:], dpt, depths_h, img_wh=(W, H))
