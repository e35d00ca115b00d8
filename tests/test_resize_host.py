"""Host-side checks of the colour frames' resize (uc_nerf_amd/csrc/resize.hip).  No GPU: tests/resize_cases.py's restatement against Pillow itself,
byte for byte; the library's coefficient function against the restatement; every refusal of the launch entry point (the checks come before any
device call, so NULL-like pointers are never dereferenced); the ABI untouched; the new names exported; DeviceScene.from_native's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_cases as RC
import sample_cases as SC

PAIRS = [(1280, 320), (1024, 256), (1920, 320), (53, 16), (16, 12), (12, 31), (7, 7), (1, 5), (5, 1), (150, 9)]


@pytest.fixture(scope="module")
def lib():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib as L
    return L.lib()


@pytest.mark.parametrize("hin,win,wh,n", RC.CASES, ids=RC.CASE_IDS)
def test_restatement_equals_pillow_byte_for_byte(hin, win, wh, n):
    Image = pytest.importorskip("PIL.Image")
    for kind in RC.KINDS:
        a, out = RC.reference(kind, n, hin, win, wh)
        assert out.shape == (n, wh[1], wh[0], 3) and out.dtype == np.uint8
        for f in range(n):
            assert np.array_equal(np.asarray(Image.fromarray(a[f]).resize(wh, Image.BILINEAR)), out[f]), (kind, f)


def test_restatement_equals_pillow_at_the_workload_size_and_beyond_the_ratio_bound():
    Image = pytest.importorskip("PIL.Image")
    for hin, win, wh in ((1024, 1280, (320, 256)), RC.REFUSED):
        a = RC.data("extremes", 1, hin, win)
        assert np.array_equal(np.asarray(Image.fromarray(a[0]).resize(wh, Image.BILINEAR)), RC.resize(a, wh)[0])


def test_an_impulse_reads_out_the_footprint():
    """40 x 150 -> (70, 9): input pixel (y, x) reaches the output pixels whose taps hold it -- here on both sides of the edges between the 8 x 32
    output tiles -- with its two coefficients applied one after the other (rounded to a byte in between); everything else stays 0."""
    hin, win, wh = 40, 150, (70, 9)
    y, x = RC.tile_edge_pixel(hin, win, wh)
    a, out = RC.reference("impulse_tile_edge", 1, hin, win, wh)
    assert a[0, y, x, 0] == 255 and a.sum() == 255
    sx, cx, kx = RC.coeffs(win, wh[0])
    sy, cy, ky = RC.coeffs(hin, wh[1])
    cols = [i for i in range(wh[0]) if sx[i] <= x < sx[i] + cx[i] and kx[i, x - sx[i]] > 0]
    rows = [i for i in range(wh[1]) if sy[i] <= y < sy[i] + cy[i] and ky[i, y - sy[i]] > 0]
    assert min(cols) < RC.TILE_W <= max(cols) and min(rows) < RC.TILE_H <= max(rows)
    hit = np.zeros((wh[1], wh[0]), bool)
    for r in rows:
        for c in cols:
            h = (2 ** 21 + 255 * int(kx[c, x - sx[c]])) >> 22
            assert out[0, r, c, 0] == (2 ** 21 + h * int(ky[r, y - sy[r]])) >> 22
            hit[r, c] = True
    assert not out[0, ..., 1:].any() and not out[0, ..., 0][~hit].any() and out[0, ..., 0][hit].all()


@pytest.mark.parametrize("i,o", PAIRS)
def test_library_coefficients_equal_the_restatement(lib, i, o):
    ks = lib.ucnerf_resize_bilinear_ksize(i, o)
    assert ks == RC.ksize(i, o)
    start, count = np.full(o, -7, np.int32), np.full(o, -7, np.int32)
    k = np.full((o, ks), -7, np.int32)
    assert lib.ucnerf_resize_bilinear_coeffs(i, o, start.ctypes.data, count.ctypes.data, k.ctypes.data) == ks
    rs, rc, rk = RC.coeffs(i, o)
    assert np.array_equal(start, rs) and np.array_equal(count, rc) and np.array_equal(k, rk)
    assert (k.sum(1) > 0).all() and (count >= 1).all() and (start + count <= i).all()
    from uc_nerf_amd import ops
    s, c, kk = ops.resize_coeffs(i, o)
    assert s.dtype == c.dtype == kk.dtype == torch.int32 and not s.is_cuda
    assert np.array_equal(s.numpy(), rs) and np.array_equal(c.numpy(), rc) and np.array_equal(kk.numpy(), rk)


def test_coefficient_functions_refuse_bad_sizes(lib):
    buf = np.zeros(64, np.int32)
    for i, o in ((0, 4), (4, 0), (-1, 4), (4, -3), ((1 << 24) + 1, 4)):
        assert lib.ucnerf_resize_bilinear_ksize(i, o) == -1 and b"outside" in lib.ucnerf_last_error()
        assert lib.ucnerf_resize_bilinear_coeffs(i, o, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == -1
    assert lib.ucnerf_resize_bilinear_coeffs(8, 4, None, buf.ctypes.data, buf.ctypes.data) == -1 and b"null" in lib.ucnerf_last_error()
    from uc_nerf_amd import ops
    with pytest.raises(RuntimeError, match="outside"):
        ops.resize_coeffs(0, 3)


def test_every_refusal_of_the_launch_comes_before_any_device_call(lib):
    from uc_nerf_amd import _lib as L
    assert lib.ucnerf_resize_bilinear_u8(None, None) == -1 and b"null params" in lib.ucnerf_last_error()

    def good():
        p = L.ResizeParams()
        p.N, p.Hin, p.Win, p.H, p.W = 2, 37, 53, 12, 16
        p.ksize_x, p.ksize_y = RC.ksize(53, 16), RC.ksize(37, 12)
        p.src_frame_stride, p.dst_frame_stride = 3 * 37 * 53, 3 * 12 * 16
        for name, tp in p._fields_:
            if tp is L.vp:
                setattr(p, name, 64)                       # non-null dummies, never dereferenced: validation fails first
        return p

    def refused(p, word):
        rc = lib.ucnerf_resize_bilinear_u8(C.addressof(p), None)
        return rc == -1 and word in lib.ucnerf_last_error()

    p = good()
    p.N = -1
    assert refused(p, b"negative")
    p = good()
    p.N = 65536
    assert refused(p, b"above 65535")
    for field in ("Hin", "Win", "H", "W"):
        for bad in (0, -5):
            p = good()
            setattr(p, field, bad)
            assert refused(p, b"below 1"), field
        p = good()
        setattr(p, field, 32769)
        assert refused(p, b"above 32768"), field
    p = good()
    p.Hin, p.Win = 32768, 32768
    assert refused(p, b"2^31")
    for name in ("src", "dst", "start_x", "count_x", "k_x", "start_y", "count_y", "k_y"):
        p = good()
        setattr(p, name, 0)
        assert refused(p, b"null"), name
    p = good()
    p.src_frame_stride -= 1
    assert refused(p, b"src_frame_stride")
    for bad in (3 * 12 * 16 - 4, 3 * 12 * 16 + 2):
        p = good()
        p.dst_frame_stride = bad
        assert refused(p, b"multiple of 4")
    p = good()
    p.H, p.W, p.ksize_x, p.ksize_y, p.dst_frame_stride = 3, 5, RC.ksize(53, 5), RC.ksize(37, 3), 45      # the frame itself: odd
    assert refused(p, b"multiple of 4")
    for name in ("src", "dst"):
        p = good()
        setattr(p, name, 66)
        assert refused(p, b"aligned"), name
    for field in ("ksize_x", "ksize_y"):
        p = good()
        setattr(p, field, getattr(p, field) + 2)
        assert refused(p, b"ksize"), field
    # the ratio bound: in <= 16 out on each axis, so that a workgroup's tile fits in LDS
    hin, win, (w, h) = RC.REFUSED
    p = good()
    p.Hin, p.Win, p.H, p.W, p.ksize_x, p.ksize_y = hin, win, h, w, RC.ksize(win, w), RC.ksize(hin, h)
    p.src_frame_stride, p.dst_frame_stride = 3 * hin * win, 20
    assert refused(p, b"ratio 16")
    p = good()
    p.Hin, p.ksize_y = 16 * 12 + 1, RC.ksize(16 * 12 + 1, 12)
    p.src_frame_stride = 3 * p.Hin * p.Win
    assert refused(p, b"ratio 16")
    # N == 0 is legal, launches nothing and looks at no pointer
    p = L.ResizeParams()
    assert lib.ucnerf_resize_bilinear_u8(C.addressof(p), None) == 0


def test_abi_version_and_earlier_struct_sizes_are_unchanged(lib):
    from uc_nerf_amd import _lib as L
    assert lib.ucnerf_abi_version() == 6 == L.ABI_VERSION
    # sizes as they were before the resize was added (x86-64, 8-byte pointers)
    assert lib.ucnerf_sizeof(b"ucnerf_sample_assemble_params") == 400 == C.sizeof(L.SampleAssembleParams)
    for cname, cls in list(L.STRUCTS.items()) + list(L.ADDED_STRUCTS.items()):
        assert lib.ucnerf_sizeof(cname.encode()) == C.sizeof(cls), cname
    assert list(L.ADDED_STRUCTS)[-1] == "ucnerf_resize_params" and lib.ucnerf_sizeof(b"ucnerf_resize_params") == 112
    assert lib.ucnerf_sizeof(b"ucnerf_no_such_params") == -1


def test_ops_exports_the_new_names():
    from uc_nerf_amd import ops
    from uc_nerf_amd.ops import data
    assert ops.resize_coeffs is data.resize_coeffs and ops.resize_bilinear_u8 is data.resize_bilinear_u8
    assert ops.RESIZE_MAX_RATIO == 16
    for src, word in ((torch.zeros((1, 4, 4, 3), dtype=torch.uint8), "ROCm device"), (np.zeros((1, 4, 4, 3), np.uint8), "ROCm device")):
        with pytest.raises(RuntimeError, match=word):
            ops.resize_bilinear_u8(src, (2, 2))


def test_from_native_refusals_that_need_no_device():
    from uc_nerf_amd.data import DeviceScene
    sc = SC.scene("c5x7")
    args = (sc["poses"], sc["focal"], sc["bounds"], sc["sparse"], list(sc["frames"]), sc["dpt"], sc["depths_h"])
    with pytest.raises(ValueError, match="img_wh"):
        DeviceScene.from_native(*args)
    with pytest.raises(ValueError, match="img_wh"):
        DeviceScene.from_native(*args, img_wh=(0, 5))
    with pytest.raises(ValueError, match="batch"):
        DeviceScene.from_native(*args, img_wh=sc["img_wh"], batch=0)
    with pytest.raises(ValueError, match="no host route"):
        DeviceScene.from_native(*args, img_wh=sc["img_wh"], device="cpu")
    record = {"poses": sc["poses"], "focal": sc["focal"], "bounds": sc["bounds"]}
    with pytest.raises(ValueError, match="img_wh"):
        DeviceScene.from_native_records(record, sc["sparse"], list(sc["frames"]), sc["dpt"])
    # the constructors that take frames at img_wh are as they were
    with pytest.raises(ValueError, match="frames must be uint8"):
        DeviceScene.from_arrays(sc["poses"], sc["focal"], sc["bounds"], sc["sparse"], sc["frames"][:, :-1], sc["dpt"], img_wh=sc["img_wh"], device="cpu")
    ds = DeviceScene.from_arrays(sc["poses"], sc["focal"], sc["bounds"], sc["sparse"], sc["frames"], sc["dpt"], sc["depths_h"], sc["img_wh"], device="cpu")
    W, H = sc["img_wh"]
    assert ds.frames.shape == (len(sc["poses"]), (3 * H * W + 3) // 4 * 4) and np.array_equal(ds.frames[:, :3 * H * W].numpy().reshape(-1, H, W, 3), sc["frames"])
