"""Host-side checks of multi-view depth fusion: the PLY writer / reader, `fusion.source_table`, the ctypes surface of the two entry points, and
the float64 restatement of tests/fusion_cases.py on its own -- against the lattice's integer index arithmetic, and the cap on undecided pixels
of every differential case (so that cap is proven before any GPU run).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fusion_cases as FC
from uc_nerf_amd.data import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ PLY
@pytest.mark.parametrize("n", [0, 1, 7, 1000])
def test_ply_round_trip_is_byte_exact(tmp_path, n):
    rs = np.random.RandomState(n)
    pts = rs.randn(n, 3).astype(np.float32)
    if n >= 7:
        pts[:5, 0] = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-42], np.float32)
    cols = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    path = str(tmp_path / "cloud.ply")
    formats.write_ply(path, pts, cols)
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\n")
    head, body = raw.split(b"end_header\n", 1)
    assert b"element vertex %d\n" % n in head and len(body) == 15 * n
    assert head.decode().split("\n")[3:9] == ["property float x", "property float y", "property float z", "property uchar red",
                                              "property uchar green", "property uchar blue"]
    got_p, got_c = formats.read_ply(path)
    assert got_p.dtype == np.float32 and got_c.dtype == np.uint8 and got_p.shape == (n, 3) and got_c.shape == (n, 3)
    assert got_p.tobytes() == pts.tobytes() and got_c.tobytes() == cols.tobytes()
    again = str(tmp_path / "again.ply")
    formats.write_ply(again, got_p, got_c)
    assert open(again, "rb").read() == raw
    # the body is x y z r g b per vertex, little-endian, no padding
    if n:
        assert body[:12] == pts[0].astype("<f4").tobytes() and body[12:15] == cols[0].tobytes()


def test_ply_refuses_what_it_does_not_write(tmp_path):
    with pytest.raises(ValueError):
        formats.write_ply(str(tmp_path / "a.ply"), np.zeros((3, 3), np.float32), np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError):
        formats.write_ply(str(tmp_path / "a.ply"), np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32))
    bad = tmp_path / "ascii.ply"
    bad.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        formats.read_ply(str(bad))
    short = tmp_path / "short.ply"
    formats.write_ply(str(short), np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8))
    short.write_bytes(short.read_bytes()[:-1])
    with pytest.raises(ValueError):
        formats.read_ply(str(short))


# ------------------------------------------------------------------------------------------------ source_table
@pytest.mark.parametrize("N,n_src", [(1, 3), (2, 4), (5, 4), (9, 3), (6, 5)])
def test_source_table_is_get_nearest_pose_ids_per_row(N, n_src):
    from uc_nerf_amd.fusion import source_table
    rs = np.random.RandomState(N * 10 + n_src)
    c2w = np.tile(np.eye(4), (N, 1, 1))
    c2w[:, :3, 3] = rs.uniform(-1, 1, (N, 3))
    for poses in (c2w, c2w[:, :3]):
        t = source_table(poses, n_src)
        assert t.dtype == np.int32 and t.shape == (N, n_src)
        for r in range(N):
            k = min(n_src, N - 1)
            want = formats.get_nearest_pose_ids(poses[r], poses, n_src, tar_id=r).tolist() if N > 1 else []
            assert t[r, :k].tolist() == want and (t[r, k:] == -1).all()
            assert r not in t[r].tolist() and len(set(t[r, :k].tolist())) == k
            d = np.linalg.norm(c2w[t[r, :k], :3, 3] - c2w[r, :3, 3], axis=1)
            assert (np.diff(d) >= 0).all()                                         # nearest first
    import torch
    assert np.array_equal(source_table(torch.from_numpy(c2w), n_src), t)


def test_scene_train_views_and_source_table_cache():
    """`DeviceScene.train_index` / `nearest_train_views` / `fusion_sources` on a host-resident scene (constants only: no launch)."""
    import system_cases as YC
    from uc_nerf_amd.fusion import source_table
    scene = YC.tiny_scene("cpu")
    for rate in (2, 3):
        train = scene.train_index(rate).tolist()
        assert train == list(range(scene.N))[rate // 2::rate]
        val = dict(scene.metas("val", YC.V, sample_rate=rate))
        for f in range(scene.N):
            near = scene.nearest_train_views(f, YC.V, sample_rate=rate)
            assert f not in near and set(near) <= set(train) and len(near) == min(YC.V - 1, len(train) - 1)
            if f in val:
                assert near == val[f]
    a = scene.fusion_sources([0, 1, 2, 4], 3)
    assert a.dtype.is_floating_point is False and a.shape == (4, 3) and np.array_equal(a.numpy(), source_table(scene.poses[[0, 1, 2, 4]], 3))
    assert scene.fusion_sources((0, 1, 2, 4), 3) is a                                # the last table is kept ...
    b = scene.fusion_sources([0, 1, 2], 3)
    assert b is not a and b.shape == (3, 3) and scene.fusion_sources([0, 1, 2, 4], 3) is not a      # ... and only the last


# ------------------------------------------------------------------------------------------------ the surface
def test_bindings_and_struct_sizes_match_the_header():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd import ops
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    for sym in ("ucnerf_depth_consistency", "ucnerf_points_compact", "ucnerf_points_compact_workspace_bytes"):
        assert sym in L.SYMBOLS and re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(C.CDLL(L.LIB_PATH), sym)
    for cname, cls in (("ucnerf_depth_consistency_params", L.DepthConsistencyParams), ("ucnerf_points_compact_params", L.PointsCompactParams)):
        assert L.ADDED_STRUCTS[cname] is cls and lib.ucnerf_sizeof(cname.encode()) == C.sizeof(cls), cname
        body = re.search(r"struct %s \{(.*?)\};" % cname, hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
        names = [re.split(r"[\s\*]+", n)[-1] for n in names]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert C.sizeof(L.DepthConsistencyParams) == 32 + 9 * 8 and C.sizeof(L.PointsCompactParams) == 24 + 9 * 8
    # the compaction's constants as the tests' case table assumes them
    assert (ops.COMPACT_BLOCK_ITEMS, ops.COMPACT_SCAN_CHUNK) == (FC.ITEMS, FC.CHUNK)
    ws = lib.ucnerf_points_compact_workspace_bytes
    assert [ws(n) for n in (0, 1, FC.ITEMS, FC.ITEMS + 1)] == [0, 4, 4, 8] and ws(-1) == -1 and b"negative" in lib.ucnerf_last_error()
    assert ops.depth_consistency.__module__ == ops.points_compact.__module__ == "uc_nerf_amd.ops.fusion"


def test_entry_points_check_their_arguments_before_any_launch():
    from uc_nerf_amd import _lib as L
    lib = L.lib()
    assert lib.ucnerf_depth_consistency(None, None) == -1 and b"null params" in lib.ucnerf_last_error()
    assert lib.ucnerf_points_compact(None, None) == -1 and b"null params" in lib.ucnerf_last_error()
    empty = L.DepthConsistencyParams()                                                                      # (kept alive for the length of the call)
    assert lib.ucnerf_depth_consistency(C.addressof(empty), None) == 0                                      # N = 0: an empty batch
    for field in ("N", "H", "W", "S"):
        p = L.DepthConsistencyParams()
        p.N, p.H, p.W, p.S = 2, 3, 4, 1
        p.depth = p.intrinsics = p.c2ws = p.src_ids = p.count = p.mask = p.fused = 64
        setattr(p, field, -1)
        assert lib.ucnerf_depth_consistency(C.addressof(p), None) == -1 and b"negative" in lib.ucnerf_last_error(), field
    p = L.DepthConsistencyParams()
    p.N, p.H, p.W, p.S = 2, 3, 4, 33
    assert lib.ucnerf_depth_consistency(C.addressof(p), None) == -1 and b"S = 33 sources above 32" in lib.ucnerf_last_error()
    p.S = 1
    assert lib.ucnerf_depth_consistency(C.addressof(p), None) == -1 and b"null input" in lib.ucnerf_last_error()
    p.N, p.H, p.W = 1 << 10, 1 << 11, 1 << 10
    assert lib.ucnerf_depth_consistency(C.addressof(p), None) == -1 and b"below 2^31" in lib.ucnerf_last_error()
    for field in ("N", "H", "W", "cap"):
        q = L.PointsCompactParams()
        q.N, q.H, q.W, q.cap = 2, 3, 4, 5
        q.fused = q.mask = q.rgb = q.intrinsics = q.c2ws = q.workspace = q.points = q.colors = q.total = 64
        setattr(q, field, -1)
        assert lib.ucnerf_points_compact(C.addressof(q), None) == -1 and b"negative" in lib.ucnerf_last_error(), field
    q = L.PointsCompactParams()
    q.N, q.H, q.W, q.cap = 2, 3, 4, 5
    assert lib.ucnerf_points_compact(C.addressof(q), None) == -1 and b"total" in lib.ucnerf_last_error()
    q.total = 64
    assert lib.ucnerf_points_compact(C.addressof(q), None) == -1 and b"null input" in lib.ucnerf_last_error()


def test_cpu_tensors_and_wrong_shapes_are_refused():
    import torch
    from uc_nerf_amd import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.depth_consistency(torch.zeros(2, 3, 4), torch.zeros(2, 3, 3), torch.zeros(2, 4, 4), torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.points_compact(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.bool), torch.zeros(2, 3, 3, 4), torch.zeros(2, 3, 3), torch.zeros(2, 4, 4))
    from uc_nerf_amd.fusion import PointCloud, fuse_views
    from uc_nerf_amd.system import UCNeRFSystem
    assert callable(fuse_views) and callable(UCNeRFSystem.reconstruct) and callable(PointCloud.trim) and callable(PointCloud.save_ply)
    with pytest.raises(TypeError, match="unknown arguments"):
        fuse_views(None, None, None, None, src_ids=[], threshold=3)


# ------------------------------------------------------------------------------------------------ the restatement on its own
@pytest.mark.parametrize("N,S", FC.LATTICE_VIEWS)
@pytest.mark.parametrize("H,W", FC.LATTICE_SHAPES)
def test_restatement_gives_the_lattice_expectations(H, W, N, S):
    case = FC.lattice_case(H, W, N, S)
    for w2cs in (None, FC.rigid_inverse(case["c2ws"]).astype(np.float32)):
        ref = FC.consistency_ref(case["depth"], case["intrinsics"], case["c2ws"], case["src_ids"], w2cs=w2cs, min_views=1)
        assert np.array_equal(ref["count"], case["count"])
        assert np.array_equal(ref["fused"], np.full((N, H, W), FC.Z0)) and np.array_equal(ref["mask"], case["count"] >= 1)
    assert np.array_equal(FC.points_ref(ref["fused"], case["intrinsics"], case["c2ws"]), case["points"].astype(np.float64))
    if N == 1:
        assert not case["count"].any()
    if N == 5 and S == 4 and (H, W) == (33, 65):
        assert case["count"].max() == 3 and case["count"].min() < 3                  # slots: three other views and the empty one


def test_color_rule():
    v = np.array([np.nan, -1, 0, 0.5, 1, 2, 127.5 / 255, 0.00196], np.float32)
    assert FC.color_rule(v).tolist() == [0, 0, 0, 128, 255, 255, 128, 0]


@pytest.mark.parametrize("i", range(len(FC.DIFF_CASES)), ids=FC.DIFF_IDS)
def test_undecided_pixels_stay_within_the_cap(i):
    case, ref = FC.diff_ref(i)
    frac = ref["undecided"].mean()
    print("undecided %.4f, masked %.3f, counts %s" % (frac, ref["mask"].mean(), np.bincount(ref["count"].reshape(-1), minlength=5).tolist()))
    assert frac <= 0.02
    # the case is worth comparing: masked and unmasked pixels, every count from 0 to S
    assert 0.2 < ref["mask"].mean() < 0.95 and len(np.unique(ref["count"])) == 5
