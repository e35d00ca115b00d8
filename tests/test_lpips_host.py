"""Host-side checks of LPIPS (no GPU): the state-dict parsing of utils.evaluation.LPIPS and every refusal it documents, the entry points'
argument checks through ctypes (they come before anything is launched), the new structs in ucnerf_sizeof, and the sanity of the float64
restatement (tests/lpips_cases.py) the device tests are measured against."""
import ctypes as C
import os

import pytest
import torch

import lpips_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_STRUCTS = {"ucnerf_conv2d_pack_params": 4 * 4 + 2 * 8, "ucnerf_conv2d_params": 10 * 4 + 6 * 8, "ucnerf_maxpool2d_params": 8 + 2 * 4 + 2 * 8,
               "ucnerf_lpips_layer_params": 6 * 4 + 4 * 8, "ucnerf_lpips_alex_params": 4 * 4 + (2 + 15 + 4) * 8}
NEW_SYMBOLS = ("ucnerf_conv2d_packed_floats", "ucnerf_conv2d_pack", "ucnerf_conv2d_bias_relu", "ucnerf_maxpool2d", "ucnerf_lpips_layer",
               "ucnerf_lpips_workspace_floats", "ucnerf_lpips_alex")


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


def _parse(alex, lin):
    from uc_nerf_amd.utils.evaluation import LPIPS
    return LPIPS.parse(alex, lin)


# ------------------------------------------------------------------------------------------------ ABI
def test_new_structs_and_symbols_are_registered_and_the_abi_stays_at_6(L):
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    for name, size in NEW_STRUCTS.items():
        assert L.lib().ucnerf_sizeof(name.encode()) == size == C.sizeof(L.ADDED_STRUCTS[name]), name
        assert "struct %s {" % name in hdr and name not in L.STRUCTS
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in L.SYMBOLS and name + "(" in hdr, name
    assert "not part of this library" not in hdr


def test_packed_and_workspace_sizes(L):
    lib = L.lib()
    # [cout tiles of 64][k padded to 32][64] weights + one tap code per padded k
    assert lib.ucnerf_conv2d_packed_floats(3, 64, 11) == 1 * 384 * 64 + 384
    assert lib.ucnerf_conv2d_packed_floats(5, 33, 3) == 1 * 64 * 64 + 64
    assert lib.ucnerf_conv2d_packed_floats(64, 192, 5) == 3 * 1600 * 64 + 1600
    assert lib.ucnerf_conv2d_packed_floats(3, 64, 12) < 0 and lib.ucnerf_conv2d_packed_floats(0, 64, 3) < 0
    # 2 n images: level 0 7 x 7, pooled 3 x 3, the rest 1 x 1 at the minimum side
    assert lib.ucnerf_lpips_workspace_floats(1, 31, 31) == 2 * (64 * 49 + 64 * 9 + 192 * 9 + 192 + 384 + 256 + 256)
    assert lib.ucnerf_lpips_workspace_floats(0, 31, 31) == 0
    o1, p1, p2 = 63 * 79, 31 * 39, 15 * 19
    assert lib.ucnerf_lpips_workspace_floats(10, 256, 320) == 20 * (64 * o1 + 64 * p1 + 192 * p1 + 192 * p2 + (384 + 256 + 256) * p2)


def test_minimum_side_refusal_names_the_minimum(L):
    lib = L.lib()
    for H, W in ((30, 31), (31, 30), (1, 1), (0, 64)):
        assert lib.ucnerf_lpips_workspace_floats(1, H, W) == -1
        assert "31" in lib.ucnerf_last_error().decode()
        p = L.LpipsAlexParams()
        p.n, p.H, p.W = 1, H, W
        assert lib.ucnerf_lpips_alex(C.addressof(p), None) == -1
        msg = lib.ucnerf_last_error().decode()
        assert "minimum side 31" in msg and "%d x %d" % (H, W) in msg
    assert lib.ucnerf_lpips_workspace_floats(-1, 64, 64) == -1


def test_empty_batches_succeed_and_bad_arguments_are_einval_before_any_launch(L):
    lib = L.lib()
    a = L.LpipsAlexParams()
    a.n, a.H, a.W = 0, 31, 31                                           # n == 0: success with every pointer NULL
    assert lib.ucnerf_lpips_alex(C.addressof(a), None) == 0
    a.n = -1
    assert lib.ucnerf_lpips_alex(C.addressof(a), None) == -1 and "negative" in lib.ucnerf_last_error().decode()
    a.n = 1                                                             # NULL arrays
    assert lib.ucnerf_lpips_alex(C.addressof(a), None) == -1 and "null" in lib.ucnerf_last_error().decode()
    c = L.Conv2dParams()
    c.n, c.cin, c.H, c.W, c.cout, c.K, c.stride, c.pad = 0, 3, 8, 8, 4, 3, 1, 1
    assert lib.ucnerf_conv2d_bias_relu(C.addressof(c), None) == 0
    c.n = 1
    assert lib.ucnerf_conv2d_bias_relu(C.addressof(c), None) == -1 and "null" in lib.ucnerf_last_error().decode()
    for field, bad in (("n", -1), ("K", 12), ("K", 0), ("stride", 0), ("pad", -1), ("cin", 0), ("cout", 0), ("H", 0)):
        c2 = L.Conv2dParams()
        c2.n, c2.cin, c2.H, c2.W, c2.cout, c2.K, c2.stride, c2.pad = 1, 3, 8, 8, 4, 3, 1, 1
        setattr(c2, field, bad)
        assert lib.ucnerf_conv2d_bias_relu(C.addressof(c2), None) == -1, field
    c.H, c.W, c.K, c.pad = 2, 2, 5, 1                                   # the padded input is smaller than the kernel
    assert lib.ucnerf_conv2d_bias_relu(C.addressof(c), None) == -1 and "smaller" in lib.ucnerf_last_error().decode()
    m = L.Maxpool2dParams()
    m.planes, m.H, m.W = 0, 3, 3
    assert lib.ucnerf_maxpool2d(C.addressof(m), None) == 0
    m.planes = 1
    assert lib.ucnerf_maxpool2d(C.addressof(m), None) == -1
    m.planes, m.H = 0, 2
    assert lib.ucnerf_maxpool2d(C.addressof(m), None) == -1 and "3 x 3" in lib.ucnerf_last_error().decode()
    m.planes, m.H = -1, 3
    assert lib.ucnerf_maxpool2d(C.addressof(m), None) == -1
    y = L.LpipsLayerParams()
    y.n, y.C, y.h, y.w = 0, 64, 1, 1
    assert lib.ucnerf_lpips_layer(C.addressof(y), None) == 0
    y.n = 2
    assert lib.ucnerf_lpips_layer(C.addressof(y), None) == -1
    y.n, y.C = 0, 0
    assert lib.ucnerf_lpips_layer(C.addressof(y), None) == -1
    k = L.Conv2dPackParams()
    k.cin, k.cout, k.K = 3, 64, 11
    assert lib.ucnerf_conv2d_pack(C.addressof(k), None) == -1 and "null" in lib.ucnerf_last_error().decode()
    for fn in ("ucnerf_conv2d_pack", "ucnerf_conv2d_bias_relu", "ucnerf_maxpool2d", "ucnerf_lpips_layer", "ucnerf_lpips_alex"):
        assert getattr(lib, fn)(None, None) == -1, fn


# ------------------------------------------------------------------------------------------------ state dicts
def test_both_key_spellings_and_both_lin_forms_parse_to_the_same_tensors():
    alex, lin = LC.weights()
    w, b, v = _parse(alex, lin)
    assert [tuple(t.shape) for t in w] == [(co, ci, K, K) for _, ci, co, K, _, _ in LC.CONVS]
    assert [t.numel() for t in b] == [64, 192, 384, 256, 256] == [t.numel() for t in v]
    bare = {k[len("features."):]: t for k, t in alex.items() if k.startswith("features.")}
    listed = [lin["lin%d.model.1.weight" % l].reshape(-1) for l in range(5)]
    w2, b2, v2 = _parse(bare, listed)
    for x, y in zip(w + b + v, w2 + b2 + v2):
        assert x.dtype == torch.float32 and x.is_contiguous() and torch.equal(x, y)
    for l, (idx, *_rest) in enumerate(LC.CONVS):
        assert torch.equal(w[l], alex["features.%d.weight" % idx]) and torch.equal(v[l], lin["lin%d.model.1.weight" % l].reshape(-1))


def test_every_refusal_names_the_offender():
    alex, lin = LC.weights()
    alex, lin = dict(alex), dict(lin)
    missing = {k: t for k, t in alex.items() if k != "features.6.bias"}
    with pytest.raises(ValueError, match=r"features\.6\.bias"):
        _parse(missing, lin)
    wrong = dict(alex)
    wrong["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight.*\(192, 64, 3, 3\).*\(192, 64, 5, 5\)"):
        _parse(wrong, lin)
    wrong = dict(alex)
    wrong["features.0.bias"] = torch.zeros(63)
    with pytest.raises(ValueError, match=r"features\.0\.bias"):
        _parse(wrong, lin)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        _parse(alex, {k: t for k, t in lin.items() if k != "lin2.model.1.weight"})
    bad = dict(lin)
    bad["lin4.model.1.weight"] = torch.zeros(1, 255, 1, 1)
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight.*255"):
        _parse(alex, bad)
    neg = dict(lin)
    neg["lin1.model.1.weight"] = lin["lin1.model.1.weight"].clone()
    neg["lin1.model.1.weight"][0, 5, 0, 0] = -0.25
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight.*negative"):
        _parse(alex, neg)
    with pytest.raises(ValueError, match="five"):
        _parse(alex, [torch.zeros(64)] * 4)
    listed = [lin["lin%d.model.1.weight" % l].reshape(-1) for l in range(5)]
    listed[3] = -listed[3] - 1
    with pytest.raises(ValueError, match=r"lin_state\[3\].*negative"):
        _parse(alex, listed)
    with pytest.raises(ValueError, match="state dict"):
        _parse(None, lin)
    with pytest.raises(ValueError, match="lin_state"):
        _parse(alex, None)


def test_from_files_loads_plain_checkpoints_and_a_cpu_device_raises(tmp_path):
    from uc_nerf_amd.utils.evaluation import LPIPS
    alex, lin = LC.weights()
    pa, pl = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex_lin.pth")
    torch.save(dict(alex), pa)
    torch.save(dict(lin), pl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # the files parse; what refuses is the device
        LPIPS.from_files(pa, pl, device="cpu")
    with pytest.raises(ValueError, match=r"features\.0\.weight"):        # the two files the wrong way round
        LPIPS.parse(torch.load(pl, weights_only=True), torch.load(pa, weights_only=True))


def test_cpu_tensors_raise_in_every_op():
    from uc_nerf_amd import ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv2d_pack(torch.zeros(4, 3, 3, 3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv2d_bias_relu(x, torch.zeros(4, 3, 3, 3), torch.zeros(4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.maxpool2d(x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.lpips_layer(x, x, torch.zeros(3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.lpips_alex(torch.zeros(1, 3, 31, 31), torch.zeros(1, 3, 31, 31), [None] * 5, [None] * 5, [None] * 5, torch.zeros(3), torch.zeros(3))


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_identity_sign_and_float32_agreement():
    alex, lin = LC.weights()
    for H, W in LC.CHAIN_SHAPES:
        a, b = LC.images(H, W)
        d64, d32 = LC.chain_reference(H, W)
        assert d64.dtype == torch.float64 and d32.dtype == torch.float32 and d64.shape == (LC.CHAIN_N,)
        assert float(d64[1]) == 0.0 and float(d32[1]) == 0.0             # the identical pair
        assert bool((d64 >= 0).all()) and float(d64[0]) > 1e-3 and float(d64[2]) > 1e-3      # lin >= 0; the perturbed pairs are apart
        assert torch.equal(LC.lpips(a, a, alex, lin, torch.float64), torch.zeros(LC.CHAIN_N, dtype=torch.float64))
        rel = ((d32.double() - d64).abs() / d64.clamp_min(1e-30))[[0, 2]]
        assert float(rel.max()) < 1e-4, (H, W, rel)                      # float32 against float64: rounding, not a different formula
        assert torch.allclose(LC.lpips(b, a, alex, lin, torch.float64), d64, rtol=1e-12, atol=0)


def test_restatement_geometry_and_zero_pixels():
    alex, _ = LC.weights()
    f = LC.features(LC.images(31, 31)[0], alex, torch.float64)
    assert [tuple(t.shape[1:]) for t in f] == [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    f = LC.features(LC.images(35, 47)[0], alex, torch.float64)
    assert [tuple(t.shape[1:]) for t in f] == [(64, 8, 11), (192, 3, 5), (384, 1, 2), (256, 1, 2), (256, 1, 2)]
    z = torch.zeros(1, 8, 2, 2, dtype=torch.float64)
    x = torch.ones(1, 8, 2, 2, dtype=torch.float64)
    lin = torch.full((8,), 0.5, dtype=torch.float64)
    assert float(LC.layer_distance(z, z, lin)) == 0.0                    # all-zero pixels: 0, never NaN
    assert abs(float(LC.layer_distance(z, x, lin)) - 0.5) < 1e-9         # |n1|^2 = 1 per pixel, times lin
