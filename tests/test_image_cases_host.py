"""Host-side checks of the whole-image path (ucnerf_image_put, ucnerf_depth_minmax, ucnerf_depth_colormap, uc_nerf_amd.utils.utils.visualize_depth,
uc_nerf_amd.utils.colormaps).  No GPU: the case builders of tests/image_cases.py hold what they promise, the package's numpy path of
visualize_depth equals the restatement bit for bit on every case, the documented saturation values are what both give, the library exports the
new entry points with nothing of ABI v6 moved, and the entry points validate their arguments before anything is launched."""
import ctypes as C
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ("ucnerf_image_put", "ucnerf_depth_minmax", "ucnerf_depth_colormap", "ucnerf_minmax_reset", "ucnerf_minmax_read", "ucnerf_image_group_pixels")
NEW_STRUCTS = {"ucnerf_image_put_params": 3 * 4 + 4 + 5 * 8, "ucnerf_depth_minmax_params": 4 + 4 + 2 * 8, "ucnerf_depth_colormap_params": 4 + 4 + 2 * 8 + 5 * 8}


def test_jet_lut_is_a_table():
    from uc_nerf_amd.utils import colormaps
    t = colormaps.jet_lut()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert not np.array_equal(t[0], t[255])
    # OpenCV's column order: the low end of Jet is blue (column 0), the high end red (column 2); green peaks in the middle
    assert t[0, 0] > 0 and t[0, 1] == 0 and t[0, 2] == 0 and t[255, 2] > 0 and t[255, 0] == 0 and t[128, 1] == 255
    t[0, 0] = 1                                              # a copy: the cached table is not the caller's to change
    assert colormaps.jet_lut()[0, 0] != 1
    assert "CANNOT BE VERIFIED AGAINST OPENCV" in colormaps.jet_lut.__doc__ and "applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET)" in colormaps.jet_lut.__doc__
    with pytest.raises(ValueError):
        colormaps.as_table(np.zeros((256, 4), np.uint8))
    with pytest.raises(ValueError):
        colormaps.as_table(np.zeros((256, 3), np.float32))


def test_builders_hold_what_they_promise():
    assert IC.depth_case("random")["depth"].size >= 4096
    lat = IC.depth_case("lattice")
    idx = IC.index_reference(lat["depth"]).reshape(-1)
    j = np.arange(256)
    # the exact lattice: with both operations correctly rounded 255 * fl(j / 255) rounds back to j for EVERY j (measured here, not assumed) -- and a
    # quotient a single unit in the last place low, what a division that is not correctly rounded may return, truncates to j - 1 almost everywhere
    assert (idx == j).all()
    low = np.nextafter(lat["depth"].reshape(-1) / F32(255.0), F32(0.0))
    assert (np.trunc(F32(255.0) * low)[1:] == j[1:] - 1).sum() >= 250, "the lattice separates nothing"
    assert (IC.index_reference(IC.depth_case("constant")["depth"]) == 0).all()
    g = IC.depth_case("given_range")
    assert g["depth"].min() < g["minmax"][0] and g["depth"].max() > g["minmax"][1]
    rgb, depth = IC.put_case()
    assert np.isnan(rgb).any() and (IC.bits(rgb) == 0x80000000).any() and np.isnan(depth).any()
    # the reference's clamp on the host: NaN stays NaN, -0.0 stays -0.0, the neighbours of 0 and 1 go to 0 and 1
    img, dep = IC.assemble_reference(rgb, depth, 5, 7)
    src = rgb.reshape(5, 7, 3).transpose(2, 0, 1)
    assert np.isnan(img[np.isnan(src)]).all() and (IC.bits(img)[IC.bits(src) == 0x80000000] == 0x80000000).all()
    assert np.nanmax(img) == 1.0 and np.nanmin(img) == 0.0 and IC.same_bits(dep.reshape(-1), depth)
    for count in IC.MINMAX_COUNTS:
        for kind in IC.MINMAX_KINDS:
            x = IC.minmax_data(count, kind)
            mi, ma = IC.minmax_reference(x)
            assert x.shape == (count,) and mi <= ma and mi == np.min(np.nan_to_num(x)) and ma == np.max(np.nan_to_num(x))
    assert IC.minmax_reference(IC.minmax_data(2085, "wild")) == (-IC.FLT_MAX, IC.FLT_MAX)
    assert IC.minmax_reference(IC.minmax_data(2085, "negative"))[1] < 0


@pytest.mark.parametrize("name", IC.DEPTH_NAMES)
def test_numpy_path_equals_the_restatement_bit_for_bit(name):
    from uc_nerf_amd.utils import colormaps
    from uc_nerf_amd.utils.utils import visualize_depth
    case = IC.depth_case(name)
    idx = IC.index_reference(case["depth"], case["minmax"])
    for table in (IC.random_table(), colormaps.jet_lut()):
        want = IC.color_reference(idx, table)
        for depth in (case["depth"], torch.from_numpy(case["depth"].copy())):            # a numpy array and a CPU tensor
            got = visualize_depth(depth, case["minmax"], table)
            assert torch.is_tensor(got) and got.dtype == torch.float32 and tuple(got.shape) == (3,) + case["depth"].shape and not got.is_cuda
            assert IC.same_bits(got.numpy(), want), name
    assert list(inspect.signature(visualize_depth).parameters) == ["depth", "minmax", "cmap"]


def test_saturation_values_are_the_documented_ones():
    """The one place the mirror is stricter than numpy: NaN -> 0, below 0 -> 0, above 255 -> 255 -- asserted as documented, on both restatement and numpy path."""
    from uc_nerf_amd.utils.utils import _depth_index_numpy
    g = IC.depth_case("given_range")
    x = g["depth"]
    for idx in (IC.index_reference(x, g["minmax"]), _depth_index_numpy(np.nan_to_num(x), g["minmax"])[0]):
        assert (idx[x < 2.0] == 0).all() and (idx[x > 5.0] == 255).all() and (x < 2.0).any() and (x > 5.0).any()
        mid = (x > 2.1) & (x < 4.9)
        assert (idx[mid] > 0).all() and (idx[mid] < 255).all()
    n = IC.depth_case("nonfinite_given")
    x = n["depth"]
    for idx in (IC.index_reference(x, n["minmax"]), _depth_index_numpy(np.nan_to_num(x), n["minmax"])[0]):
        assert (idx[np.isnan(x)] == 0).all() and (idx[x == np.inf] == 255).all() and (idx[x == -np.inf] == 0).all()
    # from the data's own range +-FLT_MAX: the denominator overflows to inf, t is 0 or inf / inf = NaN: index 0 everywhere
    assert (IC.index_reference(IC.depth_case("nonfinite")["depth"]) == 0).all()


def test_visualize_depth_numpy_starts_at_the_smallest_positive_depth():
    from uc_nerf_amd.utils.utils import visualize_depth_numpy
    table = IC.random_table()
    depth = IC.depth_case("random")["depth"].copy()
    depth[:3] = 0.0                                          # background
    img, (mi, ma) = visualize_depth_numpy(depth, cmap=table)
    assert img.shape == depth.shape + (3,) and img.dtype == np.uint8 and mi == depth[depth > 0].min() and ma == depth.max()
    assert (img[:3] == table[0]).all()                       # below the range: index 0
    img2, mm = visualize_depth_numpy(depth, minmax=(1.0, 6.0), cmap=table)
    assert np.array_equal(img2, table[IC.index_reference(depth, (1.0, 6.0))]) and mm == [1.0, 6.0]


def _library():
    from uc_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("no library is built")
    return _lib


def test_the_entry_points_are_exported_and_nothing_of_the_abi_moved():
    L = _library()
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), "library does not export " + name
        assert name in L.SYMBOLS and name + "(" in hdr
    assert "utils/utils.py:58-77" in hdr and "STRICTER THAN NUMPY" in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    for cname, cls in L.STRUCTS.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == C.sizeof(cls), cname
    for sname, size in NEW_STRUCTS.items():
        assert sname not in L.STRUCTS and "struct %s {" % sname in hdr
        cls = L.ADDED_STRUCTS[sname]
        assert L.lib().ucnerf_sizeof(sname.encode()) == C.sizeof(cls) == size, sname
        body = hdr.split("struct %s {" % sname)[1].split("};")[0]
        declared = []
        for line in body.splitlines():
            if ";" in line:
                decl = line.split(";")[0]
                for t in ("const float*", "const uint32_t*", "const uint8_t*", "uint32_t*", "uint8_t*", "float*", "int32_t", "double"):
                    decl = decl.replace(t, "")
                declared += [n.strip().split("[")[0] for n in decl.split(",")]
        assert declared == [f[0] for f in cls._fields_], (declared, [f[0] for f in cls._fields_])
    assert L.lib().ucnerf_image_group_pixels() == IC.GROUP_PIXELS
    src = open(os.path.join(ROOT, "uc_nerf_amd", "csrc", "image.hip")).read()
    assert "hipStreamSynchronize" not in src and "hipDeviceSynchronize" not in src and "hipMemcpy" not in src      # nothing waits, nothing is read back
    from uc_nerf_amd import build as B
    assert "image.hip" in B.SOURCES


def test_argument_errors_are_einval_in_a_child_process():
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    _library()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "image_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 30 and not out["problems"], out["problems"]
    assert out["group_pixels"] == IC.GROUP_PIXELS


def test_wrappers_refuse_what_they_cannot_do():
    from uc_nerf_amd import ops
    from uc_nerf_amd import validate
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.image_put(torch.rand(4, 3), torch.rand(4), 0, torch.zeros(3, 2, 2), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.depth_minmax(torch.rand(4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.depth_colormap(torch.rand(4))
    with pytest.raises(RuntimeError, match="range cell"):
        ops.minmax_value(torch.zeros(2))
    assert list(inspect.signature(validate.render_validation_image).parameters) == [
        "args", "pose_ref", "outputs", "imgs_input", "photo_confidence", "H", "W", "near_fars", "render_kwargs", "network_fn", "depth_gt", "gt_rgb", "cmap"]
    src = inspect.getsource(validate)
    code = src.split('"""', 2)[2]                             # (the module docstring may name what the code must not do)
    for banned in (".cpu()", ".item()", ".tolist()", ".numpy()"):
        assert banned not in code, banned
