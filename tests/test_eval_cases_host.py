"""Host-side checks of the evaluation metrics (ucnerf_depth_eval, ucnerf_image_eval, uc_nerf_amd.utils.evaluation).  No GPU: every case builder
of tests/eval_cases.py self-checks, the float32 numpy restatement reproduces fixture G20 -- the reference's own output, which pins what the GPU
tests compare the kernels with at other shapes --, the exact cases equal their closed forms, the library exports the new entry points with
nothing of ABI v6 moved, and the entry points validate their arguments before anything is launched."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


@pytest.mark.parametrize("name", E.MEDIAN_NAMES)
def test_median_builders_self_check(name):
    case = E.median(name)
    N = E.check_median_case(case)
    assert N == int(case["f32"]["counts"][:, 0].sum()) and case["f32"]["medians"][0].dtype == F32


@pytest.mark.parametrize("name", tuple(E.EXACT_SPECS))
def test_exact_error_cases_equal_their_closed_forms(name):
    case = E.exact(name)                                     # (check_exact ran in the builder: restatements agree, closed forms hold)
    n, N = E.EXACT_SPECS[name]
    assert case["gt"].shape == (n, 1, N + 3) and float(case["f32"]["ratio"]) == 1.0
    assert bool((case["f32"]["counts"][:, 1] < N).all()) and bool((case["f32"]["counts"][:, 3] > 0).all())      # the thresholds separate pixels


@pytest.mark.parametrize("n", E.EXACT_IMAGE_N)
@pytest.mark.parametrize("hw", E.EXACT_IMAGE_HW)
def test_exact_image_cases_equal_their_closed_forms(n, hw):
    gt, pred, want = E.exact_image(n, *hw)
    d = (gt.astype(F64) - pred.astype(F64)) ** 2
    assert E.same_bits(want, (d.reshape(n, -1).sum(-1) / (3 * hw[0] * hw[1])).astype(F32))      # the float64 quotient rounds to the same float32
    assert float(np.abs(E.image_reference(gt, pred, F64)["mse"] - want).max()) <= 2.0 ** -23 * float(want.max())


def test_float32_restatement_reproduces_the_reference_fixture():
    g = E.load_g20()
    r = E.cont_depth("g20")["f32"]
    assert g["gt_depths"].shape == (3, 12, 16) and g["gt_depths"].dtype == F32 and g["mean_errors"].dtype == F64
    assert bool((g["gt_depths"][0, 4:6] == 0).all()) and bool((g["gt_depths"][1] == 0).all())      # the band of zeros, the skipped image
    assert list(r["flags"]) == [False, True, False] and list(g["kept"]) == [0, 2]
    assert r["ratio"].dtype == F32 and r["ratio"] == g["ratio"] and r["medians"][0] == g["median_gt"] and r["medians"][1] == g["median_pred"]
    assert np.array_equal(r["counts"][g["kept"]], g["counts"])
    rel = np.abs(r["errors"][g["kept"], :4] - g["errors"][:, :4]) / np.abs(g["errors"][:, :4])
    print("restatement against G20, largest relative distance:", rel.max())
    assert rel.max() <= 1e-6
    assert np.array_equal(r["errors"][g["kept"], 4:], g["errors"][:, 4:])                              # a1, a2, a3: integer quotients in float64
    assert np.abs(r["mean"] - g["mean_errors"]).max() <= 1e-6 * np.abs(g["mean_errors"]).max()
    # lines 82-83: the restated image error against the captured one
    i = E.image_reference(g["gts"], g["predicts"], F32)
    assert E.same_bits(i["mse"], g["mse"]) and abs(float(i["psnr"].mean()) - float(g["psnr"])) <= 1e-6 * float(g["psnr"])


def test_ssim_restatement_properties():
    """Identical images give exactly 1; one window equals the sample-covariance closed form; float32 and float64 agree to float32 precision."""
    gt, pred = E.image_pair(1, 7, 7, "random")
    assert abs(float(E.ssim_reference(gt, pred, F64)[0]) - E.ssim_one_window(gt[0], pred[0])) <= 1e-12
    for kind in ("identical", "constant"):
        gt, pred = E.image_pair(2, 9, 12, kind)
        assert bool((E.ssim_reference(gt, pred, F64) == 1.0).all())
    gt, pred = E.image_pair(2, 9, 12, "complement")
    assert bool((E.ssim_reference(gt, pred, F64) < 0).all())                                        # anti-correlated
    gt, pred = E.image_pair(1, 23, 22, "random")
    assert abs(float(E.ssim_reference(gt, pred, F64)[0]) - float(E.ssim_reference(gt, pred, F32)[0])) < 1e-5


def test_bars_are_float32_sized():
    b = E.bars()
    print("continuous bars (4 x float32 restatement against float64):", b)
    assert set(b) == set(E.BAR_NAMES)
    for name in E.CONT_DEPTH_NAMES:
        c = E.cont_depth(name)
        kept = ~c["f64"]["flags"]
        scale = np.abs(c["f64"]["errors"][kept, :4]).max(0)
        for j, k in enumerate(E.ERR_NAMES):
            assert E.depth_distances(c["f32"]["errors"], c["f64"])[k] <= 2.0 ** -18 * scale[j], (name, k)
    assert b["ssim"] < 1e-4 and b["mse"] < 1e-6 and b["psnr"] < 1e-3


def test_the_entry_points_are_exported_and_nothing_of_the_abi_moved(L):
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    for name in ("ucnerf_depth_eval", "ucnerf_image_eval", "ucnerf_eval_workspace_floats"):
        assert hasattr(raw, name), "library does not export " + name
        assert name in L.SYMBOLS and name + "(" in hdr
    assert "utils/evaluation.py:8-74" in hdr and ":76-101" in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    for cname, cls in L.STRUCTS.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == C.sizeof(cls), cname
    for sname, size in (("ucnerf_depth_eval_params", 4 * 4 + 2 * 4 + 5 * 8), ("ucnerf_image_eval_params", 4 * 4 + 4 * 8)):
        assert sname not in L.STRUCTS and "struct %s {" % sname in hdr
        cls = L.ADDED_STRUCTS[sname]
        assert L.lib().ucnerf_sizeof(sname.encode()) == C.sizeof(cls) == size
        body = hdr.split("struct %s {" % sname)[1].split("};")[0]
        declared = []
        for line in body.splitlines():
            if ";" in line:
                decl = line.split(";")[0]
                for t in ("const float*", "const uint8_t*", "float*", "int32_t", "float"):
                    decl = decl.replace(t, "")
                declared += [n.strip() for n in decl.split(",")]
        assert declared == [f[0] for f in cls._fields_], (declared, [f[0] for f in cls._fields_])
    # the workspace holds the histograms, the state words and one 8-word partial per block
    ws = L.lib().ucnerf_eval_workspace_floats
    assert ws(1, 1, 1) >= 4 * 4 * 256 + 16 + 8 and ws(10, 256, 320) >= max(4 * 4 * 256 + 16 + 10 * 64 * 8, 2 * 10 * 3 * 16 * 20 + 10 * 64 * 2)
    assert ws(10, 256, 320) < 100000                          # (nothing the size of an image)


def test_argument_errors_are_einval_in_a_child_process(L):
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "eval_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 40 and not out["problems"], out["problems"]


def test_wrappers_and_mirror_refuse_what_they_cannot_do():
    import torch
    import uc_nerf_amd
    from uc_nerf_amd import ops
    from uc_nerf_amd.utils import evaluation as M
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.depth_eval(torch.rand(1, 4, 5), torch.rand(1, 4, 5))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.image_eval(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
    for name in ("compute_errors", "depth_evaluation", "rgb_evaluation"):
        assert callable(getattr(M, name))
    import inspect
    assert list(inspect.signature(M.depth_evaluation).parameters) == ["gt_depths", "pred_depths", "savedir", "pred_masks", "min_depth", "max_depth"]
    assert list(inspect.signature(M.rgb_evaluation).parameters) == ["gts", "predicts", "savedir", "lpips_fn"]
    assert list(inspect.signature(M.compute_errors).parameters) == ["gt", "pred"]
    uc_nerf_amd.install_dropin()
    import utils.evaluation as ref_named
    assert ref_named is M
