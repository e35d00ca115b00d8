"""The evaluation metrics on the GPU: ucnerf_depth_eval / ucnerf_image_eval and the uc_nerf_amd.utils.evaluation mirror against the numpy
restatements of tests/eval_cases.py (pinned to the reference's own output by fixture G20 in tests/test_eval_cases_host.py).

Medians, ratio and every count are compared exactly (np.median on float32; integers); the exact cases bit for bit; the continuous cases against
the float64 restatement under bars()[name] = 4 x the float32 restatement's own largest distance from it.

Measured on an MI355X (bars taken on a host with glibc 2.35 and numpy 2.2.6; the device's largest distance / bar over the continuous cases, per
case in profiles/eval_metrics.md): abs_rel 6.8e-8 / 2.1e-7, sq_rel 1.8e-6 / 1.2e-5, rmse 5.8e-7 / 2.3e-6, rmse_log 1.2e-7 / 3.7e-7, mse 1.6e-8 / 7.8e-8,
psnr 5.5e-7 / 1.5e-5, ssim 2.8e-8 / 2.3e-7 (2.9e-8 over the SSIM shape sweep)."""
import numpy as np
import pytest
import torch

import eval_cases as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F32, F64 = np.float32, np.float64
SSIM_TILE = E.SSIM_TILE                               # 16 windows per tile side (csrc/metrics.hip: SSIM_TILE); the staged tile is 22 x 22 pixels


def ops():
    from uc_nerf_amd import ops as o
    return o


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_depth(case):
    out = ops().depth_eval(dev(case["gt"]), dev(case["pred"]), dev(case["mask"]), case["min_depth"], case["max_depth"])
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_exact_fields(case, got):
    """Medians and ratio bit for bit (+-0 equal, NaN matching NaN), every count as an integer, the flags."""
    r = case["f32"]
    name = case["name"]
    assert bool(got["empty"][0]) == r["empty"], name
    assert E.same_bits(got["medians"], np.array(r["medians"], F32)), (name, got["medians"], r["medians"])
    assert E.same_bits(got["ratio"][0], r["ratio"]), (name, got["ratio"], r["ratio"])
    assert np.array_equal(got["counts"].astype(np.int64), r["counts"]), (name, got["counts"], r["counts"])
    assert np.array_equal(got["flags"] != 0, r["flags"]), name


@pytest.mark.parametrize("name", E.MEDIAN_NAMES)
def test_median_ratio_and_counts_are_exact(name):
    case = E.median(name)
    check_exact_fields(case, run_depth(case))


@pytest.mark.parametrize("name", tuple(E.EXACT_SPECS))
def test_exact_error_cases_bit_for_bit(name):
    case = E.exact(name)
    got = run_depth(case)
    check_exact_fields(case, got)
    assert float(got["ratio"][0]) == 1.0
    for j in (0, 1, 2):                                                   # abs_rel, sq_rel, rmse (rmse_log: log is not exact)
        assert E.same_bits(got["errors"][:, j], case["f32"]["errors"][:, j].astype(F32)), (name, E.ERR_NAMES[j], got["errors"][:, j], case["f32"]["errors"][:, j])
    n = case["f32"]["counts"][:, 0].astype(F64)
    assert E.same_bits(got["errors"][:, 4:7], (case["f32"]["counts"][:, 1:4] / n[:, None]).astype(F32))


@pytest.mark.parametrize("name", E.CONT_DEPTH_NAMES)
def test_continuous_depth_errors_within_the_bar(name):
    case = E.cont_depth(name)
    got = run_depth(case)
    check_exact_fields(case, got)
    dist = E.depth_distances(got["errors"], case["f64"])
    bars = E.bars()
    print("%s: device distance / bar  " % case["name"] + "  ".join("%s %.3e / %.3e" % (k, dist[k], bars[k]) for k in E.ERR_NAMES))
    assert not E.over_the_bar(dist, case["name"])


def test_all_invalid_sets_the_flag_and_nothing_else_breaks():
    gt = np.zeros((2, 5, 7), F32)
    got = ops().depth_eval(dev(gt), dev(gt + 1))
    assert int(got["empty"][0]) == 1 and bool(torch.isnan(got["ratio"]).all()) and got["flags"].tolist() == [1, 1]
    assert got["counts"].tolist() == [[0, 0, 0, 0]] * 2 and bool(torch.isnan(got["errors"]).all())


def run_image(gt, pred, **kw):
    out = ops().image_eval(dev(gt), dev(pred), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("n", E.EXACT_IMAGE_N)
@pytest.mark.parametrize("hw", E.EXACT_IMAGE_HW)
def test_exact_image_error_bit_for_bit(n, hw):
    gt, pred, want = E.exact_image(n, *hw)
    small = hw[0] < 7 or hw[1] < 7                                        # no SSIM window fits: the image error on its own
    got = run_image(gt, pred, ssim=not small)
    assert E.same_bits(got["mse"], want), (got["mse"], want)
    assert E.same_bits(got["gt_max"], gt.reshape(n, -1).max(-1))
    assert bool(np.isnan(got["ssim"]).all()) == small
    if small:
        with pytest.raises(RuntimeError, match="7 x 7 SSIM window"):
            ops().image_eval(dev(gt), dev(pred))


@pytest.mark.parametrize("name", E.CONT_IMAGE_NAMES)
def test_continuous_image_metrics_within_the_bar(name):
    case = E.cont_image(name)
    got = run_image(case["gt"], case["pred"])
    dist = E.image_distances(got, case["f64"])
    bars = E.bars()
    print("%s: device distance / bar  " % case["name"] + "  ".join("%s %.3e / %.3e" % (k, dist[k], bars[k]) for k in E.IMG_NAMES))
    assert not E.over_the_bar(dist, case["name"])


# 7 x 7 (one window), 7 x W, H x 7, 8 x 8; the tile of 16 x 16 windows minus one, exact and plus one in both directions (H - 6 windows down: 21, 22,
# 23) and the same around TWO tiles (37, 38, 39) and around the tile size taken as pixels (15, 16, 17)
T = SSIM_TILE
SSIM_SHAPES = [(7, 7), (7, 40), (40, 7), (8, 8)] + [(T + 6 + a, T + 6 + b) for a in (-1, 0, 1) for b in (-1, 0, 1)] + \
              [(2 * T + 6 + a, T - 1) for a in (-1, 0, 1)] + [(T + 1, 2 * T + 6 + b) for b in (-1, 0, 1)] + [(T + a, T + a) for a in (-1, 0, 1)]


@pytest.mark.parametrize("hw", SSIM_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_ssim_shapes_and_contents(hw):
    H, W = hw
    bar = E.bars()["ssim"]
    worst = 0.0
    for kind in ("identical", "constant", "complement", "random"):
        case = E.image_case(2, H, W, kind)
        got = run_image(case["gt"], case["pred"])
        d = float(np.abs(got["ssim"].astype(F64) - case["f64"]["ssim"]).max())
        worst = max(worst, d)
        assert d <= bar, (hw, kind, got["ssim"], case["f64"]["ssim"], bar)
        if kind in ("identical", "constant"):
            assert bool((got["ssim"] == 1.0).all()), (hw, kind, got["ssim"])
        if (H, W) == (7, 7):                                              # one window: the closed form in float64
            for i in range(2):
                assert abs(float(got["ssim"][i]) - E.ssim_one_window(case["gt"][i], case["pred"][i])) <= bar, (kind, i)
    print("ssim %dx%d: largest distance %.3e, bar %.3e" % (H, W, worst, bar))


def test_two_calls_and_another_stream_give_the_same_bits():
    case = E.cont_depth("d_256x320")
    gt, pred, mask = dev(case["gt"]), dev(case["pred"]), dev(case["mask"])
    icase = E.cont_image("i_33x47")
    igt, ipred = dev(icase["gt"]), dev(icase["pred"])
    torch.cuda.synchronize()
    first, again = ops().depth_eval(gt, pred, mask), ops().depth_eval(gt, pred, mask)
    ifirst, iagain = ops().image_eval(igt, ipred), ops().image_eval(igt, ipred)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other, iother = ops().depth_eval(gt, pred, mask), ops().image_eval(igt, ipred)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b, c in ((first, again, other), (ifirst, iagain, iother)):
        for k in a:
            x, y, z = (t[k].contiguous().view(torch.int32) for t in (a, b, c))      # bits, so that NaN rows compare too
            assert torch.equal(x, y), k
            assert torch.equal(x, z), k


# ------------------------------------------------------------------------------------------------ the mirror
def test_mirror_depth_evaluation_on_the_fixture(capsys):
    from uc_nerf_amd.utils import evaluation as M
    g = E.load_g20()
    bars = E.bars()
    for where in ("numpy", "device"):
        gt, pred = g["gt_depths"].copy(), g["pred_depths"].copy()
        a, b = (gt, pred) if where == "numpy" else (dev(gt), dev(pred))
        got = M.depth_evaluation(a, b)
        assert isinstance(got, np.ndarray) and got.dtype == F64 and got.shape == (7,)
        assert np.array_equal(got[4:], g["mean_errors"][4:]), (where, got, g["mean_errors"])      # a1, a2, a3: integer counts over integer counts
        for j, k in enumerate(E.ERR_NAMES):
            assert abs(got[j] - g["mean_errors"][j]) <= bars[k], (where, k, got[j], g["mean_errors"][j], bars[k])
        if where == "numpy":
            assert np.array_equal(a, g["gt_depths"]) and np.array_equal(b, g["pred_depths"])
        else:
            assert np.array_equal(a.cpu().numpy(), g["gt_depths"]) and np.array_equal(b.cpu().numpy(), g["pred_depths"])
        printed = capsys.readouterr().out
        assert printed == str(g["printed"]), (printed, str(g["printed"]))                           # the reference's two table lines
    # a full-resolution mask is honoured; another size is cv2's business
    mask = np.ones(gt.shape, bool)
    mask[0] = False
    want = E.depth_reference(gt, pred, mask.astype(np.uint8), dtype=F64)["mean"]
    got = M.depth_evaluation(gt, pred, pred_masks=mask)
    assert np.array_equal(got[4:], want[4:]) and all(abs(got[j] - want[j]) <= bars[k] for j, k in enumerate(E.ERR_NAMES))
    with pytest.raises(NotImplementedError, match="cv2.resize"):
        M.depth_evaluation(gt, pred, pred_masks=np.ones((3, 6, 8), bool))
    with pytest.raises(ValueError):
        M.depth_evaluation(np.zeros((2, 5, 7), F32), np.ones((2, 5, 7), F32))


def test_mirror_compute_errors_and_rgb_evaluation(tmp_path):
    from uc_nerf_amd.utils import evaluation as M
    bars = E.bars()
    case = E.cont_depth("d_37x53")
    v = (case["gt"] > 1e-4) & (case["gt"] < 100)
    gt, pred = case["gt"][v], np.clip(case["pred"][v] * F32(2.7), F32(0.2), F32(30))      # (no median scaling here: bring the predictions to the depths' scale)
    want, counts = E.compute_errors(gt.astype(F64), pred.astype(F64))
    got = M.compute_errors(gt, pred)
    assert len(got) == 7 and got[4:] == tuple(want[4:])
    for j, k in enumerate(E.ERR_NAMES):
        assert abs(float(got[j]) - float(want[j])) <= bars[k], (k, got[j], want[j], bars[k])
    g = E.load_g20()
    psnr, ssim, lp = M.rgb_evaluation(g["gts"], g["predicts"], str(tmp_path))
    ref = E.image_reference(g["gts"], g["predicts"], F64)
    assert abs(float(psnr) - float(g["psnr"])) <= bars["psnr"] and abs(float(ssim) - float(ref["ssim"].mean())) <= bars["ssim"]
    assert lp != lp and (tmp_path / "rgb_evaluation.txt").exists()
    seen = {}

    def lpips_fn(a, b):
        seen["range"] = (float(a.min()), float(a.max()), a.shape, b.shape, a.is_cuda)
        return torch.full((a.shape[0], 1, 1, 1), 0.25, device=a.device)

    p2, s2, lp2 = M.rgb_evaluation(dev(g["gts"]), dev(g["predicts"]), None, lpips_fn=lpips_fn)
    assert float(lp2) == 0.25 and p2 == psnr and s2 == ssim
    assert seen["range"][0] >= -1 and seen["range"][1] <= 1 and seen["range"][2] == seen["range"][3] == g["gts"].shape and seen["range"][4]
    assert M.rgb_evaluation(g["gts"], g["predicts"], None, lpips_fn=lambda a, b: 0.5)[2] == 0.5
    with pytest.raises(AssertionError):
        M.rgb_evaluation(g["gts"] * 2, g["predicts"], None)
