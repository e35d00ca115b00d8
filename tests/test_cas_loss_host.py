"""Host-side checks of the device cascade depth loss (ucnerf_cas_loss_fwd / _bwd, ops.cas_loss, utils.loss.cas_mvsnet_loss_device).  No GPU: the
library exports the entry points with nothing of ABI v6 moved, they validate their arguments before anything is launched, the case builders of
tests/cas_loss_cases.py say what the CPU mirror says (so that the GPU tests compare the kernel with the mirror and not with a builder's slip), and
the default loss route is the expression it was."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import cas_loss_cases as CC
from conftest import load_golden
from uc_nerf_amd.utils import loss as UL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ucnerf_cas_loss_workspace_floats", "ucnerf_cas_loss_fwd", "ucnerf_cas_loss_bwd")
STRUCTS = ("ucnerf_cas_loss_params", "ucnerf_cas_loss_bwd_params")


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


def test_the_entry_points_are_exported_and_nothing_of_the_abi_moved(L):
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name), "library does not export " + name
        assert name in L.SYMBOLS and name + "(" in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    assert "network/mvs_models.py:512-529" in hdr and "THE ONE DIFFERENCE FROM TORCH" in hdr
    for sname in STRUCTS:
        assert sname not in L.STRUCTS and "struct %s {" % sname in hdr
        cls = L.ADDED_STRUCTS[sname]
        assert L.lib().ucnerf_sizeof(sname.encode()) == C.sizeof(cls) > 0
        body = hdr.split("struct %s {" % sname)[1].split("};")[0]
        declared = [(m.group(2), int(m.group(3) or 1)) for line in body.splitlines() if ";" in line
                    for m in [re.match(r"\s*(?:const )?(?:float|int32_t)(\*?) ?(\w+)(?:\[(\d)\])?;", line)]]
        mirrored = [(f[0], getattr(f[1], "_length_", 1)) for f in cls._fields_]
        assert declared == mirrored, (declared, mirrored)
    assert C.sizeof(L.CasLossParams) == 32 + 8 * 17 and C.sizeof(L.CasLossBwdParams) == 32 + 8 * 15


def test_argument_errors_are_einval_in_a_child_process(L):
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cas_loss_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 50 and not out["problems"], out["problems"]


def test_ops_wrapper_refuses_cpu_tensors_and_ragged_stages():
    from uc_nerf_amd import ops
    e, g, w = CC.random_stage(48, 0.3, torch.Generator().manual_seed(1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.cas_loss([e], [g], [w], [1.0])
    with pytest.raises(RuntimeError, match="1 to 3 stages"):
        ops.cas_loss([e] * 4, [g] * 4, [w] * 4, [1.0] * 4)
    with pytest.raises(RuntimeError, match="1 to 3 stages"):
        ops.cas_loss([], [], [], [])
    with pytest.raises(RuntimeError, match="1 to 3 stages"):
        ops.cas_loss([e], [g], None, [1.0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        UL.cas_mvsnet_loss_device(*CC.dicts([(e, g, w)]))
    assert UL.cas_mvsnet_loss_device({"depth": e}, {}, {}) == (0, None) == UL.cas_mvsnet_loss({"depth": e}, {}, {})      # no stage key: as the mirror


@pytest.mark.parametrize("pattern", CC.LATTICE_PATTERNS)
def test_lattice_builders_say_what_the_mirror_says(pattern):
    """Every lattice call: the builder's masks are what its name says, the float32 mirror equals the explicit-rank float64 restatement EXACTLY
    (all of it is exact on the lattice up to the division), and |est - gt| falls on both sides of 1 and at 1 wherever there is room."""
    for sizes in CC.LATTICE_GROUPS:
        stages = CC.lattice_call(sizes, pattern)
        for n, (est, gt, w) in zip(sizes, stages):
            valid = gt > 0
            count, run = int(valid.sum()), -(-n // 1024)
            assert torch.equal(valid, w > 0) and count >= 1
            assert count == n if pattern == "all" else count & (count - 1) == 0
            assert pattern != "last_one" or (count == 1 and valid[-1])
            assert pattern != "first_run" or not valid[run:].any()
            assert pattern != "last_run" or not valid[:n - run].any()
            assert torch.equal(est * 8, (est * 8).round()) and torch.equal(gt * 8, (gt * 8).round()) and 1 <= est.min() and est.max() < 5
            assert set(w[valid].tolist()) <= {0.5, 1.0, 2.0}
            d = (est - gt)[valid].abs()
            if count >= 8:
                assert (d == 1).any() and (d < 1).any() and (d > 1).any()
        total, last, grads = CC.mirror(stages)
        want = CC.by_rank(stages)
        if pattern == "all":          # (count = n: the mirror's division rounds once)
            assert abs(float(total) - want) <= 3 * 2.0 ** -24 * want
        else:
            assert float(total) == want, (pattern, sizes)
        assert all(g.shape == s[0].shape and (g != 0).sum() <= (s[1] > 0).sum() for g, s in zip(grads, stages))


def test_rank_pairing_case_cannot_degenerate_into_an_elementwise_one():
    stages = CC.rank_pairing_stages()
    for est, gt, w in stages:
        valid, pos = gt > 0, w > 0
        assert int(valid.sum()) == int(pos.sum()) >= 64 and not torch.equal(valid, pos)
        assert w[pos].unique().numel() == int(pos.sum())                 # all distinct: any other pairing changes the sum
    total, _, _ = CC.mirror(stages, dtype=torch.float64)
    by_rank, elementwise = CC.by_rank(stages), CC.by_rank(stages, elementwise=True)
    assert abs(float(total) - by_rank) <= 1e-12 * by_rank
    assert abs(elementwise - by_rank) > 1e-2 * by_rank, "a mask * w evaluation must NOT give the mirror's value on this case"


def test_random_builder_and_mirror_reproduce_the_reference_fixture():
    """G15 (captured from the reference's own Python): the mirror through the case helpers gives loss_mvs and the stage gradients / 0.05."""
    g = load_golden("g15_losses")
    stages = [(g[k + "_depth"], g[k + "_gt"], g[k + "_w"]) for k in ("stage1", "stage2", "stage3")]
    total, last, grads = CC.mirror(stages, scale=0.05)
    torch.testing.assert_close(total, torch.as_tensor(g["loss_mvs"]).reshape(()), atol=1e-7, rtol=1e-6)
    for k, gr in enumerate(grads):
        torch.testing.assert_close(gr, g["stage%d_g" % (k + 1)], atol=1e-7, rtol=1e-6)
    assert abs(CC.by_rank(stages) - float(total)) <= 1e-5 * float(total)
    e, gt, w = CC.random_stage((1, 6, 8), 0.3, torch.Generator().manual_seed(15))
    assert e.shape == (1, 6, 8) and torch.equal(gt > 0, w > 0) and 1 <= e.min() and e.max() < 4
    assert CC.ulp32(torch.tensor([1.0, 1.5, 0.75, 0.0])).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 0.0]


def test_default_route_of_the_training_loss_is_the_expression_it_was():
    """mvs_on_device defaults to False in both loss mixes, and the default result is, bit for bit, the mix formed with cas_mvsnet_loss."""
    import inspect
    from uc_nerf_amd import train_step as T
    for fn in (UL.training_loss, T.sharded_training_loss):
        assert inspect.signature(fn).parameters["mvs_on_device"].default is False
    assert inspect.signature(UL.cas_mvsnet_loss_device).parameters["status"].default is None
    assert list(inspect.signature(UL.cas_mvsnet_loss_device).parameters)[:5] == list(inspect.signature(UL.cas_mvsnet_loss).parameters)[:5]
    g = load_golden("g15_losses")
    outputs = {k: {"depth": g[k + "_depth"]} for k in ("stage1", "stage2", "stage3")}
    gt, w = {k: g[k + "_gt"] for k in outputs}, {k: g[k + "_w"] for k in outputs}
    kw = dict(n_rays=int(g["n_rays"]), patch_num=int(g["patch_num"]), patch_size=int(g["patch_size"]))
    loss, parts = UL.training_loss(g["rgb"], g["depth_pred"], g["target_s"], g["target_depths"], g["target_weights"], g["patch_dpt"], outputs, gt, w, **kw)
    mvs = UL.cas_mvsnet_loss(outputs, gt, w)[0]
    assert torch.equal(parts["loss_mvs"], mvs)
    mix = parts["loss_nerf_depth"] * 0.05 + mvs * 0.05 + parts["smooth_loss"] * 0.05 + parts["loss_scaleinvariant"] * 0.008 + parts["img_loss"] * 5.0
    assert torch.equal(loss, mix)
    sh = T.BatchShard(kw["n_rays"], g["rgb"].shape[0], kw["patch_num"], kw["patch_size"])
    l1, _ = T.sharded_training_loss(g["rgb"], g["depth_pred"], g["target_s"], g["target_depths"], g["target_weights"], g["patch_dpt"], outputs, gt, w, sh)
    l2, _ = T.sharded_training_loss(g["rgb"], g["depth_pred"], g["target_s"], g["target_depths"], g["target_weights"], g["patch_dpt"], outputs, gt, w, sh, mvs_term=mvs)
    assert torch.equal(l1, l2)
