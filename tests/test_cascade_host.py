"""Host-side checks of the cascade link (ucnerf_depth_hypotheses, the get_*depth_range_samples mirrors, CascadeMVSNet).  No GPU: the torch
restatement of the reference's op chain (tests/cascade_stubs.py) reproduces fixture G19 -- which pins what the GPU tests compare the kernel with
at other shapes --, the library exports the new entry point with nothing of ABI v6 moved, the entry point validates its arguments before anything
is launched, and the mirror class refuses what it cannot do."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import cascade_stubs as S
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sizeof() of every ABI struct before this entry point existed (ABI v6)
KNOWN_SIZES = {
    "ucnerf_ray_gen_params": 200, "ucnerf_ndc_rays_params": 64, "ucnerf_dir_feature_params": 96, "ucnerf_sample_stratified_params": 56,
    "ucnerf_sample_cascade_params": 56, "ucnerf_ndc_project_params": 208, "ucnerf_embed_params": 32, "ucnerf_feat_gather_params": 176,
    "ucnerf_feat_gather_bwd_params": 264, "ucnerf_mlp_config": 16, "ucnerf_mlp_params": 96, "ucnerf_mlp_bwd_params": 152,
    "ucnerf_composite_params": 112, "ucnerf_composite_bwd_params": 152, "ucnerf_sample_pdf_params": 96, "ucnerf_render_params": 568,
    "ucnerf_render_bwd_params": 696, "ucnerf_merge_rows_params": 48, "ucnerf_cost_volume_params": 64, "ucnerf_depth_regress_params": 64,
    "ucnerf_cost_volume_bwd_params": 80, "ucnerf_depth_regress_bwd_params": 88, "ucnerf_cl_sources": 48, "ucnerf_cl_grads": 32,
    "ucnerf_build_rays_test_params": 200,
}


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_cascade")


def _max_err(got, want):
    return (got - want).abs().max().item()


def test_the_restated_chain_reproduces_the_reference_fixture(g19):
    g = g19
    near, far = g["near_far"][0], g["near_far"][1]
    H, W, pad = g["H"], g["W"], g["pad"]
    D1, D2, D3 = (int(d) for d in g["ndepths"])
    bar = S.bar(far)
    interval = (far - near) / 48                                          # mvs_models.py:694,698
    row = near * (1. - torch.linspace(0., 1., 48)) + far * torch.linspace(0., 1., 48)
    errs = {"stage1": _max_err(S.row_chain(row, D1, (H // 4, W // 4)), g["depth_values1"])}
    got2, _ = S.hypotheses_chain(g["depth1"], near, far, 2 * interval, D2, (H, W), (H // 2, W // 2))
    got3, _ = S.hypotheses_chain(g["depth2"], near, far, 1 * interval, D3, (H, W), (H, W), pad=pad)
    errs["stage2"], errs["stage3"] = _max_err(got2, g["depth_values2"]), _max_err(got3, g["depth_values3"])
    assert got3.shape == (D3, H + 2 * pad, W + 2 * pad) == g["depth_values3"].shape
    got_map, (lo, hi, c) = S.hypotheses_chain(g["map_cur_depth"][0], g["map_near"], g["map_far"], g["map_interval"], g["map_ndepth"],
                                              g["map_cur_depth"].shape[1:], g["map_cur_depth"].shape[1:])
    errs["map"] = _max_err(got_map, g["map_samples"][0])
    # the fixture's map exercises both clamps on part of the pixels
    half = g["map_ndepth"] / 2 * g["map_interval"]
    for bites in (c - half < g["map_near"], c + half > g["map_far"]):
        assert 0 < int(bites.sum()) < bites.numel()
    errs["row"] = _max_err(S.row_chain(g["row_in"][0], g["row_ndepth"], g["row_samples"].shape[2:]), g["row_samples"][0])
    print("restated chain against G19, max |err| (bar %.3e):" % bar, errs)
    assert all(e <= bar for e in errs.values()), errs


def test_the_entry_point_is_exported_and_nothing_of_the_abi_moved(L):
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    name = "ucnerf_depth_hypotheses"
    assert hasattr(raw, name), "library does not export " + name
    assert name in L.SYMBOLS and name + "(" in hdr
    assert "network/mvs_models.py:536-573" in hdr and "693-762" in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION
    assert "#define UCNERF_ABI_VERSION 6" in hdr
    for cname, size in KNOWN_SIZES.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == size == C.sizeof(L.STRUCTS[cname]), cname
    # the new struct: declared in the header, registered with ucnerf_sizeof() under its own name, mirrored field for field
    sname = "ucnerf_depth_hypotheses_params"
    assert sname not in KNOWN_SIZES and "struct %s {" % sname in hdr
    cls = L.ADDED_STRUCTS[sname]
    assert L.lib().ucnerf_sizeof(sname.encode()) == C.sizeof(cls) > 0
    body = hdr.split("struct %s {" % sname)[1].split("};")[0]
    declared = [n.strip().lstrip("*") for line in body.splitlines() if ";" in line
                for n in line.split(";")[0].replace("const float*", "").replace("float*", "").replace("int32_t", "").replace("float", "").split(",")]
    assert declared == [f[0] for f in cls._fields_], (declared, [f[0] for f in cls._fields_])


def test_argument_errors_are_einval_in_a_child_process(L):
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cascade_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 30 and not out["problems"], out["problems"]


def test_ops_wrapper_refuses_cpu_tensors():
    from uc_nerf_amd import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.depth_hypotheses(8, (4, 5), cur_depth=torch.rand(4, 5), near_far=torch.tensor([1.0, 2.0]), k=1 / 48)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.depth_hypotheses(8, (4, 5), row=torch.rand(48))
    with pytest.raises(RuntimeError, match="exactly one"):
        ops.depth_hypotheses(8, (4, 5))


def test_the_mirror_class_refuses_what_it_cannot_do_and_is_reachable_through_the_dropin():
    import uc_nerf_amd
    from uc_nerf_amd.network import mvs_models as M
    with pytest.raises(ValueError, match="feature.*cost_regularization"):
        M.CascadeMVSNet()
    feature, regs = S.make_stubs(3, 32, 40, [torch.zeros(s) for s in S.stage_logit_shapes(32, 40, [48, 32, 8], 2)])
    with pytest.raises(ValueError, match="cost_regularization"):
        M.CascadeMVSNet(feature=feature)
    with pytest.raises(NotImplementedError, match="other"):
        M.CascadeMVSNet(grad_method="other", feature=feature, cost_regularization=regs)
    net = M.CascadeMVSNet(feature=feature, cost_regularization=regs)
    assert net.feature is feature and len(net.cost_regularization) == 3 and net.ndepths == [48, 32, 8] and net.depth_interals_ratio == [4, 2, 1]
    assert any(k.startswith("cost_regularization.2.") for k in net.state_dict()) and any(k.startswith("feature.") for k in net.state_dict())
    shared = M.CascadeMVSNet(share_cr=True, feature=feature, cost_regularization=regs[0])
    assert shared.cost_regularization is regs[0]
    uc_nerf_amd.install_dropin()
    import network.mvs_models as ref_named
    assert ref_named is M and ref_named.CascadeMVSNet is M.CascadeMVSNet
    for name in ("CascadeMVSNet", "DepthNet", "get_depth_range_samples", "get_cur_depth_range_samples", "mvs_depth_regression"):
        assert callable(getattr(ref_named, name))
    # DepthNet's signature as its existing callers know it, plus the keyword-only switch the stage loop uses
    import inspect
    sig = inspect.signature(M.DepthNet.forward)
    assert list(sig.parameters)[:10] == ["self", "features", "affine_mat_stage", "affine_mat_inv_stage", "depth_values", "num_depth",
                                         "cost_regularization", "imgs", "pad", "prob_volume_init"]
    assert sig.parameters["depth_values_padded"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["depth_values_padded"].default is False
