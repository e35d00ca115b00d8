"""Host-side checks of the guarded fp16 split ("fp16_guarded": range detection on the device, conditional replay on bf16 terms).  No GPU: the mode is
accepted, the library exports the new entry points next to the old ones, ABI version and every struct size are what they were, and the new entry
points validate their arguments -- a null status word is UCNERF_EINVAL -- before anything is launched."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ucnerf_mlp_fwd_guarded", "ucnerf_mlp_fwd_if", "ucnerf_mlp_pack_guarded", "ucnerf_mlp_pack_if", "ucnerf_mlp_pack_tensors_guarded",
               "ucnerf_mlp_pack_tensors_if", "ucnerf_render_fused_fwd_guarded", "ucnerf_render_fused_fwd_if"]

# sizeof() of every ABI struct at the commit before this mode existed (ABI v6): the guarded calls are additive, no struct may move
PARENT_SIZES = {
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


def test_the_mode_is_accepted_everywhere_a_split_operand_is_named():
    import uc_nerf_amd
    from uc_nerf_amd import ops
    dev = torch.device("cpu")
    try:
        ops.set_split_operand("fp16_guarded")
        assert ops.split_operand() == "fp16_guarded"
        g = ops.PackedWeights.get(6, 0, dev, "bf16x3_fused")
        h = ops.PackedWeights.get(6, 0, dev, "bf16x3_fused", operand="fp16")
        b = ops.PackedWeights.get(6, 0, dev, "bf16x3_fused", operand="bf16")
        # the guard is a property of the CALL: the ABI's operand stays 1; the stream holds both term kinds, the second half for the replay
        assert g is not h and g.guarded and not h.guarded and not b.guarded
        assert (g.cfg.operand, g.cfg_bf16.operand, h.cfg.operand, b.cfg.operand) == (1, 0, 1, 0)
        assert g.operand not in (h.operand, b.operand)                 # (what the drop-in's stream cache keys on)
        assert g.n_stream == 2 * h.n_stream == 2 * b.n_stream and g.n_stream_terms == h.n_stream
        assert torch.equal(g.idx_host, h.idx_host) and torch.equal(g.idx_host, b.idx_host)      # one pack index serves both halves
        assert not ops.PackedWeights.get(6, 0, dev, "f32").guarded
        uc_nerf_amd.set_split_operand("fp16")
        assert ops.split_operand() == "fp16"
        uc_nerf_amd.install_dropin(split_operand="fp16_guarded")
        assert ops.split_operand() == "fp16_guarded"
        with pytest.raises(ValueError, match="fp16_guarded"):
            ops.set_split_operand("fp16-guarded")
    finally:
        ops.set_split_operand("bf16")
    assert callable(ops.split_guard_status) and callable(ops.split_guard_clear) and callable(uc_nerf_amd.split_guard_status)


def test_the_environment_variable_selects_the_mode():
    code = "import sys; sys.path.insert(0, %r); from uc_nerf_amd import ops; print(ops.split_operand())" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, UCNERF_SPLIT_OPERAND="fp16_guarded"), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "fp16_guarded", r.stderr[-2000:]


def test_new_entry_points_are_exported_and_nothing_of_the_abi_moved(L):
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), "library does not export " + name
        assert name in L.SYMBOLS and name + "(" in hdr, name
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION
    assert set(PARENT_SIZES) == set(L.STRUCTS)
    for cname, size in PARENT_SIZES.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == size == C.sizeof(L.STRUCTS[cname]), cname
    # the header says what holds: the "never an infinity" promise is the activation side's only
    assert "hi = inf, lo = -inf" in hdr and "activation" in hdr.split("hi = inf, lo = -inf")[0][-600:]


def test_null_status_word_and_bad_arguments_are_einval_in_a_child_process():
    """Probed through ctypes in a child (a crash must not take the run with it): the word is checked before anything could be launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "split_guard_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 30 and not out["problems"], out["problems"]
