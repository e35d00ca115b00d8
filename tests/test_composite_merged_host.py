"""Host-side checks of the merged compositing entry point (ucnerf_composite_merged_fwd).  No GPU: the library exports it with nothing of ABI v6
moved, the binding mirrors its struct field for field, and the entry point validates its arguments before anything is launched."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sizeof() of every ABI struct before this entry point existed (ABI v6 and its earlier additions)
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


def test_the_entry_point_is_exported_and_nothing_of_the_abi_moved(L):
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    name, sname = "ucnerf_composite_merged_fwd", "ucnerf_composite_merged_params"
    assert hasattr(raw, name), "library does not export " + name
    assert name in L.SYMBOLS and "int %s(const %s* p, void* stream);" % (name, sname) in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION
    assert "#define UCNERF_ABI_VERSION 6" in hdr
    for cname, size in KNOWN_SIZES.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == size == C.sizeof(L.STRUCTS[cname]), cname
    assert set(L.STRUCTS) == set(KNOWN_SIZES)                        # the v6 table itself is as it was
    for cname, cls in L.ADDED_STRUCTS.items():                       # (the earlier additions are still there)
        assert L.lib().ucnerf_sizeof(cname.encode()) == C.sizeof(cls) > 0, cname
    assert {"ucnerf_merge_rows", "ucnerf_composite_fwd"} <= set(L.SYMBOLS) and hasattr(raw, "ucnerf_merge_rows")
    # the new struct: declared in the header, registered with ucnerf_sizeof() under its own name, mirrored field for field
    assert sname not in KNOWN_SIZES and "struct %s {" % sname in hdr
    cls = L.ADDED_STRUCTS[sname]
    assert L.lib().ucnerf_sizeof(sname.encode()) == C.sizeof(cls) == 4 * 4 + 12 * 8
    body = hdr.split("struct %s {" % sname)[1].split("};")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []                                                    # (name, is a pointer)
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(float|int32_t)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        declared += [(n.strip(), bool(m.group(2))) for n in m.group(3).split(",")]
    mirrored = [(f[0], f[1] is L.vp) for f in cls._fields_]
    assert declared == mirrored, (declared, mirrored)


def test_argument_errors_are_einval_in_a_child_process(L):
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "composite_merged_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 25 and not out["problems"], out["problems"]


def test_an_evaluation_only_render_pass_is_validated(L):
    """ucnerf_render_fused_fwd without rgb_map / depth_map ends after the network (the rows go to ucnerf_composite_merged_fwd): it needs raw and
    may ask for no compositing output."""
    lib = L.lib()
    r = L.RenderParams()
    r.n, r.S, r.cfg = 4, 64, L.MlpConfig(6, 0, 3)
    r.rays_o = r.rays_d = r.z = r.workspace = r.wstream = 16
    assert lib.ucnerf_render_fused_fwd(C.addressof(r), None) == -1 and b"null pointer" in lib.ucnerf_last_error()       # neither maps nor raw
    r.raw, r.rgb_map = 16, 16
    assert lib.ucnerf_render_fused_fwd(C.addressof(r), None) == -1 and b"null pointer" in lib.ucnerf_last_error()       # one map without the other
    r.rgb_map = None
    for field in ("acc_map", "weights", "var"):
        setattr(r, field, 16)
        assert lib.ucnerf_render_fused_fwd(C.addressof(r), None) == -1 and b"evaluates the network into raw only" in lib.ucnerf_last_error(), field
        setattr(r, field, None)


def test_ops_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    import torch
    from uc_nerf_amd import ops
    a, b, z = torch.rand(2, 3, 4), torch.rand(2, 2, 4), torch.rand(2, 5)
    rank = torch.arange(5, dtype=torch.int32).repeat(2, 1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.composite_merged_fwd(a, b, rank, z)


def test_the_reuse_predicate_follows_the_tail_route_size(L):
    """ucnerf_reuse_coarse_pays: 0 exactly where the pass over all depths is of the size that composites inside its own launch (on a machine
    without a device no pass is), and 0 for sizes that are no pass at all."""
    lib = L.lib()
    assert "int32_t ucnerf_reuse_coarse_pays(int32_t n, int32_t n_coarse, int32_t n_fine);" in open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    for n in (1, 37, 300, 500, 512, 1024, 1100, 4096):
        for nc, nf in ((64, 128), (17, 40), (3, 1)):
            assert lib.ucnerf_reuse_coarse_pays(n, nc, nf) == 1 - lib.ucnerf_fused_tail_fits(n, nc + nf), (n, nc, nf)
    assert lib.ucnerf_reuse_coarse_pays(0, 64, 128) == 0 and lib.ucnerf_reuse_coarse_pays(8, 0, 128) == 0 and lib.ucnerf_reuse_coarse_pays(8, 64, 0) == 0
