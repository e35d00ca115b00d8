"""Host-side checks of the one-launch training ray builder (ucnerf_build_rays_train, ops.build_rays_train).  No GPU: the library exports the new
entry point with nothing of ABI v6 moved, the entry point validates its arguments before anything is launched, the wrapper refuses host tensors,
and the pixel plan the kernel implements -- restated in numpy below, where the GPU tests take it from -- reproduces fixture G18's pixels from G18's
recorded draws."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sizeof() of every struct of ABI v6's table
KNOWN_SIZES = {
    "ucnerf_ray_gen_params": 200, "ucnerf_ndc_rays_params": 64, "ucnerf_dir_feature_params": 96, "ucnerf_sample_stratified_params": 56,
    "ucnerf_sample_cascade_params": 56, "ucnerf_ndc_project_params": 208, "ucnerf_embed_params": 32, "ucnerf_feat_gather_params": 176,
    "ucnerf_feat_gather_bwd_params": 264, "ucnerf_mlp_config": 16, "ucnerf_mlp_params": 96, "ucnerf_mlp_bwd_params": 152,
    "ucnerf_composite_params": 112, "ucnerf_composite_bwd_params": 152, "ucnerf_sample_pdf_params": 96, "ucnerf_render_params": 568,
    "ucnerf_render_bwd_params": 696, "ucnerf_merge_rows_params": 48, "ucnerf_cost_volume_params": 64, "ucnerf_depth_regress_params": 64,
    "ucnerf_cost_volume_bwd_params": 80, "ucnerf_depth_regress_bwd_params": 88, "ucnerf_cl_sources": 48, "ucnerf_cl_grads": 32,
    "ucnerf_build_rays_test_params": 200,
}
NAME, SNAME = "ucnerf_build_rays_train", "ucnerf_build_rays_train_params"


def pixel_plan(H, W, ps, sel0, sel1, shift, ux, uy, coords):
    """include/ucnerf_hip.h, ucnerf_build_rays_train: the float pixels (row, col) [2,R] of the four segments, in the reference's order
    (utils/utils.py:179-199, :245-247, :304).  `clamped` counts the picks whose cell the clamp moved."""
    sel = np.concatenate([np.asarray(sel0, np.int64).reshape(-1), np.asarray(sel1, np.int64).reshape(-1)])
    shift = np.asarray(shift, np.int64).reshape(-1, 2)
    cell_r, cell_c = (sel // W) // ps, (sel % W) // ps
    clamped_r, clamped_c = np.clip(cell_r, 0, H // ps - 2), np.clip(cell_c, 0, W // ps - 2)
    e = np.arange(ps * ps)
    rows = (clamped_r * ps + shift[:, 0])[:, None] + (e // ps)[None, :]
    cols = (clamped_c * ps + shift[:, 1])[:, None] + (e % ps)[None, :]
    coords = np.asarray(coords, np.float32).reshape(-1, 2)
    pix = np.stack([np.concatenate([rows.reshape(-1).astype(np.float32), np.asarray(uy, np.float32).reshape(-1), coords[:, 0]]),
                    np.concatenate([cols.reshape(-1).astype(np.float32), np.asarray(ux, np.float32).reshape(-1), coords[:, 1]])])
    return pix, int((clamped_r != cell_r).sum() + (clamped_c != cell_c).sum())


def g18_draws(g):
    """G18's thirteen recorded draws as the kernel's inputs: (sel0, sel1, shift [P,2], ux, uy, t_rand)."""
    kinds = [str(k) for k in np.asarray(g["draw_kinds"]).tolist()]
    draws = [g["draw_%03d" % i] for i in range(int(g["n_draws"]))]
    assert kinds == ["multinomial"] + ["np_randint"] * 4 + ["multinomial"] + ["np_randint"] * 4 + ["randint", "randint", "rand"], kinds
    shift = torch.tensor([int(d) for d in draws[1:5] + draws[6:10]], dtype=torch.int32).reshape(-1, 2)
    return draws[0], draws[5], shift, draws[10], draws[11], draws[12]


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
    assert hasattr(raw, NAME), "library does not export " + NAME
    assert NAME in L.SYMBOLS and NAME + "(" in hdr
    assert "utils/utils.py:400-597" in hdr and ":169-215" in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION
    assert "#define UCNERF_ABI_VERSION 6" in hdr
    assert set(KNOWN_SIZES) == set(L.STRUCTS)
    for cname, size in KNOWN_SIZES.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == size == C.sizeof(L.STRUCTS[cname]), cname


def test_the_new_struct_is_registered_and_mirrored_field_for_field(L):
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    assert SNAME not in KNOWN_SIZES and SNAME not in L.STRUCTS and "struct %s {" % SNAME in hdr
    cls = L.ADDED_STRUCTS[SNAME]
    assert L.lib().ucnerf_sizeof(SNAME.encode()) == C.sizeof(cls) > 0
    body = re.sub(r"/\*.*?\*/", "", hdr.split("struct %s {" % SNAME)[1].split("};")[0], flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    declared = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const\s+)?(int32_t|int64_t|float)\s*(\*?)\s*(.+)$", decl.strip(), flags=re.S)
        if not m:
            assert not decl.strip(), decl
            continue
        for name in m.group(4).split(","):
            name, _, count = name.strip().partition("[")
            t = C.c_void_p if m.group(3) else ctype[m.group(2)]
            declared.append((name, t * int(count.rstrip("]")) if count else t))
    assert declared == list(cls._fields_), (declared, cls._fields_)


def test_argument_errors_are_einval_in_a_child_process(L):
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "build_rays_train_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 25 and not out["problems"], out["problems"]


def test_ops_wrapper_refuses_cpu_tensors():
    from uc_nerf_amd import ops
    g = load_golden("g18_build_rays")
    dvs = [g["stage%d_depth_values" % k] for k in (1, 2, 3)]
    with pytest.raises(RuntimeError, match="must live on a ROCm device"):
        ops.build_rays_train(g["imgs"], g["K"], g["c2ws"][0], g["w2cs"][0], g["K"], g["near_fars"][0], dvs, 12, 4, coords=g["coords"])


def test_the_restated_pixel_plan_reproduces_the_reference_fixture():
    g = load_golden("g18_build_rays")
    sel0, sel1, shift, ux, uy, t_rand = g18_draws(g)
    H, W, ps = int(g["H"]), int(g["W"]), int(g["patch_size"])
    assert 2 * sel0.numel() == int(g["patch_num"]) and ux.numel() == int(g["n_rays"]) - int(g["patch_num"]) * ps * ps
    pix, _ = pixel_plan(H, W, ps, sel0.numpy(), sel1.numpy(), shift.numpy(), ux.numpy(), uy.numpy(), g["coords"].numpy())
    assert pix.shape == tuple(g["pix"].shape) == (2, t_rand.shape[0])
    assert np.array_equal(pix.astype(np.int64), g["pix"].numpy())
    # every patch inside the image, as the clamp promises for shifts in [0, ps)
    n_patch = int(g["patch_num"]) * ps * ps
    assert pix[0, :n_patch].max() <= H - 1 and pix[1, :n_patch].max() <= W - 1 and pix[:, :n_patch].min() >= 0


def test_the_mirror_makes_the_reference_draws_in_order_and_hands_the_op_their_pixels(monkeypatch):
    """utils.build_rays on its one-launch route, the op replaced by a recorder (no device here): fed G18's draws through the primitives the reference
    uses -- one asked for out of order or with another shape fails --, it hands the op picks, shifts, uniform pixels and coordinates whose pixel plan is
    G18's."""
    import types
    from uc_nerf_amd import ops
    from uc_nerf_amd.utils import utils as U
    g = load_golden("g18_build_rays")
    kinds = [str(k) for k in np.asarray(g["draw_kinds"]).tolist()]
    draws = [g["draw_%03d" % i] for i in range(int(g["n_draws"]))]
    pos, seen = [0], {}

    def next_draw(kind, shape=None):
        i = pos[0]
        assert i < len(kinds) and kinds[i] == kind, "draw %d: the reference made a %s draw here, the mirror asks for %s" % (i, kinds[i] if i < len(kinds) else "no", kind)
        pos[0] += 1
        v = draws[i] if torch.is_tensor(draws[i]) else torch.as_tensor(np.asarray(draws[i]))
        assert shape is None or tuple(v.shape) == tuple(shape), "draw %d (%s): shape %s asked, the reference drew %s" % (i, kind, tuple(shape), tuple(v.shape))
        return v

    def recorder(imgs, K, c2w, w2c_ref, K_ref, near_far_ref, depth_values, S, ps, sel0, sel1, shift, ux, uy, coords, t_rand):
        seen.update(sel0=sel0, sel1=sel1, shift=shift, ux=ux, uy=uy, coords=coords, t_rand=t_rand, ps=ps, S=S)
        n = t_rand.shape[0]
        c = torch.zeros(n, S, 3)
        return dict(rays_o=torch.zeros(3), rays_d=torch.zeros(n, 3), colors=torch.zeros(n, 3), pix=torch.zeros(2, n, dtype=torch.int64), z=torch.zeros(n, S),
                    pts=c, stage1=c, stage2=c, stage3=c, ndc=c)

    monkeypatch.setattr(torch, "multinomial", lambda inp, n, *a, **k: next_draw("multinomial", (n,)))
    monkeypatch.setattr(np.random, "randint", lambda *a, **k: int(next_draw("np_randint")))
    monkeypatch.setattr(torch, "randint", lambda *a, **k: next_draw("randint", k.get("size", a[-1])))
    monkeypatch.setattr(torch, "rand", lambda *a, **k: next_draw("rand", a[0]))
    monkeypatch.setattr(ops, "build_rays_train", recorder)
    monkeypatch.setattr(U, "_fused_takes", lambda *a: True)                       # (the real one asks for device tensors)
    monkeypatch.setattr(U, "_BUILD_RAYS_FUSED", True)
    V, S = int(g["V"]), int(g["NS"])
    pose_ref = {"w2cs": g["w2cs"].clone(), "intrinsics": g["K"].repeat(V, 1, 1), "near_fars": g["near_fars"]}
    outputs = {k: {"depth_values": g[k + "_depth_values"]} for k in ("stage1", "stage2", "stage3")}
    args = types.SimpleNamespace(patch_num=int(g["patch_num"]), patch_size=int(g["patch_size"]))
    out = U.build_rays(args, g["imgs"], g["conf"], g["sparse"], g["coords"], pose_ref, g["w2cs"], g["c2ws"], g["K"].repeat(V, 1, 1), int(g["n_rays"]), S,
                       with_depth=True, outputs=outputs)
    monkeypatch.undo()
    assert pos[0] == len(kinds), "the mirror made %d of the reference's %d draws" % (pos[0], len(kinds))
    assert seen["sel0"].dtype == seen["sel1"].dtype == torch.int64 and seen["shift"].dtype == torch.int32 and tuple(seen["shift"].shape) == (args.patch_num, 2)
    pix, _ = pixel_plan(int(g["H"]), int(g["W"]), seen["ps"], seen["sel0"].numpy(), seen["sel1"].numpy(), seen["shift"].numpy(), seen["ux"].numpy(),
                        seen["uy"].numpy(), seen["coords"].numpy())
    assert np.array_equal(pix.astype(np.int64), g["pix"].numpy()) and torch.equal(seen["t_rand"], g["draw_012"])
    R = g["pix"].shape[1]
    assert len(out) == 9 and out[6] is None and tuple(out[5].shape) == (R, 3) and tuple(out[8].shape) == (2, R)
    assert out[7]["inv_scale"].tolist() == [int(g["W"]) - 1, int(g["H"]) - 1] and set(out[3]) == {"stage1", "stage2", "stage3", "ndc"}
