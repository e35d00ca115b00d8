"""CPU-side checks of tests/mlp_modes_cases.py, the case builder behind tests/test_hip_mlp_modes.py: its views of one case are the same data,
its poison sits only where intended, the oracle has the per-sample independence the permutation tests assume of the kernels, every case
keeps its relu arguments away from zero, and the ctypes mirrors the device test fills match the library."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_modes_cases as M
from oracle import ucnerf_oracle as O

F32 = np.float32
POISON_IDS = tuple(M.POISONS)


def is_poison(data, poison):
    return M.bits(data) == M.bits(np.array([poison], F32))[0]


def views(c, poison):
    out = {"dense": M.dense(c, poison), "dense_per_sample": M.dense(c, poison, per_sample=True), "strided": M.strided(c, poison),
           "strided_feats": M.strided(c, poison, feats_only=True), "one_matrix": M.one_matrix(c, poison), "encoded0": M.encoded(c, 0, poison),
           "encoded1": M.encoded(c, 1, poison), "tiled": M.tiled(c, poison), "tiled_per_sample": M.tiled(c, poison, per_sample=True)}
    return out


@pytest.mark.parametrize("name", M.NAMES)
def test_every_mode_holds_the_dense_arrays_bit_for_bit(name):
    c = M.case(name)
    m, F, S = c["m"], c["F"], c["S"]
    for mode, v in views(c, M.POISONS["nan"]).items():
        f = v.fields
        n_dirs = m if f["dirs_per_sample"] else m // S
        want_dirs = c["dirs_ps"] if f["dirs_per_sample"] else c["dirs"]
        if f["encoded"]:
            e_pts, e_dir = M.encodings(name, int(mode[-1]))
            assert M.same_bits(M.read_rows(v, "pts", m, 63), e_pts) and M.same_bits(M.read_rows(v, "dirs", m, 27), e_dir), mode
            assert M.same_bits(e_pts[:, :3], c["pts"]) and M.same_bits(e_dir[:, :3], c["dirs_ps"])
        else:
            assert M.same_bits(M.read_rows(v, "pts", m, 3), c["pts"]), mode
            assert M.same_bits(M.read_rows(v, "dirs", n_dirs, 3), want_dirs), mode
        if f["feats_tiled"]:
            assert M.same_bits(M.untile(v.bufs["feats"].data, m, F), c["feats"]), mode
        else:
            assert M.same_bits(M.read_rows(v, "feats", m, F), c["feats"]), mode
    # the directions per sample are the per-ray ones repeated, the permutation and its inverse undo each other
    assert M.same_bits(c["dirs_ps"].reshape(m // S, S, 3), np.broadcast_to(c["dirs"][:, None], (m // S, S, 3)))
    perm = c["perm"]
    p = M.subset(c, perm)
    inv = M.inverse(perm)
    assert sorted(perm.tolist()) == list(range(m)) and (m < 3 or (perm != np.arange(m)).any())
    for k in ("pts", "dirs_ps", "feats", "g_raw"):
        assert M.same_bits(p[k][inv], c[k]), k
    assert c["feats"][:, -1].min() >= 0 and c["feats"][:, -1].max() <= 1


@pytest.mark.parametrize("poison", POISON_IDS)
@pytest.mark.parametrize("name", M.NAMES)
def test_poison_sits_exactly_in_the_gaps_the_padding_and_the_tails(name, poison):
    c = M.case(name)
    m, F, S = c["m"], c["F"], c["S"]
    pv = M.POISONS[poison]
    mt = (m + 31) // 32 * 32
    want = {"dense": 3 * M.TAIL, "dense_per_sample": 3 * M.TAIL,
            "strided": 4 * m + 2 * (m // S) + 3 * m + 3 * M.TAIL, "strided_feats": 3 * m + 3 * M.TAIL, "one_matrix": M.TAIL, "encoded0": M.TAIL,
            "encoded1": M.TAIL, "tiled": (mt - m) * F + 3 * M.TAIL, "tiled_per_sample": (mt - m) * F + 3 * M.TAIL}
    clean = views(c, None)
    for mode, v in views(c, pv).items():
        assert v.expect == want[mode] == v.poisoned(), (mode, v.expect, want[mode], v.poisoned())
        for k, b in v.bufs.items():
            hit = is_poison(b.data, pv)
            assert (hit == b.mask).all(), (mode, k)                                   # the poison, all of it, and nowhere else
            assert np.isfinite(b.data[~b.mask]).all() and (np.abs(b.data[~b.mask]) < 1e30).all()
            assert M.same_bits(b.data[~b.mask], clean[mode].bufs[k].data[~b.mask]) and (clean[mode].bufs[k].data[b.mask] == 0).all()
    data, mask = M.g_feats_buffer(m, F, F + M.FEAT_PAD, 0, pv)
    assert int(mask.sum()) == M.FEAT_PAD * m and int(np.isnan(data).sum()) == m * F + (M.FEAT_PAD * m if poison == "nan" else 0)
    data, mask = M.g_feats_buffer(m, F, 63 + F + 27, 63, pv)
    assert int(mask.sum()) == 90 * m and (is_poison(data, pv) >= mask).all()


@pytest.mark.parametrize("name", M.NAMES)
def test_float64_oracle_treats_every_sample_on_its_own(name):
    """raw and d(sum raw * g_raw)/d feats of a sample do not depend on the other samples of the batch: permuting the batch permutes them, and a
    sample evaluated alone gives its row.  The bar is float64 rounding only -- a BLAS may sum a row in another order for another batch shape:
    1e-12 of the largest value, five orders above eps * (191 terms), eight below anything a dependence between samples would show."""
    c, want = M.case(name), M.oracle(name)
    m, F, n_src = c["m"], c["F"], c["n_src"]
    sd = {k: v.double() for k, v in c["sd"].items()}

    def run(d):
        t = lambda a: torch.from_numpy(np.array(a)).double()
        fo = t(d["feats"]).requires_grad_(True)
        raw = O.run_network_mvs(sd, t(d["pts"])[:, None], t(d["dirs_ps"]), fo[:, None], n_src=n_src)[:, 0]
        (raw * t(d["g_raw"])).sum().backward()
        return raw.detach(), fo.grad

    bar_raw, bar_g = 1e-12 * max(1.0, float(want["raw"].abs().max())), 1e-12 * max(1.0, float(want["g_feats"].abs().max()))
    raw, g = run(c)
    assert float((raw - want["raw"]).abs().max()) <= bar_raw and float((g - want["g_feats"]).abs().max()) <= bar_g       # (per-sample dirs == per-ray dirs)
    inv = torch.from_numpy(M.inverse(c["perm"]))
    raw_p, g_p = run(M.subset(c, c["perm"]))
    assert float((raw_p[inv] - raw).abs().max()) <= bar_raw and float((g_p[inv] - g).abs().max()) <= bar_g
    for i in sorted({0, m // 2, m - 1}):
        raw_1, g_1 = run(M.subset(c, [i]))
        assert float((raw_1[0] - raw[i]).abs().max()) <= bar_raw and float((g_1[0] - g[i]).abs().max()) <= bar_g, i


@pytest.mark.parametrize("name", M.NAMES)
def test_every_relu_argument_of_every_sample_keeps_its_margin(name):
    """No excluded samples: all m of every case.  The restatement that exposes the relu arguments is the oracle itself, to the bit."""
    c = M.case(name)
    m, S, F = c["m"], c["S"], c["F"]
    t = lambda a: torch.from_numpy(np.array(a))
    raw, pre = M.forward_with_pre(c["sd"], t(c["pts"]), t(c["dirs_ps"]), t(c["feats"]), c["n_src"])
    want = O.run_network_mvs(c["sd"], t(c["pts"])[:, None], t(c["dirs_ps"]), t(c["feats"])[:, None], n_src=c["n_src"])[:, 0]
    assert torch.equal(raw, want)
    assert pre.shape == (m, sum(M.RELU_LAYERS)) and bool(torch.isfinite(pre).all())
    ratio = M.margin_ratio(pre)
    assert ratio.shape == (m,) and float(ratio.min()) >= M.RELU_MARGIN, (name, float(ratio.min()))
    assert M.relu_margin(c) == float(ratio.min())


def test_struct_mirrors_match_the_library():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib as L
    lib = L.lib()
    assert lib.ucnerf_sizeof(b"ucnerf_mlp_params") == C.sizeof(L.MlpParams)
    assert lib.ucnerf_sizeof(b"ucnerf_mlp_bwd_params") == C.sizeof(L.MlpBwdParams)
    assert lib.ucnerf_sizeof(b"ucnerf_mlp_config") == C.sizeof(L.MlpConfig) == 16
    # every field the device test sets exists under the header's name
    for f in ("m", "S", "dirs_per_sample", "feats_tiled", "max_blocks", "encoded", "pts_stride", "dirs_stride", "feat_stride", "pts", "dirs", "feats",
              "wstream", "raw"):
        assert hasattr(L.MlpParams, f), f
    for f in ("fwd", "g_raw", "flat_params", "g_feats", "g_feat_stride", "g_flat", "workspace", "saved_valid", "bwd_mode"):
        assert hasattr(L.MlpBwdParams, f), f
    for n_src in (1, 6, 8):
        cfg = L.MlpConfig(n_src, 0, 0, 0)
        assert lib.ucnerf_mlp_param_count(C.addressof(cfg)) == M.case({1: "m31_v1", 6: "m1_v6", 8: "m32_v8"}[n_src])["flat"].size
