"""The launch modes of ucnerf_mlp_fwd, ucnerf_mlp_fwd_train and ucnerf_mlp_bwd (csrc/mlp.hip, mlp_bf16.hip, mlp_bwd.hip, mlp_bwd_chain.hip,
mlp_wgrad.hip) on the cases of tests/mlp_modes_cases.py: every addressing mode of the params structs is the same function of the same inputs,
bit for bit; what lies in stride gaps, tile padding, the readable tails and the workspace never reaches a result; a sample's results do not
depend on its neighbours.  Driven through the C ABI (ctypes): the torch wrappers do not expose the strides.  profiles/mlp_modes.md has the case
table, the reasons each equality holds to the bit, and what reading the kernels changed:

* the forward computes its encodings with the hardware sine (sincos_rev, csrc/sincos_cw.h:65) and ucnerf_embed with the Cody-Waite path
  (sincos_pe, :40): the encoded mode is NOT the dense call's bits.  It is held to the float64 oracle under the bar of
  test_hip_parity.py::test_mlp_forward_vs_reference_golden (4 x the float32 oracle's own distance, floor 2e-6 of the scale), its backward under
  the bar of test_mlp_backward_vs_oracle_autograd; its poisoned runs are held to its own clean run bit for bit.
* the split precisions refuse encoded rows and strided raw coordinates (mlp_bf16_host.hip:181), the backward refuses strided raw coordinates
  (mlp_bwd.hip:691): there "strided" strides the features (and g_feats) only, and the one-matrix mode is the f32 forward's alone.
* saved_valid = 1 after an f32 ucnerf_mlp_fwd_train is the same kernel with the same arguments as the backward's own forward: bit-identical.
  After a bf16x3 training forward the kept activations are another forward's: that route is held to the oracle.

Parameter gradients are sums of float atomics.  ATOMIC[(case, bwd_mode)] is the largest distance between two of five repeated dense calls on
the parent commit, relative to max|g_flat|; every comparison of parameter gradients uses 4 x that."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_modes_cases as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F32 = np.float32
PRECISIONS = {"f32": ("f32", 0), "bf16x3": ("bf16x3", 0), "bf16": ("bf16", 0), "bf16x3_fp16": ("bf16x3", 1), "bf16_fp16": ("bf16", 1)}
POISON_IDS = tuple(M.POISONS)
ALONE = (0, 1, 30, 31, 32, 33, 64, 96)            # rows evaluated alone: first / last lane of a tile, the same lane in another tile, the ragged tail

# largest |g_flat(call i) - g_flat(call j)| / max|g_flat| over five repeated dense calls, measured on the parent commit.  Five calls see only some
# of the orders the atomics can land in (one process's five gave 9.3e-9 for m33 / bwd_mode 1, the next process's dense call differed from its own
# repeat by 7.5e-8), so the measurement was repeated: the figure is the largest five-call maximum of 21 rounds (profiles/mlp_modes.md has every
# round's).  0.0 on the parent: m1_v6 runs one block everywhere (one atomic per element); m31_v1 and m32_v8 in bwd_mode 1 ran TWO blocks of
# the head kernel, whose two atomics per element commute on a zeroed g_flat.  Since head_bwd_kernel sums its blocks' rows itself and hands every
# weight one atomic, these three entries describe the library as it is (every element of g_flat gets one atomic at m <= 32 in bwd_mode 1); the
# bwd_mode 1 entries of the larger cases are the parent's and now upper bounds (the head layers' share of the distance is gone, the gemm_tn
# launches' is unchanged); the bwd_mode 0 entries are unaffected (that mode never launches the head kernel).  "m97_v6[:33]" is the ghost-row
# test's own 33 samples.
ATOMIC = {("m1_v6", 0): 0.0, ("m1_v6", 1): 0.0, ("m31_v1", 0): 4.27e-09, ("m31_v1", 1): 0.0, ("m32_v8", 0): 9.37e-10, ("m32_v8", 1): 0.0,
          ("m33_S3_v6", 0): 4.66e-09, ("m33_S3_v6", 1): 7.46e-08, ("m65_v1", 0): 6.75e-09, ("m65_v1", 1): 7.19e-08, ("m96_S3_v8", 0): 9.86e-09,
          ("m96_S3_v8", 1): 1.05e-07, ("m97_v6", 0): 8.49e-09, ("m97_v6", 1): 1.36e-07, ("m97_v6[:33]", 0): 1.3e-09, ("m97_v6[:33]", 1): 4.15e-08}
PREFILL = F32(2.0 ** -6)                        # ACCUMULATES: small, so that the rounding of c + g stays that of g (an exact binary fraction)


def L():
    from uc_nerf_amd import _lib
    return _lib


def up(data, guard=True):
    """Device copy of a flat float32 array with M.GUARD floats of -7.0 behind it."""
    a = np.asarray(data, F32).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(M.GUARD if guard else 0, M.GUARD_VALUE, F32)])).to(DEV)


def down(t, count, what):
    a = t.cpu().numpy()
    assert (a[count:] == M.GUARD_VALUE).all() and a.size == count + M.GUARD, "the guard behind %s was written" % what
    return a[:count]


_weights = {}


def weights(name, prec="f32", pe_layout=0):
    """(cfg, packed stream, flat parameters on the device) of a case's state dict."""
    key = (name, prec, pe_layout)
    if key not in _weights:
        from uc_nerf_amd import ops
        c = M.case(name)
        flat = torch.from_numpy(c["flat"].copy()).to(DEV)
        pw = ops.PackedWeights(c["n_src"], pe_layout, DEV, *PRECISIONS[prec])
        _weights[key] = (pw.cfg, pw.pack(flat), flat)
    return _weights[key]


def bind(p, c, v, max_blocks=0):
    keep = {k: up(b.data) for k, b in v.bufs.items()}
    for which in ("pts", "dirs", "feats"):
        buf, off = getattr(v, which)
        setattr(p, which, keep[buf].data_ptr() + 4 * off)
    for k, val in v.fields.items():
        setattr(p, k, val)
    p.m, p.max_blocks = c["m"], max_blocks
    return keep


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    assert rc == 0, (what, rc, L().lib().ucnerf_last_error())


def forward(c, v, prec="f32", pe_layout=0, max_blocks=0):
    cfg, ws, _ = weights(c["name"], prec, pe_layout)
    p = L().MlpParams()
    p.cfg = cfg
    keep = bind(p, c, v, max_blocks)
    raw = up(np.full(c["m"] * 4, np.nan, F32))
    p.wstream, p.raw = ws.data_ptr(), raw.data_ptr()
    ok(L().lib().ucnerf_mlp_fwd(C.addressof(p), stream()), "ucnerf_mlp_fwd")
    torch.cuda.synchronize()
    del keep
    return down(raw, c["m"] * 4, "raw").reshape(c["m"], 4)


def backward(c, v, mode, g_stride=0, g_col0=0, sentinel=None, saved=None, max_blocks=0, ws_fill=None, prefill=0.0, pe_layout=0):
    """ucnerf_mlp_bwd on a View.  saved: None = the backward runs its own forward; "f32" / "bf16x3" = ucnerf_mlp_fwd_train in that precision
    first, then saved_valid = 1.  ws_fill: what the workspace holds before the first call (None: zeros).  -> g_feats [m,F], g_flat."""
    lib = L().lib()
    m, F = c["m"], c["F"]
    cfg, ws, flat = weights(c["name"], saved or "f32", pe_layout)
    bp = L().MlpBwdParams()
    bp.fwd.cfg = cfg
    keep = bind(bp.fwd, c, v, max_blocks)
    n_ws = lib.ucnerf_mlp_bwd_workspace_floats(C.addressof(cfg), m)
    assert n_ws > 0
    work = up(np.full(n_ws, 0.0 if ws_fill is None else ws_fill, F32))
    stride = g_stride or F
    gdata, gmask = M.g_feats_buffer(m, F, stride, g_col0, sentinel)
    g_feats, g_flat, g_raw = up(gdata), up(np.full(flat.numel(), prefill, F32)), up(c["g_raw"])
    no_raw = up(np.full(m * 4, M.GUARD_VALUE, F32))                      # "raw is not written"
    bp.fwd.wstream, bp.fwd.raw = ws.data_ptr(), no_raw.data_ptr()
    if saved:
        raw = up(np.full(m * 4, np.nan, F32))
        bp.fwd.raw = raw.data_ptr()
        ok(lib.ucnerf_mlp_fwd_train(C.addressof(bp.fwd), C.c_void_p(work.data_ptr()), mode, stream()), "ucnerf_mlp_fwd_train")
        bp.fwd.raw = no_raw.data_ptr()
    bp.g_raw, bp.flat_params, bp.g_feats, bp.g_feat_stride = g_raw.data_ptr(), flat.data_ptr(), g_feats.data_ptr() + 4 * g_col0, g_stride
    bp.g_flat, bp.workspace, bp.saved_valid, bp.bwd_mode = g_flat.data_ptr(), work.data_ptr(), int(bool(saved)), mode
    ok(lib.ucnerf_mlp_bwd(C.addressof(bp), stream()), "ucnerf_mlp_bwd")
    torch.cuda.synchronize()
    del keep
    down(work, n_ws, "the workspace")
    assert (down(no_raw, m * 4, "fwd.raw") == M.GUARD_VALUE).all(), "the backward wrote fwd.raw"
    out = {"g_flat": down(g_flat, flat.numel(), "g_flat")}
    g = down(g_feats, m * stride, "g_feats")
    assert (M.bits(g[gmask]) == M.bits(gdata[gmask])).all(), "columns of g_feats rows outside [0, F) were written"
    out["g_feats"] = g.reshape(m, stride)[:, g_col0:g_col0 + F]
    assert not np.isnan(out["g_feats"]).any(), "a column of g_feats was not written (or is NaN)"
    if saved:
        out["raw"] = down(raw, m * 4, "raw").reshape(m, 4)
    return out


def assert_bits(got, want, what):
    bad = M.bits(got) != M.bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), np.asarray(got)[bad][:4], np.asarray(want)[bad][:4])


def flat_distance(a, b):
    return float(np.abs(a.astype(np.float64) - b).max()) / max(float(np.abs(b).max()), 1e-30)


def check_flat(c, mode, got, want, what, problems):
    """Parameter gradients: finite, within 4 x the call-to-call distance of the dense call, the three unused sets exactly zero."""
    d = flat_distance(got, want) if np.isfinite(got).all() else float("inf")
    bar = 4 * ATOMIC[(c.get("bar_case", c["name"]), mode)]
    print("%s bwd_mode %d %s: g_flat distance %.3e of max|g_flat| (bar %.3e)" % (c["name"], mode, what, d, bar))
    if not d <= bar:
        problems.append((what, d))


def unused_are_zero(c, g_flat, fill=0.0):
    sl = M.param_slices(c)
    for k in M.UNUSED_PARAMS:
        for part in (".weight", ".bias"):
            assert (g_flat[sl[k + part]] == F32(fill)).all(), k + part


# ------------------------------------------------------------------------------------------------ forward
def forward_variants(c, prec, poison):
    f32 = prec == "f32"
    yield "dense", forward(c, M.dense(c, poison), prec)
    yield "dirs per sample", forward(c, M.dense(c, poison, per_sample=True), prec)
    yield "strided", forward(c, M.strided(c, poison, feats_only=not f32), prec)
    if f32:
        yield "one matrix", forward(c, M.one_matrix(c, poison), prec)
    yield "tiled", forward(c, M.tiled(c, poison), prec)
    yield "tiled, dirs per sample, max_blocks 3", forward(c, M.tiled(c, poison, per_sample=True), prec, max_blocks=3)
    for mb in (1, 3):
        yield "max_blocks %d" % mb, forward(c, M.dense(c, poison), prec, max_blocks=mb)
    yield "strided, max_blocks 1", forward(c, M.strided(c, poison, feats_only=not f32), prec, max_blocks=1)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", M.NAMES)
def test_forward_modes_are_the_same_function(name, prec):
    c = M.case(name)
    want = forward(c, M.dense(c), prec)
    assert np.isfinite(want).all()
    for what, raw in forward_variants(c, prec, None):
        assert_bits(raw, want, what)
    if prec == "f32":                                            # the reference the bit comparisons hang on is itself right
        o = M.oracle(name)
        scale = max(1.0, float(o["raw"].abs().max()))
        assert float(np.abs(want - o["raw"].numpy()).max()) <= max(4 * o["raw32_dist"], 2e-6 * scale)


@pytest.mark.parametrize("poison", POISON_IDS)
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", M.NAMES)
def test_forward_poison_does_not_leak(name, prec, poison):
    c = M.case(name)
    want = forward(c, M.dense(c), prec)
    for what, raw in forward_variants(c, prec, M.POISONS[poison]):
        assert_bits(raw, want, what + ", poisoned")


@pytest.mark.parametrize("pe_layout", (0, 1))
@pytest.mark.parametrize("name", M.NAMES)
def test_forward_encoded_rows_against_the_float64_oracle(name, pe_layout):
    c = M.case(name)
    o = M.oracle(name, "live" if pe_layout == 0 else "interleaved")
    want = forward(c, M.encoded(c, pe_layout), "f32", pe_layout)
    scale = max(1.0, float(o["raw"].abs().max()))
    err = float(np.abs(want - o["raw"].numpy()).max())
    print("%s layout %d: encoded forward %.3e from float64, the float32 oracle %.3e" % (name, pe_layout, err, o["raw32_dist"]))
    assert err <= max(4 * o["raw32_dist"], 2e-6 * scale)
    for poison in POISON_IDS:
        for mb in (0, 1):
            assert_bits(forward(c, M.encoded(c, pe_layout, M.POISONS[poison]), "f32", pe_layout, max_blocks=mb), want, (poison, mb))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", M.NAMES)
def test_forward_of_a_sample_does_not_depend_on_its_neighbours(name, prec):
    c = M.case(name)
    want = forward(c, M.dense(c), prec)
    perm = c["perm"]
    assert_bits(forward(M.subset(c, perm), M.dense(M.subset(c, perm)), prec)[M.inverse(perm)], want, "permuted")
    for i in ALONE:
        if i < c["m"]:
            one = M.subset(c, [i])
            assert_bits(forward(one, M.dense(one), prec)[0], want[i], "sample %d alone" % i)
            assert_bits(forward(one, M.tiled(one, M.POISONS["nan"]), prec)[0], want[i], "sample %d alone, tiled, 31 poisoned padding rows" % i)


# ------------------------------------------------------------------------------------------------ backward
def backward_variants(c, mode, poison):
    F = c["F"]
    fill = dict(ws_fill=poison, sentinel=poison)
    yield "dense", backward(c, M.dense(c, poison), mode, **fill)
    yield "dirs per sample", backward(c, M.dense(c, poison, per_sample=True), mode, **fill)
    yield "strided feats and g_feats", backward(c, M.strided(c, poison, feats_only=True), mode, g_stride=F + M.FEAT_PAD, **fill)
    yield "strided g_feats, columns 2 ..", backward(c, M.dense(c, poison), mode, g_stride=F + 5, g_col0=2, **fill)
    for mb in (1, 3):
        yield "max_blocks %d" % mb, backward(c, M.dense(c, poison), mode, max_blocks=mb, **fill)
    yield "saved_valid", backward(c, M.dense(c, poison), mode, saved="f32", **fill)
    yield "saved_valid, strided, max_blocks 1", backward(c, M.strided(c, poison, feats_only=True), mode, g_stride=F + M.FEAT_PAD, saved="f32", max_blocks=1, **fill)
    if mode == 0:                                                # (the layer-by-layer backward reads row-major features: mlp_bwd.hip:657)
        yield "tiled", backward(c, M.tiled(c, poison), mode, **fill)
        yield "tiled, dirs per sample, saved_valid", backward(c, M.tiled(c, poison, per_sample=True), mode, saved="f32", **fill)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", M.NAMES)
def test_backward_modes_are_the_same_function(name, mode):
    c, o = M.case(name), M.oracle(name)
    want = backward(c, M.dense(c), mode)
    oracle_grads_close(c, o, want)                               # the reference the comparisons hang on is itself right: g_feats AND g_flat
    unused_are_zero(c, want["g_flat"])
    outs = list(backward_variants(c, mode, None))
    for what, out in outs:
        assert_bits(out["g_feats"], want["g_feats"], what)
        unused_are_zero(c, out["g_flat"])
    problems = []
    for what, out in outs:
        check_flat(c, mode, out["g_flat"], want["g_flat"], what, problems)
    assert not problems, problems


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", M.NAMES)
def test_g_flat_accumulates(name, mode):
    """g_flat pre-filled with a constant c comes back as c + g within the atomic bar of the case.  Where that bar is 0 (m1_v6; m31_v1 and
    m32_v8 in bwd_mode 1) this is fl(c + g) to the bit, which holds only if every element receives ONE atomic: two partial sums commute on zeros
    but do not associate on c.  (It is why head_bwd_kernel sums its blocks' partial sums before it touches g_flat: profiles/mlp_modes.md.)"""
    c = M.case(name)
    want = backward(c, M.dense(c), mode)
    acc = backward(c, M.dense(c), mode, prefill=PREFILL)
    assert_bits(acc["g_feats"], want["g_feats"], "prefilled g_flat")
    unused_are_zero(c, acc["g_flat"], PREFILL)
    problems = []
    check_flat(c, mode, acc["g_flat"], PREFILL + want["g_flat"], "g_flat prefilled with c = 2^-6 against c + g", problems)
    assert not problems, problems


@pytest.mark.parametrize("poison", POISON_IDS)
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", M.NAMES)
def test_backward_poison_does_not_leak(name, mode, poison):
    c = M.case(name)
    want = backward(c, M.dense(c), mode)
    outs = list(backward_variants(c, mode, M.POISONS[poison]))
    for what, out in outs:
        assert_bits(out["g_feats"], want["g_feats"], what + ", poisoned")
        assert np.isfinite(out["g_flat"]).all(), what
        unused_are_zero(c, out["g_flat"])
    problems = []
    for what, out in outs:
        check_flat(c, mode, out["g_flat"], want["g_flat"], what + ", poisoned", problems)
    assert not problems, problems


def oracle_grads_close(c, o, out):
    gs = float(o["g_feats"].abs().max())
    torch.testing.assert_close(torch.from_numpy(out["g_feats"]).double(), o["g_feats"], atol=2e-4 * gs, rtol=2e-3)
    for k, s in M.param_slices(c).items():
        got, want = torch.from_numpy(out["g_flat"][s]).double(), o["g_params"][k]
        if want is None:
            assert torch.count_nonzero(got) == 0, k
        else:
            torch.testing.assert_close(got, want.reshape(-1), atol=2e-4 * float(want.abs().max()) + 1e-7, rtol=2e-3, msg=lambda s_: k + ": " + s_)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", M.NAMES)
def test_backward_encoded_rows_against_the_float64_oracle(name, mode):
    """g_feats lands in the feature columns of a [m, 63 + F + 27] gradient matrix (g_feat_stride = the row width); the encoding columns hold a
    sentinel that survives."""
    c = M.case(name)
    X = 63 + c["F"] + 27
    for pe_layout in (0, 1):
        o = M.oracle(name, "live" if pe_layout == 0 else "interleaved")
        want = backward(c, M.encoded(c, pe_layout), mode, g_stride=X, g_col0=63, pe_layout=pe_layout)
        oracle_grads_close(c, o, want)
        problems = []
        for poison in POISON_IDS:
            pv = M.POISONS[poison]
            for saved in (None, "f32"):
                out = backward(c, M.encoded(c, pe_layout, pv), mode, g_stride=X, g_col0=63, sentinel=pv, ws_fill=pv, saved=saved, pe_layout=pe_layout)
                assert_bits(out["g_feats"], want["g_feats"], (pe_layout, poison, saved))
                unused_are_zero(c, out["g_flat"])
                check_flat(c, mode, out["g_flat"], want["g_flat"], "encoded, layout %d, %s, saved %s" % (pe_layout, poison, saved), problems)
        assert not problems, problems


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", M.NAMES)
def test_backward_after_a_bf16x3_training_forward_against_the_float64_oracle(name, mode):
    """The activations a bf16x3 ucnerf_mlp_fwd_train keeps are that forward's, not the f32 forward's the backward would run itself: the two
    saved_valid routes are not one function.  Each is held to the oracle (the f32 route in test_backward_modes_are_the_same_function)."""
    c, o = M.case(name), M.oracle(name)
    want = backward(c, M.dense(c), mode, saved="bf16x3")
    oracle_grads_close(c, o, want)
    assert_bits(want["raw"], forward(c, M.dense(c), "bf16x3"), "the training forward's raw")
    views = [M.strided(c, M.POISONS["nan"], feats_only=True), M.dense(c, M.POISONS["inf"], per_sample=True)] + ([M.tiled(c, M.POISONS["3e38"])] if mode == 0 else [])
    for v in views:
        out = backward(c, v, mode, saved="bf16x3", ws_fill=M.POISONS["nan"])
        assert_bits(out["g_feats"], want["g_feats"], v.fields)
        assert_bits(out["raw"], want["raw"], v.fields)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", M.NAMES)
def test_feature_gradient_of_a_sample_does_not_depend_on_its_neighbours(name, mode):
    c = M.case(name)
    want = backward(c, M.dense(c), mode)["g_feats"]
    perm = c["perm"]
    p = M.subset(c, perm)
    assert_bits(backward(p, M.dense(p), mode)["g_feats"][M.inverse(perm)], want, "permuted")
    for i in ALONE:
        if i < c["m"]:
            one = M.subset(c, [i])
            assert_bits(backward(one, M.dense(one), mode)["g_feats"][0], want[i], "sample %d alone" % i)


@pytest.mark.parametrize("mode", (0, 1))
def test_ghost_rows_carry_no_weight(mode):
    """33 samples; the same 33 followed by 31 real samples whose g_raw rows are zero; the 33 with poisoned tile padding: one g_flat."""
    big = M.case("m97_v6")
    c = M.subset(big, np.arange(33))
    c["bar_case"] = "m97_v6[:33]"                                 # (the call-to-call distance of these very 33 samples)
    c64 = M.subset(big, np.arange(64))
    g = c64["g_raw"].copy()
    g[33:] = 0
    c64["g_raw"] = g
    want = backward(c, M.dense(c), mode)
    more = backward(c64, M.dense(c64), mode)
    assert_bits(more["g_feats"][:33], want["g_feats"], "33 of 64")
    assert (more["g_feats"][33:] == 0).all()
    problems = []
    check_flat(c, mode, more["g_flat"], want["g_flat"], "31 more samples with zero g_raw", problems)
    if mode == 0:
        for poison in POISON_IDS:
            out = backward(c, M.tiled(c, M.POISONS[poison]), mode, ws_fill=M.POISONS[poison])
            assert_bits(out["g_feats"], want["g_feats"], poison)
            check_flat(c, mode, out["g_flat"], want["g_flat"], "tile padding of " + poison, problems)
    else:
        for poison in POISON_IDS:                                 # (row-major features only: the poison sits in the stride gaps and the workspace)
            out = backward(c, M.strided(c, M.POISONS[poison], feats_only=True), mode, ws_fill=M.POISONS[poison])
            check_flat(c, mode, out["g_flat"], want["g_flat"], "stride gaps of " + poison, problems)
    assert not problems, problems


def test_what_the_entry_points_refuse():
    """The restrictions the module docstring relies on are the library's, not this file's."""
    lib = L().lib()
    c = M.case("m33_S3_v6")
    cfg, ws, flat = weights(c["name"], "bf16x3")
    p = L().MlpParams()
    p.cfg = cfg
    keep = bind(p, c, M.strided(c))
    raw = up(np.zeros(c["m"] * 4, F32))
    p.wstream, p.raw = ws.data_ptr(), raw.data_ptr()
    assert lib.ucnerf_mlp_fwd(C.addressof(p), stream()) != 0                       # strided raw coordinates in a split precision
    cfg, ws, flat = weights(c["name"], "f32")
    for mode in (0, 1):
        bp = L().MlpBwdParams()
        bp.fwd.cfg = cfg
        keep2 = bind(bp.fwd, c, M.strided(c))
        work = up(np.zeros(lib.ucnerf_mlp_bwd_workspace_floats(C.addressof(cfg), c["m"]), F32))
        g_feats, g_flat, g_raw = up(np.zeros(c["m"] * c["F"], F32)), up(np.zeros(flat.numel(), F32)), up(c["g_raw"])
        bp.fwd.wstream, bp.fwd.raw = ws.data_ptr(), raw.data_ptr()
        bp.g_raw, bp.flat_params, bp.g_feats, bp.g_flat, bp.workspace, bp.bwd_mode = (g_raw.data_ptr(), flat.data_ptr(), g_feats.data_ptr(), g_flat.data_ptr(),
                                                                                     work.data_ptr(), mode)
        assert lib.ucnerf_mlp_bwd(C.addressof(bp), stream()) != 0                   # strided raw coordinates in the backward
        if mode == 1:
            keep2 = bind(bp.fwd, c, M.tiled(c))
            assert lib.ucnerf_mlp_bwd(C.addressof(bp), stream()) != 0               # tile layout in the layer-by-layer backward
        torch.cuda.synchronize()
        assert (down(g_feats, c["m"] * c["F"], "g_feats") == 0).all() and (down(g_flat, flat.numel(), "g_flat") == 0).all()
    del keep, keep2
