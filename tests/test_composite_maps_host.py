"""Host-side checks of the gradient fold of the compositing's extra maps (ucnerf_composite_fold_grads).  No GPU: the algebra -- the float64
restatement of the fold followed by the oracle's backward through rgb / depth / acc / weights is the oracle's autograd through var, disp and
sum w u -- on every case, the recorded float32-oracle error bars against a fresh measurement, the new struct against the header and the
library, nothing of ABI v6 moved, and the entry point's argument checks (all made on the host before anything is launched)."""
import ctypes as C
import os
import re

import pytest
import torch

import composite_maps_cases as M
from test_composite_merged_host import KNOWN_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SNAME = "ucnerf_composite_fold_grads", "ucnerf_composite_fold_params"
FIELDS = ["n", "S", "weights", "depth", "acc", "u", "g_var", "g_disp", "g_wu", "g_depth", "g_acc", "g_weights", "g_depth_out", "g_acc_out",
          "g_weights_out", "g_u"]


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------ algebra
@pytest.mark.parametrize("S", M.S_VALUES)
def test_fold_then_the_existing_backward_is_autograd_through_every_map(S):
    """Relative to the largest gradient of the case: 1e-12 is four digits above float64's roundoff over 1024 samples and ten below any slip in
    a formula."""
    for n in M.N_VALUES:
        case, ref, _ = M.dense("maps_S%d_n%d" % (S, n))
        assert len(ref) == (4 if S >= 2 else 3)
        for combo, (want_raw, want_u) in ref.items():
            g_raw, g_u = M.folded_reference(case, M.F64, combo)
            d = M.distances(g_raw, g_u, want_raw, want_u)
            scale = max(1.0, float(want_raw.abs().max()), float(want_u.abs().max()))
            assert max(d.values()) <= 1e-12 * scale, (case["name"], combo, d)
            if "wu" not in combo:
                assert not bool(want_u.any()) and not bool(g_u.any())


def test_the_clamp_and_non_finite_rows_carry_no_disp_gradient():
    """fold64 against torch.maximum's autograd off the tie: depth / acc below the clamp, negative, 0 / 0 and x / 0 give no disp term."""
    depth = torch.tensor([0.0, 1e-11, -1.0, 0.0, 1.0, 2.0], dtype=M.F64)
    acc = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.5], dtype=M.F64)
    g = torch.tensor([3.0, -2.0, 5.0, 7.0, -1.0, 4.0], dtype=M.F64)
    gd, ga, _, _ = M.fold64(torch.zeros(6, 2, dtype=M.F64), depth, acc, g_disp=g)
    assert not bool(gd[:5].any()) and not bool(ga[:5].any())
    d, a = depth[5:].clone().requires_grad_(True), acc[5:].clone().requires_grad_(True)
    (g[5:] / torch.maximum(torch.full_like(d, 1e-10), d / a)).sum().backward()
    assert torch.allclose(gd[5:], d.grad, rtol=1e-14, atol=0) and torch.allclose(ga[5:], a.grad, rtol=1e-14, atol=0)
    live = depth[:3].clone().requires_grad_(True)                                # the oracle agrees on the clamped rows it can differentiate
    (g[:3] / torch.maximum(torch.full_like(live, 1e-10), live / acc[:3])).sum().backward()
    assert not bool(live.grad.any())


def test_the_recorded_bases_are_the_measurement():
    """The float32 oracle's distance depends on the CPU it runs on (torch sums and multiplies a row in vector-width pieces: the machine with the
    device measured 1.9e-06 where the constant says 8.1e-06): the constants are the measurement on the machine they were taken on, another
    machine must not need more than a quarter above them (the float32 oracle stays inside its own bar with room) nor show them inflated by
    more than an order of magnitude."""
    got = M.measured_base()
    for combo, names in M.BASE.items():
        for k, const in names.items():
            print("%s %s: measured %.3e, recorded %.3e, bar %.3e" % (combo, k, got[combo][k], const, M.FACTOR * const))
            assert const / 10.0 <= got[combo][k] <= 1.25 * const, (combo, k, got[combo][k], const)
    assert M.FACTOR == 4.0


def test_no_ray_of_a_disp_case_is_nearly_empty_and_the_case_list_is_the_issue_s():
    assert M.S_VALUES == (1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 257, 513, 1024) and M.N_VALUES == (1, 5, 67)
    assert len(M.dense_names()) == 39
    kinds = {(na == 0, nb == 0, na == 1 and nb > 0, (na, nb) == (128, 64)) for na, nb in M.merged_specs()}
    assert len(kinds) >= 4
    for name in M.dense_names():
        case, _, _ = M.dense(name)                                              # (dense() asserts acc > ACC_MIN in float64 ...)
        acc32 = M.oracle_maps(case["raw"], case["z"], case["u"], False)["acc"]      # ... and here in float32
        assert float(acc32.min()) > M.ACC_MIN == 1e-3, name


def test_one_hot_expectation_matches_float64_where_it_is_representable():
    """expected_fold_one_hot, the operation-by-operation float32 expectation of the device test's exact cases, against fold64: g_u to the bit,
    the var term within two float32 roundings (1 / S and 1 / (S - 1) are not representable in general; the device test asks for the bits)."""
    for S in M.EXACT_S:
        w = torch.eye(S)[: min(S, 5)]
        u = torch.arange(1.0, S + 1).expand_as(w) % 5 + 1
        gv, gu = torch.tensor([1.0, -2.0, 3.0, 4.0, -1.0])[: w.shape[0]], torch.tensor([2.0, 1.0, -3.0, 1.0, 2.0])[: w.shape[0]]
        g, g_u = M.expected_fold_one_hot(w, u, gv, gu)
        _, _, g64, g_u64 = M.fold64(w.double(), torch.ones(w.shape[0]).double(), torch.ones(w.shape[0]).double(), u.double(), g_var=gv.double(),
                                    g_wu=gu.double())
        assert torch.equal(g_u.double(), g_u64)
        assert bool(((g.double() - g64).abs() <= 2.0 ** -22 * g64.abs().clamp(min=1.0)).all()), S


# ------------------------------------------------------------------------------------------------ ABI
def test_the_entry_point_is_exported_and_nothing_of_the_abi_moved(L):
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    assert hasattr(raw, NAME), "library does not export " + NAME
    assert NAME in L.SYMBOLS and "int %s(const %s* p, void* stream);" % (NAME, SNAME) in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    for cname, size in KNOWN_SIZES.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == size == C.sizeof(L.STRUCTS[cname]), cname
    assert set(L.STRUCTS) == set(KNOWN_SIZES)
    for cname, cls in L.ADDED_STRUCTS.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == C.sizeof(cls) > 0, cname
    assert L.lib().ucnerf_sizeof(b"ucnerf_composite_merged_params") == 4 * 4 + 12 * 8
    assert L.lib().ucnerf_sizeof(b"ucnerf_composite_merged_bwd_params") == 4 * 4 + 10 * 8
    assert L.lib().ucnerf_sizeof(b"ucnerf_composite_bwd_params") == C.sizeof(L.CompositeBwdParams)
    # the new struct: declared last in the header with a tag, registered with ucnerf_sizeof(), mirrored field for field at the same offsets
    assert SNAME not in KNOWN_SIZES and "struct %s {" % SNAME in hdr
    assert hdr.index("struct %s {" % SNAME) > max(hdr.index(s) for s in ("ucnerf_render_fused_bwd(", "struct ucnerf_composite_merged_bwd_params {"))
    cls = L.ADDED_STRUCTS[SNAME]
    assert L.lib().ucnerf_sizeof(SNAME.encode()) == C.sizeof(cls) == 2 * 4 + 14 * 8
    body = re.sub(r"/\*.*?\*/", "", hdr.split("struct %s {" % SNAME)[1].split("};")[0], flags=re.S)
    declared, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(float|int32_t)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        for n in m.group(3).split(","):
            size = 8 if m.group(2) else 4
            off = (off + size - 1) // size * size
            declared.append((n.strip(), bool(m.group(2)), off))
            off += size
    mirrored = [(f[0], f[1] is L.vp, getattr(cls, f[0]).offset) for f in cls._fields_]
    assert declared == mirrored, (declared, mirrored)
    assert [d[0] for d in declared] == FIELDS


def _params(L, n, S, **ptrs):
    """A parameter block over made-up, well separated addresses (never dereferenced: every check below fails, or n is 0, before a launch)."""
    p = L.CompositeFoldParams()
    p.n, p.S = n, S
    base = 0x10000000
    for i, f in enumerate(FIELDS[2:]):
        setattr(p, f, base * (i + 1))
    for k, v in ptrs.items():
        setattr(p, k, v)
    return p


def test_argument_errors_are_einval_before_anything_is_launched(L):
    lib = L.lib()
    call = lambda p: lib.ucnerf_composite_fold_grads(C.addressof(p), None)      # noqa: E731
    EINVAL = -1
    assert call(_params(L, 0, 5)) == 0                                           # an empty batch: success, nothing read, nothing launched
    assert call(_params(L, 0, 5, weights=None, g_depth_out=None)) == 0
    assert call(_params(L, -1, 5)) == EINVAL and b"negative" in lib.ucnerf_last_error()
    assert lib.ucnerf_composite_fold_grads(None, None) == EINVAL
    for S in (0, -3, 1025):
        assert call(_params(L, 4, S)) == EINVAL, S
    assert call(_params(L, 4, 1)) == EINVAL and b"g_var" in lib.ucnerf_last_error()      # the variance of one weight
    assert call(_params(L, 4, 8, u=None)) == EINVAL and b"g_wu" in lib.ucnerf_last_error()
    for required in ("weights", "depth", "acc", "g_depth_out", "g_acc_out", "g_weights_out"):
        assert call(_params(L, 4, 8, **{required: None})) == EINVAL, required
    base = _params(L, 4, 8)
    inputs, outputs = FIELDS[2:12], FIELDS[12:]
    for o in outputs:                                                            # an output on an input, exactly and by one float inside
        for i in inputs:
            assert call(_params(L, 4, 8, **{o: getattr(base, i)})) == EINVAL, (o, i)
            assert call(_params(L, 4, 8, **{o: getattr(base, i) + 4})) == EINVAL, (o, i)
            assert b"overlap" in lib.ucnerf_last_error()
    for a in range(4):                                                           # two outputs on each other
        for b in range(a + 1, 4):
            assert call(_params(L, 4, 8, **{outputs[a]: getattr(base, outputs[b])})) == EINVAL, (a, b)


def test_ops_wrappers_refuse_cpu_tensors():
    from uc_nerf_amd import ops
    from uc_nerf_amd.network import renderer
    raw, z = torch.rand(2, 5, 4), torch.rand(2, 5)
    rank = torch.arange(5, dtype=torch.int32).repeat(2, 1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.composite_fold_grads(z, z[:, 0], z[:, 0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.composite_maps(raw, z)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.composite_merged_maps(raw[:, :3], raw[:, 3:], rank, z)
    with pytest.raises(RuntimeError, match="ROCm device"):
        renderer.raw2outputs_maps(raw, z, None)
