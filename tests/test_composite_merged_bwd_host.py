"""Host-side checks of the merged compositing backward (ucnerf_composite_merged_bwd).  No GPU: the library exports it with nothing of ABI v6 moved,
the binding mirrors its struct field for field, the entry point validates its arguments before anything is launched, and the CPU restatement of
its contract (tests/composite_merged_bwd_cases.py) is what torch autograd gives through the merged forward."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import composite_cases as CC
import composite_merged_bwd_cases as MB
from test_composite_merged_host import KNOWN_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SNAME = "ucnerf_composite_merged_bwd", "ucnerf_composite_merged_bwd_params"


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
    assert NAME in L.SYMBOLS and "int %s(const %s* p, void* stream);" % (NAME, SNAME) in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION
    assert "#define UCNERF_ABI_VERSION 6" in hdr
    for cname, size in KNOWN_SIZES.items():
        assert L.lib().ucnerf_sizeof(cname.encode()) == size == C.sizeof(L.STRUCTS[cname]), cname
    assert set(L.STRUCTS) == set(KNOWN_SIZES)                        # the v6 table itself is as it was
    for cname, cls in L.ADDED_STRUCTS.items():                       # (the earlier additions are still there)
        assert L.lib().ucnerf_sizeof(cname.encode()) == C.sizeof(cls) > 0, cname
    assert L.lib().ucnerf_sizeof(b"ucnerf_composite_merged_params") == 4 * 4 + 12 * 8      # the forward's struct did not change
    assert {"ucnerf_merge_rows", "ucnerf_composite_bwd", "ucnerf_composite_merged_fwd"} <= set(L.SYMBOLS)
    # the new struct: declared in the header, registered with ucnerf_sizeof() under its own name, mirrored field for field at the same offsets
    assert SNAME not in KNOWN_SIZES and "struct %s {" % SNAME in hdr
    cls = L.ADDED_STRUCTS[SNAME]
    assert L.lib().ucnerf_sizeof(SNAME.encode()) == C.sizeof(cls) == 4 * 4 + 10 * 8
    body = hdr.split("struct %s {" % SNAME)[1].split("};")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared, off = [], 0                                            # (name, is a pointer, offset under the C layout rules)
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
    assert [d[0] for d in declared] == ["n", "na", "nb", "white_bkgd", "raw_a", "raw_b", "rank", "z", "g_rgb", "g_depth", "g_acc", "g_weights",
                                        "g_raw_a", "g_raw_b"]


def test_argument_errors_are_einval_in_a_child_process(L):
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "composite_merged_bwd_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 30 and not out["problems"], out["problems"]


def test_ops_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from uc_nerf_amd import ops
    a, b, z = torch.rand(2, 3, 4), torch.rand(2, 2, 4), torch.rand(2, 5)
    rank = torch.arange(5, dtype=torch.int32).repeat(2, 1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.composite_merged_bwd(a, b, rank, z)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.composite_merged(a, b, rank, z)


@pytest.mark.parametrize("kind", CC.RANK_KINDS)
def test_ranks_are_permutations_and_unmerge_inverts_merge(kind):
    for S in (1, 2, 5, 64, 193):
        for na in MB.na_values(S):
            rank = MB.make_rank(3, S, na, kind)
            rows = torch.arange(3 * S * 4, dtype=torch.float32).view(3, S, 4)
            a, b = MB.unmerge(rows, rank, na)
            assert tuple(a.shape) == (3, na, 4) and tuple(b.shape) == (3, S - na, 4)
            assert torch.equal(MB.merge(a, b, rank), rows)


@pytest.mark.parametrize("name,na,kind", MB.CONT_SPLITS)
def test_the_restatement_is_autograd_through_the_merged_forward(name, na, kind):
    """merge -> composite_cases.backward -> un-merge against torch autograd with raw_a and raw_b as the leaves, both in float64: the same
    derivative by two routes (torch's scatter backward is the un-merge's gather), equal but for nothing -- and the float32 restatement sits inside
    composite_cases' bars, which are 4 x its own kind of error."""
    m, ref = MB.continuous_split(name, na, kind)
    bars = CC.bars()
    for white in (False, True):
        for combo in CC.COMBOS:
            ra, rb = MB.restated(m, torch.float64, white, combo)
            assert torch.equal(ra, ref[white, combo][0]) and torch.equal(rb, ref[white, combo][1])      # (composite_cases' own targets, un-merged)
            ga, gb = MB.autograd_through_the_merge(m, white, combo)
            assert tuple(ga.shape) == (m["n"], na, 4) and tuple(gb.shape) == (m["n"], m["S"] - na, 4)
            scale = max(1.0, float(ra.abs().max()) if ra.numel() else 0.0, float(rb.abs().max()) if rb.numel() else 0.0)
            for got, want in ((ga, ra), (gb, rb)):
                assert float((got - want).abs().max()) <= 1e-12 * scale if want.numel() else True, (name, white, combo)
            fa, fb = MB.restated(m, torch.float32, white, combo)
            d = MB.distances(fa, fb, ra, rb)
            assert d["g_colour"] <= bars["g_colour"] and d["g_density"] <= bars["g_density"], (name, white, combo, d)


def test_the_exact_cases_split_too():
    """The one-hit cases of composite_cases go through expected_g_raw un-merged: the restatement in float32 gives those bits on the CPU."""
    for name, na, kind in (("hit_S65_last", 21, "random"), ("hit_S3_adjacent", 1, "reversed"), ("n5_S65", 64, "interleaved")):
        case, _ = CC.exact(name)
        m = MB.split(case, na, kind)
        for white in (False, True):
            for combo in CC.COMBOS:
                want, mask, _ = CC.expected_g_raw(case, white, combo)
                assert bool(mask.all())
                wa, wb = MB.unmerge(want, m["rank"], na)
                fa, fb = MB.restated(m, torch.float32, white, combo)
                assert CC.same_or_both_nan(fa, wa) and CC.same_or_both_nan(fb, wb), (name, white, combo)
