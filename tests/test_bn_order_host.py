"""Host-side checks of tests/bn_order_cases.py, the restatement the GPU file tests/test_hip_bn_order.py holds csrc/bn.hip to bit for bit.  No
GPU: the partition visits every value once and has the header's slice counts; every case reaches the regime its row claims (P from the
library's own ucnerf_bn_partials, pure host); the restatement's triples lie within a measured distance of exact ones; its float32 epilogue
agrees with the torch restatement of tests/bn_cases.py under the chain bar; and the cases tell the documented order from four others.
Run with -s for the regime table and the measured figures (profiles/bn_order.md)."""
import numpy as np
import pytest
import torch

import bn_cases as BC
import bn_order_cases as OC


@pytest.fixture(scope="module")
def lib():
    from uc_nerf_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_partition_visits_every_value_once_and_reaches_its_regime(lib, name):
    n, C, S, claims = OC.CASES[name]
    N = n * S
    P, L, counts = OC.slice_counts(N)
    assert lib.ucnerf_bn_partials(n, S) == P and L % 4 == 0 and (P - 1) * L < N <= P * L and sum(counts) == N and min(counts) > 0
    got = OC.regime(n, S)
    print("%-11s (%d, %d) C=%d: %s" % (name, n, S, C, " ".join("%s=%s" % kv for kv in got.items())))
    for k, v in claims.items():
        assert got[k] == v, (name, k, got[k], v)
    for trim in (False, True):
        idx, valid = OC.partition(N, trim)
        assert np.array_equal(np.bincount(idx[valid], minlength=N), np.ones(N, np.int64))            # every i exactly once
        assert valid.sum((1, 2, 3)).tolist() == counts
        assert all(idx[j][valid[j]].min() == j * L and idx[j][valid[j]].max() == j * L + counts[j] - 1 for j in range(P))
    idx, valid = OC.partition(N, trim=False)
    assert idx.shape == (P, got["chunks"], 1024, 16)
    # the regime, from the quad indices themselves: which u of chunk 0 hold a value, how many threads own a u = 1 quad, the second chunk
    quad_live = valid[0].reshape(-1, 1024, 4, 4).any(-1)                                               # [K, T, u] of slice 0
    assert [bool(quad_live[0, :, u].any()) for u in range(4)] == [u < got["live_u"] for u in range(4)]
    assert int(quad_live[0, :, 1].sum()) == got["threads_u1"] and int((~quad_live.any((0, 2))).sum()) == got["empty_threads"]
    assert int(quad_live[1:].sum()) == got["second_chunk_quads"]
    if got["second_chunk_quads"] == 1:
        assert bool(quad_live[1, 0, 0]) and bool(quad_live[0, 0].all())                                  # thread 0 merges it into a full first chunk
    last = valid[P - 1].reshape(-1, 4)
    assert int(last[last.any(-1)].sum(-1).min()) == got["last_quad"]                                  # the last slice's partial quad


def test_the_table_covers_the_regimes_the_issue_names():
    r = {name: OC.regime(n, S) for name, (n, C, S, _) in OC.CASES.items()}
    assert {v["N"] for v in r.values()} >= {2, 3, 5, 4095, 4096, 4097, 8194, 131072, 131073, 131076, 262144, 524288, 524289, 524292, 1048576}
    assert r["s131072"]["P"] == 32 and OC.partials(131071) == 32 and OC.partials(126976) == 31            # the first N of the cap with L = 4096
    assert any(v["chunks"] == 2 and v["vec"] for v in r.values()) and any(v["chunks"] == 2 and not v["vec"] for v in r.values())
    assert any(v["threads_u1"] == 1 and v["vec"] for v in r.values()) and any(v["threads_u1"] == 1 and not v["vec"] for v in r.values())
    assert OC.CASES["c65535"][1] == 65535 and max(c[0] * c[1] * c[2] for c in OC.CASES.values()) <= 1050000    # about 1 M floats at the most


@pytest.mark.parametrize("name", ("s5", "s4097", "ragged", "s131073", "s524292"))
def test_trimming_the_empty_waves_and_positions_changes_no_bit(name):
    y = OC.data(name)["y"][:, :2]
    assert np.array_equal(OC.bits(OC.stats(y, trim=True)), OC.bits(OC.stats(y, trim=False)))
    x = OC.channels(y)                                                       # and the restatement's slicing IS the partition's numbering
    idx, valid = OC.partition(x.shape[1], trim=False)
    v = OC.by_threads(x, x.shape[1])
    assert np.array_equal(v[:, valid], x[:, idx[valid]]) and not v[:, ~valid].any()


def test_restated_triples_against_exact_ones():
    worst_mean, worst_m2 = 0.0, 0.0
    for name in sorted(OC.CASES):
        y = OC.data(name)["y"][:, :3]
        ws = OC.stats(y)
        mean, m2 = OC.exact_triples(y)
        _, _, counts = OC.slice_counts(y.shape[0] * y.shape[2])
        assert np.array_equal(ws[:, :, 0], np.broadcast_to(np.array(counts, np.float64), ws.shape[:2]))
        e_mean, e_m2 = np.abs(ws[:, :, 1] - mean).astype(np.float64), np.abs(ws[:, :, 2] - m2).astype(np.float64)
        a_mean, a_m2 = np.abs(mean).astype(np.float64), np.abs(m2).astype(np.float64)
        rel_mean, rel_m2 = float((e_mean / np.maximum(a_mean, 1e-300)).max()), float((e_m2 / np.maximum(a_m2, 1e-300)).max())
        print("%-11s restatement against exact: mean %.3g, M2 %.3g (relative)" % (name, rel_mean, rel_m2))
        worst_mean, worst_m2 = max(worst_mean, rel_mean), max(worst_m2, rel_m2)
        assert bool((e_mean <= np.maximum(4 * OC.MEASURED_MEAN_REL * a_mean, OC.spacing64(a_mean.max()))).all()), name
        assert bool((e_m2 <= np.maximum(4 * OC.MEASURED_M2_REL * a_m2, OC.spacing64(a_m2.max()))).all()), name
    print("largest over the cases: mean %.3g, M2 %.3g; recorded %.3g, %.3g" % (worst_mean, worst_m2, OC.MEASURED_MEAN_REL, OC.MEASURED_M2_REL))


@pytest.mark.parametrize("name", ("s3", "s4097", "ragged", "n3_s43691", "s524292", "n3_s174763"))
def test_float32_epilogue_agrees_with_the_torch_restatement(name):
    d = OC.data(name)
    t = {k: torch.from_numpy(np.array(v)) for k, v in d.items()}
    count = d["y"].shape[0] * d["y"].shape[2]
    for relu in (True, False):
        for skip in (False, True):
            got = OC.restate(name, relu, skip)
            refs = []
            for dtype in (torch.float64, torch.float32):
                out, mean, var = BC.bn_train(t["y"], t["gamma"], t["beta"], dtype, relu=relu, skip=t["skip"] if skip else None, eps=OC.EPS)
                refs.append((mean, var) + BC.running_update(t["rm"], t["rv"], mean, var, count, dtype, momentum=OC.MOMENTUM) + (out,))
            for k, r64, r32 in zip(OC.NAMES[1:], *refs):
                bar, err32 = BC.chain_bar(r64, r32)
                err = float((torch.from_numpy(got[k]).double() - r64).abs().max())
                print("%s %s relu=%s skip=%s: restatement %.3g, float32 torch %.3g, bar %.3g" % (name, k, relu, skip, err, err32, bar))
                assert got[k].dtype == np.float32 and err <= bar, (name, k)


@pytest.mark.parametrize("order", ("waves_descending", "lane_scan", "chunk64", "chunk8"))
def test_the_cases_tell_the_documented_order_from_another(order):
    for name in OC.BIG:
        y = OC.data(name)["y"]
        want, other = OC.restate(name)["workspace"], OC.stats(y, order=order)
        assert np.array_equal(want[:, :, 0], other[:, :, 0])
        differ = OC.bits(want[:, :, 1:]) != OC.bits(other[:, :, 1:])
        close = np.abs(want - other) <= 1e-12 * np.abs(want)
        share = float(differ.any(-1).mean())
        print("%s against %s: %.3f of the triples differ in bits (mean %.3f, M2 %.3f)" % (name, order, share, differ[..., 0].mean(), differ[..., 1].mean()))
        assert bool(close.all())                                            # the same statistics all the same
        second = OC.regime(*OC.CASES[name][0:3:2])["second_chunk_quads"]
        if order == "chunk64" and second == 0:
            assert share == 0.0                                             # one chunk per thread: a chunk of 64 holds the same 16 values
        elif order == "chunk64" and second == 1:
            pass                                                            # 4 values of 16 388 in one thread: measured 0, printed above
        else:
            assert share >= 0.10, (name, order, share)
