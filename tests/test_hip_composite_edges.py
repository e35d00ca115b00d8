"""The compositing kernels against the oracle on the cases of tests/composite_cases.py: bit for bit on the exact ("one-hit") cases -- an opaque
sample on every position of every lane split, both sides of every split boundary, a ragged last block, empty rays (disp NaN) -- and under bars
derived from the float32 oracle's own distance to the float64 one on the continuous cases.

Forward:  composite_fwd_kernel<E, 0> (ops.composite_fwd: u / wu, var on and off, both backgrounds), composite_fwd_kernel<E, 1> (rays_d, noise),
          composite_merged_fwd_kernel<E> (ops.composite_merged_fwd), E in {1, 2, 3, 4, 8, 16}.
Backward: composite_bwd_kernel<E> (ops.composite_bwd with each of g_rgb, g_depth, g_acc, g_weights alone and all four, both backgrounds;
          once through ops.composite's autograd)."""
import pytest
import torch

import composite_cases as CC
from test_hip_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(t):
    return t.to(DEV)


def same(got, want, what):
    """torch.equal with NaNs required in the same places."""
    got, want = got.cpu(), want.float().reshape(got.shape)
    gn, wn = got != got, want != want
    ok = (got == want) | (gn & wn)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, reference %r"
                             % (what, len(bad), got.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))


def var_under_the_bar(out, want, what):
    if "var64" in want:
        d = (out["var"].cpu().double() - want["var64"]).abs().max().item()
        print("%s var: %.3e (bar %.3e)" % (what, d, CC.bars()["var"]))
        assert d <= CC.bars()["var"], "%s var: %.3e > bar %.3e" % (what, d, CC.bars()["var"])
    else:
        assert "var" not in out


# ------------------------------------------------------------------------------------------------ exact, forward
@pytest.mark.parametrize("name", CC.LIVE_EXACT_NAMES)
def test_live_forward_is_exact(name):
    from uc_nerf_amd import ops
    case, want = CC.exact(name)
    raw, z, u = dev(case["raw"]), dev(case["z"]), dev(case["u"])
    for white in (False, True):
        out = ops.composite_fwd(raw, z, 0, white, u=u)
        for k in CC.FWD_NAMES:
            same(out[k], want[white][k], "%s white=%s %s" % (name, white, k))
        var_under_the_bar(out, want[white], "%s white=%s" % (name, white))
        out = ops.composite_fwd(raw, z, 0, white, want_var=False)
        assert "var" not in out and "wu" not in out
        for k in ("rgb", "depth", "acc", "disp", "weights"):
            same(out[k], want[white][k], "%s white=%s %s without var" % (name, white, k))


@pytest.mark.parametrize("name", CC.HELPERS_EXACT_NAMES)
def test_helpers_forward_is_exact(name):
    from uc_nerf_amd import ops
    case, want = CC.exact(name)
    raw, z, u = dev(case["raw"]), dev(case["z"]), dev(case["u"])
    for white in (False, True):
        out = ops.composite_fwd(raw, z, 1, white, rays_d=dev(case["rays_d"]), noise=dev(case["noise"]), u=u)
        assert "var" not in out
        for k in CC.FWD_NAMES:
            same(out[k], want[white][k], "%s white=%s %s" % (name, white, k))


@pytest.mark.parametrize("S", CC.MERGED_S)
def test_merged_forward_is_exact(S):
    from uc_nerf_amd import ops
    for s, na, kind in CC.merged_specs():
        if s != S:
            continue
        m, want = CC.merged_case(S, na, kind)
        for white in (False, True):
            out = ops.composite_merged_fwd(dev(m["raw_a"]), dev(m["raw_b"]), dev(m["rank"]), dev(m["z"]), white, u=dev(m["u"]))
            for k in CC.FWD_NAMES:
                same(out[k], want[white][k], "%s white=%s %s" % (m["name"], white, k))
            var_under_the_bar(out, want[white], "%s white=%s" % (m["name"], white))
        out = ops.composite_merged_fwd(dev(m["raw_a"]), dev(m["raw_b"]), dev(m["rank"]), dev(m["z"]), True, want_var=False)
        assert "var" not in out
        same(out["weights"], want[True]["weights"], m["name"] + " weights without var")


# ------------------------------------------------------------------------------------------------ exact, backward
def _grads(case, combo):
    return {t: (dev(case[t]) if t in combo else None) for t in CC.TARGETS}


def _exact_backward(case, g_raw, white, combo, what):
    want, mask, _ = CC.expected_g_raw(case, white, combo)
    assert bool(mask.all())                          # (the builder declares every entry exact)
    same(g_raw, want, what)


@pytest.mark.parametrize("name", CC.LIVE_EXACT_NAMES)
def test_backward_is_exact(name):
    from uc_nerf_amd import ops
    case, _ = CC.exact(name)
    raw, z = dev(case["raw"]), dev(case["z"])
    for white in (False, True):
        for combo in CC.COMBOS:
            g = ops.composite_bwd(raw, z, white_bkgd=white, **_grads(case, combo))
            _exact_backward(case, g, white, combo, "%s white=%s %s" % (name, white, "+".join(combo)))


@pytest.mark.parametrize("name,white", [("hit_S65_one", True), ("hit_S257_last", False)])
def test_autograd_hands_the_four_gradients_over_in_order(name, white):
    """ops.composite: a loss through rgb, depth, acc and weights together (_Composite.backward's argument order)."""
    from uc_nerf_amd import ops
    case, _ = CC.exact(name)
    raw = dev(case["raw"]).requires_grad_(True)
    rgb, depth, acc, weights, _, _ = ops.composite(raw, dev(case["z"]), white)
    g = _grads(case, CC.TARGETS)
    ((rgb * g["g_rgb"]).sum() + (depth * g["g_depth"]).sum() + (acc * g["g_acc"]).sum() + (weights * g["g_weights"]).sum()).backward()
    _exact_backward(case, raw.grad, white, CC.TARGETS, name + " through autograd")


# ------------------------------------------------------------------------------------------------ continuous
@pytest.mark.parametrize("name", CC.CONT_NAMES)
def test_continuous_case_within_four_times_the_float32_oracle(name):
    from uc_nerf_amd import ops
    case, ref, dist, gref, gdist = CC.continuous(name)
    raw, z, u = dev(case["raw"]), dev(case["z"]), dev(case["u"])
    bars, report, fails = CC.bars(), {}, []

    def held(d, oracle_d, what):
        report[what] = {k: dict(device=v, oracle_f32=oracle_d[k], bar=bars[k]) for k, v in d.items()}
        fails.extend(CC.over_the_bar(d, "%s %s" % (name, what)))

    for white in (False, True):
        if case["variant"] == 0:
            out = ops.composite_fwd(raw, z, 0, white, u=u)
        else:
            out = ops.composite_fwd(raw, z, 1, white, rays_d=dev(case["rays_d"]), noise=dev(case["noise"]), u=u)
        out = {k: v.cpu() for k, v in out.items()}
        assert set(out) == set(ref[white])
        same(out["disp"] != out["disp"], (ref[white]["disp"] != ref[white]["disp"]), name + " NaN positions of disp")
        held(CC.fwd_distances(out, ref[white]), dist[white], "fwd white=%s" % white)
        for combo in (CC.COMBOS if case["variant"] == 0 else ()):
            g = ops.composite_bwd(raw, z, white_bkgd=white, **_grads(case, combo)).cpu()
            assert bool(torch.isfinite(g).all()), (name, white, combo)
            held(CC.bwd_distances(g, gref[white, combo]), gdist[white, combo], "bwd white=%s %s" % (white, "+".join(combo)))
    record("composite_edges/" + name, **report)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ no state, nothing accumulated
@pytest.mark.parametrize("name", ("hit_S65_last", "cont_S257"))
def test_second_call_into_the_same_buffers_gives_the_same(name):
    from uc_nerf_amd import _lib as L, ops
    case = CC.exact(name)[0] if name in CC.EXACT_NAMES else CC.continuous(name)[0]
    n, S = case["n"], case["S"]
    raw, z, u = dev(case["raw"]), dev(case["z"]), dev(case["u"])
    out = {k: torch.full(s, 7.0, device=DEV) for k, s in dict(rgb=(n, 3), depth=(n,), acc=(n,), disp=(n,), weights=(n, S), var=(n,), wu=(n,)).items()}

    def fill(p):
        p.rgb_map, p.depth_map, p.acc_map, p.disp_map = (out[k].data_ptr() for k in ("rgb", "depth", "acc", "disp"))
        p.weights, p.var, p.u, p.wu, p.z = out["weights"].data_ptr(), out["var"].data_ptr(), u.data_ptr(), out["wu"].data_ptr(), z.data_ptr()

    p = L.CompositeParams()
    p.n, p.S, p.variant, p.white_bkgd, p.raw = n, S, 0, 1, raw.data_ptr()
    fill(p)
    ops._launch("ucnerf_composite_fwd", p, raw.device)
    first = {k: v.clone() for k, v in out.items()}
    fresh = ops.composite_fwd(raw, z, 0, True, u=u)
    for k, v in first.items():
        same(v, fresh[k].cpu(), "%s %s: caller's buffers against fresh ones" % (name, k))
    ops._launch("ucnerf_composite_fwd", p, raw.device)
    for k, v in first.items():
        same(out[k], v.cpu(), "%s %s after a second forward" % (name, k))
    # the merged launch into the same buffers: rows split in the middle, identity rank
    na = S // 2
    a, b = raw[:, :na].contiguous(), raw[:, na:].contiguous()
    rank = torch.arange(S, dtype=torch.int32, device=DEV).expand(n, S).contiguous()
    m = L.CompositeMergedParams()
    m.n, m.na, m.nb, m.white_bkgd, m.raw_a, m.raw_b, m.rank = n, na, S - na, 1, a.data_ptr(), b.data_ptr(), rank.data_ptr()
    fill(m)
    for _ in range(2):
        for v in out.values():
            v.add_(1.0)                               # (stale values of another call in every output)
        ops._launch("ucnerf_composite_merged_fwd", m, raw.device)
        for k, v in first.items():
            same(out[k], v.cpu(), "%s %s from the merged launch" % (name, k))
    # backward: g_raw written, not accumulated
    g = _grads(case, CC.TARGETS)
    bp = L.CompositeBwdParams()
    bp.fwd.n, bp.fwd.S, bp.fwd.variant, bp.fwd.white_bkgd, bp.fwd.raw, bp.fwd.z = n, S, 0, 1, raw.data_ptr(), z.data_ptr()
    bp.g_rgb, bp.g_depth, bp.g_acc, bp.g_weights = (g[t].data_ptr() for t in CC.TARGETS)
    g_raw = torch.full((n, S, 4), 7.0, device=DEV)
    bp.g_raw = g_raw.data_ptr()
    ops._launch("ucnerf_composite_bwd", bp, raw.device)
    once = g_raw.clone()
    same(once, ops.composite_bwd(raw, z, white_bkgd=True, **g).cpu(), name + " g_raw: caller's buffer against a fresh one")
    ops._launch("ucnerf_composite_bwd", bp, raw.device)
    same(g_raw, once.cpu(), name + " g_raw after a second backward")
