"""ucnerf_composite_merged_bwd (composite_merged_bwd_kernel<E>, E in {1, 2, 3, 4, 8, 16}) and ops.composite_merged on the device.

Identity:      g_raw_a / g_raw_b == ucnerf_merge_rows -> ucnerf_composite_bwd -> un-merge, bit for bit (signs of zeros, NaN positions), for every
               lane split, every way of handing the rows out, every set of upstream gradients, both backgrounds;
exact:         the one-hit merged cases of tests/composite_cases.py through its closed-form gradients, un-merged;
differential:  the continuous cases against the float64 restatement (tests/composite_merged_bwd_cases.py) under composite_cases' bars;
second call:   into the same buffers, NaN-filled first: the same bits (every row written once, nothing accumulated);
autograd:      ops.composite_merged hands the four gradients over in order, matches float64 autograd, takes None for any of them."""
import pytest
import torch

import composite_cases as CC
import composite_merged_bwd_cases as MB
from test_hip_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 5                                                 # a full block of four rays and a partial one


def dev(t):
    return t.to(DEV)


def same(got, want, what):
    """Equal bit patterns but for NaN payloads, compared on the device: NaNs in the same places (composite_cases.same_or_both_nan) and, since ==
    does not see the sign of a zero, equal sign bits wherever neither is NaN."""
    want = want.to(got.device).float().reshape(got.shape)
    nan = (got != got) & (want != want)
    ok = ((got == want) & (torch.signbit(got) == torch.signbit(want))) | nan
    if not bool(ok.all()):
        assert not CC.same_or_both_nan(got, want) or bool((torch.signbit(got) != torch.signbit(want)).any())
        bad = (~ok).nonzero()
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, reference %r"
                             % (what, len(bad), got.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))


def three_steps(a, b, rank, z, white, grads):
    """The contract on the device: merge_rows -> composite_bwd -> un-merge through rank."""
    from uc_nerf_amd import ops
    g = ops.composite_bwd(ops.merge_rows(a, b, rank), z, white_bkgd=white, **grads)
    g_cat = torch.gather(g, 1, rank.long()[..., None].expand(g.shape))
    na = a.shape[1]
    return g_cat[:, :na], g_cat[:, na:]


def identity_inputs(S):
    """N rays of merged rows with what the arithmetic can trip over: densities 0.0, -0.0, 200 (exp(-s) = 0: products of 0 and huge quotients),
    -3 (alpha < 0), colours with both signs and zeros, one NaN density and one NaN colour (S >= 3), random depths and upstream gradients."""
    gen = torch.Generator().manual_seed(77 + S)
    raw = torch.cat([3.0 * torch.rand(N, S, 3, generator=gen) - 1.0, 2.0 * torch.rand(N, S, 1, generator=gen)], -1)
    pick = torch.rand(N, S, generator=gen)
    raw[..., 3][pick < 0.10] = 0.0
    raw[..., 3][(pick >= 0.10) & (pick < 0.20)] = -0.0
    raw[..., 3][(pick >= 0.20) & (pick < 0.25)] = 200.0
    raw[..., 3][(pick >= 0.25) & (pick < 0.30)] = -3.0
    raw[..., 0][pick > 0.9] = 0.0
    raw[..., 1][pick > 0.95] = -0.0
    raw[0, :, 3] = 0.0                                  # an empty ray
    if S >= 3:
        raw[3, S // 2, 3] = float("nan")
        raw[4, S - 1, 1] = float("nan")
    z = torch.sort(1.0 + 3.0 * torch.rand(N, S, generator=gen), -1)[0]
    g = dict(g_rgb=torch.randn(N, 3, generator=gen), g_depth=torch.randn(N, generator=gen), g_acc=torch.randn(N, generator=gen),
             g_weights=torch.randn(N, S, generator=gen))
    g["g_weights"][1, ::3] = 0.0
    return dev(raw), dev(z), {k: dev(v) for k, v in g.items()}


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("S", MB.IDENTITY_S)
def test_equals_merge_rows_then_composite_bwd_then_unmerge_bit_for_bit(S):
    from uc_nerf_amd import ops
    raw, z, g = identity_inputs(S)
    calls = 0
    for na in MB.na_values(S):
        for kind in CC.RANK_KINDS:
            rank = dev(MB.make_rank(N, S, na, kind, seed=1))
            cat = torch.gather(raw, 1, rank[..., None].expand(N, S, 4))
            a, b, rank = cat[:, :na].contiguous(), cat[:, na:].contiguous(), rank.int()
            for white in (False, True):
                for combo in CC.COMBOS:
                    grads = {t: (g[t] if t in combo else None) for t in CC.TARGETS}
                    want_a, want_b = three_steps(a, b, rank, z, white, grads)
                    got_a, got_b = ops.composite_merged_bwd(a, b, rank, z, white_bkgd=white, **grads)
                    what = "S=%d na=%d %s white=%s %s" % (S, na, kind, white, "+".join(combo))
                    assert tuple(got_a.shape) == (N, na, 4) and tuple(got_b.shape) == (N, S - na, 4), what
                    same(got_a, want_a, what + " g_raw_a")
                    same(got_b, want_b, what + " g_raw_b")
                    calls += 1
    assert calls == len(MB.na_values(S)) * len(CC.RANK_KINDS) * 2 * len(CC.COMBOS)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("S", CC.MERGED_S)
def test_one_hit_merged_cases_are_exact(S):
    from uc_nerf_amd import ops
    case, _ = CC.exact("hit_S%d_last" % S)
    want = {}
    for white in (False, True):
        for combo in CC.COMBOS:
            g, mask, _ = CC.expected_g_raw(case, white, combo)
            assert bool(mask.all())                      # (the builder declares every entry exact)
            want[white, combo] = dev(g)
    ups = {t: dev(case[t]) for t in CC.TARGETS}
    seen = 0
    for s, na, kind in CC.merged_specs():
        if s != S:
            continue
        m, _ = CC.merged_case(S, na, kind)
        a, b, rank, z = dev(m["raw_a"]), dev(m["raw_b"]), dev(m["rank"]), dev(m["z"])
        idx = rank.long()[..., None].expand(m["n"], S, 4)
        for white in (False, True):
            for combo in CC.COMBOS:
                got_a, got_b = ops.composite_merged_bwd(a, b, rank, z, white_bkgd=white, **{t: (ups[t] if t in combo else None) for t in CC.TARGETS})
                w_cat = torch.gather(want[white, combo], 1, idx)
                what = "%s white=%s %s" % (m["name"], white, "+".join(combo))
                same(got_a, w_cat[:, :na], what + " g_raw_a")
                same(got_b, w_cat[:, na:], what + " g_raw_b")
        seen += 1
    assert seen >= 10


# ------------------------------------------------------------------------------------------------ differential
@pytest.mark.parametrize("name,na,kind", MB.CONT_SPLITS)
def test_continuous_cases_within_the_bars_of_composite_cases(name, na, kind):
    from uc_nerf_amd import ops
    m, ref = MB.continuous_split(name, na, kind)
    a, b, rank, z = dev(m["raw_a"]), dev(m["raw_b"]), dev(m["rank"]), dev(m["z"])
    bars, report, fails = CC.bars(), {}, []
    for white in (False, True):
        for combo in CC.COMBOS:
            got_a, got_b = ops.composite_merged_bwd(a, b, rank, z, white_bkgd=white, **{t: (dev(m[t]) if t in combo else None) for t in CC.TARGETS})
            assert bool(torch.isfinite(got_a).all()) and bool(torch.isfinite(got_b).all()), (name, white, combo)
            d = MB.distances(got_a.cpu(), got_b.cpu(), *ref[white, combo])
            what = "bwd white=%s %s" % (white, "+".join(combo))
            print("%s %s: g_colour %.3e (bar %.3e)  g_density %.3e (bar %.3e)" % (m["name"], what, d["g_colour"], bars["g_colour"], d["g_density"],
                                                                                   bars["g_density"]))
            report[what] = {k: dict(device=v, bar=bars[k]) for k, v in d.items()}
            fails.extend(CC.over_the_bar(d, "%s %s" % (m["name"], what)))
    record("composite_merged_bwd/" + m["name"], **report)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ nothing accumulated, every row written
@pytest.mark.parametrize("name,na,kind", [("hit_S65_last", 21, "random"), ("cont_S257", 100, "interleaved")])
def test_second_call_into_the_same_dirty_buffers_gives_the_same_bits(name, na, kind):
    from uc_nerf_amd import ops
    case = CC.exact(name)[0] if name in CC.EXACT_NAMES else CC.continuous(name)[0]
    m = MB.split(case, na, kind, rays=torch.arange(min(N, case["n"])))
    a, b, rank, z = dev(m["raw_a"]), dev(m["raw_b"]), dev(m["rank"]), dev(m["z"])
    g = {t: dev(m[t]) for t in CC.TARGETS}
    fresh = ops.composite_merged_bwd(a, b, rank, z, white_bkgd=True, **g)
    assert bool(torch.isfinite(fresh[0]).all()) and bool(torch.isfinite(fresh[1]).all())
    out = (torch.full_like(a, float("nan")), torch.full_like(b, float("nan")))
    for call in range(2):
        got = ops.composite_merged_bwd(a, b, rank, z, white_bkgd=True, out=out, **g)
        assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
        same(out[0], fresh[0], "%s g_raw_a, call %d into the caller's buffers" % (m["name"], call))
        same(out[1], fresh[1], "%s g_raw_b, call %d into the caller's buffers" % (m["name"], call))


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_hands_the_four_gradients_over_in_order():
    """ops.composite_merged: a loss through rgb, depth, acc and weights together, on an exact case -- a swapped pair would miss by integers."""
    from uc_nerf_amd import ops
    case, _ = CC.exact("hit_S65_last")
    m = MB.split(case, 21, "random", rays=torch.arange(N))
    a, b = dev(m["raw_a"]).requires_grad_(True), dev(m["raw_b"]).requires_grad_(True)
    rgb, depth, acc, weights, disp, var = ops.composite_merged(a, b, dev(m["rank"]), dev(m["z"]), True)
    assert not disp.requires_grad and not var.requires_grad
    ((rgb * dev(m["g_rgb"])).sum() + (depth * dev(m["g_depth"])).sum() + (acc * dev(m["g_acc"])).sum() + (weights * dev(m["g_weights"])).sum()).backward()
    sub = {k: (v[:N] if torch.is_tensor(v) and v.shape[:1] == (case["n"],) else v) for k, v in case.items()}
    sub["n"] = N
    want, _, _ = CC.expected_g_raw(sub, True, CC.TARGETS)
    wa, wb = MB.unmerge(want, m["rank"], 21)
    same(a.grad, wa, "g_raw_a through autograd")
    same(b.grad, wb, "g_raw_b through autograd")
    # the forward is composite_merged_fwd's
    fwd = ops.composite_merged_fwd(a.detach(), b.detach(), dev(m["rank"]), dev(m["z"]), True)
    for k, v in dict(rgb=rgb, depth=depth, acc=acc, weights=weights, disp=disp, var=var).items():
        same(v.detach(), fwd[k], "forward " + k)


@pytest.mark.parametrize("na,nb", [(3, 2), (64, 193)])
def test_autograd_matches_float64_autograd_and_accepts_none(na, nb):
    from uc_nerf_amd import ops
    S = na + nb
    gen = torch.Generator().manual_seed(S)
    raw = torch.cat([3.0 * torch.rand(N, S, 3, generator=gen) - 1.0, 0.05 + 2.0 * torch.rand(N, S, 1, generator=gen)], -1)
    case = dict(name="auto_S%d" % S, S=S, n=N, raw=raw, z=torch.sort(1.0 + 3.0 * torch.rand(N, S, generator=gen), -1)[0],
                g_rgb=torch.randn(N, 3, generator=gen), g_depth=torch.randn(N, generator=gen), g_acc=torch.randn(N, generator=gen),
                g_weights=torch.randn(N, S, generator=gen))
    m = MB.split(case, na, "random")
    bars = CC.bars()
    seen_none = []
    for white in (False, True):
        for combo in CC.COMBOS:
            a, b = dev(m["raw_a"]).requires_grad_(True), dev(m["raw_b"]).requires_grad_(True)
            rgb, depth, acc, weights, _, _ = ops.composite_merged(a, b, dev(m["rank"]), dev(m["z"]), white)
            outs = dict(g_rgb=rgb, g_depth=depth, g_acc=acc, g_weights=weights)
            sum((outs[t] * dev(m[t])).sum() for t in combo).backward()            # the outputs outside `combo` reach backward() as None
            seen_none.append(len(CC.TARGETS) - len(combo))
            ra, rb = MB.autograd_through_the_merge(m, white, combo)
            d = MB.distances(a.grad.cpu(), b.grad.cpu(), ra, rb)
            print("S=%d white=%s %s: %s" % (S, white, "+".join(combo), d))
            assert not CC.over_the_bar(d, "S=%d white=%s %s" % (S, white, "+".join(combo))), (d, bars)
    assert max(seen_none) == 3
    # None straight into the wrapper, all four: the gradient of a constant
    za, zb = ops.composite_merged_bwd(dev(m["raw_a"]), dev(m["raw_b"]), dev(m["rank"]), dev(m["z"]))
    assert not bool(za.any()) and not bool(zb.any())
