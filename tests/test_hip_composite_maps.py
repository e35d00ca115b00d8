"""ucnerf_composite_fold_grads (composite_fold_kernel<E>, E in {1, 2, 3, 4, 8, 16}), ops.composite_maps / ops.composite_merged_maps and
CoarseFineRenderer.render_train(maps=True) on the device.

exact:         one-hit rays (tests/composite_cases.py): one-hot weights make d var / d w, g_u and, with power-of-two depth and acc, the folded
               g_depth / g_acc exactly representable -- bit equality; rows under the clamp of disp carry exactly nothing;
differential:  g_raw (g_raw_a / g_raw_b) and g_u through the autograd functions against the oracle's float64 autograd through every map, every
               element compared, bars of tests/composite_maps_cases.py (4 x the float32 oracle's own distance, measured on the CPU);
equivalences:  without a gradient on an extra map the bits of ops.composite / ops.composite_merged; merged == dense on merge_rows, bit for
               bit, with such gradients; a second call into the same dirty buffers gives the same bits;
errors:        UCNERF_EINVAL for g_var at S = 1, g_wu without u, aliased outputs; n = 0 succeeds;
render_train:  a loss on var alone trains the network (against the float64 oracle pipeline); maps=False is the parent's render_train;
no sync:       one forward and backward under torch's sync debug mode "error"."""
import functools

import pytest
import torch

import composite_cases as CC
import composite_maps_cases as M
import composite_merged_bwd_cases as MB
from test_hip_composite_merged_bwd import same
from test_hip_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(t):
    return t.to(DEV)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("S", M.EXACT_S)
def test_one_hit_rays_fold_to_the_bit(S):
    """The "one" hit sweep at S (ray r opaque at sample r): the device's own forward gives one-hot weights (asserted), and the fold's var and wu
    terms are then one float32 result per operation, whatever the reduction order -- with no upstream g_weights and with one."""
    from uc_nerf_amd import ops
    case, _ = CC.exact("hit_S%d_one" % S)
    n = case["n"]
    fwd = ops.composite_fwd(dev(case["raw"]), dev(case["z"]), u=dev(case["u"]))
    assert torch.equal(fwd["weights"].cpu(), torch.eye(S))
    gen = torch.Generator().manual_seed(S)
    g_var = torch.randint(-4, 5, (n,), generator=gen).float()
    g_wu = torch.randint(-4, 5, (n,), generator=gen).float()
    for g_weights in (None, case["g_weights"]):
        want_w, want_u = M.expected_fold_one_hot(torch.eye(S), case["u"], g_var, g_wu, g_weights)
        gd, ga, gw, gu = ops.composite_fold_grads(fwd["weights"], fwd["depth"], fwd["acc"], dev(case["u"]), g_var=dev(g_var), g_wu=dev(g_wu),
                                                  g_weights=None if g_weights is None else dev(g_weights))
        same(gw, want_w, "S=%d g_weights'" % S)
        same(gu, want_u, "S=%d g_u" % S)
        assert not bool(gd.any()) and not bool(ga.any())                       # no disp gradient, no upstream: zeros, written
    # var alone and wu alone: the other term adds nothing, not even a rounding
    z1 = torch.zeros(n)
    _, _, gw, gu = ops.composite_fold_grads(fwd["weights"], fwd["depth"], fwd["acc"], dev(case["u"]), g_var=dev(g_var))
    same(gw, M.expected_fold_one_hot(torch.eye(S), case["u"], g_var, z1)[0], "S=%d var alone" % S)
    assert not bool(gu.any())
    _, _, gw, gu = ops.composite_fold_grads(fwd["weights"], fwd["depth"], fwd["acc"], dev(case["u"]), g_wu=dev(g_wu))
    same(gw, g_wu[:, None] * case["u"], "S=%d wu alone" % S)
    same(gu, g_wu[:, None] * torch.eye(S), "S=%d g_u, wu alone" % S)


def test_power_of_two_depth_and_acc_fold_exactly_and_clamped_rows_carry_nothing():
    from uc_nerf_amd import ops
    n, S = 11, 3
    depth = torch.tensor([1.0, 2.0, 0.5, 8.0, 0.25, 4.0, 0.0, 1e-11, -1.0, 0.0, 1.0])
    acc = torch.tensor([1.0, 0.5, 0.5, 0.25, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0])      # rows 6..10: depth / acc 0, below 1e-10, negative, NaN, inf
    g_disp = torch.tensor([3.0, -2.0, 5.0, 1.0, -7.0, 6.0, 3.0, -2.0, 5.0, 7.0, -1.0])
    g_depth, g_acc = torch.arange(1.0, n + 1), -torch.arange(1.0, n + 1)
    w = torch.full((n, S), 0.25)
    live = torch.arange(n) < 6
    disp = (acc / depth).double()
    t_d = torch.where(live, -(disp * disp / acc.double()) * g_disp.double(), torch.zeros(n).double())
    t_a = torch.where(live, (disp * disp * depth.double() / (acc.double() * acc.double())) * g_disp.double(), torch.zeros(n).double())
    assert torch.equal(t_d.float().double(), t_d) and torch.equal(t_a.float().double(), t_a)      # representable: nothing to round
    for ups in ((None, None), (g_depth, g_acc)):
        want_d = t_d.float() + (ups[0] if ups[0] is not None else 0.0)
        want_a = t_a.float() + (ups[1] if ups[1] is not None else 0.0)
        assert torch.equal(want_d.double(), t_d + (ups[0].double() if ups[0] is not None else 0.0))      # (small integers and dyadic terms: exact)
        gd, ga, gw, gu = ops.composite_fold_grads(dev(w), dev(depth), dev(acc), g_disp=dev(g_disp), g_depth=None if ups[0] is None else dev(ups[0]),
                                                  g_acc=None if ups[1] is None else dev(ups[1]))
        same(gd, want_d, "g_depth'")
        same(ga, want_a, "g_acc'")
        assert gu is None and not bool(gw.any())
        if ups[0] is not None:                                                   # under the clamp: the upstream gradient, untouched
            assert torch.equal(gd.cpu()[6:], g_depth[6:]) and torch.equal(ga.cpu()[6:], g_acc[6:])
        else:
            assert not bool(gd[6:].any()) and not bool(ga[6:].any())


# ------------------------------------------------------------------------------------------------ differential
def _device_grads(case, combo, merged=None):
    """(g_raw or (g_raw_a, g_raw_b), g_u, outputs) of the loss `combo` through ops.composite_maps / ops.composite_merged_maps."""
    from uc_nerf_amd import ops
    u = dev(case["u"]).requires_grad_(True)
    if merged is None:
        raw = dev(case["raw"]).requires_grad_(True)
        outs = ops.composite_maps(raw, dev(case["z"]), case["white"], u)
        leaves = raw
    else:
        a, b = dev(merged["raw_a"]).requires_grad_(True), dev(merged["raw_b"]).requires_grad_(True)
        outs = ops.composite_merged_maps(a, b, dev(merged["rank"]), dev(merged["z"]), case["white"], u)
        leaves = (a, b)
    assert len(outs) == 7
    named = dict(zip(("rgb", "depth", "acc", "weights", "disp", "var", "wu"), outs))
    sum((named[m] * dev(case["g_" + m])).sum() for m in combo).backward()
    g_u = torch.zeros_like(u) if u.grad is None else u.grad
    return leaves, g_u, named


@pytest.mark.parametrize("S", M.S_VALUES)
def test_dense_gradients_match_float64_autograd_through_every_map(S):
    fails, report = [], {}
    for n in M.N_VALUES:
        case, ref, _ = M.dense("maps_S%d_n%d" % (S, n))
        for combo in M.combos_of(S):
            raw, g_u, named = _device_grads(case, combo)
            assert named["var"].requires_grad == (S >= 2) and named["disp"].requires_grad and named["wu"].requires_grad
            assert raw.grad is not None and bool(torch.isfinite(raw.grad).all()) and bool(torch.isfinite(g_u).all())
            d = M.distances(raw.grad.cpu(), g_u.cpu(), *ref[combo])
            what = "%s %s" % (case["name"], M.combo_name(combo))
            print(what, " ".join("%s %.3e (bar %.3e)" % (k, v, M.bar(combo, k)) for k, v in d.items()))
            report[what] = {k: dict(device=v, bar=M.bar(combo, k)) for k, v in d.items()}
            fails.extend(M.over_the_bar(d, combo, what))
            if ("wu",) == combo:
                assert int(torch.count_nonzero(raw.grad[..., 3])) > 0 and int(torch.count_nonzero(g_u)) > 0
    record("composite_maps/S%d" % S, **report)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("na,nb", M.merged_specs())
def test_merged_gradients_match_float64_autograd_through_every_map(na, nb):
    m, case, ref, _ = M.merged(na, nb)
    fails, report = [], {}
    for combo in M.combos_of(na + nb):
        (a, b), g_u, _ = _device_grads(case, combo, m)
        g_a = a.grad if a.grad is not None else torch.zeros_like(a)              # (a side without rows)
        g_b = b.grad if b.grad is not None else torch.zeros_like(b)
        d = MB.distances(g_a.cpu(), g_b.cpu(), ref[combo][0], ref[combo][1])
        d["g_u"] = (g_u.cpu().double() - ref[combo][2]).abs().max().item()
        what = "%s %s" % (case["name"], M.combo_name(combo))
        print(what, " ".join("%s %.3e (bar %.3e)" % (k, v, M.bar(combo, k)) for k, v in d.items()))
        report[what] = {k: dict(device=v, bar=M.bar(combo, k)) for k, v in d.items()}
        fails.extend(M.over_the_bar(d, combo, what))
    record("composite_maps/merged_%d_%d" % (na, nb), **report)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ equivalences
@pytest.mark.parametrize("S,n", [(1, 5), (65, 5), (193, 67), (1024, 5)])
def test_without_an_extra_map_gradient_the_bits_are_those_of_composite(S, n):
    from uc_nerf_amd import ops
    case, _, _ = M.dense("maps_S%d_n%d" % (S, n))
    for combo in (("rgb",), ("depth", "weights"), ("rgb", "depth", "acc", "weights")):
        for white in (False, True):
            grads, outs = [], []
            for fn in (ops.composite, ops.composite_maps):
                raw = dev(case["raw"]).requires_grad_(True)
                o = fn(raw, dev(case["z"]), white)
                assert len(o) == 6
                named = dict(zip(("rgb", "depth", "acc", "weights", "disp", "var"), o))
                sum((named[k] * dev(case["g_" + k])).sum() for k in combo).backward()
                grads.append(raw.grad)
                outs.append(named)
            assert torch.equal(grads[0], grads[1]), (S, combo, white)
            for k in outs[0]:
                same(outs[1][k].detach(), outs[0][k].detach(), "forward " + k)


@pytest.mark.parametrize("na,nb", [(1, 64), (128, 64), (0, 65)])
def test_merged_without_an_extra_map_gradient_is_composite_merged_and_with_one_is_dense_on_merged_rows(na, nb):
    from uc_nerf_amd import ops
    m, case, _, _ = M.merged(na, nb)
    rank, z = dev(m["rank"]), dev(m["z"])

    def run(fn, combo, u=None):
        a, b = dev(m["raw_a"]).requires_grad_(True), dev(m["raw_b"]).requires_grad_(True)
        o = fn(a, b, rank, z, True) if u is None else fn(a, b, rank, z, True, u)
        named = dict(zip(M.MAPS[:4] + ("disp", "var", "wu"), o))
        sum((named[k] * dev(case["g_" + k])).sum() for k in combo).backward()
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
        return zero(a), zero(b), named

    for combo in (("depth",), ("rgb", "depth", "acc", "weights")):
        want, got = run(ops.composite_merged, combo), run(ops.composite_merged_maps, combo)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), combo
        for k in want[2]:
            same(got[2][k].detach(), want[2][k].detach(), "forward " + k)
    for combo in M.combos_of(na + nb):
        u = dev(case["u"]).requires_grad_(True)
        g_a, g_b, named = run(ops.composite_merged_maps, combo, u)
        raw = ops.merge_rows(dev(m["raw_a"]), dev(m["raw_b"]), rank).requires_grad_(True)
        u2 = dev(case["u"]).requires_grad_(True)
        dense = dict(zip(M.MAPS[:4] + ("disp", "var", "wu"), ops.composite_maps(raw, z, True, u2)))
        sum((dense[k] * dev(case["g_" + k])).sum() for k in combo).backward()
        w_a, w_b = MB.unmerge(raw.grad, rank, na)
        same(g_a, w_a, "%s g_raw_a" % (combo,))
        same(g_b, w_b, "%s g_raw_b" % (combo,))
        for k in dense:
            same(named[k].detach(), dense[k].detach(), "forward " + k)
        if "wu" in combo:
            same(u.grad, u2.grad, "g_u")
        else:
            assert u.grad is None and u2.grad is None


@pytest.mark.parametrize("S,n", [(65, 5), (257, 67)])
def test_second_call_into_the_same_dirty_buffers_gives_the_same_bits(S, n):
    from uc_nerf_amd import ops
    case, _, _ = M.dense("maps_S%d_n%d" % (S, n))
    fwd = ops.composite_fwd(dev(case["raw"]), dev(case["z"]), u=dev(case["u"]))
    args = (fwd["weights"], fwd["depth"], fwd["acc"], dev(case["u"]))
    kw = {k: dev(case[k]) for k in ("g_var", "g_disp", "g_wu", "g_depth", "g_acc", "g_weights")}
    fresh = ops.composite_fold_grads(*args, **kw)
    assert all(bool(torch.isfinite(t).all()) for t in fresh)
    nan = float("nan")
    out = (torch.full((n,), nan, device=DEV), torch.full((n,), nan, device=DEV), torch.full((n, S), nan, device=DEV), torch.full((n, S), nan, device=DEV))
    for call in range(2):
        got = ops.composite_fold_grads(*args, out=out, **kw)
        for g, o, f, name in zip(got, out, fresh, ("g_depth'", "g_acc'", "g_weights'", "g_u")):
            assert g.data_ptr() == o.data_ptr()
            same(o, f, "%s, call %d into the caller's buffers" % (name, call))
    # ... and through autograd: two backward passes of one graph
    raw, u = dev(case["raw"]).requires_grad_(True), dev(case["u"]).requires_grad_(True)
    o = ops.composite_maps(raw, dev(case["z"]), False, u)
    loss = sum((t * dev(case["g_" + k])).sum() for t, k in zip(o, M.MAPS[:4] + ("disp", "var", "wu")))
    g1 = torch.autograd.grad(loss, (raw, u), retain_graph=True)
    g2 = torch.autograd.grad(loss, (raw, u))
    same(g2[0], g1[0], "g_raw, second backward")
    same(g2[1], g1[1], "g_u, second backward")


# ------------------------------------------------------------------------------------------------ errors
def test_argument_errors_are_einval_and_an_empty_batch_succeeds():
    import ctypes as C

    from uc_nerf_amd import _lib as L
    from uc_nerf_amd import ops
    n, S = 4, 8
    w, d, a, u = (torch.rand(n, S, device=DEV), torch.rand(n, device=DEV) + 1, torch.rand(n, device=DEV) + 0.5, torch.rand(n, S, device=DEV))
    g = torch.randn(n, device=DEV)

    def rc(weights, u_, out_w=None, **ups):
        p = L.CompositeFoldParams()
        p.n, p.S = weights.shape
        outs = [torch.empty(n, device=DEV), torch.empty(n, device=DEV), torch.empty_like(weights) if out_w is None else out_w]
        p.weights, p.depth, p.acc, p.u = weights.data_ptr(), d.data_ptr(), a.data_ptr(), 0 if u_ is None else u_.data_ptr()
        for k, v in ups.items():
            setattr(p, k, v.data_ptr())
        p.g_depth_out, p.g_acc_out, p.g_weights_out = (t.data_ptr() for t in outs)
        return L.lib().ucnerf_composite_fold_grads(C.addressof(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    EINVAL = -1
    assert rc(w[:, :1].contiguous(), None, g_var=g) == EINVAL                    # the variance of one weight
    assert rc(w, None, g_wu=g) == EINVAL                                         # sum w u without u
    assert rc(w, u, out_w=w, g_var=g) == EINVAL                                  # output on an input
    assert rc(w, u, out_w=u, g_wu=g) == EINVAL
    assert rc(w, u, g_var=g, g_wu=g, g_disp=g) == 0                              # (the same call, well formed)
    with pytest.raises(RuntimeError, match="g_var needs S >= 2"):
        ops.composite_fold_grads(w[:, :1].contiguous(), d, a, g_var=g)
    with pytest.raises(RuntimeError, match="needs the per-sample uncertainty"):
        ops.composite_fold_grads(w, d, a, g_wu=g)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.composite_fold_grads(w, d, a, g_depth=g, g_disp=g, out=(g, torch.empty_like(g), torch.empty_like(w), None))
    with pytest.raises(RuntimeError, match="elements"):
        ops.composite_fold_grads(w, d, a, g_disp=g[:2])
    e1, e2 = torch.empty(0, device=DEV), torch.empty(0, S, device=DEV)
    out = ops.composite_fold_grads(e2, e1, e1, e2, g_var=e1, g_wu=e1)            # n = 0: success, nothing launched
    assert [tuple(t.shape) for t in out] == [(0,), (0,), (0, S), (0, S)]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ render_train
def test_render_train_maps_trains_through_var_and_leaves_the_default_alone():
    """64 rays, 8 + 16 samples.  maps=False (and no argument) is the parent's render_train to the bit, outputs and gradients (see below for the
    parameter gradient, which the parent itself does not reproduce to the bit); with maps=True
    the values are the same and a loss on var alone reaches the parameters, where today it raises (var carries no history).
    The gradient arriving at the coarse rows is held to the float64 oracle's compositing under the var bar of the differential test; the
    parameter gradients against the float64 oracle pipeline are the next test."""
    import test_hip_render_train as TR
    n, nc, nf = 64, 8, 16
    i = _interior_inputs(n, nc, nf)
    kw = dict(perturb=1.0, noise=i["noise"], u=i["u"])
    target = i["target"].to(DEV)
    # ---- maps=False: bit-identical to the call without the argument.  The parent's parameter gradient is not reproducible to the bit from one
    # call to the next (the network's weight-gradient kernels add with atomics; measured on the device: two calls WITHOUT the argument differ
    # in the last bits of 40 % of the entries), so the bits are asked of everything that is: every output, and the gradient arriving at the
    # coarse rows -- through the coarse compositing and, as raw_b, the fine one: all the code the argument selects.  The parameter gradient
    # is asked to the bit when the parent's own two calls agree to the bit, and otherwise to lie within the parent's own call-to-call distance.
    res = []
    for extra in ({}, {}, dict(maps=False)):
        r, flat = TR._renderer(nc, nf)
        flat = flat.requires_grad_(True)
        out = r.render_train(i["xs"], i["ys"], flat, **kw, **extra)
        out["coarse"]["raw"].retain_grad()
        TR._loss(out["coarse"]["rgb"], out["rgb"], out["depth"], target).backward()
        res.append((out, flat.grad))
    twin = res.pop(1)
    assert set(res[0][0]) == set(res[1][0]) and set(res[0][0]["coarse"]) == set(res[1][0]["coarse"])
    for k in ("rgb", "depth", "acc", "disp", "weights", "var", "z_fine"):
        same(res[1][0][k].detach(), res[0][0][k].detach(), "maps=False " + k)
    for k in ("rgb", "depth", "weights", "raw"):
        same(res[1][0]["coarse"][k].detach(), res[0][0]["coarse"][k].detach(), "maps=False coarse." + k)
    same(res[1][0]["coarse"]["raw"].grad, res[0][0]["coarse"]["raw"].grad, "maps=False gradient at the coarse rows")
    same(twin[0]["coarse"]["raw"].grad, res[0][0]["coarse"]["raw"].grad, "the parent's own gradient at the coarse rows, second call")
    noise = float((twin[1] - res[0][1]).abs().max())
    dist = float((res[1][1] - res[0][1]).abs().max())
    print("parameter gradient: maps=False is %.3e from the call without the argument; two calls without it are %.3e apart (max|g| %.3e)"
          % (dist, noise, float(res[0][1].abs().max())))
    if noise == 0.0:
        same(res[1][1], res[0][1], "maps=False parameter gradient")
    else:
        assert dist <= 4.0 * noise, (dist, noise)
    assert not res[0][0]["var"].requires_grad and not res[0][0]["disp"].requires_grad
    with pytest.raises(RuntimeError):
        res[0][0]["var"].sum().backward()                                        # the parent: a loss on var trains nothing
    # ---- the gradient arriving at the rows, against the float64 oracle's compositing on the device's own rows: the fine pass's raw rows are
    # re-evaluated (the forward is reproducible to the bit), merged with the coarse ones, and var differentiated in float64.  The var bar
    # of the differential test applies as it stands: g_var is drawn on the scale of the case file (N(0, 1) * S).
    from uc_nerf_amd import ops
    rows = _var_step()
    out, g_var = rows["out"], rows["g_var"]
    for k in ("rgb", "depth", "acc", "disp", "weights", "var", "z_fine"):
        same(out[k].detach(), res[0][0][k].detach(), "maps=True " + k)
    assert out["var"].requires_grad and out["disp"].requires_grad and out["coarse"]["var"].requires_grad and out["coarse"]["disp"].requires_grad
    flat, r = rows["flat"], rows["r"]
    assert flat.grad is not None and bool(torch.isfinite(flat.grad).all()) and int(torch.count_nonzero(flat.grad)) > flat.numel() // 2
    rays_d, z_s, rank = out["rays_d"].detach(), out["z_samples"].detach(), out["coarse"]["merge_rank"]
    angle, _ = ops.dir_feature(rays_d, r.scene["w2cs"][0])
    with torch.no_grad():
        raw_f = r._eval_train(flat.detach(), r.pw.pack(flat.detach()), rays_d, angle, z_s)
    a = raw_f.cpu().double().requires_grad_(True)
    b = out["coarse"]["raw"].detach().cpu().double().requires_grad_(True)
    ref = M.oracle_maps(MB.merge(a, b, rank.cpu()), out["z_fine"].detach().cpu().double(), torch.zeros(n, nc + nf, dtype=torch.float64), False)
    assert float((ref["var"].detach() - out["var"].detach().cpu().double()).abs().max()) <= 1e-6      # the same rows: the same map
    (ref["var"] * g_var.double()).sum().backward()
    d = CC.bwd_distances(out["coarse"]["raw"].grad.cpu(), b.grad)
    print("var loss, gradient at the coarse rows: %s (bar %.3e), max|g| %.3e" % (d, M.bar(("var",), "g_density"), float(b.grad.abs().max())))
    assert int(torch.count_nonzero(out["coarse"]["raw"].grad[..., 3])) > n * nc // 2
    assert not M.over_the_bar(d, ("var",), "render_train(maps=True) var loss, coarse rows"), d


def _interior_inputs(n, nc, nf):
    """tests/test_hip_render_train.py's inputs with the pixels moved off the first and last row and column.  On rows 0 and H - 1 the rays of
    this scene project exactly onto the edge of the x-translated source views, where the gather's in-mask test is discontinuous: a float32
    and a float64 evaluation land on different sides of it, and no float64 pipeline can serve as a reference there (measured on the CPU,
    no device: the float32 oracle pipeline is 2e-01 of max|g| from the float64 one with those rows, 1.6e-05 without them)."""
    import test_hip_render_train as TR
    i = TR._inputs(n, nc, nf)
    i["ys"], i["xs"] = i["ys"].clamp(1, TR.H - 2), i["xs"].clamp(1, TR.W - 2)
    return i


@functools.lru_cache(maxsize=None)
def _var_step():
    """One render_train(maps=True) step at 64 rays x 8 + 16 with a loss on the fine pass's var alone."""
    import test_hip_render_train as TR
    n, nc, nf = 64, 8, 16
    i = _interior_inputs(n, nc, nf)
    r, flat = TR._renderer(nc, nf)
    flat = flat.requires_grad_(True)
    out = r.render_train(i["xs"], i["ys"], flat, maps=True, perturb=1.0, noise=i["noise"], u=i["u"])
    out["coarse"]["raw"].retain_grad()
    g_var = torch.randn(n, generator=torch.Generator().manual_seed(3)) * (nc + nf)
    (out["var"] * g_var.to(DEV)).sum().backward()
    return dict(r=r, flat=flat, out=out, g_var=g_var)


def test_render_train_var_loss_parameter_gradients_match_the_float64_oracle_pipeline():
    """The parameter gradients of a loss on var alone against the float64 oracle PIPELINE (tests/test_hip_render_train.py's: the oracle's own
    coordinates, gather and network in float64, at the device's depths and on the device's side of every relu), each tensor's distance taken
    relative to its largest gradient, under the var bar of the differential test (4 x 8.1e-06 = 3.24e-05).

    The bar is an absolute distance for gradients of O(1); a parameter tensor's gradient is a sum over all 64 x 24 samples of what arrives at the
    rows, so it is held relative to the tensor's largest entry.  The pixels are _interior_inputs': off the rows on which a float64 pipeline
    is no reference.  Measured on the device: 1.5e-06 (alpha_linear.bias) to 2.9e-05 (pts_linears.1.bias) of max|g| with the default backward
    of the network (split-bf16 data gradients), 1.0e-06 to 1.8e-05 with the layer-by-layer float32 one; the float32 oracle pipeline itself is
    1.6e-05 from the float64 one on such pixels (CPU).  The tensors the loss does not reach (views_linears, rgb_linear, confi_rgb_linear) are
    exactly zero on both sides."""
    import fuzz_grads as FG
    import test_hip_render_train as TR
    from fuzz_render import oracle_pass
    rows = _var_step()
    r, flat, out, g_var = rows["r"], rows["flat"], rows["out"], rows["g_var"]
    sd, sc = TR._sd(), TR._scene_cpu()
    rays_d, z_c, z_f, z_s = (out[k].detach() for k in ("rays_d", "z_coarse", "z_fine", "z_samples"))
    sides_c = TR._device_sides(r, flat, rays_d, z_c)
    sides_f = TR._merged_sides(TR._device_sides(r, flat, rays_d, z_s), sides_c, out["coarse"]["merge_rank"].cpu())
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    scene = {k: ([x.double() for x in v] if isinstance(v, list) else (v.double() if torch.is_tensor(v) and v.is_floating_point() else v))
             for k, v in sc.items()}
    with FG.Relus(sides_f):
        fine, _, _ = oracle_pass(p, scene, rays_d.cpu().double(), z_f.cpu().double(), False)
    (fine["var"] * g_var.double()).sum().backward()
    got = TR._by_name(sd, flat.grad.cpu(), [None] * 5)
    bar, fails, report = M.bar(("var",), "g_density"), [], {}
    for k in sd:
        if p[k].grad is None:
            assert not bool(got[k].any()), k
            continue
        scale = float(p[k].grad.abs().max())
        dist = float((got[k].double() - p[k].grad).abs().max()) / max(scale, 1e-30)
        print("%s: %.3e of max|g| = %.3e (bar %.3e)" % (k, dist, scale, bar))
        report[k] = dict(device=dist, bar=bar, scale=scale)
        if not dist <= bar:
            fails.append("%s: %.3e of max|g| > bar %.3e" % (k, dist, bar))
    record("composite_maps/render_train_var", **report)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ no synchronisation
def test_forward_and_backward_make_no_synchronising_call():
    """Under torch's sync debug mode "error" a synchronising torch call raises (the mode does not see ctypes calls: the entry point itself is a
    launch and nothing else, csrc/composite_fold.hip)."""
    from uc_nerf_amd import ops
    case, _, _ = M.dense("maps_S65_n5")
    g = {k: dev(case["g_" + k]) for k in M.MAPS}
    raw0, z, u0 = dev(case["raw"]), dev(case["z"]), dev(case["u"])

    def step():
        raw, u = raw0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
        outs = ops.composite_maps(raw, z, False, u)
        sum((o * g[k]).sum() for o, k in zip(outs, M.MAPS[:4] + ("disp", "var", "wu"))).backward()
        return raw.grad, u.grad

    step()                                                                       # warm: the library load, one-time allocations
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g_raw, g_u = step()                                                      # raises where a torch call inside synchronises
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert g_raw is not None and g_u is not None and bool(torch.isfinite(g_raw).all())
