"""FeatureNet over all views in one pass on the GPU (the group dimension of csrc/bn.hip, ops.batch_norm_train(groups=), FeatureNet.forward_views,
CascadeMVSNet(feature_views="batched")): the grouped batch-norm against G ungrouped calls on the G slabs -- bit for bit in everything but the
parameter gradients, which are float64 sums over the groups rounded once and are held to that --, its workspace, guards and determinism, the
module's batched pass against the per-view loop on a deep copy, a second training step, one training step of the whole cascade and the launch
count.

Bars.  Parameter gradients of the grouped backward: t = the float64 sum of the per-slab ungrouped results t_q; |got - t| <= 2^-23 sum |t_q| (each
t_q carries one rounding of 2^-24 relative, the grouped result one rounding of the exact sum, nothing else differs).  Parameter gradients of the
module: the project's chain rule, 4 x the float32 CPU restatement's own largest distance from float64 (tests/test_hip_feature_train.py).

Measured on an MI355X (largest figures of a run): the grouped parameter gradients reach 0.527 of their bar over 48 comparisons, the module's
and the cascade's comparisons 0.449 of the chain bar over 257 (profiles/feature_views.md)."""
import copy
import itertools

import pytest
import torch

import bn_cases as BC
import cascade_stubs as S
import feature_train_cases as FC
import feature_views_cases as VC
import mvs_cnn_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
SHARES = []                                                                # device error / chain bar of every held() comparison of this run
GROUP_SHARES = []                                                          # the same for the grouped parameter gradients' own bar
MOMENTUM = 0.1


def M():
    from uc_nerf_amd.network import mvs_models
    return mvs_models


def ops():
    from uc_nerf_amd import ops as o
    return o


def lib():
    from uc_nerf_amd import _lib
    return _lib


def held(name, got, ref64, cpu32):
    bar, err32 = FC.chain_bar(ref64, cpu32)
    err = float((got.detach().cpu().double() - ref64).abs().max())
    SHARES.append(err / bar)
    print("%s: device %.3g, float32 cpu %.3g, bar %.3g, share of the bar %.3f, largest %.3g" % (name, err, err32, bar, err / bar, float(ref64.abs().max())))
    assert got.shape == ref64.shape and got.dtype == torch.float32
    assert err <= bar, name


def partials(n, S_):
    return lib().lib().ucnerf_bn_partials(n, S_)


def geometry(y, G):
    n, C = y.shape[0] // G, y.shape[1]
    S_ = y.numel() // (y.shape[0] * C)
    return n, C, S_, partials(n, S_)


def stream():
    return torch.cuda.current_stream().cuda_stream


def raw_forward(G, y, gamma, beta, bufs, relu, skip, out, ws, saved):
    """The two grouped entry points through the C ABI (also for G == 1; the ungrouped entry points against these at G == 1: tests/test_hip_bn.py)."""
    Lb = lib()
    n, C, S_, P = geometry(y, G)
    s, a = Lb.BnStatsGroupsParams(), Lb.BnApplyGroupsParams()
    s.G, s.n, s.C, s.S, s.workspace_triples, s.y, s.workspace = G, n, C, S_, G * C * P, y.data_ptr(), ws.data_ptr()
    a.G, a.n, a.C, a.S, a.workspace_triples, a.eps, a.momentum, a.relu = G, n, C, S_, G * C * P, BC.EPS, MOMENTUM, int(relu)
    a.y, a.workspace, a.weight, a.bias, a.skip, a.out = y.data_ptr(), ws.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0 if skip is None else skip.data_ptr(), out.data_ptr()
    a.saved_mean, a.saved_var, a.running_mean, a.running_var, a.num_batches_tracked = (saved[0].data_ptr(), saved[1].data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                                                      bufs[2].data_ptr())
    Lb.call("ucnerf_bn_stats_groups", s, stream())
    Lb.call("ucnerf_bn_apply_groups", a, stream())


def raw_backward(G, go, y, saved, gamma, beta, relu, grad_y, ws, grads, eps=BC.EPS):
    Lb = lib()
    n, C, S_, P = geometry(y, G)
    r, a = Lb.BnBwdReduceGroupsParams(), Lb.BnBwdApplyGroupsParams()
    for q in (r, a):
        q.G, q.n, q.C, q.S, q.workspace_pairs, q.eps, q.relu = G, n, C, S_, G * C * P, eps, int(relu)
        q.g, q.y, q.workspace = go.data_ptr(), y.data_ptr(), ws.data_ptr()
        q.saved_mean, q.saved_var, q.weight, q.bias = saved[0].data_ptr(), saved[1].data_ptr(), gamma.data_ptr(), beta.data_ptr()
    a.grad_y, a.grad_weight, a.grad_bias = grad_y.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr()
    Lb.call("ucnerf_bn_bwd_reduce_groups", r, stream())
    Lb.call("ucnerf_bn_bwd_apply_groups", a, stream())


def grouped_forward(G, y, gamma, beta, bufs, relu, skip, inplace):
    """-> (out, saved_mean [G,C], saved_var [G,C]) of the grouped pair: through the ops for G > 1, through the C ABI for G == 1."""
    y = y.clone()
    out = y if inplace else torch.empty_like(y)
    if G > 1:
        res = ops().batch_norm_train(y, gamma, beta, *bufs, momentum=MOMENTUM, eps=BC.EPS, relu=relu, skip=skip, out=out, return_stats=True, groups=G)
        assert res[0] is out and res[1].shape == res[2].shape == (G, y.shape[1])
        return res
    n, C, S_, P = geometry(y, G)
    ws, saved = torch.empty(G * C * P * 3, dtype=torch.float64, device=DEV), torch.empty((2, G, C), device=DEV)
    raw_forward(G, y, gamma, beta, bufs, relu, skip, out, ws, saved)
    return out, saved[0], saved[1]


def slab_forward(G, y, gamma, beta, bufs, relu, skip, inplace):
    """G successive ungrouped calls, each on a copy of its group's slab alone."""
    n = y.shape[0] // G
    outs, means, variances = [], [], []
    for q in range(G):
        slab = y[q * n:(q + 1) * n].clone()
        sk = None if skip is None else skip[q * n:(q + 1) * n].clone()
        o, m, v = ops().batch_norm_train(slab, gamma, beta, *bufs, momentum=MOMENTUM, eps=BC.EPS, relu=relu, skip=sk, out=slab if inplace else None,
                                         return_stats=True)
        outs.append(o), means.append(m), variances.append(v)
    return torch.cat(outs), torch.stack(means), torch.stack(variances)


def on_device(case):
    return tuple(None if t is None else t.to(DEV) for t in case)


# ------------------------------------------------------------------------------------------------ 1. the grouped forward
@pytest.mark.parametrize("shape", VC.OP_SHAPES, ids=str)
def test_grouped_forward_is_bit_equal_to_ungrouped_calls_on_the_slabs(shape):
    G, n, C, spatial = shape = VC.op_shape(shape, partials)
    if len(spatial) == 1 and spatial[0] > 4096:
        P = partials(n, spatial[0])
        L_ = ((n * spatial[0] + P - 1) // P + 3) // 4 * 4
        assert P >= 3 and 0 < n * spatial[0] - (P - 1) * L_ < L_, shape                      # a shorter last slice
    for relu, with_skip, inplace in itertools.product((True, False), repeat=3):
        y, skip, _, gamma, beta = on_device(VC.op_inputs(shape, 61, with_skip))
        mine, theirs = ([t.to(DEV) for t in VC.buffers(C, 62)] for _ in range(2))
        got = grouped_forward(G, y, gamma, beta, mine, relu, skip, inplace)
        want = slab_forward(G, y, gamma, beta, theirs, relu, skip, inplace)
        what = (shape, relu, with_skip, inplace)
        for name, a, b in zip(("out", "saved_mean", "saved_var"), got, want):
            assert a.shape == b.shape and torch.equal(a, b), (name,) + what
        for name, a, b in zip(("running_mean", "running_var", "num_batches_tracked"), mine, theirs):
            assert torch.equal(a, b), (name,) + what
        assert int(mine[2]) == 7 + G and not torch.equal(mine[0], VC.buffers(C, 62)[0].to(DEV))
        if relu and not with_skip:
            assert bool((got[0] == 0).any()) and bool((got[0] > 0).any())


# ------------------------------------------------------------------------------------------------ 2. the grouped backward
def grouped_backward(G, go, y, saved, gamma, beta, relu, inplace, eps=BC.EPS):
    go = go.clone()
    if G > 1:
        res = ops().batch_norm_train_bwd(go, y, saved[0], saved[1], gamma, beta, eps=eps, relu=relu, out=go if inplace else None, groups=G)
        assert (res[0] is go) == inplace
        return res
    n, C, S_, P = geometry(y, G)
    ws, grads = torch.empty(G * C * P * 2, dtype=torch.float64, device=DEV), torch.empty((2, C), device=DEV)
    grad_y = go if inplace else torch.empty_like(go)
    raw_backward(G, go, y, saved, gamma, beta, relu, grad_y, ws, grads, eps)
    return grad_y, grads[0], grads[1]


def slab_backward(G, go, y, saved, gamma, beta, relu, eps=BC.EPS):
    n = y.shape[0] // G
    res = [ops().batch_norm_train_bwd(go[q * n:(q + 1) * n].clone(), y[q * n:(q + 1) * n].clone(), saved[0][q].clone(), saved[1][q].clone(), gamma, beta,
                                      eps=eps, relu=relu) for q in range(G)]
    return torch.cat([r[0] for r in res]), torch.stack([r[1] for r in res]), torch.stack([r[2] for r in res])


@pytest.mark.parametrize("shape", VC.OP_SHAPES, ids=str)
def test_grouped_backward_grad_y_is_bit_equal_and_the_parameter_gradients_are_the_float64_sums(shape):
    G, n, C, spatial = shape = VC.op_shape(shape, partials)
    for relu, inplace in itertools.product((True, False), repeat=2):
        y, _, go, gamma, beta = on_device(VC.op_inputs(shape, 63, False))
        _, mean, var = grouped_forward(G, y, gamma, beta, [t.to(DEV) for t in VC.buffers(C, 64)], relu, None, False)
        saved = (mean.contiguous(), var.contiguous())
        got = grouped_backward(G, go, y, saved, gamma, beta, relu, inplace)
        want = slab_backward(G, go, y, saved, gamma, beta, relu)
        assert torch.equal(got[0], want[0]), ("grad_y", shape, relu, inplace)
        for name, a, per_slab in (("grad_weight", got[1], want[1]), ("grad_bias", got[2], want[2])):
            t = per_slab.double().sum(0)
            bound = 2.0 ** -23 * per_slab.double().abs().sum(0)
            err = (a.double() - t).abs()
            share = float((err / bound.clamp_min(1e-300)).max())
            GROUP_SHARES.append(share)
            print("%s %s relu=%s: largest error %.3g, largest share of 2^-23 sum |t_q| %.3f" % (name, shape, relu, float(err.max()), share))
            assert a.shape == (C,) and bool((err <= bound).all()), (name, shape, relu, inplace)
            if G == 1:
                assert torch.equal(a, per_slab[0]), (name, shape)                             # the ungrouped entry's own bits


@pytest.mark.parametrize("shape", VC.OP_SHAPES[:3], ids=str)
@pytest.mark.parametrize("relu", (False, True))
def test_grouped_parameter_gradients_are_exact_on_an_integer_lattice(shape, relu):
    G, n, C, spatial = shape
    y, go, mu, var, eps = on_device(VC.exact_backward_case(G, n, C, spatial, 65)[:4]) + (VC.exact_backward_case(G, n, C, spatial, 65)[4],)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    got = grouped_backward(G, go, y, (mu, var), gamma, beta, relu, False, eps)
    want = slab_backward(G, go, y, (mu, var), gamma, beta, relu, eps)
    assert torch.equal(got[0], want[0])
    for name, a, per_slab in (("grad_weight", got[1], want[1]), ("grad_bias", got[2], want[2])):
        assert bool((per_slab * 2 == (per_slab * 2).round()).all()) and float(per_slab.abs().max()) > 0, name
        assert torch.equal(a, per_slab.sum(0)) and torch.equal(a.double(), per_slab.double().sum(0)), (name, shape)


@pytest.mark.parametrize("relu", (False, True))
def test_grouped_parameter_gradients_are_summed_in_float64_and_rounded_once(relu):
    """Groups 0 and 1 hold the same y and opposite gradients a thousand times the size of group 2's: their terms cancel EXACTLY in a float64 sum
    (B_1 = -B_0 and A_1 = -A_0 bit for bit, the same r), so grad_weight and grad_bias are the ungrouped backward's bits on slab 2 alone.  A sum
    kept in float32 rounds the first term before the second arrives and leaves that rounding, large against group 2's term, in the result."""
    n, C, S_ = 2, 5, 37
    g = torch.Generator().manual_seed(66)
    y0, go0 = 1.5 * torch.randn(n, C, S_, generator=g) + 0.5, 1000.0 * torch.randn(n, C, S_, generator=g)
    y = torch.cat([y0, y0, torch.randn(n, C, S_, generator=g)]).to(DEV)
    go = torch.cat([go0, -go0, 1e-3 * torch.randn(n, C, S_, generator=g)]).to(DEV)
    gamma, beta = (0.6 + 0.8 * torch.rand(C, generator=g)).to(DEV), (0.3 * torch.randn(C, generator=g)).to(DEV)
    _, mean, var = grouped_forward(3, y, gamma, beta, [t.to(DEV) for t in VC.buffers(C, 67)], relu, None, False)
    saved = (mean.contiguous(), var.contiguous())
    assert torch.equal(saved[0][0], saved[0][1]) and torch.equal(saved[1][0], saved[1][1])
    got = grouped_backward(3, go, y, saved, gamma, beta, relu, False)
    want = slab_backward(3, go, y, saved, gamma, beta, relu)
    assert torch.equal(got[0], want[0])
    for name, a, per_slab in (("grad_weight", got[1], want[1]), ("grad_bias", got[2], want[2])):
        assert torch.equal(per_slab[0], -per_slab[1]) and float(per_slab[0].abs().min()) > 100 * float(per_slab[2].abs().max()) > 0, name
        assert torch.equal(a, per_slab[2]), (name, relu)


# ------------------------------------------------------------------------------------------------ 3. workspace, guards, determinism
def guarded(numel, dtype=torch.float32, guard=64):
    t = torch.full((numel + 2 * guard,), float("nan"), dtype=dtype, device=DEV)
    t[:guard], t[-guard:] = -12345.0, -12345.0
    return t, t[guard:-guard]


def intact(t, guard=64):
    return bool((t[:guard] == -12345.0).all()) and bool((t[-guard:] == -12345.0).all()) and not bool(torch.isnan(t[guard:-guard]).any())


@pytest.mark.parametrize("shape", (VC.OP_SHAPES[1], VC.OP_SHAPES[2]), ids=str)
def test_grouped_kernels_write_all_of_their_outputs_and_nothing_else_and_repeat_their_bits(shape):
    G, n, C, spatial = shape
    y, _, go, gamma, beta = on_device(VC.op_inputs(shape, 66, False))
    _, _, S_, P = geometry(y, G)
    runs = []
    for _ in range(2):
        bufs = [t.to(DEV) for t in VC.buffers(C, 67)]
        ws, ws_in = guarded(G * C * P * 3, torch.float64)
        saved, saved_in = guarded(2 * G * C)
        out, out_in = guarded(y.numel())
        raw_forward(G, y, gamma, beta, bufs, True, None, out_in, ws_in, saved_in.view(2, G, C))
        ws2, ws2_in = guarded(G * C * P * 2, torch.float64)
        gy, gy_in = guarded(y.numel())
        grads, grads_in = guarded(2 * C)
        raw_backward(G, go, y, saved_in.view(2, G, C), gamma, beta, True, gy_in, ws2_in, grads_in.view(2, C))
        torch.cuda.synchronize()
        for name, t in (("workspace", ws), ("saved", saved), ("out", out), ("backward workspace", ws2), ("grad_y", gy), ("parameter gradients", grads)):
            assert intact(t), (name, shape)                                                   # every element overwritten, the guard words untouched
        runs.append([t.clone() for t in (ws, saved, out, ws2, gy, grads)] + bufs)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    res = ops().batch_norm_train(y.clone(), gamma, beta, *[t.to(DEV) for t in VC.buffers(C, 67)], momentum=MOMENTUM, eps=BC.EPS, relu=True, return_stats=True, groups=G)
    assert torch.equal(res[0].flatten(), runs[0][2][64:-64]) and torch.equal(torch.stack(res[1:]).flatten(), runs[0][1][64:-64])      # the ops run these launches


# ------------------------------------------------------------------------------------------------ 4. the module
ROUTES = ("eval", "batch_stats", "training")


def make_net(case):
    return BC.randomise_train(M().FeatureNet(8, batch_stats="device", training="device"), case[1]).to(DEV)


def run_views(net, imgs, route, batched, R=None):
    """-> ({stage: [V,C,h,w]}, image gradient or None) of one pass over the views on `route`, batched or as the loop."""
    net.train(route != "eval")
    X = imgs.clone().requires_grad_(route == "training")
    with torch.set_grad_enabled(route == "training"):
        if batched:
            outs = net.forward_views(X)
        else:
            per_view = [net(X[:, i]) for i in range(imgs.shape[1])]
            outs = {k: torch.cat([o[k] for o in per_view]) for k in VC.STAGES}
    if route != "training":
        assert all(v.grad_fn is None for v in outs.values())
        return outs, None
    for p in net.parameters():
        p.grad = None
    sum((outs[k] * R[k]).sum() for k in VC.STAGES).backward()
    return {k: v.detach() for k, v in outs.items()}, X.grad


@pytest.fixture(scope="module", params=range(len(VC.MODULE_CASES)), ids=lambda i: "imgs%s" % (VC.MODULE_CASES[i][0],))
def module_case(request):
    case = VC.MODULE_CASES[request.param]
    imgs, R = VC.module_inputs(case)
    net = make_net(case)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    r64, r32 = VC.feature_views(imgs, sd, torch.float64, R), VC.feature_views(imgs, sd, torch.float32, R)
    return case, net, sd, imgs.to(DEV), {k: v.to(DEV) for k, v in R.items()}, r64, r32


@pytest.mark.parametrize("route", ROUTES)
def test_forward_views_equals_the_loop_on_a_deep_copy(module_case, route, monkeypatch):
    case, net, sd, imgs, R, r64, r32 = module_case
    net.load_state_dict(sd)
    twin = copy.deepcopy(net)
    V = imgs.shape[1]
    groups = []
    real = ops().batch_norm_train
    monkeypatch.setattr(ops(), "batch_norm_train", lambda *a, **k: groups.append(k.get("groups", 1)) or real(*a, **k))
    real_layer = ops().conv2d_bn_train
    monkeypatch.setattr(ops(), "conv2d_bn_train", lambda *a, **k: groups.append(k.get("groups", 1)) or real_layer(*a, **k))
    got, gx = run_views(net, imgs, route, True, R)
    assert groups == {"eval": [], "batch_stats": [V] * 8, "training": [V] * 8}[route]       # the batched pass took the route's grouped launches
    want, wx = run_views(twin, imgs, route, False, R)
    for k in VC.STAGES:
        assert got[k].shape == R[k].shape and torch.equal(got[k], want[k]), (route, k)
    for (k, a), (_, b) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), (route, k)                                                  # every buffer (and parameter) as the loop leaves it
    moved = int(net.conv0[0].bn.num_batches_tracked) - int(sd["conv0.0.bn.num_batches_tracked"])
    assert moved == (0 if route == "eval" else V)
    if route == "training":
        assert not VC.relu_offenders(r64, r32)
        assert gx.shape == imgs.shape and float(gx.abs().max()) > 0 and torch.equal(gx, wx)   # the image gradient: per pixel and per group throughout
        grads, loop_grads = dict(net.named_parameters()), dict(twin.named_parameters())
        assert len(grads) == 31 == len(r64["grads"])
        for k, p in grads.items():
            held("batched grad " + k, p.grad, r64["grads"][k], r32["grads"][k])
            held("loop grad " + k, loop_grads[k].grad, r64["grads"][k], r32["grads"][k])
        for k in VC.STAGES:
            held(k, got[k], r64["out"][k], r32["out"][k])
        held("grad image", gx, r64["grad_x"], r32["grad_x"])
        for k, v in r64["sd"].items():                                                        # the buffers against V threaded float64 forwards
            if "running_" in k:
                r32v = r32["sd"][k]
                held("buffer " + k, net.state_dict()[k], v, r32v)
    elif route == "batch_stats":
        got4, _ = run_views(net, imgs[0], route, True)                                        # [V,3,H,W] means the same (the buffers move once more)
        want4, _ = run_views(twin, imgs, route, False)
        assert all(torch.equal(got4[k], want4[k]) for k in VC.STAGES)
        assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
    net.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ 5. a second training step
def test_second_training_step_follows_the_moved_buffers_and_the_new_weights():
    case = VC.MODULE_CASES[0]
    imgs, R = VC.module_inputs(case)
    imgs, R = imgs.to(DEV), {k: v.to(DEV) for k, v in R.items()}
    net = make_net(case)
    twin = copy.deepcopy(net)
    first = {}
    for name, m, batched in (("batched", net, True), ("loop", twin, False)):
        first[name] = run_views(m, imgs, "training", batched, R)[0]
        with torch.no_grad():
            for p, q in zip(m.parameters(), net.parameters()):
                p.sub_(1e-3 * q.grad)                                                         # both take the BATCHED step: the same weights go into step two
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
    got, gx = run_views(net, imgs, "training", True, R)
    want, wx = run_views(twin, imgs, "training", False, R)
    for k in VC.STAGES:
        assert torch.equal(got[k], want[k]) and not torch.equal(got[k], first["batched"][k]), k      # the packed caches followed the weights' versions
    assert torch.equal(gx, wx)
    for (k, a), (_, b) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), k
    assert int(net.conv2[2].bn.num_batches_tracked) == 2 * imgs.shape[1]
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    r64, r32 = (VC.feature_views(imgs.cpu(), sd, dt, {k: v.cpu() for k, v in R.items()}) for dt in (torch.float64, torch.float32))
    if not VC.relu_offenders(r64, r32):                                                       # (the condition is asserted for the first step's weights only)
        for k, p in net.named_parameters():
            held("second step grad " + k, p.grad, r64["grads"][k], r32["grads"][k])


# ------------------------------------------------------------------------------------------------ 6. the cascade
def test_cascade_training_step_batched_against_loop():
    case = VC.CASCADE_CASE
    (_, V, _, H, W), ndepths = case[0], [48, 32, 8]
    imgs = VC.module_inputs(case)[0].to(DEV)
    affine, affine_inv = (t.to(DEV) for t in S.cameras(V, H, W, seed=100))
    near_far = torch.tensor([2.0, 11.0], device=DEV)
    g = torch.Generator().manual_seed(99)

    def build(views):
        net = M().CascadeMVSNet.with_cnns(ndepths=ndepths, training="device", feature_training="device", feature_views=views)
        MC.randomise(net.feature, case[1])
        for i, module in enumerate(net.cost_regularization):
            MC.randomise(module, 96 + i)
        return net.to(DEV).train()

    nets = {views: build(views) for views in ("batched", "loop")}
    assert all(torch.equal(a, b) for a, b in zip(nets["batched"].state_dict().values(), nets["loop"].state_dict().values()))
    sd = {k: v.detach().cpu().clone() for k, v in nets["loop"].feature.state_dict().items()}
    from uc_nerf_amd.utils.loss import cas_mvsnet_loss_device
    results, gts = {}, None
    for views, net in nets.items():
        seen = []                                                          # the feature maps as the cascade received them, to read their gradients
        if views == "batched":
            real = net.feature.forward_views
            net.feature.forward_views = lambda x, _real=real: seen.append(_real(x)) or seen[-1]
        else:
            net.feature.register_forward_hook(lambda module, args, out: seen.append(out))
        vol, conf, depth, outputs = net(imgs, affine, affine_inv, near_far, pad=0)
        assert len(seen) == (1 if views == "batched" else V)
        for out in seen:
            for v in out.values():
                v.retain_grad()
        if gts is None:
            gts = {k: 2.0 + 9.0 * torch.rand(outputs[k]["depth"].shape, generator=g) for k in VC.STAGES}
        weights = {k: torch.ones(outputs[k]["depth"].shape) for k in VC.STAGES}
        total, _ = cas_mvsnet_loss_device({k: outputs[k] for k in VC.STAGES}, gts, weights)
        (total + 1e-3 * vol.square().mean() + 1e-3 * conf.mean()).backward()
        results[views] = (vol, conf, outputs, {k: torch.cat([out[k].grad for out in seen]).cpu() for k in VC.STAGES})
    (vol_b, conf_b, out_b, R_b), (vol_l, conf_l, out_l, R_l) = results["batched"], results["loop"]
    assert torch.equal(vol_b, vol_l) and torch.equal(conf_b, conf_l)       # volume_feature_no_ref and photometric_confidence of the last stage
    for k in VC.STAGES:
        for name in ("depth", "photometric_confidence", "volume_feature_no_ref"):
            assert torch.equal(out_b[k][name], out_l[k][name]), (k, name)
    for (k, a), (_, b) in zip(nets["batched"].state_dict().items(), nets["loop"].state_dict().items()):
        assert torch.equal(a, b), k                                        # every buffer of every CNN after the step
    # backward: each net's FeatureNet gradients against the float64 per-view restatement driven by the gradients ITS feature maps received
    for views, R in (("batched", R_b), ("loop", R_l)):
        r64, r32 = VC.feature_views(imgs.cpu(), sd, torch.float64, R), VC.feature_views(imgs.cpu(), sd, torch.float32, R)
        assert not VC.relu_offenders(r64, r32)
        for k, p in nets[views].feature.named_parameters():
            assert p.grad is not None and float(p.grad.abs().max()) > 0, k
            held("cascade %s grad %s" % (views, k), p.grad, r64["grads"][k], r32["grads"][k])


# ------------------------------------------------------------------------------------------------ 7. launches
def test_batched_forward_issues_one_view_s_launches_for_three_views(monkeypatch):
    """Every wrapper's launch goes through ops._core._launch, which the ops modules bind by name at import; the one function it calls,
    _lib.call, is looked up per call, so the count is taken there."""
    counted = []
    real = lib().call
    monkeypatch.setattr(lib(), "call", lambda name, params, stream_: counted.append(name) or real(name, params, stream_))
    case = VC.MODULE_CASES[0]
    imgs = VC.module_inputs(case)[0].to(DEV)
    assert imgs.shape[1] == 3
    net = make_net(case)
    with torch.no_grad():
        net(imgs[:, 0]), net.forward_views(imgs)                           # (warm: the raw weights are packed once)
        counted.clear()
        net(imgs[:, 0])
        one_view = list(counted)
        counted.clear()
        net.forward_views(imgs)
        batched = list(counted)
        counted.clear()
        for i in range(3):
            net(imgs[:, i])
        loop = list(counted)
    assert len(one_view) == 13 + 2 * 8 == len(batched) and len(loop) == 3 * len(one_view)
    # (one view is G = 1 of the same entry points: the very same sequence of symbols)
    assert batched == one_view and sum(n.endswith("_groups") for n in batched) == 16 and not any("ucnerf_bn" in n and not n.endswith("_groups") for n in batched)


def test_zz_largest_share_of_the_bars():
    """Prints the largest device error / bar over the comparisons this run made (profiles/feature_views.md records them)."""
    if GROUP_SHARES:
        print("grouped parameter gradients: largest share of 2^-23 sum |t_q| over %d comparisons: %.3f" % (len(GROUP_SHARES), max(GROUP_SHARES)))
        assert max(GROUP_SHARES) <= 1.0
    if SHARES:
        print("largest share of the chain bar over %d comparisons: %.3f" % (len(SHARES), max(SHARES)))
        assert max(SHARES) <= 1.0
