"""The batch-statistic batch-norm on the GPU (csrc/bn.hip, ops.batch_norm_train) and the modules' train() + no_grad device route against the
float64 restatement of tests/bn_cases.py: the op on every epilogue and in place, determinism, a large offset (what a one-pass sum of squares
loses), an exactly constant channel, a poisoned workspace with guarded outputs, both networks, the choice of route by call count, the two weight
caches, and CascadeMVSNet.with_cnns end to end.

The bar is the project's chain rule: 4 x the float32 CPU restatement's own largest distance from float64, at least one float32 spacing of the
largest value.  Every comparison prints the device's error, the float32 restatement's error and their ratio."""
import itertools

import pytest
import torch

import bn_cases as BC
import cascade_stubs as S
import mvs_cnn_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def M():
    from uc_nerf_amd.network import mvs_models
    return mvs_models


def ops():
    from uc_nerf_amd import ops as o
    return o


def partials(n, S):
    from uc_nerf_amd import _lib
    return _lib.lib().ucnerf_bn_partials(n, S)


def held(name, got, ref64, cpu32):
    bar, err32 = BC.chain_bar(ref64, cpu32)
    err = float((got.detach().cpu().double() - ref64).abs().max())
    print("%s: device %.3g, float32 cpu %.3g, ratio %.2f, bar %.3g, largest %.3g" % (name, err, err32, err / max(err32, 1e-30), bar, float(ref64.abs().max())))
    assert got.shape == ref64.shape and got.dtype == torch.float32
    assert err <= bar, name
    return bar


def agree(name, a, b, bar):
    """Two routes of the same module against each other, under the bar either was held to."""
    err = float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())
    print("%s: the two routes differ by %.3g, bar %.3g" % (name, err, bar))
    assert err <= bar, name


class Case:
    """One op call's inputs on the host (seeded), and fresh device copies of them per call."""

    def __init__(self, shape, seed, y=None):
        g = torch.Generator().manual_seed(seed)
        C = shape[1]
        self.shape, self.count = tuple(shape), shape[0] * int(torch.tensor(shape[2:]).prod())
        self.y = torch.randn(shape, generator=g) * 1.5 + 0.5 if y is None else y
        self.skip = torch.randn(shape, generator=g)
        self.gamma, self.beta = 0.6 + 0.8 * torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
        self.rm, self.rv = 0.3 * torch.randn(C, generator=g), 0.5 + 1.5 * torch.rand(C, generator=g)

    def call(self, relu=True, skip=False, inplace=False, momentum=BC.MOMENTUM):
        """-> (out, saved_mean, saved_var, running_mean, running_var, num_batches_tracked) on the device after one call."""
        y, rm, rv = self.y.to(DEV), self.rm.to(DEV), self.rv.to(DEV)
        nbt = torch.tensor(7, dtype=torch.int64, device=DEV)
        out, mean, var = ops().batch_norm_train(y, self.gamma.to(DEV), self.beta.to(DEV), rm, rv, nbt, momentum=momentum, relu=relu,
                                                skip=self.skip.to(DEV) if skip else None, out=y if inplace else None, return_stats=True)
        assert (out is y) == inplace
        if not inplace:
            assert torch.equal(y.cpu(), self.y)                            # the input is left alone
        return out, mean, var, rm, rv, nbt

    def reference(self, dtype, relu, skip):
        out, mean, var = BC.bn_train(self.y, self.gamma, self.beta, dtype, relu=relu, skip=self.skip if skip else None)
        return (out, mean, var) + BC.running_update(self.rm, self.rv, mean, var, self.count, dtype)


NAMES = ("out", "saved_mean", "saved_var", "running_mean", "running_var")


# ------------------------------------------------------------------------------------------------ 1. the op against float64
@pytest.mark.parametrize("shape", BC.OP_SHAPES + ("ragged",), ids=str)
def test_op_against_float64(shape):
    if shape == "ragged":
        shape = BC.ragged_shape(partials)
        n, _, S_ = shape
        P = partials(n, S_)
        L = (-(-n * S_ // P) + 3) // 4 * 4                                  # the documented slice length: ceil(N / P) rounded up to 4
        assert P >= 3 and 0 < n * S_ - (P - 1) * L < L, (shape, P, L)       # at least three slices, the last one shorter
    case = Case(shape, 401)
    for relu, skip in itertools.product((True, False), (False, True)):
        got = case.call(relu, skip, inplace=False)
        again = case.call(relu, skip, inplace=True)
        r64, r32 = case.reference(torch.float64, relu, skip), case.reference(torch.float32, relu, skip)
        for name, g, a, w64, w32 in zip(NAMES, got, again, r64, r32):
            held("%s %s relu=%s skip=%s" % (name, shape, relu, skip), g, w64, w32)
            assert torch.equal(g, a), name                                   # in place and out of place agree bit for bit
        assert int(got[5]) == 8 and int(again[5]) == 8


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_two_calls_give_the_same_bits():
    case = Case(BC.ragged_shape(partials), 402)
    a, b = case.call(True, True), case.call(True, True)
    for name, x, y in zip(NAMES + ("num_batches_tracked",), a, b):
        assert torch.equal(x, y), name


# ------------------------------------------------------------------------------------------------ 3. a large offset
def test_offset_keeps_the_variance():
    shape = (1, 8, 4, 16, 16)
    y = 1000.0 + 0.01 * torch.randn(shape, generator=torch.Generator().manual_seed(403))
    case = Case(shape, 404, y=y)
    out, mean, var, rm, rv, _ = case.call(relu=False)
    r64, r32 = case.reference(torch.float64, False, False), case.reference(torch.float32, False, False)
    assert 0.5e-4 < float(r64[2].min()) and float(r64[2].max()) < 2e-4
    held("saved_var at offset 1000", var, r64[2], r32[2])
    held("saved_mean at offset 1000", mean, r64[1], r32[1])
    held("running_var at offset 1000", rv, r64[4], r32[4])
    assert float(var.min()) >= 0.0 and bool(torch.isfinite(out).all())
    held("out at offset 1000", out, r64[0], r32[0])


# ------------------------------------------------------------------------------------------------ 4. an exactly constant channel
def test_constant_channel_is_exact():
    shape = BC.ragged_shape(partials)
    case = Case(shape, 405)
    case.y[:, 1] = 2.5
    out, mean, var, rm, rv, _ = case.call(relu=False)
    assert float(mean[1]) == 2.5 and float(var[1]) == 0.0
    assert torch.equal(out[:, 1].cpu(), case.beta[1].expand(shape[0], shape[2]))     # fma(0, s, beta) = beta, bit for bit
    want_rm = (1 - torch.tensor(BC.MOMENTUM)) * case.rm[1] + torch.tensor(BC.MOMENTUM) * 2.5
    assert float(rm[1].cpu()) == float(want_rm)
    assert float(rv[1].cpu()) == float((1 - torch.tensor(BC.MOMENTUM)) * case.rv[1])


# ------------------------------------------------------------------------------------------------ 5. poisoned workspace, guarded outputs
def test_poisoned_workspace_and_guard_elements():
    from uc_nerf_amd import _lib as L
    shape = BC.ragged_shape(partials)
    n, Ch, S_ = shape
    P = partials(n, S_)
    case = Case(shape, 406)
    nan, sentinel = float("nan"), -12345.0
    y = case.y.to(DEV)
    ws = torch.full((Ch * P * 3 + 3,), nan, dtype=torch.float64, device=DEV)
    ws[-3:] = sentinel
    out = torch.full((y.numel() + 1,), nan, device=DEV)
    out[-1] = sentinel
    small = {k: torch.full((Ch + 1,), sentinel, device=DEV) for k in ("saved_mean", "saved_var", "running_mean", "running_var")}
    small["saved_mean"][:Ch], small["saved_var"][:Ch] = nan, nan
    small["running_mean"][:Ch], small["running_var"][:Ch] = case.rm.to(DEV), case.rv.to(DEV)
    nbt = torch.tensor([3, -777], dtype=torch.int64, device=DEV)
    gamma, beta, skip = case.gamma.to(DEV), case.beta.to(DEV), case.skip.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    s = L.BnStatsParams()
    s.n, s.C, s.S, s.workspace_triples, s.y, s.workspace = n, Ch, S_, Ch * P, y.data_ptr(), ws.data_ptr()
    L.call("ucnerf_bn_stats", s, stream)
    a = L.BnApplyParams()
    a.n, a.C, a.S, a.workspace_triples, a.eps, a.momentum, a.relu = n, Ch, S_, Ch * P, BC.EPS, BC.MOMENTUM, 1
    a.y, a.workspace, a.weight, a.bias, a.skip, a.out = y.data_ptr(), ws.data_ptr(), gamma.data_ptr(), beta.data_ptr(), skip.data_ptr(), out.data_ptr()
    a.saved_mean, a.saved_var = small["saved_mean"].data_ptr(), small["saved_var"].data_ptr()
    a.running_mean, a.running_var, a.num_batches_tracked = small["running_mean"].data_ptr(), small["running_var"].data_ptr(), nbt.data_ptr()
    L.call("ucnerf_bn_apply", a, stream)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ws[:-3]).any()) and bool((ws[-3:] == sentinel).all())
    counts = ws[:-3].view(Ch, P, 3)[:, :, 0].cpu()
    assert bool((counts.sum(1) == n * S_).all()) and bool((counts > 0).all()) and bool((counts[:, -1] < counts[:, 0]).all())
    assert not bool(torch.isnan(out[:-1]).any()) and float(out[-1]) == sentinel
    for k, t in small.items():
        assert not bool(torch.isnan(t[:Ch]).any()) and float(t[Ch]) == sentinel, k
    assert nbt.tolist() == [4, -777]
    r64, r32 = case.reference(torch.float64, True, True), case.reference(torch.float32, True, True)
    held("out through the raw entry points", out[:-1].view(shape), r64[0], r32[0])


# ------------------------------------------------------------------------------------------------ 6. the modules
def module_pair(build, seed):
    """The same randomised module twice, in train mode on the device: batch_stats="device" and batch_stats="torch"."""
    dev, ref = BC.randomise_train(build("device"), seed).to(DEV), BC.randomise_train(build("torch"), seed).to(DEV)
    assert dev.training and ref.training and dev.batch_stats == "device" and ref.batch_stats == "torch"
    return dev, ref


def held_state(module, other, s64, s32):
    """Every running statistic of `module` against the restatement's update, and against the same module's other route."""
    theirs = other.state_dict()
    for k, v in module.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 == int(s64[k]) == int(theirs[k]), k
        elif "running_" in k:
            agree(k, v, theirs[k], held(k, v, s64[k], s32[k]))


@pytest.mark.parametrize("shape", ((1, 8, 8, 16, 16), (1, 8, 8, 16, 24), (2, 8, 16, 16, 16)), ids=str)
def test_cost_reg_net_train_route_against_float64(shape):
    dev, ref = module_pair(lambda b: M().CostRegNet(8, 8, batch_stats=b), 411)
    before = {k: v.detach().cpu().clone() for k, v in dev.state_dict().items()}
    x = torch.rand(shape, generator=torch.Generator().manual_seed(412))
    with torch.no_grad():
        cost, prob = dev(x.to(DEV))
        cost_t, prob_t = ref(x.to(DEV))
    c64, p64, s64 = BC.cost_reg_net(x, before, torch.float64)
    c32, p32, s32 = BC.cost_reg_net(x, before, torch.float32)
    agree("cost %s" % (shape,), cost, cost_t, held("cost %s" % (shape,), cost, c64, c32))
    agree("prob %s" % (shape,), prob, prob_t, held("prob %s" % (shape,), prob, p64, p32))
    held_state(dev, ref, s64, s32)


def test_feature_net_train_route_against_float64():
    dev, ref = module_pair(lambda b: M().FeatureNet(8, batch_stats=b), 413)
    before = {k: v.detach().cpu().clone() for k, v in dev.state_dict().items()}
    x = torch.rand((1, 3, 16, 24), generator=torch.Generator().manual_seed(414))
    with torch.no_grad():
        got, got_t = dev(x.to(DEV)), ref(x.to(DEV))
    r64, s64 = BC.feature_net(x, before, torch.float64)
    r32, s32 = BC.feature_net(x, before, torch.float32)
    assert sorted(got) == ["stage1", "stage2", "stage3"]
    for k in sorted(got):
        agree(k, got[k], got_t[k], held(k, got[k], r64[k], r32[k]))
    held_state(dev, ref, s64, s32)


# ------------------------------------------------------------------------------------------------ 7. routes, by call count
@pytest.fixture
def calls(monkeypatch):
    o, n = ops(), {"conv": 0, "bn": 0, "pack": 0}

    def counted(name, key):
        real = getattr(o, name)

        def f(*a, **k):
            n[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(o, name, f)

    counted("conv3d", "conv")
    counted("conv2d_bias_relu", "conv")
    counted("batch_norm_train", "bn")
    counted("conv3d_pack", "pack")
    return n


def test_routes_by_call_count(calls):
    x3 = torch.rand((1, 8, 8, 16, 16), generator=torch.Generator().manual_seed(421)).to(DEV)
    x2 = torch.rand((1, 3, 16, 24), generator=torch.Generator().manual_seed(422)).to(DEV)
    reg = BC.randomise_train(M().CostRegNet(8, 8, batch_stats="device"), 423).to(DEV)
    feat = BC.randomise_train(M().FeatureNet(8, batch_stats="device"), 424).to(DEV)

    def count(f):
        calls["conv"], calls["bn"] = 0, 0
        out = f()
        return out, calls["conv"], calls["bn"]

    with torch.no_grad():
        (cost, prob), nc, nb = count(lambda: reg(x3))
    assert (nc, nb) == (11, 10) and cost.grad_fn is None and prob.grad_fn is None
    with torch.no_grad():
        out, nc, nb = count(lambda: feat(x2))
    assert (nc, nb) == (13, 8) and all(v.grad_fn is None for v in out.values())
    (cost, prob), nc, nb = count(lambda: reg(x3))                               # grad enabled: torch's layers
    assert (nc, nb) == (0, 0) and cost.grad_fn is not None and prob.grad_fn is not None
    out, nc, nb = count(lambda: feat(x2))
    assert (nc, nb) == (0, 0) and all(v.grad_fn is not None for v in out.values())
    reg.eval()
    with torch.no_grad():
        _, nc, nb = count(lambda: reg(x3))                                      # eval(): the folded route
    assert (nc, nb) == (11, 0)
    plain = BC.randomise_train(M().CostRegNet(8, 8), 423).to(DEV)                # the default keyword: torch's layers in train mode
    with torch.no_grad():
        _, nc, nb = count(lambda: plain(x3))
    assert (nc, nb) == (0, 0)
    reg.train()
    reg.conv3.bn.momentum = None                                               # a cumulative average is not built: torch's route
    with torch.no_grad():
        _, nc, nb = count(lambda: reg(x3))
    assert (nc, nb) == (0, 0)
    reg.conv3.bn.momentum = 0.1
    small = torch.rand((1, 8, 8, 8, 8), generator=torch.Generator().manual_seed(425)).to(DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        reg(small)
    with torch.no_grad(), pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        plain(small)


# ------------------------------------------------------------------------------------------------ 8. the two caches
def test_fold_sees_the_moved_statistics_and_raw_weights_pack_once(calls):
    reg = BC.randomise_train(M().CostRegNet(8, 8, batch_stats="device"), 431).to(DEV)
    x = torch.rand((1, 8, 8, 16, 16), generator=torch.Generator().manual_seed(432))
    reg.eval()
    with torch.no_grad():
        reg(x.to(DEV))                                                          # the fold of the statistics as they are now is cached
    reg.train()
    with torch.no_grad():
        reg(x.to(DEV))                                                          # moves them through raw pointers
    assert calls["pack"] == 22
    sd = {k: v.detach().cpu().clone() for k, v in reg.state_dict().items()}
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    reg.eval()
    with torch.no_grad():
        cost, prob = reg(x.to(DEV))
    assert calls["pack"] == 33                                                  # folded again: the buffers' versions moved
    c64, p64 = MC.cost_reg_net(x, sd, torch.float64)
    c32, p32 = MC.cost_reg_net(x, sd, torch.float32)
    held("eval cost after a train-mode forward", cost, c64, c32)
    held("eval prob after a train-mode forward", prob, p64, p32)
    reg.train()
    with torch.no_grad():
        reg(x.to(DEV))
        reg(x.to(DEV))
    assert calls["pack"] == 33                                                  # the raw weights were packed once, three forwards ago
    with torch.no_grad():
        reg.conv2.conv.weight.mul_(2)
        reg(x.to(DEV))
    assert calls["pack"] == 44


# ------------------------------------------------------------------------------------------------ 9. end to end
@pytest.fixture(scope="module")
def cascade_net():
    net = M().CascadeMVSNet.with_cnns(ndepths=[48, 32, 8], batch_stats="device")
    for i, module in enumerate([net.feature] + list(net.cost_regularization)):
        MC.randomise(module, 95 + i)
    return net.to(DEV)


@pytest.mark.parametrize("pad", (0, 4))
def test_cascade_with_cnns_train_mode_end_to_end(cascade_net, pad):
    V, H, W, ndepths = 3, 32, 32, [48, 32, 8]
    g = torch.Generator().manual_seed(99)
    imgs = torch.rand(1, V, 3, H, W, generator=g).to(DEV)
    affine, affine_inv = (t.to(DEV) for t in S.cameras(V, H, W, seed=100))
    near_far = torch.tensor([2.0, 11.0], device=DEV)
    cascade_net.eval()
    with torch.no_grad():
        want = S.outputs_listing(cascade_net(imgs, affine, affine_inv, near_far, pad=pad)[3])
    cascade_net.train()
    before = {k: v.detach().cpu().clone() for k, v in cascade_net.cost_regularization[0].state_dict().items()}
    seen = []
    hook = cascade_net.cost_regularization[0].register_forward_hook(lambda m, inp, out: seen.append((inp[0].clone(), out[1].clone())))
    try:
        with torch.no_grad():
            vol, conf, depth, outputs = cascade_net(imgs, affine, affine_inv, near_far, pad=pad)
    finally:
        hook.remove()
    assert S.outputs_listing(outputs) == want
    assert vol is outputs["stage3"]["volume_feature_no_ref"] and depth.shape == (1, H, W) and conf.shape == (1, H, W)
    for k, v in outputs.items():
        for kk, t in (v.items() if isinstance(v, dict) else ((k, v),)):
            assert bool(torch.isfinite(t).all()), (k, kk)
    assert float(depth.min()) >= 2.0 and float(depth.max()) <= 11.0
    (variance, prob), = seen
    assert variance.shape == (1, 32, 48, H // 4, W // 4) and prob.shape == (1, 1, 48, H // 4, W // 4)
    held("stage-1 logits", prob, BC.cost_reg_net(variance, before, torch.float64)[1], BC.cost_reg_net(variance, before, torch.float32)[1])


# ------------------------------------------------------------------------------------------------ 9. the ungrouped entry points are G = 1
# Nothing in Python launches the four ungrouped entry points any more (ops.batch_norm_train fills the grouped structs for every G), so they are
# called here through ctypes and held bit for bit to the `_groups` entry points at G = 1 on the same inputs.
RAW_CASES = (((2, 3, 7), False),                                           # scalar quads with a ragged tail
             ((1, 4, 4352), False),                                        # two partials on the vector path
             ((3, 2, 4100), False),                                        # four partials on the vector path, an image boundary inside a slice
             ((2, 3, 8), True))                                            # a vector-eligible S on a base one float past 16-byte alignment: the scalar walk


def _guarded(rows, width):
    """`rows` float64 rows of `width` inside a NaN-filled buffer, one guard row on either side -> (the buffer, the address of the first row)."""
    buf = torch.full(((rows + 2) * width,), float("nan"), dtype=torch.float64, device=DEV)
    return buf, buf.data_ptr() + 8 * width


def _guards_held(buf, width):
    return bool(torch.isnan(buf[:width]).all()) and bool(torch.isnan(buf[-width:]).all()) and not bool(torch.isnan(buf[width:-width]).any())


def _placed(t, misaligned):
    """t on the device; `misaligned`: at a base address one float past a 16-byte boundary."""
    if not misaligned:
        return t.to(DEV)
    view = torch.empty(t.numel() + 4, device=DEV)[1:1 + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == 4
    return view.copy_(t)


def _raw_entries(grouped, case, grad, relu, skip, misaligned):
    """The four launches through the ungrouped or the grouped (G = 1) entry points, workspaces sized exactly -> every result by name."""
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd.ops._core import _launch
    n, Ch, S_ = case.shape
    P = partials(n, S_)

    def launch(kind):
        p = getattr(L, kind + ("GroupsParams" if grouped else "Params"))()
        if grouped:
            p.G = 1
        p.n, p.C, p.S = n, Ch, S_
        return p, lambda symbol: _launch(symbol + ("_groups" if grouped else ""), p, DEV)

    y, g, sk = _placed(case.y, misaligned), _placed(grad, misaligned), case.skip.to(DEV) if skip else None
    gamma, beta = case.gamma.to(DEV), case.beta.to(DEV)
    res = {"out": torch.empty(case.shape, device=DEV), "saved_mean": torch.empty(Ch, device=DEV), "saved_var": torch.empty(Ch, device=DEV),
           "running_mean": case.rm.to(DEV), "running_var": case.rv.to(DEV), "num_batches_tracked": torch.tensor(7, dtype=torch.int64, device=DEV),
           "grad_y": torch.empty(case.shape, device=DEV), "grad_weight": torch.empty(Ch, device=DEV), "grad_bias": torch.empty(Ch, device=DEV)}
    triples, triples_at = _guarded(Ch * P, 3)
    s, go = launch("BnStats")
    s.workspace_triples, s.y, s.workspace = Ch * P, y.data_ptr(), triples_at
    go("ucnerf_bn_stats")
    a, go = launch("BnApply")
    a.workspace_triples, a.eps, a.momentum, a.relu = Ch * P, BC.EPS, BC.MOMENTUM, int(relu)
    a.y, a.workspace, a.weight, a.bias, a.skip = y.data_ptr(), triples_at, gamma.data_ptr(), beta.data_ptr(), 0 if sk is None else sk.data_ptr()
    for name in ("out", "saved_mean", "saved_var", "running_mean", "running_var", "num_batches_tracked"):
        setattr(a, name, res[name].data_ptr())
    go("ucnerf_bn_apply")
    pairs, pairs_at = _guarded(Ch * P, 2)
    for kind, symbol in (("BnBwdReduce", "ucnerf_bn_bwd_reduce"), ("BnBwdApply", "ucnerf_bn_bwd_apply")):
        q, go = launch(kind)
        q.workspace_pairs, q.eps, q.relu, q.g, q.y, q.workspace = Ch * P, BC.EPS, int(relu), g.data_ptr(), y.data_ptr(), pairs_at
        q.saved_mean, q.saved_var, q.weight, q.bias = res["saved_mean"].data_ptr(), res["saved_var"].data_ptr(), gamma.data_ptr(), beta.data_ptr()
        if kind == "BnBwdApply":
            q.grad_y, q.grad_weight, q.grad_bias = res["grad_y"].data_ptr(), res["grad_weight"].data_ptr(), res["grad_bias"].data_ptr()
        go(symbol)
    torch.cuda.synchronize()
    assert _guards_held(triples, 3) and _guards_held(pairs, 2), "a workspace of exactly C P rows was overrun or not filled"
    return res


@pytest.mark.parametrize("shape,misaligned", RAW_CASES, ids=str)
def test_ungrouped_entry_points_are_the_grouped_ones_at_one_group(shape, misaligned):
    assert partials(2, 7) == 1 and partials(1, 4352) == 2 and partials(3, 4100) == 4 and partials(2, 8) == 1
    case = Case(shape, 421)
    grad = torch.randn(shape, generator=torch.Generator().manual_seed(422))
    for relu, skip in itertools.product((True, False), (False, True)):
        plain, grouped = (_raw_entries(way, case, grad, relu, skip, misaligned) for way in (False, True))
        for name, t in plain.items():
            assert torch.equal(t, grouped[name]) and not bool(torch.isnan(t).any()), (name, relu, skip)
        assert int(plain["num_batches_tracked"]) == 8
