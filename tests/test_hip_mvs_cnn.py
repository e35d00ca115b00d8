"""FeatureNet and CostRegNet on the GPU: the device route (ucnerf_conv3d / ucnerf_conv2d_bias_relu with the batch-norms folded in) against the
float64 restatement of tests/mvs_cnn_cases.py and against the golden outputs of the reference's real modules, the folded-weight cache, the choice
of route, and CascadeMVSNet.with_cnns end to end.

The bar is the project's chain rule: 4 x the float32 CPU restatement's own largest distance from float64, at least one float32 spacing of the
largest value.  Every comparison prints the device's error, the float32 restatement's error and their ratio."""
import pytest
import torch

import cascade_stubs as S
import mvs_cnn_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def M():
    from uc_nerf_amd.network import mvs_models
    return mvs_models


def held(name, got, ref64, cpu32):
    bar, err32 = MC.chain_bar(ref64, cpu32)
    err = float((got.detach().cpu().double() - ref64).abs().max())
    print("%s: device %.3g, float32 cpu %.3g, ratio %.2f, bar %.3g, largest %.3g" % (name, err, err32, err / max(err32, 1e-30), bar, float(ref64.abs().max())))
    assert got.shape == ref64.shape and got.dtype == torch.float32
    assert err <= bar, name


def run_device(module, x):
    assert module.inference == "device" and not module.training
    with torch.no_grad():
        return module(x.to(DEV))


@pytest.fixture(scope="module")
def golden_modules():
    feat, reg = M().FeatureNet(base_channels=2), M().CostRegNet(in_channels=4, base_channels=2)
    feat.load_state_dict(MC.golden_state("feature."), strict=True)
    reg.load_state_dict(MC.golden_state("reg."), strict=True)
    return feat.to(DEV).eval(), reg.to(DEV).eval()


@pytest.fixture(scope="module")
def reg8():
    return MC.randomise(M().CostRegNet(8, 8), 81).to(DEV)


def volume(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ 1. the device route against float64
@pytest.mark.parametrize("shape", ((1, 8, 8, 8, 8), (1, 8, 8, 16, 24)))
def test_cost_reg_net_device_route_against_float64(reg8, shape):
    x = volume(shape, 82)
    cost, prob = run_device(reg8, x)
    sd = reg8.state_dict()
    c64, p64 = MC.cost_reg_net(x, sd, torch.float64)
    c32, p32 = MC.cost_reg_net(x, sd, torch.float32)
    held("cost %s" % (shape,), cost, c64, c32)
    held("prob %s" % (shape,), prob, p64, p32)


def test_feature_net_device_route_against_float64():
    feat = MC.randomise(M().FeatureNet(8), 83).to(DEV)
    x = volume((1, 3, 16, 24), 84)
    got = run_device(feat, x)
    r64, r32 = MC.feature_net(x, feat.state_dict(), torch.float64), MC.feature_net(x, feat.state_dict(), torch.float32)
    assert sorted(got) == ["stage1", "stage2", "stage3"]
    assert [got[k].shape[1:] for k in sorted(got)] == [(32, 4, 6), (16, 8, 12), (8, 16, 24)]
    for k in sorted(got):
        held(k, got[k], r64[k], r32[k])


def test_golden_modules_device_route_against_float64_and_the_reference_s_outputs(golden_modules):
    feat, reg = golden_modules
    G = MC.golden()
    stages = run_device(feat, G["image"])
    cost, prob = run_device(reg, G["volume"])
    got = dict(stages, cost=cost, prob=prob)
    r64 = dict(MC.feature_net(G["image"], MC.golden_state("feature."), torch.float64))
    r32 = dict(MC.feature_net(G["image"], MC.golden_state("feature."), torch.float32))
    for d, dt in ((r64, torch.float64), (r32, torch.float32)):
        d["cost"], d["prob"] = MC.cost_reg_net(G["volume"], MC.golden_state("reg."), dt)
    for k in ("stage1", "stage2", "stage3", "cost", "prob"):
        held(k + " vs float64", got[k], r64[k], r32[k])
        bar, err32 = MC.chain_bar(r64[k], r32[k])
        err = float((got[k].cpu() - G[k]).abs().max())
        print("%s vs the reference's float32 output: %.3g, bar %.3g (the reference's own distance from float64 %.3g)"
              % (k, err, bar, float((G[k].double() - r64[k]).abs().max())))
        assert err <= bar, k


# ------------------------------------------------------------------------------------------------ 2. the cache
def test_cost_reg_net_cache_follows_in_place_changes_loads_and_moved_statistics():
    reg = MC.randomise(M().CostRegNet(8, 8), 85).to(DEV)
    x = volume((1, 8, 8, 16, 24), 86).to(DEV)

    def out():
        with torch.no_grad():
            cost, prob = reg(x)
        return torch.cat([cost.flatten(), prob.flatten()]).clone()

    def checked(before, what):
        now = out()
        sd = reg.state_dict()
        c64, p64 = MC.cost_reg_net(x, sd, torch.float64)
        c32, p32 = MC.cost_reg_net(x, sd, torch.float32)
        assert not torch.equal(now, before), what
        held("prob after " + what, now[c64.numel():].view(p64.shape), p64, p32)      # and it is the NEW weights' result, not just another one
        return now

    a = out()
    assert torch.equal(out(), a)                                         # two plain calls: the same bits, one fold
    made = reg._cache.value
    assert reg._cache.get(reg, lambda: None) is made
    with torch.no_grad():
        reg.conv1.conv.weight.mul_(2)
    b = checked(a, "weight.mul_(2)")
    reg.load_state_dict(MC.randomise(M().CostRegNet(8, 8), 87).state_dict())
    c = checked(b, "load_state_dict")
    before = reg.conv0.bn.running_mean.clone()
    reg.train()
    reg(4 * x + 1)                                                       # the torch route: moves every running statistic
    reg.eval()
    assert not torch.equal(reg.conv0.bn.running_mean, before)
    d = checked(c, "a train() forward")
    assert torch.equal(out(), d)


def test_feature_net_cache_follows_an_in_place_change():
    feat = MC.randomise(M().FeatureNet(2), 88).to(DEV)
    x = volume((1, 3, 16, 24), 89).to(DEV)
    with torch.no_grad():
        a = feat(x)["stage3"].clone()
        assert torch.equal(feat(x)["stage3"], a)
        feat.conv0[0].bn.weight.mul_(2)
        b = feat(x)["stage3"]
    assert not torch.equal(a, b)
    held("stage3 after bn.weight.mul_(2)", b, MC.feature_net(x, feat.state_dict(), torch.float64)["stage3"], MC.feature_net(x, feat.state_dict(), torch.float32)["stage3"])


# ------------------------------------------------------------------------------------------------ 3. the routes
def test_routes(monkeypatch, reg8):
    from uc_nerf_amd import ops
    calls = {"conv3d": 0, "conv2d": 0}
    real3, real2 = ops.conv3d, ops.conv2d_bias_relu
    monkeypatch.setattr(ops, "conv3d", lambda *a, **k: (calls.__setitem__("conv3d", calls["conv3d"] + 1), real3(*a, **k))[1])
    monkeypatch.setattr(ops, "conv2d_bias_relu", lambda *a, **k: (calls.__setitem__("conv2d", calls["conv2d"] + 1), real2(*a, **k))[1])
    x = volume((1, 8, 8, 8, 8), 90).to(DEV)
    with torch.no_grad():
        cost, prob = reg8(x)
    assert calls["conv3d"] == 11 and cost.grad_fn is None                # eleven launches, the skip additions inside them
    cost, prob = reg8(x)                                                 # grad enabled: torch's layers
    assert calls["conv3d"] == 11 and cost.grad_fn is not None and prob.grad_fn is not None
    as_torch = M().CostRegNet(8, 8, inference="torch").to(DEV).eval()
    as_torch.load_state_dict(reg8.state_dict())
    with torch.no_grad():
        cost_t, prob_t = as_torch(x)
        cost_d, prob_d = reg8(x)
    assert calls["conv3d"] == 22                                         # none from the torch module
    c64, p64 = MC.cost_reg_net(x, reg8.state_dict(), torch.float64)
    c32, p32 = MC.cost_reg_net(x, reg8.state_dict(), torch.float32)
    held("inference=torch prob", prob_t, p64, p32)
    with torch.no_grad():
        assert reg8(x.cpu().to(DEV))[0].grad_fn is None
        cpu_module = M().CostRegNet(8, 8).eval()
        cpu_module(x.cpu())                                              # a host input under eval() + no_grad: torch's layers, no launch
    assert calls["conv3d"] == 33
    feat = MC.randomise(M().FeatureNet(2), 91).to(DEV)
    img = volume((1, 3, 16, 24), 92).to(DEV)
    with torch.no_grad():
        feat(img)
    assert calls["conv2d"] == 13
    assert feat(img)["stage1"].grad_fn is not None and calls["conv2d"] == 13
    feat.inference = "torch"
    with torch.no_grad():
        feat(img)
    assert calls["conv2d"] == 13
    with torch.no_grad(), pytest.raises(RuntimeError, match="divisible by 8"):
        reg8(volume((1, 8, 8, 12, 8), 93).to(DEV))
    with torch.no_grad(), pytest.raises(RuntimeError, match="divisible by 4"):
        feat.inference = "device"
        feat(volume((1, 3, 16, 22), 94).to(DEV))


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def cascade_net():
    net = M().CascadeMVSNet.with_cnns(ndepths=[48, 32, 8])
    for i, module in enumerate([net.feature] + list(net.cost_regularization)):
        MC.randomise(module, 95 + i)
    return net.to(DEV).eval()


@pytest.mark.parametrize("pad", (0, 4))
def test_cascade_with_cnns_end_to_end(cascade_net, pad):
    V, H, W, ndepths = 3, 32, 32, [48, 32, 8]
    g = torch.Generator().manual_seed(99)
    imgs = torch.rand(1, V, 3, H, W, generator=g).to(DEV)
    affine, affine_inv = (t.to(DEV) for t in S.cameras(V, H, W, seed=100))
    near_far = torch.tensor([2.0, 11.0], device=DEV)
    seen = []
    hook = cascade_net.cost_regularization[0].register_forward_hook(lambda m, inp, out: seen.append((inp[0].clone(), out[1].clone())))
    try:
        with torch.no_grad():
            vol, conf, depth, outputs = cascade_net(imgs, affine, affine_inv, near_far, pad=pad)
    finally:
        hook.remove()
    # the keys and shapes the stub-CNN net gives (test_hip_cascade.py), but for the feature channels: the stubs' maps have 8 at every stage
    logits = [torch.zeros(s) for s in S.stage_logit_shapes(H, W, ndepths, pad)]
    feature, regs = S.make_stubs(V, H, W, logits)
    stub_net = M().CascadeMVSNet(ndepths=ndepths, feature=feature, cost_regularization=regs).to(DEV).eval()
    with torch.no_grad():
        _, _, _, stub_out = stub_net(imgs, affine, affine_inv, near_far, pad=pad)
    want = S.outputs_listing(stub_out)
    for k, c in (("stage1", 32), ("stage2", 16)):
        want = [r.replace("%s/img_feats:3,1,8," % k, "%s/img_feats:3,1,%d," % (k, c)) for r in want]
    assert S.outputs_listing(outputs) == want
    assert vol is outputs["stage3"]["volume_feature_no_ref"] and depth.shape == (1, H, W) and conf.shape == (1, H, W)
    assert vol.shape == (1, 8, 8, H + 2 * pad, W + 2 * pad)
    for k, v in outputs.items():
        for kk, t in (v.items() if isinstance(v, dict) else ((k, v),)):
            assert bool(torch.isfinite(t).all()), (k, kk)
    assert float(depth.min()) >= 2.0 and float(depth.max()) <= 11.0
    # stage 1: the logits are the regulariser of the kernel's own variance volume
    (variance, prob), = seen
    assert variance.shape == (1, 32, 48, H // 4, W // 4) and prob.shape == (1, 1, 48, H // 4, W // 4)
    sd = cascade_net.cost_regularization[0].state_dict()
    held("stage-1 logits", prob, MC.cost_reg_net(variance, sd, torch.float64)[1], MC.cost_reg_net(variance, sd, torch.float32)[1])
