"""Host-side checks of the batch-statistic batch-norm (csrc/bn.hip, ops.batch_norm_train, the modules' batch_stats keyword).  No GPU: the
binding, the size query, every argument check of the two entry points (all made before any device call), the wrapper's refusals, the keyword,
the CPU fall-through of the route and the restatement of tests/bn_cases.py against torch's own layer."""
import ctypes as C

import pytest
import torch

import bn_cases as BC


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


def M():
    from uc_nerf_amd.network import mvs_models
    return mvs_models


def test_symbols_and_structs_are_registered_and_the_abi_is_still_6(L):
    assert L.ABI_VERSION == 6 and L.lib().ucnerf_abi_version() == 6
    for name in ("ucnerf_bn_partials", "ucnerf_bn_stats", "ucnerf_bn_apply"):
        assert name in L.SYMBOLS
    for cname, cls in (("ucnerf_bn_stats_params", L.BnStatsParams), ("ucnerf_bn_apply_params", L.BnApplyParams)):
        assert L.ADDED_STRUCTS[cname] is cls and L.lib().ucnerf_sizeof(cname.encode()) == C.sizeof(cls)


def test_partials_positive_non_decreasing_and_negative_on_bad_input(L):
    f = L.lib().ucnerf_bn_partials
    last = 0
    for N in list(range(2, 64)) + list(range(4000, 4200)) + [8191, 8192, 8193, 100000, 131071, 131072, 131073, 10 ** 6, 10 ** 8, 2 ** 31 - 2 ** 20]:
        P = f(1, N)
        assert P >= max(last, 1), (N, P, last)
        assert f(2, N // 2) == f(1, N // 2 * 2) or N < 4                 # a function of n S alone
        last = P
    assert f(1, 4096) == 1 and f(1, 4097) == 2 and f(3, 3000) == 3 and f(1, 10 ** 8) == 32
    for n, S in ((0, 8), (8, 0), (-1, 8), (8, -1), (1, 1), (1, 2 ** 31), (2 ** 31, 1), (2 ** 20, 2 ** 20), (2 ** 62, 2 ** 62)):
        assert f(n, S) < 0, (n, S)


FAKE = 0x1000          # a non-null address: every case below fails a check before anything could read it


def _stats(L, **kw):
    p = L.BnStatsParams()
    p.n, p.C, p.S, p.workspace_triples, p.y, p.workspace = 1, 8, 64, 8, FAKE, FAKE
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _apply(L, **kw):
    p = L.BnApplyParams()
    p.n, p.C, p.S, p.workspace_triples, p.eps, p.momentum, p.relu = 1, 8, 64, 8, 1e-5, 0.1, 1
    for name in ("y", "workspace", "weight", "bias", "out", "saved_mean", "saved_var", "running_mean", "running_var", "num_batches_tracked"):
        setattr(p, name, FAKE)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


SHAPE_ERRORS = (dict(n=0), dict(n=-1), dict(C=0), dict(C=-3), dict(S=0), dict(S=-1), dict(S=1), dict(n=2 ** 31), dict(S=2 ** 31), dict(n=2 ** 20, S=2 ** 20),
                dict(n=2 ** 62, S=2 ** 62), dict(C=65536), dict(C=2 ** 62), dict(workspace_triples=7), dict(workspace_triples=-1),
                dict(S=8192, workspace_triples=8), dict(y=0), dict(workspace=0), dict(workspace=FAKE + 4))


@pytest.mark.parametrize("bad", SHAPE_ERRORS, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_stats_refuses_bad_arguments_without_a_device(L, bad):
    rc = L.lib().ucnerf_bn_stats(C.addressof(_stats(L, **bad)), None)
    assert rc == -1 and b"bn_stats" in L.lib().ucnerf_last_error()


APPLY_ERRORS = SHAPE_ERRORS + (dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan")), dict(momentum=0.0), dict(momentum=-0.1), dict(momentum=1.5),
                               dict(momentum=float("nan")), dict(weight=0), dict(bias=0), dict(out=0), dict(saved_mean=0), dict(saved_var=0),
                               dict(running_mean=0), dict(running_var=0), dict(num_batches_tracked=0), dict(num_batches_tracked=FAKE + 4))


@pytest.mark.parametrize("bad", APPLY_ERRORS, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_apply_refuses_bad_arguments_without_a_device(L, bad):
    rc = L.lib().ucnerf_bn_apply(C.addressof(_apply(L, **bad)), None)
    assert rc == -1 and b"bn_apply" in L.lib().ucnerf_last_error()


def test_null_params_are_refused(L):
    assert L.lib().ucnerf_bn_stats(None, None) == -1 and L.lib().ucnerf_bn_apply(None, None) == -1


def test_wrapper_refuses_host_tensors_and_raises_torchs_error_at_one_value():
    from uc_nerf_amd import ops
    C_ = 4
    args = [torch.ones(C_), torch.zeros(C_), torch.zeros(C_), torch.ones(C_), torch.zeros((), dtype=torch.int64)]
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.batch_norm_train(torch.zeros(1, C_, 2, 2, 2), *args)
    with pytest.raises(RuntimeError, match="batch_norm_train"):
        ops.batch_norm_train(torch.zeros(C_), *args)                      # no channel dimension
    with pytest.raises(RuntimeError, match="batch_norm_train"):
        ops.batch_norm_train([1.0, 2.0], *args)
    want = None
    try:
        torch.nn.BatchNorm3d(C_).train()(torch.zeros(1, C_, 1, 1, 1))
    except ValueError as e:
        want = str(e)
    assert want is not None and want.startswith("Expected more than 1 value per channel when training")
    with pytest.raises(ValueError) as got:
        ops.batch_norm_train(torch.zeros(1, C_, 1, 1, 1), *args)
    assert str(got.value) == want
    assert int(args[4]) == 0 and torch.equal(args[2], torch.zeros(C_))       # refused before anything moved


def test_batch_stats_keyword():
    m = M()
    assert m.FeatureNet(2).batch_stats == "torch" and m.CostRegNet(4, 2).batch_stats == "torch"
    assert m.FeatureNet(2, batch_stats="device").batch_stats == "device" and m.CostRegNet(4, 2, batch_stats="device").batch_stats == "device"
    net = m.CascadeMVSNet.with_cnns(batch_stats="device")
    assert net.feature.batch_stats == "device" and all(r.batch_stats == "device" for r in net.cost_regularization)
    assert all(r.batch_stats == "torch" for r in m.CascadeMVSNet.with_cnns().cost_regularization)
    for build in (lambda: m.FeatureNet(2, batch_stats="nope"), lambda: m.CostRegNet(4, 2, batch_stats="nope"),
                  lambda: m.CascadeMVSNet.with_cnns(batch_stats="nope"), lambda: m.CostRegNet(4, 2, batch_stats=None)):
        with pytest.raises(ValueError, match="batch_stats"):
            build()


def _held(name, got, ref64, cpu32):
    bar, err32 = BC.chain_bar(ref64, cpu32)
    err = float((got.detach().cpu().double() - ref64).abs().max())
    print("%s: module %.3g, float32 restatement %.3g, ratio %.2f, bar %.3g" % (name, err, err32, err / max(err32, 1e-30), bar))
    assert err <= bar, name


def test_cpu_module_in_train_mode_takes_torchs_route_and_matches_the_restatement(monkeypatch):
    from uc_nerf_amd import ops
    m = M()

    def never(*a, **k):
        raise AssertionError("a device op was called for a CPU input")

    for name in ("conv3d", "conv2d_bias_relu", "batch_norm_train"):
        monkeypatch.setattr(ops, name, never)
    reg = BC.randomise_train(m.CostRegNet(8, 4, batch_stats="device"), 301)
    before = {k: v.clone() for k, v in reg.state_dict().items()}
    x = torch.rand((1, 8, 8, 16, 16), generator=torch.Generator().manual_seed(302))
    with torch.no_grad():
        cost, prob = reg(x)
    c64, p64, s64 = BC.cost_reg_net(x, before, torch.float64)
    c32, p32, s32 = BC.cost_reg_net(x, before, torch.float32)
    _held("cost", cost, c64, c32)
    _held("prob", prob, p64, p32)
    after = reg.state_dict()
    for k in sorted(after):
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(before[k]) + 1 == int(s64[k])
        elif "running_" in k:
            _held(k, after[k], s64[k], s32[k])
    feat = BC.randomise_train(m.FeatureNet(4, batch_stats="device"), 303)
    before = {k: v.clone() for k, v in feat.state_dict().items()}
    x = torch.rand((1, 3, 16, 24), generator=torch.Generator().manual_seed(304))
    with torch.no_grad():
        got = feat(x)
    r64, s64 = BC.feature_net(x, before, torch.float64)
    r32, s32 = BC.feature_net(x, before, torch.float32)
    for k in sorted(got):
        _held(k, got[k], r64[k], r32[k])
    for k, v in feat.state_dict().items():
        if "running_" in k:
            _held(k, v, s64[k], s32[k])


@pytest.mark.parametrize("relu", (True, False))
def test_restatement_agrees_with_torchs_layer(relu):
    g = torch.Generator().manual_seed(305)
    y = torch.randn((2, 5, 3, 4, 5), generator=g, dtype=torch.float64) * 2 + 1
    bn = torch.nn.BatchNorm3d(5, momentum=BC.MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(5, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(5, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(5, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(5, generator=g, dtype=torch.float64) + 0.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    with torch.no_grad():
        want = bn(y)
        want = torch.relu(want) if relu else want
    out, mean, var = BC.bn_train(y, bn.weight, bn.bias, torch.float64, relu=relu)
    new_rm, new_rv = BC.running_update(rm, rv, mean, var, 2 * 3 * 4 * 5, torch.float64)
    assert float((out - want).abs().max()) < 1e-13
    assert float((new_rm - bn.running_mean).abs().max()) < 1e-14 and float((new_rv - bn.running_var).abs().max()) < 1e-14
    assert int(bn.num_batches_tracked) == 1
