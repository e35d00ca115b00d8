"""Host-side checks of FeatureNet's training route (no GPU): the new symbols and structs, the workspace query against the documented chunk formula,
every argument check of the new entry points through ctypes (they come before anything is launched), the keywords, the route's fall-through on
CPU inputs, the differentiable restatement of tests/feature_train_cases.py against torch's own layers in float64, and the ReLU-side condition of
the seeds the GPU module tests use."""
import ctypes as C
import inspect
import itertools
import os

import pytest
import torch

import bn_cases as BC
import feature_train_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_STRUCTS = {"ucnerf_conv2d_wgrad_params": 8 * 4 + 8 + 4 * 8, "ucnerf_conv2d_dgrad_s2_params": 6 * 4 + 3 * 8, "ucnerf_conv2d_bias_grad_params": 4 * 4 + 2 * 8}
NEW_SYMBOLS = ("ucnerf_conv2d_wgrad_workspace_floats", "ucnerf_conv2d_wgrad", "ucnerf_conv2d_dgrad_s2", "ucnerf_conv2d_bias_grad")


def M():
    from uc_nerf_amd.network import mvs_models
    return mvs_models


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


def test_new_structs_and_symbols_are_registered_and_the_abi_stays_at_6(L):
    from uc_nerf_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    for name, size in NEW_STRUCTS.items():
        assert L.lib().ucnerf_sizeof(name.encode()) == size == C.sizeof(L.ADDED_STRUCTS[name]), name
        assert "struct %s {" % name in hdr and name not in L.STRUCTS
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in L.SYMBOLS and name + "(" in hdr, name
    assert "conv2d_bwd.hip" in SOURCES
    from uc_nerf_amd import ops
    from uc_nerf_amd.ops import cnn
    for name in ("conv2d_wgrad", "conv2d_dgrad", "conv2d_dgrad_pack", "conv2d_bias_grad", "conv2d_bn_train", "conv2d_train"):
        assert getattr(ops, name) is getattr(cnn, name), name


# ------------------------------------------------------------------------------------------------ the workspace query
def test_workspace_query_follows_the_documented_chunking(L):
    f = L.lib().ucnerf_conv2d_wgrad_workspace_floats
    grid = itertools.product((1, 2), (1, 3, 8, 16, 33), (1, 8, 32, 33), ((1, 1), (3, 1), (3, 2), (5, 1), (5, 2)), (1, 4, 6, 48, 65, 256), (1, 4, 5, 12, 80, 150, 320))
    for n, cin, cout, (K, stride), H, W in grid:
        chunks = FC.documented_chunks(n, cin, cout, K, stride, H, W)[0]
        assert f(n, cin, cout, H, W, K, stride, (K - 1) // 2) == chunks * cout * cin * K * K, (n, cin, cout, K, stride, H, W)
    # FeatureNet(8) at 256 x 320: a chunk is one output row for every layer but the deepest, whose 64 rows over 2 channel groups make 64 chunks too
    assert FC.documented_chunks(1, 3, 8, 3, 1, 256, 320) == (256, 1, 1) and FC.documented_chunks(1, 8, 16, 5, 2, 256, 320) == (128, 1, 1)
    assert FC.documented_chunks(1, 32, 32, 3, 1, 64, 80) == (64, 1, 1)
    assert FC.documented_chunks(*FC.WGRAD_MORE[3])[:2] == (260, 2) and FC.documented_chunks(*FC.WGRAD_MORE[2]) == (5, 32, 32)
    assert f(0, 8, 8, 4, 4, 3, 1, 1) == 0                                       # n == 0: nothing to hold
    for bad in ((-1, 8, 8, 4, 4, 3, 1, 1), (1, 0, 8, 4, 4, 3, 1, 1), (1, 8, 0, 4, 4, 3, 1, 1), (1, 8, 8, 0, 4, 3, 1, 1), (1, 8, 8, 4, -1, 3, 1, 1),
                (1, 8, 8, 4, 4, 2, 1, 0), (1, 8, 8, 4, 4, 7, 1, 3), (1, 8, 8, 4, 4, 0, 1, 0), (1, 8, 8, 4, 4, 3, 3, 1), (1, 8, 8, 4, 4, 3, 0, 1),
                (1, 8, 8, 4, 4, 1, 2, 0), (1, 8, 8, 4, 4, 3, 1, 0), (1, 8, 8, 4, 4, 5, 2, 1), (1, 8, 8, 4, 4, 3, 1, -1), (1, 1 << 17, 8, 4, 4, 3, 1, 1),
                (4, 64, 8, 1 << 12, 1 << 12, 3, 1, 1)):
        assert f(*bad) == -1 and L.lib().ucnerf_last_error().decode(), bad


# ------------------------------------------------------------------------------------------------ argument checks before any device call
def _wgrad_params(L, **kw):
    p = L.Conv2dWgradParams()
    base = dict(n=1, cin=8, H=8, W=8, cout=8, K=3, stride=1, pad=1)
    base.update({k: v for k, v in kw.items() if k != "workspace_floats"})
    for k, v in base.items():
        setattr(p, k, v)
    q = L.lib().ucnerf_conv2d_wgrad_workspace_floats(p.n, p.cin, p.cout, p.H, p.W, p.K, p.stride, p.pad)
    p.workspace_floats = kw.get("workspace_floats", q)
    return p


def test_wgrad_refuses_bad_arguments_before_any_device_call(L):
    lib = L.lib()
    assert lib.ucnerf_conv2d_wgrad(None, None) == -1 and "null" in lib.ucnerf_last_error().decode()
    p = _wgrad_params(L, n=0)                                            # n == 0: success with every pointer NULL
    assert p.workspace_floats == 0 and lib.ucnerf_conv2d_wgrad(C.addressof(p), None) == 0
    p = _wgrad_params(L, n=-1, workspace_floats=0)
    assert lib.ucnerf_conv2d_wgrad(C.addressof(p), None) == -1 and "negative" in lib.ucnerf_last_error().decode()
    p = _wgrad_params(L)                                                 # NULL arrays
    assert lib.ucnerf_conv2d_wgrad(C.addressof(p), None) == -1 and "null" in lib.ucnerf_last_error().decode()
    for field, bad in (("cin", 0), ("cout", -2), ("H", 0), ("W", -3), ("K", 0), ("K", 2), ("K", 7), ("stride", 0), ("stride", 3), ("pad", 0), ("pad", 2), ("pad", -1)):
        q = _wgrad_params(L, workspace_floats=8 * 8 * 9)
        setattr(q, field, bad)
        assert lib.ucnerf_conv2d_wgrad(C.addressof(q), None) == -1 and lib.ucnerf_last_error().decode(), (field, bad)
    q = _wgrad_params(L, K=1, pad=0, stride=2, workspace_floats=1)       # a strided 1 x 1 is no layer of the network
    assert lib.ucnerf_conv2d_wgrad(C.addressof(q), None) == -1 and "stride" in lib.ucnerf_last_error().decode()
    for off in (-1, 1):                                                  # a workspace of another size
        q = _wgrad_params(L)
        q.workspace_floats += off
        assert lib.ucnerf_conv2d_wgrad(C.addressof(q), None) == -1 and "workspace" in lib.ucnerf_last_error().decode()
    q = _wgrad_params(L, n=4, cin=64, H=1 << 12, W=1 << 12, workspace_floats=1)
    assert lib.ucnerf_conv2d_wgrad(C.addressof(q), None) == -1 and "too large" in lib.ucnerf_last_error().decode()


def test_dgrad_and_bias_grad_refuse_bad_arguments_before_any_device_call(L):
    lib = L.lib()
    one = C.c_float(0)
    addr = C.addressof(one)                                              # a non-null host address: never dereferenced by a check

    def dgrad(**kw):
        p = L.Conv2dDgradS2Params()
        p.n, p.cin, p.H, p.W, p.cout, p.K, p.grad_y, p.weight, p.grad_x = 1, 8, 8, 8, 16, 5, addr, addr, addr
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ucnerf_conv2d_dgrad_s2(C.addressof(p), None), lib.ucnerf_last_error().decode()

    assert lib.ucnerf_conv2d_dgrad_s2(None, None) == -1 and "null" in lib.ucnerf_last_error().decode()
    assert dgrad(n=0, grad_y=None, weight=None, grad_x=None)[0] == 0
    for kw, word in ((dict(n=-1), "negative"), (dict(cin=0), "cin"), (dict(cout=0), "cout"), (dict(H=0), "at least 1"), (dict(W=-2), "at least 1"),
                     (dict(K=1), "K="), (dict(K=4), "K="), (dict(K=7), "K="), (dict(H=7), "even"), (dict(W=5), "even"), (dict(n=16384), "too large"),
                     (dict(H=1 << 14, W=1 << 14), "too large"), (dict(grad_y=None), "null"), (dict(weight=None), "null"), (dict(grad_x=None), "null")):
        rc, msg = dgrad(**kw)
        assert rc == -1 and word in msg, (kw, msg)

    def bias(**kw):
        p = L.Conv2dBiasGradParams()
        p.n, p.cout, p.OH, p.OW, p.grad_y, p.grad_bias = 1, 8, 4, 4, addr, addr
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ucnerf_conv2d_bias_grad(C.addressof(p), None), lib.ucnerf_last_error().decode()

    assert lib.ucnerf_conv2d_bias_grad(None, None) == -1 and "null" in lib.ucnerf_last_error().decode()
    assert bias(n=0, grad_y=None, grad_bias=None)[0] == 0
    for kw, word in ((dict(n=-1), "negative"), (dict(cout=0), "at least 1"), (dict(OH=0), "at least 1"), (dict(OW=-1), "at least 1"),
                     (dict(n=8, cout=1 << 10, OH=1 << 10, OW=1 << 10), "too large"), (dict(grad_y=None), "null"), (dict(grad_bias=None), "null")):
        rc, msg = bias(**kw)
        assert rc == -1 and word in msg, (kw, msg)


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from uc_nerf_amd import ops
    z = torch.zeros
    for call in (lambda: ops.conv2d_wgrad(z(1, 8, 4, 4), z(1, 8, 4, 4), 3), lambda: ops.conv2d_bias_grad(z(1, 8, 4, 4)),
                 lambda: ops.conv2d_bn_train(z(1, 8, 4, 4), z(8, 8, 3, 3), z(8), z(8), z(8), z(8), z(1, dtype=torch.int64)),
                 lambda: ops.conv2d_train(z(1, 8, 4, 4), z(8, 8, 1, 1)), lambda: ops.conv2d_dgrad(z(1, 8, 4, 4), z(8, 8, 3, 3), (1, 8, 4, 4))):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()
    with pytest.raises(RuntimeError, match="even H, W"):
        ops.conv2d_dgrad(z(1, 8, 3, 4), z(8, 4, 5, 5), (1, 4, 5, 8), stride=2)
    with pytest.raises(RuntimeError, match="x_shape"):
        ops.conv2d_dgrad(z(1, 8, 4, 4), z(8, 4, 3, 3), (1, 4, 4))
    for w, kw in ((z(8, 4, 3, 3), dict(stride=3)), (z(8, 4, 3, 3), dict(pad=0)), (z(8, 4, 1, 1), dict(stride=2)), (z(8, 4, 4, 4), {})):
        with pytest.raises(RuntimeError, match="conv2d_dgrad"):
            ops.conv2d_dgrad_pack(w, **kw)


# ------------------------------------------------------------------------------------------------ the keywords
def test_training_keyword_is_checked_and_handed_down():
    for bad in ("bogus", None, True, "Device"):
        with pytest.raises(ValueError, match="training="):
            M().FeatureNet(8, training=bad)
        with pytest.raises(ValueError, match="training="):
            M().CascadeMVSNet.with_cnns(feature_training=bad)
    assert M().FeatureNet(8, training="device").training_route == "device"
    assert getattr(M().FeatureNet(8), "training_route", "torch") == "torch"
    sig = inspect.signature(M().CascadeMVSNet.with_cnns).parameters
    assert sig["training"].default == "torch" == sig["feature_training"].default and sig["inference"].default == "device" and sig["batch_stats"].default == "torch"
    assert inspect.signature(M().FeatureNet.__init__).parameters["training"].default == "torch"
    net = M().CascadeMVSNet.with_cnns(feature_training="device")
    assert net.feature.training_route == "device" and all(r.training_route == "torch" for r in net.cost_regularization)
    net = M().CascadeMVSNet.with_cnns(training="device")                   # `training=` keeps meaning the CostRegNets only
    assert getattr(net.feature, "training_route", "torch") == "torch" and all(r.training_route == "device" for r in net.cost_regularization)


def test_default_keyword_and_cpu_inputs_take_torch_layers_with_the_same_values(monkeypatch):
    from uc_nerf_amd import ops
    calls = []
    for name in ("conv2d_bn_train", "conv2d_train"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    case = FC.MODULE_CASES[1]
    x, R = FC.module_inputs(case)
    dev, ref = (BC.randomise_train(M().FeatureNet(8, **kw), case[1]) for kw in (dict(training="device"), {}))
    outs = []
    for m in (dev, ref):
        o = m(x)
        assert all(v.grad_fn is not None for v in o.values())
        sum((o[k] * R[k]).sum() for k in o).backward()
        outs.append(o)
    assert not calls
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
    for (k, a), (_, b) in zip(dev.named_parameters(), ref.named_parameters()):
        assert torch.equal(a.grad, b.grad), k
    for (k, a), (_, b) in zip(dev.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ the restatement against torch's layers
def test_restatement_gradients_agree_with_torch_layers_in_float64():
    case = FC.MODULE_CASES[0]
    x, R = FC.module_inputs(case)
    m = BC.randomise_train(M().FeatureNet(8), case[1])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.double()
    X = x.double().requires_grad_(True)
    outs = m(X)
    sum((outs[k] * R[k].double()).sum() for k in outs).backward()
    r = FC.feature_net(x, sd, torch.float64, R)
    pairs = [(k, r["out"][k], outs[k].detach()) for k in outs] + [("grad_x", r["grad_x"], X.grad)]
    grads = dict(m.named_parameters())
    assert len(grads) == 31 and set(grads) == set(r["grads"])
    pairs += [(k, r["grads"][k], p.grad) for k, p in grads.items()]
    for k, got, want in pairs:
        rel = float((got - want).abs().max() / want.abs().max())
        assert rel <= 1e-10, (k, rel)
    g = torch.Generator().manual_seed(702)
    for K, stride in ((3, 1), (5, 2)):                                     # one layer against nn.Conv2d + nn.BatchNorm2d
        conv, bn = torch.nn.Conv2d(3, 5, K, stride=stride, padding=(K - 1) // 2, bias=False).double(), torch.nn.BatchNorm2d(5).double().train()
        with torch.no_grad():
            bn.weight.copy_(0.6 + 0.8 * torch.rand(5, generator=g))
            bn.bias.copy_(0.3 * torch.randn(5, generator=g))
        xx = torch.randn((2, 3, 6, 8), generator=g, dtype=torch.float64, requires_grad=True)
        out = torch.relu(bn(conv(xx)))
        go = torch.randn(out.shape, generator=g, dtype=torch.float64)
        out.backward(go)
        rr = FC.layer_grads(xx, conv.weight, bn.weight, bn.bias, go, torch.float64, stride)
        for key, want in (("out", out.detach()), ("x", xx.grad), ("w", conv.weight.grad), ("gamma", bn.weight.grad), ("beta", bn.bias.grad)):
            assert float((rr[key] - want).abs().max() / want.abs().max()) <= 1e-11, (K, key)


@pytest.mark.parametrize("index", range(len(FC.MODULE_CASES)))
def test_no_relu_of_the_module_cases_sits_within_the_chain_bar_of_zero(index):
    case = FC.MODULE_CASES[index]
    x, R = FC.module_inputs(case)
    m = BC.randomise_train(M().FeatureNet(8), case[1])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    r64, r32 = FC.feature_net(x, sd, torch.float64), FC.feature_net(x, sd, torch.float32)
    bad = FC.relu_offenders(r64, r32)
    smallest = min(float(v.abs().min()) for v in r64["z"].values())
    print("case %s: smallest |z| = %.3g over %d values" % (case, smallest, sum(v.numel() for v in r64["z"].values())))
    assert not bad, bad[:5]
