"""Host-side checks of CostRegNet's training route (no GPU): the new symbols and structs, every argument check of the new entry points through
ctypes (they come before anything is launched) and the workspace query, the wrappers' refusals, the route's fall-through on CPU inputs, the
differentiable restatement of tests/cnn_train_cases.py against torch's own layers in float64, and the ReLU-side condition of the seeds the GPU
module tests use."""
import ctypes as C
import os

import pytest
import torch

import bn_cases as BC
import cnn_train_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_STRUCTS = {"ucnerf_conv3d_wgrad_params": 10 * 4 + 8 + 4 * 8, "ucnerf_bn_bwd_reduce_params": 4 * 8 + 2 * 4 + 7 * 8,
               "ucnerf_bn_bwd_apply_params": 4 * 8 + 2 * 4 + 10 * 8}
NEW_SYMBOLS = ("ucnerf_conv3d_wgrad_workspace_floats", "ucnerf_conv3d_wgrad", "ucnerf_bn_bwd_reduce", "ucnerf_bn_bwd_apply")


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


# ------------------------------------------------------------------------------------------------ declared, exported, bound
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
    assert "conv3d_bwd.hip" in SOURCES
    from uc_nerf_amd import ops
    from uc_nerf_amd.ops import cnn
    for name in ("conv3d_wgrad", "conv3d_dgrad", "conv3d_dgrad_pack", "batch_norm_train_bwd", "conv3d_bn_train", "conv3d_train"):
        assert getattr(ops, name) is getattr(cnn, name), name


# ------------------------------------------------------------------------------------------------ the workspace query
def chunks(L, n, cin, cout, stride, D, H, W, transposed=0, pad=1):
    floats = L.lib().ucnerf_conv3d_wgrad_workspace_floats(n, cin, cout, D, H, W, 3, stride, pad, transposed)
    assert floats > 0 and floats % (cin * cout * 27) == 0
    return floats // (cin * cout * 27)


def documented_chunks(V, Ca, Cb):
    tiles = -(-Ca // 16) * -(-Cb // 16)
    c0 = min(-(-V // 32), max(1, -(-512 // tiles)))
    length = 32 * -(-V // (32 * c0))
    return -(-V // length), length


def test_workspace_query_follows_the_documented_chunking(L):
    # conv0 at stage 2 (16 -> 8, 655 360 voxels): all the parallelism from the chunks; conv6 at stage 3 (64 -> 64, 1 280 voxels): from the tiles
    assert chunks(L, 1, 16, 8, 1, 32, 128, 160) == 512 == documented_chunks(655360, 8, 16)[0]
    assert chunks(L, 1, 64, 64, 1, 8, 8, 20) == 20 and documented_chunks(1280, 64, 64) == (20, 64)
    for n, cin, cout, stride, D, H, W in TC.WGRAD_SHAPES:
        V = n * ((D - 1) // stride + 1) * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        assert chunks(L, n, cin, cout, stride, D, H, W) == documented_chunks(V, cout, cin)[0], (n, cin, cout, stride, D, H, W)
    for n, cin, cout, stride, D, H, W in TC.WGRAD_LONG_CHUNKS:                     # more than one 32-voxel round per chunk
        assert documented_chunks(n * D * H * W, cout, cin)[1] == 64 and chunks(L, n, cin, cout, stride, D, H, W) == n * D * H * W // 64
    for cin, cout, D, H, W in TC.WGRAD_TRANSPOSED:
        assert chunks(L, 2, cin, cout, 2, D, H, W, transposed=1) == documented_chunks(2 * D * H * W, cin, cout)[0]
    f = L.lib().ucnerf_conv3d_wgrad_workspace_floats
    assert f(0, 8, 8, 4, 4, 4, 3, 1, 1, 0) == 0                                   # n == 0: nothing to hold
    for bad in ((-1, 8, 8, 4, 4, 4, 3, 1, 1, 0), (1, 0, 8, 4, 4, 4, 3, 1, 1, 0), (1, 8, 0, 4, 4, 4, 3, 1, 1, 0), (1, 8, 8, 0, 4, 4, 3, 1, 1, 0),
                (1, 8, 8, 4, 4, 4, 1, 1, 0, 0), (1, 8, 8, 4, 4, 4, 5, 1, 2, 0), (1, 8, 8, 4, 4, 4, 3, 3, 1, 0), (1, 8, 8, 4, 4, 4, 3, 0, 1, 0),
                (1, 8, 8, 4, 4, 4, 3, 1, -1, 0), (1, 8, 8, 4, 4, 4, 3, 1, 1, 2), (1, 8, 8, 4, 4, 4, 3, 1, 1, 1), (1, 8, 8, 4, 4, 4, 3, 2, 0, 1),
                (1, 8, 8, 2, 2, 2, 3, 1, 0, 0), (1, 1 << 17, 8, 4, 4, 4, 3, 1, 1, 0)):
        assert f(*bad) == -1 and L.lib().ucnerf_last_error().decode(), bad


# ------------------------------------------------------------------------------------------------ argument checks before any device call
def _wgrad_params(L, **kw):
    p = L.Conv3dWgradParams()
    base = dict(n=1, cin=8, D=8, H=8, W=8, cout=8, K=3, stride=1, pad=1, transposed=0)
    base.update({k: v for k, v in kw.items() if k != "workspace_floats"})
    for k, v in base.items():
        setattr(p, k, v)
    q = L.lib().ucnerf_conv3d_wgrad_workspace_floats(p.n, p.cin, p.cout, p.D, p.H, p.W, p.K, p.stride, p.pad, p.transposed)
    p.workspace_floats = kw.get("workspace_floats", q)
    return p


def test_wgrad_refuses_bad_arguments_before_any_device_call(L):
    lib = L.lib()
    assert lib.ucnerf_conv3d_wgrad(None, None) == -1 and "null" in lib.ucnerf_last_error().decode()
    p = _wgrad_params(L, n=0)                                            # n == 0: success with every pointer NULL
    assert p.workspace_floats == 0 and lib.ucnerf_conv3d_wgrad(C.addressof(p), None) == 0
    p = _wgrad_params(L, n=-1, workspace_floats=0)
    assert lib.ucnerf_conv3d_wgrad(C.addressof(p), None) == -1 and "negative" in lib.ucnerf_last_error().decode()
    p = _wgrad_params(L)                                                 # NULL arrays
    assert lib.ucnerf_conv3d_wgrad(C.addressof(p), None) == -1 and "null" in lib.ucnerf_last_error().decode()
    for field, bad in (("cin", 0), ("cout", -2), ("D", 0), ("H", -3), ("W", 0), ("K", 1), ("K", 2), ("K", 5), ("stride", 0), ("stride", 3), ("pad", -1),
                       ("pad", 65), ("transposed", 2), ("transposed", -1)):
        q = _wgrad_params(L, workspace_floats=8 * 8 * 27)
        setattr(q, field, bad)
        assert lib.ucnerf_conv3d_wgrad(C.addressof(q), None) == -1 and lib.ucnerf_last_error().decode(), (field, bad)
    for kw in (dict(stride=1), dict(pad=0)):                             # the transposed form is stride 2, pad 1 and nothing else
        q = _wgrad_params(L, workspace_floats=1, **dict(dict(transposed=1, stride=2, pad=1), **kw))
        assert lib.ucnerf_conv3d_wgrad(C.addressof(q), None) == -1 and "transposed" in lib.ucnerf_last_error().decode(), kw
    for off in (-1, 1):                                                  # a workspace of another size
        q = _wgrad_params(L)
        q.workspace_floats += off
        assert lib.ucnerf_conv3d_wgrad(C.addressof(q), None) == -1 and "workspace" in lib.ucnerf_last_error().decode()
    q = _wgrad_params(L, D=2, H=2, W=2, pad=0, workspace_floats=1)
    assert lib.ucnerf_conv3d_wgrad(C.addressof(q), None) == -1 and "smaller" in lib.ucnerf_last_error().decode()
    q = _wgrad_params(L, n=4, cin=64, D=512, H=512, W=512, workspace_floats=1)
    assert lib.ucnerf_conv3d_wgrad(C.addressof(q), None) == -1 and "too large" in lib.ucnerf_last_error().decode()


def test_bn_backward_refuses_bad_arguments_before_any_device_call(L):
    lib = L.lib()
    one = C.c_double(0)                                                  # a non-null, 8-byte aligned host address: never dereferenced by a check
    addr = C.addressof(one)
    for fn, cls, extra in (("ucnerf_bn_bwd_reduce", L.BnBwdReduceParams, ()), ("ucnerf_bn_bwd_apply", L.BnBwdApplyParams, ("grad_y", "grad_weight", "grad_bias"))):
        f = getattr(lib, fn)
        assert f(None, None) == -1 and "null" in lib.ucnerf_last_error().decode(), fn

        def make(**kw):
            p = cls()
            p.n, p.C, p.S, p.workspace_pairs, p.eps, p.relu = 2, 3, 5, 3, 1e-5, 1
            for name in ("g", "y", "saved_mean", "saved_var", "weight", "bias", "workspace") + extra:
                setattr(p, name, addr)
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        for kw, word in ((dict(n=0), "at least 1"), (dict(C=0), "at least 1"), (dict(S=-1), "at least 1"), (dict(n=1, S=1), "at least 2"),
                         (dict(S=1 << 31), "at most"), (dict(C=65536), "65535"), (dict(eps=0.0), "eps"), (dict(eps=float("nan")), "eps"),
                         (dict(workspace_pairs=2), "pairs"), (dict(workspace=addr + 4), "aligned"), (dict(g=None), "null"), (dict(y=None), "null"),
                         (dict(saved_mean=None), "null"), (dict(saved_var=None), "null"), (dict(weight=None), "null"), (dict(bias=None), "null"),
                         (dict(workspace=None), "null")) + tuple((dict([(name, None)]), "null") for name in extra):
            p = make(**kw)
            assert f(C.addressof(p), None) == -1 and word in lib.ucnerf_last_error().decode(), (fn, kw, lib.ucnerf_last_error().decode())


# ------------------------------------------------------------------------------------------------ the wrappers' refusals
def test_wrappers_refuse_host_tensors_bad_shapes_and_odd_stride_two():
    from uc_nerf_amd import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv3d_wgrad(z(1, 8, 4, 4, 4), z(1, 8, 4, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.batch_norm_train_bwd(z(1, 8, 4, 4, 4), z(1, 8, 4, 4, 4), z(8), z(8), z(8), z(8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv3d_bn_train(z(1, 8, 4, 4, 4), z(8, 8, 3, 3, 3), z(8), z(8), z(8), z(8), z(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv3d_train(z(1, 8, 4, 4, 4), z(1, 8, 3, 3, 3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv3d_dgrad(z(1, 8, 4, 4, 4), z(8, 8, 3, 3, 3), (1, 8, 4, 4, 4))
    # shapes, before anything touches a device
    with pytest.raises(RuntimeError, match="even D, H, W"):
        ops.conv3d_dgrad(z(1, 8, 3, 4, 5), z(8, 4, 3, 3, 3), (1, 4, 5, 7, 9), stride=2, pad=1)
    with pytest.raises(RuntimeError, match="even D, H, W"):
        ops.conv3d_dgrad(z(1, 8, 2, 4, 4), z(8, 4, 3, 3, 3), (1, 4, 4, 8, 7), stride=2)
    with pytest.raises(RuntimeError, match="grad_y must be"):
        ops.conv3d_dgrad(z(1, 8, 4, 4, 5), z(8, 4, 3, 3, 3), (1, 4, 4, 4, 4))
    with pytest.raises(RuntimeError, match="grad_y must be"):
        ops.conv3d_dgrad(z(1, 8, 4, 4, 4), z(4, 8, 3, 3, 3), (1, 4, 4, 4, 4), stride=2, pad=1, transposed=True)
    with pytest.raises(RuntimeError, match="x_shape"):
        ops.conv3d_dgrad(z(1, 8, 4, 4, 4), z(8, 4, 3, 3, 3), (1, 4, 4, 4))
    for kw in (dict(stride=3), dict(pad=0), dict(stride=1, pad=1, transposed=True)):
        with pytest.raises(RuntimeError, match="stride"):
            ops.conv3d_dgrad(z(1, 8, 4, 4, 4), z(8, 4, 3, 3, 3), (1, 4, 4, 4, 4), **kw)
    with pytest.raises(RuntimeError, match="3,3,3"):
        ops.conv3d_dgrad_pack(z(8, 4, 1, 1, 1))


def test_training_keyword_is_checked_and_handed_down():
    for bad in ("miopen", None, True, "Device"):
        with pytest.raises(ValueError, match="training="):
            M().CostRegNet(8, 8, training=bad)
        with pytest.raises(ValueError, match="training="):
            M().CascadeMVSNet.with_cnns(training=bad)
    assert M().CostRegNet(8, 8).training_route == "torch" and M().CostRegNet(8, 8, training="device").training_route == "device"
    net = M().CascadeMVSNet.with_cnns(training="device")
    assert all(r.training_route == "device" for r in net.cost_regularization) and not hasattr(net.feature, "training_route")
    assert all(r.training_route == "torch" for r in M().CascadeMVSNet.with_cnns().cost_regularization)
    assert M().TRAINING_ROUTES == ("torch", "device")


def test_route_falls_through_to_torch_on_cpu_inputs_with_the_same_values():
    case = TC.MODULE_CASES[0]
    x, R1, R2 = TC.module_inputs(case)
    dev, ref = (BC.randomise_train(M().CostRegNet(case[0], case[1], training=t), case[3]) for t in ("device", "torch"))
    outs = []
    for m in (dev, ref):
        cost, prob = m(x)
        assert cost.grad_fn is not None and prob.grad_fn is not None
        ((cost * R1).sum() + (prob * R2).sum()).backward()
        outs.append((cost, prob))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for (k, a), (_, b) in zip(dev.named_parameters(), ref.named_parameters()):
        assert torch.equal(a.grad, b.grad), k
    for (k, a), (_, b) in zip(dev.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ the restatement against torch's layers
def test_restatement_gradients_agree_with_torch_layers_in_float64():
    from torch import nn
    g = torch.Generator().manual_seed(701)
    for name, stride, transposed, shape in (("conv", 1, False, (2, 3, 4, 5, 6)), ("conv /2", 2, False, (1, 3, 4, 6, 8)), ("deconv", 2, True, (2, 3, 2, 3, 2))):
        cin, cout = shape[1], 5
        conv = (nn.ConvTranspose3d(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False) if transposed
                else nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False)).double()
        bn = nn.BatchNorm3d(cout).double().train()
        with torch.no_grad():
            bn.weight.copy_(0.6 + 0.8 * torch.rand(cout, generator=g))
            bn.bias.copy_(0.3 * torch.randn(cout, generator=g))
        x = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
        y = conv(x)
        skip = torch.randn(y.shape, generator=g, dtype=torch.float64, requires_grad=True)
        out = torch.relu(bn(y)) + skip
        grad_out = torch.randn(out.shape, generator=g, dtype=torch.float64)
        out.backward(grad_out)
        r = TC.layer_grads(x, conv.weight, bn.weight, bn.bias, grad_out, torch.float64, stride, transposed, True, skip)
        for key, want in (("out", out.detach()), ("x", x.grad), ("w", conv.weight.grad), ("gamma", bn.weight.grad), ("beta", bn.bias.grad), ("skip", skip.grad)):
            rel = float((r[key] - want).abs().max() / want.abs().max())
            print("%s %s: %.3g" % (name, key, rel))
            assert rel <= 1e-11, (name, key)
    # the whole network: the restatement against the module's torch route, both in float64
    case = TC.MODULE_CASES[0]
    x, R1, R2 = TC.module_inputs(case)
    m = BC.randomise_train(M().CostRegNet(case[0], case[1]), case[3])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.double()
    X = x.double().requires_grad_(True)
    cost, prob = m(X)
    ((cost * R1.double()).sum() + (prob * R2.double()).sum()).backward()
    r = TC.cost_reg_net(x, sd, torch.float64, R1, R2)
    pairs = [("cost", r["cost"], cost.detach()), ("prob", r["prob"], prob.detach()), ("grad_x", r["grad_x"], X.grad)]
    pairs += [(k, r["grads"][k], p.grad) for k, p in m.named_parameters()]
    for k, got, want in pairs:
        rel = float((got - want).abs().max() / want.abs().max())
        assert rel <= 1e-10, (k, rel)


# ------------------------------------------------------------------------------------------------ the ReLU-side condition of the GPU tests' seeds
@pytest.mark.parametrize("index", range(len(TC.MODULE_CASES)))
def test_no_relu_of_the_module_cases_sits_within_the_chain_bar_of_zero(index):
    case = TC.MODULE_CASES[index]
    x, R1, R2 = TC.module_inputs(case)
    m = BC.randomise_train(M().CostRegNet(case[0], case[1]), case[3])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    r64, r32 = TC.cost_reg_net(x, sd, torch.float64), TC.cost_reg_net(x, sd, torch.float32)
    bad = TC.relu_offenders(r64, r32, sd)
    smallest = min(float(r64["z"][n].abs().min()) for n in TC.ORDER)
    print("case %s: smallest |z| = %.3g over %d values" % (case, smallest, sum(r64["z"][n].numel() for n in TC.ORDER)))
    assert not bad, bad[:5]
