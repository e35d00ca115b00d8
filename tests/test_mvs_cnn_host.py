"""Host-side checks of the MVS CNN mirrors (no GPU): the key names and shapes against the reference's recorded ones, the torch route against the
golden outputs of the reference's real modules, the batch-norm fold, training through torch, the refusals, and the argument checks of the
conv3d entry points through ctypes (they come before anything is launched)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import mvs_cnn_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_STRUCTS = {"ucnerf_conv3d_pack_params": 4 * 4 + 2 * 8, "ucnerf_conv3d_params": 12 * 4 + 8 + 5 * 8}
NEW_SYMBOLS = ("ucnerf_conv3d_packed_floats", "ucnerf_conv3d_pack", "ucnerf_conv3d")


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


# ------------------------------------------------------------------------------------------------ names and shapes
def test_state_dict_keys_and_shapes_are_the_reference_s():
    rec = MC.recorded_keys()
    made = {"FeatureNet(8)": M().FeatureNet(8), "CostRegNet(32,8)": M().CostRegNet(32, 8), "CostRegNet(16,8)": M().CostRegNet(16, 8),
            "CostRegNet(8,8)": M().CostRegNet(8, 8)}
    assert sorted(rec) == sorted(made)
    for title, module in made.items():
        got = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
        assert got == rec[title], title                                  # (names, shapes and their order)
    assert M().FeatureNet(8).out_channels == [32, 16, 8]


def test_golden_state_dicts_load_strictly():
    feat, reg = M().FeatureNet(base_channels=2), M().CostRegNet(in_channels=4, base_channels=2)
    assert feat.load_state_dict(MC.golden_state("feature."), strict=True).missing_keys == []
    assert reg.load_state_dict(MC.golden_state("reg."), strict=True).missing_keys == []


def test_construction_prints_nothing(capsys):
    M().FeatureNet(8)
    M().CascadeMVSNet.with_cnns()
    assert capsys.readouterr().out == ""


# ------------------------------------------------------------------------------------------------ the torch route against the real modules
def test_torch_route_on_the_cpu_reproduces_the_reference_s_outputs():
    G = MC.golden()
    feat, reg = M().FeatureNet(base_channels=2).eval(), M().CostRegNet(in_channels=4, base_channels=2).eval()
    feat.load_state_dict(MC.golden_state("feature."))
    reg.load_state_dict(MC.golden_state("reg."))
    with torch.no_grad():
        stages = feat(G["image"])
        cost, prob = reg(G["volume"])
    got = dict(stages, cost=cost, prob=prob)
    # the restatement's own float32-vs-float64 error: the scale of what a second float32 evaluation of the same network may differ by
    r64 = dict(MC.feature_net(G["image"], MC.golden_state("feature."), torch.float64))
    r32 = dict(MC.feature_net(G["image"], MC.golden_state("feature."), torch.float32))
    for d, dt in ((r64, torch.float64), (r32, torch.float32)):
        d["cost"], d["prob"] = MC.cost_reg_net(G["volume"], MC.golden_state("reg."), dt)
    for k in ("stage1", "stage2", "stage3", "cost", "prob"):
        assert got[k].shape == G[k].shape and got[k].dtype == torch.float32
        err = float((got[k] - G[k]).abs().max())
        ulp4 = 4 * MC.spacing(G[k].abs().max())
        measured4 = 4 * float((r32[k].double() - r64[k]).abs().max())
        print("%s: |torch route - golden| = %.3g, 4 spacings = %.3g, 4 x the restatement's float32 error = %.3g" % (k, err, ulp4, measured4))
        assert err <= max(ulp4, measured4), k
        assert float((r64[k] - G[k].double()).abs().max()) <= max(ulp4, measured4), k      # the restatement itself states the reference's network


# ------------------------------------------------------------------------------------------------ the fold
def _fold_cases():
    m = M()
    yield "Conv2d", m.Conv2d(3, 5, 3, 1, padding=1), (2, 3, 6, 7), lambda x, w, b: F.conv2d(x, w, b, stride=1, padding=1)
    yield "Conv2d 5x5/2", m.Conv2d(4, 6, 5, stride=2, padding=2), (1, 4, 9, 8), lambda x, w, b: F.conv2d(x, w, b, stride=2, padding=2)
    yield "Conv3d", m.Conv3d(3, 4, padding=1), (1, 3, 4, 5, 6), lambda x, w, b: F.conv3d(x, w, b, stride=1, padding=1)
    yield "Conv3d /2", m.Conv3d(3, 4, stride=2, padding=1), (1, 3, 4, 5, 6), lambda x, w, b: F.conv3d(x, w, b, stride=2, padding=1)
    yield "Conv3d no bn", m.Conv3d(3, 4, bn=False, padding=1), (1, 3, 4, 5, 6), lambda x, w, b: F.conv3d(x, w, b, stride=1, padding=1)
    yield ("Deconv3d", m.Deconv3d(5, 3, stride=2, padding=1, output_padding=1), (1, 5, 2, 3, 4),
           lambda x, w, b: F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1))
    yield "bare conv with bias", torch.nn.Conv2d(4, 3, 1, bias=True), (1, 4, 3, 3), lambda x, w, b: F.conv2d(x, w, b)
    yield "bare conv without bias", torch.nn.Conv3d(4, 1, 3, padding=1, bias=False), (1, 4, 3, 3, 3), lambda x, w, b: F.conv3d(x, w, b, padding=1)


def test_fold_equals_conv_then_batch_norm_in_float64():
    for i, (name, layer, shape, conv) in enumerate(_fold_cases()):
        layer = MC.randomise(layer, 40 + i).double()
        x = torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(i))
        with torch.no_grad():
            want = layer(x)
            w, b = M().fold_conv_bn(layer, torch.float64)
            got = conv(x, w, b)
            if getattr(layer, "relu", False):
                got = F.relu(got)
        rel = float((got - want).abs().max() / want.abs().max())
        print("%s: %.3g" % (name, rel))
        assert want.abs().max() > 0 and rel <= 1e-12, name


# ------------------------------------------------------------------------------------------------ training goes through torch
@pytest.mark.parametrize("mode", ("train", "eval with grad"))
def test_training_mode_or_grad_enabled_takes_the_torch_route(mode):
    feat, reg = M().FeatureNet(base_channels=2), M().CostRegNet(in_channels=4, base_channels=2)
    for module in (feat, reg):
        module.train(mode == "train")
    G = MC.golden()
    stages = feat(G["image"].repeat(2, 1, 1, 1))
    cost, prob = reg(G["volume"].repeat(2, 1, 1, 1, 1))
    outs = list(stages.values()) + [cost, prob]
    assert all(o.grad_fn is not None for o in outs)
    sum(o.square().mean() for o in outs).backward()
    for module in (feat, reg):
        missing = [n for n, p in module.named_parameters() if p.grad is None or not bool(p.grad.abs().sum() > 0)]
        assert not missing, missing


# ------------------------------------------------------------------------------------------------ refusals
def test_unsupported_configurations_raise_and_name_what_is_supported():
    for kw in (dict(arch_mode="unet"), dict(num_stage=2)):
        with pytest.raises(NotImplementedError, match="fpn.*num_stage=3"):
            M().FeatureNet(**kw)
    with pytest.raises(ValueError, match="device"):
        M().FeatureNet(inference="miopen")
    with pytest.raises(ValueError, match="device"):
        M().CostRegNet(8, 8, inference=None)
    with pytest.raises(NotImplementedError):
        M().CascadeMVSNet.with_cnns(arch_mode="unet")
    with pytest.raises(NotImplementedError, match="share_cr"):
        M().CascadeMVSNet.with_cnns(share_cr=True)


def test_cascade_without_cnns_still_raises_and_with_cnns_registers_the_reference_s_keys():
    with pytest.raises(ValueError, match="feature=.*cost_regularization="):
        M().CascadeMVSNet()
    net = M().CascadeMVSNet.with_cnns()
    rec = MC.recorded_keys()
    want = ["feature." + k for k, _ in rec["FeatureNet(8)"]]
    for i, title in enumerate(("CostRegNet(32,8)", "CostRegNet(16,8)", "CostRegNet(8,8)")):
        want += ["cost_regularization.%d.%s" % (i, k) for k, _ in rec[title]]
    assert list(net.state_dict()) == want
    assert net.feature.inference == "device" and all(r.inference == "device" for r in net.cost_regularization)
    assert M().CascadeMVSNet.with_cnns(inference="torch").cost_regularization[2].inference == "torch"
    small = M().CascadeMVSNet.with_cnns(cr_base_chs=[4, 2, 8])
    assert small.cost_regularization[0].conv0.conv.weight.shape == (4, 32, 3, 3, 3) and small.cost_regularization[1].prob.weight.shape[1] == 2


def test_the_cache_compares_tensors_and_versions_never_addresses():
    import inspect
    src = inspect.getsource(M()._InferenceCache)
    assert "data_ptr" not in src and "_version" in src and " is not " in src
    lin = torch.nn.Linear(2, 2)
    cache, made = M()._InferenceCache(), []
    build = lambda: made.append(1) or len(made)                          # noqa: E731
    assert cache.get(lin, build) == 1 and cache.get(lin, build) == 1
    with torch.no_grad():
        lin.weight.mul_(2)
    assert cache.get(lin, build) == 2 and cache.get(lin, build) == 2
    lin.load_state_dict(torch.nn.Linear(2, 2).state_dict())
    assert cache.get(lin, build) == 3
    lin.bias = torch.nn.Parameter(lin.bias.detach().clone())            # another tensor with the same values and version 0
    assert cache.get(lin, build) == 4 and cache.get(lin, build) == 4
    assert all(a is b for a, b in zip(cache.sources, lin.parameters()))  # the cache holds what it was made from


# ------------------------------------------------------------------------------------------------ the library's argument checks
def test_new_structs_and_symbols_are_registered_and_the_abi_stays_at_6(L):
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    for name, size in NEW_STRUCTS.items():
        assert L.lib().ucnerf_sizeof(name.encode()) == size == C.sizeof(L.ADDED_STRUCTS[name]), name
        assert "struct %s {" % name in hdr and name not in L.STRUCTS
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in L.SYMBOLS and name + "(" in hdr, name


def test_packed_sizes(L):
    f = L.lib().ucnerf_conv3d_packed_floats
    # per class [channel tiles][k padded to 32][16 or 32 rows] + one tap code per padded k
    assert f(8, 8, 3, 0) == 224 * 16 + 224
    assert f(8, 1, 3, 0) == 224 * 16 + 224
    assert f(33, 65, 3, 0) == 3 * 896 * 32 + 896
    assert f(3, 5, 1, 0) == 32 * 16 + 32
    # transposed: 8 parity classes with 1, 2, 2, 4, 2, 4, 4, 8 live taps
    assert f(16, 8, 3, 1) == sum(-(-16 * t // 32) * 32 * 17 for t in (1, 2, 2, 4, 2, 4, 4, 8))
    assert f(64, 32, 3, 1) == sum(64 * t * 33 for t in (1, 2, 2, 4, 2, 4, 4, 8))
    for bad in ((0, 8, 3, 0), (8, 0, 3, 0), (8, 8, 2, 0), (8, 8, 5, 0), (8, 8, 1, 1), (8, 8, 3, 2), (-1, 8, 3, 0)):
        assert f(*bad) == -1 and L.lib().ucnerf_last_error().decode(), bad


def _conv_params(L, **kw):
    p = L.Conv3dParams()
    base = dict(n=1, cin=8, D=8, H=8, W=8, cout=8, K=3, stride=1, pad=1, relu=1, transposed=0)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    p.packed_floats = L.lib().ucnerf_conv3d_packed_floats(p.cin, p.cout, p.K, p.transposed) if "packed_floats" not in kw else kw["packed_floats"]
    return p


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(L):
    lib = L.lib()
    for fn in ("ucnerf_conv3d_pack", "ucnerf_conv3d"):
        assert getattr(lib, fn)(None, None) == -1 and "null" in lib.ucnerf_last_error().decode(), fn
    k = L.Conv3dPackParams()
    k.cin, k.cout, k.K, k.transposed = 8, 8, 3, 0
    assert lib.ucnerf_conv3d_pack(C.addressof(k), None) == -1 and "null" in lib.ucnerf_last_error().decode()
    for field, bad in (("cin", 0), ("cout", -1), ("K", 2), ("K", 0), ("transposed", 2)):
        k2 = L.Conv3dPackParams()
        k2.cin, k2.cout, k2.K, k2.transposed = 8, 8, 3, 0
        setattr(k2, field, bad)
        assert lib.ucnerf_conv3d_pack(C.addressof(k2), None) == -1, field
    k.K, k.transposed = 1, 1
    assert lib.ucnerf_conv3d_pack(C.addressof(k), None) == -1 and "transposed" in lib.ucnerf_last_error().decode()

    p = _conv_params(L, n=0)                                             # n == 0: success with every pointer NULL
    assert lib.ucnerf_conv3d(C.addressof(p), None) == 0
    p = _conv_params(L, n=-1)
    assert lib.ucnerf_conv3d(C.addressof(p), None) == -1 and "negative" in lib.ucnerf_last_error().decode()
    p = _conv_params(L)                                                  # NULL arrays
    assert lib.ucnerf_conv3d(C.addressof(p), None) == -1 and "null" in lib.ucnerf_last_error().decode()
    for field, bad in (("cin", 0), ("cout", 0), ("D", 0), ("H", -3), ("W", 0), ("K", 2), ("K", 5), ("stride", 0), ("stride", 3), ("pad", -1),
                       ("transposed", 2), ("transposed", -1)):
        q = _conv_params(L, packed_floats=224 * 17)
        setattr(q, field, bad)
        assert lib.ucnerf_conv3d(C.addressof(q), None) == -1 and lib.ucnerf_last_error().decode(), (field, bad)
    # the transposed form is K 3, stride 2, pad 1 and nothing else
    for kw in (dict(stride=1), dict(pad=0), dict(K=1, pad=0)):
        q = _conv_params(L, **dict(dict(transposed=1, stride=2, pad=1, packed_floats=1), **kw))
        assert lib.ucnerf_conv3d(C.addressof(q), None) == -1 and "transposed" in lib.ucnerf_last_error().decode(), kw
    # a packed buffer of the wrong size (here: packed for the forward form, used transposed; and off by one)
    q = _conv_params(L, transposed=1, stride=2, pad=1, packed_floats=224 * 17)
    assert lib.ucnerf_conv3d(C.addressof(q), None) == -1 and "packed" in lib.ucnerf_last_error().decode()
    q = _conv_params(L, packed_floats=224 * 17 + 1)
    assert lib.ucnerf_conv3d(C.addressof(q), None) == -1 and "packed" in lib.ucnerf_last_error().decode()
    q = _conv_params(L, D=2, H=2, W=2, pad=0)                            # smaller than the kernel
    assert lib.ucnerf_conv3d(C.addressof(q), None) == -1 and "smaller" in lib.ucnerf_last_error().decode()
    q = _conv_params(L, n=4, cin=64, D=512, H=512, W=512, packed_floats=lib.ucnerf_conv3d_packed_floats(64, 8, 3, 0))      # 32-bit index limits
    assert lib.ucnerf_conv3d(C.addressof(q), None) == -1 and "too large" in lib.ucnerf_last_error().decode()


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from uc_nerf_amd import ops
    from uc_nerf_amd.ops import cnn
    assert ops.conv3d is cnn.conv3d and ops.conv3d_pack is cnn.conv3d_pack and ops.PackedConv3d is cnn.PackedConv3d
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv3d_pack(torch.zeros(8, 8, 3, 3, 3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.conv3d(torch.zeros(1, 8, 4, 4, 4), cnn.PackedConv3d(torch.zeros(1), 8, 8, 3, False), torch.zeros(8))
