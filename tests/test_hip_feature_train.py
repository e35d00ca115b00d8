"""FeatureNet's training route on the GPU (csrc/conv2d_bwd.hip, ops.conv2d_bn_train / conv2d_train, training="device"): the 2-D weight gradient bit
for bit on integer lattices and one-hot inputs, its workspace and determinism, the input gradient of both strides, the bias gradient, the two
layer functions and the module against the float64 restatement of tests/feature_train_cases.py, the routes by call count and one training step
of the whole cascade.

The bar wherever a division or a square root is involved is the project's chain rule: 4 x the float32 CPU restatement's own largest distance
from float64, at least one float32 spacing of the largest value.  Every comparison prints the device's error, the float32 restatement's and
their ratio."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import bn_cases as BC
import cascade_stubs as S
import feature_train_cases as FC
import mvs_cnn_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
SHARES = []                                                                # device error / chain bar of every held() comparison of this run


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
    print("%s: device %.3g, float32 cpu %.3g, ratio %.2f, bar %.3g, share of the bar %.3f, largest %.3g"
          % (name, err, err32, err / max(err32, 1e-30), bar, err / bar, float(ref64.abs().max())))
    assert got.shape == ref64.shape and got.dtype == torch.float32
    assert err <= bar, name
    return bar


def cpu_wgrad(x, gy, K, stride):
    w = torch.zeros((gy.shape[1], x.shape[1], K, K), requires_grad=True)
    F.conv2d(x, w, None, stride=stride, padding=(K - 1) // 2).backward(gy)
    return w.grad


def ragged_shape():
    """The smallest (1, 8, 8, 3, 1, H, 5) with at least three chunks and a shorter last one, by the library's own workspace query (the chunks are
    cut along rows, so it is the height that is searched)."""
    f = lib().lib().ucnerf_conv2d_wgrad_workspace_floats
    H = 3
    while True:
        chunks = f(1, 8, 8, H, 5, 3, 1, 1) // (8 * 8 * 9)
        rows = FC.documented_chunks(1, 8, 8, 3, 1, H, 5)[1]
        if chunks >= 3 and 0 < H - (chunks - 1) * rows < rows:
            return (1, 8, 8, 3, 1, H, 5)
        H += 1


# ------------------------------------------------------------------------------------------------ 1. wgrad on integer lattices
@pytest.mark.parametrize("shape", FC.WGRAD_SHAPES + FC.WGRAD_MORE + ("ragged",), ids=str)
def test_wgrad_lattice_is_bit_equal_to_torch_cpu(shape):
    if shape == "ragged":
        shape = ragged_shape()
        assert shape[5] <= 128, shape
    n, cin, cout, K, stride, H, W = shape
    OH, OW = FC.out_hw(H, W, K, stride)
    x, gy = MC.lattice((n, cin, H, W), 4, 901), MC.lattice((n, cout, OH, OW), 4, 902)
    want = cpu_wgrad(x, gy, K, stride)
    assert 0 < float(want.abs().max()) and 16 * n * OH * OW < 2 ** 24
    got = ops().conv2d_wgrad(x.to(DEV), gy.to(DEV), K, stride)
    assert torch.equal(got.cpu(), want), shape


# ------------------------------------------------------------------------------------------------ 2. wgrad, one-hot
def window(x, img, base, K):
    """The K x K taps of x[img] [c,H,W] at base + (0..K-1)^2, +0 outside -> [c,K,K]."""
    c, H, W = x.shape[1:]
    out = torch.zeros(c, K, K)
    for ky, kx in itertools.product(range(K), repeat=2):
        h, w = base[0] + ky, base[1] + kx
        if 0 <= h < H and 0 <= w < W:
            out[:, ky, kx] = x[img, :, h, w]
    return out


@pytest.mark.parametrize("K,stride", ((3, 1), (5, 2), (5, 1), (3, 2), (1, 1)))
def test_wgrad_one_hot_reads_the_window(K, stride):
    n, cin, cout, H, W = 2, 5, 3, 6, 8
    x = torch.randn((n, cin, H, W), generator=torch.Generator().manual_seed(911))
    OH, OW = FC.out_hw(H, W, K, stride)
    pad = (K - 1) // 2
    # every corner (a window over two image edges at once), one pixel per edge and an interior one, in the second image too
    spots = list(itertools.product((0, OH - 1), (0, OW - 1))) + [(OH // 2, OW // 2), (0, 1), (1, 0), (OH - 1, 1), (1, OW - 1)]
    for k, (oy, ox) in enumerate(spots):
        img, co = k % n, k % cout
        gy = torch.zeros((n, cout, OH, OW))
        gy[img, co, oy, ox] = 1.0
        got = ops().conv2d_wgrad(x.to(DEV), gy.to(DEV), K, stride).cpu()
        want = torch.zeros(cout, cin, K, K)
        want[co] = window(x, img, (oy * stride - pad, ox * stride - pad), K)
        assert torch.equal(got, want), (K, stride, oy, ox)


# ------------------------------------------------------------------------------------------------ 3. wgrad: workspace, guards, determinism
def test_wgrad_writes_all_of_its_workspace_and_nothing_else_and_repeats_its_bits():
    L = lib()
    n, cin, cout, K, stride, H, W = 2, 8, 8, 3, 1, 40, 11
    x = torch.randn((n, cin, H, W), generator=torch.Generator().manual_seed(921)).to(DEV)
    gy = torch.randn((n, cout, H, W), generator=torch.Generator().manual_seed(922)).to(DEV)
    floats = L.lib().ucnerf_conv2d_wgrad_workspace_floats(n, cin, cout, H, W, K, stride, 1)
    assert floats // (cin * cout * K * K) >= 3
    nan, sentinel, guard = float("nan"), -12345.0, 64
    results = []
    for _ in range(2):
        ws = torch.full((floats + 2 * guard,), nan, device=DEV)
        ws[:guard], ws[-guard:] = sentinel, sentinel
        out = torch.full((cout * cin * K * K + 2 * guard,), nan, device=DEV)
        out[:guard], out[-guard:] = sentinel, sentinel
        p = L.Conv2dWgradParams()
        p.n, p.cin, p.H, p.W, p.cout, p.K, p.stride, p.pad, p.workspace_floats = n, cin, H, W, cout, K, stride, 1, floats
        p.x, p.grad_y, p.workspace, p.grad_weight = x.data_ptr(), gy.data_ptr(), ws[guard:].data_ptr(), out[guard:].data_ptr()
        L.call("ucnerf_conv2d_wgrad", p, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for t in (ws, out):
            assert bool((t[:guard] == sentinel).all()) and bool((t[-guard:] == sentinel).all()) and not bool(torch.isnan(t[guard:-guard]).any())
        results.append((ws.clone(), out.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert torch.equal(results[0][1][guard:-guard].view(cout, cin, K, K), ops().conv2d_wgrad(x, gy, K, stride))
    w64 = torch.zeros((cout, cin, K, K), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.cpu().double(), w64, padding=1).backward(gy.cpu().double())
    held("wgrad on random floats", results[0][1][guard:-guard].view(cout, cin, K, K), w64.grad, cpu_wgrad(x.cpu(), gy.cpu(), K, stride))


# ------------------------------------------------------------------------------------------------ 4. dgrad
def cpu_dgrad(gy, w, x_shape, stride):
    x = torch.zeros(x_shape, requires_grad=True)
    F.conv2d(x, w, stride=stride, padding=(w.shape[2] - 1) // 2).backward(gy)
    return x.grad


@pytest.mark.parametrize("shape", ((1, 8, 8, 3, 4, 6), (2, 5, 7, 3, 5, 9), (1, 16, 32, 1, 3, 5), (1, 33, 65, 1, 4, 4)), ids=str)
def test_dgrad_stride_one_lattice_is_bit_equal_to_torch_cpu(shape):
    n, cin, cout, K, H, W = shape
    w, gy = MC.lattice((cout, cin, K, K), 4, 931), MC.lattice((n, cout, H, W), 4, 932)
    want = cpu_dgrad(gy, w, (n, cin, H, W), 1)
    got = ops().conv2d_dgrad(gy.to(DEV), w.to(DEV), (n, cin, H, W), 1)
    assert float(want.abs().max()) > 0 and torch.equal(got.cpu(), want), shape
    packed = ops().conv2d_dgrad_pack(w.to(DEV), 1)
    assert torch.equal(ops().conv2d_dgrad(gy.to(DEV), packed, (n, cin, H, W), 1).cpu(), want)


@pytest.mark.parametrize("shape", FC.DGRAD_S2_SHAPES + ((1, 2, 40, 36, 40),), ids=str)
@pytest.mark.parametrize("K", (5, 3))
def test_dgrad_stride_two_lattice_is_bit_equal_to_torch_cpu(shape, K):
    n, cin, cout, H, W = shape
    w, gy = MC.lattice((cout, cin, K, K), 4, 933), MC.lattice((n, cout, H // 2, W // 2), 4, 934)
    want = cpu_dgrad(gy, w, (n, cin, H, W), 2)
    assert 0 < float(want.abs().max()) and 16 * cout * 9 < 2 ** 24
    got = ops().conv2d_dgrad(gy.to(DEV), w.to(DEV), (n, cin, H, W), 2)
    assert torch.equal(got.cpu(), want), shape
    packed = ops().conv2d_dgrad_pack(w.to(DEV), 2)
    assert torch.equal(ops().conv2d_dgrad(gy.to(DEV), packed, (n, cin, H, W), 2).cpu(), want)


def test_dgrad_one_hot_reads_out_the_unflipped_kernel_in_every_parity_class():
    cin, cout = 3, 4
    w = torch.randn((cout, cin, 3, 3), generator=torch.Generator().manual_seed(935))
    gy = torch.zeros((1, cout, 5, 5))
    gy[0, 2, 2, 2] = 1.0
    got = ops().conv2d_dgrad(gy.to(DEV), w.to(DEV), (1, cin, 5, 5), 1).cpu()
    assert torch.equal(got[0, :, 1:4, 1:4], w[2])                          # dx[ci, o - 1 + k] = w[co, ci, k]: the kernel itself, not its mirror image
    got[0, :, 1:4, 1:4] = 0
    assert not bool(got.any())
    # stride 2, K 5: a one-hot at (oy, ox) writes w[co] to rows 2 oy - 2 .. 2 oy + 2: all four parity classes, and at the last source pixel the
    # window reaches the last row and column, which only output_padding = 1 makes part of grad_x
    w5 = torch.randn((cout, cin, 5, 5), generator=torch.Generator().manual_seed(936))
    H, W = 8, 6
    for oy, ox in ((1, 1), (0, 0), (H // 2 - 1, W // 2 - 1), (0, W // 2 - 1)):
        gy = torch.zeros((1, cout, H // 2, W // 2))
        gy[0, 1, oy, ox] = 1.0
        got = ops().conv2d_dgrad(gy.to(DEV), w5.to(DEV), (1, cin, H, W), 2).cpu()
        want = torch.zeros((1, cin, H, W))
        for ky, kx in itertools.product(range(5), repeat=2):
            iy, ix = 2 * oy - 2 + ky, 2 * ox - 2 + kx
            if 0 <= iy < H and 0 <= ix < W:
                want[0, :, iy, ix] = w5[1, :, ky, kx]
        assert torch.equal(got, want), (oy, ox)
        if (oy, ox) == (H // 2 - 1, W // 2 - 1):
            assert bool(got[0, :, H - 1, :].any()) and bool(got[0, :, :, W - 1].any())
    with pytest.raises(RuntimeError, match="even H, W"):
        ops().conv2d_dgrad(torch.zeros((1, cout, 3, 3), device=DEV), w5.to(DEV), (1, cin, 5, 6), 2)


def test_dgrad_stride_two_against_float64():
    n, cin, cout, H, W = 1, 8, 16, 12, 16                                  # 16 x 9 = 144 terms: more than four runs of 32 in the largest class
    g = torch.Generator().manual_seed(937)
    w, gy = torch.randn((cout, cin, 5, 5), generator=g), torch.randn((n, cout, H // 2, W // 2), generator=g)
    got = ops().conv2d_dgrad(gy.to(DEV), w.to(DEV), (n, cin, H, W), 2)
    x64 = torch.zeros((n, cin, H, W), dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w.double(), stride=2, padding=2).backward(gy.double())
    held("dgrad stride 2 on random floats", got, x64.grad, cpu_dgrad(gy, w, (n, cin, H, W), 2))
    assert torch.equal(got, ops().conv2d_dgrad(gy.to(DEV), w.to(DEV), (n, cin, H, W), 2))


# ------------------------------------------------------------------------------------------------ 5. the bias gradient
@pytest.mark.parametrize("shape", ((1, 32, 4, 6), (2, 5, 3, 7), (2, 8, 40, 52)), ids=str)     # the last: 2 080 pixels per image, two per thread
def test_bias_grad_against_a_float64_sum(shape):
    gy = torch.randn(shape, generator=torch.Generator().manual_seed(941)) + 0.25
    got = ops().conv2d_bias_grad(gy.to(DEV))
    want = gy.double().sum((0, 2, 3))
    err = (got.cpu().double() - want).abs()
    print("bias grad %s: largest error %.3g at a largest value of %.3g" % (shape, float(err.max()), float(want.abs().max())))
    assert got.shape == (shape[1],) and all(float(e) <= FC.spacing(abs(float(v))) for e, v in zip(err, want))
    assert torch.equal(got, ops().conv2d_bias_grad(gy.to(DEV)))


# ------------------------------------------------------------------------------------------------ 6. the layer functions
@pytest.fixture
def bwd_calls(monkeypatch):
    from uc_nerf_amd.ops import cnn
    n = {"wgrad": 0, "dgrad": 0, "bn_bwd": 0, "bias": 0}
    for name, key in (("conv2d_wgrad", "wgrad"), ("conv2d_dgrad", "dgrad"), ("batch_norm_train_bwd", "bn_bwd"), ("conv2d_bias_grad", "bias")):
        def counted(*a, _real=getattr(cnn, name), _key=key, **k):
            n[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(cnn, name, counted)
    return n


LAYERS = (("3 x 3 stride 1", 3, 1, (2, 6, 6, 8), 5), ("5 x 5 stride 2", 5, 2, (2, 6, 8, 12), 9))


def layer_inputs(kind, seed=951):
    name, K, stride, xshape, cout = kind
    g = torch.Generator().manual_seed(seed)
    cin = xshape[1]
    x = torch.randn(xshape, generator=g)
    w = torch.randn((cout, cin, K, K), generator=g) * (2.0 / (K * K * cin)) ** 0.5
    gamma, beta = 0.6 + 0.8 * torch.rand(cout, generator=g), 0.3 * torch.randn(cout, generator=g)
    return x, w, gamma, beta, torch.randn((xshape[0], cout) + FC.out_hw(xshape[2], xshape[3], K, stride), generator=g)


def run_layer(kind, tensors, needs=(True, True)):
    name, K, stride, xshape, cout = kind
    x, w, gamma, beta, grad_out = tensors
    X, W = x.to(DEV).requires_grad_(needs[0]), w.to(DEV).requires_grad_(needs[1])
    G, B = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    rm, rv, nbt = 0.1 * torch.ones(cout, device=DEV), 2 * torch.ones(cout, device=DEV), torch.tensor(3, dtype=torch.int64, device=DEV)
    out = ops().conv2d_bn_train(X, W, G, B, rm, rv, nbt, momentum=0.1, eps=BC.EPS, stride=stride, pad=(K - 1) // 2, relu=True)
    return out, (X, W, G, B), (rm, rv, nbt)


@pytest.mark.parametrize("kind", LAYERS, ids=lambda k: k[0])
def test_layer_function_against_float64(kind, bwd_calls):
    name, K, stride, xshape, cout = kind
    tensors = layer_inputs(kind)
    x, w, gamma, beta, grad_out = tensors
    out, (X, W, G, B), (rm, rv, nbt) = run_layer(kind, tensors)
    assert out.grad_fn is not None
    out.backward(grad_out.to(DEV))
    assert bwd_calls == {"wgrad": 1, "dgrad": 1, "bn_bwd": 1, "bias": 0}
    r64, r32 = (FC.layer_grads(x, w, gamma, beta, grad_out, dt, stride) for dt in (torch.float64, torch.float32))
    assert bool(((out.detach().cpu() > 0) == (r64["z"] > 0)).all())       # the device's ReLU sides are the float64 restatement's
    held(name + " out", out.detach(), r64["out"], r32["out"])
    for key, t in (("x", X), ("w", W), ("gamma", G), ("beta", B)):
        held("%s grad %s" % (name, key), t.grad, r64[key], r32[key])
    # the running statistics moved exactly as batch_norm_train alone moves them
    y = ops().conv2d_bias_relu(X.detach(), W.detach(), torch.zeros(cout, device=DEV), stride=stride, pad=(K - 1) // 2, relu=False)
    rm2, rv2, nbt2 = 0.1 * torch.ones(cout, device=DEV), 2 * torch.ones(cout, device=DEV), torch.tensor(3, dtype=torch.int64, device=DEV)
    want = ops().batch_norm_train(y, G.detach(), B.detach(), rm2, rv2, nbt2, momentum=0.1, eps=BC.EPS, relu=True)
    assert torch.equal(out.detach(), want) and torch.equal(rm, rm2) and torch.equal(rv, rv2) and int(nbt) == int(nbt2) == 4


@pytest.mark.parametrize("K,with_bias", ((1, True), (3, False)), ids=("1 x 1 with bias", "3 x 3 without bias"))
def test_bare_layer_function_against_float64(K, with_bias, bwd_calls):
    g = torch.Generator().manual_seed(953)
    x, w = torch.randn((2, 6, 6, 8), generator=g), torch.randn((7, 6, K, K), generator=g) * (2.0 / (K * K * 6)) ** 0.5
    b = 0.2 * torch.randn(7, generator=g) if with_bias else None
    gy = torch.randn((2, 7, 6, 8), generator=g)
    X, W = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    Bd = b.to(DEV).requires_grad_(True) if with_bias else None
    y = ops().conv2d_train(X, W, Bd, stride=1, pad=(K - 1) // 2)
    y.backward(gy.to(DEV))
    assert bwd_calls == {"wgrad": 1, "dgrad": 1, "bn_bwd": 0, "bias": int(with_bias)}
    r64, r32 = (FC.bare_grads(x, w, b, gy, dt) for dt in (torch.float64, torch.float32))
    for name, got, key in (("y", y.detach(), "out"), ("grad x", X.grad, "x"), ("grad w", W.grad, "w")) + ((("grad b", Bd.grad, "b"),) if with_bias else ()):
        held("bare K=%d %s" % (K, name), got, r64[key], r32[key])
    if with_bias:                                                          # a bias that asks for no gradient: no launch for it
        Bn = b.to(DEV)
        ops().conv2d_train(X, W, Bn, stride=1, pad=0).backward(gy.to(DEV))
        assert bwd_calls["bias"] == 1 and Bn.grad is None


def test_layer_function_skips_the_launch_nobody_needs_and_keeps_the_forward_s_weight(bwd_calls):
    kind = LAYERS[1]
    tensors = layer_inputs(kind, 952)
    for needs, want in (((False, True), {"wgrad": 1, "dgrad": 0}), ((True, False), {"wgrad": 0, "dgrad": 1})):
        for k in bwd_calls:
            bwd_calls[k] = 0
        out, (X, W, G, B), _ = run_layer(kind, tensors, needs)
        out.backward(tensors[4].to(DEV))
        assert {k: bwd_calls[k] for k in want} == want and bwd_calls["bn_bwd"] == 1
        assert (X.grad is None) == (not needs[0]) and (W.grad is None) == (not needs[1])
    # the weight modified in place between forward and backward: the backward still uses the forward's values (both strides)
    for kind in LAYERS:
        tensors = layer_inputs(kind, 952)
        out, (X, W, G, B), _ = run_layer(kind, tensors)
        with torch.no_grad():
            W.mul_(3.0)
        out.backward(tensors[4].to(DEV))
        out2, (X2, W2, G2, B2), _ = run_layer(kind, tensors)
        out2.backward(tensors[4].to(DEV))
        assert torch.equal(X.grad, X2.grad) and torch.equal(W.grad, W2.grad) and torch.equal(G.grad, G2.grad), kind[0]


# ------------------------------------------------------------------------------------------------ 7. the module
@pytest.fixture(scope="module", params=range(len(FC.MODULE_CASES)), ids=lambda i: "FeatureNet%s" % (FC.MODULE_CASES[i][0],))
def module_case(request):
    case = FC.MODULE_CASES[request.param]
    x, R = FC.module_inputs(case)
    net = BC.randomise_train(M().FeatureNet(8, batch_stats="device", training="device"), case[1]).to(DEV)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    r64, r32 = FC.feature_net(x, sd, torch.float64, R), FC.feature_net(x, sd, torch.float32, R)
    return case, net, sd, (x, R), r64, r32


def loss_of(outs, R):
    return sum((outs[k] * R[k].to(outs[k].device)).sum() for k in ("stage1", "stage2", "stage3"))


@pytest.mark.parametrize("image_grad", (True, False), ids=("image gradient", "no image gradient"))
def test_module_against_float64(module_case, image_grad, monkeypatch):
    case, net, sd, (x, R), r64, r32 = module_case
    net.load_state_dict(sd)
    assert not FC.relu_offenders(r64, r32)
    twin = BC.randomise_train(M().FeatureNet(8, batch_stats="device"), case[1]).to(DEV)
    twin.load_state_dict(sd)
    with torch.no_grad():
        outs0 = twin(x.to(DEV))                                            # the existing batch_stats="device" route, same weights
    dgrads = []
    real = ops().conv2d_dgrad
    monkeypatch.setattr(ops().cnn, "conv2d_dgrad", lambda *a, **k: dgrads.append(a[2]) or real(*a, **k))
    X = x.to(DEV).requires_grad_(image_grad)
    for p in net.parameters():
        p.grad = None
    outs = net(X)
    loss_of(outs, R).backward()
    assert len(dgrads) == (13 if image_grad else 12) and ((tuple(x.shape) in [tuple(s) for s in dgrads]) == image_grad)
    for k in ("stage1", "stage2", "stage3"):
        assert outs[k].grad_fn is not None and torch.equal(outs[k].detach(), outs0[k]), k
        held(k, outs[k].detach(), r64["out"][k], r32["out"][k])
    grads = dict(net.named_parameters())
    assert len(grads) == 31 == len(r64["grads"])
    for k, p in grads.items():
        held("grad " + k, p.grad, r64["grads"][k], r32["grads"][k])
    if image_grad:
        held("grad image", X.grad, r64["grad_x"], r32["grad_x"])
    else:
        assert X.grad is None
    for (k, a), (_, b) in zip(net.state_dict().items(), twin.state_dict().items()):
        if "running_" in k or "num_batches" in k:
            assert torch.equal(a, b), k                                    # the statistics moved as on the batch-statistic route, bit for bit
    assert int(net.conv0[0].bn.num_batches_tracked) == int(sd["conv0.0.bn.num_batches_tracked"]) + 1
    net.load_state_dict(sd)


@pytest.fixture
def route_calls(monkeypatch):
    o, n = ops(), {"conv": 0, "bn": 0, "layer": 0, "bare": 0, "layer3d": 0}
    for name, key in (("conv2d_bias_relu", "conv"), ("batch_norm_train", "bn"), ("conv2d_bn_train", "layer"), ("conv2d_train", "bare"), ("conv3d_bn_train", "layer3d")):
        def counted(*a, _real=getattr(o, name), _key=key, **k):
            n[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(o, name, counted)
    return n


def test_routes_by_call_count_and_the_second_step(route_calls):
    case = FC.MODULE_CASES[0]
    x, R = FC.module_inputs(case)
    xd = x.to(DEV)

    def count(net, inp):
        for k in route_calls:
            route_calls[k] = 0
        out = net(inp)
        return out, (route_calls["layer"], route_calls["bare"], route_calls["conv"], route_calls["bn"])

    def make(**kw):
        return BC.randomise_train(M().FeatureNet(8, **kw), case[1]).to(DEV)

    net = make(batch_stats="device", training="device")
    outs, n = count(net, xd)                                                 # train() + grad: the new route
    assert n == (8, 5, 0, 0) and outs["stage3"].grad_fn is not None
    with torch.no_grad():
        outs, n = count(net, xd)                                             # train() + no_grad: the batch-statistic route
    assert n == (0, 0, 13, 8) and outs["stage3"].grad_fn is None
    net.eval()
    with torch.no_grad():
        assert count(net, xd)[1] == (0, 0, 13, 0)                            # eval() + no_grad: the folded route
    outs, n = count(net, xd)                                                 # eval() + grad: torch's layers
    assert n == (0, 0, 0, 0) and outs["stage3"].grad_fn is not None
    outs, n = count(BC.randomise_train(M().FeatureNet(8, training="device"), case[1]), x)        # a CPU module and input: torch's layers
    assert n == (0, 0, 0, 0) and outs["stage3"].grad_fn is not None and not outs["stage3"].is_cuda
    assert count(make(), xd)[1] == (0, 0, 0, 0)                              # the default keyword
    assert count(make(inference="torch", training="device"), xd)[1] == (0, 0, 0, 0)
    off = make(training="device")
    off.conv1[1].bn.momentum = None                                          # a cumulative average is not built: torch's route
    assert count(off, xd)[1] == (0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="divisible by 4"):
        make(training="device")(torch.rand((1, 3, 18, 24), device=DEV))
    # two steps: the second forward + backward uses the updated weights (the packed caches follow the weights' versions)
    net = make(training="device")
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    loss_of(net(xd), R).backward()
    with torch.no_grad():
        for p in net.parameters():
            p.sub_(1e-3 * p.grad)
            p.grad = None
    sd2 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert not torch.equal(sd["conv0.0.conv.weight"], sd2["conv0.0.conv.weight"])
    X = xd.clone().requires_grad_(True)
    outs = net(X)
    loss_of(outs, R).backward()
    r64, r32 = FC.feature_net(x, sd2, torch.float64, R), FC.feature_net(x, sd2, torch.float32, R)
    if not FC.relu_offenders(r64, r32):                                      # (the condition is asserted for the first step's weights only)
        held("second step stage3", outs["stage3"].detach(), r64["out"]["stage3"], r32["out"]["stage3"])
        held("second step grad image", X.grad, r64["grad_x"], r32["grad_x"])
        held("second step grad conv1.0.conv.weight", net.conv1[0].conv.weight.grad, r64["grads"]["conv1.0.conv.weight"], r32["grads"]["conv1.0.conv.weight"])
    stale = FC.feature_net(x, dict(sd2, **{k: v for k, v in sd.items() if k.endswith("weight") and ".bn." not in k}), torch.float64)
    new, old = (float((outs["stage3"].detach().cpu().double() - r["out"]["stage3"]).abs().max()) for r in (r64, stale))
    assert new < 0.01 * float((stale["out"]["stage3"] - r64["out"]["stage3"]).abs().max()) < old


def test_cascade_with_cnns_trains_end_to_end_on_both_device_routes(route_calls):
    V, H, W, ndepths = 3, 32, 32, [48, 32, 8]
    g = torch.Generator().manual_seed(99)
    imgs = torch.rand(1, V, 3, H, W, generator=g).to(DEV)
    affine, affine_inv = (t.to(DEV) for t in S.cameras(V, H, W, seed=100))
    near_far = torch.tensor([2.0, 11.0], device=DEV)

    def build(**kw):
        net = M().CascadeMVSNet.with_cnns(ndepths=ndepths, **kw)
        for i, module in enumerate([net.feature] + list(net.cost_regularization)):
            MC.randomise(module, 95 + i)
        return net.to(DEV).train()

    only3d = build(training="device")
    only3d(imgs, affine, affine_inv, near_far, pad=0)
    assert route_calls["layer"] == 0 == route_calls["bare"] and route_calls["layer3d"] == 30     # `training=` alone: the CostRegNets only, as before
    net = build(training="device", feature_training="device")
    vol, conf, depth, outputs = net(imgs, affine, affine_inv, near_far, pad=0)
    assert route_calls["layer"] == 8 * V and route_calls["bare"] == 5 * V and route_calls["layer3d"] == 60
    from uc_nerf_amd.utils.loss import cas_mvsnet_loss_device
    keys = ["stage1", "stage2", "stage3"]
    gts = {k: 2.0 + 9.0 * torch.rand(outputs[k]["depth"].shape, generator=g) for k in keys}
    weights = {k: torch.ones(outputs[k]["depth"].shape) for k in keys}
    total, _ = cas_mvsnet_loss_device({k: outputs[k] for k in keys}, gts, weights)
    (total + 1e-3 * vol.square().mean() + 1e-3 * conf.mean()).backward()
    for k, p in net.feature.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert any(bool(p.grad.abs().sum() > 0) for p in net.feature.parameters())


def test_zz_largest_share_of_the_chain_bar():
    """Prints the largest device error / chain bar over the comparisons this run made (profiles/feature_train.md records it)."""
    if SHARES:
        print("largest share of the chain bar over %d comparisons: %.3f" % (len(SHARES), max(SHARES)))
        assert max(SHARES) <= 1.0
