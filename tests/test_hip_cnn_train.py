"""CostRegNet's training route on the GPU (csrc/conv3d_bwd.hip, the backward kernels of csrc/bn.hip, ops.conv3d_bn_train, training="device"):
the weight gradient bit for bit on integer lattices and one-hot inputs, its workspace and determinism, the input gradient on the forward
kernel, the batch-norm backward, the layer function and the module against the float64 restatement of tests/cnn_train_cases.py.

The bar wherever a division or a square root is involved is the project's chain rule: 4 x the float32 CPU restatement's own largest distance
from float64, at least one float32 spacing of the largest value.  Every comparison prints the device's error, the float32 restatement's and
their ratio."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import bn_cases as BC
import cascade_stubs as S
import cnn_train_cases as TC
import mvs_cnn_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


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
    bar, err32 = TC.chain_bar(ref64, cpu32)
    err = float((got.detach().cpu().double() - ref64).abs().max())
    print("%s: device %.3g, float32 cpu %.3g, ratio %.2f, bar %.3g, largest %.3g" % (name, err, err32, err / max(err32, 1e-30), bar, float(ref64.abs().max())))
    assert got.shape == ref64.shape and got.dtype == torch.float32
    assert err <= bar, name
    return bar


def cpu_wgrad(x, gy, w_shape, stride, transposed):
    """torch's CPU autograd weight gradient."""
    w = torch.zeros(w_shape, requires_grad=True)
    TC.conv(x, w, stride, transposed).backward(gy)
    return w.grad


def out_shape(n, cout, stride, D, H, W):
    return (n, cout) + tuple((s - 1) // stride + 1 for s in (D, H, W))


def ragged_shape():
    """The smallest (1, 8, 8, 1, 1, 1, W) with at least three chunks and a shorter last one, by the library's own workspace query."""
    f = lib().lib().ucnerf_conv3d_wgrad_workspace_floats
    W = 3
    while True:
        chunks = f(1, 8, 8, 1, 1, W, 3, 1, 1, 0) // (8 * 8 * 27)
        length = 32 * -(-W // (32 * min(-(-W // 32), 512)))                # the documented chunk length for one tile
        if chunks >= 3 and 0 < W - (chunks - 1) * length < length:
            return (1, 8, 8, 1, 1, 1, W)
        W += 1


# ------------------------------------------------------------------------------------------------ 1. wgrad on integer lattices
@pytest.mark.parametrize("shape", TC.WGRAD_SHAPES + TC.WGRAD_LONG_CHUNKS + ("ragged",), ids=str)
def test_wgrad_lattice_is_bit_equal_to_torch_cpu(shape):
    if shape == "ragged":
        shape = ragged_shape()
        assert shape[6] <= 128, shape
    n, cin, cout, stride, D, H, W = shape
    x, gy = MC.lattice((n, cin, D, H, W), 4, 801), MC.lattice(out_shape(n, cout, stride, D, H, W), 4, 802)
    want = cpu_wgrad(x, gy, (cout, cin, 3, 3, 3), stride, False)
    assert float(want.abs().max()) < 2 ** 24 and float(want.abs().max()) > 0
    got = ops().conv3d_wgrad(x.to(DEV), gy.to(DEV), stride, 1, False)
    assert torch.equal(got.cpu(), want), shape


@pytest.mark.parametrize("shape", TC.WGRAD_TRANSPOSED, ids=str)
def test_wgrad_transposed_lattice_is_bit_equal_to_torch_cpu(shape):
    cin, cout, D, H, W = shape
    x, gy = MC.lattice((2, cin, D, H, W), 4, 803), MC.lattice((2, cout, 2 * D, 2 * H, 2 * W), 4, 804)
    want = cpu_wgrad(x, gy, (cin, cout, 3, 3, 3), 2, True)
    got = ops().conv3d_wgrad(x.to(DEV), gy.to(DEV), 2, 1, True)
    assert float(want.abs().max()) > 0 and torch.equal(got.cpu(), want), shape


# ------------------------------------------------------------------------------------------------ 2. wgrad, one-hot
def window(x, img, base):
    """The 27 taps of x[img] [c,D,H,W] at base + (0..2)^3, +0 outside -> [c,27]."""
    c, D, H, W = x.shape[1:]
    out = torch.zeros(c, 27)
    for t, (td, th, tw) in enumerate(itertools.product(range(3), repeat=3)):
        d, h, w = base[0] + td, base[1] + th, base[2] + tw
        if 0 <= d < D and 0 <= h < H and 0 <= w < W:
            out[:, t] = x[img, :, d, h, w]
    return out


@pytest.mark.parametrize("stride", (1, 2))
def test_wgrad_one_hot_reads_the_window(stride):
    n, cin, cout, D, H, W = 2, 5, 3, 4, 5, 6
    x = torch.randn((n, cin, D, H, W), generator=torch.Generator().manual_seed(811))
    oshape = out_shape(n, cout, stride, D, H, W)
    OD, OH, OW = oshape[2:]
    # every corner (taps outside on three sides at once), one voxel per face and an interior one, in the second image too
    spots = list(itertools.product((0, OD - 1), (0, OH - 1), (0, OW - 1))) + [(OD // 2, OH // 2, OW // 2), (0, 1, 1), (1, 0, 1), (1, 1, 0),
                                                                              (OD - 1, 1, 1), (1, OH - 1, 1), (1, 1, OW - 1)]
    for k, (od, oh, ow) in enumerate(spots):
        img, co = k % n, k % cout
        gy = torch.zeros(oshape)
        gy[img, co, od, oh, ow] = 1.0
        got = ops().conv3d_wgrad(x.to(DEV), gy.to(DEV), stride, 1, False).cpu().view(cout, cin, 27)
        want = torch.zeros(cout, cin, 27)
        want[co] = window(x, img, (od * stride - 1, oh * stride - 1, ow * stride - 1))
        assert torch.equal(got, want), (stride, od, oh, ow)


def test_wgrad_transposed_one_hot_covers_every_parity_class():
    n, cin, cout, D, H, W = 2, 3, 5, 2, 3, 2
    gy = torch.randn((n, cout, 2 * D, 2 * H, 2 * W), generator=torch.Generator().manual_seed(812))
    # one-hot in x at s: row ci reads grad_y's window at 2 s - 1, which covers all eight parity classes of the output (and the border at s = 0)
    for k, s in enumerate(itertools.product(range(D), range(H), range(W))):
        img, ci = k % n, k % cin
        x = torch.zeros((n, cin, D, H, W))
        x[(img, ci) + s] = 1.0
        got = ops().conv3d_wgrad(x.to(DEV), gy.to(DEV), 2, 1, True).cpu().view(cin, cout, 27)
        want = torch.zeros(cin, cout, 27)
        want[ci] = window(gy, img, tuple(2 * v - 1 for v in s))
        assert torch.equal(got, want), s
    # and a one-hot in grad_y of each parity class against torch's CPU autograd
    xr = torch.randn((n, cin, D, H, W), generator=torch.Generator().manual_seed(813))
    for cls in itertools.product((0, 1), repeat=3):
        g1 = torch.zeros_like(gy)
        g1[(1, 2) + tuple(2 * (size - 1) + p for size, p in zip((D, H, W), cls))] = 1.0
        got = ops().conv3d_wgrad(xr.to(DEV), g1.to(DEV), 2, 1, True).cpu()
        assert torch.equal(got, cpu_wgrad(xr, g1, (cin, cout, 3, 3, 3), 2, True)), cls


# ------------------------------------------------------------------------------------------------ 3. wgrad: workspace, guards, determinism
def test_wgrad_writes_all_of_its_workspace_and_nothing_else_and_repeats_its_bits():
    L = lib()
    n, cin, cout, stride, D, H, W = 2, 8, 8, 1, 5, 7, 11
    x = torch.randn((n, cin, D, H, W), generator=torch.Generator().manual_seed(821)).to(DEV)
    gy = torch.randn((n, cout, D, H, W), generator=torch.Generator().manual_seed(822)).to(DEV)
    floats = L.lib().ucnerf_conv3d_wgrad_workspace_floats(n, cin, cout, D, H, W, 3, stride, 1, 0)
    assert floats // (cin * cout * 27) >= 3
    nan, sentinel, guard = float("nan"), -12345.0, 64
    results = []
    for _ in range(2):
        ws = torch.full((floats + 2 * guard,), nan, device=DEV)
        ws[:guard], ws[-guard:] = sentinel, sentinel
        out = torch.full((cout * cin * 27 + 2 * guard,), nan, device=DEV)
        out[:guard], out[-guard:] = sentinel, sentinel
        p = L.Conv3dWgradParams()
        p.n, p.cin, p.D, p.H, p.W, p.cout, p.K, p.stride, p.pad, p.transposed, p.workspace_floats = n, cin, D, H, W, cout, 3, stride, 1, 0, floats
        p.x, p.grad_y, p.workspace, p.grad_weight = x.data_ptr(), gy.data_ptr(), ws[guard:].data_ptr(), out[guard:].data_ptr()
        L.call("ucnerf_conv3d_wgrad", p, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for t in (ws, out):
            assert bool((t[:guard] == sentinel).all()) and bool((t[-guard:] == sentinel).all()) and not bool(torch.isnan(t[guard:-guard]).any())
        results.append((ws.clone(), out.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert torch.equal(results[0][1][guard:-guard].view(cout, cin, 3, 3, 3), ops().conv3d_wgrad(x, gy, stride, 1, False))
    w64 = torch.zeros((cout, cin, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv3d(x.cpu().double(), w64, padding=1).backward(gy.cpu().double())
    w32 = cpu_wgrad(x.cpu(), gy.cpu(), (cout, cin, 3, 3, 3), stride, False)
    held("wgrad on random floats", results[0][1][guard:-guard].view(cout, cin, 3, 3, 3), w64.grad, w32)


# ------------------------------------------------------------------------------------------------ 4. dgrad
DGRAD_SHAPES = ((1, 8, 8, 1, 4, 5, 7), (1, 8, 16, 2, 8, 8, 8), (2, 4, 8, 2, 4, 6, 10), (1, 16, 1, 1, 3, 4, 5), (1, 33, 65, 1, 3, 3, 3))


@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=str)
def test_dgrad_lattice_is_bit_equal_to_torch_cpu(shape):
    n, cin, cout, stride, D, H, W = shape
    w, gy = MC.lattice((cout, cin, 3, 3, 3), 4, 831), MC.lattice(out_shape(n, cout, stride, D, H, W), 4, 832)
    x = torch.zeros((n, cin, D, H, W), requires_grad=True)
    F.conv3d(x, w, stride=stride, padding=1).backward(gy)
    got = ops().conv3d_dgrad(gy.to(DEV), w.to(DEV), (n, cin, D, H, W), stride, 1, False)
    assert float(x.grad.abs().max()) > 0 and torch.equal(got.cpu(), x.grad), shape
    packed = ops().conv3d_dgrad_pack(w.to(DEV), stride, 1, False)
    assert torch.equal(ops().conv3d_dgrad(gy.to(DEV), packed, (n, cin, D, H, W), stride, 1, False).cpu(), x.grad)


@pytest.mark.parametrize("shape", TC.WGRAD_TRANSPOSED, ids=str)
def test_dgrad_transposed_lattice_is_bit_equal_to_torch_cpu(shape):
    cin, cout, D, H, W = shape
    w, gy = MC.lattice((cin, cout, 3, 3, 3), 4, 833), MC.lattice((2, cout, 2 * D, 2 * H, 2 * W), 4, 834)
    x = torch.zeros((2, cin, D, H, W), requires_grad=True)
    F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1).backward(gy)
    got = ops().conv3d_dgrad(gy.to(DEV), w.to(DEV), (2, cin, D, H, W), 2, 1, True)
    assert torch.equal(got.cpu(), x.grad), shape


def test_dgrad_one_hot_reads_out_the_unflipped_kernel():
    cin, cout, D = 3, 4, 5
    w = torch.randn((cout, cin, 3, 3, 3), generator=torch.Generator().manual_seed(835))
    gy = torch.zeros((1, cout, D, D, D))
    gy[0, 2, 2, 2, 2] = 1.0
    got = ops().conv3d_dgrad(gy.to(DEV), w.to(DEV), (1, cin, D, D, D), 1, 1, False).cpu()
    assert torch.equal(got[0, :, 1:4, 1:4, 1:4], w[2])                     # dx[ci, o - 1 + k] = w[co, ci, k]: the kernel itself, not its mirror image
    got[0, :, 1:4, 1:4, 1:4] = 0
    assert not bool(got.any())
    with pytest.raises(RuntimeError, match="even D, H, W"):
        ops().conv3d_dgrad(torch.zeros((1, cout, 3, 3, 3), device=DEV), w.to(DEV), (1, cin, 5, 5, 5), 2, 1, False)


# ------------------------------------------------------------------------------------------------ 5. batch-norm backward
def partials(n, S_):
    return lib().lib().ucnerf_bn_partials(n, S_)


class BnCase:
    def __init__(self, shape, seed, y=None):
        g = torch.Generator().manual_seed(seed)
        C = shape[1]
        self.shape = tuple(shape)
        self.y = torch.randn(shape, generator=g) * 1.5 + 0.5 if y is None else y
        self.g = torch.randn(shape, generator=g)
        self.gamma, self.beta = 0.6 + 0.8 * torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)

    def forward(self, relu):
        C = self.shape[1]
        return ops().batch_norm_train(self.y.to(DEV), self.gamma.to(DEV), self.beta.to(DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                                      torch.zeros((), dtype=torch.int64, device=DEV), relu=relu, return_stats=True)

    def call(self, relu, inplace=False):
        out, mean, var = self.forward(relu)
        g = self.g.to(DEV)
        dy, dgamma, dbeta = ops().batch_norm_train_bwd(g, self.y.to(DEV), mean, var, self.gamma.to(DEV), self.beta.to(DEV), eps=BC.EPS, relu=relu,
                                                       out=g if inplace else None)
        assert (dy is g) == inplace and (inplace or torch.equal(g.cpu(), self.g))
        return dy, dgamma, dbeta, out

    def reference(self, dtype, relu):
        Y, G, B = TC.leaf(self.y, dtype), TC.leaf(self.gamma, dtype), TC.leaf(self.beta, dtype)
        dims, shape = (0,) + tuple(range(2, Y.dim())), (1, -1) + (1,) * (Y.dim() - 2)
        mean = Y.mean(dims)
        var = ((Y - mean.view(shape)) ** 2).mean(dims)
        z = (Y - mean.view(shape)) / torch.sqrt(var.view(shape) + BC.EPS) * G.view(shape) + B.view(shape)
        (F.relu(z) if relu else z).backward(self.g.to(dtype))
        return Y.grad, G.grad, B.grad, z.detach()


@pytest.mark.parametrize("shape", BC.OP_SHAPES + ("ragged",), ids=str)
def test_bn_backward_against_float64(shape):
    if shape == "ragged":
        shape = BC.ragged_shape(partials)
        assert partials(shape[0], shape[2]) >= 3
    case = BnCase(shape, 841)
    for relu in (True, False):
        got, again = case.call(relu), case.call(relu, inplace=True)
        r64, r32 = case.reference(torch.float64, relu), case.reference(torch.float32, relu)
        sides = (got[3].cpu() > 0) == (r64[3] > 0)
        assert not relu or bool(sides.all()), "a ReLU took another side than in float64: the comparison below would not mean anything"
        for name, g_, a_, w64, w32 in zip(("grad_y", "grad_weight", "grad_bias"), got, again, r64, r32):
            held("%s %s relu=%s" % (name, shape, relu), g_, w64, w32)
            assert torch.equal(g_, a_), name                              # in place and out of place agree bit for bit
    a, b = case.call(True), case.call(True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                   # determinism


def test_bn_backward_mask_is_the_forward_s_own_sign_bit_for_bit():
    case = BnCase(BC.ragged_shape(partials), 842)
    out, mean, var = case.forward(True)
    gamma, beta, y = case.gamma.to(DEV), case.beta.to(DEV), case.y.to(DEV)
    ones = torch.ones_like(y)
    # with gamma's and the statistics' terms out of the way (g = 1: A = the mask's count, read back through grad_bias) the mask itself is visible
    dy, dgamma, dbeta = ops().batch_norm_train_bwd(ones, y, mean, var, gamma, beta, eps=BC.EPS, relu=True)
    count = (out > 0).sum(dim=(0, 2)).float()
    assert torch.equal(dbeta, count)
    # element by element: dy + sg (k1 + d k2) = sg mask; compare against the same call without ReLU, whose mask is all ones
    dy1, _, dbeta1 = ops().batch_norm_train_bwd(ones, y, mean, var, gamma, beta, eps=BC.EPS, relu=False)
    assert torch.equal(dbeta1, torch.full_like(dbeta1, y.shape[0] * y.shape[2]))
    g = case.g.to(DEV)
    masked = g * (out > 0)
    a = ops().batch_norm_train_bwd(g, y, mean, var, gamma, beta, eps=BC.EPS, relu=True)
    b = ops().batch_norm_train_bwd(masked, y, mean, var, gamma, beta, eps=BC.EPS, relu=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b))                   # mask == (out > 0), or some element's gradient would differ


def test_bn_backward_offset_constant_channel_and_poisoned_workspace():
    L = lib()
    shape = (1, 8, 4, 16, 16)
    y = 1000.0 + 0.01 * torch.randn(shape, generator=torch.Generator().manual_seed(843))
    case = BnCase(shape, 844, y=y)
    got = case.call(False)
    r64, r32 = case.reference(torch.float64, False), case.reference(torch.float32, False)
    for name, g_, w64, w32 in zip(("grad_y", "grad_weight", "grad_bias"), got, r64, r32):
        held("%s at offset 1000" % name, g_, w64, w32)
    # an exactly constant channel: sigma^2 = 0, r = 1 / sqrt(eps), everything finite; B = 0 exactly so grad_weight = 0
    shape = BC.ragged_shape(partials)
    n, Ch, S_ = shape
    case = BnCase(shape, 845)
    case.y[:, 1] = 2.5
    dy, dgamma, dbeta, _ = case.call(False)
    assert bool(torch.isfinite(dy).all()) and float(dgamma[1]) == 0.0
    r = 1.0 / (BC.EPS ** 0.5)
    g1 = case.g[:, 1].double()
    want = float(case.gamma[1]) * r * (g1 - g1.mean())
    err = float((dy[:, 1].cpu().double() - want).abs().max())
    print("constant channel: %.3g against a largest value of %.3g" % (err, float(want.abs().max())))
    assert err <= 4 * TC.spacing(want.abs().max())
    # the raw entry points with a NaN-poisoned workspace and sentinel guards
    P = partials(n, S_)
    out, mean, var = case.forward(True)
    nan, sentinel = float("nan"), -12345.0
    ws = torch.full((Ch * P * 2 + 4,), nan, dtype=torch.float64, device=DEV)
    ws[:2], ws[-2:] = sentinel, sentinel
    dyb = torch.full((case.y.numel() + 2,), nan, device=DEV)
    dyb[0], dyb[-1] = sentinel, sentinel
    small = torch.full((2, Ch + 2), nan, device=DEV)
    small[:, 0], small[:, -1] = sentinel, sentinel
    g, yd, gamma, beta = case.g.to(DEV), case.y.to(DEV), case.gamma.to(DEV), case.beta.to(DEV)
    r_, a_ = L.BnBwdReduceParams(), L.BnBwdApplyParams()
    for q in (r_, a_):
        q.n, q.C, q.S, q.workspace_pairs, q.eps, q.relu = n, Ch, S_, Ch * P, BC.EPS, 1
        q.g, q.y, q.saved_mean, q.saved_var, q.weight, q.bias = g.data_ptr(), yd.data_ptr(), mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr()
        q.workspace = ws[2:].data_ptr()
    a_.grad_y, a_.grad_weight, a_.grad_bias = dyb[1:].data_ptr(), small[0, 1:].data_ptr(), small[1, 1:].data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    L.call("ucnerf_bn_bwd_reduce", r_, stream)
    L.call("ucnerf_bn_bwd_apply", a_, stream)
    torch.cuda.synchronize()
    assert bool((ws[:2] == sentinel).all()) and bool((ws[-2:] == sentinel).all()) and not bool(torch.isnan(ws[2:-2]).any())
    assert float(dyb[0]) == sentinel == float(dyb[-1]) and not bool(torch.isnan(dyb[1:-1]).any())
    assert bool((small[:, 0] == sentinel).all()) and bool((small[:, -1] == sentinel).all()) and not bool(torch.isnan(small[:, 1:-1]).any())
    want = ops().batch_norm_train_bwd(g, yd, mean, var, gamma, beta, eps=BC.EPS, relu=True)
    assert torch.equal(dyb[1:-1].view(shape), want[0]) and torch.equal(small[0, 1:-1], want[1]) and torch.equal(small[1, 1:-1], want[2])


# ------------------------------------------------------------------------------------------------ 6. the layer function
@pytest.fixture
def bwd_calls(monkeypatch):
    from uc_nerf_amd.ops import cnn
    n = {"wgrad": 0, "dgrad": 0, "bn_bwd": 0}
    for name, key in (("conv3d_wgrad", "wgrad"), ("conv3d_dgrad", "dgrad"), ("batch_norm_train_bwd", "bn_bwd")):
        def counted(*a, _real=getattr(cnn, name), _key=key, **k):
            n[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(cnn, name, counted)
    return n


LAYERS = (("stride 1", 1, False, (1, 6, 4, 6, 8), 5, False), ("stride 2", 2, False, (2, 6, 4, 6, 8), 9, False), ("transposed + skip", 2, True, (1, 6, 2, 3, 4), 5, True))


def layer_inputs(kind, seed=851):
    name, stride, transposed, xshape, cout, with_skip = kind
    g = torch.Generator().manual_seed(seed)
    cin = xshape[1]
    x = torch.randn(xshape, generator=g)
    w = torch.randn((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), generator=g) * (2.0 / (27 * cin)) ** 0.5
    gamma, beta = 0.6 + 0.8 * torch.rand(cout, generator=g), 0.3 * torch.randn(cout, generator=g)
    oshape = (xshape[0], cout) + (tuple(2 * s for s in xshape[2:]) if transposed else tuple((s - 1) // stride + 1 for s in xshape[2:]))
    skip = torch.randn(oshape, generator=g) if with_skip else None
    return x, w, gamma, beta, skip, torch.randn(oshape, generator=g)


def run_layer(kind, tensors, needs=(True, True)):
    name, stride, transposed, xshape, cout, _ = kind
    x, w, gamma, beta, skip, grad_out = tensors
    X, W = x.to(DEV).requires_grad_(needs[0]), w.to(DEV).requires_grad_(needs[1])
    G, B = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    Sk = skip.to(DEV).requires_grad_(True) if skip is not None else None
    rm, rv, nbt = 0.1 * torch.ones(cout, device=DEV), 2 * torch.ones(cout, device=DEV), torch.tensor(3, dtype=torch.int64, device=DEV)
    out = ops().conv3d_bn_train(X, W, G, B, rm, rv, nbt, momentum=0.1, eps=BC.EPS, stride=stride, pad=1, relu=True, skip=Sk, transposed=transposed)
    return out, (X, W, G, B, Sk), (rm, rv, nbt)


@pytest.mark.parametrize("kind", LAYERS, ids=lambda k: k[0])
def test_layer_function_against_float64(kind, bwd_calls):
    name, stride, transposed, xshape, cout, with_skip = kind
    tensors = layer_inputs(kind)
    x, w, gamma, beta, skip, grad_out = tensors
    out, (X, W, G, B, Sk), (rm, rv, nbt) = run_layer(kind, tensors)
    assert out.grad_fn is not None
    go = grad_out.to(DEV)
    out.backward(go)
    assert bwd_calls == {"wgrad": 1, "dgrad": 1, "bn_bwd": 1}
    r64, r32 = (TC.layer_grads(x, w, gamma, beta, grad_out, dt, stride, transposed, True, skip) for dt in (torch.float64, torch.float32))
    if not with_skip:                                                      # the device's ReLU sides are the float64 restatement's
        assert bool(((out.detach().cpu() > 0) == (r64["z"] > 0)).all())
    held(name + " out", out.detach(), r64["out"], r32["out"])
    for key, t in (("x", X), ("w", W), ("gamma", G), ("beta", B)):
        held("%s grad %s" % (name, key), t.grad, r64[key], r32[key])
    if with_skip:
        assert torch.equal(Sk.grad, go)                                    # grad_skip is grad_out, bit for bit
    # the running statistics moved exactly as batch_norm_train alone moves them
    y = ops().conv3d(X.detach(), W.detach(), torch.zeros(cout, device=DEV), stride=stride, pad=1, relu=False, transposed=transposed)
    rm2, rv2, nbt2 = 0.1 * torch.ones(cout, device=DEV), 2 * torch.ones(cout, device=DEV), torch.tensor(3, dtype=torch.int64, device=DEV)
    want = ops().batch_norm_train(y, G.detach(), B.detach(), rm2, rv2, nbt2, momentum=0.1, eps=BC.EPS, relu=True, skip=Sk.detach() if with_skip else None)
    assert torch.equal(out.detach(), want) and torch.equal(rm, rm2) and torch.equal(rv, rv2) and int(nbt) == int(nbt2) == 4


def test_layer_function_skips_the_launch_nobody_needs_and_keeps_the_forward_s_weight(bwd_calls):
    kind = LAYERS[0]
    tensors = layer_inputs(kind, 852)
    for needs, want in (((False, True), {"wgrad": 1, "dgrad": 0}), ((True, False), {"wgrad": 0, "dgrad": 1})):
        for k in bwd_calls:
            bwd_calls[k] = 0
        out, (X, W, G, B, _), _ = run_layer(kind, tensors, needs)
        out.backward(tensors[5].to(DEV))
        assert {k: bwd_calls[k] for k in want} == want and bwd_calls["bn_bwd"] == 1
        assert (X.grad is None) == (not needs[0]) and (W.grad is None) == (not needs[1])
    # the weight modified in place between forward and backward: the backward still uses the forward's values
    out, (X, W, G, B, _), _ = run_layer(kind, tensors)
    with torch.no_grad():
        W.mul_(3.0)
    out.backward(tensors[5].to(DEV))
    out2, (X2, W2, G2, B2, _), _ = run_layer(kind, tensors)
    out2.backward(tensors[5].to(DEV))
    assert torch.equal(X.grad, X2.grad) and torch.equal(W.grad, W2.grad) and torch.equal(G.grad, G2.grad)
    # the bare variant (`prob`)
    x, w = tensors[0], torch.randn((1, 6, 3, 3, 3), generator=torch.Generator().manual_seed(853))
    X, W = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y = ops().conv3d_train(X, W, 1, 1)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(854))
    y.backward(gy.to(DEV))
    refs = []
    for dt in (torch.float64, torch.float32):
        Xc, Wc = TC.leaf(x, dt), TC.leaf(w, dt)
        yc = F.conv3d(Xc, Wc, padding=1)
        yc.backward(gy.to(dt))
        refs.append((yc.detach(), Xc.grad, Wc.grad))
    for name, got, w64, w32 in zip(("prob y", "prob grad x", "prob grad w"), (y.detach(), X.grad, W.grad), refs[0], refs[1]):
        held(name, got, w64, w32)


# ------------------------------------------------------------------------------------------------ 7. the module
@pytest.fixture(scope="module", params=range(len(TC.MODULE_CASES)), ids=lambda i: "CostRegNet(%d,%d)" % TC.MODULE_CASES[i][:2])
def module_case(request):
    case = TC.MODULE_CASES[request.param]
    x, R1, R2 = TC.module_inputs(case)
    net = BC.randomise_train(M().CostRegNet(case[0], case[1], batch_stats="device", training="device"), case[3]).to(DEV)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    r64, r32 = TC.cost_reg_net(x, sd, torch.float64, R1, R2), TC.cost_reg_net(x, sd, torch.float32, R1, R2)
    return case, net, sd, (x, R1, R2), r64, r32


def test_module_against_float64(module_case):
    case, net, sd, (x, R1, R2), r64, r32 = module_case
    net.load_state_dict(sd)
    assert not TC.relu_offenders(r64, r32, sd)
    with torch.no_grad():
        cost0, prob0 = net(x.to(DEV))                                      # the existing batch_stats="device" route, same weights
    net.load_state_dict(sd)                                                # (the running statistics moved)
    X = x.to(DEV).requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    cost, prob = net(X)
    assert cost.grad_fn is not None and prob.grad_fn is not None
    ((cost * R1.to(DEV)).sum() + (prob * R2.to(DEV)).sum()).backward()
    assert torch.equal(cost.detach(), cost0) and torch.equal(prob.detach(), prob0)
    held("cost", cost.detach(), r64["cost"], r32["cost"])
    held("prob", prob.detach(), r64["prob"], r32["prob"])
    held("grad x", X.grad, r64["grad_x"], r32["grad_x"])
    for k, p in net.named_parameters():
        held("grad " + k, p.grad, r64["grads"][k], r32["grads"][k])
    # the device's ReLU sides, layer by layer through the forward's own two steps (the batch-norm once more without the skip shows z's sign)
    net.load_state_dict(sd)
    with torch.no_grad():
        outs = {}

        def block(name, t, skip=None):
            layer = getattr(net, name)
            bn = layer.bn
            y = ops().conv3d(t, layer.conv.weight, torch.zeros(layer.out_channels, device=DEV), stride=layer.stride, pad=1, relu=False, transposed=layer.transposed)
            side = ops().batch_norm_train(y.clone(), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked) > 0
            wrong = (side.cpu() != (r64["z"][name] > 0)).flatten().nonzero().flatten().tolist()
            assert not wrong, "%s: element %d takes another ReLU side on the device (z64 = %.3g)" % (name, wrong[0], float(r64["z"][name].flatten()[wrong[0]]))
            outs[name] = ops().batch_norm_train(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, skip=skip)
            return outs[name]

        t = block("conv2", block("conv1", block("conv0", x.to(DEV))))
        t = block("conv6", block("conv5", block("conv4", block("conv3", t))))
        t = block("conv11", block("conv9", block("conv7", t, outs["conv4"]), outs["conv2"]), outs["conv0"])
        assert torch.equal(t, cost0)
    net.load_state_dict(sd)


@pytest.fixture
def route_calls(monkeypatch):
    o, n = ops(), {"conv": 0, "bn": 0, "layer": 0, "bare": 0}
    for name, key in (("conv3d", "conv"), ("batch_norm_train", "bn"), ("conv3d_bn_train", "layer"), ("conv3d_train", "bare")):
        def counted(*a, _real=getattr(o, name), _key=key, **k):
            n[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(o, name, counted)
    return n


def test_routes_by_call_count_and_caches(route_calls):
    case = TC.MODULE_CASES[0]
    x, R1, R2 = TC.module_inputs(case)
    xd = x.to(DEV)
    net = BC.randomise_train(M().CostRegNet(case[0], case[1], batch_stats="device", training="device"), case[3]).to(DEV)

    def count(f):
        for k in route_calls:
            route_calls[k] = 0
        out = f()
        return out, (route_calls["layer"], route_calls["bare"], route_calls["conv"], route_calls["bn"])

    (cost, prob), n = count(lambda: net(xd))                                 # train() + grad: the new route
    assert n == (10, 1, 0, 0) and cost.grad_fn is not None and prob.grad_fn is not None
    with torch.no_grad():
        (cost, prob), n = count(lambda: net(xd))                             # train() + no_grad: the batch-statistic route
    assert n == (0, 0, 11, 10) and cost.grad_fn is None
    net.eval()
    with torch.no_grad():
        _, n = count(lambda: net(xd))                                        # eval() + no_grad: the folded route
    assert n == (0, 0, 11, 0)
    (cost, prob), n = count(lambda: net(xd))                                 # eval() + grad: torch's layers
    assert n == (0, 0, 0, 0) and cost.grad_fn is not None
    cpu = BC.randomise_train(M().CostRegNet(case[0], case[1], batch_stats="device", training="device"), case[3])
    (cost, prob), n = count(lambda: cpu(x))                                  # a CPU module and input: torch's layers
    assert n == (0, 0, 0, 0) and cost.grad_fn is not None and not cost.is_cuda


def test_routes_of_the_other_keywords_and_the_second_step(route_calls):
    case = TC.MODULE_CASES[0]
    x, R1, R2 = TC.module_inputs(case)
    xd = x.to(DEV)

    def layer_calls(net, inp):
        route_calls["layer"] = 0
        out = net(inp)
        return out, route_calls["layer"]

    plain = BC.randomise_train(M().CostRegNet(case[0], case[1]), case[3]).to(DEV)                  # the default keyword: torch's layers
    (cost, _), n = layer_calls(plain, xd)
    assert n == 0 and cost.grad_fn is not None
    off = BC.randomise_train(M().CostRegNet(case[0], case[1], inference="torch", training="device"), case[3]).to(DEV)
    assert layer_calls(off, xd)[1] == 0
    net = BC.randomise_train(M().CostRegNet(case[0], case[1], training="device"), case[3]).to(DEV)
    net.conv3.bn.momentum = None                                               # a cumulative average is not built: torch's route
    assert layer_calls(net, xd)[1] == 0
    net.conv3.bn.momentum = 0.1
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        net(torch.rand((1, 8, 8, 8, 8), device=DEV))
    # two steps: the second forward + backward uses the updated weights (the packed caches follow the weights' versions)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    (cost, prob), n = layer_calls(net, xd)
    assert n == 10
    ((cost * R1.to(DEV)).sum() + (prob * R2.to(DEV)).sum()).backward()
    with torch.no_grad():
        for p in net.parameters():
            p.sub_(1e-3 * p.grad)
            p.grad = None
    sd2 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert not torch.equal(sd["conv0.conv.weight"], sd2["conv0.conv.weight"])
    X = xd.clone().requires_grad_(True)
    cost, prob = net(X)
    ((cost * R1.to(DEV)).sum() + (prob * R2.to(DEV)).sum()).backward()
    r64, r32 = TC.cost_reg_net(x, sd2, torch.float64, R1, R2), TC.cost_reg_net(x, sd2, torch.float32, R1, R2)
    if not TC.relu_offenders(r64, r32, sd2):                                  # (the condition is asserted for the first step's weights only)
        held("second step cost", cost.detach(), r64["cost"], r32["cost"])
        held("second step grad x", X.grad, r64["grad_x"], r32["grad_x"])
        held("second step grad conv0.conv.weight", net.conv0.conv.weight.grad, r64["grads"]["conv0.conv.weight"], r32["grads"]["conv0.conv.weight"])
    stale = TC.cost_reg_net(x, dict(sd2, **{k: v for k, v in sd.items() if k.endswith("conv.weight") or k == "prob.weight"}), torch.float64)
    assert float((cost.detach().cpu().double() - r64["cost"]).abs().max()) < 0.01 * float((stale["cost"] - r64["cost"]).abs().max())


def test_cascade_with_cnns_trains_end_to_end_on_the_device_route(route_calls):
    V, H, W, ndepths = 3, 32, 32, [48, 32, 8]
    net = M().CascadeMVSNet.with_cnns(ndepths=ndepths, training="device")
    for i, module in enumerate([net.feature] + list(net.cost_regularization)):
        MC.randomise(module, 95 + i)
    net = net.to(DEV).train()
    g = torch.Generator().manual_seed(99)
    imgs = torch.rand(1, V, 3, H, W, generator=g).to(DEV)
    affine, affine_inv = (t.to(DEV) for t in S.cameras(V, H, W, seed=100))
    near_far = torch.tensor([2.0, 11.0], device=DEV)
    vol, conf, depth, outputs = net(imgs, affine, affine_inv, near_far, pad=0)
    assert route_calls["layer"] == 30 and route_calls["bare"] == 3
    from uc_nerf_amd.utils.loss import cas_mvsnet_loss_device
    keys = ["stage1", "stage2", "stage3"]
    gts = {k: 2.0 + 9.0 * torch.rand(outputs[k]["depth"].shape, generator=g) for k in keys}
    weights = {k: torch.ones(outputs[k]["depth"].shape) for k in keys}
    total, _ = cas_mvsnet_loss_device({k: outputs[k] for k in keys}, gts, weights)
    (total + 1e-3 * vol.square().mean() + 1e-3 * conf.mean()).backward()
    for k, p in net.cost_regularization.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert any(bool(p.grad.abs().sum() > 0) for p in net.cost_regularization.parameters())
