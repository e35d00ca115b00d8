"""The summation order of the two convolution kernels on the GPU (csrc/lpips.hip: ucnerf_conv2d_bias_relu; csrc/conv3d.hip: ucnerf_conv3d, its
16-row and 32-row tiles, the cout == 1 VALU kernel and the transposed form), held BIT FOR BIT to the restatement of tests/conv_order_cases.py:
runs of 32 consecutive k, each an fmaf chain over ascending k from +0, folded ascending, then + bias, the activation, + skip.  The inputs lie
on a lattice where float32 rounds (so the order shows) and float64 numpy restates every fmaf exactly; tests/test_conv_order_host.py shows that
the cases tell the documented order from seven alternatives.  A row's bits must not depend on the tile height or on the kernel that computes
it.  The second half adds shapes the dispatch distinguishes, on the integer lattice of the older tests (bit-equal to torch on the CPU, every
sum exact).  profiles/conv_order.md has the measured picture."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_order_cases as CC
import mvs_cnn_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
GUARD = 64


def ops():
    from uc_nerf_amd import ops as o
    return o


def L():
    from uc_nerf_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV).contiguous()      # (a copy: the cached cases are read-only)


def tbits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(tbits(a), tbits(b))


def launch(name, relu, skip, w=None):
    """One launch of a case through the torch wrapper -> numpy.  `w`: another weight of the case's geometry."""
    kind, _, n, cin, cout, K, stride, pad, size = CC.CASES[name]
    d = CC.data(name)
    w = d["w"] if w is None else w
    if kind == "conv2d":
        assert not skip
        return ops().conv2d_bias_relu(dev(d["x"]), ops().conv2d_pack(dev(w)), dev(d["b"]), stride=stride, pad=pad, relu=relu).cpu().numpy()
    T = kind == "conv3dT"
    packed = ops().conv3d_pack(dev(w), transposed=T)
    b = d["b"] if packed.cout == cout else np.zeros(packed.cout, np.float32)
    return ops().conv3d(dev(d["x"]), packed, dev(b), stride=stride, pad=pad, relu=relu, skip=dev(d["skip"]) if skip else None, transposed=T).cpu().numpy()


def assert_order(name, got, relu, skip):
    want = CC.restate(name, relu, skip)
    assert got.shape == want.shape
    bad = CC.bits(got) != CC.bits(want)
    if bad.any():                                                        # which order IS it, then: differing elements per candidate
        raise AssertionError((name, relu, skip, int(bad.sum()), bad.size, CC.closest(name, got, relu, skip)))


# ------------------------------------------------------------------------------------------------ 1. the documented order, bit for bit
@pytest.mark.parametrize("name", [n for n in sorted(CC.CASES) if CC.CASES[n][0] != "conv2d"])
def test_conv3d_follows_the_documented_order_bit_for_bit(name):
    for relu in (False, True):
        for skip in (False, True):
            assert_order(name, launch(name, relu, skip), relu, skip)


@pytest.mark.parametrize("name", [n for n in sorted(CC.CASES) if CC.CASES[n][0] == "conv2d"])
def test_conv2d_follows_the_documented_order_bit_for_bit(name):
    for relu in (False, True):
        assert_order(name, launch(name, relu, False), relu, False)


# ------------------------------------------------------------------------------------------------ 2. one order whatever the kernel
@pytest.mark.parametrize("name", sorted(CC.ROW0_OF))
def test_the_single_channel_kernel_gives_the_bits_of_row_0_of_either_matrix_core_tile(name):
    """No restatement: `prob`'s VALU kernel against the same weight row inside a cout = 2 launch (16-row tile) and a cout = 17 launch (32-row)."""
    d = CC.data(name)
    single = launch(name, False, False)
    assert single.shape[1] == 1
    bias0 = d["b"][0]
    for cout in (2, 17):
        w = np.concatenate([d["w"], CC.more_rows(name, cout - 1)], 0)
        assert w.shape[0] == cout and np.array_equal(w[0], d["w"][0])
        tall = launch(name, False, False, w)                              # (bias 0: T itself)
        assert tall.shape[1] == cout
        row0 = (tall[:, :1] + bias0).astype(np.float32)
        assert np.array_equal(CC.bits(row0), CC.bits(single)), (cout, int((CC.bits(row0) != CC.bits(single)).sum()), single.size)
        assert float(np.abs(tall[:, 1:]).max()) > 0                      # the other rows were computed, not left out


@pytest.mark.parametrize("name", sorted(set(CC.ROW0_OF.values())))
def test_a_row_does_not_depend_on_the_tile_height(name):
    """The cout = 8 output of a 16-row case against rows 0 .. 7 of a cout = 20 launch (32-row tile) built from the same rows."""
    d = CC.data(name)
    assert d["w"].shape[0] == 8
    low = launch(name, False, False)
    w = np.concatenate([d["w"], CC.more_rows(name, 12)], 0)
    tall = launch(name, False, False, w)
    assert tall.shape[1] == 20
    rows = (tall[:, :8] + d["b"].reshape(1, 8, 1, 1, 1)).astype(np.float32)
    assert np.array_equal(CC.bits(rows), CC.bits(low)), (int((CC.bits(rows) != CC.bits(low)).sum()), low.size)


# ------------------------------------------------------------------------------------------------ 3. nothing behind the output is written
class Out:
    """A device output of prod(shape) floats with GUARD floats of -7.0 behind it."""

    def __init__(self, *shape):
        self.shape, self.count = shape, int(np.prod(shape))
        self.t = torch.full((self.count + GUARD,), -7.0, device=DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        a = self.t.cpu().numpy()
        assert (a[self.count:] == -7.0).all(), "the guard behind an output was written"
        return a[:self.count].reshape(self.shape)


def call(name, p):
    lib = L().lib()
    rc = getattr(lib, name)(C.addressof(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc, lib.ucnerf_last_error())
    torch.cuda.synchronize()


def test_conv3d_through_the_c_abi_leaves_the_guard_behind_y_untouched():
    name = "c3_32_two_tiles"                                             # 18 voxels of 33 channels: the last tile of either axis is mostly empty
    kind, _, n, cin, cout, K, stride, pad, size = CC.CASES[name]
    d = CC.data(name)
    x, b, skip = dev(d["x"]), dev(d["b"]), dev(d["skip"])
    packed = ops().conv3d_pack(dev(d["w"]))
    y = Out(*CC.out_shape(name))
    p = L().Conv3dParams()
    p.n, p.cin, p.D, p.H, p.W, p.cout, p.K, p.stride, p.pad = n, cin, size[0], size[1], size[2], cout, K, stride, pad
    p.relu, p.transposed, p.packed_floats = 1, 0, packed.packed.numel()
    p.x, p.packed, p.bias, p.skip, p.y = x.data_ptr(), packed.packed.data_ptr(), b.data_ptr(), skip.data_ptr(), y.ptr
    call("ucnerf_conv3d", p)
    assert_order(name, y.get(), True, True)


def test_conv2d_through_the_c_abi_leaves_the_guard_behind_y_untouched():
    name = "c2_k576"                                                     # 20 pixels of 70 channels
    kind, _, n, cin, cout, K, stride, pad, size = CC.CASES[name]
    d = CC.data(name)
    x, b = dev(d["x"]), dev(d["b"])
    packed = ops().conv2d_pack(dev(d["w"]))
    y = Out(*CC.out_shape(name))
    p = L().Conv2dParams()
    p.n, p.cin, p.H, p.W, p.cout, p.K, p.stride, p.pad, p.relu = n, cin, size[0], size[1], cout, K, stride, pad, 0
    p.x, p.packed, p.bias, p.shift, p.scale, p.y = x.data_ptr(), packed.packed.data_ptr(), b.data_ptr(), None, None, y.ptr
    call("ucnerf_conv2d_bias_relu", p)
    assert_order(name, y.get(), False, False)


# ------------------------------------------------------------------------------------------------ 4. shape edges on the integer lattice
# (n, cin, cout, K, stride, pad, D, H, W), |x|, |w|, |bias|, |skip| <= 8: 64 * 27 products of at most 64 stay below 2^17, every sum is exact.
EDGES_3D = (
    (1, 4, 8, 3, 1, 2, 2, 3, 4), (1, 4, 8, 3, 2, 2, 2, 3, 4), (1, 4, 8, 3, 1, 3, 2, 3, 4), (1, 4, 8, 3, 2, 3, 2, 3, 4),    # pad 2, 3: outputs of padding alone
    (2, 5, 8, 1, 2, 0, 3, 4, 5), (1, 5, 8, 1, 1, 1, 2, 3, 4),                                                          # K = 1 strided, K = 1 padded
    (1, 4, 8, 3, 1, 1, 1, 4, 5), (1, 4, 8, 3, 2, 1, 1, 4, 5), (1, 4, 8, 3, 1, 1, 4, 1, 5), (1, 4, 8, 3, 2, 1, 4, 1, 5),    # D = 1, H = 1, W = 1
    (1, 4, 8, 3, 1, 1, 4, 5, 1), (1, 4, 8, 3, 2, 1, 4, 5, 1), (1, 64, 64, 3, 1, 1, 1, 4, 5),                           # ... and stage 3's conv6
    (1, 1, 8, 3, 1, 1, 3, 4, 5),                                                                                       # cin = 1
    (1, 3, 16, 3, 1, 1, 2, 3, 4), (1, 3, 17, 3, 1, 1, 2, 3, 4), (1, 3, 32, 3, 1, 1, 2, 3, 4), (1, 3, 33, 3, 1, 1, 2, 3, 4))       # around the tile heights


@pytest.mark.parametrize("n,cin,cout,K,stride,pad,D,H,W", EDGES_3D)
def test_conv3d_shape_edges_on_the_integer_lattice_are_bit_equal_to_torch_cpu(n, cin, cout, K, stride, pad, D, H, W):
    x, w, b = MC.lattice((n, cin, D, H, W), 8, 11), MC.lattice((cout, cin, K, K, K), 8, 12), MC.lattice((cout,), 8, 13)
    conv = F.conv3d(x, w, b, stride=stride, padding=pad)
    skip = MC.lattice(tuple(conv.shape), 8, 14)
    if pad >= K:                                                         # the outer outputs see padding only: the bias
        assert torch.equal(conv[:, :, 0, 0, 0], b.expand(n, cout))
    packed = ops().conv3d_pack(w.to(DEV))
    for relu in (True, False):
        act = F.relu(conv) if relu else conv
        got = ops().conv3d(x.to(DEV), packed, b.to(DEV), stride=stride, pad=pad, relu=relu)
        assert same_bits(got, act), (relu, (got.cpu() - act).abs().max())
        got = ops().conv3d(x.to(DEV), packed, b.to(DEV), stride=stride, pad=pad, relu=relu, skip=skip.to(DEV))
        assert same_bits(got, act + skip), (relu, "skip", (got.cpu() - act - skip).abs().max())


# (n, cin, cout, D, H, W): 420 class voxels against the 256 of one 16-row block; 280 against the 128 of one 32-row block (140 per image: a
# 16-voxel tile spans the two)
@pytest.mark.parametrize("n,cin,cout,D,H,W", ((2, 8, 8, 5, 6, 7), (2, 8, 20, 4, 5, 7)))
def test_transposed_larger_than_one_block_on_the_integer_lattice_is_bit_equal_to_torch_cpu(n, cin, cout, D, H, W):
    x, w, b = MC.lattice((n, cin, D, H, W), 8, 15), MC.lattice((cin, cout, 3, 3, 3), 8, 16), MC.lattice((cout,), 8, 17)
    conv = F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)
    skip = MC.lattice(tuple(conv.shape), 8, 18)
    packed = ops().conv3d_pack(w.to(DEV), transposed=True)
    for relu in (True, False):
        act = F.relu(conv) if relu else conv
        got = ops().conv3d(x.to(DEV), packed, b.to(DEV), stride=2, pad=1, relu=relu, transposed=True)
        assert same_bits(got, act), (relu, (got.cpu() - act).abs().max())
        got = ops().conv3d(x.to(DEV), packed, b.to(DEV), stride=2, pad=1, relu=relu, skip=skip.to(DEV), transposed=True)
        assert same_bits(got, act + skip), (relu, "skip", (got.cpu() - act - skip).abs().max())


# (n, cin, cout, K, stride, pad, H, W): FeatureNet's layer kinds (K = 1, K = 5 / 2 pad 2, cout 8 / 16 / 32), a one-row image, and 3 x 35 = 105
# pixels, which is no multiple of the 64-pixel tile
EDGES_2D = ((2, 5, 8, 1, 1, 0, 5, 7), (2, 5, 8, 1, 1, 1, 5, 7), (1, 3, 8, 5, 2, 2, 9, 11), (1, 3, 8, 5, 2, 2, 1, 7), (2, 8, 16, 3, 2, 1, 1, 9),
            (1, 8, 8, 3, 1, 1, 5, 7), (1, 8, 16, 3, 1, 1, 5, 7), (1, 16, 32, 3, 1, 1, 5, 7), (3, 4, 8, 3, 1, 1, 5, 7))


@pytest.mark.parametrize("n,cin,cout,K,stride,pad,H,W", EDGES_2D)
def test_conv2d_shape_edges_on_the_integer_lattice_are_bit_equal_to_torch_cpu(n, cin, cout, K, stride, pad, H, W):
    x, w, b = MC.lattice((n, cin, H, W), 8, 21), MC.lattice((cout, cin, K, K), 8, 22), MC.lattice((cout,), 8, 23)
    conv = F.conv2d(x, w, b, stride=stride, padding=pad)
    packed = ops().conv2d_pack(w.to(DEV))
    for relu in (True, False):
        want = F.relu(conv) if relu else conv
        got = ops().conv2d_bias_relu(x.to(DEV), packed, b.to(DEV), stride=stride, pad=pad, relu=relu)
        assert same_bits(got, want), (relu, (got.cpu() - want).abs().max())
