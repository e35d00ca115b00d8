"""The conv3d kernels of csrc/conv3d.hip on the GPU against torch on the CPU: bit-equal on an integer lattice (every sum stays below 2^24, so
the order of the sums cannot matter), a single one in the input reading the kernel out, the epilogue (identity, NaN through the ReLU, the skip
after the activation), and determinism / independence of the batch."""
import math

import pytest
import torch
import torch.nn.functional as F

import mvs_cnn_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def ops():
    from uc_nerf_amd import ops as o
    return o


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ref_transposed(x, w, b=None):
    return F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)


# ------------------------------------------------------------------------------------------------ 1. exact lattice
# (n, cin, cout, K, stride, pad, D, H, W).  |x|, |w|, |bias|, |skip| <= 8: a sum of 33 * 27 products of at most 64 stays below 2^16.
# The last case: two images of 5 x 7 x 11 = 385 voxels each, 770 in all -- not a multiple of the 256-voxel block or the 16-voxel tile, and a
# tile that spans the two images.
LATTICE = ((1, 8, 8, 3, 1, 1, 4, 5, 7), (1, 8, 16, 3, 2, 1, 8, 8, 8), (1, 4, 8, 3, 2, 1, 5, 7, 9), (1, 16, 1, 3, 1, 1, 3, 4, 5), (1, 3, 5, 1, 1, 0, 2, 3, 4),
           (1, 33, 65, 3, 1, 1, 3, 3, 3), (2, 8, 8, 3, 1, 1, 5, 7, 11))


@pytest.mark.parametrize("n,cin,cout,K,stride,pad,D,H,W", LATTICE)
def test_forward_on_an_integer_lattice_is_bit_equal_to_torch_cpu(n, cin, cout, K, stride, pad, D, H, W):
    x = MC.lattice((n, cin, D, H, W), 8, 1)
    w = MC.lattice((cout, cin, K, K, K), 8, 2)
    b = MC.lattice((cout,), 8, 3)
    conv = F.conv3d(x, w, b, stride=stride, padding=pad)
    skip = MC.lattice(tuple(conv.shape), 8, 4)
    packed = ops().conv3d_pack(w.to(DEV))
    assert (packed.cin, packed.cout, packed.K, packed.transposed) == (cin, cout, K, False)
    for relu in (True, False):
        act = F.relu(conv) if relu else conv
        got = ops().conv3d(x.to(DEV).requires_grad_(True), packed, b.to(DEV), stride=stride, pad=pad, relu=relu)
        assert not got.requires_grad and same_bits(got, act), (relu, (got.cpu() - act).abs().max())
        got = ops().conv3d(x.to(DEV), packed, b.to(DEV), stride=stride, pad=pad, relu=relu, skip=skip.to(DEV))
        assert same_bits(got, act + skip), (relu, "skip", (got.cpu() - act - skip).abs().max())
    got = ops().conv3d(x.to(DEV), w.to(DEV), b.to(DEV), stride=stride, pad=pad, relu=False)          # a raw weight is packed on the spot
    assert same_bits(got, conv)


# (cin, cout, D, H, W)
@pytest.mark.parametrize("cin,cout,D,H,W", ((8, 4, 1, 1, 1), (16, 8, 2, 3, 5), (33, 17, 3, 2, 2)))
def test_transposed_on_an_integer_lattice_is_bit_equal_to_torch_cpu(cin, cout, D, H, W):
    n = 2
    x = MC.lattice((n, cin, D, H, W), 8, 5)
    w = MC.lattice((cin, cout, 3, 3, 3), 8, 6)
    b = MC.lattice((cout,), 8, 7)
    conv = ref_transposed(x, w, b)
    assert conv.shape == (n, cout, 2 * D, 2 * H, 2 * W)
    skip = MC.lattice(tuple(conv.shape), 8, 8)
    packed = ops().conv3d_pack(w.to(DEV), transposed=True)
    assert (packed.cin, packed.cout, packed.K, packed.transposed) == (cin, cout, 3, True)
    for relu in (True, False):
        act = F.relu(conv) if relu else conv
        got = ops().conv3d(x.to(DEV), packed, b.to(DEV), stride=2, pad=1, relu=relu, skip=skip.to(DEV), transposed=True)
        assert same_bits(got, act + skip), (relu, (got.cpu() - act - skip).abs().max())
    got = ops().conv3d(x.to(DEV), w.to(DEV), b.to(DEV), stride=2, pad=1, relu=False, transposed=True)
    assert same_bits(got, conv)


# ------------------------------------------------------------------------------------------------ 2. one-hot
@pytest.mark.parametrize("cin,cout,K,stride,pad", ((3, 5, 3, 1, 1), (2, 20, 3, 2, 1), (4, 3, 1, 1, 0)))
def test_a_single_one_reads_out_the_flipped_kernel(cin, cout, K, stride, pad):
    D, H, W = 4, 5, 6
    g = torch.Generator().manual_seed(5)
    w = torch.randn(cout, cin, K, K, K, generator=g)                    # any floats: one product 1 * w and zeros, nothing rounds
    packed = ops().conv3d_pack(w.to(DEV))
    OD, OH, OW = ((s + 2 * pad - K) // stride + 1 for s in (D, H, W))
    spots = [(0, 0, 0), (D - 1, H - 1, W - 1), (0, H - 1, 0)] + [(1 + pd, 1 + ph, 2 + pw) for pd in (0, 1) for ph in (0, 1) for pw in (0, 1)]
    x = torch.zeros(len(spots), cin, D, H, W)
    for i, (z0, y0, x0) in enumerate(spots):
        x[i, i % cin, z0, y0, x0] = 1.
    got = ops().conv3d(x.to(DEV), packed, torch.zeros(cout, device=DEV), stride=stride, pad=pad, relu=False).cpu()
    assert got.shape == (len(spots), cout, OD, OH, OW)
    for i, (z0, y0, x0) in enumerate(spots):
        want = torch.zeros(cout, OD, OH, OW)
        for oz in range(OD):
            for oy in range(OH):
                for ox in range(OW):
                    kz, ky, kx = z0 - stride * oz + pad, y0 - stride * oy + pad, x0 - stride * ox + pad
                    if 0 <= kz < K and 0 <= ky < K and 0 <= kx < K:
                        want[:, oz, oy, ox] = w[:, i % cin, kz, ky, kx]
        assert torch.equal(got[i], want), (i, z0, y0, x0)
        assert int((got[i] != 0).sum()) == int((want != 0).sum()) > 0


def test_a_single_one_reads_out_the_unflipped_kernel_of_the_transposed_form():
    cin, cout, D, H, W = 3, 6, 3, 3, 4
    g = torch.Generator().manual_seed(6)
    w = torch.randn(cin, cout, 3, 3, 3, generator=g)
    packed = ops().conv3d_pack(w.to(DEV), transposed=True)
    spots = [(0, 0, 0), (D - 1, H - 1, W - 1), (1, 1, 2), (0, 2, 1)]
    x = torch.zeros(len(spots), cin, D, H, W)
    for i, s in enumerate(spots):
        x[(i, i % cin) + s] = 1.
    got = ops().conv3d(x.to(DEV), packed, torch.zeros(cout, device=DEV), stride=2, pad=1, relu=False, transposed=True).cpu()
    assert got.shape == (len(spots), cout, 2 * D, 2 * H, 2 * W)
    classes = set()
    for i, (z0, y0, x0) in enumerate(spots):
        want = torch.zeros(cout, 2 * D, 2 * H, 2 * W)
        for kz in range(3):
            for ky in range(3):
                for kx in range(3):
                    oz, oy, ox = 2 * z0 - 1 + kz, 2 * y0 - 1 + ky, 2 * x0 - 1 + kx     # the kernel lands unflipped around 2 * position
                    if 0 <= oz < 2 * D and 0 <= oy < 2 * H and 0 <= ox < 2 * W:
                        want[:, oz, oy, ox] = w[i % cin, :, kz, ky, kx]
                        classes.add((oz & 1, oy & 1, ox & 1))
        assert torch.equal(got[i], want), (i, z0, y0, x0)
        assert int((got[i] != 0).sum()) == int((want != 0).sum()) > 0
    assert len(classes) == 8                                            # every output parity class was written by some tap


# ------------------------------------------------------------------------------------------------ 3. the epilogue
@pytest.mark.parametrize("cout", (1, 8, 20))
def test_identity_passes_negatives_nan_survives_relu_and_skip_comes_after_the_activation(cout):
    cin, D, H, W = 2, 2, 3, 4
    x = torch.ones(1, cin, D, H, W)
    w = torch.zeros(cout, cin, 1, 1, 1)
    w[:, 0] = -1.                                                       # pre-activation -1 + bias everywhere
    b = torch.zeros(cout)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    assert torch.equal(ops().conv3d(xd, wd, bd, relu=False).cpu(), torch.full((1, cout, D, H, W), -1.))
    assert torch.equal(ops().conv3d(xd, wd, bd, relu=True).cpu(), torch.zeros(1, cout, D, H, W))
    skip = torch.full((1, cout, D, H, W), 2.5)
    assert torch.equal(ops().conv3d(xd, wd, bd, relu=True, skip=skip.to(DEV)).cpu(), skip)          # relu(-1) + 2.5, not relu(-1 + 2.5)
    assert torch.equal(ops().conv3d(xd, wd, bd, relu=False, skip=skip.to(DEV)).cpu(), skip - 1.)
    xn = x.clone()
    xn[0, 0, 1, 2, 3] = math.nan
    got = ops().conv3d(xn.to(DEV), wd, bd, relu=True).cpu()
    assert bool(torch.isnan(got[0, :, 1, 2, 3]).all()) and int(torch.isnan(got).sum()) == cout


# ------------------------------------------------------------------------------------------------ 4. determinism and the batch
@pytest.mark.parametrize("transposed", (False, True))
def test_two_calls_give_the_same_bits_and_an_image_does_not_depend_on_its_batch(transposed):
    g = torch.Generator().manual_seed(9)
    cin, cout, D, H, W = 16, 8, 5, 6, 7
    x = torch.randn(3, cin, D, H, W, generator=g).to(DEV)
    w = (torch.randn((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), generator=g) * 0.1).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    packed = ops().conv3d_pack(w, transposed=transposed)
    kw = dict(stride=2, pad=1, transposed=True) if transposed else dict(stride=1, pad=1)
    first = ops().conv3d(x, packed, b, **kw)
    again = ops().conv3d(x, packed, b, **kw)
    assert same_bits(first, again)
    alone = ops().conv3d(x[1:2].contiguous(), packed, b, **kw)
    assert same_bits(alone, first[1:2])
    want = (ref_transposed(x.cpu().double(), w.cpu().double(), b.cpu().double()) if transposed
            else F.conv3d(x.cpu().double(), w.cpu().double(), b.cpu().double(), padding=1)).relu()
    assert float((first.cpu().double() - want).abs().max()) < 1e-4      # (a sanity scale; the error bars are in test_hip_mvs_cnn.py)
