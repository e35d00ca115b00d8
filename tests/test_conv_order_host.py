"""The cases of tests/conv_order_cases.py on the CPU: the exactness argument holds for every case (grids and magnitudes asserted, not assumed), the
restatement equals torch where no sum rounds and is a float32 convolution where sums do, and the cases CAN tell the documented summation order
from each alternative (a) .. (g): for every kernel variant some case differs from the alternative in at least 10 % of its outputs.  The measured
shares are in profiles/conv_order.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_order_cases as CC
import mvs_cnn_cases as MC

MIN_SHARE = 0.10


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_the_case_is_on_the_lattice_and_its_sums_stay_below_2_to_the_15(name):
    d = CC.data(name)
    kind, variant, n, cin, cout, K, stride, pad, size = CC.CASES[name]
    gemms = CC.operands(name)
    assert len(gemms) == (8 if kind == "conv3dT" else 1)
    for A, B in gemms:
        assert A.shape[0] == cout and A.shape[1] == B.shape[0]
        top = CC.check_lattice(A, B, d["b"], d["skip"])
        assert top < CC.SUM_BOUND
    if kind == "conv3dT":
        assert sorted(A.shape[1] for A, _ in gemms) == sorted(cin * t for t in (1, 2, 2, 2, 4, 4, 4, 8))
    else:
        assert gemms[0][0].shape[1] == cin * K ** len(size)
    x = d["x"]
    assert 0.08 < float((x == 0).mean()) < 0.18                          # about one in eight exactly 0
    if max(A.shape[1] for A, _ in gemms) > CC.RUN:
        assert float(np.abs(CC.restate(name)).max()) > 2.0 ** 6          # sums pass 2^6: float32 rounds on the 2^-18 grid
    assert variant == ("conv2d" if kind == "conv2d" else "%s_%s" % (kind, "single" if cout == 1 else "16" if cout <= 16 else "32"))
    if name in CC.ROW0_OF:
        first = CC.data(CC.ROW0_OF[name])
        assert np.array_equal(d["x"], first["x"]) and np.array_equal(d["w"][0], first["w"][0])


def test_the_fmaf_in_float64_is_the_fmaf():
    """One product and one addend whose exact sum needs 25 bits: rounded once it differs from multiply-round-add-round, and float64 gives the
    once-rounded value."""
    a, b, c = np.float32(2047 * 2.0 ** -10), np.float32(2045 * 2.0 ** -8), np.float32(64.0 + 3 * 2.0 ** -17)
    exact = float(a) * float(b) + float(c)
    assert exact == (2047 * 2045 + 64 * 2 ** 18 + 6) * 2.0 ** -18          # (float64 held it exactly)
    T = CC.gemm(np.array([[0.0, a]], np.float32), np.array([[0.0], [b]], np.float32), group=2)
    assert T.dtype == np.float32 and float(T[0, 0]) == float(np.float32(float(a) * float(b)))
    got = CC._r32(np.array([exact]))[0]
    assert got == float(np.float32(exact)) and abs(got - exact) <= 2.0 ** -18 and got != exact


@pytest.mark.parametrize("variant", CC.VARIANTS)
def test_every_alternative_order_shows_in_some_case_of_the_variant(variant):
    names = [n for n in sorted(CC.CASES) if CC.CASES[n][1] == variant]
    assert names
    table = {n: CC.shares(n) for n in names}
    for n in names:
        print("conv order shares %-16s %s" % (n, "  ".join("%s %.3f" % (a[:1], table[n][a]) for a in CC.ALTERNATIVES)))
    for alt in CC.ALTERNATIVES:
        best = max(table[n][alt] for n in names)
        assert best >= MIN_SHARE, (variant, alt, {n: table[n][alt] for n in names})


def test_blocking_alternatives_cannot_show_where_k_fits_one_run():
    """By construction: with k <= 16 there is one run under every blocking, and one run has nothing to fold."""
    s = CC.shares("c2_k16")
    assert s["a_chain"] == s["b_run16"] == s["c_run64"] == s["d_fold_desc"] == 0.0


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_restatement_is_a_float32_convolution_of_the_new_lattice(name):
    """A sanity bound on the restatement, not on the device: its distance from float64 torch is within 4 x the CPU float32 convolution's own."""
    kind, variant, n, cin, cout, K, stride, pad, size = CC.CASES[name]
    d = CC.data(name)
    ref64 = CC.torch_conv(kind, d["x"], d["w"], d["b"], stride, pad, torch.float64)
    cpu32 = CC.torch_conv(kind, d["x"], d["w"], d["b"], stride, pad, torch.float32)
    bar, err32 = MC.chain_bar(ref64, cpu32)
    mine = torch.from_numpy(np.array(CC.restate(name)))
    assert mine.shape == ref64.shape == CC.out_shape(name)
    err = float((mine.double() - ref64).abs().max())
    print("conv order %-16s restatement err %.3e  torch float32 err %.3e  bar %.3e" % (name, err, err32, bar))
    assert err <= bar, (err, bar)
    # the epilogue: relu and skip of the restatement against the same operations on its own pre-activation
    if kind != "conv2d":
        want = F.relu(mine) + torch.from_numpy(np.array(d["skip"]))
        assert np.array_equal(CC.bits(CC.restate(name, True, True)), CC.bits(want.numpy()))
    else:
        assert np.array_equal(CC.bits(CC.restate(name, True)), CC.bits(F.relu(mine).numpy()))


@pytest.mark.parametrize("n,cin,cout,K,stride,pad,D,H,W", CC.INT_CONV3D)
def test_restatement_equals_torch_on_the_integer_lattice_of_the_conv3d_tests(n, cin, cout, K, stride, pad, D, H, W):
    x, w, b = MC.lattice((n, cin, D, H, W), 8, 1), MC.lattice((cout, cin, K, K, K), 8, 2), MC.lattice((cout,), 8, 3)
    conv = F.conv3d(x, w, b, stride=stride, padding=pad)
    skip = MC.lattice(tuple(conv.shape), 8, 4)
    for relu in (True, False):
        want = (F.relu(conv) if relu else conv) + skip
        got = CC.conv3d(x.numpy(), w.numpy(), b.numpy(), stride, pad, relu, skip.numpy())
        assert np.array_equal(CC.bits(got), CC.bits(want.numpy())), relu
    for order in CC.ALTERNATIVES:                                         # nothing rounds: every order is the same sum
        assert np.array_equal(CC.bits(CC.conv3d(x.numpy(), w.numpy(), b.numpy(), stride, pad, order=order)), CC.bits(conv.numpy())), order


@pytest.mark.parametrize("cin,cout,D,H,W", CC.INT_CONV3DT)
def test_restatement_equals_torch_on_the_integer_lattice_of_the_transposed_tests(cin, cout, D, H, W):
    x, w, b = MC.lattice((2, cin, D, H, W), 8, 5), MC.lattice((cin, cout, 3, 3, 3), 8, 6), MC.lattice((cout,), 8, 7)
    conv = F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)
    skip = MC.lattice(tuple(conv.shape), 8, 8)
    for relu in (True, False):
        want = (F.relu(conv) if relu else conv) + skip
        got = CC.conv3d_transposed(x.numpy(), w.numpy(), b.numpy(), relu, skip.numpy())
        assert np.array_equal(CC.bits(got), CC.bits(want.numpy())), relu


@pytest.mark.parametrize("cin,cout,K,stride,pad,H,W", CC.INT_CONV2D)
def test_restatement_equals_torch_on_the_integer_lattice_of_the_conv2d_tests(cin, cout, K, stride, pad, H, W):
    x, w, b = MC.lattice((3, cin, H, W), 4, 1), MC.lattice((cout, cin, K, K), 2, 2), MC.lattice((cout,), 3, 3)   # (lpips_cases.lattice is the same draw)
    conv = F.conv2d(x, w, b, stride=stride, padding=pad)
    for relu in (True, False):
        got = CC.conv2d(x.numpy(), w.numpy(), b.numpy(), stride, pad, relu)
        assert np.array_equal(CC.bits(got), CC.bits((F.relu(conv) if relu else conv).numpy())), relu
