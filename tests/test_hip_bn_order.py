"""The batch-norm kernels (csrc/bn.hip: ucnerf_bn_stats, ucnerf_bn_apply) at the sizes the networks run them at, held BIT FOR BIT to the
summation order include/ucnerf_hip.h documents, as restated in tests/bn_order_cases.py: the workspace triples, saved_mean, saved_var, both
running statistics and out, for every row of the case table (one quad per thread up to two full chunks per thread, 16-byte and 4-byte
accesses, slices with a ragged end, C = 65535).  Then one value of 1.0 among zeros at every slice, round, image and block edge (a value lost
or counted twice shows as mean 0 or 2 / N); the same values through every layout and alignment; NaN behind every input and guards behind every
output; a NaN channel between two clean ones; three badly conditioned inputs against float64; and CostRegNet at a layer past the P cap.

Every call goes through the raw entry points with NaN around every input, a sentinel around every output and a NaN workspace with guard
triples; `run` checks them after every call.  tests/test_bn_order_host.py guards the restatement; profiles/bn_order.md has the findings."""
import itertools

import numpy as np
import pytest
import torch

import bn_cases as BC
import bn_order_cases as OC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
NAN, SENTINEL, FRONT = float("nan"), -12345.0, 4


def L():
    from uc_nerf_amd import _lib
    return _lib


def M():
    from uc_nerf_amd.network import mvs_models
    return mvs_models


class Buf:
    """A float32 array on the device inside a larger allocation: FRONT + off floats before it and OC.GUARD behind it, all `fill`."""

    def __init__(self, shape, fill, off=0, values=None):
        self.shape, self.numel, self.fill = tuple(shape), int(np.prod(shape)), fill
        self.whole = torch.full((FRONT + off + self.numel + OC.GUARD,), fill, dtype=torch.float32, device=DEV)
        assert self.whole.data_ptr() % 16 == 0
        self.view = self.whole[FRONT + off:FRONT + off + self.numel]
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).reshape(-1)))
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == 4 * off

    def numpy(self):
        return self.view.cpu().numpy().reshape(self.shape)

    def surroundings_intact(self):
        around = torch.cat([self.whole[:self.whole.numel() - self.numel - OC.GUARD], self.whole[-OC.GUARD:]])
        want = torch.full_like(around, self.fill)
        return torch.equal(around.view(torch.int32), want.view(torch.int32))


def run(y, gamma, beta, rm, rv, skip=None, relu=True, inplace=False, y_off=0, out_off=0, skip_off=0, poison=NAN):
    """ucnerf_bn_stats then ucnerf_bn_apply on y [n,C,S] -> dict of numpy arrays under OC.NAMES.  `poison` surrounds y and skip and fills the
    workspace before the call; what surrounds the outputs is checked to be as it was."""
    n, C, S = y.shape
    P = L().lib().ucnerf_bn_partials(n, S)
    assert P == OC.partials(n * S)
    yb = Buf(y.shape, poison, y_off, y)
    sb = Buf(y.shape, poison, skip_off, skip) if skip is not None else None
    ob = yb if inplace else Buf(y.shape, SENTINEL, out_off)
    ws = torch.full(((C * P + 2) * 3,), poison, dtype=torch.float64, device=DEV)
    ws[-6:] = SENTINEL
    small = {k: Buf((C,), SENTINEL, 0, v) for k, v in (("weight", gamma), ("bias", beta), ("saved_mean", np.full(C, NAN)), ("saved_var", np.full(C, NAN)),
                                                    ("running_mean", rm), ("running_var", rv))}
    nbt = torch.tensor([3, -777], dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    s = L().BnStatsParams()
    s.n, s.C, s.S, s.workspace_triples, s.y, s.workspace = n, C, S, C * P, yb.ptr, ws.data_ptr()
    L().call("ucnerf_bn_stats", s, stream)
    a = L().BnApplyParams()
    a.n, a.C, a.S, a.workspace_triples, a.eps, a.momentum, a.relu = n, C, S, C * P, OC.EPS, OC.MOMENTUM, int(relu)
    a.y, a.workspace, a.skip, a.out = yb.ptr, ws.data_ptr(), sb.ptr if sb else None, ob.ptr
    for k, b in small.items():
        setattr(a, k, b.ptr)
    a.num_batches_tracked = nbt.data_ptr()
    L().call("ucnerf_bn_apply", a, stream)
    torch.cuda.synchronize()
    assert nbt.tolist() == [4, -777] and bool((ws[-6:] == SENTINEL).all())
    for k, b in list(small.items()) + [("y", yb), ("out", ob)] + ([("skip", sb)] if sb else []):
        assert b.surroundings_intact(), k
    if not inplace:
        assert np.array_equal(OC.bits(yb.numpy()), OC.bits(np.ascontiguousarray(y, dtype=np.float32)))       # the input is left alone
    if sb:
        assert np.array_equal(OC.bits(sb.numpy()), OC.bits(np.ascontiguousarray(skip, dtype=np.float32)))
    out = {k: small[k].numpy() for k in OC.NAMES[1:5]}
    out["workspace"], out["out"] = ws[:-6].cpu().numpy().reshape(C, P, 3), ob.numpy()
    return out


def run_case(name, relu=True, skip=False, **kw):
    d = OC.data(name)
    return run(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], skip=d["skip"] if skip else None, relu=relu, **kw)


def assert_bits(what, got, want, names=OC.NAMES):
    lines = [line for line in (OC.first_difference(k, got[k], want[k]) for k in names) if line]
    assert not lines, "%s:\n  %s" % (what, "\n  ".join(lines))


def header_counts(n, C, S):
    return np.broadcast_to(np.array(OC.slice_counts(n * S)[2], np.float64), (C, OC.partials(n * S)))


# ------------------------------------------------------------------------------------------------ 1. the documented order, bit for bit
@pytest.mark.parametrize("name", list(OC.CASES))
def test_follows_the_documented_order_bit_for_bit(name):
    n, C, S, _ = OC.CASES[name]
    for relu, skip in itertools.product((True, False), (False, True)):
        got = run_case(name, relu, skip)
        assert np.array_equal(got["workspace"][:, :, 0], header_counts(n, C, S))
        assert_bits("%s relu=%s skip=%s" % (name, relu, skip), got, OC.restate(name, relu, skip))
    assert_bits("%s in place" % name, run_case(name, True, True, inplace=True), OC.restate(name, True, True))


# ------------------------------------------------------------------------------------------------ 2. one value, every edge
@pytest.mark.parametrize("name", [k for k in OC.CASES if k not in ("c65535", "s1048576")])        # (the issue's rows with C of their own)
def test_one_value_at_every_edge(name):
    n, _, S, _ = OC.CASES[name]
    N = n * S
    positions = OC.one_value_positions(n, S)
    C = len(positions)                                                    # channel c holds its 1.0 at positions[c]
    y = OC.one_value(n, S, positions)
    g = np.random.default_rng(OC.seed_of(name) + 100)
    gamma, beta = (0.6 + 0.8 * g.random(C)).astype(np.float32), (0.3 * g.standard_normal(C)).astype(np.float32)
    rm, rv = (0.3 * g.standard_normal(C)).astype(np.float32), (0.5 + 1.5 * g.random(C)).astype(np.float32)
    got = run(y, gamma, beta, rm, rv, relu=False)
    # without the restatement: the header's counts, and the mean of one 1.0 among N - 1 zeros (lost: 0; counted twice: 2 / N)
    assert np.array_equal(got["workspace"][:, :, 0], header_counts(n, C, S)) and bool((got["workspace"][:, :, 0].sum(1) == N).all())
    off = np.abs(got["saved_mean"].astype(np.float64) - 1.0 / N) / np.spacing(np.float32(1.0 / N)).astype(np.float64)
    print("%s: %d positions %s, saved_mean within %.2f float32 spacings of 1 / N" % (name, C, positions, off.max()))
    assert bool((off <= 2.0).all()), [(positions[c], float(got["saved_mean"][c])) for c in np.nonzero(off > 2.0)[0]]
    P, Ls, _ = OC.slice_counts(N)
    holds = np.zeros((C, P), bool)
    holds[np.arange(C), np.array(positions) // Ls] = True
    assert np.array_equal(got["workspace"][:, :, 1] != 0, holds) and np.array_equal(got["workspace"][:, :, 2] != 0, holds)      # in its own slice
    ws = OC.stats(y)
    want = dict(OC.apply(np.array([[[0.0, 1.0]] * C], np.float32), ws, gamma, beta, rm, rv, relu=False), workspace=ws)
    want["out"] = np.where(y == 1.0, want["out"][:, :, 1:], want["out"][:, :, :1])          # (the epilogue is elementwise: restated once per distinct value)
    assert_bits("%s, one value at %s" % (name, positions), got, want)


# ------------------------------------------------------------------------------------------------ 3. layouts are the same function
@pytest.mark.parametrize("N", (OC.LAYOUT_N, 524292))
def test_layouts_and_alignments_give_the_same_bits(N):
    assert N % 4 == 0 and (N // 4) % 4 != 0
    g = np.random.default_rng(7200 + N)
    x, sk = (1.5 * g.standard_normal(N) + 0.5).astype(np.float32), g.standard_normal(N).astype(np.float32)
    one = [np.array([v], np.float32) for v in (0.9, -0.2, 0.1, 1.3)]

    def flat(r):
        return {k: (v.reshape(-1) if k == "out" else v) for k, v in r.items()}

    base = flat(run(x.reshape(1, 1, N), *one, skip=sk.reshape(1, 1, N)))                        # (1, N), every array 16-byte aligned
    for what, kw in (("y 4 bytes in", dict(y_off=1)), ("out 4 bytes in", dict(out_off=1)), ("skip 4 bytes in", dict(skip_off=1)),
                     ("all three 4 bytes in", dict(y_off=1, out_off=1, skip_off=1)), ("in place", dict(inplace=True)),
                     ("in place, 4 bytes in", dict(inplace=True, y_off=1))):
        assert_bits("(1, %d) %s" % (N, what), flat(run(x.reshape(1, 1, N), *one, skip=sk.reshape(1, 1, N), **kw)), base)
    for off in (0, 1):
        assert_bits("(4, %d) y_off=%d" % (N // 4, off), flat(run(x.reshape(4, 1, N // 4), *one, skip=sk.reshape(4, 1, N // 4), y_off=off)), base)
    # channel 1 of a [4, 3, S] tensor against the same values as [4, 1, S]
    y3, s3 = (1.5 * g.standard_normal((4, 3, N // 4)) + 0.5).astype(np.float32), g.standard_normal((4, 3, N // 4)).astype(np.float32)
    y3[:, 1], s3[:, 1] = x.reshape(4, N // 4), sk.reshape(4, N // 4)
    vec = [np.array([7.0, v[0], -7.0], np.float32) for v in one]
    got = run(y3, *vec, skip=s3)
    got = {k: (v[:, 1].reshape(-1) if k == "out" else v[1:2]) for k, v in got.items()}
    assert_bits("channel 1 of [4, 3, %d]" % (N // 4), got, base)


# ------------------------------------------------------------------------------------------------ 4. nothing outside the extent
@pytest.mark.parametrize("name", OC.GUARDED)
def test_nothing_outside_the_extent_is_read_or_written(name):
    for kw in (dict(), dict(y_off=1, skip_off=1, out_off=1), dict(inplace=True)):
        clean = run_case(name, True, True, poison=0.0, **kw)                # (run() holds the guards behind out, the workspace and the vectors)
        dirty = run_case(name, True, True, poison=NAN, **kw)
        assert not any(bool(np.isnan(v).any()) for v in dirty.values())
        assert_bits("%s %s, NaN around y and skip and in the workspace" % (name, kw), dirty, clean)
    assert_bits(name, clean, OC.restate(name, True, True))


# ------------------------------------------------------------------------------------------------ 5. channels do not mix
@pytest.mark.parametrize("shape", ((3, 3, 43691), (1, 3, 524292)), ids=str)
def test_a_nan_channel_leaves_its_neighbours_alone(shape):
    n, C, S = shape
    N = n * S
    P, Ls, counts = OC.slice_counts(N)
    g = np.random.default_rng(7300 + S)
    y, skip = (1.5 * g.standard_normal(shape) + 0.5).astype(np.float32), g.standard_normal(shape).astype(np.float32)
    vec = [(0.6 + 0.8 * g.random(C)).astype(np.float32), (0.3 * g.standard_normal(C)).astype(np.float32), (0.3 * g.standard_normal(C)).astype(np.float32),
           (0.5 + 1.5 * g.random(C)).astype(np.float32)]
    clean = run(y, *vec, skip=skip)
    bad = y.copy()
    i_nan, i_inf = 3 * Ls + 17, (P - 1) * Ls + counts[-1] - 1               # slice 3, and the last value of the last slice
    bad[i_nan // S, 1, i_nan % S], bad[i_inf // S, 1, i_inf % S] = np.nan, np.inf
    got = run(bad, *vec, skip=skip)
    for k in OC.NAMES:
        pick = (lambda v: v[:, [0, 2]]) if k == "out" else (lambda v: v[[0, 2]])
        assert OC.first_difference(k, pick(got[k]), pick(clean[k])) is None, k
    assert all(bool(np.isnan(got[k][1])) for k in OC.NAMES[1:5]) and bool(np.isnan(got["out"][:, 1]).all())      # a NaN stays, relu or not
    ws, ws0 = got["workspace"][1], clean["workspace"][1]
    hit = np.zeros(P, bool)
    hit[[3, P - 1]] = True
    assert np.array_equal(ws[:, 0], ws0[:, 0]) and np.array_equal(OC.bits(ws[~hit]), OC.bits(ws0[~hit]))
    assert bool(np.isnan(ws[3, 1:]).all()) and not bool(np.isfinite(ws[P - 1, 1:]).any())


# ------------------------------------------------------------------------------------------------ 6. conditioning, against float64
def held(name, got, ref64, cpu32):
    bar, err32 = BC.chain_bar(ref64, cpu32)
    err = float((torch.from_numpy(np.array(got)).double() - ref64).abs().max())
    print("%s: device %.3g, float32 cpu %.3g, ratio %.2f, bar %.3g, largest %.3g" % (name, err, err32, err / max(err32, 1e-30), bar, float(ref64.abs().max())))
    assert tuple(got.shape) == tuple(ref64.shape) and got.dtype == np.float32
    assert err <= bar, name


@pytest.mark.parametrize("kind", ("offset", "ramp", "constant_slice"))
@pytest.mark.parametrize("name", OC.CONDITIONING)
def test_conditioning_at_the_large_sizes_against_float64(name, kind):
    n, C, S, _ = OC.CASES[name]
    d = OC.data(name)
    y = OC.conditioning(kind, n, C, S, OC.seed_of(name) + 200)
    got = run(y, d["gamma"], d["beta"], d["rm"], d["rv"], skip=d["skip"], relu=True)
    t = {k: torch.from_numpy(np.array(v)) for k, v in d.items()}
    refs = []
    for dtype in (torch.float64, torch.float32):
        out, mean, var = BC.bn_train(torch.from_numpy(y), t["gamma"], t["beta"], dtype, relu=True, skip=t["skip"], eps=OC.EPS)
        refs.append((mean, var) + BC.running_update(t["rm"], t["rv"], mean, var, n * S, dtype, momentum=OC.MOMENTUM) + (out,))
    for k, r64, r32 in zip(OC.NAMES[1:], *refs):
        held("%s %s %s" % (k, name, kind), got[k], r64, r32)
    assert float(got["saved_var"].min()) >= 0.0 and bool(np.isfinite(got["out"]).all())
    if kind == "constant_slice":
        assert bool((got["workspace"][:, 1, 2] == 0.0).all()) and np.array_equal(got["workspace"][:, 1, 1], 2.5 + np.arange(C))
    ws = OC.stats(y)
    want = dict(OC.apply(y, ws, d["gamma"], d["beta"], d["rm"], d["rv"], relu=True, skip=d["skip"]), workspace=ws)
    assert_bits("%s %s" % (name, kind), got, want)                          # and the documented order here too


# ------------------------------------------------------------------------------------------------ 7. one module at a layer past the cap
def test_cost_reg_net_past_the_partial_cap_against_float64():
    shape = (1, 8, 8, 128, 144)                                             # conv0 and conv11: N = 147 456 values per channel
    N = shape[2] * shape[3] * shape[4]
    assert OC.regime(1, N)["P"] == 32 and OC.regime(1, N)["L"] == 4608 and OC.regime(1, N)["live_u"] == 2
    dev, ref = (BC.randomise_train(M().CostRegNet(8, 8, batch_stats=b), 441).to(DEV) for b in ("device", "torch"))
    assert dev.training and dev.batch_stats == "device" and ref.batch_stats == "torch"
    before = {k: v.detach().cpu().clone() for k, v in dev.state_dict().items()}
    x = torch.rand(shape, generator=torch.Generator().manual_seed(442))
    with torch.no_grad():
        cost, prob = dev(x.to(DEV))
        cost_t, prob_t = ref(x.to(DEV))
    c64, p64, s64 = BC.cost_reg_net(x, before, torch.float64)
    c32, p32, s32 = BC.cost_reg_net(x, before, torch.float32)
    theirs = ref.state_dict()

    def both(name, got, other, r64, r32):
        held(name, got.detach().cpu().numpy(), r64, r32)
        bar, _ = BC.chain_bar(r64, r32)
        err = float((got.detach().cpu().double() - other.detach().cpu().double()).abs().max())
        print("%s: the two routes differ by %.3g, bar %.3g" % (name, err, bar))
        assert err <= bar, name

    both("cost %s" % (shape,), cost, cost_t, c64, c32)
    both("prob %s" % (shape,), prob, prob_t, p64, p32)
    for k, v in dev.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 == int(s64[k]) == int(theirs[k]), k
        elif "running_" in k:
            both(k, v, theirs[k], s64[k], s32[k])
