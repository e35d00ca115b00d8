"""The forward of the cascade link on the GPU at its edges: ucnerf_depth_hypotheses against the float64 chain of tests/cascade_edge_cases.py (the
cases, and the proofs that they are what they claim: tests/test_cascade_edges_host.py).

  A  exact lattice        torch.equal against the float64 chain, a second launch bit-identical
  B  footprint read-out   one launch per one-hot cur_depth pixel: zero outside the float64 footprint, the weights inside, every plane the same
  C  depth chunks         D = 7 .. 49 against float64; the line through the device's own planes 0 and D - 1; guard bands around the output
  D  the device interval  interval = [far - near] is the default, bit for bit; half and double follow the chain; row mode reads neither
  E  non-finite depths    NaN / +inf / -inf positions as torch's own float32 op chain has them; the backward on the same inputs
  F  continuous cases     |device - float64| <= cascade_stubs.bar(far) = 16 * 2^-23 * far, no element excluded; the share is printed and recorded

Run on the GPU box:  python -m pytest tests/test_hip_cascade_edges.py -m gpu -q -s   (prints the measured shares; profiles/cascade_edges.md)
"""
import pytest
import torch

import cascade_edge_cases as E
import cascade_stubs as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHARES = []                        # device error / bar of every comparison with the float64 chain this run made
GUARD = 256                        # floats on each side of the output
GUARD_BITS, FILL_BITS = 0x7FC0DEAD, 0x7FC0BEEF          # two NaN patterns: the guard bands, and the output before the launch


def ops():
    from uc_nerf_amd import ops as _ops
    return _ops


def dev(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def run(c, interval="case", **over):
    """ops.depth_hypotheses on a case of cascade_edge_cases; `interval`: a number (passed as a one-element device tensor), None, or the case's own."""
    c = dict(c, **over)
    iv = c["interval"] if interval == "case" else interval
    return ops().depth_hypotheses(c["D"], c["hw"], cur_depth=dev(c["cur"]), near_far=torch.tensor([c["near"], c["far"]], device=DEV), k=c["k"],
                                  full_hw=c["HW"], pad=c["pad"], interval=None if iv is None else torch.tensor([iv], dtype=torch.float32, device=DEV))


def held(name, got, want64, bar):
    """got (device, float32) within `bar` of the float64 reference on every element; the share of the bar is printed and recorded."""
    assert got.shape == want64.shape and got.dtype == torch.float32, (name, got.shape, want64.shape)
    err = (got.cpu().double() - want64).abs().max().item()
    SHARES.append(err / bar)
    assert err <= bar, "%s: %.3e > bar %.3e" % (name, err, bar)
    return err / bar


def border_repeats_the_edge(got, pad):
    inner = got[:, pad:got.shape[1] - pad, pad:got.shape[2] - pad]
    return torch.equal(got, torch.nn.functional.pad(inner.unsqueeze(0), (pad,) * 4, "replicate")[0])


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", list(E.LATTICE))
def test_forward_is_exact_on_the_lattice(name):
    c = E.lattice_case(name)
    want = E.reference(c)["out"]
    got, again = run(c), run(c)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.float32
    wrong = int((got.cpu().double() != want).sum())
    print("\n%s: %d of %d elements differ" % (name, wrong, got.numel()))
    assert torch.equal(got.cpu().double(), want)
    assert torch.equal(got, again)                                         # repeatability: two launches are bit-identical
    assert border_repeats_the_edge(got, c["pad"])
    # the interval as a host factor instead of a device value: k * interval folded into k, the device forms far - near itself
    span = c["far"] - c["near"]
    assert torch.equal(run(c, interval=None, k=c["k"] * c["interval"] / span), got)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("name", list(E.FOOTPRINT))
def test_one_hot_inputs_read_the_composed_footprint_out(name):
    hw0, HW, hw, D, pad = E.FOOTPRINT[name]
    exact = name.startswith("power_of_two")
    total, worst = 0, 0.0
    for i in range(hw0[0]):
        for j in range(hw0[1]):
            c = E.footprint_case(name, (i, j))
            want = E.reference(c)["out"]
            got = run(c).cpu()
            assert got.shape == want.shape
            outside = want == 0
            assert int((got[outside] != 0).sum()) == 0, "pixel (%d, %d) leaks outside its footprint" % (i, j)
            if exact:
                assert torch.equal(got.double(), want), (i, j)
            else:
                worst = max(worst, held("%s (%d, %d)" % (name, i, j), got, want, E.FOOT_BAR))
            assert all(torch.equal(got[d], got[0]) for d in range(1, D)), "planes differ for pixel (%d, %d)" % (i, j)
            total = total + got.double()
    ones = run(E.footprint_case(name)).cpu()
    share_sum = held(name + " sum of the one-hot responses", total.float(), torch.ones_like(total), E.FOOT_BAR)
    share_ones = held(name + " all ones", ones, torch.ones_like(total), E.FOOT_BAR)
    assert (total - ones.double()).abs().max().item() <= E.FOOT_BAR
    print("\n%s: %d launches; shares of the bar: one-hot %.3f, their sum %.3f, all ones %.3f" % (name, hw0[0] * hw0[1], worst, share_sum, share_ones))


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("D", E.CHUNK_DEPTHS)
def test_depth_chunks_against_float64(D):
    c = E.chunk_case(D)
    want = E.reference(c)["out"]
    got = run(c)
    bar = S.bar(c["far"])
    share = held(c["name"], got, want, bar)
    per_plane = (got.cpu().double() - want).abs().flatten(1).max(1)[0]
    assert (per_plane <= bar).all(), per_plane.tolist()
    # the volume is a line in d: every plane within the bar of the line through the device's own planes 0 and D - 1
    share_line = held(c["name"] + " line", got, E.line_through_the_ends(got.cpu()), bar)
    assert border_repeats_the_edge(got, c["pad"])
    print("\n%s: %.3f of the bar against float64 (worst plane %d), %.3f against the line through its own ends" % (c["name"], share, int(per_plane.argmax()), share_line))


@pytest.mark.parametrize("name", E.CHUNK_LATTICE)
def test_lattice_planes_lie_on_the_line_through_their_ends(name):
    got = run(E.lattice_case(name)).cpu()
    assert torch.equal(got.double(), E.line_through_the_ends(got))


def launch_between_guards(D, hw, pad, **fields):
    """The entry point itself (no wrapper) into a buffer with GUARD floats of one NaN pattern on each side and another NaN pattern in between;
    `fields`: the other members of the parameter struct, tensors as their addresses.  Both bands must come back untouched and every element between
    them written.  -> the output [D, h + 2 pad, w + 2 pad] on the host."""
    from uc_nerf_amd import _lib as L
    shape = (D, hw[0] + 2 * pad, hw[1] + 2 * pad)
    n = shape[0] * shape[1] * shape[2]
    buf = torch.full((n + 2 * GUARD,), FILL_BITS, dtype=torch.int32, device=DEV)
    buf[:GUARD] = GUARD_BITS
    buf[GUARD + n:] = GUARD_BITS
    p = L.DepthHypothesesParams()
    p.D, p.h, p.w, p.pad = D, hw[0], hw[1], pad
    for key, v in fields.items():
        setattr(p, key, v.data_ptr() if torch.is_tensor(v) else v)
    p.out = buf.data_ptr() + 4 * GUARD
    L.call("ucnerf_depth_hypotheses", p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu()
    assert (host[:GUARD] == GUARD_BITS).all() and (host[GUARD + n:] == GUARD_BITS).all(), "a guard band was written"
    body = host[GUARD:GUARD + n]
    assert int((body == FILL_BITS).sum()) == 0, "%d output elements were not written" % int((body == FILL_BITS).sum())
    return body.view(torch.float32).view(shape)


@pytest.mark.parametrize("name", E.GUARD_CASES)
def test_nothing_is_written_outside_the_output_and_every_element_inside_is(name):
    c = E.lattice_case(name)
    cur, nf, iv = dev(c["cur"]), torch.tensor([c["near"], c["far"]], device=DEV), torch.tensor([c["interval"]], dtype=torch.float32, device=DEV)
    got = launch_between_guards(c["D"], c["hw"], c["pad"], H=c["HW"][0], W=c["HW"][1], h0=cur.shape[0], w0=cur.shape[1], k=c["k"], cur_depth=cur, near_far=nf,
                                interval=iv)
    assert torch.equal(got.double(), E.reference(c)["out"])


# ------------------------------------------------------------------------------------------------ D
def test_the_device_interval_is_honoured():
    c = E.chunk_case(17)
    span32 = (torch.tensor(c["far"]) - torch.tensor(c["near"])).item()     # far - near as float32 forms it
    default = run(c)
    assert torch.equal(run(c, interval=span32), default)
    bar = S.bar(c["far"])
    for factor in (0.5, 2.0):
        iv = factor * (c["far"] - c["near"])
        got = run(c, interval=iv)
        share = held("%s interval x %.1f" % (c["name"], factor), got, E.reference(c, interval=iv)["out"], bar)
        moved = (got - default).abs().max().item()
        print("\ninterval x %.1f: %.3f of the bar against float64; moved the output by %.1f bars" % (factor, share, moved / bar))
        assert moved > 100 * bar                                           # (the host test holds the float64 chain to the same)


@pytest.mark.parametrize("pad", [0, 1])
def test_row_mode_reads_neither_near_far_nor_interval(pad):
    """The header: in row mode H, W, h0, w0, k, near_far and interval are not read.  The wrapper does not even hand them over, so the entry point
    is called directly with NaN in all three values (and between guard bands: D = 9 and 17 in row mode too)."""
    row = dev(torch.linspace(2.0, 11.0, 48))
    nan1, nan2 = torch.full((1,), float("nan"), device=DEV), torch.full((2,), float("nan"), device=DEV)
    for D in (9, 17):
        plain = ops().depth_hypotheses(D, (5, 7), row=row, pad=pad)
        held("row mode D %d" % D, plain, E.row_chain(row.cpu(), D, (5, 7), pad), S.bar(11.0))
        got = launch_between_guards(D, (5, 7), pad, D_in=48, row=row, near_far=nan2, interval=nan1, k=float("nan"))
        assert torch.equal(got, plain.cpu())


# ------------------------------------------------------------------------------------------------ E
def _nonfinite_cases():
    return [(name, kind, spot) for name in E.NONFINITE for kind in E.NONFINITE_KINDS for spot in E.NONFINITE_SPOTS] + [(name, "all", "three") for name in E.NONFINITE]


def _nonfinite_case(name, kind, spot):
    return E.nonfinite_all_three(name) if kind == "all" else E.nonfinite_case(name, kind, spot)


@pytest.mark.parametrize("name,kind,spot", _nonfinite_cases())
def test_nonfinite_depths_land_where_torch_puts_them(name, kind, spot):
    c = _nonfinite_case(name, kind, spot)
    want_classes = E.classes(E.stub_chain(c))                              # torch's own float32 ops on the CPU
    want = E.reference(c)["out"]
    got = run(c).cpu()
    got_classes = E.classes(got)
    census = lambda k: [int((k == q).sum()) for q in range(4)]             # noqa: E731
    print("\n%s: finite / NaN / +inf / -inf on the device %s, in torch %s" % (c["name"], census(got_classes), census(want_classes)))
    assert torch.equal(got_classes, want_classes)
    finite = want_classes == 0
    err = (got.double() - want)[finite].abs().max().item()
    print("%s: finite elements %.3f of the bar against float64" % (c["name"], err / S.bar(c["far"])))
    SHARES.append(err / S.bar(c["far"]))
    assert err <= S.bar(c["far"])


@pytest.mark.parametrize("name,kind,spot", _nonfinite_cases())
def test_backward_on_nonfinite_depths_follows_torch(name, kind, spot):
    """torch's clamp backward lets nothing through where c - half >= near (c + half <= far) is false, and it is false for a NaN: the gradient of a
    finite g_out is finite everywhere.  Bar: the recipe of tests/test_hip_cascade_grad.py."""
    c = _nonfinite_case(name, kind, spot)
    D, (h, w), pad = c["D"], c["hw"], c["pad"]
    g_out = torch.randn(D, h + 2 * pad, w + 2 * pad, generator=torch.Generator().manual_seed(5700))
    want = E.chain_grad64(c, g_out)
    x = c["cur"].clone().requires_grad_(True)
    S.hypotheses_chain(x, torch.tensor(c["near"]), torch.tensor(c["far"]), torch.tensor(c["k"]) * (torch.tensor(c["far"]) - torch.tensor(c["near"])), D, c["HW"],
                       c["hw"], pad)[0].backward(g_out)
    witness = (x.grad.double() - want).abs().max().item()
    bar = 4 * witness + 1e-6 * want.abs().max().item()
    got = ops().depth_hypotheses_bwd(dev(g_out), dev(c["cur"]), torch.tensor([c["near"], c["far"]], device=DEV), None, (D, h, w, pad, c["HW"][0], c["HW"][1], c["k"])).cpu()
    assert torch.equal(E.classes(got), E.classes(want)) and torch.isfinite(want).all()
    err = (got.double() - want).abs().max().item()
    print("\n%s backward: device distance %.3e / bar %.3e = %.3f; float32 witness %.3e" % (c["name"], err, bar, err / bar, witness))
    assert err <= bar


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("name", E.CONTINUOUS)
def test_continuous_cases_against_float64(name):
    c = E.continuous_case(name)
    want = E.reference(c)["out"]
    bar = S.bar(c["far"])
    got = run(c)
    share = held(name, got, want, bar)
    cpu_share = (E.stub_chain(c).double() - want).abs().max().item() / bar
    print("\n%s: device %.3f of the bar, float32 CPU chain %.3f of the bar (bar %.3e)" % (name, share, cpu_share, bar))
    assert border_repeats_the_edge(got, c["pad"])
    assert torch.equal(run(c), got)


# ------------------------------------------------------------------------------------------------ the wrapper's refusals that need device tensors
def test_wrapper_refusals():
    nf = torch.tensor([2.0, 11.0], device=DEV)
    cur = torch.rand(4, 5, device=DEV)
    with pytest.raises(RuntimeError, match="exactly one"):
        ops().depth_hypotheses(8, (4, 5), cur_depth=cur, row=torch.rand(48, device=DEV), near_far=nf, k=1 / 48)
    with pytest.raises(RuntimeError, match="must cover"):
        ops().depth_hypotheses(8, (4, 5), cur_depth=torch.rand(9, 5, device=DEV), near_far=nf, k=1 / 48, full_hw=(8, 10))          # h0 > H
    with pytest.raises(RuntimeError, match="must cover"):
        ops().depth_hypotheses(8, (4, 11), cur_depth=cur, near_far=nf, k=1 / 48, full_hw=(8, 10))                                   # w > W
    with pytest.raises(RuntimeError, match="negative size"):
        ops().depth_hypotheses(8, (4, 5), cur_depth=cur, near_far=nf, k=1 / 48, full_hw=(8, 10), pad=-1)
    with pytest.raises(RuntimeError, match="D = 1"):
        ops().depth_hypotheses(1, (4, 5), row=torch.rand(48, device=DEV))
    with pytest.raises(RuntimeError, match="near_far must hold"):
        ops().depth_hypotheses(8, (4, 5), cur_depth=cur, near_far=nf[:1], k=1 / 48)
    with pytest.raises(RuntimeError, match="near_far"):
        ops().depth_hypotheses(8, (4, 5), cur_depth=cur, k=1 / 48)


def test_zz_largest_share_of_the_bar():
    """Prints the largest device error / bar over the comparisons with the float64 chain this run made (profiles/cascade_edges.md records it)."""
    if SHARES:
        print("\nlargest share of the bar over %d comparisons: %.3f" % (len(SHARES), max(SHARES)))
        assert max(SHARES) <= 1.0
