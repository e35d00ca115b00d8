"""The cascade depth loss on the device (ucnerf_cas_loss_fwd / _bwd through ops.cas_loss and utils.loss.cas_mvsnet_loss_device).

Reference of every comparison: uc_nerf_amd.utils.loss.cas_mvsnet_loss on the CPU (tests/cas_loss_cases.py: `mirror`), in float64 where a
tolerance is involved, and fixture G15 from the reference's own Python -- never the device route itself.
  exact:        on the lattice of cas_loss_cases.lattice_stage loss and gradients are torch.equal to the float32 mirror;
  differential: relative loss error <= 1e-5, every gradient element within 4 float32 ulp of the float64 mirror (derivations: cas_loss_cases);
  capture:      the step that the boolean-mask route cannot enter -- zero_grad, loss, backward, Adam in ONE graph, replayed on NEW valid counts."""
import pytest
import torch

import cas_loss_cases as CC
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(t):
    return t.to(DEV)


def device_loss(stages, with_weight=True, keys=None, scale=None, status=None):
    """cas_mvsnet_loss_device on device copies of the stages: (total, last stage's loss, gradients of the estimates), all on the CPU."""
    from uc_nerf_amd.utils import loss as UL
    leaves = [dev(s[0]).requires_grad_(True) for s in stages]
    inputs, gt, w = CC.dicts([(e, dev(s[1]), dev(s[2])) for e, s in zip(leaves, stages)], keys)
    total, last = UL.cas_mvsnet_loss_device(inputs, gt, w, with_weight=with_weight, status=status)
    assert total.shape == () and last.shape == () and total.device == DEV
    (total if scale is None else total * scale).backward()
    return total.detach().cpu(), last.detach().cpu(), [e.grad.cpu() for e in leaves]


def same_with_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ---------------------------------------------------------------------------------------------- 1. the reference's fixture
def test_g15_loss_and_gradients_of_the_reference():
    g = load_golden("g15_losses")
    stages = [(g[k + "_depth"], g[k + "_gt"], g[k + "_w"]) for k in ("stage1", "stage2", "stage3")]
    total, last, grads = device_loss(stages)
    err = abs(float(total) - float(g["loss_mvs"])) / abs(float(g["loss_mvs"]))
    print("G15 loss_mvs: %.9g against %.9g, relative error %.3g" % (float(total), float(g["loss_mvs"]), err))
    assert err <= CC.LOSS_RTOL
    for k, got in enumerate(grads):
        want = g["stage%d_g" % (k + 1)].double() / 0.05
        assert got.shape == want.shape
        ulps = ((got.double() - want).abs() / CC.ulp32(want).clamp_min(1e-300))[want != 0]
        print("G15 stage %d gradient: %d non-zero, worst %.3g ulp" % (k + 1, ulps.numel(), ulps.max().item()))
        assert torch.equal(got[want == 0].double(), want[want == 0]) and ulps.max().item() <= CC.GRAD_ULPS
    CC.assert_close_to_mirror(total, last, grads, stages, what="G15")


# ---------------------------------------------------------------------------------------------- 2. the exact lattice
@pytest.mark.parametrize("sizes", CC.LATTICE_GROUPS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pattern", CC.LATTICE_PATTERNS)
def test_exact_lattice_is_bit_equal_to_the_mirror(pattern, sizes):
    stages = CC.lattice_call(sizes, pattern)
    want_total, want_last, want_grads = CC.mirror(stages)
    total, last, grads = device_loss(stages)
    assert torch.equal(total, want_total) and torch.equal(last, want_last), (float(total), float(want_total))
    for got, want in zip(grads, want_grads):
        assert torch.equal(got, want)
    if len(sizes) == 3:               # the keys pick the stage factors, not the positions: stages 3, 1, 2 in that order
        keys = ["stage3", "stage1", "stage2"]
        want_total, want_last, want_grads = CC.mirror(stages, keys=keys, scale=0.05)
        total, last, grads = device_loss(stages, keys=keys, scale=0.05)
        assert torch.equal(total, want_total) and torch.equal(last, want_last)
        assert all(torch.equal(a, b) for a, b in zip(grads, want_grads))


# ---------------------------------------------------------------------------------------------- 3. rank pairing
def test_weights_are_paired_by_rank_not_by_pixel():
    stages = CC.rank_pairing_stages()
    total, last, grads = device_loss(stages, keys=["stage2", "stage3"])
    CC.assert_close_to_mirror(total, last, grads, stages, keys=["stage2", "stage3"], what="rank pairing")
    assert abs(float(total) - CC.by_rank(stages, keys=["stage2", "stage3"], elementwise=True)) > 1e-2 * float(total)


# ---------------------------------------------------------------------------------------------- 4. float64 differential
@pytest.mark.parametrize("with_weight", (True, False), ids=("weighted", "plain"))
@pytest.mark.parametrize("frac", CC.DIFF_FRACTIONS)
@pytest.mark.parametrize("k,size", list(enumerate(CC.DIFF_SIZES)), ids=lambda v: str(v))
def test_random_stages_against_the_float64_mirror(k, size, frac, with_weight):
    gen = torch.Generator().manual_seed(400 + 10 * k + int(frac * 100))
    stage = CC.random_stage((128, 160) if size == 128 * 160 else size, frac, gen)
    keys = ["stage%d" % (k % 3 + 1)]
    total, last, grads = device_loss([stage], with_weight, keys)
    CC.assert_close_to_mirror(total, last, grads, [stage], with_weight, keys, what="n=%d frac=%g %s" % (size, frac, "weighted" if with_weight else "plain"))


def test_three_random_stages_in_one_call():
    gen = torch.Generator().manual_seed(44)
    stages = [CC.random_stage(s, f, gen) for s, f in (((1, 16, 20), 0.3), ((1, 32, 40), 0.02), ((1, 64, 80), 1.0))]
    total, last, grads = device_loss(stages, scale=0.05)
    CC.assert_close_to_mirror(total, last, grads, stages, scale=0.05, what="three stages")


# ---------------------------------------------------------------------------------------------- 5. edge semantics
def test_a_stage_without_a_valid_element_is_what_the_mirror_gives():
    gen = torch.Generator().manual_seed(5)
    good, empty = CC.random_stage(1025, 0.3, gen), CC.random_stage(48, 0.3, gen)
    empty = (empty[0], torch.zeros(48), torch.zeros(48))
    stages = [good, empty]
    want_total, want_last, want_grads = CC.mirror(stages)
    assert torch.isnan(want_total) and torch.isnan(want_last)             # torch's mean of nothing
    total, last, grads = device_loss(stages)
    assert same_with_nan(total, want_total) and same_with_nan(last, want_last)
    assert torch.equal(grads[1], want_grads[1])                           # whatever the mirror's autograd gives for the empty stage (zeros)
    assert not torch.isnan(grads[0]).any()
    CC.assert_close_to_mirror(*device_loss([good]), [good], what="the good stage alone")
    ulps = ((grads[0].double() - want_grads[0].double()).abs() / CC.ulp32(want_grads[0]).clamp_min(1e-300))[want_grads[0] != 0]
    assert ulps.max().item() <= CC.GRAD_ULPS                              # the stage beside it keeps its gradient, as in the mirror


def test_mismatched_counts_are_nan_and_set_a_sticky_status_bit():
    from uc_nerf_amd import ops
    from uc_nerf_amd.utils import loss as UL
    gen = torch.Generator().manual_seed(6)
    good = CC.random_stage(1025, 0.3, gen)
    est, gt, w = CC.random_stage(4355, 0.3, gen)
    fewer = w.clone()
    fewer[(w > 0).nonzero()[0]] = 0                                       # one positive weight less than valid depths
    one = torch.zeros_like(w)
    one[7] = 1.5                                                          # exactly ONE positive weight: torch would broadcast it; here a mismatch
    with pytest.raises((RuntimeError, IndexError)):
        CC.mirror([(est, gt, fewer)])                                     # (the mirror cannot: torch raises)
    assert not torch.isnan(CC.mirror([(est, gt, one)])[0])                # (torch's broadcast: the documented difference)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    UL.loss_status_clear()
    assert UL.loss_status() == 0
    for bad_w in (fewer, one):
        word.zero_()
        total, last, grads = device_loss([good, (est, gt, bad_w)], status=word)
        assert torch.isnan(total) and torch.isnan(last) and word.item() == 0b10
        assert torch.isnan(grads[1][gt > 0]).all() and (grads[1][~(gt > 0)] == 0).all() and not torch.isnan(grads[0]).any()
        total, _, _ = device_loss([good], status=word)                    # a good call leaves the bit where it is
        assert not torch.isnan(total) and word.item() == 0b10
    assert UL.loss_status() == 0                                          # the device's own word saw none of this ...
    total, _, _ = device_loss([(est, gt, fewer)], keys=["stage3"])
    assert torch.isnan(total) and ops.loss_status() == 0b1 and UL.loss_status(clear=True) == 0b1 and UL.loss_status() == 0
    total, _, _ = device_loss([(est, gt, fewer)], with_weight=False)      # weights off: nothing to mismatch
    assert not torch.isnan(total) and UL.loss_status() == 0


def test_a_nan_ground_truth_is_not_valid():
    gen = torch.Generator().manual_seed(7)
    est, gt, w = CC.random_stage(4355, 0.3, gen)
    holes = (gt == 0).nonzero().view(-1)[::7]
    gt[holes] = float("nan")
    total, last, grads = device_loss([(est, gt, w)])
    assert not torch.isnan(total) and (grads[0][holes] == 0).all()
    CC.assert_close_to_mirror(total, last, grads, [(est, gt, w)], what="NaN ground truth")


# ---------------------------------------------------------------------------------------------- 6. determinism
def test_two_calls_give_the_same_bits():
    gen = torch.Generator().manual_seed(8)
    stages = [CC.random_stage(s, 0.3, gen) for s in (1025, 4355, 128 * 160)]
    a, b = device_loss(stages), device_loss(stages)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


# ---------------------------------------------------------------------------------------------- 7. no host read
def test_the_cascade_term_is_captured_and_replayed_on_new_valid_counts():
    """zero_grad + cas_mvsnet_loss_device * 0.05 + backward + Adam as ONE train_step.GraphedStep; before every replay a ground truth with ANOTHER
    number of valid depths is copied into the static tensors.  Loss and leaves follow an eager float64 run of the CPU mirror on the same data:
    loss within LOSS_RTOL; leaves within LOSS_RTOL too (every step rounds a leaf in [1, 4) once, 1.2e-7, and moves it by lr = 1e-2 times a
    ratio that inherits the gradients' 4-ulp error, 5e-9: five steps stay below 1e-6 of leaves that are at least 1)."""
    from uc_nerf_amd.train_step import GraphedStep
    from uc_nerf_amd.utils import loss as UL
    shapes, keys = ((1, 6, 8), (1, 12, 16), (1, 24, 32)), ("stage1", "stage2", "stage3")
    gen = torch.Generator().manual_seed(9)
    batches = [[CC.random_stage(s, f, gen) for s in shapes] for f in (0.3, 0.5, 0.1, 0.8)]
    counts = [sum(int((s[1] > 0).sum()) for s in b) for b in batches]
    assert len(set(counts)) == len(counts)                                # every batch another valid count
    leaves = [dev(s[0]).requires_grad_(True) for s in batches[0]]
    gt = {k: dev(s[1]) for k, s in zip(keys, batches[0])}
    w = {k: dev(s[2]) for k, s in zip(keys, batches[0])}
    inputs = {k: {"depth": e} for k, e in zip(keys, leaves)}
    opt = torch.optim.Adam(leaves, lr=1e-2, capturable=True)

    def step():
        opt.zero_grad(set_to_none=True)
        total, _ = UL.cas_mvsnet_loss_device(inputs, gt, w)
        (total * 0.05).backward()
        opt.step()
        return total

    ref = [s[0].double().clone().requires_grad_(True) for s in batches[0]]
    ref_opt = torch.optim.Adam(ref, lr=1e-2)

    def ref_step(batch):
        ref_opt.zero_grad(set_to_none=True)
        i, g, ww = CC.dicts([(e, s[1].double(), s[2].double()) for e, s in zip(ref, batch)])
        total, _ = UL.cas_mvsnet_loss(i, g, ww)
        (total * 0.05).backward()
        ref_opt.step()
        return float(total.detach())

    graphed = GraphedStep(step, warmup=2)                                 # (the two warm-up steps have stepped the leaves; the capture executes nothing)
    for _ in range(2):
        ref_step(batches[0])
    for batch in batches[1:]:
        for k, s in zip(keys, batch):
            gt[k].copy_(dev(s[1]))
            w[k].copy_(dev(s[2]))
        got = float(graphed.replay().detach())
        want = ref_step(batch)
        print("replay: loss %.9g against %.9g" % (got, want))
        assert abs(got - want) <= CC.LOSS_RTOL * abs(want)
        for a, b in zip(leaves, ref):
            err = ((a.detach().cpu().double() - b.detach()).abs() / b.detach().abs()).max().item()
            assert err <= CC.LOSS_RTOL, err
    assert UL.loss_status() == 0


# ---------------------------------------------------------------------------------------------- 8. the switch of the loss mix
def test_training_loss_with_the_cascade_term_on_the_device():
    from uc_nerf_amd.utils import loss as UL
    g = load_golden("g15_losses")
    kw = dict(n_rays=int(g["n_rays"]), patch_num=int(g["patch_num"]), patch_size=int(g["patch_size"]))
    names = ("rgb", "depth_pred", "target_s", "target_depths", "target_weights", "patch_dpt")
    keys = ("stage1", "stage2", "stage3")

    def run(device, dtype, **route):
        to = lambda t: t.to(device=device, dtype=dtype)                  # noqa: E731
        leaves = {k: to(g[k + "_depth"]).requires_grad_(True) for k in keys}
        outputs = {k: {"depth": leaves[k]} for k in keys}
        outputs["depth"] = outputs["stage3"]["depth"]
        loss, parts = UL.training_loss(*[to(g[n]) for n in names], outputs, {k: to(g[k + "_gt"]) for k in keys}, {k: to(g[k + "_w"]) for k in keys}, **kw, **route)
        loss.backward()
        return loss.detach().cpu(), {k: v.detach().cpu() for k, v in parts.items()}, [leaves[k].grad.cpu() for k in keys]

    loss_d, parts_d, grads_d = run(DEV, torch.float32, mvs_on_device=True)
    loss_e, parts_e, grads_e = run(DEV, torch.float32)                    # the default route on the same device: the other terms are the same code
    loss_r, parts_r, grads_r = run("cpu", torch.float64)                  # the CPU statement, float64
    for k in parts_d:
        if k != "loss_mvs":
            assert torch.equal(parts_d[k], parts_e[k]), k
        err = abs(float(parts_d[k]) - float(parts_r[k])) / abs(float(parts_r[k]))
        print("%s: %.9g against %.9g (float64, CPU), relative error %.3g" % (k, float(parts_d[k]), float(parts_r[k]), err))
        assert err <= CC.LOSS_RTOL, k
    assert abs(float(loss_d) - float(loss_r)) <= CC.LOSS_RTOL * abs(float(loss_r))
    assert abs(float(parts_d["loss_mvs"]) - float(g["loss_mvs"])) <= CC.LOSS_RTOL * abs(float(g["loss_mvs"]))
    for got, want in zip(grads_d, grads_r):
        ulps = ((got.double() - want).abs() / CC.ulp32(want).clamp_min(1e-300))[want != 0]
        assert torch.equal(got[want == 0].double(), want[want == 0]) and ulps.max().item() <= CC.GRAD_ULPS, ulps.max().item()
