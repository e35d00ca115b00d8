"""Case builders and references for the device cascade depth loss (tests/test_cas_loss_host.py, tests/test_hip_cas_loss.py).

The reference of every comparison is `uc_nerf_amd.utils.loss.cas_mvsnet_loss` evaluated on the CPU (`mirror`), in float64 where a tolerance is
involved; `by_rank` restates the same numbers with explicit ranks in numpy, so that the host tests can check the builders against the mirror
without a device.  A stage is a tuple (est, gt, w) of float32 CPU tensors of one shape."""
import numpy as np
import torch

from uc_nerf_amd.utils import loss as L

STAGE_W = (0.5, 1.0, 2.0)
LATTICE_SIZES = (1, 48, 1023, 1025, 65 * 67)          # one element; less than a wave; either side of the 1024 threads; a multiple of nothing
LATTICE_PATTERNS = ("all", "pow2", "last_one", "first_run", "last_run")
LATTICE_GROUPS = ((1,), (48, 1023), (1025, 65 * 67, 1))      # sizes of the stages of one call: one, two and three stages
DIFF_SIZES = (48, 1025, 4355, 128 * 160)
DIFF_FRACTIONS = (0.02, 0.3, 1.0)
LOSS_RTOL = 1e-5          # <= (ceil(N / 1024) + 6 + 4) additions of non-negative terms, each 2^-24 relative: 90 * 2^-24 = 5.4e-6 at 256 x 320, rounded up
GRAD_ULPS = 4             # two multiplications, a clamp and a division, each correctly rounded: <= 4 float32 ulp of the float64 value


def dicts(stages, keys=None):
    """The three dict arguments of cas_mvsnet_loss for a list of stages; keys default to stage1, stage2, ..."""
    keys = keys or ["stage%d" % (k + 1) for k in range(len(stages))]
    inputs = {k: {"depth": s[0]} for k, s in zip(keys, stages)}
    return inputs, {k: s[1] for k, s in zip(keys, stages)}, {k: s[2] for k, s in zip(keys, stages)}


def mirror(stages, with_weight=True, dtype=torch.float32, keys=None, scale=None):
    """cas_mvsnet_loss on the CPU in `dtype`: (total, last stage's loss, [gradient of (total * scale) with respect to each estimate])."""
    leaves = [s[0].to(dtype).clone().requires_grad_(True) for s in stages]
    inputs, gt, w = dicts([(e, s[1].to(dtype), s[2].to(dtype)) for e, s in zip(leaves, stages)], keys)
    total, last = L.cas_mvsnet_loss(inputs, gt, w, with_weight=with_weight)
    (total if scale is None else total * scale).backward()
    return total.detach(), last.detach(), [e.grad if e.grad is not None else torch.zeros_like(e) for e in leaves]


def by_rank(stages, with_weight=True, keys=None, elementwise=False):
    """The same total in numpy float64 with the pairing written out: the k-th valid depth takes the k-th positive weight (row-major).
    elementwise=True pairs every valid depth with the weight at its own pixel instead -- what a `mask * w` rewrite would compute."""
    keys = keys or ["stage%d" % (k + 1) for k in range(len(stages))]
    total = 0.0
    for key, (est, gt, w) in zip(keys, stages):
        est, gt, w = (t.double().numpy().reshape(-1) for t in (est, gt, w))
        valid = gt > 0
        d = np.abs(est[valid] - gt[valid])
        term = np.where(d < 1, 0.5 * d * d, d - 0.5)
        if with_weight:
            term = term * (w[valid] if elementwise else w[w > 0])
        total = total + STAGE_W[int(key.replace("stage", "")) - 1] * term.sum() / valid.sum()
    return total


# ---------------------------------------------------------------------------------------------- random stages, as G15's generator draws them
def random_stage(shape, frac, gen):
    """tests/golden/make_golden.py g15: depths in [1, 4), a fraction `frac` of the pixels valid, weights in [0.1, 2) at the valid pixels."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    est = 1.0 + 3.0 * torch.rand(shape, generator=gen)
    m = torch.rand(shape, generator=gen) < frac
    if not m.any():
        m.view(-1)[m.numel() // 2] = True          # (a stage without a valid pixel is a case of its own)
    gt = torch.where(m, 1.0 + 3.0 * torch.rand(shape, generator=gen), torch.zeros(shape))
    w = torch.where(m, 0.1 + 1.9 * torch.rand(shape, generator=gen), torch.zeros(shape))
    return est, gt, w


# ---------------------------------------------------------------------------------------------- the exact lattice
def lattice_mask(n, pattern):
    run = -(-n // 1024)                            # elements of a thread's share of n over 1024 threads
    m = torch.zeros(n, dtype=torch.bool)
    pow2 = lambda k: 1 << (k.bit_length() - 1)     # noqa: E731  the largest power of two <= k
    if pattern == "all":
        m[:] = True
    elif pattern == "pow2":                        # scattered over the whole stage
        m[torch.randperm(n, generator=torch.Generator().manual_seed(n))[:pow2(n)]] = True
    elif pattern == "last_one":
        m[n - 1] = True
    elif pattern == "first_run":
        m[:pow2(run)] = True
    elif pattern == "last_run":
        m[n - pow2(run):] = True
    else:
        raise ValueError(pattern)
    return m


def lattice_stage(n, pattern, gen):
    """est, gt multiples of 1/8 in [1, 5), weights in {0.5, 1, 2}: every term is a multiple of 1/256 below 8 and a sum of 4355 of them stays below
    2^15 -- exact in float32 in any order; the valid count is a power of two except under "all" (count = n), where the one division of the exact
    sum is a single correctly rounded operation on either side."""
    m = lattice_mask(n, pattern)
    est = torch.randint(8, 40, (n,), generator=gen).float() / 8
    gt = torch.randint(8, 40, (n,), generator=gen).float() / 8
    idx = m.nonzero().view(-1)
    for j, delta in enumerate((1.0, -1.0, 0.875, -0.875, 1.125, -1.125, 0.0)[:idx.numel()]):      # |d| exactly at 1 and on either side of it
        gt[idx[j]] = 3.0
        est[idx[j]] = 3.0 + delta
    w = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=gen)]
    zero = torch.zeros(n)
    return est, torch.where(m, gt, zero), torch.where(m, w, zero)


def lattice_call(sizes, pattern, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    return [lattice_stage(n, pattern, gen) for n in sizes]


# ---------------------------------------------------------------------------------------------- rank pairing
def rank_pairing_stages():
    """Positive weights at OTHER pixels than the valid depths, equal counts, all weights distinct: (shifted by three pixels; reversed)."""
    gen = torch.Generator().manual_seed(77)
    out = []
    for n, kind in ((1025, "shift"), (65 * 67, "reverse")):
        est, gt, _ = random_stage(n, 0.3, gen)
        m = gt > 0
        mw = torch.roll(m, 3) if kind == "shift" else torch.flip(m, (0,))
        w = torch.zeros(n)
        w[mw] = 0.25 + torch.arange(int(mw.sum()), dtype=torch.float32) / 64          # distinct, in row-major order
        out.append((est, gt, w))
    return out


def ulp32(x):
    """Spacing of float32 at the magnitude of the float64 values x (normal range)."""
    x = x.double().abs()
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp_min(1e-300))) - 23), torch.zeros_like(x))


def assert_close_to_mirror(got_total, got_last, got_grads, stages, with_weight=True, keys=None, scale=None, what=""):
    """The bars of the float64 differential: loss relative error <= LOSS_RTOL, every gradient element within GRAD_ULPS float32 ulp."""
    total, last, grads = mirror(stages, with_weight, torch.float64, keys, scale)
    for name, g, r in (("total", got_total, total), ("last stage", got_last, last)):
        err = abs(float(g) - float(r)) / abs(float(r))
        print("%s %s: %.9g against %.9g, relative error %.3g (bar %.1g)" % (what, name, float(g), float(r), err, LOSS_RTOL))
        assert err <= LOSS_RTOL, (what, name, float(g), float(r))
    for s, (g, r) in enumerate(zip(got_grads, grads)):
        g = g.detach().cpu().double().reshape(r.shape)
        ulps = ((g - r).abs() / ulp32(r).clamp_min(1e-300))[r != 0]
        print("%s stage %d gradient: %d non-zero, worst %.3g ulp (bar %d)" % (what, s, ulps.numel(), ulps.max().item() if ulps.numel() else 0.0, GRAD_ULPS))
        assert torch.equal(g[r == 0], r[r == 0]), (what, s, "a gradient where the mirror has none")
        assert ulps.numel() == 0 or ulps.max().item() <= GRAD_ULPS, (what, s, ulps.max().item())
