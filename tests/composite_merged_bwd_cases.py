"""Cases and CPU restatement of the merged compositing backward (ucnerf_composite_merged_bwd) for tests/test_composite_merged_bwd_host.py and
tests/test_hip_composite_merged_bwd.py.

The entry point's contract is an identity: its g_raw_a / g_raw_b are what three steps in sequence give --
    merged[r, rank[r, j]] = cat(raw_a[r], raw_b[r])[j]                  (ucnerf_merge_rows)
    g_merged = backward of compositing on (merged, z)                   (ucnerf_composite_bwd; here composite_cases.backward, the oracle's autograd)
    cat(g_raw_a[r], g_raw_b[r])[j] = g_merged[r, rank[r, j]]            (un-merge)
restated() chains exactly these on the CPU in float32 or float64; autograd_through_the_merge() differentiates the merged forward with raw_a and
raw_b as the leaves (torch's scatter carries the gradient back), which is what a user of ops.composite_merged gets.  The two must agree: the
host test holds them together in float64.

Cases: a split of a composite_cases case (its rows handed out to raw_a / raw_b by a rank of one of RANK_KINDS, any na), so the expected values
and the bars are composite_cases' own."""
import functools

import torch

import composite_cases as CC

F32, F64 = torch.float32, torch.float64
EXTRA_S = (193, 513)                                  # on top of composite_cases.MERGED_S: E = 4 (193 = 3 * 64 + 1) and E = 16 right behind 8 * 64
IDENTITY_S = CC.MERGED_S + EXTRA_S
CONT_SPLITS = (("cont_S2", 1, "reversed"), ("cont_S65", 21, "random"), ("cont_S193", 128, "interleaved"), ("cont_S257", 0, "random"),
               ("cont_S513", 171, "random"), ("cont_S1024", 1024, "reversed"), ("cont_S1024", 341, "interleaved"))


def na_values(S):
    return sorted({0, 1, S // 3, S - 1, S})


def make_rank(n, S, na, kind, seed=0):
    """rank [n,S] int64: merged position of row j of cat(a, b) (a = the first na rows).  identity / reversed: as composite_cases.merged_case;
    interleaved: a and b take merged positions in turn while both last, the longer one the rest; random: a permutation per ray."""
    if kind == "identity":
        rank = torch.arange(S).expand(n, S)
    elif kind == "reversed":
        rank = torch.arange(S - 1, -1, -1).expand(n, S)
    elif kind == "interleaved":
        nb, both = S - na, min(na, S - na)
        pa = torch.cat([2 * torch.arange(both), 2 * both + torch.arange(na - both)])
        pb = torch.cat([2 * torch.arange(both) + 1, 2 * both + torch.arange(nb - both)])
        rank = torch.cat([pa, pb]).expand(n, S)
    elif kind == "random":
        gen = torch.Generator().manual_seed(100000 * seed + 1000 * S + na)
        rank = torch.stack([torch.randperm(S, generator=gen) for _ in range(n)])
    else:
        raise ValueError(kind)
    rank = rank.contiguous()
    assert bool((rank.sort(-1)[0] == torch.arange(S)).all())
    return rank


def merge(raw_a, raw_b, rank):
    """[n,na+nb,4]: merged[r, rank[r, j]] = cat(raw_a[r], raw_b[r])[j] (differentiable w.r.t. raw_a and raw_b)."""
    cat = torch.cat([raw_a, raw_b], 1)
    idx = rank.long()[..., None].expand(cat.shape)
    return torch.zeros_like(cat).scatter(1, idx, cat)


def unmerge(g_merged, rank, na):
    """(g_a [n,na,4], g_b [n,nb,4]): row j of their concatenation is merged row rank[j]."""
    g_cat = torch.gather(g_merged, 1, rank.long()[..., None].expand(g_merged.shape))
    return g_cat[:, :na].contiguous(), g_cat[:, na:].contiguous()


def split(case, na, kind, rays=None):
    """The live-variant `case` of composite_cases with its rows handed out to raw_a [n,na,4] / raw_b [n,S-na,4] by a rank of `kind`; z and the
    upstream gradients stay in merged order.  rays: keep these rays only."""
    sel = (lambda t: t) if rays is None else (lambda t: t[rays].contiguous())      # noqa: E731
    raw, S = sel(case["raw"]), case["S"]
    n = raw.shape[0]
    rank = make_rank(n, S, na, kind)
    cat = torch.gather(raw, 1, rank[..., None].expand(n, S, 4))                    # cat[j] = merged[rank[j]]
    m = dict(name="%s_na%d_%s" % (case["name"], na, kind), n=n, S=S, na=na, nb=S - na, rank=rank.int(), raw_a=cat[:, :na].contiguous(),
             raw_b=cat[:, na:].contiguous(), z=sel(case["z"]), merged=raw)
    m.update({t: sel(case[t]) for t in CC.TARGETS})
    assert torch.equal(merge(m["raw_a"], m["raw_b"], rank), raw)
    return m


def restated(m, dtype, white, combo):
    """(g_raw_a, g_raw_b) by the three steps of the contract, compositing's backward being composite_cases.backward in `dtype`."""
    merged = merge(m["raw_a"], m["raw_b"], m["rank"])
    g = CC.backward(dict(m, raw=merged), dtype, white, combo)
    return unmerge(g, m["rank"], m["na"])


def autograd_through_the_merge(m, white, combo, dtype=F64):
    """(g_raw_a, g_raw_b) by torch autograd through merge + the oracle's compositing, raw_a and raw_b the leaves."""
    a = m["raw_a"].to(dtype).clone().requires_grad_(True)
    b = m["raw_b"].to(dtype).clone().requires_grad_(True)
    rgb, _, acc, w, depth, _, _ = CC.O.raw2outputs_live(merge(a, b, m["rank"]), m["z"].to(dtype), white)
    outs = dict(g_rgb=rgb, g_depth=depth, g_acc=acc, g_weights=w)
    sum((outs[t] * m[t].to(dtype)).sum() for t in combo).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731 (a side without rows)
    return zero(a).detach(), zero(b).detach()


@functools.lru_cache(maxsize=None)
def continuous_split(name, na, kind):
    """(m, {(white, combo): float64 (g_raw_a, g_raw_b)}) of a continuous case of composite_cases, built once per process: the float64 targets are
    composite_cases' own (continuous(name)[3]), un-merged."""
    case, _, _, gref, _ = CC.continuous(name)
    m = split(case, na, kind)
    return m, {k: unmerge(g, m["rank"], na) for k, g in gref.items()}


def distances(g_a, g_b, ref_a, ref_b):
    """composite_cases.bwd_distances over both sides."""
    d = dict(g_colour=0.0, g_density=0.0)
    for g, r in ((g_a, ref_a), (g_b, ref_b)):
        if r.numel():
            for k, v in CC.bwd_distances(g, r).items():
                d[k] = max(d[k], v)
    return d
