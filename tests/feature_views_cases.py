"""Shared cases of the FeatureNet-over-all-views tests (the group dimension of csrc/bn.hip, ops.batch_norm_train(groups=), FeatureNet.forward_views,
CascadeMVSNet(feature_views="batched")) and the float64 restatement the batched pass is measured against.

The restatement of the module is feature_train_cases.feature_net applied VIEW BY VIEW, as the reference runs its feature net: every view is a
batch of one image with its own batch statistics, the parameter gradients are the sums over the views, and the batch-norm buffers are threaded
through the views in ascending order (bn_cases.feature_net returns the state dict a forward leaves behind).  It shares no code with the package
and does not import it."""
import torch

import bn_cases as BC
import feature_train_cases as FC

STAGES = ("stage1", "stage2", "stage3")
MAX_GROUPS = 64                                                     # the documented limit on G (include/ucnerf_hip.h)

# the grouped op's shapes (G, n, C, spatial): N = 4 per group; S % 4 != 0 with n > 1 (unaligned group bases, a walk across the image boundary);
# N = 4352 > 4096, so two partial slots per channel and group; "ragged": three slots with a shorter last slice (S from ragged_s); and G = 1, which
# is compared against the ungrouped entry points themselves
OP_SHAPES = ((3, 1, 5, (2, 2)), (2, 2, 16, (3, 5, 7)), (3, 1, 4, (64, 68)), (2, 1, 2, "ragged"), (1, 2, 16, (3, 5, 7)), (1, 1, 4, (64, 68)))


def ragged_s(partials):
    """S of the ragged case: bn_cases.ragged_shape's search (the smallest S = 4 k + 1 with three partial slots and a shorter last slice) asked
    for ONE image per group, with the library's own size query `partials(n, S)`."""
    return BC.ragged_shape(lambda n, S: partials(1, S))[2]


def op_shape(shape, partials):
    G, n, C, spatial = shape
    return (G, n, C, (ragged_s(partials),)) if spatial == "ragged" else shape


def op_inputs(shape, seed, skip):
    """-> (y [G n,C,*spatial], skip or None, grad_out, gamma, beta) of one op case: channel means well away from zero, so that a float32 mean
    would show, and an output gradient with a non-zero mean."""
    G, n, C, spatial = shape
    g = torch.Generator().manual_seed(seed)
    full = (G * n, C) + tuple(spatial)
    y = torch.randn(full, generator=g) * (0.5 + torch.rand((G * n, C) + (1,) * len(spatial), generator=g)) + 3.0 * torch.randn((1, C) + (1,) * len(spatial), generator=g)
    sk = torch.randn(full, generator=g) if skip else None
    return y, sk, torch.randn(full, generator=g) + 0.25, 0.6 + 0.8 * torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)


def buffers(C, seed):
    """Running statistics away from 0 / 1 and a counter away from 0."""
    g = torch.Generator().manual_seed(seed)
    return 0.3 * torch.randn(C, generator=g), 0.5 + 1.5 * torch.rand(C, generator=g), torch.tensor(7, dtype=torch.int64)


def exact_backward_case(G, n, C, spatial, seed):
    """Inputs on which every A_q = sum g and every B_q r_q = sum g (y - mu) r_q is an integer below 2^24, so that the grouped parameter gradients
    -- float64 sums rounded once -- must EQUAL the float32 sums of the per-slab results: gamma = 1, beta = 0, no ReLU, mu an integer per group
    and channel, sigma^2 + eps a power of four per group (so r is a power of two: sigma^2 = 4^k - eps rounds to a float32 whose sum with eps
    is 4^k again in float32 and in float64 up to 2^-24 relative -- the test asserts r itself), g and y - mu small integers.
    -> (y, grad_out, saved_mean [G,C], saved_var [G,C], eps)."""
    g = torch.Generator().manual_seed(seed)
    full = (G * n, C) + tuple(spatial)
    eps = 2.0 ** -10
    mu = torch.randint(-3, 4, (G, C), generator=g).float()
    var = (4.0 ** torch.randint(-1, 2, (G, 1), generator=g).float()).expand(G, C).contiguous() - eps
    d = torch.randint(-4, 5, full, generator=g).float()
    y = d + mu.repeat_interleave(n, 0).view((G * n, C) + (1,) * len(spatial))
    go = torch.randint(-4, 5, full, generator=g).float()
    return y, go, mu, var.float(), eps


# ---- the module: (imgs shape [1,V,3,H,W], seed of the weights, seed of the images and the projections).  The seeds are ones at which, in EVERY
# view, no ReLU's pre-activation lies within the forward chain bar of zero and the float32 restatement takes no other side
# (test_feature_views_host.py asserts it), so that a ReLU cannot take another side on the device than in float64.
MODULE_CASES = (((1, 3, 3, 8, 12), 3101, 3102), ((1, 2, 3, 16, 24), 3201, 3202))


# the cascade step: (V, H, W) = the smallest size tests/test_hip_feature_train.py's cascade step runs, the seed of the FeatureNet's weights, the seed
# of the images; the same ReLU-side condition holds in every view (asserted on the host)
CASCADE_CASE = ((1, 3, 3, 32, 32), 3301, 3302)


def module_inputs(case, c=8):
    """-> (imgs [1,V,3,H,W] in [0, 1), R = {stage: [V,C,h,w]}): the fixed random projections of the loss, sum over the stages of sum out R."""
    shape, _, seed = case
    g = torch.Generator().manual_seed(seed)
    _, V, _, H, W = shape
    imgs = torch.rand(shape, generator=g)
    R = {"stage1": torch.randn((V, 4 * c, H // 4, W // 4), generator=g), "stage2": torch.randn((V, 2 * c, H // 2, W // 2), generator=g),
         "stage3": torch.randn((V, c, H, W), generator=g)}
    return imgs, R


def feature_views(imgs, sd, dtype, R=None):
    """FeatureNet in TRAIN mode over the views of imgs [1,V,3,H,W], one view at a time in ascending order -> dict(out = {stage: [V,C,h,w]},
    views = [feature_train_cases.feature_net's result per view], sd = the state dict after the V forwards (the buffers moved V times), and with
    R: grad_x [1,V,3,H,W] and grads = {parameter key: the sum over the views})."""
    V = imgs.shape[1]
    views, state = [], {k: v.detach().cpu() for k, v in sd.items()}
    for i in range(V):
        Ri = None if R is None else {k: R[k][i:i + 1] for k in STAGES}
        views.append(FC.feature_net(imgs[:, i], sd, dtype, Ri))
        state = BC.feature_net(imgs[:, i], state, dtype)[1]
    res = dict(out={k: torch.cat([v["out"][k] for v in views]) for k in STAGES}, views=views, sd=state)
    if R is not None:
        res["grad_x"] = torch.stack([v["grad_x"][0] for v in views]).unsqueeze(0)
        res["grads"] = {k: sum(v["grads"][k] for v in views) for k in views[0]["grads"]}
    return res


def relu_offenders(r64, r32):
    """feature_train_cases.relu_offenders over every view."""
    return [(i,) + bad for i, (a, b) in enumerate(zip(r64["views"], r32["views"])) for bad in FC.relu_offenders(a, b)]
