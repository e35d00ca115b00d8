"""Shared by tests/golden/make_golden_cascade.py (which captures fixture G19 from the reference) and the cascade tests:

  * small deterministic stand-ins for the CNNs a CascadeMVSNet is built around -- the feature pyramid returns fixed random maps, the
    regulariser returns the first 8 channels of the variance volume and FIXED logits (+ 0.0 * v, as the DepthNet test of
    tests/test_hip_parity.py does): the regressed depth then does not depend on nearest-neighbour ties in the cost volume, so every stage's
    depth hypotheses are determined up to rounding;
  * a torch restatement of the op chain between two cascade stages (network/mvs_models.py:536-573, 720-746 and the replicate pad of :598),
    the reference the kernel is compared with at shapes the fixture does not hold.  tests/test_cascade_host.py pins it to G19.

Our own code; nothing here is needed by the package.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

SCALES = (4, 2, 1)                 # stage k works at 1 / SCALES[k] of the image (mvs_models.py:667-677)
CHANNELS = 8


def bar(far):
    """|got - want| <= 16 * 2^-23 * far: two convex 4-tap combinations, one clamp pair, one division and one multiply-add, each a few ulp
    of a value bounded by far."""
    return 16.0 * 2.0 ** -23 * float(far)


# ------------------------------------------------------------------------------------------------ stand-ins for the CNNs
def feature_maps(n_views, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n_views, CHANNELS, H // s, W // s, generator=g) for s in SCALES]


class FeatureStub(nn.Module):
    """Stands where FeatureNet goes: call number i (mod the number of views) returns view i's fixed maps, whatever the image."""

    def __init__(self, maps):
        super().__init__()
        for k, m in enumerate(maps):
            self.register_buffer("maps%d" % (k + 1), m.clone())
        self.calls = 0

    def forward(self, img):
        v = self.calls % self.maps1.shape[0]
        self.calls += 1
        return {"stage%d" % k: getattr(self, "maps%d" % k)[v:v + 1] for k in (1, 2, 3)}


class RegStub(nn.Module):
    """Stands where a CostRegNet goes: (volume feature, logits) = (v[:, :8], fixed logits + 0.0 * v[:, :1])."""

    def __init__(self, logits):
        super().__init__()
        self.register_buffer("logits", logits.clone())               # [1,1,D,hp,wp]

    def forward(self, v):
        return v[:, :8], self.logits + 0.0 * v[:, :1]


def stage_logit_shapes(H, W, ndepths, pad):
    return [(1, 1, D, H // s + (2 * pad if k == 2 else 0), W // s + (2 * pad if k == 2 else 0)) for k, (D, s) in enumerate(zip(ndepths, SCALES))]


def make_stubs(n_views, H, W, logits, seed=1900):
    return FeatureStub(feature_maps(n_views, H, W, seed)), nn.ModuleList([RegStub(x) for x in logits])


def cameras(n_views, H, W, seed):
    """affine_mat [n_views + 1, 3, 4, 4] = K_stage @ w2c per view (entry 0: the target view) and its inverse."""
    g = torch.Generator().manual_seed(seed)
    w2c = torch.eye(4).repeat(n_views + 1, 1, 1)
    w2c[1:, 0, 3] = 0.05 * torch.arange(1, n_views + 1) + 0.01 * torch.rand(n_views, generator=g)
    w2c[1:, 1, 3] = 0.02 * torch.rand(n_views, generator=g)
    mats = []
    for s in SCALES:
        K4 = torch.eye(4)
        K4[0, 0] = K4[1, 1] = 0.9 * W / s
        K4[0, 2], K4[1, 2] = 0.5 * W / s, 0.5 * H / s
        mats.append(K4 @ w2c)
    affine = torch.stack(mats, 1).contiguous()
    return affine, torch.inverse(affine)


# ------------------------------------------------------------------------------------------------ the op chain, restated
def hypotheses_chain(cur_depth, near, far, interval_pixel, ndepth, full_hw, out_hw, pad=0):
    """cur_depth [h0,w0] -> depth_values [ndepth, h + 2 pad, w + 2 pad] the way the reference gets there: bilinear up-sampling to full_hw,
    the clamped band, ndepth samples per full-resolution pixel, trilinear interpolation down to out_hw, replicate padding."""
    c = F.interpolate(cur_depth[None, None], [int(full_hw[0]), int(full_hw[1])], mode="bilinear", align_corners=False).squeeze(1)
    lo = (c - ndepth / 2 * interval_pixel).clamp(min=near)
    hi = (c + ndepth / 2 * interval_pixel).clamp(max=far)
    step = (hi - lo) / (ndepth - 1)
    samples = lo.unsqueeze(1) + torch.arange(0, ndepth, dtype=c.dtype, device=c.device).reshape(1, -1, 1, 1) * step.unsqueeze(1)
    out = F.interpolate(samples.unsqueeze(1), [ndepth, int(out_hw[0]), int(out_hw[1])], mode="trilinear", align_corners=False).squeeze(1)
    if pad > 0:
        out = F.pad(out, (pad, pad, pad, pad), "replicate")
    return out[0], (lo[0], hi[0], c[0])


def row_chain(row, ndepth, out_hw, pad=0):
    """row [D_in] -> [ndepth, h + 2 pad, w + 2 pad]: the band row[0] .. row[-1] in ndepth samples, the same for every pixel."""
    step = (row[-1] - row[0]) / (ndepth - 1)
    samples = row[0] + torch.arange(0, ndepth, dtype=row.dtype, device=row.device) * step
    return samples.reshape(-1, 1, 1).repeat(1, int(out_hw[0]) + 2 * pad, int(out_hw[1]) + 2 * pad)


def outputs_listing(outputs):
    """["stage1/depth:1,8,10", ..., "depth:1,32,40", ...]: every tensor of a CascadeMVSNet `outputs` dict with its shape, sorted."""
    rows = []
    for k, v in outputs.items():
        if isinstance(v, dict):
            rows += ["%s/%s:%s" % (k, kk, ",".join(map(str, vv.shape))) for kk, vv in v.items()]
        else:
            rows.append("%s:%s" % (k, ",".join(map(str, v.shape))))
    return sorted(rows)
