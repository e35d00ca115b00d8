"""Generates tests/golden/g19_cascade.npz: the reference's CascadeMVSNet.forward (network/mvs_models.py:693-762) and its
get_depth_range_samples (:536-573) on seeded inputs, with the CNNs replaced by the stand-ins of tests/cascade_stubs.py.

Run where the reference tree is present:  python tests/golden/make_golden_cascade.py
Data only: inputs (the stand-ins' fixed logits included) and the reference's outputs.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402
import cascade_stubs as S  # noqa: E402

ref = _ref_import.load()
torch.set_num_threads(1)


def main():
    out = {}
    # ---- the stage loop: 32 x 40 image, 3 source views, pad 2
    g = torch.Generator().manual_seed(1919)
    V, H, W, pad = 3, 32, 40, 2
    ndepths = [48, 32, 8]
    imgs = torch.rand(1, V, 3, H, W, generator=g)
    affine, affine_inv = S.cameras(V, H, W, seed=1920)
    near_far = torch.tensor([2.0, 11.0])
    logits = [2.0 * torch.randn(*shp, generator=g) for shp in S.stage_logit_shapes(H, W, ndepths, pad)]
    with contextlib.redirect_stdout(io.StringIO()):                      # (the constructor prints its configuration)
        net = ref.mvs.CascadeMVSNet()
    net.feature, net.cost_regularization = S.make_stubs(V, H, W, logits)
    with torch.no_grad():
        vol, conf, depth, outputs = net(imgs, affine, affine_inv, near_far, pad=pad)
    assert vol is outputs["stage3"]["volume_feature_no_ref"] and conf is outputs["stage3"]["photometric_confidence"] and depth is outputs["stage3"]["depth"]
    out.update(V=V, H=H, W=W, pad=pad, ndepths=np.array(ndepths), imgs=imgs, affine_mat=affine, affine_mat_inv=affine_inv, near_far=near_far,
               feature_seed=1900, outputs_listing=np.array(S.outputs_listing(outputs)))
    for k in (1, 2, 3):
        o = outputs["stage%d" % k]
        out.update({"logits%d" % k: logits[k - 1], "depth_values%d" % k: o["depth_values"][0], "depth%d" % k: o["depth"][0],
                    "confidence%d" % k: o["photometric_confidence"][0]})

    # ---- get_depth_range_samples on its own: a map whose clamps bite on some pixels and not on others, on both sides; and a row
    D, h, w = 8, 12, 14
    near, far, interval = 2.0, 11.0, 0.4
    cur = near + (far - near) * torch.rand(1, h, w, generator=g)
    got = ref.mvs.get_depth_range_samples(cur, D, interval, cur.device, cur.dtype, [1, h, w], max_depth=far, min_depth=near)
    lo_bites, hi_bites = (cur - D / 2 * interval < near), (cur + D / 2 * interval > far)
    assert 0 < lo_bites.sum() < cur.numel() and 0 < hi_bites.sum() < cur.numel()
    row = torch.linspace(near, far, 48).unsqueeze(0)
    got_row = ref.mvs.get_depth_range_samples(row, 48, interval, row.device, row.dtype, [1, 6, 7], max_depth=far, min_depth=near)
    out.update(map_cur_depth=cur, map_ndepth=D, map_interval=interval, map_near=near, map_far=far, map_samples=got, row_in=row, row_ndepth=48,
               row_samples=got_row)

    arrs = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "g19_cascade.npz")
    np.savez_compressed(path, **arrs)
    print("g19_cascade %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(arrs)))


if __name__ == "__main__":
    main()
