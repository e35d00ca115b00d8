"""Torch-facing wrappers of the HIP entry points: tensors in, tensors out, on the caller's current stream.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); every computation is a kernel of
libucnerf_hip.so.  All functions require float32 tensors on a ROCm device and raise otherwise.

One module per kernel family; this file only re-exports their names.  Module state (the MLP's backward mode, split operand and guard
words in `network`, the loss words in `mvs`, the target words in `data`, build_rays_test's prepared structs in `rays`) is not re-exported: a copy here would go stale.
Read it through its home module or the accessors (`backward_mode()`, `split_operand()`, `split_guard_status()`, `loss_status()`, `step_targets_status()`).
"""
from ._core import (Event, _NO_SWITCH, _NoSwitch, _cur_dev, _dev, _dev_as, _dev_f32, _f32, _launch, _mat, _on, _opt,  # noqa: F401
                    _ptr, _raw_stream, _stream)
from .rays import (RaySampler, build_rays_test, build_rays_train, dir_feature, embed, ndc_project, ndc_rays, ray_gen,  # noqa: F401
                   ray_gen_sample, sample_cascade, sample_stratified)
from .gather import (GATHER_BWD_ROUTES, ChannelLastSources, GatherSources, _FeatGather, _bind_gather_grads, _cl_ok,  # noqa: F401
                     _feat_gather_bwd_into, _gather_scratch, _strides_match, cl_img_feat_view, cl_imgs_view, cl_volume_view,
                     feat_gather, feat_gather_bwd, feat_gather_fwd)
from .network import (BACKWARD_MODES, KEPT_SETS, SPLIT_OPERANDS, PackedWeights, TensorTable, _MLP, _MLPEncoded,  # noqa: F401
                      _encoded_params, _guard_word, _launch_split, backward_mode, decode_p24, mlp, mlp_bwd, mlp_encoded, mlp_fwd,
                      mlp_fwd_encoded, mlp_fwd_train, set_backward_mode, set_split_operand, split_guard_clear,
                      split_guard_status, split_operand, untile_feats)
from .compositing import (_Composite, _CompositeMaps, _CompositeMerged, _CompositeMergedMaps, _maps_fold, _maps_outputs,  # noqa: F401
                          composite, composite_bwd, composite_fold_grads, composite_fwd, composite_maps, composite_merged,
                          composite_merged_bwd, composite_merged_fwd, composite_merged_maps, merge_rows, sample_pdf)
from .mvs import (_CasLoss, _CostVolumeFn, _DepthHypothesesFn, _DepthRegressFn, _cost_volume_fwd, _cost_volume_params,  # noqa: F401
                  _depth_hypotheses_map_params, _depth_regress_bwd_values, _depth_regress_params, _loss_word, cas_loss,
                  cost_volume, depth_hypotheses, depth_hypotheses_bwd, depth_regress, loss_status, loss_status_clear)
from .metrics import (PackedConv, _eval_workspace, _is_cell, colormap_table, conv2d_bias_relu, conv2d_pack,  # noqa: F401
                      depth_colormap, depth_eval, depth_minmax, image_eval, image_group_pixels, image_put, lpips_alex,
                      lpips_layer, lpips_workspace_floats, maxpool2d, minmax_reset, minmax_value)
from .cnn import (BN_MAX_GROUPS, PackedConv3d, PackedDgrad2d, _Conv2dBnTrain, _Conv2dTrain, _Conv3dBnTrain, _Conv3dTrain, batch_norm_train,  # noqa: F401
                  batch_norm_train_bwd, conv2d_bias_grad, conv2d_bn_train, conv2d_dgrad, conv2d_dgrad_pack, conv2d_train, conv2d_wgrad,
                  conv3d, conv3d_bn_train, conv3d_dgrad, conv3d_dgrad_pack, conv3d_pack, conv3d_train, conv3d_wgrad)
from .data import (NOVEL_MAX_CAND, RESIZE_MAX_RATIO, SAMPLE_MAX_ROWS, SAMPLE_MAX_VIEWS, _target_word, novel_assemble,  # noqa: F401
                   resize_bilinear_u8, resize_coeffs, sample_assemble, step_targets, step_targets_status, step_targets_status_clear)
from .fusion import COMPACT_BLOCK_ITEMS, COMPACT_SCAN_CHUNK, FUSION_MAX_SRC, depth_consistency, points_compact      # noqa: F401
from .render import RenderPass      # noqa: F401
