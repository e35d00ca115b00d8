"""Drop-in for the part of the reference's `network/mvs_models.py` that sits directly in front of the ray-marching
path: `DepthNet` (mvs_models.py:585-646), the depth-hypothesis helpers `get_depth_range_samples` /
`get_cur_depth_range_samples` (:536-573) and the three-stage loop `CascadeMVSNet` (:648-762).  Same call signatures and
result keys; the cost-volume assembly (`homo_warp` + mask count + variance), the depth regression and the link between
two stages (previous depth -> next stage's hypothesis volume) run as the HIP kernels `ucnerf_cost_volume` /
`ucnerf_depth_regress` / `ucnerf_depth_hypotheses`.  The CNNs -- the feature pyramid `FeatureNet` (:309-410) and the 3-D
regularisation network `CostRegNet` (:412-443) -- are mirrored here with the reference's parameter names: they train through torch's
layers (or, with training="device", through the HIP forward and backward kernels of csrc/conv2d_bwd.hip, csrc/conv3d_bwd.hip and csrc/bn.hip) and, under eval() + no_grad, run on `ucnerf_conv2d_bias_relu` / `ucnerf_conv3d` with the batch-norms folded into the weights.  Under
train() + no_grad -- how the reference's validation_step runs them (train.py:226-243) -- batch_stats="device" keeps the convolutions on those
kernels and normalises with the statistics of the batch itself on `ucnerf_bn_stats` / `ucnerf_bn_apply`, moving the running statistics as torch does.
`CascadeMVSNet(...)` still takes the caller's modules; `CascadeMVSNet.with_cnns(...)` builds its own.

The cost volume and the regression have backward kernels behind `torch.autograd.Function`s, so the feature network
trains through the variance volume and the regularisation network through depth and photometric confidence, as in the
reference.  The chain depth regression -> depth_values -> depth hypotheses -> previous depth has backward kernels too
(`ucnerf_depth_regress_bwd_values`, `ucnerf_depth_hypotheses_bwd`): with `grad_method="detach"` (the reference's
default) the depth is detached between stages and the hypothesis volume carries no gradient; with `"undetach"` it
stays in the graph, as the reference's other branch keeps it, and a loss on a later stage's depth reaches the earlier
stages' regularisers.
`features` may be a list of [1,C,H,W] maps (as the reference passes) or a stacked tensor.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


INFERENCE_ROUTES = ("device", "torch")
BATCH_STATS_ROUTES = ("torch", "device")
TRAINING_ROUTES = ("torch", "device")


class Conv2d(nn.Module):
    """mvs_models.py:21-61: conv (bias only without bn) -> BatchNorm2d -> ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, relu=True, bn=True, bn_momentum=0.1, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, bias=(not bn), **kwargs)
        self.kernel_size, self.stride = kernel_size, stride
        self.bn = nn.BatchNorm2d(out_channels, momentum=bn_momentum) if bn else None
        self.relu = relu

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        return F.relu(x) if self.relu else x


class Conv3d(nn.Module):
    """mvs_models.py:110-152: conv (bias only without bn) -> BatchNorm3d -> ReLU."""
    transposed = False

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, relu=True, bn=True, bn_momentum=0.1, **kwargs):
        super().__init__()
        if stride not in (1, 2):
            raise AssertionError("stride 1 or 2")
        self.out_channels, self.kernel_size, self.stride = out_channels, kernel_size, stride
        self.conv = (nn.ConvTranspose3d if self.transposed else nn.Conv3d)(in_channels, out_channels, kernel_size, stride=stride, bias=(not bn), **kwargs)
        self.bn = nn.BatchNorm3d(out_channels, momentum=bn_momentum) if bn else None
        self.relu = relu

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        return F.relu(x) if self.relu else x


class Deconv3d(Conv3d):
    """mvs_models.py:154-195: transposed conv (bias only without bn) -> BatchNorm3d -> ReLU: Conv3d's body around an nn.ConvTranspose3d."""
    transposed = True


def fold_conv_bn(layer, dtype=torch.float64):
    """(w', b') of one layer with its eval-mode batch-norm folded in, computed in `dtype`: per output channel s = gamma / sqrt(running_var + eps),
    w' = w s, b' = beta - running_mean s (+ the convolution's own bias times s, where it has one).  `layer` is a Conv2d / Conv3d / Deconv3d above
    or a bare nn.Conv*: then w' = w and b' = its bias or zeros.  The output channel is dimension 1 of a transposed convolution's weight."""
    conv, bn = (layer.conv, layer.bn) if hasattr(layer, "conv") else (layer, None)
    w = conv.weight.detach().to(dtype)
    cout_dim = 1 if isinstance(conv, nn.ConvTranspose3d) else 0
    cout = w.shape[cout_dim]
    b = conv.bias.detach().to(dtype) if conv.bias is not None else torch.zeros(cout, dtype=dtype, device=w.device)
    if bn is None:
        return w, b
    s = bn.weight.detach().to(dtype) / torch.sqrt(bn.running_var.detach().to(dtype) + bn.eps)
    shape = [1] * w.dim()
    shape[cout_dim] = cout
    return w * s.view(shape), bn.bias.detach().to(dtype) + (b - bn.running_mean.detach().to(dtype)) * s


class _InferenceCache:
    """What the device route made of a module's parameters and buffers (folded, packed weights), valid while every one of them is the tensor
    it was made from, at the version and on the device it had then.  The cache keeps the tensors themselves: an object it holds cannot be
    freed and its address reused by another, so identity is a sound test (an address is not: README, round 5)."""

    def __init__(self, watch=None):
        """`watch`: module -> the tensors the cached value was made from; every parameter and buffer without it."""
        self.sources, self.stamps, self.value = None, None, None
        self.watch = watch if watch is not None else (lambda module: list(module.parameters()) + list(module.buffers()))

    @staticmethod
    def _stamp(t):
        return (t._version, t.device, t.dtype)

    def get(self, module, build):
        now = self.watch(module)
        if (self.sources is None or len(now) != len(self.sources)
                or any(a is not b or self._stamp(a) != s for a, b, s in zip(now, self.sources, self.stamps))):
            self.value = build()
            self.sources, self.stamps = now, [self._stamp(t) for t in now]
        return self.value


def _check_route(inference):
    if inference not in INFERENCE_ROUTES:
        raise ValueError("uc_nerf_amd: inference=%r -- \"device\" (the HIP kernels under eval() + no_grad) or \"torch\"" % (inference,))
    return inference


def _check_batch_stats(batch_stats):
    if batch_stats not in BATCH_STATS_ROUTES:
        raise ValueError("uc_nerf_amd: batch_stats=%r -- \"torch\" (torch's layers in training mode) or \"device\" (the HIP kernels under "
                         "train() + no_grad, with inference=\"device\")" % (batch_stats,))
    return batch_stats


def _check_training(training):
    if training not in TRAINING_ROUTES:
        raise ValueError("uc_nerf_amd: training=%r -- \"torch\" (torch's layers whenever grad is enabled) or \"device\" (the HIP forward and backward "
                         "kernels under train() + grad, with inference=\"device\")" % (training,))
    return training


def _device_route(module, x):
    return module.inference == "device" and not module.training and not torch.is_grad_enabled() and x.is_cuda


def _batch_norms_on_device(module):
    """Every batch-norm keeps running statistics with a float momentum: what the batch-norm kernels update."""
    return all(bn.track_running_stats and bn.running_mean is not None and isinstance(bn.momentum, float)
               for bn in module.modules() if isinstance(bn, nn.modules.batchnorm._BatchNorm))


def _batch_stats_route(module, x):
    """train() + no_grad on the device with batch_stats="device", every batch-norm one the kernels update."""
    return (module.inference == "device" and module.batch_stats == "device" and module.training and not torch.is_grad_enabled() and x.is_cuda
            and _batch_norms_on_device(module))


def _training_route(module, x):
    """train() + grad enabled on the device with training="device", every batch-norm one the kernels update."""
    return (getattr(module, "training_route", "torch") == "device" and module.inference == "device" and module.training and torch.is_grad_enabled()
            and x.is_cuda and _batch_norms_on_device(module))


def _conv_weights(module):
    """What the raw packed weights of the batch-statistic route were made from: the convolutions' weights, not the buffers every call moves."""
    return [m.weight for m in module.modules() if isinstance(m, (nn.Conv2d, nn.Conv3d, nn.ConvTranspose3d))]


def _bn_train(layer, y, skip=None, groups=1):
    """The layer's batch-norm, ReLU and skip addition in place on its convolution's output, with the batch's own statistics (`groups` > 1: those
    of each group of images)."""
    bn = layer.bn
    return ops.batch_norm_train(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, momentum=bn.momentum, eps=bn.eps,
                                relu=layer.relu, skip=skip, out=y, groups=groups)


class FeatureNet(nn.Module):
    """mvs_models.py:309-410, the "fpn" pyramid with three stages: image [n,3,H,W] -> {"stage1": [n,4c,H/4,W/4], "stage2": [n,2c,H/2,W/2],
    "stage3": [n,c,H,W]}.  Parameter and buffer names are the reference's, so a checkpoint's `feature.*` keys load strictly.
    Two routes: torch's layers whenever grad is enabled, the module is in training mode or the input is not on a ROCm device; with
    inference="device", under eval() + no_grad, `ops.conv2d_bias_relu` with the batch-norms folded into weights and biases (packed once, cached).
    batch_stats="device" adds a third, under train() + no_grad: the same convolution launches with the raw weights, each batch-normed layer
    followed by `ops.batch_norm_train` in place (batch statistics, the running statistics moved as torch moves them).  training="device" adds a
    fourth, under train() + grad enabled: the eight batch-normed layers are `ops.conv2d_bn_train`, the five bare ones `ops.conv2d_train`, forward
    and backward on the HIP kernels (csrc/conv2d_bwd.hip), the running statistics moved as torch moves them; the two nearest-neighbour
    upsamplings and additions stay torch operations.  The default "torch" keeps torch's layers there.  The attribute `training_route` exists only
    on a module built with training="device": one without it trains through torch, as every FeatureNet did before the keyword.
    `forward_views` runs the pyramid ONCE over all the views of a sample and gives what the per-view calls give (see there)."""

    def __init__(self, base_channels=8, num_stage=3, stride=4, arch_mode="fpn", inference="device", batch_stats="torch", training="torch"):
        super().__init__()
        if arch_mode != "fpn" or num_stage != 3:
            raise NotImplementedError("uc_nerf_amd FeatureNet: arch_mode=%r num_stage=%r -- only arch_mode=\"fpn\" with num_stage=3 is built"
                                      % (arch_mode, num_stage))
        self.arch_mode, self.stride, self.base_channels, self.num_stage = arch_mode, stride, base_channels, num_stage
        self.inference = _check_route(inference)
        self.batch_stats = _check_batch_stats(batch_stats)
        if _check_training(training) == "device":
            self.training_route = "device"                   # (nn.Module owns the attribute `training`)
        c = base_channels
        self.conv0 = nn.Sequential(Conv2d(3, c, 3, 1, padding=1), Conv2d(c, c, 3, 1, padding=1))
        self.conv1 = nn.Sequential(Conv2d(c, 2 * c, 5, stride=2, padding=2), Conv2d(2 * c, 2 * c, 3, 1, padding=1), Conv2d(2 * c, 2 * c, 3, 1, padding=1))
        self.conv2 = nn.Sequential(Conv2d(2 * c, 4 * c, 5, stride=2, padding=2), Conv2d(4 * c, 4 * c, 3, 1, padding=1), Conv2d(4 * c, 4 * c, 3, 1, padding=1))
        self.out1 = nn.Conv2d(4 * c, 4 * c, 1, bias=False)
        self.inner1 = nn.Conv2d(2 * c, 4 * c, 1, bias=True)
        self.inner2 = nn.Conv2d(c, 4 * c, 1, bias=True)
        self.out2 = nn.Conv2d(4 * c, 2 * c, 3, padding=1, bias=False)
        self.out3 = nn.Conv2d(4 * c, c, 3, padding=1, bias=False)
        self.out_channels = [4 * c, 2 * c, c]
        self._cache = _InferenceCache()
        self._raw_cache = _InferenceCache(_conv_weights)
        self._dgrad_cache = _InferenceCache(_conv_weights)

    def _layers(self):
        return list(self.conv0) + list(self.conv1) + list(self.conv2) + [self.out1, self.inner1, self.inner2, self.out2, self.out3]

    def _fold(self):
        out = []
        for layer in self._layers():
            w, b = fold_conv_bn(layer)
            out.append((ops.conv2d_pack(w.float()), b.float().contiguous()))
        return out

    def _raw(self):
        out = []
        for layer in self._layers():
            conv = layer.conv if hasattr(layer, "conv") else layer
            out.append((ops.conv2d_pack(conv.weight.detach().float()), torch.zeros(conv.out_channels, device=conv.weight.device)))
        return out

    def _dgrad(self):
        out = []
        for layer in self._layers():
            conv = layer.conv if hasattr(layer, "conv") else layer
            out.append(ops.conv2d_dgrad_pack(conv.weight.detach().float(), conv.stride[0], conv.padding[0]))
        return out

    @staticmethod
    def _pyramid(x, run, trunk=None):
        """The topology, once for every route: `run(i, t)` is layer i of `_layers()` on t.  `trunk(k, t)`: conv0 / conv1 / conv2 (k = 0, 1, 2) as a
        whole -- torch's route calls the nn.Sequential containers themselves, so that hooks on them fire; without it, their layers one by one."""
        if trunk is None:
            def trunk(k, t):
                for i in ((0, 1), (2, 3, 4), (5, 6, 7))[k]:
                    t = run(i, t)
                return t
        conv0 = trunk(0, x)
        conv1 = trunk(1, conv0)
        conv2 = trunk(2, conv1)
        outputs = {"stage1": run(8, conv2)}
        intra = F.interpolate(conv2, scale_factor=2, mode="nearest") + run(9, conv1)
        outputs["stage2"] = run(11, intra)
        intra = F.interpolate(intra, scale_factor=2, mode="nearest") + run(10, conv0)
        outputs["stage3"] = run(12, intra)
        return outputs

    def forward(self, x):
        run = self._device_runner(x)
        if run is not None:
            return self._pyramid(x, run)
        layers = self._layers()
        return self._pyramid(x, lambda i, t: layers[i](t), lambda k, t: (self.conv0, self.conv1, self.conv2)[k](t))

    def forward_views(self, imgs):
        """The features of all V views of one sample in ONE pass: imgs [1,V,3,H,W] or [V,3,H,W] -> {"stage1": [V,4c,H/4,W/4], "stage2":
        [V,2c,H/2,W/2], "stage3": [V,c,H,W]}, view i's rows being what `forward(imgs[:, i])` returns when the views are run one after another in
        ascending order, the batch-norm buffers left as those V calls leave them.  The route is chosen by `forward`'s own predicates: under
        eval() + no_grad one folded pass over the V images (already per image); under train() + no_grad with batch_stats="device" the same
        launches with every batch-norm keeping its statistics per view (`ops.batch_norm_train(..., groups=V)`: outputs and buffers bit for bit
        the loop's); under train() + grad with training="device" the layer functions on the V-image batch (`ops.conv2d_bn_train(..., groups=V)`:
        outputs, buffers and the image gradient bit for bit the loop's, the parameter gradients its sums in another order).  Anywhere else --
        torch's routes, CPU tensors -- it IS the loop, concatenated."""
        if not torch.is_tensor(imgs) or imgs.dim() not in (4, 5) or (imgs.dim() == 5 and imgs.shape[0] != 1) or imgs.shape[-4] < 1:
            raise RuntimeError("uc_nerf_amd FeatureNet.forward_views: imgs must be [1,V,3,H,W] or [V,3,H,W] with at least one view, got %s"
                               % (tuple(imgs.shape) if torch.is_tensor(imgs) else type(imgs),))
        x = imgs[0] if imgs.dim() == 5 else imgs
        V = x.shape[0]
        run = self._device_runner(x, groups=V)
        if run is not None:
            return self._pyramid(x, run)
        per_view = [self.forward(x[i:i + 1]) for i in range(V)]
        return {key: torch.cat([out[key] for out in per_view]) for key in per_view[0]}

    def _device_runner(self, x, groups=1):
        """`_pyramid`'s per-layer runner for the device route `forward`'s predicates choose for x -- folded, batch statistics or training, the
        batch-norms of the last two keeping their statistics per group of images -- or None where torch's layers run (also where `groups` is
        more than the kernels take)."""
        folded, stats = _device_route(self, x), False
        if not folded:
            stats = _batch_stats_route(self, x)
            if not (stats or _training_route(self, x)) or groups > ops.BN_MAX_GROUPS:
                return None
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 4 or x.shape[3] % 4:
            raise RuntimeError("uc_nerf_amd FeatureNet: the device route takes [n,3,H,W] with H and W divisible by 4 (the pyramid's additions need "
                               "it), got %s" % (tuple(x.shape),))
        f = self._cache.get(self, self._fold) if folded else self._raw_cache.get(self, self._raw)
        d = None if folded or stats else self._dgrad_cache.get(self, self._dgrad)
        layers = self._layers()

        def run(i, t):
            layer = layers[i]
            conv, bn = (layer.conv, layer.bn) if hasattr(layer, "conv") else (layer, None)
            if d is not None:                                # training: forward and backward on the kernels
                if bn is None:
                    return ops.conv2d_train(t, conv.weight, conv.bias, stride=conv.stride[0], pad=conv.padding[0], packed=f[i][0], packed_dgrad=d[i])
                return ops.conv2d_bn_train(t, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                           momentum=bn.momentum, eps=bn.eps, stride=conv.stride[0], pad=conv.padding[0], relu=layer.relu,
                                           packed=f[i][0], packed_dgrad=d[i], groups=groups)
            if folded or bn is None:                         # (batch statistics, no batch-norm: the convolution with its own bias)
                bias = f[i][1] if folded or conv.bias is None else conv.bias.detach()
                return ops.conv2d_bias_relu(t, f[i][0], bias, stride=conv.stride[0], pad=conv.padding[0], relu=getattr(layer, "relu", False))
            y = ops.conv2d_bias_relu(t, f[i][0], f[i][1], stride=conv.stride[0], pad=conv.padding[0], relu=False)
            return _bn_train(layer, y, groups=groups)

        return run


class CostRegNet(nn.Module):
    """mvs_models.py:412-443: variance volume [n,C,D,H,W] -> (cost [n,c,D,H,W], logits [n,1,D,H,W]); an hourglass of seven convolutions, three
    transposed ones with skip additions and the one-channel `prob`.  Names as in the reference, so `cost_regularization.N.*` keys load strictly.
    Two routes as in FeatureNet; the device route is eleven `ops.conv3d` launches (batch-norm folded, the skip additions inside the launches)
    and needs D, H and W divisible by 8 -- as the reference's additions do.  training="device" adds a fourth, under train() + grad enabled: every
    layer is `ops.conv3d_bn_train` (`ops.conv3d_train` for `prob`), forward and backward on the HIP kernels, the running statistics moved as
    torch moves them; the default "torch" keeps torch's layers there."""

    ORDER = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11", "prob")

    def __init__(self, in_channels, base_channels, inference="device", batch_stats="torch", training="torch"):
        super().__init__()
        self.inference = _check_route(inference)
        self.batch_stats = _check_batch_stats(batch_stats)
        self.training_route = _check_training(training)      # (nn.Module owns the attribute `training`)
        c = base_channels
        self.conv0 = Conv3d(in_channels, c, padding=1)
        self.conv1 = Conv3d(c, 2 * c, stride=2, padding=1)
        self.conv2 = Conv3d(2 * c, 2 * c, padding=1)
        self.conv3 = Conv3d(2 * c, 4 * c, stride=2, padding=1)
        self.conv4 = Conv3d(4 * c, 4 * c, padding=1)
        self.conv5 = Conv3d(4 * c, 8 * c, stride=2, padding=1)
        self.conv6 = Conv3d(8 * c, 8 * c, padding=1)
        self.conv7 = Deconv3d(8 * c, 4 * c, stride=2, padding=1, output_padding=1)
        self.conv9 = Deconv3d(4 * c, 2 * c, stride=2, padding=1, output_padding=1)
        self.conv11 = Deconv3d(2 * c, c, stride=2, padding=1, output_padding=1)
        self.prob = nn.Conv3d(c, 1, 3, stride=1, padding=1, bias=False)
        self._cache = _InferenceCache()
        self._raw_cache = _InferenceCache(_conv_weights)
        self._dgrad_cache = _InferenceCache(_conv_weights)

    def _dgrad(self):
        out = {}
        for name in self.ORDER:
            layer = getattr(self, name)
            conv = layer.conv if hasattr(layer, "conv") else layer
            out[name] = ops.conv3d_dgrad_pack(conv.weight.detach().float(), conv.stride[0], 1, getattr(layer, "transposed", False))
        return out

    def _fold(self):
        out = {}
        for name in self.ORDER:
            layer = getattr(self, name)
            w, b = fold_conv_bn(layer)
            out[name] = (ops.conv3d_pack(w.float(), transposed=getattr(layer, "transposed", False)), b.float().contiguous())
        return out

    def _raw(self):
        out = {}
        for name in self.ORDER:
            layer = getattr(self, name)
            conv = layer.conv if hasattr(layer, "conv") else layer
            cout = conv.out_channels
            out[name] = (ops.conv3d_pack(conv.weight.detach().float(), transposed=getattr(layer, "transposed", False)),
                         torch.zeros(cout, device=conv.weight.device))
        return out

    @staticmethod
    def _hourglass(x, conv):
        """The topology, once for every route: `conv(name, t, stride, skip)` is the named layer on t with `skip` added to its result."""
        conv0 = conv("conv0", x)
        conv2 = conv("conv2", conv("conv1", conv0, 2))
        conv4 = conv("conv4", conv("conv3", conv2, 2))
        x = conv("conv6", conv("conv5", conv4, 2))
        x = conv("conv7", x, 2, skip=conv4)
        x = conv("conv9", x, 2, skip=conv2)
        cost = conv("conv11", x, 2, skip=conv0)
        return cost, conv("prob", cost)

    def forward(self, x):
        return self._hourglass(x, self._device_conv(x) or self._torch_conv)

    def _torch_conv(self, name, t, stride=1, skip=None):
        """torch's layer (the stride is its own); the skip is added OUTSIDE the layer, as the reference adds it."""
        y = getattr(self, name)(t)
        return y if skip is None else skip + y

    def _device_conv(self, x):
        """`_hourglass`'s layer function for the device route `forward`'s predicates choose for x -- folded, batch statistics or training, the
        skip additions inside the launches -- or None where torch's layers run."""
        folded, stats = _device_route(self, x), False
        if not folded:
            stats = _batch_stats_route(self, x)
            if not (stats or _training_route(self, x)):
                return None
        if x.dim() != 5 or x.shape[2] % 8 or x.shape[3] % 8 or x.shape[4] % 8:
            raise RuntimeError("uc_nerf_amd CostRegNet: the device route takes [n,C,D,H,W] with D, H and W divisible by 8 (three halvings, three "
                               "doublings and the skip additions between them), got %s" % (tuple(x.shape),))
        f = self._cache.get(self, self._fold) if folded else self._raw_cache.get(self, self._raw)
        d = None if folded or stats else self._dgrad_cache.get(self, self._dgrad)

        def conv(name, t, stride=1, skip=None):
            layer = getattr(self, name)
            bn = getattr(layer, "bn", None)
            if d is not None:                                # training: forward and backward on the kernels
                if bn is None:
                    return ops.conv3d_train(t, layer.weight, 1, 1, packed=f[name][0], packed_dgrad=d[name])
                return ops.conv3d_bn_train(t, layer.conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                           momentum=bn.momentum, eps=bn.eps, stride=stride, pad=1, relu=layer.relu, skip=skip,
                                           transposed=layer.transposed, packed=f[name][0], packed_dgrad=d[name])
            if folded or bn is None:
                return ops.conv3d(t, f[name][0], f[name][1], stride=stride, pad=1, relu=getattr(layer, "relu", False), skip=skip, transposed=f[name][0].transposed)
            y = ops.conv3d(t, f[name][0], f[name][1], stride=stride, pad=1, relu=False, skip=None, transposed=f[name][0].transposed)
            return _bn_train(layer, y, skip)

        return conv


def mvs_depth_regression(p, depth_values):                 # mvs_models.py:574-579
    if depth_values.dim() <= 2:
        depth_values = depth_values.view(*depth_values.shape, 1, 1)
    return torch.sum(p * depth_values, 1)


class DepthNet(nn.Module):
    def forward(self, features, affine_mat_stage, affine_mat_inv_stage, depth_values, num_depth, cost_regularization, imgs,
                pad=0, prob_volume_init=None, *, depth_values_padded=False):
        """`depth_values_padded` (CascadeMVSNet, whose hypothesis kernel writes the replicate border itself): depth_values already is
        [1,D,H+2pad,W+2pad] and is not padded again."""
        features = torch.stack(list(features)) if not torch.is_tensor(features) else features      # [V,B,C,H,W]
        V, B, C, H, W = features.shape
        if B != 1:
            raise RuntimeError("uc_nerf_amd DepthNet: batch size 1 (as the reference's datasets provide)")
        if pad > 0 and not depth_values_padded:
            depth_values = F.pad(depth_values, (pad, pad, pad, pad), "replicate")
        # (src_proj @ ref_proj_inv)[:3] per source view (mvs_models.py:612); entry 0 of the stage matrices is the target view
        proj = (affine_mat_stage[1:V + 1] @ affine_mat_inv_stage[0:1])[:, :3].contiguous()
        variance = ops.cost_volume(features[:, 0], proj, depth_values[0], pad=pad)
        cost_feat_no_ref, prob = cost_regularization(variance.unsqueeze(0))
        prob_pre = prob.squeeze(1)
        prob_volume, depth, conf = ops.depth_regress(prob_pre[0], depth_values[0],
                                                     None if prob_volume_init is None else prob_volume_init[0], pad=pad)
        return {"depth": depth.unsqueeze(0), "photometric_confidence": conf.unsqueeze(0),
                "volume_feature_no_ref": cost_feat_no_ref, "depth_values": depth_values, "img_feats": features,
                "prob_volume": prob_volume.unsqueeze(0)}


def _dev_scalar(v, device):
    """A near / far / interval handed over as a tensor (wherever it lives) or a number -> one float32 element on `device`; a device value
    is never read back."""
    if torch.is_tensor(v):
        return v.detach().to(device=device, dtype=torch.float32).reshape(1)
    return torch.tensor([float(v)], dtype=torch.float32, device=device)


def _batch_one(t, what):
    if t.shape[0] != 1:
        raise RuntimeError("uc_nerf_amd %s: batch size 1 (as the reference's datasets provide)" % what)
    return t[0]


def get_cur_depth_range_samples(cur_depth, ndepth, depth_inteval_pixel, shape, max_depth=192.0, min_depth=0.0):
    """mvs_models.py:536-551.  cur_depth [1,H,W] -> [1,D,H,W]: `ucnerf_depth_hypotheses` with the output at the map's own resolution.
    Differentiable with respect to cur_depth, as the reference's torch expressions are (the bounds and the interval get no gradient)."""
    if tuple(cur_depth.shape) != tuple(shape):
        raise AssertionError("cur_depth:{}, input shape:{}".format(cur_depth.shape, shape))
    c = _batch_one(cur_depth, "get_cur_depth_range_samples")
    dev = c.device
    near_far = torch.cat([_dev_scalar(min_depth, dev), _dev_scalar(max_depth, dev)])
    out = ops.depth_hypotheses(ndepth, c.shape, cur_depth=c, near_far=near_far, k=1.0, interval=_dev_scalar(depth_inteval_pixel, dev))
    return out.unsqueeze(0)


def get_depth_range_samples(cur_depth, ndepth, depth_inteval_pixel, device, dtype, shape, max_depth=192.0, min_depth=0.0):
    """mvs_models.py:554-573.  cur_depth [1,H,W] (a depth map) or [1,D_in] (a hypothesis row: the band row[0] .. row[-1] for every pixel)
    -> [1,D,H,W], float32 on cur_depth's device."""
    if cur_depth.dim() == 2:
        row = _batch_one(cur_depth, "get_depth_range_samples")
        return ops.depth_hypotheses(ndepth, (shape[1], shape[2]), row=row).unsqueeze(0)
    return get_cur_depth_range_samples(cur_depth, ndepth, depth_inteval_pixel, shape, max_depth, min_depth)


class CascadeMVSNet(nn.Module):
    """mvs_models.py:648-762: the three-stage loop around the caller's CNNs.  `feature` (the reference's FeatureNet: image [1,3,H,W] ->
    {"stage1": [1,C1,H/4,W/4], "stage2": ..., "stage3": ...}) and `cost_regularization` (its CostRegNets: variance volume [1,C,D,h,w] ->
    (volume feature, logits [1,1,D,h,w]); an nn.ModuleList / sequence with one per stage, or ONE module with share_cr) are handed in --
    they are registered under the reference's attribute names, so a reference checkpoint's `feature.*` / `cost_regularization.*` keys load.
    Per stage: `ucnerf_depth_hypotheses` (one launch, replicate border included) -> `DepthNet` (cost volume, the caller's regulariser,
    depth regression).  grad_method "detach": the previous stage's depth is detached before the next stage's hypotheses are built; "undetach"
    (the other branch of :716-719): it is not, and the hypotheses, the regressed depth and so the earlier stages carry its gradient.  The reference
    takes ANY other string for that branch; here a value that is neither of the two is refused, so that a misspelt "detach" does not silently
    change what trains.
    `feature_views`: "loop" (the default, the reference's: `feature` is called once per view) or "batched": `feature.forward_views(imgs)` is
    called once for all views (FeatureNet's gives the loop's features, see there) and `DepthNet` reads its [V,C,h,w] tensors where they are."""

    GRAD_METHODS = ("detach", "undetach")
    FEATURE_VIEWS = ("loop", "batched")

    def __init__(self, view_num=11, ndepths=[48, 32, 8], depth_interals_ratio=[4, 2, 1], share_cr=False, grad_method="detach",
                 arch_mode="fpn", cr_base_chs=[8, 8, 8], *, feature=None, cost_regularization=None, feature_views="loop"):
        super().__init__()
        if not isinstance(feature_views, str) or feature_views not in self.FEATURE_VIEWS:
            raise ValueError("uc_nerf_amd CascadeMVSNet: feature_views=%r -- \"loop\" (the feature net is called once per view) or \"batched\" (its "
                             "forward_views once for all of them)" % (feature_views,))
        if grad_method not in self.GRAD_METHODS:
            raise NotImplementedError("uc_nerf_amd CascadeMVSNet: grad_method=%r -- \"detach\" (the reference's default: the depth is detached between "
                                      "stages) or \"undetach\" (it stays in the graph)" % (grad_method,))
        missing = [n for n, m in (("feature", feature), ("cost_regularization", cost_regularization)) if m is None]
        if missing:
            raise ValueError("uc_nerf_amd CascadeMVSNet: the CNNs are the caller's modules -- pass %s=... (the reference's FeatureNet / "
                             "CostRegNets, see INTEGRATION.md)" % "=..., ".join(missing))
        if len(ndepths) != len(depth_interals_ratio):
            raise AssertionError("ndepths and depth_interals_ratio differ in length")
        self.share_cr, self.ndepths, self.depth_interals_ratio = share_cr, list(ndepths), list(depth_interals_ratio)
        self.grad_method, self.arch_mode, self.cr_base_chs = grad_method, arch_mode, cr_base_chs
        self.view_num = view_num
        self.num_stage = len(ndepths)
        self.refine = False
        self.stage_infos = {"stage1": {"scale": 4.0}, "stage2": {"scale": 2.0}, "stage3": {"scale": 1.0}}
        if self.num_stage > len(self.stage_infos):
            raise ValueError("uc_nerf_amd CascadeMVSNet: at most %d stages" % len(self.stage_infos))
        if feature_views == "batched" and not callable(getattr(feature, "forward_views", None)):
            raise ValueError("uc_nerf_amd CascadeMVSNet: feature_views=\"batched\" needs a feature module with a forward_views(imgs) method (as "
                             "uc_nerf_amd's FeatureNet has), got %s" % type(feature).__name__)
        self.feature_views = feature_views
        self.feature = feature
        per_stage = isinstance(cost_regularization, (list, tuple, nn.ModuleList))
        if share_cr:
            if per_stage:
                raise ValueError("uc_nerf_amd CascadeMVSNet: share_cr=True takes ONE cost_regularization module")
        else:
            if not per_stage or len(cost_regularization) != self.num_stage:
                raise ValueError("uc_nerf_amd CascadeMVSNet: cost_regularization must hold one module per stage (%d)" % self.num_stage)
            if not isinstance(cost_regularization, nn.ModuleList) and all(isinstance(m, nn.Module) for m in cost_regularization):
                cost_regularization = nn.ModuleList(cost_regularization)
        self.cost_regularization = cost_regularization
        self.DepthNet = DepthNet()

    @classmethod
    def with_cnns(cls, view_num=11, ndepths=[48, 32, 8], depth_interals_ratio=[4, 2, 1], share_cr=False, grad_method="detach",
                  arch_mode="fpn", cr_base_chs=[8, 8, 8], inference="device", batch_stats="torch", training="torch", feature_training="torch",
                  feature_views="loop"):
        """The net with its own `FeatureNet` and one `CostRegNet` per stage (mvs_models.py:678-687), so that a reference checkpoint loads and
        runs without the reference's source.  `inference`: the route both kinds of module take under eval() + no_grad ("device" or "torch");
        `batch_stats`: the one they take under train() + no_grad ("torch", or "device" with inference="device"); `training`: the one the
        `CostRegNet`s take under train() + grad enabled ("torch", or "device" with inference="device": forward and backward on the HIP kernels);
        `feature_training`: the same choice for the `FeatureNet`.  With both "device" a training step stays on the project's kernels end to end.
        `feature_views`: "loop" or "batched", as in the constructor."""
        if not isinstance(feature_views, str) or feature_views not in cls.FEATURE_VIEWS:
            raise ValueError("uc_nerf_amd CascadeMVSNet.with_cnns: feature_views=%r -- \"loop\" or \"batched\"" % (feature_views,))
        if share_cr:
            raise NotImplementedError("uc_nerf_amd CascadeMVSNet.with_cnns: share_cr=True (one regulariser for stages whose feature channels "
                                      "differ; the reference's constructor fails on it too) -- hand a module in through CascadeMVSNet(...)")
        feature = FeatureNet(base_channels=8, stride=4, num_stage=len(ndepths), arch_mode=arch_mode, inference=inference, batch_stats=batch_stats,
                             training=feature_training)
        regs = nn.ModuleList([CostRegNet(in_channels=feature.out_channels[i], base_channels=cr_base_chs[i], inference=inference, batch_stats=batch_stats,
                                         training=training)
                              for i in range(len(ndepths))])
        return cls(view_num, ndepths, depth_interals_ratio, share_cr, grad_method, arch_mode, cr_base_chs, feature=feature, cost_regularization=regs,
                   feature_views=feature_views)

    def forward(self, imgs, affine_mat, affine_mat_inv, near_far, pad):
        if imgs.shape[0] != 1:
            raise RuntimeError("uc_nerf_amd CascadeMVSNet: batch size 1 (as the reference's datasets provide)")
        dev = imgs.device
        H, W = imgs.shape[3], imgs.shape[4]
        # (near, far) on the device: read there by the kernel.  The stage-1 row of the reference, near * (1 - t) + far * t over 48 steps
        # (:694-699), is only ever read at its two ends -- near and far themselves -- so the pair stands for it.
        near_far = torch.cat([_dev_scalar(near_far[0], dev), _dev_scalar(near_far[1], dev)])
        if self.feature_views == "batched":
            batched = self.feature.forward_views(imgs)                                   # {stage: [V,C,h,w]}
        else:
            features = [self.feature(imgs[:, i]) for i in range(imgs.size(1))]
        outputs = {}
        depth = None
        for stage_idx in range(self.num_stage):
            key = "stage{}".format(stage_idx + 1)
            # ([V,1,C,h,w] as a view: DepthNet takes a tensor as it is, no torch.stack copy)
            features_stage = batched[key].unsqueeze(1) if self.feature_views == "batched" else [feat[key] for feat in features]
            scale = int(self.stage_infos[key]["scale"])
            stage_pad = pad if stage_idx == 2 else 0                                     # :735-740
            D = self.ndepths[stage_idx]
            if depth is None:
                depth_value = ops.depth_hypotheses(D, (H // scale, W // scale), row=near_far, pad=stage_pad)
            else:
                cur_depth = depth.detach() if self.grad_method == "detach" else depth                # :716-719
                # depth_inteval_pixel = ratio * (far - near) / 48: the reference divides by the literal 48 (:694,698), not by ndepths[0]
                depth_value = ops.depth_hypotheses(D, (H // scale, W // scale), cur_depth=cur_depth[0], near_far=near_far,
                                                   k=self.depth_interals_ratio[stage_idx] / 48.0, full_hw=(H, W), pad=stage_pad)
            cr = self.cost_regularization if self.share_cr else self.cost_regularization[stage_idx]
            outputs_stage = self.DepthNet(features_stage, affine_mat[:, stage_idx], affine_mat_inv[:, stage_idx], depth_values=depth_value.unsqueeze(0),
                                          num_depth=D, cost_regularization=cr, imgs=imgs, pad=stage_pad, depth_values_padded=True)
            depth = outputs_stage["depth"]
            outputs[key] = outputs_stage
            outputs.update(outputs_stage)
        return outputs["stage3"]["volume_feature_no_ref"], outputs["stage3"]["photometric_confidence"], outputs["stage3"]["depth"], outputs
