"""The MLP: backward mode and split operand (this module owns both settings and the guard word), weight packing, forward / backward."""
import ctypes as C
import os

import torch

from .. import _lib as L
from ._core import _cur_dev, _f32, _launch, _on, _ptr, _stream

BACKWARD_MODES = {"chain": 0, "layerwise": 1}
_backward_mode = BACKWARD_MODES[os.environ.get("UCNERF_BWD_MODE", "chain")]


def set_backward_mode(mode):
    """MLP backward: "chain" (default) = the register-resident gradient chain (one kernel walks the network backwards per 32-sample tile,
    split-bf16 data gradients, include/ucnerf_hip.h: bwd_mode 0), "layerwise" = the exact-fp32 layer-by-layer GEMMs (bwd_mode 1)."""
    global _backward_mode
    _backward_mode = BACKWARD_MODES[mode]


def backward_mode():
    return ("chain", "layerwise")[_backward_mode]


# (2 is this module's own code for the guarded mode: the ABI knows operands 0 and 1 -- the guard is a property of the call, PackedWeights.guarded)
SPLIT_OPERANDS = {"bf16": 0, "fp16": 1, "fp16_guarded": 2}
_split_operand = SPLIT_OPERANDS[os.environ.get("UCNERF_SPLIT_OPERAND", "bf16")]


def set_split_operand(kind):
    """The 16-bit terms of the split precisions ("bf16x3", "bf16x3_fused", "bf16") from now on (ucnerf_mlp_config.operand, ABI v6): "bf16" (default:
    8 significant bits per term, float32's range) or "fp16" (11 bits per term at the same matrix-core rate -- the three-product split then holds ~22
    bits and the renders sit at float32 level, no measurable kernel time (+0.1 %) -- but fp16's range: an activation beyond 131 008 is clamped, a term below 6e-5 is held
    to 3e-8 absolute; a WEIGHT beyond 65 504 packs to infinities and renders NaN).  Takes effect
    for every weight stream packed afterwards (PackedWeights.get keys on it); inference only.

    "fp16_guarded": the fp16 terms with their range watched on the device.  Every pack and every no_grad launch runs kernels that compute exactly
    what "fp16" computes and OR a bit into a per-device status word when a value left fp16's safe range (bit 0: an activation or input with
    |x| >= 65 504 -- conservative, clamping starts at 131 008; bit 1: a weight whose hi term is not finite or reaches 65 504).  Directly behind each
    such launch, and before anything consumes its outputs, the same pass is enqueued once more on bf16 terms under `run_if = status`: its kernels return
    at once while the word is zero.  No host synchronisation; the outputs of a call are bit-identical to "fp16" when nothing saturated and to "bf16"
    when something did.  The word is STICKY -- the library never clears it, so after one saturated call every later call replays (and equals "bf16")
    until split_guard_clear(): the safe direction.  Not caught, and unchanged from "fp16": terms below 6e-5 lose relative precision (they stay
    within the absolute bar).  Cost: the range checks (a few vector instructions per split), one skipped launch per pass, and a pass's bf16 time
    on top when it does replay.  A weight stream holds both term kinds (twice the floats)."""
    global _split_operand
    if kind not in SPLIT_OPERANDS:
        raise ValueError("uc_nerf_amd: split operand must be 'bf16', 'fp16' or 'fp16_guarded', got %r" % (kind,))
    _split_operand = SPLIT_OPERANDS[kind]


def split_operand():
    return ("bf16", "fp16", "fp16_guarded")[_split_operand]


# one status word per device of the guarded split, allocated once and kept for the life of the process: captured graphs hold its address
_guard_words = {}


def _guard_word(device):
    device = torch.device(device)
    idx = device.index if device.index is not None else _cur_dev()
    w = _guard_words.get(idx)
    if w is None:
        w = _guard_words[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return w


def split_guard_status(clear=False, device=None):
    """The guarded split's status word of `device` (default: the current one) as an int: bit 0 = an activation or input reached 65 504 in a
    "fp16_guarded" launch, bit 1 = a weight did in a pack; 0 = every call since the last clear ran on fp16 terms.  SYNCHRONISES (reads the word back);
    clear=True also zeroes it afterwards.  The word is sticky: while it is non-zero every guarded call replays on bf16 terms."""
    w = _guard_word(device if device is not None else torch.device("cuda", _cur_dev()))
    v = int(w.item()) & 0xffffffff
    if clear:
        w.zero_()
    return v


def split_guard_clear(device=None):
    """Enqueues a clear of the status word on the current stream (no synchronisation): calls enqueued afterwards run on fp16 terms again."""
    _guard_word(device if device is not None else torch.device("cuda", _cur_dev())).zero_()


def _launch_split(pw, name, params, device):
    """_launch for the entry points that run the network (`params`: .cfg and .wstream): in the guarded mode the fp16 launch with range detection, then
    the same call on the bf16 half of the stream under run_if = the status word -- same stream, same inputs, before anything reads the outputs."""
    if not pw.guarded:
        return _launch(name, params, device)
    word = _ptr(_guard_word(device))
    lib = L.lib()
    ws = params.wstream
    with _on(device):
        st = C.c_void_p(_stream())
        L.check(getattr(lib, name + "_guarded")(C.addressof(params), C.c_void_p(word), st), name + "_guarded")
        params.cfg.operand, params.wstream = 0, ws + 4 * pw.n_stream_terms
        try:
            L.check(getattr(lib, name + "_if")(C.addressof(params), C.c_void_p(word), st), name + "_if")
        finally:
            params.cfg.operand, params.wstream = 1, ws


class PackedWeights:
    """Pack index (host-built by the library, cached on device) + packing of a flat parameter vector."""
    _cache = {}

    PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2, "bf16x3_fused": 3}     # 3: bf16x3 with the gather inside the MLP kernel (render passes only)

    def __init__(self, n_src, pe_layout, device, precision="f32", operand=0):
        operand = 0 if precision == "f32" else int(operand)
        # operand 2 = "fp16_guarded": the ABI's operand 1 with guarded calls; the stream is [fp16 terms | bf16 terms], the second half for the replay
        self.guarded = operand == 2
        self.cfg = L.MlpConfig(n_src, pe_layout, self.PRECISIONS[precision], 1 if self.guarded else operand)
        self.precision, self.operand = precision, operand
        lib = L.lib()
        self.n_params = lib.ucnerf_mlp_param_count(C.addressof(self.cfg))
        self.n_stream_terms = lib.ucnerf_mlp_stream_count(C.addressof(self.cfg))       # floats of ONE term kind's stream (the same for both kinds)
        self.n_stream = self.n_stream_terms * (2 if self.guarded else 1)
        if self.guarded:
            self.cfg_bf16 = L.MlpConfig(n_src, pe_layout, self.PRECISIONS[precision], 0)
            if torch.device(device).type == "cuda":
                _guard_word(device)                     # (made here: never inside a graph capture)
        n_idx = lib.ucnerf_mlp_index_count(C.addressof(self.cfg))
        if self.n_params < 0 or self.n_stream < 0 or n_idx < 0:
            raise RuntimeError("uc_nerf_amd: unsupported MLP config n_src=%d precision=%s: %s"
                               % (n_src, precision, lib.ucnerf_last_error().decode()))
        idx = torch.empty(n_idx, dtype=torch.int32)
        L.check(lib.ucnerf_mlp_pack_index(C.addressof(self.cfg), C.c_void_p(idx.data_ptr())), "ucnerf_mlp_pack_index")
        self.idx_host = idx
        self.idx = idx.to(device)
        self.device = device

    @classmethod
    def get(cls, n_src, pe_layout, device, precision="f32", operand=None):
        """operand: None = the module's current setting (set_split_operand); "bf16" / "fp16" / "fp16_guarded" / 0 / 1 / 2 to pin it."""
        op = _split_operand if operand is None else SPLIT_OPERANDS.get(operand, operand)
        op = 0 if precision == "f32" else int(op)
        key = (n_src, pe_layout, str(device), precision, op)
        if key not in cls._cache:
            cls._cache[key] = cls(n_src, pe_layout, device, precision, op)
        return cls._cache[key]

    def pack(self, flat, out=None):
        """The packed stream of a flat parameter vector; into `out` (a stream buffer of this packer) when given."""
        flat = _f32(flat, "flat parameters")
        if flat.numel() != self.n_params:
            raise RuntimeError("uc_nerf_amd: flat parameter vector has %d floats, expected %d"
                               % (flat.numel(), self.n_params))
        if out is None:
            out = torch.empty(self.n_stream, device=flat.device)
        elif out.numel() != self.n_stream or out.dtype != torch.float32 or not out.is_contiguous() or out.device != flat.device:
            raise RuntimeError("uc_nerf_amd: stream buffer must be %d contiguous float32 on the parameters' device" % self.n_stream)
        with _on(flat.device):
            if self.guarded:
                self._pack_guarded("ucnerf_mlp_pack", (_ptr(flat),), out)
            else:
                L.check(L.lib().ucnerf_mlp_pack(C.addressof(self.cfg), _ptr(flat), _ptr(self.idx), _ptr(out), _stream()), "ucnerf_mlp_pack")
        return out

    def _pack_guarded(self, name, src_args, out):
        """The guarded fp16 pack into the first half of `out`, the bf16 pack into the second.  The bf16 half is packed UNCONDITIONALLY (the plain
        entry point, not ucnerf_*_pack*_if under the status word): a launch that saturates later -- an activation, with finite weights -- replays
        against this half, so it has to be there whatever the word reads at pack time."""
        lib, st = L.lib(), C.c_void_p(_stream())
        idx, o = C.c_void_p(_ptr(self.idx)), _ptr(out)
        L.check(getattr(lib, name + "_guarded")(C.addressof(self.cfg), *src_args, idx, C.c_void_p(o), C.c_void_p(_ptr(_guard_word(out.device))), st),
                name + "_guarded")
        L.check(getattr(lib, name)(C.addressof(self.cfg_bf16), *src_args, idx, C.c_void_p(o + 4 * self.n_stream_terms), st), name)

    def pack_table(self, table, out):
        """Packs the stream straight from separate parameter tensors (TensorTable) into `out`, in place: one launch, no concatenation."""
        if table.total != self.n_params:
            raise RuntimeError("uc_nerf_amd: the parameter tensors hold %d floats, expected %d" % (table.total, self.n_params))
        if out.numel() != self.n_stream or out.dtype != torch.float32 or not out.is_contiguous():
            raise RuntimeError("uc_nerf_amd: stream buffer must be %d contiguous float32" % self.n_stream)
        with _on(out.device):
            if self.guarded:
                self._pack_guarded("ucnerf_mlp_pack_tensors", (table.n, table.ptrs, table.numel), out)
            else:
                L.check(L.lib().ucnerf_mlp_pack_tensors(C.addressof(self.cfg), table.n, table.ptrs, table.numel, _ptr(self.idx), _ptr(out), _stream()),
                        "ucnerf_mlp_pack_tensors")
        return out

    def unpack_grad(self, g_stream):
        g_flat = torch.zeros(self.n_params, device=g_stream.device)
        with _on(g_stream.device):
            L.check(L.lib().ucnerf_mlp_unpack_grad(_ptr(g_stream), _ptr(self.idx), _ptr(g_flat), self.n_stream, _stream()),
                    "ucnerf_mlp_unpack_grad")
        return g_flat


class TensorTable:
    """Host-side table of device pointers / element counts of a network's parameter tensors (state_dict order) for
    PackedWeights.pack_table; `key` = the data pointers it was built from."""

    def __init__(self, tensors):
        tensors = list(tensors)
        for t in tensors:
            if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("uc_nerf_amd.TensorTable: parameters must be contiguous float32 tensors on a ROCm device")
        self.n = len(tensors)
        self.key = tuple(t.data_ptr() for t in tensors)
        self.ptrs = (C.c_void_p * self.n)(*self.key)
        self.numel = (C.c_int64 * self.n)(*[t.numel() for t in tensors])
        self.total = sum(t.numel() for t in tensors)


def mlp_fwd(pw, wstream, pts, dirs, feats, S, feats_tiled=False, max_blocks=0):
    """pts [m,3] (any leading shape), dirs [m/S,3] or [m,3], feats [m,F] or tiled buffer -> raw [m,4]."""
    pts, dirs, feats = _f32(pts, "pts"), _f32(dirs, "dirs"), _f32(feats, "feats")
    m = pts.numel() // 3
    p = L.MlpParams()
    p.cfg = pw.cfg
    p.m, p.S = m, int(S)
    n_dirs = dirs.numel() // 3
    if n_dirs == m:
        p.dirs_per_sample = 1
    elif S > 0 and n_dirs * S == m:
        p.dirs_per_sample = 0
    else:
        raise RuntimeError("uc_nerf_amd.mlp_fwd: %d directions for %d samples (S=%d)" % (n_dirs, m, S))
    F = 24 + 12 * pw.cfg.n_src + 1
    need = ((m + 31) // 32) * 32 * F if feats_tiled else m * F
    if feats.numel() != need:
        raise RuntimeError("uc_nerf_amd.mlp_fwd: feats has %d floats, expected %d" % (feats.numel(), need))
    p.feats_tiled, p.max_blocks = int(feats_tiled), int(max_blocks)
    raw = torch.empty(m, 4, device=pts.device)
    p.pts, p.dirs, p.feats, p.wstream, p.raw = _ptr(pts), _ptr(dirs), _ptr(feats), _ptr(wstream), _ptr(raw)
    _launch_split(pw, "ucnerf_mlp_fwd", p, pts.device)
    return raw


KEPT_SETS = ("bd", "h0", "h1", "h2", "h3", "h4", "h5", "bc", "ft", "vc")       # order of the activation sets at the head of the backward workspace


def decode_p24(buf, m, cols=128):
    """fp32 [m, cols] view-copy of a set kept in the 24-bit format of csrc/p24.h (rows of 3 * cols bytes: the top three bytes of every fp32)."""
    b = buf.view(torch.uint8)[: m * cols * 3].view(m, cols, 3).to(torch.int32)
    bits = (b[..., 0] << 8) | (b[..., 1] << 16) | (b[..., 2] << 24)
    return bits.view(torch.float32)


def mlp_fwd_train(pw, wstream, pts, dirs, feats, S, bwd_mode=None):
    """ucnerf_mlp_fwd_train: the forward that keeps its activation sets for ucnerf_mlp_bwd (tests / diagnostics).  Returns (raw, sets): the ten
    [m,128] sets decoded to fp32, whatever format the backward mode keeps them in (0 / "chain": 24-bit floats, 1 / "layerwise": fp32)."""
    pts, dirs, feats = _f32(pts), _f32(dirs), _f32(feats)
    mode = _backward_mode if bwd_mode is None else BACKWARD_MODES[bwd_mode] if isinstance(bwd_mode, str) else int(bwd_mode)
    m = pts.numel() // 3
    p = L.MlpParams()
    p.cfg = pw.cfg
    p.m, p.S = m, int(S)
    n_dirs = dirs.numel() // 3
    p.dirs_per_sample = int(n_dirs == m)
    if not p.dirs_per_sample and n_dirs * int(S) != m:
        raise RuntimeError("uc_nerf_amd.mlp_fwd_train: %d directions for %d samples (S=%d)" % (n_dirs, m, S))
    raw = torch.empty(m, 4, device=pts.device)
    ws = torch.zeros(L.lib().ucnerf_mlp_bwd_workspace_floats(C.addressof(pw.cfg), m), device=pts.device)
    p.pts, p.dirs, p.feats, p.wstream, p.raw = _ptr(pts), _ptr(dirs), _ptr(feats), _ptr(wstream), _ptr(raw)
    with _on(pts.device):
        L.check(L.lib().ucnerf_mlp_fwd_train(C.addressof(p), _ptr(ws), mode, _stream()), "ucnerf_mlp_fwd_train")
    per = (m * 128 + 3) // 4 * 4
    sets = {}
    for i, name in enumerate(KEPT_SETS):
        chunk = ws[i * per:(i + 1) * per]
        sets[name] = decode_p24(chunk, m) if mode == 0 else chunk[: m * 128].view(m, 128).clone()
    return raw, sets


def mlp_bwd(pw, wstream, flat, pts, dirs, feats, S, g_raw):
    """Gradients of sum(raw * g_raw) w.r.t. feats [m,F] and the flat parameter vector."""
    pts, dirs, feats, g_raw, flat = _f32(pts), _f32(dirs), _f32(feats), _f32(g_raw), _f32(flat)
    m = pts.numel() // 3
    F = 24 + 12 * pw.cfg.n_src + 1
    bp = L.MlpBwdParams()
    p = bp.fwd
    p.cfg = pw.cfg
    p.m, p.S = m, int(S)
    n_dirs = dirs.numel() // 3
    if n_dirs == m:
        p.dirs_per_sample = 1
    elif S > 0 and n_dirs * S == m:
        p.dirs_per_sample = 0
    else:
        raise RuntimeError("uc_nerf_amd.mlp_bwd: %d directions for %d samples (S=%d)" % (n_dirs, m, S))
    if feats.numel() != m * F or g_raw.numel() != m * 4:
        raise RuntimeError("uc_nerf_amd.mlp_bwd: feats must be [m,%d] row-major and g_raw [m,4]" % F)
    need = L.lib().ucnerf_mlp_bwd_workspace_floats(C.addressof(pw.cfg), m)
    ws = torch.empty(need, device=pts.device)
    g_feats = torch.empty(m, F, device=pts.device)
    g_flat = torch.zeros(pw.n_params, device=pts.device)
    p.pts, p.dirs, p.feats, p.wstream, p.raw = _ptr(pts), _ptr(dirs), _ptr(feats), _ptr(wstream), _ptr(g_raw)
    bp.g_raw, bp.flat_params, bp.g_feats, bp.g_flat, bp.workspace = _ptr(g_raw), _ptr(flat), _ptr(g_feats), _ptr(g_flat), _ptr(ws)
    bp.bwd_mode = _backward_mode
    _launch("ucnerf_mlp_bwd", bp, pts.device)
    return g_feats, g_flat


class _MLP(torch.autograd.Function):
    """raw = MLP(PE(pts), feats, PE(dirs)); differentiable w.r.t. the flat parameters and feats."""

    @staticmethod
    def forward(ctx, flat, feats, pts, dirs, pw, S, ws=None):
        ws = pw.pack(flat) if ws is None else ws        # (a stream already packed from these very parameters may be handed in)
        ctx.pw, ctx.S = pw, S
        ctx.save_for_backward(flat, feats, pts, dirs, ws)
        return mlp_fwd(pw, ws, pts, dirs, feats.reshape(-1, feats.shape[-1]), S)

    @staticmethod
    def backward(ctx, g_raw):
        flat, feats, pts, dirs, ws = ctx.saved_tensors
        g_feats, g_flat = mlp_bwd(ctx.pw, ws, flat, pts, dirs, feats.reshape(-1, feats.shape[-1]), ctx.S, g_raw)
        return g_flat, g_feats.view(feats.shape), None, None, None, None, None


def mlp(flat, feats, pts, dirs, pw, S, wstream=None):
    return _MLP.apply(flat, feats, pts, dirs, pw, S, wstream)


def _encoded_params(p, pw, x):
    """Points pts / feats / dirs of an MlpParams into the columns of x [m, 63 + F + 27]."""
    F = 24 + 12 * pw.cfg.n_src + 1
    X = 63 + F + 27
    if x.shape[-1] != X:
        raise RuntimeError("uc_nerf_amd: encoded MLP input must have %d columns (63 + %d + 27), got %d" % (X, F, x.shape[-1]))
    p.cfg = pw.cfg
    p.m, p.S, p.dirs_per_sample, p.encoded = x.shape[0], 1, 1, 1
    p.pts_stride = p.dirs_stride = p.feat_stride = X
    base = x.data_ptr()
    p.pts, p.feats, p.dirs = base, base + 4 * 63, base + 4 * (63 + F)
    return F, X


def mlp_fwd_encoded(pw, wstream, x):
    x = _f32(x, "x")
    p = L.MlpParams()
    _encoded_params(p, pw, x)
    raw = torch.empty(x.shape[0], 4, device=x.device)
    p.wstream, p.raw = _ptr(wstream), _ptr(raw)
    _launch_split(pw, "ucnerf_mlp_fwd", p, x.device)
    return raw


class _MLPEncoded(torch.autograd.Function):
    """UCNeRF.forward(x) on the reference's pre-encoded 187-wide rows.  Gradients: parameters and the feature
    columns of x; the encoded pts/dir columns get zeros (positions are not differentiable on this path)."""

    @staticmethod
    def forward(ctx, flat, x, pw, ws=None):
        ws = pw.pack(flat) if ws is None else ws
        x = _f32(x, "x")
        if x.requires_grad or flat.requires_grad:
            # the weight-gradient kernel reads its operands in 16-byte pieces: the last piece of the last row (direction columns 24 .. 27 of 27)
            # ends four bytes past the matrix -- keep the copy the backward reads inside a buffer that has them
            buf = torch.empty(x.numel() + 4, device=x.device)
            xp = buf[:x.numel()].view(x.shape)
            xp.copy_(x)
            x = xp
        ctx.pw = pw
        ctx.save_for_backward(flat, x, ws)
        return mlp_fwd_encoded(pw, ws, x)

    @staticmethod
    def backward(ctx, g_raw):
        flat, x, ws = ctx.saved_tensors
        pw = ctx.pw
        g_raw = _f32(g_raw)
        bp = L.MlpBwdParams()
        F, X = _encoded_params(bp.fwd, pw, x)
        m = x.shape[0]
        wsz = L.lib().ucnerf_mlp_bwd_workspace_floats(C.addressof(pw.cfg), m)
        work = torch.empty(wsz, device=x.device)
        g_x = torch.zeros(m, X, device=x.device)
        g_flat = torch.zeros(pw.n_params, device=x.device)
        bp.fwd.wstream, bp.fwd.raw = _ptr(ws), _ptr(g_raw)
        bp.g_raw, bp.flat_params, bp.g_flat, bp.workspace = _ptr(g_raw), _ptr(flat), _ptr(g_flat), _ptr(work)
        bp.g_feats, bp.g_feat_stride = g_x.data_ptr() + 4 * 63, X
        bp.bwd_mode = _backward_mode
        _launch("ucnerf_mlp_bwd", bp, x.device)
        return g_flat, g_x, None, None


def mlp_encoded(flat, x, pw, wstream=None):
    return _MLPEncoded.apply(flat, x, pw, wstream)


def untile_feats(feats, m, F):
    """Row-major [m, F] view-copy of features kept in the MLP's tile layout [ceil(m/32)][F][32] (what a training forward keeps)."""
    return feats.view(-1, F, 32).permute(0, 2, 1).reshape(-1, F)[:m]
