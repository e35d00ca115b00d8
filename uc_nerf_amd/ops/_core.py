"""Argument checks, the current stream and device, and the one launch path every wrapper of this package goes through."""
import ctypes as C

import torch

from .. import _lib as L


def _dev(t):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("uc_nerf_amd: expected a tensor on a ROCm device, got %s"
                           % (t.device if torch.is_tensor(t) else type(t)))
    return t.device


def _f32(t, name="tensor"):
    _dev(t)
    if t.dtype != torch.float32:
        raise RuntimeError("uc_nerf_amd: %s must be float32, got %s" % (name, t.dtype))
    return t.contiguous()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _opt(t, name="tensor"):
    """An optional tensor (an upstream gradient autograd left out, a coordinate set not given) as contiguous float32, or None."""
    return _f32(t, name) if t is not None else None


def _dev_f32(t, name, numel=None, dev=None):
    """`t` as it is when it is a contiguous float32 tensor on the device (read in place by a kernel); one conversion otherwise."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        t = torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
        if not t.is_cuda:
            raise RuntimeError("uc_nerf_amd: %s must live on a ROCm device" % name)
    if numel is not None and t.numel() < numel:
        raise RuntimeError("uc_nerf_amd: %s has %d elements, expected at least %d" % (name, t.numel(), numel))
    return t


def _dev_as(t, name, dtype):
    """`t` as a contiguous `dtype` tensor on its own device (converted there when it has to be); never uploaded, never read back."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("uc_nerf_amd: %s must live on a ROCm device" % name)
    return t if t.dtype == dtype and t.is_contiguous() else t.to(dtype).contiguous()


# the raw handle of torch's current stream / the current device index: torch.cuda.current_stream() builds a Stream object (~5 us a call);
# the public calls are the fallback where a torch build lacks the two private ones
_cur_dev = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _stream():
    return _raw_stream(_cur_dev())


def _mat(dst, src, rows, cols):
    """Copies the top-left rows x cols block of a (host or device) matrix into a ctypes float array."""
    m = torch.as_tensor(src, dtype=torch.float32).detach().cpu()
    for r in range(rows):
        for c in range(cols):
            dst[r * cols + c] = float(m[r, c])


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(device):
    """Context that makes `device` current for the library call inside: nothing at all when it already is (one process per GPU)."""
    idx = device.index
    return _NO_SWITCH if idx is None or idx == _cur_dev() else torch.cuda.device(device)


def _launch(name, params, device):
    with _on(device):                                     # (no switch, no context manager when the device is current: one process per GPU)
        L.call(name, params, _stream())


class Event:
    """HIP timing event created by the library (usable with any stream the kernels run on)."""

    def __init__(self):
        self.h = L.lib().ucnerf_event_create()
        if not self.h:
            raise RuntimeError("uc_nerf_amd: event_create failed")

    def record(self):
        L.check(L.lib().ucnerf_event_record(self.h, _stream()), "ucnerf_event_record")

    def elapsed_ms(self, stop):
        ms = C.c_float(0)
        L.check(L.lib().ucnerf_event_elapsed_ms(self.h, stop.h, C.addressof(ms)), "ucnerf_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            L.lib().ucnerf_event_destroy(self.h)
        except Exception:
            pass
