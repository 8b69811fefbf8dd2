"""Which kernel the rasterizer backward runs (reduce_by_face in csrc/raster.hip) and how a test steers it: k_bwd_runs needs D = 4 and
16-byte-aligned features and gradients, everything else goes to k_bwd_sorted.  A D = 4 feature tensor 4 bytes off such a boundary (a
slice of a larger tensor, in a user's hands) therefore takes k_bwd_sorted, and the library's own per-kernel launch counters
(deftet_profile_select / deftet_profile_read) say that it did."""
import ctypes

import torch

KERNELS = (b"k_bwd_runs", b"k_bwd_sorted")


def off_by_four_bytes(t):
    """a contiguous copy of the fp32 tensor `t` whose storage starts 4 bytes past a 16-byte boundary"""
    assert t.dtype == torch.float32
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert flat.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def launches(kernel, fn):
    """fn() with the launches of `kernel` counted -> (what fn returned, the count); the counter is off again afterwards"""
    from deftet_amd import _lib
    lib = _lib.load()
    ms, count = ctypes.c_double(0), ctypes.c_longlong(0)
    lib.deftet_profile_select(kernel)
    try:
        out = fn()
        torch.cuda.synchronize()
        lib.deftet_profile_read(ctypes.byref(ms), ctypes.byref(count))
    finally:
        lib.deftet_profile_select(b"")
    return out, count.value


def ran_only(kernel, fn):
    """fn() twice, once per counter (one kernel is counted at a time): `kernel` was launched, the other one was not.
    -> what the first fn() returned"""
    assert kernel in KERNELS
    other = KERNELS[1 - KERNELS.index(kernel)]
    out, n = launches(kernel, fn)
    _, n_other = launches(other, fn)
    assert n > 0 and n_other == 0, "%s launched %d times, %s %d times" % (kernel.decode(), n, other.decode(), n_other)
    return out
