"""hgym: thin Python layer over libhgym_hip.so (ctypes).  Importing it requires the built HIP library."""
from . import _lib
from ._lib import lib, check, HgymError
from .env_buffers import EnvBuffers, default_env_config, log_stats_summary
from .net import NetBuffers, make_net_config, make_ppo_config, make_batch, activation_spec, diag_from_block, DIAG_KEYS, opt_summary
from .net import check_obs_norm, norm_layout


def mirror_rows(src, dst, src_col, sign, zero_to=None):
    """hgym_mirror_rows on the current stream: dst[m, c] = src[m, src_col[c]] with the sign bit inverted where sign[c] < 0, for
    c < width = src_col.numel(); dst[m, width:zero_to] = +0 (zero_to=None: no pad columns).  src, dst: (M, >= width) float32 or
    bfloat16 device tensors of one dtype whose rows are contiguous (stride(1) == 1; the row stride is the leading dimension).
    src_col int32 (width,), sign float32 (width,): device tensors; their contents are the caller's business (MirrorSpec validates)."""
    import ctypes as C
    import torch
    assert src.dim() == 2 and dst.dim() == 2 and src.shape[0] == dst.shape[0] and src.dtype == dst.dtype
    assert src.dtype in (torch.float32, torch.bfloat16) and src.is_cuda and dst.is_cuda
    assert src_col.dtype == torch.int32 and sign.dtype == torch.float32 and src_col.is_cuda and sign.is_cuda
    assert src_col.is_contiguous() and sign.is_contiguous() and src_col.numel() == sign.numel()
    width, M = int(src_col.numel()), int(src.shape[0])
    ld = lambda t: max(int(t.stride(0)), int(t.shape[1]))      # (a one-row tensor may carry any row stride)
    assert (src.shape[1] == 1 or src.stride(1) == 1) and (dst.shape[1] == 1 or dst.stride(1) == 1)
    check(lib.hgym_mirror_rows(M, width, C.cast(src_col.data_ptr(), C.POINTER(C.c_int32)), _lib.fptr(sign), C.c_void_p(src.data_ptr()), ld(src),
                               C.c_void_p(dst.data_ptr()), ld(dst), width if zero_to is None else int(zero_to),
                               _lib.F32 if src.dtype == torch.float32 else _lib.BF16, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "hgym_mirror_rows")
