"""hgym: thin Python layer over libhgym_hip.so (ctypes).  Importing it requires the built HIP library."""
from . import _lib
from ._lib import lib, check, HgymError
from .env_buffers import EnvBuffers, default_env_config, log_stats_summary
from .net import NetBuffers, make_net_config, make_ppo_config, make_batch, activation_spec, diag_from_block, DIAG_KEYS, opt_summary
from .net import check_obs_norm, norm_layout
from .net import make_bc_config, make_bc_batch, BC_LOSS_TYPES


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


def adv_normalize_minibatches(idx, adv, out, segments, scratch):
    """hgym_adv_normalize_minibatches on the current stream: idx int64 (segments * seg_len,) distinct rows of the columns adv / out (float32,
    contiguous, the same number of rows, not overlapping); segment s = idx[s * seg_len:(s + 1) * seg_len] ->
    out[idx[j]] = (adv[idx[j]] - mean_s) / (std_s + 1e-8), the segment's own mean and unbiased deviation.  Rows of `out` that idx does not
    name are left alone.  scratch: _lib.adv_mb_scratch(segments, seg_len, device), zero-filled once, reusable from call to call."""
    import ctypes as C
    import torch
    segments = int(segments)
    assert idx.dtype == torch.int64 and idx.is_cuda and idx.is_contiguous() and idx.dim() == 1
    assert segments >= 1 and idx.numel() % segments == 0
    seg_len = idx.numel() // segments
    for t in (adv, out):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    assert adv.numel() == out.numel()
    assert scratch.dtype == torch.float64 and scratch.is_cuda and scratch.is_contiguous()
    assert scratch.numel() >= _lib.adv_mb_scratch_doubles(segments, seg_len)
    check(lib.hgym_adv_normalize_minibatches(segments, seg_len, _lib.i64ptr(idx), _lib.fptr(adv), _lib.fptr(out), int(adv.numel()),
                                             _lib.f64ptr(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "hgym_adv_normalize_minibatches")
