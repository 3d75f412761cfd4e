"""hgym: thin Python layer over libhgym_hip.so (ctypes).  Importing it requires the built HIP library."""
from . import _lib
from ._lib import lib, check, HgymError
from .env_buffers import EnvBuffers, default_env_config, log_stats_summary
from .net import NetBuffers, make_net_config, make_ppo_config, make_batch, activation_spec, diag_from_block, DIAG_KEYS, opt_summary
from .net import check_obs_norm, norm_layout
from .net import make_bc_config, make_bc_batch, BC_LOSS_TYPES
from .net import make_vf_config, make_vf_batch
from .net import make_smooth, smooth_ld, smooth_mirror_partials
from .net import make_guide, make_guide_schedule, guide_schedule, guide_schedule_coef, GUIDE_MODES


def smooth_pairs(idx, dones, N, next_idx, next_weight):
    """hgym_smooth_pairs on the current stream: next_idx[b] = idx[b] + N, next_weight[b] = 0 where dones[idx[b]] else 1.  idx, next_idx int64
    (B,), next_weight float32 (B,), dones uint8 / bool over the stored rows (flat); contiguous device tensors."""
    import ctypes as C
    import torch
    assert idx.dtype == torch.int64 and next_idx.dtype == torch.int64 and next_weight.dtype == torch.float32
    assert dones.dtype in (torch.uint8, torch.bool) and dones.is_contiguous()
    assert idx.is_contiguous() and next_idx.is_contiguous() and next_weight.is_contiguous()
    assert next_idx.numel() >= idx.numel() and next_weight.numel() >= idx.numel()
    check(lib.hgym_smooth_pairs(int(idx.numel()), int(N), _lib.i64ptr(idx), _lib.u8ptr(dones), _lib.i64ptr(next_idx), _lib.fptr(next_weight),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_smooth_pairs")


def perturb_rows(src, noise_std, seed, opt_state, dst, idx=None):
    """hgym_perturb_rows on the current stream: dst[m, c] = src[row, c] + noise_std[c] * z, row = idx[m] (idx=None: m), z the Philox normal
    of (seed, step = opt_state[OPT_STEP], row, slot 128 + c // 4).  src (rows, width) float32 with contiguous rows; dst (M, ld) float32,
    ld = its row stride, a multiple of 4 and >= smooth_ld(width), 16-byte aligned; noise_std float32 (width,); opt_state float64 (16,)."""
    import ctypes as C
    import torch
    assert src.dim() == 2 and dst.dim() == 2 and src.dtype == torch.float32 and dst.dtype == torch.float32
    assert (src.shape[1] == 1 or src.stride(1) == 1) and (dst.shape[1] == 1 or dst.stride(1) == 1)
    width = int(src.shape[1])
    assert noise_std.dtype == torch.float32 and noise_std.is_contiguous() and noise_std.numel() == width
    assert opt_state.dtype == torch.float64 and opt_state.is_contiguous() and opt_state.numel() >= _lib.OPT_STATE
    assert idx is None or (idx.dtype == torch.int64 and idx.is_contiguous())
    M = int(dst.shape[0]) if idx is None else int(idx.numel())
    assert dst.shape[0] >= M and (idx is not None or src.shape[0] >= M)
    ld = lambda t: max(int(t.stride(0)), int(t.shape[1]))
    check(lib.hgym_perturb_rows(M, width, _lib.fptr(src), ld(src), _lib.i64ptr(idx), _lib.fptr(noise_std), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                _lib.f64ptr(opt_state), _lib.fptr(dst), ld(dst), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "hgym_perturb_rows")


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


def _value_norm_args(x, block, eps=None):
    import torch
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous()
    assert block.dtype == torch.float64 and block.is_cuda and block.is_contiguous() and block.numel() >= _lib.VALUE_NORM_BLOCK_DOUBLES
    return None if eps is None else float(eps)


def value_denormalize(src, block, eps, out=None):
    """hgym_value_denormalize on the current stream: out[i] = src[i] * scale_f + mean_f, mean_f = (float)block[1], scale_f =
    (float)sqrt(block[2]) + eps.  src, out float32 contiguous device tensors of one size (out=None: in place); block: _lib.value_norm_block.
    -> out."""
    import ctypes as C
    import torch
    out = src if out is None else out
    eps = _value_norm_args(src, block, eps)
    _value_norm_args(out, block)
    assert out.numel() == src.numel()
    check(lib.hgym_value_denormalize(int(src.numel()), _lib.fptr(src), _lib.fptr(out), _lib.f64ptr(block), eps,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_value_denormalize")
    return out


def value_norm_merge(returns, block, scratch):
    """hgym_value_norm_merge on the current stream: the fp64 statistics of the float32 values `returns` (fixed order: the same bits in every
    run) -> scratch[0:3] = n, mean, population variance, merged into block = (count, mean, var).  scratch:
    _lib.value_norm_scratch(returns.numel(), device), zero-filled once, reusable from call to call."""
    import ctypes as C
    import torch
    _value_norm_args(returns, block)
    assert scratch.dtype == torch.float64 and scratch.is_cuda and scratch.is_contiguous()
    assert scratch.numel() >= _lib.value_norm_scratch_doubles(returns.numel())
    check(lib.hgym_value_norm_merge(int(returns.numel()), _lib.fptr(returns), _lib.f64ptr(block), _lib.f64ptr(scratch),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_value_norm_merge")


def value_normalize(x, block, eps):
    """hgym_value_normalize on the current stream: x[i] = (x[i] - mean_f) / scale_f in place (the floats as value_denormalize forms them).
    -> x."""
    import ctypes as C
    import torch
    eps = _value_norm_args(x, block, eps)
    check(lib.hgym_value_normalize(int(x.numel()), _lib.fptr(x), _lib.f64ptr(block), eps, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "hgym_value_normalize")
    return x
