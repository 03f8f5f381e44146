"""Drop-in for the reference's native extension module ``MultiScaleDeformableAttention``.

The reference imports it as ``import MultiScaleDeformableAttention as MSDA`` in
  mm_interleaved/models/utils/ops/functions/ms_deform_attn_func.py:18-21
  mm_interleaved/models/encoders/vit_adapter/ops/functions/ms_deform_attn_func.py:19-22
and calls exactly two functions, exported by its pybind module
(mm_interleaved/models/utils/ops/src/vision.cpp:13-16):

    ms_deform_attn_forward(value, spatial_shapes, level_start_index,
                           sampling_loc, attn_weight, im2col_step) -> Tensor[B, Nq, H*D]
    ms_deform_attn_backward(value, spatial_shapes, level_start_index,
                            sampling_loc, attn_weight, grad_output, im2col_step)
        -> [grad_value, grad_sampling_loc, grad_attn_weight]

Putting this directory on ``sys.path`` makes that import resolve here; the two
functions keep the reference's argument order, preconditions and error
behaviour (ms_deform_attn_cuda.cu:29-53, 94-118) and run the hand-written gfx950
kernels of ``libmmfs_msda.so`` through its C ABI (include/mmfs_msda.h) with ctypes.

There is NO CPU or PyTorch fallback: CPU tensors raise, exactly as the reference
does (src/ms_deform_attn.h:29-38: "Not implemented on the CPU"), and a missing
shared library raises at import time.
"""
import collections
import ctypes
import os

import numpy as np
import torch

import mmfs_abi

__all__ = ["ms_deform_attn_forward", "ms_deform_attn_backward", "register_level_tables", "library_path",
           "build_info", "check_level_table_status", "value_row_map", "quantize_bank_fp8", "quantize_bank_fp8_reference",
           "dequantize_bank_fp8", "FP8_BANK_DTYPE"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("MMFS_MSDA_LIB", os.path.join(_HERE, "libmmfs_msda.so"))

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"MultiScaleDeformableAttention: {_LIB_PATH} not found. Build it with "
        f"`make -C {os.path.join(_HERE, 'csrc')}` (hipcc, gfx950); there is no fallback path.")

_lib = ctypes.CDLL(_LIB_PATH)

_ABI_VERSION = 14
if _lib.mmfs_msda_abi_version() != _ABI_VERSION:
    raise ImportError(f"{_LIB_PATH}: ABI version {_lib.mmfs_msda_abi_version()} != {_ABI_VERSION}")
mmfs_abi.bind(_lib)                 # the signature of every entry point of include/mmfs_msda.h, from the one table

# enum mmfs_dtype (include/mmfs_msda.h); _FLOAT_CODE: without fp64, what every entry point besides the op itself takes
_DTYPE_CODE, _FLOAT_CODE = mmfs_abi.DTYPE_CODE, mmfs_abi.FLOAT_CODE


def library_path():
    return _LIB_PATH


def reload_env():
    """The library reads its ``MMFS_*`` tuning / test knobs ONCE (csrc/msda_env.h); a process that changes one afterwards
    (the tests do, to hold every formulation to the oracle) says so here.  Also drops what this module derived from them."""
    _lib.mmfs_env_reload()
    _ws_cache.clear()


def env_knobs():
    """[(name, documentation, value or None)] -- the library's whole table of environment knobs."""
    out, i = [], 0
    name, doc, val = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_char_p()
    while _lib.mmfs_env_knob(i, ctypes.byref(name), ctypes.byref(doc), ctypes.byref(val)) == 0:
        out.append((name.value.decode(), doc.value.decode(), None if val.value is None else val.value.decode()))
        i += 1
    return out


def build_info():
    return _lib.mmfs_msda_build_info().decode()


def _check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: {_lib.mmfs_msda_status_string(status).decode()} (status {status})")


def _require(cond, msg):
    # AT_ASSERTM in the reference raises a RuntimeError
    if not cond:
        raise RuntimeError(msg)


def _check_step(B, im2col_step):
    # the reference walks the batch im2col_step rows at a time (.cu:51-53); the kernels here take it whole
    step = min(B, int(im2col_step)) if B > 0 else 1
    _require(step > 0 and B % step == 0, f"batch({B}) must divide im2col_step({step})")


def _validate(named, value):
    # (messages are only built when a check fails: this runs on every call of a ~100 us step)
    dev = value.device
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} tensor has to be contiguous")
        # PyTorch-ROCm exposes HIP devices under the "cuda" device type
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")   # reference wording, .cu:35-39
        if t.device != dev:
            raise RuntimeError(f"{name} must be on the same device as value")


def _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    if value.dim() != 4:
        raise RuntimeError("value must be [B, S, H, D]")
    B, S, H, D = value.shape
    if spatial_shapes.dim() != 2 or spatial_shapes.shape[1] != 2:
        raise RuntimeError("spatial_shapes must be [L, 2]")
    L = spatial_shapes.shape[0]
    if sampling_loc.dim() != 6:
        raise RuntimeError("sampling_loc must be [B, Nq, H, L, P, 2]")
    Nq, P = sampling_loc.shape[1], sampling_loc.shape[4]
    if sampling_loc.shape != (B, Nq, H, L, P, 2):
        raise RuntimeError(f"sampling_loc shape {tuple(sampling_loc.shape)} != {(B, Nq, H, L, P, 2)}")
    if attn_weight.shape != (B, Nq, H, L, P):
        raise RuntimeError(f"attn_weight shape {tuple(attn_weight.shape)} != {(B, Nq, H, L, P)}")
    if level_start_index.numel() != L:
        raise RuntimeError("level_start_index must have one entry per level")
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("spatial_shapes and level_start_index must be int64 (reference reads data<int64_t>)")
    return B, S, H, D, L, Nq, P


# How a bank of batch Bv serves a query batch B = g * Bv (include/mmfs_msda.h, MMFS_BANK_*): query row b reads bank row
# (b / div) % Bv, div = 1 for "tile" (the order of torch.cat([bank] * g): classifier-free guidance) and g for "interleave"
# (the order of bank.repeat_interleave(g, 0): beam search).
_VALUE_REPEAT = {"tile": 0, "interleave": 1}


def value_row_map(B, Bv, value_repeat):
    """The bank row each of the B query rows reads (a list of ints): what the kernels compute, on the host."""
    _require(value_repeat in _VALUE_REPEAT, f"value_repeat must be None, 'tile' or 'interleave', not {value_repeat!r}")
    _require(Bv > 0 and B % Bv == 0, f"value_repeat={value_repeat!r}: the bank's batch ({Bv}) must divide the query batch ({B})")
    div = 1 if value_repeat == "tile" else B // Bv
    return [(b // div) % Bv for b in range(B)]


def _dims_shared(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, value_repeat):
    """``_dims`` for a bank of batch Bv = value.shape[0] shared by the B = sampling_loc.shape[0] query rows:
    (B, S, H, D, L, Nq, P, Bv)."""
    _require(value_repeat in _VALUE_REPEAT, f"value_repeat must be None, 'tile' or 'interleave', not {value_repeat!r}")
    if value.dim() != 4 or sampling_loc.dim() != 6:
        return _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight) + (value.shape[0],)
    Bv, B = value.shape[0], sampling_loc.shape[0]
    _require(Bv > 0 and B % Bv == 0, f"value_repeat={value_repeat!r}: the bank's batch ({Bv}) must divide the query batch ({B})")
    # (the other checks against the expanded bank's shape, on a tensor without storage)
    shape_only = torch.empty((B,) + tuple(value.shape[1:]), device="meta")
    return _dims(shape_only, spatial_shapes, level_start_index, sampling_loc, attn_weight) + (Bv,)


def _expand_bank(value, B, value_repeat):
    """The bank as ``g`` explicit copies in the query order: what a shared call is defined against."""
    g = B // value.shape[0]
    return value.repeat(g, *([1] * (value.dim() - 1))) if value_repeat == "tile" else value.repeat_interleave(g, 0)


def _same_dtype(value, sampling_loc, attn_weight):
    """The reference reads all three through one scalar_t (.cu:67-73).  softmax under
    autocast may hand an fp32 attn_weight next to fp16 values; cast instead of reading
    garbage (SURVEY.md section 8a "Dtype flow")."""
    _require(value.dtype in _DTYPE_CODE, f"unsupported dtype {value.dtype}")
    if sampling_loc.dtype != value.dtype:
        sampling_loc = sampling_loc.to(value.dtype)
    if attn_weight.dtype != value.dtype:
        attn_weight = attn_weight.to(value.dtype)
    return sampling_loc, attn_weight


def _aligned(t, nbytes=16):
    return t if t.data_ptr() % nbytes == 0 else t.clone(memory_format=torch.contiguous_format)


def _plain(t):
    """a tensor as the attention entries take it: detached, contiguous, aligned to 16 bytes"""
    t = t.detach()
    return _aligned(t if t.is_contiguous() else t.contiguous())


# ---- what the attention functions (functions/*attn*_func.py, llama_train_func.py) check and allocate alike

def _attn_supported(q, heads, probe, *more):
    """a device tensor q [B, L, H D] of bf16 or fp16, outside autocast, that the library's ``probe`` (dtype, D, L, *more) takes"""
    if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dim() == 3) or torch.is_autocast_enabled():
        return False
    if q.dtype not in (torch.float16, torch.bfloat16) or heads < 1 or q.shape[2] % heads:
        return False
    return bool(getattr(_lib, probe)(_DTYPE_CODE[q.dtype], q.shape[2] // heads, q.shape[1], *more))


def _require_qkv(what, q, k, v, heads, head_dim):
    """q, k, v [B, L, H head_dim] of one half type, shape and device, outside autocast; else a RuntimeError that names ``what``"""
    _require(all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3 for t in (q, k, v)) and
             q.dtype in (torch.float16, torch.bfloat16), f"{what}: q, k, v must be device tensors [B, L, H {head_dim}] of bf16 or fp16")
    _require(k.shape == q.shape and v.shape == q.shape and k.dtype == q.dtype and v.dtype == q.dtype and
             k.device == q.device and v.device == q.device, f"{what}: k and v must have q's shape, type and device")
    _require(heads >= 1 and q.shape[2] == heads * head_dim, f"{what}: {q.shape[2]} channels are not {heads} heads of {head_dim}")
    _require(not torch.is_autocast_enabled(), f"{what}: not under autocast")


def _tiles(entry, n):
    """how a kernel family cuts its work, where its paths change: ``entry``(0 .. n - 1)"""
    return tuple(int(getattr(_lib, entry)(i)) for i in range(n))


def _float_workspace(entry, device, *dims):
    """the fp32 workspace that ``entry``(*dims) sizes in bytes (the caching allocator's, like the outputs: no device
    allocation in a steady loop)"""
    return torch.empty(max(getattr(_lib, entry)(*dims) // 4, 4), dtype=torch.float32, device=device)


def _stream(device):
    return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())


class _on_device:
    """torch.cuda.device(dev) without the context-manager cost when dev is already current."""
    __slots__ = ("ctx",)

    def __init__(self, device):
        idx = device.index
        self.ctx = None if idx is None or idx == torch.cuda.current_device() else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


# host-only size queries of the library, memoised (they depend on the numbers only; the level table enters
# through the identity + version of its host copy)
_ws_cache = {}


def _memo(key, ask):
    n = _ws_cache.get(key)
    if n is None:
        if len(_ws_cache) > 4096:
            _ws_cache.clear()
        n = _ws_cache[key] = ask()
    return n


# bench.py sets this to a list to time individual kernels with HIP events recorded on
# the very stream the kernel is launched on: entries are (kernel_name, start, end).
_event_log = None


def _launch(name, device, fn, *args):
    if _event_log is None:
        return fn(*args)
    st = torch.cuda.current_stream(device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(st)
    status = fn(*args)
    t1.record(st)
    _event_log.append((name, t0, t1))
    return status


def _call(log_name, entry, device, *args, refuse_ok=False, what=None):
    """One launch through the C ABI: ``_lib``'s ``entry`` (looked up now, by name) with ``args`` and the current stream of
    ``device`` behind them, on that device, logged as ``log_name``.  A status other than 0 raises, named ``what``
    (default: the entry point) -- except, with ``refuse_ok``, MMFS_E_UNSUPPORTED, which is returned: the caller then
    takes its documented other path."""
    with _on_device(device):
        status = _launch(log_name, device, getattr(_lib, entry), *args, _stream(device))
    if status != 0 and not (refuse_ok and status == _E_UNSUPPORTED):
        _check(status, what or entry)
    return status


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- level tables the shim has never seen are checked ON THE DEVICE by the backward (no device->host copy per
# call).  A table the sorted backward cannot serve (overlapping / out-of-range / >= 65536-wide levels) gets the
# reference's float-atomic scatter IN THE SAME CALL (csrc/msda_bwd_refused.hip: three launches that read the plan's
# verdict on the device and return at once for every ordinary table), so grad_value is what the reference computes
# either way.  The plan also reports such a table through this word -- one int32 of pinned, device-visible host
# memory per device -- and the next call into the shim (or check_level_table_status()) turns it into ONE warning:
# the fallback is slow, and a caller that builds such tables should register them.  No device trap, no exception.
_status_words = {}
_BAD_TABLE_MSG = ("ms_deform_attn_backward: an earlier call on this device was handed a level table with overlapping, "
                  "out-of-range or >= 65536-wide levels that the shim had never seen; its grad_value came from the "
                  "float-atomic fallback (correct, as the reference computes it, but slow).  Register such tables "
                  "(MultiScaleDeformableAttention.register_level_tables): they then take the float-atomic path directly")
_bad_table_warned = False


def _status_word(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    w = _status_words.get(idx)
    if w is None:
        t = torch.zeros(1, dtype=torch.int32).pin_memory()
        w = _status_words[idx] = (t, t.numpy())
    return w


def check_level_table_status(device=None, synchronize=False):
    """True (and, once per process, a RuntimeWarning) if a backward on ``device`` (default: every device used so far)
    met a level table the device-side check refused since the last time this was asked; the flag is consumed.
    ``synchronize=True`` waits for the device first (a test's use; the op itself only looks at what has already
    arrived).  The gradients of such a call are correct: it took the float-atomic fallback."""
    global _bad_table_warned
    if synchronize:
        torch.cuda.synchronize(device)
    words = _status_words.values() if device is None else [_status_word(torch.device(device))]
    seen = False
    for _, flag in words:
        if flag[0]:
            flag[0] = 0
            seen = True
    if seen and not _bad_table_warned:
        _bad_table_warned = True
        import warnings
        warnings.warn(_BAD_TABLE_MSG, RuntimeWarning, stacklevel=2)
    return seen


# ---- the inference-only fp8 value bank (include/mmfs_msda.h "fp8 bank"): q [Bv, S, H, D] OCP e4m3
# (torch.float8_e4m3fn -- not the fnuz format) with one fp32 scale per (bank row, channel), scale [Bv, H*D]; element
# (b, s, h, d) stands for float(q) * scale[b, h*D + d].
FP8_BANK_DTYPE = torch.float8_e4m3fn
_FP8_MAX = 448.0
_FP8_NAN = 0x7f


def _bank_dims(x):
    _require(x.dim() in (4, 5), f"a bank is [Bv, S, H, D] or a batch of banks [K, Bv, S, H, D], not {tuple(x.shape)}")
    S, H, D = x.shape[-3:]
    return tuple(x.shape[:-3]), int(S), int(H) * int(D)


def quantize_bank_fp8_reference(x):
    """The quantiser's rule as torch operations (the CPU path, and what the kernel is tested against bit for bit):
    x [Bv, S, H, D] (or [K, Bv, S, H, D]) -> (q e4m3 of x's shape, scale fp32 [Bv, H*D] (or [K, Bv, H*D])).
        amax = max |x| over the FINITE elements of a (bank row, channel) column;  scale = amax / 448 (fp32 division);
        q = e4m3(RNE(clamp(x / scale, -448, 448)));  scale == 0 -> +0;  a non-finite x -> the NaN code 0x7f, unclamped."""
    lead, S, C = _bank_dims(x)
    xr = x.float().reshape(*lead, S, C)
    finite = torch.isfinite(xr)
    if S > 0:
        amax = torch.where(finite, xr.abs(), torch.zeros((), device=xr.device)).amax(dim=-2)
    else:
        amax = torch.zeros(*lead, C, device=xr.device)
    scale = amax / _FP8_MAX
    s = scale.unsqueeze(-2)
    y = torch.where(s != 0, (xr / torch.where(s != 0, s, torch.ones((), device=xr.device))).clamp(-_FP8_MAX, _FP8_MAX),
                    torch.zeros((), device=xr.device))
    qb = y.to(FP8_BANK_DTYPE).view(torch.uint8)
    qb = torch.where(finite, qb, torch.full((), _FP8_NAN, dtype=torch.uint8, device=xr.device))
    return qb.view(FP8_BANK_DTYPE).reshape(x.shape), scale.contiguous()


def quantize_bank_fp8(x):
    """x [Bv, S, H, D] or a batch of K banks [K, Bv, S, H, D] (f32 / f16 / bf16) -> (q, scale) by the rule of
    ``quantize_bank_fp8_reference``: on the GPU the kernel (csrc/mmfs_bank_fp8.hip, every bank in one call, bit-identical
    to the rule), on the CPU the rule itself.  Inference only: nothing here is differentiable."""
    lead, S, C = _bank_dims(x)
    if not x.is_cuda:
        return quantize_bank_fp8_reference(x)
    _require(x.dtype in (torch.float32, torch.float16, torch.bfloat16), f"quantize_bank_fp8: unsupported dtype {x.dtype}")
    x = _aligned(x.contiguous())
    q = torch.empty(x.shape, dtype=FP8_BANK_DTYPE, device=x.device)
    scale = torch.empty(*lead, C, dtype=torch.float32, device=x.device)
    K = lead[0] if len(lead) == 2 else 1
    Bv = lead[-1]
    if _call("bank_quantize_fp8", "mmfs_bank_quantize_fp8", x.device, _DTYPE_CODE[x.dtype], x.data_ptr(), K, Bv, S, C,
             q.data_ptr(), scale.data_ptr(), refuse_ok=True, what="quantize_bank_fp8"):
        return quantize_bank_fp8_reference(x)        # (H*D not a multiple of 16: the rule, on the device)
    return q, scale


def dequantize_bank_fp8(q, scale, dtype=torch.float32):
    """float(q) * scale as ``dtype`` -- the bank an fp8 bank stands for."""
    lead, S, C = _bank_dims(q)
    return (q.float().reshape(*lead, S, C) * scale.float().unsqueeze(-2)).to(dtype).reshape(q.shape)


def _forward_fp8(value, value_scale, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step,
                 value_repeat):
    """ms_deform_attn_forward on an fp8 bank: the output has attn_weight's type."""
    _validate([("value_scale", value_scale)], value)
    if value_repeat is None:
        B, S, H, D, L, Nq, P = _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
        Bv, layout = B, _VALUE_REPEAT["tile"]
    else:
        B, S, H, D, L, Nq, P, Bv = _dims_shared(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                                value_repeat)
        layout = _VALUE_REPEAT[value_repeat]
    _check_step(B, im2col_step)
    dt = attn_weight.dtype
    _require(dt in (torch.float32, torch.float16, torch.bfloat16), f"fp8 bank: unsupported output dtype {dt}")
    _require(value_scale.dtype == torch.float32 and tuple(value_scale.shape) == (value.shape[0], H * D),
             f"value_scale must be fp32 [{value.shape[0]}, {H * D}], not {value_scale.dtype} {tuple(value_scale.shape)}")
    if sampling_loc.dtype != dt:
        sampling_loc = sampling_loc.to(dt)
    value, value_scale = _aligned(value), _aligned(value_scale)
    out = torch.empty((B, Nq, H * D), dtype=dt, device=value.device)
    if _call("msda_fwd", "mmfs_msda_forward_fp8", value.device, _DTYPE_CODE[dt], value.data_ptr(), value_scale.data_ptr(),
             spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(),
             out.data_ptr(), B, Bv, layout, S, H, D, L, Nq, P, refuse_ok=True, what="ms_deform_attn_forward"):
        # a head width the fp8 kernels do not serve (D not 16 * 2^k, k <= 4): the documented slow path -- the bank
        # dequantised to the output type, then the ordinary forward
        return ms_deform_attn_forward(dequantize_bank_fp8(value, value_scale, dt), spatial_shapes, level_start_index,
                                      sampling_loc, attn_weight, im2col_step, value_repeat=value_repeat)
    return out


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                           im2col_step, *, value_repeat=None, value_scale=None):
    """Reference: ms_deform_attn_cuda_forward, src/cuda/ms_deform_attn_cuda.cu:21-81.
    ``value_repeat`` (an addition): None, or "tile" / "interleave" when ``value`` [Bv, S, H, D] is a bank shared by the
    B = g * Bv query rows of ``sampling_loc`` -- query row b reads bank row b % Bv ("tile", the order of
    ``torch.cat([value] * g)``) or b // g ("interleave", of ``value.repeat_interleave(g, 0)``).  The result is the op on
    the expanded bank, bit for bit; the copy is never made (mmfs_msda_forward_shared).
    ``value_scale`` (an addition too): with ``value`` an fp8 bank (``FP8_BANK_DTYPE``, from ``quantize_bank_fp8``), its fp32
    scales [Bv, H*D]; the output then has ``attn_weight``'s type (mmfs_msda_forward_fp8).  Forward only."""
    _require(isinstance(value, torch.Tensor) and value.is_cuda, "Not implemented on the CPU")
    if _status_words:
        check_level_table_status()
    _validate([("value", value), ("spatial_shapes", spatial_shapes),
               ("level_start_index", level_start_index), ("sampling_loc", sampling_loc),
               ("attn_weight", attn_weight)], value)
    if value.dtype == FP8_BANK_DTYPE or value_scale is not None:
        _require(value.dtype == FP8_BANK_DTYPE and value_scale is not None,
                 "an fp8 bank (torch.float8_e4m3fn) comes with its value_scale, and value_scale with an fp8 bank")
        return _forward_fp8(value, value_scale, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step,
                            value_repeat)
    if value_repeat is None:
        B, S, H, D, L, Nq, P = _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    else:
        B, S, H, D, L, Nq, P, Bv = _dims_shared(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                                value_repeat)
    _check_step(B, im2col_step)
    sampling_loc, attn_weight = _same_dtype(value, sampling_loc, attn_weight)
    value = _aligned(value)
    out = torch.empty((B, Nq, H * D), dtype=value.dtype, device=value.device)
    if value_repeat is None:
        entry, bank = "mmfs_msda_forward_flags", ()
    else:
        entry, bank = "mmfs_msda_forward_shared", (Bv, _VALUE_REPEAT[value_repeat])
    name, algo = "msda_fwd", _fwd_algo
    if algo in ("lds", "slices", "waves") and S * H * D * value.element_size() > _MAX_SLAB_BYTES:
        # none of the kernels that can be asked for by name takes a (b) slab its 32-bit row offsets cannot span
        # (csrc/msda_device.h, kMaxSlabBytes): the row gather's flat-address kernel serves the call, as it does under
        # "auto" and as the backward does for its named LDS-levels kernel -- decided here, on the size alone, whatever
        # else the named kernel would have refused.  Under the limit a named kernel's refusal raises, as before.
        name, algo = "msda_fwd_gather", "gather"
    _call(name, entry, value.device, _DTYPE_CODE[value.dtype], value.data_ptr(), spatial_shapes.data_ptr(),
          level_start_index.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(), out.data_ptr(), B, *bank,
          S, H, D, L, Nq, P, _FWD_FLAGS[algo], what="ms_deform_attn_forward")
    return out


# tests / measurements: which formulation of the forward runs (include/mmfs_msda.h, mmfs_msda_forward_flags):
# "auto" | "gather" (csrc/msda_fwd.hip) | "lds" (csrc/msda_fwd_mma.hip; unsupported shapes raise -- but a value slab of
# 2 GiB or more, which none of the named kernels takes, goes to the row gather: logged as "msda_fwd_gather")
_fwd_algo = "auto"
_MAX_SLAB_BYTES = 0x7fffffff      # kMaxSlabBytes of csrc/msda_device.h: what a buffer descriptor's 32-bit byte offsets span
_FWD_FLAGS = {"auto": 0, "gather": 1, "lds": 2, "slices": 4, "waves": 8}        # "slices": csrc/msda_fwd_q8.hip; "waves": msda_fwd_wq.hip


# flags of mmfs_msda_backward (include/mmfs_msda.h)
_BWD_CANONICAL_LEVELS = 1
_BWD_FORCE_ATOMIC = 2
_BWD_DENSE_TAPS = 4
_BWD_LAZY_ZERO_ATTN = 16
_BWD_DEVICE_CHECKED_LEVELS = 32
_BWD_TAPS_ROW_GATHER = 64
_BWD_TAPS_LDS_LEVELS = 128
_E_UNSUPPORTED = -5

# tests / measurements: which formulation computes grad_loc / grad_attn (include/mmfs_msda.h):
# "auto" | "gather" (csrc/msda_bwd.hip + msda_dense.hip) | "lds" (csrc/msda_taps_mma.hip; unsupported shapes raise) |
# "sorted" (csrc/msda_bwd_taps_sorted.hip: from the grad_value sort's records -- parity-green, measured slower than the gather
# kernels on every shipped geometry, DESIGN.md 4.2c: opt-in; arguments mmfs_msda_backward_sorted does not take raise).
# MMFS_TAPS_ROUTE=sorted in the environment takes it wherever it applies, for a whole process (measurements).
_taps_algo = "auto"
_taps_prefer_sorted = os.environ.get("MMFS_TAPS_ROUTE") == "sorted"      # wherever it applies, silently not elsewhere
route_counts = {"sorted": 0}                  # backward calls that took mmfs_msda_backward_sorted (tests: "the route ran")
_TAPS_FLAGS = {"auto": 0, "gather": _BWD_TAPS_ROW_GATHER, "lds": _BWD_TAPS_LDS_LEVELS, "sorted": 0}

# tests / measurements: "auto" | "atomic" (force the float-atomic path)
_bwd_algo = "auto"
# tests / measurements: False keeps grad_loc / grad_attn of every level on the row-gather kernel
# (True: levels of at most min(256, 64*P) pixels take the matrix-core product, csrc/msda_dense.hip)
_hybrid = os.environ.get("MMFS_HYBRID", "1") != "0"

# stage bits of mmfs_msda_backward_sorted (include/mmfs_msda.h)
_SRT_BWD_STAGES = (("msda_bwd_value_prepare", 1), ("msda_bwd_value_sort", 2), ("msda_bwd_taps", 4), ("msda_bwd_value_reduce", 8))
_SRT_BWD_ALL = 15

# stage bits of mmfs_msda_backward_hybrid (include/mmfs_msda.h)
_HYB_BWD_STAGES = (("msda_bwd_taps", 1), ("msda_bwd_taps_coarse", 2), ("msda_bwd_value_prepare", 4),
                   ("msda_bwd_value_sort", 8), ("msda_bwd_value_reduce", 16))
_HYB_BWD_ALL = 31

# the library's own sequence on a canonical table, one entry point per kernel
_STAGED_BWD = (("msda_bwd_taps", "mmfs_msda_backward_taps"), ("msda_bwd_value_prepare", "mmfs_msda_backward_value_prepare"),
               ("msda_bwd_value_sort", "mmfs_msda_backward_value_sort"), ("msda_bwd_value_reduce", "mmfs_msda_backward_value_reduce"))
_LIBRARY_BWD = (("msda_bwd_atomic", "mmfs_msda_backward_checked"),)
# which of the backward's pointers -- value, shapes, start, loc, attn, grad_out, grad_value, grad_loc, grad_attn: 0 .. 8 -- each
# of the per-kernel entry points takes, and whether (workspace, workspace_bytes) follow them
_STAGED_ARGS = {"mmfs_msda_backward_taps": ((0, 1, 2, 3, 4, 5, 7, 8), False), "mmfs_msda_backward_value_prepare": ((3, 4), True),
                "mmfs_msda_backward_value_sort": ((1, 2), True), "mmfs_msda_backward_value_reduce": ((5, 6), True)}


def levels_are_canonical(spatial_shapes, level_start_index, S):
    """True when start[l] == sum_{k<l} H_k*W_k and sum_l H_l*W_l == S (the packing every
    caller in the reference builds: modeling_llama_mmfs.py:303-305, sd_mmfs.py:35-37).

    The tables live in device memory (reference API), so this query costs one small
    device->host copy the first time a pair of tensor objects is asked about; the answer is
    cached on the tensor object (keyed by the in-place version counters).  The op itself never
    asks: it uses the answer when it is there (``mmfs_amd.levels.make_level_tables`` pre-seeds
    it) and lets the library check the table on the device otherwise."""
    return _level_info(spatial_shapes, level_start_index, S)[0]


def _level_key(spatial_shapes, level_start_index, S):
    return (spatial_shapes._version, level_start_index._version, level_start_index.data_ptr(), int(S))


def _level_info(spatial_shapes, level_start_index, S, sync=True):
    """(canonical, host copy of spatial_shapes, host copy of level_start_index) -- the host
    copies are contiguous int64 numpy arrays (what the hybrid entry points take).  Cached on
    the spatial_shapes tensor object; with sync=False returns None instead of copying."""
    key = _level_key(spatial_shapes, level_start_index, S)
    cached = getattr(spatial_shapes, "_mmfs_canonical", None)
    if cached is not None and cached[0] == key:
        return cached[1:]
    if not sync:
        return None
    sh = spatial_shapes.detach().cpu().contiguous()
    st = level_start_index.detach().cpu().reshape(-1).contiguous()
    return _seed_level_info(spatial_shapes, key, sh, st, S)


def _seed_level_info(spatial_shapes, key, sh, st, S):
    px = sh[:, 0] * sh[:, 1]
    canon = bool((sh >= 0).all()) and bool((sh < 65536).all()) and \
        bool(torch.equal(st, px.cumsum(0) - px)) and int(px.sum()) == int(S)
    info = (canon, np.ascontiguousarray(sh.numpy(), dtype=np.int64),
            np.ascontiguousarray(st.numpy(), dtype=np.int64))
    try:
        spatial_shapes._mmfs_canonical = (key,) + info
    except Exception:
        pass
    return info


def host_level_counts(host_shapes):
    """(4x4 pixel blocks of all levels, levels with pixels) of a host level table [L, 2]: what the sorted and hybrid
    backwards are told.  A level of H * W == 0 has neither (it owns no pixel and no sort tile)."""
    hs = np.asarray(host_shapes, dtype=np.int64).reshape(-1, 2)
    live = (hs[:, 0] > 0) & (hs[:, 1] > 0)
    return int((((hs[:, 0] + 3) // 4) * ((hs[:, 1] + 3) // 4))[live].sum()), int(live.sum())


def register_level_tables(spatial_shapes, level_start_index, S, host_shapes=None, host_start=None):
    """Tell the shim what a pair of device level tables contains (one device->host copy now, or
    none when the host copies are passed), so that neither pass ever has to look: enables the
    pixel-stationary backward and the hybrid routing of small levels from the first call."""
    key = _level_key(spatial_shapes, level_start_index, S)
    if host_shapes is None or host_start is None:
        return _level_info(spatial_shapes, level_start_index, S)
    sh = torch.as_tensor(host_shapes, dtype=torch.long).reshape(-1, 2).contiguous()
    st = torch.as_tensor(host_start, dtype=torch.long).reshape(-1).contiguous()
    return _seed_level_info(spatial_shapes, key, sh, st, S)




# What one backward call does, decided from numbers alone (_backward_plan):
#   route        "sorted" (mmfs_msda_backward_sorted) | "hybrid" (mmfs_msda_backward_hybrid) | "staged" (the library's own
#                sequence, one entry point per kernel) | "library" (that sequence in one call of mmfs_msda_backward_checked)
#   flags        of mmfs_msda_backward, as every call of the route passes them
#   ws_bytes     of the route's workspace
#   stages       what to launch, in order: (name in the event log, stage bits for "sorted" / "hybrid", else the entry point)
#   blocks4      4x4 pixel blocks of the table ("sorted" only)
#   status_word  whether the call is handed the device's status word (a table the device has to check)
_BackwardPlan = collections.namedtuple("_BackwardPlan", "route flags ws_bytes stages blocks4 status_word")


def _backward_plan(code, dims, slab_bytes, info, lazy_zero_attn):
    """The route of a backward of type ``code`` and ``dims`` = (B, S, H, D, L, Nq, P): no tensor is looked at.
    ``slab_bytes``: one batch row of value; ``info``: what ``_level_info`` knows about the level table, or None.
    Reads the knobs (_taps_algo, _taps_prefer_sorted, _bwd_algo, _hybrid) and, for "one call or one per kernel",
    _event_log; asks the library's host-only queries through ``_memo``."""
    per_kernel = _event_log is not None
    over_limit = slab_bytes > _MAX_SLAB_BYTES
    # (as the forward: the LDS-levels kernel named for a value slab its 32-bit row offsets cannot span -- a matter of
    # size, so the call goes to the row gather's flat-address kernel instead of raising)
    taps = "gather" if _taps_algo == "lds" and over_limit else _taps_algo
    flags = (_BWD_LAZY_ZERO_ATTN if lazy_zero_attn else 0) | _TAPS_FLAGS[taps]
    if _bwd_algo == "atomic":
        flags |= _BWD_FORCE_ATOMIC
    elif info is None:
        flags |= _BWD_DEVICE_CHECKED_LEVELS
    elif info[0]:
        flags |= _BWD_CANONICAL_LEVELS
    canonical = bool(flags & _BWD_CANONICAL_LEVELS)                 # a table the HOST has verified
    # opt-in: grad_loc / grad_attn from the grad_value sort's records (csrc/msda_bwd_taps_sorted.hip): a host-verified
    # canonical table, 16-bit storage, shapes the sort's kept scan takes
    if (_taps_algo == "sorted" or (_taps_prefer_sorted and _taps_algo == "auto")) and canonical and code in (1, 2):
        srt_bytes = _memo(("sorted", code, dims, flags),
                          lambda: _lib.mmfs_msda_backward_sorted_workspace_bytes(code, *dims, flags))
        if srt_bytes > 0:
            return _BackwardPlan("sorted", flags, srt_bytes, _SRT_BWD_STAGES if per_kernel else (("msda_bwd", _SRT_BWD_ALL),),
                                 host_level_counts(info[1])[0], False)
    # ("sorted" by name raises where the route does not apply -- except for a value slab over the limit: the call then
    # goes on to the routes below, like the other named kernels'.  Decided on the size alone, whatever else the route
    # would have refused: fp32 storage, an unregistered or non-canonical table, the float-atomic route asked for.)
    _require(_taps_algo != "sorted" or over_limit,
             "taps algo 'sorted': mmfs_msda_backward_sorted does not apply to these arguments")
    if _hybrid and canonical and code in (1, 2):
        # small levels on the matrix cores, the others through the gather / sort / reduce kernels
        flags |= _BWD_DENSE_TAPS
        # (keyed by the table's CONTENT: a freed host copy's address can come back with another table)
        hyb_bytes = _memo((code, dims, flags, info[1].tobytes(), info[2].tobytes()),
                          lambda: _lib.mmfs_msda_backward_hybrid_workspace_bytes(code, info[1].ctypes.data, info[2].ctypes.data,
                                                                                 *dims, flags))
        if hyb_bytes > 0:
            stages = (("msda_bwd", _HYB_BWD_ALL),)
            if per_kernel:
                stages = _HYB_BWD_STAGES
                # (one kernel does every level: the dense stage has nothing to launch)
                if _memo(("fused", code, dims, flags), lambda: _lib.mmfs_msda_backward_taps_fused(code, *dims, flags)):
                    stages = tuple(s for s in stages if s[0] != "msda_bwd_taps_coarse")
            return _BackwardPlan("hybrid", flags, hyb_bytes, stages, 0, False)
    # the library's own sequence: taps + sort + reduce when the level table is canonical and the head width has a vector
    # path, else (odd head width, fp64, gapped or overlapping levels) float-atomic accumulation (needs an fp32 scratch for
    # 16-bit storage).  One call, unless each kernel is to be timed and the host knows that the table is canonical.
    ws_bytes = _memo((code, dims, flags), lambda: _lib.mmfs_msda_backward_workspace_bytes(code, *dims, flags))
    if canonical and per_kernel:
        return _BackwardPlan("staged", flags, ws_bytes, _STAGED_BWD, 0, False)
    return _BackwardPlan("library", flags, ws_bytes, _LIBRARY_BWD, 0, bool(flags & _BWD_DEVICE_CHECKED_LEVELS))


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                            grad_output, im2col_step, lazy_zero_attn=False, *, value_repeat=None):
    """Reference: ms_deform_attn_cuda_backward, src/cuda/ms_deform_attn_cuda.cu:84-166.
    Returns [grad_value, grad_sampling_loc, grad_attn_weight] shaped and typed like the
    corresponding inputs.  ``lazy_zero_attn`` (an addition, MMFS_BWD_LAZY_ZERO_ATTN): the caller
    never reads grad_attn_weight where attn_weight is exactly 0 (MMFS's masked softmax multiplies it
    by the weight), so those entries may come back as 0 without their value rows being read.
    ``value_repeat`` (another, see ``ms_deform_attn_forward``): a shared bank.  Correct and deterministic, NOT fast --
    sharing is for generation, not training: the backward above runs on the expanded bank (the g copies are made inside
    the call) and grad_value [Bv, S, H, D] is the sum over the copies (``view(...).sum(dim)``), bit for bit what autograd
    returns through ``value.expand``."""
    _require(isinstance(value, torch.Tensor) and value.is_cuda, "Not implemented on the CPU")
    if value_repeat is not None:
        _validate([("value", value), ("sampling_loc", sampling_loc)], value)
        B, S, H, D, L, Nq, P, Bv = _dims_shared(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                                value_repeat)
        g = B // Bv
        grad_value, grad_loc, grad_attn = ms_deform_attn_backward(
            _expand_bank(value, B, value_repeat), spatial_shapes, level_start_index, sampling_loc, attn_weight,
            grad_output, im2col_step, lazy_zero_attn)
        rest = grad_value.shape[1:]
        if value_repeat == "tile":
            grad_value = grad_value.view(g, Bv, *rest).sum(0)
        else:
            grad_value = grad_value.view(Bv, g, *rest).sum(1)
        return [grad_value, grad_loc, grad_attn]
    if _status_words:
        check_level_table_status()
    _validate([("value", value), ("spatial_shapes", spatial_shapes),
               ("level_start_index", level_start_index), ("sampling_loc", sampling_loc),
               ("attn_weight", attn_weight), ("grad_output", grad_output)], value)
    B, S, H, D, L, Nq, P = dims = _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    _require(grad_output.numel() == B * Nq * H * D, "grad_output must be [B, Nq, H*D]")
    _check_step(B, im2col_step)
    loc_dtype, attn_dtype = sampling_loc.dtype, attn_weight.dtype
    sampling_loc, attn_weight = _same_dtype(value, sampling_loc, attn_weight)
    if grad_output.dtype != value.dtype:
        grad_output = grad_output.to(value.dtype)
    value, grad_output = _aligned(value), _aligned(grad_output)
    dt, dev = value.dtype, value.device
    code = _DTYPE_CODE[dt]

    # What the level tables contain is only looked up, never fetched: tables that came from
    # mmfs_amd.levels.make_level_tables / register_level_tables (or were seen by levels_are_canonical)
    # carry their host copy; for any other pair -- the reference's own callers build fresh tensors on
    # every call -- the library checks the table on the device (no device->host copy, no sync).
    info = _level_info(spatial_shapes, level_start_index, S, sync=False)
    plan = _backward_plan(code, dims, S * H * D * value.element_size(), info, lazy_zero_attn)

    grad_value = torch.empty(value.shape, dtype=dt, device=dev)
    grad_loc = torch.empty(sampling_loc.shape, dtype=dt, device=dev)
    grad_attn = torch.empty(attn_weight.shape, dtype=dt, device=dev)
    workspace = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=dev) if plan.ws_bytes else None
    ws = (workspace.data_ptr() if workspace is not None else None, plan.ws_bytes)
    # the pointers every entry point takes some of, in the order of mmfs_msda_backward (include/mmfs_msda.h)
    ptrs = (value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(),
            attn_weight.data_ptr(), grad_output.data_ptr(), grad_value.data_ptr(), grad_loc.data_ptr(), grad_attn.data_ptr())
    if plan.route == "sorted":
        route_counts["sorted"] += 1
    with _on_device(dev):
        stream = _stream(dev)
        word = _status_word(dev)[0].data_ptr() if plan.status_word else None

        tables = (info[1].ctypes.data, info[2].ctypes.data) if plan.route == "hybrid" else None

        def call(stage, ws):
            """(entry point, its arguments between the type code and the stream) of one stage: ``stage`` is the stage bits
            of the plan's route, or the name of an entry point of the library's own sequence."""
            if stage == "mmfs_msda_backward_checked":
                return stage, (*ptrs, *ws, *dims, plan.flags, word)
            if plan.route == "sorted":
                return "mmfs_msda_backward_sorted", (*ptrs, *ws, *dims, plan.blocks4, plan.flags, stage)
            if plan.route == "hybrid":
                return "mmfs_msda_backward_hybrid", (*ptrs[:3], *tables, *ptrs[3:], *ws, *dims, plan.flags, stage)
            take, with_ws = _STAGED_ARGS[stage]
            return stage, (*[ptrs[i] for i in take], *(ws if with_ws else ()), *dims)

        def run(stages, ws):
            for name, stage in stages:
                entry, args = call(stage, ws)
                status = _launch(name, dev, getattr(_lib, entry), code, *args, stream)
                if status != 0:
                    return status
            return 0
        status = run(plan.stages, ws)
        if status == _E_UNSUPPORTED and plan.route in ("hybrid", "staged"):
            # refused, so fall back: the library's one call with the flags the route had (_BWD_DENSE_TAPS included) and the
            # workspace that was asked about -- none in the hybrid route's case, where only the hybrid workspace was
            status = run(_LIBRARY_BWD, ws if plan.route == "staged" else (None, 0))
        _check(status, "ms_deform_attn_backward")
    if loc_dtype != dt:
        grad_loc = grad_loc.to(loc_dtype)
    if attn_dtype != dt:
        grad_attn = grad_attn.to(attn_dtype)
    return [grad_value, grad_loc, grad_attn]
