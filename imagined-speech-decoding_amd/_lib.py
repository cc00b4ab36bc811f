"""ctypes binding of libisd_hip.so (the C ABI of include/isd_hip.h).

There is no CPU fallback: if the library is missing or a call fails the
product raises.  Build it with ``python -m isd_amd.build`` (or
``__graft_entry__.build()``).
"""
import ctypes as C
import os

import numpy as np
import torch

from .build import LIB_PATH

ISD_OK = 0
ISD_ERR_INVALID, ISD_ERR_UNSUPPORTED, ISD_ERR_HIP, ISD_ERR_NO_DEVICE = -1, -2, -3, -4
FB_F32, FB_F64, FB_AUTO, FB_MIXED = 0, 1, 2, 3
BP_MAGNITUDE, BP_POWER, BP_LOGPOWER = 0, 1, 2


class IsdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libisd_hip error {code}: {msg}")
        self.code = code


class IsdUnsupported(IsdError):
    pass


_p, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
_pi, _pd = C.POINTER(C.c_int), C.POINTER(C.c_double)

# name -> (restype, argtypes); every symbol include/isd_hip.h declares
SIGNATURES = {
    "isd_abi_version": (_i, []),
    "isd_last_error": (C.c_char_p, []),
    "isd_shader_clock_probe": (_i, [_p, _i, _p]),
    "isd_wall_clock_khz": (_i, []),
    "isd_exact_sum_workspace_bytes": (_i64, []),
    "isd_exact_sum": (_i, [_p, _i64, _p, _p, _p]),
    "isd_device_count": (_i, []),
    "isd_adamw_step": (_i, [_p, _p, _p, _p, _i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i64,
                       _p, _p, _p]),
    "isd_adamw_multi_step": (_i, [_i, _p, _p, _p, _p, _p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                             _i64, _p, _p, _p]),
    "isd_fb_plan_create": (_i, [C.POINTER(_p), _i, _i, _pd, _pd, _i]),
    "isd_fb_plan_destroy": (_i, [_p]),
    "isd_fb_plan_precision": (_i, [_p]),
    "isd_fb_forward": (_i, [_p, _p, _p, _i64, _i64, _i64, _p]),
    "isd_stft_plan_create": (_i, [C.POINTER(_p), _i, _i, _i]),
    "isd_stft_plan_destroy": (_i, [_p]),
    "isd_stft_plan_frames": (_i, [_p]),
    "isd_stft_plan_bins": (_i, [_p]),
    "isd_stft_forward": (_i, [_p, _p, _p, _i64, _p]),
    "isd_stft_bandpower": (_i, [_p, _p, _p, _i64, _i64, _i, _i, _pi, _pi, _i, _f, _p]),
    "isd_stft_bandpower_last_path": (_i, []),
    "isd_features_fused": (_i, [_p, _p, _p, _p, _i64, _i64, _pi, _pi, _i, _f, _p]),
    "isd_features_fused_bf16": (_i, [_p, _p, _p, _p, _i64, _i64, _pi, _pi, _i, _f, _p]),
    "isd_features_fused_last_path": (_i, []),
    "isd_features_fused_last_serial_waves": (_i, []),
    "isd_features_backward_workspace_bytes": (_i64, [_p, _p, _i64, _i64, _pi, _pi]),
    "isd_features_backward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i64, _pi, _pi, _i, _f, _p]),
    "isd_attr_mix": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _i, _i64, _i, _p]),
    "isd_attr_accumulate": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _i, _i64, _i, _f, _p]),
    "isd_fir_plan_create": (_i, [C.POINTER(_p), _i, _pd]),
    "isd_fir_plan_destroy": (_i, [_p]),
    "isd_fir_plan_taps": (_i, [_p]),
    "isd_fir_zero_phase_f32": (_i, [_p, _p, _p, _i64, _i, _p]),
    "isd_fir_zero_phase_f64": (_i, [_p, _p, _p, _i64, _i, _p]),
    "isd_trial_cov_f32": (_i, [_p, _p, _i64, _i, _i, _p]),
    "isd_trial_cov_f64": (_i, [_p, _p, _i64, _i, _i, _p]),
    "isd_cov_group_mean": (_i, [_p, _i, _p, _p, _i, _p, _i64, _i, _i, _p]),
    "isd_csp_power_f32": (_i, [_p, _p, _p, _i64, _i, _i, _i, _i, _p]),
    "isd_csp_power_f64": (_i, [_p, _p, _p, _i64, _i, _i, _i, _i, _p]),
    "isd_fb_trial_cov": (_i, [_p, _p, _p, _i64, _i, _i, _p]),
    "isd_fb_csp_power": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _i, _p]),
    "isd_ica_step_work_bytes": (_i64, [_i64, _i, _i, _i, _i]),
    "isd_ica_step_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i, _i, _i, _p]),
    "isd_ica_step_f64": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i, _i, _i, _p]),
    "isd_spatial_apply_f32": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "isd_spatial_apply_f64": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "isd_spd_congruence": (_i, [_p, _i, _p, _p, _p, _i64, _i, _i, _p]),
    "isd_spd_eigfun": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "isd_psd_plan_create": (_i, [C.POINTER(_p), _i, _i, _i, _i, _i, _pd, C.c_double, _i]),
    "isd_psd_plan_destroy": (_i, [_p]),
    "isd_psd_plan_bins": (_i, [_p]),
    "isd_psd_plan_segments": (_i64, [_p, _i64]),
    "isd_psd_work_bytes": (_i64, [_p, _i64, _i64, _i]),
    "isd_psd_welch_f32": (_i, [_p, _p, _p, _i64, _i64, _i, _p, _p]),
    "isd_psd_welch_f64": (_i, [_p, _p, _p, _i64, _i64, _i, _p, _p]),
    "isd_csd_chunk_bytes": (_i64, [_i64]),
    "isd_csd_work_bytes": (_i64, [_p, _i64, _i64, _i64, _i, _i]),
    "isd_csd_welch_f32": (_i, [_p, _p, _p, _i64, _i64, _i64, _i, _i, _p, _p]),
    "isd_csd_welch_f64": (_i, [_p, _p, _p, _i64, _i64, _i64, _i, _i, _p, _p]),
    "isd_envcorr_work_bytes": (_i64, [_i64, _i64, _i64, _i]),
    "isd_envcorr_f32": (_i, [_p, _p, _i64, _i64, _i64, _i, _p, _p]),
    "isd_envcorr_f64": (_i, [_p, _p, _i64, _i64, _i64, _i, _p, _p]),
    "isd_contime_f32": (_i, [_p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _p]),
    "isd_contime_f64": (_i, [_p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _p]),
    "isd_pac_work_bytes": (_i64, [_i64, _i64, _i64, _i64, _i]),
    "isd_pac_f32": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i, C.c_double, _p, _p]),
    "isd_pac_f64": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i, C.c_double, _p, _p]),
    "isd_tfr_plan_create": (_i, [C.POINTER(_p), _i, _pi, _pd, _i]),
    "isd_tfr_plan_destroy": (_i, [_p]),
    "isd_tfr_plan_out_len": (_i64, [_p, _i64]),
    "isd_tfr_plan_padded_taps": (_i64, [_p]),
    "isd_tfr_work_bytes": (_i64, [_p, _i64, _i64, _i64, _i, _i]),
    "isd_tfr_cwt_f32": (_i, [_p, _p, _p, _i64, _i64, _i64, _i, _p, _p]),
    "isd_tfr_cwt_f64": (_i, [_p, _p, _p, _i64, _i64, _i64, _i, _p, _p]),
    "isd_resample_plan_create": (_i, [C.POINTER(_p), _i, _i, _i, _pd, _i]),
    "isd_resample_plan_destroy": (_i, [_p]),
    "isd_resample_out_len": (_i64, [_p, _i64]),
    "isd_resample_poly_f32": (_i, [_p, _p, _p, _i64, _i, _i, C.c_double, _p, _p]),
    "isd_resample_poly_f64": (_i, [_p, _p, _p, _i64, _i, _i, C.c_double, _p, _p]),
    "isd_conv4_plan_create": (_i, [C.POINTER(_p), _i, _i, _pi, _pi, _i, _i, _i, _i]),
    "isd_conv4_plan_destroy": (_i, [_p]),
    "isd_conv4_plan_set_activation_dtype": (_i, [_p, _i]),
    "isd_conv4_param_count": (_i64, [_p]),
    "isd_conv4_param_offset": (_i64, [_p, _i, _i]),
    "isd_conv4_windows": (_i, [_p, _i64]),
    "isd_conv4_workspace_bytes": (_i64, [_p, _i64, _i64]),
    "isd_conv4_forward": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _p]),
    "isd_conv4_backward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i64, _p]),
    "isd_conv4_backward_x": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _p]),
    "isd_linear_forward": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "isd_linear_residual_forward": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _p]),
    "isd_linear_workspace_bytes": (_i64, [_i64, _i, _i]),
    "isd_embed_forward": (_i, [_p, _p, _p, _p, _i64, _i, _i, _p]),
    "isd_embed_backward": (_i, [_p, _p, _p, _p, _i64, _i, _i, _p]),
    "isd_layernorm_forward": (_i, [_p, _p, _p, _p, _p, _i64, _i, _f, _p]),
    "isd_layernorm_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _p]),
    "isd_attention_forward": (_i, [_p, _p, _p, _i64, _i, _i, _i, _f, C.c_uint64, _p]),
    "isd_attention_backward": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _f, C.c_uint64, _p]),
    "isd_tail_fused_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "isd_tail_fused_param_count": (_i64, [_i, _i, _i, _i]),
    "isd_tail_fused_save_floats": (_i64, [_i64, _i, _i, _i]),
    "isd_tail_fused_workspace_floats": (_i64, [_i64, _i, _i, _i, _i, _i]),
    "isd_tail_fused_forward": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, C.c_uint64, _p,
                                    _p]),
    "isd_tail_fused_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f,
                                     C.c_uint64, _p, _p]),
    "isd_linear_backward": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "isd_eegnet_plan_create": (_i, [C.POINTER(_p), _i, _i, _i, _i]),
    "isd_featcnn_supported": (_i, [_p, _i64, _i64, _i]),
    "isd_first_layer_last_path": (_i, []),
    "isd_first_wgrad_last_stage_loop": (_i, []),
    "isd_featcnn_step": (_i, [_p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _i64, _i64, _i, _f, _p]),
    "isd_featcnn_step_bf16": (_i, [_p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _i64, _i64, _i, _f, _p]),
    "isd_paperhead_plan_create": (_i, [C.POINTER(_p), _i, _i, _i]),
    "isd_paperhead_plan_destroy": (_i, [_p]),
    "isd_paperhead_param_count": (_i64, [_p]),
    "isd_paperhead_buffer_count": (_i64, [_p]),
    "isd_paperhead_workspace_bytes": (_i64, [_p, _i64]),
    "isd_paperhead_forward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _f, _f, _p]),
    "isd_paperhead_backward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _p]),
    "isd_paperhead_backward_x": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _p]),
    "isd_paperhead_forward_stage": (_i, [_p, _i, _p, _p, _p, _p, _p, _i64, _i, _f, _f, _i, _p]),
    "isd_paperhead_backward_stage": (_i, [_p, _i, _p, _p, _p, _p, _p, _i64, _i, _p]),
    "isd_paperhead_sync_block": (_i, [_p, _i64, _i, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "isd_paperhead_sync_block_kind": (_i, [_i, _i]),
    "isd_eegnet_sync_block_kind": (_i, [_i, _i]),
    "isd_zone_batch_begin": (_i, []),
    "isd_zone_batch_next": (_i, []),
    "isd_zone_batch_launch": (_i, [_p]),
    "isd_zone_batch_abort": (_i, []),
    "isd_cvblock_plan_create": (_i, [C.POINTER(_p), _i, _i, _i]),
    "isd_cvblock_flat_dim": (_i64, [_p]),
    "isd_eegnet_plan_set_seed_counter": (_i, [_p, _p]),
    "isd_eegnet_plan_set_input_dtype": (_i, [_p, _i]),
    "isd_eegnet_plan_destroy": (_i, [_p]),
    "isd_eegnet_param_count": (_i64, [_p]),
    "isd_eegnet_buffer_count": (_i64, [_p]),
    "isd_eegnet_workspace_bytes": (_i64, [_p, _i64]),
    "isd_eegnet_forward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _f, _f, _f, C.c_uint64, _p]),
    "isd_eegnet_backward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _f, C.c_uint64, _p]),
    "isd_eegnet_backward_x": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _f, C.c_uint64, _p]),
    "isd_eegnet_forward_stage": (_i, [_p, _i, _p, _p, _p, _p, _p, _i64, _i, _f, _f, _f, C.c_uint64, _i, _p]),
    "isd_eegnet_backward_stage": (_i, [_p, _i, _p, _p, _p, _p, _p, _i64, _f, C.c_uint64, _i, _p]),
    "isd_eegnet_sync_block": (_i, [_p, _i64, _i, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "isd_softmax_ce_workspace_bytes": (_i64, [_i64]),
    "isd_softmax_ce": (_i, [_p, _p, _i, _p, _p, _p, _p, _i64, _i, _i, _f, _p, _p]),
    "isd_tsception_plan_create": (_i, [C.POINTER(_p), _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "isd_tsception_plan_destroy": (_i, [_p]),
    "isd_tsception_param_count": (_i64, [_p]),
    "isd_tsception_buffer_count": (_i64, [_p]),
    "isd_tsception_workspace_bytes": (_i64, [_p, _i64]),
    "isd_tsception_forward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _f, _f, _f, C.c_uint64, _p]),
    "isd_tsception_backward": (_i, [_p, _p, _p, _p, _p, _p, _i64, _f, C.c_uint64, _p]),
    "isd_tsception_temporal_probe": (_i, [_p, _p, _p, _p, _i64, _i, _p]),
}

_lib = None


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                "There is no CPU fallback for the product path.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)           # AttributeError if the header and the .so disagree
            fn.restype, fn.argtypes = res, args
        if h.isd_abi_version() != 1:
            raise ImportError(f"{LIB_PATH}: ABI version {h.isd_abi_version()} != 1; rebuild")
        _lib = h
    return _lib


def check(rc):
    if rc != ISD_OK:
        msg = lib().isd_last_error().decode("utf-8", "replace")
        raise (IsdUnsupported if rc == ISD_ERR_UNSUPPORTED else IsdError)(rc, msg)
    return rc


class Handle:
    """Owner of one library plan: ``_create`` fills ``_h`` through a ``*_plan_create`` entry point, and the wrapper's
    end releases it through the entry point the subclass names in ``_destroy``."""
    _destroy = None

    def _create(self, create, *args):
        self._h = C.c_void_p()
        check(getattr(lib(), create)(C.byref(self._h), *args))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(lib(), self._destroy)(h)
            except Exception:
                pass


def stream():
    """The current stream of the current device, as the library's ``stream`` argument."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device):
    """The uint8 scratch tensor a ``*_work_bytes`` entry point asked for; its negative answer is the library's error."""
    if nbytes < 0:
        check(int(nbytes))
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def typed(stem, dtype):
    """The entry point of a float32 / float64 pair for ``dtype``: ``lib().<stem>_f32`` or ``lib().<stem>_f64``."""
    return getattr(lib(), stem + {torch.float32: "_f32", torch.float64: "_f64"}[dtype])


def _names(dtypes):
    return " or ".join(str(d).replace("torch.", "") for d in dtypes)


def check_array(x, name, dtypes=(torch.float32, torch.float64)):
    """The type rules of an array argument, none of which needs a GPU -> (x, is_tensor): a CUDA tensor of one of
    ``dtypes`` as it is, anything else as a floating-point ndarray.  Rank and shape are the caller's."""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise TypeError("tensor input must live on the GPU (there is no CPU fallback)")
        if x.dtype not in dtypes:
            raise TypeError(f"{name} must be {_names(dtypes)}")
        return x, True
    x = np.asarray(x)
    if x.dtype.kind != "f":
        raise TypeError(f"{name} must be floating point")
    return x, False


def check_cuda(x, name, max_channels, dtypes=(torch.float32, torch.float64), square=False):
    """The argument of a kernel wrapper: a CUDA tensor [n, C, T] (``square``: [n, C, C]) of one of ``dtypes`` with
    1 <= C <= ``max_channels`` and T >= 1 -> x, contiguous."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in dtypes):
        raise TypeError(f"{name} must be a {_names(dtypes)} CUDA tensor")
    shape = "[n, C, C]" if square else "[n, C, T]"
    if x.ndim != 3 or (square and x.shape[1] != x.shape[2]):
        raise ValueError(f"{name} must be {shape}, got {tuple(x.shape)}")
    if not 1 <= x.shape[1] <= max_channels or x.shape[2] < 1:
        raise ValueError(f"{name} {shape} needs 1 <= C <= {max_channels}{'' if square else ' and T >= 1'}, "
                         f"got {tuple(x.shape)}")
    return x.contiguous()


def to_device(x, is_tensor, who, dtype=np.float64, device=None):
    """x of ``check_array`` on the GPU: a tensor made contiguous, an ndarray uploaded as ``dtype`` to ``device`` (the
    current one by default).  A read-only array (np.frombuffer, a memory map) is copied first: torch warns about
    sharing one."""
    if is_tensor:
        return x.contiguous()
    if not torch.cuda.is_available():
        raise RuntimeError(f"isd_amd.{who} needs an MI355X GPU: there is no CPU fallback")
    arr = np.ascontiguousarray(x, dtype=dtype)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(dev)


def int_array(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


def double_array(vals):
    return (C.c_double * len(vals))(*[float(v) for v in vals])
