"""ctypes binding of libdfengine.so (C ABI: include/df_engine.h).

PyTorch is used only as plumbing here: device memory (``tensor.data_ptr()``), the current HIP stream
and dtype/shape bookkeeping.  There is NO fallback: if the shared library is missing or a call fails,
a RuntimeError is raised -- results never come from a torch/CPU path.
"""
import ctypes as C
import itertools
import os
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdfengine.so")            # bf16 MFMA operands (BASELINE configs[1]'s literal wording)
LIB_PATHS = {"bf16": LIB_PATH, "fp16": os.path.join(_HERE, "libdfengine_f16.so")}   # same sources, -DDF_OPERAND_F16
OPERAND_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def default_precision():
    """MFMA operand type of engines created without an explicit ``precision``: env DF_PRECISION or "fp16".

    fp16 is the default because it is the operand type whose decoded mel meets the north-star tolerance (25-step DDIM mel MAE
    5.8e-4 < 1e-3 vs the fp32 CPU reference); the bf16 build runs at the same speed with 8x the operand rounding (mel MAE
    4.5e-3: outside the tolerance) and is selected explicitly, ``precision="bf16"`` / ``DF_PRECISION=bf16``."""
    p = os.environ.get("DF_PRECISION", "fp16")
    if p not in LIB_PATHS:
        raise RuntimeError(f"DF_PRECISION={p!r}: expected one of {sorted(LIB_PATHS)}")
    return p


class GemmDesc(C.Structure):
    """include/df_engine.h df_test_gemm_desc (df_test_gemm_ex / df_test_gemm_valid); `size` is filled in here."""
    _fields_ = [("size", C.c_int64), ("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p)] + [
        (n, C.c_int) for n in ("M", "N", "K", "lda", "ldc", "out_operand", "conv", "NB", "H", "Wd", "Cin", "stride", "batch", "tile",
                               "splitk", "gm")] + [
        (n, C.c_int64) for n in ("a_bs", "w_bs", "c_bs", "res_bs")] + [
        ("alpha", C.c_float), ("bias", C.c_void_p), ("rowbias", C.c_void_p), ("ld_rowbias", C.c_int), ("rows_per_sample", C.c_int),
        ("rowbias_mode", C.c_int), ("res", C.c_void_p), ("ldr", C.c_int), ("relu", C.c_int), ("silu", C.c_int), ("aux", C.c_void_p),
        ("ld_aux", C.c_int), ("stats", C.c_void_p), ("stats_slots", C.c_int), ("ln_stats", C.c_void_p), ("ln_slots", C.c_int),
        ("ln_C", C.c_int), ("ln_eps", C.c_float), ("ln_cs", C.c_void_p), ("w_rows", C.c_int), ("sm_w", C.c_int),
        ("sm_valid", C.c_int), ("dup_rows", C.c_int), ("no_c_store", C.c_int), ("store_nchw", C.c_int), ("hw_out", C.c_int),
        ("cfg_out", C.c_void_p), ("cfg_scale", C.c_float), ("defer_reduce", C.c_int), ("slabs_out", C.c_void_p),
        ("ups", C.c_int), ("zstuff", C.c_int), ("A2", C.c_void_p), ("lda2", C.c_int), ("Cin2", C.c_int), ("geglu", C.c_int),
        ("vt", C.c_void_p), ("vt_col0", C.c_int), ("vt_T", C.c_int), ("ldvt", C.c_int)]

    def __init__(self, **kw):
        kw.setdefault("alpha", 1.0)
        super().__init__(size=C.sizeof(GemmDesc), **kw)


class GemmTile(C.Structure):
    """include/df_engine.h df_test_gemm_tile: one row of the GEMM tile table (csrc/gemm_tiles.def)."""
    _fields_ = [("size", C.c_int64), ("name", C.c_char_p)] + [(n, C.c_int) for n in ("family", "bm", "bn", "dma_threads", "ring", "modes")]


class GemmLaunch(C.Structure):
    """include/df_engine.h df_test_gemm_launch: the launch constants launch_gemm hands a GEMM-family kernel (csrc/gemm.h GemmLaunch)."""
    class Magic(C.Structure):
        """x // d == (x * mul) >> (32 + sh) for 0 <= x < 2^31; d == 1: x"""
        _fields_ = [("mul", C.c_uint32), ("sh", C.c_int), ("d", C.c_int)]

    MAGIC = ("per", "rows", "last", "wrb", "ohw", "ow", "cin")      # what magic[i] divides by (include/df_engine.h)
    _fields_ = ([("size", C.c_int64)] + [(n, C.c_int) for n in ("nbm", "nbn", "nblk", "xq", "xr", "gm")] + [("magic", Magic * 7)] +
                [(n, C.c_int) for n in ("nk", "kper", "n2tot", "used", "per2")] +
                [(n, C.c_int) for n in ("HWp", "PPX", "PB", "HR", "APASS", "npx", "npy", "pimg", "npatch")] +
                [(n, C.c_float) for n in ("inv_hwp", "inv_tw2", "inv_pimg", "inv_npx", "inv_ppx", "inv_tw")] +
                [("th", C.c_int), ("tw", C.c_int)])


TILE_FAMILIES = ("generic", "halo", "ps", "pgeglu", "wgeglu", "retired")      # df_test_gemm_tile.family


def gemm_tiles(L=None):
    """The tile table of a loaded build (host only): {id: dict(name, family, bm, bn, dma_threads, ring, modes)}."""
    L = L or lib()
    out, t = {}, GemmTile(size=C.sizeof(GemmTile))
    while L.df_test_gemm_tile_info(len(out), C.byref(t)) == 0:
        out[len(out)] = dict(name=t.name.decode(), family=TILE_FAMILIES[t.family], bm=t.bm, bn=t.bn, dma_threads=t.dma_threads,
                             ring=t.ring, modes=tuple(m for m in range(4) if t.modes >> m & 1))
    return out


class UNetConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("model_channels", C.c_int),
                ("num_res_blocks", C.c_int), ("channel_mult", C.c_int * 8), ("n_mult", C.c_int),
                ("attention_resolutions", C.c_int * 8), ("n_attn", C.c_int), ("num_heads", C.c_int),
                ("context_dim", C.c_int)]


class VaeConfig(C.Structure):
    _fields_ = [("z_channels", C.c_int), ("embed_dim", C.c_int), ("ch", C.c_int), ("num_res_blocks", C.c_int),
                ("out_ch", C.c_int), ("ch_mult", C.c_int * 8), ("n_mult", C.c_int), ("scale_factor", C.c_float)]


class VaeEncoderConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int)]


class CondConfig(C.Structure):
    _fields_ = [("origin_dim", C.c_int), ("embed_dim", C.c_int), ("seq_len", C.c_int)]


class CavpConfig(C.Structure):
    _fields_ = [("stage_blocks", C.c_int * 4), ("base_channels", C.c_int), ("embed_dim", C.c_int)]


class CavpSpecConfig(C.Structure):
    _fields_ = [("n_mels", C.c_int), ("channels", C.c_int * 6), ("fc_dim", C.c_int), ("embed_dim", C.c_int)]


_libs = {}

_SIGS = {
    "df_create": [C.c_int, C.POINTER(C.c_void_p)],
    "df_config_unet": [C.c_void_p, C.POINTER(UNetConfig)],
    "df_config_vae": [C.c_void_p, C.POINTER(VaeConfig)],
    "df_config_cond": [C.c_void_p, C.POINTER(CondConfig)],
    "df_config_vae_encoder": [C.c_void_p, C.POINTER(VaeEncoderConfig)],
    "df_config_vae_encoder_only": [C.c_void_p, C.POINTER(VaeConfig), C.POINTER(VaeEncoderConfig)],
    "df_config_cavp": [C.c_void_p, C.POINTER(CavpConfig)],
    "df_cavp_encode": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_cavp_pool": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_config_cavp_spec": [C.c_void_p, C.POINTER(CavpSpecConfig)],
    "df_cavp_spec_encode": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_cavp_similarity": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p],
    "df_config_classifier": [C.c_void_p, C.POINTER(UNetConfig)],
    "df_load_tensor": [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int],
    "df_load_tensor_dev": [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int],
    "df_finalize": [C.c_void_p],
    "df_autotune": [C.c_void_p, C.c_int],
    "df_cond_encode": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "df_unet_set_context": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "df_unet_forward": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_unet_forward_cfg": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                            C.c_void_p],
    "df_unet_set_timesteps": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_unet_forward_ts": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_unet_forward_cfg_ts": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                               C.c_void_p],
    "df_vae_decode": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_vae_encode": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_posterior_sample": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p],
    "df_align_verdict": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "df_classifier_forward": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_void_p],
    "df_classifier_grad": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                           C.c_int, C.c_int, C.c_void_p],
    "df_classifier_grad_cached": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_uint64, C.c_void_p],
    "df_prepack": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int],
    "df_packed_size": [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "df_export_packed": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "df_import_packed": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p],
    "df_frames_to_tensor": [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                                                  C.c_void_p, C.c_int, C.c_void_p],
    "df_mel_to_stft": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p,
                       C.c_void_p],
    "df_griffinlim": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 9,
    "df_wave_to_mel": [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                       C.c_void_p, C.c_void_p],
    "df_wave_to_mel_tile": [],
    "df_cfg_combine": [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p],
    "df_lincomb": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.c_int, C.c_int64, C.c_void_p],
    "df_q_sample_blend": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                          C.c_float, C.c_float, C.c_void_p],
    "df_q_sample": [C.c_void_p] * 6 + [C.c_int, C.c_int64, C.c_int, C.c_void_p],
    "df_diffusion_loss": [C.c_void_p] * 7 + [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p],
    "df_dpm_data_prediction": [C.c_void_p] * 4 + [C.c_int, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p],
    "df_dpm_adaptive_error": [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_float, C.c_float, C.c_void_p],
    "df_window_gather": [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p],
    "df_window_blend": [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p],
    "df_ddim_update": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                       C.c_float, C.c_float, C.c_void_p],
    "df_plan_count": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "df_unet_plan_stats": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "df_profile_begin": [C.c_void_p],
    "df_profile_end": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)],
    "df_profile_dump": [C.c_void_p, C.c_char_p],
    "df_tune_cache_export": [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)],
    "df_tune_cache_import": [C.c_char_p, C.c_int64],
    "df_debug_checksums": [C.c_void_p, C.c_int, C.c_int64],
    "df_debug_checksums_read": [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_int64)],
    "df_debug_checksum_label": [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64],
    "df_test_geglu": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                      C.c_int, C.c_void_p],
    "df_test_scratch_read": [C.c_void_p, C.c_int64],
    "df_test_conv3x3_fewout": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p],
    "df_test_conv3x3_fewin": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p],
    "df_test_conv3x3_fewin_gemm": [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p],
    "df_test_vae_encode_tap": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_test_conv3x3_down": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p],
    "df_test_conv3x3_down_valid": [C.c_int] * 8,
    "df_debug_saturations": [C.c_void_p, C.c_int, C.c_int64],
    "df_debug_saturations_read": [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_int64)],
    "df_debug_saturation_label": [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64],
    "df_debug_requant": [C.c_void_p, C.c_char_p],
    "df_debug_poison": [C.c_void_p, C.c_int],
    "df_test_poison_selftest": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "df_test_gemm_epi": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                         C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_test_gemm_dual": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                          C.c_void_p],
    "df_test_gemm": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_test_ln_chain": [C.c_void_p] * 11 + [C.c_int] * 10 + [C.c_void_p],
    "df_test_linear_rows": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p],
    "df_test_unet_block": [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6
                          + [C.c_void_p],
    "df_test_conv3x3": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.c_void_p],
    "df_test_conv3x3_skip": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p],
    "df_test_conv3x3_ups4": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.c_int, C.c_int, C.c_void_p],
    "df_test_groupnorm": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                          C.c_void_p, C.c_void_p],
    "df_test_groupnorm_own_slabs": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "df_test_groupnorm_form": [C.c_int] * 4,
    "df_test_attention_form": [C.c_int] * 3,
    "df_test_groupnorm_ex": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p,
                             C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                             C.c_int, C.c_void_p],
    "df_test_layernorm": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "df_test_layernorm_ex": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "df_test_attention": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p],
    "df_test_groupnorm_bwd": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                              C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "df_test_layernorm_bwd": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p],
    "df_test_geglu_fwd": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
    "df_test_geglu_bwd": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
    "df_test_attention_bwd": [C.c_void_p, C.c_int] * 7 + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_void_p],
    "df_test_cls_head_bwd": [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p],
    "df_test_pack_linear_t": [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p],
    "df_test_pack_conv_bwd": [C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p],
    "df_test_conv3x3_bwd_data": [C.c_void_p] * 5 + [C.c_int] * 8 + [C.c_void_p],
    "df_test_gemm_ex": [C.POINTER(GemmDesc), C.c_void_p],
    "df_test_gemm_valid": [C.POINTER(GemmDesc), C.c_int, C.c_int, C.c_int],
    "df_test_gemm_why": [C.POINTER(GemmDesc), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int],
    "df_test_gemm_key": [C.POINTER(GemmDesc), C.c_int, C.c_char_p, C.c_int],
    "df_test_gemm_tile_info": [C.c_int, C.POINTER(GemmTile)],
    "df_test_gemm_launch_constants": [C.POINTER(GemmDesc), C.c_int, C.c_int, C.c_int, C.POINTER(GemmLaunch)],
    "df_test_xattn_chain": [C.c_void_p] * 10 + [C.c_int] * 6 + [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_void_p],
    "df_test_pack_ffproj": [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p],
    "df_test_softmax_rows": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_test_timestep_embedding": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "df_test_timestep_embedding_b16": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "df_test_pack_latent": [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p],
    "df_test_pack_latent_bcast": [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "df_test_bcast_rows": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "df_test_cast_bf16": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "df_test_cast_bf16_2d": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p],
    "df_test_avgpool": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "df_test_pack_conv_weight": [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p],
    "df_test_pack_conv_skip": [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p],
    "df_test_pack_geglu": [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p],
    "df_test_pack_ln_linear": [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p],
    "df_test_grad_scale_per_sample": [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p],
    "df_test_stem_im2col": [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p],
    "df_test_maxpool3x3s2": [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p],
    "df_test_subsample2": [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p],
    "df_test_tcat3": [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p],
    "df_test_pack_conv3d_bn": [C.c_void_p] * 5 + [C.c_float, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p],
    "df_test_maxpool_time": [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p],
    "df_test_l2norm_rows": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "df_test_spec_conv_in": [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p), C.c_float, C.c_void_p] + [C.c_int] * 5
                            + [C.c_void_p],
    "df_test_avgpool_nhwc": [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p],
    "df_test_spec_head_pool": [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p],
    "df_test_cavp_spec_tap": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p],
    "df_test_peak": [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p],
    "df_test_fill": [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p],
}


def lib(precision=None):
    """Load libdfengine[_f16].so (built in-tree by __graft_entry__.build / csrc/build.sh).  Fails loudly."""
    if precision is None and _libs:          # precision-independent entry points: any loaded build will do
        return next(iter(_libs.values()))
    precision = precision or default_precision()
    if precision not in _libs:
        path = os.environ.get("DF_LIB_OVERRIDE") or LIB_PATHS[precision]      # tools: A/B against another build
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with diff_foley_amd/csrc/build.sh "
                               "(there is no CPU/torch fallback for the sampling path)")
        L = C.CDLL(path)
        for name, args in _SIGS.items():
            if os.environ.get("DF_LIB_OVERRIDE") and not hasattr(L, name):
                continue                      # tools: A/B against an older build that predates an entry point
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        L.df_last_error.restype = C.c_char_p
        L.df_destroy.argtypes = [C.c_void_p]
        L.df_destroy.restype = None
        L.df_abi_version.restype = C.c_int
        L.df_operand_dtype.restype = C.c_char_p
        want = {"bf16": b"bf16", "fp16": b"f16"}[precision]
        if L.df_operand_dtype() != want:
            raise RuntimeError(f"{path} was built for {L.df_operand_dtype()!r} operands, expected {want!r}")
        _libs[precision] = L
    return _libs[precision]


def exported_symbols():
    return list(_SIGS.keys()) + ["df_last_error", "df_destroy", "df_abi_version", "df_operand_dtype"]


def _chk(rc, L=None):
    if rc != 0:
        raise RuntimeError("libdfengine: " + (L or lib()).df_last_error().decode())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _dev_f32(t, device):
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    return t


def _want_dim(what, got, want):
    """The C ABI takes raw pointers: a tensor with the wrong feature width would be read out of bounds, not rejected."""
    if want is not None and int(got) != int(want):
        raise RuntimeError(f"{what}: last dimension is {got}, the loaded model expects {want}")


class Configured:
    """What the ``config_*`` calls of one engine were given: per family, the integers its forward calls check a tensor against and size
    their outputs with.  The C ABI takes raw pointers, so no forward call runs without them: asking for a family that was never
    configured raises and names the call it needs.  Plain Python: no ctypes, no device."""
    NEEDS = dict(unet="config_unet", cls="config_classifier", vae="config_vae / config_vae_encoder_only",
                 vae_encoder="config_vae_encoder / config_vae_encoder_only", cond="config_cond", cavp="config_cavp",
                 cavp_spec="config_cavp_spec")

    def __init__(self):
        self._of = {}

    def record(self, family, **ints):
        self._of[family] = types.SimpleNamespace(**{k: tuple(int(i) for i in v) if isinstance(v, (list, tuple)) else int(v)
                                                    for k, v in ints.items()})

    def drop(self, family):
        self._of.pop(family, None)

    def of(self, family):
        """The record of ``family`` (attributes named as recorded), the very object stored: no copy per call."""
        try:
            return self._of[family]
        except KeyError:
            raise RuntimeError(f"{family} is not configured: call Engine.{self.NEEDS[family]}(...) first") from None


class PositionOutOfRange(IndexError, RuntimeError):
    """More frames than the cond stage's positional table has rows.  The reference looks the positions up in an nn.Embedding
    (video_feat_encoder.py:16), which answers an index past the table with an IndexError on the CPU and with a RuntimeError (device-side
    assert) on a GPU: a caller that catches either catches this."""


def _want_nchw(what, x, channels):
    """x must be [N][channels][H][W]: the engine derives every address from these four numbers."""
    if x.ndim != 4:
        raise RuntimeError(f"{what}: expected a 4-D NCHW tensor, got shape {tuple(x.shape)}")
    if channels is not None and int(x.shape[1]) != int(channels):
        raise RuntimeError(f"{what}: {x.shape[1]} channels, the loaded model expects {channels}")


def _timesteps(t, n, device):
    """One timestep per batch row.  A one-element t stands for all rows (the reference's time embedding broadcasts over the
    batch, openai_unetmodel.py:262-271); any other length is the reference's shape error, not an out-of-bounds read."""
    t = _dev_f32(t, device).reshape(-1)
    if t.numel() == 1 and n != 1:
        t = t.expand(n).contiguous()
    if t.numel() != n:
        raise RuntimeError(f"timesteps: {t.numel()} values for a batch of {n}")
    return t


def _ilist(cls, n, vals):
    a = (C.c_int * n)()
    for i, v in enumerate(vals):
        a[i] = int(v)
    return a


def unet_config(cfg):
    u = UNetConfig()
    u.in_channels, u.out_channels = cfg["in_channels"], cfg["out_channels"]
    u.model_channels, u.num_res_blocks = cfg["model_channels"], cfg["num_res_blocks"]
    u.channel_mult = _ilist(C.c_int, 8, cfg["channel_mult"])
    u.n_mult = len(cfg["channel_mult"])
    u.attention_resolutions = _ilist(C.c_int, 8, cfg["attention_resolutions"])
    u.n_attn = len(cfg["attention_resolutions"])
    u.num_heads, u.context_dim = cfg["num_heads"], cfg["context_dim"]
    return u


TUNED_DIR = os.path.join(_HERE, "tuned")
_feat_tokens = itertools.count(1)      # process-wide: tokens of different engines / classifiers never coincide
_tuned_loaded = {}      # precision -> path of the shipped plan table imported into that library (or None)


def tuned_defaults_path(device, precision):
    """Package-data file with the autotuner's choices for this GPU model: tuned/<arch>_<CUs>cu_<precision>.txt
    (e.g. gfx950_256cu_fp16.txt; text lines 'key tile splitk gm', the df_tune_cache_export format).  None when this build
    ships no table for the device."""
    if os.environ.get("DF_TUNED_TABLE"):          # tools: A/B of two tables on one box
        return os.environ["DF_TUNED_TABLE"]
    pr = torch.cuda.get_device_properties(device)
    arch = getattr(pr, "gcnArchName", "").split(":")[0] or "unknown"
    path = os.path.join(TUNED_DIR, f"{arch}_{pr.multi_processor_count}cu_{precision}.txt")
    return path if os.path.exists(path) else None


def load_tuned_defaults(L, device, precision):
    """The shipped plan table becomes the product default (round 6): the reference has no tuning step
    (inference/diff_foley_inference.ipynb:80-95 goes straight from load_state_dict to sample), so the drop-in must run the
    benchmarked kernels without one.  The table holds, per distinct GEMM of the BASELINE shapes, the (tile, split-K, tile walk)
    the in-plan autotuner picked on an MI355X; it is imported once per process and library (df_tune_cache_import), every plan
    built afterwards takes its GEMMs' entries from it, and shapes it does not know fall back to the cost model's tiles.
    ``DF_TUNED_DEFAULTS=0`` skips the import (tests and bench.py's `modes.untuned` time the cost-model plans that way)."""
    if precision in _tuned_loaded:
        return _tuned_loaded[precision]
    path = None
    if os.environ.get("DF_TUNED_DEFAULTS", "1") != "0":
        path = tuned_defaults_path(device, precision)
        if path is not None:
            with open(path, "rb") as f:
                text = f.read()
            _chk(L.df_tune_cache_import(text, len(text)), L)
    _tuned_loaded[precision] = path
    return path


class Engine:
    """One engine context per device per process (owns packed weights and plan workspaces)."""

    def __init__(self, device=None, precision=None):
        if not torch.cuda.is_available():
            raise RuntimeError("diff_foley_amd needs a ROCm GPU (MI355X); no CPU fallback exists")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.precision = precision or default_precision()
        self.L = lib(self.precision)
        self.tuned_defaults = load_tuned_defaults(self.L, self.device, self.precision)
        self.operand_dtype = OPERAND_DTYPE[self.precision]
        h = C.c_void_p()
        _chk(self.L.df_create(self.device.index or 0, C.byref(h)), self.L)
        self._h = h
        self._keep = []
        self._last_stream = {}            # plan family -> the torch stream of its previous call (_on)
        self._cls_feat = None             # (feature tensor, (shape, dtype, version), token) of the last classifier_grad call
        self.autotune_on = False
        self.configured = Configured()

    def close(self):
        if getattr(self, "_h", None):
            self.L.df_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- model definition
    def config_unet(self, cfg):
        _chk(self.L.df_config_unet(self._h, C.byref(unet_config(cfg))), self.L)
        self.configured.record("unet", in_channels=cfg["in_channels"], out_channels=cfg["out_channels"], context_dim=cfg["context_dim"])

    def config_classifier(self, cfg):
        _chk(self.L.df_config_classifier(self._h, C.byref(unet_config(cfg))), self.L)
        self.configured.record("cls", in_channels=cfg["in_channels"], out_channels=cfg["out_channels"], context_dim=cfg["context_dim"])

    @staticmethod
    def _vae_config(cfg, scale_factor):
        v = VaeConfig()
        v.z_channels, v.embed_dim, v.ch = cfg["z_channels"], cfg["embed_dim"], cfg["ch"]
        v.num_res_blocks, v.out_ch = cfg["num_res_blocks"], cfg["out_ch"]
        v.ch_mult = _ilist(C.c_int, 8, cfg["ch_mult"])
        v.n_mult = len(cfg["ch_mult"])
        v.scale_factor = float(scale_factor)
        return v

    def _record_vae(self, cfg):
        self.configured.record("vae", z_channels=cfg["z_channels"], embed_dim=cfg["embed_dim"], out_ch=cfg["out_ch"],
                               n_mult=len(cfg["ch_mult"]))

    def config_vae(self, cfg, scale_factor):
        _chk(self.L.df_config_vae(self._h, C.byref(self._vae_config(cfg, scale_factor))), self.L)
        self._record_vae(cfg)

    def config_vae_encoder_only(self, cfg, scale_factor):
        """The VAE encoder + quant_conv in a context that never decodes (df_config_vae_encoder_only): ``cfg`` is the VAE's dict with
        ``in_channels``; no decoder tensor is loaded, and df_vae_decode refuses ("vae not configured")."""
        e = VaeEncoderConfig(int(cfg["in_channels"]))
        _chk(self.L.df_config_vae_encoder_only(self._h, C.byref(self._vae_config(cfg, scale_factor)), C.byref(e)), self.L)
        self._record_vae(cfg)
        self.configured.record("vae_encoder", in_channels=cfg["in_channels"])

    def config_vae_encoder(self, cfg):
        """cfg: dict(in_channels=...) with the encoder's tensors about to be loaded, or None: no encoder (encode raises)."""
        if cfg is None:
            _chk(self.L.df_config_vae_encoder(self._h, None), self.L)
            self.configured.drop("vae_encoder")
            return
        e = VaeEncoderConfig(int(cfg["in_channels"]))
        _chk(self.L.df_config_vae_encoder(self._h, C.byref(e)), self.L)
        self.configured.record("vae_encoder", in_channels=cfg["in_channels"])

    def config_cond(self, cfg):
        k = CondConfig(cfg["origin_dim"], cfg["embed_dim"], cfg["seq_len"])
        _chk(self.L.df_config_cond(self._h, C.byref(k)), self.L)
        self.configured.record("cond", origin_dim=cfg["origin_dim"], embed_dim=cfg["embed_dim"], seq_len=cfg["seq_len"])

    def config_cavp(self, cfg):
        k = CavpConfig((C.c_int * 4)(*cfg["stage_blocks"]), cfg["base_channels"], cfg["embed_dim"])
        _chk(self.L.df_config_cavp(self._h, C.byref(k)), self.L)
        self.configured.record("cavp", embed_dim=cfg["embed_dim"])

    def cavp_encode(self, video, normalize=True):
        """video (B,T,3,H,W) fp32 RGB in [0,1] -> (B,T,embed) (CAVP_Inference.encode_video, pool=False)."""
        video = _dev_f32(video, self.device)
        if video.ndim != 5 or video.shape[2] != 3:
            raise RuntimeError(f"cavp_encode: video must be (B,T,3,H,W), got shape {tuple(video.shape)}")
        B, T, c3, H, W = video.shape
        out = torch.empty(B, T, self.configured.of("cavp").embed_dim, device=self.device, dtype=torch.float32)
        if out.numel() == 0:              # no clips / no frames: an empty result, like the reference's Conv3d stack on an empty batch
            return out
        _chk(self.L.df_cavp_encode(self._h, _ptr(video), _ptr(out), B, T, H, W, int(bool(normalize)), self._on("cavp")), self.L)
        return out

    def cavp_encode_pooled(self, video, normalize=True, kernel=16):
        """encode_video(pool=True) (cavp_model.py:58-59): MaxPool1d(16) over the frames of the projected features, then the
        optional L2 normalisation; (B, T // 16, embed), squeezed to (B, embed) for one window like the reference's squeeze(2)."""
        return self.cavp_pool(self.cavp_encode(video, normalize=False), normalize, "encode_video", "frames", kernel)

    def cavp_pool(self, feat, normalize, what, rows, kernel=16):
        """The contrastive head of either tower on un-normalised features (B, T, C) (cavp_model.py:58-63, 77-82): MaxPool1d(kernel)
        over the rows, then the optional L2 normalisation -- df_cavp_pool.  ``what`` / ``rows`` name the caller in the messages."""
        B, T, Cc = feat.shape
        if T < kernel:
            raise RuntimeError(f"{what}(pool=True): {T} {rows} are fewer than the MaxPool1d window of {kernel}")
        if normalize and T // kernel > 1:
            # F.normalize(dim=-1) then runs over the WINDOW axis of the reference's (B, C, T // 16) tensor (squeeze(2) is a no-op
            # there) -- a shape the contrastive head is never used with; refused rather than guessed
            raise NotImplementedError(f"{what}(pool=True, normalize=True) is defined for one {kernel}-row window ({kernel}..{2 * kernel - 1} "
                                      f"{rows}): the reference normalises across the windows there")
        out = torch.empty(B, T // kernel, Cc, device=self.device, dtype=torch.float32)
        if out.numel():
            _chk(self.L.df_cavp_pool(_ptr(feat), _ptr(out), B, T, Cc, kernel, int(bool(normalize)), _stream()), self.L)
        return out[:, 0] if out.shape[1] == 1 else out.permute(0, 2, 1)      # reference layout before squeeze(2): (B, C, T/16)

    def config_cavp_spec(self, cfg):
        """cfg: dict(n_mels, channels[6], fc_dim, embed_dim) -- synth.CAVP_AUDIO_FULL is the reference's Cnn14."""
        k = CavpSpecConfig(int(cfg["n_mels"]), (C.c_int * 6)(*[int(v) for v in cfg["channels"]]), int(cfg["fc_dim"]),
                           int(cfg["embed_dim"]))
        _chk(self.L.df_config_cavp_spec(self._h, C.byref(k)), self.L)
        self.configured.record("cavp_spec", n_mels=cfg["n_mels"], channels=cfg["channels"], embed_dim=cfg["embed_dim"])

    @staticmethod
    def cavp_spec_rows(frames):
        """Output rows of a ``frames``-long mel: four floor-halvings (the (2, 2) pools of conv_block1 .. 4)."""
        return int(frames) // 2 // 2 // 2 // 2

    def _cavp_spec_input(self, spec):
        cfg = self.configured.of("cavp_spec")
        spec = _dev_f32(spec, self.device)
        if spec.ndim != 3:
            raise RuntimeError(f"encode_spec: spec must be (B, n_mels, T), got shape {tuple(spec.shape)}")
        B, M, T = spec.shape
        if M != cfg.n_mels:
            raise RuntimeError(f"encode_spec: spec has {M} mel bins, the encoder's input BatchNorm has {cfg.n_mels}")
        if self.cavp_spec_rows(T) < 1:
            raise RuntimeError(f"encode_spec: {T} frames give no output row (the four (2, 2) pools need at least 16)")
        return spec

    def cavp_spec_encode(self, spec, normalize=False):
        """spec (B, n_mels, T) fp32 normalised log-mel -> (B, T // 16, embed) (CAVP_Inference.encode_spec, pool=False)."""
        spec = self._cavp_spec_input(spec)
        B, M, T = spec.shape
        out = torch.empty(B, self.cavp_spec_rows(T), self.configured.of("cavp_spec").embed_dim, device=self.device, dtype=torch.float32)
        if B == 0:                # no clips: an empty result, like the reference's conv stack on an empty batch
            return out
        _chk(self.L.df_cavp_spec_encode(self._h, _ptr(spec), _ptr(out), B, M, T, int(bool(normalize)), self._on("cavpspec")), self.L)
        return out

    def cavp_spec_encode_tap(self, spec, tap, normalize=False):
        """Tests: (features, one ConvBlock's output as fp32 NCHW (B, C, t, mel)) -- df_test_cavp_spec_tap, tap 1 .. 6."""
        spec = self._cavp_spec_input(spec)
        B, M, T = spec.shape
        out = torch.empty(B, self.cavp_spec_rows(T), self.configured.of("cavp_spec").embed_dim, device=self.device, dtype=torch.float32)
        h, w = T, M
        for i in range(min(tap, 5)):
            h, w = (h // 2 if i < 4 else h), w // 2
        ch = self.configured.of("cavp_spec").channels[tap - 1]
        stage = torch.empty(B, h, w, ch, device=self.device, dtype=torch.float32 if tap == 6 else self.operand_dtype)
        _chk(self.L.df_test_cavp_spec_tap(self._h, _ptr(spec), _ptr(out), _ptr(stage), int(tap), B, M, T, int(bool(normalize)),
                                          self._on("cavpspec")), self.L)
        return out, stage.float().permute(0, 3, 1, 2).contiguous()

    def cavp_similarity(self, v, s, scale=1.0):
        """out[i][j] = scale * mean_t <v[i,t,:], s[j,t,:]> for v (Bv, T, D), s (Bs, T, D) -> (Bv, Bs) (df_cavp_similarity)."""
        v, s = _dev_f32(v, self.device), _dev_f32(s, self.device)
        if v.ndim != 3 or s.ndim != 3 or v.shape[1:] != s.shape[1:]:
            raise RuntimeError(f"cavp_similarity: features must be (Bv, T, D) and (Bs, T, D) with the same T and D, got "
                               f"{tuple(v.shape)} and {tuple(s.shape)}")
        out = torch.empty(v.shape[0], s.shape[0], device=self.device, dtype=torch.float32)
        if out.numel() == 0:
            return out
        _chk(self.L.df_cavp_similarity(_ptr(v), _ptr(s), _ptr(out), v.shape[0], s.shape[0], v.shape[1], v.shape[2], float(scale),
                                       _stream()), self.L)
        return out

    def load_tensor(self, name, t):
        shape = (C.c_int64 * t.dim())(*t.shape)
        if t.is_cuda:
            t = t.detach().to(torch.float32).contiguous()
            _chk(self.L.df_load_tensor_dev(self._h, name.encode(), _ptr(t), shape, t.dim()), self.L)
        else:
            t = t.detach().to(torch.float32).contiguous()
            _chk(self.L.df_load_tensor(self._h, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()), self.L)

    def finalize(self):
        _chk(self.L.df_finalize(self._h), self.L)

    def autotune(self, enable=True):
        _chk(self.L.df_autotune(self._h, int(enable)), self.L)
        self.autotune_on = bool(enable)

    def tune_cache_export(self):
        """The autotuner's choices of this process as bytes (text lines 'key tile splitk gm')."""
        n = C.c_int64()
        _chk(self.L.df_tune_cache_export(None, 0, C.byref(n)), self.L)
        buf = C.create_string_buffer(max(n.value, 1))
        _chk(self.L.df_tune_cache_export(buf, n.value, C.byref(n)), self.L)
        return buf.raw[:n.value]

    def tune_cache_import(self, text):
        _chk(self.L.df_tune_cache_import(bytes(text), len(text)), self.L)

    # ---- packed-operand blob (multi-GPU weight distribution: pack once on the root rank, broadcast, import elsewhere)
    def export_packed(self, B, H, W, T):
        """Builds every operand packing the UNet (CFG batch 2B) / VAE / cond-stage plans of this shape need and returns
        (manifest: uint8 CPU tensor, blob: uint8 tensor on the engine's device)."""
        _chk(self.L.df_prepack(self._h, B, H, W, T), self.L)
        mb, bb = C.c_size_t(), C.c_size_t()
        _chk(self.L.df_packed_size(self._h, C.byref(mb), C.byref(bb)), self.L)
        manifest = torch.empty(mb.value, dtype=torch.uint8)
        blob = torch.empty(bb.value, dtype=torch.uint8, device=self.device)
        _chk(self.L.df_export_packed(self._h, C.c_void_p(manifest.data_ptr()), _ptr(blob), _stream()), self.L)
        torch.cuda.current_stream().synchronize()
        return manifest, blob

    def import_packed(self, manifest, blob):
        manifest = manifest.cpu().contiguous()
        if blob.device != self.device:
            blob = blob.to(self.device)
        _chk(self.L.df_import_packed(self._h, C.c_void_p(manifest.data_ptr()), manifest.numel(), _ptr(blob), blob.numel(),
                                     _stream()), self.L)

    # ---- network calls (all asynchronous on the current torch stream)
    def _on(self, family):
        """The current stream's handle for a call into the plans of ``family``.  A torch module may be called from one stream after
        another without an explicit wait (its activations are fresh allocations); a plan's workspace, context operands and timestep
        table are state that lives across calls, so a call from ANOTHER stream than the family's previous one first waits for that
        stream's submitted work (one event, only when the stream changes).  Families are independent of each other -- the classifier
        gradient runs beside the UNet step on a second stream (samplers._eps_and_classifier_grad)."""
        cur = torch.cuda.current_stream(self.device)
        last = self._last_stream.get(family)
        if last is not None and last != cur:
            cur.wait_stream(last)
        self._last_stream[family] = cur
        return C.c_void_p(cur.cuda_stream)

    def cond_encode(self, feats):
        feats = _dev_f32(feats, self.device)
        B, T, D = feats.shape
        cond = self.configured.of("cond")
        _want_dim("get_learned_conditioning: video features", D, cond.origin_dim)
        if T > cond.seq_len:
            raise PositionOutOfRange(f"get_learned_conditioning: {T} frames, the positional table has {cond.seq_len} rows (index out of range)")
        out = torch.empty(B, T, cond.embed_dim, device=self.device, dtype=torch.float32)
        if out.numel() == 0:      # an empty batch / sequence gives an empty result, like the reference's Linear + pos_emb[:0]
            return out
        _chk(self.L.df_cond_encode(self._h, _ptr(feats), _ptr(out), B, T, self._on("cond")), self.L)
        return out

    def set_context(self, ctx):
        ctx = _dev_f32(ctx, self.device)
        N, T, D = ctx.shape
        _want_dim("cross-attention context", D, self.configured.of("unet").context_dim)
        if N == 0:                # empty batch: nothing to precompute (the forward calls return empty tensors)
            return
        _chk(self.L.df_unet_set_context(self._h, _ptr(ctx), N, T, self._on("unet")), self.L)

    def set_timesteps(self, timesteps, batch, H, W, cfg):
        """Hoists the time embedding of a whole sample() call out of the step loop (df_unet_set_timesteps): ``timesteps`` are
        the values the sampler is going to visit, each shared by the whole batch; afterwards ``unet_forward*(…, ts_index=i)``
        takes the table row instead of the time-embedding launches.  ``batch`` = sampler batch (the CFG plan doubles it)."""
        if int(batch) == 0:
            return
        ts = (C.c_float * len(timesteps))(*[float(v) for v in timesteps])
        _chk(self.L.df_unet_set_timesteps(self._h, ts, len(timesteps), int(batch), int(H), int(W), 1 if cfg else 0, self._on("unet")),
             self.L)

    def _unet(self, x, t, out, ts_index, scale=None):
        """unet_forward (scale None) and unet_forward_cfg: one of the four ABI entries, by guidance and by ts_index."""
        x = _dev_f32(x, self.device)
        unet = self.configured.of("unet")
        _want_nchw("UNet input", x, unet.in_channels)
        N, Cc, H, W = x.shape
        if out is None:
            out = torch.empty(N, unet.out_channels, H, W, device=self.device, dtype=torch.float32)
        if N == 0:                # an empty batch is an empty result (torch modules accept it; no plan exists for it)
            return out
        fn = getattr(self.L, "df_unet_forward" + ("" if scale is None else "_cfg") + ("" if ts_index is None else "_ts"))
        if ts_index is None:
            t = _timesteps(t, N, self.device)
        at = _ptr(t) if ts_index is None else int(ts_index)
        guidance = () if scale is None else (float(scale),)
        _chk(fn(self._h, _ptr(x), at, _ptr(out), N, H, W, *guidance, self._on("unet")), self.L)
        return out

    def unet_forward(self, x, t, out=None, ts_index=None):
        return self._unet(x, t, out, ts_index)

    def unet_forward_cfg(self, x, t, scale, out=None, ts_index=None):
        return self._unet(x, t, out, ts_index, scale)

    def vae_decode(self, z):
        z = _dev_f32(z, self.device)
        vae = self.configured.of("vae")
        _want_nchw("decode_first_stage: latent", z, vae.z_channels)
        B, Cc, H, W = z.shape
        up = 2 ** (vae.n_mult - 1)
        out = torch.empty(B, vae.out_ch, H * up, W * up, device=self.device, dtype=torch.float32)
        if B == 0:
            return out
        _chk(self.L.df_vae_decode(self._h, _ptr(z), _ptr(out), B, H, W, self._on("vae")), self.L)
        return out

    def _vae_encode_io(self, x):
        """(the image as checked fp32 NCHW on the device, the empty moments [B][2*embed_dim][H/f][W/f])."""
        x = _dev_f32(x, self.device)
        vae = self.configured.of("vae")
        _want_nchw("encode_first_stage: image", x, self.configured.of("vae_encoder").in_channels)
        B, Cc, H, W = x.shape
        f = 2 ** (vae.n_mult - 1)
        if H <= 0 or W <= 0 or H % f or W % f:
            raise RuntimeError(f"encode_first_stage: image {H}x{W} is not a positive multiple of the encoder's downsampling ({f}) "
                               "(the reference floors such maps; this engine refuses them)")
        return x, torch.empty(B, 2 * vae.embed_dim, H // f, W // f, device=self.device, dtype=torch.float32)

    def vae_encode(self, x):
        """x [B][in_channels][H][W] -> moments [B][2*embed_dim][H/f][W/f] = quant_conv(encoder(x)) (df_vae_encode)."""
        x, out = self._vae_encode_io(x)
        B, Cc, H, W = x.shape
        if B == 0:
            return out
        _chk(self.L.df_vae_encode(self._h, _ptr(x), _ptr(out), B, H, W, self._on("vaeenc")), self.L)
        return out

    def vae_encode_tap(self, x, tap, tap_hwc):
        """Tests: (moments, one intermediate stage as NCHW) of vae_encode -- df_test_vae_encode_tap; tap_hwc = (h, w, C) of the stage."""
        x, out = self._vae_encode_io(x)
        B, Cc, H, W = x.shape
        h, w, ch = tap_hwc
        stage = torch.empty(B, h, w, ch, device=self.device, dtype=torch.float32)
        _chk(self.L.df_test_vae_encode_tap(self._h, _ptr(x), _ptr(out), _ptr(stage), int(tap), B, H, W, self._on("vaeenc")), self.L)
        return out, stage.permute(0, 3, 1, 2).contiguous()

    def _cls_inputs(self, x, t, feat):
        """(x, t, feat, the record) as the classifier plans take them: fp32 on the device, checked against the configured backbone."""
        x, feat = _dev_f32(x, self.device), _dev_f32(feat, self.device)
        cls = self.configured.of("cls")
        _want_nchw("classifier input", x, cls.in_channels)
        B = x.shape[0]
        if feat.ndim != 3 or feat.shape[0] != B:
            raise RuntimeError(f"classifier video_feat: expected [{B}][frames][dim], got shape {tuple(feat.shape)}")
        _want_dim("classifier video_feat", feat.shape[2], cls.context_dim)
        return x, _timesteps(t, B, self.device), feat, cls

    def classifier_forward(self, x, t, feat):
        x, t, feat, cls = self._cls_inputs(x, t, feat)
        B, Cc, H, W = x.shape
        out = torch.empty(B, cls.out_channels, device=self.device, dtype=torch.float32)
        if B == 0:
            return out
        _chk(self.L.df_classifier_forward(self._h, _ptr(x), _ptr(t), _ptr(feat), _ptr(out), B, H, W, feat.shape[1],
                                         self._on("cls")), self.L)
        return out

    def _feat_token(self, feat):
        """Token naming the CONTENTS of the caller's feature tensor for df_classifier_grad_cached: the same token as long as the
        caller passes the very same tensor object with an unchanged version counter (a guidance loop hands origin_cond through all
        its steps: ddim.py:374-380), a new one otherwise.  Same rule as the UNet's context cache (ldm.LatentDiffusion.apply_model):
        the tensor is held by a strong reference so that its storage cannot be handed to another tensor while it is the key;
        tensors without a version counter (torch.inference_mode) get token 0 = recompute every call."""
        try:
            ver = feat._version
        except RuntimeError:
            self._cls_feat = None
            return 0
        key = (tuple(feat.shape), feat.dtype, ver)
        if self._cls_feat is None or self._cls_feat[0] is not feat or self._cls_feat[1] != key:
            self._cls_feat = (feat, key, next(_feat_tokens))
        return self._cls_feat[2]

    def classifier_grad(self, x, t, feat, want_prob=False):
        token = 0 if os.environ.get("DF_CLS_FEAT_CACHE", "1") == "0" else self._feat_token(feat)
        x, t, feat, _ = self._cls_inputs(x, t, feat)
        B, Cc, H, W = x.shape
        grad = torch.empty_like(x)
        prob = torch.empty(B, 1, device=self.device, dtype=torch.float32) if want_prob else None
        if B == 0:
            return (grad, prob) if want_prob else grad
        _chk(self.L.df_classifier_grad_cached(self._h, _ptr(x), _ptr(t), _ptr(feat), _ptr(prob) if want_prob else None,
                                             _ptr(grad), B, H, W, feat.shape[1], token, self._on("clsgrad")), self.L)
        return (grad, prob) if want_prob else grad

    def test_block(self, prefix, kind, x, semb=None, context=None, cout=None):
        """One UNet block in isolation (df_test_unet_block): x NCHW fp32 -> NCHW fp32."""
        x = _dev_f32(x, self.device)
        N, Cin, H, W = x.shape
        cout = Cin if cout is None else cout
        OH, OW = (H // 2, W // 2) if kind == 2 else ((H * 2, W * 2) if kind == 3 else (H, W))
        xin = x.permute(0, 2, 3, 1).contiguous()
        out = torch.empty(N, OH, OW, cout, device=self.device, dtype=torch.float32)
        semb = None if semb is None else _dev_f32(semb, self.device)
        context = None if context is None else _dev_f32(context, self.device)
        T = 0 if context is None else context.shape[1]
        _chk(self.L.df_test_unet_block(self._h, prefix.encode(), kind, _ptr(xin), _ptr(semb) if semb is not None else None,
                                       _ptr(context) if context is not None else None, _ptr(out), N, H, W, Cin, cout, T,
                                       self._on("unet")), self.L)
        return out.permute(0, 3, 1, 2).contiguous()

    def profile_begin(self):
        _chk(self.L.df_profile_begin(self._h), self.L)

    def profile_end(self):
        ms, cnt = (C.c_double * 5)(), (C.c_int64 * 5)()
        _chk(self.L.df_profile_end(self._h, ms, cnt), self.L)
        names = ("gemm", "attention", "groupnorm", "layernorm", "other")
        return {n: dict(ms=ms[i], launches=cnt[i]) for i, n in enumerate(names)}

    def profile_dump(self, path):
        _chk(self.L.df_profile_dump(self._h, path.encode()), self.L)

    def debug_checksums(self, enable, capacity=1 << 16):
        """Debug: checksum every plan workspace after every op (see include/df_engine.h)."""
        _chk(self.L.df_debug_checksums(self._h, int(bool(enable)), int(capacity)), self.L)

    def debug_checksums_read(self):
        n = C.c_int64()
        _chk(self.L.df_debug_checksums_read(self._h, None, 0, C.byref(n)), self.L)
        out = (C.c_uint64 * max(n.value, 1))()
        _chk(self.L.df_debug_checksums_read(self._h, out, n.value, C.byref(n)), self.L)
        return list(out[:n.value])

    def debug_checksum_label(self, i):
        buf = C.create_string_buffer(200)
        _chk(self.L.df_debug_checksum_label(self._h, int(i), buf, 200), self.L)
        return buf.value.decode()

    def debug_requant(self, prefixes=""):
        """fp16 build: re-round the operand-type outputs of the ops whose tag starts with one of ``prefixes`` (comma separated, "*" =
        all, "" = off) to bf16 precision -- tools/error_budget.py."""
        _chk(self.L.df_debug_requant(self._h, prefixes.encode()), self.L)

    def debug_saturations(self, enable, capacity=1 << 16):
        """Debug: after every op, count the operand-type values it stored at the fp16 saturation value +-65504 (fp16 build;
        non-finite values in the bf16 build) -- include/df_engine.h."""
        _chk(self.L.df_debug_saturations(self._h, int(bool(enable)), int(capacity)), self.L)

    def debug_saturations_read(self):
        """[(label, count)] of every op executed since debug_saturations(True)."""
        n = C.c_int64()
        _chk(self.L.df_debug_saturations_read(self._h, None, 0, C.byref(n)), self.L)
        out = (C.c_uint64 * max(n.value, 1))()
        _chk(self.L.df_debug_saturations_read(self._h, out, n.value, C.byref(n)), self.L)
        buf = C.create_string_buffer(200)
        res = []
        for i in range(n.value):
            _chk(self.L.df_debug_saturation_label(self._h, i, buf, 200), self.L)
            res.append((buf.value.decode(), int(out[i])))
        return res

    def debug_poison(self, enable):
        """Debug: build plan workspaces poisoned (0xFF bytes = NaN) and poison every block again where its plan releases it, so that an
        op which reads what its plan did not write in the same run produces NaN (include/df_engine.h).  Drops the cached plans."""
        _chk(self.L.df_debug_poison(self._h, int(bool(enable))), self.L)

    def poison_selftest(self, defect):
        """Tests: the four-op plan of df_test_poison_selftest with planted defect 0 (none), 1 or 2 -> its 512 outputs."""
        out = torch.empty(512, device=self.device, dtype=torch.float32)
        _chk(self.L.df_test_poison_selftest(self._h, int(defect), _ptr(out), _stream()), self.L)
        return out

    def check_saturations(self):
        """Raises if any op since debug_saturations(True) stored a saturated / non-finite operand value; names the ops."""
        bad = [(lab, n) for lab, n in self.debug_saturations_read() if n]
        if bad:
            shown = ", ".join(f"{lab}: {n}" for lab, n in bad[:8])
            raise RuntimeError(f"{self.precision} operands saturated in {len(bad)} op(s) -- {shown}"
                               + (" ..." if len(bad) > 8 else "") +
                               ("; the activations left the fp16 range (+-65504): use precision='bf16'" if self.precision == "fp16" else ""))

    def plan_count(self):
        n, b = C.c_int64(), C.c_int64()
        _chk(self.L.df_plan_count(self._h, C.byref(n), C.byref(b)), self.L)
        return n.value, b.value

    def plan_stats(self):
        n, f, w = C.c_int64(), C.c_double(), C.c_double()
        _chk(self.L.df_unet_plan_stats(self._h, C.byref(n), C.byref(f), C.byref(w)), self.L)
        return dict(launches=n.value, gemm_flops=f.value, weight_bytes=w.value)


# ---- sampler arithmetic (module-level: no ctx needed) --------------------------------------------------------
def cfg_combine(e2, scale):
    B = e2.shape[0] // 2
    e = torch.empty((B,) + tuple(e2.shape[1:]), device=e2.device, dtype=torch.float32)
    if e.numel() == 0:
        return e
    _chk(lib().df_cfg_combine(_ptr(e2), _ptr(e), e.numel(), float(scale), _stream()))
    return e


def lincomb(terms, out=None):
    """out = sum(coef * tensor) over up to 4 (coef, tensor) pairs of identical shape (fp32, contiguous)."""
    n = len(terms)
    ts = [t.contiguous() for _, t in terms]
    if out is None:
        out = torch.empty_like(ts[0])
    if out.numel() == 0:
        return out
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    coefs = (C.c_float * n)(*[float(c) for c, _ in terms])
    _chk(lib().df_lincomb(_ptr(out), ptrs, coefs, n, out.numel(), _stream()))
    return out


def _window_args(what, x, starts):
    """(x as fp32 NCHW on its device, the int32 host array of the window starts, K)."""
    if not x.is_cuda:
        raise RuntimeError(f"{what}: the tensor must live on the GPU (there is no CPU path)")
    x = _dev_f32(x, x.device)
    if x.ndim != 4:
        raise RuntimeError(f"{what}: expected a 4-D NCHW tensor, got shape {tuple(x.shape)}")
    starts = [int(s) for s in starts]
    return x, (C.c_int32 * max(len(starts), 1))(*starts), len(starts)


def window_gather(x, starts, width):
    """x [B][C][H][W] -> [B * K][C][H][width], row b * K + k = x[b, :, :, starts[k] : starts[k] + width] (df_window_gather, a copy).
    The geometry is checked by the C entry (every column covered, no window outside): a bad one raises RuntimeError, nothing runs."""
    x, arr, K = _window_args("window_gather", x, starts)
    B, Cc, H, W = x.shape
    out = torch.empty(B * K, Cc, H, max(int(width), 0), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _chk(lib().df_window_gather(_ptr(x), _ptr(out), arr, K, B, Cc * H, int(width), W, _stream()))
    return out


def window_blend(win, starts, W):
    """win [B * K][C][H][Ww] -> [B][C][H][W]: the tent-weighted mean of the windows over every column (df_window_blend; weight
    min(j + 1, Ww - j) of window column j, fp32 accumulation in ascending k, one multiply by fp32(1 / sum of weights))."""
    win, arr, K = _window_args("window_blend", win, starts)
    N, Cc, H, Ww = win.shape
    if K < 1 or N % K:
        raise RuntimeError(f"window_blend: {N} window rows are no multiple of {K} windows")
    out = torch.empty(N // K, Cc, H, max(int(W), 0), device=win.device, dtype=torch.float32)
    with torch.cuda.device(win.device):
        _chk(lib().df_window_blend(_ptr(win), _ptr(out), arr, K, N // K, Cc * H, Ww, int(W), _stream()))
    return out


def posterior_sample(moments, noise=None, scale=1.0):
    """scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) for moments [B][2 zc][H][W] = (mean | logvar), noise [B][zc][H][W]
    (DiagonalGaussianDistribution.sample, stage1_autoencoder/model.py:38-47); noise None: scale * mean."""
    B, c2, H, W = moments.shape
    if c2 % 2:
        raise ValueError(f"posterior parameters with {c2} channels (mean | logvar need an even count)")
    moments = moments.contiguous()
    z = torch.empty(B, c2 // 2, H, W, device=moments.device, dtype=torch.float32)
    if z.numel() == 0:
        return z
    if noise is not None:
        noise = _dev_f32(noise, moments.device)
        if tuple(noise.shape) != tuple(z.shape):
            raise ValueError(f"noise of shape {tuple(noise.shape)} for a posterior of shape {tuple(z.shape)}")
    _chk(lib().df_posterior_sample(_ptr(moments), _ptr(noise) if noise is not None else None, _ptr(z), B, c2 // 2, H * W,
                                   float(scale), _stream()))
    return z


def align_verdict(prob, labels, counts, pred=None):
    """One batch of the Align-Acc count (evaluation/align_acc.py:85-86, df_align_verdict): pred = round-half-even(prob),
    counts[0] += #(pred == label), counts[1] += B.  prob (B,) or (B, 1) fp32; labels the same count of values or None (all 1);
    counts an int64 device tensor of two elements that the caller zeroed.  Returns pred, shaped like prob.  No host synchronisation."""
    prob = _dev_f32(prob, prob.device)
    B = prob.numel()
    if prob.ndim > 2 or (prob.ndim == 2 and prob.shape[1] != 1):
        raise ValueError(f"align_verdict: prob must be (B,) or (B, 1), got shape {tuple(prob.shape)}")
    if counts.dtype != torch.int64 or counts.numel() != 2 or counts.device != prob.device or not counts.is_contiguous():
        raise ValueError("align_verdict: counts must be a contiguous int64 tensor of two elements on prob's device")
    if pred is None:
        pred = torch.empty_like(prob)
    elif pred.shape != prob.shape or pred.dtype != torch.float32 or pred.device != prob.device or not pred.is_contiguous():
        raise ValueError("align_verdict: pred must be a contiguous fp32 tensor of prob's shape on prob's device")
    if labels is not None:
        labels = _dev_f32(labels, prob.device).reshape(-1)
        if labels.numel() != B:
            raise ValueError(f"align_verdict: {labels.numel()} labels for {B} probabilities")
    if B == 0:
        return pred
    _chk(lib().df_align_verdict(_ptr(prob), _ptr(labels) if labels is not None else None, _ptr(pred), _ptr(counts), B, _stream()))
    return pred


def q_sample_blend(img, x0, noise, mask, sqrt_acp, sqrt_one_minus_acp):
    """img <- q_sample(x0, t) * mask + (1 - mask) * img (the samplers' inpainting blend; ddim.py:206-209, ddpm.py:279-282).
    img / x0 / noise fp32 [B][C][H][W]; mask [B][1][H][W] or [B][C][H][W]."""
    B, Cc, H, W = img.shape
    assert x0.shape == img.shape and noise.shape == img.shape, (x0.shape, noise.shape, img.shape)
    if mask.dim() != 4 or mask.shape[0] != B or mask.shape[1] not in (1, Cc) or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f"mask of shape {tuple(mask.shape)} does not match a latent of shape {tuple(img.shape)} ([B][1|C][H][W])")
    out = torch.empty_like(img)
    if out.numel() == 0:
        return out
    _chk(lib().df_q_sample_blend(_ptr(img), _ptr(x0), _ptr(noise), _ptr(mask), _ptr(out), img.numel(), Cc * H * W, H * W,
                                 int(mask.shape[1]), float(sqrt_acp), float(sqrt_one_minus_acp), _stream()))
    return out


def _timestep_indices(t, B, T, device, what):
    """t as an int64 device vector of B table indices.  A host tensor or a list is range-checked HERE (IndexError, as indexing the
    table on the host would raise) and uploaded; a device tensor is passed on unread -- no host synchronisation -- and the kernel
    answers an index outside [0, T) with NaN instead of an out-of-bounds read."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if t.is_floating_point() or t.dtype == torch.bool:
        raise TypeError(f"{what}: t must hold integer table indices, got dtype {t.dtype}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"{what}: t of shape {tuple(t.shape)}, expected ({B},) -- one table index per sample")
    if t.device.type == "cpu":
        bad = [int(v) for v in t.tolist() if not 0 <= int(v) < T]
        if bad:
            raise IndexError(f"{what}: index {bad[0]} is out of bounds for a table of {T} entries")
    return t.to(device=device, dtype=torch.int64).contiguous()


def _table(tab, device, what):
    tab = _dev_f32(tab, device)
    if tab.ndim != 1 or tab.numel() < 1:
        raise ValueError(f"{what}: a table must be a non-empty vector, got shape {tuple(tab.shape)}")
    return tab


def q_sample(x0, noise, t, sqrt_acp, sqrt_one_minus_acp):
    """out[b] = sqrt_acp[t[b]] * x0[b] + sqrt_one_minus_acp[t[b]] * noise[b] (ddpm.py:279-282, ddim.py:412-413; df_q_sample).
    x0 fp32 [B][...] on its device, noise of x0's shape, t (B,) integer indices (device tensor: not read on the host), the two tables
    fp32 vectors of one length."""
    dev = x0.device
    x0 = _dev_f32(x0, dev)
    if tuple(noise.shape) != tuple(x0.shape):
        raise ValueError(f"q_sample: noise of shape {tuple(noise.shape)}, expected {tuple(x0.shape)} (the shape of x_start)")
    noise = _dev_f32(noise, dev)
    A, S = _table(sqrt_acp, dev, "q_sample"), _table(sqrt_one_minus_acp, dev, "q_sample")
    if A.numel() != S.numel():
        raise ValueError(f"q_sample: tables of {A.numel()} and {S.numel()} entries")
    B = int(x0.shape[0]) if x0.ndim else 0
    t = _timestep_indices(t, B, A.numel(), dev, "q_sample")
    out = torch.empty_like(x0)
    if out.numel() == 0:
        return out
    _chk(lib().df_q_sample(_ptr(x0), _ptr(noise), _ptr(t), _ptr(A), _ptr(S), _ptr(out), B, out.numel() // B, A.numel(), _stream()))
    return out


LOSS_TYPES = {"l2": 0, "l1": 1}


def diffusion_loss(pred, target, t, logvar, lvlb_weights, loss_type="l2", l_simple_weight=1.0, original_elbo_weight=0.0):
    """(loss_simple [B], scalars [5]) of df_diffusion_loss, both fp32 on pred's device and not read here: the per-sample mean of
    (target - pred)^2 | |target - pred| and { mean(loss_simple), mean(loss_simple / exp(logvar[t]) + logvar[t]),
    mean(lvlb_weights[t] * loss_simple), l_simple_weight * [1] + original_elbo_weight * [2], mean(logvar) } (ddpm.py:1061-1079).
    An empty batch returns an empty loss_simple and NaN scalars (the mean of nothing), without a launch."""
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError(f"unknown loss type '{loss_type}'")
    dev = pred.device
    pred = _dev_f32(pred, dev)
    if tuple(target.shape) != tuple(pred.shape):
        raise ValueError(f"diffusion_loss: target of shape {tuple(target.shape)}, expected {tuple(pred.shape)} (the shape of pred)")
    target = _dev_f32(target, dev)
    lv, w = _table(logvar, dev, "diffusion_loss"), _table(lvlb_weights, dev, "diffusion_loss")
    if lv.numel() != w.numel():
        raise ValueError(f"diffusion_loss: tables of {lv.numel()} and {w.numel()} entries")
    B = int(pred.shape[0]) if pred.ndim else 0
    t = _timestep_indices(t, B, lv.numel(), dev, "diffusion_loss")
    loss_simple = torch.empty(B, device=dev, dtype=torch.float32)
    if pred.numel() == 0:
        return loss_simple.fill_(float("nan")), torch.full((5,), float("nan"), device=dev, dtype=torch.float32)
    scalars = torch.empty(5, device=dev, dtype=torch.float32)
    _chk(lib().df_diffusion_loss(_ptr(pred), _ptr(target), _ptr(t), _ptr(lv), _ptr(w), _ptr(loss_simple), _ptr(scalars), B,
                                 pred.numel() // B, lv.numel(), LOSS_TYPES[loss_type], float(l_simple_weight),
                                 float(original_elbo_weight), _stream()))
    return loss_simple, scalars


def dpm_data_prediction(x, eps, alpha, sigma, thresholding=False, max_val=1.0, return_s=False):
    """x0 = (x - sigma * eps) / alpha over fp32 [B][...] (dpm_solver.py:386-393); thresholding: per sample
    s = max(quantile_0.995(|x0|), max_val), x0 = clamp(x0, -s, s) / s (:394-398) -- df_dpm_data_prediction.  return_s: (x0, s [B])."""
    dev = x.device
    x = _dev_f32(x, dev)
    if tuple(eps.shape) != tuple(x.shape):
        raise ValueError(f"dpm_data_prediction: eps of shape {tuple(eps.shape)}, expected {tuple(x.shape)} (the shape of x)")
    eps = _dev_f32(eps, dev)
    B = int(x.shape[0]) if x.ndim else 0
    out = torch.empty_like(x)
    s = torch.empty(B, device=dev, dtype=torch.float32) if return_s else None
    if out.numel() > 0:
        _chk(lib().df_dpm_data_prediction(_ptr(x), _ptr(eps), _ptr(out), _ptr(s) if return_s else None, B, out.numel() // B,
                                          float(alpha), float(sigma), 1 if thresholding else 0, float(max_val), _stream()))
    return (out, s) if return_s else out


def dpm_adaptive_error(x_hi, x_lo, x_prev, atol, rtol):
    """(E [1], norm [B]) of df_dpm_adaptive_error, fp32 on x_hi's device and not read here:
    norm[b] = sqrt(mean(((x_hi - x_lo) / max(atol, rtol * max(|x_lo|, |x_prev|)))^2)), E = max_b norm[b] (dpm_solver.py:952-954)."""
    dev = x_hi.device
    x_hi = _dev_f32(x_hi, dev)
    for name, v in (("x_lo", x_lo), ("x_prev", x_prev)):
        if tuple(v.shape) != tuple(x_hi.shape):
            raise ValueError(f"dpm_adaptive_error: {name} of shape {tuple(v.shape)}, expected {tuple(x_hi.shape)} (the shape of x_hi)")
    x_lo, x_prev = _dev_f32(x_lo, dev), _dev_f32(x_prev, dev)
    B = int(x_hi.shape[0]) if x_hi.ndim else 0
    if x_hi.numel() == 0:
        raise ValueError("dpm_adaptive_error: empty input")
    norm = torch.empty(B, device=dev, dtype=torch.float32)
    out = torch.empty(1, device=dev, dtype=torch.float32)
    _chk(lib().df_dpm_adaptive_error(_ptr(x_hi), _ptr(x_lo), _ptr(x_prev), _ptr(norm), _ptr(out), B, x_hi.numel() // B, float(atol),
                                     float(rtol), _stream()))
    return out, norm


def ddim_update(x, e, a_t, a_prev, sigma_t, sqrt_one_minus_at, noise=None):
    x_prev = torch.empty_like(x)
    pred_x0 = torch.empty_like(x)
    if x.numel() == 0:
        return x_prev, pred_x0
    _chk(lib().df_ddim_update(_ptr(x), _ptr(e), _ptr(noise) if noise is not None else None, _ptr(x_prev),
                              _ptr(pred_x0), x.numel(), float(a_t), float(a_prev), float(sigma_t),
                              float(sqrt_one_minus_at), _stream()))
    return x_prev, pred_x0
