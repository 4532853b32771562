"""ctypes binding of the C ABI declared in include/sbi_amd_nsf.h.

There is no CPU fallback: if the shared library cannot be loaded, or a call is
made with tensors that are not on a ROCm device, the call raises.
"""

from __future__ import annotations

import ctypes
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p
from typing import Optional

import torch

from sbi_amd import _build

_LIB: Optional[ctypes.CDLL] = None
ABI_VERSION = 119    # must equal sbi_amd_nsf_abi_version() (csrc/nsf_plan.cpp) and SBI_AMD_NSF_ABI_VERSION (include/)

E_UNSUPPORTED, E_BADARG, E_LDS = -1, -2, -3
_ERRORS = {
    E_UNSUPPORTED: "configuration not supported by the HIP kernels "
    "(need 1<=D<=64, hidden_features<=64 (<=128 for theta-dim 2..16 with x-dim<=32), num_bins in {4,5,8,10,16}, num_transforms<=16, num_blocks<=4)",
    E_BADARG: "bad argument",
    E_LDS: "configuration needs more than 160 KiB of LDS per workgroup (one transform's weight image plus the "
    "kernel's tiles must fit: e.g. with hidden_features=50, 10 bins, 2 blocks training reaches x-dim 94 at theta-dim "
    "10, x-dim 54 at theta-dim 20, theta-dim 24 with x-dim 32; hidden_features=32 reaches theta-dim 32 with x-dim 48; "
    "smaller hidden_features / theta-dim / x-dim / num_bins fit more, an embedding_net shrinks x-dim)",
}


class NSFConfigC(Structure):
    """Mirror of ``struct sbi_amd_nsf_config``."""

    _fields_ = [
        ("D", c_int32), ("C", c_int32), ("H", c_int32), ("K", c_int32), ("T", c_int32), ("NB", c_int32),
        ("tail_bound", c_float), ("min_bin_width", c_float), ("min_bin_height", c_float),
        ("min_derivative", c_float), ("lu_eps", c_float), ("ctx_layers", c_int32),
    ]


class MAFConfigC(Structure):
    """Mirror of ``struct sbi_amd_maf_config`` (include/sbi_amd_maf.h)."""

    _fields_ = [
        ("D", c_int32), ("C", c_int32), ("H", c_int32), ("K", c_int32), ("T", c_int32), ("NB", c_int32),
        ("tail_bound", c_float), ("min_bin_width", c_float), ("min_bin_height", c_float),
        ("min_derivative", c_float), ("scale_by_sqrt_hidden", c_int32), ("variant", c_int32),
    ]


class MAFAffineConfigC(Structure):
    """Mirror of ``struct sbi_amd_maf_affine_config`` (include/sbi_amd_maf_affine.h)."""

    _fields_ = [("D", c_int32), ("C", c_int32), ("H", c_int32), ("T", c_int32), ("NB", c_int32), ("epsilon", c_float)]


class MDNConfigC(Structure):
    """Mirror of ``struct sbi_amd_mdn_config`` (include/sbi_amd_mdn.h)."""

    _fields_ = [("D", c_int32), ("C", c_int32), ("H", c_int32), ("K", c_int32), ("epsilon", c_float)]


class MNLEConfigC(Structure):
    """Mirror of ``struct sbi_amd_mnle_config`` (include/sbi_amd_mnle.h)."""

    _fields_ = [("V", c_int32), ("num_categories", c_int32 * 4), ("C", c_int32), ("discrete_hidden", c_int32),
                ("discrete_blocks", c_int32), ("embedding", c_int32), ("hidden", c_int32), ("num_bins", c_int32),
                ("num_transforms", c_int32), ("context_layers", c_int32), ("log_transform", c_int32),
                ("tail_bound", c_float), ("min_bin_width", c_float), ("min_bin_height", c_float),
                ("min_derivative", c_float)]


class NREConfigC(Structure):
    """Mirror of ``struct sbi_amd_nre_config`` (include/sbi_amd_nsf.h, NRE section)."""

    _fields_ = [("D", c_int32), ("C", c_int32), ("H", c_int32), ("NB", c_int32)]


class FMPEConfigC(Structure):
    """Mirror of ``struct sbi_amd_fmpe_config`` (include/sbi_amd_fmpe.h)."""

    _fields_ = [
        ("D", c_int32), ("C", c_int32), ("H", c_int32), ("L", c_int32), ("E", c_int32),
        ("max_freq", c_float), ("noise_scale", c_float), ("ln_eps", c_float),
    ]


class NPSEConfigC(Structure):
    """Mirror of ``struct sbi_amd_npse_config`` (include/sbi_amd_npse.h)."""

    _fields_ = [
        ("net", FMPEConfigC), ("sde", c_int32), ("weight", c_int32), ("beta_min", c_float), ("beta_max", c_float),
        ("sigma_min", c_float), ("sigma_max", c_float), ("cv_threshold", c_float), ("t_min", c_float), ("t_max", c_float),
    ]


class LC2STConfigC(Structure):
    """Mirror of ``struct sbi_amd_lc2st_config`` (include/sbi_amd_lc2st.h)."""

    _fields_ = [
        ("D", c_int32), ("Dx", c_int32), ("H", c_int32), ("B", c_int32), ("lr", c_float), ("weight_decay", c_float),
        ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("patience", c_int32), ("threshold", c_float),
        ("max_epochs", c_int32),
    ]


class FCEmbedConfigC(Structure):
    """Mirror of ``struct sbi_amd_fc_embed_config`` (include/sbi_amd_embed.h)."""

    _fields_ = [("in_dim", c_int32), ("hidden", c_int32), ("out_dim", c_int32), ("num_layers", c_int32)]


class PermInvConfigC(Structure):
    """Mirror of ``struct sbi_amd_perminv_config`` (include/sbi_amd_embed.h)."""

    _fields_ = [("trial", FCEmbedConfigC), ("head", FCEmbedConfigC), ("aggregation", c_int32)]


class CNNConfigC(Structure):
    """Mirror of ``struct sbi_amd_cnn_config`` (include/sbi_amd_cnn.h)."""

    _fields_ = [("ndim", c_int32), ("in_channels", c_int32), ("spatial", c_int32 * 2), ("num_conv_layers", c_int32),
                ("out_channels", c_int32 * 4), ("kernel_size", c_int32), ("pool_kernel_size", c_int32)]


class LRUConfigC(Structure):
    """Mirror of ``struct sbi_amd_lru_config`` (include/sbi_amd_lru.h)."""

    _fields_ = [("input_dim", c_int32), ("hidden_dim", c_int32), ("state_dim", c_int32), ("num_blocks", c_int32),
                ("bidirectional", c_int32), ("aggregation", c_int32)]


class CausalCNNConfigC(Structure):
    """Mirror of ``struct sbi_amd_ccnn_config`` (include/sbi_amd_causal_cnn.h)."""

    _fields_ = [("in_channels", c_int32), ("T", c_int32), ("num_conv_layers", c_int32), ("out_channels", c_int32 * 16),
                ("dilation", c_int32 * 16), ("kernel_size", c_int32), ("pool_kernel_size", c_int32),
                ("negative_slope", c_float)]


class SCConfigC(Structure):
    """Mirror of ``struct sbi_amd_sc_config`` (include/sbi_amd_sc.h)."""

    _fields_ = [("in_channels", c_int32), ("conv_channels", c_int32), ("out_channels", c_int32), ("modes", c_int32),
                ("num_layers", c_int32), ("n_points", c_int32), ("has_positions", c_int32)]


_SIGNATURES = {
    "sbi_amd_nsf_param_count": (c_int64, [POINTER(NSFConfigC)]),
    "sbi_amd_nsf_layer_offset": (c_int64, [POINTER(NSFConfigC), c_int32]),
    "sbi_amd_nsf_lu_offset": (c_int64, [POINTER(NSFConfigC), c_int32]),
    "sbi_amd_nsf_packed_floats": (c_int64, [POINTER(NSFConfigC)]),
    "sbi_amd_nsf_pack": (c_int, [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p]),
    "sbi_amd_nsf_image_kind": (c_int, [POINTER(NSFConfigC), c_int64, c_int32]),
    "sbi_amd_nsf_set_coop_max_rows": (c_int64, [c_int64]),
    "sbi_amd_nsf_coop_selfcheck": (c_int, [POINTER(NSFConfigC)]),
    "sbi_amd_nsf_pack_images": (c_int, [POINTER(NSFConfigC), c_void_p, c_void_p, c_int32, c_void_p]),
    "sbi_amd_nsf_log_prob": (
        c_int,
        [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
         c_void_p],
    ),
    "sbi_amd_nsf_log_prob_trials_workspace_floats": (c_int64, [POINTER(NSFConfigC), c_int64, c_int64]),
    "sbi_amd_nsf_log_prob_trials": (
        c_int,
        [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
         c_void_p],
    ),
    "sbi_amd_nsf_sample": (
        c_int,
        [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
         c_void_p],
    ),
    "sbi_amd_nsf_train_workspace_floats": (c_int64, [POINTER(NSFConfigC), c_int64]),
    "sbi_amd_nsf_loss_fwd_bwd": (
        c_int,
        [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
         c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_nsf_train_forward": (
        c_int,
        [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
         c_void_p],
    ),
    "sbi_amd_nsf_train_backward": (
        c_int,
        [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_float,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_adam_clip_step": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float, c_float, c_float,
         c_void_p, c_void_p],
    ),
    "sbi_amd_nsf_train_sqnorm_parts": (c_void_p, [POINTER(NSFConfigC), c_int64, c_void_p, POINTER(c_int64)]),
    "sbi_amd_adam_clip_step_parts": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float, c_float, c_float,
         c_void_p, c_int64, c_void_p, c_void_p],
    ),
    "sbi_amd_nsf_step_map_ints": (c_int64, [POINTER(NSFConfigC)]),
    "sbi_amd_nsf_step_map_workspace_floats": (c_int64, [POINTER(NSFConfigC)]),
    "sbi_amd_nsf_build_step_map": (
        c_int, [POINTER(NSFConfigC), c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_nsf_table_pack": (c_int, [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_nsf_release_step_map": (c_int, [c_void_p]),
    "sbi_amd_rccl_unique_id_bytes": (c_int32, []),
    "sbi_amd_rccl_unique_id": (c_int, [c_void_p]),
    "sbi_amd_rccl_comm_init": (c_int, [POINTER(c_void_p), c_int32, c_int32, c_void_p]),
    "sbi_amd_rccl_comm_destroy": (c_int, [c_void_p]),
    "sbi_amd_allreduce_flat": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "sbi_amd_mcmc_slice_run": (
        c_int,
        [POINTER(NSFConfigC), c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_int32, c_int32, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_atomic_atoms": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_atomic_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p,
                                       c_void_p]),
    "sbi_amd_accept_compact_scan_words": (c_int64, [c_int64, c_int32]),
    "sbi_amd_accept_compact": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p,
         c_void_p, ctypes.c_uint32, c_void_p],
    ),
    "sbi_amd_shuffled_gather": (
        c_int,
        [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64, c_uint64, c_int64, c_int64, c_void_p, c_void_p,
         c_void_p, c_void_p],
    ),
    "sbi_amd_rq_spline": (
        c_int,
        [c_int32, c_int32, c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
         c_void_p],
    ),
    "sbi_amd_mcmc_slice_tick": (
        c_int,
        [c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_int32, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p],
    ),
    "sbi_amd_mcmc_to_constrained": (
        c_int,
        [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_fmpe_param_count": (c_int64, [POINTER(FMPEConfigC)]),
    "sbi_amd_fmpe_param_offset": (c_int64, [POINTER(FMPEConfigC), c_int32, c_int32]),
    "sbi_amd_fmpe_packed_floats": (c_int64, [POINTER(FMPEConfigC)]),
    "sbi_amd_fmpe_pack": (c_int, [POINTER(FMPEConfigC), c_void_p, c_void_p, c_void_p]),
    "sbi_amd_fmpe_velocity": (
        c_int,
        [POINTER(FMPEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
         c_void_p, c_void_p],
    ),
    "sbi_amd_fmpe_velocity_div": (
        c_int,
        [POINTER(FMPEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
         c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_fmpe_loss": (
        c_int,
        [POINTER(FMPEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_void_p, c_void_p],
    ),
    "sbi_amd_fmpe_train_workspace_floats": (c_int64, [POINTER(FMPEConfigC), c_int64]),
    "sbi_amd_fmpe_loss_fwd_bwd": (
        c_int,
        [POINTER(FMPEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
         c_int64, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_dopri5_init": (c_int, [c_void_p, c_double, c_double, c_double, c_double, c_double, c_void_p]),
    "sbi_amd_dopri5_stage": (c_int, [c_void_p, POINTER(c_void_p), c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "sbi_amd_dopri5_finish": (c_int, [c_void_p, c_void_p, POINTER(c_void_p), c_void_p, c_void_p, c_int64, c_void_p]),
    "sbi_amd_maf_param_count": (c_int64, [POINTER(MAFConfigC)]),
    "sbi_amd_maf_packed_floats": (c_int64, [POINTER(MAFConfigC)]),
    "sbi_amd_maf_param_offset": (c_int64, [POINTER(MAFConfigC), c_int32, c_int32, c_int32]),
    "sbi_amd_maf_pack": (c_int, [POINTER(MAFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_maf_log_prob": (
        c_int,
        [POINTER(MAFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_maf_sample": (
        c_int,
        [POINTER(MAFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_maf_plan_waves": (c_int32, [POINTER(MAFConfigC), c_int64]),
    "sbi_amd_maf_train_workspace_floats": (c_int64, [POINTER(MAFConfigC), c_int64]),
    "sbi_amd_maf_loss_fwd_bwd": (
        c_int,
        [POINTER(MAFConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_float,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_nsf_plan_waves": (c_int, [POINTER(NSFConfigC), c_int64, c_int32]),
    "sbi_amd_nre_param_count": (c_int64, [POINTER(NREConfigC)]),
    "sbi_amd_nre_param_offset": (c_int64, [POINTER(NREConfigC), c_int32, c_int32]),
    "sbi_amd_nre_packed_floats": (c_int64, [POINTER(NREConfigC)]),
    "sbi_amd_nre_pack": (c_int, [POINTER(NREConfigC), c_void_p, c_void_p, c_void_p]),
    "sbi_amd_nre_log_ratio": (
        c_int, [POINTER(NREConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "sbi_amd_nre_log_ratio_trials_workspace_floats": (c_int64, [POINTER(NREConfigC), c_int64, c_int64]),
    "sbi_amd_nre_log_ratio_trials": (
        c_int,
        [POINTER(NREConfigC), c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
         c_void_p],
    ),
    "sbi_amd_nre_train_workspace_floats": (c_int64, [POINTER(NREConfigC), c_int64]),
    "sbi_amd_nre_train_forward": (
        c_int,
        [POINTER(NREConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_nre_loss_weights": (
        c_int, [c_int32, c_void_p, c_int32, c_int32, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_nre_train_backward": (
        c_int, [POINTER(NREConfigC), c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_nre_mcmc_slice_run": (
        c_int,
        [POINTER(NREConfigC), c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_int32, c_int32,
         c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int32, c_void_p],
    ),
    "sbi_amd_nsf_abi_version": (c_int, []),
    "sbi_amd_nsf_arch": (c_char_p, []),
}


# include/sbi_amd_npse.h (the NPSE path; `exported_symbols_npse()` is what its header is checked against)
_SIGNATURES_NPSE = {
    "sbi_amd_npse_score": (
        c_int,
        [POINTER(NPSEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32,
         c_void_p, c_void_p],
    ),
    "sbi_amd_npse_loss": (
        c_int,
        [POINTER(NPSEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_void_p, c_void_p],
    ),
    "sbi_amd_npse_train_workspace_floats": (c_int64, [POINTER(NPSEConfigC), c_int64]),
    "sbi_amd_npse_loss_fwd_bwd": (
        c_int,
        [POINTER(NPSEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
         c_int64, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_npse_sample_sde": (
        c_int,
        [POINTER(NPSEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_float, c_void_p,
         c_uint64, c_int64, c_int64, c_void_p, c_void_p],
    ),
}


# include/sbi_amd_npse_iid.h (NPSE with iid observations: the composed score and its sampler)
_SIGNATURES_NPSE_IID = {
    "sbi_amd_npse_iid_workspace_floats": (c_int64, [POINTER(NPSEConfigC), c_int64]),
    "sbi_amd_npse_score_iid": (
        c_int,
        [POINTER(NPSEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
         c_int64, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_npse_compose_iid": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32,
                                         c_void_p, c_void_p]),
    "sbi_amd_npse_sde_normals": (c_int, [c_uint64, c_int64, c_int32, c_int64, c_int32, c_void_p, c_void_p]),
    "sbi_amd_npse_sample_sde_iid": (
        c_int,
        [POINTER(NPSEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_float, c_void_p,
         c_void_p, c_void_p, c_void_p, c_uint64, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    ),
}


# include/sbi_amd_lc2st.h (the L-C2ST classifier ensemble; `exported_symbols_lc2st()` is what its header is checked against)
_SIGNATURES_LC2ST = {
    "sbi_amd_lc2st_param_count": (c_int64, [POINTER(LC2STConfigC)]),
    "sbi_amd_lc2st_train_epochs": (
        c_int,
        [POINTER(LC2STConfigC), c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
         c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_int32, c_void_p],
    ),
    "sbi_amd_lc2st_batch_grad": (
        c_int,
        [POINTER(LC2STConfigC), c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
         c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p],
    ),
    "sbi_amd_lc2st_eval": (
        c_int,
        [POINTER(LC2STConfigC), c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p,
         c_void_p],
    ),
}


# include/sbi_amd_mdn.h (the mixture-density-network posterior estimator)
_SIGNATURES_MDN = {
    "sbi_amd_mdn_param_count": (c_int64, [POINTER(MDNConfigC)]),
    "sbi_amd_mdn_packed_floats": (c_int64, [POINTER(MDNConfigC)]),
    "sbi_amd_mdn_param_offset": (c_int64, [POINTER(MDNConfigC), c_int32, c_int32]),
    "sbi_amd_mdn_pack": (c_int, [POINTER(MDNConfigC), c_void_p, c_void_p, c_void_p]),
    "sbi_amd_mdn_components": (
        c_int, [POINTER(MDNConfigC), c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_mdn_log_prob": (
        c_int, [POINTER(MDNConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "sbi_amd_mdn_sample": (
        c_int,
        [POINTER(MDNConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
         c_void_p]),
    "sbi_amd_mdn_train_workspace_floats": (c_int64, [POINTER(MDNConfigC), c_int64]),
    "sbi_amd_mdn_loss_fwd_bwd": (
        c_int,
        [POINTER(MDNConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_float, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p]),
}


# include/sbi_amd_mnle.h (mixed discrete / continuous likelihood estimator)
_SIGNATURES_MNLE = {
    "sbi_amd_mnle_param_count": (c_int64, [POINTER(MNLEConfigC)]),
    "sbi_amd_mnle_packed_floats": (c_int64, [POINTER(MNLEConfigC)]),
    "sbi_amd_mnle_param_offset": (c_int64, [POINTER(MNLEConfigC), c_int32, c_int32]),
    "sbi_amd_mnle_pack": (c_int, [POINTER(MNLEConfigC), c_void_p, c_void_p, c_void_p]),
    "sbi_amd_mnle_log_prob": (
        c_int,
        [POINTER(MNLEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32,
         c_void_p, c_void_p, c_void_p]),
    "sbi_amd_mnle_log_prob_trials": (
        c_int,
        [POINTER(MNLEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
         c_void_p, c_void_p]),
    "sbi_amd_mnle_sample": (
        c_int,
        [POINTER(MNLEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
         c_void_p]),
    "sbi_amd_mnle_train_workspace_floats": (c_int64, [POINTER(MNLEConfigC), c_int64]),
    "sbi_amd_mnle_loss_fwd_bwd": (
        c_int,
        [POINTER(MNLEConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
         c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

_AFFP = POINTER(MAFAffineConfigC)
_SIGNATURES_MAF_AFFINE = {
    "sbi_amd_maf_affine_param_count": (c_int64, [_AFFP]),
    "sbi_amd_maf_affine_packed_floats": (c_int64, [_AFFP]),
    "sbi_amd_maf_affine_param_offset": (c_int64, [_AFFP, c_int32, c_int32, c_int32]),
    "sbi_amd_maf_affine_plan_waves": (c_int32, [_AFFP, c_int64, c_int32]),
    "sbi_amd_maf_affine_pack": (c_int, [_AFFP, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_maf_affine_log_prob": (
        c_int, [_AFFP, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_maf_affine_sample": (
        c_int, [_AFFP, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_maf_affine_train_workspace_floats": (c_int64, [_AFFP, c_int64]),
    "sbi_amd_maf_affine_loss_fwd_bwd": (
        c_int,
        [_AFFP, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_float, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_maf_affine_log_prob_trials": (
        c_int, [_AFFP, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
}

# include/sbi_amd_sir.h (the selection step of sampling-importance-resampling)
_SIGNATURES_SIR = {
    "sbi_amd_sir_resample": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_vi.h (the Gaussian variational family of VIPosterior: draw, log_prob, one optimiser iteration)
class VIConfigC(Structure):
    """Mirror of ``struct sbi_amd_vi_config`` (include/sbi_amd_vi.h)."""

    _fields_ = [("D", c_int32), ("full_cov", c_int32), ("method", c_int32), ("K", c_int32),
                ("stick_the_landing", c_int32), ("dreg", c_int32), ("unbiased", c_int32), ("alpha", c_float)]


_SIGNATURES_VI = {
    "sbi_amd_vi_gauss_plan": (c_int, [c_int32, c_int64, POINTER(c_int64)]),
    "sbi_amd_vi_gauss_draw": (
        c_int,
        [c_int32, c_int32, c_void_p, c_void_p, c_int64, c_uint64, ctypes.c_uint32, c_uint64, c_void_p, c_void_p,
         c_void_p, c_void_p]),
    "sbi_amd_vi_gauss_log_prob": (c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "sbi_amd_vi_gauss_step": (
        c_int,
        [POINTER(VIConfigC), c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
         c_float, c_float, c_float, c_float, c_int64, c_uint64, ctypes.c_uint32, c_void_p, c_void_p, c_int32,
         c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_mmd.h (RBF-kernel two-sample sums: the misspecification test's permutation baseline, the MMD metrics)
_SIGNATURES_MMD = {
    "sbi_amd_mmd_rbf_splits": (
        c_int,
        [c_void_p, c_int64, c_int32, c_void_p, c_uint64, c_uint64, c_int64, c_int32, c_int32, c_int32, c_int32,
         c_void_p, c_float, c_void_p, c_void_p]),
}

# include/sbi_amd_abc.h (ABC: the pairwise mixture log-sum-exp of the SMC weights / the KDE, the persistent Sinkhorn)
_SIGNATURES_ABC = {
    "sbi_amd_mixture_lse": (
        c_int,
        [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
         c_void_p, c_void_p, c_void_p]),
    "sbi_amd_sinkhorn": (
        c_int,
        [c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_float,
         c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_mog.h (NPE-A: the analytic MoG proposal correction, log_prob / sample of an arbitrary mixture)
_SIGNATURES_MOG = {
    "sbi_amd_mog_correct_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32, c_int32, c_int64]),
    "sbi_amd_mog_correct": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
         c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_mog_log_prob": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p,
         c_void_p, c_void_p]),
    "sbi_amd_mog_sample": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_embed.h (the embedding nets: FCEmbedding, PermutationInvariantEmbedding)
_FCEP, _PIP = POINTER(FCEmbedConfigC), POINTER(PermInvConfigC)
_SIGNATURES_EMBED = {
    "sbi_amd_embed_param_count": (c_int64, [_FCEP, POINTER(c_int64)]),
    "sbi_amd_embed_workspace_bytes": (c_int64, [_FCEP, c_int64]),
    "sbi_amd_embed_plan": (c_int, [_FCEP, c_int64, c_int64, POINTER(c_int32), POINTER(c_int32)]),
    "sbi_amd_fc_embed_forward": (c_int, [_FCEP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "sbi_amd_fc_embed_backward": (
        c_int, [_FCEP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_perminv_forward": (
        c_int, [_PIP, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_perminv_backward": (
        c_int,
        [_PIP, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p]),
}

# include/sbi_amd_cnn.h (the convolution stack of CNNEmbedding)
_CNNP = POINTER(CNNConfigC)
_SIGNATURES_CNN = {
    "sbi_amd_cnn_param_count": (c_int64, [_CNNP, POINTER(c_int64)]),
    "sbi_amd_cnn_feature_count": (c_int64, [_CNNP]),
    "sbi_amd_cnn_plan": (c_int, [_CNNP, c_int64, POINTER(c_int32), POINTER(c_int32)]),
    "sbi_amd_cnn_workspace_bytes": (c_int64, [_CNNP, c_int64]),
    "sbi_amd_cnn_forward": (c_int, [_CNNP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "sbi_amd_cnn_backward": (c_int, [_CNNP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_lru.h (the recurrent stack of LRUEmbedding)
_LRUP = POINTER(LRUConfigC)
_SIGNATURES_LRU = {
    "sbi_amd_lru_param_count": (c_int64, [_LRUP, POINTER(c_int64)]),
    "sbi_amd_lru_plan": (c_int, [_LRUP, c_int64, c_int64, POINTER(c_int32), POINTER(c_int32)]),
    "sbi_amd_lru_workspace_bytes": (c_int64, [_LRUP, c_int64, c_int64, c_int32]),
    "sbi_amd_lru_forward": (c_int, [_LRUP, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_lru_backward": (
        c_int, [_LRUP, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_causal_cnn.h (the dilated causal stack + average pool of CausalCNNEmbedding)
_CCNNP = POINTER(CausalCNNConfigC)
_SIGNATURES_CAUSAL_CNN = {
    "sbi_amd_ccnn_param_count": (c_int64, [_CCNNP, POINTER(c_int64)]),
    "sbi_amd_ccnn_plan": (c_int, [_CCNNP, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "sbi_amd_ccnn_workspace_bytes": (c_int64, [_CCNNP, c_int64]),
    "sbi_amd_ccnn_forward": (c_int, [_CCNNP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "sbi_amd_ccnn_backward": (c_int, [_CCNNP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_sc.h (SpectralConvEmbedding, the whole module)
_SCP = POINTER(SCConfigC)
_SIGNATURES_SC = {
    "sbi_amd_sc_param_count": (c_int64, [_SCP, POINTER(c_int64)]),
    "sbi_amd_sc_plan": (c_int, [_SCP, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "sbi_amd_sc_workspace_bytes": (c_int64, [_SCP, c_int64]),
    "sbi_amd_sc_forward": (
        c_int, [_SCP, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "sbi_amd_sc_backward": (
        c_int,
        [_SCP, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
         c_void_p]),
}

# include/sbi_amd_tr.h (TransformerEmbedding in series mode)
class TRConfigC(Structure):
    """Mirror of ``struct sbi_amd_tr_config`` (include/sbi_amd_tr.h)."""

    _fields_ = [("feature_space_dim", c_int32), ("num_attention_heads", c_int32), ("num_key_value_heads", c_int32),
                ("head_dim", c_int32), ("intermediate_size", c_int32), ("num_hidden_layers", c_int32),
                ("final_emb_dimension", c_int32), ("pos_emb", c_int32), ("activation", c_int32),
                ("is_causal", c_int32), ("scalar_input", c_int32), ("rms_norm_eps", ctypes.c_float),
                ("div_term", ctypes.c_float * 32)]


_TRP = POINTER(TRConfigC)
_SIGNATURES_TR = {
    "sbi_amd_tr_param_count": (c_int64, [_TRP, POINTER(c_int64)]),
    "sbi_amd_tr_plan": (c_int, [_TRP, c_int64, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "sbi_amd_tr_workspace_bytes": (c_int64, [_TRP, c_int64, c_int64, c_int32]),
    "sbi_amd_tr_forward": (
        c_int, [_TRP, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, ctypes.c_float, ctypes.c_uint64,
                c_void_p, c_void_p, c_int32, c_void_p]),
    "sbi_amd_tr_backward": (
        c_int, [_TRP, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, ctypes.c_float, ctypes.c_uint64,
                c_void_p, c_void_p, c_void_p, c_void_p]),
    "sbi_amd_tr_dropout_mask": (
        c_int, [_TRP, c_int64, c_int64, ctypes.c_float, ctypes.c_uint64, c_int32, c_void_p, c_void_p]),
}

# include/sbi_amd_resnet.h (the trunk of ResNetEmbedding1D)
class ResNetConfigC(Structure):
    """Mirror of ``struct sbi_amd_resnet_config`` (include/sbi_amd_resnet.h)."""

    _fields_ = [("c_in", c_int32), ("c_internal", c_int32), ("c_hidden", c_int32), ("n_blocks", c_int32)]


_RNP = POINTER(ResNetConfigC)
_SIGNATURES_RESNET = {
    "sbi_amd_resnet_param_count": (c_int64, [_RNP, POINTER(c_int64)]),
    "sbi_amd_resnet_plan": (c_int, [_RNP, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "sbi_amd_resnet_workspace_bytes": (c_int64, [_RNP, c_int64, c_int32]),
    "sbi_amd_resnet_forward": (c_int, [_RNP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    "sbi_amd_resnet_backward": (
        c_int, [_RNP, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/sbi_amd_cond.h (conditional-density grids: fill, fp64 moments / correlation coefficient, conditioned expand)
_SIGNATURES_COND = {
    "sbi_amd_cond_grid_fill": (
        c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_void_p, c_void_p]),
    "sbi_amd_cond_grid_moments": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
         c_void_p]),
    "sbi_amd_cond_expand": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
}


def exported_symbols():
    return list(_SIGNATURES)


def exported_symbols_cond():
    return list(_SIGNATURES_COND)


def exported_symbols_embed():
    return list(_SIGNATURES_EMBED)


def exported_symbols_cnn():
    return list(_SIGNATURES_CNN)


def exported_symbols_lru():
    return list(_SIGNATURES_LRU)


def exported_symbols_causal_cnn():
    return list(_SIGNATURES_CAUSAL_CNN)


def exported_symbols_sc():
    return list(_SIGNATURES_SC)


def exported_symbols_resnet():
    return list(_SIGNATURES_RESNET)


def exported_symbols_mmd():
    return list(_SIGNATURES_MMD)


def exported_symbols_abc():
    return list(_SIGNATURES_ABC)


def exported_symbols_vi():
    return list(_SIGNATURES_VI)


def exported_symbols_sir():
    return list(_SIGNATURES_SIR)


def exported_symbols_maf_affine():
    return list(_SIGNATURES_MAF_AFFINE)


def exported_symbols_mnle():
    return list(_SIGNATURES_MNLE)


def exported_symbols_mdn():
    return list(_SIGNATURES_MDN)


def exported_symbols_mog():
    return list(_SIGNATURES_MOG)


def exported_symbols_lc2st():
    return list(_SIGNATURES_LC2ST)


def exported_symbols_npse():
    return list(_SIGNATURES_NPSE)


def exported_symbols_npse_iid():
    return list(_SIGNATURES_NPSE_IID)


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load libsbi_amd_nsf.so (building it in-tree with hipcc if needed)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB_PATH
    import os

    override = os.environ.get("SBI_AMD_LIB")
    if override:      # developer aid (the -DNSF_DEBUG build of tools/timeline.py): never silent
        import sys

        print(f"sbi_amd: WARNING: SBI_AMD_LIB={override}: loading a non-default kernel library "
              "(debug / timing build: results may be INVALID)", file=sys.stderr)
        path = _build.Path(override)
        build_if_missing = False
        if not path.exists():
            raise RuntimeError(f"SBI_AMD_LIB={override} does not exist")
    if override:
        pass
    elif not path.exists() and not build_if_missing:
        raise RuntimeError(f"{path} is missing; run `python -c 'import __graft_entry__ as g; g.build()'`")
    if build_if_missing:
        try:
            _build.build()      # no-op when the library matches the sources on disk (content hash, file-locked)
        except _build.HipccMissing as e:
            # a machine with a prebuilt library but no hipcc must stay usable -- but only with a library that was built
            # from THESE sources: kernel / packed-image layouts change without an ABI-version bump, so the stored
            # content hash is compared whenever it exists, and a library without one is loaded with a loud warning
            if not path.exists():
                raise
            import warnings

            if _build.HASH_PATH.exists():
                if _build.HASH_PATH.read_text().strip() != _build.source_hash():
                    raise RuntimeError(f"{path} was built from different sources than the ones on disk and cannot be "
                                       f"rebuilt here ({e}); refusing to load a stale kernel library") from e
            else:
                warnings.warn(f"sbi_amd: {path.name} has no source hash next to it and cannot be checked against the "
                              f"sources ({e}); loading it as is (only the ABI version is verified)", stacklevel=2)
    elif not override and _build.needs_build():
        raise RuntimeError(f"{path} is stale (built from different sources); rebuild it with "
                           "`python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(str(path))
    for name, (restype, argtypes) in {**_SIGNATURES, **_SIGNATURES_NPSE, **_SIGNATURES_NPSE_IID, **_SIGNATURES_LC2ST, **_SIGNATURES_MDN,
                                      **_SIGNATURES_MNLE, **_SIGNATURES_MAF_AFFINE, **_SIGNATURES_SIR,
                                      **_SIGNATURES_MMD, **_SIGNATURES_ABC, **_SIGNATURES_MOG,
                                      **_SIGNATURES_EMBED, **_SIGNATURES_COND, **_SIGNATURES_CNN, **_SIGNATURES_LRU,
                                      **_SIGNATURES_CAUSAL_CNN, **_SIGNATURES_SC, **_SIGNATURES_TR, **_SIGNATURES_RESNET,
                                      **_SIGNATURES_VI}.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.sbi_amd_nsf_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {got}, this binding expects {ABI_VERSION} (stale library?)")
    _LIB = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError(f"sbi_amd: {what}: {_ERRORS.get(rc, rc)}")
    raise RuntimeError(f"sbi_amd: {what}: HIP error {rc}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_device(*tensors: torch.Tensor) -> torch.device:
    """All tensors must live on one ROCm device, fp32, contiguous."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "sbi_amd: the NSF hot path runs only on a ROCm device (MI355X); got a "
                f"{t.device} tensor. There is deliberately no CPU fallback."
            )
        if t.dtype != torch.float32:
            raise TypeError(f"sbi_amd: expected float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError("sbi_amd: expected contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"sbi_amd: tensors on different devices ({dev} vs {t.device})")
    assert dev is not None
    return dev


def current_stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream
