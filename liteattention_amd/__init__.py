"""liteattention_amd — MI355X-native QK-Skip attention (drop-in for ``lite_attention``).

Public surface = the reference's (/root/reference/hopper/__init__.py:4-6) plus the functional op.
Importing this package loads the HIP extension; it raises if the extension is missing.
"""
__version__ = "0.1.0"

import sys as _sys

from . import _cabi

# `python -m liteattention_amd.build` must be able to run when the library is missing or stale: it is the one
# entry point that does not load it. Everything else fails loudly here, at import — there is no CPU fallback.
_BUILDING = "liteattention_amd.build" in getattr(_sys, "orig_argv", [])
if not _BUILDING:
    _cabi.load()

if not _BUILDING:
    from .flash_attn_interface import (combine_partials, flash_attn_combine, flash_attn_func, get_tile_sizes,  # noqa: E402
                                       skip_list_stats, skip_list_stats_heads)
    from .lite_attention import LiteAttention, SeqParallelLiteAttention  # noqa: E402
    from .compat import (blockmask_to_skip_lists, fa2_flash_attn_func, flash_attn_varlen_func,  # noqa: E402
                         flash_blocksparse_attn_func, flash_blocksparse_attn_qkvpacked_func)
    from .calibration import (ErrorStats, calibrate_error_schedule, calibrate_head_thresholds, calibrate_threshold,  # noqa: E402
                              output_error)
    from .qk_prep import RopeTables, qk_prep, qk_prep_reference, rope_tables, wan_rope_parts  # noqa: E402
    from .qk_prep import E4m3Scales, descale_from_amax, qk_prep_amax, qk_prep_fp8, qk_prep_fp8_reference  # noqa: E402
    from .qk_prep import (SmoothedQK, colsum_finish, lse_unshift, qk_prep_colmean, qk_prep_smooth, qk_prep_smooth_parts,  # noqa: E402
                          qk_prep_smooth_reference)
    from .v_prep import (SmoothedV, attn_unshift, attn_unshift_reference, v_colstats, v_colstats_parts,  # noqa: E402
                         v_colstats_reference, v_shift_as_bias)
    from .v_prep import PreparedV, v_prep_tiles, v_prep_tiles_reference, v_tiles_bytes  # noqa: E402
    from .v_prep import RowScaledE4m3, attn_out_fp8, attn_out_fp8_reference  # noqa: E402
    from .token_order import TokenOrder, brick_order  # noqa: E402
    from .parallel import (HeadShardedLiteAttention, RingSeqParallelLiteAttention,  # noqa: E402
                           UlyssesLiteAttention)

__all__ = ["LiteAttention", "SeqParallelLiteAttention", "flash_attn_func", "flash_attn_combine", "combine_partials",
           "get_tile_sizes", "skip_list_stats", "fa2_flash_attn_func", "flash_attn_varlen_func",
           "flash_blocksparse_attn_func", "flash_blocksparse_attn_qkvpacked_func", "blockmask_to_skip_lists", "calibrate_threshold",
           "calibrate_error_schedule", "output_error", "ErrorStats", "skip_list_stats_heads", "calibrate_head_thresholds",
           "qk_prep", "qk_prep_reference", "rope_tables", "wan_rope_parts", "RopeTables",
           "qk_prep_fp8", "qk_prep_amax", "descale_from_amax", "qk_prep_fp8_reference", "E4m3Scales",
           "qk_prep_smooth", "qk_prep_colmean", "colsum_finish", "qk_prep_smooth_parts", "qk_prep_smooth_reference", "lse_unshift", "SmoothedQK",
           "v_colstats", "v_colstats_parts", "v_colstats_reference", "attn_unshift", "attn_unshift_reference", "v_shift_as_bias", "SmoothedV",
           "v_prep_tiles", "v_prep_tiles_reference", "v_tiles_bytes", "PreparedV",
           "attn_out_fp8", "attn_out_fp8_reference", "RowScaledE4m3",
           "TokenOrder", "brick_order",
           "HeadShardedLiteAttention", "UlyssesLiteAttention", "RingSeqParallelLiteAttention", "__version__"]
