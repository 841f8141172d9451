"""dusk_plonk_amd — MI355X-native backend for dusk-plonk's hot path.

BLS12-381 Fr NTT family (poly_commit::Fft) and the G1 MSM behind KZG commit
(zksnarks PlonkParams::commit), as hand-written HIP kernels for gfx950 behind the C ABI
in include/plk.h. See DESIGN.md.
"""
from .plonk import (  # noqa: F401
    ABI_SYMBOLS, Coefficients, Commitment, Context, Fft, OpeningKey, PLK_E_ARG, PLK_E_DEGREE,
    PLK_E_DEVICE, PLK_E_NODEV, PLK_E_OOM, PLK_OK, PlonkError, PlonkParams, PointsValue, build_info, check_build,
    debug_pairing, device_count, g1_decompress, g1_subgroup_check, g1_sum, ingest_last_ms, msm_points, msm_points_ranges, msm_sharded,
    SrsVerdict, debug_glv_split, g1_mul, g1_mul_last_ms, g2_from_bytes, g2_to_bytes,
    check_last_ms, debug_f12_op, debug_miller, debug_g1_ntt, kzg_last_open_ms,
    debug_g1_ntt_batch, debug_g1_colsum,
)
from .prover import CircuitReport, GateFailure  # noqa: F401,E402

__all__ = [
    "ABI_SYMBOLS", "Coefficients", "Commitment", "Context", "Fft", "OpeningKey", "PlonkError",
    "PlonkParams",
    "PointsValue", "build_info", "check_build", "debug_pairing", "device_count", "g1_decompress",
    "g1_subgroup_check", "g1_sum", "ingest_last_ms", "msm_points",
    "msm_points_ranges", "msm_sharded",
    "SrsVerdict", "debug_glv_split", "g1_mul", "g1_mul_last_ms", "g2_from_bytes", "g2_to_bytes",
    "CircuitReport", "GateFailure", "check_last_ms", "debug_f12_op",
    "debug_miller", "debug_g1_ntt", "kzg_last_open_ms", "debug_g1_ntt_batch", "debug_g1_colsum",
]
