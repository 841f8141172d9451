"""Host-side mirror of the reference's hot-path interface, over the C ABI (include/plk.h).

The reference exposes the path through Rust structs of un-vendored crates:
``poly_commit::Fft`` (new / dft / idft / coset_dft / coset_idft / size / size_inv /
generator / generator_inv / elements / compute_vanishing_poly_over_coset),
``Coefficients`` / ``PointsValue`` (``pub Vec<F>`` newtypes), and
``zksnarks::plonk::PlonkParams`` (setup / trim / commit). This module keeps those names,
argument meanings and error behaviour:

* NTT calls are infallible for valid lengths and take their input "by value" (a new
  array is returned, the argument is not modified), as the Rust API moves its ``Vec``.
* ``PlonkParams.commit`` raises :class:`PlonkError` with ``status == PLK_E_DEGREE`` when
  the polynomial (trailing zeros ignored) is longer than the trimmed SRS — the only way
  the reference's ``create_proof`` fails on an unsatisfied circuit (prover.rs:262-265).

Field elements are ``numpy.uint64`` arrays of shape ``[n, 4]`` holding Montgomery-form
limbs (R = 2^256, exactly the reference's in-memory ``BlsScalar``); G1 points are
``[n, 13]`` (Montgomery Fp x, y, infinity flag). There is no CPU fallback: without the
HIP library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
# PLK_LIB: an alternative build of the same library (tools/ A/B experiments)
_LIB_PATH = Path(os.environ["PLK_LIB"]) if os.environ.get("PLK_LIB") else _PKG / "libplk.so"

PLK_OK, PLK_E_DEGREE, PLK_E_ARG, PLK_E_DEVICE, PLK_E_OOM, PLK_E_NODEV = range(6)

# the entry points of csrc/srs_io.hip: an SRS and an opening key from bytes, the SRS fold and its
# verification (bound only when the loaded library has them: a PLK_LIB build may be older)
_SRS_IO_SYMBOLS = (
    "plk_srs_load_bytes", "plk_srs_export_bytes", "plk_srs_last_load_ms", "plk_srs_fold",
    "plk_srs_verify", "plk_srs_last_verify_ms", "plk_opening_key_load_bytes",
    "plk_opening_key_to_bytes", "plk_debug_srs_weights", "plk_debug_f2_sqrt",
)

# the entry points of csrc/g1_mul.hip and the SRS update of csrc/srs_io.hip (bound only when the
# loaded library has them, as above)
_SRS_UPDATE_SYMBOLS = (
    "plk_g1_mul_batch", "plk_g1_mul_last_ms", "plk_opening_key_update", "plk_srs_update",
    "plk_srs_verify_update", "plk_g2_to_bytes", "plk_g2_from_bytes", "plk_debug_glv_split",
)

# the entry points of csrc/circuit_check.hip (bound only when the loaded library has them, as above)
_CHECK_SYMBOLS = ("plk_composer_check", "plk_prover_diagnose", "plk_key_diagnose", "plk_check_last_ms")

# the entry points of csrc/kzg.hip and csrc/g1_ntt.hip (bound only when the loaded library has
# them, as above)
_KZG_SYMBOLS = ("plk_kzg_open", "plk_kzg_open_domain", "plk_kzg_last_open_ms", "plk_kzg_fold",
                "plk_debug_g1_ntt", "plk_kzg_open_cosets", "plk_kzg_fold_cosets",
                "plk_debug_g1_ntt_batch", "plk_debug_g1_colsum")

# the MSM stage snapshot of csrc/debug.hip (bound only when the loaded library has it, as above)
_MSM_DEBUG_SYMBOLS = ("plk_debug_msm_snapshot",)
# the MSM table's layout report and policy (csrc/api.hip; optional in the same way)
_MSM_LAYOUT_SYMBOLS = ("plk_srs_table_layout", "plk_msm_table_policy")

# Symbols declared in include/plk.h (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    "plk_abi_version", "plk_status_str", "plk_build_info", "plk_device_count", "plk_ctx_create",
    "plk_ctx_destroy", "plk_ctx_stream", "plk_ctx_synchronize", "plk_domain_get",
    "plk_domain_info", "plk_domain_elements", "plk_domain_vanishing_over_coset", "plk_ntt",
    "plk_ntt_dev", "plk_ntt_batch_dev", "plk_srs_setup", "plk_srs_load", "plk_srs_destroy",
    "plk_srs_len", "plk_srs_points", "plk_msm", "plk_commit", "plk_commit_dev",
    "plk_srs_last_msm_stats", "plk_debug_field_op", "plk_debug_rx_op", "plk_debug_g1r_op",
    "plk_debug_block_eval", "plk_debug_ntt_lazy_op", "plk_debug_prover_stage", "plk_debug_prover_round3",
    "plk_commit_batch_dev",
    "plk_commit_batch_dev_part",
    "plk_srs_setup_range", "plk_g1_sum", "plk_msm_sharded", "plk_srs_msm_stats_reset",
    "plk_srs_cum_msm_stats", "plk_ntt_stream", "plk_aggregate_witness",
    "plk_aggregate_witness_dev",
    # prover (dusk-plonk_amd/prover.py binds these)
    "plk_composer_create", "plk_composer_destroy", "plk_composer_size",
    "plk_composer_append_witness", "plk_composer_witness_value", "plk_composer_set_witness",
    "plk_composer_append_public", "plk_composer_append_gate", "plk_composer_append_custom_gate",
    "plk_composer_gate_eval", "plk_composer_assert_equal", "plk_composer_assert_equal_constant",
    "plk_composer_component_boolean", "plk_composer_component_range",
    "plk_composer_synthetic_chain",
    "plk_composer_public_inputs", "plk_composer_export", "plk_key_compile", "plk_key_destroy",
    "plk_key_info",
    "plk_prove", "plk_prover_create", "plk_prover_destroy", "plk_prover_stream",
    "plk_prover_prove", "plk_prover_msm_stats", "plk_prover_shard", "plk_prover_shard_buckets",
    "plk_proof_encode", "plk_proof_decode",
    # variable-base MSM and the verifier (Verifier in dusk-plonk_amd/prover.py)
    "plk_msm_points", "plk_msm_points_ranges", "plk_verifier_create", "plk_verifier_destroy",
    "plk_verifier_challenges", "plk_verifier_fold", "plk_verifier_last_fold_stats",
    # the verifier's device-side transcript replay
    "plk_verifier_set_replay", "plk_verifier_challenges_batch", "plk_verifier_last_replay_ms",
    "plk_debug_fold_weights",
    # Lagrange-basis SRS and the wire commits' basis report
    "plk_srs_lagrange", "plk_prover_commit_info",
    # opening key, pairing check and the verdicts (OpeningKey here, Verifier in prover.py)
    "plk_opening_key_setup", "plk_opening_key_load", "plk_opening_key_points",
    "plk_opening_key_destroy", "plk_pairing_check", "plk_pairing_check_batch",
    "plk_opening_key_last_pairing_ms", "plk_debug_pairing", "plk_debug_f12_op", "plk_debug_miller",
    "plk_verifier_pairs",
    "plk_verifier_verify", "plk_verifier_verify_each", "plk_verifier_last_each_stats",
    # compact proofs and the ingest stage (g1_decompress / g1_subgroup_check here, the rest in
    # prover.py)
    "plk_proof_encode_compact", "plk_proof_decode_compact", "plk_g1_decompress_batch",
    "plk_g1_subgroup_check_batch", "plk_proofs_ingest", "plk_ingest_last_ms",
    "plk_verifier_verify_each_bytes",
    *_SRS_IO_SYMBOLS,
    *_SRS_UPDATE_SYMBOLS,
    # the circuit check and the prover's diagnosis (Plonk.check / Prover.diagnose in prover.py)
    *_CHECK_SYMBOLS,
    # KZG openings (PlonkParams.open / open_domain, OpeningKey.fold_openings) and the G1 transform
    *_KZG_SYMBOLS,
    # the fixed-base MSM's stage snapshot (debug_msm_snapshot here)
    *_MSM_DEBUG_SYMBOLS,
    *_MSM_LAYOUT_SYMBOLS,
)

# per-item status of the ingest calls (include/plk.h PLK_INGEST_*)
INGEST_OK, INGEST_ENCODING, INGEST_RANGE, INGEST_OFF_CURVE, INGEST_SUBGROUP = range(5)
# verdicts of PlonkParams.verify (include/plk.h PLK_SRS_*)
SRS_OK, SRS_POINT, SRS_SUBGROUP, SRS_INFINITY, SRS_GENERATOR, SRS_CHAIN = range(6)
# and of PlonkParams.verify_update (PLK_SRS_WITNESS / PLK_SRS_LINK)
SRS_WITNESS, SRS_LINK = 6, 7
# byte forms of points (include/plk.h PLK_G1_COMPRESSED / PLK_G1_UNCOMPRESSED)
_FORMATS = {"compressed": 0, "uncompressed": 1}


class PlonkError(RuntimeError):
    def __init__(self, status: int, what: str = "", bad_index: int | None = None,
                 bad_status: int | None = None):
        self.status = status
        # create_proof(..., explain=True) on an unsatisfied circuit: the CircuitReport
        self.report = None
        # PlonkParams.from_bytes: the smallest rejected index and its INGEST_* code
        self.bad_index, self.bad_status = bad_index, bad_status
        msg = _lib().plk_status_str(status).decode() if _LIB is not None else str(status)
        super().__init__(f"{what}: {msg} (status {status})" if what else msg)


_LIB = None


def _lib():
    """Load libplk.so (built in-tree by build_ext.py). Fails loudly when absent."""
    global _LIB
    if _LIB is None:
        if not _LIB_PATH.exists():
            raise ImportError(f"{_LIB_PATH} not built — run __graft_entry__.build() first")
        # One HIP runtime per process: torch ships its own libamdhip64 (same SONAME as
        # /opt/rocm's). Loading torch first makes libplk bind to that copy, so device
        # pointers and hipStream_t handles from torch are valid in our calls.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(str(_LIB_PATH))
        vp, u32, u64, sz, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int
        pp = C.POINTER(C.c_void_p)
        sig = {
            "plk_abi_version": (i32, []),
            "plk_status_str": (C.c_char_p, [i32]),
            "plk_build_info": (C.c_char_p, []),
            "plk_device_count": (i32, [C.POINTER(i32)]),
            "plk_ctx_create": (i32, [i32, pp]),
            "plk_ctx_destroy": (i32, [vp]),
            "plk_ctx_stream": (i32, [vp, pp]),
            "plk_ctx_synchronize": (i32, [vp]),
            "plk_domain_get": (i32, [vp, u32, pp]),
            "plk_domain_info": (i32, [vp, C.POINTER(u64), vp, vp, vp, vp, vp]),
            "plk_domain_elements": (i32, [vp, vp]),
            "plk_domain_vanishing_over_coset": (i32, [vp, u64, vp]),
            "plk_ntt": (i32, [vp, vp, sz, i32, i32]),
            "plk_ntt_dev": (i32, [vp, vp, vp, sz, i32, i32, vp, vp]),
            "plk_ntt_stream": (i32, [vp, vp, sz, i32, i32, vp]),
            "plk_aggregate_witness": (i32, [vp, vp, vp, sz, vp, vp, vp, C.POINTER(sz)]),
            "plk_aggregate_witness_dev": (i32, [vp, vp, vp, sz, vp, vp, vp, C.POINTER(sz), vp]),
            "plk_ntt_batch_dev": (i32, [vp, vp, sz, i32, i32, vp]),
            "plk_srs_setup": (i32, [vp, vp, sz, vp, pp]),
            "plk_srs_load": (i32, [vp, vp, sz, pp]),
            "plk_srs_destroy": (i32, [vp]),
            "plk_srs_len": (i32, [vp, C.POINTER(sz)]),
            "plk_srs_points": (i32, [vp, sz, sz, vp]),
            "plk_msm": (i32, [vp, vp, sz, vp]),
            "plk_commit": (i32, [vp, vp, sz, vp]),
            "plk_commit_dev": (i32, [vp, vp, sz, vp, vp]),
            "plk_srs_last_msm_stats": (i32, [vp, C.POINTER(C.c_float), C.POINTER(u64),
                                             C.POINTER(u32)]),
            "plk_debug_field_op": (i32, [vp, i32, i32, vp, vp, vp, sz]),
            "plk_debug_rx_op": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, sz]),
            "plk_debug_ntt_lazy_op": (i32, [vp, i32, vp, vp, sz]),
            "plk_debug_g1r_op": (i32, [vp, i32, vp, vp, vp, vp, sz]),
            "plk_debug_block_eval": (i32, [vp, vp, sz, vp, sz, C.POINTER(i32)]),
            "plk_debug_prover_stage": (i32, [vp, i32, vp, vp, sz, vp, sz, vp, sz, vp, sz]),
            "plk_debug_msm_snapshot": (i32, [vp, vp, vp, sz, vp, vp, vp]),
            "plk_commit_batch_dev": (i32, [vp, vp, vp, sz, vp, vp, vp]),
            "plk_commit_batch_dev_part": (i32, [vp, vp, vp, sz, u32, u32, vp, vp, vp]),
            "plk_srs_setup_range": (i32, [vp, vp, u64, sz, vp, pp]),
            "plk_g1_sum": (i32, [vp, sz, vp]),
            "plk_msm_sharded": (i32, [vp, i32, vp, sz, vp]),
            "plk_msm_points": (i32, [vp, vp, vp, sz, vp]),
            "plk_msm_points_ranges": (i32, [vp, vp, vp, sz, vp, vp, sz, vp]),
            "plk_srs_msm_stats_reset": (i32, [vp]),
            "plk_srs_cum_msm_stats": (i32, [vp, C.POINTER(C.c_double), C.POINTER(u64),
                                            C.POINTER(u64), C.POINTER(u64)]),
            "plk_opening_key_setup": (i32, [vp, pp]),
            "plk_opening_key_load": (i32, [vp, vp, pp]),
            "plk_opening_key_points": (i32, [vp, vp, vp]),
            "plk_opening_key_destroy": (i32, [vp]),
            "plk_pairing_check": (i32, [vp, vp, C.POINTER(i32)]),
            "plk_pairing_check_batch": (i32, [vp, vp, vp, sz, vp]),
            "plk_opening_key_last_pairing_ms": (i32, [vp, C.POINTER(C.c_float)]),
            "plk_debug_pairing": (i32, [vp, vp, vp, sz, vp]),
            "plk_debug_f12_op": (i32, [vp, i32, vp, vp, sz, vp]),
            "plk_debug_miller": (i32, [vp, vp, vp, vp, vp, sz, vp]),
            "plk_g1_decompress_batch": (i32, [vp, vp, sz, i32, vp, vp]),
            "plk_g1_subgroup_check_batch": (i32, [vp, vp, sz, vp]),
            "plk_ingest_last_ms": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
            "plk_srs_load_bytes": (i32, [vp, vp, sz, i32, i32, pp, C.POINTER(u64), C.POINTER(C.c_uint8)]),
            "plk_srs_export_bytes": (i32, [vp, sz, sz, i32, vp]),
            "plk_srs_last_load_ms": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
            "plk_srs_fold": (i32, [vp, vp, vp]),
            "plk_srs_verify": (i32, [vp, vp, vp, vp, C.POINTER(i32), C.POINTER(u64)]),
            "plk_srs_last_verify_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
            "plk_opening_key_load_bytes": (i32, [vp, vp, i32, pp]),
            "plk_opening_key_to_bytes": (i32, [vp, i32, vp, vp]),
            "plk_debug_srs_weights": (i32, [vp, vp, sz, vp]),
            "plk_debug_f2_sqrt": (i32, [vp, vp, C.POINTER(i32)]),
            "plk_g1_mul_batch": (i32, [vp, vp, vp, sz, i32, vp]),
            "plk_g1_mul_last_ms": (i32, [vp, C.POINTER(C.c_float)]),
            "plk_opening_key_update": (i32, [vp, vp, pp, vp]),
            "plk_srs_update": (i32, [vp, vp, vp, pp, pp, vp, C.POINTER(u64)]),
            "plk_srs_verify_update": (i32, [vp, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(u64)]),
            "plk_g2_to_bytes": (i32, [vp, i32, vp]),
            "plk_g2_from_bytes": (i32, [vp, i32, vp]),
            "plk_debug_glv_split": (i32, [vp, vp, sz, vp]),
            "plk_check_last_ms": (i32, [vp, C.POINTER(C.c_float)]),
            "plk_kzg_open": (i32, [vp, vp, sz, vp, sz, vp, vp]),
            "plk_kzg_open_domain": (i32, [vp, u32, vp, sz, vp, vp, C.POINTER(u64)]),
            "plk_kzg_last_open_ms": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                           C.POINTER(C.c_float)]),
            "plk_kzg_fold": (i32, [vp, vp, vp, vp, vp, vp, sz, vp, vp]),
            "plk_debug_g1_ntt": (i32, [vp, vp, u32, i32, vp]),
            "plk_kzg_open_cosets": (i32, [vp, u32, u32, vp, sz, vp, vp, C.POINTER(u64)]),
            "plk_kzg_fold_cosets": (i32, [vp, u32, vp, vp, vp, vp, sz, vp, vp]),
            "plk_debug_g1_ntt_batch": (i32, [vp, vp, u32, sz, i32, vp]),
            "plk_debug_g1_colsum": (i32, [vp, vp, sz, sz, vp]),
            "plk_srs_table_layout": (i32, [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]),
            "plk_msm_table_policy": (i32, [u64, u32, i32, C.POINTER(u32), C.POINTER(u64)]),
        }
        for name, (res, args) in sig.items():
            if (name in _SRS_IO_SYMBOLS + _SRS_UPDATE_SYMBOLS + _CHECK_SYMBOLS + _KZG_SYMBOLS
                    + _MSM_DEBUG_SYMBOLS + _MSM_LAYOUT_SYMBOLS and not hasattr(lib, name)):
                continue  # a PLK_LIB build from before srs_io.hip still loads; a use fails loudly
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        _LIB = lib
    return _LIB


def build_info() -> dict:
    """plk_build_info of the loaded library: {'src', 'flags', 'variant', 'lib'}."""
    raw = _lib().plk_build_info().decode()
    d = dict(kv.split("=", 1) for kv in raw.split())
    d["lib"] = str(_LIB_PATH)
    return d


def check_build(root: Path | None = None) -> dict:
    """Refuse a library built from other sources than the tree it is loaded from (round-5
    verdict: a pushed prebuilt libplk.so was not tied to its sources). The default library
    must also carry the default flags; a PLK_LIB variant (tools/ab.py) may differ in flags.
    Returns build_info() with the tree's ids; raises ImportError on a mismatch."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_plk_build_ext", _PKG / "build_ext.py")
    be = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(be)
    info = build_info()
    tree_src = be.source_id(root or be.ROOT)
    info["tree_src"] = tree_src
    if os.environ.get("PLK_LIB") and os.environ.get("PLK_LIB_ANY_SRC") == "1":
        info["src_check"] = "skipped (PLK_LIB variant with PLK_LIB_ANY_SRC=1: an A/B against another tree)"
        return info
    if info.get("src") != tree_src:
        raise ImportError(f"{_LIB_PATH} was built from other sources (library src={info.get('src')}, "
                          f"tree src={tree_src}): rebuild with __graft_entry__.build()")
    if not os.environ.get("PLK_LIB") and info.get("flags") != be.flags_id():
        raise ImportError(f"{_LIB_PATH} was built with other flags (library flags={info.get('flags')}, "
                          f"default flags={be.flags_id()}): rebuild with __graft_entry__.build()")
    return info


def _check(status: int, what: str):
    if status != PLK_OK:
        raise PlonkError(status, what)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    n = C.c_int(0)
    _check(_lib().plk_device_count(C.byref(n)), "plk_device_count")
    return n.value


# ------------------------------------------------------------------------------ context
class Context:
    """One plk_ctx per GPU (device memory, stream, cached Fft domains)."""

    _default: dict[int, "Context"] = {}

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(_lib().plk_ctx_create(device, C.byref(h)), "plk_ctx_create")
        self.handle = h
        self.device = device
        self._domains: dict[int, C.c_void_p] = {}

    @classmethod
    def default(cls, device: int | None = None) -> "Context":
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) if "LOCAL_RANK" in os.environ else 0
            try:
                import torch  # noqa: F401 — only to follow torch's current device when present
                if torch.cuda.is_available():
                    device = torch.cuda.current_device()
            except Exception:
                pass
        if device not in cls._default:
            cls._default[device] = Context(device)
        return cls._default[device]

    def stream(self) -> int:
        s = C.c_void_p()
        _check(_lib().plk_ctx_stream(self.handle, C.byref(s)), "plk_ctx_stream")
        return s.value or 0

    def synchronize(self):
        _check(_lib().plk_ctx_synchronize(self.handle), "plk_ctx_synchronize")

    def field_op(self, field: str, op: str, a: np.ndarray, b: np.ndarray | None = None):
        """Elementwise device field arithmetic (test support): field 'fr'|'fp',
        op 'mul'|'add'|'sub'|'sqr'|'inv'; Montgomery limbs in and out."""
        w = 4 if field == "fr" else 6
        a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, w))
        bb = None if b is None else np.ascontiguousarray(np.asarray(b, dtype=np.uint64).reshape(-1, w))
        out = np.zeros_like(a)
        code = {"mul": 0, "add": 1, "sub": 2, "sqr": 3, "inv": 4}[op]
        _check(_lib().plk_debug_field_op(self.handle, 0 if field == "fr" else 1, code, _ptr(a),
                                         None if bb is None else _ptr(bb), _ptr(out), a.shape[0]),
               "plk_debug_field_op")
        return out

    # op -> (code, operand rows, output rows) of plk_debug_rx_op (include/plk.h)
    RX_OPS = {"mul": (0, 2, 1), "sqr": (1, 1, 1), "mul_add": (2, 4, 1), "mul2": (3, 4, 2),
              "mul2_asm": (4, 4, 2), "sqr2": (5, 2, 2), "sqr2_asm": (6, 2, 2),
              "mul_add_mul2": (7, 4, 3), "mul_add_mul2_asm": (8, 4, 3), "mul3": (9, 4, 3),
              "add": (10, 2, 1), "sub": (11, 2, 1), "sub_lazy": (12, 2, 1), "sub2_n6": (13, 3, 1),
              "small_mul2": (14, 1, 1), "small_mul3": (15, 1, 1), "canon": (16, 1, 1),
              "is_zero": (17, 1, 1), "is_zero_u": (18, 1, 1), "unpack_pack": (19, 1, 2),
              "sub_u": (100, 2, 1), "sub_n": (200, 2, 1)}
    G1R_OPS = {"madd_000": 0, "madd_100": 1, "madd_110": 2, "madd_111": 3, "madd_lazy": 4,
               "add_lazy": 5, "add_quad": 6, "dbl_lazy": 7, "lazy_finish": 8, "add": 9,
               "add_affine": 10, "dbl": 11, "dbl_affine": 12}

    def rx_op(self, field: str, op: str, *rows, cp: int = 0) -> np.ndarray:
        """The redundant-limb field (csrc/ffr.hpp) on raw uint32 limb rows (test support):
        field 'fr' (9 limbs) | 'fp' (13), op a key of RX_OPS ('sub_u' / 'sub_n' take cp);
        returns [n, outputs, limbs]."""
        L = 9 if field == "fr" else 13
        code, nin, nout = self.RX_OPS[op]
        if len(rows) != nin:
            raise ValueError(f"rx_op {op} takes {nin} operand arrays")
        ops = [np.ascontiguousarray(np.asarray(r, dtype=np.uint32).reshape(-1, L)) for r in rows]
        n = ops[0].shape[0]
        if any(o.shape[0] != n for o in ops):
            raise ValueError("rx_op operands differ in length")
        out = np.zeros((n, nout, L), dtype=np.uint32)
        ptrs = [_ptr(o) for o in ops] + [None] * (4 - nin)
        _check(_lib().plk_debug_rx_op(self.handle, 0 if field == "fr" else 1, code + cp, *ptrs,
                                      _ptr(out), n), "plk_debug_rx_op")
        return out

    # op -> (code, operand rows, output rows) of plk_debug_ntt_lazy_op (include/plk.h)
    NTT_LAZY_OPS = {"reduce_q": (0, 1, 1), "add_u": (1, 2, 1), "sub_u": (2, 2, 1),
                    "sub_u2_11": (3, 2, 1), "r4": (4, 7, 4), "r4_h1": (5, 5, 4),
                    "r2first": (6, 3, 2), "odd_last": (7, 2, 2), "store0": (8, 1, 1),
                    "store1": (9, 2, 1), "store2": (10, 2, 1)}

    def ntt_lazy_op(self, op: str, *rows) -> np.ndarray:
        """The NTT pass kernel's lazy butterfly helpers (csrc/ntt.hip) on raw rows of 9 uint32
        limbs (test support): op a key of NTT_LAZY_OPS, one array of n rows per operand; returns
        [n, outputs, 9]. 'store1' applies the scale row of case 0 to every case."""
        code, nin, nout = self.NTT_LAZY_OPS[op]
        if len(rows) != nin:
            raise ValueError(f"ntt_lazy_op {op} takes {nin} operand arrays")
        ops = [np.asarray(r, dtype=np.uint32).reshape(-1, 9) for r in rows]
        n = ops[0].shape[0]
        if any(o.shape[0] != n for o in ops):
            raise ValueError("ntt_lazy_op operands differ in length")
        cases = np.ascontiguousarray(np.stack(ops, axis=1))  # [n, operands, 9]
        out = np.zeros((n, nout, 9), dtype=np.uint32)
        _check(_lib().plk_debug_ntt_lazy_op(self.handle, code, _ptr(cases), _ptr(out), n),
               "plk_debug_ntt_lazy_op")
        return out

    def g1r_op(self, op: str, p, q=None, flags=None) -> np.ndarray:
        """The XYZZ group law (csrc/g1r.hpp) on raw rows of 4 x 13 uint32 limbs (test support):
        op a key of G1R_OPS; returns [n, 4, 13], for 'add_quad' [n, 4 lanes, 4, 13]."""
        p = np.ascontiguousarray(np.asarray(p, dtype=np.uint32).reshape(-1, 4, 13))
        n = p.shape[0]
        if q is not None:
            q = np.ascontiguousarray(np.asarray(q, dtype=np.uint32).reshape(-1, 4, 13))
        if flags is not None:
            flags = np.ascontiguousarray(np.asarray(flags, dtype=np.uint32).reshape(-1))
        if any(x is not None and x.shape[0] != n for x in (q, flags)):
            raise ValueError("g1r_op operands differ in length")
        out = np.zeros((n, 4, 4, 13) if op == "add_quad" else (n, 4, 13), dtype=np.uint32)
        _check(_lib().plk_debug_g1r_op(self.handle, self.G1R_OPS[op], _ptr(p),
                                       None if q is None else _ptr(q),
                                       None if flags is None else _ptr(flags), _ptr(out), n),
               "plk_debug_g1r_op")
        return out

    # stage -> code of plk_debug_prover_stage (include/plk.h)
    PROVER_STAGES = {"perm_numden": 0, "scan": 1, "quotient": 2, "pi_sparse": 3, "pi_coef": 4,
                     "coset_combine": 5, "eval": 6, "lincomb": 7, "scale_powers": 8, "ruffini": 9,
                     "quotient_top": 10, "coset_combine_top": 11}

    def prover_stage(self, stage, arrays=(), scalars=(), params=(), out_len: int = 0) -> np.ndarray:
        """One pk_* launcher of the prover (csrc/prover_kernels.hip) on host arrays (test
        support): stage a key of PROVER_STAGES (or a raw code), arrays uint64[len, 4] Montgomery
        words each, scalars uint64[k, 4], params integers; returns uint64[out_len, 4]."""
        return _prover_stage(self.handle, stage, arrays, scalars, params, out_len)

    def domain(self, k: int) -> C.c_void_p:
        if k not in self._domains:
            d = C.c_void_p()
            _check(_lib().plk_domain_get(self.handle, k, C.byref(d)), "plk_domain_get")
            self._domains[k] = d
        return self._domains[k]


def _prover_stage(handle, stage, arrays, scalars, params, out_len: int) -> np.ndarray:
    code = Context.PROVER_STAGES[stage] if isinstance(stage, str) else int(stage)
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, 4)) for a in arrays]
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if a.shape[0] else None for a in arrs])
    lens = (C.c_size_t * max(len(arrs), 1))(*[a.shape[0] for a in arrs])
    sc = np.ascontiguousarray(np.asarray(scalars, dtype=np.uint64).reshape(-1, 4))
    par = np.ascontiguousarray(np.asarray(list(params), dtype=np.uint64).reshape(-1))
    out = np.zeros((out_len, 4), dtype=np.uint64)
    _check(_lib().plk_debug_prover_stage(
        handle, code, ptrs if arrs else None, lens if arrs else None, len(arrs),
        _ptr(sc) if sc.shape[0] else None, sc.shape[0], _ptr(par) if par.shape[0] else None,
        par.shape[0], _ptr(out) if out_len else None, out_len), "plk_debug_prover_stage")
    return out


def quotient_top(arrays, scalars, params) -> np.ndarray:
    """Stage "quotient_top" of plk_debug_prover_stage (include/plk.h): the quotient's coefficients
    4n .. 4n + 6 from the factor polynomials' top coefficients. Host code: no GPU, no Context."""
    return _prover_stage(None, "quotient_top", arrays, scalars, params, 7)


# ------------------------------------------------------------------------ value types
def _as_fr_array(values) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    if a.ndim == 1 and a.size % 4 == 0:
        a = a.reshape(-1, 4)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("expected uint64[n, 4] Montgomery Fr limbs")
    return a


class Coefficients:
    """poly_commit::Coefficients<Fr> — ``pub Vec<F>`` of coefficients (``.0`` is ``.values``)."""

    def __init__(self, values):
        self.values = _as_fr_array(values)

    def __len__(self):
        return self.values.shape[0]

    def clone(self):
        return type(self)(self.values.copy())

    def degree(self) -> int:
        """Index of the last non-zero coefficient (0 for the zero polynomial)."""
        nz = np.nonzero(self.values.any(axis=1))[0]
        return int(nz[-1]) if nz.size else 0


class PointsValue(Coefficients):
    """poly_commit::PointsValue<Fr> — evaluations over a domain."""

    def cosets(self, log_l: int) -> np.ndarray:
        """The n = 2^k values in the domain's natural order as the cosets of l = 2^log_l points
        PlonkParams.open_cosets opens: a view uint64[r, l, 4], r = n / l, whose row j holds
        f(omega^(j + r i)), i < l, the values on omega^j <omega^r> in the order
        OpeningKey.fold_cosets takes them."""
        n, l = self.values.shape[0], 1 << log_l
        if n == 0 or n & (n - 1) or l > n:
            raise ValueError("cosets: 2^k values and l <= 2^k")
        return self.values.reshape(l, n // l, 4).transpose(1, 0, 2)


# ------------------------------------------------------------------------------- Fft
class Fft:
    """poly_commit::Fft<Fr> on the GPU: ``Fft(k)`` = ``Fft::new(k)`` (n = 2^k).

    w = ROOT_OF_UNITY^(2^(32-k)); cosets use g = 7; tables live in HBM per context.
    """

    def __init__(self, k: int, ctx: Context | None = None):
        self.ctx = ctx or Context.default()
        self.k = k
        self._d = self.ctx.domain(k)
        n = C.c_uint64()
        self._consts = [np.zeros(4, dtype=np.uint64) for _ in range(5)]
        _check(_lib().plk_domain_info(self._d, C.byref(n), *[_ptr(c) for c in self._consts]),
               "plk_domain_info")
        self._n = n.value
        self._elements = None

    # -- accessors (key.rs:205-207, prover.rs:252,446)
    def size(self) -> int:
        return self._n

    def generator(self) -> np.ndarray:
        return self._consts[0].copy()

    def generator_inv(self) -> np.ndarray:
        return self._consts[1].copy()

    def size_inv(self) -> np.ndarray:
        return self._consts[2].copy()

    def coset_generator(self) -> np.ndarray:
        return self._consts[3].copy()

    @property
    def elements(self) -> np.ndarray:
        """elements[i] = w^i (permutation.rs:148)."""
        if self._elements is None:
            out = np.zeros((self._n, 4), dtype=np.uint64)
            _check(_lib().plk_domain_elements(self._d, _ptr(out)), "plk_domain_elements")
            self._elements = out
        return self._elements

    def compute_vanishing_poly_over_coset(self, poly_degree: int) -> PointsValue:
        out = np.zeros((self._n, 4), dtype=np.uint64)
        _check(_lib().plk_domain_vanishing_over_coset(self._d, poly_degree, _ptr(out)),
               "plk_domain_vanishing_over_coset")
        return PointsValue(out)

    # -- transforms
    def _run(self, vals: np.ndarray, direction: int, coset: int, stream: int = 0) -> np.ndarray:
        """stream != 0: plk_ntt_stream on that hipStream_t (own staging, so threads with
        their own streams may share this Fft); else plk_ntt on the context's stream."""
        vals = _as_fr_array(vals)
        if vals.shape[0] > self._n:
            raise ValueError(f"input of length {vals.shape[0]} exceeds the domain size {self._n}")
        buf = np.zeros((self._n, 4), dtype=np.uint64)
        buf[: vals.shape[0]] = vals
        if stream:
            _check(_lib().plk_ntt_stream(self._d, _ptr(buf), vals.shape[0], direction, coset,
                                         C.c_void_p(stream)), "plk_ntt_stream")
        else:
            _check(_lib().plk_ntt(self._d, _ptr(buf), vals.shape[0], direction, coset), "plk_ntt")
        return buf

    def dft(self, coeffs: Coefficients, stream: int = 0) -> PointsValue:
        return PointsValue(self._run(coeffs.values, 1, 0, stream))

    def idft(self, points: PointsValue, stream: int = 0) -> Coefficients:
        return Coefficients(self._run(points.values, -1, 0, stream))

    def coset_dft(self, coeffs: Coefficients, stream: int = 0) -> PointsValue:
        return PointsValue(self._run(coeffs.values, 1, 1, stream))

    def coset_idft(self, points: PointsValue, stream: int = 0) -> Coefficients:
        return Coefficients(self._run(points.values, -1, 1, stream))

    # -- device-resident variants (torch tensors of dtype int64, shape [n, 4], on cuda)
    def ntt_dev(self, d_in_ptr: int, d_out_ptr: int, len_in: int, direction: int, coset: bool,
                stream: int = 0, d_scratch_ptr: int = 0):
        _check(_lib().plk_ntt_dev(self._d, C.c_void_p(d_in_ptr), C.c_void_p(d_out_ptr), len_in,
                                  direction, int(coset), C.c_void_p(d_scratch_ptr or None),
                                  C.c_void_p(stream or None)), "plk_ntt_dev")


# ------------------------------------------------------------------------------ KZG
class Commitment:
    """Commitment<G1Affine>: one canonical affine point (uint64[13])."""

    def __init__(self, words: np.ndarray):
        self.words = np.asarray(words, dtype=np.uint64).reshape(13)

    @property
    def is_identity(self) -> bool:
        return bool(self.words[12])

    def __eq__(self, other):
        return isinstance(other, Commitment) and np.array_equal(self.words, other.words)

    def __repr__(self):
        return "Commitment(identity)" if self.is_identity else \
            f"Commitment(x0={int(self.words[0]):#x}...)"


def g1_sum(points: np.ndarray) -> Commitment:
    """Host-side sum of affine points uint64[n, 13] (no GPU needed)."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    out = np.zeros(13, dtype=np.uint64)
    _check(_lib().plk_g1_sum(_ptr(pts), pts.shape[0], _ptr(out)), "plk_g1_sum")
    return Commitment(out)


def msm_sharded(shards, scalars) -> Commitment:
    """One MSM over consecutive SRS slices held by different GPUs of this process
    (PlonkParams.setup_range per device, in order): plk_msm_sharded."""
    vals = _as_fr_array(scalars)
    hs = (C.c_void_p * len(shards))(*[s._h.value for s in shards])
    out = np.zeros(13, dtype=np.uint64)
    _check(_lib().plk_msm_sharded(hs, len(shards), _ptr(vals), vals.shape[0], _ptr(out)),
           "plk_msm_sharded")
    return Commitment(out)


def msm_points_ranges(points, scalars, ranges, ctx: "Context | None" = None) -> list:
    """Several variable-base MSMs over disjoint index ranges [(start, len), ...] of one point
    array as one GPU batch (plk_msm_points_ranges); returns a Commitment per range."""
    ctx = ctx or Context.default()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    vals = _as_fr_array(scalars) if len(scalars) else np.zeros((0, 4), dtype=np.uint64)
    if pts.shape[0] != vals.shape[0]:
        raise ValueError("msm_points: as many scalars as points")
    k = len(ranges)
    starts = (C.c_size_t * max(k, 1))(*[int(a) for a, _ in ranges])
    lens = (C.c_size_t * max(k, 1))(*[int(n) for _, n in ranges])
    outs = np.zeros((max(k, 1), 13), dtype=np.uint64)
    _check(_lib().plk_msm_points_ranges(ctx.handle, _ptr(pts), _ptr(vals), pts.shape[0], starts,
                                        lens, k, _ptr(outs)), "msm_points")
    return [Commitment(outs[i]) for i in range(k)]


def msm_points(points, scalars, ctx: "Context | None" = None) -> Commitment:
    """msm_curve_addition(&[G1Affine], &[Fr]) for arbitrary affine points uint64[n, 13]
    (proof.rs:507): plk_msm_points, the variable-base Pippenger. Identity points are skipped;
    PlonkError(PLK_E_ARG) for a finite point off the curve."""
    ctx = ctx or Context.default()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    vals = _as_fr_array(scalars) if len(scalars) else np.zeros((0, 4), dtype=np.uint64)
    if pts.shape[0] != vals.shape[0]:
        raise ValueError("msm_points: as many scalars as points")
    out = np.zeros(13, dtype=np.uint64)
    _check(_lib().plk_msm_points(ctx.handle, _ptr(pts), _ptr(vals), pts.shape[0], _ptr(out)),
           "msm_points")
    return Commitment(out)


def g1_decompress(blob, subgroup: bool = True, ctx: "Context | None" = None):
    """n zkcrypto-compressed G1 points (48 n bytes) -> (points uint64[n, 13], status uint8[n]),
    decoded on the GPU (plk_g1_decompress_batch). status[i] is an INGEST_* code; a rejected
    point's row is zero. subgroup=False skips the membership test."""
    ctx = ctx or Context.default()
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    if raw.size == 0 or raw.size % 48:
        raise PlonkError(PLK_E_ARG, "g1_decompress: a positive multiple of 48 bytes")
    n = raw.size // 48
    pts = np.zeros((n, 13), dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    _check(_lib().plk_g1_decompress_batch(ctx.handle, _ptr(raw), n, int(bool(subgroup)), _ptr(pts),
                                          _ptr(status)), "g1_decompress")
    return pts, status


def g1_subgroup_check(points, ctx: "Context | None" = None) -> np.ndarray:
    """bool[n]: whether each ABI point uint64[n, 13] has order r (the identity does), on the GPU
    (plk_g1_subgroup_check_batch). PlonkError(PLK_E_ARG) for a non-canonical or off-curve point."""
    ctx = ctx or Context.default()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    ok = np.zeros(max(1, pts.shape[0]), dtype=np.uint8)
    _check(_lib().plk_g1_subgroup_check_batch(ctx.handle, _ptr(pts), pts.shape[0], _ptr(ok)),
           "g1_subgroup_check")
    return ok[:pts.shape[0]].astype(bool)


def g1_mul(points, scalars, assume_subgroup: bool = False, ctx: "Context | None" = None) -> np.ndarray:
    """out[i] = [scalars[i]] points[i] as uint64[n, 13], one point and one scalar per GPU lane
    (plk_g1_mul_batch). points: ABI rows uint64[n, 13], scalars: Montgomery Fr uint64[n, 4].
    assume_subgroup=False tests every point for order r first and raises PlonkError(PLK_E_ARG)
    for a non-member; True: the caller vouches for membership. PLK_E_ARG also for a non-canonical
    or off-curve point, an infinity word other than 0 / 1 and a scalar >= r."""
    ctx = ctx or Context.default()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    vals = np.ascontiguousarray(np.asarray(scalars, dtype=np.uint64).reshape(-1, 4))
    if pts.shape[0] != vals.shape[0]:
        raise ValueError("g1_mul: as many scalars as points")
    out = np.zeros((max(1, pts.shape[0]), 13), dtype=np.uint64)
    _check(_lib().plk_g1_mul_batch(ctx.handle, _ptr(pts), _ptr(vals), pts.shape[0],
                                   int(bool(assume_subgroup)), _ptr(out)), "g1_mul")
    return out[:pts.shape[0]]


def g1_mul_last_ms(ctx: "Context | None" = None) -> float:
    """Milliseconds of the multiplication kernel of the most recent g1_mul / PlonkParams.update
    on the context (HIP events)."""
    ctx = ctx or Context.default()
    a = C.c_float()
    _check(_lib().plk_g1_mul_last_ms(ctx.handle, C.byref(a)), "plk_g1_mul_last_ms")
    return a.value


def debug_glv_split(scalars, ctx: "Context | None" = None) -> np.ndarray:
    """Test support (plk_debug_glv_split): uint64[n, 4] rows a_lo, a_hi, b_lo, b_hi of the split of
    each Montgomery scalar uint64[n, 4]. ctx = None: the host mirror; otherwise the device function."""
    vals = np.ascontiguousarray(np.asarray(scalars, dtype=np.uint64).reshape(-1, 4))
    out = np.zeros((max(1, vals.shape[0]), 4), dtype=np.uint64)
    _check(_lib().plk_debug_glv_split(ctx.handle if ctx is not None else None, _ptr(vals), vals.shape[0],
                                      _ptr(out)), "plk_debug_glv_split")
    return out[:vals.shape[0]]


def g2_to_bytes(point, fmt: str = "compressed") -> bytes:
    """One G2 point uint64[25] (a witness) in zkcrypto's byte form: 96 bytes compressed, 192
    uncompressed (plk_g2_to_bytes, host only)."""
    q = np.ascontiguousarray(np.asarray(point, dtype=np.uint64).reshape(G2_WORDS))
    out = np.zeros(96 if _FORMATS[fmt] == 0 else 192, dtype=np.uint8)
    _check(_lib().plk_g2_to_bytes(_ptr(q), _FORMATS[fmt], _ptr(out)), "plk_g2_to_bytes")
    return out.tobytes()


def g2_from_bytes(blob, fmt: str = "compressed") -> np.ndarray:
    """The inverse: strict decoding to uint64[25] (plk_g2_from_bytes); the subgroup check is the
    consumer's (PlonkParams.verify_update makes it)."""
    size = 96 if _FORMATS[fmt] == 0 else 192
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    if raw.size != size:
        raise PlonkError(PLK_E_ARG, f"g2_from_bytes: {size} bytes")
    out = np.zeros(G2_WORDS, dtype=np.uint64)
    _check(_lib().plk_g2_from_bytes(_ptr(raw), _FORMATS[fmt], _ptr(out)), "plk_g2_from_bytes")
    return out


def kzg_last_open_ms(ctx: "Context | None" = None):
    """(transform ms, multiplication ms, table-build ms) of the most recent
    PlonkParams.open_domain on the context (HIP events; the table build is 0 when it was cached)."""
    ctx = ctx or Context.default()
    a, b, c = C.c_float(), C.c_float(), C.c_float()
    _check(_lib().plk_kzg_last_open_ms(ctx.handle, C.byref(a), C.byref(b), C.byref(c)),
           "plk_kzg_last_open_ms")
    return a.value, b.value, c.value


def debug_g1_ntt(points, k: int, direction: int, ctx: "Context | None" = None) -> np.ndarray:
    """Test support (plk_debug_g1_ntt): the transform over G1 of uint64[2^k, 13] ABI points,
    direction +1 / -1 (the inverse with n^-1), natural order, as uint64[2^k, 13]."""
    ctx = ctx or Context.default()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    if pts.shape[0] != 1 << k:
        raise ValueError("debug_g1_ntt: 2^k points")
    out = np.zeros_like(pts)
    _check(_lib().plk_debug_g1_ntt(ctx.handle, _ptr(pts), k, direction, _ptr(out)), "plk_debug_g1_ntt")
    return out


def debug_g1_ntt_batch(points, k: int, batch: int, direction: int, ctx: "Context | None" = None) -> np.ndarray:
    """Test support (plk_debug_g1_ntt_batch): `batch` transforms of 2^k points each, one after the
    other in uint64[batch * 2^k, 13], through the batched launcher; otherwise as debug_g1_ntt."""
    ctx = ctx or Context.default()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    if pts.shape[0] != batch << k:
        raise ValueError("debug_g1_ntt_batch: batch * 2^k points")
    out = np.zeros_like(pts)
    _check(_lib().plk_debug_g1_ntt_batch(ctx.handle, _ptr(pts), k, batch, direction, _ptr(out)),
           "plk_debug_g1_ntt_batch")
    return out


def debug_g1_colsum(points, rows: int, cols: int, ctx: "Context | None" = None) -> np.ndarray:
    """Test support (plk_debug_g1_colsum): out[t] = sum_a points[a * cols + t] over uint64[rows *
    cols, 13] ABI points (any points of the curve), as uint64[cols, 13]."""
    ctx = ctx or Context.default()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    if pts.shape[0] != rows * cols:
        raise ValueError("debug_g1_colsum: rows * cols points")
    out = np.zeros((cols, 13), dtype=np.uint64)
    _check(_lib().plk_debug_g1_colsum(ctx.handle, _ptr(pts), rows, cols, _ptr(out)), "plk_debug_g1_colsum")
    return out


def _fr_limbs(s) -> np.ndarray:
    """A canonical int or uint64[4] Montgomery limbs -> uint64[4] Montgomery limbs (an int is NOT
    reduced: a value >= r reaches the library as it is and is refused there)."""
    if isinstance(s, (int, np.integer)):
        v = int(s)
        m = v * (1 << 256) % _FR_MOD if 0 <= v < _FR_MOD else v
        if m >> 256:
            raise PlonkError(PLK_E_ARG, "a scalar is below 2^256")
        return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    return np.ascontiguousarray(np.asarray(s, dtype=np.uint64).reshape(4))


def ingest_last_ms(ctx: "Context | None" = None):
    """(decompress kernel ms, subgroup kernel ms) of the most recent ingest call on the context."""
    ctx = ctx or Context.default()
    a, b = C.c_float(), C.c_float()
    _check(_lib().plk_ingest_last_ms(ctx.handle, C.byref(a), C.byref(b)), "plk_ingest_last_ms")
    return a.value, b.value


def check_last_ms(ctx: "Context | None" = None) -> float:
    """k_gate_check's kernel ms in the most recent Plonk.check / diagnose on the context."""
    ctx = ctx or Context.default()
    a = C.c_float()
    _check(_lib().plk_check_last_ms(ctx.handle, C.byref(a)), "plk_check_last_ms")
    return a.value


def _seed32(seed) -> np.ndarray:
    raw = np.frombuffer(bytes(seed), dtype=np.uint8)
    if raw.size != 32:
        raise ValueError("a seed is 32 bytes")
    return raw


class SrsVerdict:
    """Result of PlonkParams.verify / verify_update: ok, verdict (an SRS_* class; SRS_WITNESS and
    SRS_LINK come from verify_update alone) and bad_index (the smallest offending index for
    SRS_POINT / SRS_SUBGROUP / SRS_INFINITY, else None)."""

    NAMES = {SRS_OK: "ok", SRS_POINT: "point", SRS_SUBGROUP: "subgroup", SRS_INFINITY: "infinity",
             SRS_GENERATOR: "generator", SRS_CHAIN: "chain", SRS_WITNESS: "witness", SRS_LINK: "link"}

    def __init__(self, ok: bool, verdict: int, bad_index: int | None):
        self.ok, self.verdict, self.bad_index = ok, verdict, bad_index

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return (f"SrsVerdict(ok={self.ok}, verdict={self.verdict} "
                f"({self.NAMES.get(self.verdict, '?')}), bad_index={self.bad_index})")


def srs_last_load_ms(ctx: "Context | None" = None):
    """(decode kernel ms, subgroup kernel ms) of the most recent PlonkParams.from_bytes on the context."""
    ctx = ctx or Context.default()
    a, b = C.c_float(), C.c_float()
    _check(_lib().plk_srs_last_load_ms(ctx.handle, C.byref(a), C.byref(b)), "plk_srs_last_load_ms")
    return a.value, b.value


def debug_srs_weights(seed, n: int, ctx: "Context | None" = None) -> np.ndarray:
    """Test support (plk_debug_srs_weights): the n - 1 fold weights of an n-point SRS for `seed`,
    uint64[n - 1, 4] Montgomery limbs. ctx = None: the host mirror; otherwise the kernel."""
    out = np.zeros((max(1, n - 1), 4), dtype=np.uint64)
    _check(_lib().plk_debug_srs_weights(ctx.handle if ctx is not None else None, _ptr(_seed32(seed)), n,
                                        _ptr(out)), "plk_debug_srs_weights")
    return out[:n - 1]


class PlonkParams:
    """zksnarks::plonk::PlonkParams<TatePairing> (the G1 side used by the prover).

    ``setup(k, tau)`` restates ``PlonkParams::setup(k, rng)`` with an explicit secret tau
    (Montgomery Fr limbs) so the CPU and GPU paths see identical randomness; it emits
    2^k + 8 powers because the blinded z (n+3) and t_4 (up to n+7) overrun 2^k.
    """

    SLACK = 8

    def __init__(self, handle: C.c_void_p, n_points: int, ctx: Context):
        self._h = handle
        self.n = n_points
        self.ctx = ctx

    @classmethod
    def setup(cls, k: int, tau, ctx: Context | None = None, n_points: int | None = None):
        ctx = ctx or Context.default()
        n = n_points if n_points is not None else (1 << k) + cls.SLACK
        tau = _as_fr_array(tau).reshape(4)
        h = C.c_void_p()
        _check(_lib().plk_srs_setup(ctx.handle, _ptr(tau), n, None, C.byref(h)), "plk_srs_setup")
        return cls(h, n, ctx)

    @classmethod
    def setup_range(cls, tau, start: int, count: int, ctx: Context | None = None):
        """The slice [start, start + count) of the SRS of `tau` (a sharded MSM's shard)."""
        ctx = ctx or Context.default()
        tau = _as_fr_array(tau).reshape(4)
        h = C.c_void_p()
        _check(_lib().plk_srs_setup_range(ctx.handle, _ptr(tau), start, count, None, C.byref(h)),
               "plk_srs_setup_range")
        return cls(h, count, ctx)

    @classmethod
    def load(cls, points: np.ndarray, ctx: Context | None = None):
        ctx = ctx or Context.default()
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
        h = C.c_void_p()
        _check(_lib().plk_srs_load(ctx.handle, _ptr(pts), pts.shape[0], C.byref(h)), "plk_srs_load")
        return cls(h, pts.shape[0], ctx)

    @classmethod
    def from_bytes(cls, blob, fmt: str = "compressed", subgroup: bool = True,
                   ctx: Context | None = None) -> "PlonkParams":
        """An SRS from a bare array of zkcrypto-encoded points (48 bytes each compressed, 96
        uncompressed), decoded and checked on the GPU (plk_srs_load_bytes). One rejected point
        raises PlonkError(PLK_E_ARG) carrying bad_index (the smallest rejected index) and
        bad_status (its INGEST_* code). subgroup=False skips the membership test; verify() then
        runs it."""
        ctx = ctx or Context.default()
        size = 48 if _FORMATS[fmt] == 0 else 96
        raw = np.frombuffer(bytes(blob), dtype=np.uint8)
        if raw.size == 0 or raw.size % size:
            raise PlonkError(PLK_E_ARG, f"PlonkParams.from_bytes: a positive multiple of {size} bytes")
        n = raw.size // size
        h, idx, code = C.c_void_p(), C.c_uint64(0), C.c_uint8(0)
        st = _lib().plk_srs_load_bytes(ctx.handle, _ptr(raw), n, _FORMATS[fmt], int(bool(subgroup)),
                                       C.byref(h), C.byref(idx), C.byref(code))
        if st == PLK_E_ARG and code.value != INGEST_OK:
            raise PlonkError(st, f"plk_srs_load_bytes: point {idx.value} rejected (status {code.value})",
                             bad_index=idx.value, bad_status=code.value)
        _check(st, "plk_srs_load_bytes")
        return cls(h, n, ctx)

    def to_bytes(self, fmt: str = "compressed", start: int = 0, count: int | None = None) -> bytes:
        """Points [start, start + count) in zkcrypto's byte form, encoded on the GPU
        (plk_srs_export_bytes); from_bytes of the result reproduces points() bit for bit."""
        count = self.n - start if count is None else count
        out = np.zeros(max(1, count * (48 if _FORMATS[fmt] == 0 else 96)), dtype=np.uint8)
        _check(_lib().plk_srs_export_bytes(self._h, start, count, _FORMATS[fmt], _ptr(out)),
               "plk_srs_export_bytes")
        return out[:count * (48 if _FORMATS[fmt] == 0 else 96)].tobytes()

    def fold_chain(self, seed: bytes | None = None) -> np.ndarray:
        """(C, W) as uint64[2, 13]: C = sum rho_i g1[i+1], W = sum rho_i g1[i] over weights drawn
        from `seed` (None: OS entropy, the sound form) — plk_srs_fold. The SRS is a chain of powers
        of the opening key's tau iff OpeningKey.check((C, W)) holds, up to 2^-128."""
        out = np.zeros((2, 13), dtype=np.uint64)
        sd = None if seed is None else _ptr(_seed32(seed))
        _check(_lib().plk_srs_fold(self._h, sd, _ptr(out)), "plk_srs_fold")
        return out

    def verify(self, opening_key: "OpeningKey", seed: bytes | None = None) -> "SrsVerdict":
        """Is this SRS ([tau^i]G)_i for the tau of `opening_key`? (plk_srs_verify.) A bad SRS is a
        verdict, never an exception."""
        verdict, idx = C.c_int(-1), C.c_uint64(0xFFFFFFFFFFFFFFFF)
        sd = None if seed is None else _ptr(_seed32(seed))
        _check(_lib().plk_srs_verify(self.ctx.handle, self._h, opening_key._h, sd, C.byref(verdict),
                                     C.byref(idx)), "plk_srs_verify")
        bad = idx.value if verdict.value in (SRS_POINT, SRS_SUBGROUP, SRS_INFINITY) else None
        return SrsVerdict(verdict.value == SRS_OK, verdict.value, bad)

    def update(self, opening_key: "OpeningKey", s=None):
        """Contribute to this SRS: (new PlonkParams, new OpeningKey, witness) with g1'[i] =
        [s^i] g1[i], beta_h' = [s] beta_h and witness = [s]H as uint64[25] (plk_srs_update). s = None
        draws the secret from OS entropy inside the library, which wipes it before returning
        (best effort): the form meant for use. An explicit s (a canonical int or Montgomery limbs)
        is for tests. PlonkError(PLK_E_ARG) for s = 0, s >= r, fewer than 2 points, or a point
        that is not on the curve or not in G1 (bad_index then names the smallest such index)."""
        sp = None if s is None else _ptr(_fr_limbs(s))
        h, k, idx = C.c_void_p(), C.c_void_p(), C.c_uint64(0xFFFFFFFFFFFFFFFF)
        wit = np.zeros(G2_WORDS, dtype=np.uint64)
        st = _lib().plk_srs_update(self._h, opening_key._h, sp, C.byref(h), C.byref(k), _ptr(wit),
                                   C.byref(idx))
        if st == PLK_E_ARG and idx.value != 0xFFFFFFFFFFFFFFFF:
            raise PlonkError(st, f"plk_srs_update: point {idx.value} is not a point of G1",
                             bad_index=idx.value)
        _check(st, "plk_srs_update")
        return PlonkParams(h, self.n, self.ctx), OpeningKey(k), wit

    def verify_update(self, prev_tau_g1, opening_key: "OpeningKey", witness,
                      seed: bytes | None = None) -> "SrsVerdict":
        """Is this SRS with `opening_key` a well-formed SRS whose tau is the previous string's
        times the secret behind `witness`? prev_tau_g1: points()[1] of the string that was updated
        (uint64[13]). plk_srs_verify_update: SRS_WITNESS, then every class of verify(), then
        SRS_LINK. A bad update is a verdict, never an exception."""
        prev = np.ascontiguousarray(np.asarray(prev_tau_g1, dtype=np.uint64).reshape(13))
        wit = np.ascontiguousarray(np.asarray(witness, dtype=np.uint64).reshape(G2_WORDS))
        verdict, idx = C.c_int(-1), C.c_uint64(0xFFFFFFFFFFFFFFFF)
        sd = None if seed is None else _ptr(_seed32(seed))
        _check(_lib().plk_srs_verify_update(self.ctx.handle, _ptr(prev), self._h, opening_key._h,
                                            _ptr(wit), sd, C.byref(verdict), C.byref(idx)),
               "plk_srs_verify_update")
        bad = idx.value if verdict.value in (SRS_POINT, SRS_SUBGROUP, SRS_INFINITY) else None
        return SrsVerdict(verdict.value == SRS_OK, verdict.value, bad)

    def last_verify_ms(self):
        """(fold ms, pairing ms) of the most recent verify() that reached the fold (host wall time)."""
        a, b = C.c_double(), C.c_double()
        _check(_lib().plk_srs_last_verify_ms(self._h, C.byref(a), C.byref(b)), "plk_srs_last_verify_ms")
        return a.value, b.value

    def lagrange(self, k: int) -> "PlonkParams":
        """The Lagrange-basis SRS of the 2^k domain (plk_srs_lagrange): 2^k + 3 points, the
        last three for a blinder b(X)(X^n - 1). commit([p(w^0) .. p(w^(n-1)), b0, b1, b2]) on it
        equals commit(p + b (X^n - 1)) on this SRS, which must hold 2^k + 3 points."""
        f = _lib().plk_srs_lagrange  # bound on use: a PLK_LIB build from before it still loads
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        _check(f(self._h, k, C.byref(h)), "plk_srs_lagrange")
        return PlonkParams(h, (1 << k) + 3, self.ctx)

    def trim(self, n: int) -> "PlonkParams":
        """Keep the first n + SLACK powers (key.rs:81-82)."""
        keep = min(self.n, n + self.SLACK)
        if keep == self.n:
            return self
        return PlonkParams.load(self.points(0, keep), self.ctx)

    def points(self, start: int = 0, count: int | None = None) -> np.ndarray:
        count = self.n - start if count is None else count
        out = np.zeros((count, 13), dtype=np.uint64)
        _check(_lib().plk_srs_points(self._h, start, count, _ptr(out)), "plk_srs_points")
        return out

    def commit(self, poly: Coefficients) -> Commitment:
        vals = _as_fr_array(poly.values if isinstance(poly, Coefficients) else poly)
        out = np.zeros(13, dtype=np.uint64)
        _check(_lib().plk_commit(self._h, _ptr(vals), vals.shape[0], _ptr(out)), "commit")
        return Commitment(out)

    def msm(self, scalars) -> Commitment:
        vals = _as_fr_array(scalars)
        out = np.zeros(13, dtype=np.uint64)
        _check(_lib().plk_msm(self._h, _ptr(vals), vals.shape[0], _ptr(out)), "msm")
        return Commitment(out)

    def msm_points(self, points, scalars) -> Commitment:
        """msm_curve_addition over arbitrary points (not this SRS) on this SRS's context."""
        return msm_points(points, scalars, self.ctx)

    def commit_dev(self, d_ptr: int, length: int, stream: int = 0) -> Commitment:
        out = np.zeros(13, dtype=np.uint64)
        _check(_lib().plk_commit_dev(self._h, C.c_void_p(d_ptr), length, _ptr(out),
                                     C.c_void_p(stream or None)), "commit_dev")
        return Commitment(out)

    def commit_batch_dev(self, ptrs_lens, stream: int = 0, raise_on_error: bool = True,
                         part: int = 0, parts: int = 1):
        """Commit several device-resident polynomials [(ptr, len), ...] as one batch.
        Returns a list of Commitment (or PlonkError per failed slot when not raising).
        parts > 1: only bucket range `part` of `parts` (plk_commit_batch_dev_part): the
        returned points are that range's shares, which sum over the parts to the commits."""
        k = len(ptrs_lens)
        ptrs = (C.c_void_p * k)(*[C.c_void_p(p) for p, _ in ptrs_lens])
        lens = (C.c_size_t * k)(*[n for _, n in ptrs_lens])
        outs = np.zeros((k, 13), dtype=np.uint64)
        sts = (C.c_int * k)()
        if parts == 1:
            st = _lib().plk_commit_batch_dev(self._h, ptrs, lens, k, _ptr(outs), sts,
                                             C.c_void_p(stream or None))
        else:
            st = _lib().plk_commit_batch_dev_part(self._h, ptrs, lens, k, part, parts, _ptr(outs),
                                                  sts, C.c_void_p(stream or None))
        if st not in (PLK_OK, PLK_E_DEGREE) or (raise_on_error and st != PLK_OK):
            raise PlonkError(st, "commit_batch_dev")
        return [Commitment(outs[i]) if sts[i] == PLK_OK else PlonkError(sts[i], "commit")
                for i in range(k)]

    def compute_aggregate_witness(self, polys, point, challenge) -> Coefficients:
        """PlonkParams::compute_aggregate_witness (prover.rs:422-450):
        (sum_i challenge^i polys[i]) / (X - point), remainder dropped (plk_aggregate_witness)."""
        arrs = [_as_fr_array(p.values if isinstance(p, Coefficients) else p) for p in polys]
        k = len(arrs)
        ptrs = (C.c_void_p * max(k, 1))(*[C.c_void_p(a.ctypes.data) for a in arrs])
        lens = (C.c_size_t * max(k, 1))(*[a.shape[0] for a in arrs])
        pt = _as_fr_array(point).reshape(4)
        ch = _as_fr_array(challenge).reshape(4)
        m = max((a.shape[0] for a in arrs), default=0)
        out = np.zeros((max(m - 1, 1), 4), dtype=np.uint64)
        n_out = C.c_size_t()
        _check(_lib().plk_aggregate_witness(self.ctx.handle, ptrs, lens, k, _ptr(pt), _ptr(ch),
                                            _ptr(out), C.byref(n_out)), "compute_aggregate_witness")
        return Coefficients(out[: n_out.value])

    def open(self, poly, points):
        """Open one polynomial at arbitrary points (plk_kzg_open): (values uint64[m, 4], witnesses
        uint64[m, 13]) with values[j] = poly(points[j]) and witnesses[j] the commitment to
        (poly - values[j]) / (X - points[j]). PlonkError(PLK_E_DEGREE) when the polynomial is
        longer than the SRS, PLK_E_ARG for a scalar >= r."""
        vals = _as_fr_array(poly.values if isinstance(poly, Coefficients) else poly)
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 4))
        m = pts.shape[0]
        values = np.zeros((max(m, 1), 4), dtype=np.uint64)
        wit = np.zeros((max(m, 1), 13), dtype=np.uint64)
        _check(_lib().plk_kzg_open(self._h, _ptr(vals), vals.shape[0], _ptr(pts), m, _ptr(values),
                                   _ptr(wit)), "plk_kzg_open")
        return values[:m], wit[:m]

    def open_domain(self, k: int, poly):
        """Open one polynomial of at most 2^k coefficients at every point of the 2^k domain
        (plk_kzg_open_domain, Feist-Khovratovich on the GPU): (PointsValue of the values,
        witnesses uint64[2^k, 13]), entry i for Fft(k).generator^i. The first call per k builds
        and caches a table of 2^(k+1) points in this SRS. PlonkError(PLK_E_ARG) with bad_index
        when an SRS point is not in G1."""
        vals = _as_fr_array(poly.values if isinstance(poly, Coefficients) else poly)
        n = 1 << k if 1 <= k <= 20 else 1  # outside the range the library refuses before it writes
        values = np.zeros((n, 4), dtype=np.uint64)
        wit = np.zeros((n, 13), dtype=np.uint64)
        idx = C.c_uint64(0xFFFFFFFFFFFFFFFF)
        st = _lib().plk_kzg_open_domain(self._h, k, _ptr(vals), vals.shape[0], _ptr(values), _ptr(wit),
                                        C.byref(idx))
        if st == PLK_E_ARG and idx.value != 0xFFFFFFFFFFFFFFFF:
            raise PlonkError(st, f"plk_kzg_open_domain: point {idx.value} is not a point of G1",
                             bad_index=idx.value)
        _check(st, "plk_kzg_open_domain")
        return PointsValue(values), wit

    def open_cosets(self, k: int, log_l: int, poly):
        """Open one polynomial of at most n = 2^k coefficients on every coset of l = 2^log_l points
        of the 2^k domain (plk_kzg_open_cosets, the Feist-Khovratovich multiproofs on the GPU):
        (PointsValue of the n values in the domain's natural order, witnesses uint64[r, 13]),
        r = n / l. Witness j is the commitment to poly div (X^l - w^(l j)), one point for the l
        values values.cosets(log_l)[j] on the coset w^j <w^r>, w = Fft(k).generator. log_l = 0
        is open_domain. The first call per (k, log_l) builds and caches a table of 2^(k+1) points
        in this SRS. Verify with OpeningKey.check_cosets on the key of tau^l.
        PlonkError(PLK_E_ARG) with bad_index when an SRS point is not in G1."""
        vals = _as_fr_array(poly.values if isinstance(poly, Coefficients) else poly)
        ok = 1 <= k <= 20 and 0 <= log_l <= k  # outside the range the library refuses before it writes
        n = 1 << k if ok else 1
        values = np.zeros((n, 4), dtype=np.uint64)
        wit = np.zeros((n >> log_l if ok else 1, 13), dtype=np.uint64)
        idx = C.c_uint64(0xFFFFFFFFFFFFFFFF)
        st = _lib().plk_kzg_open_cosets(self._h, k, log_l if log_l >= 0 else 0xFFFFFFFF, _ptr(vals),
                                        vals.shape[0], _ptr(values), _ptr(wit), C.byref(idx))
        if st == PLK_E_ARG and idx.value != 0xFFFFFFFFFFFFFFFF:
            raise PlonkError(st, f"plk_kzg_open_cosets: point {idx.value} is not a point of G1",
                             bad_index=idx.value)
        _check(st, "plk_kzg_open_cosets")
        return PointsValue(values), wit

    def power_key_matches(self, key: "OpeningKey", log_l: int) -> bool:
        """Is `key` the opening key of tau^l, l = 2^log_l, for this SRS's tau? e(g1[l], H) ==
        e(g1[0], key.beta_h) through plk_pairing_check on the pair (g1[l], g1[0]): a key read
        from a ceremony's G2 powers need not be taken on faith before OpeningKey.check_cosets
        relies on it. The SRS must hold more than l points."""
        l = 1 << log_l
        if l >= self.n:
            raise PlonkError(PLK_E_ARG, "power_key_matches: the SRS holds no point g1[2^log_l]")
        return key.check(np.stack([self.points(l, 1)[0], self.points(0, 1)[0]]))

    def open_multiple(self, polys, point, challenge):
        """The reference's aggregate opening (commitment_scheme.rs open_multiple): (values
        uint64[t, 4] of every polynomial at `point`, the Commitment to
        (sum_i challenge^i polys[i]) / (X - point)). Composed from compute_aggregate_witness and
        commit; the values through open()."""
        pt = _as_fr_array(point).reshape(1, 4)
        values = np.stack([self.open(p, pt)[0][0] for p in polys])
        w = self.compute_aggregate_witness(polys, point, challenge)
        return values, self.commit(w)

    def compute_aggregate_witness_dev(self, ptrs_lens, point, challenge, d_out: int,
                                      stream: int = 0) -> int:
        """Device form (plk_aggregate_witness_dev): [(ptr, len)] -> d_out; returns its length."""
        k = len(ptrs_lens)
        ptrs = (C.c_void_p * max(k, 1))(*[C.c_void_p(p) for p, _ in ptrs_lens])
        lens = (C.c_size_t * max(k, 1))(*[n for _, n in ptrs_lens])
        pt = _as_fr_array(point).reshape(4)
        ch = _as_fr_array(challenge).reshape(4)
        n_out = C.c_size_t()
        _check(_lib().plk_aggregate_witness_dev(self.ctx.handle, ptrs, lens, k, _ptr(pt), _ptr(ch),
                                                C.c_void_p(d_out or None), C.byref(n_out),
                                                C.c_void_p(stream or None)),
               "compute_aggregate_witness_dev")
        return n_out.value

    def msm_stats_reset(self):
        _check(_lib().plk_srs_msm_stats_reset(self._h), "plk_srs_msm_stats_reset")

    def cum_msm_stats(self):
        """(accumulate ms, launches, point adds, MSM points) since msm_stats_reset."""
        ms, ln, adds, pts = C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(_lib().plk_srs_cum_msm_stats(self._h, C.byref(ms), C.byref(ln), C.byref(adds),
                                            C.byref(pts)), "plk_srs_cum_msm_stats")
        return ms.value, ln.value, adds.value, pts.value

    def last_msm_stats(self):
        ms, adds, c = C.c_float(), C.c_uint64(), C.c_uint32()
        _check(_lib().plk_srs_last_msm_stats(self._h, C.byref(ms), C.byref(adds), C.byref(c)),
               "plk_srs_last_msm_stats")
        return ms.value, adds.value, c.value

    def table_layout(self) -> dict:
        """The MSM table this SRS got: {"naf": row table (True) or window table, "rows",
        "table_bytes"} (plk_srs_table_layout)."""
        naf, rows, nbytes = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(_lib().plk_srs_table_layout(self._h, C.byref(naf), C.byref(rows), C.byref(nbytes)),
               "plk_srs_table_layout")
        return {"naf": bool(naf.value), "rows": rows.value, "table_bytes": nbytes.value}

    def __del__(self):
        try:
            if self._h and _LIB is not None:
                _LIB.plk_srs_destroy(self._h)
        except Exception:
            pass
        self._h = None


# ------------------------------------------------------------------- opening key, pairing
G2_WORDS = 25  # plk_g2: x.c0, x.c1, y.c0, y.c1 (6 Montgomery u64 limbs each) + the infinity flag
_FR_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _as_pairs(pairs) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint64))
    if a.ndim == 2 and a.shape == (2, 13):
        a = a.reshape(1, 2, 13)
    if a.ndim != 3 or a.shape[1:] != (2, 13):
        raise ValueError("expected uint64[n, 2, 13]: (C, W) ABI points per pair")
    return a


class OpeningKey:
    """The G2 half of the reference's EvaluationKey: H and beta_h = [tau]H with their Miller-loop
    lines prepared on the host (plk_opening_key). Points are uint64[25] rows in plk_g2 layout."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def setup(cls, tau) -> "OpeningKey":
        """H = the G2 generator, beta_h = [tau]H; tau: a canonical int or uint64[4] Montgomery
        limbs (the explicit trapdoor of PlonkParams.setup)."""
        if isinstance(tau, (int, np.integer)):
            m = (int(tau) % _FR_MOD) * (1 << 256) % _FR_MOD
            limbs = np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        else:
            limbs = np.ascontiguousarray(np.asarray(tau, dtype=np.uint64).reshape(4))
        h = C.c_void_p()
        _check(_lib().plk_opening_key_setup(_ptr(limbs), C.byref(h)), "OpeningKey::setup")
        return cls(h)

    @classmethod
    def load(cls, h, beta_h) -> "OpeningKey":
        """An existing key; PlonkError(PLK_E_ARG) for a non-canonical limb, a point off the twist,
        a point outside the order-r subgroup or the point at infinity."""
        a = np.ascontiguousarray(np.asarray(h, dtype=np.uint64).reshape(G2_WORDS))
        b = np.ascontiguousarray(np.asarray(beta_h, dtype=np.uint64).reshape(G2_WORDS))
        out = C.c_void_p()
        _check(_lib().plk_opening_key_load(_ptr(a), _ptr(b), C.byref(out)), "OpeningKey::load")
        return cls(out)

    @classmethod
    def from_bytes(cls, h: bytes, beta_h: bytes, fmt: str = "compressed") -> "OpeningKey":
        """A key from zkcrypto's G2 byte forms (96 bytes per point compressed, 192 uncompressed;
        plk_opening_key_load_bytes). Strict decoding, then every check of load()."""
        size = 96 if _FORMATS[fmt] == 0 else 192
        a, b = np.frombuffer(bytes(h), dtype=np.uint8), np.frombuffer(bytes(beta_h), dtype=np.uint8)
        if a.size != size or b.size != size:
            raise PlonkError(PLK_E_ARG, f"OpeningKey.from_bytes: {size} bytes per point")
        out = C.c_void_p()
        _check(_lib().plk_opening_key_load_bytes(_ptr(a), _ptr(b), _FORMATS[fmt], C.byref(out)),
               "OpeningKey::from_bytes")
        return cls(out)

    def update(self, s):
        """(new OpeningKey, witness): the same H with beta_h' = [s] beta_h, and witness = [s]H as
        uint64[25] (plk_opening_key_update, host only). s: a canonical int or Montgomery limbs;
        PlonkError(PLK_E_ARG) for 0 or a value >= r."""
        out, wit = C.c_void_p(), np.zeros(G2_WORDS, dtype=np.uint64)
        _check(_lib().plk_opening_key_update(self._h, _ptr(_fr_limbs(s)), C.byref(out), _ptr(wit)),
               "plk_opening_key_update")
        return OpeningKey(out), wit

    def to_bytes(self, fmt: str = "compressed"):
        """(H, beta_h) in zkcrypto's G2 byte form (plk_opening_key_to_bytes)."""
        size = 96 if _FORMATS[fmt] == 0 else 192
        a, b = np.zeros(size, dtype=np.uint8), np.zeros(size, dtype=np.uint8)
        _check(_lib().plk_opening_key_to_bytes(self._h, _FORMATS[fmt], _ptr(a), _ptr(b)),
               "plk_opening_key_to_bytes")
        return a.tobytes(), b.tobytes()

    def points(self):
        """(H, beta_h) as uint64[25] rows."""
        a, b = np.zeros(G2_WORDS, dtype=np.uint64), np.zeros(G2_WORDS, dtype=np.uint64)
        _check(_lib().plk_opening_key_points(self._h, _ptr(a), _ptr(b)), "plk_opening_key_points")
        return a, b

    def check(self, pair) -> bool:
        """e(C, H) == e(W, beta_h) on the host (plk_pairing_check); pair: (C, W) as uint64[2, 13]."""
        a = _as_pairs(pair)
        ok = C.c_int(0)
        _check(_lib().plk_pairing_check(self._h, _ptr(a), C.byref(ok)), "plk_pairing_check")
        return bool(ok.value)

    def check_batch(self, pairs, ctx: "Context | None" = None) -> np.ndarray:
        """The same check for uint64[n, 2, 13] pairs on the GPU, one pair per lane
        (plk_pairing_check_batch): bool[n]."""
        a = _as_pairs(pairs)
        ctx = ctx or Context.default()
        ok = np.zeros(a.shape[0], dtype=np.uint8)
        _check(_lib().plk_pairing_check_batch(ctx.handle, self._h, _ptr(a), a.shape[0], _ptr(ok)),
               "plk_pairing_check_batch")
        return ok.astype(bool)

    def fold_openings(self, g, commitments, points, values, witnesses, weights=None,
                      ctx: "Context | None" = None) -> np.ndarray:
        """(C, W) as uint64[2, 13] for n openings (commitments uint64[n, 13], points and values
        uint64[n, 4], witnesses uint64[n, 13]) of commitments on the base point g (uint64[13]):
        C = sum rho_k (C_k - y_k g + z_k W_k), W = sum rho_k W_k (plk_kzg_fold). weights=None draws
        128-bit weights inside the library (the sound form); explicit weights uint64[n, 4] are for
        callers with their own Fiat-Shamir. All openings hold iff check((C, W)), up to 2^-128."""
        ctx = ctx or Context.default()
        gp = np.ascontiguousarray(np.asarray(g, dtype=np.uint64).reshape(13))
        cm = np.ascontiguousarray(np.asarray(commitments, dtype=np.uint64).reshape(-1, 13))
        n = cm.shape[0]
        zs = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 4))
        ys = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1, 4))
        ws = np.ascontiguousarray(np.asarray(witnesses, dtype=np.uint64).reshape(-1, 13))
        if not (zs.shape[0] == ys.shape[0] == ws.shape[0] == n):
            raise ValueError("fold_openings: one point, value and witness per commitment")
        wp = None
        if weights is not None:
            wt = np.ascontiguousarray(np.asarray(weights, dtype=np.uint64).reshape(-1, 4))
            if wt.shape[0] != n:
                raise ValueError("fold_openings: one weight per opening")
            wp = _ptr(wt)
        out = np.zeros((2, 13), dtype=np.uint64)
        _check(_lib().plk_kzg_fold(ctx.handle, _ptr(gp), _ptr(cm), _ptr(zs), _ptr(ys), _ptr(ws), n, wp,
                                   _ptr(out)), "plk_kzg_fold")
        return out

    def check_openings(self, g, commitments, points, values, witnesses, weights=None,
                       ctx: "Context | None" = None) -> bool:
        """Do all the openings hold? fold_openings, then check on the pair."""
        return self.check(self.fold_openings(g, commitments, points, values, witnesses, weights, ctx))

    def fold_cosets(self, pp: "PlonkParams", log_l: int, commitments, shifts, values, witnesses,
                    weights=None) -> np.ndarray:
        """(C, W) as uint64[2, 13] for n coset openings on the SRS pp (plk_kzg_fold_cosets):
        opening k says that the polynomial committed in commitments[k] takes the l = 2^log_l
        values[k] (uint64[n, l, 4], row k = f(z_k w^i), i < l, w the l-point domain's generator;
        a row of PointsValue.cosets(log_l)) on the coset z_k <w>, z_k = shifts[k] any non-zero
        scalar (for PlonkParams.open_cosets: Fft(k).generator^j for coset j), with the witness
        witnesses[k]. One commitment (uint64[13]) may stand for all openings.
        C = sum rho_k (C_k + z_k^l W_k) - sum_i P_i g1[i], W = sum rho_k W_k, the interpolants
        reduced to the l scalars P_i on the GPU. All openings hold iff check((C, W)) on the key
        of tau^l, up to 2^-128: self must be OpeningKey.setup(tau^l) or a ceremony's l-th G2
        power (OpeningKey.load / from_bytes; PlonkParams.power_key_matches tells), NOT the key
        of tau that check_openings wants. After an SRS update by s that key follows by
        update(s^l) (plk_opening_key_update(key_l, s^l)). weights as fold_openings."""
        l = 1 << log_l if 0 <= log_l <= 20 else 1  # outside the range the library refuses
        zs = np.ascontiguousarray(np.asarray(shifts, dtype=np.uint64).reshape(-1, 4))
        n = zs.shape[0]
        cm = np.ascontiguousarray(np.asarray(commitments, dtype=np.uint64).reshape(-1, 13))
        if cm.shape[0] == 1 and n > 1:
            cm = np.ascontiguousarray(np.tile(cm, (n, 1)))
        ys = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1, 4))
        ws = np.ascontiguousarray(np.asarray(witnesses, dtype=np.uint64).reshape(-1, 13))
        if not (cm.shape[0] == ws.shape[0] == n and ys.shape[0] == n * l):
            raise ValueError("fold_cosets: one shift, witness and row of 2^log_l values per opening")
        wp = None
        if weights is not None:
            wt = np.ascontiguousarray(np.asarray(weights, dtype=np.uint64).reshape(-1, 4))
            if wt.shape[0] != n:
                raise ValueError("fold_cosets: one weight per opening")
            wp = _ptr(wt)
        out = np.zeros((2, 13), dtype=np.uint64)
        _check(_lib().plk_kzg_fold_cosets(pp._h, log_l, _ptr(cm), _ptr(zs), _ptr(ys), _ptr(ws), n, wp,
                                          _ptr(out)), "plk_kzg_fold_cosets")
        return out

    def check_cosets(self, pp: "PlonkParams", log_l: int, commitments, shifts, values, witnesses,
                     weights=None) -> bool:
        """Do all the coset openings hold? fold_cosets, then check on the pair; self is the key
        of tau^l (see fold_cosets)."""
        return self.check(self.fold_cosets(pp, log_l, commitments, shifts, values, witnesses, weights))

    def last_pairing_ms(self) -> float:
        """HIP-event milliseconds of the pairing kernel of the most recent device check."""
        a = C.c_float()
        _check(_lib().plk_opening_key_last_pairing_ms(self._h, C.byref(a)), "plk_opening_key_last_pairing_ms")
        return a.value

    def __del__(self):
        try:
            if self._h:
                _lib().plk_opening_key_destroy(self._h)
        except Exception:
            pass
        self._h = None


def debug_f2_sqrt(a):
    """Test support (plk_debug_f2_sqrt): the host Fp2 square root. a: uint64[12] (c0, c1 Montgomery
    limbs) -> (root uint64[12], is_square)."""
    v = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(12))
    out, ok = np.zeros(12, dtype=np.uint64), C.c_int(0)
    _check(_lib().plk_debug_f2_sqrt(_ptr(v), _ptr(out), C.byref(ok)), "plk_debug_f2_sqrt")
    return out, bool(ok.value)


def debug_pairing(points, q, ctx: "Context | None" = None) -> np.ndarray:
    """Test support (plk_debug_pairing): e(p_i, q)^3 for uint64[n, 13] G1 points and one uint64[25]
    G2 point, as uint64[n, 72] (six Fp2 coefficients of w^0 .. w^5, Montgomery limbs). ctx = None:
    the host code; otherwise the kernel."""
    a = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 13))
    g = np.ascontiguousarray(np.asarray(q, dtype=np.uint64).reshape(G2_WORDS))
    out = np.zeros((a.shape[0], 72), dtype=np.uint64)
    _check(_lib().plk_debug_pairing(None if ctx is None else ctx.handle, _ptr(a), _ptr(g), a.shape[0],
                                    _ptr(out)), "plk_debug_pairing")
    return out


# plk_debug_f12_op's op codes (include/plk.h)
F12_OPS = {"f2_mul": 0, "f2_sqr": 1, "f2_inv": 2, "f2_mul_xi": 3, "mul": 4, "sqr": 5, "cyc_sqr": 6,
           "inv_even": 7, "conj": 8, "frob1": 9, "frob2": 10, "mul_line": 11, "final_exp": 12}
F12_IN_PLACE = 0x100


def debug_f12_op(op, a, b=None, ctx: "Context | None" = None, in_place: bool = False) -> np.ndarray:
    """Test support (plk_debug_f12_op): one operation of the pairing's tower (a name of F12_OPS) on
    uint64[n, 72] rows (debug_pairing's layout); b: the second operand's rows for f2_mul and mul,
    (c0, c2, y) in limbs 0..29 for mul_line. in_place: conj / frob1 / frob2 on the operand's own
    slot. ctx = None: the host code; otherwise the kernel. uint64[n, 72]."""
    x = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, 72))
    y = None
    if b is not None:
        y = np.ascontiguousarray(np.asarray(b, dtype=np.uint64).reshape(-1, 72))
        if y.shape != x.shape:
            raise PlonkError(PLK_E_ARG, "debug_f12_op: a and b hold the same number of rows")
    out = np.zeros_like(x)
    code = F12_OPS[op] | (F12_IN_PLACE if in_place else 0)
    _check(_lib().plk_debug_f12_op(None if ctx is None else ctx.handle, code, _ptr(x),
                                   None if y is None else _ptr(y), x.shape[0], _ptr(out)),
           "plk_debug_f12_op")
    return out


def debug_miller(p0, q0, p1=None, q1=None, ctx: "Context | None" = None) -> np.ndarray:
    """Test support (plk_debug_miller): the raw Miller value ML(p0_i, q0), or with p1 / q1 the
    check's ML(p0_i, q0) ML(-p1_i, q1), for uint64[n, 13] G1 points and uint64[25] G2 points, as
    uint64[n, 72]. ctx = None: the host code; otherwise the kernel."""
    a = np.ascontiguousarray(np.asarray(p0, dtype=np.uint64).reshape(-1, 13))
    g0 = np.ascontiguousarray(np.asarray(q0, dtype=np.uint64).reshape(G2_WORDS))
    c = g1 = None
    if p1 is not None:
        c = np.ascontiguousarray(np.asarray(p1, dtype=np.uint64).reshape(-1, 13))
        g1 = np.ascontiguousarray(np.asarray(q1, dtype=np.uint64).reshape(G2_WORDS))
        if c.shape != a.shape:
            raise PlonkError(PLK_E_ARG, "debug_miller: p0 and p1 hold the same number of points")
    out = np.zeros((a.shape[0], 72), dtype=np.uint64)
    _check(_lib().plk_debug_miller(None if ctx is None else ctx.handle, _ptr(a), _ptr(g0),
                                   None if c is None else _ptr(c), None if g1 is None else _ptr(g1),
                                   a.shape[0], _ptr(out)), "plk_debug_miller")
    return out


# plk_msm_snapshot of include/plk.h and the names of its header words
MSM_SNAPSHOT_HDR = ("B", "W", "narrow", "c", "chunk", "rb", "fb", "NC", "NR", "G", "nbits", "nout",
                    "wide", "sort_one", "hold", "task_stride", "sorted_stride", "max_tasks_used",
                    "b_lo", "n_srs", "gen", "part", "parts", "has_inf")
_MSM_SNAPSHOT_BUFS = ("offsets", "task_off", "sorted", "tasks", "partials", "bsum", "rsum", "ys",
                      "zs", "bits", "readback")


class _MsmSnapshot(C.Structure):
    _fields_ = ([(n, C.c_uint32) for n in ("shared_chip", "tail_quad", "part", "parts",
                                           "guard_limit", "reserved")] +
                [("cap_sorted", C.c_uint64), ("cap_tasks", C.c_uint64)] +
                [(n, C.c_void_p) for n in _MSM_SNAPSHOT_BUFS] +
                [("hdr", C.c_uint64 * len(MSM_SNAPSHOT_HDR)), ("n_tasks", C.c_uint32 * 16)])


def debug_msm_snapshot(pp: "PlonkParams", slots, shared_chip: bool = False, tail_quad: int = 1,
                       part: int = 0, parts: int = 1, guard_limit: int = 0, points: bool = True):
    """Test support (plk_debug_msm_snapshot): one fixed-base MSM batch over `slots` (1..16 arrays of
    Montgomery scalars, uint64[len, 4]) on a workspace of its own, and what the batch left there.
    Returns (hdr, per-slot dicts): hdr maps MSM_SNAPSHOT_HDR to integers; a slot holds offsets,
    task_off (uint32[B + 1]), sorted (uint32[entries]), tasks (uint32[n, 2]), flag, entries,
    max_count, bits (uint32[nout, 48]), point (uint64[13]), status, and with points=True partials
    (uint32[n, 48]) and bsum (uint32[B, 48]) or rsum, ys, zs (uint32[B | NR, 48]). The batch runs
    twice: once for the header that sizes the buffers, once for the buffers."""
    arrs = [_as_fr_array(s) for s in slots]
    k = len(arrs)
    ptrs = (C.c_void_p * max(k, 1))(*[C.c_void_p(a.ctypes.data if a.shape[0] else None) for a in arrs])
    lens = (C.c_size_t * max(k, 1))(*[a.shape[0] for a in arrs])
    outs = np.zeros((max(k, 1), 13), dtype=np.uint64)
    sts = (C.c_int * max(k, 1))()

    def call(snap):
        snap.shared_chip, snap.tail_quad = int(bool(shared_chip)), tail_quad
        snap.part, snap.parts, snap.guard_limit = part, parts, guard_limit
        st = _lib().plk_debug_msm_snapshot(pp._h, ptrs, lens, k, C.byref(snap), _ptr(outs), sts)
        if st not in (PLK_OK, PLK_E_DEGREE):
            raise PlonkError(st, "plk_debug_msm_snapshot")
        return dict(zip(MSM_SNAPSHOT_HDR, (int(v) for v in snap.hdr)))

    h = call(_MsmSnapshot())
    B, NR, nout = h["B"], h["NR"], h["nout"]
    cap_sorted = max(1, h["W"] * max(a.shape[0] for a in arrs))
    cap_tasks = h["max_tasks_used"] + 1
    u32 = np.uint32
    bufs = {"offsets": np.zeros((k, B + 1), u32), "task_off": np.zeros((k, B + 1), u32),
            "sorted": np.zeros((k, cap_sorted), u32), "tasks": np.zeros((k, cap_tasks, 2), u32),
            "bits": np.zeros((k, nout, 48), u32), "readback": np.zeros((k, 3), u32)}
    if points:
        bufs["partials"] = np.zeros((k, cap_tasks, 48), u32)
        if h["wide"]:
            bufs.update(rsum=np.zeros((k, B, 48), u32), ys=np.zeros((k, NR, 48), u32),
                        zs=np.zeros((k, NR, 48), u32))
        else:
            bufs["bsum"] = np.zeros((k, B, 48), u32)
    snap = _MsmSnapshot()
    snap.cap_sorted, snap.cap_tasks = cap_sorted, cap_tasks
    for name, a in bufs.items():
        setattr(snap, name, a.ctypes.data)
    h2 = call(snap)
    assert h2 == h, (h, h2)
    out = []
    for i in range(k):
        n, ent = int(snap.n_tasks[i]), int(bufs["offsets"][i, B])
        d = {"offsets": bufs["offsets"][i], "task_off": bufs["task_off"][i],
             "sorted": bufs["sorted"][i, :ent], "tasks": bufs["tasks"][i, :n],
             "bits": bufs["bits"][i], "flag": int(bufs["readback"][i, 0]),
             "entries": int(bufs["readback"][i, 1]), "max_count": int(bufs["readback"][i, 2]),
             "point": outs[i].copy(), "status": int(sts[i])}
        if points:
            d["partials"] = bufs["partials"][i, :n]
            for name in ("bsum", "rsum", "ys", "zs"):
                if name in bufs:
                    d[name] = bufs[name][i]
        out.append(d)
    return h, out
