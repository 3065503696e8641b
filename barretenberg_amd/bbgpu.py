"""ctypes mirror of the reference's operator interface for the hot path, over the C ABI of libbbgpu.so.

Names follow the reference: ``pippenger`` / ``batched_scalar_multiplications``
(src/barretenberg/curves/bn254/scalar_multiplication.hpp:60-96) and ``fft`` / ``ifft`` / ``coset_fft`` / ``coset_ifft`` /
``fft_with_constant`` / ``ifft_with_constant`` / ``coset_fft_with_constant``
(src/barretenberg/polynomials/polynomial_arithmetic.hpp:27-41).  Arrays are numpy uint64 in the reference's memory
layout: field element (4,), affine point (8,), Jacobian (12,).  Device-resident variants take raw device pointers
(e.g. ``torch.Tensor.data_ptr()``); torch is plumbing only.
"""
import ctypes as C
import os
import subprocess

import numpy as np

try:  # plumbing: when torch is around, let it load ITS HIP runtime first so that device pointers handed over from torch
    import torch  # noqa: F401  tensors and libbbgpu.so share one runtime (two runtimes in one process cannot both see the GPU)
except Exception:  # pragma: no cover - torch is optional for the library itself
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
# The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); kernels of two streams that share a queue run one
# after the other.  The library's MSM slots want their own queues (libbbgpu sets the same default when it makes the process's first HIP call);
# effective only if HIP has not been initialised yet -- import this module before torch touches the GPU, or export the variable.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
u64p = C.POINTER(C.c_uint64)

NTT_KINDS = {
    "fft": 0,
    "ifft": 1,
    "coset_fft": 2,
    "coset_ifft": 3,
    "fft_with_constant": 4,
    "ifft_with_constant": 5,
    "coset_fft_with_constant": 6,
}

C_ABI_SYMBOLS = [
    "bbgpu_init", "bbgpu_shutdown", "bbgpu_device_count", "bbgpu_last_error", "bbgpu_version", "bbgpu_ntt",
    "bbgpu_ntt_device", "bbgpu_ntt_device_batch", "bbgpu_srs_register", "bbgpu_srs_release", "bbgpu_srs_generate", "bbgpu_srs_generate_range", "bbgpu_set_precompute",
    "bbgpu_srs_num_windows", "bbgpu_transcript_read_g1", "bbgpu_transcript_write", "bbgpu_msm_g1", "bbgpu_msm_g1_plain",
    "bbgpu_msm_g1_batch", "bbgpu_msm_num_windows", "bbgpu_msm_g1_device", "bbgpu_msm_g1_device_async", "bbgpu_msm_g1_device_rows_async", "bbgpu_msm_g1_device_buckets_async", "bbgpu_srs_has_window_tables", "bbgpu_msm_g1_wait",
    "bbgpu_msm_g1_device_batch_async", "bbgpu_msm_g1_batch_wait",
    "bbgpu_g1_sum", "bbgpu_last_timing", "bbgpu_set_host_thresholds", "bbgpu_srs_cache_stats", "bbgpu_set_table_share", "bbgpu_set_point_share", "bbgpu_selftest_field", "bbgpu_selftest_g1",
    "bbgpu_set_timing",
    "bbgpu_fr_evaluate_device", "bbgpu_fr_batch_invert_device", "bbgpu_fr_product_scan_device", "bbgpu_fr_mul_device",
    "bbgpu_kate_opening_device", "bbgpu_lagrange_l1_fft_device", "bbgpu_divide_by_pseudo_vanishing_device",
    "bbgpu_permutation_lagrange_base_device",
    "bbgpu_fr_evaluate", "bbgpu_kate_opening", "bbgpu_lagrange_l1_fft", "bbgpu_divide_by_pseudo_vanishing", "bbgpu_lagrange_evaluations",
    "bbgpu_generate_point_table",
    "bbgpu_plonk_prover_create", "bbgpu_plonk_prover_set_witness", "bbgpu_plonk_construct_proof", "bbgpu_plonk_preprocess", "bbgpu_plonk_last_challenges",
    "bbgpu_plonk_last_timing", "bbgpu_plonk_prover_destroy", "bbgpu_plonk_challenges_from_proof",
    "bbgpu_plonk_construct_proof_batch", "bbgpu_plonk_batch_challenges", "bbgpu_plonk_last_batch_timing",
    "bbgpu_host_msm_g1", "bbgpu_host_ntt", "bbgpu_host_fr_evaluate", "bbgpu_host_kate_opening", "bbgpu_host_lagrange_l1_fft",
    "bbgpu_host_divide_by_pseudo_vanishing", "bbgpu_memory_stats", "bbgpu_fault_inject", "bbgpu_fault_stats", "bbgpu_srs_set_validate",
    "bbgpu_init_devices", "bbgpu_num_contexts", "bbgpu_memory_stats_context",
    "bbgpu_plonk_check_witness", "bbgpu_plonk_check_witness_batch", "bbgpu_plonk_set_witness_check", "bbgpu_plonk_last_witness_report",
    "bbgpu_host_plonk_check_witness",
    "bbgpu_plonk_prover_set_wire_map", "bbgpu_plonk_prover_set_witness_from", "bbgpu_plonk_construct_proof_batch_from",
    "bbgpu_plonk_check_witness_batch_from",
    "bbgpu_host_pairing", "bbgpu_host_pairing_check", "bbgpu_transcript_read_g2", "bbgpu_srs_check", "bbgpu_host_srs_check",
    "bbgpu_plonk_verifier_create", "bbgpu_plonk_verifier_destroy", "bbgpu_plonk_verify_batch", "bbgpu_host_plonk_verify_batch", "bbgpu_plonk_verify_last_timing",
    "bbgpu_plonk_verify_multi", "bbgpu_host_plonk_verify_multi",
    "bbgpu_srs_update", "bbgpu_host_srs_update", "bbgpu_host_srs_update_check", "bbgpu_transcript_write_g2", "bbgpu_selftest_endo_split",
    "bbgpu_srs_lagrange", "bbgpu_host_srs_lagrange",
    "bbgpu_fr_evaluate_lagrange_device", "bbgpu_kate_opening_lagrange_device", "bbgpu_host_fr_evaluate_lagrange", "bbgpu_host_kate_opening_lagrange",
    "bbgpu_srs_lagrange_check", "bbgpu_host_srs_lagrange_check",
    "bbgpu_lagrange_opening_begin", "bbgpu_lagrange_opening_evaluate", "bbgpu_lagrange_opening_open", "bbgpu_lagrange_opening_open_folded",
    "bbgpu_lagrange_opening_end", "bbgpu_fr_fold_device", "bbgpu_host_fr_fold", "bbgpu_host_kate_opening_lagrange_folded", "bbgpu_host_kzg_check_openings",
    "bbgpu_selftest_plonk_round",
    "bbgpu_kzg_open_all_setup", "bbgpu_kzg_open_all_release", "bbgpu_kzg_open_all_device", "bbgpu_host_kzg_open_all",
    "bbgpu_kzg_open_cosets_setup", "bbgpu_kzg_open_cosets_release", "bbgpu_kzg_open_cosets_device", "bbgpu_host_kzg_open_cosets",
    "bbgpu_kzg_open_cosets_setup_bounded", "bbgpu_host_kzg_open_cosets_bounded",
    "bbgpu_kzg_check_openings", "bbgpu_kzg_check_open_all", "bbgpu_host_kzg_check_openings_batch", "bbgpu_host_kzg_check_open_all",
    "bbgpu_kzg_check_last_timing", "bbgpu_kzg_check_cells", "bbgpu_kzg_check_open_cosets", "bbgpu_host_kzg_check_cells",
    "bbgpu_host_kzg_check_open_cosets", "bbgpu_host_kzg_cells_key_check", "bbgpu_kzg_check_cells_layout", "bbgpu_kzg_check_open_cosets_layout",
    "bbgpu_host_kzg_check_cells_layout", "bbgpu_host_kzg_check_open_cosets_layout", "bbgpu_kzg_recover_cells", "bbgpu_host_kzg_recover_cells",
    "bbgpu_kzg_recover_cells_each", "bbgpu_host_kzg_recover_cells_each",
    "bbgpu_g1_ntt", "bbgpu_host_g1_ntt", "bbgpu_g1_recover", "bbgpu_host_g1_recover", "bbgpu_g1_set_stage_mapping",
    "bbgpu_g1_recover_each", "bbgpu_host_g1_recover_each",
    "bbgpu_fr_ntt_columns_device", "bbgpu_host_fr_ntt_columns", "bbgpu_fr_recover_columns_device", "bbgpu_host_fr_recover_columns",
]
ERR_WITNESS = -6  # BBGPU_ERR_WITNESS: the opt-in witness check of the resident prover refused a witness


class MemoryInfo(C.Structure):
    """bbgpu_memory_info (include/bbgpu.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("srs_points_bytes", "srs_table_bytes", "srs_auto_bytes", "srs_cache_cap_bytes", "ntt_table_bytes", "ntt_table_cap_bytes",
                                          "ntt_table_sets", "msm_workspace_bytes", "staging_bytes", "pinned_host_bytes")]


class FaultInfo(C.Structure):
    """bbgpu_fault_info (include/bbgpu.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("alloc_calls", "h2d_calls", "d2h_calls", "launch_checks", "armed", "fired", "absorbed", "live_allocations",
                                          "live_bytes", "slots_pending")]


class WitnessReport(C.Structure):
    """bbgpu_plonk_witness_report (include/bbgpu.h)"""
    _fields_ = [("gate_failures", C.c_uint64), ("copy_failures", C.c_uint64)] + \
        [(k, C.c_uint32) for k in ("first_gate", "first_gate_kinds", "kinds", "first_copy", "first_copy_target", "_pad")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "_pad"}


class SrsReport(C.Structure):
    """bbgpu_srs_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # first_bad_point / first_bad_power when there is none
    _fields_ = [("n", C.c_uint64), ("bad_points", C.c_uint64), ("first_bad_point", C.c_uint64), ("first_is_generator", C.c_uint32), ("g2_ok", C.c_uint32),
                ("powers_checked", C.c_uint32), ("powers_ok", C.c_uint32), ("first_bad_power", C.c_uint64), ("seed", C.c_uint64 * 4), ("a", C.c_uint64 * 8),
                ("b", C.c_uint64 * 8)]
    g2_given = True  # set by the binding: was an x * G2 passed to the check?

    @property
    def ok(self):
        """the table is good: every row on the curve and, when x * G2 was given, a usable x * G2 and the powers test passed"""
        return self.bad_points == 0 and (not self.g2_given or (self.g2_ok == 1 and self.powers_ok == 1))

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, t in self._fields_ if t in (C.c_uint64, C.c_uint32)}
        d.update(seed=[int(v) for v in self.seed], a=[int(v) for v in self.a], b=[int(v) for v in self.b], ok=bool(self.ok))
        return d


class SrsUpdateReport(C.Structure):
    """bbgpu_srs_update_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # first_bad_point when there is none
    _fields_ = [("n", C.c_uint64), ("first_power", C.c_uint64), ("bad_points", C.c_uint64), ("first_bad_point", C.c_uint64), ("g2_ok", C.c_uint32),
                ("_pad", C.c_uint32), ("y_g2", C.c_uint64 * 16), ("g2_x_out", C.c_uint64 * 16)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, t in self._fields_ if t in (C.c_uint64, C.c_uint32) and k != "_pad"}
        d.update(y_g2=[int(v) for v in self.y_g2], g2_x_out=[int(v) for v in self.g2_x_out])
        return d


class SrsLagrangeReport(C.Structure):
    """bbgpu_srs_lagrange_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # first_bad_point / first_infinity_row when there is none
    _fields_ = [(k, C.c_uint64) for k in ("n", "bad_points", "first_bad_point", "infinity_rows", "first_infinity_row")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SrsLagrangeCheckReport(C.Structure):
    """bbgpu_srs_lagrange_check_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # first_bad_point / first_bad_row when there is none
    _fields_ = [("n", C.c_uint64), ("bad_points", C.c_uint64), ("first_bad_point", C.c_uint64), ("basis_checked", C.c_uint32), ("basis_ok", C.c_uint32),
                ("first_bad_row", C.c_uint64), ("seed", C.c_uint64 * 4), ("a", C.c_uint64 * 8), ("b", C.c_uint64 * 8)]

    @property
    def ok(self):
        """the table is the Lagrange form of the string: every row on the curve and the basis test passed"""
        return self.bad_points == 0 and self.basis_ok == 1

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, t in self._fields_ if t in (C.c_uint64, C.c_uint32)}
        d.update(seed=[int(v) for v in self.seed], a=[int(v) for v in self.a], b=[int(v) for v in self.b], ok=bool(self.ok))
        return d


class PlonkVerifyReport(C.Structure):
    """bbgpu_plonk_verify_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # first_bad_status / first_bad_proof when there is none
    BAD_POINT, ZERO_EVAL = 1, 2  # status bits
    _fields_ = [("count", C.c_uint64), ("bad_status", C.c_uint64), ("first_bad_status", C.c_uint64), ("pairing_checked", C.c_uint32),
                ("pairing_ok", C.c_uint32), ("first_bad_proof", C.c_uint64), ("seed", C.c_uint64 * 4), ("a", C.c_uint64 * 8), ("b", C.c_uint64 * 8)]
    status = None  # set by the binding: (count,) uint32, the per-proof bit masks

    @property
    def ok(self):
        """every proof of the batch is valid"""
        return self.bad_status == 0 and self.pairing_checked == 1 and self.pairing_ok == 1

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, t in self._fields_ if t in (C.c_uint64, C.c_uint32)}
        d.update(seed=[int(v) for v in self.seed], a=[int(v) for v in self.a], b=[int(v) for v in self.b], ok=bool(self.ok),
                 status=[int(v) for v in self.status] if self.status is not None else None)
        return d


class KzgCheckReport(C.Structure):
    """bbgpu_kzg_check_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # first_bad when there is none
    _fields_ = [("count", C.c_uint64), ("bad_points", C.c_uint64), ("first_bad", C.c_uint64), ("first_bad_is_proof", C.c_uint32), ("g2_ok", C.c_uint32),
                ("ok", C.c_uint32), ("rounds", C.c_uint32), ("first_failing", C.c_int64), ("seed", C.c_uint64 * 4), ("a", C.c_uint64 * 8), ("b", C.c_uint64 * 8)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, t in self._fields_ if t in (C.c_uint64, C.c_uint32, C.c_int64)}
        d.update(seed=[int(v) for v in self.seed], a=[int(v) for v in self.a], b=[int(v) for v in self.b])
        return d


class KzgRecoverReport(C.Structure):
    """bbgpu_kzg_recover_report (include/bbgpu.h)"""
    _fields_ = [("consistent", C.c_uint32), ("first_bad_poly", C.c_uint32), ("first_bad_coeff", C.c_uint64), ("missing", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class G1RecoverReport(C.Structure):
    """bbgpu_g1_recover_report (include/bbgpu.h)"""
    _fields_ = [("consistent", C.c_uint32), ("first_bad_column", C.c_uint32), ("first_bad_coeff", C.c_uint64), ("missing", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class KzgRecoverEachReport(C.Structure):
    """bbgpu_kzg_recover_each_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # an entry of first_bad when the polynomial has none
    _fields_ = [("consistent", C.c_uint32), ("first_bad_poly", C.c_uint32), ("first_bad_coeff", C.c_uint64), ("max_missing", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class G1RecoverEachReport(C.Structure):
    """bbgpu_g1_recover_each_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFFFFFFFFFF  # an entry of first_bad when the column has none
    _fields_ = [("consistent", C.c_uint32), ("first_bad_column", C.c_uint32), ("first_bad_coeff", C.c_uint64), ("max_missing", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class FrRecoverColumnsReport(C.Structure):
    """bbgpu_fr_recover_columns_report (include/bbgpu.h)"""
    NONE = 0xFFFFFFFF  # an entry of first_bad when the column has none
    _fields_ = [("consistent", C.c_uint32), ("first_bad_column", C.c_uint32), ("first_bad_coeff", C.c_uint64), ("max_missing", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PlonkVerifyKey(C.Structure):
    """bbgpu_plonk_verify_key (include/bbgpu.h)"""
    _fields_ = [("n", C.c_size_t), ("widgets", C.c_int), ("vk", C.c_void_p)]


class PlonkWitness(C.Structure):
    """bbgpu_plonk_witness (include/bbgpu.h)"""
    WIRES, VARIABLES = 0, 1  # form
    HOST, DEVICE = 0, 1      # where
    _fields_ = [("form", C.c_int), ("where", C.c_int), ("w_l", C.c_void_p), ("w_r", C.c_void_p), ("w_o", C.c_void_p), ("variables", C.c_void_p),
                ("hip_stream", C.c_void_p)]


class BbGpuError(RuntimeError):
    pass


def library_path():
    # BBGPU_LIB: alternative build of the same library (A/B timing of kernel variants); default = the in-tree build
    return os.environ.get("BBGPU_LIB") or os.path.join(HERE, "libbbgpu.so")


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of libbbgpu.so, in-tree (cross-compiles without a GPU)."""
    src = os.path.join(HERE, "csrc")
    if force:
        subprocess.run(["make", "-C", src, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", src, "-j4"], check=True, stdout=subprocess.DEVNULL)
    return library_path()


class MsmJob(C.Structure):
    """layout of scalar_multiplication::multiplication_state (scalar_multiplication.hpp:88-94)"""
    _fields_ = [("points", u64p), ("scalars", u64p), ("num_elements", C.c_size_t), ("_pad", C.c_uint64),
                ("output", C.c_uint64 * 12)]


def _ptr(a):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "need C-contiguous uint64"
    return a.ctypes.data_as(u64p)


class BbGpu:
    def __init__(self, device=0, init=True, devices=None):
        """devices: bind one device context per entry (bbgpu_init_devices; entries may repeat) -- the host-pointer MSMs of at least
        2^17 points are then split over them.  Otherwise one context on `device` (bbgpu_init)."""
        path = library_path()
        if not os.path.exists(path):
            raise BbGpuError("libbbgpu.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = self.lib = C.CDLL(path)
        L.bbgpu_last_error.restype = C.c_char_p
        L.bbgpu_version.restype = C.c_char_p
        L.bbgpu_ntt.argtypes = [u64p, C.c_size_t, C.c_int, u64p]
        L.bbgpu_ntt_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, u64p, C.c_void_p]
        L.bbgpu_ntt_device_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, u64p, C.c_void_p]
        L.bbgpu_srs_register.argtypes = [u64p, C.c_size_t]
        L.bbgpu_srs_generate.argtypes = [u64p, C.c_size_t, u64p]
        if hasattr(L, "bbgpu_srs_generate_range"):  # absent from older A/B builds loaded through BBGPU_LIB
            L.bbgpu_srs_generate_range.argtypes = [u64p, C.c_size_t, C.c_size_t, u64p]
        L.bbgpu_msm_g1.argtypes = [u64p, u64p, C.c_size_t, u64p]
        if hasattr(L, "bbgpu_fault_inject"):  # absent from older A/B builds loaded through BBGPU_LIB
            L.bbgpu_fault_inject.argtypes = [C.c_char_p]
        L.bbgpu_msm_g1_plain.argtypes = [u64p, u64p, C.c_size_t, u64p]
        L.bbgpu_msm_g1_batch.argtypes = [C.POINTER(MsmJob), C.c_size_t]
        L.bbgpu_msm_num_windows.argtypes = [C.c_size_t]
        L.bbgpu_srs_num_windows.argtypes = [C.c_int, C.c_size_t]
        L.bbgpu_msm_g1_device.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, u64p, C.c_void_p]
        L.bbgpu_msm_g1_device_async.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.bbgpu_msm_g1_device_rows_async.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bbgpu_srs_has_window_tables.argtypes = [C.c_int]
        L.bbgpu_msm_g1_wait.argtypes = [C.c_int, u64p]
        L.bbgpu_msm_g1_device_batch_async.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_void_p]
        L.bbgpu_msm_g1_batch_wait.argtypes = [C.c_int, u64p]
        L.bbgpu_g1_sum.argtypes = [u64p, C.c_size_t, u64p]
        L.bbgpu_last_timing.argtypes = [C.POINTER(C.c_float), C.c_int]
        vp, sz = C.c_void_p, C.c_size_t
        L.bbgpu_fr_evaluate_device.argtypes = [vp, sz, u64p, u64p, vp]
        L.bbgpu_fr_batch_invert_device.argtypes = [vp, sz, vp]
        L.bbgpu_fr_product_scan_device.argtypes = [vp, vp, sz, C.c_int, C.c_int, vp]
        L.bbgpu_fr_mul_device.argtypes = [vp, vp, vp, sz, vp]
        L.bbgpu_kate_opening_device.argtypes = [vp, vp, sz, u64p, u64p, vp]
        L.bbgpu_lagrange_l1_fft_device.argtypes = [vp, sz, sz, vp]
        L.bbgpu_divide_by_pseudo_vanishing_device.argtypes = [vp, sz, sz, vp]
        L.bbgpu_permutation_lagrange_base_device.argtypes = [vp, vp, sz, vp]
        if devices is not None:
            devices = [int(d) for d in devices]
            device = devices[0] if devices else device
        self.device = device
        if init and devices is not None:
            arr = (C.c_int * max(1, len(devices)))(*devices)
            self._chk(L.bbgpu_init_devices(arr, len(devices)))
        elif init:
            self._chk(L.bbgpu_init(device))

    def _chk(self, rc):
        if rc < 0:
            raise BbGpuError("bbgpu error %d: %s" % (rc, self.lib.bbgpu_last_error().decode()))
        return rc

    def version(self):
        return self.lib.bbgpu_version().decode()

    def device_count(self):
        return int(self.lib.bbgpu_device_count())

    def shutdown(self):
        self.lib.bbgpu_shutdown()

    # ---- polynomial_arithmetic ------------------------------------------------------------------------------------
    def ntt(self, coeffs, kind, constant=None):
        """in place on a (n, 4) uint64 host array"""
        kind = NTT_KINDS[kind] if isinstance(kind, str) else kind
        cp = _ptr(np.ascontiguousarray(constant, dtype=np.uint64)) if constant is not None else None
        self._chk(self.lib.bbgpu_ntt(_ptr(coeffs), coeffs.shape[0], kind, cp))
        return coeffs

    def fft(self, coeffs): return self.ntt(coeffs, "fft")
    def ifft(self, coeffs): return self.ntt(coeffs, "ifft")
    def coset_fft(self, coeffs): return self.ntt(coeffs, "coset_fft")
    def coset_ifft(self, coeffs): return self.ntt(coeffs, "coset_ifft")
    def fft_with_constant(self, coeffs, value): return self.ntt(coeffs, "fft_with_constant", value)
    def ifft_with_constant(self, coeffs, value): return self.ntt(coeffs, "ifft_with_constant", value)
    def coset_fft_with_constant(self, coeffs, constant): return self.ntt(coeffs, "coset_fft_with_constant", constant)

    def ntt_device(self, d_ptr, n, kind, constant=None, stream=None):
        kind = NTT_KINDS[kind] if isinstance(kind, str) else kind
        cp = _ptr(np.ascontiguousarray(constant, dtype=np.uint64)) if constant is not None else None
        self._chk(self.lib.bbgpu_ntt_device(C.c_void_p(d_ptr), n, kind, cp, C.c_void_p(stream or 0)))

    def ntt_device_batch(self, d_ptr, n, batch, kind, constant=None, stride=None, stream=None):
        """`batch` transforms of consecutive n-element vectors (stride elements apart) in one set of launches"""
        kind = NTT_KINDS[kind] if isinstance(kind, str) else kind
        cp = _ptr(np.ascontiguousarray(constant, dtype=np.uint64)) if constant is not None else None
        self._chk(self.lib.bbgpu_ntt_device_batch(C.c_void_p(d_ptr), n, stride or n, batch, kind, cp, C.c_void_p(stream or 0)))

    # ---- the O(n) helpers between transforms and commitments, on device-resident vectors (raw device pointers) -----
    def evaluate_device(self, d_coeffs, n, z, stream=None):
        """polynomial_arithmetic::evaluate (polynomial_arithmetic.cpp:337-373)"""
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.bbgpu_fr_evaluate_device(d_coeffs, n, _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(out), stream or 0))
        return out

    def batch_invert_device(self, d_values, n, stream=None):
        """fr::batch_invert (fields/field.hpp:503-522), in place"""
        self._chk(self.lib.bbgpu_fr_batch_invert_device(d_values, n, stream or 0))

    def product_scan_device(self, d_in, d_out, n, reverse=False, inclusive=False, stream=None):
        """running products (prover.cpp:194-202 is the exclusive prefix form)"""
        self._chk(self.lib.bbgpu_fr_product_scan_device(d_in, d_out, n, int(reverse), int(inclusive), stream or 0))

    def mul_device(self, d_out, d_a, d_b, n, stream=None):
        """polynomial_arithmetic::mul (:328-335)"""
        self._chk(self.lib.bbgpu_fr_mul_device(d_out, d_a, d_b, n, stream or 0))

    def compute_kate_opening_coefficients_device(self, d_src, d_dest, n, z, stream=None):
        """polynomial_arithmetic::compute_kate_opening_coefficients (:562-591); returns F(z)"""
        f = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.bbgpu_kate_opening_device(d_src, d_dest, n, _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(f), stream or 0))
        return f

    def evaluate_lagrange_device(self, d_values, n, z, batch=1, stride=None, stream=None):
        """bbgpu_fr_evaluate_lagrange_device: `batch` polynomials given by their values on the size-n domain (stride elements apart), at z -> (batch, 4)"""
        out = np.zeros((max(int(batch), 1), 4), dtype=np.uint64)
        self.lib.bbgpu_fr_evaluate_lagrange_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, C.c_void_p]
        self._chk(self.lib.bbgpu_fr_evaluate_lagrange_device(d_values, n, n if stride is None else stride, batch,
                                                             _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(out), stream or 0))
        return out

    def kate_opening_lagrange_device(self, d_values, d_quotient, n, z, batch=1, stride=None, want_f=True, stream=None):
        """bbgpu_kate_opening_lagrange_device: the values of (f_b(X) - f_b(z)) / (X - z) on the domain into d_quotient (may be d_values itself); returns
        f_b(z) as (batch, 4), or None with want_f=False (then only the batch inversion synchronises)"""
        f = np.zeros((max(int(batch), 1), 4), dtype=np.uint64) if want_f else None
        self.lib.bbgpu_kate_opening_lagrange_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, C.c_void_p]
        self._chk(self.lib.bbgpu_kate_opening_lagrange_device(d_values, d_quotient, n, n if stride is None else stride, batch,
                                                              _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(f) if want_f else None, stream or 0))
        return f

    # ---- opening sessions: several points over one shared inversion, folded openings (bbgpu_lagrange_opening_*) ----
    def lagrange_opening_begin(self, n, z, points=None, stream=None):
        """bbgpu_lagrange_opening_begin: z (points, 4) -> session handle; the inverses of all points by one launch and one batch inversion"""
        z = None if z is None else np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        points = (z.shape[0] if z is not None else 1) if points is None else points
        self.lib.bbgpu_lagrange_opening_begin.argtypes = [C.c_size_t, u64p, C.c_int, C.c_void_p]
        return self._chk(self.lib.bbgpu_lagrange_opening_begin(n, _ptr(z) if z is not None else None, points, stream or 0))

    def lagrange_opening_evaluate(self, session, point, d_values, n, batch=1, stride=None, stream=None):
        """bbgpu_lagrange_opening_evaluate -> (batch, 4): what evaluate_lagrange_device returns at the session's z_point (n: the session's, for the default stride)"""
        out = np.zeros((max(int(batch), 1), 4), dtype=np.uint64)
        self.lib.bbgpu_lagrange_opening_evaluate.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, u64p, C.c_void_p]
        self._chk(self.lib.bbgpu_lagrange_opening_evaluate(session, point, d_values, n if stride is None else stride, batch, _ptr(out), stream or 0))
        return out

    def lagrange_opening_open(self, session, point, d_values, d_quotient, n, batch=1, stride=None, want_f=True, stream=None):
        """bbgpu_lagrange_opening_open: what kate_opening_lagrange_device writes and returns at the session's z_point; None with want_f=False"""
        f = np.zeros((max(int(batch), 1), 4), dtype=np.uint64) if want_f else None
        self.lib.bbgpu_lagrange_opening_open.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, u64p, C.c_void_p]
        self._chk(self.lib.bbgpu_lagrange_opening_open(session, point, d_values, d_quotient, n if stride is None else stride, batch,
                                                       _ptr(f) if want_f else None, stream or 0))
        return f

    def lagrange_opening_open_folded(self, session, point, d_values, n, gamma, d_quotient, batch=None, stride=None, accumulate=False, want_f=True, stream=None):
        """bbgpu_lagrange_opening_open_folded: d_quotient (n elements) = or += the opening of sum_b gamma_b f_b at the session's z_point; returns F(z) as
        (4,), or None with want_f=False.  gamma (batch, 4); batch defaults to its rows"""
        g = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.uint64).reshape(-1, 4)
        batch = g.shape[0] if batch is None else batch
        f = np.zeros(4, dtype=np.uint64) if want_f else None
        self.lib.bbgpu_lagrange_opening_open_folded.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, u64p, C.c_void_p, C.c_int, u64p, C.c_void_p]
        self._chk(self.lib.bbgpu_lagrange_opening_open_folded(session, point, d_values, n if stride is None else stride, batch, _ptr(g) if g is not None else None,
                                                              d_quotient, int(bool(accumulate)), _ptr(f) if want_f else None, stream or 0))
        return f

    def lagrange_opening_end(self, session):
        self.lib.bbgpu_lagrange_opening_end.argtypes = [C.c_int]
        self._chk(self.lib.bbgpu_lagrange_opening_end(session))

    def fold_device(self, d_out, d_values, n, gamma, batch=None, stride=None, accumulate=False, stream=None):
        """bbgpu_fr_fold_device: d_out[i] = or += sum_b gamma_b v_{b,i}; any n in [1, 2^24]"""
        g = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.uint64).reshape(-1, 4)
        batch = g.shape[0] if batch is None else batch
        self.lib.bbgpu_fr_fold_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, u64p, C.c_int, C.c_void_p]
        self._chk(self.lib.bbgpu_fr_fold_device(d_out, d_values, n, n if stride is None else stride, batch, _ptr(g) if g is not None else None,
                                                int(bool(accumulate)), stream or 0))

    def compute_lagrange_polynomial_fft_device(self, d_l_1, n_src, n_target, stream=None):
        """polynomial_arithmetic::compute_lagrange_polynomial_fft (:381-476)"""
        self._chk(self.lib.bbgpu_lagrange_l1_fft_device(d_l_1, n_src, n_target, stream or 0))

    def divide_by_pseudo_vanishing_polynomial_device(self, d_coeffs, n_src, n_target, stream=None):
        """polynomial_arithmetic::divide_by_pseudo_vanishing_polynomial (:478-560), in place"""
        self._chk(self.lib.bbgpu_divide_by_pseudo_vanishing_device(d_coeffs, n_src, n_target, stream or 0))

    def compute_permutation_lagrange_base_single_device(self, d_out, d_mapping, n, stream=None):
        """waffle::compute_permutation_lagrange_base_single (permutation.hpp:15-87)"""
        self._chk(self.lib.bbgpu_permutation_lagrange_base_device(d_out, d_mapping, n, stream or 0))

    # ---- scalar_multiplication ------------------------------------------------------------------------------------
    def srs_register(self, points_endo_table):
        return self._chk(self.lib.bbgpu_srs_register(_ptr(points_endo_table), points_endo_table.shape[0] // 2))

    def srs_generate(self, x_mont, n, want_host_table=False, first=0):
        """resident points x^(first + i) G, i < n (first > 0: the slice of a rank of a point-range split)"""
        table = np.zeros((2 * n, 8), dtype=np.uint64) if want_host_table else None
        xa = np.ascontiguousarray(x_mont, dtype=np.uint64)
        xp, tp = _ptr(xa), (_ptr(table) if want_host_table else None)
        h = self._chk(self.lib.bbgpu_srs_generate_range(xp, first, n, tp) if first else self.lib.bbgpu_srs_generate(xp, n, tp))
        return (h, table) if want_host_table else h

    def read_transcript(self, path, degree):
        """io::read_transcript (io.hpp:159-181), G1 part -> the (2 * degree, 8) endo table the reference's ReferenceString holds"""
        self.lib.bbgpu_transcript_read_g1.argtypes = [C.c_char_p, C.c_size_t, u64p]
        table = np.zeros((2 * degree, 8), dtype=np.uint64)
        self._chk(self.lib.bbgpu_transcript_read_g1(path.encode(), degree, _ptr(table)))
        return table

    def write_transcript(self, path, points_endo_table, degree, x_mont):
        """the file io::read_transcript accepts for this SRS: degree - 1 G1 points + {G2, x G2} (io.hpp:36-182)"""
        self.lib.bbgpu_transcript_write.argtypes = [C.c_char_p, u64p, C.c_size_t, u64p]
        self._chk(self.lib.bbgpu_transcript_write(path.encode(), _ptr(points_endo_table), degree, _ptr(np.ascontiguousarray(x_mont, dtype=np.uint64))))

    def transcript_read_g2(self, path):
        """the other half of io::read_transcript: the file's second G2 point, x * G2 (io.hpp:100-135,171-180) as (16,) uint64, Montgomery"""
        self.lib.bbgpu_transcript_read_g2.argtypes = [C.c_char_p, u64p]
        out = np.zeros(16, dtype=np.uint64)
        self._chk(self.lib.bbgpu_transcript_read_g2(path.encode(), _ptr(out)))
        return out

    # ---- is this table an SRS?  (bbgpu_srs_check and its host twin; the pairing is host code, no GPU needed) -----------------------
    def host_pairing(self, p, q):
        """pairing::reduced_ate_pairing(P, Q): p (8,) affine G1, q (16,) affine G2 -> (12, 4) fq in the reference's fq12 order"""
        p, q = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1)[:8].copy(), np.ascontiguousarray(q, dtype=np.uint64).reshape(16)
        out = np.zeros((12, 4), dtype=np.uint64)
        self.lib.bbgpu_host_pairing.argtypes = [u64p, u64p, u64p]
        self._chk(self.lib.bbgpu_host_pairing(_ptr(p), _ptr(q), _ptr(out)))
        return out

    def host_pairing_check(self, ps, qs):
        """prod_k e(ps[k], qs[k]) == 1, one shared final exponentiation; ps (k, 8), qs (k, 16)"""
        ps = np.ascontiguousarray(ps, dtype=np.uint64).reshape(-1, 8)
        qs = np.ascontiguousarray(qs, dtype=np.uint64).reshape(-1, 16)
        assert ps.shape[0] == qs.shape[0]
        one = C.c_int(0)
        self.lib.bbgpu_host_pairing_check.argtypes = [u64p, u64p, C.c_size_t, C.POINTER(C.c_int)]
        self._chk(self.lib.bbgpu_host_pairing_check(_ptr(ps), _ptr(qs), ps.shape[0], C.byref(one)))
        return one.value == 1

    @staticmethod
    def _srs_check_args(g2_x, seed, locate):
        g2 = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16) if g2_x is not None else None
        sd = np.ascontiguousarray(seed, dtype=np.uint64).reshape(4) if seed is not None else None
        return g2, sd, (_ptr(g2) if g2 is not None else None), (_ptr(sd) if sd is not None else None), (1 if locate else 0)

    def srs_check(self, handle, n, g2_x=None, seed=None, locate=False):
        """bbgpu_srs_check: rows [0, n) of a resident table on the curve, and -- with g2_x = x * G2 -- P_{i+1} = x P_i for every i by two MSMs and one
        pairing check.  seed None: drawn from the operating system (the table's maker must not know it).  Returns an SrsReport (.ok, .as_dict())."""
        g2, sd, g2p, sdp, flags = self._srs_check_args(g2_x, seed, locate)
        rep = SrsReport()
        self.lib.bbgpu_srs_check.argtypes = [C.c_int, C.c_size_t, u64p, u64p, C.c_int, C.POINTER(SrsReport)]
        self._chk(self.lib.bbgpu_srs_check(int(handle), int(n), g2p, sdp, flags, C.byref(rep)))
        rep.g2_given = g2 is not None
        return rep

    def host_srs_check(self, table, n=None, g2_x=None, seed=None, locate=False):
        """bbgpu_host_srs_check: the same check over the even entries of a (2n, 8) endo table, on the host; no GPU needed"""
        n = table.shape[0] // 2 if n is None else n
        g2, sd, g2p, sdp, flags = self._srs_check_args(g2_x, seed, locate)
        rep = SrsReport()
        self.lib.bbgpu_host_srs_check.argtypes = [u64p, C.c_size_t, u64p, u64p, C.c_int, C.POINTER(SrsReport)]
        self._chk(self.lib.bbgpu_host_srs_check(_ptr(table), int(n), g2p, sdp, flags, C.byref(rep)))
        rep.g2_given = g2 is not None
        return rep

    # ---- make this SRS your own  (bbgpu_srs_update, its host twin, the proof of an update, the writer for a string nobody holds the secret of) ----
    def _srs_update_error(self, rc, rep):
        err = BbGpuError("bbgpu error %d: %s" % (rc, self.lib.bbgpu_last_error().decode()))
        err.report = rep  # filled when rows off the curve were the reason
        return err

    def srs_update(self, handle, n, y_mont, g2_x=None, want_host_table=False, first=0):
        """bbgpu_srs_update: rows [0, n) of a resident table times y^(first + i) -> (new handle, its (2n, 8) host table or None, SrsUpdateReport).
        A row off the curve raises BbGpuError with the report in .report; no table is made."""
        table = np.zeros((2 * n, 8), dtype=np.uint64) if want_host_table else None
        ya = np.ascontiguousarray(y_mont, dtype=np.uint64).reshape(4) if y_mont is not None else None
        g2 = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16) if g2_x is not None else None
        rep = SrsUpdateReport()
        self.lib.bbgpu_srs_update.argtypes = [C.c_int, C.c_size_t, C.c_size_t, u64p, u64p, u64p, C.POINTER(SrsUpdateReport)]
        h = self.lib.bbgpu_srs_update(int(handle), int(n), int(first), _ptr(ya) if ya is not None else None, _ptr(g2) if g2 is not None else None,
                                      _ptr(table) if want_host_table else None, C.byref(rep))
        if h < 0:
            raise self._srs_update_error(h, rep)
        return h, table, rep

    def host_srs_update(self, table, n, y_mont, g2_x=None, first=0, out=None):
        """bbgpu_host_srs_update: the same over the even entries of a (2n, 8) endo table, on the host -> (table, SrsUpdateReport); out: the array to write
        (may be `table` itself), default a new one"""
        out = np.zeros((2 * n, 8), dtype=np.uint64) if out is None else out
        ya = np.ascontiguousarray(y_mont, dtype=np.uint64).reshape(4) if y_mont is not None else None
        g2 = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16) if g2_x is not None else None
        rep = SrsUpdateReport()
        self.lib.bbgpu_host_srs_update.argtypes = [u64p, C.c_size_t, C.c_size_t, u64p, u64p, u64p, C.POINTER(SrsUpdateReport)]
        rc = self.lib.bbgpu_host_srs_update(_ptr(table), int(n), int(first), _ptr(ya) if ya is not None else None, _ptr(g2) if g2 is not None else None,
                                            _ptr(out), C.byref(rep))
        if rc < 0:
            raise self._srs_update_error(rc, rep)
        return out, rep

    def host_srs_update_check(self, old_p1, new_p1, y_g2):
        """bbgpu_host_srs_update_check: is new_p1 = y old_p1 for the y behind y_g2 = y G2 (row 1 of the old and of the new table)?"""
        a = np.ascontiguousarray(old_p1, dtype=np.uint64).reshape(-1)[:8].copy()
        b = np.ascontiguousarray(new_p1, dtype=np.uint64).reshape(-1)[:8].copy()
        q = np.ascontiguousarray(y_g2, dtype=np.uint64).reshape(16)
        ok = C.c_int(0)
        self.lib.bbgpu_host_srs_update_check.argtypes = [u64p, u64p, u64p, C.POINTER(C.c_int)]
        self._chk(self.lib.bbgpu_host_srs_update_check(_ptr(a), _ptr(b), _ptr(q), C.byref(ok)))
        return ok.value == 1

    def write_transcript_g2(self, path, table, degree, g2_x):
        """bbgpu_transcript_write_g2: write_transcript for a string whose secret nobody holds; g2_x = x G2 (16,)"""
        self.lib.bbgpu_transcript_write_g2.argtypes = [C.c_char_p, u64p, C.c_size_t, u64p]
        self._chk(self.lib.bbgpu_transcript_write_g2(path.encode(), _ptr(table), degree, _ptr(np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16))))

    # ---- the same string in the Lagrange basis  (bbgpu_srs_lagrange and its host twin) ----
    def srs_lagrange(self, handle, n, want_host_table=False):
        """bbgpu_srs_lagrange: rows [0, n) of a resident table -> (new handle of L_i = n^-1 sum_j omega^(-ij) P_j, its (2n, 8) host table or None,
        SrsLagrangeReport).  A row off the curve or an output row at infinity raises BbGpuError with the report in .report; no table is made."""
        table = np.zeros((2 * n, 8), dtype=np.uint64) if want_host_table else None
        rep = SrsLagrangeReport()
        self.lib.bbgpu_srs_lagrange.argtypes = [C.c_int, C.c_size_t, u64p, C.POINTER(SrsLagrangeReport)]
        h = self.lib.bbgpu_srs_lagrange(int(handle), int(n), _ptr(table) if want_host_table else None, C.byref(rep))
        if h < 0:
            raise self._srs_update_error(h, rep)
        return h, table, rep

    def host_srs_lagrange(self, table, n, out=None):
        """bbgpu_host_srs_lagrange: the same over the even entries of a (2n, 8) endo table, on the host -> (table, SrsLagrangeReport); out: the array to
        write (may be `table` itself), default a new one"""
        out = np.zeros((2 * n, 8), dtype=np.uint64) if out is None else out
        rep = SrsLagrangeReport()
        self.lib.bbgpu_host_srs_lagrange.argtypes = [u64p, C.c_size_t, u64p, C.POINTER(SrsLagrangeReport)]
        rc = self.lib.bbgpu_host_srs_lagrange(_ptr(table), int(n), _ptr(out), C.byref(rep))
        if rc < 0:
            raise self._srs_update_error(rc, rep)
        return out, rep

    # ---- a polynomial opened at every point of its domain  (bbgpu_kzg_open_all_* and the host twin) ----
    def kzg_open_all_setup(self, handle, n):
        """bbgpu_kzg_open_all_setup: DFT_2n of the reversed rows [0, n - 1) of a resident monomial table, kept on the device -> setup handle"""
        self.lib.bbgpu_kzg_open_all_setup.argtypes = [C.c_int, C.c_size_t]
        return self._chk(self.lib.bbgpu_kzg_open_all_setup(int(handle), int(n)))

    def kzg_open_all_release(self, setup):
        self.lib.bbgpu_kzg_open_all_release.argtypes = [C.c_int]
        self._chk(self.lib.bbgpu_kzg_open_all_release(int(setup)))

    def kzg_open_all_device(self, setup, d_coeffs, n, batch=1, stride=None, stream=None, out=None):
        """bbgpu_kzg_open_all_device: `batch` polynomials in coefficient form on the device (stride elements apart) -> (batch, n, 8): the affine KZG proof
        of polynomial b at omega^i, infinity flagged in bit 63 of y[3]"""
        out = np.zeros((max(int(batch), 1), int(n), 8), dtype=np.uint64) if out is None else out
        self.lib.bbgpu_kzg_open_all_device.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, u64p, C.c_void_p]
        self._chk(self.lib.bbgpu_kzg_open_all_device(int(setup), d_coeffs, n if stride is None else stride, batch, _ptr(out), stream or 0))
        return out

    def host_kzg_open_all(self, table, n, coeffs, batch=1, stride=None):
        """bbgpu_host_kzg_open_all: the same on the host, over the even entries of a (>= 2 (n - 1), 8) endo table; coeffs (batch * stride, 4) -> (batch, n, 8)"""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        stride = coeffs.shape[0] // max(int(batch), 1) if stride is None else stride
        out = np.zeros((max(int(batch), 1), int(n), 8), dtype=np.uint64)
        self.lib.bbgpu_host_kzg_open_all.argtypes = [u64p, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p]
        self._chk(self.lib.bbgpu_host_kzg_open_all(_ptr(table), int(n), _ptr(coeffs), stride, batch, _ptr(out)))
        return out

    # ---- a polynomial opened on every coset of its domain  (bbgpu_kzg_open_cosets_* and the host twin) ----
    def kzg_open_cosets_setup(self, handle, n, coset, degree_bound=None):
        """bbgpu_kzg_open_cosets_setup: per residue e < coset, DFT_(2n/coset) of the reversed rows e, e + coset, .. of a resident monomial table (rows
        [0, n - coset) are read), kept on the device -> setup handle.  With degree_bound = d (bbgpu_kzg_open_cosets_setup_bounded): for polynomials of
        degree < d, transforms of length 2d/coset over rows [0, d - coset) -- a table of d rows is enough"""
        if degree_bound is None:
            self.lib.bbgpu_kzg_open_cosets_setup.argtypes = [C.c_int, C.c_size_t, C.c_size_t]
            return self._chk(self.lib.bbgpu_kzg_open_cosets_setup(int(handle), int(n), int(coset)))
        self.lib.bbgpu_kzg_open_cosets_setup_bounded.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t]
        return self._chk(self.lib.bbgpu_kzg_open_cosets_setup_bounded(int(handle), int(n), int(coset), int(degree_bound)))

    def kzg_open_cosets_release(self, setup):
        self.lib.bbgpu_kzg_open_cosets_release.argtypes = [C.c_int]
        self._chk(self.lib.bbgpu_kzg_open_cosets_release(int(setup)))

    def kzg_open_cosets_device(self, setup, d_coeffs, n, coset, batch=1, stride=None, stream=None, out=None):
        """bbgpu_kzg_open_cosets_device: `batch` polynomials in coefficient form on the device (stride elements apart) -> (batch, n / coset, 8): the affine
        KZG proof of polynomial b on coset k = { omega^(k + (n / coset) j) }, infinity flagged in bit 63 of y[3].  The stride is judged by the library alone:
        over a setup with a degree bound d it may be as small as d (coefficients from d on are not read), so pass it -- the default is n"""
        out = np.zeros((max(int(batch), 1), max(int(n) // max(int(coset), 1), 1), 8), dtype=np.uint64) if out is None else out
        self.lib.bbgpu_kzg_open_cosets_device.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, u64p, C.c_void_p]
        self._chk(self.lib.bbgpu_kzg_open_cosets_device(int(setup), d_coeffs, n if stride is None else stride, batch, _ptr(out), stream or 0))
        return out

    def host_kzg_open_cosets(self, table, n, coset, coeffs, batch=1, stride=None, degree_bound=None):
        """bbgpu_host_kzg_open_cosets: the same on the host, over the even entries of a (>= 2 (n - coset), 8) endo table; coeffs (batch * stride, 4) ->
        (batch, n / coset, 8).  With degree_bound = d (bbgpu_host_kzg_open_cosets_bounded): rows [0, d - coset) and coefficients [0, d) are read"""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        stride = coeffs.shape[0] // max(int(batch), 1) if stride is None else stride
        out = np.zeros((max(int(batch), 1), max(int(n) // max(int(coset), 1), 1), 8), dtype=np.uint64)
        if degree_bound is not None:
            self.lib.bbgpu_host_kzg_open_cosets_bounded.argtypes = [u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p]
            self._chk(self.lib.bbgpu_host_kzg_open_cosets_bounded(_ptr(table), int(n), int(coset), int(degree_bound), _ptr(coeffs), stride, batch, _ptr(out)))
            return out
        self.lib.bbgpu_host_kzg_open_cosets.argtypes = [u64p, C.c_size_t, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p]
        self._chk(self.lib.bbgpu_host_kzg_open_cosets(_ptr(table), int(n), int(coset), _ptr(coeffs), stride, batch, _ptr(out)))
        return out

    # ---- polynomials recovered from a subset of their cells  (bbgpu_kzg_recover_cells and the host twin) ----
    RECOVER_TILE = 256  # KZG_RECOVER_TILE (csrc/bbgpu_internal.h): roots of missing cells per LDS tile of k_recover_vanish

    @staticmethod
    def _kzg_recover_args(cell, values, coset, batch):
        cell = np.ascontiguousarray(cell, dtype=np.uint32).reshape(-1)
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        if values.shape[0] < max(int(batch), 1) * cell.shape[0] * max(int(coset), 1):  # the library would read past the end
            raise ValueError("kzg_recover_cells: %d values for batch %d of %d cells of %d" % (values.shape[0], batch, cell.shape[0], coset))
        return cell, values, cell.ctypes.data_as(C.POINTER(C.c_uint32))

    def kzg_recover_cells(self, cell, values, n, coset, degree_bound, d_coeffs_out, batch=1, stride=None, want_values=True, stream=None, out=None):
        """bbgpu_kzg_recover_cells: `batch` polynomials of degree < degree_bound from the same listed cells (cell: distinct indices below n / coset, any
        order; values (batch, count, coset, 4): polynomial b, listed cell t, point j, on the host) -> coefficients [0, n) of polynomial b at element b *
        stride of the device buffer d_coeffs_out, what kzg_open_cosets_device takes.  Returns ((batch, n, 4) the size-n transforms -- `out` when given --,
        or None without want_values; the report as a dict)."""
        cell, values, cp = self._kzg_recover_args(cell, values, coset, batch)
        if want_values and out is None:
            out = np.zeros((max(int(batch), 1), max(int(n), 1), 4), dtype=np.uint64)
        out = out if want_values else None
        rep = KzgRecoverReport()
        self.lib.bbgpu_kzg_recover_cells.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                                     C.c_size_t, u64p, C.POINTER(KzgRecoverReport), C.c_void_p]
        self._chk(self.lib.bbgpu_kzg_recover_cells(cp, cell.shape[0], _ptr(values), int(n), int(coset), int(degree_bound), int(batch), d_coeffs_out,
                                                   int(n) if stride is None else int(stride), _ptr(out) if want_values else None, C.byref(rep), stream or 0))
        return out, rep.as_dict()

    def host_kzg_recover_cells(self, cell, values, n, coset, degree_bound, batch=1, stride=None, want_values=True, out=None):
        """bbgpu_host_kzg_recover_cells: the same on the host -> ((batch * stride, 4) coefficients -- `out` when given, whose elements [n, stride) of every
        polynomial stay as they are --, the transforms or None, the report as a dict)"""
        cell, values, cp = self._kzg_recover_args(cell, values, coset, batch)
        stride = int(n) if stride is None else int(stride)
        coeffs = np.zeros((max(int(batch), 1) * max(stride, 1), 4), dtype=np.uint64) if out is None else out
        vals = np.zeros((max(int(batch), 1), max(int(n), 1), 4), dtype=np.uint64) if want_values else None
        rep = KzgRecoverReport()
        self.lib.bbgpu_host_kzg_recover_cells.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, u64p,
                                                          C.c_size_t, u64p, C.POINTER(KzgRecoverReport)]
        self._chk(self.lib.bbgpu_host_kzg_recover_cells(cp, cell.shape[0], _ptr(values), int(n), int(coset), int(degree_bound), int(batch), _ptr(coeffs), stride,
                                                        _ptr(vals) if want_values else None, C.byref(rep)))
        return coeffs, vals, rep.as_dict()

    # ---- the same for polynomials whose cell sets differ  (bbgpu_kzg_recover_cells_each and the host twin) ----
    RECOVER_EACH_LEAF = 64  # KZG_RECOVER_EACH_LEAF (csrc/bbgpu_internal.h): roots per leaf of the product tree

    @staticmethod
    def _kzg_recover_each_args(cells, values, coset):
        lists = [np.ascontiguousarray(c, dtype=np.uint32).reshape(-1) for c in cells]
        offsets = np.zeros(len(lists) + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum([c.shape[0] for c in lists])
        cell = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, dtype=np.uint32)]))  # never empty
        if isinstance(values, np.ndarray):  # one array for the whole call, already in the order of the lists: handed over as it is
            flat = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
            if flat.shape[0] < int(offsets[-1]) * max(int(coset), 1):
                raise ValueError("kzg_recover_cells_each: %d values for %d cells of %d" % (flat.shape[0], int(offsets[-1]), coset))
            return offsets, cell, flat, len(lists)
        vals = [np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4) for v in values]
        if len(lists) != len(vals):
            raise ValueError("kzg_recover_cells_each: %d cell lists, %d value arrays" % (len(lists), len(vals)))
        for b, (c, v) in enumerate(zip(lists, vals)):
            if v.shape[0] < c.shape[0] * max(int(coset), 1):  # the library would read past the end
                raise ValueError("kzg_recover_cells_each: polynomial %d: %d values for %d cells of %d" % (b, v.shape[0], c.shape[0], coset))
        flat = np.ascontiguousarray(np.concatenate([v[:c.shape[0] * max(int(coset), 1)] for c, v in zip(lists, vals)] + [np.zeros((1, 4), dtype=np.uint64)]))
        return offsets, cell, flat, len(lists)

    def kzg_recover_cells_each(self, cells, values, n, coset, degree_bound, d_coeffs_out, stride=None, want_values=True, stream=None, out=None):
        """bbgpu_kzg_recover_cells_each: len(cells) polynomials of degree < degree_bound, polynomial b from ITS OWN listed cells (cells[b]: distinct indices
        below n / coset, any order; values[b] (count_b, coset, 4): listed cell t, point j, on the host -- or ONE array that holds them all in that order, which is not copied) -> coefficients [0, n) of polynomial b at element b
        * stride of the device buffer d_coeffs_out.  Returns ((batch, n, 4) the size-n transforms -- `out` when given --, or None without want_values; the
        report as a dict; (batch,) uint64 first_bad, KzgRecoverEachReport.NONE where a polynomial has none)."""
        offsets, cell, flat, batch = self._kzg_recover_each_args(cells, values, coset)
        if want_values and out is None:
            out = np.zeros((max(batch, 1), max(int(n), 1), 4), dtype=np.uint64)
        out = out if want_values else None
        rep, first_bad = KzgRecoverEachReport(), np.zeros(max(batch, 1), dtype=np.uint64)
        u32p = C.POINTER(C.c_uint32)
        self.lib.bbgpu_kzg_recover_cells_each.argtypes = [u32p, u32p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, u64p, u64p,
                                                          C.POINTER(KzgRecoverEachReport), C.c_void_p]
        self._chk(self.lib.bbgpu_kzg_recover_cells_each(offsets.ctypes.data_as(u32p), cell.ctypes.data_as(u32p), _ptr(flat), int(n), int(coset), int(degree_bound),
                                                        batch, d_coeffs_out, int(n) if stride is None else int(stride), _ptr(out) if want_values else None,
                                                        _ptr(first_bad), C.byref(rep), stream or 0))
        return out, rep.as_dict(), first_bad

    def host_kzg_recover_cells_each(self, cells, values, n, coset, degree_bound, stride=None, want_values=True, out=None):
        """bbgpu_host_kzg_recover_cells_each: the same on the host -> ((batch * stride, 4) coefficients -- `out` when given, whose elements [n, stride) of
        every polynomial stay as they are --, the transforms or None, the report as a dict, first_bad)"""
        offsets, cell, flat, batch = self._kzg_recover_each_args(cells, values, coset)
        stride = int(n) if stride is None else int(stride)
        coeffs = np.zeros((max(batch, 1) * max(stride, 1), 4), dtype=np.uint64) if out is None else out
        vals = np.zeros((max(batch, 1), max(int(n), 1), 4), dtype=np.uint64) if want_values else None
        rep, first_bad = KzgRecoverEachReport(), np.zeros(max(batch, 1), dtype=np.uint64)
        u32p = C.POINTER(C.c_uint32)
        self.lib.bbgpu_host_kzg_recover_cells_each.argtypes = [u32p, u32p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, u64p, C.c_size_t, u64p, u64p,
                                                               C.POINTER(KzgRecoverEachReport)]
        self._chk(self.lib.bbgpu_host_kzg_recover_cells_each(offsets.ctypes.data_as(u32p), cell.ctypes.data_as(u32p), _ptr(flat), int(n), int(coset),
                                                             int(degree_bound), batch, _ptr(coeffs), stride, _ptr(vals) if want_values else None, _ptr(first_bad),
                                                             C.byref(rep)))
        return coeffs, vals, rep.as_dict(), first_bad

    # ---- columns of curve points: transforms and erasure decoding  (bbgpu_g1_ntt, bbgpu_g1_recover and the host twins) ----
    @staticmethod
    def _g1_ntt_args(points, n, batch, out):
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        if points.shape[0] < max(int(batch), 1) * max(int(n), 1):  # the library would read past the end
            raise ValueError("g1_ntt: %d points for batch %d of %d" % (points.shape[0], batch, n))
        if out is None:
            out = np.zeros((max(int(batch), 1), max(int(n), 1), 8), dtype=np.uint64)
        return points, out

    def g1_ntt(self, points, n, kind="fft", batch=1, stream=None, out=None):
        """bbgpu_g1_ntt: `batch` columns of n affine points (points (batch, n, 8) on the host, the reference's memory format, infinity as its flag) ->
        (batch, n, 8) their transforms, "fft" or "ifft" -- `out` when given, which may be `points` itself"""
        points, out = self._g1_ntt_args(points, n, batch, out)
        self.lib.bbgpu_g1_ntt.argtypes = [u64p, u64p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        self._chk(self.lib.bbgpu_g1_ntt(_ptr(points), _ptr(out), int(n), int(batch), NTT_KINDS[kind] if isinstance(kind, str) else int(kind), stream or 0))
        return out

    def host_g1_ntt(self, points, n, kind="fft", batch=1, out=None):
        """bbgpu_host_g1_ntt: the same on the host"""
        points, out = self._g1_ntt_args(points, n, batch, out)
        self.lib.bbgpu_host_g1_ntt.argtypes = [u64p, u64p, C.c_size_t, C.c_int, C.c_int]
        self._chk(self.lib.bbgpu_host_g1_ntt(_ptr(points), _ptr(out), int(n), int(batch), NTT_KINDS[kind] if isinstance(kind, str) else int(kind)))
        return out

    @staticmethod
    def _g1_recover_args(row, points, n, batch, out):
        row = np.ascontiguousarray(row, dtype=np.uint32).reshape(-1)
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        if points.shape[0] < max(int(batch), 1) * row.shape[0]:  # the library would read past the end
            raise ValueError("g1_recover: %d points for batch %d of %d rows" % (points.shape[0], batch, row.shape[0]))
        if out is None:
            out = np.zeros((max(int(batch), 1), max(int(n), 1), 8), dtype=np.uint64)
        return row, points, out, row.ctypes.data_as(C.POINTER(C.c_uint32))

    def g1_recover(self, row, points, n, degree_bound, batch=1, stream=None, out=None):
        """bbgpu_g1_recover: `batch` columns of n points, each a codeword of degree < degree_bound, from the same listed rows (row: distinct indices below n,
        any order; points (batch, count, 8): column b, listed row t, on the host) -> ((batch, n, 8) all n points of every column -- `out` when given --,
        the report as a dict)"""
        row, points, out, rp = self._g1_recover_args(row, points, n, batch, out)
        rep = G1RecoverReport()
        self.lib.bbgpu_g1_recover.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, C.POINTER(G1RecoverReport),
                                              C.c_void_p]
        self._chk(self.lib.bbgpu_g1_recover(rp, row.shape[0], _ptr(points), int(n), int(degree_bound), int(batch), _ptr(out), C.byref(rep), stream or 0))
        return out, rep.as_dict()

    def host_g1_recover(self, row, points, n, degree_bound, batch=1, out=None):
        """bbgpu_host_g1_recover: the same on the host"""
        row, points, out, rp = self._g1_recover_args(row, points, n, batch, out)
        rep = G1RecoverReport()
        self.lib.bbgpu_host_g1_recover.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, C.POINTER(G1RecoverReport)]
        self._chk(self.lib.bbgpu_host_g1_recover(rp, row.shape[0], _ptr(points), int(n), int(degree_bound), int(batch), _ptr(out), C.byref(rep)))
        return out, rep.as_dict()

    # ---- the same for columns whose row sets differ  (bbgpu_g1_recover_each and the host twin) ----
    @staticmethod
    def _g1_recover_each_args(rows, points, n, out):
        lists = [np.ascontiguousarray(r, dtype=np.uint32).reshape(-1) for r in rows]
        offsets = np.zeros(len(lists) + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum([r.shape[0] for r in lists])
        row = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, dtype=np.uint32)]))  # never empty
        if isinstance(points, np.ndarray):  # one array for the whole call, already in the order of the lists: handed over as it is
            flat = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
            if flat.shape[0] < int(offsets[-1]):
                raise ValueError("g1_recover_each: %d points for %d rows" % (flat.shape[0], int(offsets[-1])))
        else:
            pts = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8) for p in points]
            if len(lists) != len(pts):
                raise ValueError("g1_recover_each: %d row lists, %d point arrays" % (len(lists), len(pts)))
            for b, (r, p) in enumerate(zip(lists, pts)):
                if p.shape[0] < r.shape[0]:  # the library would read past the end
                    raise ValueError("g1_recover_each: column %d: %d points for %d rows" % (b, p.shape[0], r.shape[0]))
            flat = np.ascontiguousarray(np.concatenate([p[:r.shape[0]] for r, p in zip(lists, pts)] + [np.zeros((1, 8), dtype=np.uint64)]))
        batch = len(lists)
        if out is None:
            out = np.zeros((max(batch, 1), max(int(n), 1), 8), dtype=np.uint64)
        return offsets, row, flat, batch, out

    def g1_recover_each(self, rows, points, n, degree_bound, stream=None, out=None):
        """bbgpu_g1_recover_each: len(rows) columns of n points, each a codeword of degree < degree_bound, column b from ITS OWN listed rows (rows[b]:
        distinct indices below n, any order; points[b] (count_b, 8): listed row t, on the host -- or ONE array that holds them all in that order, which is
        not copied) -> ((batch, n, 8) all n points of every column -- `out` when given --, the report as a dict, (batch,) uint64 first_bad,
        G1RecoverEachReport.NONE where a column has none)."""
        offsets, row, flat, batch, out = self._g1_recover_each_args(rows, points, n, out)
        rep, first_bad = G1RecoverEachReport(), np.zeros(max(batch, 1), dtype=np.uint64)
        u32p = C.POINTER(C.c_uint32)
        self.lib.bbgpu_g1_recover_each.argtypes = [u32p, u32p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, C.POINTER(G1RecoverEachReport), C.c_void_p]
        self._chk(self.lib.bbgpu_g1_recover_each(offsets.ctypes.data_as(u32p), row.ctypes.data_as(u32p), _ptr(flat), int(n), int(degree_bound), batch, _ptr(out),
                                                 _ptr(first_bad), C.byref(rep), stream or 0))
        return out, rep.as_dict(), first_bad

    def host_g1_recover_each(self, rows, points, n, degree_bound, out=None):
        """bbgpu_host_g1_recover_each: the same on the host"""
        offsets, row, flat, batch, out = self._g1_recover_each_args(rows, points, n, out)
        rep, first_bad = G1RecoverEachReport(), np.zeros(max(batch, 1), dtype=np.uint64)
        u32p = C.POINTER(C.c_uint32)
        self.lib.bbgpu_host_g1_recover_each.argtypes = [u32p, u32p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, C.POINTER(G1RecoverEachReport)]
        self._chk(self.lib.bbgpu_host_g1_recover_each(offsets.ctypes.data_as(u32p), row.ctypes.data_as(u32p), _ptr(flat), int(n), int(degree_bound), batch,
                                                      _ptr(out), _ptr(first_bad), C.byref(rep)))
        return out, rep.as_dict(), first_bad

    # ---- transforms and the erasure decoder down the columns of a row-major matrix  (bbgpu_fr_ntt_columns_device, bbgpu_fr_recover_columns_device, twins) ----
    def fr_ntt_columns_device(self, d_ptr, rows, width, kind="fft", stride=None, stream=None):
        """bbgpu_fr_ntt_columns_device: every column of the resident rows x stride matrix at d_ptr (row r at element r * stride, columns [0, width))
        transformed in place, "fft" or "ifft" """
        self.lib.bbgpu_fr_ntt_columns_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
        self._chk(self.lib.bbgpu_fr_ntt_columns_device(d_ptr, int(rows), int(width), int(width) if stride is None else int(stride),
                                                       NTT_KINDS[kind] if isinstance(kind, str) else int(kind), stream or 0))

    def host_fr_ntt_columns(self, mem, rows, width, kind="fft", stride=None):
        """bbgpu_host_fr_ntt_columns: the same on a host matrix `mem` ((rows * stride, 4) uint64, or None for the refusal of a null pointer), in place"""
        self.lib.bbgpu_host_fr_ntt_columns.argtypes = [u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        self._chk(self.lib.bbgpu_host_fr_ntt_columns(_ptr(mem) if mem is not None else None, int(rows), int(width), int(width) if stride is None else int(stride),
                                                     NTT_KINDS[kind] if isinstance(kind, str) else int(kind)))
        return mem

    @staticmethod
    def _fr_columns_sets(row_sets, offsets, sets):
        lists = [np.ascontiguousarray(r, dtype=np.uint32).reshape(-1) for r in row_sets]
        if offsets is None:
            offsets = np.zeros(len(lists) + 1, dtype=np.uint32)
            offsets[1:] = np.cumsum([r.shape[0] for r in lists])
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        row = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, dtype=np.uint32)]))  # never empty
        return offsets, row, len(lists) if sets is None else int(sets)

    def fr_recover_columns_device(self, row_sets, d_ptr, rows, width, degree_bound, stride=None, want_first_bad=True, stream=None, offsets=None, sets=None):
        """bbgpu_fr_recover_columns_device: the rows that column j's set (row_sets[j mod len(row_sets)]: the PRESENT rows, distinct, any order) misses are
        written into the resident matrix at d_ptr, every column a codeword of degree < degree_bound -> (the report as a dict, (width,) uint32 first_bad
        -- FrRecoverColumnsReport.NONE where a column has none -- or None without want_first_bad).  offsets / sets: the raw arguments in place of the ones
        derived from the lists (the refusals)."""
        offsets, row, sets = self._fr_columns_sets(row_sets, offsets, sets)
        rep, first_bad = FrRecoverColumnsReport(), np.zeros(max(int(width), 1), dtype=np.uint32) if want_first_bad else None
        u32p = C.POINTER(C.c_uint32)
        self.lib.bbgpu_fr_recover_columns_device.argtypes = [u32p, u32p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, u32p,
                                                             C.POINTER(FrRecoverColumnsReport), C.c_void_p]
        self._chk(self.lib.bbgpu_fr_recover_columns_device(offsets.ctypes.data_as(u32p), row.ctypes.data_as(u32p), sets, d_ptr, int(rows), int(width),
                                                           int(width) if stride is None else int(stride), int(degree_bound),
                                                           first_bad.ctypes.data_as(u32p) if want_first_bad else None, C.byref(rep), stream or 0))
        return rep.as_dict(), first_bad

    def host_fr_recover_columns(self, row_sets, mem, rows, width, degree_bound, stride=None, want_first_bad=True, offsets=None, sets=None, first_bad=None,
                                report=None):
        """bbgpu_host_fr_recover_columns: the same on a host matrix `mem` ((rows * stride, 4) uint64), in place.  first_bad / report: the caller's own
        buffers (so that a refusal can be seen to leave them alone)."""
        offsets, row, sets = self._fr_columns_sets(row_sets, offsets, sets)
        rep = FrRecoverColumnsReport() if report is None else report
        if first_bad is None and want_first_bad:
            first_bad = np.zeros(max(int(width), 1), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self.lib.bbgpu_host_fr_recover_columns.argtypes = [u32p, u32p, C.c_int, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, u32p,
                                                           C.POINTER(FrRecoverColumnsReport)]
        self._chk(self.lib.bbgpu_host_fr_recover_columns(offsets.ctypes.data_as(u32p), row.ctypes.data_as(u32p), sets, _ptr(mem) if mem is not None else None,
                                                         int(rows), int(width), int(width) if stride is None else int(stride), int(degree_bound),
                                                         first_bad.ctypes.data_as(u32p) if first_bad is not None else None, C.byref(rep)))
        return rep.as_dict(), first_bad

    def g1_set_stage_mapping(self, mapping):
        """bbgpu_g1_set_stage_mapping: 0 the library's choice of stage kernel for g1_ntt and g1_recover, 1 k_lagrange_stage and 2 k_g1_stage_cols for every
        shape (tools/g1_recover_bench.py)"""
        self._chk(self.lib.bbgpu_g1_set_stage_mapping(int(mapping)))

    # ---- do these openings hold?  (bbgpu_kzg_check_openings, bbgpu_kzg_check_open_all and the host twins) ----
    def _kzg_check_openings(self, fn, commitments, z, y, proofs, g2_x, which, seed, locate):
        cs = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
        ps = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8)
        zs, ys = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4), np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 4)
        labels = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1) if which is not None else None
        count = ps.shape[0]
        if zs.shape[0] != count or ys.shape[0] != count or (labels is None and cs.shape[0] != count) or (labels is not None and labels.shape[0] != count):
            raise ValueError("kzg_check_openings: %d proofs, %d z, %d y, %d commitments, %s labels" %
                             (count, zs.shape[0], ys.shape[0], cs.shape[0], "no" if labels is None else labels.shape[0]))
        g2, sd, g2p, sdp, flags = self._srs_check_args(g2_x, seed, locate)
        rep = KzgCheckReport()
        fn.argtypes = [u64p, C.POINTER(C.c_uint32), C.c_size_t, u64p, u64p, u64p, C.c_size_t, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        lp = labels.ctypes.data_as(C.POINTER(C.c_uint32)) if labels is not None else None
        self._chk(fn(_ptr(cs), lp, cs.shape[0], _ptr(zs), _ptr(ys), _ptr(ps), count, g2p, sdp, flags, C.byref(rep)))
        return rep.as_dict()

    def _kzg_check_open_all(self, fn, commitments, values, proofs, n, g2_x, batch, stride, seed, locate):
        cs = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
        ps = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8)
        vs = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        batch = cs.shape[0] if batch is None else int(batch)
        stride = int(n) if stride is None else int(stride)
        if 1 <= batch <= 64 and int(n) >= 1 and (cs.shape[0] < batch or ps.shape[0] < batch * int(n) or vs.shape[0] < (batch - 1) * stride + int(n)):
            raise ValueError("kzg_check_open_all: batch %d of n = %d at stride %d over %d commitments, %d values, %d proofs" %
                             (batch, n, stride, cs.shape[0], vs.shape[0], ps.shape[0]))
        g2, sd, g2p, sdp, flags = self._srs_check_args(g2_x, seed, locate)
        rep = KzgCheckReport()
        fn.argtypes = [u64p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        self._chk(fn(_ptr(cs), _ptr(vs), stride, _ptr(ps), int(n), batch, g2p, sdp, flags, C.byref(rep)))
        return rep.as_dict()

    def kzg_check_openings(self, commitments, z, y, proofs, g2_x, which=None, seed=None, locate=False):
        """bbgpu_kzg_check_openings: up to 2^20 claims (C, z_t, y_t, pi_t) checked on the GPU by two MSMs and ONE pairing product.  which None: one
        commitment per claim, (count, 8); else (count,) labels into at most 64 shared commitments.  seed None: drawn from the operating system (whoever
        made the proofs must not know it).  Returns the report as a dict (ok, bad_points, first_bad, first_failing, rounds, seed, a, b ...)."""
        return self._kzg_check_openings(self.lib.bbgpu_kzg_check_openings, commitments, z, y, proofs, g2_x, which, seed, locate)

    def host_kzg_check_openings_batch(self, commitments, z, y, proofs, g2_x, which=None, seed=None, locate=False):
        """bbgpu_host_kzg_check_openings_batch: the same definition on the host; no GPU needed"""
        return self._kzg_check_openings(self.lib.bbgpu_host_kzg_check_openings_batch, commitments, z, y, proofs, g2_x, which, seed, locate)

    def kzg_check_open_all(self, commitments, values, proofs, n, g2_x, batch=None, stride=None, seed=None, locate=False):
        """bbgpu_kzg_check_open_all: what kzg_open_all_device writes, checked in one call: commitments (batch, 8), values (batch * stride, 4) with
        values[b * stride + i] = f_b(omega^i), proofs (batch, n, 8).  Returns the report as a dict."""
        return self._kzg_check_open_all(self.lib.bbgpu_kzg_check_open_all, commitments, values, proofs, n, g2_x, batch, stride, seed, locate)

    def host_kzg_check_open_all(self, commitments, values, proofs, n, g2_x, batch=None, stride=None, seed=None, locate=False):
        """bbgpu_host_kzg_check_open_all: the same definition on the host; no GPU needed"""
        return self._kzg_check_open_all(self.lib.bbgpu_host_kzg_check_open_all, commitments, values, proofs, n, g2_x, batch, stride, seed, locate)

    def kzg_check_last_timing(self):
        """bbgpu_kzg_check_last_timing: wall ms of the last kzg_check_openings, kzg_check_open_all, kzg_check_cells or kzg_check_open_cosets by stage
        (claims_ms: the uploads and the per-claim kernel, for cells the per-cell and the coefficient kernel)"""
        buf = (C.c_double * 5)()
        self.lib.bbgpu_kzg_check_last_timing.argtypes = [C.POINTER(C.c_double)]
        self._chk(self.lib.bbgpu_kzg_check_last_timing(buf))
        return dict(zip(("total_ms", "claims_ms", "fold_ms", "msm_ms", "host_tail_ms"), buf))

    # ---- do these cell proofs hold?  (bbgpu_kzg_check_cells, bbgpu_kzg_check_open_cosets, the host twins and the key check) ----
    def _kzg_check_cells(self, fn, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed, locate, flags):
        cs = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
        ps = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8)
        vs = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        head = np.ascontiguousarray(g1_head, dtype=np.uint64).reshape(-1, 8)
        labels, cells = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1), np.ascontiguousarray(cell, dtype=np.uint32).reshape(-1)
        count = ps.shape[0]
        if labels.shape[0] != count or cells.shape[0] != count or (1 <= int(coset) <= 64 and (vs.shape[0] != count * int(coset) or head.shape[0] < int(coset))):
            raise ValueError("kzg_check_cells: %d proofs, %d labels, %d cell indices, %d values, %d head rows at coset %d" %
                             (count, labels.shape[0], cells.shape[0], vs.shape[0], head.shape[0], coset))
        g2, sd, g2p, sdp, fl = self._srs_check_args(g2_xl, seed, locate)
        rep = KzgCheckReport()
        u32p = C.POINTER(C.c_uint32)
        fn.argtypes = [u64p, C.c_size_t, u32p, u32p, u64p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        self._chk(fn(_ptr(cs), cs.shape[0], labels.ctypes.data_as(u32p), cells.ctypes.data_as(u32p), _ptr(vs), _ptr(ps), count, int(n), int(coset), _ptr(head),
                     g2p, sdp, fl if flags is None else int(flags), C.byref(rep)))
        return rep.as_dict()

    def _kzg_check_open_cosets(self, fn, commitments, values, proofs, n, coset, g1_head, g2_xl, batch, stride, seed, locate, flags, max_batch=64):
        cs = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
        ps = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8)
        vs = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        head = np.ascontiguousarray(g1_head, dtype=np.uint64).reshape(-1, 8)
        batch = cs.shape[0] if batch is None else int(batch)
        stride = int(n) if stride is None else int(stride)
        if 1 <= batch <= max_batch and 1 <= int(coset) <= 64 and int(n) >= 1 and (cs.shape[0] < batch or ps.shape[0] < batch * (int(n) // int(coset)) or
                                                                            vs.shape[0] < (batch - 1) * stride + int(n) or head.shape[0] < int(coset)):
            raise ValueError("kzg_check_open_cosets: batch %d of n = %d, coset %d at stride %d over %d commitments, %d values, %d proofs, %d head rows" %
                             (batch, n, coset, stride, cs.shape[0], vs.shape[0], ps.shape[0], head.shape[0]))
        g2, sd, g2p, sdp, fl = self._srs_check_args(g2_xl, seed, locate)
        rep = KzgCheckReport()
        fn.argtypes = [u64p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        self._chk(fn(_ptr(cs), _ptr(vs), stride, _ptr(ps), int(n), int(coset), batch, _ptr(head), g2p, sdp, fl if flags is None else int(flags), C.byref(rep)))
        return rep.as_dict()

    def kzg_check_cells(self, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed=None, locate=False, flags=None):
        """bbgpu_kzg_check_cells: `count` cell proofs checked on the GPU by two MSMs and ONE pairing product.  Cell t is cell cell[t] (< n / coset) of
        commitments[which[t]] (at most 64 of them); values (count * coset, 4): f(omega^(k + (n / coset) j)), j < coset, per cell; proofs (count, 8);
        g1_head (coset, 8): the first rows of the monomial string; g2_xl: [x^coset] G2.  seed None: drawn from the operating system (whoever made the
        proofs must not know it).  Returns the report as a dict (ok, bad_points, first_bad, first_failing, rounds, seed, a, b ...)."""
        return self._kzg_check_cells(self.lib.bbgpu_kzg_check_cells, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed, locate, flags)

    def host_kzg_check_cells(self, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed=None, locate=False, flags=None):
        """bbgpu_host_kzg_check_cells: the same definition on the host; no GPU needed"""
        return self._kzg_check_cells(self.lib.bbgpu_host_kzg_check_cells, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed, locate,
                                     flags)

    def kzg_check_open_cosets(self, commitments, values, proofs, n, coset, g1_head, g2_xl, batch=None, stride=None, seed=None, locate=False, flags=None):
        """bbgpu_kzg_check_open_cosets: what kzg_open_cosets_device writes, checked in one call: commitments (batch, 8), values (batch * stride, 4) the
        size-n transforms (ntt_device), proofs (batch, n / coset, 8).  Returns the report as a dict; its count is in cells."""
        return self._kzg_check_open_cosets(self.lib.bbgpu_kzg_check_open_cosets, commitments, values, proofs, n, coset, g1_head, g2_xl, batch, stride, seed,
                                           locate, flags)

    def host_kzg_check_open_cosets(self, commitments, values, proofs, n, coset, g1_head, g2_xl, batch=None, stride=None, seed=None, locate=False, flags=None):
        """bbgpu_host_kzg_check_open_cosets: the same definition on the host; no GPU needed"""
        return self._kzg_check_open_cosets(self.lib.bbgpu_host_kzg_check_open_cosets, commitments, values, proofs, n, coset, g1_head, g2_xl, batch, stride,
                                           seed, locate, flags)

    # ---- the same for a 2-D layout: up to 2^16 commitments per call (bbgpu_kzg_check_cells_layout, bbgpu_kzg_check_open_cosets_layout, the host twins) ----
    MAX_LAYOUT_COMMITMENTS = 1 << 16

    def kzg_check_cells_layout(self, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed=None, locate=False, flags=None):
        """bbgpu_kzg_check_cells_layout: kzg_check_cells over up to 2^16 commitments -- they are tested and converted on the GPU, the cells grouped by label
        there once per call.  Same arguments, same report; up to 64 commitments the report is kzg_check_cells' field for field."""
        return self._kzg_check_cells(self.lib.bbgpu_kzg_check_cells_layout, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed, locate,
                                     flags)

    def host_kzg_check_cells_layout(self, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed=None, locate=False, flags=None):
        """bbgpu_host_kzg_check_cells_layout: the same definition on the host; no GPU needed"""
        return self._kzg_check_cells(self.lib.bbgpu_host_kzg_check_cells_layout, commitments, which, cell, values, proofs, n, coset, g1_head, g2_xl, seed,
                                     locate, flags)

    def kzg_check_open_cosets_layout(self, commitments, values, proofs, n, coset, g1_head, g2_xl, batch=None, stride=None, seed=None, locate=False, flags=None):
        """bbgpu_kzg_check_open_cosets_layout: kzg_check_open_cosets over a batch of up to 2^16 polynomials (batch x n <= 2^20)"""
        return self._kzg_check_open_cosets(self.lib.bbgpu_kzg_check_open_cosets_layout, commitments, values, proofs, n, coset, g1_head, g2_xl, batch, stride,
                                           seed, locate, flags, max_batch=self.MAX_LAYOUT_COMMITMENTS)

    def host_kzg_check_open_cosets_layout(self, commitments, values, proofs, n, coset, g1_head, g2_xl, batch=None, stride=None, seed=None, locate=False,
                                          flags=None):
        """bbgpu_host_kzg_check_open_cosets_layout: the same definition on the host; no GPU needed"""
        return self._kzg_check_open_cosets(self.lib.bbgpu_host_kzg_check_open_cosets_layout, commitments, values, proofs, n, coset, g1_head, g2_xl, batch,
                                           stride, seed, locate, flags, max_batch=self.MAX_LAYOUT_COMMITMENTS)

    def host_kzg_cells_key_check(self, g1_head, coset, g2_x, g2_xl):
        """bbgpu_host_kzg_cells_key_check: is g2_xl = [x^coset] G2 for the x of g1_head (coset, 8) and g2_x?  One pairing product; host only -> bool"""
        head = np.ascontiguousarray(g1_head, dtype=np.uint64).reshape(-1, 8)
        if 1 <= int(coset) <= 64 and head.shape[0] < int(coset):
            raise ValueError("host_kzg_cells_key_check: %d head rows at coset %d" % (head.shape[0], coset))
        a, b = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16), np.ascontiguousarray(g2_xl, dtype=np.uint64).reshape(16)
        ok = C.c_int(0)
        self.lib.bbgpu_host_kzg_cells_key_check.argtypes = [u64p, C.c_size_t, u64p, u64p, C.POINTER(C.c_int)]
        self._chk(self.lib.bbgpu_host_kzg_cells_key_check(_ptr(head), int(coset), _ptr(a), _ptr(b), C.byref(ok)))
        return bool(ok.value)

    # ---- is this table the Lagrange form of that string?  (bbgpu_srs_lagrange_check and its host twin) ----
    def srs_lagrange_check(self, lagrange_handle, monomial_handle, n, seed=None, locate=False):
        """bbgpu_srs_lagrange_check: rows [0, n) of the Lagrange handle on the curve, and equal to L_i of the monomial handle's rows by two MSMs and one
        transform.  seed None: drawn from the operating system.  Returns an SrsLagrangeCheckReport (.ok, .as_dict())."""
        sd = np.ascontiguousarray(seed, dtype=np.uint64).reshape(4) if seed is not None else None
        rep = SrsLagrangeCheckReport()
        self.lib.bbgpu_srs_lagrange_check.argtypes = [C.c_int, C.c_int, C.c_size_t, u64p, C.c_int, C.POINTER(SrsLagrangeCheckReport)]
        self._chk(self.lib.bbgpu_srs_lagrange_check(int(lagrange_handle), int(monomial_handle), int(n), _ptr(sd) if sd is not None else None,
                                                    1 if locate else 0, C.byref(rep)))
        return rep

    def host_srs_lagrange_check(self, lagrange_table, monomial_table, n=None, seed=None, locate=False):
        """bbgpu_host_srs_lagrange_check: the same check over the even entries of two (2n, 8) endo tables, on the host; no GPU needed"""
        n = lagrange_table.shape[0] // 2 if n is None else n
        sd = np.ascontiguousarray(seed, dtype=np.uint64).reshape(4) if seed is not None else None
        rep = SrsLagrangeCheckReport()
        self.lib.bbgpu_host_srs_lagrange_check.argtypes = [u64p, u64p, C.c_size_t, u64p, C.c_int, C.POINTER(SrsLagrangeCheckReport)]
        self._chk(self.lib.bbgpu_host_srs_lagrange_check(_ptr(lagrange_table), _ptr(monomial_table), int(n), _ptr(sd) if sd is not None else None,
                                                         1 if locate else 0, C.byref(rep)))
        return rep

    def selftest_endo_split(self, k, on_device=True):
        """bbgpu_selftest_endo_split: k (n, 4) plain integers -> (n, 6): |k1| (2), |k2| (2), flags, 0"""
        k = np.ascontiguousarray(k, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((k.shape[0], 6), dtype=np.uint64)
        self.lib.bbgpu_selftest_endo_split.argtypes = [C.c_int, u64p, C.c_size_t, u64p]
        self._chk(self.lib.bbgpu_selftest_endo_split(1 if on_device else 0, _ptr(k), k.shape[0], _ptr(out)))
        return out

    # ---- is this proof valid?  (bbgpu_plonk_verify_batch and its host twin) ----------------------------------------------------------
    WIDGET_BOOL, WIDGET_MIMC, WIDGET_SEQUENTIAL = 1, 2, 4

    @staticmethod
    def _verify_args(proofs, seed):
        proofs = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 120)
        sd = np.ascontiguousarray(seed, dtype=np.uint64).reshape(4) if seed is not None else None
        return proofs, sd, (_ptr(sd) if sd is not None else None), np.zeros(max(1, proofs.shape[0]), dtype=np.uint32)

    def plonk_verifier_create(self, n, widgets, vk, g2_x):
        """bbgpu_plonk_verifier_create: vk as bbgpu_plonk_preprocess writes it ((8..12, 8) uint64), g2_x = x * G2 (16,); host work only"""
        key = np.zeros(96, dtype=np.uint64)
        v = np.ascontiguousarray(vk, dtype=np.uint64).reshape(-1)
        key[:v.size] = v
        g2 = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16)
        self.lib.bbgpu_plonk_verifier_create.argtypes = [C.c_size_t, C.c_int, u64p, u64p]
        h = self.lib.bbgpu_plonk_verifier_create(int(n), int(widgets), _ptr(key), _ptr(g2))
        self._chk(min(h, 0))
        return h

    def plonk_verifier_destroy(self, verifier):
        self._chk(self.lib.bbgpu_plonk_verifier_destroy(int(verifier)))

    def plonk_verify_batch(self, verifier, proofs, seed=None, locate=False):
        """bbgpu_plonk_verify_batch: proofs (count, 120) uint64 of the handle's circuit.  seed None: drawn from the operating system (whoever made the
        proofs must not know it).  Returns a PlonkVerifyReport (.ok, .status, .as_dict())."""
        proofs, sd, sdp, status = self._verify_args(proofs, seed)
        rep = PlonkVerifyReport()
        self.lib.bbgpu_plonk_verify_batch.argtypes = [C.c_int, u64p, C.c_size_t, u64p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(PlonkVerifyReport)]
        self._chk(self.lib.bbgpu_plonk_verify_batch(int(verifier), _ptr(proofs), proofs.shape[0], sdp, 1 if locate else 0,
                                                    status.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rep)))
        rep.status = status[:proofs.shape[0]]
        return rep

    def plonk_verify_last_timing(self):
        """bbgpu_plonk_verify_last_timing: wall ms of the last plonk_verify_batch or plonk_verify_multi by stage"""
        buf = (C.c_double * 5)()
        self.lib.bbgpu_plonk_verify_last_timing.argtypes = [C.POINTER(C.c_double)]
        self._chk(self.lib.bbgpu_plonk_verify_last_timing(buf))
        return dict(zip(("total_ms", "terms_ms", "fold_ms", "msm_ms", "host_tail_ms"), buf))

    def host_plonk_verify_batch(self, n, widgets, vk, g2_x, proofs, seed=None, locate=False):
        """bbgpu_host_plonk_verify_batch: the same definition on the host; no GPU needed"""
        proofs, sd, sdp, status = self._verify_args(proofs, seed)
        key = np.ascontiguousarray(vk, dtype=np.uint64).reshape(-1).copy()
        g2 = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16)
        rep = PlonkVerifyReport()
        self.lib.bbgpu_host_plonk_verify_batch.argtypes = [C.c_size_t, C.c_int, u64p, u64p, u64p, C.c_size_t, u64p, C.c_int, C.POINTER(C.c_uint32),
                                                           C.POINTER(PlonkVerifyReport)]
        self._chk(self.lib.bbgpu_host_plonk_verify_batch(int(n), int(widgets), _ptr(key), _ptr(g2), _ptr(proofs), proofs.shape[0], sdp,
                                                         1 if locate else 0, status.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rep)))
        rep.status = status[:proofs.shape[0]]
        return rep

    @staticmethod
    def _verify_labels(circuit):
        labels = np.ascontiguousarray(circuit, dtype=np.uint32).reshape(-1)
        return labels, labels.ctypes.data_as(C.POINTER(C.c_uint32))

    def plonk_verify_multi(self, verifiers, circuit, proofs, seed=None, locate=False):
        """bbgpu_plonk_verify_multi: proofs (count, 120) uint64 of SEVERAL circuits under one x * G2 in one batch; verifiers: the handles, circuit (count,):
        proof j claims the circuit of verifiers[circuit[j]].  One pairing check for all.  Returns a PlonkVerifyReport."""
        proofs, sd, sdp, status = self._verify_args(proofs, seed)
        labels, lp = self._verify_labels(circuit)
        if labels.shape[0] != proofs.shape[0]:
            raise ValueError("plonk_verify_multi: %d labels for %d proofs" % (labels.shape[0], proofs.shape[0]))
        hs = (C.c_int * max(1, len(verifiers)))(*[int(h) for h in verifiers])
        rep = PlonkVerifyReport()
        self.lib.bbgpu_plonk_verify_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint32), u64p, C.c_size_t, u64p, C.c_int,
                                                      C.POINTER(C.c_uint32), C.POINTER(PlonkVerifyReport)]
        self._chk(self.lib.bbgpu_plonk_verify_multi(hs, len(verifiers), lp, _ptr(proofs), proofs.shape[0], sdp, 1 if locate else 0,
                                                    status.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rep)))
        rep.status = status[:proofs.shape[0]]
        return rep

    def host_plonk_verify_multi(self, keys, g2_x, circuit, proofs, seed=None, locate=False):
        """bbgpu_host_plonk_verify_multi: the same definition on the host; keys: one (n, widgets, vk) per circuit; no GPU needed"""
        proofs, sd, sdp, status = self._verify_args(proofs, seed)
        labels, lp = self._verify_labels(circuit)
        if labels.shape[0] != proofs.shape[0]:
            raise ValueError("host_plonk_verify_multi: %d labels for %d proofs" % (labels.shape[0], proofs.shape[0]))
        vks = [np.ascontiguousarray(vk, dtype=np.uint64).reshape(-1).copy() for _, _, vk in keys]
        ks = (PlonkVerifyKey * max(1, len(keys)))(*[PlonkVerifyKey(int(n), int(w), v.ctypes.data) for (n, w, _), v in zip(keys, vks)])
        g2 = np.ascontiguousarray(g2_x, dtype=np.uint64).reshape(16)
        rep = PlonkVerifyReport()
        self.lib.bbgpu_host_plonk_verify_multi.argtypes = [C.POINTER(PlonkVerifyKey), C.c_int, u64p, C.POINTER(C.c_uint32), u64p, C.c_size_t, u64p,
                                                           C.c_int, C.POINTER(C.c_uint32), C.POINTER(PlonkVerifyReport)]
        self._chk(self.lib.bbgpu_host_plonk_verify_multi(ks, len(keys), _ptr(g2), lp, _ptr(proofs), proofs.shape[0], sdp, 1 if locate else 0,
                                                         status.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rep)))
        rep.status = status[:proofs.shape[0]]
        return rep

    def srs_cache_stats(self):
        """(live tables, of which registered on first sight, device bytes those hold)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_uint64(0)
        self._chk(self.lib.bbgpu_srs_cache_stats(C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def init_devices(self, devices):
        """bind one device context per entry of `devices` (bbgpu_init_devices)"""
        devices = [int(d) for d in devices]
        arr = (C.c_int * max(1, len(devices)))(*devices)
        self._chk(self.lib.bbgpu_init_devices(arr, len(devices)))

    def num_contexts(self):
        return int(self.lib.bbgpu_num_contexts())

    def memory_stats(self, context=None):
        """device / pinned bytes the library holds for the life of the process, as a dict (bbgpu_memory_stats: the sum over the device
        contexts; context=k: context k's share, bbgpu_memory_stats_context)"""
        info = MemoryInfo()
        if context is None:
            self._chk(self.lib.bbgpu_memory_stats(C.byref(info)))
        else:
            self._chk(self.lib.bbgpu_memory_stats_context(int(context), C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in MemoryInfo._fields_}

    def fault_inject(self, spec):
        """testing: "alloc:k" | "h2d:k" | "d2h:k" | "launch:k" makes the k-th such call from now on fail once; None disarms (bbgpu_fault_inject)"""
        self._chk(self.lib.bbgpu_fault_inject(spec.encode() if spec else None))

    def fault_stats(self):
        """funnel counters since the last spec, live device allocations, MSM slots in flight, as a dict (bbgpu_fault_stats)"""
        info = FaultInfo()
        self._chk(self.lib.bbgpu_fault_stats(C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in FaultInfo._fields_}

    def srs_set_validate(self, handle, full):
        """exact mode of the address-keyed table cache: host-pointer MSMs re-hash every row they use (handle -1: default for tables registered from now on)"""
        self._chk(self.lib.bbgpu_srs_set_validate(int(handle), 1 if full else 0))

    def srs_release(self, handle):
        self._chk(self.lib.bbgpu_srs_release(handle))

    def pippenger(self, scalars, points_endo_table, n=None):
        """returns the normalised g1::element (12,) -- or the infinity flag in y limb 3"""
        n = scalars.shape[0] if n is None else n
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.lib.bbgpu_msm_g1(_ptr(scalars), _ptr(points_endo_table), n, _ptr(out)))
        return out

    def pippenger_low_memory(self, scalars, points, n=None):
        """scalar_multiplication::pippenger_low_memory (:142-262): `points` is the PLAIN n-entry table (n x 8 u64), not the endo table"""
        n = scalars.shape[0] if n is None else n
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.lib.bbgpu_msm_g1_plain(_ptr(scalars), _ptr(points), n, _ptr(out)))
        return out

    def batched_scalar_multiplications(self, jobs):
        """jobs: list of (points_endo_table, scalars, n); returns list of normalised outputs"""
        arr = (MsmJob * len(jobs))()
        for j, (pts, sc, n) in zip(arr, jobs):
            j.points, j.scalars, j.num_elements = _ptr(pts), _ptr(sc), n
        self._chk(self.lib.bbgpu_msm_g1_batch(arr, len(jobs)))
        return [np.array(list(j.output), dtype=np.uint64) for j in arr]

    def msm_num_windows(self, n):
        return int(self.lib.bbgpu_msm_num_windows(n))

    def srs_num_windows(self, handle, n):
        return self._chk(self.lib.bbgpu_srs_num_windows(handle, n))

    def set_host_thresholds(self, msm_max_points, ntt_max_elements):
        """SURVEY 8b small sizes: host-pointer MSMs / transforms up to these sizes are answered on the host (0, 0: everything on the GPU)"""
        self.lib.bbgpu_set_host_thresholds(int(msm_max_points), int(ntt_max_elements))

    def set_table_share(self, rank, world):
        """tables registered from now on keep only the digit windows rank `rank` of `world` touches (multi-GPU row split); (0, 1): full tables"""
        self.lib.bbgpu_set_table_share(int(rank), int(world))

    def set_point_share(self, world):
        """tables registered from now on are a rank's n / world points of a larger MSM (point-range split): window size as for the whole; 1: default"""
        self.lib.bbgpu_set_point_share(int(world))

    def set_precompute(self, on=True):
        self.lib.bbgpu_set_precompute(1 if on else 0)

    def msm_device(self, handle, d_scalars_ptr, n, offset=0, window_begin=0, window_end=None, stream=None):
        if window_end is None:
            window_end = self.srs_num_windows(handle, n)
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.lib.bbgpu_msm_g1_device(handle, offset, C.c_void_p(d_scalars_ptr), n, window_begin, window_end,
                                               _ptr(out), C.c_void_p(stream or 0)))
        return out

    def msm_device_async(self, handle, d_scalars_ptr, n, offset=0, window_begin=0, window_end=None, stream=None):
        """enqueue; returns a ticket for msm_wait().  At most eight MSMs in flight."""
        if window_end is None:
            window_end = self.srs_num_windows(handle, n)
        return self._chk(self.lib.bbgpu_msm_g1_device_async(handle, offset, C.c_void_p(d_scalars_ptr), n, window_begin, window_end,
                                                           C.c_void_p(stream or 0)))

    def msm_device_rows_async(self, handle, d_scalars_ptr, n, row_begin, row_end, offset=0, stream=None):
        """share [row_begin, row_end) of the W * n (window, point) pairs, window-major (row = w * n + i): a split that need not follow
        window boundaries (needs the window tables); returns a ticket for msm_wait()"""
        return self._chk(self.lib.bbgpu_msm_g1_device_rows_async(handle, offset, C.c_void_p(d_scalars_ptr), n, row_begin, row_end,
                                                                C.c_void_p(stream or 0)))

    def msm_device_buckets_async(self, handle, d_scalars_ptr, n, share, share_count, offset=0, stream=None):
        """share `share` of `share_count` of the BUCKET range (all windows, all points; needs complete window tables): 1 / N of the mixed
        additions and 1 / N of the bucket reduction; returns a ticket for msm_wait()"""
        self.lib.bbgpu_msm_g1_device_buckets_async.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        return self._chk(self.lib.bbgpu_msm_g1_device_buckets_async(handle, offset, C.c_void_p(d_scalars_ptr), n, share, share_count, C.c_void_p(stream or 0)))

    def srs_has_window_tables(self, handle):
        return self._chk(self.lib.bbgpu_srs_has_window_tables(handle)) == 1

    def msm_wait(self, ticket):
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.lib.bbgpu_msm_g1_wait(ticket, _ptr(out)))
        return out

    def msm_device_batch_async(self, handle, d_scalars_ptrs, n, offset=0, stream=None):
        """several MSMs over the same resident points as one pass (table mode); returns a ticket for msm_batch_wait()"""
        arr = (C.c_void_p * len(d_scalars_ptrs))(*d_scalars_ptrs)
        t = self._chk(self.lib.bbgpu_msm_g1_device_batch_async(handle, offset, arr, len(d_scalars_ptrs), n, C.c_void_p(stream or 0)))
        return t, len(d_scalars_ptrs)

    def msm_batch_wait(self, ticket):
        t, jobs = ticket
        out = np.zeros((jobs, 12), dtype=np.uint64)
        self._chk(self.lib.bbgpu_msm_g1_batch_wait(t, _ptr(out)))
        return out

    def g1_sum(self, points12):
        points12 = np.ascontiguousarray(points12, dtype=np.uint64).reshape(-1, 12)
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.lib.bbgpu_g1_sum(_ptr(points12), points12.shape[0], _ptr(out)))
        return out

    # ---- host fallbacks of the drop-in boundary (what the C++ shim computes with after a GPU call has failed; no GPU needed) -----
    def host_msm(self, scalars, points, n=None, plain=False):
        n = scalars.shape[0] if n is None else n
        out = np.zeros(12, dtype=np.uint64)
        self.lib.bbgpu_host_msm_g1.argtypes = [u64p, u64p, C.c_size_t, C.c_int, u64p]
        self._chk(self.lib.bbgpu_host_msm_g1(_ptr(scalars), _ptr(points), n, int(plain), _ptr(out)))
        return out

    def host_ntt(self, coeffs, kind, constant=None):
        kind = NTT_KINDS[kind] if isinstance(kind, str) else kind
        cp = _ptr(np.ascontiguousarray(constant, dtype=np.uint64)) if constant is not None else None
        self.lib.bbgpu_host_ntt.argtypes = [u64p, C.c_size_t, C.c_int, u64p]
        self._chk(self.lib.bbgpu_host_ntt(_ptr(coeffs), coeffs.shape[0], kind, cp))
        return coeffs

    def host_evaluate(self, coeffs, z):
        out = np.zeros(4, dtype=np.uint64)
        self.lib.bbgpu_host_fr_evaluate.argtypes = [u64p, C.c_size_t, u64p, u64p]
        self._chk(self.lib.bbgpu_host_fr_evaluate(_ptr(coeffs), coeffs.shape[0], _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(out)))
        return out

    def host_kate_opening(self, src, z):
        dest, f = np.zeros_like(src), np.zeros(4, dtype=np.uint64)
        self.lib.bbgpu_host_kate_opening.argtypes = [u64p, u64p, C.c_size_t, u64p, u64p]
        self._chk(self.lib.bbgpu_host_kate_opening(_ptr(src), _ptr(dest), src.shape[0], _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(f)))
        return dest, f

    def host_evaluate_lagrange(self, values, z, n=None, batch=1, stride=None):
        """bbgpu_host_fr_evaluate_lagrange: values (batch * stride, 4) -> (batch, 4); n defaults to the stride, the stride to rows / batch"""
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        stride = values.shape[0] // max(int(batch), 1) if stride is None else stride
        n = stride if n is None else n
        out = np.zeros((max(int(batch), 1), 4), dtype=np.uint64)
        self.lib.bbgpu_host_fr_evaluate_lagrange.argtypes = [u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p]
        self._chk(self.lib.bbgpu_host_fr_evaluate_lagrange(_ptr(values), n, stride, batch, _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(out)))
        return out

    def host_kate_opening_lagrange(self, values, z, n=None, batch=1, stride=None, out=None):
        """bbgpu_host_kate_opening_lagrange -> (quotient values in the layout of `values`, f(z) as (batch, 4)); out: the array to write (may be `values`
        itself), default a copy of `values` (so that the elements between the polynomials show they were left alone)"""
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        stride = values.shape[0] // max(int(batch), 1) if stride is None else stride
        n = stride if n is None else n
        out = values.copy() if out is None else out
        f = np.zeros((max(int(batch), 1), 4), dtype=np.uint64)
        self.lib.bbgpu_host_kate_opening_lagrange.argtypes = [u64p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p]
        self._chk(self.lib.bbgpu_host_kate_opening_lagrange(_ptr(values), _ptr(out), n, stride, batch, _ptr(np.ascontiguousarray(z, dtype=np.uint64)), _ptr(f)))
        return out, f

    def host_fold(self, values, gamma, n=None, batch=None, stride=None, out=None):
        """bbgpu_host_fr_fold -> (n, 4): sum_b gamma_b v_b, or `out` with that added to it"""
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        g = np.ascontiguousarray(gamma, dtype=np.uint64).reshape(-1, 4)
        batch = g.shape[0] if batch is None else batch
        stride = values.shape[0] // max(int(batch), 1) if stride is None else stride
        n = stride if n is None else n
        acc = out is not None
        out = np.zeros((max(int(n), 1), 4), dtype=np.uint64) if out is None else out
        self.lib.bbgpu_host_fr_fold.argtypes = [u64p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, C.c_int]
        self._chk(self.lib.bbgpu_host_fr_fold(_ptr(out), _ptr(values), n, stride, batch, _ptr(g), int(acc)))
        return out

    def host_kate_opening_lagrange_folded(self, values, gamma, z, n=None, batch=None, stride=None, out=None):
        """bbgpu_host_kate_opening_lagrange_folded -> (quotient (n, 4), F(z) as (4,)); with `out` the quotient is added to it"""
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        g = np.ascontiguousarray(gamma, dtype=np.uint64).reshape(-1, 4)
        batch = g.shape[0] if batch is None else batch
        stride = values.shape[0] // max(int(batch), 1) if stride is None else stride
        n = stride if n is None else n
        acc = out is not None
        out = np.zeros((max(int(n), 1), 4), dtype=np.uint64) if out is None else out
        f = np.zeros(4, dtype=np.uint64)
        self.lib.bbgpu_host_kate_opening_lagrange_folded.argtypes = [u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, u64p, C.c_int, u64p]
        self._chk(self.lib.bbgpu_host_kate_opening_lagrange_folded(_ptr(values), n, stride, batch, _ptr(g), _ptr(np.ascontiguousarray(z, dtype=np.uint64)),
                                                                   _ptr(out), int(acc), _ptr(f)))
        return out, f

    def host_kzg_check_openings(self, commitments, z, y, proofs, g2_x, seed=None):
        """bbgpu_host_kzg_check_openings: k claims (C_t, z_t, y_t, pi_t) -> bool, by one pairing product of two pairs; commitments / proofs (k, 8) affine"""
        cs = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
        ps = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8)
        zs, ys = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4), np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 4)
        assert cs.shape[0] == ps.shape[0] == zs.shape[0] == ys.shape[0]
        g2, sd, g2p, sdp, _ = self._srs_check_args(g2_x, seed, False)
        ok = C.c_int(0)
        self.lib.bbgpu_host_kzg_check_openings.argtypes = [u64p, u64p, u64p, u64p, C.c_size_t, u64p, u64p, C.POINTER(C.c_int)]
        self._chk(self.lib.bbgpu_host_kzg_check_openings(_ptr(cs), _ptr(zs), _ptr(ys), _ptr(ps), cs.shape[0], g2p, sdp, C.byref(ok)))
        return ok.value == 1

    def host_lagrange_l1_fft(self, n_src, n_target):
        out = np.zeros((n_target, 4), dtype=np.uint64)
        self.lib.bbgpu_host_lagrange_l1_fft.argtypes = [u64p, C.c_size_t, C.c_size_t]
        self._chk(self.lib.bbgpu_host_lagrange_l1_fft(_ptr(out), n_src, n_target))
        return out

    def host_divide_by_pseudo_vanishing(self, coeffs, n_src, n_target):
        self.lib.bbgpu_host_divide_by_pseudo_vanishing.argtypes = [u64p, C.c_size_t, C.c_size_t]
        self._chk(self.lib.bbgpu_host_divide_by_pseudo_vanishing(_ptr(coeffs), n_src, n_target))
        return coeffs

    # ---- device self-test (known-answer entry points of the field / group layer) ---------------------------------------
    SELFTEST_FIELD_OPS = {"mul": 0, "sqr": 1, "add": 2, "sub": 3, "neg": 4, "mul_add": 5, "mul_sub": 6, "lazy_limbs": 7, "lazy_weak": 8,
                          "lazy_value": 9, "reduce": 10, "sqr_lazy": 11, "zero_tests": 12, "mul_addhi": 13, "sqr_addhi": 14,
                          "wide_mul": 15, "wide_sqr": 16, "wide_mul2": 17, "wide_mul_ip": 18, "wide_mul2_ip": 19, "wide_mul_addhi_ip": 20, "wide_sqr_addhi": 21,
                          "wide_chain": 22}
    SELFTEST_G1_OPS = {"madd": 0, "add": 1, "dbl": 2, "dbl_affine": 3, "madd_neg": 4, "quad_add": 5, "madd_ip": 6, "madd_ip_chain": 7}

    def selftest_field(self, field, op, a, b):
        """field: 'fq' | 'fr'; a, b: (n, 4) uint64 Montgomery operands -> (n, 4) canonical results of the DEVICE arithmetic"""
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros_like(a)
        self.lib.bbgpu_selftest_field.argtypes = [C.c_int, C.c_int, u64p, u64p, C.c_size_t, u64p]
        self._chk(self.lib.bbgpu_selftest_field({"fq": 0, "fr": 1}[field], self.SELFTEST_FIELD_OPS[op], _ptr(a), _ptr(b), a.shape[0], _ptr(out)))
        return out

    def selftest_field_raw(self, field, op, ac, bd):
        """the raw-limb ops ('wide_*'): ac, bd: (cases, 18) uint32 -- the nine limbs of a then c, of b then d (or the addend e) -> (cases, 9) uint32
        result limbs of the device arithmetic"""
        ac = np.ascontiguousarray(ac, dtype=np.uint32).reshape(-1, 18)
        bd = np.ascontiguousarray(bd, dtype=np.uint32).reshape(-1, 18)
        rows = [np.zeros((ac.shape[0], 24), dtype=np.uint32) for _ in range(3)]
        rows[0][:, :18] = ac
        rows[1][:, :18] = bd
        a, b, out = (r.view(np.uint64).reshape(-1, 4) for r in rows)
        self.lib.bbgpu_selftest_field.argtypes = [C.c_int, C.c_int, u64p, u64p, C.c_size_t, u64p]
        self._chk(self.lib.bbgpu_selftest_field({"fq": 0, "fr": 1}[field], self.SELFTEST_FIELD_OPS[op], _ptr(a), _ptr(b), a.shape[0], _ptr(out)))
        return rows[2][:, :9].copy()

    def selftest_g1(self, op, p, q):
        """p, q: (n, 12) uint64 Jacobian -> (n, 16): X, Y, ZZ, ZZZ of the device result"""
        p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 12)
        q = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 12)
        out = np.zeros((p.shape[0], 16), dtype=np.uint64)
        self.lib.bbgpu_selftest_g1.argtypes = [C.c_int, u64p, u64p, C.c_size_t, u64p]
        self._chk(self.lib.bbgpu_selftest_g1(self.SELFTEST_G1_OPS[op], _ptr(p), _ptr(q), p.shape[0], _ptr(out)))
        return out

    # ---- one round kernel of the PLONK prover on its own (bbgpu_selftest_plonk_round) --------------------------------------------------
    SELFTEST_PLONK_KERNELS = {"z_terms": 0, "quot_large": 1, "quot_mid": 2, "quot_seq": 3, "quot_bool": 4, "quot_mimc": 5, "lincomb": 6, "mul2c": 7,
                              "sigma_prepare": 8, "copy_pad": 9, "add_inplace": 10, "divide_vanishing": 11, "scan": 12, "evaluate": 13}

    @staticmethod
    def _plonk_round_out_lens(kernel, length, params):
        """per-lane length of every output of bbgpu_selftest_plonk_round (the `out` column of its table in include/bbgpu.h)"""
        if kernel == "z_terms":
            return [length, length]
        if kernel in ("sigma_prepare", "copy_pad", "add_inplace"):
            return [int(params[0])]
        if kernel == "divide_vanishing":
            return [int(params[1])]
        if kernel == "scan":
            return [length] * bool(int(params[1]) & 4) + [1] * bool(int(params[1]) & 8)
        return [1] if kernel == "evaluate" else [length]

    def selftest_plonk_round(self, kernel, lanes, length, inputs, consts=None, params=()):
        """kernel: a name of SELFTEST_PLONK_KERNELS; inputs: lane-major (lanes * per-lane length, 4) uint64 arrays in the order of the table in
        include/bbgpu.h; consts: (k, 4) canonical Montgomery values, lane-major; params: the kernel's integers -> list of (lanes * per-lane length, 4)
        arrays, canonical.  What the kernel does not support raises BbGpuError (-3)."""
        try:
            out_lens = self._plonk_round_out_lens(kernel, int(length), params)
        except (IndexError, TypeError):
            out_lens = [int(length)]  # too few parameters: the entry refuses the call
        ins = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4) for a in inputs]
        cs = np.ascontiguousarray(consts if consts is not None else np.zeros((0, 4)), dtype=np.uint64).reshape(-1, 4)
        outs = [np.zeros((max(0, int(lanes) * int(n)), 4), dtype=np.uint64) for n in out_lens]
        pr = (C.c_uint32 * max(1, len(params)))(*[int(v) for v in params])
        inp = (u64p * max(1, len(ins)))(*[_ptr(a) for a in ins])
        outp = (u64p * max(1, len(outs)))(*[_ptr(a) for a in outs])
        self.lib.bbgpu_selftest_plonk_round.argtypes = [C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint32), C.c_int, C.POINTER(u64p), C.c_int, u64p,
                                                        C.c_size_t, C.POINTER(u64p), C.c_int]
        self._chk(self.lib.bbgpu_selftest_plonk_round(self.SELFTEST_PLONK_KERNELS.get(kernel, -1), int(lanes), int(length), pr, len(params), inp, len(ins),
                                                      _ptr(cs) if cs.shape[0] else None, cs.shape[0], outp, len(outs)))
        return outs

    # ---- instrumentation ---------------------------------------------------------------------------------------------
    def set_timing(self, on=True):
        """False / 0: off; True / 1: an event after every stage; 2: only the accumulation kernel (light: for timed regions)"""
        self.lib.bbgpu_set_timing(int(on))

    def last_timing(self):
        buf = (C.c_float * 8)()
        k = self.lib.bbgpu_last_timing(buf, 8)
        return [float(buf[i]) for i in range(k)]
