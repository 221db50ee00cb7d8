"""ctypes binding for libsmvp_amd.so (include/smvp_amd.h).

The product is the C-ABI library plus the C command-line program; this module
only exposes that ABI to Python for the tests and for bench.py.  It holds no
compute of its own and there is no fallback: if the library is missing, or no
HIP device is visible, the calls fail.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))          # smvp-toolkit_amd/
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.environ.get("SMVP_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libsmvp_amd.so")   # (the override: A/B of two builds in one gpurun call)
CLI_PATH = os.path.join(PKG_ROOT, "bin", "smvp-toolkit-cli")

OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_ALLOC, ERR_IO, ERR_UNSUPPORTED = 1, 2, 3, 4, 5, 6
MM_COULD_NOT_READ_FILE, MM_PREMATURE_EOF, MM_NOT_MTX, MM_NO_HEADER, MM_UNSUPPORTED_TYPE = 11, 12, 13, 14, 15
CSR_KERNEL_AUTO, CSR_KERNEL_VECTOR, CSR_KERNEL_STREAM, CSR_KERNEL_STREAM_CARRY, CSR_KERNEL_COLSWEEP = 0, 1, 2, 3, 4
CSR_KERNEL_BINNED = 5
CSR_KERNEL_STREAM_PACKED = 6
MEM_HOST, MEM_DEVICE = 0, 1
SYNTH_MEMPLUS_SHAPED, SYNTH_UNIFORM = 1, 2
TJDS_MODE_AUTO, TJDS_MODE_ATOMIC, TJDS_MODE_TWO_PHASE, TJDS_MODE_ROW_GATHER = 0, 1, 2, 3
TIMING_AUTO, TIMING_EVENTS, TIMING_DEVICE, TIMING_DEVICE_GRAPH = 0, 1, 2, 3
MAX_ENTRIES = 2 ** 31 - 1 - 65536   # the most entries a matrix may hold (include/smvp_amd.h): more is ERR_UNSUPPORTED

COO_DTYPE = np.dtype([("row", "<i4"), ("col", "<i4"), ("val", "<f8")], align=True)


def set_option(name, value):
    """smvp_set_option: a plan option for experiments and tests (include/smvp_amd.h); value < 0 or None = the library's default."""
    _check(lib().smvp_set_option(name.encode(), -1 if value is None else int(value)), "smvp_set_option")


def get_option(name):
    v = C.c_int()
    _check(lib().smvp_get_option(name.encode(), C.byref(v)), "smvp_get_option")
    return v.value


class option:
    """with sm.option("csr_col16", 0): ...  -- sets a plan option for the block and restores what was there."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def sweep_parts(rows_per_block, parts, chunks=0):
    """SMVP_CSR_SWEEP_PARTS / SMVP_CSR_SWEEP_PARAM: the column sweep's kernel parameter with 2 or 4 column parts per strip and,
    for experiments, the chunks a wavefront keeps in flight forced to 1, 2 or 4 (include/smvp_amd.h)."""
    return int(rows_per_block) | ({1: 0, 2: 1, 4: 2, 8: 3}[int(parts)] << 24) | ({0: 0, 1: 1, 2: 2, 4: 3}[int(chunks)] << 26)


class TimeStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("time_total", "time_avg", "time_stdev", "time_min", "time_max")]


class RunOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("csr_kernel", C.c_int), ("csr_param", C.c_int),
                ("tjds_ref_quirks", C.c_int), ("convert_on_device", C.c_int), ("ngpus", C.c_int),
                ("iterate", C.c_int), ("normalize", C.c_int), ("tjds_mode", C.c_int), ("timing", C.c_int),
                ("shard_exchange", C.c_int), ("repeat_patience_us", C.c_int), ("x", C.c_void_p)]


class PlanInfo(C.Structure):
    _fields_ = [("matrix_bytes", C.c_double), ("plan_bytes", C.c_double), ("build_ms", C.c_double)]


class RunInfo(C.Structure):
    _fields_ = [("timing", C.c_int), ("graph_replays", C.c_int), ("wall_ms", C.c_double), ("device_clock_khz", C.c_double),
                ("repeat_launches", C.c_int), ("repeat_gave_up", C.c_int)]


class ShardOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("chunks", C.c_int), ("balance", C.c_int), ("exchange", C.c_int)]


class PowerOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("max_steps", C.c_int), ("check_every", C.c_int), ("tol", C.c_double)]


class PowerResult(C.Structure):
    _fields_ = [("steps", C.c_int), ("reason", C.c_int), ("index", C.c_int), ("eigenvalue", C.c_double),
                ("residual", C.c_double), ("scale", C.c_double)]


class CgOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("max_steps", C.c_int), ("check_every", C.c_int), ("tol", C.c_double)]


class CgResult(C.Structure):
    _fields_ = [("steps", C.c_int), ("updates", C.c_int), ("reason", C.c_int), ("pad", C.c_int), ("rr", C.c_double), ("bb", C.c_double)]


class PcgResult(C.Structure):
    _fields_ = [("steps", C.c_int), ("updates", C.c_int), ("reason", C.c_int), ("pad", C.c_int), ("rr", C.c_double), ("rz", C.c_double),
                ("bb", C.c_double)]


class BicgstabOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("max_steps", C.c_int), ("check_every", C.c_int), ("tol", C.c_double)]


class BicgstabResult(C.Structure):
    _fields_ = [("steps", C.c_int), ("full", C.c_int), ("half", C.c_int), ("reason", C.c_int), ("rr", C.c_double), ("bb", C.c_double)]


class GmresOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("max_steps", C.c_int), ("check_every", C.c_int), ("restart", C.c_int), ("tol", C.c_double)]


class GmresResult(C.Structure):
    _fields_ = [("steps", C.c_int), ("cycles", C.c_int), ("columns", C.c_int), ("reason", C.c_int), ("rr", C.c_double), ("bb", C.c_double)]


class LsqrOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("max_steps", C.c_int), ("check_every", C.c_int), ("pad", C.c_int), ("tol", C.c_double),
                ("atol", C.c_double)]


class LsqrResult(C.Structure):
    _fields_ = [("steps", C.c_int), ("updates", C.c_int), ("reason", C.c_int), ("pad", C.c_int), ("rnorm", C.c_double),
                ("arnorm", C.c_double), ("anorm", C.c_double), ("bnorm", C.c_double)]


class TrsvInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("levels", C.c_int), ("max_level_width", C.c_int), ("launches", C.c_int), ("chains", C.c_int),
                ("chain_width", C.c_int), ("missing_diagonals", C.c_int), ("lanes_per_row", C.c_int), ("entries", C.c_longlong),
                ("plan_bytes", C.c_double), ("build_ms", C.c_double)]


class Ilu0Info(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("levels", C.c_int), ("max_level_width", C.c_int), ("launches", C.c_int), ("chains", C.c_int),
                ("chain_width", C.c_int), ("lanes_per_row", C.c_int), ("entries", C.c_longlong), ("pivots", C.c_longlong),
                ("plan_bytes", C.c_double), ("build_ms", C.c_double)]


class ColorOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("seed", C.c_uint), ("max_rounds", C.c_int)]


class ColorInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("colors", C.c_int), ("rounds", C.c_int), ("largest_class", C.c_int),
                ("smallest_class", C.c_int), ("lanes_per_row", C.c_int), ("entries", C.c_longlong), ("build_ms", C.c_double)]


POWER_CONVERGED, POWER_MAX_STEPS, POWER_ZERO, POWER_NONFINITE = 0, 1, 2, 3
TRSV_LOWER, TRSV_UPPER = 0, 1
TRSV_DIAG_STORED, TRSV_DIAG_UNIT = 0, 1
CG_CONVERGED, CG_MAX_STEPS, CG_BREAKDOWN, CG_NONFINITE = 0, 1, 2, 3
BICGSTAB_CONVERGED, BICGSTAB_MAX_STEPS, BICGSTAB_BREAKDOWN, BICGSTAB_NONFINITE = 0, 1, 2, 3
GMRES_CONVERGED, GMRES_MAX_STEPS, GMRES_BREAKDOWN, GMRES_NONFINITE = 0, 1, 2, 3
LSQR_CONVERGED, LSQR_LEAST_SQUARES, LSQR_MAX_STEPS, LSQR_NONFINITE = 0, 1, 2, 3
GATHER_NONE, GATHER_OVERLAPPED, GATHER_AFTER = 0, 1, 2
EXCHANGE_RCCL, EXCHANGE_COPIES, EXCHANGE_DIRECT, EXCHANGE_AUTO = 0, 1, 2, 3
EXCHANGE_NAMES = {EXCHANGE_RCCL: "rccl", EXCHANGE_COPIES: "copies", EXCHANGE_DIRECT: "direct", EXCHANGE_AUTO: "auto"}


class SmvpError(RuntimeError):
    def __init__(self, code, where, msg=None):
        self.code = code
        if msg is None:
            msg = lib().smvp_last_error().decode(errors="replace")
        super().__init__("%s failed with status %d: %s" % (where, code, msg))


def _check_entries(nnz, where):
    """The library's limit on the entries of a matrix, checked before a wrapper allocates outputs for them."""
    if nnz > MAX_ENTRIES:
        raise SmvpError(ERR_UNSUPPORTED, where, "%d entries: more than the %d a matrix may hold" % (nnz, MAX_ENTRIES))


_lib = None

# every symbol include/smvp_amd.h declares; tests check that all of them resolve
EXPORTS = [
    "smvp_last_error", "smvp_version_string", "smvp_set_option", "smvp_get_option",
    "smvp_mm_read_banner", "smvp_mm_read_mtx_crd_size", "smvp_mm_read_coo_entries",
    "smvp_mm_read_header_path", "smvp_mm_read_coo_path", "smvp_mm_expanded_count", "smvp_mm_expand_symmetric",
    "smvp_cache_write_csr", "smvp_cache_read_header", "smvp_cache_read_csr", "smvp_coo_from_csr",
    "smvp_csr_from_coo", "smvp_tjds_from_coo", "smvp_csr_from_coo_device", "smvp_tjds_from_coo_device",
    "smvp_device_count", "smvp_device_info", "smvp_csr_plan_info", "smvp_tjds_plan_info",
    "smvp_csr_create", "smvp_csr_create_block", "smvp_csr_far_share", "smvp_csr_set_kernel", "smvp_csr_get_kernel", "smvp_csr_gather_spread", "smvp_csr_spmv",
    "smvp_csr_describe", "smvp_csr_plan_launches", "smvp_csr_destroy", "smvp_csr_spmm", "smvp_csr_spmm_describe",
    "smvp_csr_create_transposed", "smvp_csr_device_arrays", "smvp_tjds_spmv_transposed", "smvp_tjds_transposed_describe",
    "smvp_tjds_spmm_transposed", "smvp_tjds_spmm_transposed_describe", "smvp_tjds_spmm", "smvp_tjds_spmm_describe",
    "smvp_power_opts_default", "smvp_csr_power_method", "smvp_tjds_power_method",
    "smvp_vector_dot", "smvp_cg_opts_default", "smvp_csr_cg", "smvp_tjds_cg",
    "smvp_csr_diagonal", "smvp_tjds_diagonal", "smvp_csr_pcg", "smvp_tjds_pcg", "smvp_csr_cg_multi", "smvp_tjds_cg_multi",
    "smvp_bicgstab_opts_default", "smvp_csr_bicgstab", "smvp_tjds_bicgstab",
    "smvp_csr_trsv_create", "smvp_trsv_solve", "smvp_trsv_info", "smvp_trsv_schedule", "smvp_trsv_destroy", "smvp_csr_trsv_levels",
    "smvp_csr_trsv_create_sweeps", "smvp_trsv_sweeps",
    "smvp_csr_pcg_tri", "smvp_tjds_pcg_tri",
    "smvp_csr_pbicgstab", "smvp_tjds_pbicgstab",
    "smvp_gmres_opts_default", "smvp_csr_gmres", "smvp_tjds_gmres",
    "smvp_lsqr_opts_default", "smvp_csr_lsqr", "smvp_tjds_lsqr",
    "smvp_csr_ilu0_create", "smvp_ilu0_factor", "smvp_ilu0_matrix", "smvp_ilu0_info", "smvp_ilu0_destroy", "smvp_csr_ilu0_check",
    "smvp_csr_ilu0_host",
    "smvp_color_opts_default", "smvp_csr_color", "smvp_csr_color_host", "smvp_perm_from_classes", "smvp_csr_create_permuted",
    "smvp_vector_gather",
    "smvp_tjds_create", "smvp_tjds_set_x", "smvp_tjds_zero_y", "smvp_tjds_spmv",
    "smvp_tjds_set_ref_quirks", "smvp_tjds_set_mode", "smvp_tjds_set_tile", "smvp_tjds_set_value_cache", "smvp_tjds_get_value_cache", "smvp_tjds_describe", "smvp_tjds_destroy",
    "smvp_shard_opts_default", "smvp_csr_sharded_create", "smvp_csr_sharded_create_ex", "smvp_tjds_sharded_create",
    "smvp_tjds_sharded_create_ex", "smvp_sharded_layout", "smvp_sharded_set_csr_kernel", "smvp_sharded_probe_exchange", "smvp_sharded_exchange_info", "smvp_sharded_set_exchange", "smvp_sharded_set_x", "smvp_sharded_spmv",
    "smvp_sharded_synchronize", "smvp_sharded_feed_back", "smvp_sharded_get_y", "smvp_sharded_info", "smvp_sharded_destroy",
    "smvp_run_opts_default", "smvp_csr_compute", "smvp_tjds_compute", "smvp_last_run_info",
    "smvp_time_stats", "smvp_generate_report_text", "smvp_cisr_coegen", "smvp_cisr_coegen_path",
    "smvp_synth_row_lengths", "smvp_synth_fill", "smvp_partition_rows", "smvp_vector_random",
]


def lib():
    """The loaded library.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C smvp-toolkit_amd` first" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.smvp_last_error.restype = C.c_char_p
        L.smvp_version_string.restype = C.c_char_p
        L.smvp_set_option.argtypes = [C.c_char_p, C.c_int]
        L.smvp_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        vp, ci = C.c_void_p, C.c_int
        L.smvp_csr_create.argtypes = [C.POINTER(vp), ci, ci, ci, ci, vp, vp, vp, ci, vp]
        L.smvp_csr_create_block.argtypes = [C.POINTER(vp), ci, ci, ci, ci, vp, vp, vp, ci, vp, C.c_longlong]
        L.smvp_csr_far_share.argtypes = [vp, C.POINTER(C.c_double)]
        L.smvp_csr_set_kernel.argtypes = [vp, ci, ci]
        L.smvp_csr_get_kernel.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
        L.smvp_csr_gather_spread.argtypes = [vp, C.POINTER(C.c_double)]
        L.smvp_csr_spmv.argtypes = [vp, vp, vp, vp]
        L.smvp_csr_describe.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]
        L.smvp_csr_plan_launches.argtypes = [vp, C.POINTER(ci)]
        L.smvp_csr_plan_info.argtypes = [vp, C.POINTER(PlanInfo)]
        L.smvp_tjds_plan_info.argtypes = [vp, C.POINTER(PlanInfo)]
        L.smvp_csr_destroy.argtypes = [vp]
        L.smvp_csr_destroy.restype = None
        L.smvp_csr_spmm.argtypes = [vp, ci, vp, C.c_longlong, vp, C.c_longlong, vp]
        L.smvp_csr_spmm_describe.argtypes = [vp, ci, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(PlanInfo)]
        L.smvp_csr_create_transposed.argtypes = [C.POINTER(vp), vp, vp]
        L.smvp_csr_device_arrays.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.smvp_tjds_spmv_transposed.argtypes = [vp, vp, vp, vp]
        L.smvp_tjds_transposed_describe.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]
        L.smvp_tjds_spmm_transposed.argtypes = [vp, ci, vp, C.c_longlong, vp, C.c_longlong, vp]
        L.smvp_tjds_spmm_transposed_describe.argtypes = [vp, ci, C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]
        L.smvp_tjds_spmm.argtypes = [vp, ci, vp, C.c_longlong, vp, C.c_longlong, vp]
        L.smvp_tjds_spmm_describe.argtypes = [vp, ci, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(PlanInfo)]
        L.smvp_power_opts_default.argtypes = [C.POINTER(PowerOpts)]
        L.smvp_power_opts_default.restype = None
        L.smvp_csr_power_method.argtypes = [vp, C.POINTER(PowerOpts), vp, vp, C.POINTER(PowerResult), vp, vp, vp]
        L.smvp_tjds_power_method.argtypes = [vp, C.POINTER(PowerOpts), vp, vp, C.POINTER(PowerResult), vp, vp, vp]
        L.smvp_vector_dot.argtypes = [ci, ci, vp, vp, C.POINTER(C.c_double), vp]
        L.smvp_cg_opts_default.argtypes = [C.POINTER(CgOpts)]
        L.smvp_cg_opts_default.restype = None
        L.smvp_csr_cg.argtypes = [vp, C.POINTER(CgOpts), vp, vp, vp, C.POINTER(CgResult), vp, vp, vp]
        L.smvp_tjds_cg.argtypes = [vp, C.POINTER(CgOpts), vp, vp, vp, C.POINTER(CgResult), vp, vp, vp]
        L.smvp_csr_diagonal.argtypes = [vp, vp, vp]
        L.smvp_tjds_diagonal.argtypes = [vp, vp, vp]
        L.smvp_csr_pcg.argtypes = [vp, C.POINTER(CgOpts), vp, vp, vp, vp, C.POINTER(PcgResult), vp, vp, vp, vp]
        L.smvp_tjds_pcg.argtypes = [vp, C.POINTER(CgOpts), vp, vp, vp, vp, C.POINTER(PcgResult), vp, vp, vp, vp]
        ll = C.c_longlong
        L.smvp_csr_cg_multi.argtypes = [vp, C.POINTER(CgOpts), ci, vp, ll, vp, ll, vp, ll, vp, C.POINTER(PcgResult), vp, vp, vp, vp]
        L.smvp_tjds_cg_multi.argtypes = [vp, C.POINTER(CgOpts), ci, vp, ll, vp, ll, vp, ll, vp, C.POINTER(PcgResult), vp, vp, vp, vp]
        L.smvp_bicgstab_opts_default.argtypes = [C.POINTER(BicgstabOpts)]
        L.smvp_bicgstab_opts_default.restype = None
        L.smvp_csr_bicgstab.argtypes = [vp, C.POINTER(BicgstabOpts), vp, vp, vp, C.POINTER(BicgstabResult), vp, vp, vp]
        L.smvp_tjds_bicgstab.argtypes = [vp, C.POINTER(BicgstabOpts), vp, vp, vp, C.POINTER(BicgstabResult), vp, vp, vp]
        L.smvp_csr_trsv_create.argtypes = [C.POINTER(vp), vp, ci, ci, vp]
        L.smvp_trsv_solve.argtypes = [vp, vp, vp, vp]
        L.smvp_trsv_info.argtypes = [vp, C.POINTER(TrsvInfo)]
        L.smvp_trsv_schedule.argtypes = [vp, vp, vp]
        L.smvp_trsv_destroy.argtypes = [vp]
        L.smvp_trsv_destroy.restype = None
        L.smvp_csr_trsv_levels.argtypes = [ci, vp, vp, ci, vp, C.POINTER(ci)]
        L.smvp_csr_trsv_create_sweeps.argtypes = [C.POINTER(vp), vp, ci, ci, ci, vp]
        L.smvp_trsv_sweeps.argtypes = [vp, C.POINTER(ci)]
        L.smvp_csr_pcg_tri.argtypes = [vp, C.POINTER(CgOpts), vp, vp, vp, vp, vp, vp, C.POINTER(PcgResult), vp, vp, vp, vp]
        L.smvp_tjds_pcg_tri.argtypes = [vp, C.POINTER(CgOpts), vp, vp, vp, vp, vp, vp, C.POINTER(PcgResult), vp, vp, vp, vp]
        L.smvp_csr_pbicgstab.argtypes = [vp, C.POINTER(BicgstabOpts), vp, vp, vp, vp, vp, vp, C.POINTER(BicgstabResult), vp, vp, vp]
        L.smvp_tjds_pbicgstab.argtypes = [vp, C.POINTER(BicgstabOpts), vp, vp, vp, vp, vp, vp, C.POINTER(BicgstabResult), vp, vp, vp]
        L.smvp_gmres_opts_default.argtypes = [C.POINTER(GmresOpts)]
        L.smvp_gmres_opts_default.restype = None
        L.smvp_csr_gmres.argtypes = [vp, C.POINTER(GmresOpts), vp, vp, vp, vp, vp, vp, C.POINTER(GmresResult), vp, vp, vp]
        L.smvp_tjds_gmres.argtypes = [vp, C.POINTER(GmresOpts), vp, vp, vp, vp, vp, vp, C.POINTER(GmresResult), vp, vp, vp]
        L.smvp_lsqr_opts_default.argtypes = [C.POINTER(LsqrOpts)]
        L.smvp_lsqr_opts_default.restype = None
        L.smvp_csr_lsqr.argtypes = [vp, vp, C.POINTER(LsqrOpts), vp, vp, vp, C.POINTER(LsqrResult), vp, vp, vp]
        L.smvp_tjds_lsqr.argtypes = [vp, C.POINTER(LsqrOpts), vp, vp, vp, C.POINTER(LsqrResult), vp, vp, vp]
        L.smvp_csr_ilu0_create.argtypes = [C.POINTER(vp), vp, vp]
        L.smvp_ilu0_factor.argtypes = [vp, vp]
        L.smvp_ilu0_matrix.argtypes = [vp, C.POINTER(vp)]
        L.smvp_ilu0_info.argtypes = [vp, C.POINTER(Ilu0Info)]
        L.smvp_ilu0_destroy.argtypes = [vp]
        L.smvp_ilu0_destroy.restype = None
        L.smvp_csr_ilu0_check.argtypes = [ci, vp, vp, vp, C.POINTER(ci)]
        L.smvp_csr_ilu0_host.argtypes = [ci, vp, vp, vp, vp]
        L.smvp_color_opts_default.argtypes = [C.POINTER(ColorOpts)]
        L.smvp_color_opts_default.restype = None
        L.smvp_csr_color.argtypes = [vp, vp, C.POINTER(ColorOpts), vp, C.POINTER(ColorInfo), vp]
        L.smvp_csr_color_host.argtypes = [ci, vp, vp, vp, vp, C.c_uint, vp, C.POINTER(ci), C.POINTER(ci)]
        L.smvp_perm_from_classes.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp]
        L.smvp_csr_create_permuted.argtypes = [C.POINTER(vp), vp, vp, vp]
        L.smvp_vector_gather.argtypes = [ci, ci, vp, vp, vp, vp]
        L.smvp_tjds_create.argtypes = [C.POINTER(vp), ci, ci, ci, ci, ci, vp, vp, vp, vp, ci]
        L.smvp_tjds_set_x.argtypes = [vp, vp, vp]
        L.smvp_tjds_zero_y.argtypes = [vp, vp, vp]
        L.smvp_tjds_spmv.argtypes = [vp, vp, vp]
        L.smvp_tjds_set_ref_quirks.argtypes = [vp, ci, ci, ci]
        L.smvp_tjds_set_mode.argtypes = [vp, ci]
        L.smvp_tjds_set_tile.argtypes = [vp, ci]
        L.smvp_tjds_set_value_cache.argtypes = [vp, ci]
        L.smvp_tjds_get_value_cache.argtypes = [vp, C.POINTER(ci), C.POINTER(C.c_longlong)]
        L.smvp_last_run_info.argtypes = [C.POINTER(RunInfo)]
        L.smvp_tjds_describe.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]
        L.smvp_tjds_destroy.argtypes = [vp]
        L.smvp_tjds_destroy.restype = None
        L.smvp_csr_from_coo.argtypes = [vp, ci, ci, vp, vp, vp]
        L.smvp_tjds_from_coo.argtypes = [vp, ci, ci, ci, vp, vp, ci, vp, vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.smvp_csr_sharded_create.argtypes = [C.POINTER(vp), ci, vp, ci, ci, ci, vp, vp, vp]
        L.smvp_tjds_sharded_create.argtypes = [C.POINTER(vp), ci, vp, vp, ci, ci, ci]
        L.smvp_csr_sharded_create_ex.argtypes = [C.POINTER(vp), ci, vp, ci, ci, ci, vp, vp, vp, C.POINTER(ShardOpts)]
        L.smvp_tjds_sharded_create_ex.argtypes = [C.POINTER(vp), ci, vp, vp, ci, ci, ci, C.POINTER(ShardOpts)]
        L.smvp_shard_opts_default.argtypes = [C.POINTER(ShardOpts)]
        L.smvp_shard_opts_default.restype = None
        L.smvp_sharded_layout.argtypes = [vp, C.POINTER(ci), vp, vp]
        L.smvp_sharded_set_csr_kernel.argtypes = [vp, ci, ci]
        L.smvp_sharded_probe_exchange.argtypes = [vp, ci]
        L.smvp_sharded_exchange_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), vp, C.POINTER(ci)]
        L.smvp_sharded_set_exchange.argtypes = [vp, ci]
        L.smvp_sharded_set_x.argtypes = [vp, vp]
        L.smvp_sharded_spmv.argtypes = [vp, ci, ci]
        L.smvp_sharded_synchronize.argtypes = [vp, C.POINTER(C.c_double)]
        L.smvp_sharded_get_y.argtypes = [vp, ci, ci, vp]
        L.smvp_sharded_feed_back.argtypes = [vp, ci]
        L.smvp_sharded_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
        L.smvp_sharded_destroy.argtypes = [vp]
        L.smvp_sharded_destroy.restype = None
        L.smvp_csr_from_coo_device.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp]
        L.smvp_tjds_from_coo_device.argtypes = [vp, ci, ci, ci, vp, vp, ci, vp, vp, C.POINTER(ci), C.POINTER(ci),
                                                C.POINTER(ci), vp]
        L.smvp_csr_compute.argtypes = [vp, ci, ci, ci, ci, C.POINTER(RunOpts), vp, vp, C.POINTER(TimeStats)]
        L.smvp_tjds_compute.argtypes = [vp, ci, ci, ci, ci, C.POINTER(RunOpts), vp, vp, C.POINTER(TimeStats)]
        L.smvp_run_opts_default.argtypes = [C.POINTER(RunOpts)]
        L.smvp_run_opts_default.restype = None
        L.smvp_time_stats.argtypes = [vp, ci, C.POINTER(TimeStats)]
        L.smvp_generate_report_text.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, ci, ci, ci, vp,
                                                C.POINTER(TimeStats), C.c_ulong, C.c_char_p, C.c_size_t]
        i64, u64 = C.c_int64, C.c_uint64
        L.smvp_synth_row_lengths.argtypes = [ci, u64, i64, i64, ci, i64, i64, vp]
        L.smvp_synth_fill.argtypes = [ci, u64, i64, i64, ci, i64, i64, vp, vp, vp, ci]
        L.smvp_partition_rows.argtypes = [vp, ci, ci, vp]
        L.smvp_vector_random.argtypes = [vp, C.c_int64, C.c_uint64]
        L.smvp_mm_read_header_path.argtypes = [C.c_char_p, vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.smvp_mm_read_coo_path.argtypes = [C.c_char_p, vp, ci, vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.smvp_mm_expanded_count.argtypes = [vp, vp, ci, C.POINTER(ci)]
        L.smvp_mm_expand_symmetric.argtypes = [vp, vp, ci, ci, ci, vp, ci, C.POINTER(ci)]
        L.smvp_cache_write_csr.argtypes = [C.c_char_p, C.c_char_p, vp, ci, ci, ci, ci, vp, vp, vp]
        L.smvp_cache_read_header.argtypes = [C.c_char_p, C.c_char_p, vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.smvp_cache_read_csr.argtypes = [C.c_char_p, ci, ci, vp, vp, vp]
        L.smvp_coo_from_csr.argtypes = [ci, vp, vp, vp, vp]
        L.smvp_cisr_coegen_path.argtypes = [vp, ci, ci, ci, C.c_char_p]
        L.smvp_device_count.argtypes = [C.POINTER(ci)]
        L.smvp_device_info.argtypes = [ci, C.c_char_p, C.c_size_t, C.POINTER(ci), C.POINTER(C.c_size_t)]
        _lib = L
    return _lib


def _check(code, where):
    if code != OK:
        raise SmvpError(code, where)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _arr(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if a.size else np.zeros(1, dtype=dtype)


# ---------------------------------------------------------------- Matrix Market
def mm_read_header(path):
    """-> (status, typecode str, rows, cols, nnz); status is an mmio code, not raised."""
    tc = C.create_string_buffer(4)
    m, n, nz = C.c_int(), C.c_int(), C.c_int()
    rc = lib().smvp_mm_read_header_path(os.fsencode(path), C.cast(tc, C.c_void_p), C.byref(m), C.byref(n), C.byref(nz))
    return rc, tc.raw.decode(), m.value, n.value, nz.value


def mm_read_coo(path):
    """-> (typecode, rows, cols, coo structured array).  Raises SmvpError on a bad file."""
    rc, tc, m, n, nz = mm_read_header(path)
    _check(rc, "smvp_mm_read_header_path")
    coo = np.zeros(max(nz, 1), dtype=COO_DTYPE)
    tcb = C.create_string_buffer(4)
    mm, nn, nzz = C.c_int(), C.c_int(), C.c_int()
    _check(lib().smvp_mm_read_coo_path(os.fsencode(path), _p(coo), nz, C.cast(tcb, C.c_void_p), C.byref(mm),
                                       C.byref(nn), C.byref(nzz)), "smvp_mm_read_coo_path")
    return tcb.raw.decode(), mm.value, nn.value, coo[:nz]


def mm_expand_symmetric(typecode, coo, rows, cols):
    """Mirror the off-diagonal entries of symmetric / skew-symmetric storage (NOT the reference's behaviour) -> coo."""
    nnz = len(coo)
    coo = _arr(coo, COO_DTYPE)
    tc = C.create_string_buffer(typecode.encode()[:4].ljust(4), 4)
    want = C.c_int()
    _check(lib().smvp_mm_expanded_count(C.cast(tc, C.c_void_p), _p(coo), nnz, C.byref(want)), "smvp_mm_expanded_count")
    out = np.zeros(max(want.value, 1), dtype=COO_DTYPE)
    got = C.c_int()
    _check(lib().smvp_mm_expand_symmetric(C.cast(tc, C.c_void_p), _p(coo), nnz, rows, cols, _p(out), want.value,
                                          C.byref(got)), "smvp_mm_expand_symmetric")
    return out[:got.value]


def cache_write_csr(cache_path, mtx_path, typecode, rows, cols, row_ptr, col_ind, val, expanded=False):
    rp, ci, v = _arr(row_ptr, np.int32), _arr(col_ind, np.int32), _arr(val, np.float64)
    tc = C.create_string_buffer(typecode.encode()[:4].ljust(4), 4)
    _check(lib().smvp_cache_write_csr(os.fsencode(cache_path), os.fsencode(mtx_path), C.cast(tc, C.c_void_p), int(expanded),
                                      rows, cols, int(rp[rows]), _p(rp), _p(ci), _p(v)), "smvp_cache_write_csr")


def cache_read_csr(cache_path, mtx_path=None):
    """-> (typecode, expanded, rows, cols, row_ptr, col_ind, val); raises SmvpError (ERR_IO: no cache, ERR_INVALID: stale)."""
    tc = C.create_string_buffer(4)
    fl, m, n, nz = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _check(lib().smvp_cache_read_header(os.fsencode(cache_path), None if mtx_path is None else os.fsencode(mtx_path),
                                        C.cast(tc, C.c_void_p), C.byref(fl), C.byref(m), C.byref(n), C.byref(nz)),
           "smvp_cache_read_header")
    rp = np.zeros(m.value + 1, dtype=np.int32)
    ci = np.zeros(max(nz.value, 1), dtype=np.int32)
    v = np.zeros(max(nz.value, 1), dtype=np.float64)
    _check(lib().smvp_cache_read_csr(os.fsencode(cache_path), m.value, nz.value, _p(rp), _p(ci), _p(v)), "smvp_cache_read_csr")
    return tc.raw.decode(), bool(fl.value & 1), m.value, n.value, rp, ci[:nz.value], v[:nz.value]


def coo_from_csr(rows, row_ptr, col_ind, val):
    rp, ci, v = _arr(row_ptr, np.int32), _arr(col_ind, np.int32), _arr(val, np.float64)
    out = np.zeros(max(int(rp[rows]), 1), dtype=COO_DTYPE)
    _check(lib().smvp_coo_from_csr(rows, _p(rp), _p(ci), _p(v), _p(out)), "smvp_coo_from_csr")
    return out[:int(rp[rows])]


def cisr_coegen(coo, rows, slots, path):
    """CISR .coe file of the matrix (smvp_cisr_coegen_path); raises SmvpError (ERR_UNSUPPORTED: the reference's overrun exit)."""
    n = len(coo)
    _check(lib().smvp_cisr_coegen_path(_p(_arr(coo, COO_DTYPE)), rows, n, slots, os.fsencode(path)), "smvp_cisr_coegen_path")
    return open(path).read()


def make_coo(rows_idx, cols_idx, vals):
    coo = np.zeros(len(rows_idx), dtype=COO_DTYPE)
    coo["row"], coo["col"], coo["val"] = rows_idx, cols_idx, vals
    return coo


# ------------------------------------------------------------------ conversion
def csr_from_coo(coo, rows):
    coo = np.ascontiguousarray(coo, dtype=COO_DTYPE)
    nnz = len(coo)
    row_ptr = np.zeros(rows + 1, dtype=np.int32)
    col_ind = np.zeros(max(nnz, 1), dtype=np.int32)
    val = np.zeros(max(nnz, 1), dtype=np.float64)
    _check(lib().smvp_csr_from_coo(_p(_arr(coo, COO_DTYPE)), rows, nnz, _p(row_ptr), _p(col_ind), _p(val)),
           "smvp_csr_from_coo")
    return row_ptr, col_ind[:nnz], val[:nnz]


class TjdsArrays:
    """perm / start_pos / row_ind / val plus the two reference-quirk scalars."""


def tjds_from_coo(coo, rows, cols):
    coo = np.ascontiguousarray(coo, dtype=COO_DTYPE)
    nnz = len(coo)
    t = TjdsArrays()
    t.rows, t.cols, t.nnz = rows, cols, nnz
    perm = np.zeros(max(cols, 1), dtype=np.int32)
    cap = max(rows, nnz) + 2
    sp = np.zeros(cap, dtype=np.int32)
    row_ind = np.zeros(max(nnz, 1), dtype=np.int32)
    val = np.zeros(max(nnz, 1), dtype=np.float64)
    nd, rn, ls = C.c_int(), C.c_int(), C.c_int()
    _check(lib().smvp_tjds_from_coo(_p(_arr(coo, COO_DTYPE)), rows, cols, nnz, _p(perm), _p(sp), cap, _p(row_ind),
                                    _p(val), C.byref(nd), C.byref(rn), C.byref(ls)), "smvp_tjds_from_coo")
    t.num_diag, t.ref_num_tjdiag, t.last_diag_single = nd.value, rn.value, ls.value
    t.perm, t.start_pos = perm[:cols], sp[:t.num_diag + 1].copy()
    t.row_ind, t.val = row_ind[:nnz], val[:nnz]
    return t


def csr_from_coo_device(d_coo, rows, cols, nnz, stream=None):
    """COO -> CSR on the GPU.  d_coo: torch uint8 CUDA tensor holding nnz smvp_coo_t (16 B each).
    Returns (row_ptr, col_ind, val) as torch CUDA tensors."""
    import torch

    _check_entries(nnz, "smvp_csr_from_coo_device")

    row_ptr = torch.empty(rows + 1, dtype=torch.int32, device=d_coo.device)
    col_ind = torch.empty(max(nnz, 1), dtype=torch.int32, device=d_coo.device)
    val = torch.empty(max(nnz, 1), dtype=torch.float64, device=d_coo.device)
    _check(lib().smvp_csr_from_coo_device(_dev_ptr(d_coo), rows, cols, nnz, _dev_ptr(row_ptr), _dev_ptr(col_ind),
                                          _dev_ptr(val), _stream_ptr(stream)), "smvp_csr_from_coo_device")
    return row_ptr, col_ind[:nnz], val[:nnz]


def tjds_from_coo_device(d_coo, rows, cols, nnz, stream=None):
    """COO -> TJDS on the GPU -> TjdsArrays whose arrays are torch CUDA tensors."""
    import torch

    _check_entries(nnz, "smvp_tjds_from_coo_device")

    t = TjdsArrays()
    t.rows, t.cols, t.nnz = rows, cols, nnz
    cap = max(rows, nnz) + 2
    perm = torch.empty(max(cols, 1), dtype=torch.int32, device=d_coo.device)
    sp = torch.empty(cap, dtype=torch.int32, device=d_coo.device)
    row_ind = torch.empty(max(nnz, 1), dtype=torch.int32, device=d_coo.device)
    val = torch.empty(max(nnz, 1), dtype=torch.float64, device=d_coo.device)
    nd, rn, ls = C.c_int(), C.c_int(), C.c_int()
    _check(lib().smvp_tjds_from_coo_device(_dev_ptr(d_coo), rows, cols, nnz, _dev_ptr(perm), _dev_ptr(sp), cap,
                                           _dev_ptr(row_ind), _dev_ptr(val), C.byref(nd), C.byref(rn), C.byref(ls),
                                           _stream_ptr(stream)), "smvp_tjds_from_coo_device")
    t.num_diag, t.ref_num_tjdiag, t.last_diag_single = nd.value, rn.value, ls.value
    t.perm, t.start_pos = perm[:cols], sp[:t.num_diag + 1]
    t.row_ind, t.val = row_ind[:nnz], val[:nnz]
    return t


def partition_rows(row_ptr, parts):
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
    bounds = np.zeros(parts + 1, dtype=np.int32)
    _check(lib().smvp_partition_rows(_p(row_ptr), len(row_ptr) - 1, parts, _p(bounds)), "smvp_partition_rows")
    return bounds


def vector_random(n, seed=67890):
    """The operand of `--x random`: uniform [0, 1), a pure function of (seed, index)."""
    x = np.zeros(max(n, 1), dtype=np.float64)
    _check(lib().smvp_vector_random(_p(x), n, seed), "smvp_vector_random")
    return x[:n]


# ------------------------------------------------------------------- synthetic
def synth_csr(kind, seed, rows_total, cols_total, param=0, row_begin=0, row_end=None, threads=None):
    """Row block [row_begin, row_end) of a synthetic matrix -> (row_ptr, col_ind, val), local row numbering."""
    row_end = rows_total if row_end is None else row_end
    n = row_end - row_begin
    lens = np.zeros(max(n, 1), dtype=np.int32)
    _check(lib().smvp_synth_row_lengths(kind, seed, rows_total, cols_total, param, row_begin, row_end, _p(lens)),
           "smvp_synth_row_lengths")
    row_ptr64 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens[:n], out=row_ptr64[1:])
    if row_ptr64[-1] >= 2 ** 31:
        raise ValueError("row block holds %d entries: 32-bit indices (the reference's) cannot address it" % row_ptr64[-1])
    row_ptr = row_ptr64.astype(np.int32)
    nnz = int(row_ptr[-1])
    col_ind = np.empty(max(nnz, 1), dtype=np.int32)
    val = np.empty(max(nnz, 1), dtype=np.float64)
    if threads is None:
        threads = max(1, min(16, (os.cpu_count() or 1)))
    _check(lib().smvp_synth_fill(kind, seed, rows_total, cols_total, param, row_begin, row_end, _p(row_ptr),
                                 _p(col_ind), _p(val), threads), "smvp_synth_fill")
    return row_ptr, col_ind[:nnz], val[:nnz]


# ---------------------------------------------------------------------- device
def device_count():
    n = C.c_int()
    _check(lib().smvp_device_count(C.byref(n)), "smvp_device_count")
    return n.value


def device_info(device=0):
    name = C.create_string_buffer(256)
    cus, mem = C.c_int(), C.c_size_t()
    _check(lib().smvp_device_info(device, name, 256, C.byref(cus), C.byref(mem)), "smvp_device_info")
    return name.value.decode(), cus.value, mem.value


def _dev_ptr(t):
    """Device address of a torch tensor (or a raw int address)."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def _stream_ptr(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)   # torch.cuda.Stream


def spmm_operands(X, Y, rows, cols):
    """(k, ldx, ldy) of the operands of CsrMatrix.spmm: X of shape (cols, k) and Y of shape (rows, k), float64 tensors whose
    rows are contiguous (stride(1) == 1; the leading dimension is stride(0) >= k).  Raises ValueError otherwise.  Checks
    shapes and strides only, so it runs on CPU tensors too."""
    for name, t, n in (("X", X, cols), ("Y", Y, rows)):
        if not hasattr(t, "stride") or not hasattr(t, "dim") or t.dim() != 2:
            raise ValueError("%s must be a 2-D tensor" % name)
        if str(t.dtype) != "torch.float64":
            raise ValueError("%s must be float64, not %s" % (name, t.dtype))
        if t.shape[0] != n:
            raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.shape[0], n))
    k = X.shape[1]
    if k < 1 or Y.shape[1] != k:
        raise ValueError("X and Y need the same number of columns k >= 1 (X has %d, Y %d)" % (X.shape[1], Y.shape[1]))
    for name, t in (("X", X), ("Y", Y)):
        if t.stride(1) != 1 or t.stride(0) < k:
            raise ValueError("%s must be row-major with contiguous rows (stride(1) == 1, stride(0) >= k); its strides are %s"
                             % (name, tuple(t.stride())))
    return k, X.stride(0), Y.stride(0)


def _spmm(fn, handle, X, Y, out_rows, in_rows, stream):
    """smvp_csr_spmm / smvp_tjds_spmm / smvp_tjds_spmm_transposed: X of in_rows and Y of out_rows rows, checked by spmm_operands."""
    k, ldx, ldy = spmm_operands(X, Y, out_rows, in_rows)
    if not (X.is_cuda and Y.is_cuda):
        raise ValueError("X and Y must be device tensors")
    _check(getattr(lib(), fn)(handle, k, _dev_ptr(X), ldx, _dev_ptr(Y), ldy, _stream_ptr(stream)), fn)


def _spmm_describe(fn, handle, k, with_plan):
    """The describe call of a block product -> (kernel symbols, algorithmic bytes for k vectors) and, with_plan, {plan_bytes,
    build_ms} of its plan."""
    name, b, i = C.create_string_buffer(256), C.c_double(), PlanInfo()
    _check(getattr(lib(), fn)(handle, k, name, 256, C.byref(b), *([C.byref(i)] if with_plan else [])), fn)
    plan = ({"plan_bytes": i.plan_bytes, "build_ms": i.build_ms},) if with_plan else ()
    return (name.value.decode(), b.value) + plan


def transposed_operands(x, y, rows, cols):
    """Checks the operands of TjdsMatrix.spmv_transposed: x of `rows` and y of `cols` float64 elements, contiguous tensors.
    Raises ValueError otherwise.  Checks dtype, size and strides only, so it runs on CPU tensors too."""
    for name, t, n in (("x", x, rows), ("y", y, cols)):
        if not hasattr(t, "is_contiguous") or not hasattr(t, "numel"):
            raise ValueError("%s must be a tensor" % name)
        if str(t.dtype) != "torch.float64":
            raise ValueError("%s must be float64, not %s" % (name, t.dtype))
        if t.numel() != n:
            raise ValueError("%s has %d elements, the matrix needs %d" % (name, t.numel(), n))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous; its strides are %s" % (name, tuple(t.stride())))


def power_opts(max_steps, tol=0.0, check_every=1):
    """smvp_power_opts_t from smvp_power_opts_default with the three fields set."""
    o = PowerOpts()
    lib().smvp_power_opts_default(C.byref(o))
    o.max_steps, o.check_every, o.tol = int(max_steps), int(check_every), float(tol)
    return o


def _power_method(fn, handle, x0, x, max_steps, tol, check_every, stream):
    """smvp_csr_power_method / smvp_tjds_power_method -> (PowerResult, lambda_each, residual_each), the histories cut to the
    steps done."""
    o = power_opts(max_steps, tol, check_every)
    r = PowerResult()
    lam, res = np.zeros(max(int(max_steps), 1)), np.zeros(max(int(max_steps), 1))
    _check(getattr(lib(), fn)(handle, C.byref(o), _dev_ptr(x0), _dev_ptr(x), C.byref(r), _p(lam), _p(res), _stream_ptr(stream)), fn)
    return r, lam[:r.steps], res[:r.steps]


def cg_opts(max_steps=100, tol=1e-10, check_every=10):
    """smvp_cg_opts_t from smvp_cg_opts_default with the three fields set."""
    o = CgOpts()
    lib().smvp_cg_opts_default(C.byref(o))
    o.max_steps, o.check_every, o.tol = int(max_steps), int(check_every), float(tol)
    return o


def _device_vectors(**named):
    """Raises ValueError for a tensor that is not on the device (None passes): its address would mean nothing there."""
    for name, t in named.items():
        if t is not None and not isinstance(t, int) and not t.is_cuda:
            raise ValueError("%s must be a device tensor" % name)


def vector_dot(a, b, stream=None):
    """dot(a, b) of two float64 CUDA tensors of equal length in the order of additions include/smvp_amd.h defines
    (smvp_vector_dot): one right answer, bit for bit.  Returns a numpy float64 after the work on `stream` has finished."""
    _device_vectors(a=a, b=b)
    if a.numel() != b.numel() or a.numel() > 2 ** 31 - 1:
        raise ValueError("a has %d elements, b has %d (need the same number, an int's at the most)" % (a.numel(), b.numel()))
    out = C.c_double()
    _check(lib().smvp_vector_dot(a.device.index or 0, a.numel(), _dev_ptr(a), _dev_ptr(b), C.byref(out), _stream_ptr(stream)),
           "smvp_vector_dot")
    return np.float64(out.value)


def _cg(fn, handle, b, x, x0, max_steps, tol, check_every, stream):
    """smvp_csr_cg / smvp_tjds_cg -> (CgResult, rr_each, sigma_each), the histories cut to the filled elements."""
    _device_vectors(b=b, x=x, x0=x0)
    o = cg_opts(max_steps, tol, check_every)
    r = CgResult()
    rr, sigma = np.zeros(max(int(max_steps), 0) + 1), np.zeros(max(int(max_steps), 1))
    _check(getattr(lib(), fn)(handle, C.byref(o), _dev_ptr(b), _dev_ptr(x0), _dev_ptr(x), C.byref(r), _p(rr), _p(sigma),
                              _stream_ptr(stream)), fn)
    return r, rr[:r.updates + 1], sigma[:r.steps]


def _diagonal(fn, handle, rows, out, stream):
    """smvp_csr_diagonal / smvp_tjds_diagonal into `out`, a contiguous float64 CUDA tensor of `rows` elements."""
    _device_vectors(out=out)
    if str(out.dtype) != "torch.float64" or out.numel() != rows or not out.is_contiguous():
        raise ValueError("out must be a contiguous float64 tensor of %d elements (it has %d of %s)" % (rows, out.numel(), out.dtype))
    _check(getattr(lib(), fn)(handle, _dev_ptr(out), _stream_ptr(stream)), fn)
    return out


def _pcg(fn, handle, b, x, m, x0, max_steps, tol, check_every, stream):
    """smvp_csr_pcg / smvp_tjds_pcg -> (PcgResult, rr_each, rz_each, sigma_each), the histories cut to the filled elements."""
    _device_vectors(b=b, x=x, m=m, x0=x0)
    o = cg_opts(max_steps, tol, check_every)
    r = PcgResult()
    rr, rz, sigma = np.zeros(max(int(max_steps), 0) + 1), np.zeros(max(int(max_steps), 0) + 1), np.zeros(max(int(max_steps), 1))
    _check(getattr(lib(), fn)(handle, C.byref(o), _dev_ptr(b), _dev_ptr(x0), _dev_ptr(x), _dev_ptr(m), C.byref(r), _p(rr), _p(rz),
                              _p(sigma), _stream_ptr(stream)), fn)
    return r, rr[:r.updates + 1], rz[:r.updates + 1], sigma[:r.steps]


def cg_multi_operands(B, X, X0, m, n):
    """(k, ldb, ldx, ldx0) of the operands of CsrMatrix.cg_multi: B, X and X0 (or None) float64 tensors of shape (n, k) whose rows are
    contiguous (stride(1) == 1; the leading dimension is stride(0) >= k), m (or None) a contiguous float64 tensor of n elements.
    Raises ValueError otherwise.  Checks shapes, dtypes and strides only, so it runs on CPU tensors too."""
    named = [("B", B), ("X", X)] + ([("X0", X0)] if X0 is not None else [])
    for name, t in named:
        if not hasattr(t, "stride") or not hasattr(t, "dim") or t.dim() != 2:
            raise ValueError("%s must be a 2-D tensor" % name)
        if str(t.dtype) != "torch.float64":
            raise ValueError("%s must be float64, not %s" % (name, t.dtype))
        if t.shape[0] != n:
            raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.shape[0], n))
    k = B.shape[1]
    if k < 1 or any(t.shape[1] != k for _, t in named):
        raise ValueError("B, X and X0 need the same number of columns k >= 1 (they have %s)" % [t.shape[1] for _, t in named])
    for name, t in named:
        if t.stride(1) != 1 or t.stride(0) < k:
            raise ValueError("%s must be row-major with contiguous rows (stride(1) == 1, stride(0) >= k); its strides are %s"
                             % (name, tuple(t.stride())))
    if m is not None and (str(m.dtype) != "torch.float64" or m.numel() != n or not m.is_contiguous()):
        raise ValueError("m must be a contiguous float64 tensor of %d elements (it has %d of %s)" % (n, m.numel(), m.dtype))
    return k, B.stride(0), X.stride(0), X0.stride(0) if X0 is not None else 0


def _cg_multi(fn, handle, n, B, X, m, X0, max_steps, tol, check_every, stream):
    """smvp_csr_cg_multi / smvp_tjds_cg_multi -> (results, rr_each, rz_each or None, sigma_each): a list of k PcgResult and the
    histories as (k, max_steps + 1), (k, max_steps + 1) and (k, max_steps) numpy arrays, NaN beyond a column's filled elements
    (rr, rz: 0 .. updates; sigma: 0 .. steps - 1)."""
    k, ldb, ldx, ldx0 = cg_multi_operands(B, X, X0, m, n)
    _device_vectors(B=B, X=X, m=m, X0=X0)
    o = cg_opts(max_steps, tol, check_every)
    r = (PcgResult * k)()
    steps = max(int(max_steps), 0)
    rr, sigma = np.full((k, steps + 1), np.nan), np.full((k, max(steps, 1)), np.nan)
    rz = np.full((k, steps + 1), np.nan) if m is not None else None
    _check(getattr(lib(), fn)(handle, C.byref(o), k, _dev_ptr(B), ldb, _dev_ptr(X0), ldx0, _dev_ptr(X), ldx, _dev_ptr(m), r, _p(rr),
                              _p(rz) if rz is not None else None, _p(sigma), _stream_ptr(stream)), fn)
    return list(r), rr, rz, sigma[:, :steps]


def bicgstab_opts(max_steps=100, tol=1e-10, check_every=10):
    """smvp_bicgstab_opts_t from smvp_bicgstab_opts_default with the three fields set."""
    o = BicgstabOpts()
    lib().smvp_bicgstab_opts_default(C.byref(o))
    o.max_steps, o.check_every, o.tol = int(max_steps), int(check_every), float(tol)
    return o


def _bicgstab(fn, handle, b, x, x0, max_steps, tol, check_every, stream):
    """smvp_csr_bicgstab / smvp_tjds_bicgstab -> (BicgstabResult, rr_each, ss_each), the histories cut to the filled elements.
    ss_each has result.steps elements, one fewer where rule A ended the run: the result block does not say which, so the array
    starts as -0.0, which no ss can be (the dot's accumulators start at +0.0), and an element left so was not filled."""
    _device_vectors(b=b, x=x, x0=x0)
    o = bicgstab_opts(max_steps, tol, check_every)
    r = BicgstabResult()
    rr, ss = np.zeros(max(int(max_steps), 0) + 1), np.full(max(int(max_steps), 1), -0.0)
    _check(getattr(lib(), fn)(handle, C.byref(o), _dev_ptr(b), _dev_ptr(x0), _dev_ptr(x), C.byref(r), _p(rr), _p(ss),
                              _stream_ptr(stream)), fn)
    filled = r.steps
    if filled > 0 and ss[filled - 1] == 0.0 and np.signbit(ss[filled - 1]):
        filled -= 1
    return r, rr[:r.full + 1], ss[:filled]


def trsv_levels(rows, row_ptr, col_ind, uplo):
    """(level_of_row, levels) of the `uplo` triangle of CSR arrays on the host (smvp_csr_trsv_levels, K15): the analysis a
    TrsvPlan rests on, with no device touched."""
    rp, ci = _arr(row_ptr, np.int32), _arr(col_ind, np.int32)
    level = np.zeros(max(int(rows), 1), dtype=np.int32)
    levels = C.c_int()
    _check(lib().smvp_csr_trsv_levels(int(rows), _p(rp), _p(ci), int(uplo), _p(level), C.byref(levels)), "smvp_csr_trsv_levels")
    return level[:max(int(rows), 0)], levels.value


class TrsvPlan:
    """A triangular solve on a CsrMatrix (smvp_trsv_t, K15): T x = b for the `uplo` triangle of the matrix as stored.  It borrows
    the matrix's device arrays and keeps a reference to the CsrMatrix.  sweeps=None is the exact, level-scheduled solve; an int is
    that many Jacobi sweeps on the triangular system instead (smvp_csr_trsv_create_sweeps, K21), exact from levels - 1 sweeps on."""

    def __init__(self, matrix, uplo, diag=TRSV_DIAG_STORED, stream=None, sweeps=None):
        self._t = C.c_void_p()
        self.matrix, self.rows, self.uplo, self.diag = matrix, matrix.rows, int(uplo), int(diag)
        if sweeps is None:
            _check(lib().smvp_csr_trsv_create(C.byref(self._t), matrix._h, int(uplo), int(diag), _stream_ptr(stream)), "smvp_csr_trsv_create")
        else:
            _check(lib().smvp_csr_trsv_create_sweeps(C.byref(self._t), matrix._h, int(uplo), int(diag), int(sweeps), _stream_ptr(stream)),
                   "smvp_csr_trsv_create_sweeps")

    @property
    def sweeps(self):
        """None for an exact plan, else the number of Jacobi sweeps a solve makes (smvp_trsv_sweeps)."""
        n = C.c_int()
        _check(lib().smvp_trsv_sweeps(self._t, C.byref(n)), "smvp_trsv_sweeps")
        return None if n.value < 0 else n.value

    def solve(self, b, x, stream=None):
        """x = T^-1 b, asynchronous on `stream`: b and x are contiguous float64 CUDA tensors of `rows` elements; x may be b
        itself.  Returns x."""
        _device_vectors(b=b, x=x)
        for name, t in (("b", b), ("x", x)):
            if str(t.dtype) != "torch.float64" or t.numel() != self.rows or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float64 tensor of %d elements (it has %d of %s)"
                                 % (name, self.rows, t.numel(), t.dtype))
        _check(lib().smvp_trsv_solve(self._t, _dev_ptr(b), _dev_ptr(x), _stream_ptr(stream)), "smvp_trsv_solve")
        return x

    def info(self):
        """smvp_trsv_info_t as a dict."""
        i = TrsvInfo()
        i.struct_size = C.sizeof(TrsvInfo)
        _check(lib().smvp_trsv_info(self._t, C.byref(i)), "smvp_trsv_info")
        return {name: getattr(i, name) for name, _ in TrsvInfo._fields_[1:]}

    def schedule(self):
        """(level_ptr, order): the rows by (level, row) ascending and where each level begins in them."""
        level_ptr, order = np.zeros(self.info()["levels"] + 1, dtype=np.int32), np.zeros(max(self.rows, 1), dtype=np.int32)
        _check(lib().smvp_trsv_schedule(self._t, _p(level_ptr), _p(order)), "smvp_trsv_schedule")
        return level_ptr, order[:self.rows]

    def close(self):
        if self._t:
            lib().smvp_trsv_destroy(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pcg_tri(fn, handle, b, x, first, second, m, x0, max_steps, tol, check_every, stream):
    """smvp_csr_pcg_tri / smvp_tjds_pcg_tri -> (PcgResult, rr_each, rz_each, sigma_each), the histories cut to the filled
    elements.  first and second are open TrsvPlans; m may be None."""
    for name, t in (("first", first), ("second", second)):
        if not isinstance(t, TrsvPlan):
            raise ValueError("%s must be a TrsvPlan, not %s" % (name, type(t).__name__))
        if not t._t:
            raise ValueError("%s is a closed TrsvPlan" % name)
    _device_vectors(b=b, x=x, m=m, x0=x0)
    o = cg_opts(max_steps, tol, check_every)
    r = PcgResult()
    rr, rz, sigma = np.zeros(max(int(max_steps), 0) + 1), np.zeros(max(int(max_steps), 0) + 1), np.zeros(max(int(max_steps), 1))
    _check(getattr(lib(), fn)(handle, C.byref(o), _dev_ptr(b), _dev_ptr(x0), _dev_ptr(x), first._t, _dev_ptr(m), second._t, C.byref(r),
                              _p(rr), _p(rz), _p(sigma), _stream_ptr(stream)), fn)
    return r, rr[:r.updates + 1], rz[:r.updates + 1], sigma[:r.steps]


def _pbicgstab(fn, handle, b, x, first, second, m, x0, max_steps, tol, check_every, stream):
    """smvp_csr_pbicgstab / smvp_tjds_pbicgstab -> (BicgstabResult, rr_each, ss_each), the histories cut to the filled elements as
    _bicgstab cuts them.  first and second are open TrsvPlans or None; m may be None (all three None is the library's refusal)."""
    for name, t in (("first", first), ("second", second)):
        if t is None:
            continue
        if not isinstance(t, TrsvPlan):
            raise ValueError("%s must be a TrsvPlan or None, not %s" % (name, type(t).__name__))
        if not t._t:
            raise ValueError("%s is a closed TrsvPlan" % name)
    _device_vectors(b=b, x=x, m=m, x0=x0)
    o = bicgstab_opts(max_steps, tol, check_every)
    r = BicgstabResult()
    rr, ss = np.zeros(max(int(max_steps), 0) + 1), np.full(max(int(max_steps), 1), -0.0)
    _check(getattr(lib(), fn)(handle, C.byref(o), _dev_ptr(b), _dev_ptr(x0), _dev_ptr(x), first._t if first else None, _dev_ptr(m),
                              second._t if second else None, C.byref(r), _p(rr), _p(ss), _stream_ptr(stream)), fn)
    filled = r.steps
    if filled > 0 and ss[filled - 1] == 0.0 and np.signbit(ss[filled - 1]):
        filled -= 1
    return r, rr[:r.full + 1], ss[:filled]


def gmres_opts(max_steps=100, tol=1e-10, check_every=10, restart=30):
    """smvp_gmres_opts_t from smvp_gmres_opts_default with the four fields set."""
    o = GmresOpts()
    lib().smvp_gmres_opts_default(C.byref(o))
    o.max_steps, o.check_every, o.restart, o.tol = int(max_steps), int(check_every), int(restart), float(tol)
    return o


def _gmres(fn, handle, b, x, first, second, m, x0, restart, max_steps, tol, check_every, stream):
    """smvp_csr_gmres / smvp_tjds_gmres -> (GmresResult, rr_each, restart_each), the histories cut to the filled elements.  rr_each
    has result.steps + 1 elements, one fewer where rule S1 ended the run: the result block does not say which, so the array starts
    as -0.0, which no rr can be, and an element left so was not filled.  first and second are open TrsvPlans or None; m may be None;
    all three None is plain GMRES."""
    for name, t in (("first", first), ("second", second)):
        if t is None:
            continue
        if not isinstance(t, TrsvPlan):
            raise ValueError("%s must be a TrsvPlan or None, not %s" % (name, type(t).__name__))
        if not t._t:
            raise ValueError("%s is a closed TrsvPlan" % name)
    _device_vectors(b=b, x=x, m=m, x0=x0)
    o = gmres_opts(max_steps, tol, check_every, restart)
    r = GmresResult()
    steps, every = max(int(max_steps), 1), min(max(int(restart), 1), 64)
    rr, tr = np.full(steps + 1, -0.0), np.full(-(-steps // every) + 1, -0.0)
    _check(getattr(lib(), fn)(handle, C.byref(o), _dev_ptr(b), _dev_ptr(x0), _dev_ptr(x), first._t if first else None, _dev_ptr(m),
                              second._t if second else None, C.byref(r), _p(rr), _p(tr), _stream_ptr(stream)), fn)
    filled = r.steps + 1
    if filled > 1 and rr[filled - 1] == 0.0 and np.signbit(rr[filled - 1]):
        filled -= 1
    return r, rr[:filled], tr[:r.cycles]


def lsqr_opts(max_steps=100, tol=1e-10, atol=1e-10, check_every=10):
    """smvp_lsqr_opts_t from smvp_lsqr_opts_default with the four fields set."""
    o = LsqrOpts()
    lib().smvp_lsqr_opts_default(C.byref(o))
    o.max_steps, o.check_every, o.tol, o.atol = int(max_steps), int(check_every), float(tol), float(atol)
    return o


def _lsqr(fn, handles, b, x, x0, max_steps, tol, atol, check_every, stream):
    """smvp_csr_lsqr (handles = h, ht) / smvp_tjds_lsqr (handles = h,) -> (LsqrResult, rnorm_each, arnorm_each), the histories cut to
    the result.updates + 1 filled elements."""
    _device_vectors(b=b, x=x, x0=x0)
    o = lsqr_opts(max_steps, tol, atol, check_every)
    r = LsqrResult()
    rn, arn = np.zeros(max(int(max_steps), 0) + 1), np.zeros(max(int(max_steps), 0) + 1)
    _check(getattr(lib(), fn)(*handles, C.byref(o), _dev_ptr(b), _dev_ptr(x0), _dev_ptr(x), C.byref(r), _p(rn), _p(arn), _stream_ptr(stream)), fn)
    return r, rn[:r.updates + 1], arn[:r.updates + 1]


def ilu0_check(rows, row_ptr, col_ind):
    """diag_pos, the position of every row's (i, i), for CSR arrays on the host that admit an ILU(0) (smvp_csr_ilu0_check, K17):
    every row's columns strictly ascending, a stored diagonal in every row.  Raises SmvpError otherwise; its bad_row attribute is the
    first offending row."""
    rp, ci = _arr(row_ptr, np.int32), _arr(col_ind, np.int32)
    diag_pos = np.zeros(max(int(rows), 1), dtype=np.int32)
    bad = C.c_int(-1)
    code = lib().smvp_csr_ilu0_check(int(rows), _p(rp), _p(ci), _p(diag_pos), C.byref(bad))
    if code != OK:
        e = SmvpError(code, "smvp_csr_ilu0_check")
        e.bad_row = bad.value
        raise e
    return diag_pos[:max(int(rows), 0)]


def ilu0_host(rows, row_ptr, col_ind, val):
    """The values of the ILU(0) factor of CSR arrays on the host, by the serial loop of the header on one core
    (smvp_csr_ilu0_host, K17): what every element of Ilu0.matrix's values is, bit for bit."""
    rp, ci, v = _arr(row_ptr, np.int32), _arr(col_ind, np.int32), _arr(val, np.float64)
    nnz = int(rp[rows]) if rows > 0 else 0
    out = np.zeros(max(nnz, 1), dtype=np.float64)
    _check(lib().smvp_csr_ilu0_host(int(rows), _p(rp), _p(ci), _p(v), _p(out)), "smvp_csr_ilu0_host")
    return out[:nnz]


def color_host(rows, row_ptr, col_ind, t_row_ptr=None, t_col_ind=None, seed=0):
    """(color, colors, depth): the multicolour ordering's definition on one core (smvp_csr_color_host, K23), no device touched.
    t_row_ptr / t_col_ind: the transposed pattern, both or neither."""
    rp, ci = _arr(row_ptr, np.int32), _arr(col_ind, np.int32)
    trp = None if t_row_ptr is None else _arr(t_row_ptr, np.int32)
    tci = None if t_col_ind is None else _arr(t_col_ind, np.int32)
    color = np.zeros(max(int(rows), 1), dtype=np.int32)
    colors, depth = C.c_int(), C.c_int()
    _check(lib().smvp_csr_color_host(int(rows), _p(rp), _p(ci), None if trp is None else _p(trp), None if tci is None else _p(tci),
                                     int(seed) & 0xffffffff, _p(color), C.byref(colors), C.byref(depth)), "smvp_csr_color_host")
    return color[:max(int(rows), 0)], colors.value, depth.value


def _int32_vector(name, t, n):
    _device_vectors(**{name: t})
    if str(t.dtype) != "torch.int32" or t.numel() != n or not t.is_contiguous():
        raise ValueError("%s must be a contiguous int32 tensor of %d elements (it has %d of %s)" % (name, n, t.numel(), t.dtype))


def perm_from_classes(classes_tensor, n_classes, stream=None):
    """(old_of_new, new_of_old, class_ptr) of an int32 CUDA tensor of classes in [0, n_classes) (smvp_perm_from_classes, K23): the
    new order is by (class, old index) ascending.  The first two are int32 CUDA tensors, class_ptr a numpy array of n_classes + 1."""
    import torch

    n = classes_tensor.numel()
    _int32_vector("classes_tensor", classes_tensor, n)
    old_of_new = torch.empty(n, dtype=torch.int32, device=classes_tensor.device)
    new_of_old = torch.empty(n, dtype=torch.int32, device=classes_tensor.device)
    class_ptr = np.zeros(max(int(n_classes), 0) + 1, dtype=np.int32)
    _check(lib().smvp_perm_from_classes(classes_tensor.device.index or 0, n, int(n_classes), _dev_ptr(classes_tensor), _dev_ptr(old_of_new),
                                        _dev_ptr(new_of_old), _p(class_ptr), _stream_ptr(stream)), "smvp_perm_from_classes")
    return old_of_new, new_of_old, class_ptr


def vector_gather(index, src, out, stream=None):
    """out[p] = src[index[p]] (smvp_vector_gather, K23): index an int32, src and out float64 CUDA tensors of one length, out not
    overlapping src.  Asynchronous on `stream`.  Returns out."""
    _device_vectors(src=src, out=out)
    n = index.numel()
    _int32_vector("index", index, n)
    for name, t in (("src", src), ("out", out)):
        if str(t.dtype) != "torch.float64" or t.numel() != n or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 tensor of %d elements (it has %d of %s)" % (name, n, t.numel(), t.dtype))
    _check(lib().smvp_vector_gather(index.device.index or 0, n, _dev_ptr(index), _dev_ptr(src), _dev_ptr(out), _stream_ptr(stream)),
           "smvp_vector_gather")
    return out


class Multicolored:
    """A CsrMatrix in multicolour order (CsrMatrix.multicolored, K23): `matrix` = P A P^T, a CsrMatrix of its own; old_of_new and
    new_of_old, int32 CUDA tensors; color_ptr, where every colour's rows begin in the new order; colors; info, smvp_csr_color's."""

    def __init__(self, matrix, old_of_new, new_of_old, color_ptr, info):
        self.matrix, self.old_of_new, self.new_of_old, self.color_ptr, self.info = matrix, old_of_new, new_of_old, color_ptr, info
        self.colors = info["colors"]

    def to_new(self, v, out, stream=None):
        """out = P v: a vector of A's numbering in B's."""
        return vector_gather(self.old_of_new, v, out, stream)

    def to_old(self, v, out, stream=None):
        """out = P^T v: a vector of B's numbering in A's."""
        return vector_gather(self.new_of_old, v, out, stream)

    def close(self):
        self.matrix.close()


class Ilu0:
    """An ILU(0) of a CsrMatrix on its own pattern (smvp_ilu0_t, K17).  `matrix` is the factor as a CsrMatrix over a handle this
    object owns: strictly below the diagonal L (unit diagonal implied), on and above it U.  It borrows the CsrMatrix's device arrays
    and keeps a reference to it; `matrix` in turn keeps this object alive, so plans made on it (which keep `matrix`) may outlive
    the caller's own reference to the Ilu0: `L, U = A.ilu0().plans()` is safe.  close() ends that: close the plans first."""

    def __init__(self, matrix, stream=None):
        self._f = C.c_void_p()
        self.source, self.rows = matrix, matrix.rows
        _check(lib().smvp_csr_ilu0_create(C.byref(self._f), matrix._h, _stream_ptr(stream)), "smvp_csr_ilu0_create")
        h = C.c_void_p()
        _check(lib().smvp_ilu0_matrix(self._f, C.byref(h)), "smvp_ilu0_matrix")
        self.matrix = CsrMatrix._wrap(h, matrix.rows, matrix.cols, matrix.nnz, owner=self)

    def factor(self, stream=None):
        """Factorises the source matrix's current values again, asynchronous on `stream`; plans made on `matrix` see the new
        factors.  Returns self."""
        _check(lib().smvp_ilu0_factor(self._f, _stream_ptr(stream)), "smvp_ilu0_factor")
        return self

    def info(self):
        """smvp_ilu0_info_t as a dict."""
        i = Ilu0Info()
        i.struct_size = C.sizeof(Ilu0Info)
        _check(lib().smvp_ilu0_info(self._f, C.byref(i)), "smvp_ilu0_info")
        return {name: getattr(i, name) for name, _ in Ilu0Info._fields_[1:]}

    def plans(self, stream=None, sweeps=None):
        """(first, second) for pcg_tri with m=None: the LOWER / DIAG_UNIT and the UPPER / DIAG_STORED TrsvPlan of `matrix`, exact
        or, with an int, of that many Jacobi sweeps each.  Close them before this object."""
        return (self.matrix.trsv_plan(TRSV_LOWER, TRSV_DIAG_UNIT, stream, sweeps),
                self.matrix.trsv_plan(TRSV_UPPER, TRSV_DIAG_STORED, stream, sweeps))

    def close(self):
        if self._f:
            lib().smvp_ilu0_destroy(self._f)
            self._f = C.c_void_p()
            self.matrix._h = C.c_void_p()                    # (the borrowed handle went with it)
            self.matrix._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CsrMatrix:
    """Device-resident CSR matrix (smvp_csr_t).  Arrays may be numpy (copied to HBM) or torch CUDA tensors (adopted)."""

    def __init__(self, rows, cols, row_ptr, col_ind, val, device=0, first_row=0):
        """first_row: global number of the first row when this is a row block of a larger matrix (smvp_csr_create_block)."""
        self.rows, self.cols = rows, cols
        self._h = C.c_void_p()
        self._keep = None
        if isinstance(row_ptr, np.ndarray):
            rp, ci, v = _arr(row_ptr, np.int32), _arr(col_ind, np.int32), _arr(val, np.float64)
            self.nnz = int(rp[rows]) if rows >= 0 else 0
            _check(lib().smvp_csr_create_block(C.byref(self._h), device, rows, cols, self.nnz, _p(rp), _p(ci), _p(v),
                                               MEM_HOST, None, int(first_row)), "smvp_csr_create_block")
        else:
            host_rp = _arr(row_ptr.cpu().numpy(), np.int32)
            self.nnz = int(host_rp[rows])
            self._keep = (row_ptr, col_ind, val)
            _check(lib().smvp_csr_create_block(C.byref(self._h), device, rows, cols, self.nnz, _dev_ptr(row_ptr),
                                               _dev_ptr(col_ind), _dev_ptr(val), MEM_DEVICE, _p(host_rp), int(first_row)),
                   "smvp_csr_create_block")

    def set_kernel(self, kernel, param=0):
        _check(lib().smvp_csr_set_kernel(self._h, kernel, param), "smvp_csr_set_kernel")

    def get_kernel(self):
        k, p = C.c_int(), C.c_int()
        _check(lib().smvp_csr_get_kernel(self._h, C.byref(k), C.byref(p)), "smvp_csr_get_kernel")
        return k.value, p.value

    def launches(self):
        """Kernel launches per product of the current plan."""
        n = C.c_int()
        _check(lib().smvp_csr_plan_launches(self._h, C.byref(n)), "smvp_csr_plan_launches")
        return n.value

    def plan_info(self):
        """{matrix_bytes, plan_bytes, build_ms} of the current launch plan."""
        i = PlanInfo()
        _check(lib().smvp_csr_plan_info(self._h, C.byref(i)), "smvp_csr_plan_info")
        return {"matrix_bytes": i.matrix_bytes, "plan_bytes": i.plan_bytes, "build_ms": i.build_ms}

    def far_share(self):
        """Share of the entries further than 4096 from the diagonal of the whole matrix (AUTO's choice of the binned plan); -1: not measured."""
        v = C.c_double()
        _check(lib().smvp_csr_far_share(self._h, C.byref(v)), "smvp_csr_far_share")
        return v.value

    def gather_spread(self):
        """Share of the gathers that pull their own line of x (what AUTO's choice of the column sweep rests on); -1: not sampled."""
        v = C.c_double()
        _check(lib().smvp_csr_gather_spread(self._h, C.byref(v)), "smvp_csr_gather_spread")
        return v.value

    def spmv(self, x, y, stream=None):
        """y = A x, asynchronous on `stream`; x, y are torch CUDA float64 tensors."""
        _check(lib().smvp_csr_spmv(self._h, _dev_ptr(x), _dev_ptr(y), _stream_ptr(stream)), "smvp_csr_spmv")

    def describe(self):
        name = C.create_string_buffer(256)
        b = C.c_double()
        _check(lib().smvp_csr_describe(self._h, name, 256, C.byref(b)), "smvp_csr_describe")
        return name.value.decode(), b.value

    def power_method(self, x0, x, max_steps, tol=0.0, check_every=1, stream=None):
        """The scaled power method on this handle's product (smvp_csr_power_method, K11): x0 (None = ones) and x are float64 CUDA
        tensors of `rows` elements, x receives the last iterate and may be x0.  Returns (PowerResult, lambda_each,
        residual_each) after the work on `stream` has finished; the two histories are numpy arrays of result.steps elements."""
        return _power_method("smvp_csr_power_method", self._h, x0, x, max_steps, tol, check_every, stream)

    def cg(self, b, x, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Conjugate gradients for A x = b on this handle's product (smvp_csr_cg, K12; A symmetric positive definite): b, x and
        x0 (None = zeros) are float64 CUDA tensors of `rows` elements, x receives the solution and may be x0.  Returns (CgResult,
        rr_each, sigma_each) after the work on `stream` has finished: rr_each has result.updates + 1 squared residual norms,
        sigma_each result.steps values of p.Ap.  Nothing depends on check_every but how often the host waits."""
        return _cg("smvp_csr_cg", self._h, b, x, x0, max_steps, tol, check_every, stream)

    def diagonal(self, out, stream=None):
        """The diagonal of the matrix into `out`, a float64 CUDA tensor of `rows` elements (smvp_csr_diagonal, K14): element i is
        the sum of the stored entries (i, i) in storage order from +0.0 -- on a row block, of the entries at column first_row + i.
        Asynchronous on `stream`; needs no plan and leaves the handle alone.  Returns `out`."""
        return _diagonal("smvp_csr_diagonal", self._h, self.rows, out, stream)

    def pcg(self, b, x, m, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Conjugate gradients for A x = b preconditioned with diag(m) (smvp_csr_pcg, K14; A symmetric positive definite, m
        positive -- usually diagonal()'s output): operands as cg(), m a float64 CUDA tensor of `rows` elements.  Returns
        (PcgResult, rr_each, rz_each, sigma_each) after the work on `stream` has finished: rr_each and rz_each have
        result.updates + 1 values of r.r and r.z, sigma_each result.steps values of p.Ap.  The stop rule is cg()'s, on r.r."""
        return _pcg("smvp_csr_pcg", self._h, b, x, m, x0, max_steps, tol, check_every, stream)

    def cg_multi(self, B, X, m=None, X0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """k conjugate-gradient runs that share every read of the matrix and every launch (smvp_csr_cg_multi, K20): column v of X
        receives the solution of A x = B[:, v] from X0[:, v] (None = zeros), by cg()'s rules, or pcg()'s with m given.  B, X and X0
        are float64 CUDA tensors of shape (rows, k) with contiguous rows -- contiguous, or column slices of wider tensors: the
        leading dimensions are the tensors' stride(0) --, X may be X0, m has `rows` elements.  Returns (results, rr_each, rz_each or
        None, sigma_each) after the work on `stream` has finished: a list of k PcgResult, and (k, .) numpy arrays of the histories
        that hold NaN beyond a column's filled elements.  The product is spmm()'s: the kernel set_kernel chose plays no part."""
        return _cg_multi("smvp_csr_cg_multi", self._h, self.rows, B, X, m, X0, max_steps, tol, check_every, stream)

    def trsv_plan(self, uplo, diag=TRSV_DIAG_STORED, stream=None, sweeps=None):
        """A TrsvPlan for the `uplo` triangle of this matrix as stored (smvp_csr_trsv_create, K15): TRSV_LOWER or TRSV_UPPER,
        the diagonal as stored or taken as ones.  Analysed on the host once; close the plan before the matrix.  sweeps=None is
        the exact solve; an int makes the plan that many Jacobi sweeps instead (smvp_csr_trsv_create_sweeps, K21)."""
        return TrsvPlan(self, uplo, diag, stream, sweeps)

    def pcg_tri(self, b, x, first, second, m=None, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Conjugate gradients for A x = b preconditioned with M = T1 diag(m)^-1 T2 (smvp_csr_pcg_tri, K16): z = M^-1 r is
        first.solve, a multiplication by m (skipped for m=None), second.solve.  first and second are TrsvPlans of any CsrMatrix
        of `rows` rows on this device -- for symmetric Gauss-Seidel trsv_plan(TRSV_LOWER) and trsv_plan(TRSV_UPPER) of this
        matrix with m = diagonal().  Operands, stop rule and return value as pcg()."""
        return _pcg_tri("smvp_csr_pcg_tri", self._h, b, x, first, second, m, x0, max_steps, tol, check_every, stream)

    def bicgstab(self, b, x, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """BiCGSTAB for A x = b on this handle's product (smvp_csr_bicgstab, K13; A any square matrix): b, x and x0 (None = zeros)
        are float64 CUDA tensors of `rows` elements, x receives the solution and may be x0.  Returns (BicgstabResult, rr_each,
        ss_each) after the work on `stream` has finished: rr_each has result.full + 1 squared residual norms, ss_each the squared
        norm of s of every step that got as far.  Nothing depends on check_every but how often the host waits."""
        return _bicgstab("smvp_csr_bicgstab", self._h, b, x, x0, max_steps, tol, check_every, stream)

    def pbicgstab(self, b, x, first=None, second=None, m=None, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Right-preconditioned BiCGSTAB for A x = b with M = T1 diag(m)^-1 T2 (smvp_csr_pbicgstab, K18; A any square matrix):
        first and second are TrsvPlans of any CsrMatrix with as many rows, m a float64 CUDA tensor, each of the three optional but
        not all None.  m = 1 / diagonal() alone is Jacobi; ilu0().plans() is ILU(0); the LOWER and UPPER / STORED plans of this
        matrix with m = diagonal() are symmetric Gauss-Seidel.  Operands and result as bicgstab: (BicgstabResult, rr_each,
        ss_each).  With plans, choose a small check_every: a step enqueued in vain runs four solves."""
        return _pbicgstab("smvp_csr_pbicgstab", self._h, b, x, first, second, m, x0, max_steps, tol, check_every, stream)

    def gmres(self, b, x, first=None, second=None, m=None, x0=None, restart=30, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Right-preconditioned restarted GMRES(restart) for A x = b with M = T1 diag(m)^-1 T2 (smvp_csr_gmres, K19; A any square
        matrix): the preconditioner as for pbicgstab, and all of first, second and m None is plain GMRES.  restart is 1 .. 64.
        Returns (GmresResult, rr_each, restart_each) after the work on `stream` has finished: rr_each holds tr_0 and the estimate
        of the squared residual norm after every step, restart_each the true squared residual norm at every cycle's start.
        Nothing depends on check_every but how often the host waits."""
        return _gmres("smvp_csr_gmres", self._h, b, x, first, second, m, x0, restart, max_steps, tol, check_every, stream)

    def lsqr(self, b, x, at=None, x0=None, max_steps=100, tol=1e-10, atol=1e-10, check_every=10, stream=None):
        """LSQR for min |A x - b| on any rows x cols matrix (smvp_csr_lsqr, K22): b holds rows elements, x and x0 cols; x0 = None
        starts from zeros, and x may be x0.  at is a CsrMatrix of A^T, cols x rows -- transposed() makes one, and a caller who
        solves more than once keeps it; at = None builds transposed() for this call and closes it afterwards.  Each matrix
        multiplies on its own current kernel.  Returns (LsqrResult, rnorm_each, arnorm_each) after the work on `stream` has
        finished: the estimates of |b - A x| and |A^T (b - A x)| after every update of x, element 0 for x0.  reason is
        LSQR_CONVERGED (|r| <= tol |b|), LSQR_LEAST_SQUARES (|A^T r| <= atol |A|_F |r|), LSQR_MAX_STEPS or LSQR_NONFINITE.
        Nothing depends on check_every but how often the host waits."""
        if at is not None and not isinstance(at, CsrMatrix):
            raise ValueError("at must be a CsrMatrix or None, not %s" % type(at).__name__)
        own = self.transposed(stream) if at is None else None
        try:
            return _lsqr("smvp_csr_lsqr", (self._h, (own or at)._h), b, x, x0, max_steps, tol, atol, check_every, stream)
        finally:
            if own is not None:
                own.close()

    def spmm(self, X, Y, stream=None):
        """Y = A X for k vectors at once (smvp_csr_spmm): X (cols x k) and Y (rows x k) are float64 CUDA tensors with
        stride(1) == 1, ldx = X.stride(0), ldy = Y.stride(0).  Every column of Y is the serial loop's bits.  Asynchronous on
        `stream`; the first call builds the plan."""
        _spmm("smvp_csr_spmm", self._h, X, Y, self.rows, self.cols, stream)

    def spmm_describe(self, k):
        """(kernel symbols, algorithmic bytes for k vectors, {plan_bytes, build_ms} of the SpMM plan: 0 before the first spmm)."""
        return _spmm_describe("smvp_csr_spmm_describe", self._h, k, True)

    @classmethod
    def _wrap(cls, handle, rows, cols, nnz, owner=None):
        """A CsrMatrix over a handle the library made itself (it owns its arrays).  owner: the object the handle belongs to (an
        Ilu0 and its factor) -- close() then destroys nothing, and the wrapper keeps the owner alive as long as it lives itself."""
        m = cls.__new__(cls)
        m.rows, m.cols, m.nnz = rows, cols, nnz
        m._h, m._keep = handle, owner
        m._borrowed = owner is not None
        return m

    def ilu0(self, stream=None):
        """The ILU(0) of this matrix on its own pattern (smvp_csr_ilu0_create, K17) as an Ilu0: every row's columns must be
        strictly ascending and every row must store its diagonal.  Returns after the first factorisation has finished; close the
        Ilu0 before the matrix."""
        return Ilu0(self, stream)

    def transposed(self, stream=None):
        """A^T as a CsrMatrix of its own (smvp_csr_create_transposed): cols x rows, built on the device, independent of this
        one.  Returns after the work on `stream` has finished."""
        h = C.c_void_p()
        _check(lib().smvp_csr_create_transposed(C.byref(h), self._h, _stream_ptr(stream)), "smvp_csr_create_transposed")
        return CsrMatrix._wrap(h, self.cols, self.rows, self.nnz)

    def color(self, color_out, at=None, seed=0, max_rounds=4096, stream=None):
        """The multicolour ordering's colours into color_out, an int32 CUDA tensor of `rows` elements (smvp_csr_color, K23); at: the
        CsrMatrix of A^T for a matrix that is not structurally symmetric.  Returns smvp_color_info_t as a dict."""
        _int32_vector("color_out", color_out, self.rows)
        o = ColorOpts()
        lib().smvp_color_opts_default(C.byref(o))
        o.seed, o.max_rounds = int(seed) & 0xffffffff, int(max_rounds)
        i = ColorInfo()
        i.struct_size = C.sizeof(ColorInfo)
        _check(lib().smvp_csr_color(self._h, None if at is None else at._h, C.byref(o), _dev_ptr(color_out), C.byref(i), _stream_ptr(stream)),
               "smvp_csr_color")
        return {name: getattr(i, name) for name, _ in ColorInfo._fields_[1:]}

    def permuted(self, new_of_old, stream=None):
        """B = P A P^T as a CsrMatrix of its own (smvp_csr_create_permuted, K23): B[new_of_old[r], new_of_old[c]] = A[r, c] for an
        int32 CUDA tensor that is a permutation of 0 .. rows-1.  Returns after the work on `stream` has finished."""
        _int32_vector("new_of_old", new_of_old, self.rows)
        h = C.c_void_p()
        _check(lib().smvp_csr_create_permuted(C.byref(h), self._h, _dev_ptr(new_of_old), _stream_ptr(stream)), "smvp_csr_create_permuted")
        return CsrMatrix._wrap(h, self.rows, self.cols, self.nnz)

    def multicolored(self, at=None, seed=0, max_rounds=4096, stream=None):
        """color -> perm_from_classes -> permuted, as a Multicolored: every triangular plan and ILU(0) made on its `matrix` has at most
        `colors` levels (with a structurally symmetric matrix, or with `at`).  The tensors are made on torch's current device, which
        must be the matrix's."""
        import torch

        color = torch.empty(self.rows, dtype=torch.int32, device="cuda")
        info = self.color(color, at, seed, max_rounds, stream)
        old_of_new, new_of_old, color_ptr = perm_from_classes(color, info["colors"], stream)
        return Multicolored(self.permuted(new_of_old, stream), old_of_new, new_of_old, color_ptr, info)

    def device_arrays(self):
        """(row_ptr, col_ind, val): the device addresses the handle multiplies from, as ints; valid until close()."""
        rp, ci, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().smvp_csr_device_arrays(self._h, C.byref(rp), C.byref(ci), C.byref(v)), "smvp_csr_device_arrays")
        return rp.value or 0, ci.value or 0, v.value or 0

    def close(self):
        if self._h and not getattr(self, "_borrowed", False):
            lib().smvp_csr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TjdsMatrix:
    """Device-resident TJDS matrix (smvp_tjds_t) built from TjdsArrays."""

    def __init__(self, t, device=0):
        self.rows, self.cols, self.nnz = t.rows, t.cols, t.nnz
        self._t = t
        self._h = C.c_void_p()
        if isinstance(t.perm, np.ndarray):
            _check(lib().smvp_tjds_create(C.byref(self._h), device, t.rows, t.cols, t.nnz, t.num_diag,
                                          _p(_arr(t.perm, np.int32)), _p(_arr(t.start_pos, np.int32)),
                                          _p(_arr(t.row_ind, np.int32)), _p(_arr(t.val, np.float64)), MEM_HOST),
                   "smvp_tjds_create")
        else:       # torch CUDA tensors (smvp_tjds_from_coo_device): adopted in place
            _check(lib().smvp_tjds_create(C.byref(self._h), device, t.rows, t.cols, t.nnz, t.num_diag,
                                          _dev_ptr(t.perm), _dev_ptr(t.start_pos), _dev_ptr(t.row_ind),
                                          _dev_ptr(t.val), MEM_DEVICE), "smvp_tjds_create")

    def set_x(self, x, stream=None):
        _check(lib().smvp_tjds_set_x(self._h, _dev_ptr(x), _stream_ptr(stream)), "smvp_tjds_set_x")

    def zero_y(self, y, stream=None):
        _check(lib().smvp_tjds_zero_y(self._h, _dev_ptr(y), _stream_ptr(stream)), "smvp_tjds_zero_y")

    def spmv(self, y, stream=None):
        _check(lib().smvp_tjds_spmv(self._h, _dev_ptr(y), _stream_ptr(stream)), "smvp_tjds_spmv")

    def power_method(self, x0, x, max_steps, tol=0.0, check_every=1, stream=None):
        """The scaled power method on this handle's product in its current mode (smvp_tjds_power_method, K11; ROW_GATHER or
        TWO_PHASE, no ref-quirks): operands and result as CsrMatrix.power_method.  Afterwards the handle's permuted operand is the
        last step's: call set_x again before the next spmv."""
        return _power_method("smvp_tjds_power_method", self._h, x0, x, max_steps, tol, check_every, stream)

    def cg(self, b, x, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Conjugate gradients for A x = b on this handle's product in its current mode (smvp_tjds_cg, K12; ROW_GATHER or
        TWO_PHASE, no ref-quirks): operands and result as CsrMatrix.cg.  Afterwards the handle's permuted operand is the last
        direction's: call set_x again before the next spmv."""
        return _cg("smvp_tjds_cg", self._h, b, x, x0, max_steps, tol, check_every, stream)

    def diagonal(self, out, stream=None):
        """The diagonal of the matrix into `out`, a float64 CUDA tensor of `rows` elements (smvp_tjds_diagonal, K14), from the TJDS
        arrays themselves: the bits CsrMatrix.diagonal gives for the same entries.  Asynchronous on `stream`; needs no set_x and
        leaves the forward product's state alone.  Returns `out`."""
        return _diagonal("smvp_tjds_diagonal", self._h, self.rows, out, stream)

    def pcg(self, b, x, m, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Conjugate gradients preconditioned with diag(m) on this handle's product in its current mode (smvp_tjds_pcg, K14;
        ROW_GATHER or TWO_PHASE, no ref-quirks): operands and result as CsrMatrix.pcg.  Afterwards the handle's permuted operand is
        the last direction's: call set_x again before the next spmv."""
        return _pcg("smvp_tjds_pcg", self._h, b, x, m, x0, max_steps, tol, check_every, stream)

    def cg_multi(self, B, X, m=None, X0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """k conjugate-gradient runs that share every read of the matrix and every launch (smvp_tjds_cg_multi, K20): operands and
        result as CsrMatrix.cg_multi.  The product is spmm()'s, in every mode, ATOMIC and ref-quirks included; the permuted operand
        of set_x is neither read nor written."""
        return _cg_multi("smvp_tjds_cg_multi", self._h, self.rows, B, X, m, X0, max_steps, tol, check_every, stream)

    def pcg_tri(self, b, x, first, second, m=None, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Conjugate gradients preconditioned with M = T1 diag(m)^-1 T2 on this handle's product in its current mode
        (smvp_tjds_pcg_tri, K16; ROW_GATHER or TWO_PHASE, no ref-quirks): operands and result as CsrMatrix.pcg_tri.  The
        TrsvPlans belong to CsrMatrix objects of the same size.  Afterwards call set_x again before the next spmv."""
        return _pcg_tri("smvp_tjds_pcg_tri", self._h, b, x, first, second, m, x0, max_steps, tol, check_every, stream)

    def bicgstab(self, b, x, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """BiCGSTAB for A x = b on this handle's product in its current mode (smvp_tjds_bicgstab, K13; ROW_GATHER or TWO_PHASE, no
        ref-quirks): operands and result as CsrMatrix.bicgstab.  Afterwards the handle's permuted operand is the last vector
        multiplied: call set_x before the next spmv."""
        return _bicgstab("smvp_tjds_bicgstab", self._h, b, x, x0, max_steps, tol, check_every, stream)

    def pbicgstab(self, b, x, first=None, second=None, m=None, x0=None, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Right-preconditioned BiCGSTAB for A x = b on this handle's product in its current mode (smvp_tjds_pbicgstab, K18;
        ROW_GATHER or TWO_PHASE, no ref-quirks): operands and result as CsrMatrix.pbicgstab.  The plans belong to CsrMatrix
        objects; Jacobi (m = 1 / diagonal() alone) needs none."""
        return _pbicgstab("smvp_tjds_pbicgstab", self._h, b, x, first, second, m, x0, max_steps, tol, check_every, stream)

    def gmres(self, b, x, first=None, second=None, m=None, x0=None, restart=30, max_steps=100, tol=1e-10, check_every=10, stream=None):
        """Right-preconditioned restarted GMRES(restart) for A x = b on this handle's product in its current mode (smvp_tjds_gmres,
        K19; ROW_GATHER or TWO_PHASE, no ref-quirks): operands and result as CsrMatrix.gmres.  The plans belong to CsrMatrix
        handles; afterwards the handle's permuted operand is the last vector multiplied: call set_x again."""
        return _gmres("smvp_tjds_gmres", self._h, b, x, first, second, m, x0, restart, max_steps, tol, check_every, stream)

    def lsqr(self, b, x, x0=None, max_steps=100, tol=1e-10, atol=1e-10, check_every=10, stream=None):
        """LSQR for min |A x - b| on this handle alone (smvp_tjds_lsqr, K22): A v is the product of the current mode (ROW_GATHER or
        TWO_PHASE, no ref-quirks), A^T u is spmv_transposed, from the same arrays.  Operands and result as CsrMatrix.lsqr.  Call
        set_x again before the next spmv."""
        return _lsqr("smvp_tjds_lsqr", (self._h,), b, x, x0, max_steps, tol, atol, check_every, stream)

    def spmv_transposed(self, x, y, stream=None):
        """y = A^T x from the TJDS arrays themselves (smvp_tjds_spmv_transposed, K8): x of `rows`, y of `cols` float64 CUDA
        elements.  Asynchronous on `stream`; needs no set_x and leaves the forward product's state alone."""
        transposed_operands(x, y, self.rows, self.cols)
        if not (x.is_cuda and y.is_cuda):
            raise ValueError("x and y must be device tensors")
        _check(lib().smvp_tjds_spmv_transposed(self._h, _dev_ptr(x), _dev_ptr(y), _stream_ptr(stream)),
               "smvp_tjds_spmv_transposed")

    def transposed_describe(self):
        """(kernel symbol, algorithmic bytes) of spmv_transposed."""
        name = C.create_string_buffer(128)
        b = C.c_double()
        _check(lib().smvp_tjds_transposed_describe(self._h, name, 128, C.byref(b)), "smvp_tjds_transposed_describe")
        return name.value.decode(), b.value

    def spmm_transposed(self, X, Y, stream=None):
        """Y = A^T X for k vectors at once from the TJDS arrays themselves (smvp_tjds_spmm_transposed, K9): X (rows x k) and
        Y (cols x k) are float64 CUDA tensors with stride(1) == 1, ldx = X.stride(0), ldy = Y.stride(0).  Every column of Y is
        the transposed product's bits.  Asynchronous on `stream`; needs no set_x and no plan."""
        _spmm("smvp_tjds_spmm_transposed", self._h, X, Y, self.cols, self.rows, stream)

    def spmm_transposed_describe(self, k):
        """(kernel symbols, algorithmic bytes for k vectors) of spmm_transposed."""
        return _spmm_describe("smvp_tjds_spmm_transposed_describe", self._h, k, False)

    def spmm(self, X, Y, stream=None):
        """Y = A X for k vectors at once from a TJDS handle (smvp_tjds_spmm, K10): X (cols x k) and Y (rows x k) are float64
        CUDA tensors with stride(1) == 1, ldx = X.stride(0), ldy = Y.stride(0).  Every column of Y is the serial sum over the
        row in TJDS position order.  Asynchronous on `stream`; needs no set_x; the first call builds the plan."""
        _spmm("smvp_tjds_spmm", self._h, X, Y, self.rows, self.cols, stream)

    def spmm_describe(self, k):
        """(kernel symbols, algorithmic bytes for k vectors, {plan_bytes, build_ms} of the SpMM plan: 0 before the first spmm)."""
        return _spmm_describe("smvp_tjds_spmm_describe", self._h, k, True)

    def set_mode(self, mode):
        _check(lib().smvp_tjds_set_mode(self._h, mode), "smvp_tjds_set_mode")

    def set_tile(self, entries_per_tile):
        _check(lib().smvp_tjds_set_tile(self._h, entries_per_tile), "smvp_tjds_set_tile")

    def set_value_cache(self, min_tiles):
        """Keep a second copy of the values of val lines shared by `min_tiles` tiles or more (0 = none)."""
        _check(lib().smvp_tjds_set_value_cache(self._h, int(min_tiles)), "smvp_tjds_set_value_cache")

    def get_value_cache(self):
        """(min_tiles, cached entries)."""
        m, n = C.c_int(), C.c_longlong()
        _check(lib().smvp_tjds_get_value_cache(self._h, C.byref(m), C.byref(n)), "smvp_tjds_get_value_cache")
        return m.value, n.value

    def plan_info(self):
        """{matrix_bytes, plan_bytes, build_ms}: the plans of the modes selected so far."""
        i = PlanInfo()
        _check(lib().smvp_tjds_plan_info(self._h, C.byref(i)), "smvp_tjds_plan_info")
        return {"matrix_bytes": i.matrix_bytes, "plan_bytes": i.plan_bytes, "build_ms": i.build_ms}

    def set_ref_quirks(self, enable=True):
        _check(lib().smvp_tjds_set_ref_quirks(self._h, int(enable), self._t.ref_num_tjdiag,
                                              self._t.last_diag_single), "smvp_tjds_set_ref_quirks")

    def describe(self):
        name = C.create_string_buffer(128)
        b = C.c_double()
        _check(lib().smvp_tjds_describe(self._h, name, 128, C.byref(b)), "smvp_tjds_describe")
        return name.value.decode(), b.value

    def close(self):
        if self._h:
            lib().smvp_tjds_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedMatrix:
    """Row blocks of one matrix on several GPUs of this process (smvp_sharded_t), RCCL all-gather of y."""

    def __init__(self, fmt, ngpus, rows, cols, coo=None, csr=None, devices=None, chunks=0, balance=True, exchange=EXCHANGE_AUTO):
        self._h = C.c_void_p()
        devs = None if devices is None else (C.c_int * ngpus)(*devices)
        o = ShardOpts()
        lib().smvp_shard_opts_default(C.byref(o))
        o.chunks, o.balance, o.exchange = int(chunks), int(balance), int(exchange)
        if fmt == "csr":
            rp, ci, v = csr
            nnz = int(rp[rows])
            _check(lib().smvp_csr_sharded_create_ex(C.byref(self._h), ngpus, devs, rows, cols, nnz, _p(_arr(rp, np.int32)),
                                                    _p(_arr(ci, np.int32)), _p(_arr(v, np.float64)), C.byref(o)),
                   "smvp_csr_sharded_create_ex")
        else:
            nnz = len(coo)
            _check(lib().smvp_tjds_sharded_create_ex(C.byref(self._h), ngpus, devs, _p(_arr(coo, COO_DTYPE)), rows, cols,
                                                     nnz, C.byref(o)), "smvp_tjds_sharded_create_ex")
        self.rows, self.cols = rows, cols

    def layout(self):
        """(chunks per GPU, block bounds[ngpus + 1], chunk bounds[ngpus][chunks + 1]) in global rows."""
        n, _ = self.info()
        c = C.c_int()
        _check(lib().smvp_sharded_layout(self._h, C.byref(c), None, None), "smvp_sharded_layout")
        bounds = np.zeros(n + 1, dtype=np.int32)
        cb = np.zeros(n * (c.value + 1), dtype=np.int32)
        _check(lib().smvp_sharded_layout(self._h, C.byref(c), _p(bounds), _p(cb)), "smvp_sharded_layout")
        return c.value, bounds, cb.reshape(n, c.value + 1)

    def set_csr_kernel(self, kernel, param=0):
        _check(lib().smvp_sharded_set_csr_kernel(self._h, kernel, param), "smvp_sharded_set_csr_kernel")

    def probe_exchange(self, reps=3):
        """Time one product's exchange of y under every available form (AUTO handles then keep the fastest)."""
        _check(lib().smvp_sharded_probe_exchange(self._h, int(reps)), "smvp_sharded_probe_exchange")
        return self.exchange_info()

    def exchange_info(self):
        """{"active": EXCHANGE_*, "available": [EXCHANGE_*...], "ms": {name: ms of the last probe}, "rccl_ranks": n}."""
        act, av, rk = C.c_int(), C.c_int(), C.c_int()
        ms = (C.c_double * 3)()
        _check(lib().smvp_sharded_exchange_info(self._h, C.byref(act), C.byref(av), ms, C.byref(rk)), "smvp_sharded_exchange_info")
        return {"active": act.value, "active_name": EXCHANGE_NAMES[act.value],
                "available": [e for e in range(3) if av.value >> e & 1],
                "ms": {EXCHANGE_NAMES[e]: ms[e] for e in range(3) if ms[e] >= 0}, "rccl_ranks": rk.value}

    def set_exchange(self, exchange):
        _check(lib().smvp_sharded_set_exchange(self._h, int(exchange)), "smvp_sharded_set_exchange")

    def set_x(self, x=None):
        keep = None if x is None else _arr(x, np.float64)
        _check(lib().smvp_sharded_set_x(self._h, None if keep is None else _p(keep)), "smvp_sharded_set_x")

    def spmv(self, allgather=GATHER_OVERLAPPED, timed=True):
        """allgather: GATHER_NONE / GATHER_OVERLAPPED (True) / GATHER_AFTER."""
        _check(lib().smvp_sharded_spmv(self._h, int(allgather), int(timed)), "smvp_sharded_spmv")

    def feed_back(self, normalize=False):
        _check(lib().smvp_sharded_feed_back(self._h, int(normalize)), "smvp_sharded_feed_back")

    def synchronize(self):
        ms = C.c_double()
        _check(lib().smvp_sharded_synchronize(self._h, C.byref(ms)), "smvp_sharded_synchronize")
        return ms.value

    def get_y(self, slot=0, gathered=True):
        y = np.zeros(max(self.rows, 1), dtype=np.float64)
        _check(lib().smvp_sharded_get_y(self._h, slot, int(gathered), _p(y)), "smvp_sharded_get_y")
        return y[:self.rows]

    def info(self):
        n, b = C.c_int(), C.c_int()
        _check(lib().smvp_sharded_info(self._h, C.byref(n), C.byref(b)), "smvp_sharded_info")
        return n.value, b.value

    def close(self):
        if self._h:
            lib().smvp_sharded_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------- reference-shaped entry points
def _run_opts(device, csr_kernel, csr_param, ref_quirks, x, device_convert=False, ngpus=0, iterate=False,
              normalize=False, tjds_mode=TJDS_MODE_AUTO, timing=TIMING_AUTO, exchange=EXCHANGE_AUTO, repeat_patience_us=0):
    o = RunOpts()
    lib().smvp_run_opts_default(C.byref(o))
    o.device, o.csr_kernel, o.csr_param, o.tjds_ref_quirks = device, csr_kernel, csr_param, int(ref_quirks)
    o.convert_on_device, o.ngpus = int(device_convert), int(ngpus)
    o.iterate, o.normalize = int(iterate), int(normalize)
    o.tjds_mode, o.timing, o.shard_exchange = int(tjds_mode), int(timing), int(exchange)
    o.repeat_patience_us = int(repeat_patience_us)
    keep = None
    if x is not None:
        keep = _arr(x, np.float64)
        o.x = keep.ctypes.data
    return o, keep


def last_run_info():
    """How the last *_compute on this thread timed its products -> RunInfo (timing, graph_replays, wall_ms, ...)."""
    r = RunInfo()
    _check(lib().smvp_last_run_info(C.byref(r)), "smvp_last_run_info")
    return r


def csr_compute(coo, rows, cols, iters=1, device=0, kernel=CSR_KERNEL_AUTO, param=0, x=None, device_convert=False,
                ngpus=0, iterate=False, normalize=False, timing=TIMING_AUTO, exchange=EXCHANGE_AUTO, repeat_patience_us=0):
    """smvp_csr_compute: COO in, (y, per-iteration ms, TimeStats) out."""
    nnz = len(coo)
    coo = _arr(coo, COO_DTYPE)
    y = np.zeros(max(rows, 1), dtype=np.float64)
    ms = np.zeros(iters, dtype=np.float64)
    st = TimeStats()
    o, keep = _run_opts(device, kernel, param, False, x, device_convert, ngpus, iterate, normalize, timing=timing, exchange=exchange,
                        repeat_patience_us=repeat_patience_us)
    _check(lib().smvp_csr_compute(_p(coo), rows, cols, nnz, iters, C.byref(o), _p(y), _p(ms), C.byref(st)),
           "smvp_csr_compute")
    return y[:rows], ms, st


def tjds_compute(coo, rows, cols, iters=1, device=0, ref_quirks=False, x=None, device_convert=False, ngpus=0,
                 iterate=False, normalize=False, mode=TJDS_MODE_AUTO, timing=TIMING_AUTO, exchange=EXCHANGE_AUTO, repeat_patience_us=0):
    """smvp_tjds_compute: COO in, (y, per-iteration ms, TimeStats) out."""
    nnz = len(coo)
    coo = _arr(coo, COO_DTYPE)
    y = np.zeros(max(rows, 1), dtype=np.float64)
    ms = np.zeros(iters, dtype=np.float64)
    st = TimeStats()
    o, keep = _run_opts(device, CSR_KERNEL_AUTO, 0, ref_quirks, x, device_convert, ngpus, iterate, normalize,
                        tjds_mode=mode, timing=timing, exchange=exchange, repeat_patience_us=repeat_patience_us)
    _check(lib().smvp_tjds_compute(_p(coo), rows, cols, nnz, iters, C.byref(o), _p(y), _p(ms), C.byref(st)),
           "smvp_tjds_compute")
    return y[:rows], ms, st


# -------------------------------------------------------------- stats + report
def time_stats(ms):
    ms = _arr(ms, np.float64)
    st = TimeStats()
    _check(lib().smvp_time_stats(_p(ms), len(ms), C.byref(st)), "smvp_time_stats")
    return st


def generate_report_text(input_name, report_dir, alg_name, nnz, y, iters, stats, unix_time=0):
    rows = len(y)
    y = _arr(y, np.float64)
    out = C.create_string_buffer(4096)
    _check(lib().smvp_generate_report_text(os.fsencode(input_name), os.fsencode(report_dir or ""),
                                           alg_name.encode(), nnz, rows, iters, _p(y), C.byref(stats),
                                           unix_time, out, 4096), "smvp_generate_report_text")
    return out.value.decode()
