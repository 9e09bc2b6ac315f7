"""ctypes binding of the C-ABI in the headers under include/ (libvggsfm_amd.so, built for gfx950).

There is NO fallback: if the shared library is missing or was built for another target, importing
a product function that needs it raises.  torch is imported first so that the library resolves
``libamdhip64.so.7`` to the HIP runtime torch already loaded (same streams, same allocations).

The C type of every argument of every entry is declared once, in ``HEADERS`` below: one row per entry, grouped by the public
header that declares it, and applied when the library is loaded, so callers pass tensors, ``None``, ints and floats as they
are.  A new C-ABI entry needs a prototype in a header under include/ and a row under that header's key
(tests/test_c_abi.py compares the two, type by type, and both with the library's symbols).
"""
import ctypes
import operator
import os

import torch  # noqa: F401  (must be loaded before the HIP library, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (VGGSFM_AMD_LIB: an alternative build of the same library, for A/B measurements of kernel variants)
LIB_PATH = os.environ.get("VGGSFM_AMD_LIB") or os.path.join(_HERE, "libvggsfm_amd.so")

VGG_OK = 0
ABI_VERSION = 2       # VGG_ABI_VERSION of include/vggsfm_amd.h this binding was written against
_ERRORS = {-1: "invalid argument", -2: "HIP runtime error", -3: "workspace too small / missing",
           -4: "unsupported configuration"}


class BAProblem(ctypes.Structure):
    _fields_ = [("num_cams", ctypes.c_int32), ("num_pts", ctypes.c_int32), ("num_obs", ctypes.c_int32),
                ("num_intr", ctypes.c_int32), ("camera_model", ctypes.c_int32), ("refine_focal", ctypes.c_int32),
                ("refine_extra", ctypes.c_int32), ("loss", ctypes.c_int32), ("loss_scale", ctypes.c_double),
                ("cam_q", ctypes.c_void_p), ("cam_t", ctypes.c_void_p), ("intr", ctypes.c_void_p),
                ("pts", ctypes.c_void_p), ("row_ptr", ctypes.c_void_p), ("obs_cam", ctypes.c_void_p),
                ("obs_uv", ctypes.c_void_p), ("col_ptr", ctypes.c_void_p), ("cobs_pt", ctypes.c_void_p),
                ("cobs_uv", ctypes.c_void_p), ("cam_const", ctypes.c_void_p), ("intr_const", ctypes.c_void_p),
                ("pt_const", ctypes.c_void_p), ("num_chunks", ctypes.c_int32), ("num_tile_batches", ctypes.c_int32),
                ("chunk_desc", ctypes.c_void_p),
                ("entries", ctypes.c_void_p), ("num_segments", ctypes.c_int32), ("obs_slot", ctypes.c_void_p),
                ("num_tiles", ctypes.c_int32), ("tile_desc", ctypes.c_void_p), ("tile_batches", ctypes.c_void_p),
                ("chol_split_a", ctypes.c_int32), ("chol_split_b", ctypes.c_int32), ("chol_first_blk", ctypes.c_void_p), ("merged_tile_launch", ctypes.c_int32)]


class BAOptions(ctypes.Structure):
    _fields_ = [("max_num_iterations", ctypes.c_int32), ("max_num_consecutive_invalid_steps", ctypes.c_int32),
                ("jacobi_scaling", ctypes.c_int32), ("function_tolerance", ctypes.c_double),
                ("gradient_tolerance", ctypes.c_double), ("parameter_tolerance", ctypes.c_double),
                ("initial_trust_region_radius", ctypes.c_double), ("max_trust_region_radius", ctypes.c_double),
                ("min_trust_region_radius", ctypes.c_double), ("min_lm_diagonal", ctypes.c_double),
                ("max_lm_diagonal", ctypes.c_double), ("min_relative_decrease", ctypes.c_double),
                ("overlap_factorization", ctypes.c_int32)]


class BAIteration(ctypes.Structure):
    _fields_ = [("iteration", ctypes.c_int32), ("successful", ctypes.c_int32), ("cost", ctypes.c_double),
                ("cost_change", ctypes.c_double), ("gradient_max_norm", ctypes.c_double),
                ("step_norm", ctypes.c_double), ("relative_decrease", ctypes.c_double), ("radius", ctypes.c_double)]


class BASummary(ctypes.Structure):
    _fields_ = [("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                ("num_iterations", ctypes.c_int32), ("num_successful_steps", ctypes.c_int32),
                ("num_unsuccessful_steps", ctypes.c_int32), ("termination", ctypes.c_int32),
                ("n_reduced", ctypes.c_int32), ("num_log", ctypes.c_int32)]


class _P:
    """A pointer parameter: None (NULL), a tensor (its data_ptr(): device or host memory, the entry decides) or whatever
    ctypes passes as void* (c_void_p, byref(...), a ctypes array or pointer)."""
    kind = "pointer"
    ready = (type(None), ctypes.c_void_p, type(ctypes.byref(ctypes.c_int())))   # what ctypes passes as it is (the cheap exit)

    @staticmethod
    def from_param(v):
        if type(v) in _P.ready:
            return v
        return ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else ctypes.c_void_p.from_param(v)


def _integer(kind, ctype):
    """An integer parameter of C type `kind`: anything with __index__ (int, bool, numpy integer) or a ctypes integer.  A
    value that does not fit is refused (plain ctypes argtypes would mask it to the low bits), and so is a float."""
    def from_param(v):
        if isinstance(v, ctype):
            return v
        i = v if type(v) is int else operator.index(v.value if isinstance(v, ctypes._SimpleCData) else v)
        c = ctype(i)
        if c.value != i:                                    # (ctypes kept the low bits only)
            raise OverflowError(f"{i} does not fit the C type {kind}")
        return c
    return type(kind, (), {"kind": kind, "from_param": staticmethod(from_param)})


_I, _L, _Z, _U = (_integer(*kc) for kc in (("int", ctypes.c_int), ("long", ctypes.c_long), ("size_t", ctypes.c_size_t),
                                            ("unsigned long long", ctypes.c_ulonglong)))
_D, _INT, _SIZE = ctypes.c_double, ctypes.c_int, ctypes.c_size_t

# header under include/ -> {name: (return type, parameter types)} of every function it declares, in the header's order.
# vgg_ba_phase, called four to eight times per LM iteration, has ctypes' own types: converted in C, at the price that its
# caller wraps the workspace (_lib.ptr) and that an out-of-range phase number would be masked, not refused.
HEADERS = {
    "vggsfm_amd.h": {
        "vgg_build_arch": (ctypes.c_char_p, []),
        "vgg_abi_version": (_INT, []),
        "vgg_abi_sizeof": (_SIZE, [_I]),
        "vgg_project_points": (_INT, [_P, _I, _P, _P, _P, _I, _I, _P, _P, _P]),
        "vgg_filter_points_workspace_bytes": (_SIZE, [_I]),
        "vgg_filter_points": (_INT, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _D, _D, _I, _D, _D, _P, _P, _P, _P]),
        "vgg_cam_from_img_workspace_bytes": (_SIZE, [_I, _I, _I]),
        "vgg_cam_from_img": (_INT, [_P, _I, _P, _P, _I, _I, _I, _P, _I, _D, _D, _D, _P, _P, _P]),
        "vgg_triangulate_chunks_workspace_bytes": (_SIZE, [_I, _I]),
        "vgg_triangulate_tracks_chunks": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _D, _P, _P, _P, _P, _P, _P]),
        "vgg_triangulate_tracks_chunks_enqueue": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _D, _P, _P, _P, _P, _P, _P, _P]),
        "vgg_triangulate_by_pair": (_INT, [_P, _P, _I, _I, _P, _P]),
        "vgg_triangulate_workspace_bytes": (_SIZE, [_I, _I, _I, _I]),
        "vgg_triangulate_tracks": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _D, _P, _P, _P, _P, _P, _P]),
        "vgg_ba_workspace_bytes": (_SIZE, [_P, _P]),
        "vgg_ba_solve": (_INT, [_P, _P, _P, _Z, _P, _P, _I, _P]),
        "vgg_ba_begin": (_INT, [_P, _P, _P, _Z, _I, _I, _P]),
        "vgg_ba_phase": (_INT, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
        "vgg_ba_reduce_buffer": (_INT, [_P, _P, _P, _I, _P, _P]),
        "vgg_ba_finish": (_INT, [_P, _P, _P, _P, _P, _I, _P]),
        "vgg_ba_poll_done": (_INT, [_P, _P, _P, _P, _P]),
        "vgg_pose_refine": (_INT, [_P, _P, _I, _P, _I, _I, _P, _I, _P, _P, _P, _I, _P, _P, _I, _D, _P, _P]),
        "vgg_p3p_ransac_workspace_bytes": (_SIZE, [_I, _I]),
        "vgg_p3p_ransac": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
        "vgg_fmat_seven_point": (_INT, [_P, _P, _P, _I, _I, _I, _P, _P, _P]),
        "vgg_fmat_score": (_INT, [_P, _P, _P, _P, _P, _I, _I, _I, _D, _P, _P, _P]),
        "vgg_fmat_eight_point": (_INT, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P, _P]),
        "vgg_fmat_residuals": (_INT, [_P, _P, _P, _P, _I, _I, _P, _P]),
        "vgg_ba_tuning": (_INT, [_I, _I, _I, _I]),
        "vgg_ba_set_tile_rhs": (_INT, [_I]),
        "vgg_ba_profile": (_INT, [_I, _I]),
        "vgg_ba_profile_read": (_INT, [_I, _P, _P, _I]),
        "vgg_cholesky_workspace_bytes": (_SIZE, [_I]),
        "vgg_cholesky_solve": (_INT, [_P, _P, _I, _P, _P, _P]),
        "vgg_cholesky_solve_split": (_INT, [_P, _P, _I, _I, _I, _P, _P, _P]),
        "vgg_cholesky_solve_envelope": (_INT, [_P, _P, _I, _P, _P, _P, _P]),
        "vgg_sparse_depth": (_INT, [_P, _P, _P, _P, _P, _P, _L, _P, _P, _P]),
        "vgg_depth_align_workspace_bytes": (_SIZE, [_L]),
        "vgg_depth_align": (_INT, [_P, _P, _P, _P, _P, _P, _I, _L, _P, _I, _U, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
        "vgg_depth_apply": (_INT, [_P, _P, _P, _P, _P, _I, _L, _P, _P, _P]),
        "vgg_depth_unproject": (_INT, [_P, _P, _L, _P, _P, _P, _P, _P, _P, _P]),
        "vgg_reproj_stats_workspace_bytes": (_SIZE, [_L]),
        "vgg_reproj_stats": (_INT, [_P, _P, _L, _I, _P, _P, _Z, _P]),
        "vgg_reproj_visible": (_INT, [_P, _P, _P, _P, _P, _P, _I, _I, _L, _L, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
        "vgg_reproj_draw": (_INT, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
        "vgg_color_gather": (_INT, [_P, _I, _I, _I, _I, _I, _P, _L, _L, _P, _P, _L, _P, _P, _P]),
        "vgg_color_reduce": (_INT, [_P, _L, _L, _P, _P, _P, _P, _P]),
        "vgg_track_owner": (_INT, [_P, _I, _P, _I, _I, _I, _I, _L, _I, _I, _I, _I, _P, _P, _P]),
        "vgg_track_resolve": (_INT, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    },
    "vggsfm_amd_multiview.h": {         # csrc/multiview.hip
        "vggx_multiview_workspace_bytes": (_SIZE, [_L, _I]),
        "vggx_view_centers": (_INT, [_P, _L, _P, _P]),
        "vggx_multiview_triangulate": (_INT, [_P, _L, _I, _P, _I, _L, _L, _P, _I, _L, _L, _P, _L, _I, _I, _I, _D, _P, _P, _P, _P,
                                              _P, _P]),
        "vggx_max_tri_angle": (_INT, [_P, _L, _I, _P, _L, _I, _I, _D, _P, _P, _P, _P]),
        "vggx_tri_angle_table": (_INT, [_P, _L, _P, _L, _I, _D, _P, _P, _P]),
        "vggx_tri_angle_pairs": (_INT, [_P, _P, _L, _P, _L, _D, _P, _P]),
        "vggx_angular_error": (_INT, [_P, _P, _P, _L, _L, _L, _I, _P, _P, _P]),
    },
    "vggsfm_amd_essential.h": {         # csrc/essential.hip
        "vgge_emat_five_point": (_INT, [_P, _P, _P, _I, _I, _I, _P, _P, _P]),
        "vgge_emat_solve": (_INT, [_P, _P, _P, _L, _I, _P, _P, _P]),
        "vgge_emat_score": (_INT, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
        "vgge_emat_refine": (_INT, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    },
    "vggsfm_amd_pnp.h": {               # csrc/epnp.hip
        "vggp_epnp_solve": (_INT, [_P, _I, _P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
        "vggp_pose_score": (_INT, [_P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P]),
        "vggp_epnp_lo": (_INT, [_P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P, _P]),
    },
    "vggsfm_amd_sim3.h": {              # csrc/sim3.hip
        "vggs_sim3_workspace_bytes": (_SIZE, [_I, _I, _I]),
        "vggs_sim3_fit": (_INT, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _Z, _P]),
        "vggs_sim3_score": (_INT, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _Z, _P]),
        "vggs_sim3_ransac": (_INT, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
        "vggs_pose_pair_errors": (_INT, [_P, _P, _I, _P, _P, _P]),
    },
    "vggsfm_amd_covariance.h": {        # csrc/covariance.hip
        "vggc_spd_inverse_workspace_bytes": (_SIZE, [_I]),
        "vggc_spd_inverse": (_INT, [_P, _I, _P, _P, _P]),
        "vggc_ba_covariance_workspace_bytes": (_SIZE, [_P, _P, _I]),
        "vggc_ba_covariance": (_INT, [_P, _P, _P, _Z, _I, _P, _P, _P, _P, _P, _P, _P]),
    },
}
SIGNATURES = {name: row for table in HEADERS.values() for name, row in table.items()}
EXPORTED = list(SIGNATURES)
COV_CAMERAS, COV_POINTS = 1, 2      # VGGC_COV_* of include/vggsfm_amd_covariance.h

_lib = None


def lib():
    """Load the HIP library or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the gfx950 HIP library has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C vggsfm_amd/csrc`). "
            "vggsfm_amd has no CPU or eager fallback.")
    L = ctypes.CDLL(LIB_PATH)
    L.vgg_build_arch.restype = ctypes.c_char_p
    arch = L.vgg_build_arch().decode()
    if arch != "gfx950":
        raise RuntimeError(f"libvggsfm_amd.so was built for {arch}, expected gfx950")
    # a stale or variant build (VGGSFM_AMD_LIB) with another struct layout would be driven with shifted pointers: refuse it
    if not hasattr(L, "vgg_abi_sizeof") or L.vgg_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: ABI version {L.vgg_abi_version()} but this binding speaks {ABI_VERSION}; rebuild "
                           "the library (`make -C vggsfm_amd/csrc`)")
    L.vgg_abi_sizeof.restype = ctypes.c_size_t
    for which, st in enumerate((BAProblem, BAOptions, BAIteration, BASummary)):
        if int(L.vgg_abi_sizeof(which)) != ctypes.sizeof(st):
            raise RuntimeError(f"{LIB_PATH}: sizeof({st.__name__}) is {int(L.vgg_abi_sizeof(which))} in the library and "
                               f"{ctypes.sizeof(st)} in the binding -- header and binding are out of step")
    bind(L, SIGNATURES)
    _lib = L
    return L


def bind(L, signatures):
    """Give every entry of a loaded library the C types of its row ({name: (return type, parameter types)})."""
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes


_side = {}


def load_side_library(path, signatures, arch_entry, what, make_dir):
    """Load the shared object of csrc/<make_dir> or fail loudly; loaded once per path.

    The rule of the side libraries, stated here once: each has a shared object, a header beside its source and a ``_lib_*``
    module with a table of its own, because the entries of every library, this one's included, are a closed, counted set
    under one prefix.  The parameter types, ``check``, ``stream_ptr`` and ``require_gpu`` are this module's, and as here there
    is NO fallback: a missing library or one built for another target raises.  A new one is a row of
    ``__graft_entry__.SIDE_LIBRARIES``; tests/test_side_libraries.py compares every row's table with its header type by type
    and with the library's symbols."""
    if path in _side:
        return _side[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the gfx950 HIP library of {what} has not been built. Run "
            f"`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C vggsfm_amd/csrc/{make_dir}`). "
            "vggsfm_amd has no CPU or eager fallback.")
    L = ctypes.CDLL(path)
    bind(L, signatures)
    arch = getattr(L, arch_entry)().decode()
    if arch != "gfx950":
        raise RuntimeError(f"{os.path.basename(path)} was built for {arch}, expected gfx950")
    _side[path] = L
    return L


def check(rc, what):
    if rc != VGG_OK:
        raise RuntimeError(f"{what} failed: {_ERRORS.get(rc, rc)}")


def ptr(t):
    """Device (or host) address of a tensor as void*; None -> NULL."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def reduce_buffer(problem, options, workspace, which):
    """(device address, number of doubles) of reduce buffer `which` of a BA workspace (vgg_ba_reduce_buffer); `problem` and
    `options` by reference, as the entry takes them."""
    address, count = ctypes.c_void_p(), ctypes.c_size_t()
    check(lib().vgg_ba_reduce_buffer(problem, options, workspace, which, ctypes.byref(address), ctypes.byref(count)),
          "vgg_ba_reduce_buffer")
    return address.value or 0, count.value


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("vggsfm_amd kernels need tensors on an MI355X (cuda) device; there is no CPU path")
