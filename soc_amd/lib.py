"""ctypes binding of libsoc_hip.so (include/soc_hip.h) and a thin ``Engine`` object.

The engine is the HIP library and nothing else: if the library cannot be loaded or no GPU
is present the constructor raises -- there is no CPU fallback in the product path.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBNAME = os.path.join(HERE, "libsoc_hip.so")

TALLY_TABS = 0
TALLY_INT = 1
TALLY_XAB = 2
TALLY_INTX, TALLY_INTY, TALLY_INTZ = 3, 4, 5      # with_int == 2 (SAVE_INTENSITY 2)

SOC_OK, SOC_ERR_ARG, SOC_ERR_STATE, SOC_ERR_HIP = 0, -1, -2, -3      # include/soc_hip.h

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
_U = C.POINTER(C.c_uint32)

# every symbol include/soc_hip.h declares: (restype, argtypes)
API = {
    "soc_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "soc_destroy": (None, [C.c_void_p]),
    "soc_last_error": (C.c_char_p, [C.c_void_p]),
    "soc_version": (C.c_char_p, []),
    "soc_device_bytes": (C.c_int64, []),
    "soc_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "soc_set_grid": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _I, _F]),
    "soc_set_features": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "soc_set_exec": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "soc_last_form": (C.c_int, [C.c_void_p]),
    "soc_last_variant": (C.c_int, [C.c_void_p]),
    "soc_set_tuning": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "soc_last_passes": (C.c_int, [C.c_void_p]),
    "soc_set_optical": (C.c_int, [C.c_void_p, _F, _F, C.c_int]),
    "soc_set_opt": (C.c_int, [C.c_void_p, _F]),
    "soc_set_scatter_table": (C.c_int, [C.c_void_p, _F, _F, C.c_int]),
    "soc_set_opt_half": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_set_scatter_tables": (C.c_int, [C.c_void_p, C.c_int, _F, _F, C.c_int]),
    "soc_set_step_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "soc_set_emission": (C.c_int, [C.c_void_p, _F, _F]),
    "soc_set_emindex": (C.c_int, [C.c_void_p, _I]),
    "soc_set_ali": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_zero": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_sim_pb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                             _F, _F, C.c_int, _I, _I, _F, C.c_int, C.c_int, C.c_int]),
    "soc_sim_cl": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                             C.c_int, C.c_int, C.c_int]),
    "soc_sim_bg_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int]),
    "soc_sim_hp_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]),
    "soc_split_skipped": (C.c_int64, [C.c_void_p]),
    "soc_split_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "soc_split_max_depth": (C.c_int64, [C.c_void_p]),
    "soc_batch_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_batch_end": (C.c_int, [C.c_void_p]),
    "soc_batch_begin_int": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_batch_begin_shared_int": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_batch_begin_int_groups": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_batch_next_int": (C.c_int, [C.c_void_p]),
    "soc_batch_read_int": (C.c_int, [C.c_void_p, C.c_int, _F, C.c_long]),
    "soc_set_mirror": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_set_hpbg": (C.c_int, [C.c_void_p, _F, _F]),
    "soc_set_abundances": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _F]),
    "soc_set_optical_abu": (C.c_int, [C.c_void_p, _F, _F, C.c_int]),
    "soc_read_opt": (C.c_int, [C.c_void_p, _F]),
    "soc_set_roi_save": (C.c_int, [C.c_void_p, _I, C.c_int, C.c_int]),
    "soc_roi_zero": (C.c_int, [C.c_void_p]),
    "soc_roi_read": (C.c_int, [C.c_void_p, _F, C.c_long]),
    "soc_set_roi_load": (C.c_int, [C.c_void_p, _I, C.c_int, _F]),
    "soc_sim_hp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]),
    "soc_sca_set_view": (C.c_int, [C.c_void_p, C.c_int, _F, _F, _F, C.c_int, C.c_int, C.c_float, _F, C.c_int]),
    "soc_sca_set_healpix": (C.c_int, [C.c_void_p, C.c_int, _F, C.c_int]),
    "soc_sca_sim_hp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]),
    "soc_sca_zero": (C.c_int, [C.c_void_p]),
    "soc_sca_sim_ps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, _F, _F, C.c_int, _I, _I, _F,
                                 C.c_int, C.c_int, C.c_int]),
    "soc_sca_sim_pb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _F, _F, C.c_int,
                                 _I, _I, _F, C.c_int, C.c_int, C.c_int]),
    "soc_sca_sim_cl": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]),
    "soc_sca_read_out": (C.c_int, [C.c_void_p, _F, C.c_int64]),
    "soc_sca_out_ptr": (C.c_void_p, [C.c_void_p]),
    "soc_sca_batch_images": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_sca_batch_select": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_sca_batch_read": (C.c_int, [C.c_void_p, C.c_int, _F, C.c_int64]),
    "soc_sca_bind_out": (C.c_int, [C.c_void_p, C.c_void_p]),
    "soc_sync": (C.c_int, [C.c_void_p]),
    "soc_read_tally": (C.c_int, [C.c_void_p, C.c_int, _F, C.c_int64]),
    "soc_write_tally": (C.c_int, [C.c_void_p, C.c_int, _F, C.c_int64]),
    "soc_tally_ptr": (C.c_void_p, [C.c_void_p, C.c_int]),
    "soc_bind_tally": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "soc_read_par": (C.c_int, [C.c_void_p, _I, C.c_int64]),
    "soc_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "soc_sca_ray_steps": (C.c_int64, [C.c_void_p]),
    "soc_timer_start": (C.c_int, [C.c_void_p]),
    "soc_timer_stop": (C.c_int, [C.c_void_p, _F]),
    "soc_solve_temperature": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, _F, C.c_float, C.c_float, _F, _F]),
    "soc_set_cr_heating": (C.c_int, [C.c_void_p, C.c_float]),
    "soc_set_map_threshold": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_set_map_interpolation": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_a2e_pre": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, _F, _F, _F, _F, _F, _I, _I, _F, _I, _F]),
    "soc_set_map_roi": (C.c_int, [C.c_void_p, _I]),
    "soc_set_temperature": (C.c_int, [C.c_void_p, _F]),
    "soc_emission": (C.c_int, [C.c_void_p, C.c_int, _F, _F, C.c_float, C.c_float, _F]),
    "soc_map": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, _F, _F, _F, _F, _F, _F, C.c_float, C.c_float, C.c_int,
                          C.c_float, _F, _F]),
    "soc_map_levels": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, _F, _F, _F, _F, _F, _F, C.c_float, C.c_float, _F]),
    "soc_map_block_max": (C.c_int, []),
    "soc_map_set_block": (C.c_int, [C.c_void_p, C.c_int, _F, _F, _F, _F]),
    "soc_map_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, _F, _F, _F, _F, _F, C.c_float, _F, _F, _F]),
    "soc_map_block_levels": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, _F, _F, _F, _F, _F, _F]),
    "soc_map_block_levels_width": (C.c_int, [C.c_void_p]),
    "soc_set_bfield": (C.c_int, [C.c_void_p, _F, _F, _F]),
    "soc_polmap": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, _F, _F, _F, _F, _F,
                             C.c_float, C.c_float, C.c_float, _F]),
    "soc_polmap_healpix": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, _F, _F,
                                     C.c_float, C.c_float, C.c_float, _F]),
    "soc_ps_tau": (C.c_int, [C.c_void_p, C.c_int, _F, _F, C.c_float, C.c_float, C.c_float, _F, _F]),
    "soc_a2e_set_size": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _F, _I, _I, _F, _F, _I, _F]),
    "soc_a2e_launch_shape": (C.c_int, [C.c_void_p, _I]),
    "soc_a2e_solve": (C.c_int, [C.c_void_p, C.c_int, _F, _F]),
    "soc_a2e_upload": (C.c_int, [C.c_void_p, C.c_int, _F]),
    "soc_a2e_run": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_a2e_download": (C.c_int, [C.c_void_p, C.c_int, _F]),
    "soc_a2e_resident_begin": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "soc_a2e_resident_upload": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_a2e_resident_solve": (C.c_int, [C.c_void_p]),
    "soc_a2e_resident_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_a2e_resident_end": (C.c_int, [C.c_void_p]),
    "soc_a2e_resident_begin_pol": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    "soc_a2e_resident_upload_aalg": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F, _F]),
    "soc_a2e_set_size_aalg": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]),
    "soc_a2e_resident_download_p": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_a2e_set_eq_sizes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, _F, _F, _F, _F, _F, _F, _F, C.c_float, _F, _F]),
    "soc_a2e_resident_solve_eq": (C.c_int, [C.c_void_p]),
    "soc_a2e_eqtemp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                 C.c_float, C.c_float, _F, _F, _F, _F, _F, _F]),
    "soc_eqsolver": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                               C.c_float, C.c_float, _F, _F, _F, _F, _F, _F]),
    "soc_mabu_begin": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "soc_mabu_upload": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_mabu_set_tables": (C.c_int, [C.c_void_p, _F, C.POINTER(C.c_double)]),
    "soc_mabu_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "soc_mabu_solve_eq": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _F, _F, _F]),
    "soc_mabu_accumulate": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_mabu_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_mabu_read_part": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_mabu_end": (C.c_int, [C.c_void_p]),
    "soc_mabu_begin_pol": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "soc_mabu_pol_eq": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "soc_mabu_accumulate_p": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_mabu_ratio": (C.c_int, [C.c_void_p]),
    "soc_mabu_download_p": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_mabu_download_t": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_a2e_resident_keep_teq": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_a2e_resident_download_teq": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, _F]),
    "soc_a2e_solve_dump": (C.c_int, [C.c_void_p, C.c_int, _F, _F, _F]),
    "soc_a2e_resident_solve_dump": (C.c_int, [C.c_void_p, _F]),
    "soc_emitted_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_emitted_upload": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_emitted_from_mabu": (C.c_int, [C.c_void_p, C.c_int64]),
    "soc_emitted_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_set_emission_column": (C.c_int, [C.c_void_p, C.c_int, _F]),
    "soc_read_emission": (C.c_int, [C.c_void_p, _F, C.c_int64]),
    "soc_emitted_end": (C.c_int, [C.c_void_p]),
    "soc_emitted_change": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), _F, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "soc_emitted_read_luminosity": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_double)]),
    "soc_absorbed_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "soc_absorbed_add_tally": (C.c_int, [C.c_void_p, C.c_int]),
    "soc_absorbed_add_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "soc_absorbed_keep": (C.c_int, [C.c_void_p]),
    "soc_absorbed_restore": (C.c_int, [C.c_void_p]),
    "soc_absorbed_to_mabu": (C.c_int, [C.c_void_p, C.c_int64, _F, C.c_float]),
    "soc_absorbed_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F, _F, C.c_float]),
    "soc_absorbed_end": (C.c_int, [C.c_void_p]),
    "soc_library_set": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, _F, _F, _F, _F, _F, _F, _F, _F, C.c_int, _I]),
    "soc_library_solve": (C.c_int, [C.c_void_p, C.c_int64, _F, _F, _I, C.POINTER(C.c_int64)]),
    "soc_library_solve_resident": (C.c_int, [C.c_void_p, _I, _I, C.POINTER(C.c_int64)]),
    "soc_library_build": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, _F, _I, _F, _F, _F, _F, _F, _F, _I, _F, _F, _F]),
    "soc_mabu_library_begin": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "soc_mabu_library_set": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _F, _F, _F, _F, _F, _F, _F, _F, C.c_int, _I]),
    "soc_mabu_library_upload": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_mabu_library_set_tables": (C.c_int, [C.c_void_p, _F, C.POINTER(C.c_double)]),
    "soc_mabu_library_solve": (C.c_int, [C.c_void_p]),
    "soc_mabu_library_download": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _F]),
    "soc_mabu_library_misses": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _U]),
    "soc_mabu_library_end": (C.c_int, [C.c_void_p]),
    "soc_mabu_gather_rows": (C.c_int, [C.c_void_p, _I, C.c_int64, _F]),
    "soc_probe_rng": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_int, _U, _U]),
    "soc_probe_math": (C.c_int, [C.c_void_p, C.c_int, _F, _F, C.c_int64]),
    "soc_probe_math2": (C.c_int, [C.c_void_p, C.c_int, _F, _F, _F, C.c_int64]),
    "soc_probe_trace": (C.c_int, [C.c_void_p, _F, _F, C.c_int, _I, _I, _F, _F, _I]),
}

_lib = None

VARIANT_FORMS = ("direct", "cartesian", "global_tree", "brick_local")


def decode_variant(code):
    """soc_last_variant's code (bit layout: include/soc_hip.h) as a dict; None for -1 (no kernel has run)"""
    code = int(code)
    if code < 0:
        return None
    return dict(form=code & 3, kind=(code >> 2) & 7, wint=(code >> 5) & 3, octree=(code >> 7) & 1, dbl=(code >> 8) & 1,
                abu=(code >> 9) & 1, ali=(code >> 10) & 1, rays=(code >> 11) & 1, healpix=(code >> 12) & 1, hpsky=(code >> 13) & 1,
                split=(code >> 14) & 1, sca=(code >> 15) & 1, code=code)


class SocError(RuntimeError):
    pass


class DoesNotFit(SocError):
    """mabu_begin: the cells do not fit the free device memory; cells_fit of them would.  emitted_begin: the resident emission does
    not fit (cells_fit 0: it is held for all cells or not at all); absorbed_begin: nor do the resident absorptions"""

    def __init__(self, text, cells_fit):
        SocError.__init__(self, text)
        self.cells_fit = int(cells_fit)


def _torch_runtime_first():
    """torch ships its own copy of the HIP runtime (torch/lib/libamdhip64.so, without a soname), libsoc_hip.so is linked against the
    system's (libamdhip64.so.7): a process that uses both holds two runtimes, and the one initialised second finds no device.
    With torch's runtime loaded first both work -- so where torch is installed it is imported before libsoc_hip.so is opened,
    whatever the order of the caller's own imports.  (Without torch there is one runtime and nothing to do.)"""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        if importlib.util.find_spec("torch") is not None:
            import torch                                   # noqa: F401
    except Exception:                                      # a broken torch installation must not stop a run that does not need it
        pass


def load_library(path=None):
    """dlopen libsoc_hip.so and declare every prototype.  Raises SocError if it is missing.
    Safe to call before or after `import torch` (see _torch_runtime_first)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    _torch_runtime_first()
    path = path or LIBNAME
    if not os.path.exists(path):
        raise SocError("%s not found: build it with `python -m soc_amd.build` "
                       "(there is no CPU fallback)" % path)
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise SocError("cannot load %s: %s" % (path, e))
    for name, (res, args) in API.items():
        fn = getattr(lib, name)          # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_bytes():
    """Bytes of device memory the engines of this process hold (soc_device_bytes): their own allocations, the packet records, queues
    and bricks of their brick sweeps included; not a caller's bound tensors."""
    return int(load_library().soc_device_bytes())


def _f(a):
    return None if a is None else a.ctypes.data_as(_F)


def _i(a):
    return None if a is None else a.ctypes.data_as(_I)


def _rows_out(who, n, NFREQ, out):
    """the rows [n, NFREQ] that a download fills: new ones, or the caller's `out` -- the library writes n x NFREQ floats to whatever it gets"""
    if out is None:
        return np.zeros((max(int(n), 0), NFREQ), np.float32)
    if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable and out.shape == (int(n), NFREQ)):
        raise SocError("%s: out must be a writeable C-contiguous float32 array of shape (%d, %d)" % (who, int(n), NFREQ))
    return out


def _vector_out(who, n, out):
    """the n floats that a download of one value per cell fills: new ones, or the caller's `out`"""
    if out is None:
        return np.zeros(max(int(n), 0), np.float32)
    if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable and out.shape == (int(n),)):
        raise SocError("%s: out must be a writeable C-contiguous float32 array of shape (%d,)" % (who, int(n)))
    return out


def _view_vectors(*vectors):
    """(DIR, RA, DE, CENTRE, INTOBS) of a map call as the float3 the C ABI takes: three contiguous floats each, None kept"""
    return [None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).ravel()[:3]) for a in vectors]


class Engine:
    """One GPU's packet engine.  Method names follow the C ABI one to one."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.soc_create(int(device), C.byref(h))
        if rc != 0:
            raise SocError("soc_create(device=%d) failed: %s" %
                           (device, self.lib.soc_last_error(None).decode()))
        self.h = h
        self.device = int(device)
        self.CELLS = 0
        self.NPAR = 0
        self.LEVELS = 0
        self._a2e_res = (0, 0)                             # (cells, NFREQ) of the resident block of the last a2e_resident_begin or mabu_begin
        self._mabu = None                                  # (cells, NFREQ, NDUST) between mabu_begin and mabu_end
        self._emitted = None                               # NFREQ between emitted_begin and emitted_end (set_grid ends it)
        self._absorbed = None                              # NFREQ between absorbed_begin and absorbed_end (set_grid ends it)

    def close(self):
        if getattr(self, "h", None):
            self.lib.soc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise SocError("%s (code %d)" % (self.lib.soc_last_error(self.h).decode(), rc))

    # ---- model ----
    def set_stream(self, stream_ptr):
        self._chk(self.lib.soc_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_grid(self, NX, NY, NZ, LEVELS, LCELLS, DENS):
        LCELLS = np.ascontiguousarray(LCELLS, np.int32)
        DENS = np.ascontiguousarray(DENS, np.float32)
        if len(LCELLS) < LEVELS or DENS.size != int(LCELLS[:LEVELS].sum()):
            raise SocError("set_grid: DENS has %d values, LCELLS sums to %d" % (DENS.size, int(LCELLS[:LEVELS].sum())))
        self._chk(self.lib.soc_set_grid(self.h, int(NX), int(NY), int(NZ), int(LEVELS), _i(LCELLS), _f(DENS)))
        self.CELLS = int(DENS.size)
        self.NPAR = self.CELLS - int(NX) * int(NY) * int(NZ)
        self.LEVELS = int(LEVELS)
        self._emitted = None
        self._absorbed = None

    def set_cloud(self, cloud):
        self.set_grid(cloud.NX, cloud.NY, cloud.NZ, cloud.LEVELS, cloud.LCELLS, cloud.DENS)

    def set_features(self, with_int=0, ps_method=0, use_emweight=0):
        self._chk(self.lib.soc_set_features(self.h, int(with_int), int(ps_method), int(use_emweight)))

    def batch_begin(self, max_launches=0):
        """Defer the following sim_pb launches and run them together (brick sweep, TABS only)."""
        self._chk(self.lib.soc_batch_begin(self.h, int(max_launches)))

    def batch_begin_int(self, max_launches=0):
        """like batch_begin, for launches that keep the per-frequency INT tally: each deferred launch gets its own;
        read them with batch_read_int(k) after batch_end"""
        self._chk(self.lib.soc_batch_begin_int(self.h, int(max_launches)))

    def batch_begin_shared_int(self, max_launches=0):
        """Launches until batch_end() that keep the INT tally are deferred too and tally into the handle's INT buffer together:
        the source blocks of one frequency (zero(1) before, read_tally(1) after)."""
        self._chk(self.lib.soc_batch_begin_shared_int(self.h, int(max_launches)))

    def batch_begin_int_groups(self, max_groups=0):
        """As batch_begin_int, but the launches between two batch_next_int() calls -- the source blocks of one frequency -- share an
        INT tally; batch_read_int(k) reads the k-th group's after batch_end()."""
        self._chk(self.lib.soc_batch_begin_int_groups(self.h, int(max_groups)))

    def batch_next_int(self):
        self._chk(self.lib.soc_batch_next_int(self.h))

    def batch_read_int(self, k):
        out = np.zeros(self.CELLS, np.float32)
        self._chk(self.lib.soc_batch_read_int(self.h, int(k), _f(out), out.size))
        return out

    def batch_end(self):
        self._chk(self.lib.soc_batch_end(self.h))

    def set_mirror(self, mask=0):
        """reflecting faces, bits x,X,y,Y,z,Z = 1,2,4,8,16,32"""
        self._chk(self.lib.soc_set_mirror(self.h, int(mask)))

    def set_exec(self, mode=-1, brick_log2=4):
        """0 direct kernel, 1 brick sweep (LDS tallies), -1 automatic."""
        self._chk(self.lib.soc_set_exec(self.h, int(mode), int(brick_log2)))

    def last_form(self):
        """0 direct kernel, 1 brick sweep (Cartesian), 2 hierarchy in global memory, 3 brick-local hierarchies"""
        return int(self.lib.soc_last_form(self.h))

    def last_variant(self):
        """the compiled kernel of the last launch or sweep (absorption, packet splitting `split`, direct scattered light `sca`):
        decode_variant(soc_last_variant), None before any ran"""
        return decode_variant(self.lib.soc_last_variant(self.h))

    def set_tuning(self, **params):
        """shape of the brick sweep (soc_set_tuning): threads, chunk, steps_per_visit, swap_lanes, climb_lanes,
        brick_cells, brick_partition (brick-local hierarchies: 1 the tiles of 16^3 root cells alone, 2 -- and 0 -- the partition with the
        smaller total face area), tail_lanes, park_below, population, hash_slots, general_kernel, oversubscribe, verbose, abu_local
        (1: launches with per-cell opacities take the brick-local walk of a hierarchy that has one), float_local (1: hierarchies
        whose Index() runs in float -- NX <= 100, or <= 399 with two levels -- take the brick-local walk too, in its float form);
        0 = built-in"""
        for k, v in params.items():
            self._chk(self.lib.soc_set_tuning(self.h, k.encode(), int(v)))

    def last_passes(self):
        return int(self.lib.soc_last_passes(self.h))

    def set_optical(self, ABS, SCA):
        a = np.asarray([ABS], np.float32).ravel()
        s = np.asarray([SCA], np.float32).ravel()
        self._chk(self.lib.soc_set_optical(self.h, _f(a), _f(s), 1))

    def set_opt(self, OPT):
        if OPT is None:
            self._chk(self.lib.soc_set_opt(self.h, None))
            return
        OPT = np.ascontiguousarray(OPT, np.float32)
        if OPT.size != 2 * self.CELLS:
            raise SocError("set_opt: OPT must hold 2*CELLS floats")
        self._chk(self.lib.soc_set_opt(self.h, _f(OPT)))

    def set_abundances(self, ABU, single=False):
        """abundances once per run: ABU[CELLS, NDUST], or ABU[CELLS] with single=True (two species, ABU and 1-ABU);
        None forgets them.  set_optical_abu then builds OPT on the device for every frequency."""
        if ABU is None:
            self._chk(self.lib.soc_set_abundances(self.h, 0, 0, None))
            return
        ABU = np.ascontiguousarray(ABU, np.float32)
        ndust = 2 if single else (ABU.shape[1] if ABU.ndim == 2 else 1)
        if ABU.size != self.CELLS * (1 if single else ndust):
            raise SocError("set_abundances: ABU must hold CELLS x NDUST values")
        self._chk(self.lib.soc_set_abundances(self.h, int(ndust), int(bool(single)), _f(ABU)))

    def set_optical_abu(self, AFABS, AFSCA):
        a = np.ascontiguousarray(AFABS, np.float32).ravel()
        s = np.ascontiguousarray(AFSCA, np.float32).ravel()
        self._chk(self.lib.soc_set_optical_abu(self.h, _f(a), _f(s), int(a.size)))

    def set_cr_heating(self, rate):
        """-D CR_HEATING_RATE (with -D CR_HEATING=1): added to the absorbed energy in solve_temperature; 0 = off"""
        self._chk(self.lib.soc_set_cr_heating(self.h, float(rate)))

    def set_map_interpolation(self, mode):
        """-D MAP_INTERPOLATION (ini key mapint): 1 | 2 = flat maps blend every cell on the ray with two neighbours; 0 = off"""
        self._chk(self.lib.soc_set_map_interpolation(self.h, int(mode)))

    def set_map_threshold(self, level):
        """-D LEVEL_THRESHOLD: flat maps leave out the emission of coarser levels; 0 = off"""
        self._chk(self.lib.soc_set_map_threshold(self.h, int(level)))

    def set_map_roi(self, ROI):
        """-D ROI_MAP: maps of the emission inside ROI = [x0,x1,y0,y1,z0,z1] only; None = all cells"""
        r = None if ROI is None else np.ascontiguousarray(ROI, np.int32)
        self._chk(self.lib.soc_set_map_roi(self.h, _i(r)))

    def set_opt_half(self, on=True):
        """-D OPT_IS_HALF: OPT of later set_opt / set_optical_abu calls is rounded to fp16 as the reference stores it"""
        self._chk(self.lib.soc_set_opt_half(self.h, int(bool(on))))

    def read_opt(self):
        out = np.zeros((self.CELLS, 2), np.float32)
        self._chk(self.lib.soc_read_opt(self.h, _f(out)))
        return out

    def set_scatter_table(self, DSC, CSC):
        CSC = np.ascontiguousarray(CSC, np.float32)
        DSC = None if DSC is None else np.ascontiguousarray(DSC, np.float32)
        self._chk(self.lib.soc_set_scatter_table(self.h, _f(DSC), _f(CSC), int(CSC.size)))

    def set_scatter_tables(self, DSC, CSC):
        """-D WITH_MSF: CSC[NDUST, BINS] (and DSC) per dust species; needs set_abundances + set_optical_abu per frequency"""
        CSC = np.ascontiguousarray(CSC, np.float32)
        if CSC.ndim != 2:
            raise SocError("set_scatter_tables: CSC[NDUST, BINS]")
        DSC = None if DSC is None else np.ascontiguousarray(DSC, np.float32)
        if DSC is not None and DSC.shape != CSC.shape:
            raise SocError("set_scatter_tables: DSC and CSC differ in shape")
        self._chk(self.lib.soc_set_scatter_tables(self.h, int(CSC.shape[0]), _f(DSC), _f(CSC), int(CSC.shape[1])))

    def set_step_weight(self, mode, SW_A=0.0, SW_B=0.0):
        """values of -D STEP_WEIGHT, -D SW_A, -D SW_B (kernel_ASOC.c:516-535); mode 0 = off"""
        self._chk(self.lib.soc_set_step_weight(self.h, int(mode), float(SW_A), float(SW_B)))

    def set_emission(self, EMIT, EMWEI=None):
        EMIT = np.ascontiguousarray(EMIT, np.float32)
        EMWEI = None if EMWEI is None else np.ascontiguousarray(EMWEI, np.float32)
        if EMIT.size != self.CELLS or (EMWEI is not None and EMWEI.size != self.CELLS):
            raise SocError("set_emission: arrays must hold CELLS floats")
        self._chk(self.lib.soc_set_emission(self.h, _f(EMIT), _f(EMWEI)))

    def set_emindex(self, EMINDEX):
        EMINDEX = np.ascontiguousarray(EMINDEX, np.int32)
        if EMINDEX.size != self.CELLS:
            raise SocError("set_emindex: EMINDEX must hold CELLS ints")
        self._chk(self.lib.soc_set_emindex(self.h, _i(EMINDEX)))

    def set_ali(self, with_ali=1):
        self._chk(self.lib.soc_set_ali(self.h, int(with_ali)))

    # ---- launches ----
    def zero(self, tag):
        self._chk(self.lib.soc_zero(self.h, int(tag)))

    def sim_pb(self, SOURCE, PACKETS, BATCH, SEED, BG, TW, PSPOS=None, PS=None, XPS=None,
               GLOBAL=None, gid_first=0, gid_count=None):
        NO_PS = 0
        pspos = ps = nside = side = area = None
        if SOURCE == 0:
            p = np.asarray(PSPOS, np.float32)
            if p.ndim == 1:
                p = p.reshape(-1, 3)
            NO_PS = p.shape[0]
            pspos = np.zeros((NO_PS, 4), np.float32)
            pspos[:, :3] = p[:, :3]
            ps = np.ascontiguousarray(PS, np.float32)
            if XPS is not None:
                nside = np.ascontiguousarray(XPS[0], np.int32)
                side = np.ascontiguousarray(XPS[1], np.int32)
                area = np.ascontiguousarray(XPS[2], np.float32)
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sim_pb(self.h, int(SOURCE), int(PACKETS), int(BATCH), np.float32(SEED),
                                      np.float32(BG), np.float32(TW), _f(pspos), _f(ps), NO_PS,
                                      _i(nside), _i(side), _f(area), int(GLOBAL), int(gid_first), int(gid_count)))

    def sim_bg_split(self, PACKETS, BATCH, SEED, BG, TW, SELEM, max_split=0, GLOBAL=None, gid_first=0, gid_count=None):
        """isotropic background with packet splitting (`split 1`, SimBgSplit): BATCH root rays from each of the SELEM surface
        elements of a work item; max_split 0 = the reference's 4300 stack entries per work item"""
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sim_bg_split(self.h, int(PACKETS), int(BATCH), np.float32(SEED), np.float32(BG), np.float32(TW),
                                            int(SELEM), int(max_split), int(GLOBAL), int(gid_first), int(gid_count)))

    def sim_hp_split(self, PACKETS, BATCH, SEED, TW, max_split=0, GLOBAL=None, gid_first=0, gid_count=None):
        """Healpix sky (set_hpbg) with packet splitting (`split 1` + `hpbg`, SimHpSplit): BATCH root rays per work item;
        max_split 0 = the reference's 4300 stack entries per work item"""
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sim_hp_split(self.h, int(PACKETS), int(BATCH), np.float32(SEED), np.float32(TW),
                                            int(max_split), int(GLOBAL), int(gid_first), int(gid_count)))

    SPLIT_COUNTERS = ("roots", "splits", "deep_splits", "ended_below_RL", "overflow_drops", "long_returns")

    def split_stats(self, reset=False):
        """counters of the sim_bg_split and sim_hp_split launches since the last reset (SPLIT_COUNTERS, summed over work items),
        max_depth, the largest number of stack entries a work item held, and skipped_splits, the splits sim_hp_split launches
        skipped on a nearly full stack"""
        out = (C.c_uint64 * 6)()
        self._chk(self.lib.soc_split_stats(self.h, out, int(reset)))
        st = {k: int(out[i]) for i, k in enumerate(self.SPLIT_COUNTERS)}
        st["max_depth"] = int(self.lib.soc_split_max_depth(self.h))
        st["skipped_splits"] = int(self.lib.soc_split_skipped(self.h))
        return st

    def sim_cl(self, SOURCE, PACKETS, BATCH, SEED, TW, GLOBAL, gid_first=0, gid_count=None):
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sim_cl(self.h, int(SOURCE), int(PACKETS), int(BATCH), np.float32(SEED),
                                      np.float32(TW), int(GLOBAL), int(gid_first), int(gid_count)))

    def set_hpbg(self, BG, HPBGP=None):
        """Healpix sky of the current frequency (49152 pixels, photons per package); HPBGP = cumulative
        pixel probability for weighted sampling."""
        BG = np.ascontiguousarray(BG, np.float32)
        HPBGP = None if HPBGP is None else np.ascontiguousarray(HPBGP, np.float32)
        if BG.size != 49152 or (HPBGP is not None and HPBGP.size != 49152):
            raise SocError("set_hpbg: the sky map must hold 49152 pixels (NSIDE 64)")
        self._chk(self.lib.soc_set_hpbg(self.h, _f(BG), _f(HPBGP)))

    # ---- region of interest (nested runs) ----
    def set_roi_save(self, ROI, ROI_STEP=1, ROI_NSIDE=16):
        """record the packets that step into ROI = [x0,x1,y0,y1,z0,z1] (root cells, inclusive) during sim_pb / sim_cl;
        ROI=None turns recording off.  Returns the number of record entries."""
        if ROI is None:
            self._chk(self.lib.soc_set_roi_save(self.h, None, 0, 0))
            self._roi_n = 0
            return 0
        ROI = np.ascontiguousarray(ROI, np.int32)
        if ROI.size != 6:
            raise SocError("set_roi_save: ROI = [x0, x1, y0, y1, z0, z1]")
        self._chk(self.lib.soc_set_roi_save(self.h, ROI.ctypes.data_as(_I), int(ROI_STEP), int(ROI_NSIDE)))
        n = [(int(ROI[2 * i + 1]) - int(ROI[2 * i]) + 1) * int(ROI_STEP) for i in range(3)]
        self._roi_n = (n[0] * n[1] + n[1] * n[2] + n[2] * n[0]) * 12 * int(ROI_NSIDE) ** 2
        return self._roi_n

    def roi_zero(self):
        self._chk(self.lib.soc_roi_zero(self.h))

    def roi_read(self):
        out = np.zeros(getattr(self, "_roi_n", 0), np.float32)
        self._chk(self.lib.soc_roi_read(self.h, _f(out), out.size))
        return out

    def set_roi_load(self, DIM, ROI_NSIDE, LOAD):
        """the record of one frequency to send in with sim_pb(SOURCE=3): LOAD[nelem, 12*NSIDE^2] photons on the
        (nx, ny, nz) = DIM surface discretisation; LOAD=None turns it off"""
        if LOAD is None:
            self._chk(self.lib.soc_set_roi_load(self.h, None, 0, None))
            return
        DIM = np.ascontiguousarray(DIM, np.int32)
        LOAD = np.ascontiguousarray(LOAD, np.float32)
        nelem = int(DIM[0]) * int(DIM[1]) + int(DIM[1]) * int(DIM[2]) + int(DIM[2]) * int(DIM[0])
        if DIM.size != 3 or LOAD.size != nelem * 12 * int(ROI_NSIDE) ** 2:
            raise SocError("set_roi_load: LOAD must hold %d x %d values" % (nelem, 12 * int(ROI_NSIDE) ** 2))
        self._chk(self.lib.soc_set_roi_load(self.h, DIM.ctypes.data_as(_I), int(ROI_NSIDE), _f(LOAD)))

    def sim_hp(self, PACKETS, BATCH, SEED, TW, GLOBAL, gid_first=0, gid_count=None):
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sim_hp(self.h, int(PACKETS), int(BATCH), np.float32(SEED), np.float32(TW), int(GLOBAL),
                                      int(gid_first), int(gid_count)))

    # ---- equilibrium temperature and emission ----
    def solve_temperature(self, adhoc, kE, Emin, TTT, FACTOR, LENGTH, EABS):
        """EABS[CELLS]: integrated absorbed energy; returns TNEW[CELLS] (kept on the device for emission())"""
        TTT = np.ascontiguousarray(TTT, np.float32)
        EABS = np.ascontiguousarray(EABS, np.float32)
        if EABS.size != self.CELLS:
            raise SocError("solve_temperature: EABS must hold CELLS floats")
        T = np.zeros(self.CELLS, np.float32)
        self._chk(self.lib.soc_solve_temperature(self.h, np.float32(adhoc), np.float32(kE), np.float32(Emin), int(TTT.size), _f(TTT),
                                                 np.float32(FACTOR), np.float32(LENGTH), _f(EABS), _f(T)))
        return T

    def set_temperature(self, T):
        T = np.ascontiguousarray(T, np.float32)
        if T.size != self.CELLS:
            raise SocError("set_temperature: T must hold CELLS floats")
        self._chk(self.lib.soc_set_temperature(self.h, _f(T)))

    def emission(self, FREQ, FABS, FACTOR, LENGTH):
        """EMITTED[CELLS, nfreq] (FACTOR x photons/Hz/cm3) at the device temperatures"""
        FREQ = np.ascontiguousarray(FREQ, np.float32)
        FABS = np.ascontiguousarray(FABS, np.float32)
        out = np.zeros((self.CELLS, FREQ.size), np.float32)
        self._chk(self.lib.soc_emission(self.h, int(FREQ.size), _f(FREQ), _f(FABS), np.float32(FACTOR), np.float32(LENGTH), _f(out)))
        return out

    # ---- map making ----
    def map(self, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, INTOBS=None, save_colden=0, LENGTH=1.0, healpix=0):
        """One map (kernel_ASOC_map.c Mapping / HealpixMapping).  Returns (MAP, SAVETAU): [NPIX.y, NPIX.x] or [12*NSIDE^2]."""
        EMIT = np.ascontiguousarray(EMIT, np.float32)
        if EMIT.size != self.CELLS:
            raise SocError("map: EMIT must hold CELLS floats")
        v = _view_vectors(DIR, RA, DE, CENTRE, INTOBS)
        nx, ny = (int(healpix), 1) if healpix else (int(NPIX[0]), int(NPIX[1]))
        shape = (12 * nx * nx,) if healpix else (ny, nx)
        MAP, TAU = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        self._chk(self.lib.soc_map(self.h, int(bool(healpix)), nx, ny, np.float32(MAP_DX), _f(EMIT), _f(v[0]), _f(v[1]), _f(v[2]),
                                   _f(v[3]), _f(v[4]), np.float32(ABS), np.float32(SCA), int(save_colden), np.float32(LENGTH),
                                   _f(MAP), _f(TAU)))
        return MAP, TAU

    @property
    def map_block_max(self):
        """the most frequencies one set_map_block batch may hold (soc_map_block_max)"""
        return int(self.lib.soc_map_block_max())

    def set_map_block(self, EMITX, ABS=None, SCA=None, OPT=None):
        """One batch of frequencies for map_block, resident on the device until the next call: EMITX[CELLS, nf] emission,
        ABS[nf] and SCA[nf] scalar opacities, OPT[CELLS, nf, 2] per-cell opacities used instead when given (the OPT of
        set_opt plays no part in map_block).  set_map_block(None) frees the batch."""
        if EMITX is None:
            self._chk(self.lib.soc_map_set_block(self.h, 0, None, None, None, None))
            self._map_block_nf = 0
            return
        EMITX = np.ascontiguousarray(EMITX, np.float32)
        if EMITX.ndim != 2 or EMITX.shape[0] != self.CELLS or EMITX.shape[1] < 1:
            raise SocError("set_map_block: EMITX must be [CELLS, nf] with nf >= 1")
        nf = int(EMITX.shape[1])
        ABS = np.ascontiguousarray(ABS, np.float32).ravel()
        SCA = np.ascontiguousarray(SCA, np.float32).ravel()
        if ABS.size != nf or SCA.size != nf:
            raise SocError("set_map_block: ABS and SCA must hold one value per frequency (%d)" % nf)
        if OPT is not None:
            OPT = np.ascontiguousarray(OPT, np.float32)
            if OPT.shape != (self.CELLS, nf, 2):
                raise SocError("set_map_block: OPT must be [CELLS, nf, 2]")
        # (a refused call leaves the resident batch, and so the plane count map_block allocates for, as it was)
        self._chk(self.lib.soc_map_set_block(self.h, nf, _f(EMITX), _f(ABS), _f(SCA), _f(OPT)))
        self._map_block_nf = nf

    def map_block(self, DIR, RA, DE, NPIX, MAP_DX, CENTRE, INTOBS=None, LENGTH=1.0, healpix=0):
        """The maps of the resident batch for one view, from one walk per pixel (the arguments and switches of map).  Returns
        (MAPX, TAUX, COLDEN): [nf, NPIX.y, NPIX.x] twice and [NPIX.y, NPIX.x] -- or [nf, 12*NSIDE^2] and [12*NSIDE^2]; plane f
        of MAPX and TAUX is what map gives for frequency f, COLDEN what it gives as SAVETAU with save_colden=1."""
        v = _view_vectors(DIR, RA, DE, CENTRE, INTOBS)
        nx, ny = (int(healpix), 1) if healpix else (int(NPIX[0]), int(NPIX[1]))
        shape = (12 * nx * nx,) if healpix else (max(ny, 0), max(nx, 0))
        nf = getattr(self, "_map_block_nf", 0)
        MAPX, TAUX = np.zeros((nf,) + shape, np.float32), np.zeros((nf,) + shape, np.float32)
        COLDEN = np.zeros(shape, np.float32)
        self._chk(self.lib.soc_map_block(self.h, int(bool(healpix)), nx, ny, np.float32(MAP_DX), _f(v[0]), _f(v[1]), _f(v[2]), _f(v[3]),
                                         _f(v[4]), np.float32(LENGTH), _f(MAPX), _f(TAUX), _f(COLDEN)))
        return MAPX, TAUX, COLDEN

    def map_block_levels(self, DIR, RA, DE, NPIX, MAP_DX, CENTRE, INTOBS=None, healpix=0):
        """The levels of the plain map (`maplevels 1`) for the resident batch and one view, with the arguments and switches of
        map_block: [nf, LEVELS, NPIX.y, NPIX.x] -- or [nf, LEVELS, 12*NSIDE^2] with healpix = NSIDE.  Plane (f, l) is, bit for
        bit, what map gives for frequency f when the emission of every cell not on level l is 0: what level l emits towards the
        pixel, seen through everything in front of it.  The planes of a pixel add up to map_block's value up to the order of
        the additions.  The batch is read, not changed.  Not the reference's per-level product: that is map_levels."""
        v = _view_vectors(DIR, RA, DE, CENTRE, INTOBS)
        nx, ny = (int(healpix), 1) if healpix else (int(NPIX[0]), int(NPIX[1]))
        shape = (12 * nx * nx,) if healpix else (max(ny, 0), max(nx, 0))
        nf = getattr(self, "_map_block_nf", 0)
        MAPL = np.zeros((nf, self.LEVELS) + shape, np.float32)
        self._chk(self.lib.soc_map_block_levels(self.h, int(bool(healpix)), nx, ny, np.float32(MAP_DX), _f(v[0]), _f(v[1]), _f(v[2]),
                                                _f(v[3]), _f(v[4]), _f(MAPL)))
        return MAPL

    @property
    def map_block_levels_width(self):
        """the most frequencies one launch of map_block_levels' kernel takes for the model set (wider batches: several launches)"""
        w = int(self.lib.soc_map_block_levels_width(self.h))
        if w < 1:
            self._chk(w)
        return w

    def map_levels(self, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, INTOBS=None):
        """One image per hierarchy level (the Mapping of kernel_ASOC_map_H.c, `mapping nx ny dx 999`): [LEVELS, NPIX.y, NPIX.x],
        plane l the emission of the cells of level l seen through everything in front of them.  INTOBS: the longitude x latitude
        image seen from that position instead of the orthographic map.  `mapint`, `threshold` and `roimap` (set_map_interpolation,
        set_map_threshold, set_map_roi) have no effect here, as in the reference."""
        EMIT = np.ascontiguousarray(EMIT, np.float32)
        if EMIT.size != self.CELLS:
            raise SocError("map_levels: EMIT must hold CELLS floats")
        v = _view_vectors(DIR, RA, DE, CENTRE, INTOBS)
        nx, ny = int(NPIX[0]), int(NPIX[1])
        MAP = np.zeros((self.LEVELS, max(ny, 0), max(nx, 0)), np.float32)
        self._chk(self.lib.soc_map_levels(self.h, nx, ny, np.float32(MAP_DX), _f(EMIT), _f(v[0]), _f(v[1]), _f(v[2]), _f(v[3]), _f(v[4]),
                                          np.float32(ABS), np.float32(SCA), _f(MAP)))
        return MAP

    def set_bfield(self, Bx, By=None, Bz=None):
        """The magnetic field of the polarisation maps: three arrays of CELLS floats (cloud-file order, parents included).
        set_bfield(None) frees it."""
        if Bx is None:
            self._chk(self.lib.soc_set_bfield(self.h, None, None, None))
            return
        B = [np.ascontiguousarray(b, np.float32).ravel() for b in (Bx, By, Bz)]
        if any(b.size != self.CELLS for b in B):
            raise SocError("set_bfield: Bx, By and Bz must hold CELLS floats each")
        self._chk(self.lib.soc_set_bfield(self.h, _f(B[0]), _f(B[1]), _f(B[2])))

    def polmap(self, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, polstat=0, polred=0, rho_weight=0, p0=0.2, LENGTH=1.0):
        """One polarisation map (kernel_ASOC_map.c PolMapping): [4, NPIX.y, NPIX.x] = I, Q, U, column density (polstat 0),
        rT, rI, jT, jI (polstat 1) or <B>, <B_LOS>, <B_POS>, tau (polstat 3)."""
        EMIT = np.ascontiguousarray(EMIT, np.float32)
        if EMIT.size != self.CELLS:
            raise SocError("polmap: EMIT must hold CELLS floats")
        v = [np.ascontiguousarray(np.asarray(a, np.float32).ravel()[:3]) for a in (DIR, RA, DE, CENTRE)]
        nx, ny = int(NPIX[0]), int(NPIX[1])
        MAP = np.zeros((4, max(ny, 0), max(nx, 0)), np.float32)
        self._chk(self.lib.soc_polmap(self.h, int(polstat), int(polred), int(rho_weight), np.float32(p0), nx, ny, np.float32(MAP_DX),
                                      _f(EMIT), _f(v[0]), _f(v[1]), _f(v[2]), _f(v[3]), np.float32(ABS), np.float32(SCA),
                                      np.float32(LENGTH), _f(MAP)))
        return MAP

    def polmap_healpix(self, EMIT, NSIDE, INTOBS, ABS, SCA, polred=0, p0=0.2, interpolate=0, minlos=-1.0, maxlos=1e10, y_shear=0.0,
                       LENGTH=1.0):
        """One all-sky polarisation map seen from INTOBS (kernel_ASOC_map_H.c PolHealpixMapping, POLSTAT 0):
        [4, 12*NSIDE^2] = I, Q, U, column density in RING order."""
        EMIT = np.ascontiguousarray(EMIT, np.float32)
        if EMIT.size != self.CELLS:
            raise SocError("polmap_healpix: EMIT must hold CELLS floats")
        obs = np.ascontiguousarray(np.asarray(INTOBS, np.float32).ravel()[:3])
        if obs.size != 3:
            raise SocError("polmap_healpix: INTOBS must hold three floats")
        nside = int(NSIDE)
        MAP = np.zeros((4, 12 * max(nside, 0) ** 2), np.float32)
        self._chk(self.lib.soc_polmap_healpix(self.h, nside, int(polred), np.float32(p0), int(interpolate), np.float32(minlos),
                                              np.float32(maxlos), np.float32(y_shear), _f(EMIT), _f(obs), np.float32(ABS), np.float32(SCA),
                                              np.float32(LENGTH), _f(MAP)))
        return MAP

    def ps_tau(self, PSPOS, DIR, ABS, SCA, LENGTH=1.0):
        """PSTau: (column density * LENGTH, optical depth) from every point source towards the observer direction DIR"""
        P = np.zeros((len(PSPOS), 4), np.float32)
        P[:, :3] = np.asarray(PSPOS, np.float32)[:, :3]
        d = np.ascontiguousarray(np.asarray(DIR, np.float32).ravel()[:3])
        col, tau = np.zeros(len(P), np.float32), np.zeros(len(P), np.float32)
        self._chk(self.lib.soc_ps_tau(self.h, len(P), _f(P), _f(d), np.float32(ABS), np.float32(SCA), np.float32(LENGTH), _f(col), _f(tau)))
        return col, tau

    # ---- scattered-light images (ASOCS) ----
    @staticmethod
    def _sources(PSPOS, PS, XPS):
        p = np.asarray(PSPOS, np.float32)
        if p.ndim == 1:
            p = p.reshape(-1, p.size // max(1, np.asarray(PS).size))
        pspos = np.zeros((p.shape[0], 4), np.float32)
        pspos[:, :3] = p[:, :3]
        ps = np.ascontiguousarray(PS, np.float32)
        nside = side = area = None
        if XPS is not None:
            nside = np.ascontiguousarray(XPS[0], np.int32)
            side = np.ascontiguousarray(XPS[1], np.int32)
            area = np.ascontiguousarray(XPS[2], np.float32)
        return pspos, ps, nside, side, area

    def sca_set_view(self, ODIR, RA, DE, NPIX, MAP_DX, CENTRE, FFS=1):
        """ODIR, RA, DE: [NDIR,4] float32 (launch.set_observer_directions); NPIX = (x, y)."""
        ODIR, RA, DE = (np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in (ODIR, RA, DE))
        cen = np.asarray(CENTRE, np.float32).ravel()[:3].copy()
        self.sca_shape = (len(ODIR), int(NPIX[1]), int(NPIX[0]))
        self._chk(self.lib.soc_sca_set_view(self.h, len(ODIR), _f(ODIR), _f(RA), _f(DE), int(NPIX[0]), int(NPIX[1]),
                                            np.float32(MAP_DX), _f(cen), int(FFS)))

    def sca_set_healpix(self, NSIDE, OBSERVER, FFS=1):
        """one Healpix map (RING) of scattered light seen from the position OBSERVER [root-grid units]"""
        obs = np.asarray(OBSERVER, np.float32).ravel()[:3].copy()
        self.sca_shape = (12 * int(NSIDE) * int(NSIDE),)
        self._chk(self.lib.soc_sca_set_healpix(self.h, int(NSIDE), _f(obs), int(FFS)))

    def sca_sim_hp(self, PACKETS, BATCH, SEED, GLOBAL, gid_first=0, gid_count=None):
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sca_sim_hp(self.h, int(PACKETS), int(BATCH), np.float32(SEED), int(GLOBAL), int(gid_first),
                                          int(gid_count)))

    def sca_zero(self):
        self._chk(self.lib.soc_sca_zero(self.h))

    def sca_sim_ps(self, PACKETS, BATCH, SEED, BG, PSPOS, PS, XPS=None, GLOBAL=None, gid_first=0, gid_count=None):
        pspos, ps, nside, side, area = self._sources(PSPOS, PS, XPS)
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sca_sim_ps(self.h, int(PACKETS), int(BATCH), np.float32(SEED), np.float32(BG), _f(pspos), _f(ps),
                                          len(ps), _i(nside), _i(side), _f(area), int(GLOBAL), int(gid_first), int(gid_count)))

    def sca_sim_pb(self, SOURCE, PACKETS, BATCH, SEED, BG, PSPOS=None, PS=None, XPS=None, GLOBAL=None, gid_first=0,
                   gid_count=None):
        pspos = ps = nside = side = area = None
        NO_PS = 0
        if SOURCE == 0:
            pspos, ps, nside, side, area = self._sources(PSPOS, PS, XPS)
            NO_PS = len(ps)
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sca_sim_pb(self.h, int(SOURCE), int(PACKETS), int(BATCH), np.float32(SEED), np.float32(BG),
                                          _f(pspos), _f(ps), NO_PS, _i(nside), _i(side), _f(area), int(GLOBAL),
                                          int(gid_first), int(gid_count)))

    def sca_sim_cl(self, SOURCE, PACKETS, BATCH, SEED, GLOBAL, gid_first=0, gid_count=None):
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self._chk(self.lib.soc_sca_sim_cl(self.h, int(SOURCE), int(PACKETS), int(BATCH), np.float32(SEED), int(GLOBAL),
                                          int(gid_first), int(gid_count)))

    def sca_read_out(self):
        out = np.zeros(self.sca_shape, np.float32)
        self._chk(self.lib.soc_sca_read_out(self.h, _f(out), out.size))
        return out

    def sca_out_ptr(self):
        return self.lib.soc_sca_out_ptr(self.h)

    def sca_batch_images(self, n):
        """n zeroed images for the scattered-light launches of a batch (batch_begin ... batch_end), 0 = the one image again"""
        self._chk(self.lib.soc_sca_batch_images(self.h, int(n)))

    def sca_batch_select(self, k):
        self._chk(self.lib.soc_sca_batch_select(self.h, int(k)))

    def sca_batch_read(self, k):
        out = np.zeros(self.sca_shape, np.float32)
        self._chk(self.lib.soc_sca_batch_read(self.h, int(k), _f(out), out.size))
        return out

    def sca_bind_out(self, device_ptr):
        self._chk(self.lib.soc_sca_bind_out(self.h, C.c_void_p(device_ptr) if device_ptr else None))

    def sync(self):
        self._chk(self.lib.soc_sync(self.h))

    # ---- results ----
    def read_tally(self, which=TALLY_TABS):
        out = np.zeros(self.CELLS, np.float32)
        self._chk(self.lib.soc_read_tally(self.h, int(which), _f(out), self.CELLS))
        return out

    def write_tally(self, which, values):
        v = np.ascontiguousarray(values, np.float32)
        self._chk(self.lib.soc_write_tally(self.h, int(which), _f(v), v.size))

    def tally_ptr(self, which=TALLY_TABS):
        return self.lib.soc_tally_ptr(self.h, int(which))

    def bind_tally(self, which, device_ptr, n=None):
        """caller-owned device memory (n floats, default CELLS) as tally `which`; device_ptr None/0 = back to the library's"""
        if not device_ptr:
            self._chk(self.lib.soc_bind_tally(self.h, int(which), None, 0))
        else:
            self._chk(self.lib.soc_bind_tally(self.h, int(which), C.c_void_p(device_ptr), int(self.CELLS if n is None else n)))

    def read_par(self):
        out = np.zeros(max(self.NPAR, 1), np.int32)
        self._chk(self.lib.soc_read_par(self.h, _i(out), self.NPAR))
        return out[:self.NPAR]

    def stats(self, reset=False):
        out = (C.c_uint64 * 3)()
        self._chk(self.lib.soc_stats(self.h, out, int(reset)))
        return dict(tally_events=int(out[0]), packets=int(out[1]), scatterings=int(out[2]))

    def sca_ray_steps(self):
        """cell steps of the rays of the scattered-light sweeps, as of the last stats() call"""
        return int(self.lib.soc_sca_ray_steps(self.h))

    def timer_start(self):
        self._chk(self.lib.soc_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.lib.soc_timer_stop(self.h, C.byref(ms)))
        return float(ms.value)

    # ---- A2E ----
    def a2e_pre(self, FREQ, Ef, SKABS, E, T, FACTOR):
        """One grain size of a solver file (A2E_pre.py:233-256): integration weights and cooling rates on the enthalpy grid
        E[NE+1] (temperatures T[NE+1]); SKABS = pi a^2 Q_abs per grain.  Returns dict(Iw (packed as in the file), L1, L2, Tdown)."""
        FREQ, Ef, SKABS = (np.ascontiguousarray(a, np.float32) for a in (FREQ, Ef, SKABS))
        E, T = np.ascontiguousarray(E, np.float32), np.ascontiguousarray(T, np.float32)
        NFREQ, NE = FREQ.size, E.size - 1
        if Ef.size != NFREQ or SKABS.size != NFREQ or T.size != NE + 1:
            raise SocError("a2e_pre: Ef, SKABS must hold NFREQ floats, E and T NE+1")
        L1, L2 = np.zeros(NE * NE, np.int32), np.zeros(NE * NE, np.int32)
        Iw, noIw, Tdown = np.zeros(NE * NE * NFREQ, np.float32), np.zeros(NE - 1, np.int32), np.zeros(NE, np.float32)
        self._chk(self.lib.soc_a2e_pre(self.h, int(NFREQ), int(NE), np.float32(FACTOR), _f(FREQ), _f(Ef), _f(SKABS), _f(E), _f(T),
                                       _i(L1), _i(L2), _f(Iw), _i(noIw), _f(Tdown)))
        packed = np.concatenate([Iw[l * NE * NFREQ:l * NE * NFREQ + noIw[l]] for l in range(NE - 1)]) if NE > 1 else Iw[:0]
        L1[0] = -2                                         # A2E_pre.py:246, :249
        L2[0] = -2
        return dict(Iw=packed, L1=L1, L2=L2, Tdown=Tdown, noIw=noIw)

    def a2e_set_size(self, NE, NFREQ, size, AF):
        """size: dict with Iw, L1, L2, Tdown, EA, Ibeg of one grain size (solver file)."""
        a = {k: np.ascontiguousarray(size[k], t) for k, t in (("Iw", np.float32), ("L1", np.int32), ("L2", np.int32),
                                                                ("Tdown", np.float32), ("EA", np.float32), ("Ibeg", np.int32))}
        AF = np.ascontiguousarray(AF, np.float32)
        if a["L1"].size != NE * NE or a["L2"].size != NE * NE or a["Tdown"].size != NE or a["EA"].size != NE * NFREQ \
                or a["Ibeg"].size != NFREQ or AF.size != NFREQ:
            raise SocError("a2e_set_size: array sizes do not match NE=%d NFREQ=%d" % (NE, NFREQ))
        self._chk(self.lib.soc_a2e_set_size(self.h, int(NE), int(NFREQ), int(a["Iw"].size), _f(a["Iw"]), _i(a["L1"]),
                                            _i(a["L2"]), _f(a["Tdown"]), _f(a["EA"]), _i(a["Ibeg"]), _f(AF)))
        self._a2e_nfreq = NFREQ                              # (a refused size leaves the one before in place)
        self._a2e_ne = int(NE)

    def a2e_launch_shape(self):
        """(cells per workgroup, threads per workgroup, dynamic LDS bytes) of DoSolve for the size of the last a2e_set_size."""
        out = np.zeros(3, np.int32)
        self._chk(self.lib.soc_a2e_launch_shape(self.h, _i(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def a2e_solve(self, AABS):
        AABS = np.ascontiguousarray(AABS, np.float32)
        out = np.zeros_like(AABS)
        self._chk(self.lib.soc_a2e_solve(self.h, AABS.shape[0], _f(AABS), _f(out)))
        return out

    def a2e_solve_dump(self, AABS):
        """a2e_solve that also returns the populations of the enthalpy levels, clamped to [1e-35, 10] as the reference's DUMP_TDUST
        build leaves them: (EMIT[batch, NFREQ], X[batch, NE]); EMIT has the bits of a2e_solve"""
        AABS = np.ascontiguousarray(AABS, np.float32)
        NE = getattr(self, "_a2e_ne", 0)
        if NE < 1:
            raise SocError("a2e_solve_dump: call a2e_set_size first")
        if AABS.ndim != 2 or AABS.shape[0] < 1 or AABS.shape[1] != self._a2e_nfreq:
            raise SocError("a2e_solve_dump: an array of shape %s for rows of %d frequencies" % (AABS.shape, self._a2e_nfreq))
        out, X = np.zeros_like(AABS), np.zeros((AABS.shape[0], NE), np.float32)
        self._chk(self.lib.soc_a2e_solve_dump(self.h, AABS.shape[0], _f(AABS), _f(out), _f(X)))
        return out, X

    def a2e_upload(self, AABS):
        AABS = np.ascontiguousarray(AABS, np.float32)
        self._chk(self.lib.soc_a2e_upload(self.h, AABS.shape[0], _f(AABS)))

    # the cells resident in device memory: absorptions up once, the sum over the sizes down once (soc_a2e_resident_*)
    def a2e_resident_begin(self, cells, NFREQ, polarised=False):
        """polarised: also a second, weighted sum for the polarised emission (a2e_resident_upload_aalg, a2e_set_size_aalg,
        a2e_resident_download_p)"""
        if polarised:
            self._chk(self.lib.soc_a2e_resident_begin_pol(self.h, int(cells), int(NFREQ), 1))
        else:
            self._chk(self.lib.soc_a2e_resident_begin(self.h, int(cells), int(NFREQ)))
        self._a2e_res = (int(cells), int(NFREQ))

    def a2e_resident_upload_aalg(self, c0, aalg):
        """rows [c0, c0 + len(aalg)) of the minimum aligned grain size; its log10 is numpy's float32 one (A2E.py:425)"""
        aalg = np.ascontiguousarray(aalg, np.float32)
        if aalg.ndim != 1 or aalg.size < 1:
            raise SocError("a2e_resident_upload_aalg: one value per cell, an array of shape %s was given" % (aalg.shape,))
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.ascontiguousarray(np.log10(aalg), np.float32)
        self._chk(self.lib.soc_a2e_resident_upload_aalg(self.h, int(c0), aalg.size, _f(aalg), _f(lg)))

    def a2e_set_size_aalg(self, ASIZE, isize):
        """the weights of size `isize` of the solver file's ASIZE for the polarised sum, after a2e_set_size (which clears them)"""
        ASIZE = np.asarray(ASIZE, np.float32)
        last = isize >= ASIZE.size - 1
        lg = np.log10(ASIZE[isize])
        step = np.float32(0.0) if last else np.log10(ASIZE[isize + 1]) - lg
        self._chk(self.lib.soc_a2e_set_size_aalg(self.h, ASIZE[isize], np.float32(0.0) if last else ASIZE[isize + 1], np.float32(lg), np.float32(step)))

    def a2e_resident_download_p(self, c0, n, out=None):
        out = _rows_out("a2e_resident_download_p", n, self._a2e_res[1], out)
        self._chk(self.lib.soc_a2e_resident_download_p(self.h, int(c0), int(n), _f(out)))
        return out

    def a2e_resident_upload(self, c0, AABS):
        AABS = np.ascontiguousarray(AABS, np.float32)
        if AABS.ndim != 2 or AABS.shape[1] != self._a2e_res[1]:
            raise SocError("a2e_resident_upload: an array of shape %s for rows of %d frequencies" % (AABS.shape, self._a2e_res[1]))
        self._chk(self.lib.soc_a2e_resident_upload(self.h, int(c0), AABS.shape[0], _f(AABS)))

    def a2e_resident_solve(self):
        self._chk(self.lib.soc_a2e_resident_solve(self.h))

    def a2e_resident_solve_dump(self, out=None):
        """a2e_resident_solve that also returns X[cells, NE], the clamped populations of the current size in every resident cell (read
        back chunk by chunk: the device holds those of one chunk); out: a C-contiguous float32 array [cells, NE] to fill"""
        NE = getattr(self, "_a2e_ne", 0)
        if NE < 1 or self._a2e_res[0] < 1:
            raise SocError("a2e_resident_solve_dump: call a2e_resident_begin (or mabu_begin) and a2e_set_size first")
        X = _rows_out("a2e_resident_solve_dump", self._a2e_res[0], NE, out)
        self._chk(self.lib.soc_a2e_resident_solve_dump(self.h, _f(X)))
        return X

    def a2e_set_eq_sizes(self, NIP, FACTOR, FREQ, AF, KABS, TTT, Emin, kE, oplgkE, GD, S_FRAC, SIZE_A=None):
        """the tables of the equilibrium sizes of a dust, in the order in which a2e_resident_solve_eq adds their emission: AF, KABS
        [nsizes, NFREQ], TTT[nsizes, NIP], Emin, kE, oplgkE, S_FRAC [nsizes]; SIZE_A[nsizes]: they also add to the polarised sum"""
        AF, KABS, TTT = (np.ascontiguousarray(a, np.float32) for a in (AF, KABS, TTT))
        FREQ, Emin, kE, oplgkE, S_FRAC = (np.ascontiguousarray(a, np.float32).ravel() for a in (FREQ, Emin, kE, oplgkE, S_FRAC))
        SIZE_A = None if SIZE_A is None else np.ascontiguousarray(SIZE_A, np.float32).ravel()
        if AF.ndim != 2:
            raise SocError("a2e_set_eq_sizes: AF[nsizes, NFREQ], an array of shape %s was given" % (AF.shape,))
        ns, NFREQ = AF.shape
        if KABS.shape != (ns, NFREQ) or TTT.shape != (ns, int(NIP)) or FREQ.size != NFREQ or \
                any(a.size != ns for a in (Emin, kE, oplgkE, S_FRAC)) or (SIZE_A is not None and SIZE_A.size != ns):
            raise SocError("a2e_set_eq_sizes: array sizes do not match nsizes=%d NFREQ=%d NIP=%d" % (ns, NFREQ, NIP))
        self._chk(self.lib.soc_a2e_set_eq_sizes(self.h, ns, NFREQ, int(NIP), np.float32(FACTOR), _f(FREQ), _f(AF), _f(KABS), _f(TTT),
                                                _f(Emin), _f(kE), _f(oplgkE), np.float32(GD), _f(S_FRAC), _f(SIZE_A)))

    def a2e_resident_solve_eq(self):
        """the sizes of a2e_set_eq_sizes on the resident cells (a2e_resident_begin or mabu_begin), added to the sum after the
        stochastic sizes' a2e_resident_solve calls"""
        self._chk(self.lib.soc_a2e_resident_solve_eq(self.h))

    def a2e_resident_keep_teq(self, on=True):
        """on: every a2e_resident_solve_eq of this resident block also keeps the temperature of every (size, cell) for
        a2e_resident_download_teq; the block's end (a2e_resident_end, mabu_end) switches it off"""
        self._chk(self.lib.soc_a2e_resident_keep_teq(self.h, int(bool(on))))

    def a2e_resident_download_teq(self, slot, c0, n, out=None):
        """T[n] of the cells [c0, c0 + n) for size number `slot` of the last a2e_set_eq_sizes, after an a2e_resident_solve_eq that
        kept them; out: a C-contiguous float32 array [n] to fill"""
        out = _vector_out("a2e_resident_download_teq", n, out)
        self._chk(self.lib.soc_a2e_resident_download_teq(self.h, int(slot), int(c0), int(n), _f(out)))
        return out

    def a2e_resident_download(self, c0, n, out=None):
        out = _rows_out("a2e_resident_download", n, self._a2e_res[1], out)
        self._chk(self.lib.soc_a2e_resident_download(self.h, int(c0), int(n), _f(out)))
        return out

    def a2e_resident_end(self):
        self._chk(self.lib.soc_a2e_resident_end(self.h))

    def a2e_run(self, batch):
        self._chk(self.lib.soc_a2e_run(self.h, int(batch)))

    def a2e_download(self, batch):
        out = np.zeros((batch, self._a2e_nfreq), np.float32)
        self._chk(self.lib.soc_a2e_download(self.h, int(batch), _f(out)))
        return out

    def eqsolver(self, icell, CELLS, NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, ABS):
        """SolveEquilibriumDust of A2E_MABU.py for one batch: ABS[batch, NFREQ] -> T[batch], EMIT[batch, NFREQ]"""
        ABS = np.ascontiguousarray(ABS, np.float32)
        batch, NFREQ = ABS.shape
        FREQ, KABS, TTT = (np.ascontiguousarray(a, np.float32) for a in (FREQ, KABS, TTT))
        T = np.zeros(batch, np.float32)
        E = np.zeros((batch, NFREQ), np.float32)
        self._chk(self.lib.soc_eqsolver(self.h, batch, int(icell), int(CELLS), NFREQ, int(NE), np.float32(FACTOR),
                                        np.float32(kE), np.float32(oplgkE), np.float32(Emin), _f(FREQ), _f(KABS),
                                        _f(TTT), _f(ABS), _f(T), _f(E)))
        return T, E

    def a2e_eqtemp(self, icell, CELLS, NIP, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, ABS):
        ABS = np.ascontiguousarray(ABS, np.float32)
        batch, NFREQ = ABS.shape
        FREQ, KABS, TTT = (np.ascontiguousarray(a, np.float32) for a in (FREQ, KABS, TTT))
        T = np.zeros(batch, np.float32)
        E = np.zeros((batch, NFREQ), np.float32)
        self._chk(self.lib.soc_a2e_eqtemp(self.h, batch, int(icell), int(CELLS), NFREQ, int(NIP), np.float32(FACTOR),
                                          np.float32(kE), np.float32(oplgkE), np.float32(Emin), _f(FREQ), _f(KABS),
                                          _f(TTT), _f(ABS), _f(T), _f(E)))
        return T, E

    # ---- the multi-dust stage with the cells resident in device memory (soc_mabu_*; driven by soc_amd.mabu.solve_emission) ----
    def mabu_begin(self, cells, NFREQ, NDUST, polarised=False):
        """polarised: also the arrays of the `polarisation` lines (mabu_pol_eq, mabu_accumulate_p, mabu_ratio, mabu_download_p)"""
        fit = C.c_int64(0)
        if polarised:
            rc = self.lib.soc_mabu_begin_pol(self.h, int(cells), int(NFREQ), int(NDUST), 1, C.byref(fit))
        else:
            rc = self.lib.soc_mabu_begin(self.h, int(cells), int(NFREQ), int(NDUST), C.byref(fit))
        if rc == SOC_ERR_STATE and 0 < fit.value < int(cells):    # with a cell count: not enough device memory
            raise DoesNotFit("%s (code %d)" % (self.lib.soc_last_error(self.h).decode(), rc), fit.value)
        self._chk(rc)
        self._mabu = (int(cells), int(NFREQ), int(NDUST))
        self._a2e_res = self._mabu[:2]                     # (the dust's share and its emission are the arrays of a2e_resident_*)

    def _mabu_open(self, who):
        """(cells, NFREQ, NDUST) of the open mabu_begin"""
        if self._mabu is None:
            raise SocError("%s: call mabu_begin first" % who)
        return self._mabu

    def mabu_upload(self, c0, ABS):
        NFREQ = self._mabu_open("mabu_upload")[1]
        ABS = np.ascontiguousarray(ABS, np.float32)
        if ABS.ndim != 2 or ABS.shape[1] != NFREQ:
            raise SocError("mabu_upload: an array of shape %s for rows of %d frequencies" % (ABS.shape, NFREQ))
        self._chk(self.lib.soc_mabu_upload(self.h, int(c0), ABS.shape[0], _f(ABS)))

    def mabu_set_tables(self, ABU, RABS):
        cells, NFREQ, NDUST = self._mabu_open("mabu_set_tables")
        ABU, RABS = np.ascontiguousarray(ABU, np.float32), np.ascontiguousarray(RABS, np.float64)
        if ABU.shape != (cells, NDUST) or RABS.shape != (NFREQ, NDUST):
            raise SocError("mabu_set_tables: ABU%s, RABS%s for %d cells, %d frequencies, %d dusts" % (ABU.shape, RABS.shape, cells, NFREQ, NDUST))
        self._chk(self.lib.soc_mabu_set_tables(self.h, _f(ABU), RABS.ctypes.data_as(C.POINTER(C.c_double))))

    def mabu_split(self, idust, clip_last=False):
        self._chk(self.lib.soc_mabu_split(self.h, int(idust), int(bool(clip_last))))

    def mabu_solve_eq(self, NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT):
        NFREQ = self._mabu_open("mabu_solve_eq")[1]
        FREQ, KABS, TTT = (np.ascontiguousarray(a, np.float32) for a in (FREQ, KABS, TTT))
        if FREQ.size != NFREQ or KABS.size != NFREQ or TTT.size != int(NE):
            raise SocError("mabu_solve_eq: FREQ, KABS must hold %d floats, TTT %d" % (NFREQ, int(NE)))
        self._chk(self.lib.soc_mabu_solve_eq(self.h, int(NE), np.float32(FACTOR), np.float32(kE), np.float32(oplgkE), np.float32(Emin),
                                             _f(FREQ), _f(KABS), _f(TTT)))

    def mabu_accumulate(self, idust):
        self._chk(self.lib.soc_mabu_accumulate(self.h, int(idust)))

    def mabu_download(self, c0, n, out=None):
        """rows [c0, c0 + n) of the sum; out: a C-contiguous float32 array [n, NFREQ] to fill (anything else is refused)"""
        out = _rows_out("mabu_download", n, self._mabu_open("mabu_download")[1], out)
        self._chk(self.lib.soc_mabu_download(self.h, int(c0), int(n), _f(out)))
        return out

    def mabu_download_t(self, c0, n, out=None):
        """T[n] of the cells [c0, c0 + n): the temperatures the last mabu_solve_eq left (the <dust>.T of A2E_MABU.py:551); out: a
        C-contiguous float32 array [n] to fill"""
        self._mabu_open("mabu_download_t")
        out = _vector_out("mabu_download_t", n, out)
        self._chk(self.lib.soc_mabu_download_t(self.h, int(c0), int(n), _f(out)))
        return out

    def mabu_pol_eq(self, apol, tab):
        """PEM = EM * ipR_f(a_alg) of an equilibrium dust: apol[NA] increasing, tab[NFREQ, NA] float64 (mabu.rpol_table)"""
        NFREQ = self._mabu_open("mabu_pol_eq")[1]
        apol, tab = np.ascontiguousarray(apol, np.float64), np.ascontiguousarray(tab, np.float64)
        if apol.ndim != 1 or tab.shape != (NFREQ, apol.size):
            raise SocError("mabu_pol_eq: apol%s, tab%s for %d frequencies" % (apol.shape, tab.shape, NFREQ))
        D = C.POINTER(C.c_double)
        self._chk(self.lib.soc_mabu_pol_eq(self.h, int(apol.size), apol.ctypes.data_as(D), tab.ctypes.data_as(D)))

    def mabu_accumulate_p(self, idust):
        self._chk(self.lib.soc_mabu_accumulate_p(self.h, int(idust)))

    def mabu_ratio(self):
        self._chk(self.lib.soc_mabu_ratio(self.h))

    def mabu_download_p(self, c0, n, out=None):
        """rows [c0, c0 + n) of the polarised sum -- after mabu_ratio, of R; out as in mabu_download"""
        out = _rows_out("mabu_download_p", n, self._mabu_open("mabu_download_p")[1], out)
        self._chk(self.lib.soc_mabu_download_p(self.h, int(c0), int(n), _f(out)))
        return out

    def mabu_read_part(self, c0, n):
        out = _rows_out("mabu_read_part", n, self._mabu_open("mabu_read_part")[1], None)
        self._chk(self.lib.soc_mabu_read_part(self.h, int(c0), int(n), _f(out)))
        return out

    def mabu_end(self):
        self._chk(self.lib.soc_mabu_end(self.h))
        self._mabu = None

    # ---- the emission of a re-emission iteration, resident for the next one's cell-emission launches (soc_emitted_*; driven by
    # soc_amd.driver through mabu.solve_emission and AbsorptionRun.simulate_cell_emission) ----
    def emitted_begin(self, NFREQ):
        """ET[NFREQ, CELLS] of the grid's cells, zeroed; DoesNotFit where the free device memory does not take it (nothing is reserved)"""
        if self.CELLS < 1:
            raise SocError("emitted_begin: call set_grid first")
        rc = self.lib.soc_emitted_begin(self.h, int(NFREQ))
        if rc == -2:                                           # (an array that is open stays as it is)
            raise DoesNotFit("%s (code %d)" % (self.lib.soc_last_error(self.h).decode(), rc), 0)
        self._chk(rc)
        self._emitted = int(NFREQ)

    def _emitted_rows(self, who, n, rows):
        """the open emitted_begin's NFREQ; rows, where given, must be a C-contiguous float32 [n, NFREQ] (a refused call must not read or
        write past a host array; the device side checks the cell range)"""
        if self._emitted is None:
            raise SocError("%s: call emitted_begin first" % who)
        if rows is not None and not (isinstance(rows, np.ndarray) and rows.dtype == np.float32 and rows.flags.c_contiguous
                                     and rows.shape == (int(n), self._emitted)):
            raise SocError("%s: a C-contiguous float32 array of shape (%d, %d) is needed" % (who, int(n), self._emitted))
        return self._emitted

    def emitted_upload(self, c0, rows):
        """rows[n, NFREQ] as the emitted file holds them -> cells [c0, c0 + n)"""
        rows = np.ascontiguousarray(rows, np.float32)
        self._emitted_rows("emitted_upload", rows.shape[0], rows)
        self._chk(self.lib.soc_emitted_upload(self.h, int(c0), rows.shape[0], _f(rows)))

    def emitted_from_mabu(self, c0):
        """the sum of the open mabu_begin, device to device -> cells [c0, c0 + its cells)"""
        self._emitted_rows("emitted_from_mabu", 0, None)
        self._chk(self.lib.soc_emitted_from_mabu(self.h, int(c0)))

    def emitted_download(self, c0, n, out=None):
        """rows [c0, c0 + n) back as [n, NFREQ]; out: a writeable C-contiguous float32 array of that shape to fill"""
        out = _rows_out("emitted_download", n, self._emitted_rows("emitted_download", 0, None), out)
        self._chk(self.lib.soc_emitted_download(self.h, int(c0), int(n), _f(out)))
        return out

    def set_emission_column(self, ifreq, COEFF):
        """the emission of the next sim_cl from frequency ifreq of the resident array: EMIT = ET[ifreq] * (COEFF[level] * DENS), 0 in
        links and empty cells; COEFF[LEVELS] float32 = GL*PARSEC/8**level/FACTOR"""
        self._emitted_rows("set_emission_column", 0, None)
        COEFF = np.ascontiguousarray(COEFF, np.float32)
        if COEFF.size != self.LEVELS:
            raise SocError("set_emission_column: COEFF must hold LEVELS = %d floats" % self.LEVELS)
        self._chk(self.lib.soc_set_emission_column(self.h, int(ifreq), _f(COEFF)))

    def read_emission(self):
        """EMIT[CELLS] as the next sim_cl would use it (tests)"""
        out = np.zeros(self.CELLS, np.float32)
        self._chk(self.lib.soc_read_emission(self.h, _f(out), self.CELLS))
        return out

    def emitted_change(self, W, COEFF):
        """the change of the resident emission since the call before (soc_amd.converge has the statements): W[NFREQ] float64, the
        integration weights, COEFF[LEVELS] float32 as set_emission_column takes it -> dict(S_abs, S_new, S_old, M, bad); the
        luminosities L[CELLS] of this call stay on the device for the next.  DoesNotFit where the free device memory does not take them"""
        NFREQ = self._emitted_rows("emitted_change", 0, None)
        W = np.ascontiguousarray(W, np.float64)
        COEFF = np.ascontiguousarray(COEFF, np.float32)
        if W.ndim != 1 or W.size != NFREQ:
            raise SocError("emitted_change: W must hold NFREQ = %d doubles" % NFREQ)
        if COEFF.ndim != 1 or COEFF.size != self.LEVELS:
            raise SocError("emitted_change: COEFF must hold LEVELS = %d floats" % self.LEVELS)
        stats, bad = np.zeros(4, np.float64), C.c_int64(0)
        rc = self.lib.soc_emitted_change(self.h, W.ctypes.data_as(C.POINTER(C.c_double)), _f(COEFF),
                                         stats.ctypes.data_as(C.POINTER(C.c_double)), C.byref(bad))
        if rc == -2:                                           # (nothing was reserved, the emission stays as it is)
            raise DoesNotFit("%s (code %d)" % (self.lib.soc_last_error(self.h).decode(), rc), 0)
        self._chk(rc)
        return dict(S_abs=float(stats[0]), S_new=float(stats[1]), S_old=float(stats[2]), M=float(stats[3]), bad=int(bad.value))

    def emitted_read_luminosity(self, c0, n):
        """L of cells [c0, c0 + n) as the last emitted_change left it, float64; zeros before the first (tests)"""
        self._emitted_rows("emitted_read_luminosity", 0, None)
        out = np.zeros(max(int(n), 0), np.float64)
        self._chk(self.lib.soc_emitted_read_luminosity(self.h, int(c0), int(n), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def emitted_end(self):
        self._chk(self.lib.soc_emitted_end(self.h))
        self._emitted = None

    # ---- the absorptions of the transfer stage, resident for the multi-dust stage (soc_absorbed_*; driven by soc_amd.driver through
    # AbsorptionRun.simulate_constant_sources / simulate_cell_emission and mabu.solve_emission) ----
    def absorbed_begin(self, NFREQ, keep_constant=False):
        """AT[NFREQ, CELLS] of the grid's cells, zeroed; keep_constant: also the second plane of absorbed_keep / absorbed_restore.
        DoesNotFit where the free device memory does not take them (nothing is reserved)"""
        if self.CELLS < 1:
            raise SocError("absorbed_begin: call set_grid first")
        rc = self.lib.soc_absorbed_begin(self.h, int(NFREQ), int(bool(keep_constant)))
        if rc == -2:                                           # (arrays that are open stay as they are)
            raise DoesNotFit("%s (code %d)" % (self.lib.soc_last_error(self.h).decode(), rc), 0)
        self._chk(rc)
        self._absorbed = int(NFREQ)

    def _absorbed_open(self, who, K=None):
        """the open absorbed_begin's NFREQ; K, where given, as the float32 [LEVELS] the library reads"""
        if self._absorbed is None:
            raise SocError("%s: call absorbed_begin first" % who)
        if K is None:
            return self._absorbed, None
        K = np.ascontiguousarray(K, np.float32)
        if K.ndim != 1 or K.size != self.LEVELS:
            raise SocError("%s: K must hold LEVELS = %d floats" % (who, self.LEVELS))
        return self._absorbed, K

    def absorbed_add_tally(self, ifreq):
        """AT[ifreq] += the INT tally (what read_tally(1) reads), on the device"""
        self._absorbed_open("absorbed_add_tally")
        self._chk(self.lib.soc_absorbed_add_tally(self.h, int(ifreq)))

    def absorbed_add_slot(self, ifreq, k):
        """AT[ifreq] += INT slot k of the ended batch (what batch_read_int(k) reads), on the device"""
        self._absorbed_open("absorbed_add_slot")
        self._chk(self.lib.soc_absorbed_add_slot(self.h, int(ifreq), int(k)))

    def absorbed_keep(self):
        self._absorbed_open("absorbed_keep")
        self._chk(self.lib.soc_absorbed_keep(self.h))

    def absorbed_restore(self):
        self._absorbed_open("absorbed_restore")
        self._chk(self.lib.soc_absorbed_restore(self.h))

    def absorbed_to_mabu(self, c0, K, nnnlimit=0.0):
        """all rows of the open mabu_begin from cells [c0, c0 + its cells), scaled as the absorbed file holds them: x K[level] / DENS,
        -1e20 where DENS <= nnnlimit; K[LEVELS] float32 (files.absorbed_scale_factors)"""
        if K is None:
            raise SocError("absorbed_to_mabu: K must hold LEVELS = %d floats" % self.LEVELS)
        _, K = self._absorbed_open("absorbed_to_mabu", K)
        self._chk(self.lib.soc_absorbed_to_mabu(self.h, int(c0), _f(K), np.float32(nnnlimit)))

    def absorbed_download(self, c0, n, K=None, nnnlimit=0.0, out=None):
        """rows [c0, c0 + n) back as [n, NFREQ]: scaled as absorbed_to_mabu hands them over, or, with K None, bit for bit what was
        accumulated; out: a writeable C-contiguous float32 array of that shape to fill"""
        NFREQ, K = self._absorbed_open("absorbed_download", K)
        out = _rows_out("absorbed_download", n, NFREQ, out)
        self._chk(self.lib.soc_absorbed_download(self.h, int(c0), int(n), _f(out), _f(K), np.float32(nnnlimit)))
        return out

    def absorbed_end(self):
        self._chk(self.lib.soc_absorbed_end(self.h))
        self._absorbed = None

    # ---- the library method for dust emission (soc_library_*; driven by soc_amd.library) ----
    LIBRARY_TABLES = ("I1", "dI1", "I2", "dI2", "X", "Y", "Z")

    def library_set(self, lib, ocol=None):
        """Make a library resident: lib is a dict with N, I0, dI0, I1[N], dI1[N], I2[N,N], dI2[N,N], X, Y, Z [N,N,N] and
        E[N^3, NFREQ] (soc_amd.library.read_library); ocol selects and orders emission columns.  library_set(None) forgets it."""
        if lib is None:
            self._chk(self.lib.soc_library_set(self.h, 0, 0, 0.0, 0.0, None, None, None, None, None, None, None, None, 0, None))
            self._lib_nout = 0
            return
        N = int(lib["N"])
        t = [np.ascontiguousarray(lib[k], np.float32) for k in self.LIBRARY_TABLES]
        E = np.ascontiguousarray(lib["E"], np.float32)
        if N < 1 or [a.size for a in t] != [N, N, N * N, N * N, N ** 3, N ** 3, N ** 3] or E.ndim != 2 or E.shape[0] != N ** 3:
            raise SocError("library_set: the tables do not have the sizes of N = %d" % N)
        oc = None if ocol is None else np.ascontiguousarray(ocol, np.int32)
        nout = E.shape[1] if oc is None else oc.size
        self._chk(self.lib.soc_library_set(self.h, N, int(E.shape[1]), np.float32(lib["I0"]), np.float32(lib["dI0"]),
                                           *[_f(a) for a in t], _f(E), int(nout), _i(oc)))
        self._lib_nout = int(nout)

    def library_solve(self, ABS3):
        """ABS3[n, 3], the absorptions at the three reference frequencies -> (EMI[n, nout], the missed cells in ascending order);
        a missed row is 1e32 followed by zeros"""
        ABS3 = np.ascontiguousarray(ABS3, np.float32)
        if ABS3.ndim != 2 or ABS3.shape[1] != 3:
            raise SocError("library_solve: ABS3 must be [n, 3]")
        n = ABS3.shape[0]
        EMI = np.zeros((n, getattr(self, "_lib_nout", 0)), np.float32)
        miss, nmiss = np.zeros(n, np.int32), C.c_int64(0)
        self._chk(self.lib.soc_library_solve(self.h, n, _f(ABS3), _f(EMI), _i(miss), C.byref(nmiss)))
        return EMI, miss[:nmiss.value].copy()

    def library_solve_resident(self, cols):
        """the look-up on the absorptions of a2e_resident_begin / _upload, reference columns cols[3]; the emission is left in the
        resident sum (a2e_resident_download).  Returns the missed cells in ascending order."""
        cols = np.ascontiguousarray(cols, np.int32)
        if cols.size != 3:
            raise SocError("library_solve_resident: three columns")
        miss, nmiss = np.zeros(self._a2e_res[0], np.int32), C.c_int64(0)
        self._chk(self.lib.soc_library_solve_resident(self.h, _i(cols), _i(miss), C.byref(nmiss)))
        return miss[:nmiss.value].copy()

    def library_build(self, N, ABS3=None, cols=None):
        """The grid of a library and every bin's representative cell from ABS3[cells, 3], or from the columns cols[3] of the
        resident absorptions (ABS3 None).  Returns dict(N, I0, dI0, I1, dI1, I2, dI2, IND[N^3], X, Y, Z [N,N,N])."""
        N = int(N)
        if ABS3 is not None:
            ABS3 = np.ascontiguousarray(ABS3, np.float32)
            if ABS3.ndim != 2 or ABS3.shape[1] != 3:
                raise SocError("library_build: ABS3 must be [cells, 3]")
            cells, cols = ABS3.shape[0], None
        else:
            cols = np.ascontiguousarray(cols, np.int32)
            if cols.size != 3 or not self._a2e_res[0]:
                raise SocError("library_build: ABS3, or three columns of the resident absorptions")
            cells = self._a2e_res[0]
        if not 2 <= N <= 64:
            raise SocError("library_build: N = %d (2..64)" % N)
        I0, dI0 = np.zeros(1, np.float32), np.zeros(1, np.float32)
        I1, dI1 = np.zeros(N, np.float32), np.zeros(N, np.float32)
        I2, dI2 = np.zeros((N, N), np.float32), np.zeros((N, N), np.float32)
        IND = np.zeros(N ** 3, np.int32)
        X, Y, Z = (np.zeros((N, N, N), np.float32) for _ in range(3))
        self._chk(self.lib.soc_library_build(self.h, N, int(cells), _f(ABS3), _i(cols), _f(I0), _f(dI0), _f(I1), _f(dI1), _f(I2), _f(dI2),
                                             _i(IND), _f(X), _f(Y), _f(Z)))
        return dict(N=N, I0=I0[0], dI0=dI0[0], I1=I1, dI1=dI1, I2=I2, dI2=dI2, IND=IND, X=X, Y=Y, Z=Z)

    # ---- the library method for several dust components (soc_mabu_library_*; driven by soc_amd.mabu.solve_emission_library) ----
    def mabu_library_begin(self, cells, NDUST, nout):
        """reserve the arrays of a look-up of `cells` cells: NDUST libraries of nout emission columns each; DoesNotFit where the
        cells do not fit the free device memory (cells_fit of them would)"""
        fit = C.c_int64(0)
        rc = self.lib.soc_mabu_library_begin(self.h, int(cells), int(NDUST), int(nout), C.byref(fit))
        if rc == SOC_ERR_STATE and 0 < fit.value < int(cells):
            raise DoesNotFit("%s (code %d)" % (self.lib.soc_last_error(self.h).decode(), rc), fit.value)
        self._chk(rc)
        self._mlib = (int(cells), int(NDUST), int(nout))

    def _mlib_open(self, who):
        """(cells, NDUST, nout) of the open mabu_library_begin"""
        if getattr(self, "_mlib", None) is None:
            raise SocError("%s: call mabu_library_begin first" % who)
        return self._mlib

    def mabu_library_set(self, idust, lib, ocol=None):
        """the library of dust idust (the dict of soc_amd.library.read_library), its E reduced to the columns ocol at upload"""
        self._mlib_open("mabu_library_set")
        N = int(lib["N"])
        t = [np.ascontiguousarray(lib[k], np.float32) for k in self.LIBRARY_TABLES]
        E = np.ascontiguousarray(lib["E"], np.float32)
        if N < 1 or [a.size for a in t] != [N, N, N * N, N * N, N ** 3, N ** 3, N ** 3] or E.ndim != 2 or E.shape[0] != N ** 3:
            raise SocError("mabu_library_set: the tables do not have the sizes of N = %d" % N)
        oc = None if ocol is None else np.ascontiguousarray(ocol, np.int32)
        nout = E.shape[1] if oc is None else oc.size
        self._chk(self.lib.soc_mabu_library_set(self.h, int(idust), N, int(E.shape[1]), np.float32(lib["I0"]), np.float32(lib["dI0"]),
                                                *[_f(a) for a in t], _f(E), int(nout), _i(oc)))

    def mabu_library_upload(self, c0, ABS3):
        self._mlib_open("mabu_library_upload")
        ABS3 = np.ascontiguousarray(ABS3, np.float32)
        if ABS3.ndim != 2 or ABS3.shape[1] != 3:
            raise SocError("mabu_library_upload: ABS3 must be [n, 3]")
        self._chk(self.lib.soc_mabu_library_upload(self.h, int(c0), ABS3.shape[0], _f(ABS3)))

    def mabu_library_set_tables(self, ABU, RABS3):
        cells, NDUST, _ = self._mlib_open("mabu_library_set_tables")
        ABU, RABS3 = np.ascontiguousarray(ABU, np.float32), np.ascontiguousarray(RABS3, np.float64)
        if ABU.shape != (cells, NDUST) or RABS3.shape != (3, NDUST):
            raise SocError("mabu_library_set_tables: ABU%s, RABS3%s for %d cells, %d dusts" % (ABU.shape, RABS3.shape, cells, NDUST))
        self._chk(self.lib.soc_mabu_library_set_tables(self.h, _f(ABU), RABS3.ctypes.data_as(C.POINTER(C.c_double))))

    def mabu_library_solve(self):
        self._chk(self.lib.soc_mabu_library_solve(self.h))

    def mabu_library_download(self, c0, n, out=None):
        """rows [c0, c0 + n) of the sum as [n, nout]; out as in mabu_download"""
        out = _rows_out("mabu_library_download", n, self._mlib_open("mabu_library_download")[2], out)
        self._chk(self.lib.soc_mabu_library_download(self.h, int(c0), int(n), _f(out)))
        return out

    def mabu_library_misses(self, c0, n):
        """uint32 [n]: bit d set where dust d had no answer for the cell"""
        self._mlib_open("mabu_library_misses")
        out = np.zeros(max(int(n), 0), np.uint32)
        self._chk(self.lib.soc_mabu_library_misses(self.h, int(c0), int(n), out.ctypes.data_as(_U)))
        return out

    def mabu_library_end(self):
        self._chk(self.lib.soc_mabu_library_end(self.h))
        self._mlib = None

    def mabu_gather_rows(self, idx):
        """rows idx[n] (repeats allowed) of the current dust's emission in the open mabu_begin, as [n, NFREQ]"""
        NFREQ = self._mabu_open("mabu_gather_rows")[1]
        idx = np.ascontiguousarray(idx, np.int32).ravel()
        out = np.zeros((idx.size, NFREQ), np.float32)
        if idx.size:
            self._chk(self.lib.soc_mabu_gather_rows(self.h, _i(idx), idx.size, _f(out)))
        return out

    # ---- probes ----
    def probe_rng(self, SEED, gid_first, n, ndraw):
        st = np.zeros((n, 2), np.uint32)
        dr = np.zeros((n, max(ndraw, 1)), np.uint32)
        self._chk(self.lib.soc_probe_rng(self.h, np.float32(SEED), int(gid_first), int(n), int(ndraw),
                                         st.ctypes.data_as(_U), dr.ctypes.data_as(_U)))
        return st, dr[:, :ndraw]

    def probe_math(self, fn, x, x2=None):
        """soc_math.h on the device; pown(x, n = x2), atan2(y = x, x = x2) and fmod(x, x2) take the second array"""
        code = dict(exp=0, log=1, sin=2, cos=3, acos=4, sqrt=5, fmod1=6, rcp=7, expm1=8, pow15=9, logd=10,
                    exp_small=11, log10=12, floor=13, pown=14, atan2=15, fmod=16)[fn]
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros_like(x)
        if x2 is None:
            self._chk(self.lib.soc_probe_math(self.h, code, _f(x), _f(y), x.size))
            return y
        x2 = np.ascontiguousarray(x2, np.float32)
        if x2.shape != x.shape:
            raise SocError("probe_math: the two arguments differ in shape")
        self._chk(self.lib.soc_probe_math2(self.h, code, _f(x), _f(x2), _f(y), x.size))
        return y

    def probe_trace(self, pos, direction, maxsteps=100000):
        pos = np.ascontiguousarray(pos, np.float32)
        d = np.ascontiguousarray(direction, np.float32)
        lev = np.zeros(maxsteps, np.int32)
        ind = np.zeros(maxsteps, np.int32)
        ds = np.zeros(maxsteps, np.float32)
        end = np.zeros(3, np.float32)
        n = C.c_int32()
        self._chk(self.lib.soc_probe_trace(self.h, _f(pos), _f(d), maxsteps, _i(lev), _i(ind), _f(ds), _f(end), C.byref(n)))
        n = n.value
        return lev[:n].copy(), ind[:n].copy(), ds[:n].copy(), end
