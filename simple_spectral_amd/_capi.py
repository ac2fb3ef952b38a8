"""ctypes view of the C ABI (include/ssx.h) and of the host library (include/ssx_host.h)."""
import ctypes as C
import os

from . import build as _build


class SsxSpectrum(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("n", C.c_uint32), ("low", C.c_float), ("high", C.c_float),
                ("delta_recip", C.c_float)]


class SsxVertex(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("st", C.c_float * 2)]


class SsxQuad(C.Structure):
    _fields_ = [("v00", SsxVertex), ("v10", SsxVertex), ("v11", SsxVertex), ("v01", SsxVertex),
                ("normal0", C.c_float * 3), ("normal1", C.c_float * 3),
                ("material", C.c_uint32), ("flags", C.c_uint32)]   # SSX_PRIM_LIGHT | SSX_PRIM_TRI


class SsxMaterial(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("albedo_mode", C.c_uint32), ("albedo_spectrum", C.c_uint32),
                ("albedo_texture", C.c_uint32), ("emission_spectrum", C.c_uint32)]


class SsxTexture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.POINTER(C.c_uint8))]


class SsxMengGrid(C.Structure):
    _fields_ = [("grid_w", C.c_uint32), ("grid_h", C.c_uint32), ("n_points", C.c_uint32), ("n_samples", C.c_uint32),
                ("sample_min", C.c_float), ("sample_max", C.c_float), ("xy_to_uv", C.c_float * 6),
                ("cells", C.POINTER(C.c_int32)), ("points", C.POINTER(C.c_float))]


class SsxSceneDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_uint32),
        ("pv_inv", C.c_double * 16), ("cam_pos", C.c_float * 3),
        ("lambda_min", C.c_float), ("lambda_step", C.c_float),
        ("spec_xbar", C.c_uint32), ("spec_ybar", C.c_uint32), ("spec_zbar", C.c_uint32),
        ("spec_basis_r", C.c_uint32), ("spec_basis_g", C.c_uint32), ("spec_basis_b", C.c_uint32),
        ("spectra", C.POINTER(SsxSpectrum)), ("n_spectra", C.c_uint32),
        ("samples", C.POINTER(C.c_float)), ("n_samples", C.c_uint32),
        ("materials", C.POINTER(SsxMaterial)), ("n_materials", C.c_uint32),
        ("quads", C.POINTER(SsxQuad)), ("n_quads", C.c_uint32),
        ("lights", C.POINTER(C.c_uint32)), ("n_lights", C.c_uint32),
        ("textures", C.POINTER(SsxTexture)), ("n_textures", C.c_uint32),
        ("srgb_to_linear", C.c_float * 256),
        ("uplift", C.c_uint32), ("jh_res", C.c_uint32),
        ("jh_scale", C.POINTER(C.c_float)), ("jh_data", C.POINTER(C.c_float)),
        ("meng", C.POINTER(SsxMengGrid)),
        ("cam_dir", C.c_float * 3), ("reserved2", C.c_uint32),
    ]


class SsxRenderParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32),
                ("indirect_only", C.c_uint32), ("tile_first", C.c_uint32), ("tile_stride", C.c_uint32),
                ("spp_per_launch", C.c_uint32), ("no_explicit_light_sampling", C.c_uint32), ("no_flat_field_correction", C.c_uint32),
                ("tile_major", C.c_uint32), ("tile_skew", C.c_uint32), ("seed", C.c_uint64), ("libm", C.c_uint32), ("reserved3", C.c_uint32)]


class SsxSumsInfo(C.Structure):
    """ssx_sums_info_t: what a set of exported pixel sums belongs to."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("done_spp", C.c_uint32), ("seed", C.c_uint64),
                ("indirect_only", C.c_uint32), ("no_explicit_light_sampling", C.c_uint32), ("no_flat_field_correction", C.c_uint32), ("libm", C.c_uint32),
                ("rgb_mode", C.c_uint32), ("tile_first", C.c_uint32), ("tile_stride", C.c_uint32), ("tile_skew", C.c_uint32),
                ("noise_batches", C.c_uint32), ("reserved", C.c_uint32), ("scene_digest", C.c_uint64)]


class SsxSpectralInfo(C.Structure):
    """ssx_spectral_info_t: what ssx_spectral_read's arrays belong to."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("bins", C.c_uint32), ("done_spp", C.c_uint32),
                ("reserved", C.c_uint32), ("lambda_min", C.c_float), ("bin_width", C.c_float)]


class SsxDemodParams(C.Structure):
    """ssx_demod_params: rays per pixel axis of the albedo bins and the floor under the albedo a pixel is divided by."""
    _fields_ = [("struct_size", C.c_uint32), ("supersample", C.c_uint32), ("albedo_floor", C.c_float)]


SSX_DEMOD_DEFAULT_SUPERSAMPLE, SSX_DEMOD_DEFAULT_FLOOR, SSX_DEMOD_DEFAULT_SIGMA_L = 2, 0.0625, 1.0  # include/ssx.h; DESIGN.md section 15


class SsxDenoiseParams(C.Structure):
    """ssx_denoise_params: levels of the a-trous filter and its two edge-stopping scales."""
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_uint32), ("sigma_l", C.c_float), ("sigma_a", C.c_float)]


class SsxOpticsParams(C.Structure):
    """ssx_optics_params: the optical centre and the per-bin magnification, radius and taps of the lens."""
    _fields_ = [("struct_size", C.c_uint32), ("cx", C.c_float), ("cy", C.c_float), ("max_radius", C.c_uint32),
                ("scale", C.c_void_p), ("radius", C.c_void_p), ("taps", C.c_void_p)]


SSX_OPTICS_MAX_RADIUS = 12  # include/ssx.h


class SsxDefocusParams(C.Structure):
    """ssx_defocus_params: the largest circle of confusion, the gain and the per-bin inverse focus distances of the aperture."""
    _fields_ = [("struct_size", C.c_uint32), ("max_radius", C.c_uint32), ("gain", C.c_float), ("focus", C.c_void_p)]


SSX_DEFOCUS_MAX_RADIUS = 12  # include/ssx.h


class SsxSensorParams(C.Structure):
    """ssx_sensor_params: the colour filter array, the noise, the electron and ADC scales, and the three tables of a sensor."""
    _fields_ = [("struct_size", C.c_uint32), ("cfa", C.c_uint32 * 4), ("noise", C.c_uint32), ("seed", C.c_uint32), ("frame", C.c_uint32),
                ("exposure", C.c_float), ("inv_exposure", C.c_float), ("read_var", C.c_float), ("dn_per_e", C.c_float), ("e_per_dn", C.c_float),
                ("black", C.c_float), ("white", C.c_float), ("weights", C.c_void_p), ("taps", C.c_void_p), ("ccm", C.c_void_p)]


SSH_DEMOSAIC_BILINEAR, SSH_DEMOSAIC_MHC = 0, 1  # include/ssx_host.h


class SsxGlareParams(C.Structure):
    """ssx_glare_params: the radius, the padded extents, and the per-bin switches, point spread functions and the twiddle tables of a glare."""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("px", C.c_uint32), ("py", C.c_uint32),
                ("on", C.c_void_p), ("psf", C.c_void_p), ("twiddle_x", C.c_void_p), ("twiddle_y", C.c_void_p)]


SSX_GLARE_MAX_RADIUS, SSX_GLARE_MAX_EXTENT = 256, 4096  # include/ssx.h


class SsxLocalParams(C.Structure):
    """ssx_local_params: the radius and the scales of LOCAL, the local tone map of a finish."""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("exposure", C.c_float), ("y_lo", C.c_float), ("y_hi", C.c_float), ("eps", C.c_float),
                ("pivot", C.c_float), ("compress", C.c_float), ("boost", C.c_float)]


class SsxToneParams(C.Structure):
    """ssx_tone_params: the channel gains, the matrix and the curve table of TONE."""
    _fields_ = [("struct_size", C.c_uint32), ("shift", C.c_uint32), ("curve_len", C.c_uint32), ("lo", C.c_float), ("hi", C.c_float), ("gains", C.c_float * 3),
                ("matrix", C.c_float * 9), ("curve", C.c_void_p)]


SSX_METER_KEYS, SSX_LOCAL_MAX_RADIUS, SSX_TONE_MAX_CURVE = 4096, 32, 16384  # include/ssx.h
SSH_TONE_CLIP, SSH_TONE_REINHARD, SSH_TONE_FILMIC = 0, 1, 2  # include/ssx_host.h
(SSH_METER_LOG_AVERAGE, SSH_METER_EXPOSURE, SSH_METER_WHITE, SSH_METER_WHITE_EXPOSED, SSH_METER_PIVOT, SSH_METER_GREY, SSH_METER_PATCH, SSH_METER_COUNT,
 SSH_METER_OUT) = 0, 1, 2, 3, 4, 5, 8, 11, 16


class SshSpectrum(C.Structure):
    """ssh_spectrum_t: n uniform samples over [low, high] (include/ssx_host.h)."""
    _fields_ = [("samples", C.POINTER(C.c_float)), ("n", C.c_uint32), ("low", C.c_float), ("high", C.c_float)]


SSH_SPACE_XYZ, SSH_SPACE_LRGB = 0, 1
SSX_LIBM_BUILD, SSX_LIBM_GLIBC_2_35 = 0, 1
LIBM_MODES = {"build": SSX_LIBM_BUILD, "glibc-2.35": SSX_LIBM_GLIBC_2_35}


SSX_MODE_RGB, SSX_UPLIFT_OURS, SSX_UPLIFT_MENG, SSX_UPLIFT_JH = 0, 1, 2, 3
SSX_PRIM_LIGHT, SSX_PRIM_TRI = 1, 0x100
SSX_OK, SSX_ERR_DATA, SSX_ERR_ARG, SSX_ERR_SCENE, SSX_ERR_DEVICE, SSX_ERR_STATE = 0, -1, -2, -3, -10, -11
SSX_ABI_VERSION = 2   # include/ssx.h; checked against the library at load
SSX_JIT_OFF, SSX_JIT_AT_UPLOAD, SSX_JIT_BACKGROUND = 0, 1, 2
# ssx_scene_traits / ssx_render_traits (include/ssx.h): what keeps a render off the kernels with the render switches compiled in
(SSX_TRAIT_INDIRECT_ONLY, SSX_TRAIT_NO_ELS, SSX_TRAIT_MIRROR, SSX_TRAIT_TRI_LIGHT, SSX_TRAIT_UPLIFT, SSX_TRAIT_RGB_MODE, SSX_TRAIT_NO_FLAT_FIELD,
 SSX_TRAIT_KEEP_SAMPLES, SSX_TRAIT_LIBM, SSX_TRAIT_SPECTRAL_BINS, SSX_TRAIT_FORCED_OFF) = (1 << i for i in range(11))
SSX_JIT_STATE_NONE, SSX_JIT_STATE_GENERIC_MEANWHILE, SSX_JIT_STATE_SPECIALISED, SSX_JIT_STATE_FAILED = 0, 1, 2, -1

# every symbol include/ssx.h and include/ssx_host.h declare (tests check the libraries export them)
HIP_SYMBOLS = ["ssx_create", "ssx_destroy", "ssx_upload_scene", "ssx_render_start", "ssx_render_stop",
               "ssx_is_rendering", "ssx_progress", "ssx_render_wait", "ssx_render_device", "ssx_last_error",
               "ssx_abi_version", "ssx_kernel_info", "ssx_plan_info", "ssx_set_timing", "ssx_get_timing",
               "ssx_device_framebuffer", "ssx_device_index", "ssx_read_framebuffer", "ssx_accumulate_peer",
               "ssx_debug_eval", "ssx_debug_samples", "ssx_debug_sweep", "ssx_kernel_variant", "ssx_kernel_name", "ssx_scratch_info", "ssx_calibration_info", "ssx_set_jit", "ssx_debug_pass1_source", "ssx_done_spp", "ssx_reduce_rccl", "ssx_sums_info", "ssx_rccl_groups_made", "ssx_jit_status", "ssx_jit_counters", "ssx_done_tiles", "ssx_render_device_wait", "ssx_units_info", "ssx_rccl_probe",
               "ssx_render_continue", "ssx_scene_digest", "ssx_sums_export", "ssx_sums_import", "ssx_set_noise_estimate", "ssx_noise_info",
               "ssx_set_spectral_bins", "ssx_spectral_read", "ssx_debug_sample_flux",
               "ssx_guides", "ssx_denoise_images", "ssx_denoise", "ssx_denoise_channels", "ssx_denoise_spectral",
               "ssx_develop_images", "ssx_spectral_develop",
               "ssx_albedo_bins", "ssx_denoise_spectral_demod", "ssx_spectral_develop_demod",
               "ssx_spectral_import",
               "ssx_set_spectral_moments", "ssx_spectral_variance", "ssx_spectral_probe", "ssx_probe_arrays",
               "ssx_spectral_noise", "ssx_spectral_noise_reduce",
               "ssx_spectral_moments_import",
               "ssx_spectral_compare", "ssx_spectral_compare_arrays",
               "ssx_delta_e_images", "ssx_spectral_delta_e",
               "ssx_optics_images", "ssx_spectral_develop_optics",
               "ssx_defocus_images", "ssx_spectral_develop_lens",
               "ssx_sensor_images", "ssx_demosaic_images", "ssx_spectral_develop_sensor",
               "ssx_glare_images", "ssx_spectral_develop_glare",
               "ssx_meter_images", "ssx_local_images", "ssx_tone_images",
               "ssx_debug_tile_mask", "ssx_debug_spectral_accumulate", "ssx_debug_fold", "ssx_debug_step",
               "ssx_debug_generate", "ssx_generate_info",
               "ssx_scene_traits", "ssx_render_traits", "ssx_switches_info"]
SSX_GENERATE_FILL_BYTE = 0xA6   # ssx_debug_generate: what a word no lane wrote holds, byte by byte (include/ssx.h)
# ssx_debug_fold: a sample's row of levels (include/ssx.h)
SSX_FOLD_ROW_WORDS, SSX_FOLD_LAMBDA0, SSX_FOLD_CAM_DIR, SSX_FOLD_HIT, SSX_FOLD_N, SSX_FOLD_LEVEL0, SSX_FOLD_LEVEL_WORDS = 160, 0, 1, 4, 5, 10, 15
SSX_FOLD_L_FS, SSX_FOLD_L_NDL, SSX_FOLD_L_PDF, SSX_FOLD_L_FLAGS, SSX_FOLD_L_EMISSION, SSX_FOLD_L_NEE = 0, 4, 5, 6, 7, 11
SSX_FOLD_EMISSION, SSX_FOLD_NEE, SSX_FOLD_NEE_VISIBLE = 1, 2, 4
# ssx_debug_step: a row (one lane's path in front of the trace) and its answer (include/ssx.h)
SSX_STEP_ROW_WORDS, SSX_STEP_R_ORIG, SSX_STEP_R_DIR, SSX_STEP_R_IGNORE, SSX_STEP_R_DEPTH, SSX_STEP_R_LAMBDA0, SSX_STEP_R_RNG, SSX_STEP_R_PREV_SLOT = 16, 0, 3, 6, 7, 8, 9, 13
SSX_STEP_NO_SLOT, SSX_STEP_OUT_WORDS = 0x1FFF, 40
(SSX_STEP_O_FLAGS, SSX_STEP_O_HIT_TRI, SSX_STEP_O_HIT_DIST, SSX_STEP_O_HIT_ST, SSX_STEP_O_EMISSION, SSX_STEP_O_NEE, SSX_STEP_O_NEE_TERM, SSX_STEP_O_FS, SSX_STEP_O_NDL,
 SSX_STEP_O_PDF, SSX_STEP_O_PREV_SLOT, SSX_STEP_O_TAIL_DEPTH, SSX_STEP_O_TAIL_HIT, SSX_STEP_O_NEXT_ORIG, SSX_STEP_O_NEXT_DIR, SSX_STEP_O_NEXT_IGNORE,
 SSX_STEP_O_NEXT_DEPTH, SSX_STEP_O_RNG, SSX_STEP_O_SLOT) = 0, 1, 2, 3, 5, 9, 13, 17, 21, 22, 23, 24, 25, 26, 29, 32, 33, 34, 36
SSX_STEP_HIT, SSX_STEP_CONTINUED, SSX_STEP_EMISSION, SSX_STEP_PARKED, SSX_STEP_VISIBLE = 1, 2, 4, 8, 16
(SSX_SWEEP_RCP, SSX_SWEEP_SQRT, SSX_SWEEP_INVERSESQRT, SSX_SWEEP_SIN, SSX_SWEEP_COS, SSX_SWEEP_ACOS, SSX_SWEEP_DIV_PI,
 SSX_SWEEP_RCP64, SSX_SWEEP_DIV_PAIRS, SSX_SWEEP_ACOS_SIN, SSX_SWEEP_SIN_PROOF, SSX_SWEEP_COS_PROOF, SSX_SWEEP_ACOS_PROOF) = range(1, 14)
# ssx_debug_eval ops (include/ssx.h)
(SSX_DBG_FMATH, SSX_DBG_SPHTRI, SSX_DBG_ARVO, SSX_DBG_SAMPLE_LIGHT, SSX_DBG_COSHEMI, SSX_DBG_TRACE, SSX_DBG_RAND_CHOICE,
 SSX_DBG_ALBEDO, SSX_DBG_FLUX_TO_XYZ, SSX_DBG_RAND_1F) = range(1, 11)
# ... and of libm = glibc-2.35 (the _glibc kernels' units), with the sweeps of include/ssx_glibc_math.h on the device
(SSX_DBG_GLIBC_MATH, SSX_DBG_SPHTRI_GLIBC, SSX_DBG_ARVO_GLIBC, SSX_DBG_SAMPLE_LIGHT_GLIBC, SSX_DBG_COSHEMI_GLIBC) = range(11, 16)
(SSX_SWEEP_GLIBC_SIN, SSX_SWEEP_GLIBC_COS, SSX_SWEEP_GLIBC_ACOS, SSX_SWEEP_GLIBC_COS_LDS) = range(14, 18)
SSX_DBG_TRACE_TOPO = 17     # SSX_DBG_TRACE's row + has_ray: the trace specialised to the context's topology (1, 2, or 3 = the scene's own pattern), as its renders run it
SSX_DBG_TRACE_MASKED = 16   # SSX_DBG_TRACE's row + mask[4]: the masked pass 1 of the generate kernel's trace (rows in blocks of 64 sharing one mask)
HOST_SYMBOLS = ["ssh_scene_create", "ssh_scene_create_ex", "ssh_scene_destroy", "ssh_scene_desc", "ssh_xyza_to_srgba", "ssh_save_image",
                "ssh_load_png_rgb8", "ssh_free", "ssh_color_values", "ssh_last_error", "ssh_checkpoint_save", "ssh_checkpoint_load", "ssh_sums_merge", "ssh_save_npy_f32",
                "ssh_develop_weights", "ssh_relight_gain", "ssh_emitter_spectrum",
                "ssh_checkpoint_save_spectral", "ssh_checkpoint_load_spectral", "ssh_spectral_merge",
                "ssh_probe_derive", "ssh_probe_save_csv", "ssh_spectral_noise_derive", "ssh_spectral_noise_save_csv",
                "ssh_checkpoint_save_moments", "ssh_checkpoint_load_moments", "ssh_moments_merge",
                "ssh_compare_derive", "ssh_compare_save_csv",
                "ssh_delta_e_derive", "ssh_delta_e_save_csv", "ssh_develop_white",
                "ssh_optics_lens", "ssh_defocus_thin_lens", "ssh_scene_vfov",
                "ssh_sensor_bayer", "ssh_sensor_exposure", "ssh_sensor_ccm", "ssh_sensor_standin_curve",
                "ssh_glare_plan", "ssh_glare_twiddles", "ssh_glare_aperture",
                "ssh_meter_derive", "ssh_tone_curve", "ssh_display_matrix"]

_hip = None
_host = None


def host_lib():
    global _host
    if _host is None:
        path = _build.HOST_LIB
        if not os.path.exists(path):
            _build.build_host()
        lib = C.CDLL(path)
        vp = C.c_void_p
        lib.ssh_last_error.restype = C.c_char_p
        lib.ssh_scene_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, vp, C.c_uint32, C.c_uint32, C.c_char_p,
                                         C.c_float, C.POINTER(vp)]
        lib.ssh_scene_create_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int, vp, C.c_uint32, C.c_uint32, C.c_char_p,
                                            C.c_float, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(vp)]
        lib.ssh_scene_destroy.argtypes = [vp]
        lib.ssh_scene_desc.restype = C.POINTER(SsxSceneDesc)
        lib.ssh_scene_desc.argtypes = [vp]
        lib.ssh_xyza_to_srgba.argtypes = [vp, vp, vp, C.c_size_t]
        lib.ssh_save_image.argtypes = [C.c_char_p, vp, C.c_uint32, C.c_uint32]
        lib.ssh_load_png_rgb8.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]
        lib.ssh_free.argtypes = [vp]
        lib.ssh_color_values.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_int]
        lib.ssh_checkpoint_save.argtypes = [C.c_char_p, C.POINTER(SsxSumsInfo), C.c_char_p, C.c_char_p, vp, vp]
        lib.ssh_checkpoint_load.argtypes = [C.c_char_p, C.POINTER(SsxSumsInfo), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                            C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double))]
        lib.ssh_sums_merge.argtypes = [vp, vp, vp, vp, C.POINTER(SsxSumsInfo)]
        lib.ssh_checkpoint_save_spectral.argtypes = [C.c_char_p, C.POINTER(SsxSumsInfo), C.c_char_p, C.c_char_p, vp, vp, C.POINTER(SsxSpectralInfo), vp, vp]
        lib.ssh_checkpoint_load_spectral.argtypes = [C.c_char_p, C.POINTER(SsxSumsInfo), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                                     C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double)),
                                                     C.POINTER(SsxSpectralInfo), C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_uint32))]
        lib.ssh_spectral_merge.argtypes = [vp, vp, vp, vp, C.c_uint32, C.POINTER(SsxSumsInfo)]
        lib.ssh_checkpoint_save_moments.argtypes = lib.ssh_checkpoint_save_spectral.argtypes + [vp]
        lib.ssh_checkpoint_load_moments.argtypes = lib.ssh_checkpoint_load_spectral.argtypes + [C.POINTER(C.POINTER(C.c_double))]
        lib.ssh_moments_merge.argtypes = [vp, vp, C.c_uint32, C.POINTER(SsxSumsInfo)]
        lib.ssh_save_npy_f32.argtypes = [C.c_char_p, vp, C.POINTER(C.c_uint32), C.c_uint32]
        lib.ssh_probe_derive.argtypes = [C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
        lib.ssh_probe_save_csv.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, vp, vp, vp, vp]
        lib.ssh_spectral_noise_derive.argtypes = [C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
        lib.ssh_spectral_noise_save_csv.argtypes = [C.c_char_p, C.c_uint32, C.c_float, C.c_float, vp, vp, vp, vp]
        lib.ssh_compare_derive.argtypes = [C.c_uint32, C.c_uint32] + [vp] * 12
        lib.ssh_compare_save_csv.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float] + [vp] * 6
        lib.ssh_delta_e_derive.argtypes = [C.c_uint32] + [vp] * 11
        lib.ssh_delta_e_save_csv.argtypes = [C.c_char_p, C.c_uint32] + [vp] * 6
        lib.ssh_develop_white.argtypes = [vp, C.c_uint32, C.c_float, C.c_float, C.POINTER(SshSpectrum), vp]
        lib.ssh_develop_weights.argtypes = [C.c_char_p, C.c_int, C.POINTER(SshSpectrum), C.c_uint32, C.POINTER(SshSpectrum), vp, C.c_int, C.c_uint32,
                                            C.c_float, C.c_float, vp, vp]
        lib.ssh_relight_gain.argtypes = [C.POINTER(SshSpectrum), C.POINTER(SshSpectrum), C.c_uint32, C.c_float, C.c_float, vp]
        lib.ssh_emitter_spectrum.argtypes = [C.POINTER(SsxSceneDesc), C.POINTER(C.c_uint32)]
        lib.ssh_optics_lens.argtypes = [C.c_uint32, C.c_float, C.c_float, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, vp, vp, vp]
        lib.ssh_defocus_thin_lens.argtypes = [C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp]
        lib.ssh_scene_vfov.argtypes = [vp, vp]
        lib.ssh_sensor_bayer.argtypes = [C.c_char_p, C.c_int, vp, vp]
        lib.ssh_sensor_exposure.argtypes = [C.c_double, C.c_double, C.c_uint32, C.c_double, C.c_double, vp]
        lib.ssh_sensor_ccm.argtypes = [vp, vp, C.c_uint32, vp]
        lib.ssh_sensor_standin_curve.argtypes = [C.c_uint32, vp, vp, vp]
        lib.ssh_glare_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
        lib.ssh_glare_twiddles.argtypes = [C.c_uint32, vp]
        lib.ssh_glare_aperture.argtypes = [C.c_uint32, C.c_float, C.c_float, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint32, vp, vp]
        lib.ssh_meter_derive.argtypes = [vp, vp, C.c_double, C.c_double, vp, C.c_uint32, vp, vp]
        lib.ssh_tone_curve.argtypes = [C.c_int, C.c_double, C.c_float, C.c_float, C.c_uint32, vp, C.c_uint32]
        lib.ssh_display_matrix.argtypes = [C.c_char_p, C.c_int, vp]
        _host = lib
    return _host


def mapped_hip_runtimes():
    """The distinct libamdhip64 files mapped into this process."""
    out = set()
    try:
        for ln in open("/proc/self/maps"):
            f = ln.split(None, 5)
            if len(f) == 6 and "libamdhip64.so" in os.path.basename(f[5].strip()):
                out.add(os.path.realpath(f[5].strip()))
    except OSError:
        pass
    return sorted(out)


def _elf_dynamic(path):
    """(SONAME, [NEEDED ...]) of a 64-bit little-endian ELF file, from its dynamic section; (None, []) if it cannot be read."""
    import struct
    try:
        with open(path, "rb") as f:
            eh = f.read(64)
            if eh[:6] != b"\x7fELF\x02\x01":
                return None, []
            shoff, = struct.unpack_from("<Q", eh, 0x28)
            shentsize, shnum = struct.unpack_from("<HH", eh, 0x3A)
            f.seek(shoff)
            sh = [struct.unpack_from("<IIQQQQIIQQ", f.read(shentsize)) for _ in range(shnum)]
            dyn = next((x for x in sh if x[1] == 6), None)           # SHT_DYNAMIC
            if dyn is None:
                return None, []
            strtab = sh[dyn[6]]                                      # sh_link: its string table
            f.seek(strtab[4]); names = f.read(strtab[5])
            f.seek(dyn[4]); raw = f.read(dyn[5])
        soname, needed = None, []
        for k in range(0, len(raw) - 15, 16):
            tag, val = struct.unpack_from("<qQ", raw, k)
            if tag in (1, 14):                                       # DT_NEEDED, DT_SONAME
                name = names[val:names.index(b"\0", val)].decode()
                if tag == 14:
                    soname = name
                else:
                    needed.append(name)
        return soname, needed
    except Exception:
        return None, []


def _one_hip_runtime_before_load(path):
    """ONE HIP runtime per process, whatever the import order (this used to be a usage rule).
    libssx_hip.so needs a libamdhip64 by soname ("libamdhip64.so.7" with ROCm 7); torch bundles its own copy.  Streams, events and
    device pointers are handed between torch and this library (bench.py, dist.py), which only works inside one runtime.  So:
      * a runtime is already mapped (torch was imported first, or the host linked one): the loader binds libssx_hip.so to it
        by soname -- nothing to do;
      * none is mapped, torch is installed AND its bundled copy carries the soname libssx_hip.so asks for: that copy is mapped NOW
        (RTLD_GLOBAL), so that libssx_hip.so binds to it and a later `import torch` finds its own runtime already in place;
      * no torch, or a torch built against another ROCm generation (another soname: preloading it would not satisfy the library's
        NEEDED entry and only put a second runtime into a renderer-only process): libssx_hip.so brings /opt/rocm's through its RUNPATH.
    _one_hip_runtime_after_load checks the outcome instead of trusting it."""
    if mapped_hip_runtimes():
        return
    try:
        import importlib.util
        wanted = [n for n in _elf_dynamic(path)[1] if n.startswith("libamdhip64.so")]
        spec = importlib.util.find_spec("torch")
        if wanted and spec and spec.submodule_search_locations:
            cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(cand) and _elf_dynamic(cand)[0] == wanted[0]:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # (then the library's own RUNPATH decides; the check below still holds)


def _one_hip_runtime_after_load(path):
    rts = mapped_hip_runtimes()                                      # (/proc/self/maps: read here, once per process -- hip_lib() caches the library)
    if len(rts) > 1:
        raise RuntimeError("two HIP runtimes are mapped into this process (%s) after loading %s: streams and device pointers cannot be "
                           "handed between them.  Import simple_spectral_amd (or torch) before whatever loaded the other one, or "
                           "point LD_LIBRARY_PATH at one of them." % (", ".join(rts), path))


def hip_lib():
    """The HIP library.  There is no fallback: a missing library is an error."""
    global _hip
    if _hip is None:
        # SSX_HIP_LIB_OVERRIDE: A/B and profiling builds (tools/ab_bench.sh, tools/lanestat.py); like the library's own A/B
        # switches it is honoured only under the master switch SSX_DEBUG_ENV=1
        path = (os.environ.get("SSX_HIP_LIB_OVERRIDE") if os.environ.get("SSX_DEBUG_ENV") == "1" else None) or _build.HIP_LIB
        if not os.path.exists(path):
            raise RuntimeError("%s is missing: run `python -m simple_spectral_amd.build` (needs hipcc). "
                               "simple_spectral_amd has no CPU or PyTorch fallback path." % path)
        _one_hip_runtime_before_load(path)
        lib = C.CDLL(path)
        _one_hip_runtime_after_load(path)
        override = path != _build.HIP_LIB
        if not override and lib.ssx_abi_version() != SSX_ABI_VERSION:  # (an A/B library of an older revision is loaded as it is)
            raise RuntimeError("%s implements ABI version %d, this binding version %d (include/ssx.h): rebuild with `python -m simple_spectral_amd.build`"
                               % (path, lib.ssx_abi_version(), SSX_ABI_VERSION))
        vp = C.c_void_p
        lib.ssx_last_error.restype = C.c_char_p
        lib.ssx_last_error.argtypes = [vp]
        lib.ssx_create.argtypes = [C.c_int, C.POINTER(vp)]
        lib.ssx_destroy.argtypes = [vp]
        lib.ssx_destroy.restype = None
        lib.ssx_upload_scene.argtypes = [vp, C.POINTER(SsxSceneDesc)]
        lib.ssx_render_start.argtypes = [vp, C.POINTER(SsxRenderParams)]
        lib.ssx_render_stop.argtypes = [vp]
        lib.ssx_is_rendering.argtypes = [vp]
        lib.ssx_progress.argtypes = [vp]
        lib.ssx_progress.restype = C.c_float
        lib.ssx_render_wait.argtypes = [vp, vp]
        lib.ssx_render_device.argtypes = [vp, C.POINTER(SsxRenderParams), vp, vp]
        lib.ssx_kernel_info.argtypes = [vp] + [C.POINTER(C.c_int)] * 5
        lib.ssx_plan_info.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        lib.ssx_set_timing.argtypes = [vp, C.c_int]
        lib.ssx_get_timing.argtypes = [vp, C.POINTER(C.c_float)]
        lib.ssx_device_framebuffer.argtypes = [vp]
        lib.ssx_device_framebuffer.restype = vp
        lib.ssx_device_index.argtypes = [vp]
        lib.ssx_read_framebuffer.argtypes = [vp, vp]
        lib.ssx_accumulate_peer.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, C.c_uint32, vp]
        lib.ssx_debug_eval.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32]
        lib.ssx_debug_samples.argtypes = [vp, C.POINTER(SsxRenderParams), vp, vp, vp]
        lib.ssx_debug_sweep.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
        if not override or hasattr(lib, "ssx_scratch_info"):
            lib.ssx_calibration_info.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]
            lib.ssx_scratch_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if not override or hasattr(lib, "ssx_set_jit"):
            lib.ssx_set_jit.argtypes = [vp, C.c_int]
            lib.ssx_done_spp.argtypes = [vp]
            lib.ssx_done_spp.restype = C.c_uint32
            lib.ssx_reduce_rccl.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32]
            lib.ssx_debug_pass1_source.argtypes = [C.POINTER(C.c_uint8), C.c_uint32, C.c_char_p, C.c_char_p, C.c_size_t]
        if not override or hasattr(lib, "ssx_sums_info"):
            lib.ssx_sums_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(lib, "ssx_rccl_probe"):
            lib.ssx_rccl_probe.argtypes = [C.c_char_p, C.c_size_t]
        if hasattr(lib, "ssx_units_info"):  # (new in round 6: an older build loaded through SSX_HIP_LIB_OVERRIDE has none)
            lib.ssx_units_info.argtypes = [vp, C.POINTER(C.c_uint64)]
        if not override or hasattr(lib, "ssx_jit_status"):
            lib.ssx_jit_status.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
            lib.ssx_jit_counters.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            lib.ssx_jit_counters.restype = None
            lib.ssx_rccl_groups_made.restype = C.c_uint64
            lib.ssx_render_device_wait.argtypes = [vp]
            lib.ssx_done_tiles.argtypes = [vp]
            lib.ssx_done_tiles.restype = C.c_uint32
        if not override or hasattr(lib, "ssx_render_continue"):  # progressive rendering
            lib.ssx_render_continue.argtypes = [vp, C.c_uint32]
            lib.ssx_scene_digest.argtypes = [vp]
            lib.ssx_scene_digest.restype = C.c_uint64
            lib.ssx_sums_export.argtypes = [vp, C.POINTER(SsxSumsInfo), vp, vp]
            lib.ssx_sums_import.argtypes = [vp, C.POINTER(SsxRenderParams), C.POINTER(SsxSumsInfo), vp, vp]
            lib.ssx_set_noise_estimate.argtypes = [vp, C.c_int]
            lib.ssx_noise_info.argtypes = [vp, vp, C.POINTER(C.c_double)]
        if not override or hasattr(lib, "ssx_set_spectral_bins"):  # spectral output
            lib.ssx_set_spectral_bins.argtypes = [vp, C.c_uint32]
            lib.ssx_spectral_read.argtypes = [vp, C.POINTER(SsxSpectralInfo), vp, vp, vp]
            lib.ssx_debug_sample_flux.argtypes = [vp, C.POINTER(SsxRenderParams), vp, vp]
        if not override or hasattr(lib, "ssx_denoise"):  # denoising
            lib.ssx_guides.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
            lib.ssx_denoise_images.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
            lib.ssx_denoise.argtypes = [vp, C.POINTER(SsxDenoiseParams), vp, vp]
        if not override or hasattr(lib, "ssx_denoise_spectral"):  # extra channels under the filter's weights
            lib.ssx_denoise_channels.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp]
            lib.ssx_denoise_spectral.argtypes = [vp, C.POINTER(SsxDenoiseParams), vp, vp, vp]
        if not override or hasattr(lib, "ssx_spectral_develop"):  # developing the spectral bins
            lib.ssx_develop_images.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp]
            lib.ssx_spectral_develop.argtypes = [vp, C.POINTER(SsxDenoiseParams), vp, C.c_uint32, vp]
        if not override or hasattr(lib, "ssx_albedo_bins"):  # demodulated denoising
            lib.ssx_albedo_bins.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]
            lib.ssx_denoise_spectral_demod.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.POINTER(SsxDemodParams), vp, vp, vp, vp]
            lib.ssx_spectral_develop_demod.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.POINTER(SsxDemodParams), vp, vp, C.c_uint32, vp]
        if not override or hasattr(lib, "ssx_spectral_import"):  # the bins through checkpoint and resume
            lib.ssx_spectral_import.argtypes = [vp, C.POINTER(SsxSpectralInfo), vp, vp]
        if not override or hasattr(lib, "ssx_set_spectral_moments"):  # error bars for the bins: second moments, variances, region probes
            lib.ssx_set_spectral_moments.argtypes = [vp, C.c_int]
            lib.ssx_spectral_variance.argtypes = [vp, C.POINTER(SsxSpectralInfo), vp, vp]
            lib.ssx_spectral_probe.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp]
            lib.ssx_probe_arrays.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp]
        if not override or hasattr(lib, "ssx_spectral_noise"):  # the spectral noise figure: tile partials and totals
            lib.ssx_spectral_noise.argtypes = [vp] * 10
            lib.ssx_spectral_noise_reduce.argtypes = [vp, C.c_uint32, C.c_uint32] + [vp] * 8
        if not override or hasattr(lib, "ssx_spectral_compare"):  # comparing two spectral renders: region sums and maps
            lib.ssx_spectral_compare.argtypes = [vp, C.POINTER(SsxSpectralInfo), vp, vp, vp, vp, C.c_uint32, C.c_double] + [vp] * 8
            lib.ssx_spectral_compare_arrays.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32] + [vp] * 7 + [C.c_uint32, C.c_double] + [vp] * 8
        if not override or hasattr(lib, "ssx_delta_e_images"):  # the colour difference of two developments: maps and region figures
            lib.ssx_delta_e_images.argtypes = [vp, C.c_uint32, C.c_uint32] + [vp] * 5 + [C.c_uint32] + [vp] * 9
            lib.ssx_spectral_delta_e.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.c_int, C.c_int] + [vp] * 5 + [C.c_uint32] + [vp] * 9
        if not override or hasattr(lib, "ssx_optics_images"):  # developing through a lens: per-bin warp and blur
            lib.ssx_optics_images.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(SsxOpticsParams), vp]
            lib.ssx_spectral_develop_optics.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.POINTER(SsxOpticsParams), vp, C.c_uint32, vp, vp]
        if not override or hasattr(lib, "ssx_defocus_images"):  # depth of field after the render: per-bin defocus from the depth guide
            lib.ssx_defocus_images.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(SsxDefocusParams), vp]
            lib.ssx_spectral_develop_lens.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.POINTER(SsxDefocusParams), C.POINTER(SsxOpticsParams), vp, C.c_uint32, vp, vp]
        if not override or hasattr(lib, "ssx_sensor_images"):  # developing onto a sensor: mosaic, noise, ADC and demosaic
            lib.ssx_sensor_images.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(SsxSensorParams), vp, vp]
            lib.ssx_demosaic_images.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(SsxSensorParams), vp]
            lib.ssx_spectral_develop_sensor.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.POINTER(SsxDefocusParams), C.POINTER(SsxOpticsParams), C.POINTER(SsxSensorParams), vp, vp, vp]
        if not override or hasattr(lib, "ssx_glare_images"):  # veiling glare and diffraction: per-bin convolution by FFT
            lib.ssx_glare_images.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(SsxGlareParams), vp]
            lib.ssx_spectral_develop_glare.argtypes = [vp, C.POINTER(SsxDenoiseParams), C.POINTER(SsxDefocusParams), C.POINTER(SsxOpticsParams), C.POINTER(SsxGlareParams), vp, C.c_uint32, vp, vp]
        if not override or hasattr(lib, "ssx_meter_images"):  # finishing a development for a display: meter, local tone map, tone curve
            lib.ssx_meter_images.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
            lib.ssx_local_images.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(SsxLocalParams), vp, vp]
            lib.ssx_tone_images.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(SsxToneParams), vp]
        if not override or hasattr(lib, "ssx_spectral_moments_import"):  # the second moments through checkpoint and resume
            lib.ssx_spectral_moments_import.argtypes = [vp, C.POINTER(SsxSpectralInfo), vp]
        if not override or hasattr(lib, "ssx_debug_tile_mask"):  # the camera-ray pre-trace's tile masks, read back
            lib.ssx_debug_tile_mask.argtypes = [vp, C.POINTER(SsxRenderParams), vp]
        if not override or hasattr(lib, "ssx_debug_spectral_accumulate"):  # the bin and moment kernels on the caller's sample records
            lib.ssx_debug_spectral_accumulate.argtypes = [vp] + [C.c_uint32] * 6 + [C.c_float, C.c_float, C.c_uint32] + [vp] * 6
        if not override or hasattr(lib, "ssx_debug_fold"):  # the path kernel's fold on the caller's levels
            lib.ssx_debug_fold.argtypes = [vp, C.POINTER(SsxRenderParams), C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
        if not override or hasattr(lib, "ssx_debug_step"):  # one iteration of the path loop on the caller's paths
            lib.ssx_debug_step.argtypes = [vp, C.POINTER(SsxRenderParams), C.c_uint32, C.c_uint32, vp, vp]
        if not override or hasattr(lib, "ssx_debug_generate"):  # the generate kernel's records, read back; which launches made their samples where
            lib.ssx_debug_generate.argtypes = [vp, C.POINTER(SsxRenderParams), C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp]
            lib.ssx_generate_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.ssx_kernel_variant.argtypes = [vp]
        lib.ssx_kernel_name.argtypes = [vp]
        lib.ssx_kernel_name.restype = C.c_char_p
        if hasattr(lib, "ssx_switches_info"):  # (an older build loaded through SSX_HIP_LIB_OVERRIDE for an A/B run has none of the three)
            lib.ssx_switches_info.argtypes = [vp]
            lib.ssx_scene_traits.argtypes = [vp]
            lib.ssx_render_traits.argtypes = [vp]
        _hip = lib
    return _hip
