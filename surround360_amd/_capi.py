"""ctypes bindings of libs360.so (include/s360.h). The library is built in-tree by
surround360_amd/csrc/Makefile; importing this module never builds anything and never falls
back to a CPU implementation — if the shared object is missing, loading fails loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libs360.so")

OK = 0
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_UNKNOWN_ALG, ERR_IO, ERR_STATE = -1, -2, -3, -4, -5, -6
HINT = {"UNKNOWN": 0, "RIGHT": 1, "DOWN": 2, "LEFT": 3, "UP": 4}


class Camera(C.Structure):
    _fields_ = [
        ("type", C.c_int32), ("is_side", C.c_int32),
        ("position", C.c_double * 3), ("rotation", C.c_double * 9), ("resolution", C.c_double * 2),
        ("principal", C.c_double * 2), ("distortion", C.c_double * 2), ("focal", C.c_double * 2),
        ("fov_threshold", C.c_double), ("id", C.c_char * 32),
    ]


class Params(C.Structure):
    _fields_ = [
        ("interpupilary_dist", C.c_double), ("zero_parallax_dist", C.c_double), ("sharpening", C.c_double),
        ("side_alpha_feather_size", C.c_int32), ("std_alpha_feather_size", C.c_int32),
        ("enable_top", C.c_int32), ("enable_bottom", C.c_int32),
        ("eqr_width", C.c_int32), ("eqr_height", C.c_int32),
        ("final_eqr_width", C.c_int32), ("final_eqr_height", C.c_int32),
        ("side_flow_alg", C.c_char * 32), ("polar_flow_alg", C.c_char * 32),
        ("enable_pole_removal", C.c_int32), ("poleremoval_flow_alg", C.c_char * 32),
    ]


class Geometry(C.Structure):
    _fields_ = [
        ("cam_image_width", C.c_int32), ("cam_image_height", C.c_int32),
        ("overlap_image_width", C.c_int32), ("num_novel_views", C.c_int32),
        ("top_rows", C.c_int32), ("bottom_rows", C.c_int32), ("out_width", C.c_int32), ("out_height", C.c_int32),
        ("h_radians", C.c_float), ("v_radians", C.c_float), ("fov_horizontal_radians", C.c_float),
        ("verge_at_infinity_slab_displacement", C.c_float), ("zero_parallax_novel_view_shift_pixels", C.c_float),
    ]


ISP_MAX_CURVE_POINTS = 16


class IspConfig(C.Structure):
    """s360_isp_config (include/s360.h)."""
    _fields_ = [
        ("black_level", C.c_float * 3), ("clamp_min", C.c_float * 3), ("clamp_max", C.c_float * 3),
        ("white_balance_gain", C.c_float * 3), ("ccm", C.c_float * 9), ("saturation", C.c_float),
        ("contrast", C.c_float), ("gamma", C.c_float * 3), ("low_key_boost", C.c_float * 3),
        ("high_key_boost", C.c_float * 3), ("sharpening", C.c_float * 3), ("sharpening_support", C.c_float),
        ("noise_core", C.c_float), ("n_vignette_h", C.c_int32), ("n_vignette_v", C.c_int32),
        ("vignette_roll_off_h", (C.c_float * 3) * ISP_MAX_CURVE_POINTS),
        ("vignette_roll_off_v", (C.c_float * 3) * ISP_MAX_CURVE_POINTS),
        ("stuck_pixel_radius", C.c_int32), ("bayer_pattern", C.c_int32), ("output_bpp", C.c_int32),
        ("demosaic_filter", C.c_int32), ("resize", C.c_int32), ("disable_tone_curve", C.c_int32),
        ("black_level_offset", C.c_int32),
        ("stuck_pixel_threshold", C.c_int32), ("stuck_pixel_darkness_threshold", C.c_float),
        ("pipe", C.c_int32),
    ]


# every symbol include/s360.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "s360_version", "s360_device_count", "s360_last_error", "s360_rig_load_json", "s360_camera_init",
    "s360_camera_pixel", "s360_camera_get_fov", "s360_rig_find_top", "s360_rig_find_bottom", "s360_rig_find_bottom2", "s360_camera_usable_pixels_radius", "s360_derive_geometry",
    "s360_pole_ramp", "s360_create",
    "s360_destroy", "s360_get_geometry", "s360_stream", "s360_synchronize", "s360_set_sharpening", "s360_compute_optical_flow",
    "s360_compute_optical_flow_batch", "s360_bicubic_remap_to_spherical", "s360_spherical_warp_map",
    "s360_combine_lazy_novel_views", "s360_generate_novel_views", "s360_interpolate_views", "s360_flatten_layers_deghost_prefer_base", "s360_offset_horizontal_wrap",
    "s360_feather_alpha_channel", "s360_pole_to_side_flow", "s360_sharpen", "s360_frame_upload_side",
    "s360_frame_upload_top", "s360_frame_upload_bottom", "s360_frame_upload_pole_removal", "s360_frame_set_prev_pole_removal", "s360_frame_render", "s360_frame_render_pairs",
    "s360_frame_set_prev_side", "s360_frame_set_prev_pole", "s360_frame_strip_ptr", "s360_frame_finish", "s360_frame_download_equirect", "s360_frame_equirect_dev",
    "s360_frame_cubemap", "s360_frame_get_u8", "s360_frame_get_f32", "s360_set_keep_intermediates", "s360_set_sweep_mode", "s360_set_frame_pipelining", "s360_debug_flow_levels",
    "s360_profile_enable", "s360_profile_get", "s360_save_flow_to_file", "s360_read_flow_from_file",
    "s360_comm_get_unique_id", "s360_comm_library_path", "s360_comm_init_rank", "s360_comm_init_all", "s360_comm_destroy", "s360_comm_size", "s360_comm_rank", "s360_comm_stats",
    "s360_frame_gather_strips", "s360_frame_exchange_strips", "s360_frame_pole_units", "s360_frame_gather_pole_layers", "s360_frame_composite", "s360_comm_loopback", "s360_frame_set_partition",
    "s360_frame_download_equirect_of", "s360_set_frame_slots", "s360_select_frame_slot", "s360_frame_render_batch", "s360_frame_render_slots",
    "s360_isp_config_defaults", "s360_isp_config_from_json", "s360_isp_create", "s360_isp_destroy", "s360_isp_process",
    "s360_isp_config_tables", "s360_isp_process_packed", "s360_frame_upload_raw", "s360_frame_upload_packed", "s360_isp_pipe_generated",
    "s360_host_alloc", "s360_host_free", "s360_frame_uploads_complete",
    "s360_set_output_double_buffer", "s360_set_png_encode", "s360_frame_png_bound", "s360_frame_download_png", "s360_frame_download_png_slot", "s360_frame_download_equirect_slot", "s360_png_bound", "s360_encode_png",
]
# ... and every symbol include/s360_cubemap.h declares (the cubemap of every frame; s360.h includes that header)
CUBEMAP_SYMBOLS = [
    "s360_set_cubemap_output", "s360_frame_cubemap_size", "s360_frame_download_cubemap", "s360_frame_download_cubemap_slot",
    "s360_frame_cubemap_png_bound", "s360_frame_download_cubemap_png", "s360_frame_download_cubemap_png_slot",
]
# ... and every symbol include/s360_state_png.h declares (RGBA and batched PNG encode; s360.h includes that header too)
STATE_PNG_SYMBOLS = [
    "s360_png_bound_c", "s360_encode_png_c", "s360_encode_png_batch",
    "s360_frame_encode_state_pngs", "s360_frame_state_png_bound", "s360_frame_download_state_png",
]
# ... and every symbol include/s360_png_decode.h declares (banded PNG files decoded on the device; s360.h includes that header too)
PNG_DECODE_SYMBOLS = [
    "s360_png_decodable", "s360_decode_png_batch", "s360_png_decode_stats", "s360_png_decode_round_histogram", "s360_png_decode_failure",
    "s360_frame_set_prev_images_png", "s360_frame_set_prev_flow",
]
# ... and every symbol include/s360_isp_png.h declares (16-bit PNG encode, the ISP's result as a finished file; s360.h includes it too)
ISP_PNG_SYMBOLS = [
    "s360_png_bound_16", "s360_encode_png16", "s360_isp_png_bound", "s360_isp_process_png", "s360_isp_process_packed_png",
]
# ... and every symbol include/s360_input_png.h declares (camera images as banded PNG files, 8- or 16-bit, decoded on the device)
INPUT_PNG_SYMBOLS = ("s360_input_png_decodable", "s360_decode_input_png_batch", "s360_frame_upload_png")
# ... and every symbol include/s360_input_jpeg.h declares (camera images as baseline JPEG files decoded on the device)
INPUT_JPEG_SYMBOLS = ("s360_input_jpeg_decodable", "s360_decode_input_jpeg_batch", "s360_frame_upload_jpeg", "s360_jpeg_decode_stats",
                      "s360_jpeg_decode_failure")
# ... and every symbol include/s360_pole_inputs.h declares (pole removal's secondary camera as a camera; the masks resident per context)
POLE_INPUTS_SYMBOLS = ("s360_frame_upload_bottom2", "s360_set_pole_masks")
S360_CAMERA_BOTTOM2 = -3
# ... and its test tap, include/s360_debug_input_jpeg.h
DEBUG_INPUT_JPEG_SYMBOLS = ("s360_debug_input_jpeg_blocks",)
# ... and every symbol include/s360_frame_jpeg.h declares (a finished frame's equirect and cubemap as JPEG files encoded on the device)
FRAME_JPEG_SYMBOLS = ("s360_set_jpeg_encode", "s360_frame_jpeg_bound", "s360_frame_cubemap_jpeg_bound", "s360_frame_download_jpeg",
                      "s360_frame_download_jpeg_slot", "s360_frame_download_cubemap_jpeg", "s360_frame_download_cubemap_jpeg_slot")
# ... and its test tap, include/s360_debug_frame_jpeg.h
DEBUG_FRAME_JPEG_SYMBOLS = ("s360_debug_frame_jpeg",)
# ... and every symbol include/s360_debug_images.h declares (the reference's debug images of a frame; pole removal as an operator)
DEBUG_IMAGES_SYMBOLS = ("s360_set_debug_images", "s360_frame_debug_image_count", "s360_frame_debug_image_info", "s360_frame_get_debug_image",
                        "s360_frame_encode_debug_pngs", "s360_frame_debug_png_bound", "s360_frame_download_debug_png",
                        "s360_pole_removal_combine")
# ... and its test tap, include/s360_debug_views.h
DEBUG_VIEWS_SYMBOLS = ("s360_debug_views",)
# ... and the test taps include/s360_debug.h declares (not part of the API)
DEBUG_SYMBOLS = ["s360_debug_entry_downscale"]
# ... and the one include/s360_debug_final_flow.h declares
DEBUG_FINAL_FLOW_SYMBOLS = ["s360_debug_upscale_blur"]
# ... and the one include/s360_debug_isp.h declares
DEBUG_ISP_SYMBOLS = ["s360_debug_isp_stages"]

# ... and the one include/s360_debug_flow_level.h declares
DEBUG_FLOW_LEVEL_SYMBOLS = ["s360_debug_flow_level"]
FLOW_LEVEL_INFO = ("lanes_per_pixel", "bands", "waves", "fast_division", "median_tile", "sweep_error")  # S360_FLI_*
FLOW_LEVEL_INFO_COUNT = 8
# ... and the ones include/s360_debug_remap.h declares
DEBUG_REMAP_SYMBOLS = ["s360_debug_remap_packed", "s360_debug_pole_warp_packed", "s360_debug_remap_by_flow"]
# ... and the ones include/s360_debug_flow_pyramid.h declares
DEBUG_FLOW_PYRAMID_SYMBOLS = ["s360_debug_flow_prepare", "s360_debug_resize_linear_f32", "s360_debug_resize_cubic_flow"]
# ... and the ones include/s360_debug_cubemap.h declares
DEBUG_CUBEMAP_SYMBOLS = ["s360_debug_cubemap_tiles", "s360_debug_cubemap"]
# ... and the ones include/s360_preview.h declares (a header of its own: pole-camera previews from packed capture frames)
PREVIEW_SYMBOLS = ["s360_preview_create", "s360_preview_destroy", "s360_preview_cameras", "s360_preview_render_packed",
                   "s360_preview_submit_packed", "s360_preview_fetch", "s360_preview_last_times",
                   "s360_preview_set_jpeg", "s360_preview_jpeg_bound", "s360_preview_fetch_jpeg", "s360_preview_last_jpeg_time"]
# ... and its test taps, include/s360_debug_preview.h
DEBUG_PREVIEW_SYMBOLS = ["s360_debug_preview_camera", "s360_debug_preview_map", "s360_debug_preview_set_maps",
                         "s360_debug_preview_developed", "s360_debug_preview_remapped"]
# ... and the ones include/s360_jpeg.h declares (a header of its own: baseline JPEG files encoded on the device)
JPEG_SYMBOLS = ["s360_jpeg_create", "s360_jpeg_destroy", "s360_jpeg_bound", "s360_jpeg_encode", "s360_jpeg_last_time"]
# ... and its test tap, include/s360_debug_jpeg.h
DEBUG_JPEG_SYMBOLS = ["s360_debug_jpeg_blocks"]


class DebugView(C.Structure):
    """s360_debug_view (include/s360_debug_views.h)."""
    _fields_ = [("src_off", C.c_uint64), ("dst_off", C.c_uint64)] + \
               [(n, C.c_int32) for n in ("src_pitch", "src_rows", "x0", "y0", "w", "h", "shift", "pad_rows", "channels_in", "channels_out")]


class FlowPrepareOut(C.Structure):
    """s360_flow_prepare_out (include/s360_debug_flow_pyramid.h)."""
    _fields_ = [("cap_levels", C.c_int), ("cap_pixels", C.c_size_t)] + \
               [(n, C.c_void_p) for n in ("level_w", "level_h", "n_levels", "factors", "pyr_images", "prev_pyr", "motion_pyr")]


class FlowLevelOut(C.Structure):
    """s360_flow_level_out (include/s360_debug_flow_level.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("gradients", "initial_flow", "blurred_flow", "updated", "row_flags", "sweep_forward",
                                          "median_first", "sweep_backward", "median_second", "diffused", "final_flow")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libs360.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(surround360_amd has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.s360_version.restype = C.c_char_p
        L.s360_last_error.restype = C.c_char_p
        L.s360_last_error.argtypes = [C.c_void_p]
        L.s360_camera_get_fov.restype = C.c_double
        L.s360_camera_usable_pixels_radius.restype = C.c_float
        L.s360_comm_library_path.restype = C.c_char_p
        L.s360_stream.restype = C.c_void_p
        L.s360_stream.argtypes = [C.c_void_p]
        L.s360_host_alloc.restype = C.c_void_p
        L.s360_host_alloc.argtypes = [C.c_size_t]
        L.s360_host_free.restype = None
        L.s360_frame_png_bound.restype = C.c_size_t
        L.s360_frame_png_bound.argtypes = [C.c_void_p]
        L.s360_frame_cubemap_png_bound.restype = C.c_size_t
        L.s360_frame_cubemap_png_bound.argtypes = [C.c_void_p]
        L.s360_png_bound.restype = C.c_size_t
        L.s360_png_bound.argtypes = [C.c_int, C.c_int]
        L.s360_host_free.argtypes = [C.c_void_p]
        L.s360_png_bound_c.restype = C.c_size_t
        L.s360_png_bound_c.argtypes = [C.c_int, C.c_int, C.c_int]
        L.s360_encode_png_c.restype = C.c_int
        L.s360_encode_png_c.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_encode_png_batch.restype = C.c_int
        L.s360_encode_png_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.s360_frame_encode_state_pngs.restype = C.c_int
        L.s360_frame_encode_state_pngs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
        L.s360_frame_state_png_bound.restype = C.c_size_t
        L.s360_frame_state_png_bound.argtypes = [C.c_void_p, C.c_int]
        L.s360_frame_download_state_png.restype = C.c_int
        L.s360_frame_download_state_png.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_png_decodable.restype = C.c_int
        L.s360_png_decodable.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.s360_decode_png_batch.restype = C.c_int
        L.s360_decode_png_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.s360_png_decode_stats.restype = C.c_int
        L.s360_png_decode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.s360_png_decode_round_histogram.restype = C.c_int
        L.s360_png_decode_round_histogram.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.s360_png_decode_failure.restype = C.c_int
        L.s360_png_decode_failure.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.s360_frame_set_prev_images_png.restype = C.c_int
        L.s360_frame_set_prev_images_png.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_size_t)]
        L.s360_frame_set_prev_flow.restype = C.c_int
        L.s360_frame_set_prev_flow.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        L.s360_png_bound_16.restype = C.c_size_t
        L.s360_png_bound_16.argtypes = [C.c_int, C.c_int]
        L.s360_encode_png16.restype = C.c_int
        L.s360_encode_png16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_isp_png_bound.restype = C.c_size_t
        L.s360_isp_png_bound.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.s360_isp_process_png.restype = C.c_int
        L.s360_isp_process_png.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_isp_process_packed_png.restype = C.c_int
        L.s360_isp_process_packed_png.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                  C.POINTER(C.c_size_t)]
        L.s360_input_png_decodable.restype = C.c_int
        L.s360_input_png_decodable.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.s360_decode_input_png_batch.restype = C.c_int
        L.s360_decode_input_png_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_int)]
        L.s360_frame_upload_png.restype = C.c_int
        L.s360_frame_upload_png.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.s360_input_jpeg_decodable.restype = C.c_int
        L.s360_input_jpeg_decodable.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.s360_decode_input_jpeg_batch.restype = C.c_int
        L.s360_decode_input_jpeg_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                                   C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.s360_frame_upload_jpeg.restype = C.c_int
        L.s360_frame_upload_jpeg.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.s360_jpeg_decode_stats.restype = C.c_int
        L.s360_jpeg_decode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int]
        L.s360_jpeg_decode_failure.restype = C.c_int
        L.s360_jpeg_decode_failure.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.s360_frame_upload_bottom2.restype = C.c_int
        L.s360_frame_upload_bottom2.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.s360_set_pole_masks.restype = C.c_int
        L.s360_set_pole_masks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.s360_debug_input_jpeg_blocks.restype = C.c_int
        L.s360_debug_input_jpeg_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_set_jpeg_encode.restype = C.c_int
        L.s360_set_jpeg_encode.argtypes = [C.c_void_p, C.c_int, C.c_int]
        for name in ("s360_frame_jpeg_bound", "s360_frame_cubemap_jpeg_bound"):
            getattr(L, name).restype = C.c_size_t
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("s360_frame_download_jpeg", "s360_frame_download_cubemap_jpeg"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        for name in ("s360_frame_download_jpeg_slot", "s360_frame_download_cubemap_jpeg_slot"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_debug_frame_jpeg.restype = C.c_int
        L.s360_debug_frame_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t] + \
                                           [C.POINTER(C.c_size_t)] * 3 + [C.POINTER(C.c_float)]
        L.s360_set_debug_images.restype = C.c_int
        L.s360_set_debug_images.argtypes = [C.c_void_p, C.c_int]
        L.s360_frame_debug_image_count.restype = C.c_int
        L.s360_frame_debug_image_count.argtypes = [C.c_void_p]
        L.s360_frame_debug_image_info.restype = C.c_int
        L.s360_frame_debug_image_info.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
        L.s360_frame_get_debug_image.restype = C.c_int
        L.s360_frame_get_debug_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.s360_frame_encode_debug_pngs.restype = C.c_int
        L.s360_frame_encode_debug_pngs.argtypes = [C.c_void_p]
        L.s360_frame_debug_png_bound.restype = C.c_size_t
        L.s360_frame_debug_png_bound.argtypes = [C.c_void_p, C.c_int]
        L.s360_frame_download_debug_png.restype = C.c_int
        L.s360_frame_download_debug_png.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_pole_removal_combine.restype = C.c_int
        L.s360_pole_removal_combine.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                                                                C.c_char_p] + [C.c_void_p] * 5
        L.s360_debug_views.restype = C.c_int
        L.s360_debug_views.argtypes = [C.c_void_p, C.c_int, C.POINTER(DebugView), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.s360_debug_isp_stages.restype = C.c_int
        L.s360_debug_isp_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
        L.s360_debug_flow_level.restype = C.c_int
        L.s360_debug_flow_level.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(FlowLevelOut),
                                            C.c_void_p]
        L.s360_debug_flow_prepare.restype = C.c_int
        L.s360_debug_flow_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_char_p, C.c_int, C.POINTER(FlowPrepareOut)]
        L.s360_debug_resize_linear_f32.restype = C.c_int
        L.s360_debug_resize_linear_f32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.s360_debug_resize_cubic_flow.restype = C.c_int
        L.s360_debug_resize_cubic_flow.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.s360_debug_remap_packed.restype = C.c_int
        L.s360_debug_remap_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3
        L.s360_debug_pole_warp_packed.restype = C.c_int
        L.s360_debug_pole_warp_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_float] * 4 + [C.c_void_p] * 3
        L.s360_debug_remap_by_flow.restype = C.c_int
        L.s360_debug_remap_by_flow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.s360_debug_cubemap_tiles.restype = C.c_int
        L.s360_debug_cubemap_tiles.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 4
        L.s360_debug_cubemap.restype = C.c_int
        L.s360_debug_cubemap.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 2
        L.s360_preview_create.restype = C.c_int
        L.s360_preview_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p] + [C.c_int] * 6 + [C.c_double] * 2
        L.s360_preview_destroy.restype = None
        L.s360_preview_destroy.argtypes = [C.c_void_p]
        L.s360_preview_cameras.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.s360_preview_render_packed.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        L.s360_preview_submit_packed.argtypes = [C.c_void_p] * 4 + [C.c_int]
        L.s360_preview_fetch.argtypes = [C.c_void_p, C.c_void_p]
        L.s360_preview_last_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.s360_debug_preview_camera.argtypes = [C.c_void_p, C.c_int, C.POINTER(Camera)]
        L.s360_debug_preview_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.s360_debug_preview_set_maps.argtypes = [C.c_void_p] * 4
        L.s360_debug_preview_developed.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.s360_debug_preview_remapped.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.s360_preview_set_jpeg.restype = C.c_int
        L.s360_preview_set_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.s360_preview_jpeg_bound.restype = C.c_size_t
        L.s360_preview_jpeg_bound.argtypes = [C.c_void_p]
        L.s360_preview_fetch_jpeg.restype = C.c_int
        L.s360_preview_fetch_jpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_preview_last_jpeg_time.restype = C.c_int
        L.s360_preview_last_jpeg_time.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.s360_jpeg_create.restype = C.c_int
        L.s360_jpeg_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 4
        L.s360_jpeg_destroy.restype = None
        L.s360_jpeg_destroy.argtypes = [C.c_void_p]
        L.s360_jpeg_bound.restype = C.c_size_t
        L.s360_jpeg_bound.argtypes = [C.c_int, C.c_int]
        L.s360_jpeg_encode.restype = C.c_int
        L.s360_jpeg_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.s360_jpeg_last_time.restype = C.c_int
        L.s360_jpeg_last_time.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.s360_debug_jpeg_blocks.restype = C.c_int
        L.s360_debug_jpeg_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.s360_isp_config_defaults.restype = None
        L.s360_isp_destroy.restype = None
        L.s360_isp_destroy.argtypes = [C.c_void_p]
        for name in ("s360_destroy", "s360_synchronize", "s360_get_geometry"):
            getattr(L, name).argtypes = None
        _lib = L
    return _lib


class S360Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("s360 error %d: %s" % (code, msg))
        self.code = code


def check(rc, ctx=None):
    if rc < 0:
        msg = lib().s360_last_error(ctx)
        raise S360Error(rc, msg.decode() if msg else "")
    return rc
