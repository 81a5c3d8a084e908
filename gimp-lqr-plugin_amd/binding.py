"""ctypes binding of the LqrCarver C ABI (include/lqr.h) -- the Python-side mirror of the
interface gimp-lqr-plugin's src/render.c and src/io_functions.c consume.

`engine_api()` binds the MI355X engine (liblqr-hip.so, next to this file).  `Api(path, prefix)`
binds any other library exporting the same ABI (the tests bind their CPU oracle and, where one
exists, a genuine liblqr-1 this way -- nothing in this package knows about either).
An Api may carry `absent`, a set of names its library does not export: the bind_* helpers of the
later surfaces leave those out instead of failing.

Call order in `Carver.configure` mirrors the reference's render_init_carver
(src/render.c:220-248); read-out mirrors write_carver_to_layer (src/io_functions.c:155-164).
"""
import ctypes as C
import os

import numpy as np

try:        # if torch is going to be used in this process, its bundled HIP runtime must load first
    import torch  # noqa: F401
except Exception:      # the engine does not need torch
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
# (LQR_HIP_LIB: another build of the same library, for A/B runs of bench.py and the tests)
ENGINE_LIB = os.environ.get("LQR_HIP_LIB") or os.path.join(HERE, "liblqr-hip.so")

LQR_ERROR, LQR_OK, LQR_NOMEM, LQR_USRCANCEL = 0, 1, 2, 3
LQR_RES_ORDER_HOR, LQR_RES_ORDER_VERT = 0, 1
(LQR_EF_GRAD_NORM, LQR_EF_GRAD_SUMABS, LQR_EF_GRAD_XABS, LQR_EF_LUMA_GRAD_NORM,
 LQR_EF_LUMA_GRAD_SUMABS, LQR_EF_LUMA_GRAD_XABS, LQR_EF_NULL) = range(7)

_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]

PROGRESS_INIT = C.CFUNCTYPE(C.c_int, C.c_char_p)
PROGRESS_UPDATE = C.CFUNCTYPE(C.c_int, C.c_double)
PROGRESS_END = C.CFUNCTYPE(C.c_int, C.c_char_p)
VMAP_FUNC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)

# name -> (restype, argtypes); every symbol include/lqr.h declares
_P, _I, _F, _D = C.c_void_p, C.c_int, C.c_float, C.c_double
SYMBOLS = {
    "lqr_carver_new": (_P, [_P, _I, _I, _I]),
    "lqr_carver_init": (_I, [_P, _I, _F]),
    "lqr_carver_destroy": (None, [_P]),
    "lqr_carver_attach": (_I, [_P, _P]),
    "lqr_carver_set_energy_function_builtin": (_I, [_P, _I]),
    "lqr_carver_set_resize_order": (None, [_P, _I]),
    "lqr_carver_set_progress": (None, [_P, _P]),
    "lqr_carver_set_side_switch_frequency": (None, [_P, C.c_uint]),
    "lqr_carver_set_enl_step": (_I, [_P, _F]),
    "lqr_carver_get_enl_step": (_F, [_P]),
    "lqr_carver_set_dump_vmaps": (None, [_P]),
    "lqr_carver_bias_add_rgb_area": (_I, [_P, _P, _I, _I, _I, _I, _I, _I]),
    "lqr_carver_rigmask_add_rgb_area": (_I, [_P, _P, _I, _I, _I, _I, _I]),
    "lqr_carver_resize": (_I, [_P, _I, _I]),
    "lqr_carver_flatten": (_I, [_P]),
    "lqr_carver_scan_line": (_I, [_P, C.POINTER(_I), C.POINTER(_P)]),
    "lqr_carver_scan_by_row": (_I, [_P]),
    "lqr_carver_scan_reset": (None, [_P]),
    "lqr_carver_get_width": (_I, [_P]),
    "lqr_carver_get_height": (_I, [_P]),
    "lqr_carver_get_channels": (_I, [_P]),
    "lqr_carver_get_ref_width": (_I, [_P]),
    "lqr_carver_get_ref_height": (_I, [_P]),
    "lqr_carver_get_orientation": (_I, [_P]),
    "lqr_carver_get_depth": (_I, [_P]),
    "lqr_carver_list_start": (_P, [_P]),
    "lqr_carver_list_current": (_P, [_P]),
    "lqr_carver_list_next": (_P, [_P]),
    "lqr_vmap_dump": (_P, [_P]),
    "lqr_vmap_destroy": (None, [_P]),
    "lqr_vmap_get_data": (C.POINTER(_I), [_P]),
    "lqr_vmap_get_width": (_I, [_P]),
    "lqr_vmap_get_height": (_I, [_P]),
    "lqr_vmap_get_depth": (_I, [_P]),
    "lqr_vmap_get_orientation": (_I, [_P]),
    "lqr_vmap_list_start": (_P, [_P]),
    "lqr_vmap_list_current": (_P, [_P]),
    "lqr_vmap_list_next": (_P, [_P]),
    "lqr_vmap_list_foreach": (_I, [_P, VMAP_FUNC, _P]),
    "lqr_progress_new": (_P, []),
    "lqr_progress_set_init": (_I, [_P, PROGRESS_INIT]),
    "lqr_progress_set_update": (_I, [_P, PROGRESS_UPDATE]),
    "lqr_progress_set_end": (_I, [_P, PROGRESS_END]),
    "lqr_progress_set_update_step": (_I, [_P, _F]),
    "lqr_progress_set_init_width_message": (_I, [_P, C.c_char_p]),
    "lqr_progress_set_init_height_message": (_I, [_P, C.c_char_p]),
    "lqr_progress_set_end_width_message": (_I, [_P, C.c_char_p]),
    "lqr_progress_set_end_height_message": (_I, [_P, C.c_char_p]),
    "lqrx_carver_get_energy": (_I, [_P, _P]),
    "lqrx_carver_frame_width": (_I, [_P]),
    "lqrx_carver_frame_height": (_I, [_P]),
    "lqrx_carver_debug_maps": (_I, [_P, _P, _P, _P]),
    "lqrx_set_debug": (None, [_I]),
    "lqrx_carver_debug_width": (_I, [_P]),
    "lqrx_carver_debug_height": (_I, [_P]),
    "lqrx_carver_debug_snapshot": (_I, [_P, _P, _P, _P]),
    "lqrx_carver_read_image": (_I, [_P, _P]),
    "lqrx_carver_resize_batch": (_I, [C.POINTER(_P), _I, _I, _I]),
    "lqrx_carver_read_image_device": (_I, [_P, _P]),
    "lqrx_guess_new_size": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I]),
    "lqrx_vmap_to_rgba": (_I, [_P, C.POINTER(_D), C.POINTER(_D), _P]),
    "lqrx_carver_reload_device_batch": (_I, [C.POINTER(_P), _I, C.POINTER(_P)]),
}
# liblqr-1 proper exports only the lqr_* part
LIBLQR_SYMBOLS = [s for s in SYMBOLS if s.startswith("lqr_")]

# include/lqr_coldepth.h: the colour-depth surface (liblqr 0.4's lqr_carver_new_ext and its read-out), kept apart from SYMBOLS,
# which is exactly what lqr.h declares
LQR_COLDEPTH_8I, LQR_COLDEPTH_16I, LQR_COLDEPTH_32F, LQR_COLDEPTH_64F = range(4)
COLDEPTH_DTYPES = {LQR_COLDEPTH_8I: np.uint8, LQR_COLDEPTH_16I: np.uint16, LQR_COLDEPTH_32F: np.float32, LQR_COLDEPTH_64F: np.float64}
COLDEPTH_SYMBOLS = {
    "lqr_carver_new_ext": (_P, [_P, _I, _I, _I, _I]),
    "lqr_carver_set_preserve_input_image": (None, [_P]),
    "lqr_carver_scan": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_P)]),
    "lqr_carver_scan_ext": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_P)]),
    "lqr_carver_scan_line_ext": (_I, [_P, C.POINTER(_I), C.POINTER(_P)]),
    "lqr_carver_get_col_depth": (_I, [_P]),
    "lqr_carver_get_image_type": (_I, [_P]),
    "lqr_carver_get_bpp": (_I, [_P]),
}


def bind_coldepth(api):
    """add COLDEPTH_SYMBOLS to a bound Api (the engine, or a genuine liblqr-1); returns it"""
    if not getattr(api, "has_coldepth", False):
        for name, (res, args) in COLDEPTH_SYMBOLS.items():
            if name in getattr(api, "absent", ()):
                continue
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.has_coldepth = hasattr(api, "lqr_carver_new_ext")      # (an Api whose `absent` covers the surface has none of it)
    return api


# include/lqr_imagetype.h: liblqr 0.4's image types (CMY, CMYK, CMYKA, custom channels) and the channel limit, in a table of their own
(LQR_RGB_IMAGE, LQR_RGBA_IMAGE, LQR_GREY_IMAGE, LQR_GREYA_IMAGE, LQR_CMY_IMAGE, LQR_CMYK_IMAGE, LQR_CMYKA_IMAGE,
 LQR_CUSTOM_IMAGE) = range(8)
IMGTYPE_SYMBOLS = {
    "lqr_carver_set_image_type": (_I, [_P, _I]),
    "lqr_carver_set_alpha_channel": (_I, [_P, _I]),
    "lqr_carver_set_black_channel": (_I, [_P, _I]),
    "lqrx_set_max_channels": (_I, [_I]),
}


def bind_imagetype(api):
    """add IMGTYPE_SYMBOLS (and COLDEPTH_SYMBOLS) to a bound Api; a genuine liblqr-1 has no lqrx_set_max_channels and keeps none"""
    bind_coldepth(api)
    if not getattr(api, "has_imagetype", False):
        for name, (res, args) in IMGTYPE_SYMBOLS.items():
            if name.startswith("lqrx_") and not api.has_ext:
                continue
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.has_imagetype = True
    return api


# include/lqr_masks.h: liblqr's computed-mask calls (gdouble planes, single values, clears) and the engine's device forms and plane
# read-outs, in a table of their own
_Z = C.c_size_t
MASK_SYMBOLS = {
    "lqr_carver_bias_add_xy": (_I, [_P, _D, _I, _I]),
    "lqr_carver_bias_add_area": (_I, [_P, _P, _I, _I, _I, _I, _I]),
    "lqr_carver_bias_add": (_I, [_P, _P, _I]),
    "lqr_carver_bias_add_rgb": (_I, [_P, _P, _I, _I]),
    "lqr_carver_bias_clear": (None, [_P]),
    "lqr_carver_rigmask_add_xy": (_I, [_P, _D, _I, _I]),
    "lqr_carver_rigmask_add_area": (_I, [_P, _P, _I, _I, _I, _I]),
    "lqr_carver_rigmask_add": (_I, [_P, _P]),
    "lqr_carver_rigmask_add_rgb": (_I, [_P, _P, _I]),
    "lqr_carver_rigmask_clear": (None, [_P]),
    "lqrx_carver_bias_add_area_device": (_I, [_P, _P, _I, _I, _I, _I, _I, _I]),
    "lqrx_carver_rigmask_add_area_device": (_I, [_P, _P, _I, _I, _I, _I, _I]),
    "lqrx_carver_get_bias": (_I, [_P, _P]),
    "lqrx_carver_get_rigmask": (_I, [_P, _P]),
}


def bind_masks(api):
    """add MASK_SYMBOLS (and COLDEPTH_SYMBOLS) to a bound Api; a genuine liblqr-1 has none of the lqrx_ ones"""
    bind_coldepth(api)
    if not getattr(api, "has_masks", False):
        for name, (res, args) in MASK_SYMBOLS.items():
            if (name.startswith("lqrx_") and not api.has_ext) or name in getattr(api, "absent", ()):
                continue
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        if api.has_ext and "lqrhip_debug_mask_flushes" not in getattr(api, "absent", ()):
            api.lqrhip_debug_mask_flushes = api.lib.lqrhip_debug_mask_flushes
            api.lqrhip_debug_mask_flushes.restype, api.lqrhip_debug_mask_flushes.argtypes = C.c_ulonglong, []
        api.has_masks = True
    return api


# include/lqr_energy.h: liblqr's energy read-outs (as they are, normalised, as a picture) and the engine's forms into device memory
ENERGY_SYMBOLS = {
    "lqr_carver_get_energy": (_I, [_P, _P, _I]),
    "lqr_carver_get_true_energy": (_I, [_P, _P, _I]),
    "lqr_carver_get_energy_image": (_I, [_P, _P, _I, _I, _I]),
    "lqrx_carver_get_energy_device": (_I, [_P, _P, _I, _I]),
    "lqrx_carver_get_energy_image_device": (_I, [_P, _P, _I, _I, _I]),
}
IMAGE_TYPE_CHANNELS = {LQR_RGB_IMAGE: 3, LQR_RGBA_IMAGE: 4, LQR_GREY_IMAGE: 1, LQR_GREYA_IMAGE: 2, LQR_CMY_IMAGE: 3, LQR_CMYK_IMAGE: 4,
                       LQR_CMYKA_IMAGE: 5}


def bind_energy(api):
    """add ENERGY_SYMBOLS (and COLDEPTH_SYMBOLS) to a bound Api; a genuine liblqr-1 has none of the lqrx_ ones"""
    bind_coldepth(api)
    if not getattr(api, "has_energy", False):
        for name, (res, args) in ENERGY_SYMBOLS.items():
            if (name.startswith("lqrx_") and not api.has_ext) or name in getattr(api, "absent", ()):
                continue
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.has_energy = True
    return api


# include/lqr_vmap.h: liblqr's way to take a seam map back (lqr_vmap_new, lqr_vmap_load, lqr_vmap_internal_dump) and the engine's forms
# for a map in device memory and for one map shared by a batch
VMAP_SYMBOLS = {
    "lqr_vmap_new": (_P, [_P, _I, _I, _I, _I]),
    "lqr_vmap_load": (_I, [_P, _P]),
    "lqr_vmap_internal_dump": (_I, [_P]),
    "lqrx_vmap_load_device": (_I, [_P, _P, _I, _I, _I, _I]),
    "lqrx_vmap_load_batch": (_I, [C.POINTER(_P), _I, _P]),
}


def bind_vmap(api):
    """add VMAP_SYMBOLS to a bound Api; a genuine liblqr-1 has none of the lqrx_ ones"""
    if not getattr(api, "has_vmap", False):
        for name, (res, args) in VMAP_SYMBOLS.items():
            if name.startswith("lqrx_") and not api.has_ext:
                continue
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.has_vmap = True
    return api


# include/lqr_control.h: lqr_carver_cancel, the five small carver-control calls and the two extensions.  LqrDataTok is a union of one
# word (a pointer, a gint, a pointer) passed by value: the C ABI passes it as one integer register, and ctypes, which does not pass
# unions by value, passes it as the pointer-sized integer it is
(LQR_GF_NORM, LQR_GF_NORM_BIAS, LQR_GF_SUMABS, LQR_GF_XABS, LQR_GF_YABS, LQR_GF_NULL) = range(6)
DATA_TOK = C.c_void_p
CARVER_FUNC = C.CFUNCTYPE(C.c_int, C.c_void_p, DATA_TOK)
CONTROL_SYMBOLS = {
    "lqr_carver_cancel": (_I, [_P]),
    "lqr_carver_set_use_cache": (None, [_P, _I]),
    "lqr_carver_set_no_dump_vmaps": (None, [_P]),
    "lqr_carver_list_foreach": (_I, [_P, CARVER_FUNC, DATA_TOK]),
    "lqr_carver_list_foreach_recursive": (_I, [_P, CARVER_FUNC, DATA_TOK]),
    "lqr_carver_set_gradient_function": (None, [_P, _I]),
    "lqrx_carver_cancelled": (_I, [_P]),
    "lqrx_carver_cancel_clear": (_I, [_P]),
}


def bind_control(api):
    """add CONTROL_SYMBOLS to a bound Api; a genuine liblqr-1 has none of the lqrx_ ones"""
    if not getattr(api, "has_control", False):
        for name, (res, args) in CONTROL_SYMBOLS.items():
            if name.startswith("lqrx_") and not api.has_ext:
                continue
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.has_control = True
    return api


# include/lqr_sizes.h: a carver read at many sizes in one pass over its pixels and map
SIZES_SYMBOLS = {
    "lqrx_carver_size_range": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "lqrx_carver_read_sizes_device": (_I, [_P, C.POINTER(_I), _I, C.POINTER(_P)]),
    "lqrx_carver_read_sizes": (_I, [_P, C.POINTER(_I), _I, C.POINTER(_P)]),
}


def bind_sizes(api):
    """add SIZES_SYMBOLS to a bound Api (the engine: a genuine liblqr-1 has none of them); returns it"""
    if not getattr(api, "has_sizes", False):
        for name, (res, args) in SIZES_SYMBOLS.items():
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.has_sizes = True
    return api


# include_ext/lqr_forward.h: forward-energy seam maps built on the device (into device memory, as a caller-owned LqrVMap, for a batch),
# loaded in place, and the resize made of the two.  The engine's own: a genuine liblqr-1 has none of them
FORWARD_SYMBOLS = {
    "lqrx_carver_forward_map_device": (_I, [_P, _I, _I, _P]),
    "lqrx_carver_forward_map": (_P, [_P, _I, _I]),
    "lqrx_carver_forward_maps_device": (_I, [C.POINTER(_P), _I, _I, _I, C.POINTER(_P)]),
    "lqrx_carver_load_forward": (_I, [_P, _I, _I]),
    "lqrx_carver_resize_forward": (_I, [_P, _I, _I]),
}


def bind_forward(api):
    """add FORWARD_SYMBOLS (and VMAP_SYMBOLS) and the build's test hooks to a bound Api (the engine); returns it"""
    bind_vmap(api)
    if not getattr(api, "has_forward", False):
        for name, (res, args) in FORWARD_SYMBOLS.items():
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.lqrhip_forward_launches = api.lib.lqrhip_forward_launches
        api.lqrhip_forward_launches.restype, api.lqrhip_forward_launches.argtypes = C.c_ulonglong, [_I]
        api.lqrhip_read_forward_intensity = api.lib.lqrhip_read_forward_intensity
        api.lqrhip_read_forward_intensity.restype, api.lqrhip_read_forward_intensity.argtypes = _I, [_P, _I, _P]
        api.has_forward = True
    return api


# include_ext/lqr_static.h: static seams for a clip -- the frames folded into one energy plane (to device or host memory), the seam map
# found on it, the map loaded into every frame, and the batch resize made of the two.  The engine's own, as the forward calls are
_F = C.c_float
STATIC_SYMBOLS = {
    "lqrx_carvers_static_energy_device": (_I, [C.POINTER(_P), _I, _I, _F, _P]),
    "lqrx_carvers_static_energy": (_I, [C.POINTER(_P), _I, _I, _F, _P]),
    "lqrx_carvers_static_map": (_P, [C.POINTER(_P), _I, _I, _I, _F, _I, _F]),
    "lqrx_carvers_load_static": (_I, [C.POINTER(_P), _I, _I, _I, _F, _I, _F]),
    "lqrx_carvers_resize_static": (_I, [C.POINTER(_P), _I, _I, _I, _F, _I, _F]),
}


def bind_static(api):
    """add STATIC_SYMBOLS (and what they compose: the forward hooks, seam maps, sizes) to a bound Api (the engine); returns it"""
    bind_sizes(bind_forward(api))
    if not getattr(api, "has_static", False):
        for name, (res, args) in STATIC_SYMBOLS.items():
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.has_static = True
    return api


# include_ext/lqr_clipforward.h: forward-energy seams for a clip -- one seam map from the forward costs of all frames (into device memory
# or as a caller-owned LqrVMap), the map loaded into every frame from device memory, and the batch resize made of the two
CLIPFORWARD_SYMBOLS = {
    "lqrx_clip_forward_map_device": (_I, [C.POINTER(_P), _I, _I, _I, _F, _P]),
    "lqrx_clip_forward_map": (_P, [C.POINTER(_P), _I, _I, _I, _F]),
    "lqrx_clip_load_forward": (_I, [C.POINTER(_P), _I, _I, _I, _F]),
    "lqrx_clip_resize_forward": (_I, [C.POINTER(_P), _I, _I, _I, _F]),
}


def bind_clipforward(api):
    """add CLIPFORWARD_SYMBOLS (and what they compose: the forward hooks, seam maps, sizes) and the build's launch counter to a bound
    Api (the engine); returns it"""
    bind_sizes(bind_forward(api))
    if not getattr(api, "has_clipforward", False):
        for name, (res, args) in CLIPFORWARD_SYMBOLS.items():
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.lqrhip_clipfwd_launches = api.lib.lqrhip_clipfwd_launches
        api.lqrhip_clipfwd_launches.restype, api.lqrhip_clipfwd_launches.argtypes = C.c_ulonglong, [_I]
        api.has_clipforward = True
    return api


# include_ext/lqr_remove.h: object removal -- the scan of the discard mask (which marked pixels are visible, the most in one line) and the
# resize that carves until none is left.  The engine's own, as the forward calls are
LQRX_REMOVE_MIN_STEP = 16
LQRX_ORIENTATION_AUTO = -1
REMOVE_SYMBOLS = {
    "lqrx_carver_discard_scan": (_I, [_P, _I, _F, C.POINTER(_I), C.POINTER(_I)]),
    "lqrx_carver_remove_discarded": (_I, [_P, _I, _F, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
}


def bind_remove(api):
    """add REMOVE_SYMBOLS (and the masks' surface, whose planes they read) and the scan's launch counter to a bound Api (the engine);
    returns it"""
    bind_masks(api)
    if not getattr(api, "has_remove", False):
        for name, (res, args) in REMOVE_SYMBOLS.items():
            fn = getattr(api.lib, api.prefix + name)      # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(api, name, fn)
        api.lqrhip_discard_launches = api.lib.lqrhip_discard_launches
        api.lqrhip_discard_launches.restype, api.lqrhip_discard_launches.argtypes = None, [C.POINTER(C.c_ulonglong), _I]
        api.has_remove = True
    return api


def _vmap_new(api, m):
    """a LqrVMap around a malloc'd copy of m["data"] (h x w int32, image orientation), which the map owns"""
    data = np.ascontiguousarray(m["data"], dtype=np.int32)
    assert data.ndim == 2
    v = bind_vmap(api).lqr_vmap_new(_malloc_copy(data.view(np.uint8)), data.shape[1], data.shape[0], int(m["depth"]), int(m["orientation"]))
    if not v:
        raise MemoryError("lqr_vmap_new returned NULL")
    return v


class Api:
    """Resolved function table of one library exporting the ABI."""

    def __init__(self, path, prefix="", symbols=None):
        self.path, self.prefix = path, prefix
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        self.has_ext = True
        for name in (symbols or SYMBOLS):
            res, args = SYMBOLS[name]
            fn = getattr(self.lib, prefix + name)   # AttributeError = missing export
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)


_apis = {}


def engine_api():
    if "engine" not in _apis:
        if not os.path.exists(ENGINE_LIB):
            raise RuntimeError("HIP engine library missing: %s (run python -c 'import __graft_entry__ as g; g.build()')" % ENGINE_LIB)
        _apis["engine"] = Api(ENGINE_LIB, "")
    return _apis["engine"]


def engine_imagetype_api():
    """the engine with the colour-depth and image-type surfaces bound"""
    return bind_imagetype(engine_api())


def engine_masks_api():
    """the engine with the colour-depth and computed-mask surfaces bound"""
    return bind_masks(engine_api())


def engine_energy_api():
    """the engine with the colour-depth and energy read-out surfaces bound"""
    return bind_energy(engine_api())


def engine_vmap_api():
    """the engine with the colour-depth and seam-map loading surfaces bound"""
    return bind_vmap(bind_coldepth(engine_api()))


def engine_sizes_api():
    """the engine with the colour-depth and many-sizes surfaces bound"""
    return bind_sizes(bind_coldepth(engine_api()))


def engine_forward_api():
    """the engine with the colour-depth, seam-map loading and forward-energy surfaces bound"""
    return bind_forward(bind_coldepth(engine_api()))


def engine_static_api():
    """the engine with everything the static-seam calls compose bound: depths, types, masks, energies, maps, sizes, forward hooks"""
    return bind_static(bind_energy(bind_masks(bind_imagetype(bind_coldepth(engine_api())))))


def engine_clipforward_api():
    """the engine with everything the clip's forward calls compose bound: depths, types, masks, energies, maps, sizes, forward hooks"""
    return bind_clipforward(bind_energy(bind_masks(bind_imagetype(bind_coldepth(engine_api())))))


def engine_remove_api():
    """the engine with everything a removal composes bound: depths, types, masks, seam maps, sizes, control, the two calls"""
    return bind_remove(bind_control(bind_sizes(bind_vmap(bind_imagetype(bind_coldepth(engine_api()))))))


def engine_control_api():
    """the engine with the carver-control surface bound"""
    return bind_control(engine_api())


def engine_coldepth_api():
    """the engine with the colour-depth surface bound"""
    return bind_coldepth(engine_api())


def _malloc_copy(arr):
    """The carver takes ownership of a malloc'd buffer (render.c:220-223)."""
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    p = _libc.malloc(max(arr.nbytes, 1))
    if not p:
        raise MemoryError
    C.memmove(p, arr.ctypes.data, arr.nbytes)
    return p


class Carver:
    """One LqrCarver driven through the C ABI."""

    def __init__(self, api, img, init=True, delta_x=1, rigidity=0.0):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim == 2:
            img = img[:, :, None]
        self.api = api
        self.h0, self.w0, self.ch = img.shape
        self._cbs = []
        self.events = []
        self.p = api.lqr_carver_new(_malloc_copy(img), self.w0, self.h0, self.ch)
        if not self.p:
            raise MemoryError("lqr_carver_new returned NULL")
        self.aux = []
        if init:
            ret = api.lqr_carver_init(self.p, delta_x, float(rigidity))
            assert ret == LQR_OK, ret

    @classmethod
    def from_buffer(cls, api, buf, w, h, ch, delta_x=1, rigidity=0.0):
        """lqr_carver_new + lqr_carver_init (render.c:222-224) on a malloc'ed interleaved u8 buffer the library takes
        ownership of (_malloc_copy): the two C calls and nothing else, for callers that time the upload"""
        self = cls.__new__(cls)
        self.api = api
        self.h0, self.w0, self.ch = h, w, ch
        self._cbs = []
        self.events = []
        self.aux = []
        self.p = api.lqr_carver_new(buf, w, h, ch)
        if not self.p:
            raise MemoryError("lqr_carver_new returned NULL")
        ret = api.lqr_carver_init(self.p, delta_x, float(rigidity))
        assert ret == LQR_OK, ret
        return self

    @classmethod
    def from_ext(cls, api, array, depth=None, init=True, delta_x=1, rigidity=0.0, preserve=False):
        """lqr_carver_new_ext on an h x w (x ch) array of the depth's dtype (depth: LqrColDepth, by default from the dtype).
        preserve=False: the library owns a malloc'ed copy, as liblqr callers hand theirs over.  preserve=True: the carver reads
        the caller's buffer (self.buffer, a numpy array kept alive here) under lqr_carver_set_preserve_input_image"""
        bind_coldepth(api)
        array = np.asarray(array)
        if depth is None:
            depth = {np.dtype(v): k for k, v in COLDEPTH_DTYPES.items()}[array.dtype]
        array = np.ascontiguousarray(array, dtype=COLDEPTH_DTYPES[depth])
        if array.ndim == 2:
            array = array[:, :, None]
        self = cls.__new__(cls)
        self.api = api
        self.h0, self.w0, self.ch = array.shape
        self.depth = depth
        self._cbs, self.events, self.aux = [], [], []
        if preserve:
            self.buffer = array.copy()
            ptr = self.buffer.ctypes.data
        else:
            self.buffer = None
            ptr = _malloc_copy(array.view(np.uint8))
        self.p = api.lqr_carver_new_ext(ptr, self.w0, self.h0, self.ch, depth)
        if not self.p:
            raise MemoryError("lqr_carver_new_ext returned NULL")
        if preserve:
            api.lqr_carver_set_preserve_input_image(self.p)
        if init:
            ret = api.lqr_carver_init(self.p, delta_x, float(rigidity))
            assert ret == LQR_OK, ret
        return self

    def init(self, delta_x=1, rigidity=0.0):
        """lqr_carver_init on a carver made with init=False; returns the LqrRetVal"""
        return self.api.lqr_carver_init(self.p, int(delta_x), float(rigidity))

    def attach_ext(self, array, depth=None):
        """an attached carver of any depth"""
        aux = Carver.from_ext(self.api, array, depth, init=False)
        ret = self.api.lqr_carver_attach(self.p, aux.p)
        assert ret == LQR_OK, ret
        self.aux.append(aux)
        return aux

    # -- the image type (include/lqr_imagetype.h); each returns the call's LqrRetVal
    def set_image_type(self, image_type):
        return bind_imagetype(self.api).lqr_carver_set_image_type(self.p, int(image_type))

    def set_alpha_channel(self, index):
        return bind_imagetype(self.api).lqr_carver_set_alpha_channel(self.p, int(index))

    def set_black_channel(self, index):
        return bind_imagetype(self.api).lqr_carver_set_black_channel(self.p, int(index))

    def _px(self):
        depth = getattr(self, "depth", LQR_COLDEPTH_8I)
        dt = np.dtype(COLDEPTH_DTYPES[depth])
        return dt, self.ch * dt.itemsize

    def scan_partial(self):
        """a lqr_carver_scan_ext loop given up part-way: all but the last pixel of the first line; returns the pixels visited"""
        a = self.api
        W, H = a.lqr_carver_get_width(self.p), a.lqr_carver_get_height(self.p)
        n = (W if a.lqr_carver_scan_by_row(self.p) else H) - 1
        x, y, px = C.c_int(0), C.c_int(0), C.c_void_p()
        a.lqr_carver_scan_reset(self.p)
        for _ in range(n):
            assert a.lqr_carver_scan_ext(self.p, C.byref(x), C.byref(y), C.byref(px))
        return n

    def scan_ext(self, reset=True):
        """the lqr_carver_scan_ext loop: (image, [(x, y) in visiting order]); reset=False: from wherever the cursor is"""
        a = self.api
        dt, nb = self._px()
        W, H = a.lqr_carver_get_width(self.p), a.lqr_carver_get_height(self.p)
        out = np.zeros((H, W, self.ch), dt)
        x, y, px = C.c_int(0), C.c_int(0), C.c_void_p()
        order = []
        if reset:
            a.lqr_carver_scan_reset(self.p)
        while a.lqr_carver_scan_ext(self.p, C.byref(x), C.byref(y), C.byref(px)):
            out[y.value, x.value] = np.frombuffer(C.string_at(px.value, nb), dt)
            order.append((x.value, y.value))
        return out, order

    def scan_line_ext(self):
        """the lqr_carver_scan_line_ext loop: (image, [line numbers in order])"""
        a = self.api
        dt, nb = self._px()
        W, H = a.lqr_carver_get_width(self.p), a.lqr_carver_get_height(self.p)
        out = np.zeros((H, W, self.ch), dt)
        n, line = C.c_int(0), C.c_void_p()
        lines = []
        a.lqr_carver_scan_reset(self.p)
        while a.lqr_carver_scan_line_ext(self.p, C.byref(n), C.byref(line)):
            by_row = a.lqr_carver_scan_by_row(self.p)
            length = W if by_row else H
            buf = np.frombuffer(C.string_at(line.value, length * nb), dt).reshape(length, self.ch)
            if by_row:
                out[n.value] = buf
            else:
                out[:, n.value] = buf
            lines.append(n.value)
        return out, lines

    def read_image_ext(self):
        """lqrx_carver_read_image at the carver's depth (engine only)"""
        a = self.api
        dt, _ = self._px()
        W, H = a.lqr_carver_get_width(self.p), a.lqr_carver_get_height(self.p)
        out = np.zeros((H, W, self.ch), dt)
        assert a.lqrx_carver_read_image(self.p, out.ctypes.data) == LQR_OK
        return out

    def input_bytes(self):
        """the caller's buffer as it is now (preserve=True only)"""
        return self.buffer.tobytes()

    def free_input(self):
        """(preserve=True: the buffer is self.buffer, numpy's; nothing to hand back)"""

    def scan_rets(self):
        """what the 8-bit scans return on this carver (first call after a reset)"""
        a = self.api
        x, y, px = C.c_int(0), C.c_int(0), C.c_void_p()
        a.lqr_carver_scan_reset(self.p)
        r1 = a.lqr_carver_scan(self.p, C.byref(x), C.byref(y), C.byref(px))
        a.lqr_carver_scan_reset(self.p)
        r2 = a.lqr_carver_scan_line(self.p, C.byref(x), C.byref(px))
        a.lqr_carver_scan_reset(self.p)
        return [r1, r2]

    def getters_ext(self):
        a = self.api
        g = self.getters()
        g.update(col_depth=a.lqr_carver_get_col_depth(self.p), image_type=a.lqr_carver_get_image_type(self.p),
                 bpp=a.lqr_carver_get_bpp(self.p))
        return g

    # -- configuration, in the order of render.c:225-248 ------------------
    def bias_add(self, mask, factor, x_off=0, y_off=0):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if mask.ndim == 2:
            mask = mask[:, :, None]
        h, w, ch = mask.shape
        return self.api.lqr_carver_bias_add_rgb_area(self.p, mask.ctypes.data, int(factor), ch, w, h, x_off, y_off)

    def rigmask_add(self, mask, x_off=0, y_off=0):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if mask.ndim == 2:
            mask = mask[:, :, None]
        h, w, ch = mask.shape
        return self.api.lqr_carver_rigmask_add_rgb_area(self.p, mask.ctypes.data, ch, w, h, x_off, y_off)

    # -- computed masks (include/lqr_masks.h); each returns the call's LqrRetVal.  Masks are h x w arrays of float64
    @staticmethod
    def _fmask(mask):
        mask = np.ascontiguousarray(mask, dtype=np.float64)
        assert mask.ndim == 2
        return mask

    def bias_add_f(self, mask, factor, x_off=None, y_off=None):
        """lqr_carver_bias_add_area; without offsets lqr_carver_bias_add (the mask must then have the carver's size)"""
        a, mask = bind_masks(self.api), self._fmask(mask)
        if x_off is None:
            return a.lqr_carver_bias_add(self.p, mask.ctypes.data, int(factor))
        return a.lqr_carver_bias_add_area(self.p, mask.ctypes.data, int(factor), mask.shape[1], mask.shape[0], int(x_off), int(y_off))

    def rigmask_add_f(self, mask, x_off=None, y_off=None):
        a, mask = bind_masks(self.api), self._fmask(mask)
        if x_off is None:
            return a.lqr_carver_rigmask_add(self.p, mask.ctypes.data)
        return a.lqr_carver_rigmask_add_area(self.p, mask.ctypes.data, mask.shape[1], mask.shape[0], int(x_off), int(y_off))

    def bias_add_rgb(self, mask, factor):
        """lqr_carver_bias_add_rgb: an 8-bit mask of the carver's size"""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        return bind_masks(self.api).lqr_carver_bias_add_rgb(self.p, mask.ctypes.data, int(factor), 1 if mask.ndim == 2 else mask.shape[2])

    def rigmask_add_rgb(self, mask):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        return bind_masks(self.api).lqr_carver_rigmask_add_rgb(self.p, mask.ctypes.data, 1 if mask.ndim == 2 else mask.shape[2])

    def bias_add_xy(self, entries):
        """one lqr_carver_bias_add_xy per (x, y, value), in order; returns the list of return values"""
        f = bind_masks(self.api).lqr_carver_bias_add_xy
        return [f(self.p, float(v), int(x), int(y)) for x, y, v in entries]

    def rigmask_add_xy(self, entries):
        f = bind_masks(self.api).lqr_carver_rigmask_add_xy
        return [f(self.p, float(v), int(x), int(y)) for x, y, v in entries]

    def _add_device(self, fn, tensor, more, x_off, y_off):
        """tensor: a contiguous h x w float32 / float64 torch tensor on the device"""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.dim() == 2
        depth = {torch.float32: LQR_COLDEPTH_32F, torch.float64: LQR_COLDEPTH_64F}[tensor.dtype]
        torch.cuda.current_stream().synchronize()          # the engine reads the buffer on a stream of its own
        return fn(self.p, tensor.data_ptr(), depth, *more, tensor.shape[1], tensor.shape[0], int(x_off), int(y_off))

    def bias_add_device(self, tensor, factor, x_off=0, y_off=0):
        return self._add_device(bind_masks(self.api).lqrx_carver_bias_add_area_device, tensor, [int(factor)], x_off, y_off)

    def rigmask_add_device(self, tensor, x_off=0, y_off=0):
        return self._add_device(bind_masks(self.api).lqrx_carver_rigmask_add_area_device, tensor, [], x_off, y_off)

    def bias_clear(self):
        bind_masks(self.api).lqr_carver_bias_clear(self.p)

    def rigmask_clear(self):
        bind_masks(self.api).lqr_carver_rigmask_clear(self.p)

    def _get_plane(self, fn):
        a = self.api
        out = np.zeros((a.lqr_carver_get_height(self.p), a.lqr_carver_get_width(self.p)), np.float32)
        ret = fn(self.p, out.ctypes.data)
        assert ret == LQR_OK, ret
        return out

    def get_bias(self):
        """the bias plane of a flat carver in image orientation (zeros if there is none)"""
        return self._get_plane(bind_masks(self.api).lqrx_carver_get_bias)

    def get_rigmask(self):
        return self._get_plane(bind_masks(self.api).lqrx_carver_get_rigmask)

    # -- the energy read-outs (include/lqr_energy.h)
    def energy_call(self, form, orientation, depth=LQR_COLDEPTH_32F, image_type=LQR_GREY_IMAGE, nbytes=0, guard=64, null=False):
        """one read-out (form 0 lqr_carver_get_true_energy, 1 lqr_carver_get_energy, 2 lqr_carver_get_energy_image) into a buffer of
        nbytes + guard bytes of 0xA5 (null: a NULL buffer): (LqrRetVal, the bytes afterwards)"""
        a = bind_energy(self.api)
        buf = np.full(nbytes + guard, 0xa5, np.uint8)
        ptr = None if null else buf.ctypes.data
        if form == 2:
            ret = a.lqr_carver_get_energy_image(self.p, ptr, int(orientation), int(depth), int(image_type))
        else:
            ret = (a.lqr_carver_get_energy if form else a.lqr_carver_get_true_energy)(self.p, ptr, int(orientation))
        return ret, buf

    def _image_size(self):
        return self.api.lqr_carver_get_height(self.p), self.api.lqr_carver_get_width(self.p)

    def get_energy(self, orientation, true=False):
        """lqr_carver_get_energy (true=True: lqr_carver_get_true_energy) as seams of `orientation` see it: height x width float32 in
        image orientation.  The carver is left in that orientation"""
        h, w = self._image_size()
        ret, buf = self.energy_call(0 if true else 1, orientation, nbytes=4 * w * h, guard=0)
        assert ret == LQR_OK, ret
        return buf.view(np.float32).reshape(h, w)

    def get_energy_image(self, orientation, depth, image_type):
        """lqr_carver_get_energy_image: height x width x channels of the depth's dtype"""
        h, w = self._image_size()
        dt, ch = np.dtype(COLDEPTH_DTYPES[depth]), IMAGE_TYPE_CHANNELS[image_type]
        ret, buf = self.energy_call(2, orientation, depth, image_type, nbytes=w * h * ch * dt.itemsize, guard=0)
        assert ret == LQR_OK, ret
        return buf.view(dt).reshape(h, w, ch)

    def get_energy_device(self, tensor, orientation, true=False):
        """the float forms into a contiguous float32 torch tensor of height x width elements on the device; returns the LqrRetVal"""
        h, w = self._image_size()
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype == torch.float32 and tensor.numel() == h * w
        torch.cuda.current_stream().synchronize()          # the engine writes the buffer on a stream of its own
        return bind_energy(self.api).lqrx_carver_get_energy_device(self.p, tensor.data_ptr(), int(orientation), 0 if true else 1)

    def get_energy_image_device(self, tensor, orientation, depth, image_type):
        """the picture into a contiguous torch tensor of height x width x channels elements of the depth's dtype on the device"""
        h, w = self._image_size()
        dt = {LQR_COLDEPTH_8I: torch.uint8, LQR_COLDEPTH_16I: (torch.uint16, torch.int16), LQR_COLDEPTH_32F: torch.float32,
              LQR_COLDEPTH_64F: torch.float64}[depth]
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == h * w * IMAGE_TYPE_CHANNELS[image_type]
        assert tensor.dtype in dt if isinstance(dt, tuple) else tensor.dtype == dt
        torch.cuda.current_stream().synchronize()
        return bind_energy(self.api).lqrx_carver_get_energy_image_device(self.p, tensor.data_ptr(), int(orientation), int(depth), int(image_type))

    def configure(self, nrg_func=LQR_EF_GRAD_XABS, res_order=LQR_RES_ORDER_HOR, switch_freq=2,
                  enl_step=1.5, dump_vmaps=False, progress=False):
        a = self.api
        assert a.lqr_carver_set_energy_function_builtin(self.p, nrg_func) == LQR_OK
        a.lqr_carver_set_resize_order(self.p, res_order)
        if progress:
            self.set_progress_recorder()
        a.lqr_carver_set_side_switch_frequency(self.p, switch_freq)
        assert a.lqr_carver_set_enl_step(self.p, float(enl_step)) == LQR_OK
        if dump_vmaps:
            a.lqr_carver_set_dump_vmaps(self.p)
        return self

    def set_energy(self, nrg_func):
        """change the built-in energy function of a carver that may already have been resized"""
        return self.api.lqr_carver_set_energy_function_builtin(self.p, nrg_func)

    def set_progress_recorder(self):
        a = self.api
        prog = a.lqr_progress_new()
        ev = self.events
        cb_i = PROGRESS_INIT(lambda m: (ev.append(("init", m.decode())), 1)[1])
        cb_u = PROGRESS_UPDATE(lambda f: (ev.append(("update", f)), self._on_event("update"), 1)[2])
        cb_e = PROGRESS_END(lambda m: (ev.append(("end", m.decode() if m else "")), self._on_event("end"), 1)[2])
        self._cbs += [cb_i, cb_u, cb_e]
        a.lqr_progress_set_init(prog, cb_i)
        a.lqr_progress_set_update(prog, cb_u)
        a.lqr_progress_set_end(prog, cb_e)
        a.lqr_progress_set_init_width_message(prog, b"Resizing width...")
        a.lqr_progress_set_init_height_message(prog, b"Resizing height...")
        a.lqr_carver_set_progress(self.p, prog)

    # -- carver control (include/lqr_control.h)
    def cancel(self):
        """lqr_carver_cancel; the LqrRetVal.  The one call another thread may make while this carver is inside a call"""
        return bind_control(self.api).lqr_carver_cancel(self.p)

    def cancelled(self):
        return bind_control(self.api).lqrx_carver_cancelled(self.p)

    def cancel_clear(self):
        return bind_control(self.api).lqrx_carver_cancel_clear(self.p)

    def cancel_at_update(self, n, target=None, via=None, event="update"):
        """the recorder's n-th update callback from now on (0: disarmed; event="end": its n-th end callback) calls lqr_carver_cancel on
        `target` (this carver by default); via: a callable that makes the call in its place (a test's second thread) and returns its
        LqrRetVal"""
        self._hook = dict(at=int(n), seen=0, target=target or self, via=via, event=event, fired=False, ret=0) if n else None

    def cancel_result(self):
        """(whether the armed call was made, what it returned)"""
        h = getattr(self, "_hook", None)
        return (h["fired"], h["ret"]) if h else (False, 0)

    def _on_event(self, event):
        h = getattr(self, "_hook", None)
        if h and not h["fired"] and h["event"] == event:
            h["seen"] += 1
            if h["seen"] == h["at"]:
                h["ret"] = h["via"](h["target"]) if h["via"] else h["target"].cancel()
                h["fired"] = True

    def set_use_cache(self, on):
        bind_control(self.api).lqr_carver_set_use_cache(self.p, int(on))

    def set_dump_vmaps(self):
        self.api.lqr_carver_set_dump_vmaps(self.p)

    def set_no_dump_vmaps(self):
        bind_control(self.api).lqr_carver_set_no_dump_vmaps(self.p)

    def set_gradient_function(self, gf):
        bind_control(self.api).lqr_carver_set_gradient_function(self.p, int(gf))

    def list_foreach(self, recursive=False, stop_at=0, stop_ret=0, token=0):
        """lqr_carver_list_foreach (_recursive) over the attached carvers with a callback that returns stop_ret at its stop_at-th call
        (0: never): (LqrRetVal, [index of each visited carver in self.aux], [the tokens the callback saw])"""
        a = bind_control(self.api)
        seen = []

        def cb(carver, tok):
            seen.append((carver, tok or 0))
            return stop_ret if stop_at and len(seen) == stop_at else LQR_OK
        fn = CARVER_FUNC(cb)
        f = a.lqr_carver_list_foreach_recursive if recursive else a.lqr_carver_list_foreach
        ret = f(a.lqr_carver_list_start(self.p), fn, token)
        ps = [x.p for x in self.aux]
        return ret, [ps.index(c) for c, _ in seen], [t for _, t in seen]

    def attach(self, img):
        """attach_aux_carver, render.c:881-900"""
        aux = Carver(self.api, img, init=False)
        ret = self.api.lqr_carver_attach(self.p, aux.p)
        assert ret == LQR_OK, ret
        self.aux.append(aux)
        return aux

    # -- run ---------------------------------------------------------------
    def resize(self, w1, h1):
        return self.api.lqr_carver_resize(self.p, int(w1), int(h1))

    def flatten(self):
        return self.api.lqr_carver_flatten(self.p)

    # -- readout: the loop of io_functions.c:155-164 -------------------------
    def read_scanlines(self):
        a = self.api
        W, H, ch = a.lqr_carver_get_width(self.p), a.lqr_carver_get_height(self.p), self.ch
        out = np.zeros((H, W, ch), np.uint8)
        n, line = C.c_int(0), C.c_void_p()
        count = 0
        a.lqr_carver_scan_reset(self.p)
        while a.lqr_carver_scan_line(self.p, C.byref(n), C.byref(line)):
            by_row = a.lqr_carver_scan_by_row(self.p)
            length = W if by_row else H
            buf = np.ctypeslib.as_array(C.cast(line, C.POINTER(C.c_ubyte)), shape=(length * ch,)).reshape(length, ch)
            if by_row:
                out[n.value] = buf
            else:
                out[:, n.value] = buf
            count += 1
        return out, count

    def read_image(self):
        a = self.api
        if not a.has_ext:
            return self.read_scanlines()[0]
        W, H = a.lqr_carver_get_width(self.p), a.lqr_carver_get_height(self.p)
        out = np.zeros((H, W, self.ch), np.uint8)
        assert a.lqrx_carver_read_image(self.p, out.ctypes.data) == LQR_OK
        return out

    def getters(self):
        a = self.api
        return dict(width=a.lqr_carver_get_width(self.p), height=a.lqr_carver_get_height(self.p),
                    channels=a.lqr_carver_get_channels(self.p), ref_width=a.lqr_carver_get_ref_width(self.p),
                    ref_height=a.lqr_carver_get_ref_height(self.p), orientation=a.lqr_carver_get_orientation(self.p),
                    depth=a.lqr_carver_get_depth(self.p), enl_step=a.lqr_carver_get_enl_step(self.p))

    def _vmap_to_dict(self, v):
        a = self.api
        w, h = a.lqr_vmap_get_width(v), a.lqr_vmap_get_height(v)
        data = np.ctypeslib.as_array(a.lqr_vmap_get_data(v), shape=(h * w,)).reshape(h, w).copy()
        return dict(data=data, depth=a.lqr_vmap_get_depth(v), orientation=a.lqr_vmap_get_orientation(v))

    def vmap_dump(self):
        v = self.api.lqr_vmap_dump(self.p)
        assert v
        d = self._vmap_to_dict(v)
        self.api.lqr_vmap_destroy(v)
        return d

    # -- loading a seam map (include/lqr_vmap.h); each returns the call's LqrRetVal
    def vmap_load(self, m):
        """lqr_vmap_load of the dict vmap_dump returns (data: h x w int32 in image orientation, depth, orientation)"""
        a = bind_vmap(self.api)
        v = _vmap_new(a, m)
        ret = a.lqr_vmap_load(self.p, v)
        a.lqr_vmap_destroy(v)
        return ret

    def vmap_load_device(self, tensor, depth, orientation):
        """lqrx_vmap_load_device: a contiguous h x w int32 torch tensor on the device, read where it lies"""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.dim() == 2 and tensor.dtype == torch.int32
        torch.cuda.current_stream().synchronize()          # the engine reads the buffer on a stream of its own
        return bind_vmap(self.api).lqrx_vmap_load_device(self.p, tensor.data_ptr(), tensor.shape[1], tensor.shape[0], int(depth), int(orientation))


    # -- forward-energy seam maps (include_ext/lqr_forward.h)
    def _forward_line(self, orientation):
        a = self.api
        return a.lqr_carver_get_height(self.p) if orientation else a.lqr_carver_get_width(self.p)

    def forward_map(self, depth, orientation):
        """lqrx_carver_forward_map: the dict vmap_dump returns, or None where the call returned NULL"""
        a = bind_forward(self.api)
        v = a.lqrx_carver_forward_map(self.p, int(depth), int(orientation))
        if not v:
            return None
        d = self._vmap_to_dict(v)
        a.lqr_vmap_destroy(v)
        return d

    def forward_map_device(self, tensor, depth, orientation):
        """lqrx_carver_forward_map_device into a contiguous h x w int32 torch tensor on the device; the LqrRetVal"""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype == torch.int32
        assert tensor.numel() >= self.api.lqr_carver_get_width(self.p) * self.api.lqr_carver_get_height(self.p)
        torch.cuda.current_stream().synchronize()          # the engine writes the buffer on a stream of its own
        return bind_forward(self.api).lqrx_carver_forward_map_device(self.p, int(depth), int(orientation), tensor.data_ptr())

    def load_forward(self, depth, orientation):
        return bind_forward(self.api).lqrx_carver_load_forward(self.p, int(depth), int(orientation))

    def resize_forward(self, w1, h1):
        return bind_forward(self.api).lqrx_carver_resize_forward(self.p, int(w1), int(h1))

    def forward_intensity(self, orientation):
        """test hook: the I plane a forward build forms for this (flat) carver, lines x line length float32 in the carving frame"""
        a = bind_forward(self.api)
        w, h = a.lqr_carver_get_width(self.p), a.lqr_carver_get_height(self.p)
        out = np.zeros((w, h) if orientation else (h, w), np.float32)
        ret = a.lqrhip_read_forward_intensity(self.p, int(orientation), out.ctypes.data)
        assert ret == 0, ret
        return out

    # -- object removal (include_ext/lqr_remove.h)
    def discard_scan(self, orientation, strength=0.0):
        """lqrx_carver_discard_scan: (LqrRetVal, marked, need)"""
        marked, need = C.c_int(-1), C.c_int(-1)
        ret = bind_remove(self.api).lqrx_carver_discard_scan(self.p, int(orientation), float(strength), C.byref(marked), C.byref(need))
        return ret, marked.value, need.value

    def remove_discarded(self, orientation, strength=0.0, max_seams=1 << 20, restore=False):
        """lqrx_carver_remove_discarded: dict(ret, orientation_used, seams, left); the three are None where the call did not write them"""
        o, seams, left = C.c_int(-9), C.c_int(-9), C.c_int(-9)
        ret = bind_remove(self.api).lqrx_carver_remove_discarded(self.p, int(orientation), float(strength), int(max_seams), int(bool(restore)),
                                                                 C.byref(o), C.byref(seams), C.byref(left))
        val = lambda v: None if v.value == -9 else v.value
        return dict(ret=ret, orientation_used=val(o), seams=val(seams), left=val(left))

    # -- many sizes in one pass (include/lqr_sizes.h)
    def size_range(self):
        """lqrx_carver_size_range: (direction, smallest size, largest size)"""
        lo, hi = C.c_int(0), C.c_int(0)
        d = bind_sizes(self.api).lqrx_carver_size_range(self.p, C.byref(lo), C.byref(hi))
        return d, lo.value, hi.value

    def _sizes_shape(self, size):
        """the image at `size` in the direction of the map: (rows, columns, channels)"""
        a = self.api
        if a.lqr_carver_get_orientation(self.p):
            return int(size), a.lqr_carver_get_width(self.p), self.ch
        return a.lqr_carver_get_height(self.p), int(size), self.ch

    def read_sizes(self, sizes):
        """lqrx_carver_read_sizes: a list of numpy arrays (rows x columns x channels of the carver's dtype), one per size"""
        dt, _ = self._px()
        outs = [np.zeros(self._sizes_shape(s), dt) for s in sizes]
        arr = (C.c_int * len(outs))(*[int(s) for s in sizes])
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        ret = bind_sizes(self.api).lqrx_carver_read_sizes(self.p, arr, len(outs), ptrs)
        if ret != LQR_OK:
            raise MemoryError("lqrx_carver_read_sizes") if ret == LQR_NOMEM else ValueError("lqrx_carver_read_sizes returned %d" % ret)
        return outs

    def read_sizes_device(self, sizes, tensors):
        """lqrx_carver_read_sizes_device into torch tensors on the device, one per size: each contiguous, of the carver's dtype (any
        dtype of the same item size) and of at least rows x columns x channels elements; returns the LqrRetVal"""
        dt, _ = self._px()
        assert len(sizes) == len(tensors)
        for s, t in zip(sizes, tensors):
            rows, cols, ch = self._sizes_shape(s)
            assert t.is_cuda and t.is_contiguous() and t.element_size() == dt.itemsize and t.numel() >= rows * cols * ch
        torch.cuda.current_stream().synchronize()          # the engine writes the buffers on a stream of its own
        arr = (C.c_int * len(sizes))(*[int(s) for s in sizes])
        ptrs = (C.c_void_p * len(sizes))(*[t.data_ptr() for t in tensors])
        return bind_sizes(self.api).lqrx_carver_read_sizes_device(self.p, arr, len(sizes), ptrs)

    def vmap_internal_dump(self):
        return bind_vmap(self.api).lqr_vmap_internal_dump(self.p)

    def dumped_vmaps(self):
        """write_all_vmaps, io_functions.c:292-314: foreach over the carver's list"""
        out = []

        def cb(v, _):
            out.append(self._vmap_to_dict(v))
            return LQR_OK
        fn = VMAP_FUNC(cb)
        ret = self.api.lqr_vmap_list_foreach(self.api.lqr_vmap_list_start(self.p), fn, None)
        assert ret == LQR_OK
        return out

    def energy(self):
        a = self.api
        ret_w = a.lqrx_carver_frame_width(self.p)
        ret_h = a.lqrx_carver_frame_height(self.p)
        buf = np.zeros((ret_h, ret_w), np.float32)
        ret = a.lqrx_carver_get_energy(self.p, buf.ctypes.data)
        assert ret == LQR_OK, ret
        w, h = a.lqrx_carver_frame_width(self.p), a.lqrx_carver_frame_height(self.p)
        if (w, h) != (ret_w, ret_h):      # the call flattened the carver
            buf = np.zeros((h, w), np.float32)
            assert a.lqrx_carver_get_energy(self.p, buf.ctypes.data) == LQR_OK
        return buf

    def debug_snapshot(self):
        a = self.api
        w, h = a.lqrx_carver_debug_width(self.p), a.lqrx_carver_debug_height(self.p)
        en, m, dx = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.int32)
        assert a.lqrx_carver_debug_snapshot(self.p, en.ctypes.data, m.ctypes.data, dx.ctypes.data) == LQR_OK
        return en, m, dx

    def destroy(self):
        if self.p:
            self.api.lqr_carver_destroy(self.p)   # also frees attached carvers
            self.p = None
            for x in self.aux:
                x.p = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def vmap_to_rgba(api, vmap_dict_or_ptr, col_start, col_end, carver=None):
    """write_vmap_to_layer's colour ramp (io_functions.c:249-279) over a dumped map; returns h x w x 4 u8.
    `vmap_dict_or_ptr` is a LqrVMap* (c_void_p / int)."""
    v = vmap_dict_or_ptr
    w, h = api.lqr_vmap_get_width(v), api.lqr_vmap_get_height(v)
    out = np.zeros((h, w, 4), np.uint8)
    cs = (C.c_double * 3)(*[float(x) for x in col_start])
    ce = (C.c_double * 3)(*[float(x) for x in col_end])
    ret = api.lqrx_vmap_to_rgba(v, cs, ce, out.ctypes.data)
    assert ret == LQR_OK, ret
    return out


def reload_device_batch(api, carvers, device_ptrs):
    arr = (C.c_void_p * len(carvers))(*[c.p for c in carvers])
    ptrs = (C.c_void_p * len(carvers))(*[int(p) for p in device_ptrs])
    return api.lqrx_carver_reload_device_batch(arr, len(carvers), ptrs)


def vmap_load_batch(carvers, m):
    """lqrx_vmap_load_batch: one map (the dict vmap_dump returns) into every carver of the list; the LqrRetVal"""
    a = bind_vmap(carvers[0].api)
    arr = (C.c_void_p * len(carvers))(*[c.p for c in carvers])
    v = _vmap_new(a, m)
    ret = a.lqrx_vmap_load_batch(arr, len(carvers), v)
    a.lqr_vmap_destroy(v)
    return ret


def resize_batch(api, carvers, w1, h1):
    arr = (C.c_void_p * len(carvers))(*[c.p for c in carvers])
    return api.lqrx_carver_resize_batch(arr, len(carvers), int(w1), int(h1))


def forward_maps_device(carvers, tensors, depth, orientation):
    """lqrx_carver_forward_maps_device: one contiguous int32 torch tensor on the device per carver; the LqrRetVal"""
    a = bind_forward(carvers[0].api)
    for t in tensors:
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int32
    torch.cuda.current_stream().synchronize()
    arr = (C.c_void_p * len(carvers))(*[c.p for c in carvers])
    ptrs = (C.c_void_p * len(carvers))(*[t.data_ptr() for t in tensors])
    return a.lqrx_carver_forward_maps_device(arr, len(carvers), int(depth), int(orientation), ptrs)


def _frames(carvers):
    return (C.c_void_p * len(carvers))(*[c.p for c in carvers])


def static_energy(carvers, orientation, alpha, guard=0):
    """lqrx_carvers_static_energy: (LqrRetVal, h x w float32 in image orientation, the `guard` bytes after it -- 0xA5 when intact)"""
    a = bind_static(carvers[0].api)
    w, h = a.lqr_carver_get_width(carvers[0].p), a.lqr_carver_get_height(carvers[0].p)
    buf = np.full(w * h * 4 + guard, 0xa5, np.uint8)
    ret = a.lqrx_carvers_static_energy(_frames(carvers), len(carvers), int(orientation), float(alpha), buf.ctypes.data)
    return ret, buf[:w * h * 4].view(np.float32).reshape(h, w).copy(), buf[w * h * 4:].copy()


def static_energy_device(carvers, tensor, orientation, alpha):
    """lqrx_carvers_static_energy_device into a contiguous float32 torch tensor on the device; the LqrRetVal"""
    a = bind_static(carvers[0].api)
    assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype == torch.float32
    assert tensor.numel() >= a.lqr_carver_get_width(carvers[0].p) * a.lqr_carver_get_height(carvers[0].p)
    torch.cuda.current_stream().synchronize()          # the engine writes the buffer on a stream of its own
    return a.lqrx_carvers_static_energy_device(_frames(carvers), len(carvers), int(orientation), float(alpha), tensor.data_ptr())


def static_map(carvers, depth, orientation, alpha, delta_x=1, rigidity=0.0):
    """lqrx_carvers_static_map: the dict vmap_dump returns, or None where the call returned NULL"""
    a = bind_static(carvers[0].api)
    v = a.lqrx_carvers_static_map(_frames(carvers), len(carvers), int(depth), int(orientation), float(alpha), int(delta_x), float(rigidity))
    if not v:
        return None
    d = carvers[0]._vmap_to_dict(v)
    a.lqr_vmap_destroy(v)
    return d


def load_static(carvers, depth, orientation, alpha, delta_x=1, rigidity=0.0):
    a = bind_static(carvers[0].api)
    return a.lqrx_carvers_load_static(_frames(carvers), len(carvers), int(depth), int(orientation), float(alpha), int(delta_x), float(rigidity))


def resize_static(carvers, w1, h1, alpha, delta_x=1, rigidity=0.0):
    a = bind_static(carvers[0].api)
    return a.lqrx_carvers_resize_static(_frames(carvers), len(carvers), int(w1), int(h1), float(alpha), int(delta_x), float(rigidity))


def clip_forward_map(carvers, depth, orientation, temporal):
    """lqrx_clip_forward_map: the dict vmap_dump returns, or None where the call returned NULL"""
    a = bind_clipforward(carvers[0].api)
    v = a.lqrx_clip_forward_map(_frames(carvers), len(carvers), int(depth), int(orientation), float(temporal))
    if not v:
        return None
    d = carvers[0]._vmap_to_dict(v)
    a.lqr_vmap_destroy(v)
    return d


def clip_forward_map_device(carvers, tensor, depth, orientation, temporal):
    """lqrx_clip_forward_map_device into a contiguous h x w int32 torch tensor on the device; the LqrRetVal"""
    a = bind_clipforward(carvers[0].api)
    assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype == torch.int32
    assert tensor.numel() >= a.lqr_carver_get_width(carvers[0].p) * a.lqr_carver_get_height(carvers[0].p)
    torch.cuda.current_stream().synchronize()          # the engine writes the buffer on a stream of its own
    return a.lqrx_clip_forward_map_device(_frames(carvers), len(carvers), int(depth), int(orientation), float(temporal), tensor.data_ptr())


def clip_load_forward(carvers, depth, orientation, temporal):
    a = bind_clipforward(carvers[0].api)
    return a.lqrx_clip_load_forward(_frames(carvers), len(carvers), int(depth), int(orientation), float(temporal))


def clip_resize_forward(carvers, w1, h1, temporal):
    a = bind_clipforward(carvers[0].api)
    return a.lqrx_clip_resize_forward(_frames(carvers), len(carvers), int(w1), int(h1), float(temporal))
