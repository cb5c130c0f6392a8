"""The reference's debug images (TestRenderStereoPanorama --save_debug_images, TestPoleRemoval) of a frame rendered on the device:
Python mirror of include/s360_debug_images.h, and of the test tap include/s360_debug_views.h. Every function takes the
render.Context it works on."""
import ctypes as C

import numpy as np

from ._capi import DebugView, lib
from .render import _p, _u8


def set_debug_images(ctx, on=True):
    """s360_set_debug_images: the frames rendered from now on keep the reference's debug images (one frame at a time: no frame
    pipelining, one frame slot, a render call returns when its frame is complete)."""
    ctx._ck(lib().s360_set_debug_images(ctx.h, int(bool(on))))


def debug_image_list(ctx):
    """[(name, w, h, channels)] of the selected slot's latest frame, in the library's fixed order; name is the reference's path
    relative to debug/<frame>/."""
    n = ctx._ck(lib().s360_frame_debug_image_count(ctx.h))
    out = []
    for i in range(n):
        name = C.create_string_buffer(96)
        whc = (C.c_int * 3)()
        ctx._ck(lib().s360_frame_debug_image_info(ctx.h, i, name, whc))
        out.append((name.value.decode(), whc[0], whc[1], whc[2]))
    return out


def get_debug_image(ctx, i):
    """Image i as an (h, w, channels) uint8 array, B,G,R[,A]."""
    name = C.create_string_buffer(96)
    whc = (C.c_int * 3)()
    ctx._ck(lib().s360_frame_debug_image_info(ctx.h, int(i), name, whc))
    d = np.empty((whc[1], whc[0], whc[2]), np.uint8)
    ctx._ck(lib().s360_frame_get_debug_image(ctx.h, int(i), _p(d)))
    return d


def encode_debug_pngs(ctx):
    """s360_frame_encode_debug_pngs: enqueues the batched encode of every image of the list; waits for nothing."""
    ctx._ck(lib().s360_frame_encode_debug_pngs(ctx.h))


def debug_png_bound(ctx, i):
    return int(lib().s360_frame_debug_png_bound(ctx.h, int(i)))


def download_debug_png(ctx, i, out=None):
    """File i of the last encode_debug_pngs call: a view of its bytes in `out` (a uint8 buffer; default: one of the file's bound)."""
    if out is None:
        out = np.empty(max(debug_png_bound(ctx, i), 1), np.uint8)
    assert out.dtype == np.uint8 and out.ndim == 1 and out.flags["C_CONTIGUOUS"]
    n = C.c_size_t(0)
    ctx._ck(lib().s360_frame_download_debug_png(ctx.h, int(i), _p(out), C.c_size_t(out.size), C.byref(n)))
    return out[:n.value]


def pole_removal_combine(ctx, bottom, bottom2, mask, mask2, radius, radius2, flip180, feather_size=31, flow_alg="pixflow_low"):
    """s360_pole_removal_combine on four (h, w, 3) B,G,R images: {"bottomImage", "bottomImage2", "bottomWarp2", "_bottomCombined"}
    -> (h, w, 4) B,G,R,A arrays, and "flow" -> (h, w, 2) float32."""
    imgs = [_u8(a) for a in (bottom, bottom2, mask, mask2)]
    h, w = imgs[0].shape[:2]
    for a in imgs:
        assert a.shape == (h, w, 3), "four B,G,R images of one size"
    names = ("bottomImage", "bottomImage2", "bottomWarp2", "_bottomCombined")
    out = {n: np.empty((h, w, 4), np.uint8) for n in names}
    out["flow"] = np.empty((h, w, 2), np.float32)
    ctx._ck(lib().s360_pole_removal_combine(ctx.h, _p(imgs[0]), _p(imgs[1]), _p(imgs[2]), _p(imgs[3]), w, h, C.c_float(radius),
                                            C.c_float(radius2), int(bool(flip180)), int(feather_size), flow_alg.encode(),
                                            *[_p(out[n]) for n in names], _p(out["flow"])))
    return out


def debug_views(ctx, views, src, dst):
    """Test tap s360_debug_views: one k_debug_views launch over `views` — dicts with the fields of s360_debug_view (channels_in
    defaults to 4) — reading the uint8 area `src`, writing into a copy of the uint8 area `dst`, which is returned."""
    arr = (DebugView * len(views))()
    for k, v in enumerate(views):
        arr[k].channels_in = 4
        for name, val in v.items():
            setattr(arr[k], name, int(val))
    src = np.ascontiguousarray(src, np.uint8).ravel()
    out = np.array(dst, np.uint8).ravel()
    ctx._ck(lib().s360_debug_views(ctx.h, len(views), arr, _p(src), C.c_size_t(src.size), _p(out), C.c_size_t(out.size)))
    return out
