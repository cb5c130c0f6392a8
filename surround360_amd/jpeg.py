"""Baseline JPEG files encoded on the GPU, over the C ABI of libs360 (include/s360_jpeg.h and the test tap of
include/s360_debug_jpeg.h). The file is the one host/jpeg_io.hpp's writer — and cv::imwrite through libjpeg, and PIL's
save(quality=q, subsampling=2) — produces from the same pixels, byte for byte."""
import ctypes as C

import numpy as np

from ._capi import check, lib


def bound(w, h):
    """A size no file of w x h exceeds."""
    return int(lib().s360_jpeg_bound(int(w), int(h)))


def _bgr(bgr):
    a = np.ascontiguousarray(bgr, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("an image is h x w x 3 uint8 (B,G,R)")
    return a


class JpegEncoder:
    """One encoder for images of up to max_w x max_h on one GPU; quality as libjpeg's (clamped to 1..100)."""

    def __init__(self, max_w, max_h, quality=95, device=0):
        self.max_w, self.max_h = int(max_w), int(max_h)
        self.h = None
        h = C.c_void_p()
        check(lib().s360_jpeg_create(C.byref(h), int(device), self.max_w, self.max_h, int(quality)))
        self.h = h
        self._out = np.empty(bound(self.max_w, self.max_h), np.uint8)

    def encode(self, bgr, cap=None):
        """bgr: h x w x 3 uint8, B,G,R -> the file as bytes. cap: the size of the output buffer handed to the library (tests)."""
        a = _bgr(bgr)
        n = C.c_size_t(0)
        self.needed = None
        try:
            check(lib().s360_jpeg_encode(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0],
                                         self._out.ctypes.data_as(C.c_void_p), self._out.size if cap is None else int(cap), C.byref(n)))
        finally:
            self.needed = n.value  # (the size needed, also where cap was too small)
        return self._out[:n.value].tobytes()

    def debug_blocks(self, bgr):
        """(coefficients n x 64 int16, bit lengths n uint32) of the n = 6 * ceil(w/16) * ceil(h/16) emitted blocks."""
        a = _bgr(bgr)
        n = 6 * ((a.shape[1] + 15) // 16) * ((a.shape[0] + 15) // 16)
        coef, bits = np.empty((n, 64), np.int16), np.empty(n, np.uint32)
        check(lib().s360_debug_jpeg_blocks(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0],
                                           coef.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p)))
        return coef, bits

    def last_time(self):
        """Device time of the last encode's kernels, ms."""
        ms = C.c_float(0)
        check(lib().s360_jpeg_last_time(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            lib().s360_jpeg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
