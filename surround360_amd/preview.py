"""Host-side mirror of the reference's PreviewRenderer (SR/test/TestHyperPreview.cpp:77-185) over the C ABI of libs360
(include/s360_preview.h, and the test taps of include/s360_debug_preview.h):

  PreviewRenderer()                                    Preview(cameras, raw_w, raw_h, eqr_w, eqr_h, gamma, softmax_coef)
  addTopImage / addBottomImage / addBottomImage2 +     render_packed(top, bottom, bottom2, bits); None keeps a layer's
  render                                               previous raw image

Everything computes on the GPU; numpy arrays stand in for cv::Mat. Frames are the sensor's packed bytes as a capture's .bin
container holds them (8 or 12 bits per pixel)."""
import ctypes as C

import numpy as np

from ._capi import Camera, check, lib

LAYERS = ("top", "bottom", "bottom2")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Preview:
    """One rig, raw size and equirect size on one GPU."""

    def __init__(self, cameras, raw_w, raw_h, eqr_w=2048, eqr_h=1024, gamma=1.0, softmax_coef=30.0, device=0):
        """cameras: the whole rig, a ctypes array of _capi.Camera (RigDescription(...).rig) or a list of them."""
        n = len(cameras)
        arr = cameras if isinstance(cameras, C.Array) else (Camera * n)(*cameras)
        self.raw_w, self.raw_h, self.eqr_w, self.eqr_h = int(raw_w), int(raw_h), int(eqr_w), int(eqr_h)
        self.h = None
        h = C.c_void_p()
        check(lib().s360_preview_create(C.byref(h), C.cast(arr, C.c_void_p), n, int(device), self.raw_w, self.raw_h, self.eqr_w,
                                        self.eqr_h, float(gamma), float(softmax_coef)))
        self.h = h

    def frame_bytes(self, bits):
        return self.raw_w * self.raw_h if bits == 8 else self.raw_h * (3 * self.raw_w // 2)

    def _frames(self, frames, bits):
        out = []
        for f in frames:
            if f is not None:
                f = np.ascontiguousarray(f, np.uint8).reshape(-1)
                if f.size != self.frame_bytes(bits):
                    raise ValueError("a %d-bit frame of %d x %d has %d bytes, not %d" % (bits, self.raw_w, self.raw_h,
                                                                                      self.frame_bytes(bits), f.size))
            out.append(f)
        return out

    def camera_indices(self):
        """Indices into the rig of the top, bottom and secondary bottom camera the object chose."""
        idx = (C.c_int * 3)()
        check(lib().s360_preview_cameras(self.h, idx))
        return list(idx)

    def render_packed(self, top, bottom, bottom2, bits):
        """eqr_h x eqr_w x 3 uint8, B,G,R: the image the reference hands to its JPEG encoder."""
        t, b, b2 = self._frames((top, bottom, bottom2), bits)
        out = np.empty((self.eqr_h, self.eqr_w, 3), np.uint8)
        check(lib().s360_preview_render_packed(self.h, _p(t), _p(b), _p(b2), int(bits), _p(out)))
        return out

    def submit_packed(self, top, bottom, bottom2, bits):
        """The first half of render_packed; up to two frames may wait for fetch()."""
        t, b, b2 = self._frames((top, bottom, bottom2), bits)
        check(lib().s360_preview_submit_packed(self.h, _p(t), _p(b), _p(b2), int(bits)))

    def fetch(self, out=None):
        """The oldest submitted frame that was not fetched yet."""
        if out is None:
            out = np.empty((self.eqr_h, self.eqr_w, 3), np.uint8)
        check(lib().s360_preview_fetch(self.h, _p(out)))
        return out

    def last_times(self):
        """(develop ms, compose ms) of the last submitted frame, device time."""
        d, c = C.c_float(0), C.c_float(0)
        check(lib().s360_preview_last_times(self.h, C.byref(d), C.byref(c)))
        return d.value, c.value

    # ---- the frame as a .jpg file encoded on the device (include/s360_jpeg.h) ----
    def set_jpeg(self, on, quality=95):
        """Frames submitted from now on are also (on) / no longer (off) encoded behind the compose kernel."""
        check(lib().s360_preview_set_jpeg(self.h, 1 if on else 0, int(quality)))

    def jpeg_bound(self):
        return int(lib().s360_preview_jpeg_bound(self.h))

    def fetch_jpeg(self, cap=None):
        """The oldest submitted frame that was not fetched yet, as the bytes of its .jpg file."""
        if getattr(self, "_jpeg_out", None) is None:
            self._jpeg_out = np.empty(self.jpeg_bound(), np.uint8)
        n = C.c_size_t(0)
        check(lib().s360_preview_fetch_jpeg(self.h, _p(self._jpeg_out), self._jpeg_out.size if cap is None else int(cap), C.byref(n)))
        return self._jpeg_out[:n.value].tobytes()

    def render_packed_jpeg(self, top, bottom, bottom2, bits):
        """render_packed with the file instead of the pixels (the encoder must be on)."""
        self.submit_packed(top, bottom, bottom2, bits)
        return self.fetch_jpeg()

    def last_jpeg_time(self):
        """Device time of the encoder's kernels for the last frame submitted with the encoder on, ms."""
        ms = C.c_float(0)
        check(lib().s360_preview_last_jpeg_time(self.h, C.byref(ms)))
        return ms.value

    # ---- test taps (include/s360_debug_preview.h); layer: 0 top, 1 bottom, 2 secondary bottom ----
    def debug_camera(self, layer):
        c = Camera()
        check(lib().s360_debug_preview_camera(self.h, int(layer), C.byref(c)))
        return c

    def debug_map(self, layer):
        m = np.empty((self.eqr_h, self.eqr_w, 2), np.float32)
        check(lib().s360_debug_preview_map(self.h, int(layer), _p(m)))
        return m

    def debug_set_maps(self, maps):
        """maps: three eqr_h x eqr_w x 2 float32 arrays (None leaves a layer's map), used by every render that follows."""
        ms = [None if m is None else np.ascontiguousarray(m, np.float32) for m in maps]
        for m in ms:
            if m is not None and m.shape != (self.eqr_h, self.eqr_w, 2):
                raise ValueError("a map is eqr_h x eqr_w x 2")
        check(lib().s360_debug_preview_set_maps(self.h, _p(ms[0]), _p(ms[1]), _p(ms[2])))

    def debug_developed(self, layer):
        d = np.empty((self.raw_h // 2, self.raw_w // 2, 4), np.float32)
        check(lib().s360_debug_preview_developed(self.h, int(layer), _p(d)))
        return d

    def debug_remapped(self, layer):
        d = np.empty((self.eqr_h, self.eqr_w, 4), np.float32)
        check(lib().s360_debug_preview_remapped(self.h, int(layer), _p(d)))
        return d

    def close(self):
        if self.h:
            lib().s360_preview_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
