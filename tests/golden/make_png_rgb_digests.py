"""Records tests/golden/png_rgb_digests.json: SHA-256 of the file s360_encode_png writes for four 3-channel images of
tests/test_gpu_png.py::cases(). Run ONCE, on the commit in front of the 4-channel encoder, against that commit's
tools/libs360_emu.so (the encoder is integer-only: emulation and device write the same bytes):

    S360_TEST_EMULATED_LIB_PATH=<that build>/tools/libs360_emu.so python tests/golden/make_png_rgb_digests.py

tests/test_gpu_state_png.py holds every later encoder to these digests."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ["smooth", "mixed", "flat", "one_pixel"]


def main():
    from surround360_amd import _capi
    _capi.LIB_PATH = os.environ["S360_TEST_EMULATED_LIB_PATH"]
    from surround360_amd import render as R
    import test_gpu_png as T
    ctx = R.Context(R.RigDescription(os.path.join(HERE, "rig_17cam.json")), R.make_params(eqr_width=252, eqr_height=126))
    cases = T.cases()
    out = {n: hashlib.sha256(ctx.encode_png(cases[n])).hexdigest() for n in NAMES}
    ctx.close()
    with open(os.path.join(HERE, "png_rgb_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
