#!/usr/bin/env python
"""Writes tests/golden/debug_images_golden.json: per case of tests/debug_images_cases.py, the SHA-256 of the decoded pixels and the
shape of every file the REFERENCE'S OWN PROGRAM (oracle/_ref/TestRenderStereoPanorama, built by `make -C oracle ref`) writes under
debug/<frame>/ outside flow_images/ when it is run with --save_debug_images. It also asserts that the flag changes nothing else in
the reference — the other outputs of the two cases tests/golden/refprogram_golden.json knows still have its digests — and that the
pole-removal debug images of a first frame are, pixel for pixel, the state images of the same name. Run where the reference exists:
    make -C oracle ref && python tests/golden/make_debug_images_golden.py
`--check` compares with the committed file instead of writing it (tests/test_cpu_debug_images.py)."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import debug_images_cases as D  # noqa: E402
import refprog  # noqa: E402


def make():
    assert os.path.exists(refprog.REF_EXE), "build it first: make -C oracle ref"
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        rig = D.small_rig(tmp)
        for name in D.CASES:
            out = D.run_case(refprog.REF_EXE, os.path.join(tmp, name), rig, name)
            res[name] = D.digests(out, name)
            print(name, len(res[name]), "files")
            if D.CASES[name][4]:
                D.check_other_outputs(out, name)
            if name == "pole_removal":
                f = D.CASES[name][0][0]
                for fn in ("bottomImage.png", "bottomImage2.png"):
                    a = refprog._digest_png(os.path.join(out, "debug", f, fn))
                    b = refprog._digest_png(os.path.join(out, "debug", f, "flow_images", fn))
                    assert a == b, "debug/%s/%s differs from the state image of that name" % (f, fn)
    return res


if __name__ == "__main__":
    res = make()
    if "--check" in sys.argv[1:]:
        want = json.load(open(D.GOLDEN))
        assert res == want, "the reference's debug images differ from tests/golden/debug_images_golden.json: %s" % sorted(
            "%s/%s" % (c, k) for c in set(res) | set(want) for k in set(res.get(c, {})) | set(want.get(c, {}))
            if res.get(c, {}).get(k) != want.get(c, {}).get(k))[:10]
        print("debug_images_golden.json: up to date")
    else:
        json.dump(res, open(D.GOLDEN, "w"), indent=0, sort_keys=True)
