#!/usr/bin/env python
"""Writes tests/golden/isp_edge_digests.json: digests of the outputs of the reference's own ISPs (oracle/_ref/libref_isp.so: its
CameraIsp.h compiled; libref_isppipe.so: its generator CameraIspGen.cpp executed under its CameraIspPipe.h) for every case of
tests/isp_edge_cases.py — digests rather than arrays, to stay small. Run where the reference checkout exists (make -C oracle ref):
python tests/golden/make_isp_edge_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import isp_edge_cases as E  # noqa: E402
import oracle_lib as O  # noqa: E402

assert O.ref_isp_lib() is not None and O.ref_isp_pipe_lib() is not None, "needs the reference checkout (make -C oracle ref)"
out = {}
for case in E.all_cases():
    assert case.id not in out, case.id
    out[case.id] = E.digest(E.reference_output(O, case))
path = os.path.join(HERE, "isp_edge_digests.json")
with open(path, "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote %d cases, %d bytes" % (len(out), os.path.getsize(path)))
