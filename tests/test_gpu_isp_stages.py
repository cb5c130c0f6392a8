"""The ISP's float intermediates on the GPU against the oracle's, bit for bit (isp_kernels.hip through the test tap
s360_debug_isp_stages, include/s360_debug_isp.h; oracle/isp.h: IspStages, oracle/isp_pipe.h: IspPipeStages).

tests/test_gpu_isp.py compares finished 8- / 16-bit images: every float goes through (int)clamp(v, 0, 4095) into a tone table, then
through the unsharp mask, then is truncated — an error of one ulp along a border changes no output sample (DESIGN.md section 2 has
the counts). Here every stage is compared as uint32 bit patterns (flags and the output as bytes) on tests/isp_edge_cases.py's
cases: the shapes at which the kernels take another branch, and content the smooth test scene never holds. The pipeline's planes
are compared over their whole extended area, the soft ISP's over the image. No tolerance: the library is built with
-ffp-contract=off to be bit-exact. One ISP object develops a group's cases one after the other — small, large, small — so its
buffers grow and are reused."""
import numpy as np
import pytest

import isp_edge_cases as E

pytestmark = pytest.mark.gpu

GROUPS = E.groups()


def _first_difference(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    a = got.view(np.uint32) if got.dtype == np.float32 else got
    b = want.view(np.uint32) if want.dtype == np.float32 else want
    if np.array_equal(a, b):
        return None
    bad = np.argwhere(a != b)
    at = tuple(bad[0].tolist())
    return "stage %s: %d of %d differ, first at (y, x[, c]) = %s: got %r, want %r" % (name, len(bad), a.size, at, got[at], want[at])


def check_case(isp, oracle, case):
    raw = E.raw_of(case)
    ocfg = oracle.isp_config_from_json(E.json_of(case), case.bpp, case.dm, case.resize)
    with oracle.coverage() as cov:
        if case.pipe:
            want_out, want = oracle.isp_pipe_run_stages(ocfg, raw, fast=case.pipe == E.PIPE_FAST)
        else:
            want_out, want = oracle.isp_run_stages(ocfg, raw)
    prefix = "pipe_" if case.pipe else "isp_"
    for name in case.counters:
        assert cov.counts[prefix + name] > 0, "%s: the case does not reach %s%s" % (case.id, prefix, name)
    got_out, got = isp.debug_stages(raw)
    assert sorted(got) == sorted(k for k in want if k != "low_first"), (case.id, sorted(got), sorted(want))
    if "low_first" in want:  # the first direction's low pass, which the second overwrites: the sequence stopped behind it
        none, first = isp.debug_stages(raw, stop_after=1)
        assert none is None
        got["low_first"] = first["low_first"]
    assert sorted(got) == sorted(want)
    for name in ("plane", "flag", "gV", "gH", "green", "tone", "low_first", "low"):
        if name in want:
            msg = _first_difference(name, got[name], want[name])
            assert msg is None, "%s: %s" % (case.id, msg)
    msg = _first_difference("output", got_out, want_out)
    assert msg is None, "%s: %s" % (case.id, msg)
    assert np.array_equal(isp.get_image(raw), want_out), "%s: s360_isp_process after the tap" % case.id


@pytest.mark.parametrize("group", list(GROUPS), ids=list(GROUPS))
def test_isp_stages_equal_the_oracle(oracle, s360lib, group):
    from surround360_amd import isp as I
    cases = GROUPS[group]
    first = cases[0]
    assert len({(c.pipe, c.config, c.bpp, c.dm, c.resize, c.stuck) for c in cases}) == 1  # one object's worth
    assert len(cases) == 1 or any((a.w, a.h) != (b.w, b.h) for a, b in zip(cases, cases[1:]))
    isp = I.CameraIsp(I.config_from_json(E.json_of(first), first.bpp, first.dm, first.resize, pipe=first.pipe))
    try:
        for case in cases:
            check_case(isp, oracle, case)
    finally:
        isp.close()


def test_every_counter_is_assigned_to_a_case():
    """The content cases together reach every edge the oracle counts."""
    import oracle_lib
    soft = {n for c in E.all_cases() if not c.pipe for n in c.counters}
    pipe = {n for c in E.all_cases() if c.pipe == E.PIPE for n in c.counters}
    assert soft == set(oracle_lib.ISP_COVERAGE_NAMES)
    assert pipe == set(oracle_lib.PIPE_COVERAGE_NAMES)


def test_the_tap_refuses_what_a_configuration_does_not_have(s360lib):
    """A stage pointer that names a buffer the configuration never fills is an error, not a stale buffer."""
    import ctypes as C
    import isputil
    from surround360_amd import _capi, isp as I
    raw = isputil.bayer_frame(32, 24, seed=1)
    buf = np.zeros((24 + 16) * (32 + 16) * 3, np.float32)
    p, z = buf.ctypes.data_as(C.c_void_p), None
    rp = raw.ctypes.data_as(C.c_void_p)
    f = _capi.lib().s360_debug_isp_stages
    for cfg, args in (
            (I.config_from_json(isputil.CONFIG_FULL, 16, 0), (0, z, p, z, z, z, z, z, z)),               # bilinear: no flags
            (I.config_from_json(isputil.CONFIG_FULL, 16, 0), (0, z, z, p, z, z, z, z, z)),               # ... no gV
            (I.config_from_json(isputil.CONFIG_GRBG_NOSHARP, 16, 2), (0, z, z, z, z, z, z, p, z)),       # no sharpening: no low pass
            (I.config_from_json(isputil.CONFIG_GRBG_NOSHARP, 16, 2), (1, z, z, z, z, z, z, z, z)),
            (I.config_from_json(isputil.CONFIG_FULL, 16, 2), (1, z, z, z, z, z, z, p, p)),               # stopped early: no output
            (I.config_from_json(isputil.CONFIG_FULL, 16, 2), (2, z, z, z, z, z, z, z, z)),
            (I.config_from_json(isputil.CONFIG_FULL, 16, 2, pipe=I.PIPE), (0, z, z, p, z, z, z, z, z)),  # the pipeline has no gV
            (I.config_from_json(isputil.CONFIG_FULL, 16, 2, pipe=I.PIPE_FAST), (0, z, z, z, z, p, z, z, z))):
        isp = I.CameraIsp(cfg)
        try:
            assert f(isp.h, rp, 32, 24, *args) == _capi.ERR_INVALID_ARG
        finally:
            isp.close()


def test_test_tap_is_declared_listed_and_exported(s360lib):
    import os
    import re
    from surround360_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "s360_debug_isp.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.DEBUG_ISP_SYMBOLS) == ["s360_debug_isp_stages"]
    for n in names:
        assert hasattr(s360lib, n), n
