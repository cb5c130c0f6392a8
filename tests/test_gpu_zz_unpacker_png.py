"""host/Unpacker --device_png and host/Raw2Rgb --device_png end to end: the 16-bit (or 8-bit) PNG encoded on the device behind the ISP
(include/s360_isp_png.h) holds the pixels of the file the same program writes without the flag; directory layout, renaming and
the raw TIFFs are untouched; the renderer reads an imgs_dir unpacked with the flag to the same equirect bytes; host/png_io.hpp
reads a device-encoded 16-bit file back to the same samples. The check functions take the programs' paths:
tests/test_cpu_png16.py runs them on the programs linked against the emulated library."""
import json
import os
import subprocess

import numpy as np
import pytest

import isputil
import refprog
import test_gpu_png16 as P
from test_gpu_zz_unpacker import _png16_bgr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = ["--device_png"]


def listing(root):
    return sorted(os.path.relpath(os.path.join(dp, f), str(root)) for dp, _, fs in os.walk(str(root)) for f in fs)


def run_unpacker(exe, tmp_path, tag, binp, ispd, extra=(), env=None, raw=True):
    out, rawd = tmp_path / (tag + "_rgb"), tmp_path / (tag + "_raw")
    out.mkdir()
    rawd.mkdir()
    cmd = [exe, "--isp_dir", str(ispd), "--output_dir", str(out), "--bin_list", str(binp)] + (["--output_raw_dir", str(rawd)] if raw else [])
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, rawd, r.stderr


def check_unpacker_png(exe, tmp_path, bits, soft, by_environment=False):
    """The small capture of test_gpu_zz_unpacker.check_unpacker — 128 x 96, two cameras, three frames — unpacked with and without
    the flag (or with S360_UNPACKER_DEVICE_PNG=1 in its place)."""
    w, h, nf = 128, 96, 3
    serials = [17430921, 16241093]
    configs = [isputil.CONFIG_FULL, isputil.CONFIG_GRBG_NOSHARP]
    frames = [[isputil.bayer_frame(w, h, seed=10 * f + c + bits) for c in range(2)] for f in range(nf)]
    binp, ispd = tmp_path / "0.bin", tmp_path / "isp"
    isputil.footage_file(str(binp), frames, bits, serials)
    ispd.mkdir()
    for s, js in zip(serials, configs):
        (ispd / ("%d.json" % s)).write_text(js)
    soft_flag = ["--soft_isp"] if soft else []
    host, host_raw, host_err = run_unpacker(exe, tmp_path, "host", binp, ispd, soft_flag)
    if by_environment:
        dev, dev_raw, dev_err = run_unpacker(exe, tmp_path, "dev", binp, ispd, soft_flag, env=dict(os.environ, S360_UNPACKER_DEVICE_PNG="1"))
    else:
        dev, dev_raw, dev_err = run_unpacker(exe, tmp_path, "dev", binp, ispd, soft_flag + FLAG)
    want = ["cam%d/%06d.png" % (c, f) for c in range(2) for f in range(nf)]
    assert listing(host) == want and listing(dev) == want
    assert listing(host_raw) == listing(dev_raw) and len(listing(dev_raw)) == 2 * nf
    for f in listing(host_raw):
        assert (host_raw / f).read_bytes() == (dev_raw / f).read_bytes(), f
    assert sorted(host_err.replace(str(tmp_path), "").splitlines()) == sorted(dev_err.replace(str(tmp_path), "").splitlines())
    for f in want:
        got, rows, bands = P.decode16((dev / f).read_bytes())  # (asserts the device encoder's layout: sbNd, a chunk per band)
        px = _png16_bgr(str(host / f))
        assert px.std() > 5 and np.array_equal(got, px), f


@pytest.fixture(scope="module")
def programs(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host")


@pytest.mark.parametrize("soft", [False, True], ids=["pipe", "soft_isp"])
@pytest.mark.parametrize("bits", [12, 8])
def test_unpacker_device_png(tmp_path, programs, bits, soft):
    check_unpacker_png(os.path.join(programs, "Unpacker"), tmp_path, bits, soft)


def test_unpacker_device_png_by_environment(tmp_path, programs):
    check_unpacker_png(os.path.join(programs, "Unpacker"), tmp_path, 12, False, by_environment=True)


def check_renderer_reads_device_pngs(unpacker_exe, trsp_exe, tmp_path):
    """The small rig and sizes of test_gpu_zz_unpacker.check_bin_list, one frame: --imgs_dir unpacked with the flag and without."""
    import rigutil
    cam = refprog.CAM
    rig = rigutil.scaled_rig_json(os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), str(tmp_path / "rig_small.json"), cam / 2048.0)
    n = len(json.load(open(rig))["cameras"])
    serials = [40000 + 7 * k for k in range(n)]
    configs = [isputil.CONFIG_GRBG_NOSHARP if k % 3 else isputil.CONFIG_FULL for k in range(n)]
    pats = ["GRBG" if k % 3 else "RGGB" for k in range(n)]
    frames = [[isputil.bayer_frame(cam, cam, seed=k, pattern=pats[k]) for k in range(n)]]
    binp, ispd = tmp_path / "0.bin", tmp_path / "isp"
    isputil.footage_file(str(binp), frames, 12, serials)
    ispd.mkdir()
    for s, js in zip(serials, configs):
        (ispd / ("%d.json" % s)).write_text(js)
    eqr = {}
    for tag, extra in (("host", []), ("dev", FLAG)):
        imgs, _, _ = run_unpacker(unpacker_exe, tmp_path, tag, binp, ispd, extra, raw=False)
        out = tmp_path / (tag + "_out")
        for d in (out, out / "flow", out / "debug", out / "flow" / "000000", out / "debug" / "000000", out / "debug" / "000000" / "flow_images"):
            d.mkdir(exist_ok=True)
        r = subprocess.run([trsp_exe, "--rig_json_file", rig, "--eqr_width", str(refprog.EQR_W), "--eqr_height", str(refprog.EQR_H),
                            "--final_eqr_width", str(refprog.FINAL), "--final_eqr_height", str(refprog.FINAL), "--enable_top",
                            "--enable_bottom", "--sharpening", "0.25", "--imgs_dir", str(imgs), "--frame_number", "000000",
                            "--output_data_dir", str(out), "--prev_frame_data_dir", "NONE", "--output_equirect_path", str(out / "eqr.png")],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, "%s: rc %d\n%s" % (tag, r.returncode, r.stderr[-2000:])
        eqr[tag] = (out / "eqr.png").read_bytes()
    assert refprog.png_pixels_bgr(str(tmp_path / "host_out" / "eqr.png")).std() > 5
    assert eqr["dev"] == eqr["host"]


def test_renderer_reads_an_imgs_dir_unpacked_on_the_device(tmp_path, programs):
    check_renderer_reads_device_pngs(os.path.join(programs, "Unpacker"), os.path.join(programs, "TestRenderStereoPanorama"), tmp_path)


def check_raw2rgb_png(exe, tmp_path, bpp, accelerate):
    from PIL import Image
    w, h = 128, 96
    raw = isputil.bayer_frame(w, h, seed=bpp, pattern="RGGB")
    Image.fromarray(raw).save(str(tmp_path / "raw.png"))
    (tmp_path / "isp.json").write_text(isputil.CONFIG_FULL)
    files = {}
    for tag, extra in (("host", []), ("dev", FLAG)):
        out = tmp_path / (tag + ".png")
        r = subprocess.run([exe, "--input_image_path", str(tmp_path / "raw.png"), "--isp_config_path", str(tmp_path / "isp.json"),
                            "--output_image_path", str(out), "--output_bpp", str(bpp)] + (["--accelerate"] if accelerate else []) + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "Runtime = " in r.stderr, r.stderr[-2000:]
        files[tag] = out
    if bpp == 16:
        got, _, _ = P.decode16(files["dev"].read_bytes())
        want = _png16_bgr(str(files["host"]))
    else:
        got, want = refprog.png_pixels_bgr(str(files["dev"])), refprog.png_pixels_bgr(str(files["host"]))
        assert P.T.chunks(files["dev"].read_bytes())[1][0] == b"sbNd"
    assert want.shape == (h, w, 3) and want.std() > 5 and np.array_equal(got, want)


@pytest.mark.parametrize("accelerate", [False, True], ids=["soft", "accelerate"])
@pytest.mark.parametrize("bpp", [8, 16])
def test_raw2rgb_device_png(tmp_path, programs, bpp, accelerate):
    check_raw2rgb_png(os.path.join(programs, "Raw2Rgb"), tmp_path, bpp, accelerate)


@pytest.fixture(scope="module")
def ctx16(tmp_path_factory, rig_json, s360lib):
    import rigutil
    from surround360_amd import render as R
    d = tmp_path_factory.mktemp("rig_png16_host")
    path = rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), P.CAM / 2048.0)
    c = R.Context(R.RigDescription(path), R.make_params(eqr_width=P.EQR_W, eqr_height=P.EQR_H, enable_top=1, enable_bottom=1,
                                                        final_eqr_width=240, final_eqr_height=240, sharpening=0.25))
    yield c
    c.close()


def test_our_file_reader_reads_a_device_encoded_16_bit_file(ctx16, tmp_path):
    """host/png_io.hpp reads the file on its sequential path whatever the thread setting (its band-parallel path takes 8-bit files
    only): pngio::read is imread's 8-bit decode, so what comes back is every sample's high byte, in B,G,R order."""
    src = tmp_path / "rd.cpp"
    src.write_text(r'''
#include "png_io.hpp"
int main(int argc, char** argv) {  // argv: in.png out.raw threads
  pngio::g_read_threads = std::atoi(argv[3]);
  pngio::Image im = pngio::read(argv[1], false);
  FILE* f = std::fopen(argv[2], "wb");
  std::fwrite(im.px.data(), 1, im.px.size(), f);
  std::fclose(f);
  return im.c == 3 ? 0 : 1;
}
''')
    exe = str(tmp_path / "rd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "host"), "-o", exe, str(src), "-lz", "-lpthread"])
    a = P.cases16()["mixed"]
    p = tmp_path / "m.png"
    p.write_bytes(ctx16.encode_png16(a))
    for threads in ("3", "-1"):
        subprocess.check_call([exe, str(p), str(tmp_path / "m.raw"), threads])
        assert np.array_equal(np.fromfile(str(tmp_path / "m.raw"), np.uint8).reshape(a.shape), (a >> 8).astype(np.uint8)), threads
