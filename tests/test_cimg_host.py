"""The hosts' CImg input/output branch (-DMI_BLUR_WITH_CIMG), the reference's own image path
(heterogeneous_blur.c:20,106-135: `CImg<unsigned char> img(file)` + planar -> interleaved; split_image_blur.c:40-56:
interleaved -> planar + `save()`).

CImg is the reference's third-party dependency and is NOT vendored in this repo: the branch is compiled here against
the header where it lies in the reference tree (`-I/root/reference/CImg`), into a temporary directory, and only in the
build container — the whole module is skipped where that tree is absent (the GPU box).  JPEG decoding needs libjpeg
headers; the image has them only under /opt/conda, so the JPEG case links that copy through a private directory (so
that conda's older libstdc++ is not picked up) and is skipped when it is missing.

CPU-device runs only (no GPU here): what is checked is that CImg-decoded pixels reach the blur as the interleaved
stream the kernel contract wants, and that CImg-encoded output holds the blurred pixels — bit-exact against the oracle
for lossless formats (PPM in, BMP out; JPEG in -> decoded input saved as BMP, blur(saved input) == saved output).
"""
import os
import subprocess

import numpy as np
import pytest

from filter_harness import write_ppm

REF_CIMG_DIR = "/root/reference/CImg"
REF_JPEG = "/root/reference/image_320x240.jpg"
CONDA_JPEG_H = "/opt/conda/include/jpeglib.h"
CONDA_JPEG_SO = "/opt/conda/lib/libjpeg.so.9"

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF_CIMG_DIR, "CImg.h")),
                                reason="reference tree (CImg.h) not present: build-container-only test")


@pytest.fixture(scope="module")
def cimg_hosts(pkg, tmp_path_factory):
    pkg.build_native()
    d = tmp_path_factory.mktemp("cimg_hosts")
    with_jpeg = os.path.exists(CONDA_JPEG_H) and os.path.exists(CONDA_JPEG_SO)
    flags = ["-DMI_BLUR_WITH_CIMG", "-I", REF_CIMG_DIR]
    libs = []
    if with_jpeg:
        jl = d / "jpeglib"
        jl.mkdir()
        os.symlink(os.path.realpath(CONDA_JPEG_SO), jl / "libjpeg.so.9")
        os.symlink(os.path.realpath(CONDA_JPEG_SO), jl / "libjpeg.so")
        flags += ["-Dcimg_use_jpeg", "-idirafter", "/opt/conda/include"]
        libs = ["-L", str(jl), f"-Wl,-rpath,{jl}", "-ljpeg"]
    exes = {}
    for app in ("heterogeneous_blur", "split_image_blur"):
        exe = d / (app + "_cimg")
        cmd = [pkg.HIPCC, "-O1", "-std=c++17", "-w"] + flags + ["-I", os.path.join(pkg.ROOT, "include"), "-o", str(exe),
               os.path.join(pkg.APPS, app + ".cpp"), "-L", pkg.PKG_DIR, "-lmi_blur", f"-Wl,-rpath,{pkg.PKG_DIR}"] + libs + ["-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f"{app} does not compile with -DMI_BLUR_WITH_CIMG:\n{r.stderr[-3000:]}"
        exes[app] = str(exe)
    return exes, with_jpeg


def read_image(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_cimg_lossless_round_trip_through_the_blur(cimg_hosts, O, tmp_path):
    """PPM decoded by CImg (planar) -> interleaved stream -> blur -> CImg-encoded BMP: pixels == oracle, both kernel sizes."""
    exes, _ = cimg_hosts
    img = O.lcg_image(48, 64, 3)
    write_ppm(tmp_path / "in.ppm", img)
    for ksize, radius in (("3", 1), ("5", 2)):
        r = subprocess.run([exes["heterogeneous_blur"], "cpu", "0.5", "35", "--image", "in.ppm", "--images", "70", "--ksize", ksize,
                            "--save", "out.bmp", "--save-input", "in_copy.bmp"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Original image loaded: 64x48, 3 channels" in r.stdout, r.stdout + r.stderr
        assert "Original image source: in.ppm" in r.stdout
        assert np.array_equal(read_image(tmp_path / "in_copy.bmp"), img)              # CImg load + planar->interleaved
        assert np.array_equal(read_image(tmp_path / "out.bmp"), O.blur(img, radius))  # ... blur ... interleaved->planar + save


def test_cimg_frames_stream(cimg_hosts, O, tmp_path):
    """--frames in the CImg build: every frame is decoded by CImg — whose storage IS planar, so the decode is the planar
    batch buffer — blurred (cpu device here) and saved through CImg as BMP; interleaved and planar output, 3x3 and 5x5.
    Every saved frame == oracle blur of its own input."""
    exes, _ = cimg_hosts
    frames = O.lcg_stream(9, 36, 52, 3, first_index=700)
    os.makedirs(tmp_path / "in")
    for i in range(len(frames)):
        write_ppm(tmp_path / "in" / f"f_{i:03d}.ppm", frames[i])
    for extra, ksize, radius, outdir in (([], "3", 1, "o1"), (["--planar-out"], "5", 2, "o2")):
        r = subprocess.run([exes["heterogeneous_blur"], "cpu", "0.5", "4", "--frames", "in", "--save-dir", outdir, "--ksize", ksize] + extra,
                           cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "10. FRAME INGEST" in r.stdout, r.stdout + r.stderr
        want = O.blur_batch(frames, radius)
        for i in range(len(frames)):
            assert np.array_equal(read_image(tmp_path / outdir / f"f_{i:03d}.bmp"), want[i]), (i, extra)
    r = subprocess.run([exes["heterogeneous_blur"], "cpu", "0.5", "4", "--frames", "in", "--native-layout"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--native-layout ignored in a CImg build" in r.stdout


def test_cimg_jpeg_input_is_the_reference_default(cimg_hosts, O, golden, tmp_path):
    """The reference's default input (`./image_320x240.jpg`, heterogeneous_blur.c:43) decoded by CImg + libjpeg as the
    reference does: the host picks it up from the CWD with NO --image flag; blur(decoded input) == saved output bit for
    bit, and the decoded pixels agree with PIL's decode of the same file (tests/golden/ref_images.npz) to JPEG-decoder
    tolerance."""
    exes, with_jpeg = cimg_hosts
    if not with_jpeg or not os.path.exists(REF_JPEG):
        pytest.skip("no libjpeg headers/library in this image, or the reference JPEG is absent")
    os.symlink(REF_JPEG, tmp_path / "image_320x240.jpg")
    r = subprocess.run([exes["heterogeneous_blur"], "cpu", "0.5", "35", "--images", "70", "--save", "out.bmp", "--save-input", "in.bmp"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Input file: ./image_320x240.jpg" in r.stdout and "Original image loaded: 320x240, 3 channels" in r.stdout
    assert "Original image source: ./image_320x240.jpg" in r.stdout                   # not the synthetic stand-in
    decoded = read_image(tmp_path / "in.bmp")
    assert np.array_equal(read_image(tmp_path / "out.bmp"), O.blur(np.ascontiguousarray(decoded), 1))
    pil = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_images.npz"))["image_320x240"]
    mse = float(((decoded.astype(np.int32) - pil.astype(np.int32)) ** 2).mean())
    assert decoded.shape == pil.shape and 10 * np.log10(255.0 ** 2 / max(mse, 1e-9)) > 40.0      # two IDCTs, same picture


def test_cimg_split_host_compiles_and_loads(cimg_hosts, L, tmp_path):
    """split_image_blur's CImg branch (load + save_one_image_rgb, split_image_blur.c:40-56,106-139): compiled above; with
    no GPU here it must get as far as the reference does — past the image load — and stop at the device check."""
    exes, _ = cimg_hosts
    if L.mi_blur_device_count() > 0:
        pytest.skip("a GPU is visible here")
    img = np.arange(32 * 24 * 3, dtype=np.uint32).astype(np.uint8).reshape(24, 32, 3)
    write_ppm(tmp_path / "in.ppm", img)
    r = subprocess.run([exes["split_image_blur"], "0.837", "35", "--image", "in.ppm", "--images", "10", "--save-input", "in.bmp"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert "Original image loaded: 32x24, 3 channels" in r.stdout and "Error: Could not find both CPU and GPU devices" in r.stdout
    assert r.returncode != 0
    assert np.array_equal(read_image(tmp_path / "in.bmp"), img)
