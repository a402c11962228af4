"""CPU tests of the Middlebury flow colour code: the numpy restatement (tests/colorcode_ref.py) against the reference's own compiled
code (tests/golden/colorcode_ref.npz, made by tests/golden/make_colorcode_golden.py), the PNG writers, the C++ shim and example,
the CLI's argument handling, the C-ABI declarations."""
import os
import subprocess

import numpy as np
import pytest

import colorcode_ref as R
from conftest import ROOT
from host_checks import run_cli


def test_restatement_matches_reference_compute_color():
    v, ref, kind, _ = R.load_fixture()
    got = R.compute_color(v[:, 0], v[:, 1])
    d = np.abs(got.astype(int) - ref.astype(int))
    assert np.array_equal(got[kind == 1], ref[kind == 1])                 # +-0, axes, |v| == 1: exact
    assert d.max() <= 1                                                  # elsewhere: the atan2 deviation moves at most one step
    grid = kind == 0
    assert grid.sum() == 160000 and np.count_nonzero(d[grid].max(1)) <= 1e-5 * grid.sum()
    # wheel boundaries: where a 1-ulp difference of the angle moves k0 -- the deviation is confined there
    assert np.count_nonzero(d[kind == 2].max(1)) <= 8
    assert (kind == 2).sum() == 55 * 9


def test_grid_vectors_are_what_the_fixture_was_made_from():
    """the grid's inputs are made again by integer arithmetic, not stored: pin their spread and a few exact values"""
    v = R.grid_vectors()
    rad = np.sqrt((v.astype(np.float64) ** 2).sum(1))
    assert v.dtype == np.float32 and v.shape == (160000, 2) and len(np.unique(v, axis=0)) == 160000
    assert rad.min() < 0.01 and rad.max() > 200 and (rad <= 1).sum() > 40000 and (rad > 1).sum() > 40000
    ang = np.arctan2(v[:, 1], v[:, 0])
    assert np.histogram(ang, bins=55, range=(-np.pi, np.pi))[0].min() > 1000


def test_restatement_matches_reference_motion_to_color():
    _, _, _, runs = R.load_fixture()
    assert {r[0] for r in runs} == {"alley", "alley_max5", "noisy", "noisy_max0", "threshold", "zero", "unknown", "below"}
    for name, flow, mm, step, ref, ref_st in runs:
        rgb, st = R.motion_to_color(flow, mm)
        d = np.abs(rgb[::step].astype(int) - ref.astype(int))
        assert d.max() <= 1 and np.count_nonzero(d.max(-1)) <= 1e-5 * d.shape[0] * d.shape[1], name
        assert np.array_equal(st, ref_st), (name, st, ref_st)
        if name == "unknown":
            assert np.array_equal(ref_st, [-1, 999, -999, 999, -999]) and not ref.any()
        if name == "threshold":
            assert ref_st[0] > 1e9 and ref_st[2] == 1e9 and ref_st[3] == -1e9          # |u| == 1e9 is known, beyond it is not
        if name == "noisy":
            assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 1000


def test_write_png_roundtrip(tmp_path):
    from PIL import Image
    from flowonthego_amd.color import write_png
    rng = np.random.default_rng(1)
    for h, w in ((1, 1), (17, 33), (200, 301)):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = str(tmp_path / "a.png")
        write_png(p, a)
        assert np.array_equal(np.asarray(Image.open(p).convert("RGB")), a)
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "b.png"), np.zeros((3, 3, 4), np.uint8))


SHIM_DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/flowcolor.h"
#include "fotg/flowio.h"
int main(int argc, char **argv)
{
  // argv: rgb.raw w h out.png in.flo out.flo
  const int w = atoi(argv[2]), h = atoi(argv[3]);
  std::vector<unsigned char> rgb((size_t)w * h * 3);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) return 2;
  fclose(f);
  if (!OFC::SavePNG(rgb.data(), w, h, argv[4])) return 3;
  std::vector<float> flow;
  int fw, fh;
  if (!OFC::ReadFlowFile(flow, fw, fh, argv[5])) return 4;
  if (OFC::ReadFlowFile(flow, fw, fh, argv[1])) return 5;          // not a .flo
  OFC::ReadFlowFile(flow, fw, fh, argv[5]);
  if (!OFC::SaveFlowFile(flow.data(), fw, fh, argv[6])) return 6;
  return 0;
}
'''


def test_cpp_shim_png_and_flo(tmp_path):
    """include/fotg/flowcolor.h compiles with plain g++ (no HIP, no libpng, no zlib): SavePNG decodes (PIL) to the pixels write_png
    writes, ReadFlowFile reads what the .flo writers write"""
    from PIL import Image
    from flowonthego_amd.color import write_png
    from flowonthego_amd.flo import read_flo, write_flo
    src = tmp_path / "drv.cpp"
    src.write_text(SHIM_DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    rng = np.random.default_rng(2)
    for h, w in ((1, 1), (5, 7), (300, 250)):                          # 300 x 751 bytes: more than one stored block
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        raw, png, png_py = (str(tmp_path / n) for n in ("a.raw", "a.png", "b.png"))
        a.tofile(raw)
        flo = (rng.standard_normal((h, w, 2)) * 4).astype(np.float32)
        flo[0, 0] = (np.nan, np.inf)
        fin, fout = str(tmp_path / "in.flo"), str(tmp_path / "out.flo")
        write_flo(fin, flo)
        r = subprocess.run([exe, raw, str(w), str(h), png, fin, fout])
        assert r.returncode == 0, r.returncode
        write_png(png_py, a)
        assert np.array_equal(np.asarray(Image.open(png)), np.asarray(Image.open(png_py)))
        assert np.array_equal(np.asarray(Image.open(png)), a)
        assert np.array_equal(read_flo(fout), flo, equal_nan=True)


def test_color_flow_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "color_flow"))


def test_cli_argument_errors(tmp_path):
    for args in ([], ["a.flo"], ["-quiet", "a.flo"], ["a.flo", "b.png", "3", "extra"]):
        r = run_cli("color_flow", args)
        assert r.returncode != 0 and "usage: color_flow [-quiet] in.flo out.png [maxmotion]" in r.stderr, args
    r = run_cli("color_flow", ["a.txt", "b.png"])
    assert r.returncode != 0 and "extension .flo expected" in r.stderr
    r = run_cli("color_flow", [str(tmp_path / "none.flo"), "b.png"])
    assert r.returncode != 0 and "ReadFlowFile" in r.stderr
    r = run_cli("color_flow", ["a.flo", "b.png", "fast"])
    assert r.returncode != 0 and "maxmotion" in r.stderr


def test_color_entry_points_declared_and_bound():
    import flowonthego_amd as F
    hdr = open(os.path.join(ROOT, "include", "fotg.h")).read()
    for name in ("fotg_flow_color", "fotg_upsample_crop_color"):
        assert "int %s(" % name in hdr and name in {s[0] for s in F._lib.SYMBOLS}
        assert hasattr(F.lib(), name)
    src = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "flowcolor.hip.h")).read() + \
        open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_color.hip")).read()
    assert "getenv" not in src
    txt = open(os.path.join(ROOT, "flowonthego_amd", "libfotg.resusage.txt")).read()
    for k in ("flow_range_kernel", "flow_color_kernel", "flow_stats_kernel"):
        assert k in txt, k
