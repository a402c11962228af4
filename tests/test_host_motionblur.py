"""The motion blur's host side (no GPU needed): the C-ABI is declared and bound, examples/motion_blur.cpp compiles and links against
the C++ shim, the compiler's resource table lists exactly the expected instantiations of the mblur_ kernels, all without a
private-memory segment, and the arguments the entry points refuse are refused before the device is touched.  With a GPU: the CLI
writes what the call returns."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from host_checks import cli_refuses, entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_motion_blur", "fotg_upsample_crop_motion_blur")
FOTG_ERR_ARG = 1


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "blur.h")
    from flowonthego_amd import motionblur
    assert F.upsample_crop_motion_blur is motionblur.upsample_crop_motion_blur and callable(motionblur.ofc_motion_blur)
    assert F.BLUR_STATS == motionblur.STATS and len(F.BLUR_STATS) == 8 and len(set(F.BLUR_STATS)) == 8
    assert callable(F.motion_blur) and F.motion_blur.__name__ == "flowonthego_amd.motion_blur"          # the tool's module, callable
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.motion_blur) and callable(OFClass.upsample_crop_motion_blur)
    # the definition is written at the head of the kernel and in the public header; the C-ABI file sits on the shared scaffold
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "motionblur.hip.h")).read()
    for text in (head, hdr):
        for expr in ("(float)shutter256 / 32", "cap16 = 16 max_blur", "hx = hx cap16 / len", "lowest linear pixel index",
                     "first in raster order", "lenD < 8", "L = (lenD + 15) / 16", "(2 |Dx| a + L) / (2 L)", "(ox + 8) >> 4", "d_k = lenD a / L",
                     "|Hx(P) Dx + Hy(P) Dy| / lenD", "clamp(max(r(Y_k), r(X)) + 16 - d_k, 0, 16)", "(2 sum w_k c_k + W) / (2 W)",
                     "acc + (float)w_k c_k", "acc / (float)W"):
            assert expr in text, expr
    # the integer root is the histograms' routine, not a second copy
    assert '#include "histograms.hip.h"' in head and "mh_mag(" in head and "sqrt" not in head
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_motionblur.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi and "Scratch mem(" in capi
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_motionblur.hip" in mk and " motionblur.hip.h" in mk


def test_motion_blur_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "motion_blur")
    assert os.path.exists(exe)
    for args in ([], ["a.flo"], ["a.flo", "o.pgm", "0"], ["a.flo", "o.pgm", "2.5"], ["a.flo", "o.pgm", "0.5", "33"], ["a.flo", "o.pgm", "0.5", "8", "x"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_blur_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if "mblur_" in n)
    # Itanium-mangled: pass A over DenseSrc | UpsampleSrc, pass B over float | unsigned char x 1 | 3 channels, the fold -- nothing else
    want = ["mblur_vectors_kernelINS_8DenseSrcEEE", "mblur_vectors_kernelINS_11UpsampleSrcEEE", "mblur_gather_kernelIfLi1EE",
            "mblur_gather_kernelIfLi3EE", "mblur_gather_kernelIhLi1EE", "mblur_gather_kernelIhLi3EE", "mblur_fold_kernelE"]
    assert len(mine) == len(want), mine
    for frag in want:
        hit = [n for n in mine if frag in n]
        assert len(hit) == 1, (frag, mine)
        assert table[hit[0]] == 0, hit
    # the names stay clear of the substrings by which the other resource-table tests count their kernels
    for n in mine:
        assert not any(s in n for s in ("motion_", "comp_", "obj", "warp_", "flowfilter_", "temporal_", "blockmv_", "mh_kernel")), n
    # the histograms' header has a second includer now: its kernel is still compiled once per source
    assert sum("mh_kernel" in n for n in names) == 2


def test_arguments_are_refused_before_the_device_is_touched():
    """every pointer is a host address that is never dereferenced: FOTG_ERR_ARG is decided first"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps

    def call(n=1, s=far(1), ty=0, ch=1, f=far(2), w=8, h=8, m=None, sh=128, mb=32, d=far(3), c=None, v=None, st=None):
        return L.fotg_motion_blur(0, n, s, ty, ch, f, w, h, m, sh, mb, d, c, v, st, None)

    for bad in (dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=0), dict(w=16385), dict(h=16385), dict(ty=2), dict(ty=-1), dict(ch=0),
                dict(ch=2), dict(ch=4), dict(sh=0), dict(sh=513), dict(sh=-128), dict(mb=0), dict(mb=33), dict(mb=-1), dict(s=None), dict(f=None),
                dict(d=None), dict(d=far(1)), dict(d=far(2)), dict(c=far(1)), dict(c=far(2)), dict(v=far(1)), dict(v=far(2)), dict(st=far(1)),
                dict(st=far(2)), dict(m=far(3)), dict(m=far(4), c=far(4)), dict(m=far(4), v=far(4)), dict(m=far(4), st=far(4)),
                dict(c=far(3)), dict(v=far(3)), dict(st=far(3)), dict(c=far(4), v=far(4)), dict(c=far(4), st=far(4)), dict(v=far(4), st=far(4)),
                dict(ty=1, d=C.c_void_p(0x10000000 * 2 + 8 * 8 * 4 - 1))):
        assert call(**bad) == FOTG_ERR_ARG, bad
    assert L.fotg_upsample_crop_motion_blur(None, 1, far(1), 0, 1, far(2), None, 128, 32, far(3), None, None, None, None) == FOTG_ERR_ARG


def test_cli_refuses_bad_arguments():
    cli_refuses("motion_blur", ([], ["a.npy"], ["a.npy", "b.flo", "c.png", "d"], ["a.npy", "b.flo", "c.png", "--shutter", "0"],
                                ["a.npy", "b.flo", "c.png", "--shutter", "2.5"], ["a.npy", "b.flo", "c.png", "--max-blur", "33"],
                                ["a.npy", "b.flo", "c.png", "--max-blur", "0"], ["a.npy", "b.npy", "--mask", "m.png"],
                                ["a.npy", "b.flo", "c.png", "--occlusion"]))


@pytest.mark.gpu
def test_cli_writes_what_the_call_returns(tmp_path):
    import numpy as np
    import torch
    import flowonthego_amd as F
    import motionblur_ref as R
    from flowonthego_amd.flo import write_flo
    from flowonthego_amd.color import write_png
    rng = np.random.default_rng(11)
    h, w = 37, 70
    flow = (rng.integers(-1024, 1025, (h, w, 2)) / 512.0).astype(np.float32)
    flow[10:20, 5:15] = (30.0, -7.5)
    flow[3, 3] = (np.nan, 0.0)
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    fr, fl, out, cd = (str(tmp_path / n) for n in ("f.npy", "f.flo", "out.png", "code.png"))
    np.save(fr, frame)
    write_flo(fl, flow)
    run = run_cli("motion_blur", [fr, fl, out, "--shutter", "0.75", "--max-blur", "9", "--code", cd])
    assert run.returncode == 0, run.stderr
    dst, code, st = F.motion_blur(torch.from_numpy(frame).cuda(), torch.from_numpy(flow).cuda(), None, 0.75, 9, code=True, stats=True)
    wd, wc, _, ws = R.blur(frame[None], flow[None], None, 192, 9)
    assert np.array_equal(dst.cpu().numpy(), wd[0]) and np.array_equal(code.cpu().numpy(), wc[0]) and np.array_equal(st.cpu().numpy(), ws[0])
    assert (wc == 1).any() and (wc == 2).any() and (wc == 3).sum() == 1
    # the PNGs hold the call's bytes
    ref_png, ref_code = str(tmp_path / "ref.png"), str(tmp_path / "refcode.png")
    write_png(ref_png, wd[0])
    from flowonthego_amd.motion_blur import CODE_RGB
    write_png(ref_code, np.array(CODE_RGB, np.uint8)[wc[0]])
    assert open(out, "rb").read() == open(ref_png, "rb").read() and open(cd, "rb").read() == open(ref_code, "rb").read()
    px = float(h * w)
    assert run.stdout.startswith("untouched %.4f  blurred %.4f  clamped %.4f  unknown %.4f  taps per pixel %.3f" % (
        ws[0, 0] / px, ws[0, 1] / px, ws[0, 2] / px, ws[0, 3] / px, ws[0, 4] / px))
