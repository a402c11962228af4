"""The background subtraction's host side (no GPU needed): the C-ABI is declared and bound, examples/subtract_background.cpp compiles
and links against the C++ shim, the compiler's resource table lists exactly the expected instantiations of subtract_kernel, all
without a private-memory segment, the arguments the entry points refuse are refused before the device is touched, and the tool
refuses bad arguments and bad files.  With a GPU: the CLI writes what the call returns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from host_checks import cli_refuses, entry_points, read_png_rgb, resource_table, run_cli

NEW_SYMBOLS = ("fotg_subtract", "fotg_subtract_u8", "fotg_subtract_motion", "fotg_subtract_motion_u8", "fotg_upsample_crop_subtract",
               "fotg_upsample_crop_subtract_u8")
FOTG_ERR_ARG = 1


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "subtract.h")
    from flowonthego_amd import subtract
    for name in ("subtract_background", "upsample_crop_subtract_background", "frame_motions", "foreground_objects", "foreground_mask"):
        assert getattr(F, name) is getattr(subtract, name) and F.LAZY[name] == ("subtract", name)
    assert callable(subtract.ofc_foreground) and len(subtract.STATS) == 7 and len(set(subtract.STATS)) == 7 and subtract.FG == (1, 4)
    assert callable(F.foreground) and F.foreground.__name__ == "flowonthego_amd.foreground" and "foreground" in F.CLI_MODULES
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.foreground) and callable(OFClass.upsample_crop_subtract_background)
    # the definition is written at the head of the kernel and in the public header; the C-ABI file sits on the shared scaffold
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "subtract.hip.h")).read()
    for text in (head, hdr):
        for expr in ("mask[i][y][x] != 0", "Xc = (float)(x + ox) + u", "Yc = (float)(y + oy) + v", "warp_inside(Xc, Yc, W, H)",
                     "four clamped tap pixels", "warp_taps(plate[index[i]], W, H, Xc, Yc)", "e = fabsf(f_ch - s_ch)", "d = e > d ? e : d",
                     "Dq = (int)(fminf(d * 16.f, 32767.f) + 0.5f)", "L = lrintf(16 low), Hh = lrintf(16 high)", "S >= Hh * C", "S >= L * C",
                     "motion_predict(motion_coef(P_i, w, h), 2x - (w-1), 2y - (h-1))", "code == 4 ? 1 : 0", "4 strong foreground"):
            assert expr in text, expr
    assert "overlap_any" in hdr and "overlap_among" in hdr
    for inc in ('#include "warp.hip.h"', '#include "plate.hip.h"', "warp_taps<T, NOC>", "warp_inside(", "warp_sat(", "clampi(", "__syncthreads"):
        assert inc in head, inc
    body = head.split("#pragma once")[1]
    assert "struct MotionSrc" not in body and "atomicAdd(stats" in body and "double" not in body        # integer atomics only
    assert body.count("__syncthreads") == 2                                                           # the tile, then the statistics
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_subtract.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi and "Scratch mem(" in capi
    assert "fused_geom(" in capi and "upsample_src(" in capi and "hipMemsetAsync(stats" in capi
    for sync in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc(", "hipEventSynchronize"):
        assert sync not in capi, sync
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_subtract.hip" in mk and " subtract.hip.h" in mk


def test_subtract_background_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "subtract_background")
    assert os.path.exists(exe)
    for args in ([], ["a.raw"], ["a.raw", "8", "8", "1", "o.raw"], ["a.raw", "8", "8", "33", "o.raw"], ["a.raw", "8", "8", "4", "o.raw", "-1"],
                 ["a.raw", "8", "8", "4", "o.raw", "9", "8"], ["a.raw", "8", "8", "4", "o.raw", "8", "2048"],
                 ["a.raw", "8", "8", "4", "o.raw", "8", "24", "3"], ["a.raw", "8", "8", "4", "o.raw", "8", "24", "1", "5"],
                 ["a.raw", "0", "8", "4", "o.raw"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_subtract_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if "subtract_" in n)
    # Itanium-mangled: subtract_kernel over DenseSrc | MotionSrc | UpsampleSrc x float | unsigned char x 1 | 3 channels -- nothing else
    want = ["subtract_kernelINS_%s%sLi%dEE" % (s, t, c) for s in ("8DenseSrcE", "9MotionSrcE", "11UpsampleSrcE") for t in "fh" for c in (1, 3)]
    assert len(mine) == len(want) == 12, mine
    for frag in want:
        hit = [n for n in mine if frag in n]
        assert len(hit) == 1, (frag, mine)
        assert table[hit[0]] == 0, hit
    # the names stay clear of the substrings by which the other resource-table tests count their kernels
    for n in mine:
        assert not any(s in n for s in ("motion_", "comp_", "obj", "warp_", "flowfilter_", "temporal_", "blockmv_", "mh_kernel", "mblur_",
                                        "plate_", "layers_")), n
    # including plate.hip.h for MotionSrc compiles no second plate kernel
    assert sum("plate_kernel" in n for n in names) == 12


def test_arguments_are_refused_before_the_device_is_touched():
    """every pointer is a host address that is never dereferenced: FOTG_ERR_ARG is decided first (index is read, so it is real)"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)

    def call(fn=L.fotg_subtract, n=2, f=far(1), w=8, h=8, ch=1, P=3, pl=far(2), W=9, H=7, ox=0, oy=0, ix=(0, 2), s=far(3), pc=None, mk=None,
             low=8.0, high=24.0, r=1, cd=far(4), df=None, ev=None, st=None):
        return fn(0, n, f, w, h, ch, P, pl, W, H, ox, oy, ints(ix), s, pc, mk, C.c_float(low), C.c_float(high), r, cd, df, ev, st, None)

    bad = (dict(n=0), dict(n=-1), dict(n=65536), dict(P=0), dict(P=65536), dict(w=0), dict(h=0), dict(w=16385), dict(h=16385), dict(W=0),
           dict(H=0), dict(W=16385), dict(H=16385), dict(ox=(1 << 20) + 1), dict(oy=-(1 << 20) - 1), dict(ch=0), dict(ch=2), dict(ch=4),
           dict(r=-1), dict(r=3), dict(low=-1.0), dict(low=25.0), dict(high=2048.0), dict(low=float("nan")), dict(high=float("inf")),
           dict(high=float("nan")), dict(low=-float("inf")), dict(ix=(0, 3)), dict(ix=(-1, 0)), dict(ix=None), dict(f=None), dict(pl=None),
           dict(s=None), dict(cd=None), dict(cd=far(1)), dict(cd=far(2)), dict(cd=far(3)), dict(df=far(1)), dict(ev=far(2)), dict(st=far(3)),
           dict(pc=far(4)), dict(mk=far(4)), dict(pc=far(5), df=far(5)), dict(mk=far(5), ev=far(5)), dict(df=far(4)), dict(ev=far(4)),
           dict(st=far(4)), dict(df=far(5), ev=far(5)), dict(df=far(5), st=far(5)), dict(ev=far(5), st=far(5)),
           dict(cd=C.c_void_p(0x10000000 * 4 + 2 * 8 * 8 * 2 * 4 - 1)))
    for fn in (L.fotg_subtract, L.fotg_subtract_u8, L.fotg_subtract_motion, L.fotg_subtract_motion_u8):
        for b in bad[:-1]:
            assert call(fn, **b) == FOTG_ERR_ARG, b
    assert call(**bad[-1]) == FOTG_ERR_ARG                          # the last byte of the flows
    for fn in (L.fotg_upsample_crop_subtract, L.fotg_upsample_crop_subtract_u8):
        assert fn(None, 1, far(1), far(2), 1, 1, far(3), 9, 7, 0, 0, None, None, None, C.c_float(8), C.c_float(24), 1, far(4), None, None, None,
                  None) == FOTG_ERR_ARG


def test_cli_refuses_bad_arguments():
    cli_refuses("foreground", ([], ["a.npy"], ["a.npy", "b.npy", "c"], ["a.npy", "b.npy", "--model", "homography"],
                               ["a.npy", "b.npy", "--low", "-1"], ["a.npy", "b.npy", "--low", "30"], ["a.npy", "b.npy", "--high", "2048"],
                               ["a.npy", "b.npy", "--low", "nan"], ["a.npy", "b.npy", "--window", "3"], ["a.npy", "b.npy", "--min-area", "0"],
                               ["a.npy", "b.npy", "--ref", "-1"], ["a.npy", "b.npy", "--ref"]))


def test_cli_refuses_bad_files(tmp_path):
    """one line "foreground: <message>" and return value 1, before the device is touched"""
    p = lambda n: str(tmp_path / n)
    np.save(p("one.npy"), np.zeros((1, 8, 8), np.uint8))
    np.save(p("many.npy"), np.zeros((33, 8, 8), np.uint8))
    np.save(p("f64.npy"), np.zeros((3, 8, 8)))
    np.save(p("rgba.npy"), np.zeros((3, 8, 8, 4), np.uint8))
    np.save(p("ok.npy"), np.zeros((3, 8, 8), np.uint8))
    open(p("junk.npy"), "wb").write(b"not an array")
    for args in ([p("missing.npy"), p("o.npy")], [p("one.npy"), p("o.npy")], [p("many.npy"), p("o.npy")], [p("f64.npy"), p("o.npy")],
                 [p("rgba.npy"), p("o.npy")], [p("junk.npy"), p("o.npy")], [p("ok.npy"), p("o.npy"), "--ref", "3"]):
        r = run_cli("foreground", args)
        assert r.returncode == 1 and r.stderr.startswith("foreground: ") and len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)
        assert not os.path.exists(p("o.npy"))


def test_the_tool_imports_no_other_tool_and_ends_callable():
    src = open(os.path.join(ROOT, "flowonthego_amd", "foreground.py")).read()
    import flowonthego_amd as F
    for other in F.CLI_MODULES:
        assert "from .%s " % other not in src and "import %s" % other not in src, other
    assert "refusing(" in src and "frame_sequence(" in src and "sequence_context(" in src
    assert src.index("callable_module(") > src.index("def main(")
    assert src.index("ap.error(") < src.index("import numpy")                     # the parser's checks come before numpy or torch load


@pytest.mark.gpu
def test_cli_writes_what_the_call_returns(tmp_path, natural_images):
    import torch
    import motion_ref as M
    from flowonthego_amd._cli import CODE_RGB, sequence_context
    from flowonthego_amd.foreground import STRONG_RGB
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    fr, out, cd, pl = (str(tmp_path / n) for n in ("f.npy", "out.npy", "code.png", "plate.png"))
    np.save(fr, frames)
    run = run_cli("foreground", [fr, out, "--ref", "1", "--model", "similarity", "--low", "6", "--high", "30", "--window", "2", "--min-area", "32",
                                 "--code", cd, "--plate", pl])
    assert run.returncode == 0, run.stderr
    ofc = sequence_context(frames, 2, bidir=False, max_batch=4)
    mask, objects, confirmed, plate, code = ofc.foreground(torch.from_numpy(frames).cuda(), ref=1, model="similarity", low=6.0, high=30.0,
                                                           window=2, min_area=32)
    mask, confirmed, plate, code = mask.cpu().numpy(), confirmed.cpu().numpy(), plate.cpu().numpy(), code.cpu().numpy()
    got = np.load(out)
    assert got.dtype == np.uint8 and got.shape == frames.shape and np.array_equal(got, mask) and mask.any()
    palette = np.array(CODE_RGB + (STRONG_RGB,), np.uint8)
    assert len(palette) == 5 and len({tuple(c) for c in palette.tolist()}) == 5
    assert np.array_equal(read_png_rgb(cd), palette[code[1]])
    assert np.array_equal(read_png_rgb(pl), np.broadcast_to(plate[..., None], plate.shape + (3,)))
    lines = run.stdout.strip().splitlines()
    assert lines[0] == "foreground of 5 frames of 320 x 192 against the plate on frame 1:" and len(lines) == 6
    for k in range(5):
        assert lines[1 + k] == "  frame %d: %d confirmed objects, foreground %.4f" % (k, confirmed[k].sum(), mask[k].mean())
    ofc.close()
