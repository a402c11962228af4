"""The background plate's host side (no GPU needed): the C-ABI is declared and bound, examples/background_plate.cpp compiles and
links against the C++ shim, the compiler's resource table lists exactly the expected instantiations of plate_kernel, all without a
private-memory segment, the arguments the entry points refuse are refused before the device is touched, and the tool refuses bad
arguments and bad files.  With a GPU: the CLI writes what the call returns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from host_checks import cli_refuses, entry_points, read_png_rgb, resource_table, run_cli

NEW_SYMBOLS = ("fotg_plate", "fotg_plate_u8", "fotg_plate_motion", "fotg_plate_motion_u8", "fotg_upsample_crop_plate",
               "fotg_upsample_crop_plate_u8")
FOTG_ERR_ARG = 1


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "plate.h")
    entry_points(("fotg_plate_rows",), "plate.h", in_shim=())
    from flowonthego_amd import plate
    for name in ("background_plate", "upsample_crop_background_plate", "plate_motions", "mosaic_canvas"):
        assert getattr(F, name) is getattr(plate, name) and F.LAZY[name] == ("plate", name)
    assert callable(plate.ofc_background) and len(plate.STATS) == 6 and len(set(plate.STATS)) == 6
    assert callable(F.background) and F.background.__name__ == "flowonthego_amd.background" and "background" in F.CLI_MODULES
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.background) and callable(OFClass.upsample_crop_background_plate)
    # the definition is written at the head of the kernel and in the public header; the C-ABI file sits on the shared scaffold
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "plate.hip.h")).read()
    for text in (head, hdr):
        for expr in ("2x - (w-1), 2y - (h-1)", "u and v are finite", "occ[i][k][Y][X] == 0", "four clamped tap pixels", "is NaN",
                     "ties keeping the k order", "s[(m-1)/2]", "(s[m/2 - 1] + s[m/2]) * 0.5f", "sum / (float)m", "coverage < min_count"):
            assert expr in text, expr
    assert "overlap_any" in hdr and "overlap_among" in hdr
    for inc in ('#include "warp.hip.h"', '#include "motion_model.hip.h"', "struct MotionSrc", "extern __shared__", "warp_taps<T, NOC>"):
        assert inc in head, inc
    assert "__syncthreads" not in head and "atomic" not in head.split("#pragma once")[1]
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_plate.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi and "Scratch mem(" in capi
    assert "lds_opt_in(" in capi and "hipFuncSetAttribute" not in capi and "warp_fold(" in capi
    # one attribute helper for the whole library
    srcs = [f for f in os.listdir(os.path.join(ROOT, "flowonthego_amd", "csrc")) if f.endswith((".hip", ".h"))]
    assert [f for f in srcs if "hipFuncSetAttribute(" in open(os.path.join(ROOT, "flowonthego_amd", "csrc", f)).read()] == ["host_call.h"]
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_plate.hip" in mk and " plate.hip.h" in mk


def test_background_plate_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "background_plate")
    assert os.path.exists(exe)
    for args in ([], ["a.raw"], ["a.raw", "8", "8", "0", "o.raw"], ["a.raw", "8", "8", "33", "o.raw"], ["a.raw", "8", "8", "4", "o.raw", "5"],
                 ["a.raw", "8", "8", "4", "o.raw", "1", "mode"], ["a.raw", "8", "8", "4", "o.raw", "1", "mean", "9"], ["a.raw", "0", "8", "4", "o.raw"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_plate_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if "plate_" in n)
    # Itanium-mangled: plate_kernel over DenseSrc | MotionSrc | UpsampleSrc x float | unsigned char x 1 | 3 channels -- nothing else
    want = ["plate_kernelINS_%s%sLi%dEE" % (s, t, c) for s in ("8DenseSrcE", "9MotionSrcE", "11UpsampleSrcE") for t in "fh" for c in (1, 3)]
    assert len(mine) == len(want) == 12, mine
    for frag in want:
        hit = [n for n in mine if frag in n]
        assert len(hit) == 1, (frag, mine)
        assert table[hit[0]] == 0, hit
    # the names stay clear of the substrings by which the other resource-table tests count their kernels
    for n in mine:
        assert not any(s in n for s in ("motion_", "comp_", "obj", "warp_", "flowfilter_", "temporal_", "blockmv_", "mh_kernel", "mblur_")), n
    # the fold is the warp's, compiled once
    assert sum("warp_fold_kernel" in n for n in names) == 1


def test_arguments_are_refused_before_the_device_is_touched():
    """every pointer is a host address that is never dereferenced: FOTG_ERR_ARG is decided first (index is read, so it is real)"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)

    def call(fn=L.fotg_plate, n=1, K=2, T=3, f=far(1), w=8, h=8, ch=1, ix=(0, -1), s=far(2), W=9, H=7, ox=0, oy=0, occ=None, ex=None, mode=0,
             mc=1, ref=None, d=far(3), cnt=None, cd=None, st=None):
        return fn(0, n, K, T, f, w, h, ch, ints(ix), s, W, H, ox, oy, occ, ex, mode, mc, C.c_float(0), ref, d, cnt, cd, st, None)

    bad = (dict(n=0), dict(n=-1), dict(n=65536), dict(K=0), dict(K=33, ix=(0,) * 33), dict(T=0), dict(w=0), dict(h=0), dict(w=16385),
           dict(h=16385), dict(W=0), dict(H=0), dict(W=16385), dict(H=16385), dict(ox=1 << 21), dict(oy=-(1 << 21)), dict(ch=0), dict(ch=2),
           dict(ch=4), dict(mode=2), dict(mode=-1), dict(mc=0), dict(mc=3), dict(ix=(0, 3)), dict(ix=(-2, 0)), dict(ix=None), dict(f=None),
           dict(s=None), dict(d=None), dict(d=far(1)), dict(d=far(2)), dict(cnt=far(1)), dict(cd=far(2)), dict(st=far(1)),
           dict(occ=far(3)), dict(ex=far(3)), dict(ref=far(3)), dict(occ=far(4), cnt=far(4)), dict(ex=far(4), cd=far(4)),
           dict(ref=far(4), st=far(4)), dict(cnt=far(3)), dict(cd=far(3)), dict(st=far(3)), dict(cnt=far(4), cd=far(4)),
           dict(cnt=far(4), st=far(4)), dict(cd=far(4), st=far(4)), dict(d=C.c_void_p(0x10000000 * 3 + 2 * 9 * 7 * 2 * 4 - 1)))
    for fn in (L.fotg_plate, L.fotg_plate_u8, L.fotg_plate_motion, L.fotg_plate_motion_u8):
        for b in bad[:-1]:
            assert call(fn, **b) == FOTG_ERR_ARG, b
    assert call(**bad[-1]) == FOTG_ERR_ARG                          # the last byte of the flows
    for fn in (L.fotg_upsample_crop_plate, L.fotg_upsample_crop_plate_u8):
        assert fn(None, 1, 2, 3, far(1), far(2), 1, ints((0, 1)), None, None, 0, 1, C.c_float(0), None, far(3), None, None, None, None) == FOTG_ERR_ARG


def test_cli_refuses_bad_arguments():
    cli_refuses("background", ([], ["a.npy"], ["a.npy", "b.png", "c"], ["a.npy", "b.png", "--model", "homography"],
                               ["a.npy", "b.png", "--mode", "mode"], ["a.npy", "b.png", "--min-count", "0"],
                               ["a.npy", "b.png", "--min-count", "33"], ["a.npy", "b.png", "--ref", "-1"], ["a.npy", "b.png", "--ref"]))


def test_cli_refuses_bad_files(tmp_path):
    """one line "background: <message>" and return value 1, before the device is touched"""
    p = lambda n: str(tmp_path / n)
    np.save(p("one.npy"), np.zeros((1, 8, 8), np.uint8))
    np.save(p("many.npy"), np.zeros((33, 8, 8), np.uint8))
    np.save(p("f64.npy"), np.zeros((3, 8, 8)))
    np.save(p("rgba.npy"), np.zeros((3, 8, 8, 4), np.uint8))
    np.save(p("ok.npy"), np.zeros((3, 8, 8), np.uint8))
    open(p("junk.npy"), "wb").write(b"not an array")
    for args in ([p("missing.npy"), p("o.png")], [p("one.npy"), p("o.png")], [p("many.npy"), p("o.png")], [p("f64.npy"), p("o.png")],
                 [p("rgba.npy"), p("o.png")], [p("junk.npy"), p("o.png")], [p("ok.npy"), p("o.png"), "--ref", "3"],
                 [p("ok.npy"), p("o.png"), "--min-count", "4"]):
        r = run_cli("background", args)
        assert r.returncode == 1 and r.stderr.startswith("background: ") and len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)
        assert not os.path.exists(p("o.png"))


@pytest.mark.gpu
def test_cli_writes_what_the_call_returns(tmp_path, natural_images):
    import torch
    import motion_ref as M
    from flowonthego_amd._cli import CODE_RGB, sequence_context
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    fr, out, cd, cn = (str(tmp_path / n) for n in ("f.npy", "out.png", "code.png", "count.png"))
    np.save(fr, frames)
    run = run_cli("background", [fr, out, "--ref", "1", "--model", "similarity", "--mosaic", "--min-count", "2", "--code", cd, "--count", cn])
    assert run.returncode == 0, run.stderr
    ofc = sequence_context(frames, 2, bidir=False, max_batch=4)
    plate, code, count = ofc.background(torch.from_numpy(frames).cuda(), ref=1, model="similarity", mosaic=True, min_count=2)
    plate, code, count = plate.cpu().numpy(), code.cpu().numpy(), count.cpu().numpy()
    H, W = code.shape
    assert (W, H) != (frames.shape[2], frames.shape[1]) and (code == 0).any() and (code == 2).any()
    assert np.array_equal(read_png_rgb(out), np.broadcast_to(plate[..., None], (H, W, 3)))
    assert np.array_equal(read_png_rgb(cd), np.array(CODE_RGB, np.uint8)[code])
    assert np.array_equal(read_png_rgb(cn)[..., 0], (count.astype(np.uint32) * 255 // 5).astype(np.uint8))
    n = np.bincount(code.ravel(), minlength=3) / float(H * W)
    assert run.stdout.startswith("plate %d x %d from 5 frames of 320 x 192: estimated %.4f  hidden %.4f  uncovered %.4f" % (W, H, n[0], n[1], n[2]))
    ofc.close()
