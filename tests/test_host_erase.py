"""The object removal's host side (no GPU needed): the C-ABI is declared and bound, examples/remove_objects.cpp compiles and links
against the C++ shim, the definition stands word for word in the kernel's header and in the public one, the compiler's resource
table lists exactly the expected instantiations of erase_kernel, all without a private-memory segment and without adding to any
other feature's kernels, the arguments the entry points refuse are refused before the device is touched, and the tool refuses bad
arguments and bad files."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from host_checks import cli_refuses, entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_erase", "fotg_erase_u8", "fotg_erase_motion", "fotg_erase_motion_u8", "fotg_upsample_crop_erase",
               "fotg_upsample_crop_erase_u8")
FOTG_ERR_ARG = 1
# the substrings by which the resource-table tests of the other features count their kernels
OTHERS = ("motion_", "comp_", "objvote", "objlink", "objtrack", "warp_", "flowfilter_", "temporal_", "blockmv_", "mh_kernel", "mblur_", "plate_",
          "layers_", "subtract_", "interp")


def _definition(text, prefix):
    """the lines of the definition, from "n frames of" to the sentence on grow_mask, without the comment prefix"""
    lines = text.splitlines()
    a = next(i for i, ln in enumerate(lines) if ln.startswith(prefix + "n frames of w x h with 1 or 3 interleaved channels"))
    b = next(i for i, ln in enumerate(lines) if i > a and "flowonthego_amd.erase.grow_mask" in ln)
    assert all(ln.startswith(prefix) for ln in lines[a:b + 1])
    return [ln[len(prefix):] for ln in lines[a:b + 1]]


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "erase.h")
    from flowonthego_amd import erase
    for name in ("upsample_crop_remove_objects", "grow_mask"):
        assert getattr(F, name) is getattr(erase, name) and F.LAZY[name] == ("erase", name)
    assert "remove_objects" not in F.LAZY and callable(erase.remove_objects)       # the package's name for it is the callable tool module
    assert callable(erase.ofc_remove_objects) and len(erase.STATS) == 8 and len(set(erase.STATS)) == 8 and len(erase.CODES) == 5
    assert callable(F.remove_objects) and F.remove_objects.__name__ == "flowonthego_amd.remove_objects" and "remove_objects" in F.CLI_MODULES
    import flowonthego_amd.erase as module
    assert callable(module) and F.CLI_MODULES.count("remove_objects") == 1
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.remove_objects) and callable(OFClass.upsample_crop_remove_objects)
    import inspect
    assert str(inspect.signature(OFClass.remove_objects)) == ("(self, frames, ref=0, model='affine', low=8.0, high=24.0, window=1, min_area=64, "
                                                              "max_objects=256, grow=2, feather=3)")
    # the definition is written at the head of the kernel and in the public header, word for word the same
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "erase.hip.h")).read()
    mine, public = _definition(head, "// "), _definition(hdr, " * ")
    assert mine == public and len(mine) > 20
    for text in (head, hdr):
        for expr in ("|x - x'| <= R and |y - y'| <= R", "D2 <= G * G: alpha = 256", "D16 = floor(sqrt(256 * D2))", "E = 16 * (G + F) - D16",
                     "alpha = E <= 0 ? 0 : min(256, (256 * E + 8 * F) / (16 * F))", "mask[i][y][x] != 0", "Xc = (float)(x + ox) + u",
                     "Yc = (float)(y + oy) + v", "warp_inside(Xc, Yc, W, H)", "four clamped tap pixels", "warp_taps(plate[index[i]], W, H, Xc, Yc)",
                     "a = (float)alpha * 0.00390625f", "dst = f + (s - f) * a", "warp_to_u8(s)", "a NaN in the frame pixel does not disqualify",
                     "0 untouched, 1 replaced, 2 no plate there (kept), 3 unknown (kept), 4 blended", "n x 8 int64"):
            assert expr in text, expr
    assert "overlap_any" in hdr and "overlap_among" in hdr
    for inc in ('#include "warp.hip.h"', '#include "plate.hip.h"', "warp_taps<T, NOC>", "warp_inside(", "warp_sat(", "clampi(", "warp_store4<T, NOC>",
                "warp_store_code4(", "__ballot(", "__syncthreads", "bank"):
        assert inc in head, inc
    body = head.split("#pragma once")[1]
    assert "struct MotionSrc" not in body and "atomicAdd(stats" in body and "double" not in body        # integer atomics only
    assert "sqrtf((float)n)" in body and "__umul24(s + 1, s + 1) <= n" in body                         # the estimate, then the exact products
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_erase.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi and "Scratch mem(" in capi
    assert "fused_geom(" in capi and "upsample_src(" in capi and "hipMemsetAsync(stats" in capi
    for sync in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc(", "hipEventSynchronize"):
        assert sync not in capi, sync
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_erase.hip" in mk and " erase.hip.h" in mk


def test_remove_objects_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "remove_objects")
    assert os.path.exists(exe)
    ok = ["a.raw", "m.raw", "8", "8", "4", "o.raw"]
    for args in ([], ["a.raw"], ok[:5], ["a.raw", "m.raw", "8", "8", "1", "o.raw"], ["a.raw", "m.raw", "8", "8", "33", "o.raw"],
                 ["a.raw", "m.raw", "0", "8", "4", "o.raw"], ["a.raw", "m.raw", "8", "-1", "4", "o.raw"], ok + ["-1"], ok + ["9"], ok + ["2", "-1"],
                 ok + ["2", "9"], ok + ["2", "3", "0"], ok + ["2", "3", "5"], ok + ["2", "3", "2", "x"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_erase_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if "erase" in n)
    # Itanium-mangled: erase_kernel over DenseSrc | MotionSrc | UpsampleSrc x float | unsigned char x 1 | 3 channels -- nothing else:
    # grow_mask runs the dense f32 one-channel instantiation with alpha as its only output
    want = ["erase_kernelINS_%s%sLi%dEE" % (s, t, c) for s in ("8DenseSrcE", "9MotionSrcE", "11UpsampleSrcE") for t in "fh" for c in (1, 3)]
    assert len(mine) == len(want) == 12, mine
    for frag in want:
        hit = [n for n in mine if frag in n]
        assert len(hit) == 1, (frag, mine)
        assert table[hit[0]] == 0, hit
    for n in mine:
        assert not any(s in n for s in OTHERS), n
    # what the other features' tests count is what it was: including warp.hip.h, plate.hip.h and flowsrc.hip.h instantiates no second
    # warp, plate or subtract kernel
    count = lambda s: sum(s in n for n in names)
    assert count("subtract_") == 12 and count("plate_kernel") == 12 and count("warp_kernel") == len(set(n for n in names if "warp_kernel" in n))
    assert count("warp_fold_kernel") == 1
    assert len(names) - 12 == len([n for n in names if "erase" not in n])
    # every kernel of the library is still free of private memory
    assert not [n for n in names if table[n]]


def test_arguments_are_refused_before_the_device_is_touched():
    """every pointer is a host address that is never dereferenced: FOTG_ERR_ARG is decided first (index is read, so it is real)"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)

    def call(fn=L.fotg_erase, n=2, f=far(1), w=8, h=8, ch=1, P=3, pl=far(2), W=9, H=7, ox=0, oy=0, ix=(0, 2), s=far(3), pc=None, mk=None,
             rm=far(6), G=2, Fe=3, d=far(4), cd=None, al=None, st=None):
        return fn(0, n, f, w, h, ch, P, pl, W, H, ox, oy, ints(ix), s, pc, mk, rm, G, Fe, d, cd, al, st, None)

    bad = (dict(n=0), dict(n=-1), dict(n=65536), dict(P=0), dict(P=65536), dict(w=0), dict(h=0), dict(w=16385), dict(h=16385), dict(W=0),
           dict(H=0), dict(W=16385), dict(H=16385), dict(ox=(1 << 20) + 1), dict(oy=-(1 << 20) - 1), dict(ch=0), dict(ch=2), dict(ch=4),
           dict(G=-1), dict(G=9), dict(Fe=-1), dict(Fe=9), dict(G=1 << 30), dict(Fe=-(1 << 31)),
           dict(ix=(0, 3)), dict(ix=(-1, 0)), dict(ix=None), dict(f=None), dict(pl=None), dict(s=None), dict(rm=None),
           dict(d=None), dict(d=None, al=far(7), f=None, pl=None, s=None, rm=None),            # no output; alpha alone still needs remove
           dict(d=None, cd=far(4), pl=None), dict(d=None, st=far(4), s=None),                  # code or stats alone still sample
           dict(d=far(1)), dict(d=far(2)), dict(d=far(3)), dict(d=far(6)), dict(pc=far(4)), dict(mk=far(4)),     # dst on an input
           dict(cd=far(1)), dict(al=far(2)), dict(st=far(3)), dict(cd=far(6)), dict(pc=far(5), al=far(5)), dict(mk=far(5), st=far(5)),
           dict(cd=far(4)), dict(al=far(4)), dict(st=far(4)), dict(cd=far(5), al=far(5)), dict(cd=far(5), st=far(5)), dict(al=far(5), st=far(5)),
           dict(d=C.c_void_p(0x10000000 * 4 + 2 * 8 * 8 * 2 * 4 - 1)))
    for fn in (L.fotg_erase, L.fotg_erase_u8, L.fotg_erase_motion, L.fotg_erase_motion_u8):
        for b in bad[:-1]:
            assert call(fn, **b) == FOTG_ERR_ARG, b
    assert call(**bad[-1]) == FOTG_ERR_ARG                          # the last byte of the flows
    for fn in (L.fotg_upsample_crop_erase, L.fotg_upsample_crop_erase_u8):
        assert fn(None, 1, far(1), far(2), 1, 1, far(3), 9, 7, 0, 0, None, None, None, far(5), 2, 3, far(4), None, None, None, None) == FOTG_ERR_ARG


def test_cli_refuses_bad_arguments():
    cli_refuses("remove_objects", ([], ["a.npy"], ["a.npy", "b.npy", "c"], ["a.npy", "b.npy", "--model", "homography"],
                                   ["a.npy", "b.npy", "--low", "-1"], ["a.npy", "b.npy", "--low", "30"], ["a.npy", "b.npy", "--high", "2048"],
                                   ["a.npy", "b.npy", "--low", "nan"], ["a.npy", "b.npy", "--window", "3"], ["a.npy", "b.npy", "--min-area", "0"],
                                   ["a.npy", "b.npy", "--ref", "-1"], ["a.npy", "b.npy", "--ref"], ["a.npy", "b.npy", "--grow", "9"],
                                   ["a.npy", "b.npy", "--grow", "-1"], ["a.npy", "b.npy", "--feather", "9"], ["a.npy", "b.npy", "--feather", "1.5"],
                                   ["a.npy", "b.npy", "--mask"]))


def test_cli_refuses_bad_files(tmp_path):
    """one line "remove_objects: <message>" and return value 1, before the device is touched"""
    p = lambda n: str(tmp_path / n)
    np.save(p("one.npy"), np.zeros((1, 8, 8), np.uint8))
    np.save(p("many.npy"), np.zeros((33, 8, 8), np.uint8))
    np.save(p("f64.npy"), np.zeros((3, 8, 8)))
    np.save(p("rgba.npy"), np.zeros((3, 8, 8, 4), np.uint8))
    np.save(p("ok.npy"), np.zeros((3, 8, 8), np.uint8))
    np.save(p("rgb.npy"), np.zeros((3, 8, 8, 3), np.uint8))
    np.save(p("m2.npy"), np.zeros((2, 8, 8), np.uint8))
    np.save(p("mf.npy"), np.zeros((3, 8, 8), np.float32))
    open(p("junk.npy"), "wb").write(b"not an array")
    for args in ([p("missing.npy"), p("o.npy")], [p("one.npy"), p("o.npy")], [p("many.npy"), p("o.npy")], [p("f64.npy"), p("o.npy")],
                 [p("rgba.npy"), p("o.npy")], [p("junk.npy"), p("o.npy")], [p("ok.npy"), p("o.npy"), "--ref", "3"],
                 [p("ok.npy"), p("o.npy"), "--mask", p("m2.npy")], [p("ok.npy"), p("o.npy"), "--mask", p("mf.npy")],
                 [p("rgb.npy"), p("o.npy"), "--mask", p("rgb.npy")], [p("ok.npy"), p("o.npy"), "--mask", p("missing.npy")],
                 [p("ok.npy"), p("o.npy"), "--mask", p("junk.npy")]):
        r = run_cli("remove_objects", args)
        assert r.returncode == 1 and r.stderr.startswith("remove_objects: ") and len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)
        assert not os.path.exists(p("o.npy"))


def test_the_tool_imports_no_other_tool_and_ends_callable():
    src = open(os.path.join(ROOT, "flowonthego_amd", "remove_objects.py")).read()
    import flowonthego_amd as F
    for other in F.CLI_MODULES:
        assert "from .%s " % other not in src and not re.search(r"import %s\b" % other, src), other
    assert "refusing(" in src and "frame_sequence(" in src and "sequence_context(" in src and "load_array(" in src
    assert src.index("callable_module(") > src.index("def main(")
    assert src.index("ap.error(") < src.index("import numpy")                     # the parser's checks come before numpy or torch load
