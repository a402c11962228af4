"""The hole filling's host side (no GPU needed): the C-ABI is declared and bound, examples/fill_holes.cpp compiles and links against
the C++ shim, the definition stands word for word in the kernels' header and in the public one, the compiler's resource table lists
exactly the thirteen fill_ kernels, none with a private-memory segment and without adding to any other feature's kernels, the
arguments the entry points refuse are refused before the device is touched, fotg_fill_scratch equals its formula, the level geometry
(csrc/fill_levels.h) passes its stand-alone driver under the address and undefined-behaviour sanitizers, and the tool refuses bad
arguments and bad files."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from host_checks import cli_refuses, entry_points, gray_png_bytes, resource_table, run_cli

NEW_SYMBOLS = ("fotg_fill", "fotg_fill_u8", "fotg_fill_scratch")
FOTG_ERR_ARG = 1
HERE = os.path.dirname(os.path.abspath(__file__))
# the substrings by which the resource-table tests of the other features count their kernels
OTHERS = ("erase", "subtract_", "plate_", "layers_", "motion_", "comp_", "obj", "warp_", "flowfilter_", "temporal_", "blockmv_", "mh_kernel",
          "mblur_", "interp", "morph")


def _definition(text, prefix):
    """the lines of the definition, from "n images of" to the sentence on stats, without the comment prefix"""
    lines = text.splitlines()
    a = next(i for i, ln in enumerate(lines) if ln.startswith(prefix + "n images of w x h pixels with ch interleaved channels, 1 <= w, h <= 16384"))
    b = next(i for i, ln in enumerate(lines) if i > a and "with integer atomics and integer maxima: the same bytes every run." in ln)
    assert all(ln.startswith(prefix) for ln in lines[a:b + 1])
    return [ln[len(prefix):] for ln in lines[a:b + 1]]


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "fill.h")
    from flowonthego_amd import fill
    from flowonthego_amd.oflow import OFClass
    assert F.fill_flow is fill.fill_flow and F.LAZY["fill_flow"] == ("fill", "fill_flow") and F.fill_removed is fill.fill_removed
    assert F.FILL_CODES == ("known", "filled", "unfilled") and F.FILL_STATS == ("known", "filled", "unfilled", "depth")
    assert "fill_holes" not in F.LAZY and callable(fill.fill_holes)                # the package's name for it is the callable tool module
    assert callable(F.fill_holes) and F.fill_holes.__name__ == "flowonthego_amd.fill_holes" and F.CLI_MODULES.count("fill_holes") == 1
    assert str(inspect.signature(fill.fill_holes)) == "(src, hole=None, fg=None, dst=True, code=False, stats=False)"
    assert str(inspect.signature(fill.fill_flow)) == "(flow, mask=None)"
    assert str(inspect.signature(fill.upsample_crop_fill_flow)) == "(ofc, coarse, mask=None)"
    assert str(inspect.signature(OFClass.calc_filled)) == "(self, I0, I1, both=False, code=False, stats=False)"
    assert str(inspect.signature(OFClass.remove_objects_filled)) == "(self, frames, **kw)"
    # no existing signature changed
    assert str(inspect.signature(OFClass.remove_objects)).endswith("max_objects=256, grow=2, feather=3)")
    assert str(inspect.signature(OFClass.calc_filtered)).startswith("(self, I0, I1, radius=3, sigma=None, spatial=None, tau=20.0, iters=1")
    # the definition is written at the head of the kernels and in the public header, word for word the same
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fill.hip.h")).read()
    mine, public = _definition(head, "// "), _definition(hdr, " * ")
    assert mine == public and len(mine) >= 20
    for text in (head, hdr):
        for expr in ("b < 8 && ((fg_codes >> b) & 1)", "|v| <= 32768", "q = lrintf(256 v)", "w_{l+1} = (w_l + 1) >> 1", "|S| <= 2^51",
                     "M_l = (float)((double)S_l / (double)(256 N_l))", "px2 = clamp(px + (x & 1 ? 1 : -1), 0, w_{l+1} - 1)",
                     "F_l = ((a*9 + b*3) + (c*3 + d)) * 0.0625", "keeps its source value bit for bit", "clamped to [0, 255]",
                     "0 known (kept), 1 filled, 2 nothing", "known, filled, unfilled, depth", "n x 4 int64"):
            assert expr in text, expr
    assert "overlap_any" in hdr and "overlap_among" in hdr and "fotg_fill_scratch" in hdr and "1 GiB" in hdr
    body = head.split("#pragma once")[1]
    for used in ("__syncthreads", "atomicAdd(stats", "atomicMax(", "__shfl_xor(", "fill_levels.h", "(double)S / (double)"):
        assert used in body, used
    for absent in ("while (", "__threadfence", "volatile", "atomicCAS", "sleep"):          # no workgroup waits for another
        assert absent not in body, absent
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_fill.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi and "Scratch mem(" in capi
    assert "overlap_any(" in capi and "overlap_among(" in capi and "hipMemsetAsync(stats" in capi and capi.count("<<<") == 3
    for sync in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc(", "hipEventSynchronize"):
        assert sync not in capi, sync
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_fill.hip" in mk and " fill.hip.h" in mk and " fill_levels.h" in mk


def test_fill_holes_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "fill_holes")
    assert os.path.exists(exe)
    ok = ["f.raw", "m.raw", "8", "8", "3", "2", "o.raw"]
    for args in ([], ["f.raw"], ok[:6], ok + ["x"], ["f.raw", "m.raw", "0", "8", "3", "2", "o.raw"], ["f.raw", "m.raw", "8", "-1", "3", "2", "o.raw"],
                 ["f.raw", "m.raw", "8", "16385", "3", "2", "o.raw"], ["f.raw", "m.raw", "8", "8", "2", "2", "o.raw"],
                 ["f.raw", "m.raw", "8", "8", "4", "2", "o.raw"], ["f.raw", "m.raw", "8", "8", "3", "0", "o.raw"],
                 ["f.raw", "m.raw", "8", "8", "3", "65536", "o.raw"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_fill_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if "fill_" in n)
    pull = [n for n in mine if "fill_pull_kernel" in n]
    top = [n for n in mine if "fill_top_kernel" in n]
    push = [n for n in mine if "fill_push_kernel" in n]
    # <float, 1 | 2 | 3> and <unsigned char, 1 | 3> of pull and push, <1 | 2 | 3> of top
    assert len(mine) == 13 and len(pull) == 5 and len(top) == 3 and len(push) == 5, mine
    for group in (pull, push):
        assert sorted(re.search(r"kernelI(\w)Li(\d)E", n).groups() for n in group) == [("f", "1"), ("f", "2"), ("f", "3"), ("h", "1"), ("h", "3")]
    assert sorted(re.search(r"kernelILi(\d)E", n).group(1) for n in top) == ["1", "2", "3"]
    assert all(table[n] == 0 for n in mine)
    assert not any(s in n for s in OTHERS for n in mine), mine
    # what the other features' tests count is what it was
    count = lambda s: sum(s in n for n in names)
    assert count("erase") == 12 and count("subtract_") == 12 and count("plate_kernel") == 12 and count("warp_fold_kernel") == 1 and count("morph") == 1
    assert len(names) - 13 == len([n for n in names if "fill_" not in n])
    # every kernel of the library is still free of private memory
    assert not [n for n in names if table[n]]


def test_arguments_are_refused_before_the_device_is_touched():
    """src, hole and the outputs are host addresses that are never dereferenced: FOTG_ERR_ARG is decided first"""
    import flowonthego_amd as F
    L = F.lib()
    A = 0x10000000
    far = lambda k: C.c_void_p(A * (k + 1))                   # never touched: far apart, so that nothing overlaps
    at = lambda v: C.c_void_p(v)

    def call(fn="fotg_fill", n=2, s=far(1), w=8, h=8, ch=3, ho=far(2), fg=0, d=far(3), c=None, st=None):
        return getattr(L, fn)(0, n, s, w, h, ch, ho, fg, d, c, st, None)

    px, f32b = 2 * 8 * 8, 2 * 8 * 8 * 3 * 4
    bad = (dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=0), dict(w=-3), dict(w=16385), dict(h=16385), dict(ch=0), dict(ch=4), dict(ch=-1),
           dict(fn="fotg_fill_u8", ch=2), dict(fn="fotg_fill_u8", ch=4), dict(fn="fotg_fill_u8", ho=None), dict(s=None),
           dict(fg=-1), dict(fg=256), dict(d=None),                                    # no output
           dict(d=far(1)), dict(d=far(2)), dict(c=far(1)), dict(c=far(2)), dict(c=far(3)), dict(st=far(1)), dict(st=far(2)), dict(st=far(3)),
           dict(d=None, c=far(4), st=far(4)),                                          # the outputs on each other
           dict(d=at(A * 2 - f32b + 1)), dict(d=at(A * 2 + f32b - 1)), dict(c=at(A * 3 + px - 1)), dict(c=at(A * 4 - px + 1)),        # by one byte
           dict(st=at(A * 4 - 2 * 4 * 8 + 1)), dict(fn="fotg_fill_u8", d=at(A * 3 + px - 1)))
    for b in bad:
        assert call(**b) == FOTG_ERR_ARG, b
    # the last case overlaps hole only as far as a uint8 dst reaches: the float form of the same addresses is fine to refuse too
    assert call(d=at(A * 3 + px - 1)) == FOTG_ERR_ARG
    nb = C.c_longlong(0)
    for a in ((0, 8, 8, 1), (65536, 8, 8, 1), (1, 0, 8, 1), (1, 8, 16385, 1), (1, 8, 8, 0), (1, 8, 8, 4)):
        assert L.fotg_fill_scratch(*a, C.byref(nb)) == FOTG_ERR_ARG, a
    assert L.fotg_fill_scratch(1, 8, 8, 1, None) == FOTG_ERR_ARG


def scratch_formula(n, w, h, ch):
    """csrc/fill_levels.h restated: the bytes of one image's levels, and of a call"""
    al = lambda v, a: (v + a - 1) // a * a
    dim = lambda v, l: (v + (1 << l) - 1) >> l
    L = 0
    while dim(w, L) > 1 or dim(h, L) > 1:
        L += 1
    tw, th = dim(w, 6), dim(h, 6)
    at = 0
    for l in range(1, 6):
        at = al(at + (tw << (6 - l)) * (th << (6 - l)) * ch * 4, 16)
    at = al(at + tw * th * 4, 16)
    for l in range(6, max(L, 6) + 1):
        blocks = dim(w, l) * dim(h, l)
        for each in (ch * 8, 4, ch * 4):
            at = al(at + blocks * each, 16)
    per = al(at + 16, 256)
    return per * max(1, min(n, (1 << 30) // per))


def test_scratch_equals_the_formula():
    from flowonthego_amd.fill import scratch_bytes
    for n, w, h, ch in ((1, 1, 1, 1), (1, 64, 64, 3), (1, 65, 64, 2), (3, 150, 139, 3), (64, 1920, 1080, 3), (64, 1920, 1080, 1), (720, 1024, 1024, 3),
                        (65535, 3, 2, 3), (1, 16384, 16384, 3), (5, 16384, 16384, 1), (1, 16384, 1, 2), (10930, 256, 256, 3)):
        assert scratch_bytes(n, w, h, ch) == scratch_formula(n, w, h, ch), (n, w, h, ch)
    per = scratch_bytes(1, 1920, 1080, 1)
    assert 0.33 * 1920 * 1080 * 4 < per < 0.40 * 1920 * 1080 * 4                      # about a third of the float frame
    assert scratch_bytes(64, 1920, 1080, 3) <= 2 ** 30 and scratch_bytes(2, 16384, 16384, 3) == scratch_bytes(1, 16384, 16384, 3) > 2 ** 30


def test_level_geometry_driver_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fill_levels_drv")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "fill_levels_drv.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "fill_levels ok" in r.stdout, r.stdout


def test_cli_refuses_bad_arguments():
    cli_refuses("fill_holes", ([], ["a.npy"], ["a.npy", "b.npy", "c.npy"], ["a.txt", "b.npy"], ["a.npy", "b.txt"], ["a.png", "b.png"],
                               ["a.npy", "b.npy", "--hole"], ["a.npy", "b.npy", "--hole", "m.txt"], ["a.npy", "b.npy", "--code", "c.npy"],
                               ["a.npy", "b.npy", "--fg", "2,3"], ["a.npy", "b.npy", "--hole", "m.npy", "--fg", "8"],
                               ["a.npy", "b.npy", "--hole", "m.npy", "--fg", "1,x"], ["a.npy", "b.npy", "--hole", "m.npy", "--fg", ""],
                               ["a.npy", "b.npy", "--hole", "m.npy", "--fg", "-1"], ["a.npy", "b.npy", "--radius", "2"]))


def test_cli_refuses_bad_files(tmp_path):
    """one line "fill_holes: <message>" and return value 1, before the device is touched"""
    p = lambda n: str(tmp_path / n)
    np.save(p("ok.npy"), np.zeros((8, 8), np.float32))
    np.save(p("u8.npy"), np.zeros((8, 8, 3), np.uint8))
    np.save(p("stack.npy"), np.zeros((2, 8, 8, 3), np.float32))
    np.save(p("f64.npy"), np.zeros((8, 8), np.float64))
    np.save(p("ch4.npy"), np.zeros((8, 8, 4), np.float32))
    np.save(p("u8ch2.npy"), np.zeros((8, 8, 2), np.uint8))
    np.save(p("empty.npy"), np.zeros((0, 8), np.float32))
    np.save(p("m.npy"), np.zeros((8, 8), np.uint8))
    np.save(p("m9.npy"), np.zeros((9, 8), np.uint8))
    np.save(p("mf.npy"), np.zeros((8, 8), np.float32))
    open(p("junk.npy"), "wb").write(b"not an array")
    open(p("junk.png"), "wb").write(b"not a picture")
    open(p("junk.flo"), "wb").write(b"not a flow")
    open(p("short.png"), "wb").write(gray_png_bytes(np.zeros((8, 8), np.uint8), rows=4))
    o = p("o.npy")
    for args in ([p("missing.npy"), o], [p("missing.flo"), o], [p("stack.npy"), o], [p("f64.npy"), o], [p("ch4.npy"), o], [p("empty.npy"), o],
                 [p("junk.npy"), o], [p("junk.flo"), o], [p("u8.npy"), o], [p("u8ch2.npy"), o, "--hole", p("m.npy")],
                 [p("junk.png"), o, "--hole", p("m.npy")], [p("short.png"), o, "--hole", p("m.npy")],
                 [p("ok.npy"), o, "--hole", p("missing.npy")], [p("ok.npy"), o, "--hole", p("m9.npy")], [p("ok.npy"), o, "--hole", p("mf.npy")],
                 [p("ok.npy"), o, "--hole", p("junk.png")], [p("ok.npy"), p("o.flo")]):
        r = run_cli("fill_holes", args)
        assert r.returncode == 1 and r.stderr.startswith("fill_holes: ") and len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)
        assert not os.path.exists(o) and not os.path.exists(p("o.flo"))


def test_the_tool_imports_no_other_tool_and_ends_callable():
    src = open(os.path.join(ROOT, "flowonthego_amd", "fill_holes.py")).read()
    import flowonthego_amd as F
    for other in F.CLI_MODULES:
        assert "from .%s " % other not in src and not re.search(r"import %s\b" % other, src), other
    assert 'with refusing("fill_holes")' in src and "load_array(" in src and "load_mask_png(" in src and "load_flow(" in src and "to_device(" in src
    for copied in ("torch.from_numpy", "import zlib", "import struct"):
        assert copied not in src, copied
    assert src.index("callable_module(") > src.index("def main(")
    assert src.index("ap.error(") < src.index("import numpy")                     # the parser's checks come before numpy or torch load
