"""The binary morphology's host side (no GPU needed): the C-ABI is declared and bound, examples/clean_mask.cpp compiles and links
against the C++ shim, the definition stands word for word in the kernel's header and in the public one, the compiler's resource
table lists exactly one morph_kernel, without a private-memory segment and without adding to any other feature's kernels, the
arguments the entry point refuses are refused before the device is touched, and the tool refuses bad arguments and bad files."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from host_checks import cli_refuses, entry_points, gray_png_bytes, resource_table, run_cli

NEW_SYMBOLS = ("fotg_morph",)
FOTG_ERR_ARG = 1
# the substrings by which the resource-table tests of the other features count their kernels
OTHERS = ("erase", "subtract_", "plate_", "layers_", "motion_", "comp_", "obj", "warp_", "flowfilter_", "temporal_", "blockmv_", "mh_kernel",
          "mblur_", "interp")


def _definition(text, prefix):
    """the lines of the definition, from "n maps of" to the sentence on stats, without the comment prefix"""
    lines = text.splitlines()
    a = next(i for i, ln in enumerate(lines) if ln.startswith(prefix + "n maps of w x h bytes, 1 <= w, h <= 16384, n <= 65535."))
    b = next(i for i, ln in enumerate(lines) if i > a and "accumulated by integer atomics: the same bytes every run." in ln)
    assert all(ln.startswith(prefix) for ln in lines[a:b + 1])
    return [ln[len(prefix):] for ln in lines[a:b + 1]]


def test_entry_point_is_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "morph.h")
    from flowonthego_amd import morph
    assert F.morphology is morph.morphology and F.LAZY["morphology"] == ("morph", "morphology")
    assert "clean_mask" not in F.LAZY and callable(morph.clean_mask)              # the package's name for it is the callable tool module
    assert callable(F.clean_mask) and F.clean_mask.__name__ == "flowonthego_amd.clean_mask" and F.CLI_MODULES.count("clean_mask") == 1
    assert callable(morph.chain) and len(morph.STATS) == 4 and morph.OPS == ("erode", "dilate", "open", "close")
    assert str(inspect.signature(morph.morphology)) == "(mask, op, radius, fg=None, stats=False)"
    assert str(inspect.signature(morph.clean_mask)) == "(mask, open=1, close=2, fg=None, stats=False)"
    # the pipeline: trailing keywords whose defaults change nothing; OFClass.remove_objects keeps its signature
    from flowonthego_amd import erase, subtract
    from flowonthego_amd.oflow import OFClass
    for fn in (subtract.foreground_objects, subtract.ofc_foreground, subtract._ofc_foreground, OFClass.foreground, erase.ofc_remove_objects):
        assert str(inspect.signature(fn)).endswith(", open=0, close=0)"), fn
    assert str(inspect.signature(subtract.foreground_objects)) == "(code, evidence, connectivity=8, min_area=64, max_objects=256, open=0, close=0)"
    assert "open" not in inspect.signature(OFClass.remove_objects).parameters
    # the definition is written at the head of the kernel and in the public header, word for word the same
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "morph.hip.h")).read()
    mine, public = _definition(head, "// "), _definition(hdr, " * ")
    assert mine == public and len(mine) >= 14
    for text in (head, hdr):
        for expr in ("dx^2 + dy^2 <= r^2", "r an integer in 0 .. 8", "b < 8 && ((fg_codes >> b) & 1)", "fg_codes == 0 every non-zero byte",
                     "some pixel of the frame within the disc", "every pixel of the frame within the disc", "the frame border does not erode",
                     "erode(X, r) = not dilate(not X, r)", "r = 0 is the identity", "open(X, r) = dilate(erode(X, r), r)",
                     "close(X, r) = erode(dilate(X, r), r)", "n x 4 int64"):
            assert expr in text, expr
    assert "overlap_any" in hdr and "overlap_among" in hdr
    body = head.split("#pragma once")[1]
    for used in ("__ballot(", "__syncthreads", "__popc(", "atomicAdd(stats", "__builtin_nontemporal_store", "__shfl_xor("):
        assert used in body, used
    for absent in ("float", "double", "erase.hip.h", "sqrt"):                     # integers only, and no distance transform
        assert absent not in body, absent
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_morph.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi
    assert "overlap_any(" in capi and "overlap_among(" in capi and "hipMemsetAsync(stats" in capi and capi.count("<<<") == 1
    for sync in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc(", "hipEventSynchronize"):
        assert sync not in capi, sync
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_morph.hip" in mk and " morph.hip.h" in mk


def test_clean_mask_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "clean_mask")
    assert os.path.exists(exe)
    ok = ["m.raw", "8", "8", "2", "o.raw"]
    for args in ([], ["m.raw"], ok[:4], ["m.raw", "0", "8", "2", "o.raw"], ["m.raw", "8", "-1", "2", "o.raw"], ["m.raw", "8", "16385", "2", "o.raw"],
                 ["m.raw", "8", "8", "0", "o.raw"], ["m.raw", "8", "8", "65536", "o.raw"], ok + ["-1"], ok + ["9"], ok + ["1", "-1"], ok + ["1", "9"],
                 ok + ["1", "2", "x"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_morph_kernel_without_scratch():
    names, table = resource_table()
    mine = [n for n in names if "morph" in n]
    assert len(mine) == 1 and "morph_kernel" in mine[0] and table[mine[0]] == 0, mine     # one kernel, no template: every chain is its argument
    assert not any(s in mine[0] for s in OTHERS), mine
    # what the other features' tests count is what it was
    count = lambda s: sum(s in n for n in names)
    assert count("erase") == 12 and count("subtract_") == 12 and count("plate_kernel") == 12 and count("warp_fold_kernel") == 1
    assert len(names) - 1 == len([n for n in names if "morph" not in n])
    # every kernel of the library is still free of private memory
    assert not [n for n in names if table[n]]


def test_arguments_are_refused_before_the_device_is_touched():
    """src, out and stats are host addresses that are never dereferenced: FOTG_ERR_ARG is decided first (ops and radii are read, so
    they are real)"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)

    def call(n=2, s=far(1), w=8, h=8, fg=0, ns=2, ops=(0, 1), radii=(1, 1), o=far(2), st=None):
        return L.fotg_morph(0, n, s, w, h, fg, ns, ints(ops), ints(radii), o, st, None)

    bad = (dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=0), dict(w=-3), dict(w=16385), dict(h=16385), dict(s=None),
           dict(fg=-1), dict(fg=256), dict(ns=0), dict(ns=3), dict(ns=-1), dict(ops=None), dict(radii=None),
           dict(ops=(2, 1)), dict(ops=(0, -1)), dict(ops=(0, 2)), dict(radii=(9, 0)), dict(radii=(0, 9)), dict(radii=(-1, 0)), dict(radii=(1, 1 << 30)),
           dict(ns=1, ops=(3,), radii=(1,)), dict(ns=1, ops=(1,), radii=(9,)),
           dict(o=None), dict(o=far(1)), dict(o=None, st=far(1)), dict(st=far(2)),           # no output; an output on src; the outputs on each other
           dict(o=C.c_void_p(0x10000000 * 2 + 2 * 8 * 8 - 1)), dict(o=C.c_void_p(0x10000000 * 2 - 2 * 8 * 8 + 1)),      # src's last byte, out's last
           dict(st=C.c_void_p(0x10000000 * 2 - 2 * 4 * 8 + 1)))
    for b in bad:
        assert call(**b) == FOTG_ERR_ARG, b


def test_cli_refuses_bad_arguments():
    cli_refuses("clean_mask", ([], ["a.npy"], ["a.npy", "b.png", "c"], ["a.npy", "b.png", "--open", "9"], ["a.npy", "b.png", "--open", "-1"],
                               ["a.npy", "b.png", "--close", "9"], ["a.npy", "b.png", "--close", "1.5"], ["a.npy", "b.png", "--close"],
                               ["a.npy", "b.png", "--fg", "8"], ["a.npy", "b.png", "--fg", "1,x"], ["a.npy", "b.png", "--fg", ""],
                               ["a.npy", "b.png", "--fg", "-1"], ["a.npy", "b.png", "--op", "open"], ["a.npy", "b.png", "--radius", "2"],
                               ["a.npy", "b.png", "--op", "grow", "--radius", "2"], ["a.npy", "b.png", "--op", "open", "--radius", "9"],
                               ["a.npy", "b.png", "--op", "open", "--radius", "1", "--open", "1"]))
    for tool in ("foreground", "remove_objects"):
        cli_refuses(tool, (["a.npy", "b.npy", "--open", "9"], ["a.npy", "b.npy", "--open", "-1"], ["a.npy", "b.npy", "--close", "9"],
                           ["a.npy", "b.npy", "--close", "x"], ["a.npy", "b.npy", "--close"]))


def test_cli_refuses_bad_files(tmp_path):
    """one line "clean_mask: <message>" and return value 1, before the device is touched"""
    p = lambda n: str(tmp_path / n)
    np.save(p("stack.npy"), np.zeros((2, 8, 8), np.uint8))
    np.save(p("f32.npy"), np.zeros((8, 8), np.float32))
    np.save(p("empty.npy"), np.zeros((0, 8), np.uint8))
    open(p("junk.npy"), "wb").write(b"not an array")
    open(p("junk.png"), "wb").write(b"not a picture")
    open(p("short.png"), "wb").write(gray_png_bytes(np.zeros((8, 8), np.uint8), rows=4))
    for args in ([p("missing.npy"), p("o.png")], [p("missing.png"), p("o.png")], [p("stack.npy"), p("o.png")], [p("f32.npy"), p("o.png")],
                 [p("empty.npy"), p("o.png")], [p("junk.npy"), p("o.png")], [p("junk.png"), p("o.png")], [p("short.png"), p("o.png")]):
        r = run_cli("clean_mask", args)
        assert r.returncode == 1 and r.stderr.startswith("clean_mask: ") and len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)
        assert not os.path.exists(p("o.png"))


def test_the_tool_imports_no_other_tool_and_ends_callable():
    src = open(os.path.join(ROOT, "flowonthego_amd", "clean_mask.py")).read()
    import flowonthego_amd as F
    for other in F.CLI_MODULES:
        assert "from .%s " % other not in src and not re.search(r"import %s\b" % other, src), other
    assert 'with refusing("clean_mask")' in src and "load_array(" in src and "load_mask_png(" in src and "to_device(" in src
    for copied in ("torch.from_numpy", "import zlib", "import struct"):
        assert copied not in src, copied
    assert src.index("callable_module(") > src.index("def main(")
    assert src.index("ap.error(") < src.index("import numpy")                     # the parser's checks come before numpy or torch load
