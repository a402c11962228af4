"""The motion layers' host side (no GPU needed): the C-ABI is declared and bound, examples/motion_layers.cpp compiles and links
against the C++ shim, the compiler's resource table lists exactly the expected instantiations of the layer kernels, each without a
private-memory segment, the arguments the entry points refuse are refused before the device is touched, the Python bindings refuse
theirs before any launch, and the command-line tool refuses bad arguments and files."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from host_checks import cli_refuses, entry_points, gray_png_bytes, resource_table

NEW_SYMBOLS = ("fotg_motion_layers", "fotg_upsample_crop_motion_layers")
FOTG_ERR_ARG = 1


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "layers.h")
    from flowonthego_amd import layers
    for name in ("upsample_crop_motion_layers", "layer_summary"):
        assert getattr(F, name) is getattr(layers, name) and callable(getattr(F, name))
    assert F.LAYER == layers.LAYER and len(F.LAYER) == 8 and F.LAYER_STATS == ("unassigned", "masked", "unknown", "live")
    assert (F.UNASSIGNED, F.MASKED, F.UNKNOWN) == (253, 254, 255)
    assert F.LAZY["layer_summary"] == ("layers", "layer_summary") and "motion_layers" in F.CLI_MODULES
    assert callable(F.motion_layers) and F.motion_layers.__name__ == "flowonthego_amd.motion_layers"      # the tool's module, callable
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.motion_layers) and callable(OFClass.upsample_crop_motion_layers)
    # the definition is written at the head of the kernels and in the public header; the C-ABI file sits on the shared scaffold
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "layers.hip.h")).read()
    for text in (head, hdr):
        assert "32 x 32" in text and "never displaces a value" in text and "253" in text and "live = fitted" in text
    assert '#include "motion.hip.h"' in head
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_layers.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_layers.hip" in mk and " layers.hip.h" in mk
    # the tool follows the rules test_host.py sets for the tools it lists
    tool = open(os.path.join(ROOT, "flowonthego_amd", "motion_layers.py")).read()
    assert "from ._cli import" in tool and 'with refusing("motion_layers")' in tool and "torch.from_numpy" not in tool
    assert tool.rstrip().endswith("sys.exit(main())") and "callable_module(__name__" in tool


def test_motion_layers_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "motion_layers")
    assert os.path.exists(exe)
    for args in ([], ["a.flo"], ["a.flo", "l.pgm", "0"], ["a.flo", "l.pgm", "9"], ["a.flo", "l.pgm", "3x"], ["a.flo", "l.pgm", "3", "projective"],
                 ["a.flo", "l.pgm", "3", "affine", "x"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_layer_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if "layers_" in n)
    # Itanium-mangled: layers_tile_kernel<DenseSrc | UpsampleSrc>, layers_pass_kernel<DenseSrc | UpsampleSrc, round | assign | final>,
    # layers_fold_kernel<12 | 4>, and the four plain kernels -- and nothing else
    srcs = ("NS_8DenseSrcE", "NS_11UpsampleSrcE")
    want = ["layers_tile_kernelI%sE" % s for s in srcs] + ["layers_pass_kernelI%sLi%dE" % (s, p) for s in srcs for p in (0, 1, 2)]
    want += ["layers_fold_kernelILi12E", "layers_fold_kernelILi4E", "layers_select_kernelE", "layers_init_kernelE", "layers_solve_kernelE",
             "layers_records_kernelE"]
    assert len(mine) == len(want), mine
    for frag in want:
        hit = [n for n in mine if frag in n]
        assert len(hit) == 1, (frag, mine)
        assert table[hit[0]] == 0, hit
    # the names stay clear of the substrings by which the other resource-table tests count their kernels
    for n in mine:
        assert not any(s in n for s in ("motion_", "comp_", "obj", "warp_", "flowfilter_", "temporal_", "blockmv_", "mh_kernel", "mblur_", "plate_")), n
    # the fit's kernels are still compiled once, although layers.hip.h includes motion.hip.h
    assert sum("motion_solve_kernel" in n for n in names) == 1 and sum("motion_flow_kernel" in n for n in names) == 1
    assert sum("motion_fold_kernel" in n for n in names) == 2 and sum("motion_pass_kernel" in n for n in names) == 6
    assert all(b == 0 for b in table.values())
    # the assign pass forms its per-pixel products inside the layer loop (an optimiser fence in layers.hip.h keeps them there):
    # hoisted out they cost 88 registers, 180 VGPRs in all and 2 waves per SIMD instead of 110 and 4
    txt = open(os.path.join(ROOT, "flowonthego_amd", "libfotg.resusage.txt")).read()
    for src in srcs:
        for mode, ceiling in ((0, 96), (1, 128), (2, 96)):
            m = re.search(r"Function Name: \S*layers_pass_kernelI%sLi%dE\S*.*?\bVGPRs: (\d+)" % (src, mode), txt, re.S)
            assert m and int(m.group(1)) <= ceiling, (src, mode, m and m.group(1))


def test_arguments_are_refused_before_the_device_is_touched():
    """every pointer is a host address that is never dereferenced: FOTG_ERR_ARG is decided first"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps

    def call(n=1, f=far(1), m=None, w=8, h=8, K=3, model=2, iters=3, rounds=3, th=1.0, init=None, p=far(2), lab=far(3), res=far(4),
             rec=far(5), st=far(6), sm=far(7)):
        return L.fotg_motion_layers(0, n, f, m, w, h, K, model, iters, rounds, C.c_float(th), init, p, lab, res, rec, st, sm, None)

    for bad in (dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=0), dict(w=-3), dict(w=16385), dict(h=16385), dict(K=0), dict(K=9),
                dict(K=-1), dict(model=-1), dict(model=3), dict(iters=-1), dict(iters=65), dict(rounds=-1), dict(rounds=65), dict(th=-1.0),
                dict(th=float("nan")), dict(f=None), dict(p=None),
                # an output on an input
                dict(p=far(1)), dict(lab=far(1)), dict(res=far(1)), dict(rec=far(1)), dict(st=far(1)), dict(sm=far(1)),
                dict(m=far(2)), dict(m=far(3)), dict(m=far(4)), dict(m=far(7)), dict(init=far(2)), dict(init=far(5)), dict(init=far(6)),
                # an output on another output
                dict(lab=far(2)), dict(res=far(3)), dict(rec=far(4)), dict(st=far(5)), dict(sm=far(6)), dict(sm=far(2))):
        assert call(**bad) == FOTG_ERR_ARG, bad
    # the flow's end runs into the params: 8 x 8 x 2 floats are 512 bytes
    assert call(p=C.c_void_p(0x20000000 + 511)) == FOTG_ERR_ARG
    fused = lambda ctx, n, f: L.fotg_upsample_crop_motion_layers(ctx, n, f, None, 3, 2, 3, 3, C.c_float(1.0), None, far(1), None, None, None, None,
                                                                None, None)
    assert fused(None, 1, far(0)) == FOTG_ERR_ARG


def test_python_refusals_are_raised_before_any_launch():
    """what the bindings refuse needs no device: a host tensor is refused at the first check, bad settings before the tensors"""
    import torch
    import flowonthego_amd as F
    from flowonthego_amd.layers import layer_summary, motion_layers
    flow = torch.zeros((2, 5, 7, 2))
    for bad in (lambda: motion_layers(flow), lambda: motion_layers(flow[..., :1]), lambda: motion_layers(flow[0, 0]), lambda: motion_layers(None),
                lambda: motion_layers(torch.zeros((1, 0, 7, 2))), lambda: layer_summary(torch.zeros((2, 3, 7)), 7, 5), lambda: layer_summary(None, 7, 5)):
        with pytest.raises(F.FotgError):
            bad()
    from flowonthego_amd.layers import _layer_args
    for bad in (dict(layers=0), dict(layers=9), dict(layers=2.0), dict(layers=True), dict(iters=-1), dict(iters=65), dict(rounds=-1),
                dict(rounds=65), dict(rounds=1.5), dict(thresh=-0.5), dict(thresh=float("nan"))):
        with pytest.raises(F.FotgError):
            _layer_args(**dict(dict(layers=3, iters=3, rounds=3, thresh=1.0), **bad))
    _layer_args(8, 64, 64, 0.0)
    s = layer_summary(torch.tensor([[10, 10, 1, 1, 3, -20, 40, 2560], [0, 0, 0, 0, -1, 0, 0, 0]]), 7, 5)
    assert s[0].tolist() == [2.0, 4.0, 1.0] and bool(torch.isnan(s[1]).all())


def test_cli_argument_and_file_errors(tmp_path, capsys):
    cli_refuses("motion_layers", ([], ["a.flo"], ["a.flo", "o.png", "x.png"], ["a.flo", "o.png", "--layers", "0"], ["a.flo", "o.png", "--layers", "9"],
                                  ["a.flo", "o.png", "--iters", "-1"], ["a.flo", "o.png", "--rounds", "65"], ["a.flo", "o.png", "--thresh", "-2"],
                                  ["a.flo", "o.png", "--thresh", "nan"], ["a.flo", "o.png", "--mask"], ["a.flo", "o.png", "--model", "projective"]))
    # the files it cannot use, in this process (the tool's main): one line "motion_layers: ..." naming the file, return value 1
    from flowonthego_amd.flo import write_flo
    from flowonthego_amd.motion_layers import main
    fl, out, notflo, mk = (str(tmp_path / n) for n in ("f.flo", "o.png", "n.flo", "m.png"))
    write_flo(fl, np.zeros((6, 9, 2), np.float32))
    open(notflo, "wb").write(b"PIEX" + b"\0" * 20)
    open(mk, "wb").write(gray_png_bytes(np.zeros((6, 8), np.uint8)))
    for args, word in (([str(tmp_path / "missing.flo"), out], "missing.flo"), ([notflo, out], "n.flo"), ([fl, out, "--mask", mk], "m.png"),
                       ([fl, out, "--mask", str(tmp_path / "none.png")], "none.png")):
        assert main(args) == 1, args
        err = capsys.readouterr().err
        assert err.startswith("motion_layers: ") and word in err and len(err.splitlines()) == 1, (args, err)
        assert not os.path.exists(out)
