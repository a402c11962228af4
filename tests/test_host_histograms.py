"""The motion histograms' host side (no GPU needed): the C-ABI is declared and bound, examples/motion_histograms.cpp compiles and
links against the C++ shim, the compiler's resource table lists exactly the two instantiations of the histogram kernel, both
without a private-memory segment, and the arguments the entry points refuse are refused before the device is touched.  With a GPU:
the CLI writes what the calls return."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from host_checks import entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_motion_histograms", "fotg_upsample_crop_motion_histograms")
FOTG_ERR_ARG = 1


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "histograms.h")
    from flowonthego_amd import histograms
    for name in ("upsample_crop_motion_histograms", "motion_descriptors"):
        assert getattr(F, name) is getattr(histograms, name) and callable(getattr(F, name))
    assert F.HIST == histograms.HIST and len(F.HIST) == 32 and len(set(F.HIST)) == 32
    assert callable(F.motion_histograms) and F.motion_histograms.__name__ == "flowonthego_amd.motion_histograms"   # the tool's module, callable
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.motion_histograms) and callable(OFClass.upsample_crop_motion_histograms)
    # the definition is written at the head of the kernel and in the public header; both C-ABI files sit on the shared scaffold
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "histograms.hip.h")).read()
    for text in (head, hdr):
        assert "(b0 + 1) & 7" in text and "1024 + phi" in text and "thresh256" in text
    capi = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "fotg_histograms.hip")).read()
    assert '#include "host_call.h"' in capi and "struct DevGuard" not in capi and "struct Span" not in capi
    mk = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "Makefile")).read()
    assert "fotg_histograms.hip" in mk and " histograms.hip.h" in mk


def test_motion_histograms_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "motion_histograms")
    assert os.path.exists(exe)
    for args in ([], ["a.flo", "12"], ["a.flo", "16", "x"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_histogram_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if "mh_kernel" in n)
    # Itanium-mangled: mh_kernel<DenseSrc | UpsampleSrc> -- and nothing else
    want = ["mh_kernelINS_8DenseSrcEEE", "mh_kernelINS_11UpsampleSrcEEE"]
    assert len(mine) == len(want), mine
    for frag in want:
        hit = [n for n in mine if frag in n]
        assert len(hit) == 1, (frag, mine)
        assert table[hit[0]] == 0, hit
    # the names stay clear of the substrings by which the other resource-table tests count their kernels
    for n in mine:
        assert not any(s in n for s in ("motion_", "comp_", "obj", "warp_fold_kernel", "flowfilter_fold_kernel", "temporal_fold_kernel")), n
    # the motion model moved to a header of its own: the fit's kernels are still compiled once
    assert sum("motion_solve_kernel" in n for n in names) == 1 and sum("motion_flow_kernel" in n for n in names) == 1


def test_arguments_are_refused_before_the_device_is_touched():
    """every pointer is a host address that is never dereferenced: FOTG_ERR_ARG is decided first"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps

    def call(n=1, f=far(1), w=8, h=8, m=None, p=None, cell=8, t=102, c=far(2), i=far(3), rows=4, o=far(4)):
        return L.fotg_motion_histograms(0, n, f, w, h, m, p, cell, t, c, i, rows, o, None)

    for bad in (dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=0), dict(w=16385), dict(h=16385), dict(f=None), dict(cell=0), dict(cell=4),
                dict(cell=24), dict(cell=64), dict(t=-1), dict(c=None, o=None), dict(i=None), dict(rows=0), dict(rows=-5), dict(rows=1025),
                dict(c=far(1)), dict(o=far(1)), dict(c=far(3)), dict(o=far(3)), dict(m=far(2)), dict(m=far(4)), dict(p=far(2)), dict(p=far(4)),
                dict(o=far(2))):
        assert call(**bad) == FOTG_ERR_ARG, bad
    assert L.fotg_upsample_crop_motion_histograms(None, 1, far(0), None, None, 8, 102, far(1), None, 4, None, None) == FOTG_ERR_ARG


@pytest.mark.gpu
def test_cli_writes_what_the_call_returns(tmp_path):
    import numpy as np
    import torch
    import flowonthego_amd as F
    import histograms_ref as R
    from flowonthego_amd.flo import write_flo
    rng = np.random.default_rng(9)
    h, w = 37, 70
    ys, xs = np.mgrid[0:h, 0:w]
    flow = np.stack([0.01 * xs + 1.5, -0.02 * ys + 0.25], -1) + 0.3 * rng.standard_normal((h, w, 2))
    flow = flow.astype(np.float32)
    ids = (xs // 24 - 1).astype(np.int32)
    fl, out, idf = (str(tmp_path / n) for n in ("f.flo", "out.npz", "ids.npy"))
    write_flo(fl, flow)
    np.save(idf, ids)
    run = run_cli("motion_histograms", [fl, out, "--cell", "8", "--thresh", "0.5", "--model", "affine",
                          "--ids", idf, "--rows", "3"])
    assert run.returncode == 0, run.stderr
    dflow = torch.from_numpy(flow).cuda()
    params = F.fit_motion(dflow, None, "affine")
    cells, objs = F.motion_histograms(dflow, None, params, 8, 0.5, torch.from_numpy(ids).cuda(), 3)
    z = np.load(out)
    assert sorted(z.files) == ["cells", "descriptors", "objects", "params"]
    assert np.array_equal(z["cells"], cells.cpu().numpy()) and np.array_equal(z["objects"], objs.cpu().numpy())
    assert np.array_equal(z["params"], params.cpu().numpy()) and z["descriptors"].shape == cells.shape[:-1] + (25,)
    wc, wo = R.histograms(flow[None], None, params.cpu().numpy()[None], 8, 128, ids[None], 3)
    assert np.array_equal(z["cells"], wc[0]) and np.array_equal(z["objects"], wo[0])
    tot = wc[0].reshape(-1, 32).sum(0)
    lines = run.stdout.splitlines()
    assert lines[0] == "HOF " + " ".join("%d" % v for v in tot[:8]) and lines[1].startswith("zero bin %d of %d admissible" % (tot[8], tot[25]))
