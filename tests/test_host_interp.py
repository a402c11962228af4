"""The frame interpolation's host side (no GPU needed): the C-ABI is declared and bound, examples/interp_frame.cpp compiles and
links against the C++ shim, the CLI refuses bad arguments, the argument checks that precede any GPU work answer without one, and
the compiler's resource table lists every interpolation kernel without a private-memory segment.  With a GPU: the CLI writes the
restatement's frame."""
import ctypes as C
import os

import numpy as np
import pytest

import interp_ref as I
from host_checks import cli_refuses, entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_interp", "fotg_interp_u8", "fotg_upsample_crop_interp", "fotg_upsample_crop_interp_u8")
FOTG_ERR_ARG = 1


def test_entry_points_are_declared_bound_and_exported():
    F, _ = entry_points(NEW_SYMBOLS, "interp.h")
    assert callable(F.interpolate) and callable(F.upsample_crop_interpolate)
    from flowonthego_amd.oflow import OFClass
    assert all(hasattr(OFClass, m) for m in ("interpolate", "upsample_crop_interpolate", "bidirectional_flows"))


def test_argument_checks_answer_before_any_gpu_work():
    """every refusal below is decided before the device is touched; the pointers are never dereferenced"""
    import flowonthego_amd as F
    L = F.lib()
    buf = (C.c_char * 64)()
    q = C.cast(buf, C.c_void_p)
    call = lambda n=1, a=q, b=q, f=q, g=q, w=2, h=2, ch=1, t=0.5, mf=q, mb=q, d=None, c=q: L.fotg_interp(
        0, n, a, b, f, g, w, h, ch, C.c_float(t), mf, mb, C.c_float(0.01), C.c_float(0.5), None, d, c, None, None)
    for bad in (dict(n=0), dict(n=70000), dict(a=None), dict(b=None), dict(f=None), dict(g=None), dict(w=0), dict(h=-1), dict(ch=2),
                dict(ch=4), dict(t=0.0), dict(t=1.0), dict(t=-1.0), dict(t=float("nan")), dict(t=float("inf")), dict(mf=None),
                dict(mb=None), dict(c=None), dict(d=q), dict(w=65536, h=65536)):
        assert call(**bad) == FOTG_ERR_ARG, bad
    assert L.fotg_interp_u8(0, 1, None, q, q, q, 2, 2, 1, C.c_float(0.5), None, None, C.c_float(0.01), C.c_float(0.5), None, None, q,
                            None, None) == FOTG_ERR_ARG
    for fn in (L.fotg_upsample_crop_interp, L.fotg_upsample_crop_interp_u8):
        assert fn(None, 1, q, q, q, q, 1, C.c_float(0.5), None, None, C.c_float(0.01), C.c_float(0.5), None, None, q, None,
                  None) == FOTG_ERR_ARG


def test_interp_frame_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "interp_frame"))


def test_cli_argument_errors():
    cli_refuses("interp_frame", ([], ["a.npy"], ["a.npy", "b.npy", "0.5"], ["a.npy", "b.npy", "x", "d.png"], ["a.npy", "b.npy", "1.0", "d.png"],
                                 ["a.npy", "b.npy", "0", "d.png"], ["a.npy", "b.npy", "0.5", "d.png", "--ref"]))


def test_resource_table_lists_the_interpolation_kernels_without_scratch():
    names, table = resource_table()
    for kernel in ("23interp_candidate_kernel", "21interp_resolve_kernel"):
        for src in ("NS_8DenseSrcE", "NS_11UpsampleSrcE"):
            for t in ("f", "h"):
                for noc in (1, 3):
                    hit = [n for n in names if "%sI%s%sLi%dE" % (kernel, src, t, noc) in n]
                    assert len(hit) == 1, (kernel, src, t, noc)
                    assert table[hit[0]] == 0, hit
    # the fold kernel of the statistics is shared with the warp, not compiled a second time
    assert len([n for n in names if "warp_fold_kernel" in n]) == 1


@pytest.mark.gpu
def test_cli_writes_the_frame_of_the_restatement(tmp_path, alley):
    from oracle import oracle as O
    from host_checks import read_png_rgb
    f0, f1 = alley["frame_0001"][100:292, 300:620].copy(), alley["frame_0002"][100:292, 300:620].copy()
    a, b, out = (str(tmp_path / n) for n in ("f0.npy", "f1.npy", "out.png"))
    np.save(a, f0)
    np.save(b, f1)
    r = run_cli("interp_frame", [a, b, "0.25", out, "--ref", b])
    assert r.returncode == 0, r.stderr
    g0, g1 = f0.astype(np.float32), f1.astype(np.float32)
    dst, code, st = I.interp(f0, f1, O.full_flow(g0, g1), O.full_flow(g1, g0), 0.25, ref=f1)
    assert np.array_equal(read_png_rgb(out), np.repeat(dst[..., None], 3, axis=2))
    got = [float(t) for t in r.stdout.split()[1::2]]
    want = list(st[:4] / f0.size) + [st[4] / f0.size, st[5] / f0.size]
    assert np.allclose(got, want, atol=1e-4), (got, want)
