"""The frame warp's host side (no GPU needed): the C-ABI is declared and bound, examples/warp_frame.cpp compiles and links against
the C++ shim, the CLI refuses bad arguments, and the compiler's resource table lists every warp_kernel instantiation without a
private-memory segment.  With a GPU: the CLI writes the restatement's frame and prints its numbers."""
import os

import numpy as np
import pytest

import warp_ref as W
from host_checks import cli_refuses, entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_warp", "fotg_warp_u8", "fotg_upsample_crop_warp", "fotg_upsample_crop_warp_u8")


def test_entry_points_are_declared_bound_and_exported():
    F, _ = entry_points(NEW_SYMBOLS, "warp.h")
    assert callable(F.warp) and callable(F.upsample_crop_warp)


def test_warp_frame_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "warp_frame"))


def test_cli_argument_errors(tmp_path):
    cli_refuses("warp_frame", ([], ["a.npy"], ["a.npy", "b.npy", "c.flo"], ["a.npy", "b.npy", "c.flo", "d.png", "--fill", "x"],
                               ["a.npy", "b.npy", "c.flo", "d.png", "--occ"]))


def test_resource_table_lists_the_warp_kernels_without_scratch():
    names, table = resource_table()
    # Src x element type x channels, Itanium-mangled: warp_kernel<DenseSrc | UpsampleSrc, float | unsigned char, 1 | 3>
    for src in ("NS_8DenseSrcE", "NS_11UpsampleSrcE"):
        for t in ("f", "h"):
            for noc in (1, 3):
                hit = [n for n in names if "warp_kernelI%s%sLi%dE" % (src, t, noc) in n]
                assert len(hit) == 1, (src, t, noc)
                assert table[hit[0]] == 0, hit
    fold = [n for n in names if "warp_fold_kernel" in n]
    assert len(fold) == 1 and table[fold[0]] == 0


@pytest.mark.gpu
def test_cli_writes_the_frame_of_the_restatement(tmp_path):
    from flowonthego_amd.flo import write_flo
    from host_checks import read_png_rgb
    rng = np.random.default_rng(4)
    h, w = 23, 41
    f0 = rng.integers(0, 256, (h, w)).astype(np.uint8)
    f1 = rng.integers(0, 256, (h, w)).astype(np.uint8)
    flow = (rng.standard_normal((h, w, 2)) * 3).astype(np.float32)
    flow[0, 0] = (np.nan, 0)
    occ = (rng.random((h, w)) < 0.2).astype(np.uint8)
    a, b, c, m, out = (str(tmp_path / n) for n in ("f0.npy", "f1.npy", "fw.flo", "occ.npy", "out.png"))
    np.save(a, f0)
    np.save(b, f1)
    np.save(m, occ)
    write_flo(c, flow)
    r = run_cli("warp_frame", [a, b, c, out, "--occ", m, "--fill", "9"])
    assert r.returncode == 0, r.stderr
    dst, code, st = W.warp(f1, flow, ref=f0, occ=occ, fill_mode=1, fill=9.0)
    assert np.array_equal(read_png_rgb(out), np.repeat(dst[..., None], 3, axis=2))
    got = [float(t) for t in r.stdout.split()[1::2]]
    want = list(st[:4] / (h * w)) + [st[4] / st[0], st[5] / st[0]]
    assert np.allclose(got, want, atol=1e-4), (got, want)
