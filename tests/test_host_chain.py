"""Flow chaining's host side (no GPU needed): the C-ABI is declared and bound, examples/chain_flow.cpp compiles and links against
the C++ shim, the CLI refuses bad arguments, and the compiler's resource table lists every chain kernel instantiation without a
private-memory segment."""
import os

from conftest import ROOT
from host_checks import cli_refuses, entry_points, resource_table

NEW_SYMBOLS = ("fotg_flow_chain", "fotg_track_points", "fotg_upsample_crop_flow_chain", "fotg_upsample_crop_track_points")


def test_entry_points_are_declared_bound_and_exported():
    F, _ = entry_points(NEW_SYMBOLS, "chain.h")
    for name in ("chain", "track_points", "upsample_crop_chain", "upsample_crop_track_points"):
        assert callable(getattr(F, name)), name
    from flowonthego_amd.oflow import OFClass
    for name in ("upsample_crop_chain", "upsample_crop_track_points", "track"):
        assert callable(getattr(OFClass, name)), name


def test_chain_flow_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "chain_flow"))


def test_cli_argument_errors(tmp_path):
    cli_refuses("chain_flow", ([], ["a.flo"], ["a.flo", "b.flo", "out.flo", "--bw", "c.flo"], ["a.flo", "out.flo", "--bw"],
                               ["a.flo", "out.flo", "--points", "p.npy"], ["a.flo", "out.flo", "--frames", "3"]))


def test_resource_table_lists_the_chain_kernels_without_scratch():
    names, table = resource_table()
    # kernel x Src x with / without backward flows, Itanium-mangled: chain_dense_kernel<DenseSrc | UpsampleSrc, false | true>
    for kernel in ("chain_dense_kernel", "chain_points_kernel"):
        for src in ("NS_8DenseSrcE", "NS_11UpsampleSrcE"):
            for bw in (0, 1):
                hit = [n for n in names if "%sI%sLb%dE" % (kernel, src, bw) in n]
                assert len(hit) == 1, (kernel, src, bw)
                assert table[hit[0]] == 0, hit
