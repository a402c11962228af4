"""Flow chaining's host side (no GPU needed): the C-ABI is declared and bound, examples/chain_flow.cpp compiles and links against
the C++ shim, the CLI refuses bad arguments, and the compiler's resource table lists every chain kernel instantiation without a
private-memory segment."""
import os
import re
import subprocess
import sys

from conftest import ROOT

NEW_SYMBOLS = ("fotg_flow_chain", "fotg_track_points", "fotg_upsample_crop_flow_chain", "fotg_upsample_crop_track_points")


def test_entry_points_are_declared_bound_and_exported():
    import flowonthego_amd as F
    from flowonthego_amd._lib import SYMBOLS
    L = F.lib()
    hdr = open(os.path.join(ROOT, "include", "fotg.h")).read()
    bound = {s[0]: s for s in SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound and hasattr(L, name)
    # one ctypes argument per parameter of the declaration
    for name in NEW_SYMBOLS:
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(bound[name][2]), name
    shim = open(os.path.join(ROOT, "include", "fotg", "chain.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in shim
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
    env = dict(os.environ, PYTHONPATH=ROOT)
    for args in ([], ["a.flo"], ["a.flo", "b.flo", "out.flo", "--bw", "c.flo"], ["a.flo", "out.flo", "--bw"],
                 ["a.flo", "out.flo", "--points", "p.npy"], ["a.flo", "out.flo", "--frames", "3"]):
        r = subprocess.run([sys.executable, "-m", "flowonthego_amd.chain_flow"] + args, capture_output=True, text=True, cwd=ROOT, env=env)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_resource_table_lists_the_chain_kernels_without_scratch():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "flowonthego_amd", "csrc")], stdout=subprocess.DEVNULL)
    txt = open(os.path.join(ROOT, "flowonthego_amd", "libfotg.resusage.txt")).read()
    names = re.findall(r"Function Name: (\S+)", txt)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(names) == len(scratch)
    table = dict(zip(names, scratch))
    # kernel x Src x with / without backward flows, Itanium-mangled: chain_dense_kernel<DenseSrc | UpsampleSrc, false | true>
    for kernel in ("chain_dense_kernel", "chain_points_kernel"):
        for src in ("NS_8DenseSrcE", "NS_11UpsampleSrcE"):
            for bw in (0, 1):
                hit = [n for n in names if "%sI%sLb%dE" % (kernel, src, bw) in n]
                assert len(hit) == 1, (kernel, src, bw)
                assert table[hit[0]] == 0, hit
