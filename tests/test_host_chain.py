"""Flow chaining's host side (no GPU needed): the C-ABI is declared and bound, examples/chain_flow.cpp compiles and links against
the C++ shim, the CLI refuses bad arguments, and the compiler's resource table lists every chain kernel instantiation without a
private-memory segment.  With a GPU: the CLI writes what the calls return."""
import os

import pytest

from conftest import ROOT
from host_checks import cli_refuses, entry_points, resource_table, run_cli

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


@pytest.mark.gpu
def test_cli_writes_what_the_calls_return(tmp_path):
    import numpy as np
    import torch
    import flowonthego_amd as F
    from flowonthego_amd.chain import STATS
    from flowonthego_amd.flo import write_flo
    rng = np.random.default_rng(21)
    h, w = 17, 29
    fw = (rng.standard_normal((2, h, w, 2)) * 2).astype(np.float32)
    bw = (-fw + 0.3 * rng.standard_normal((2, h, w, 2))).astype(np.float32)
    pts = np.array([(3.5, 4.25), (20.0, 9.0), (-2.0, 5.0)], np.float32)            # the last one starts outside the frame
    f0, f1, b0, b1, out, want, pf, tr = (str(tmp_path / n) for n in ("f0.flo", "f1.flo", "b0.flo", "b1.flo", "out.flo", "want.flo", "pts.npy",
                                                                     "traj.npy"))
    for path, f in ((f0, fw[0]), (f1, fw[1]), (b0, bw[0]), (b1, bw[1])):
        write_flo(path, f)
    np.save(pf, pts)
    run = run_cli("chain_flow", [f0, f1, out, "--bw", b0, b1, "--points", pf, tr])
    assert run.returncode == 0, run.stderr
    Fd, Bd = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    total, _, _, st = F.chain(Fd, Bd, stats=True)
    traj, code, _ = F.track_points(torch.from_numpy(pts).cuda(), Fd, Bd)
    write_flo(want, total.cpu().numpy())
    assert open(out, "rb").read() == open(want, "rb").read()
    got = np.load(tr)
    assert got.shape == (3, 3, 2) and got.dtype == np.float32 and got.tobytes() == traj.cpu().numpy().tobytes()
    assert int(code[2]) == 2 and np.array_equal(got[:, 2], np.tile(pts[2], (3, 1)))
    st = st.cpu().numpy()
    assert run.stdout == "  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(STATS[:4], st[:4])) + "  mean_steps %.4f\n" % (st[4] / (h * w))
