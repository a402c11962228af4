"""The flow filter's host side (no GPU needed): the C-ABI is declared and bound, examples/filter_flow.cpp compiles and links against
the C++ shim, the CLI refuses bad arguments, and the compiler's resource table lists every flowfilter_kernel instantiation without a
private-memory segment.  With a GPU: the CLI writes what filter_flow returns and prints its numbers."""
import os
import re

import numpy as np
import pytest

from host_checks import cli_refuses, entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_flow_filter", "fotg_flow_filter_u8", "fotg_upsample_crop_flow_filter", "fotg_upsample_crop_flow_filter_u8")


def test_entry_points_are_declared_bound_and_exported():
    F, _ = entry_points(NEW_SYMBOLS, "flowfilter.h")
    assert callable(F.filter_flow) and callable(F.upsample_crop_filter_flow) and callable(F.spatial_table)
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.calc_filtered) and callable(OFClass.upsample_crop_filter_flow)


def test_spatial_table_is_the_gaussian_rounded_to_f32():
    import math
    import flowonthego_amd as F
    t = F.spatial_table(3, 1.5)
    assert t == [float(np.float32(math.exp(-(i * i) / 4.5))) for i in range(4)] and t[0] == 1.0
    for bad in ((0, 1.0), (8, 1.0), (3, 0.0), (3, float("nan"))):
        with pytest.raises(F.FotgError):
            F.spatial_table(*bad)


def test_filter_flow_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "filter_flow"))


def test_cli_argument_errors(tmp_path):
    base = ["a.flo", "g.npy", "o.flo"]
    cli_refuses("filter_flow", ([], ["a.flo"], ["a.flo", "g.npy"], base + ["extra"], base + ["--radius", "x"], base + ["--radius", "0"],
                                base + ["--radius", "8"], base + ["--iters", "0"], base + ["--iters", "5"], base + ["--tau", "0"],
                                base + ["--tau", "nan"], base + ["--tau"], base + ["--sigma", "0"], base + ["--sigma", "-1"], base + ["--bw"],
                                base + ["--code"], base + ["--nosuch"]))


def test_resource_table_lists_the_flowfilter_kernels_without_scratch():
    names, table = resource_table()
    # Src x guide type x channels, Itanium-mangled: flowfilter_kernel<DenseSrc | UpsampleSrc, float | unsigned char, 1 | 3>
    for src in ("NS_8DenseSrcE", "NS_11UpsampleSrcE"):
        for t in ("f", "h"):
            for noc in (1, 3):
                hit = [n for n in names if "flowfilter_kernelI%s%sLi%dE" % (src, t, noc) in n]
                assert len(hit) == 1, (src, t, noc)
                assert table[hit[0]] == 0, hit
    fold = [n for n in names if "flowfilter_fold_kernel" in n]
    assert len(fold) == 1 and table[fold[0]] == 0


@pytest.mark.gpu
def test_cli_writes_what_the_call_returns(tmp_path):
    import torch
    from flowonthego_amd.consistency import fb_check
    from flowonthego_amd.flo import read_flo, write_flo
    from flowonthego_amd.flowfilter import filter_flow
    rng = np.random.default_rng(4)
    h, w = 48, 64
    ys, xs = np.mgrid[0:h, 0:w]
    guide = np.clip(90 + 80 * (xs > 30) + rng.normal(0, 3, (h, w)), 0, 255).astype(np.uint8)
    fw = (np.where((xs > 30)[..., None], (3.0, 1.0), (-1.0, 0.0)) + rng.normal(0, 0.2, (h, w, 2))).astype(np.float32)
    bw = (-fw + rng.normal(0, 0.1, (h, w, 2))).astype(np.float32)
    a, g, b, o, c = (str(tmp_path / n) for n in ("fw.flo", "guide.npy", "bw.flo", "out.flo", "code.png"))
    write_flo(a, fw)
    write_flo(b, bw)
    np.save(g, guide)
    r = run_cli("filter_flow", [a, g, o, "--bw", b, "--radius", "4", "--sigma", "2",
                        "--tau", "15", "--iters", "2", "--code", c])
    assert r.returncode == 0, r.stderr
    dev = lambda x: torch.from_numpy(x).cuda()
    mask = fb_check(dev(fw), dev(bw))[0]
    out, code, st = filter_flow(dev(fw), dev(guide), mask=mask, radius=4, sigma=2.0, tau=15.0, iters=2, stats=True)
    got = read_flo(o)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), out.cpu().numpy().view(np.uint32))
    assert os.path.getsize(c) > 0
    st = st.cpu().numpy()
    nums = [float(t) for t in re.findall(r"(-?\d+\.\d+)", r.stdout)]
    want = [st[0] / (h * w), st[1] / (h * w), st[2] / (h * w), st[3] / max(2.0 * st[0], 1.0)]
    assert len(nums) == 4 and np.allclose(nums, want, atol=1e-4), (r.stdout, want)
    assert st[1] > 0                                               # the check rejected some vectors and the filter filled them
