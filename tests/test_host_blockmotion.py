"""The block motion vectors' host side (no GPU needed): the C-ABI is declared and bound, examples/block_motion.cpp compiles and links
against the C++ shim, the CLI refuses bad arguments, and the compiler's resource table lists every blockmv_kernel instantiation
without a private-memory segment.  With a GPU: the CLI writes what block_motion returns and prints its numbers."""
import os
import re

import numpy as np
import pytest

from host_checks import cli_refuses, entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_block_motion", "fotg_upsample_crop_block_motion")


def test_entry_points_are_declared_bound_and_exported():
    F, _ = entry_points(NEW_SYMBOLS, "blockmotion.h")
    assert callable(F.block_motion) and callable(F.upsample_crop_block_motion)
    from flowonthego_amd.blockmotion import block_motion, upsample_crop_block_motion
    assert F.upsample_crop_block_motion is upsample_crop_block_motion and callable(block_motion)
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.block_motion) and callable(OFClass.upsample_crop_block_motion)


def test_block_motion_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "block_motion"))


def test_cli_argument_errors(tmp_path):
    base = ["c.npy", "r.npy", "f.flo", "o.npz"]
    cli_refuses("block_motion", ([], ["c.npy"], base[:2], base[:3], base + ["extra"], base + ["--block", "x"], base + ["--block", "12"],
                                 base + ["--block", "64"], base + ["--block"], base + ["--refine", "4"], base + ["--refine", "-1"],
                                 base + ["--refine", "1.5"], base + ["--refine"], base + ["--bw"], base + ["--pred"], base + ["--nosuch"]))


def test_resource_table_lists_the_blockmv_kernels_without_scratch():
    names, table = resource_table()
    # Src x channels x block, Itanium-mangled: blockmv_kernel<DenseSrc | UpsampleSrc, 1 | 3, 8 | 16 | 32>
    for src in ("NS_8DenseSrcE", "NS_11UpsampleSrcE"):
        for noc in (1, 3):
            for block in (8, 16, 32):
                hit = [n for n in names if "blockmv_kernelI%sLi%dELi%dEE" % (src, noc, block) in n]
                assert len(hit) == 1, (src, noc, block)
                assert table[hit[0]] == 0, hit
    fold = [n for n in names if "blockmv_fold_kernel" in n]
    assert len(fold) == 1 and table[fold[0]] == 0


@pytest.mark.gpu
def test_cli_writes_what_the_call_returns(tmp_path):
    import torch
    import blockmotion_ref as R
    from flowonthego_amd.blockmotion import block_motion
    from flowonthego_amd.consistency import fb_check
    from flowonthego_amd.flo import write_flo
    h, w = 40, 70
    cur, ref, flow, _ = R.scene(h, w, 3, 7, n=1)
    cur, ref, fw = cur[0], ref[0], np.where(np.isfinite(flow[0]), flow[0], np.float32(0))
    bw = (-fw + np.random.default_rng(8).normal(0, 0.3, fw.shape)).astype(np.float32)
    c, r, a, b, o, p = (str(tmp_path / n) for n in ("cur.npy", "ref.npy", "fw.flo", "bw.flo", "out.npz", "pred.png"))
    np.save(c, cur)
    np.save(r, ref)
    write_flo(a, fw)
    write_flo(b, bw)
    run = run_cli("block_motion", [c, r, a, o, "--block", "8", "--refine", "3", "--bw", b,
                          "--pred", p])
    assert run.returncode == 0, run.stderr
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    mask = fb_check(dev(fw), dev(bw))[0]
    mv, cost, kind, st = block_motion(dev(cur), dev(ref), dev(fw), mask=mask, block=8, refine=3, stats=True)
    z = np.load(o)
    assert sorted(z.files) == ["cost", "kind", "mv"]
    for k, t, dt in (("mv", mv, np.int16), ("cost", cost, np.uint32), ("kind", kind, np.uint8)):
        assert z[k].dtype == dt and np.array_equal(z[k], t.cpu().numpy()), k
    assert os.path.getsize(p) > 0
    st = st.cpu().numpy()
    nums = re.findall(r"(\d+(?:\.\d+)?)", run.stdout)
    assert [int(nums[0]), int(nums[1])] == st[:2].tolist() and abs(float(nums[2]) - R.psnr(st[2], cur.size)) < 0.006, run.stdout
