"""The object tracks' host side (no GPU needed): the C-ABI is declared and bound, examples/track_objects.cpp compiles and links
against the C++ shim, the compiler's resource table lists exactly the objvote / objlink / objtrack instantiations, all without a
private-memory segment, and the arguments the entry points refuse are refused before the device is touched.  With a GPU: the CLI
writes what OFClass.track_objects returns and prints a line per track."""
import ctypes as C
import os
import re

import pytest

from host_checks import cli_refuses, entry_points, resource_table, run_cli

NEW_SYMBOLS = ("fotg_object_overlap", "fotg_upsample_crop_object_overlap", "fotg_object_links", "fotg_object_tracks")
FOTG_ERR_ARG = 1


def test_entry_points_are_declared_bound_and_exported():
    F, _ = entry_points(NEW_SYMBOLS, "tracks.h")
    from flowonthego_amd import tracks
    for name in ("object_overlap", "upsample_crop_object_overlap", "object_links", "link_tracks"):
        assert getattr(F, name) is getattr(tracks, name) and callable(getattr(F, name))
    assert F.TRACK == tracks.TRACK and len(F.TRACK) == 8 and F.TRACK_STATS == tracks.TRACK_STATS and len(F.TRACK_STATS) == 4
    assert callable(F.track_objects) and F.track_objects.__name__ == "flowonthego_amd.track_objects"     # the tool's module, callable
    from flowonthego_amd.oflow import OFClass
    assert callable(OFClass.track_objects) and callable(OFClass.upsample_crop_object_overlap)


def test_track_objects_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    assert os.path.exists(_build_example(tmp_path, "track_objects"))


def test_cli_argument_errors():
    base = ["f.npy", "o.npz"]
    cli_refuses("track_objects", ([], base[:1], base + ["extra"], base + ["--model", "rigid"], base + ["--min-area", "0"], base + ["--min-votes", "0"],
                                  base + ["--min-frac", "1.5"], base + ["--max-objects", "1025"], base + ["--ids"], base + ["--nosuch"]))


def test_resource_table_lists_the_object_track_kernels_without_scratch():
    names, table = resource_table()
    mine = sorted(n for n in names if re.search(r"obj(vote|link|track)", n))
    # Itanium-mangled: objvote_kernel<DenseSrc | UpsampleSrc>, objlink_kernel, objtrack_kernel -- and nothing else
    want = ["objvote_kernelINS_8DenseSrcEEE", "objvote_kernelINS_11UpsampleSrcEEE", "14objlink_kernelE", "15objtrack_kernelE"]
    assert len(mine) == len(want), mine
    for frag in want:
        hit = [n for n in mine if frag in n]
        assert len(hit) == 1, (frag, mine)
        assert table[hit[0]] == 0, hit
    # the names stay clear of the substrings by which the other resource-table tests count their kernels
    for n in mine:
        assert not any(s in n for s in ("motion_", "comp_", "warp_fold_kernel", "flowfilter_fold_kernel", "temporal_fold_kernel")), n


def test_arguments_are_refused_before_the_device_is_touched():
    """every pointer is a host address that is never dereferenced: FOTG_ERR_ARG is decided first"""
    import flowonthego_amd as F
    L = F.lib()
    far = lambda k: C.c_void_p(0x10000000 * (k + 1))          # never touched: far apart, so that nothing overlaps

    def overlap(n=1, a=far(1), b=far(2), w=8, h=8, f=far(3), m=None, ka=4, kb=4, v=far(4), s=far(5)):
        return L.fotg_object_overlap(0, n, a, b, w, h, f, m, ka, kb, v, s, None)

    for bad in (dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=0), dict(w=16385), dict(h=16385), dict(ka=0), dict(kb=0),
                dict(ka=1025), dict(kb=1025), dict(a=None), dict(b=None), dict(f=None), dict(v=None), dict(s=None),
                dict(v=far(1)), dict(s=far(3)), dict(v=far(2)), dict(s=far(4)), dict(m=far(5))):
        assert overlap(**bad) == FOTG_ERR_ARG, bad

    def links(n=1, v=far(1), oa=far(2), ob=far(3), ka=4, kb=4, mv=1, mf=64, ab=far(4), ba=far(5)):
        return L.fotg_object_links(0, n, v, oa, ob, ka, kb, mv, mf, ab, ba, None)

    for bad in (dict(n=0), dict(n=65536), dict(ka=0), dict(kb=1025), dict(mv=0), dict(mv=-3), dict(mf=-1), dict(mf=257), dict(v=None),
                dict(oa=None), dict(ob=None), dict(ab=None), dict(ba=None), dict(ab=far(1)), dict(ba=far(3)), dict(ab=far(5))):
        assert links(**bad) == FOTG_ERR_ARG, bad

    def tracks(T=2, K=4, o=far(1), ab=far(2), ba=far(3), mt=8, tr=far(4), tb=far(5), st=far(6)):
        return L.fotg_object_tracks(0, T, K, o, ab, ba, mt, tr, tb, st, None)

    for bad in (dict(T=0), dict(T=65536), dict(K=0), dict(K=1025), dict(mt=0), dict(mt=65537), dict(o=None), dict(ab=None), dict(ba=None),
                dict(tr=None), dict(tb=None), dict(tr=far(1)), dict(tb=far(2)), dict(st=far(3)), dict(tb=far(4)), dict(st=far(5))):
        assert tracks(**bad) == FOTG_ERR_ARG, bad
    assert L.fotg_upsample_crop_object_overlap(None, 1, far(0), far(1), far(2), None, 4, 4, far(4), far(5), None) == FOTG_ERR_ARG


@pytest.mark.gpu
def test_cli_writes_what_the_call_returns(tmp_path, natural_images):
    import numpy as np
    import torch
    import flowonthego_amd as F
    import motion_ref as M
    from flowonthego_amd.oflow import OFClass
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=3, patch=True)
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    fr, out, ids = (str(tmp_path / n) for n in ("frames.npy", "out.npz", "ids.npy"))
    np.save(fr, frames)
    run = run_cli("track_objects", [fr, out, "--min-area", "16", "--max-objects", "32",
                          "--min-votes", "8", "--max-tracks", "64", "--ids", ids])
    assert run.returncode == 0, run.stderr
    op = F.operating_point(2, w, 1)
    op.bidir = True
    o = OFClass(op, F.img_params(width=w, height=h), max_batch=T)
    want = o.track_objects(torch.from_numpy(frames).cuda(), min_area=16, max_objects=32, min_votes=8, max_tracks=64, track_ids=True, stats=True)
    z = np.load(out)
    assert sorted(z.files) == ["objects", "params", "stats", "track", "tracks"]
    for k, t in zip(("params", "objects", "track", "tracks", "stats"), want[:4] + want[5:]):
        assert z[k].dtype == t.cpu().numpy().dtype and np.array_equal(z[k], t.cpu().numpy()), k
    assert np.array_equal(np.load(ids), want[4].cpu().numpy())
    st = want[5].cpu().numpy()
    lines = [l for l in run.stdout.splitlines() if "  frames " in l or " tracks over " in l]
    assert len(lines) == st[1] + 1 and lines[-1].startswith("%d tracks over %d object maps (%d links, %d alive" % (st[0], T, st[2], st[3])), run.stdout
    o.close()
