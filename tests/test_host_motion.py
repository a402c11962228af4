"""The global-motion fit's host side (no GPU needed): the C-ABI is declared and bound, examples/fit_motion.cpp compiles and links
against the C++ shim, the two command-line tools refuse bad arguments, and the compiler's resource table lists every instantiation
of the motion kernels without a private-memory segment.  With a GPU: the two tools write and print what the calls return."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from host_checks import cli_refuses, entry_points, gray_png_bytes, read_png_rgb, resource_table, run_cli

NEW_SYMBOLS = ("fotg_fit_motion", "fotg_upsample_crop_fit_motion", "fotg_motion_flow", "fotg_motion_ending")


def test_entry_points_are_declared_bound_and_exported():
    F, hdr = entry_points(NEW_SYMBOLS, "motion.h", in_shim=NEW_SYMBOLS[:3])
    for name in ("fit_motion", "motion_flow", "upsample_crop_fit_motion", "stabilize", "smoothing_motions"):
        assert callable(getattr(F, name)), name
    assert F.MODELS == ("translation", "similarity", "affine") and len(F.CODES) == 4
    import flowonthego_amd.motion as M
    for name in ("fit_motion", "motion_flow", "stabilize", "MODELS", "CODES"):
        assert hasattr(M, name), name
    from flowonthego_amd.oflow import OFClass
    for name in ("upsample_crop_fit_motion", "camera_motion", "stabilize"):
        assert callable(getattr(OFClass, name)), name
    # the definition and the overflow limit of the sums are written at the head of the kernels and in the public header
    head = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "motion.hip.h")).read()
    for text in (head, hdr):
        assert "2^62" in text and "16384" in text


def test_the_ending_switch_needs_no_gpu():
    import flowonthego_amd as F
    L = F.lib()
    first = L.fotg_motion_ending(-1)
    assert first in (0, 1)
    assert L.fotg_motion_ending(1 - first) == first and L.fotg_motion_ending(7) == 1 - first
    assert L.fotg_motion_ending(first) == 1 - first and L.fotg_motion_ending(-1) == first


def test_fit_motion_example_builds(tmp_path):
    import flowonthego_amd as F
    F.lib()
    from test_host import _build_example
    exe = _build_example(tmp_path, "fit_motion")
    assert os.path.exists(exe)
    for args in ([], ["a.flo", "projective"], ["a.flo", "affine", "x"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, args


def test_cli_argument_errors(tmp_path):
    bad = {"fit_motion": ([], ["a.flo", "b.flo"], ["a.flo", "--model", "projective"], ["a.flo", "--iters", "-1"], ["a.flo", "--thresh", "-2"],
                          ["a.flo", "--mask"]),
           "stabilize": ([], ["frames.npy"], ["frames.npy", "out.npy", "--model", "homography"], ["frames.npy", "out.npy", "--radius", "-1"],
                         ["frames.npy", "out.npy", "extra.npy"])}
    for tool, cases in bad.items():
        cli_refuses(tool, cases)


def test_gray_png_reader_reads_every_filter(tmp_path):
    """the mask reader of the fit_motion tool against a PNG written here with each of the five row filters"""
    import struct
    import zlib
    from flowonthego_amd.fit_motion import read_gray_png
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (10, 7), dtype=np.uint8)
    img[:, 3] = 0
    rows, prev = [], np.zeros(7, np.int32)
    for y in range(10):
        ft, cur, line = y % 5, img[y].astype(np.int32), []
        for x in range(7):
            a, b, c = (cur[x - 1] if x else 0), prev[x], (prev[x - 1] if x else 0)
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            line.append((cur[x] - (0, a, b, (a + b) // 2, paeth)[ft]) & 255)
        rows.append(bytes([ft] + line))
        prev = cur
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    path = str(tmp_path / "m.png")
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 10, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(b"".join(rows))) + chunk(b"IEND", b""))
    assert np.array_equal(read_gray_png(path), img)


def test_resource_table_lists_the_motion_kernels_without_scratch():
    names, table = resource_table()
    # Itanium-mangled: motion_pass_kernel<DenseSrc | UpsampleSrc, round 0 | later round | final>, motion_fold_kernel<12 | 4>
    want = ["motion_pass_kernelI%sLi%dE" % (src, p) for src in ("NS_8DenseSrcE", "NS_11UpsampleSrcE") for p in (0, 1, 2)]
    want += ["motion_fold_kernelILi12E", "motion_fold_kernelILi4E", "motion_solve_kernelE", "motion_flow_kernelE"]
    for w in want:
        hit = [n for n in names if w in n]
        assert len(hit) == 1, w
        assert table[hit[0]] == 0, hit
    assert len([n for n in names if "motion_" in n]) == len(want)                  # and no instantiation beyond these


@pytest.mark.gpu
def test_fit_motion_cli_prints_and_writes_what_the_call_returns(tmp_path):
    import torch
    import flowonthego_amd as F
    from flowonthego_amd.flo import write_flo
    rng = np.random.default_rng(15)
    h, w = 23, 41
    ys, xs = np.mgrid[0:h, 0:w]
    flow = (np.stack([0.02 * xs - 0.01 * ys + 1.5, 0.01 * xs + 0.03 * ys - 0.5], -1) + 0.2 * rng.standard_normal((h, w, 2))).astype(np.float32)
    flow[5:11, 20:30] += 4.0                              # a patch that moves on its own
    flow[3, 7] = (np.nan, 0)
    mask = (rng.random((h, w)) < 0.1).astype(np.uint8) * 200
    fl, mk, cd = (str(tmp_path / n) for n in ("f.flo", "m.png", "code.png"))
    write_flo(fl, flow)
    open(mk, "wb").write(gray_png_bytes(mask))
    run = run_cli("fit_motion", [fl, "--mask", mk, "--model", "affine", "--code", cd])
    assert run.returncode == 0, run.stderr
    params, code, st = F.fit_motion(torch.from_numpy(flow).cuda(), torch.from_numpy(mask).cuda(), "affine", 3, 1.0, code=True, stats=True)
    lines = run.stdout.splitlines()
    assert len(lines) == 2 and lines[0] == " ".join("%.9g" % v for v in params.cpu().numpy())
    code, st = code.cpu().numpy(), st.cpu().numpy()
    assert len(set(code.ravel().tolist())) == 4           # follows, independent, masked and unknown all occur
    assert lines[1] == "  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(F.CODES, st[:4]))
    palette = np.array([(255, 255, 255), (220, 30, 30), (128, 128, 128), (0, 0, 0)], np.uint8)
    assert np.array_equal(read_png_rgb(cd), palette[code])


def _stabilize_frames(form):
    ys, xs = np.mgrid[0:48, 0:64]
    rgb = np.stack([np.stack([128 + 60 * np.sin((ys + k + 3 * c) / 6.0) + 50 * np.cos((xs - 2 * k - c) / 5.0) for c in range(3)], -1)
                    for k in range(4)])
    rgb = np.clip(np.rint(rgb), 0, 255)
    return {"gray": rgb[..., 0].astype(np.uint8), "gray_c1": rgb[..., :1].astype(np.uint8), "rgb_u8": rgb.astype(np.uint8),
            "rgb_f32": rgb.astype(np.float32)}[form]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gray", "gray_c1", "rgb_u8", "rgb_f32"])
def test_stabilize_cli_writes_what_the_call_returns(tmp_path, form):
    """the context as the tool's text describes it: both directions, one pair per frame step; 8-bit gray frames (with or without
    a trailing channel of 1) on one channel, 8-bit colour made gray from R, G, B on load, float32 colour on three channels"""
    import torch
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    frames = _stabilize_frames(form)
    a, b = str(tmp_path / "frames.npy"), str(tmp_path / "out.npy")
    np.save(a, frames)
    run = run_cli("stabilize", [a, b, "--radius", "2"])
    assert run.returncode == 0, run.stderr
    given = frames[..., 0] if form == "gray_c1" else frames
    op = F.operating_point(2, 64, 3 if form == "rgb_f32" else 1)
    op.bidir = True
    if form == "rgb_u8":
        op.u8_color = 2
    ofc = OFClass(op, F.img_params(width=64, height=48), max_batch=3)
    out, code = ofc.stabilize(torch.from_numpy(given).cuda(), model="similarity", radius=2, fill=None)
    want = out.cpu().numpy()
    holes = (code != 0).float().mean(dim=(1, 2)).cpu().numpy()
    ofc.close()
    got = np.load(b)
    assert got.dtype == frames.dtype and got.shape == given.shape and got.tobytes() == want.tobytes()
    assert run.stdout == "unfilled share per frame: " + " ".join("%.4f" % v for v in holes) + "\n"
