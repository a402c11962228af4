"""GPU tests of the Middlebury flow colour code (fotg_flow_color / fotg_upsample_crop_color, flowonthego_amd.color): byte-identical
to the numpy restatement of the reference's code (tests/colorcode_ref.py), the fused form byte-identical to colouring
fotg_upsample_crop's output, per-image normalisation, 64-bit batch offsets, the tools, argument checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import colorcode_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def _F():
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    return F, OFClass


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ref_batch(flows, maxmotion=-1.0):
    out = [R.motion_to_color(f, maxmotion) for f in flows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def check_dense(flows, maxmotion=None):
    from flowonthego_amd.color import flow_to_color
    rgb, st = flow_to_color(dev(flows), maxmotion=maxmotion, stats=True)
    want, want_st = ref_batch(flows, -1.0 if maxmotion is None else maxmotion)
    got = rgb.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.nonzero(np.any(got != want, axis=-1))
    assert bad[0].size == 0, (bad[0].size, [(tuple(int(i) for i in b), got[b], want[b], flows[b]) for b in list(zip(*bad))[:3]])
    assert np.array_equal(st.cpu().numpy(), want_st), (st.cpu().numpy(), want_st)


def noisy_field(rng, h, w, scale=6.0, n_bad=40):
    f = (rng.standard_normal((h, w, 2)) * scale).astype(np.float32)
    flat = f.reshape(-1)
    idx = rng.choice(flat.size, min(n_bad, flat.size), replace=False)
    vals = np.array([np.nan, np.inf, -np.inf, 2e9, -2e9, 1e9, -1e9, 0.0, -0.0], np.float32)
    flat[idx] = vals[np.arange(idx.size) % vals.size]
    return f


def test_flow_color_matches_restatement_on_the_fixture_vectors():
    v, _, _, runs = R.load_fixture()
    n = (len(v) // 512) * 512
    img = v[:n].reshape(-1, 512, 2)                    # the vector set laid out as 512-wide images, normalised by maxmotion 1
    from flowonthego_amd.color import flow_to_color
    got = flow_to_color(dev(img[None]), maxmotion=1.0).cpu().numpy().reshape(-1, 3)
    assert np.array_equal(got, R.compute_color(v[:n, 0], v[:n, 1]))
    # and the fixture's fields through the auto and fixed normalisations, the printed statistics the reference's
    for name, flow, mm, step, ref, ref_st in runs:
        check_dense(flow[None], mm)
        assert np.array_equal(R.motion_to_color(flow, mm)[1], ref_st), name


def test_flow_color_fields_and_normalisation():
    rng = np.random.default_rng(3)
    check_dense(np.stack([noisy_field(rng, 37, 53), noisy_field(rng, 37, 53, scale=0.01), noisy_field(rng, 37, 53, scale=300)]))
    for mm in (None, 2.5, 0.0, -3.0, 1e-3):
        check_dense(np.stack([noisy_field(rng, 20, 31), noisy_field(rng, 20, 31, scale=50)]), mm)
    check_dense(np.zeros((2, 9, 10, 2), np.float32))
    check_dense(np.full((2, 5, 6, 2), np.nan, np.float32))
    for h, w in ((1, 1), (1, 7), (7, 1), (3, 5), (13, 1022), (2, 3)):
        check_dense(np.stack([noisy_field(rng, h, w, n_bad=2) for _ in range(3)]))


def test_flow_color_normalises_per_image():
    from flowonthego_amd.color import flow_to_color
    rng = np.random.default_rng(11)
    a, b = noisy_field(rng, 40, 64, scale=0.5, n_bad=0), noisy_field(rng, 40, 64, scale=200.0, n_bad=0)
    both = flow_to_color(dev(np.stack([a, b]))).cpu().numpy()
    alone = [flow_to_color(dev(x)).cpu().numpy() for x in (a, b)]
    assert np.array_equal(both[0], alone[0]) and np.array_equal(both[1], alone[1])
    assert not np.array_equal(both[0], flow_to_color(dev(a), maxmotion=float(np.abs(b).max() * 2)).cpu().numpy())


def _ctx(F, OFClass, w, h, op_pt=2, sc_l=None, max_batch=2, depth=False):
    op = F.operating_point(op_pt, w, 1)
    if sc_l is not None:
        op.finest_scale = sc_l
        op.coarsest_scale = max(op.coarsest_scale, sc_l)
    op.depth_mode = depth
    return OFClass(op, F.img_params(width=w, height=h, padding=op.patch_size), max_batch=max_batch)


def fused_equals_unfused(ofc, coarse, maxmotion=None):
    from flowonthego_amd.color import flow_to_color
    fused, st = ofc.upsample_crop_color(coarse, maxmotion=maxmotion, stats=True)
    full = ofc.upsample_crop(coarse)
    unf, st2 = flow_to_color(full, maxmotion=maxmotion, stats=True)
    assert np.array_equal(fused.cpu().numpy(), unf.cpu().numpy())
    assert np.array_equal(st.cpu().numpy(), st2.cpu().numpy())
    return full


def test_fused_upsample_crop_color_op_points_and_scales():
    F, OFClass = _F()
    rng = np.random.default_rng(5)
    for op_pt in (1, 2, 3, 4):
        ofc = _ctx(F, OFClass, 1920, 1080, op_pt)
        w, h = ofc.out_size()
        coarse = dev(np.stack([noisy_field(rng, h, w, 3.0), noisy_field(rng, h, w, 30.0)]))
        full = fused_equals_unfused(ofc, coarse)
        # and both are the restatement applied to fotg_upsample_crop's output
        want, _ = ref_batch(full.cpu().numpy())
        assert np.array_equal(ofc.upsample_crop_color(coarse).cpu().numpy(), want)
        ofc.close()
    for (w, h) in ((333, 201), (97, 61), (1023, 437)):
        for sc_l in (0, 1, 2, 3):
            ofc = _ctx(F, OFClass, w, h, 2, sc_l=sc_l)
            cw, ch = ofc.out_size()
            coarse = dev(np.stack([noisy_field(rng, ch, cw, 2.0, n_bad=5), noisy_field(rng, ch, cw, 9.0, n_bad=0)]))
            fused_equals_unfused(ofc, coarse)
            fused_equals_unfused(ofc, coarse, maxmotion=4.0)
            ofc.close()


def test_fused_color_on_engine_outputs(alley, natural_images):
    F, OFClass = _F()
    a0, a1 = alley["frame_0001"].astype(np.float32), alley["frame_0002"].astype(np.float32)
    ofc = _ctx(F, OFClass, 1024, 436, 2, max_batch=1)
    out = ofc.calc(dev(a0), dev(a1))
    fused_equals_unfused(ofc, out[None].contiguous())
    ofc.close()
    road = natural_images["road_HD"].astype(np.float32)
    n = 64
    I0 = np.stack([road] * n)
    I1 = np.stack([np.roll(road, (i % 5 - 2, i % 7 - 3), axis=(0, 1)) for i in range(n)])
    ofc = _ctx(F, OFClass, 1920, 1080, 2, max_batch=n)
    flows = ofc.calc_batch(dev(I0[..., None]), dev(I1[..., None]))
    torch.cuda.synchronize()
    fused_equals_unfused(ofc, flows[:1].contiguous())
    fused_equals_unfused(ofc, flows)
    ofc.close()


def test_fused_color_64bit_offsets():
    """96 x 3840 x 2160 through the fused form (2.4 GB of RGB): the last pair equals that pair coloured alone"""
    F, OFClass = _F()
    n = 96
    ofc = _ctx(F, OFClass, 3840, 2160, 1, max_batch=n)
    w, h = ofc.out_size()
    g = torch.Generator(device="cuda").manual_seed(1)
    coarse = torch.randn((n, h, w, 2), device="cuda", generator=g) * torch.linspace(0.5, 50, n, device="cuda").view(n, 1, 1, 1)
    rgb = ofc.upsample_crop_color(coarse)
    assert rgb.shape == (n, 2160, 3840, 3) and rgb.numel() > 2 ** 31
    last = ofc.upsample_crop_color(coarse[n - 1:].contiguous())
    assert torch.equal(rgb[n - 1], last[0])
    first = ofc.upsample_crop_color(coarse[:1].contiguous())
    assert torch.equal(rgb[0], first[0])
    del rgb
    ofc.close()


def _build_example(tmp_path):
    exe = os.path.join(str(tmp_path), "color_flow")
    libdir = os.path.join(ROOT, "flowonthego_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "color_flow.cpp"),
                           "-L" + libdir, "-lfotg", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_color_flow_tools_match_reference(tmp_path):
    from PIL import Image
    from flowonthego_amd.flo import write_flo
    runs = {r[0]: r for r in R.load_fixture()[3]}
    flo = str(tmp_path / "alley.flo")
    write_flo(flo, np.load(os.path.join(GOLDEN, "alley_0001_flo.npz"))["flow"])
    exe = _build_example(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for args, name in (([], "alley"), (["5"], "alley_max5")):
        p_cpp, p_py = str(tmp_path / "cpp.png"), str(tmp_path / "py.png")
        r1 = subprocess.run([exe, flo, p_cpp] + args, capture_output=True, text=True, timeout=120)
        r2 = subprocess.run([sys.executable, "-m", "flowonthego_amd.color_flow", flo, p_py] + args, capture_output=True, text=True,
                            timeout=300, env=env, cwd=ROOT)
        assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
        assert r1.stdout == r2.stdout and r1.stdout.startswith("max motion: 7.1662  motion range: u = -7.152 .. -1.186;"), r1.stdout
        def tool_lines(err):                           # (the runtime may add lines of its own to stderr)
            return [l for l in err.splitlines() if l.startswith(("normalizing by", "Writing image"))]
        assert tool_lines(r1.stderr) == tool_lines(r2.stderr.replace(p_py, p_cpp)) and len(tool_lines(r1.stderr)) == 2, (r1.stderr, r2.stderr)
        a, b = np.asarray(Image.open(p_cpp)), np.asarray(Image.open(p_py))
        assert np.array_equal(a, b)
        _, _, _, step, ref, _ = runs[name]
        d = np.abs(a[::step].astype(int) - ref.astype(int))
        assert d.max() <= 1 and np.count_nonzero(d.max(-1)) <= 1e-5 * d.shape[0] * d.shape[1]
    r = subprocess.run([exe, "-quiet", flo, str(tmp_path / "q.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "normalizing" not in r.stderr and r.stdout.startswith("max motion:")


def test_color_wheel_legend():
    import flowonthego_amd as F
    img = F.color_wheel(5, 151)
    assert img.shape == (151, 151, 3) and img.dtype == np.uint8
    assert not img[75].any() and not img[:, 75].any()        # axes
    f32 = np.float32
    rng = f32(1.04 * 5.0)
    x, y = 20, 110
    fx, fy = f32(x) / f32(75) * rng - rng, f32(y) / f32(75) * rng - rng
    assert np.array_equal(img[y, x], R.compute_color(np.array([fx / f32(5)]), np.array([fy / f32(5)]))[0])


def test_bad_arguments_and_depth_mode():
    F, OFClass = _F()
    L = F.lib()
    buf = torch.zeros(64, device="cuda")
    rgb = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p, q = C.c_void_p(buf.data_ptr()), C.c_void_p(rgb.data_ptr())
    for args in ((0, 0, p, 2, 2), (0, 1, None, 2, 2), (0, 1, p, 0, 2), (0, 1, p, 2, -1)):
        assert L.fotg_flow_color(*args, C.c_float(-1), q, None, None) == 1, args
    assert L.fotg_flow_color(0, 1, p, 2, 2, C.c_float(-1), None, None, None) == 1
    # stats == NULL: the keys live in stream-ordered memory of the library's own
    assert L.fotg_flow_color(0, 1, p, 4, 4, C.c_float(-1), q, None, None) == 0
    torch.cuda.synchronize()
    ofc = _ctx(F, OFClass, 96, 64, 2, max_batch=2)
    w, h = ofc.out_size()
    coarse = torch.zeros((3, h, w, 2), device="cuda")
    out = torch.zeros((3, 64, 96, 3), dtype=torch.uint8, device="cuda")
    cp, op_ = C.c_void_p(coarse.data_ptr()), C.c_void_p(out.data_ptr())
    for n in (0, 3):
        assert L.fotg_upsample_crop_color(ofc._h, n, cp, C.c_float(-1), op_, None, None) == 1, n
    assert L.fotg_upsample_crop_color(None, 1, cp, C.c_float(-1), op_, None, None) == 1
    assert L.fotg_upsample_crop_color(ofc._h, 1, None, C.c_float(-1), op_, None, None) == 1
    assert L.fotg_upsample_crop_color(ofc._h, 1, cp, C.c_float(-1), None, None, None) == 1
    ofc.close()
    dctx = _ctx(F, OFClass, 96, 64, 2, max_batch=1, depth=True)
    assert L.fotg_upsample_crop_color(dctx._h, 1, cp, C.c_float(-1), op_, None, None) == 1
    with pytest.raises(F.FotgError):
        dctx.upsample_crop_color(coarse[:1, ..., :1].contiguous())
    dctx.close()
