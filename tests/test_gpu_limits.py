"""GPU tests of the add-ons at the limits their headers promise (warp, fb-check, colour, interp, temporal, flow filter, block motion,
chain, motion fit, layers, components, tracks, histograms, motion blur, plate, subtract, erase, morph), in four parts:

1. accumulators at the promised extremes: 16384 x 16384 images whose exact integer sums reach the top of the documented ranges
   (|sum XU| = 2^61, area 2^28, sum U = 2^48, 2^28 votes in an int32), against the closed forms of tests/limits_ref.py, which
   tests/test_limits.py proves against the restatements at small sizes;
2. the largest dimension on thin frames (16384 x 1, 1 x 16384, 16384 x 3, 3 x 16384; 65535 tile rows for the two kernels that
   refuse more), every add-on against its own restatement by the comparison of its own GPU test;
3. the largest batch: one C-ABI call of 65535 images of 3 x 2 pixels per entry point that documents n <= 65535, outputs between
   guard elements;
4. offsets beyond 2^31 elements: one call per add-on against the same call on chunks of eight images.

Every input stays inside the documented limits; the only refused calls are the two of part 2, which return before a launch.

Measured once on an MI355X (wall time of the slowest case of a test, peak device memory of its tensors):
  part 1   motion sums 0.05 s / 2.0 GiB; far corners 0.13 s / 4.3 GiB; layers 0.26 s / 2.0 GiB; components 0.25 s / 6.8 GiB (one
           label_components call at 16384 x 16384: 0.03 s for the single object, 0.01 s for 8192 stripes, so no shape was cut);
           votes 0.01 s / 5.3 GiB; morphology 0.05 s / 4.5 GiB
  part 2   every case below 0.6 s but block motion (1.35 s) and motion blur (1.17 s), whose restatements walk blocks or taps on the
           host; plate 0.77 s; the two 65535-tile-row tests 0.75 s and 1.06 s; all below 0.1 GiB
  part 3   every test below 0.4 s and 0.1 GiB
  part 4   interp 0.48 s / 18.3 GiB; temporal 0.83 s / 10.9; flow filter 0.60 s / 19.8; block motion 0.06 s / 12.1; chain 1.17 s /
           16.3; motion fit 0.09 s / 19.8; layers 1.34 s / 9.7; components 0.20 s / 19.1; votes 1.62 s / 17.0; histograms 0.03 s /
           8.8; motion blur 0.05 s / 13.8; plate 0.36 s / 10.4; subtract 0.03 s / 20.1; erase 0.04 s / 23.1; morphology 0.04 s / 14.4"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import limits_ref as X
import morph_ref as MR

pytestmark = pytest.mark.gpu

N = X.LIMIT
f32 = np.float32


def _F():
    import flowonthego_amd as F
    return F


def f64_bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ints(t):
    return t.cpu().numpy().astype(np.int64)


@pytest.fixture(autouse=True)
def _time_and_memory(request):
    """prints what the docstrings quote: the test's wall time and its peak device memory"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\n[limits] %s: %.2f s, peak %.2f GiB" % (request.node.name, time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2.0 ** 30))
    torch.cuda.empty_cache()


def separable_flow(ux, vy):
    """(h, w, 2) f32 on the device: u = ux[x], v = vy[y], written by two broadcast copies"""
    flow = torch.empty((len(vy), len(ux), 2), dtype=torch.float32, device="cuda")
    flow[..., 0] = torch.from_numpy(ux).cuda()[None, :]
    flow[..., 1] = torch.from_numpy(vy).cuda()[:, None]
    return flow


@pytest.fixture(scope="module")
def sgn_flow():
    """the 2 GiB flow u = 4096 sgn(X), v = -4096 sgn(Y) at 16384 x 16384, shared by the motion and the layer tests, never written"""
    ux, vy = X.sgn_profiles(N, N)
    flow = separable_flow(ux, vy)
    yield ux, vy, flow
    del flow
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- 1. accumulators at the promised extremes --------------------------------------------------------------------------------------
def test_motion_sums_reach_2_pow_61(sgn_flow):
    """fit_motion at 16384 x 16384, |sum XU| = |sum YV| = 2^61: sums, stats and the parameters' f64 bits, every model, both endings"""
    from flowonthego_amd.motion import fit_motion
    L = _F().lib()
    ux, vy, flow = sgn_flow
    prev = L.fotg_motion_ending(-1)
    try:
        for model in (0, 1, 2):
            want = X.motion_expected(ux, vy, model, 1.0)
            assert abs(want["sums"][7]) == 1 << 61 and want["sums"][0] == 1 << 28
            for ending in (prev, 1 - prev):
                L.fotg_motion_ending(ending)
                params, stats, sums = fit_motion(flow.unsqueeze(0), None, model, 0, 1.0, code=False, residual=False, stats=True, sums=True)
                torch.cuda.synchronize()
                assert ints(sums[0]).tolist() == want["sums"], (model, ending, ints(sums[0]).tolist(), want["sums"])
                assert ints(stats[0]).tolist() == want["stats"], (model, ending, ints(stats[0]).tolist(), want["stats"])
                assert np.array_equal(f64_bits(params[0]), f64_bits(want["params"])), (model, ending, params[0].tolist(), want["params"])
    finally:
        L.fotg_motion_ending(prev)
    torch.cuda.synchronize()


def test_motion_reads_the_far_corners(sgn_flow):
    """a mask that leaves only the four corners of 16384 x 16384, iters = 3: the system is usable, the sums are tiny, and they hold
    the far corner's coordinates"""
    from flowonthego_amd.motion import fit_motion
    ux, vy, flow = sgn_flow
    mask = torch.ones((N, N), dtype=torch.uint8, device="cuda")
    xs, ys = X.corners(N, N)
    mask[torch.from_numpy(ys).cuda(), torch.from_numpy(xs).cuda()] = 0
    assert int(mask.sum()) == N * N - 4 and int(mask[N - 1, N - 1]) == 0
    for model in (0, 1, 2):
        want = X.motion_corners_expected(ux, vy, model, 3, 1.0)
        params, stats, sums = fit_motion(flow, mask, model, 3, 1.0, stats=True, sums=True)
        torch.cuda.synchronize()
        assert ints(sums).tolist() == want["sums"], (model, ints(sums).tolist(), want["sums"])
        assert ints(stats).tolist() == want["stats"], (model, ints(stats).tolist(), want["stats"])
        assert np.array_equal(f64_bits(params), f64_bits(want["params"])), (model, params.tolist(), want["params"])
    assert X.motion_corners_expected(ux, vy, 2, 3, 1.0)["stats"] == [4, 0, N * N - 4, 0, 4, 1]
    del mask
    torch.cuda.synchronize()


def test_layers_inherit_the_motion_sums(sgn_flow):
    """motion_layers with one layer at 16384 x 16384: layer 0 equals fit_motion (sums and f64 bits), with rounds = 0 and, where
    every pixel stays within thresh (8192 px), after a refinement round; the records follow the closed form -- also at thresh = 1,
    where the refinement fits the few pixels that follow"""
    from flowonthego_amd.layers import motion_layers
    from flowonthego_amd.motion import fit_motion
    ux, vy, flow = sgn_flow
    for model in (0, 1, 2):
        fit_p, fit_s = fit_motion(flow, None, model, 0, 8192.0, sums=True)
        for thresh in (8192.0, 1.0):
            for rounds in (0, 1):
                want = X.layers_expected(ux, vy, model, rounds, thresh)
                params, records, stats, sums = motion_layers(flow, None, 1, model, 0, rounds, thresh, records=True, stats=True, sums=True)
                torch.cuda.synchronize()
                tag = (model, thresh, rounds)
                assert ints(sums).tolist() == want["sums"], (tag, ints(sums).tolist(), want["sums"])
                assert ints(records).tolist() == want["records"], (tag, ints(records).tolist(), want["records"])
                assert ints(stats).tolist() == want["stats"], (tag, ints(stats).tolist(), want["stats"])
                assert np.array_equal(f64_bits(params), f64_bits(want["params"])), (tag, params.tolist(), want["params"])
                if thresh == 8192.0:
                    assert want["records"][0][0] == 1 << 28                                   # every pixel labelled
                    assert torch.equal(sums[0], fit_s) and np.array_equal(f64_bits(params[0]), f64_bits(fit_p)), tag
    torch.cuda.synchronize()


COMPONENT_SHAPES = {"all": [(N, N)], "rows": [(N, N)], "columns": [(N, N)]}           # (w, h) per pattern


@pytest.mark.parametrize("pattern,w,h", [(p, w, h) for p in X.PATTERNS for w, h in COMPONENT_SHAPES[p]])
def test_components_at_the_limit(pattern, w, h):
    """label_components of a map that sends every merge of an image to one root per stripe: one object of area 2^28 with
    sum U = 2^48, or 8192 stripes of 16384 pixels; connectivity 4 and 8; objects, stats, labels and ids against the closed form"""
    from flowonthego_amd.objects import label_components
    code = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    if pattern == "all":
        code[:] = 1
    elif pattern == "rows":
        code[0::2] = 1
    else:
        code[:, 0::2] = 1
    values = torch.empty((h, w, 2), dtype=torch.float32, device="cuda")
    values[..., 0] = X.VALUE_U
    values[..., 1] = X.VALUE_V
    max_objects = 65536
    want = X.components_expected(pattern, w, h, max_objects)
    wl, wi = (torch.from_numpy(a).cuda().to(torch.int32) for a in X.component_labels(pattern, w, h, max_objects))
    for conn in (4, 8):
        t0 = time.perf_counter()
        objects, labels, ids, stats = label_components(code, (1,), conn, values, 1, max_objects, labels=True, ids=True, stats=True)
        torch.cuda.synchronize()
        print("\n[limits] label_components %s %d x %d connectivity %d: %.3f s" % (pattern, w, h, conn, time.perf_counter() - t0))
        assert ints(stats).tolist() == want["stats"], (conn, ints(stats).tolist(), want["stats"])
        got = ints(objects)
        assert np.array_equal(got, want["objects"]), (conn, got[:3], want["objects"][:3], np.argwhere(got != want["objects"])[:8])
        assert bool((labels == wl).all()) and bool((ids == wi).all()), conn
        del objects, labels, ids, stats
    del code, values
    torch.cuda.synchronize()


def test_object_votes_reach_2_pow_28():
    """object_overlap at 16384 x 16384 with one object that covers both frames: 2^28 votes in one int32 counter, and each column of
    `sent` at 2^28 in turn.  A vector of (16384, 0) is beyond +-4096 px, so the definition counts it as inadmissible (column 3),
    not as outside (column 2); (4096, -4096), the longest admissible vector, sends 7 x 2^24 pixels outside and 9 x 2^24 votes."""
    from flowonthego_amd.tracks import object_overlap
    ids = torch.zeros((N, N), dtype=torch.int32, device="cuda")
    flow = torch.zeros((N, N, 2), dtype=torch.float32, device="cuda")
    ones = torch.ones((N, N), dtype=torch.uint8, device="cuda")
    for u, v, masked in ((0.0, 0.0, False), (16384.0, 0.0, False), (4096.0, -4096.0, False), (0.0, 0.0, True)):
        flow[..., 0] = u
        flow[..., 1] = v
        wv, ws = X.votes_expected(N, N, u, v, masked, 2, 3)
        votes, sent = object_overlap(ids, ids, flow, ones if masked else None, 2, 3)
        torch.cuda.synchronize()
        assert votes.dtype == torch.int32 and np.array_equal(votes.cpu().numpy(), wv), (u, v, masked, votes.tolist(), wv.tolist())
        assert np.array_equal(ints(sent), ws), (u, v, masked, sent.tolist(), ws.tolist())
    assert X.votes_expected(N, N, 0.0, 0.0, False, 2, 3)[0][0, 0] == 1 << 28
    del ids, flow, ones
    torch.cuda.synchronize()


def test_morphology_at_the_limit():
    """morphology at 16384 x 16384, every op, r = 1 and 8: a uniform map stays as it is (the border does not erode); a map with one
    clear byte in the last corner equals the restatement there and the closed-form counts everywhere"""
    from flowonthego_amd.morph import morphology
    x = torch.empty((N, N), dtype=torch.uint8, device="cuda")
    for op in X.MORPH_OPS:
        for r in (1, 8):
            for fillv in (1, 0):
                x.fill_(fillv)
                out, stats = morphology(x, op, r, stats=True)
                torch.cuda.synchronize()
                assert bool((out == fillv).all()), (op, r, fillv)
                assert ints(stats).tolist() == [fillv * N * N, fillv * N * N, 0, 0], (op, r, fillv, stats.tolist())
            x.fill_(1)
            x[N - 1, N - 1] = 0
            out, stats = morphology(x, op, r, stats=True)
            torch.cuda.synchronize()
            want = MR.morphology(x[-128:, -128:].cpu().numpy(), op, r)[0][-64:, -64:]
            assert np.array_equal(out[-64:, -64:].cpu().numpy(), want), (op, r)
            assert ints(stats).tolist() == X.pinhole_expected(N, N, op, r), (op, r, stats.tolist(), X.pinhole_expected(N, N, op, r))
            assert int(out.sum(dtype=torch.int64)) == X.pinhole_expected(N, N, op, r)[1], (op, r)
            del out, stats
    del x
    torch.cuda.synchronize()


# ---- 2. the largest dimensions on thin frames, against the restatements --------------------------------------------------------------
# 16384 x 1, 1 x 16384, 16384 x 3 and 3 x 16384: 256 tile columns by one tile row (or the transpose), every halo clipped on both
# sides, a last partial quad or strip.  Every add-on goes through its Python wrapper and is compared with its own restatement by the
# comparison of its own GPU test (imported from that module), n >= 2 images of different content, with non-finite and out-of-range
# vectors in the first and the last quad of the first and the last row.
THIN_IDS = ["%dx%d" % s for s in X.THIN]
thin = pytest.mark.parametrize("w,h", X.THIN, ids=THIN_IDS)
kinds = pytest.mark.parametrize("noc,u8", [(1, False), (3, True), (1, True), (3, False)], ids=["f32-1", "u8-3", "u8-1", "f32-3"])
two_kinds = pytest.mark.parametrize("noc,u8", [(1, False), (3, True)], ids=["f32-1", "u8-3"])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seed_of(w, h, *more):
    return 7 * w + 3 * h + sum((i + 2) * int(m) for i, m in enumerate(more))


@thin
@kinds
def test_thin_warp(w, h, noc, u8):
    import test_gpu_warp as T
    s = seed_of(w, h, noc, u8)
    src, ref = X.thin_images(w, h, 2, noc, u8, s), X.thin_images(w, h, 2, noc, u8, s + 1)
    flow, occ = X.thin_flow(w, h, 2, s), X.thin_mask(w, h, 2, s)
    flow[0, :, -1, 0], flow[1, -1, :, 1] = 0.0, 0.0                  # targets exactly on the last column and the last row
    T.assert_dense_matches(src, flow, ref, occ, None)
    _, code, _ = T.assert_dense_matches(src, flow, ref, None, 17.5)
    assert set(np.unique(code)) >= {0, 2, 3}


@thin
def test_thin_fb_check(w, h):
    import test_gpu_bidir as T
    s = seed_of(w, h)
    fw = X.thin_flow(w, h, 2, s)
    bw = X.edge_specials(-fw + X.thin_flow(w, h, 2, s + 1, 0.3, specials=False), 5)
    T.assert_dense_matches(fw, bw)
    T.assert_dense_matches(fw, bw, 0.0, 1.0)


@thin
def test_thin_colour(w, h):
    import test_gpu_color as T
    flows = X.thin_flow(w, h, 2, seed_of(w, h), 6.0)
    flows[1] *= f32(0.25)                                            # another maximum per image
    T.check_dense(flows)
    T.check_dense(flows, 5.0)


@thin
@kinds
def test_thin_interp(w, h, noc, u8):
    import test_gpu_interp as T
    s = seed_of(w, h, noc, u8)
    I0, I1, ref = (X.thin_images(w, h, 2, noc, u8, s + k) for k in range(3))
    F, B = X.thin_flow(w, h, 2, s), X.thin_flow(w, h, 2, s + 1, 2.0)
    mF, mB = X.thin_mask(w, h, 2, s), X.thin_mask(w, h, 2, s + 1)
    T.assert_dense_matches(I0, I1, F, B, 0.3, mF, mB, ref)
    T.assert_dense_matches(I0, I1, F, B, 0.5)                        # the call's own consistency check


@thin
@two_kinds
def test_thin_temporal(w, h, noc, u8):
    import test_gpu_temporal as T
    s = seed_of(w, h, noc, u8)
    n, K = len(T.CENTER), 2
    frames, ref = X.thin_images(w, h, T.T, noc, u8, s), X.thin_images(w, h, n, noc, u8, s + 1)
    flows = X.thin_flow(w, h, n * K, s, 0.4).reshape(n, K, h, w, 2)
    masks = X.thin_mask(w, h, n * K, s).reshape(n, K, h, w)
    used = T.assert_dense_matches(frames, K, flows, masks, 40.0, T.GAINS[:K], ref)
    assert 0 in used and K in used
    T.assert_dense_matches(frames, K, flows, None, 40.0, None, None)


@thin
@two_kinds
def test_thin_flow_filter(w, h, noc, u8):
    import flowfilter_ref as R
    import test_gpu_flowfilter as T
    s = seed_of(w, h, noc, u8)
    flow, guide, mask = X.thin_flow(w, h, 2, s, 2.0), X.thin_images(w, h, 2, noc, u8, s), X.thin_mask(w, h, 2, s)
    codes = T.assert_dense_matches(flow, guide, mask, 3, R.spatial_table(3, 1.5), 40.0, 2)
    assert set(np.unique(codes)) >= {0, 1}
    T.assert_dense_matches(flow, guide, None, 7, None, 8.0, 1)


@thin
@pytest.mark.parametrize("noc,block,refine", [(1, 8, 0), (3, 32, 0), (1, 32, 2)])
def test_thin_block_motion(w, h, noc, block, refine):
    """the restatement walks the blocks in Python (2048 of them at block 8): the refinement is tested at block 32 only, where a case
    stays within a few seconds"""
    import blockmotion_ref as R
    import test_gpu_blockmotion as T
    from flowonthego_amd.blockmotion import block_motion
    cur, ref, flow, mask = R.scene(h, w, noc, seed_of(w, h, noc), n=2)
    flow = X.edge_specials(flow)
    got = block_motion(dev(cur), dev(ref), dev(flow), mask=dev(mask), block=block, refine=refine, pred=True, stats=True)
    torch.cuda.synchronize()
    T.assert_equals_restatement(got, R.block_motion(cur, ref, flow, mask, block, refine), (w, h, noc, block, refine))


@thin
def test_thin_chain(w, h):
    import chain_ref as R
    import test_gpu_chain as T
    from flowonthego_amd.chain import chain, track_points
    s = seed_of(w, h)
    n_seq, steps_n = 2, 3
    F = X.thin_flow(w, h, n_seq * steps_n, s, 1.5).reshape(n_seq, steps_n, h, w, 2)
    B = X.edge_specials(-F.reshape(-1, h, w, 2) + X.thin_flow(w, h, n_seq * steps_n, s + 1, 0.2, specials=False), 3).reshape(F.shape)
    F[:, 1:, :, :, :] = X.thin_flow(w, h, n_seq * (steps_n - 1), s + 2, 1.5, specials=False).reshape(n_seq, steps_n - 1, h, w, 2)
    F[0, 1].reshape(-1, 2)[-3:] = (np.nan, 0.0)                     # a later step has its specials at the end of the frame
    pts = R.make_points(w, h, n_seq, 300)
    pts[:, -1] = (w - 1, h - 1)
    for bw in (None, B):
        got = chain(dev(F), dev(bw), stats=True)
        traj, pc, ps, pst = track_points(dev(pts), dev(F), dev(bw), stats=True)
        torch.cuda.synchronize()
        want = [R.chain(F[q], None if bw is None else bw[q]) for q in range(n_seq)]
        for j, nm in enumerate(("total", "code", "steps")):
            assert T.same(got[j], np.stack([r[j] for r in want])), (nm, bw is not None)
        assert T.same(got[3], np.stack([R.stats(r[1], r[2]) for r in want]).astype(np.int64))
        wp = [R.track(pts[q], F[q], None if bw is None else bw[q]) for q in range(n_seq)]
        assert T.same_traj(traj, np.stack([r[0] for r in wp])) and T.same(pc, np.stack([r[1] for r in wp]))
        assert T.same(ps, np.stack([r[2] for r in wp])) and T.same(pst, np.stack([R.stats(r[1], r[2]) for r in wp]).astype(np.int64))
    assert set(np.unique(np.stack([r[1] for r in want]))) >= {0, 2, 3}


def motion_scene(w, h, s):
    import motion_ref as R
    sc = [R.make_scene(w, h, seed=s + i) for i in range(2)]
    return X.edge_specials(np.stack([c[0] for c in sc])), np.stack([c[1] for c in sc])


@thin
def test_thin_motion_fit(w, h):
    import motion_ref as R
    import test_gpu_motion as T
    flow, mask = motion_scene(w, h, seed_of(w, h))
    mask.reshape(2, -1)[:, -1] = (0, 1)
    dF, dM = dev(flow), dev(mask)
    for model in (0, 1, 2):
        for masked, iters in ((False, 0), (True, 3)):
            got = T.gpu_fit(dF, dM if masked else None, model, iters)
            torch.cuda.synchronize()
            want = [R.fit(flow[i], mask[i] if masked else None, model, iters) for i in range(2)]
            for k in T.KEYS:
                assert T.same(got[k], np.stack([r[k] for r in want])), (model, masked, iters, k)


@thin
def test_thin_layers(w, h):
    import layers_ref as LR
    import motion_ref as R
    import test_gpu_layers as T
    import flowonthego_amd as F
    s = seed_of(w, h)
    flow = X.edge_specials(np.stack([LR.three_motions(w, h, seed=s)[0], R.make_scene(w, h, seed=s + 1)[0]]))
    mask = np.stack([np.zeros((h, w), np.uint8), R.make_scene(w, h, seed=s + 1)[1]])
    for K, model, iters, rounds, thresh in ((3, 2, 1, 2, 1.0), (2, 0, 0, 1, 2.5), (1, 1, 2, 0, 1.0)):
        kw = dict(layers=K, model=model, iters=iters, rounds=rounds, thresh=thresh)
        got = F.motion_layers(dev(flow), dev(mask), **dict(kw, model=R.MODELS[model]), **T.ALL)
        torch.cuda.synchronize()
        T.check(got, LR.layers_batch(flow, mask, **kw), (w, h, kw))


@thin
def test_thin_components(w, h):
    import objects_ref as R
    import test_gpu_objects as T
    s = seed_of(w, h)
    rng = np.random.default_rng(s)
    code = X.thin_runs(w, h, 2)
    code[(code == 0) & (rng.random(code.shape) < 0.1)] = 2                       # a second foreground code, and bytes beyond the set
    code[(code == 0) & (rng.random(code.shape) < 0.1)] = 9
    values = X.thin_flow(w, h, 2, s)
    for conn in (4, 8):
        for fg, val, mo in (((1,), values, 64), ((1, 2), None, 4096)):
            got = T.gpu(code, fg, conn, val, 1, mo)
            want = R.components_batch(code, R.fg_set(fg), conn, val, 1, mo)
            T.assert_same(got, want, (w, h, conn, fg))
    runs = R.components_batch(X.thin_runs(w, h, 2), 2, 8, None, 1, 64)["objects"]
    assert (runs[:, :, 1] == 1).any() and (runs[:, :, 1] > max(w, h) - 200).any()  # the single pixel and the run over every tile edge
    assert (runs[:, :, 4 if w > h else 5] == max(w, h) - 1).any()                 # a run that ends in the last column (row)


@thin
def test_thin_tracks(w, h):
    import tracks_ref as R
    import test_gpu_tracks as T
    from flowonthego_amd.tracks import object_overlap, track_objects
    s = seed_of(w, h)
    K = 16
    ids, objects = R.labelled(X.thin_runs(w, h, 3), K)
    flows, masks = X.thin_flow(w, h, 2, s, 2.0), X.thin_mask(w, h, 2, s)
    for m in (None, masks):
        got = object_overlap(dev(ids[:-1]), dev(ids[1:]), dev(flows), dev(m), ka=K, kb=K)
        torch.cuda.synchronize()
        T.assert_equal(got, R.overlap_batch(ids[:-1], ids[1:], flows, m, K, K), (w, h, m is not None))
    want = R.track_objects(ids, objects, flows, masks, 1, 0, 64)
    track, table, st = track_objects(dev(ids), dev(objects), dev(flows), dev(masks), min_votes=1, min_frac=0.0, max_tracks=64, stats=True)
    torch.cuda.synchronize()
    T.assert_equal((track, table, st), (want["track"], want["tracks"], want["stats"]), (w, h, "tracks"))
    assert want["sent"][..., 0].sum() > 0 and want["sent"][..., 3].sum() > 0 and want["stats"][2] > 0


@thin
def test_thin_histograms(w, h):
    import histograms_ref as R
    import test_gpu_histograms as T
    from flowonthego_amd.histograms import motion_histograms
    flow, mask, params, ids = T.scene(h, w)
    flow = X.edge_specials(flow)
    for cell, masked, moved in ((8, True, True), (32, False, False)):
        m, p = (mask if masked else None), (params if moved else None)
        got = motion_histograms(dev(flow), dev(m), dev(p), cell, ids=dev(ids), rows=T.K)
        torch.cuda.synchronize()
        T.assert_equal(got, R.histograms(flow, m, p, cell, R.THRESH256, ids, T.K), (w, h, cell))


@thin
@two_kinds
def test_thin_motion_blur(w, h, noc, u8):
    import motionblur_ref as R
    import test_gpu_motionblur as T
    from flowonthego_amd.motionblur import motion_blur
    flow, mask, frames = T.scene(h, w)
    flow = X.edge_specials(flow)
    fr = frames["%s-%d" % ("u8" if u8 else "f32", noc)]
    for m in (None, mask):
        got = motion_blur(dev(fr), dev(flow), dev(m), **T.ALL)
        torch.cuda.synchronize()
        T.assert_equal(got, R.blur(fr, flow, m), (w, h, noc, u8, m is not None))


def thin_canvas(w, h):
    """a plate canvas (W, H, ox, oy) around a thin frame: the long side as it is (16384 is the largest canvas too), the short one
    with a margin"""
    return (w if w > h else w + 4, h if h > w else h + 3, 0 if w > h else 2, 0 if h > w else 1)


@thin
@two_kinds
def test_thin_plate(w, h, noc, u8):
    import plate_ref as R
    import test_gpu_plate as T
    s = seed_of(w, h, noc, u8)
    rng = np.random.default_rng(s)
    W, H, ox, oy = canvas = thin_canvas(w, h)
    n, K, nframes = 2, 3, 4
    frames = X.thin_images(w, h, nframes, noc, u8, s)
    index = np.array([[0, 2, 3], [1, -1, 2]])
    flows = X.thin_flow(W, H, n * K, s, 2.0).reshape(n, K, H, W, 2)
    flows[..., 0] += f32(ox)
    flows[..., 1] += f32(oy)
    motions = rng.normal(0, 1e-5, (n, K, 6))
    motions[..., [2, 5]] = rng.normal(0, 1.5, (n, K, 2))
    if min(w, h) == 1:                                                # one line: a motion with a part across it leaves the frame
        motions[..., [0, 1, 3, 4]] = 0
        motions[..., 5 if h == 1 else 2] = 0
    occ = X.thin_mask(W, H, n * K, s).reshape(n, K, H, W)
    exclude = (rng.random((nframes, h, w)) < 0.08).astype(np.uint8)
    ref = X.thin_images(W, H, n, noc, u8, s + 1)
    for mode in (0, 1):
        kw = dict(occ=occ, exclude=exclude, min_count=mode + 1, fill=7.25, ref=ref)
        for src in (dict(flows=flows), dict(motions=motions)):
            got = T.gpu_plate(frames, index, canvas, mode=("median", "mean")[mode], **kw, **src)
            sk = {("params" if k == "motions" else k): v for k, v in src.items()}
            T.assert_equal_to_ref(got, R.plate(frames, index, W, H, ox, oy, mode=mode, **kw, **sk), (w, h, mode, list(src)))


@thin
@two_kinds
def test_thin_subtract(w, h, noc, u8):
    import test_gpu_subtract as T
    canvas = thin_canvas(w, h)
    frames, plates, index, flows, motions, pcode, mask = T.case(noc, u8, seed_of(w, h, noc, u8), (h, w), canvas, 2, 2)
    flows = X.edge_specials(flows)
    for source, r in (("dense", 1), ("motion", 2), ("dense", 0)):
        src = T.sources(flows, motions)[source]
        kw = dict(plate_code=pcode, mask=mask, low=20.0, high=60.0, window=r)
        T.assert_same(T.gpu(frames, plates, canvas, src, index, **kw), T.ref(frames, plates, canvas, src, index, **kw), (w, h, source, r))


@thin
@two_kinds
def test_thin_erase(w, h, noc, u8):
    import test_gpu_erase as T
    import test_gpu_subtract as S
    canvas = thin_canvas(w, h)
    frames, plates, index, flows, motions, pcode, mask = S.case(noc, u8, seed_of(w, h, noc, u8), (h, w), canvas, 2, 2)
    flows = X.edge_specials(flows)
    runs = X.thin_runs(w, h, 2)
    rm = np.zeros_like(runs)
    rm[0] = runs[0] * (np.arange(h * w).reshape(h, w) % 211 < 40)    # pieces of every run, on both sides of many tile edges
    rm[1] = runs[1] * 7 * (np.arange(h * w).reshape(h, w) % 1999 > 1900)
    rm[1, h - 1, w - 1] = 255
    for source, G, Fe in (("dense", 2, 3), ("motion", 8, 8), ("dense", 0, 1)):
        src = S.sources(flows, motions)[source]
        kw = dict(plate_code=pcode, mask=mask, grow=G, feather=Fe)
        want = T.ref(frames, plates, rm, canvas, src, index, **kw)
        T.assert_same(T.gpu(frames, plates, rm, canvas, src, index, **kw), want, (w, h, source, G, Fe))
        assert want[3][:, 6].min() > 0


@thin
def test_thin_morphology(w, h):
    import test_gpu_morph as T
    rng = np.random.default_rng(seed_of(w, h))
    P = X.thin_runs(w, h, 2).astype(bool)
    P ^= rng.random(P.shape) < 0.02                                   # pin-holes in the runs, speckle between them
    for fg in (None, (1, 4)):
        x = T.as_bytes(P, fg, seed_of(w, h))
        for stages in ((("erode", 1),), (("dilate", 8),), (("erode", 2), ("dilate", 2)), (("dilate", 8), ("erode", 8))):
            T.assert_chain(x, stages, fg, (w, h))


TALL = 65535 * 16                                                     # the most rows of a 16-row tile grid: gridDim.y = 65535


def test_temporal_at_65535_tile_rows_and_one_row_more():
    """h = 65535 x 16, w = 1 is accepted and equals the restatement; one row more is FOTG_ERR_ARG and nothing is launched"""
    import test_gpu_temporal as T
    s = seed_of(1, TALL)
    n, K = len(T.CENTER), 1
    frames, ref = X.thin_images(1, TALL, T.T, 1, True, s), X.thin_images(1, TALL, n, 1, True, s + 1)
    flows = X.thin_flow(1, TALL, n * K, s, 0.4).reshape(n, K, TALL, 1, 2)
    used = T.assert_dense_matches(frames, K, flows, None, 40.0, None, ref)
    assert 0 in used and K in used
    st = T._raw(h=TALL + 1, w=1)                                     # buffers of the larger size, outputs pre-filled
    assert T._call(st) == T.FOTG_ERR_ARG
    torch.cuda.synchronize()
    assert bool((st["dst"] == -7.0).all()) and bool((st["used"] == 99).all()) and bool((st["stats"] == -7.0).all())
    assert T._call(st, h=TALL) == 0
    torch.cuda.synchronize()
    assert bool((st["dst"].flatten()[:2 * TALL] != -7.0).all())


def test_flow_filter_at_65535_tile_rows_and_one_row_more():
    """h = 65535 x 16, w = 1 is accepted and equals the restatement; one row more is FOTG_ERR_ARG and nothing is launched"""
    import test_gpu_flowfilter as T
    s = seed_of(1, TALL)
    flow, guide, mask = X.thin_flow(1, TALL, 2, s, 2.0), X.thin_images(1, TALL, 2, 1, False, s), X.thin_mask(1, TALL, 2, s)
    codes = T.assert_dense_matches(flow, guide, mask, 2, None, 40.0, 2)
    assert set(np.unique(codes)) >= {0, 1}
    st = T._raw(h=TALL + 1, w=1)
    assert T._call(st) == T.FOTG_ERR_ARG
    torch.cuda.synchronize()
    assert bool((st["out"] == -7.0).all()) and bool((st["code"] == 99).all()) and bool((st["stats"] == -7.0).all())
    assert T._call(st, h=TALL) == 0
    torch.cuda.synchronize()
    assert bool((st["code"].flatten()[:2 * TALL] != 99).all())


# ---- 4. offsets beyond 2^31 elements -------------------------------------------------------------------------------------------------
# One call per add-on whose largest per-pixel array passes 2^31 elements, compared chunk by chunk (8 images) with the same call on
# the chunk alone (the pattern of test_fused_dst_beyond_2_pow_31_bytes in tests/test_gpu_warp.py).  The inputs are random all the
# way (no image repeats, so a wrapped offset cannot land on equal data) and the last image holds NaN vectors or a lone foreground
# pixel in its last row.
BW, BH = 4096, 2048                                                  # 2^23 pixels an image
N_BYTE, N_FLOW, N_RGB = 264, 136, 88                                  # images for a byte map, a two-float flow, a three-byte frame
CHUNK = 8
assert N_BYTE * BW * BH > 2 ** 31 and N_FLOW * BW * BH * 2 > 2 ** 31 and N_RGB * BW * BH * 3 > 2 ** 31


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def big_flow(n, g, scale=2.0, shape=None):
    f = torch.randn(shape or (n, BH, BW, 2), device="cuda", generator=g)
    f *= scale
    f.view(-1, BH, BW, 2)[-1, BH - 1, BW - 8:] = float("nan")         # the last image: NaN vectors at the end of its last row
    return f


def big_bytes(shape, g, top=256):
    return torch.randint(0, top, shape, device="cuda", dtype=torch.uint8, generator=g)


def big_mask(shape, g, one_in=10):
    """a uint8 map with a non-zero byte in about one pixel of one_in"""
    return (big_bytes(shape, g, one_in) == 0).to(torch.uint8)


def tbits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def assert_chunks(call, n, step=CHUNK):
    """call(lo, hi) runs the add-on on the images lo .. hi - 1 and returns a tuple of tensors with the batch first"""
    whole = call(0, n)
    torch.cuda.synchronize()
    for s in range(0, n, step):
        part = call(s, min(s + step, n))
        for k, (a, b) in enumerate(zip(whole, part)):
            assert a.dtype == b.dtype and torch.equal(tbits(a[s:s + step]), tbits(b)), (s, k)
        del part
    return whole


def test_offsets_interp():
    from flowonthego_amd.interp import interpolate
    g = gen(41)
    n = N_RGB
    I0, I1 = big_bytes((n, BH, BW, 3), g), big_bytes((n, BH, BW, 3), g)
    F, B = big_flow(n, g), big_flow(n, g)
    assert I0.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: interpolate(I0[a:b], I1[a:b], F[a:b], B[a:b], 0.5, stats=True), n)
    assert not torch.equal(out[1][n - 1], out[1][n - 2])
    del I0, I1, F, B, out
    torch.cuda.synchronize()


def test_offsets_temporal():
    from flowonthego_amd.temporal import temporal_filter
    g = gen(42)
    n, nframes = N_FLOW, 8
    frames = big_bytes((nframes, BH, BW), g)
    flows = big_flow(n, g, 0.5).view(n, 1, BH, BW, 2)
    assert flows.numel() > 2 ** 31
    cen, nbr = [k % nframes for k in range(n)], [[(3 * k + 1) % nframes] for k in range(n)]
    out = assert_chunks(lambda a, b: temporal_filter(frames, cen[a:b], nbr[a:b], flows[a:b], tau=200.0, stats=True), n)
    assert float(out[2][n - 1, 0]) > 0
    del frames, flows, out
    torch.cuda.synchronize()


def test_offsets_flow_filter():
    from flowonthego_amd.flowfilter import filter_flow
    g = gen(43)
    n = N_FLOW
    flow, guide = big_flow(n, g), big_bytes((n, BH, BW), g)
    assert flow.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: filter_flow(flow[a:b], guide[a:b], radius=1, tau=300.0, stats=True), n)
    assert float(out[2][n - 1, 0]) > 0
    del flow, guide, out
    torch.cuda.synchronize()


def test_offsets_block_motion():
    from flowonthego_amd.blockmotion import block_motion
    g = gen(44)
    n = N_RGB
    cur, ref, flow = big_bytes((n, BH, BW, 3), g), big_bytes((n, BH, BW, 3), g), big_flow(n, g)
    assert cur.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: block_motion(cur[a:b], ref[a:b], flow[a:b], block=32, refine=0, pred=True, stats=True), n)
    assert int(out[4][n - 1, 0]) > 0
    del cur, ref, flow, out
    torch.cuda.synchronize()


def test_offsets_chain():
    from flowonthego_amd.chain import chain
    g = gen(45)
    n, steps_n = N_FLOW // 2, 2
    flows = big_flow(n * steps_n, g, 1.0).view(n, steps_n, BH, BW, 2)
    assert flows.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: chain(flows[a:b], stats=True), n)
    assert int(out[3][n - 1, 3]) > 0                                  # the NaN vectors of the last sequence's last step
    del flows, out
    torch.cuda.synchronize()


def test_offsets_motion_fit():
    from flowonthego_amd.motion import fit_motion
    g = gen(46)
    n = N_FLOW
    flow, mask = big_flow(n, g), big_mask((n, BH, BW), g)
    assert flow.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: fit_motion(flow[a:b], mask[a:b], "affine", 1, 3.0, code=True, residual=True, stats=True, sums=True), n)
    assert int(out[3][n - 1, 3]) == 8
    del flow, mask, out
    torch.cuda.synchronize()


def test_offsets_layers():
    from flowonthego_amd.layers import motion_layers
    g = gen(47)
    n = N_FLOW
    flow = big_flow(n, g)
    assert flow.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: motion_layers(flow[a:b], None, 2, "translation", 1, 1, 3.0, labels=True, records=True, stats=True,
                                                   sums=True), n)
    assert int(out[3][n - 1, 2]) == 8
    del flow, out
    torch.cuda.synchronize()


def test_offsets_components():
    from flowonthego_amd.objects import label_components
    g = gen(48)
    n = N_BYTE
    code = big_mask((n, BH, BW), g, 3)                               # a third of the pixels: many small components
    code[n - 1, BH - 1] = 0
    code[n - 1, BH - 1, BW - 1] = 1                                   # a lone foreground pixel at the very end
    assert code.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: label_components(code[a:b], (1,), 8, None, 1, 64, labels=True, ids=True, stats=True), n)
    assert int(out[1][n - 1, BH - 1, BW - 1]) == BH * BW - 1
    del code, out
    torch.cuda.synchronize()


def test_offsets_object_overlap():
    from flowonthego_amd.tracks import object_overlap
    g = gen(49)
    n = N_FLOW
    flow = big_flow(n, g)
    ids_a = torch.randint(-1, 8, (n, BH, BW), device="cuda", dtype=torch.int32, generator=g)
    ids_b = torch.randint(-1, 8, (n, BH, BW), device="cuda", dtype=torch.int32, generator=g)
    assert flow.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: object_overlap(ids_a[a:b], ids_b[a:b], flow[a:b], None, 8, 8), n)
    assert int(out[1][n - 1, :, 3].sum()) > 0
    del flow, ids_a, ids_b, out
    torch.cuda.synchronize()


def test_offsets_histograms():
    from flowonthego_amd.histograms import motion_histograms
    g = gen(50)
    n = N_FLOW
    flow = big_flow(n, g)
    assert flow.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: (motion_histograms(flow[a:b], cell=32),), n)
    assert int(out[0][n - 1, -1, -1, 27]) == 8                        # n_bad of the last cell of the last image
    del flow, out
    torch.cuda.synchronize()


def test_offsets_motion_blur():
    from flowonthego_amd.motionblur import motion_blur
    g = gen(51)
    n = N_RGB
    frame, flow = big_bytes((n, BH, BW, 3), g), big_flow(n, g, 4.0)
    assert frame.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: motion_blur(frame[a:b], flow[a:b], None, 0.5, 8, code=True, vectors=True, stats=True), n)
    assert int(out[3][n - 1, 3]) >= 8
    del frame, flow, out
    torch.cuda.synchronize()


def test_offsets_plate():
    from flowonthego_amd.plate import background_plate
    g = gen(52)
    n, K, nframes = N_FLOW // 2, 2, 4
    frames = big_bytes((nframes, BH, BW), g)
    flows = big_flow(n * K, g, 1.0).view(n, K, BH, BW, 2)
    index = [[k % nframes, (k + 1 + k // nframes) % nframes] for k in range(n)]
    assert flows.numel() > 2 ** 31
    out = assert_chunks(lambda a, b: background_plate(frames, index[a:b], flows=flows[a:b], count=True, code=True, stats=True), n)
    last = out[1][n - 1]                                              # the second sample has NaN vectors at the end of the last row
    assert int(last[BH - 1, BW - 8:].max()) <= 1 and int(last.max()) == 2
    del frames, flows, out
    torch.cuda.synchronize()


def plate_inputs(g, n):
    frames, plate, flows = big_bytes((n, BH, BW, 3), g), big_bytes((2, BH, BW, 3), g), big_flow(n, g, 1.0)
    index = [(k // 3) % 2 for k in range(n)]
    assert frames.numel() > 2 ** 31
    return frames, plate, flows, index


def test_offsets_subtract():
    from flowonthego_amd.subtract import subtract_background
    n = N_RGB
    frames, plate, flows, index = plate_inputs(gen(53), n)
    out = assert_chunks(lambda a, b: subtract_background(frames[a:b], plate, flows=flows[a:b], index=index[a:b], low=60.0, high=90.0,
                                                         code=True, diff=True, stats=True), n)
    assert int(out[2][n - 1, 3]) >= 8
    del frames, plate, flows, out
    torch.cuda.synchronize()


def test_offsets_erase():
    from flowonthego_amd.erase import remove_objects
    n = N_RGB
    g = gen(54)
    frames, plate, flows, index = plate_inputs(g, n)
    remove = big_mask((n, BH, BW), g, 200)
    remove[n - 1, BH - 1, BW - 1] = 1
    out = assert_chunks(lambda a, b: remove_objects(frames[a:b], plate, remove[a:b], flows=flows[a:b], index=index[a:b], grow=2, feather=3,
                                                    dst=True, code=True, alpha=True, stats=True), n)
    assert int(out[2][n - 1, BH - 1, BW - 1]) == 256 and int(out[1][n - 1, BH - 1, BW - 1]) == 3
    del frames, plate, flows, remove, out
    torch.cuda.synchronize()


def test_offsets_morphology():
    from flowonthego_amd.morph import morphology
    g = gen(55)
    n = N_BYTE
    x = big_mask((n, BH, BW), g, 2)
    x[n - 1, BH - 9:] = 0
    x[n - 1, BH - 1, BW - 1] = 1                                      # a lone set pixel at the very end: a dilation grows it, an opening deletes it
    assert x.numel() > 2 ** 31
    for op, r in (("dilate", 2), ("open", 1)):
        out = assert_chunks(lambda a, b: morphology(x[a:b], op, r, stats=True), n)
        assert int(out[0][n - 1, BH - 1, BW - 3]) == (1 if op == "dilate" else 0) and int(out[0][n - 1, BH - 1, BW - 1]) == (op == "dilate")
        del out
    del x
    torch.cuda.synchronize()


# ---- 3. the largest batch ------------------------------------------------------------------------------------------------------------
# n = 65535 is gridDim.y / gridDim.z's limit (and the limit of the source index in interp's key).  One C-ABI call per entry point that
# documents it, 65535 images of 3 x 2 pixels made of five distinct ones tiled along the batch: image k must equal the restatement
# of image k mod 5, checked by one comparison on the device.  Every output is pre-filled and sits between guard elements.
NB, W3, H3 = 65535, 3, 2
REP = NB // 5
GUARD = 16
FILL = {torch.float32: -7.0, torch.float64: -7.0, torch.uint8: 249, torch.int16: -7, torch.int32: -7, torch.int64: -7}
assert REP * 5 == NB


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def cints(v):
    return (C.c_int * len(v))(*[int(i) for i in v])


def tile5(a):
    """(5, ...) on the host -> (65535, ...) on the device, image k a copy of image k mod 5"""
    t = dev(np.asarray(a))
    return t.repeat((REP,) + (1,) * (t.dim() - 1)).contiguous()


class Guarded:
    """an output of the given shape inside a larger pre-filled allocation, GUARD elements to either side"""

    def __init__(self, shape, dtype):
        self.numel = int(np.prod(shape))
        self.fillv = FILL[dtype]
        self.big = torch.full((self.numel + 2 * GUARD,), self.fillv, dtype=dtype, device="cuda")
        self.out = self.big[GUARD:GUARD + self.numel].view(shape)

    def clean(self):
        return bool((self.big[:GUARD] == self.fillv).all()) and bool((self.big[GUARD + self.numel:] == self.fillv).all())


def outputs(want5):
    """a Guarded per expected array (5, ...), of its dtype (uint32 and uint64 as their signed twins)"""
    twin = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    want5 = [np.ascontiguousarray(a).astype(twin.get(a.dtype, a.dtype), copy=False) for a in want5]
    return want5, [Guarded((NB,) + a.shape[1:], torch.from_numpy(a[:1]).dtype) for a in want5]


def assert_tiled(outs, want5, tol5=None, what=""):
    """every output equals its five expected images tiled, bit for bit (a NaN where a NaN is expected; within tol5[k] where that is
    given: the residual sums), and no guard element was touched"""
    torch.cuda.synchronize()
    for k, (o, w5) in enumerate(zip(outs, want5)):
        want = tile5(w5)
        got = o.out
        assert got.shape == want.shape and got.dtype == want.dtype, (what, k, got.shape, want.shape, got.dtype, want.dtype)
        if tol5 is not None and tol5[k] is not None:
            ok = (got - want).abs() <= tile5(tol5[k])
        else:
            ok = tbits(got) == tbits(want)
            if got.is_floating_point():
                ok |= torch.isnan(got) & torch.isnan(want)
        assert bool(ok.all()), (what, k, torch.nonzero(~ok)[:4].tolist())
        assert o.clean(), (what, k, "guard")
        del want, ok


def sum_tol(stats5, cols, nterms):
    """the bound of tests/test_gpu_warp.py on a sum of nterms non-negative doubles in any order, nterms 2^-53 sum, for the columns
    `cols` of stats (5, C); zero (bit for bit) for the other columns"""
    tol = np.zeros_like(stats5)
    tol[:, cols] = nterms * 2.0 ** -53 * np.abs(stats5[:, cols])
    return tol


def small_flow(seed, lead=(5,), scale=1.0):
    """flows (lead..., 2, 3, 2) of about a pixel, with a NaN, an infinity, a 5000 px vector and one of exactly -4096 px"""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal(lead + (H3, W3, 2)) * scale).astype(f32)
    f[..., ::2, ::2, :] = np.round(f[..., ::2, ::2, :] * 4) / 4
    g = f.reshape(-1, H3 * W3, 2)
    for i in range(len(g)):
        g[i, (i + seed) % 6] = X.SPECIALS[(i + seed) % len(X.SPECIALS)]
    g[-1, 5] = (0.0, -4096.0)
    return f


def small_images(seed, noc, u8, count=5):
    return X.thin_images(W3, H3, count, noc, u8, seed)


def small_mask(seed, lead=(5,)):
    return np.random.default_rng(seed).choice(np.array([0, 0, 0, 0, 1, 3, 200], np.uint8), lead + (H3, W3))


def stack5(res, j):
    return np.stack([r[j] for r in res])


def test_batch_65535_warp():
    import warp_ref as R
    L = _F().lib()
    for u8, noc, fn in ((False, 1, L.fotg_warp), (True, 3, L.fotg_warp_u8)):
        src5, ref5, flow5, occ5 = small_images(1, noc, u8), small_images(2, noc, u8), small_flow(3), small_mask(4)
        res = [R.warp(src5[k], flow5[k], ref5[k], occ5[k], 1, 17.5, terms=True) for k in range(5)]
        want5, outs = outputs([stack5(res, 0), stack5(res, 1), stack5(res, 2)])
        src, ref, flow, occ = tile5(src5), tile5(ref5), tile5(flow5), tile5(occ5)
        assert fn(0, NB, p(src), p(flow), W3, H3, noc, p(ref), p(occ), 1, 17.5, *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, [None, None, sum_tol(want5[2], [4, 5], len(res[0][3]))], ("warp", u8))


def test_batch_65535_fb_check():
    import fbcheck_ref as R
    L = _F().lib()
    fw5 = small_flow(5)
    bw5 = (-fw5 + small_flow(6, scale=0.2)).astype(f32)
    m5, mb5 = R.fb_check(fw5, bw5)
    want5, outs = outputs([m5, mb5, R.counts(m5, mb5).astype(np.int32)])
    fw, bw = tile5(fw5), tile5(bw5)
    assert L.fotg_fb_check(0, NB, p(fw), p(bw), W3, H3, 0.01, 0.5, *(p(o.out) for o in outs), None) == 0
    assert_tiled(outs, want5, None, "fb_check")


def test_batch_65535_interp():
    """65535 is also the largest source index the 32-bit field of the key holds"""
    import interp_ref as R
    L = _F().lib()
    for u8, noc, fn in ((False, 3, L.fotg_interp), (True, 1, L.fotg_interp_u8)):
        I05, I15, ref5 = small_images(7, noc, u8), small_images(8, noc, u8), small_images(9, noc, u8)
        F5, B5, mF5, mB5 = small_flow(10), small_flow(11), small_mask(12), small_mask(13)
        res = [R.interp(I05[k], I15[k], F5[k], B5[k], 0.25, mF5[k], mB5[k], ref5[k], terms=True) for k in range(5)]
        want5, outs = outputs([stack5(res, 0), stack5(res, 1), stack5(res, 2)])
        t = [tile5(a) for a in (I05, I15, F5, B5, mF5, mB5, ref5)]
        assert fn(0, NB, p(t[0]), p(t[1]), p(t[2]), p(t[3]), W3, H3, noc, 0.25, p(t[4]), p(t[5]), 0.01, 0.5, p(t[6]),
                  *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, [None, None, sum_tol(want5[2], [4, 5], len(res[0][3]))], ("interp", u8))


def test_batch_65535_chain_and_points():
    import chain_ref as R
    L = _F().lib()
    steps_n, P = 2, 4
    F5 = small_flow(14, (5, steps_n), 0.7)
    B5 = (-F5 + small_flow(15, (5, steps_n), 0.1)).astype(f32)
    res = [R.chain(F5[q], B5[q]) for q in range(5)]
    st5 = np.stack([R.stats(r[1], r[2]) for r in res]).astype(np.int64)
    want5, outs = outputs([stack5(res, 0), stack5(res, 1), stack5(res, 2).astype(np.int32), st5])
    F, B = tile5(F5), tile5(B5)
    assert L.fotg_flow_chain(0, NB, steps_n, p(F), p(B), W3, H3, 0.01, 0.5, *(p(o.out) for o in outs), None) == 0
    assert_tiled(outs, want5, None, "chain")
    pts5 = R.make_points(W3, H3, 5, P)
    pts5[:, 0] = (1.0, 0.5)
    rp = [R.track(pts5[q], F5[q], B5[q]) for q in range(5)]
    sp5 = np.stack([R.stats(r[1], r[2]) for r in rp]).astype(np.int64)
    want5, outs = outputs([stack5(rp, 0), stack5(rp, 1), stack5(rp, 2).astype(np.int32), sp5])
    pts = tile5(pts5)
    assert L.fotg_track_points(0, NB, steps_n, p(F), p(B), W3, H3, 0.01, 0.5, P, p(pts), *(p(o.out) for o in outs), None) == 0
    assert_tiled(outs, want5, None, "track_points")


def test_batch_65535_motion_fit_and_motion_flow():
    import motion_ref as R
    L = _F().lib()
    flow5, mask5 = small_flow(16), small_mask(17)
    mask5[2] = 1                                                      # an image with everything masked: unfitted, the others unaffected
    for model, iters in ((2, 0), (0, 2)):
        res = [R.fit(flow5[k], mask5[k], model, iters, 1.0) for k in range(5)]
        want5, outs = outputs([np.stack([r[k] for r in res]) for k in ("params", "code", "residual", "stats", "sums")])
        flow, mask = tile5(flow5), tile5(mask5)
        assert L.fotg_fit_motion(0, NB, p(flow), p(mask), W3, H3, model, iters, 1.0, *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("fit_motion", model, iters))
    P5 = np.array([[0.01, -0.02, 3.5, 0.03, 0.005, -1.25], [0, 0, 0, 0, 0, 0], [0.5, 0, -1, 0, 0.5, 1], [0, 0, 4096, 0, 0, -4096],
                   [1e-3, 1e-3, 0.125, -1e-3, 1e-3, 0.25]], np.float64)
    want5, outs = outputs([np.stack([R.motion_flow(P, W3, H3) for P in P5])])
    prm = tile5(P5)
    assert L.fotg_motion_flow(0, NB, p(prm), W3, H3, p(outs[0].out), None) == 0
    assert_tiled(outs, want5, None, "motion_flow")


def test_batch_65535_layers():
    import layers_ref as R
    L = _F().lib()
    flow5, mask5 = small_flow(18, scale=2.0), small_mask(19)
    kw = dict(layers=2, model=0, iters=1, rounds=1, thresh=1.0)
    res = [R.layers(flow5[k], mask5[k], **kw) for k in range(5)]
    want5, outs = outputs([np.stack([r[k] for r in res]) for k in ("params", "labels", "residual", "records", "stats", "sums")])
    flow, mask = tile5(flow5), tile5(mask5)
    assert L.fotg_motion_layers(0, NB, p(flow), p(mask), W3, H3, 2, 0, 1, 1, 1.0, None, *(p(o.out) for o in outs), None) == 0
    assert_tiled(outs, want5, None, "layers")


def test_batch_65535_components():
    import objects_ref as R
    L = _F().lib()
    code5 = np.array([[[1, 0, 1], [0, 1, 0]], [[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 0]], [[1, 0, 2], [9, 0, 1]], [[0, 1, 0], [1, 0, 1]]], np.uint8)
    values5 = small_flow(20, scale=3.0)
    for conn in (4, 8):
        res = [R.components(code5[k], R.fg_set((1,)), conn, values5[k], 1, 4) for k in range(5)]
        want5, outs = outputs([np.stack([r[k] for r in res]) for k in ("labels", "ids", "objects", "stats")])
        code, values = tile5(code5), tile5(values5)
        assert L.fotg_label_components(0, NB, p(code), W3, H3, R.fg_set((1,)), conn, p(values), 1, 4, *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("components", conn))


def test_batch_65535_temporal():
    import temporal_ref as R
    L = _F().lib()
    K, nframes = 2, 5
    for u8, noc, fn in ((False, 1, L.fotg_temporal_filter), (True, 3, L.fotg_temporal_filter_u8)):
        frames, ref5 = small_images(21, noc, u8, nframes), small_images(22, noc, u8)
        flows5, masks5 = small_flow(23, (5, K), 0.3), small_mask(24, (5, K))
        cen5, nbr5, gains = [0, 1, 2, 3, 4], [[1, 3], [2, -1], [3, 0], [4, 1], [0, 4]], [1.0, 0.5]
        res = [R.filter_one(frames, cen5[k], nbr5[k], flows5[k], masks5[k], 40.0, gains, ref5[k], terms=True) for k in range(5)]
        want5, outs = outputs([stack5(res, 0), stack5(res, 1), stack5(res, 2)])
        cen, nbr = cints(cen5 * REP), cints([v for r in nbr5 for v in r] * REP)
        fr, ref, flows, masks = dev(frames), tile5(ref5), tile5(flows5), tile5(masks5)
        assert fn(0, NB, K, nframes, p(fr), W3, H3, noc, cen, nbr, p(flows), p(masks), 40.0, (C.c_float * K)(*gains), p(ref),
                  *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, [None, None, sum_tol(want5[2], [2, 3], len(res[0][3]))], ("temporal", u8))


def test_batch_65535_flow_filter():
    import flowfilter_ref as R
    L = _F().lib()
    for u8, noc, fn in ((False, 3, L.fotg_flow_filter), (True, 1, L.fotg_flow_filter_u8)):
        flow5, guide5, mask5 = small_flow(25, scale=2.0), small_images(26, noc, u8), small_mask(27)
        res = [R.filter_one(flow5[k], guide5[k], mask5[k], 1, None, 40.0, 2, terms=True) for k in range(5)]
        want5, outs = outputs([stack5(res, 0), stack5(res, 1), stack5(res, 2)])
        flow, guide, mask = tile5(flow5), tile5(guide5), tile5(mask5)
        assert fn(0, NB, p(flow), p(guide), W3, H3, noc, p(mask), 1, None, 40.0, 2, *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, [None, None, sum_tol(want5[2], [3], max(1, max(len(r[3]) for r in res)))], ("flow_filter", u8))


def test_batch_65535_block_motion():
    import blockmotion_ref as R
    L = _F().lib()
    for noc, block, refine in ((1, 8, 2), (3, 32, 0)):
        cur5, ref5, flow5, mask5 = small_images(28, noc, True), small_images(29, noc, True), small_flow(30), small_mask(31)
        want5, outs = outputs(list(R.block_motion(cur5, ref5, flow5, mask5, block, refine)))
        cur, ref, flow, mask = tile5(cur5), tile5(ref5), tile5(flow5), tile5(mask5)
        assert L.fotg_block_motion(0, NB, p(cur), p(ref), W3, H3, noc, p(flow), p(mask), block, refine, *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("block_motion", noc, block))


def test_batch_65535_tracks():
    """n = 65535 pairs through the votes and the links, and a sequence of T = 65535 links through the track table"""
    import tracks_ref as R
    L = _F().lib()
    ka, kb = 2, 3
    rng = np.random.default_rng(32)
    a5, b5 = rng.integers(-1, 3, (5, H3, W3)).astype(np.int32), rng.integers(-1, 4, (5, H3, W3)).astype(np.int32)
    flow5, mask5 = small_flow(33), small_mask(34)
    votes5, sent5 = R.overlap_batch(a5, b5, flow5, mask5, ka, kb)
    want5, outs = outputs([votes5, sent5])
    t = [tile5(x) for x in (a5, b5, flow5, mask5)]
    assert L.fotg_object_overlap(0, NB, p(t[0]), p(t[1]), W3, H3, p(t[2]), p(t[3]), ka, kb, *(p(o.out) for o in outs), None) == 0
    assert_tiled(outs, want5, None, "overlap")
    votes5 = rng.integers(0, 5, (5, ka, kb)).astype(np.int32)
    oa5, ob5 = np.zeros((5, ka, 11), np.int64), np.zeros((5, kb, 11), np.int64)
    oa5[..., 1], ob5[..., 1] = rng.integers(1, 9, (5, ka)), rng.integers(1, 9, (5, kb))
    ab5, ba5 = R.links_batch(votes5, oa5, ob5, 2, 64)
    want5, outs = outputs([ab5, ba5])
    t = [tile5(x) for x in (votes5, oa5, ob5)]
    assert L.fotg_object_links(0, NB, p(t[0]), p(t[1]), p(t[2]), ka, kb, 2, 64, *(p(o.out) for o in outs), None) == 0
    assert_tiled(outs, want5, None, "links")
    # the tracks run along the sequence, so the whole of it is restated: K = 2 rows, links of period 5, most tracks short
    K, steps_n, max_tracks = 2, NB, 65536
    objects = np.zeros((steps_n + 1, K, 11), np.int64)
    objects[:, :, 1] = 1 + (np.arange(steps_n + 1)[:, None] + np.arange(K)[None, :]) % 7
    objects[3::11, 1, 1] = 0                                          # unwritten rows now and then
    v5 = rng.integers(0, 4, (5, K, K)).astype(np.int32)
    ab5, ba5 = R.links_batch(v5, objects[:5], objects[1:6], 1, 0)     # (min_frac 0: the links do not depend on the areas)
    link_ab, link_ba = np.tile(ab5, (REP, 1, 1)), np.tile(ba5, (REP, 1, 1))
    track, table, st = R.tracks(objects, link_ab, link_ba, max_tracks)
    outs = [Guarded(track.shape, torch.int32), Guarded(table.shape, torch.int64), Guarded(st.shape, torch.int64)]
    assert L.fotg_object_tracks(0, steps_n, K, p(dev(objects)), p(dev(link_ab)), p(dev(link_ba)), max_tracks, *(p(o.out) for o in outs), None) == 0
    torch.cuda.synchronize()
    for o, w_, nm in zip(outs, (track, table, st), ("track", "tracks", "stats")):
        assert torch.equal(o.out, dev(w_)) and o.clean(), nm
    assert st[0] > 1000 and st[2] > 1000                              # many tracks started, many links followed


def test_batch_65535_histograms():
    import histograms_ref as R
    L = _F().lib()
    flow5, mask5 = small_flow(35, scale=2.0), small_mask(36)
    P5 = np.array([[0.004, -0.011, 1.75, 0.009, 0.006, -2.5], [0, 0, -1, 0, 0, 1], [0.001, 0, np.nan, 0, 0, 0.5], [0, 0, 0, 0, 0, 0],
                   [0, 0, 4000, 0, 0, 0]], np.float64)
    ids5 = np.random.default_rng(37).integers(-2, 4, (5, H3, W3)).astype(np.int32)
    want5, outs = outputs(list(R.histograms(flow5, mask5, P5, 8, R.THRESH256, ids5, 2)))
    flow, mask, prm, ids = tile5(flow5), tile5(mask5), tile5(P5), tile5(ids5)
    assert L.fotg_motion_histograms(0, NB, p(flow), W3, H3, p(mask), p(prm), 8, R.THRESH256, p(outs[0].out), p(ids), 2, p(outs[1].out), None) == 0
    assert_tiled(outs, want5, None, "histograms")


def test_batch_65535_motion_blur():
    import motionblur_ref as R
    L = _F().lib()
    for u8, noc in ((True, 3), (False, 1)):
        frame5, flow5, mask5 = small_images(38, noc, u8), small_flow(39, scale=6.0), small_mask(40)
        want5, outs = outputs(list(R.blur(frame5, flow5, mask5, 128, 32)))
        frame, flow, mask = tile5(frame5), tile5(flow5), tile5(mask5)
        assert L.fotg_motion_blur(0, NB, p(frame), 0 if u8 else 1, noc, p(flow), W3, H3, p(mask), 128, 32, *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("motion_blur", u8))


def test_batch_65535_plate():
    import plate_ref as R
    L = _F().lib()
    K, nframes = 2, 4
    rng = np.random.default_rng(41)
    index5 = np.array([[0, 1], [2, -1], [3, 0], [1, 2], [3, 3]])
    occ5 = small_mask(42, (5, K))
    exclude = (rng.random((nframes, H3, W3)) < 0.1).astype(np.uint8)
    for u8, noc, motion, fn in ((False, 1, False, L.fotg_plate), (True, 3, True, L.fotg_plate_motion_u8)):
        frames, ref5 = small_images(43, noc, u8, nframes), small_images(44, noc, u8)
        if motion:
            src5 = np.zeros((5, K, 6))
            src5[..., [2, 5]] = rng.integers(-2, 3, (5, K, 2)) * 0.5
            kw = dict(params=src5)
        else:
            src5 = small_flow(45, (5, K), 0.6)
            kw = dict(flows=src5)
        res = R.plate(frames, index5, W3, H3, 0, 0, occ=occ5, exclude=exclude, mode=0, min_count=1, fill=7.25, ref=ref5, **kw)
        want5, outs = outputs(list(res[:4]))
        ix = cints([v for r in index5.tolist() for v in r] * REP)
        fr, src, occ, ex, ref = dev(frames), tile5(src5), tile5(occ5), dev(exclude), tile5(ref5)
        assert fn(0, NB, K, nframes, p(fr), W3, H3, noc, ix, p(src), W3, H3, 0, 0, p(occ), p(ex), 0, 1, 7.25, p(ref),
                  *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("plate", u8, motion))


def plate_case5(seed, noc, u8):
    """five frames with a plate each (n = P = 65535 once tiled, plate k for frame k), vectors, motions, the plate's code and a mask"""
    rng = np.random.default_rng(seed)
    frames5, plates5 = small_images(seed, noc, u8), small_images(seed + 1, noc, u8)
    flows5 = small_flow(seed + 2, scale=0.6)
    motions5 = np.zeros((5, 6))
    motions5[:, [2, 5]] = rng.integers(-2, 3, (5, 2)) * 0.5
    pcode5 = rng.choice(np.array([0] * 8 + [1, 2], np.uint8), (5, H3, W3))
    return frames5, plates5, flows5, motions5, pcode5, small_mask(seed + 3)


def test_batch_65535_subtract():
    """n = 65535 frames and P = 65535 plates"""
    import subtract_ref as R
    L = _F().lib()
    for u8, noc, motion, fn in ((False, 3, False, L.fotg_subtract), (True, 1, True, L.fotg_subtract_motion_u8)):
        frames5, plates5, flows5, motions5, pcode5, mask5 = plate_case5(50, noc, u8)
        kw = dict(params=motions5) if motion else dict(flows=flows5)
        want5, outs = outputs(list(R.subtract(frames5, plates5, list(range(5)), 0, 0, plate_code=pcode5, mask=mask5, low=4.0, high=12.0,
                                              window=1, **kw)))
        t = [tile5(a) for a in (frames5, plates5, motions5 if motion else flows5, pcode5, mask5)]
        ix = cints(range(NB))
        assert fn(0, NB, p(t[0]), W3, H3, noc, NB, p(t[1]), W3, H3, 0, 0, ix, p(t[2]), p(t[3]), p(t[4]), 4.0, 12.0, 1,
                  *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("subtract", u8, motion))


def test_batch_65535_erase():
    """n = 65535 frames and P = 65535 plates"""
    import erase_ref as R
    L = _F().lib()
    remove5 = (np.random.default_rng(60).random((5, H3, W3)) < 0.3).astype(np.uint8) * 5
    remove5[2] = 0
    for u8, noc, motion, fn in ((True, 3, False, L.fotg_erase_u8), (False, 1, True, L.fotg_erase_motion)):
        frames5, plates5, flows5, motions5, pcode5, mask5 = plate_case5(61, noc, u8)
        kw = dict(params=motions5) if motion else dict(flows=flows5)
        want5, outs = outputs(list(R.erase(frames5, plates5, remove5, list(range(5)), 0, 0, plate_code=pcode5, mask=mask5, grow=1, feather=1, **kw)))
        t = [tile5(a) for a in (frames5, plates5, motions5 if motion else flows5, pcode5, mask5, remove5)]
        ix = cints(range(NB))
        assert fn(0, NB, p(t[0]), W3, H3, noc, NB, p(t[1]), W3, H3, 0, 0, ix, p(t[2]), p(t[3]), p(t[4]), p(t[5]), 1, 1,
                  *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("erase", u8, motion))


def test_batch_65535_morphology():
    L = _F().lib()
    x5 = np.random.default_rng(70).choice(np.array([0, 1, 1, 200], np.uint8), (5, H3, W3))
    x5[1], x5[2] = 1, 0
    for stages in ((("erode", 1), ("dilate", 1)), (("dilate", 1),)):
        want5, outs = outputs(list(MR.chain(x5, stages)))
        x = tile5(x5)
        ops, radii = cints([0 if o == "erode" else 1 for o, _ in stages]), cints([r for _, r in stages])
        assert L.fotg_morph(0, NB, p(x), W3, H3, 0, len(stages), ops, radii, *(p(o.out) for o in outs), None) == 0
        assert_tiled(outs, want5, None, ("morph", stages))
