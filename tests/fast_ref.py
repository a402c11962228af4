"""Cases, inputs and references of the tolerance mode's pointwise tests (fotg_params::fast_math).

The yardstick is the oracle compiled a second time with double as its real type (oracle/libdis_oracle_f64.so, oracle.varref64 /
oracle.Grid64): R64.  The f32 oracle's own distance from it, e_ref = |R32 - R64|, is what "the same arithmetic, rounded
differently" costs on a given input; the tolerance mode's e_fast = |F - R64| is bounded by a fixed multiple of it, for the mean,
the 99th percentile and the maximum (bound()).  Nothing here comes from the code under test.

tests/test_oracle_f64.py proves on the CPU that every input below is fit for that purpose; tests/test_gpu_fast_refine.py and
tests/test_gpu_fast_lk.py run the kernels on the same cases.  Every reference is computed once per session (lru_cache) and
returned read-only."""
import functools
import os

import numpy as np

from conftest import GOLDEN, synth_pair
from oracle import oracle as O

PAD = 8                    # padding of the refinement's level images (the context's patch size)
REFINE_FACTOR = 4          # e_fast <= 4 x e_ref: v_rcp / v_rsq + a multiplication (about 1.5 ulp) against 0.5 ulp, rounded up
LK_FACTOR = 8              # the fast LK kernel is a reformulation (centred projections, explicit inverse Hessian), not a re-rounding


def _ro(a):
    a.setflags(write=False)
    return a


def stats3(e):
    e = np.asarray(e, np.float64).ravel()
    return float(e.mean()), float(np.percentile(e, 99)), float(e.max())


def bound(e_fast, e_ref, factor, what):
    """mean, p99 and max of e_fast within factor x those of e_ref; prints the six figures and the ratios first"""
    f, r = stats3(e_fast), stats3(e_ref)
    ratios = tuple(a / b if b > 0 else (0.0 if a == 0 else float("inf")) for a, b in zip(f, r))
    print("%s: e_ref mean %.3g p99 %.3g max %.3g | e_fast mean %.3g p99 %.3g max %.3g | ratio %.2f %.2f %.2f"
          % ((what,) + r + f + ratios))
    for name, a, b in zip(("mean", "p99", "max"), f, r):
        assert a <= factor * b, "%s: %s(e_fast) = %.4g > %d x %s(e_ref) = %.4g" % (what, name, a, factor, name, factor * b)
    return ratios


# ------------------------------------------------------------------------------------------------------------------------------
# refinement: one level through VarRefClass
# ------------------------------------------------------------------------------------------------------------------------------

def refine_params(lvl, noc, sweeps=3, innerit=1):
    """the oracle's parameters of F.operating_point(2, 1024, noc) with coarsest_scale = finest_scale = lvl"""
    p = O.op_point(2, 1024, noc)
    p.sc_f = p.sc_l = lvl
    p.tv_solverit, p.tv_innerit = sweeps, innerit
    return p


@functools.lru_cache(maxsize=None)
def refine_inputs(w, h, noc):
    """a batch of two pairs at the level's own size: padded level images I0, I1 (2, h + 16, w + 16, noc) and the input flow
    (2, h, w, 2) = the pair's true flow plus a smooth 0.3 px perturbation; pair 1 is pair 0 with the frames swapped and the flow
    negated.  The flow points out of the image along two borders: those cells have mask == 0."""
    f0, f1, truth = synth_pair(h, w, noc=noc, shift=(1.0, -0.5), truth=True)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    # the perturbation points away from the centre, 0.3 px at the borders: with it every pair of every level below has between
    # 1 % and 20 % of its cells outside (tests/test_oracle_f64.py); pair 1 gets it pointing inwards
    pert = 0.3 * np.stack([2 * xx / (w - 1) - 1, 2 * yy / (h - 1) - 1], -1)
    flow = (truth.astype(np.float64) + pert).astype(np.float32)
    pad = lambda a: np.pad(a.reshape(h, w, noc), ((PAD, PAD), (PAD, PAD), (0, 0)), mode="edge")
    a, b = pad(f0), pad(f1)
    return _ro(np.stack([a, b])), _ro(np.stack([b, a])), _ro(np.stack([flow, -flow]))


def refine_masks(w, h, noc):
    """image_warp's mask of both pairs by the oracle's own dis_image_warp (opticalflow_aux.c:18-60), in its f32 and its f64 build:
    (2, h, w) bool each"""
    import ctypes as C
    flow = refine_inputs(w, h, noc)[2]
    st = O.lib().dis_stride(w)
    out = []
    for L, t, ptr in ((O.lib(), np.float32, O.P), (O.lib64(), np.float64, O.P64)):
        masks = []
        for k in range(2):
            wx, wy = (np.zeros((h, st), t) for _ in range(2))
            wx[:, :w], wy[:, :w] = flow[k, ..., 0], flow[k, ..., 1]
            src, dst, mask = np.zeros((h, st), t), np.zeros((h, st), t), np.zeros((h, st), t)
            L.dis_image_warp(ptr(dst), ptr(mask), ptr(src), ptr(wx), ptr(wy), C.c_int(w), C.c_int(h), C.c_int(1))
            masks.append(mask[:, :w] != 0)
        out.append(np.stack(masks))
    return out


@functools.lru_cache(maxsize=None)
def refine_reference(w, h, lvl, noc, sor_mode=0, sweeps=3, innerit=1):
    """(R32, R64): the refined flows (2, h, w, 2) of both pairs by the f32 and the f64 oracle"""
    I0, I1, flow = refine_inputs(w, h, noc)
    p = refine_params(lvl, noc, sweeps, innerit)
    r32 = np.stack([O.varref(I0[k], I1[k], w, h, lvl, p, flow[k], sor_mode) for k in range(2)])
    r64 = np.stack([O.varref64(I0[k], I1[k], w, h, lvl, p, flow[k], sor_mode) for k in range(2)])
    return _ro(r32), _ro(r64)


def cell_err(a, r64):
    """per cell, the larger of the two components' |a - R64|"""
    return np.abs(np.asarray(a, np.float64) - r64).max(-1)


def _rc(name, w, h, lvl, noc=1, sor_mode=0, sweeps=3, innerit=1, env=None, ran=(), not_ran=()):
    return dict(name=name, w=w, h=h, lvl=lvl, noc=noc, sor_mode=sor_mode, sweeps=sweeps, innerit=innerit, env=env or {},
                ran=ran, not_ran=not_ran)


def _refine_cases():
    """every refinement variant at the smallest level that reaches it.  env: switches read at context creation; ran / not_ran:
    launch counters (fotg_debug_counter) that must / must not move in the tolerance-mode run"""
    c = []
    for noc, tag in ((1, "gray"), (3, "rgb")):                               # the fused per-level kernel
        c.append(_rc("fused_41x23_l1_" + tag, 41, 23, 1, noc))
        c.append(_rc("fused_64x28_l4_" + tag, 64, 28, 4, noc))
    c.append(_rc("fused_cglobal_100x30_l4", 100, 30, 4, ran=("fused_cglobal",)))
    c.append(_rc("sor_pipe_120x60_l4", 120, 60, 4, ran=("sor_pipe",)))
    for w, h in ((120, 68), (120, 67), (100, 75)):                           # levels of 65..96 rows
        c.append(_rc("stream_%dx%d_l4" % (w, h), w, h, 4, ran=("sor_stream",)))
        c.append(_rc("stream_off_%dx%d_l4" % (w, h), w, h, 4, env={"FOTG_VR_STREAM": "0"}, not_ran=("sor_stream",)))
    for noc, tag in ((1, "gray"), (3, "rgb")):                               # three bands, the third of 4 rows
        c.append(_rc("levelpipe_160x132_l2_" + tag, 160, 132, 2, noc, ran=("level_pipe",)))
        c.append(_rc("tiles_160x132_l2_" + tag, 160, 132, 2, noc, env={"FOTG_VR_LEVELPIPE": "0"}, ran=("sor_tiles",), not_ran=("level_pipe",)))
    c.append(_rc("tiles_160x132_l2_sweeps1", 160, 132, 2, sweeps=1, ran=("sor_tiles",), not_ran=("level_pipe",)))
    c.append(_rc("levelpipe_160x132_l2_sweeps2", 160, 132, 2, sweeps=2, ran=("level_pipe",)))
    c.append(_rc("levelpipe_160x132_l2_sweeps4", 160, 132, 2, sweeps=4, ran=("level_pipe",)))
    tall = (76, 1304, 0)                                                     # more than 1024 rows, a width that is no multiple of 32
    c.append(_rc("levelpipe_76x1304_l0", *tall, ran=("level_pipe",)))
    c.append(_rc("tiles_76x1304_l0", *tall, env={"FOTG_VR_LEVELPIPE": "0"}, ran=("sor_tiles",), not_ran=("level_pipe",)))
    c.append(_rc("tall_76x1304_l0", *tall, env={"FOTG_VR_PATH": "1"}, ran=("sor_tall",), not_ran=("level_pipe", "sor_tiles")))
    c.append(_rc("tiles_76x1304_l0_sweeps6", *tall, sweeps=6, ran=("sor_tiles",), not_ran=("level_pipe",)))
    for w, h in ((64, 28), (120, 68)):                                       # the fall-back paths
        c.append(_rc("path1_%dx%d_l4" % (w, h), w, h, 4, env={"FOTG_VR_PATH": "1"}, not_ran=("sor_stream", "sor_pipe")))
        c.append(_rc("path2_%dx%d_l4" % (w, h), w, h, 4, env={"FOTG_VR_PATH": "2"}))
        c.append(_rc("path2_nofirst_%dx%d_l4" % (w, h), w, h, 4, env={"FOTG_VR_PATH": "2", "FOTG_VR_FIRST_DATA": "0"}))
    for w, h, lvl in ((120, 68, 4), (160, 132, 2)):                          # the other solvers, two inner iterations per level step
        c.append(_rc("redblack_%dx%d_l%d" % (w, h, lvl), w, h, lvl, sor_mode=1))
        c.append(_rc("point_%dx%d_l%d" % (w, h, lvl), w, h, lvl, sor_mode=2))
        c.append(_rc("innerit2_%dx%d_l%d" % (w, h, lvl), w, h, lvl, innerit=2))
    return c


REFINE_CASES = _refine_cases()
REFINE_SWITCHES = ("FOTG_VR_PATH", "FOTG_VR_STREAM", "FOTG_VR_LEVELPIPE", "FOTG_VR_FIRST_DATA")


def refine_key(c):
    """what the oracle's result depends on (the switches and counters do not enter)"""
    return (c["w"], c["h"], c["lvl"], c["noc"], c["sor_mode"], c["sweeps"], c["innerit"])


# ------------------------------------------------------------------------------------------------------------------------------
# patch stage: one level, one LK iteration from a synthetic coarser flow
# ------------------------------------------------------------------------------------------------------------------------------

def _lk_frames(level, noc):
    """(f0, f1, lvl, true flow or None): alley3 = Sintel alley_1 at level 3 (448 patches of 8 x 8: a single patch column shorter than a wave);
    rgb328 = the 328 x 200 RGB pair at level 2 (273 patches); c100 = a 400 x 240 pair at level 2 (100 x 60, odd patch counts)"""
    if level == "alley3":
        z = np.load(os.path.join(GOLDEN, "alley_1_gray.npz"))
        return z["frame_0001"].astype(np.float32), z["frame_0002"].astype(np.float32), 3, None
    if level == "rgb328":
        return synth_pair(200, 328, seed=9, noc=3) + (2, None)
    if level == "c100":
        f0, f1, truth = synth_pair(240, 400, seed=21, noc=noc, truth=True)
        return f0, f1, 2, truth
    raise KeyError(level)


@functools.lru_cache(maxsize=None)
def lk_level(level, noc, ps):
    """the oracle's pyramid images of the level, for up to three pairs of a batch.  Returns (w, h, lvl, w0, h0, I0, I0x, I0y, I1,
    coarse): images (3, h + 2 ps, w + 2 ps, noc), coarse (3, h // 2, w // 2, 2) the synthetic coarser flows.  Pair 1 is pair 0
    backwards, pair 2 is pair 0 from another start."""
    f0, f1, lvl, truth = _lk_frames(level, noc)
    P0 = O.Pyramid(O.pad_frame(f0, lvl), lvl, ps)
    P1 = O.Pyramid(O.pad_frame(f1, lvl), lvl, ps)
    w, h = P0.level_wh(lvl)
    yy, xx = np.mgrid[0:h // 2, 0:w // 2].astype(np.float64)
    def smooth(ph):          # up to 0.45 px at the coarser level = 0.9 px at this one
        return (0.45 * np.stack([np.sin(2 * np.pi * xx / (w // 2) + ph) * np.cos(np.pi * yy / (h // 2)),
                                 np.cos(2 * np.pi * yy / (h // 2) + ph) * np.sin(np.pi * xx / (w // 2) + 0.3)], -1)).astype(np.float32)
    c0, c2 = smooth(0.0), smooth(1.1)
    if truth is not None:    # c100: the pair's true flow at the coarser level, off by a third of that (patches of 4 x 4 are reset
        s = 2 << lvl         # after a step of 2 px: they need a start this close)
        t = truth[s // 2::s, s // 2::s][:h // 2, :w // 2] / s
        c0, c2 = t + c0 / 3, t - c0 / 6
    I0 = np.stack([P0.im[lvl], P1.im[lvl], P0.im[lvl]]); I0x = np.stack([P0.dx[lvl], P1.dx[lvl], P0.dx[lvl]])
    I0y = np.stack([P0.dy[lvl], P1.dy[lvl], P0.dy[lvl]]); I1 = np.stack([P1.im[lvl], P0.im[lvl], P1.im[lvl]])
    return (w, h, lvl, P0.w0, P0.h0) + tuple(_ro(a) for a in (I0, I0x, I0y, I1, np.stack([c0, -c0, c2])))


def lk_params(lvl, noc, ps, stride, patnorm, iters=1):
    p = O.op_point(2, 1024, noc)
    p.sc_f = p.sc_l = lvl
    p.ps, p.patove, p.patnorm = ps, stride, int(patnorm)
    p.max_iter = p.min_iter = iters
    p.usetvref = 0
    return p


STRIDE = {4: 0.5, 8: 0.4, 12: 0.75, 16: 0.5}      # op-pt 2, op-pt 3, and test_fast_math_other_configurations' for 4 and 16


def _lk(name, level, noc, ps, patnorm=True, n=1, env=None):
    return dict(name=name, level=level, noc=noc, ps=ps, stride=STRIDE[ps], patnorm=patnorm, n=n, env=env or {})


def _lk_cases():
    c = []
    for ps in (4, 8, 12, 16):                                               # every <PS, NOC> instantiation, with and without the mean
        for noc, tag in ((1, "gray"), (3, "rgb")):
            for patnorm in (True, False):
                c.append(_lk("c100_ps%d_%s%s" % (ps, tag, "" if patnorm else "_nomean"), "c100", noc, ps, patnorm))
    for ps in (8, 12):                                                      # gray 8 / 12: the staged radius-2 window, and without it
        c.append(_lk("alley3_ps%d" % ps, "alley3", 1, ps))
        c.append(_lk("alley3_ps%d_whole_window" % ps, "alley3", 1, ps, env={"FOTG_LK_FAST_R": "0"}))
        c.append(_lk("c100_ps%d_gray_whole_window" % ps, "c100", 1, ps, env={"FOTG_LK_FAST_R": "0"}))
        # every evaluation through the level image: the path an evaluation outside the staged window takes (a test tap)
        c.append(_lk("alley3_ps%d_level_image" % ps, "alley3", 1, ps, env={"FOTG_TEST_TAPS": "1", "FOTG_LK_SHW": "3"}))
    c.append(_lk("rgb328_ps8", "rgb328", 3, 8))
    c.append(_lk("c100_ps8_gray_batch3", "c100", 1, 8, n=3))                # three pairs: the banded placement
    c.append(_lk("c100_ps12_rgb_batch3", "c100", 3, 12, n=3))
    c.append(_lk("alley3_ps8_batch3", "alley3", 1, 8, n=3))
    return c


LK_CASES = _lk_cases()


def lk_key(c):
    return (c["level"], c["noc"], c["ps"], c["stride"], c["patnorm"])


@functools.lru_cache(maxsize=None)
def lk_reference(level, noc, ps, stride, patnorm):
    """one LK iteration of all three pairs by both oracles: dict of p_init (3, nop, 2), p32 / w32 / cnt32 (f32 oracle), p64 / w64 /
    cnt64 (f64 oracle); cnt = iterations run: 0 where the start lies outside the image (the patch keeps it, with zero weights)"""
    w, h, lvl, _, _, I0, I0x, I0y, I1, coarse = lk_level(level, noc, ps)
    p = lk_params(lvl, noc, ps, stride, patnorm)
    out = {k: [] for k in ("p_init", "p32", "w32", "cnt32", "p64", "w64", "cnt64")}
    for k in range(3):
        for G, tag in ((O.Grid, "32"), (O.Grid64, "64")):
            g = G(w, h, lvl, p)
            g.init(I0[k], I0x[k], I0y[k])
            g.init_from_coarser(coarse[k])
            g.optimize(I1[k])
            out["p" + tag].append(g.p_iter); out["w" + tag].append(g.pweight)
            out["cnt" + tag].append(g.cnt)
            if tag == "32":
                out["p_init"].append(g.p_init)
    return {k: _ro(np.stack(v)) for k, v in out.items()}


def patch_err(a, p64):
    """per patch, the larger of the two components' |a - P64|"""
    return np.abs(np.asarray(a, np.float64) - p64).max(-1)


# ---- two iterations whose first step is longer than 2 px: the second evaluation leaves the staged radius-2 window.
# The 384 x 256 pair of test_fast_math_large_motion_leaves_the_small_window at one scale, from a zero start.  That pair's texture
# decorrelates within two pixels: a first LK step on it never exceeds 1 px at scale 1 (1.9 px at scale 0).  Both frames are therefore
# smoothed (eight passes of the binomial filter 1 4 6 4 1, sigma about 2.8 px, back to 8-bit values) and the one scale is 0, where
# the motion is 4 +- 2 px: a fifth of the patches then moves more than 2 px in step one (tests/test_oracle_f64.py: at least 5 %).
LK2_FRAME = (384, 256, 0)              # frame width, height, the one scale
LK2_PATCH_SIZES = (8, 12)              # the two gray patch sizes that stage a radius-2 window


def _smooth(a, passes=8):
    a = a.astype(np.float64)
    for _ in range(passes):
        for ax in (0, 1):
            n = a.shape[ax]
            p = np.pad(a, [(2, 2) if i == ax else (0, 0) for i in range(2)], mode="edge")
            t = (lambda o: p[o:o + n]) if ax == 0 else (lambda o: p[:, o:o + n])
            a = (t(0) + 4 * t(1) + 6 * t(2) + 4 * t(3) + t(4)) / 16
    return a


@functools.lru_cache(maxsize=None)
def lk2_level(ps):
    """(w, h, w0, h0, I0, I0x, I0y, I1): the level's images from the oracle's pyramid; no coarser level, every patch starts at zero"""
    wf, hf, lvl = LK2_FRAME
    f0, f1 = synth_pair(hf, wf, seed=31, shift=(4.0, -3.0))
    f0, f1 = _smooth(f0), _smooth(f1)
    lo, hi = min(f0.min(), f1.min()), max(f0.max(), f1.max())
    f0, f1 = (np.round((f - lo) * (255.0 / (hi - lo))).astype(np.float32) for f in (f0, f1))
    P0 = O.Pyramid(O.pad_frame(f0, lvl), lvl, ps)
    P1 = O.Pyramid(O.pad_frame(f1, lvl), lvl, ps)
    w, h = P0.level_wh(lvl)
    return (w, h, P0.w0, P0.h0) + tuple(_ro(a) for a in (P0.im[lvl], P0.dx[lvl], P0.dy[lvl], P1.im[lvl]))


@functools.lru_cache(maxsize=None)
def lk2_reference(ps):
    """two LK iterations by both oracles (p32 / w32, p64 / w64), the f64 oracle's first step length (step1) and the patches that
    the reference ALONE shows to sit on a branch (excluded): e_ref > 1e-4 (the f32 oracle itself flips there), a distance from the
    start within 1e-3 relative of the outlier threshold ps / 2, or a position within 1e-3 px of a bound, after either iteration"""
    lvl = LK2_FRAME[2]
    w, h, _, _, I0, I0x, I0y, I1 = lk2_level(ps)
    p = lk_params(lvl, 1, ps, STRIDE[ps], True, iters=2)
    res = {}
    for G, tag in ((O.Grid, "32"), (O.Grid64, "64")):
        g = G(w, h, lvl, p)
        g.init(I0, I0x, I0y)
        tr = g.optimize(I1, trace=True)
        res["p" + tag], res["w" + tag], res["tr" + tag] = g.p_iter, g.pweight, tr
    pos = res["tr64"][:, 1:3, :2].astype(np.float64)                        # p after iterations 1 and 2 (the start is zero)
    dist = np.sqrt((pos ** 2).sum(-1))
    thr = ps / 2.0
    pt = g.pt_ref.astype(np.float64)[:, None, :] + pos
    near_thr = (np.abs(dist - thr) <= 1e-3 * thr).any(-1)
    near_bound = ((np.abs(pt - g.lb) <= 1e-3).any(-1) | (np.abs(pt[..., 0] - g.ubw) <= 1e-3) | (np.abs(pt[..., 1] - g.ubh) <= 1e-3)).any(-1)
    e_ref = patch_err(res["p32"], res["p64"])
    res.update(e_ref=e_ref, step1=dist[:, 0], flips=e_ref > 1e-4, near_thr=near_thr, near_bound=near_bound,
               excluded=(e_ref > 1e-4) | near_thr | near_bound, pt_ref=g.pt_ref)
    return {k: _ro(np.asarray(v)) for k, v in res.items()}
