"""The LK / densification / scale-loop half of the oracle pinned bit for bit to the reference's OWN C++ code.

oracle/_ref/libkroeger_{of,de}_{gray,rgb}.so is kroeger/{oflow,patch,patchgrid,refine_variational}.cpp + FDF1.0.1 compiled
unmodified against the project-written minimal Eigen headers oracle/eigen_min (`make -C oracle ref`, oracle/kroeger_ref.py).
Its numeric semantics (the redux order of the dynamic-vector sums, the LLT) are DEFINITIONS following Eigen 3.3 on an SSE
build; test_eigen_min_* check them against numpy float32 step by step.

Live or stored (like tests/test_oracle.py's RefCalls): where oracle/_ref is built every kroeger call runs live and its outputs
must have the digests stored in tests/golden/kroeger_ref_live.npz; elsewhere the stored digests stand in for the outputs.  The
inputs are rebuilt here from integer arithmetic and the golden images, and their digest must equal the stored one, so a stored
output digest pins exactly the computation it was recorded from.  A digest (SHA-256 of the float32 bytes) is compared with
np.array_equal's strictness: equal digests <=> equal bits.  tests/golden/make_kroeger_golden.py records the file.
"""
import hashlib
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN, synth_pair
from oracle import oracle as O
from oracle import kroeger_ref as K

H, W = 96, 128


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


class KroegerCalls:
    """live kroeger build or its stored digests (module docstring).  Per call three SHA-256 digests are kept: of the inputs, of
    the final flow and of all outputs (final flow + every level's flow before / after refinement, in order)."""
    PATH = os.path.join(GOLDEN, "kroeger_ref_live.npz")

    def __init__(self):
        self.stored = None
        if os.path.exists(self.PATH):
            z = np.load(self.PATH)
            self.stored = dict(zip(z["keys"].tolist(), z["digests"]))
        self.recorded = {}

    def live(self, depth, noc):
        return K.available(depth, noc)

    def save(self, path):
        keys = sorted(self.recorded)
        np.savez_compressed(path, keys=np.array(keys), digests=np.stack([self.recorded[k] for k in keys]))

    def check(self, key, inputs, outputs):
        """outputs: the live build's list of float32 arrays, or None to use the stored digests.  Returns the digests
        (final flow, all outputs)."""
        din = _digest(*inputs)
        if outputs is not None:
            dig = np.stack([din, _digest(outputs[0]), _digest(*outputs)])
            self.recorded[key] = dig
            if self.stored is not None and key in self.stored:
                assert np.array_equal(self.stored[key][0], din), (key, "inputs changed since the golden file was made")
                assert np.array_equal(self.stored[key], dig), (key, "live build != its stored outputs")
            return dig[1], dig[2]
        assert self.stored is not None, "neither oracle/_ref nor %s" % self.PATH
        assert key in self.stored, (key, "not in the stored kroeger outputs")
        assert np.array_equal(self.stored[key][0], din), (key, "inputs differ from the recorded ones")
        return self.stored[key][1], self.stored[key][2]


KREF = KroegerCalls()


# ------------------------------------------------------------------------------------------------------------------------
# inputs: (h, w) float32 frames with 8-bit or quarter-step values, rebuilt from integer arithmetic or the golden images
# ------------------------------------------------------------------------------------------------------------------------
def _grid(h=H, w=W):
    yy, xx = np.mgrid[0:h, 0:w]
    return yy.astype(np.int64), xx.astype(np.int64)


def _ramp(a, b, shift=(2, 1)):
    """linear ramp along direction (a, b) (0 deg: (1, 0), 45 deg: (1, 1), 63 deg: (1, 2)), slope 0.75 per step: every patch
    is rank deficient (det H == 0 before the 1e-10 lift).  The second frame is the first moved by `shift` and with 1.25 x the
    contrast (a pure shift of a ramp is a constant offset, which the patch mean normalisation removes: no residual at all)"""
    yy, xx = _grid()
    f = lambda dx, dy: (((xx - dx) * a + (yy - dy) * b) * 3).astype(np.float32) * 0.25
    return f(0, 0), f(*shift) * np.float32(1.25)


def _stripes(a, b, shift=(3, 1)):
    """straight triangle-wave stripes along (a, b), period 16 steps, values 0..128: linear pieces and straight edges"""
    yy, xx = _grid()

    def f(dx, dy):
        t = ((xx - dx) * a + (yy - dy) * b) % 16
        return (16 * np.abs(t - 8)).astype(np.float32)
    return f(0, 0), f(*shift)


def _inputs(alley, natural_images):
    road = natural_images["road_HD"]
    plateau0, plateau1 = synth_pair(H, W, seed=11)
    for f in (plateau0, plateau1):
        f[:, :36] = 0.0
        f[:, -36:] = 255.0
    c = {
        "alley": (alley["frame_0001"][150:150 + H, 400:400 + W].astype(np.float32),
                  alley["frame_0002"][150:150 + H, 400:400 + W].astype(np.float32)),
        "road": (road[500:500 + H, 800:800 + W].astype(np.float32), road[498:498 + H, 797:797 + W].astype(np.float32)),
        "texture": synth_pair(H, W, seed=7),
        "ramp0": _ramp(1, 0), "ramp45": _ramp(1, 1), "ramp63": _ramp(1, 2),
        "stripes0": _stripes(1, 0), "stripes45": _stripes(1, 1), "stripes63": _stripes(1, 2),
        "constant": (np.full((H, W), 100.0, np.float32), np.full((H, W), 100.0, np.float32)),
        "plateau": (plateau0, plateau1),
        "padded": synth_pair(H + 5, W + 29, seed=9),        # 101 x 157: padded to a multiple of 2^sc_f on both axes
    }
    return c


def _rgb(f):
    """three channels from one gray frame, integer arithmetic: the frame, its mirror 255 - f (ramps stay ramps) and a
    quarter-step scaled copy"""
    return np.stack([f, 255.0 - f, np.floor(f * 0.5) + 0.25 * (f % 4)], -1).astype(np.float32)


def _params(op, w, noc, costfct, usefbcon, depth):
    p = O.op_point(op, w, noc)
    p.costfct, p.usefbcon, p.depth = costfct, usefbcon, depth
    return p


def _initflow(p, wp, hp):
    """an even-sized warm start of the coarsest level (D5, the odd-size clamp, stays a documented departure)"""
    nch = 1 if p.depth else 2
    h2, w2 = hp >> (p.sc_f + 1), wp >> (p.sc_f + 1)
    assert (hp >> p.sc_f) % 2 == 0 and (wp >> p.sc_f) % 2 == 0
    k = np.arange(h2 * w2 * nch).reshape(h2, w2, nch)
    return (((k * 7) % 9) - 4).astype(np.float32) * 0.25


def _run_pair(key, f0, f1, p, initflow=False):
    """oracle in the Eigen-style packet order (set_sum_order(2)) vs the kroeger build, every level before / after refinement and
    the final flow; returns (oracle final flow, kroeger output digests, oracle output digests)"""
    P0 = O.Pyramid(O.pad_frame(f0, p.sc_f), p.sc_f, p.ps)
    P1 = O.Pyramid(O.pad_frame(f1, p.sc_f), p.sc_f, p.ps)
    ini = _initflow(p, P0.w0, P0.h0) if initflow else None
    O.set_sum_order(2)
    try:
        out, lv = O.flow_pyr(P0, P1, p, dump=True, initflow=ini)
    finally:
        O.set_sum_order(0)
    mine = [out] + [a for l in sorted(lv, reverse=True) for a in lv[l]]
    inputs = [O.f32(f0), O.f32(f1), np.array([getattr(p, n) for n, _ in O.DisParams._fields_], np.float64)]
    if ini is not None:
        inputs.append(ini)
    # (the driver cannot restart a level's "before refinement" with the backward grid's start: with usefbcon and usetvref
    # both on, the "before" dumps are left out on both sides)
    keep = [True] + [not (p.usefbcon and p.usetvref) or i % 2 == 1 for i in range(len(mine) - 1)]
    mine = [a for a, k in zip(mine, keep) if k]
    live = None
    if KREF.live(p.depth, p.noc):
        kout, klv = K.flow_pyr(P0, P1, p, dump=True, initflow=ini)
        live = [kout] + [a for l in sorted(klv, reverse=True) for a in klv[l]]
        assert [a is not None for a in live] == keep, key
        live = [a for a in live if a is not None]
        diff = [i for i, (a, b) in enumerate(zip(live, mine)) if not np.array_equal(a, b)]
        assert not diff, (key, "outputs that differ (0 = final flow, then each level before / after refinement)", diff)
    theirs = KREF.check(key, inputs, live)
    return out, theirs, (_digest(mine[0]), _digest(*mine))


PARAMS = list(itertools.product((1, 3), (1, 2, 3, 4), (0, 1, 2), (0, 1), (0, 1)))


@pytest.fixture(scope="module")
def inputs(alley, natural_images):
    return _inputs(alley, natural_images)


@pytest.mark.parametrize("noc,op,costfct,usefbcon,depth", PARAMS,
                         ids=["noc%d-op%d-cost%d-fb%d-%s" % (n, o, c, f, "de" if d else "of") for n, o, c, f, d in PARAMS])
def test_oracle_equals_kroeger_bit_exact(inputs, noc, op, costfct, usefbcon, depth):
    """the oracle with the Eigen-style sum order == the reference's own LK code, every level's flow (before and after the
    variational refinement) and the final flow, on natural crops, texture, ramps / stripes at 0, 45 and 63 degrees (rank-
    deficient Hessians: Eigen's LLT stops early there), a constant frame, saturated plateaus, a padded size and an initflow"""
    bad = []
    names = list(inputs) + ["texture+initflow"]
    for name in names:
        f0, f1 = inputs["texture" if name == "texture+initflow" else name]
        if noc == 3:
            f0, f1 = _rgb(f0), _rgb(f1)
        p = _params(op, f0.shape[1], noc, costfct, usefbcon, depth)
        key = "%s/noc%d/op%d/c%d/fb%d/d%d" % (name, noc, op, costfct, usefbcon, depth)
        try:
            _, theirs, mine = _run_pair(key, f0, f1, p, initflow=name.endswith("initflow"))
        except AssertionError as e:          # (live build: the levels that differ)
            bad.append(str(e))
            continue
        if not np.array_equal(theirs[1], mine[1]):
            bad.append((key, "final flow" if not np.array_equal(theirs[0], mine[0]) else "a level's flow"))
    assert not bad, bad[:10]


def _full(f0, f1, flow_lvl, p):
    _, _, padw, padh = O.padded_size(f0.shape[1], f0.shape[0], p.sc_f)
    return O.upsample_crop(flow_lvl, p.sc_l, padw, padh, f0.shape[1], f0.shape[0])


@pytest.mark.parametrize("noc", (1, 3))
def test_d1_order_within_pin3_only_on_well_conditioned_inputs(inputs, noc):
    """Pin 3: at op-pt 2, the oracle's own summation order D1 (the engine's) stays within mean 1e-4 / max 1e-3 px of
    kroeger on the alley crop, texture, the saturated plateaus and the padded frame.  It does not on straight stripes, nor on
    the road_HD crop (large uniform asphalt): an ill-conditioned Hessian turns a last-bit difference of a sum into a different
    patch update, so there only a bit-exact comparison pins anything -- written down here as a difference that must be there.
    (kroeger's flow is the oracle's in sum order 2: test_oracle_equals_kroeger_bit_exact checks exactly these keys.)"""
    for name in ("alley", "texture", "plateau", "padded", "road", "stripes45"):
        f0, f1 = inputs[name]
        if noc == 3:
            f0, f1 = _rgb(f0), _rgb(f1)
        p = _params(2, f0.shape[1], noc, 0, 0, 0)
        key = "%s/noc%d/op2/c0/fb0/d0" % (name, noc)
        ref, theirs, mine = _run_pair(key, f0, f1, p)
        assert np.array_equal(theirs[0], mine[0]), key
        P0 = O.Pyramid(O.pad_frame(f0, p.sc_f), p.sc_f, p.ps)
        P1 = O.Pyramid(O.pad_frame(f1, p.sc_f), p.sc_f, p.ps)
        d1 = O.flow_pyr(P0, P1, p)
        e = np.sqrt(((_full(f0, f1, d1, p) - _full(f0, f1, ref, p)) ** 2).sum(-1))
        if name in ("road", "stripes45"):
            assert e.max() > 1e-2, (key, "expected the order to matter here", e.max())
        else:
            assert e.mean() <= 1e-4 and e.max() <= 1e-3, (key, e.mean(), e.max())


# ------------------------------------------------------------------------------------------------------------------------
# the eigen_min definitions themselves, against numpy float32 restatements
# ------------------------------------------------------------------------------------------------------------------------
def _np_redux(v):
    """Eigen 3.3 LinearVectorizedTraversal redux, restated in numpy float32: packets of 4, two accumulators over alternating
    packets, their sum, a trailing odd packet, predux (a0 + a2) + (a1 + a3), scalar tail"""
    v = v.astype(np.float32)
    n = v.size
    if n < 4:
        r = v[0]
        for x in v[1:]:
            r = np.float32(r + x)
        return r
    al, al2 = n // 4 * 4, n // 8 * 8
    p0 = v[0:4].copy()
    if al > 4:
        p1 = v[4:8].copy()
        for i in range(8, al2, 8):
            p0 = p0 + v[i:i + 4]
            p1 = p1 + v[i + 4:i + 8]
        p0 = p0 + p1
        if al > al2:
            p0 = p0 + v[al2:al2 + 4]
    r = np.float32(np.float32(p0[0] + p0[2]) + np.float32(p0[1] + p0[3]))
    for x in v[al:]:
        r = np.float32(r + x)
    return r


@pytest.mark.parametrize("n", (1, 3, 4, 8, 12, 20, 64, 144, 192, 432))
def test_eigen_min_redux_order(n):
    rng = np.random.default_rng(100 + n)
    v = (rng.standard_normal(n) * 1000).astype(np.float32)
    w = (rng.standard_normal(n) * 10).astype(np.float32)
    s, d, l1 = K.eigen_redux(v, w)
    assert s == _np_redux(v) and d == _np_redux(v * w) and l1 == _np_redux(np.abs(v))
    # the oracle's Eigen-style order (set_sum_order(2)) is this redux
    O.set_sum_order(2)
    try:
        assert O.lib().dis_sum(O.P(v), n, 1) == s
    finally:
        O.set_sum_order(0)


def test_eigen_min_fixed_size_ops():
    u = np.array([3.1, -4.7], np.float32)
    Hm = np.array([[2.5, 1.25], [0.75, 3.5]], np.float32)
    sq, nrm, det = K.eigen_fixed(u, Hm)
    assert sq == np.float32(u[0] * u[0] + u[1] * u[1])
    assert nrm == np.sqrt(np.float32(u[0] * u[0] + u[1] * u[1]))
    assert det == np.float32(np.float32(Hm[0, 0] * Hm[1, 1]) - np.float32(Hm[1, 0] * Hm[0, 1]))


def _np_llt2(Hm, b):
    """Eigen 3.3 LLT (unblocked, early return at a pivot <= 0) and its triangular solves, numpy float32"""
    f = np.float32
    h00, h01, h11 = f(Hm[0, 0]), f(Hm[1, 0]), f(Hm[1, 1])
    if h00 <= 0:
        l00, l10, l11, k = h00, h01, h11, 0
    else:
        l00 = np.sqrt(h00)
        l10 = f(h01 / l00)
        x = f(h11 - f(l10 * l10))
        l11, k = (h11, 1) if x <= 0 else (np.sqrt(x), -1)
    y0 = f(f(b[0]) / l00)
    y1 = f(f(f(b[1]) - f(l10 * y0)) / l11)
    x1 = f(y1 / l11)
    x0 = f(f(y0 - f(l10 * x1)) / l00)
    return l00, l10, l11, np.array([x0, x1], np.float32), k


def test_eigen_min_llt_and_its_early_return():
    """H.llt().solve(b) on a well-posed system, on the rank-1 [[4,2],[2,1]] (pivot exactly 0), on a pivot one ulp below
    zero, and on h00 <= 0 (nothing factored): the factor keeps the unfactored entries, the solve uses them, nothing is NaN"""
    f = np.float32
    one_ulp_below = np.nextafter(f(1.0), f(0.0))          # h11 = 1 - ulp: l10^2 = 1, x = -ulp < 0
    cases = {
        "spd": ([[4.0, 2.0], [2.0, 3.0]], -1),
        "rank1": ([[4.0, 2.0], [2.0, 1.0]], 1),
        "ulp_below": ([[4.0, 2.0], [2.0, one_ulp_below]], 1),
        "h00_zero": ([[0.0, 2.0], [2.0, 5.0]], 0),
        "h00_negative": ([[-1.0, 0.5], [0.5, 2.0]], 0),
    }
    b = np.array([1.5, -2.25], np.float32)
    for name, (Hm, want_k) in cases.items():
        Hm = np.array(Hm, np.float32)
        l, x, k = K.eigen_llt(Hm, b)
        l00, l10, l11, xw, kw = _np_llt2(Hm, b)
        assert k == kw == want_k, name
        assert (l[0, 0], l[1, 0], l[1, 1]) == (l00, l10, l11), (name, l)
        assert l[0, 1] == Hm[0, 1], name                    # the upper triangle is the copied input, never read
        assert np.array_equal(x, xw), (name, x, xw)
        if name != "h00_zero":
            assert np.isfinite(x).all(), name
    l, x, k = K.eigen_llt(np.array([[4.0, 2.0], [2.0, 1.0]], np.float32), np.array([1.0, 2.0], np.float32))
    assert (l[1, 1], x[0], x[1]) == (1.0, -0.5, 1.5)       # l11 stays h11 = 1: y = (0.5, 1.5), x = (-0.5, 1.5)
    # 1x1 (depth mode)
    for h, kw in ((4.0, -1), (0.0, 0), (-2.0, 0)):
        l, x, k = K.eigen_llt(np.array([[h]], np.float32), np.array([3.0], np.float32))
        lw = np.sqrt(f(h)) if h > 0 else f(h)
        assert k == kw and l[0, 0] == lw and x[0] == f(f(f(3.0) / lw) / lw), h


def test_oracle_solves_rank_deficient_patches_like_eigen():
    """the oracle's LK step on a ramp: every patch's Hessian is rank deficient and Eigen's LLT stops at its second pivot; the
    oracle must then keep l11 = h11 and take the finite step (no D3 reset) -- the patches go on iterating"""
    f0, f1 = _ramp(1, 1)
    p = O.op_point(2, W, 1)
    P0 = O.Pyramid(O.pad_frame(f0, p.sc_f), p.sc_f, p.ps)
    P1 = O.Pyramid(O.pad_frame(f1, p.sc_f), p.sc_f, p.ps)
    lw, lh = P0.level_wh(p.sc_l)
    g = O.Grid(lw, lh, p.sc_l, p)
    g.init(P0.im[p.sc_l], P0.dx[p.sc_l], P0.dy[p.sc_l])
    hes = g.hes.astype(np.float32)
    h00, h01, h11 = hes[:, 0], hes[:, 1], hes[:, 2]
    l10 = (h01 / np.sqrt(h00)).astype(np.float32)
    fail = (h11 - (l10 * l10).astype(np.float32)) <= 0
    assert fail.mean() > 0.5, fail.mean()
    g.optimize(P1.im[p.sc_l])
    assert np.isfinite(g.p_iter).all()
    assert (g.cnt[fail] > 1).mean() > 0.9       # a D3 reset would stop every one of them at its first iteration
