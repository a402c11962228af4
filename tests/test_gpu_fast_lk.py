"""The patch stage of the tolerance mode (lk_fast_kernel, csrc/lk_fast.hip.h), every <patch size, channels> instantiation, bounded
PER PATCH against the oracle in double precision (tests/fast_ref.py): one level, the oracle's pyramid images, one LK iteration from a
synthetic coarser flow.  With P32 / P64 the f32 / f64 oracle's p_iter, G the parity mode and F the tolerance mode,

    G == P32 bit for bit (and the patch weights)
    e_ref = |P32 - P64|, e_fast = |F - P64| per patch (the larger component); nothing is left out
    mean, p99 and max of e_fast <= 8 x those of e_ref, and the same for the patch weights per element

The fast kernel is a reformulation, not a re-rounding -- centred projections minus a patch constant, an explicit inverse Hessian,
blocked sums with fused multiply-adds -- hence 8 and not the refinement's 4; the factor is not tuned to what the kernel returns.
tests/test_oracle_f64.py checks on the CPU that no patch of the f64 oracle is reset and that e_ref <= 1e-4 px everywhere.

Then two iterations from a zero start on a pair whose first step exceeds 2 px on a fifth of the patches, so that the second
evaluation leaves the staged radius-2 window: the same bound, max included, on every patch that the reference alone does not show
to sit on a branch (at most 0.5 % are left out; asserted on the CPU)."""
import numpy as np
import pytest

import fast_ref as R
from test_gpu_parity import _mods, dev, oracle_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LK_SWITCHES = ("FOTG_LK_FAST_R", "FOTG_LK_SHW", "FOTG_TEST_TAPS")


def patch_stage_on_gpu(c, fast, n):
    """InitializeGrid / InitializeFromCoarserOF / Optimize of the first n pairs of the case's level -> (p_iter (n, nop, 2), pweight)"""
    F, OFClass, _, O = _mods()
    w, h, lvl, w0, h0, I0, I0x, I0y, I1, coarse = R.lk_level(c["level"], c["noc"], c["ps"])
    op = F.operating_point(2, 1024, c["noc"])
    op.coarsest_scale = op.finest_scale = lvl
    op.patch_size, op.patch_stride, op.use_mean_normalization = c["ps"], c["stride"], c["patnorm"]
    op.grad_descent_iter, op.use_var_ref, op.fast_math = 1, False, fast
    p, q = oracle_params(O, op), R.lk_params(lvl, c["noc"], c["ps"], c["stride"], c["patnorm"])
    assert all(getattr(p, name) == getattr(q, name) for name, _ in O.DisParams._fields_)
    ofc = OFClass(op, F.img_params(width=w0, height=h0, padding=op.patch_size), max_batch=n)
    g = ofc.grid[0]
    up = lambda arr: dev(np.array(arr[:n]))               # (a writable copy: the references are read-only)
    g.InitializeGrid(up(I0), up(I0x), up(I0y))
    g.SetTargetImage(up(I1))
    g.InitializeFromCoarserOF(up(coarse))
    g.Optimize()
    st = [g.read_state(k) for k in range(n)]
    ofc.close()
    return np.stack([s["p_iter"] for s in st]), np.stack([s["pweight"] for s in st])


@pytest.mark.parametrize("c", R.LK_CASES, ids=[c["name"] for c in R.LK_CASES])
def test_tolerance_mode_patch_stage_is_bounded_per_patch(c, monkeypatch):
    for k in LK_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    n = c["n"]
    ref = R.lk_reference(*R.lk_key(c))
    gp, gw = patch_stage_on_gpu(c, False, n)
    assert np.array_equal(gp, ref["p32"][:n]) and np.array_equal(gw, ref["w32"][:n]), "the parity mode is not the f32 oracle"
    fp, fw = patch_stage_on_gpu(c, True, n)
    assert np.isfinite(fp).all() and np.isfinite(fw).all()
    # the fast kernel ran: a quiet fall-back to the exact kernel would return the parity mode's bits and pass every bound at ratio 1
    assert not np.array_equal(fp, gp) and not np.array_equal(fw, gw), "the tolerance mode returned the parity mode's bits"
    failures = []
    for k in range(n):
        e_ref, e_fast = R.patch_err(ref["p32"][k], ref["p64"][k]), R.patch_err(fp[k], ref["p64"][k])
        w_ref, w_fast = np.abs(ref["w32"][k] - ref["w64"][k]), np.abs(fw[k] - ref["w64"][k])
        for what, ef, er in (("p_iter", e_fast, e_ref), ("pweight", w_fast, w_ref)):
            try:
                R.bound(ef, er, R.LK_FACTOR, "%s pair %d %s" % (c["name"], k, what))
            except AssertionError as err:
                over = np.argwhere(ef > R.LK_FACTOR * er.max())[:, 0]
                failures.append("%s; %d above %d x max(e_ref): patches %s (wave = patch // 4 at 16 lanes per patch, column = patch // rows)"
                                % (err, len(set(over.tolist())), R.LK_FACTOR, sorted(set(over.tolist()))[:24]))
    assert not failures, "\n".join(failures)


def two_iterations_on_gpu(ps, fast):
    F, OFClass, _, O = _mods()
    wf, hf, lvl = R.LK2_FRAME
    w, h, w0, h0, I0, I0x, I0y, I1 = R.lk2_level(ps)
    op = F.operating_point(2, wf, 1)
    op.coarsest_scale = op.finest_scale = lvl
    op.patch_size, op.patch_stride = ps, R.STRIDE[ps]
    op.grad_descent_iter, op.use_var_ref, op.fast_math = 2, False, fast
    p, q = oracle_params(O, op), R.lk_params(lvl, 1, ps, R.STRIDE[ps], True, iters=2)
    assert all(getattr(p, name) == getattr(q, name) for name, _ in O.DisParams._fields_)
    ofc = OFClass(op, F.img_params(width=w0, height=h0, padding=ps))
    g = ofc.grid[0]
    up = lambda arr: dev(np.array(arr))[None]
    g.InitializeGrid(up(I0), up(I0x), up(I0y))
    g.SetTargetImage(up(I1))
    g.Optimize()
    st = g.read_state(0)
    ofc.close()
    return st["p_iter"], st["pweight"]


@pytest.mark.parametrize("ps", R.LK2_PATCH_SIZES)
def test_two_iterations_that_leave_the_staged_window(ps, monkeypatch):
    for k in LK_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    ref = R.lk2_reference(ps)
    gp, gw = two_iterations_on_gpu(ps, False)
    assert np.array_equal(gp, ref["p32"]) and np.array_equal(gw, ref["w32"]), "the parity mode is not the f32 oracle"
    fp, fw = two_iterations_on_gpu(ps, True)
    assert np.isfinite(fp).all() and not np.array_equal(fp, gp), "the tolerance mode returned the parity mode's bits"
    keep = ~ref["excluded"]
    e_fast = R.patch_err(fp, ref["p64"])
    flipped = e_fast > 1e-4
    print("two iterations, ps %d: %d of %d patches left out on the reference's evidence; the tolerance mode is off by more than 1e-4 px on %d "
          "patches, %d of them among the kept" % (ps, (~keep).sum(), keep.size, flipped.sum(), (flipped & keep).sum()))
    try:
        R.bound(e_fast[keep], ref["e_ref"][keep], R.LK_FACTOR, "two iterations ps %d p_iter" % ps)
    except AssertionError as err:
        over = np.flatnonzero(keep & (e_fast > R.LK_FACTOR * ref["e_ref"][keep].max()))
        raise AssertionError("%s; %d kept patches above %d x max(e_ref): %s, first steps %s px, at %s"
                             % (err, over.size, R.LK_FACTOR, over[:16].tolist(), np.round(ref["step1"][over[:16]], 3).tolist(),
                                ref["pt_ref"][over[:16]].tolist()))
