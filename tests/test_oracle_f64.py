"""The double-precision build of the oracle (oracle/libdis_oracle_f64.so) and the inputs of the tolerance mode's pointwise tests
(tests/fast_ref.py), proven fit for purpose without a GPU: on every case of tests/test_gpu_fast_refine.py and
tests/test_gpu_fast_lk.py the two builds agree within fixed sanity limits -- 3 to 10 times what they were measured at, so a build
that solved another problem, or an input on which f32 itself is unstable, fails here -- and the conditions those tests rely on
hold (mask shares, no branch the two precisions take differently)."""
import numpy as np
import pytest

import fast_ref as R
from oracle import oracle as O


def test_f64_build_is_the_same_source_in_double():
    """the ctypes mirrors match the library's layout (a level's geometry comes back right) and the by-value reals are doubles"""
    p = O.op_point(2, 1024, 1)
    q = O.params64(p)
    for name, _ in O.DisParams._fields_:
        assert getattr(q, name) == getattr(p, name), name                  # every real keeps its f32 value
    g32, g64 = O.Grid(100, 60, 2, p), O.Grid64(100, 60, 2, p)
    assert (g64.nop, g64.nopw, g64.noph, g64.steps) == (g32.nop, g32.nopw, g32.noph, g32.steps) == (375, 25, 15, 4)
    assert (g64.lb, g64.ubw, g64.ubh) == (g32.lb, g32.ubw, g32.ubh)
    assert g64.pt_ref.dtype == np.float64 and np.array_equal(g64.pt_ref, g32.pt_ref)
    v = np.float32(np.random.default_rng(0).uniform(-1, 1, 64))
    s32 = O.lib().dis_sum(O.P(v), 64, 1)
    v64 = O.f64(v)
    s64 = O.lib64().dis_sum(O.P64(v64), 64, 1)
    assert abs(s64 - float(np.sum(v64))) <= 1e-13 and abs(s32 - s64) <= 1e-5 and s32 != s64


def test_f64_grid_stages_on_exact_data():
    """template extraction, Hessian and the start from a coarser flow involve no rounding an integer-valued image could show:
    tmpl without the mean, tdx, tdy and p_init are the f32 oracle's values; the Hessian and the normalised template differ by
    rounding only"""
    w, h, lvl, _, _, I0, I0x, I0y, I1, coarse = R.lk_level("c100", 1, 8)
    for patnorm in (False, True):
        p = R.lk_params(lvl, 1, 8, 0.4, patnorm)
        g32, g64 = O.Grid(w, h, lvl, p), O.Grid64(w, h, lvl, p)
        for g in (g32, g64):
            g.init(I0[0], I0x[0], I0y[0])
            g.init_from_coarser(coarse[0])
        assert np.array_equal(g64.tdx, g32.tdx) and np.array_equal(g64.tdy, g32.tdy) and np.array_equal(g64.p_init, g32.p_init)
        if not patnorm:
            assert np.array_equal(g64.tmpl, g32.tmpl)
        assert np.abs(g64.tmpl - g32.tmpl).max() <= 1e-4
        assert (np.abs(g64.hes - g32.hes) <= 1e-6 * np.abs(g64.hes).max()).all()


@pytest.mark.parametrize("key", sorted({R.refine_key(c) for c in R.REFINE_CASES}), ids=lambda k: "%dx%d_l%d_c%d_m%d_s%d_i%d" % k)
def test_refinement_inputs_and_reference_error(key):
    w, h, lvl, noc, sor_mode, sweeps, innerit = key
    m32, m64 = R.refine_masks(w, h, noc)
    assert np.array_equal(m32, m64), "a cell whose mask depends on the precision"
    for k in range(2):
        share = 1.0 - m64[k].mean()
        assert 0.01 <= share <= 0.20, (k, share)
    r32, r64 = R.refine_reference(*key)
    assert r64.dtype == np.float64 and np.isfinite(r64).all()
    for k in range(2):
        mean, p99, mx = R.stats3(R.cell_err(r32[k], r64[k]))
        print("refinement %s pair %d: |R32 - R64| mean %.3g p99 %.3g max %.3g px; mask == 0 on %.1f %%" % (key, k, mean, p99, mx, 100 * (1 - m64[k].mean())))
        assert mean <= 1e-5 and mx <= 1e-3, (k, mean, p99, mx)
    assert np.abs(r64[0] - R.refine_inputs(w, h, noc)[2][0]).max() > 0.05        # the refinement moved the flow


@pytest.mark.parametrize("key", sorted({R.lk_key(c) for c in R.LK_CASES}), ids=lambda k: "%s_c%d_ps%d_%g_%d" % k)
def test_patch_stage_inputs_and_reference_error(key):
    ref = R.lk_reference(*key)
    for k in range(3):
        ran = ref["cnt64"][k] == 1               # the others start outside the image (patches of 4 x 4 at a border): no iteration
        assert np.array_equal(ref["cnt64"][k], ref["cnt32"][k]) and ran.mean() >= 0.9, "a start whose side of the bound depends on the precision"
        assert np.array_equal(ref["p64"][k][~ran], ref["p_init"][k][~ran]) and not ref["w64"][k][~ran].any()
        assert (ref["p64"][k] != ref["p_init"][k]).any(-1)[ran].all(), "the f64 oracle reset a patch"
        e = R.patch_err(ref["p32"][k], ref["p64"][k])
        mean, p99, mx = R.stats3(e)
        ew = R.stats3(np.abs(ref["w32"][k] - ref["w64"][k]))
        print("patch stage %s pair %d (%d patches): |p32 - p64| mean %.3g p99 %.3g max %.3g px; |w32 - w64| mean %.3g p99 %.3g max %.3g"
              % ((key, k, e.size, mean, p99, mx) + ew))
        assert mx <= 1e-4, (k, mean, p99, mx)
        assert np.abs(ref["p64"][k] - ref["p_init"][k]).max() > 0.05             # the iteration moved the patches


def test_patch_counts_of_the_named_levels():
    """alley level 3: 448 patches in columns of 14 (shorter than a wave); the 328 x 200 RGB level 2: 273 (odd); 100 x 60: 375"""
    for level, noc, nop in (("alley3", 1, 448), ("rgb328", 3, 273), ("c100", 1, 375)):
        w, h, lvl = R.lk_level(level, noc, 8)[:3]
        g = O.Grid64(w, h, lvl, R.lk_params(lvl, noc, 8, 0.4, True))
        assert g.nop == nop and (level != "alley3" or g.noph == 14)


def test_corner_rule_beyond_256_is_the_f32_one_in_both_builds():
    """a level wider than 256 px from an integer start: in f32 ceil(x + 1e-5) == x from 256 on (the 1e-5 is absorbed), so those
    patches sample one pixel to the left -- the behaviour the parity mode is pinned to.  The f64 build takes the same corner: after
    one iteration from a zero start the two builds differ by rounding on BOTH sides of x = 256, not by a pixel's worth"""
    f0, f1 = R.synth_pair(64, 384, seed=5, shift=(0.6, -0.4))
    P0, P1 = O.Pyramid(f0, 0, 8), O.Pyramid(f1, 0, 8)
    p = R.lk_params(0, 1, 8, 0.4, True)
    g32, g64 = O.Grid(384, 64, 0, p), O.Grid64(384, 64, 0, p)
    for g in (g32, g64):
        g.init(P0.im[0], P0.dx[0], P0.dy[0])
        g.optimize(P1.im[0])
    e = R.patch_err(g32.p_iter, g64.p_iter)
    right = g64.pt_ref[:, 0] >= 256
    assert right.sum() > 100 and (~right).sum() > 100
    print("one iteration from zero, x < 256: max |p32 - p64| %.3g px; x >= 256: %.3g px" % (e[~right].max(), e[right].max()))
    assert e[~right].max() <= 1e-4 and e[right].max() <= 1e-4
    assert np.abs(g64.pweight - g32.pweight).max() <= 1e-2                # (a pixel's shift changes the residuals by whole grey levels)


@pytest.mark.parametrize("ps", R.LK2_PATCH_SIZES)
def test_two_iteration_case_leaves_the_window_and_few_patches_sit_on_a_branch(ps):
    ref = R.lk2_reference(ps)
    n = ref["e_ref"].size
    far = float((ref["step1"] > 2.0).mean())
    print("two iterations, ps %d: %d patches, %.1f %% move more than 2 px in step one; f32 / f64 branch flips %d, near the outlier threshold %d, "
          "near a bound %d, left out %d" % (ps, n, 100 * far, ref["flips"].sum(), ref["near_thr"].sum(), ref["near_bound"].sum(), ref["excluded"].sum()))
    assert far >= 0.05
    assert ref["excluded"].mean() <= 0.005
    keep = ~ref["excluded"]
    print("  kept patches: |p32 - p64| mean %.3g p99 %.3g max %.3g px" % R.stats3(ref["e_ref"][keep]))
