"""The refinement alone in the tolerance mode (fotg_params::fast_math), every solver variant, bounded POINTWISE against the oracle
in double precision (tests/fast_ref.py): with R32 / R64 the f32 / f64 oracle, G the parity mode and F the tolerance mode,

    G == R32 bit for bit                                    (the anchor: the variant under test is the one the parity suite pins)
    e_ref = |R32 - R64|, e_fast = |F - R64| per cell (the larger component)
    mean, p99 and max of e_fast <= 4 x those of e_ref       (v_rcp / v_rsq + a multiplication: about 1.5 ulp against 0.5 ulp)

per pair of a batch of two.  The factor is not tuned to what the kernels return.  The planes DESIGN section 3 calls parity code (mask
and the image derivatives) are the parity mode's bits in the tolerance mode, the second pair of the batch equals the same pair alone
bit for bit, and the library's launch counters prove that the variant named by the case ran.  tests/test_oracle_f64.py checks the
inputs (1 % .. 20 % of the cells have mask == 0, |R32 - R64| is rounding) on the CPU."""
import numpy as np
import pytest

import fast_ref as R
from test_gpu_parity import _mods, dev, oracle_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_PLANES = ("mask", "Ix", "Iy", "Iz", "Ixx", "Ixy", "Iyy", "Ixz", "Iyz")


def refine_on_gpu(c, fast, pairs, taps):
    """one level through VarRefClass for the given pairs of the case's batch -> (flows (n, h, w, 2), {plane: (n, k, h, w)} with taps)"""
    F, OFClass, VarRefClass, O = _mods()
    w, h, lvl, noc = c["w"], c["h"], c["lvl"], c["noc"]
    op = F.operating_point(2, 1024, noc)
    op.coarsest_scale = op.finest_scale = lvl
    op.sor_mode, op.var_ref_iter, op.var_ref_inner_iter, op.fast_math = c["sor_mode"], c["sweeps"], c["innerit"], fast
    p, q = oracle_params(O, op), R.refine_params(lvl, noc, c["sweeps"], c["innerit"])
    assert all(getattr(p, name) == getattr(q, name) for name, _ in O.DisParams._fields_ if name != "usefbcon")
    ofc = OFClass(op, F.img_params(width=w << lvl, height=h << lvl, padding=R.PAD), max_batch=len(pairs))
    if taps:
        F.lib().fotg_enable_taps(ofc._h, 1)
    I0, I1, flow_in = R.refine_inputs(w, h, noc)
    flow = dev(flow_in[pairs]).contiguous()
    VarRefClass(dev(I0[pairs]), dev(I1[pairs]), ofc.iparams[0], ofc.op, flow)
    out = flow.cpu().numpy()
    planes = {}
    st = ((w + 3) // 4) * 4
    for nm in PARITY_PLANES if taps else ():
        k = 1 if nm == "mask" else noc
        buf = np.zeros((len(pairs), k, h, st), np.float32)
        for i in range(len(pairs)):
            F._lib.check(F.lib().fotg_varref_plane(ofc._h, i, nm.encode(), lvl, buf[i].ctypes.data))
        planes[nm] = buf[..., :w]
    assert F.lib().fotg_ctx_counter(ofc._h, b"tile_timeouts") == 0
    ofc.close()
    return out, planes


@pytest.mark.parametrize("c", R.REFINE_CASES, ids=[c["name"] for c in R.REFINE_CASES])
def test_tolerance_mode_refinement_is_bounded_pointwise(c, monkeypatch):
    F = _mods()[0]
    L = F.lib()
    for k in R.REFINE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    r32, r64 = R.refine_reference(*R.refine_key(c))
    g, g_planes = refine_on_gpu(c, False, [0, 1], taps=True)
    assert np.array_equal(g, r32), "the parity mode is not the f32 oracle: max |d| = %g" % np.abs(g - r32).max()
    watched = tuple(c["ran"]) + tuple(c["not_ran"])
    before = {n: L.fotg_debug_counter(n.encode()) for n in watched}
    f, f_planes = refine_on_gpu(c, True, [0, 1], taps=True)
    for n in c["ran"]:
        assert L.fotg_debug_counter(n.encode()) > before[n], "the %s variant did not run" % n
    for n in c["not_ran"]:
        assert L.fotg_debug_counter(n.encode()) == before[n], "the %s variant ran" % n
    for nm in PARITY_PLANES:
        assert np.array_equal(f_planes[nm], g_planes[nm]), "plane %s of the tolerance mode is not the parity mode's" % nm
    alone, _ = refine_on_gpu(c, True, [1], taps=False)
    assert np.array_equal(alone[0], f[1]), "the second pair of the batch is not the same pair alone"
    assert np.isfinite(f).all()
    # the tolerance arithmetic ran: a quiet fall-back to the exact code would return the parity mode's bits and pass at ratio 1
    assert not np.array_equal(f, g), "the tolerance mode returned the parity mode's bits"
    failures = []
    for k in range(2):
        e_ref, e_fast = R.cell_err(r32[k], r64[k]), R.cell_err(f[k], r64[k])
        try:
            R.bound(e_fast, e_ref, R.REFINE_FACTOR, "%s pair %d" % (c["name"], k))
        except AssertionError as err:
            y, x = np.unravel_index(np.argmax(e_fast), e_fast.shape)
            over = np.argwhere(e_fast > R.REFINE_FACTOR * e_ref.max())
            failures.append("%s; largest e_fast at row %d column %d; %d cells above %d x max(e_ref), rows %s"
                            % (err, y, x, len(over), R.REFINE_FACTOR, sorted(set(over[:, 0].tolist()))[:20]))
    assert not failures, "\n".join(failures)
