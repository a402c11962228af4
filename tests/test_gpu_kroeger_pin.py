"""GPU tests on the inputs of the kroeger pin (tests/test_kroeger_pin.py): ramps and straight stripes at 0 / 45 / 63 degrees
(rank-deficient Hessians, where Eigen's LLT stops early and solves with the unfactored pivot), a constant frame, saturated
plateaus, natural crops and texture.

- parity mode: the engine == the oracle, batched, gray and RGB, op-pts 1-4;
- where the oracle's summation orders D1 (the engine's) and Eigen's (kroeger's) give the same bits, the engine == the reference's
  own LK code: the live build in oracle/_ref, or the digests it recorded (tests/golden/kroeger_ref_live.npz);
- fast mode: finite everywhere, and the tolerance of tests/test_gpu_fast.py on the well-conditioned inputs, where that
  tolerance is meaningful (on stripes a last-bit change of a sum moves the flow by pixels, DESIGN 2 Pin 3)."""
import numpy as np
import pytest

from test_gpu_parity import _mods, dev, epe, oracle_params
from test_gpu_fast import TOL_MEAN
import test_kroeger_pin as KP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EDGE = ("ramp0", "ramp45", "ramp63", "stripes0", "stripes45", "stripes63", "constant", "plateau")


@pytest.fixture(scope="module")
def inputs(alley, natural_images):
    return KP._inputs(alley, natural_images)


def _stack(inputs, names, noc):
    f0 = [inputs[n][0] for n in names]
    f1 = [inputs[n][1] for n in names]
    if noc == 3:
        f0, f1 = [KP._rgb(f) for f in f0], [KP._rgb(f) for f in f1]
    return f0, f1


def _engine(F, OFClass, f0, f1, op_point, noc, fast=False, **kw):
    h, w = f0[0].shape[:2]
    op = F.operating_point(op_point, w, noc)
    for k, v in kw.items():
        setattr(op, k, v)
    op.fast_math = fast
    ofc = OFClass(op, F.img_params(width=w, height=h, padding=op.patch_size), max_batch=len(f0))
    lo = ofc.calc_batch(dev(np.stack(f0)), dev(np.stack(f1)))
    out = lo.cpu().numpy(), ofc.upsample_crop(lo).cpu().numpy()
    ofc.close()
    return op, out


def _oracle(O, f0, f1, p, order=0):
    O.set_sum_order(order)
    try:
        return O.flow(O.pad_frame(f0, p.sc_f), O.pad_frame(f1, p.sc_f), p, 0)
    finally:
        O.set_sum_order(0)


@pytest.mark.parametrize("noc", (1, 3))
@pytest.mark.parametrize("op_point", (1, 2, 3, 4))
def test_edge_inputs_parity(inputs, op_point, noc):
    """parity mode on rank-deficient / degenerate frames, one batch of eight pairs: every pair == the oracle"""
    F, OFClass, _, O = _mods()
    f0, f1 = _stack(inputs, EDGE, noc)
    op, (lo, _) = _engine(F, OFClass, f0, f1, op_point, noc)
    p = oracle_params(O, op)
    for k, name in enumerate(EDGE):
        assert np.array_equal(lo[k], _oracle(O, f0[k], f1[k], p)), (name, op_point, noc)


@pytest.mark.parametrize("noc", (1, 3))
def test_edge_inputs_parity_other_costs_and_fb_merge(inputs, noc):
    """the same with the L1 and pseudo-Huber costs and the forward-backward merge (op-pt 2)"""
    F, OFClass, _, O = _mods()
    f0, f1 = _stack(inputs, EDGE, noc)
    for kw in ({"cost_func": 1}, {"cost_func": 2}, {"use_fbcon": True}):
        op, (lo, _) = _engine(F, OFClass, f0, f1, 2, noc, **kw)
        p = oracle_params(O, op)
        for k, name in enumerate(EDGE):
            assert np.array_equal(lo[k], _oracle(O, f0[k], f1[k], p)), (name, kw, noc)


@pytest.mark.parametrize("noc", (1, 3))
def test_engine_equals_kroeger_where_the_sum_order_is_free(inputs, noc):
    """where the oracle gives the same bits in D1 order (the engine's) and in Eigen's packet order (kroeger's), the engine's
    flow is the reference's own LK code's, bit for bit (live oracle/_ref, or its recorded output digests)"""
    F, OFClass, _, O = _mods()
    names = [n for n in inputs if n != "padded"]
    f0, f1 = _stack(inputs, names, noc)
    checked = []
    for op_point in (1, 2, 3, 4):
        op, (lo, _) = _engine(F, OFClass, f0, f1, op_point, noc)
        for k, name in enumerate(names):
            p = KP._params(op_point, f0[k].shape[1], noc, 0, 0, 0)
            if not np.array_equal(_oracle(O, f0[k], f1[k], p, 0), _oracle(O, f0[k], f1[k], p, 2)):
                continue
            key = "%s/noc%d/op%d/c0/fb0/d0" % (name, noc, op_point)
            _, theirs, _ = KP._run_pair(key, f0[k], f1[k], p)
            assert np.array_equal(KP._digest(lo[k]), theirs[0]), key
            checked.append(key)
    assert any(c.startswith("constant/") for c in checked) and len(checked) >= 4, checked


@pytest.mark.parametrize("noc", (1, 3))
def test_fast_math_edge_inputs(inputs, noc):
    """tolerance mode on the same frames: no NaN / inf anywhere; the mean EPE bound of tests/test_gpu_fast.py against the parity
    mode on the well-conditioned ones -- those test_kroeger_pin.py finds within Pin 3 (alley crop, texture) and the constant
    frame.  Not on ramps, stripes, the plateaus' straight edges or the road_HD crop's uniform asphalt: patches there have
    (nearly) rank-deficient Hessians, whether det H is exactly 0 (the 1e-10 lift) and whether the second pivot is <= 0 (Eigen's
    early return) are decided by the last bits of sums the tolerance mode rounds differently, and the step along the null
    direction follows the branch (measured: 0.049 px mean on the 45-degree ramp at op-pt 3, 0.013 px on the RGB plateaus and
    1.3e-3 px on the RGB road crop at op-pt 2)"""
    F, OFClass, _, O = _mods()
    names = EDGE + ("alley", "road", "texture")
    f0, f1 = _stack(inputs, names, noc)
    for op_point in (1, 2, 3, 4):
        _, (ex_lo, ex_full) = _engine(F, OFClass, f0, f1, op_point, noc)
        _, (fa_lo, fa_full) = _engine(F, OFClass, f0, f1, op_point, noc, fast=True)
        assert np.isfinite(fa_lo).all() and np.isfinite(fa_full).all(), (op_point, noc)
        for k, name in enumerate(names):
            if name in ("alley", "texture", "constant"):
                assert epe(fa_full[k], ex_full[k]).mean() <= TOL_MEAN, (name, op_point, noc)
