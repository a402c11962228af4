"""GPU test of the bindings' argument scaffold (flowonthego_amd/_args.py): every dense form of the add-ons, called once on a batch
of two and once per element as a single input, returns the same number of outputs with the same dtypes, and every output of the
single call is torch.equal to its slice of the batched output.

One size, (n, h, w) = (2, 9, 13): two pairs and an odd width are the smallest case in which an un-batching or unsqueeze mistake
shows (an output indexed at the wrong place, an optional input left without its batch dimension).  Every call accepts it.  The
vectors are finite, so torch.equal compares every value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W = 2, 9, 13
_INPUTS = {}


def inputs():
    """the inputs of every case on the device, made once (nobody writes to them)"""
    if not _INPUTS:
        rng = np.random.default_rng(913)
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        _INPUTS.update(
            flow=cuda(rng.uniform(-3, 3, (N, H, W, 2)).astype(np.float32)), bw=cuda(rng.uniform(-3, 3, (N, H, W, 2)).astype(np.float32)),
            seq=cuda(rng.uniform(-2, 2, (N, 2, H, W, 2)).astype(np.float32)), seq_bw=cuda(rng.uniform(-2, 2, (N, 2, H, W, 2)).astype(np.float32)),
            I0=cuda(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)), I1=cuda(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)),
            ref=cuda(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)), gray=cuda(rng.integers(0, 256, (N, H, W), dtype=np.uint8)),
            mask=cuda((rng.integers(0, 8, (N, H, W)) // 5).astype(np.uint8)), mask_bw=cuda((rng.integers(0, 8, (N, H, W)) // 5).astype(np.uint8)),
            ids_a=cuda(rng.integers(-1, 4, (N, H, W)).astype(np.int32)), ids_b=cuda(rng.integers(-1, 4, (N, H, W)).astype(np.int32)),
            motion=cuda(rng.uniform(-0.01, 0.01, (N, 6))))
    return _INPUTS


def _cases():
    from flowonthego_amd.blockmotion import block_motion
    from flowonthego_amd.chain import chain
    from flowonthego_amd.color import flow_to_color
    from flowonthego_amd.consistency import fb_check
    from flowonthego_amd.flowfilter import filter_flow
    from flowonthego_amd.histograms import motion_histograms
    from flowonthego_amd.interp import interpolate
    from flowonthego_amd.motion import fit_motion
    from flowonthego_amd.tracks import object_overlap
    from flowonthego_amd.warp import warp
    # name -> (the call, the names of its batched inputs in the call's order)
    return {
        "fb_check": (lambda fw, bw: fb_check(fw, bw, stats=True), ("flow", "bw")),
        "warp": (lambda src, flow, ref, occ: warp(src, flow, ref=ref, occ=occ, fill=7.0, stats=True), ("I1", "flow", "I0", "mask")),
        "warp_plain": (lambda src, flow: warp(src, flow), ("gray", "flow")),
        "interpolate": (lambda a, b, fw, bw, mf, mb, ref: interpolate(a, b, fw, bw, 0.25, mask_fw=mf, mask_bw=mb, ref=ref, stats=True),
                        ("I0", "I1", "flow", "bw", "mask", "mask_bw", "ref")),
        "chain": (lambda fw, bw: chain(fw, bw, stats=True), ("seq", "seq_bw")),
        "fit_motion": (lambda flow, mask: fit_motion(flow, mask, code=True, residual=True, stats=True, sums=True), ("flow", "mask")),
        "fit_motion_plain": (lambda flow: fit_motion(flow), ("flow",)),
        "filter_flow": (lambda flow, guide, mask: filter_flow(flow, guide, mask=mask, sigma=1.5, stats=True), ("flow", "I0", "mask")),
        "block_motion": (lambda cur, ref, flow, mask: block_motion(cur, ref, flow, mask=mask, block=8, pred=True, stats=True),
                         ("I0", "I1", "flow", "mask")),
        "object_overlap": (lambda a, b, flow, mask: object_overlap(a, b, flow, mask=mask, ka=4, kb=4), ("ids_a", "ids_b", "flow", "mask")),
        "motion_histograms": (lambda flow, mask, motion, ids: motion_histograms(flow, mask, motion, cell=8, ids=ids, rows=4),
                              ("flow", "mask", "motion", "ids_a")),
        "flow_to_color": (lambda flow: flow_to_color(flow), ("flow",)),
    }


CASES = ("fb_check", "warp", "warp_plain", "interpolate", "chain", "fit_motion", "fit_motion_plain", "filter_flow", "block_motion",
         "object_overlap", "motion_histograms", "flow_to_color")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.uint32 else t          # torch.equal on the same bits


@pytest.mark.parametrize("case", CASES)
def test_a_single_input_returns_its_slice_of_the_batch(case):
    call, names = _cases()[case]
    args = [inputs()[k] for k in names]
    batched = call(*args)
    many = isinstance(batched, tuple)
    batched = batched if many else (batched,)
    for i in range(N):
        single = call(*(a[i] for a in args))
        assert isinstance(single, tuple) == many, case
        single = single if many else (single,)
        assert len(single) == len(batched), case
        for k, (s, b) in enumerate(zip(single, batched)):
            assert s.dtype == b.dtype and s.shape == b.shape[1:], (case, i, k, s.dtype, tuple(s.shape), b.dtype, tuple(b.shape))
            assert torch.equal(_bits(s), _bits(b[i])), (case, i, k)
