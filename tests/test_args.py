"""The argument scaffold of the Python bindings (flowonthego_amd/_args.py) on the CPU: every dense and every fused form of the add-ons
refuses a malformed flow, a flow on the host, an empty flow, a depth-mode context and a batch beyond max_batch with FotgError before
the library is reached, and the helpers do to CPU tensors what they do to device tensors.  No GPU needed."""
import importlib
from types import SimpleNamespace

import pytest
import torch

from flowonthego_amd import FotgError, _args

MODULES = ("color", "consistency", "warp", "interp", "chain", "motion", "objects", "temporal", "flowfilter", "blockmotion", "tracks",
           "histograms")
# imported here, before the fixture below replaces lib: a module imported after that would keep the replacement for good
_MODS = {name: importlib.import_module("flowonthego_amd." + name) for name in MODULES + ("oflow",)}
_mod = _MODS.__getitem__

IMG = torch.zeros((4, 5), dtype=torch.uint8)
IDS = torch.zeros((4, 5), dtype=torch.int32)
# name -> (module, the call given the flow)
DENSE = {
    "fb_check": ("consistency", lambda m, f: m.fb_check(f, f)),
    "warp": ("warp", lambda m, f: m.warp(IMG, f)),
    "interpolate": ("interp", lambda m, f: m.interpolate(IMG, IMG, f, f, 0.5)),
    "chain": ("chain", lambda m, f: m.chain(f)),
    "fit_motion": ("motion", lambda m, f: m.fit_motion(f)),
    "filter_flow": ("flowfilter", lambda m, f: m.filter_flow(f, IMG)),
    "block_motion": ("blockmotion", lambda m, f: m.block_motion(IMG, IMG, f)),
    "object_overlap": ("tracks", lambda m, f: m.object_overlap(IDS, IDS, f)),
    "motion_histograms": ("histograms", lambda m, f: m.motion_histograms(f)),
    "flow_to_color": ("color", lambda m, f: m.flow_to_color(f)),
}
FLOWS = {"three_components": torch.zeros((4, 5, 3)), "on_the_host": torch.zeros((4, 5, 2), dtype=torch.float32), "empty": torch.zeros((0, 5, 2))}

COARSE = torch.zeros((1, 4, 5, 2))
FRAMES = torch.zeros((1, 8, 10), dtype=torch.uint8)
# name -> (module, the call given the context and the coarse flow)
FUSED = {
    "upsample_crop_color": ("color", lambda m, o, c: m.upsample_crop_color(o, c)),
    "upsample_crop_fb_check": ("consistency", lambda m, o, c: m.upsample_crop_fb_check(o, c, c)),
    "upsample_crop_warp": ("warp", lambda m, o, c: m.upsample_crop_warp(o, c, FRAMES)),
    "upsample_crop_interpolate": ("interp", lambda m, o, c: m.upsample_crop_interpolate(o, c, c, FRAMES, FRAMES, 0.5)),
    "upsample_crop_chain": ("chain", lambda m, o, c: m.upsample_crop_chain(o, c)),
    "upsample_crop_track_points": ("chain", lambda m, o, c: m.upsample_crop_track_points(o, torch.zeros((3, 2)), c)),
    "upsample_crop_fit_motion": ("motion", lambda m, o, c: m.upsample_crop_fit_motion(o, c)),
    "upsample_crop_filter_flow": ("flowfilter", lambda m, o, c: m.upsample_crop_filter_flow(o, c, FRAMES)),
    "upsample_crop_block_motion": ("blockmotion", lambda m, o, c: m.upsample_crop_block_motion(o, c, FRAMES, FRAMES)),
    "upsample_crop_object_overlap": ("tracks", lambda m, o, c: m.upsample_crop_object_overlap(o, c, FRAMES.int(), FRAMES.int())),
    "upsample_crop_motion_histograms": ("histograms", lambda m, o, c: m.upsample_crop_motion_histograms(o, c)),
    "upsample_crop_temporal_filter": ("temporal", lambda m, o, c: m.upsample_crop_temporal_filter(o, c, FRAMES, [0], [[0]])),
}


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    """a refusal that reached the library fails the test"""
    def lib():
        raise AssertionError("the library was reached")
    monkeypatch.setattr("flowonthego_amd._lib.lib", lib)
    for m in _MODS.values():        # each module holds the name it imported
        monkeypatch.setattr(m, "lib", lib)


@pytest.mark.parametrize("flow", sorted(FLOWS))
@pytest.mark.parametrize("form", sorted(DENSE))
def test_dense_forms_refuse_a_bad_flow(form, flow):
    module, call = DENSE[form]
    with pytest.raises(FotgError):
        call(_mod(module), FLOWS[flow])


@pytest.mark.parametrize("form", sorted(FUSED))
def test_fused_forms_refuse_a_depth_context_and_a_batch_beyond_max_batch(form):
    module, call = FUSED[form]
    cpu = torch.device("cpu")
    with pytest.raises(FotgError) as e:
        call(_mod(module), SimpleNamespace(nch=1, max_batch=2, device=cpu), COARSE)
    assert "depth-mode" in str(e.value)
    with pytest.raises(FotgError) as e:
        call(_mod(module), SimpleNamespace(nch=2, max_batch=0, device=cpu), COARSE)
    if form != "upsample_crop_temporal_filter":          # which looks at its frames first
        assert "max_batch" in str(e.value)


def test_the_helpers_still_come_from_oflow():
    from flowonthego_amd import oflow
    assert oflow._ptr is _args._ptr and oflow._stream is _args._stream and oflow._dev_f32 is _args._dev_f32


def test_unbatch():
    a, b = torch.arange(6).reshape(2, 3), torch.arange(2)
    assert _args.unbatch((a, None, b), False) == (a, b) and _args.unbatch((a, None, b), False)[1] is b
    got = _args.unbatch((a, None, b), True)
    assert isinstance(got, tuple) and len(got) == 2 and torch.equal(got[0], a[0]) and torch.equal(got[1], b[0])
    assert _args.unbatch((None, a, None), False) is a and torch.equal(_args.unbatch((None, a, None), True), a[0])
    one = _args.unbatch((a, None), True, always_tuple=True)
    assert isinstance(one, tuple) and len(one) == 1 and torch.equal(one[0], a[0])


def test_cat_chunks():
    a, b = torch.arange(6).reshape(2, 3), torch.arange(6, 9).reshape(1, 3)
    assert _args.cat_chunks([a]) is a
    assert torch.equal(_args.cat_chunks([a, b]), torch.arange(9).reshape(3, 3))
    u = lambda t: (t.to(torch.int32) + 2 ** 31 - 4).view(torch.uint32)           # values on both sides of 2^31
    got = _args.cat_chunks([(a, None, u(a)), (b, None, u(b))])
    assert isinstance(got, tuple) and len(got) == 3 and got[1] is None and torch.equal(got[0], torch.cat((a, b)))
    assert got[2].dtype == torch.uint32 and got[2].shape == (3, 3)
    assert got[2].view(torch.int32).tolist() == torch.cat((u(a).view(torch.int32), u(b).view(torch.int32))).tolist()
    nested = _args.cat_chunks([((a, b), a), ((b, a), b)])
    assert torch.equal(nested[0][0], torch.cat((a, b))) and torch.equal(nested[0][1], torch.cat((b, a))) and torch.equal(nested[1], torch.cat((a, b)))
    assert _args.cat_chunks([(a, (b, None))]) == (a, (b, None))


def test_optional_and_batched():
    assert _args.optional(None, "mask", torch.device("cpu"), (1, 2, 3)) is None
    assert _args.optional(None, "mask", None, (1, 2, 3), torch.uint8, single=True) is None
    with pytest.raises(FotgError):
        _args.optional(torch.zeros((2, 3)), "mask", None, (1, 2, 3), single=True)         # on the host
    t = torch.zeros((2, 3))
    assert _args.batched(t, False) is t and _args.batched(t, True).shape == (1, 2, 3) and _args.batched(None, True) is None
    assert _args.batched(7, True) == 7


def test_image_stack_refusals():
    cpu = torch.device("cpu")
    f32u8 = (torch.float32, torch.uint8)
    for bad in (None, torch.zeros((4, 5, 3), dtype=torch.float64), torch.zeros((5,)), torch.zeros((1, 4, 5, 2)), torch.zeros((2, 4, 5)),
                torch.zeros((1, 4, 5, 0)), torch.zeros((1, 4, 5))):                       # the last: on the host
        with pytest.raises(FotgError):
            _args.image_stack(bad, "src", 1, 4, 5, cpu, f32u8)
    with pytest.raises(FotgError):
        _args.image_stack(torch.zeros((3, 0, 5)), "frames", None, None, None, cpu, f32u8)
    with pytest.raises(FotgError):
        _args.image_stack(torch.zeros((4, 5), dtype=torch.float32), "cur", 1, 4, 5, cpu, (torch.uint8,), single=True)
