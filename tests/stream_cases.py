"""One table for the stream-order tests (tests/test_gpu_streams.py): a row per entry point of include/fotg.h that takes a
`void *stream` or `void *after_stream`, tests/test_stream_cases.py holds the table to the header.

A row names its C-ABI entry point and the fotg_*.hip file that defines it, builds two input sets A and B of identical shapes and
dtypes (host arrays, from the generators of the add-ons' own tests), and has a call(x, slot) that reaches the entry point through
its Python binding on torch's CURRENT stream -- the harness enters torch.cuda.stream(S) -- with every optional output asked for,
and returns the output tensors.  (A binding allocates its outputs itself, on the current stream; the harness lays sentinels under
them.)  Three rows have no binding that reaches their case and call lib().fotg_* with _ptr and _stream: the flow filter without
`out` (its fifth buffer) and the two colour calls without `stats` (their only stream-ordered allocation).

slot: include/fotg.h says "A pipe is used from one thread at a time (like a context)", and a context's buffers belong to the one
call that is in flight on it, so a core row keeps one context (or pipe) per slot and the two-stream test gives each stream its own.  The fused
fotg_upsample_crop_* rows and fotg_upsample_crop read only the context's geometry and share one context over every slot, stream
and host thread.

Shapes: the smallest of the add-on's own test at which the call issues every launch, memset and scratch allocation it can --
more than one tile or workgroup each way, iters >= 1 where there is a count, a second fold round for the motion sums (640 x 420)."""
import numpy as np
import torch

import limits_ref as X

f32 = np.float32
FUSED_W, FUSED_H, FUSED_BATCH = 640, 420, 6          # the shared context of the fused rows: 263 workgroups of the motion sums
CORE_W, CORE_H = 640, 360

# the entry points that take a stream and have no row, each with its reason
EXEMPT = {
    "fotg_pyramid": "stage-level debug entry point: a stage of fotg_calc_batch, whose rows run it",
    "fotg_pyramid_pair": "stage-level debug entry point: a stage of fotg_calc_batch, whose rows run it",
    "fotg_pyramid_pair_u8": "stage-level debug entry point: a stage of fotg_calc_batch_u8, whose row runs it",
    "fotg_grid_init": "stage-level debug entry point (PatGridClass): a stage of fotg_calc_batch, whose rows run it",
    "fotg_grid_init_from_coarser": "stage-level debug entry point (PatGridClass): a stage of fotg_calc_batch, whose rows run it",
    "fotg_grid_optimize": "stage-level debug entry point (PatGridClass): a stage of fotg_calc_batch, whose rows run it",
    "fotg_grid_aggregate": "stage-level debug entry point (PatGridClass): a stage of fotg_calc_batch, whose rows run it",
    "fotg_varref": "stage-level debug entry point (VarRefClass): a stage of fotg_calc_batch, whose rows run it",
    "fotg_bench_sor_call": "a timing hook of the solver on the context's own state: it has no inputs and no outputs to order",
}

TABLE = {}                                            # entry point -> its rows
ROWS = []
_CACHE = {}


class Row:
    def __init__(self, name, entry, file, build, call, also=(), core=False, settle=None, counter=None):
        self.name, self.entry, self.file, self._build, self.call, self.core, self.settle = name, entry, file, build, call, core, settle
        self.counter = counter                        # a launch counter of the library (fotg_debug_counter) that the call must advance
        ROWS.append(self)
        for e in (entry,) + tuple(also):
            TABLE.setdefault(e, []).append(self)

    def build(self):
        """(A, B): two lists of host arrays, built once"""
        if self.name not in _CACHE:
            A, B = self._build()
            A, B = [np.ascontiguousarray(a) for a in A], [np.ascontiguousarray(b) for b in B]
            assert [(a.shape, a.dtype) for a in A] == [(b.shape, b.dtype) for b in B], self.name
            _CACHE[self.name] = (A, B)
        return _CACHE[self.name]

    def __repr__(self):
        return self.name


def two(gen, sa=11, sb=12):
    return lambda: (gen(sa), gen(sb))


def F():
    import flowonthego_amd
    return flowonthego_amd


# ---- contexts ------------------------------------------------------------------------------------------------------------------------
_CTX = {}


def context(key, make):
    if key not in _CTX:
        _CTX[key] = make()
    return _CTX[key]


def close_all():
    for o in _CTX.values():
        o.close()
    _CTX.clear()


def fused_ctx():
    """the one context of every fused row, on every stream and thread: the fused entry points read its geometry alone"""
    from test_gpu_warp import make_ctx
    return context("fused", lambda: make_ctx(2, FUSED_W, FUSED_H, max_batch=FUSED_BATCH, bidir=True))


def core_ctx(slot, bidir=False):
    from test_gpu_warp import make_ctx
    return context(("core", slot, bidir), lambda: make_ctx(2, CORE_W, CORE_H, max_batch=2, bidir=bidir))


def fused_size():
    """(wl, hl) of the fused context's coarse flow, without a context (the CPU test builds the inputs too)"""
    op = F().operating_point(2, FUSED_W, 1).derive()
    wp, hp = F().padded_size(FUSED_W, FUSED_H, op.coarsest_scale)[:2]
    return wp >> op.finest_scale, hp >> op.finest_scale


def coarse(n, seed, scale=3.0):
    wl, hl = fused_size()
    return X.thin_flow(wl, hl, n, seed, scale)


def big(kind, n, noc, u8, seed):
    """images, masks at the fused context's frame size"""
    if kind == "mask":
        return X.thin_mask(FUSED_W, FUSED_H, n, seed)
    return X.thin_images(FUSED_W, FUSED_H, n, noc, u8, seed)


# ---- the core -------------------------------------------------------------------------------------------------------------------------
def pairs(h, w, seeds):
    from conftest import synth_pair
    ps = [synth_pair(h, w, seed=s) for s in seeds]
    return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])


def core_frames(u8=False):
    def build():
        a, b = pairs(CORE_H, CORE_W, (301, 302)), pairs(CORE_H, CORE_W, (303, 304))
        cast = (lambda t: t.astype(np.uint8)) if u8 else (lambda t: t)       # synth_pair's grey levels are whole numbers
        return [cast(t) for t in a], [cast(t) for t in b]
    return build


def core_sequence(u8=False):
    def build():
        (a0, a1), (b0, b1) = pairs(CORE_H, CORE_W, (301, 302)), pairs(CORE_H, CORE_W, (303, 304))
        A, B = np.stack([a0[0], a1[0], a0[1]]), np.stack([b0[0], b1[0], b0[1]])
        return ([A.astype(np.uint8)], [B.astype(np.uint8)]) if u8 else ([A], [B])
    return build


def tup(o):
    return tuple(o) if isinstance(o, (tuple, list)) else (o,)


CAPI = "fotg_capi.hip"
Row("calc_batch", "fotg_calc_batch", CAPI, core_frames(), lambda x, s: tup(core_ctx(s).calc_batch(*x)), core=True)
Row("calc_batch_u8", "fotg_calc_batch_u8", CAPI, core_frames(True), lambda x, s: tup(core_ctx(s).calc_batch_u8(*x)), core=True)
Row("calc_sequence", "fotg_calc_sequence", CAPI, core_sequence(), lambda x, s: tup(core_ctx(s).calc_sequence(*x)), core=True)
Row("calc_sequence_u8", "fotg_calc_sequence_u8", CAPI, core_sequence(True), lambda x, s: tup(core_ctx(s).calc_sequence(*x)), core=True)
Row("calc_bidir", "fotg_calc_bidir", CAPI, core_frames(), lambda x, s: tup(core_ctx(s, True).calc_bidirectional(*x)), core=True)
Row("calc_bidir_u8", "fotg_calc_bidir_u8", CAPI, core_frames(True), lambda x, s: tup(core_ctx(s, True).calc_bidirectional_u8(*x)), core=True)
Row("calc_sequence_bidir", "fotg_calc_sequence_bidir", CAPI, core_sequence(),
    lambda x, s: tup(core_ctx(s, True).calc_sequence_bidirectional(*x)), core=True)
Row("calc_sequence_bidir_u8", "fotg_calc_sequence_bidir_u8", CAPI, core_sequence(True),
    lambda x, s: tup(core_ctx(s, True).calc_sequence_bidirectional(*x)), core=True)

# fotg_calc_batch once per kept solver variant: the geometries of test_default_dispatch_reaches_every_kept_solver_variant
# (tests/test_gpu_parity.py); the harness reads the variant's launch counter around the call; B is A's pair the other way round
VARIANTS = ((1600, 480, 4, 5, "fused_cglobal"), (1920, 960, 4, 5, "sor_pipe"), (1920, 1080, 4, 5, "sor_stream"), (960, 544, 2, 3, "level_pipe"))


def variant_ctx(w, h, sc_l, sc_f, slot):
    def make():
        from flowonthego_amd.oflow import OFClass
        op = F().operating_point(2, w, 1)
        op.finest_scale, op.coarsest_scale, op.grad_descent_iter = sc_l, sc_f, 6
        return OFClass(op, F().img_params(width=w, height=h, padding=op.patch_size))
    return context(("variant", w, h, slot), make)


def variant_row(w, h, sc_l, sc_f, counter):
    def build():
        f0, f1 = pairs(h, w, (61,))
        return [f0, f1], [f1, f0]
    Row("calc_batch_" + counter, "fotg_calc_batch", CAPI, build, lambda x, s: tup(variant_ctx(w, h, sc_l, sc_f, s).calc_batch(*x)), core=True,
        counter=counter)


for _v in VARIANTS:
    variant_row(*_v)


def pipe(slot):
    def make():
        from flowonthego_amd.pipeline import FlowPipeline
        op = F().operating_point(2, CORE_W, 1)
        return FlowPipeline(op, F().img_params(width=CORE_W, height=CORE_H, padding=op.patch_size), max_batch=2, depth=2)
    return context(("pipe", slot), make)


def pipe_call(**kw):
    def call(x, s):
        """after_stream = the current stream, then that stream waits for the ticket on the device (host_wait = 0)"""
        ticket, out = pipe(s).submit(x[0], x[1], **kw)
        pipe(s).wait(ticket)
        return (out,)
    return call


def pipe_settle(slot):
    pipe(slot).synchronize()


Row("pipe_submit", "fotg_pipe_submit", CAPI, core_frames(), pipe_call(), also=("fotg_pipe_wait",), core=True, settle=pipe_settle)
Row("pipe_submit_u8", "fotg_pipe_submit_u8", CAPI, core_frames(True), pipe_call(), also=("fotg_pipe_wait",), core=True, settle=pipe_settle)
Row("pipe_submit_ex", "fotg_pipe_submit_ex", CAPI, core_frames(), pipe_call(no_recompute=True), also=("fotg_pipe_wait",), core=True,
    settle=pipe_settle)

Row("upsample_crop", "fotg_upsample_crop", CAPI, two(lambda s: [coarse(2, s)]), lambda x, s: tup(fused_ctx().upsample_crop(x[0])))


def gradmag(u8):
    from flowonthego_amd.oflow import gradient_magnitude
    return (two(lambda s: [X.thin_images(150, 139, 2, 3, u8, s)]), lambda x, s: tup(gradient_magnitude(x[0], 4)))


Row("gradient_magnitude", "fotg_gradient_magnitude", CAPI, *gradmag(False))
Row("gradient_magnitude_u8", "fotg_gradient_magnitude_u8", CAPI, *gradmag(True))


# ---- the add-ons ------------------------------------------------------------------------------------------------------------------
def add(entry, file, build, call, name=None):
    return Row(name or entry[5:], entry, file, build, call)


# colour code
def _color(x, s):
    from flowonthego_amd.color import flow_to_color
    return flow_to_color(x[0], stats=True)


def _color_fused(x, s):
    from flowonthego_amd.color import upsample_crop_color
    return upsample_crop_color(fused_ctx(), x[0], stats=True)


def _color_no_stats(x, s):
    """fotg_flow_color with rgb alone: the per-image keys are then the call's own stream-ordered memory, which the binding, always
    passing stats, never takes"""
    import ctypes as C
    from flowonthego_amd._args import _ptr, _stream
    from flowonthego_amd._lib import check
    n, h, w = x[0].shape[:3]
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=x[0].device)
    check(F().lib().fotg_flow_color(0, n, _ptr(x[0]), w, h, C.c_float(-1.0), _ptr(rgb), None, _stream(x[0].device)))
    return (rgb,)


def _color_fused_no_stats(x, s):
    import ctypes as C
    from flowonthego_amd._args import _ptr, _stream
    from flowonthego_amd._lib import check
    o = fused_ctx()
    n = x[0].shape[0]
    rgb = torch.empty((n, FUSED_H, FUSED_W, 3), dtype=torch.uint8, device=x[0].device)
    check(F().lib().fotg_upsample_crop_color(o._h, n, _ptr(x[0]), C.c_float(-1.0), _ptr(rgb), None, _stream(o.device)))
    return (rgb,)


add("fotg_flow_color", "fotg_color.hip", two(lambda s: [X.thin_flow(131, 67, 2, s, 6.0)]), _color)
add("fotg_flow_color", "fotg_color.hip", two(lambda s: [X.thin_flow(131, 67, 2, s, 6.0)]), _color_no_stats, name="flow_color_own_keys")
add("fotg_upsample_crop_color", "fotg_color.hip", two(lambda s: [coarse(2, s, 6.0)]), _color_fused_no_stats, name="upsample_crop_color_own_keys")
add("fotg_upsample_crop_color", "fotg_color.hip", two(lambda s: [coarse(2, s, 6.0)]), _color_fused)


# forward-backward check
def fb_pair(fw, seed, shape):
    n, h, w = shape
    return X.edge_specials(-fw + X.thin_flow(w, h, n, seed, 0.3, specials=False), 5)


def _fb_gen(s):
    fw = X.thin_flow(131, 67, 2, s)
    return [fw, fb_pair(fw, s + 50, (2, 67, 131))]


def _fb_gen_fused(s):
    fw = coarse(2, s)
    return [fw, fb_pair(fw, s + 50, fw.shape[:3])]


def _fb(x, s):
    from flowonthego_amd.consistency import fb_check
    return fb_check(x[0], x[1], stats=True)


def _fb_fused(x, s):
    from flowonthego_amd.consistency import upsample_crop_fb_check
    return upsample_crop_fb_check(fused_ctx(), x[0], x[1], stats=True, fused=True)


add("fotg_fb_check", "fotg_fbcheck.hip", two(_fb_gen), _fb)
add("fotg_upsample_crop_fb_check", "fotg_fbcheck.hip", two(_fb_gen_fused), _fb_fused)


# warp
def warp_gen(u8, noc):
    def gen(s):
        import test_gpu_warp as T
        rng = np.random.default_rng(s)
        n, h, w = 2, 67, 131
        shape = (n, h, w) + ((noc,) if noc > 1 else ())
        return [T.image(rng, shape, u8), T.odd_flow(rng, n, h, w), T.image(rng, shape, u8), X.thin_mask(w, h, n, s)]
    return two(gen)


def warp_gen_fused(u8, noc):
    return two(lambda s: [coarse(2, s), big("image", 2, noc, u8, s), big("image", 2, noc, u8, s + 1), big("mask", 2, 0, 0, s)])


def _warp(x, s):
    from flowonthego_amd.warp import warp
    return warp(x[0], x[1], ref=x[2], occ=x[3], fill=17.5, stats=True)


def _warp_fused(x, s):
    from flowonthego_amd.warp import upsample_crop_warp
    return upsample_crop_warp(fused_ctx(), x[0], x[1], ref=x[2], occ=x[3], fill=17.5, stats=True, fused=True)


WARP_FUSED = add("fotg_upsample_crop_warp", "fotg_warp.hip", warp_gen_fused(False, 1), _warp_fused)
add("fotg_warp", "fotg_warp.hip", warp_gen(False, 1), _warp)
add("fotg_warp_u8", "fotg_warp.hip", warp_gen(True, 3), _warp)
add("fotg_upsample_crop_warp_u8", "fotg_warp.hip", warp_gen_fused(True, 3), _warp_fused)


# interpolation: without masks, so that the call runs the consistency check itself and takes its own masks from the stream's pool
def interp_gen(u8, noc):
    def gen(s):
        w, h, n = 131, 67, 2
        return [X.thin_images(w, h, n, noc, u8, s + k) for k in range(3)] + [X.thin_flow(w, h, n, s), X.thin_flow(w, h, n, s + 1, 2.0)]
    return two(gen)


def interp_gen_fused(u8, noc):
    return two(lambda s: [big("image", 2, noc, u8, s + k) for k in range(3)] + [coarse(2, s), coarse(2, s + 1, 2.0)])


def _interp(x, s):
    from flowonthego_amd.interp import interpolate
    return interpolate(x[0], x[1], x[3], x[4], 0.3, ref=x[2], stats=True)


def _interp_fused(x, s):
    from flowonthego_amd.interp import upsample_crop_interpolate
    return upsample_crop_interpolate(fused_ctx(), x[3], x[4], x[0], x[1], 0.3, ref=x[2], stats=True, fused=True)


add("fotg_interp", "fotg_interp.hip", interp_gen(False, 3), _interp)
add("fotg_interp_u8", "fotg_interp.hip", interp_gen(True, 1), _interp)
add("fotg_upsample_crop_interp", "fotg_interp.hip", interp_gen_fused(False, 3), _interp_fused)
add("fotg_upsample_crop_interp_u8", "fotg_interp.hip", interp_gen_fused(True, 1), _interp_fused)


# chains and point tracks
def chain_gen(s):
    import chain_ref as R
    Fw, Bw = R.make_flows(131, 67, 2, 3, seed=s)
    return [Fw, Bw, R.make_points(131, 67, 2, 300)]


def chain_gen_fused(s):
    import chain_ref as R
    fw = coarse(3, s, 1.5)
    return [fw, fb_pair(fw, s + 50, fw.shape[:3]), R.make_points(FUSED_W, FUSED_H, 1, 300)[0]]


def _chain(x, s):
    from flowonthego_amd.chain import chain
    return chain(x[0], x[1], stats=True)


def _points(x, s):
    from flowonthego_amd.chain import track_points
    return track_points(x[2], x[0], x[1], stats=True)


def _chain_fused(x, s):
    from flowonthego_amd.chain import upsample_crop_chain
    return upsample_crop_chain(fused_ctx(), x[0], x[1], stats=True, fused=True)


def _points_fused(x, s):
    from flowonthego_amd.chain import upsample_crop_track_points
    return upsample_crop_track_points(fused_ctx(), x[2], x[0], x[1], stats=True, fused=True)


add("fotg_flow_chain", "fotg_chain.hip", two(chain_gen), _chain)
add("fotg_track_points", "fotg_chain.hip", two(chain_gen), _points)
add("fotg_upsample_crop_flow_chain", "fotg_chain.hip", two(chain_gen_fused), _chain_fused)
add("fotg_upsample_crop_track_points", "fotg_chain.hip", two(chain_gen_fused), _points_fused)


# motion fit: 640 x 420, 263 workgroups, so that the fold of the partial sums has a second round; iters = 2
FIT = dict(model="affine", iters=2, thresh=1.0, code=True, residual=True, stats=True, sums=True)


def fit_gen(s):
    import motion_ref as R
    flow, mask, _ = R.make_scene(640, 420, seed=40 + s)
    return [flow[None], mask[None]]


def _fit(x, s):
    from flowonthego_amd.motion import fit_motion
    return fit_motion(x[0], x[1], **FIT)


def _fit_fused(x, s):
    from flowonthego_amd.motion import upsample_crop_fit_motion
    return upsample_crop_fit_motion(fused_ctx(), x[0], x[1], fused=True, **FIT)


def _motion_flow(x, s):
    from flowonthego_amd.motion import motion_flow
    return tup(motion_flow(x[0], 131, 67))


def plate_motions_of(s):
    import test_gpu_plate as T
    return T.case(3, 1, True, s)[3].reshape(-1, 6)


add("fotg_fit_motion", "fotg_motion.hip", two(fit_gen), _fit)
FIT_FUSED = add("fotg_upsample_crop_fit_motion", "fotg_motion.hip", two(lambda s: [coarse(2, s), big("mask", 2, 0, 0, s)]), _fit_fused)
add("fotg_motion_flow", "fotg_motion.hip", two(lambda s: [plate_motions_of(s)]), _motion_flow)


# motion layers
def layers_gen():
    import test_gpu_layers as T
    flow, mask = T.batch(157, 93)
    return [flow[[0, 1]], mask[[0, 1]]], [flow[[1, 2]], mask[[1, 0]]]


def _layers(x, s):
    import test_gpu_layers as T
    from flowonthego_amd.layers import motion_layers
    return motion_layers(x[0], x[1], layers=3, model="affine", iters=1, rounds=2, thresh=1.0, **T.ALL)


def _layers_fused(x, s):
    import test_gpu_layers as T
    from flowonthego_amd.layers import upsample_crop_motion_layers
    return upsample_crop_motion_layers(fused_ctx(), x[0], x[1], layers=2, model="affine", iters=1, rounds=1, thresh=1.0, fused=True, **T.ALL)


add("fotg_motion_layers", "fotg_layers.hip", layers_gen, _layers)
add("fotg_upsample_crop_motion_layers", "fotg_layers.hip", two(lambda s: [coarse(2, s), big("mask", 2, 0, 0, s)]), _layers_fused)


# connected components: 67 x 45 x 3
def components_gen(s):
    import test_gpu_fill as T
    P = T.patterns(45, 67, s)[[9, 18, 19]]
    return [T.as_bytes(P, (1,), s), X.thin_flow(67, 45, 3, s)]


def _components(x, s):
    from flowonthego_amd.objects import label_components
    return label_components(x[0], (1,), 8, x[1], 1, 64, labels=True, ids=True, stats=True)


add("fotg_label_components", "fotg_components.hip", two(components_gen), _components)


# temporal filter
def temporal_gen(u8, noc):
    def gen(s):
        import test_gpu_temporal as T
        frames, ref, flows, masks = T.case(40, 130, 2, noc, u8, s)
        return [frames, ref, flows, masks]
    return two(gen)


def temporal_gen_fused(u8, noc):
    def gen(s):
        n, K = 3, 2
        return [big("image", 5, noc, u8, s), big("image", n, noc, u8, s + 1), coarse(n * K, s, 0.4),
                big("mask", n * K, 0, 0, s).reshape(n, K, FUSED_H, FUSED_W)]
    return two(gen)


def _temporal(x, s):
    import test_gpu_temporal as T
    from flowonthego_amd.temporal import temporal_filter
    return temporal_filter(x[0], T.CENTER, T.neighbors(2), x[2], masks=x[3], tau=40.0, gains=T.GAINS[:2], ref=x[1], stats=True)


def _temporal_fused(x, s):
    import test_gpu_temporal as T
    from flowonthego_amd.temporal import upsample_crop_temporal_filter
    return upsample_crop_temporal_filter(fused_ctx(), x[2], x[0], T.CENTER, T.neighbors(2), masks=x[3], tau=40.0, gains=T.GAINS[:2], ref=x[1],
                                         stats=True, fused=True)


add("fotg_temporal_filter", "fotg_temporal.hip", temporal_gen(False, 1), _temporal)
add("fotg_temporal_filter_u8", "fotg_temporal.hip", temporal_gen(True, 3), _temporal)
add("fotg_upsample_crop_temporal_filter", "fotg_temporal.hip", temporal_gen_fused(False, 1), _temporal_fused)
add("fotg_upsample_crop_temporal_filter_u8", "fotg_temporal.hip", temporal_gen_fused(True, 3), _temporal_fused)


# flow filter: three passes with statistics take four buffers from the stream's pool beside `out`; the fifth (a second vector
# buffer) is taken only without `out`, which the binding always passes, so that case calls the library itself
def filter_gen(u8, noc):
    def gen(s):
        import test_gpu_flowfilter as T
        return list(T.case(40, 130, noc, u8, s, n=2))
    return two(gen)


def filter_gen_fused(u8, noc):
    return two(lambda s: [coarse(2, s, 2.0), big("image", 2, noc, u8, s), big("mask", 2, 0, 0, s)])


FILTER = dict(radius=3, sigma=1.5, tau=40.0, iters=3, code=True, stats=True)


def _filter(x, s):
    from flowonthego_amd.flowfilter import filter_flow
    return filter_flow(x[0], x[1], mask=x[2], **FILTER)


def _filter_fused(x, s):
    from flowonthego_amd.flowfilter import upsample_crop_filter_flow
    return upsample_crop_filter_flow(fused_ctx(), x[0], x[1], mask=x[2], fused=True, **FILTER)


def _filter_no_out(x, s):
    """fotg_flow_filter with code and stats alone: the call keeps the vectors of every pass in its own two buffers"""
    import ctypes as C
    from flowonthego_amd._args import _ptr, _stream
    from flowonthego_amd._lib import check
    flow, guide, mask = x
    n, h, w = flow.shape[:3]
    code = torch.empty((n, h, w), dtype=torch.uint8, device=flow.device)
    stats = torch.empty((n, 4), dtype=torch.float64, device=flow.device)
    check(F().lib().fotg_flow_filter(0, n, _ptr(flow), _ptr(guide), w, h, 1, _ptr(mask), 2, None, C.c_float(40.0), 3, None, _ptr(code),
                    _ptr(stats), _stream(flow.device)))
    return code, stats


add("fotg_flow_filter", "fotg_flowfilter.hip", filter_gen(False, 3), _filter)
add("fotg_flow_filter", "fotg_flowfilter.hip", filter_gen(False, 1), _filter_no_out, name="flow_filter_five_buffers")
add("fotg_flow_filter_u8", "fotg_flowfilter.hip", filter_gen(True, 1), _filter)
add("fotg_upsample_crop_flow_filter", "fotg_flowfilter.hip", filter_gen_fused(False, 3), _filter_fused)
add("fotg_upsample_crop_flow_filter_u8", "fotg_flowfilter.hip", filter_gen_fused(True, 1), _filter_fused)


# block motion
def block_gen(s):
    import blockmotion_ref as R
    return list(R.scene(40, 130, 3, 1000 + s, n=2))


BLOCK = dict(block=16, refine=2, pred=True, stats=True)


def _block(x, s):
    from flowonthego_amd.blockmotion import block_motion
    return block_motion(x[0], x[1], x[2], mask=x[3], **BLOCK)


def _block_fused(x, s):
    from flowonthego_amd.blockmotion import upsample_crop_block_motion
    return upsample_crop_block_motion(fused_ctx(), x[2], x[0], x[1], mask=x[3], fused=True, **BLOCK)


add("fotg_block_motion", "fotg_blockmotion.hip", two(block_gen), _block)
add("fotg_upsample_crop_block_motion", "fotg_blockmotion.hip",
    two(lambda s: [big("image", 2, 3, True, s), big("image", 2, 3, True, s + 1), coarse(2, s), big("mask", 2, 0, 0, s)]), _block_fused)


# object tracks
def overlap_gen(s):
    import test_gpu_tracks as T
    a, b, _, _, flow, mask = T.scene(40, 130, seed=s)
    return [a, b, flow, mask]


def big_ids():
    import test_gpu_histograms as T
    return T.scene(FUSED_H, FUSED_W)[3]


def links_gen(s):
    import test_gpu_tracks as T
    import tracks_ref as R
    a, b, oa, ob, flow, mask = T.scene(19, 67, seed=s)
    return [R.overlap_batch(a, b, flow, mask, T.K, T.K)[0], oa, ob]


def tracks_gen(s):
    import test_gpu_tracks as T
    import tracks_ref as R
    ids, objects, flows = T.sequence(19, 67, seed=s)
    votes = R.overlap_batch(ids[:-1], ids[1:], flows, None, T.K, T.K)[0]
    ab, ba = R.links_batch(votes, objects[:-1], objects[1:], 1, 64)
    return [objects, ab.astype(np.int32), ba.astype(np.int32)]


def _overlap(x, s):
    import test_gpu_tracks as T
    from flowonthego_amd.tracks import object_overlap
    return object_overlap(x[0], x[1], x[2], x[3], T.K, T.K)


def _overlap_fused(x, s):
    import test_gpu_histograms as T
    from flowonthego_amd.tracks import upsample_crop_object_overlap
    return upsample_crop_object_overlap(fused_ctx(), x[0], x[1], x[2], mask=x[3], ka=T.K, kb=T.K, fused=True)


def _links(x, s):
    from flowonthego_amd.tracks import object_links
    return object_links(x[0], x[1], x[2], min_votes=1, min_frac=0.25)


def _tracks(x, s):
    from flowonthego_amd.tracks import link_tracks
    return link_tracks(x[0], x[1], x[2], max_tracks=64, stats=True)


add("fotg_object_overlap", "fotg_objtracks.hip", two(overlap_gen, 0, 1), _overlap)
add("fotg_upsample_crop_object_overlap", "fotg_objtracks.hip",
    two(lambda s: [coarse(2, s), big_ids()[:2], big_ids()[1:3], big("mask", 2, 0, 0, s)]), _overlap_fused)
add("fotg_object_links", "fotg_objtracks.hip", two(links_gen, 0, 1), _links)
add("fotg_object_tracks", "fotg_objtracks.hip", two(tracks_gen, 3, 4), _tracks)


# motion histograms
def hist_gen():
    import test_gpu_histograms as T
    sc = T.scene(40, 130)
    return [a[[0, 1]] for a in sc], [a[[2, 0]] for a in sc]


def hist_gen_fused(s):
    import test_gpu_histograms as T
    _, mask, params, ids = T.scene(FUSED_H, FUSED_W)
    k = [s % 3, (s + 1) % 3]
    return [coarse(2, s), mask[k], params[k], ids[k]]


def _hist(x, s):
    import test_gpu_histograms as T
    from flowonthego_amd.histograms import motion_histograms
    return motion_histograms(x[0], x[1], x[2], cell=8, thresh=0.4, ids=x[3], rows=T.K, cells=True)


def _hist_fused(x, s):
    import test_gpu_histograms as T
    from flowonthego_amd.histograms import upsample_crop_motion_histograms
    return upsample_crop_motion_histograms(fused_ctx(), x[0], x[1], x[2], cell=8, thresh=0.4, ids=x[3], rows=T.K, cells=True, fused=True)


add("fotg_motion_histograms", "fotg_histograms.hip", hist_gen, _hist)
add("fotg_upsample_crop_motion_histograms", "fotg_histograms.hip", two(hist_gen_fused), _hist_fused)


# motion blur
def blur_gen():
    import test_gpu_motionblur as T
    flow, mask, frames = T.scene(40, 130)
    fr = frames["u8-3"]
    return [fr[[0, 1]], flow[[0, 1]], mask[[0, 1]]], [fr[[2, 0]], flow[[2, 0]], mask[[2, 0]]]


def _blur(x, s):
    import test_gpu_motionblur as T
    from flowonthego_amd.motionblur import motion_blur
    return motion_blur(x[0], x[1], x[2], **T.ALL)


def _blur_fused(x, s):
    import test_gpu_motionblur as T
    from flowonthego_amd.motionblur import upsample_crop_motion_blur
    return upsample_crop_motion_blur(fused_ctx(), x[1], x[0], x[2], fused=True, **T.ALL)


add("fotg_motion_blur", "fotg_motionblur.hip", blur_gen, _blur)
add("fotg_upsample_crop_motion_blur", "fotg_motionblur.hip",
    two(lambda s: [big("image", 2, 1, False, s), coarse(2, s, 6.0), big("mask", 2, 0, 0, s)]), _blur_fused)


# background plate; the index is a host argument: both sets use set A's
PLATE = dict(mode="median", min_count=1, fill=7.25, count=True, code=True, stats=True)


def plate_index():
    import test_gpu_plate as T
    if "plate_index" not in _CACHE:
        _CACHE["plate_index"] = T.case(3, 1, True, 11)[1].tolist()
    return _CACHE["plate_index"]


def plate_gen(u8, noc):
    def gen(s):
        import test_gpu_plate as T
        frames, _, flows, motions, occ, exclude, ref = T.case(3, noc, u8, s)
        return [frames, flows, motions, occ, exclude, ref]
    return two(gen)


def plate_gen_fused(u8, noc):
    def gen(s):
        n, K = 2, 3
        return [big("image", 6, noc, u8, s), coarse(n * K, s, 2.0), big("mask", n * K, 0, 0, s).reshape(n, K, FUSED_H, FUSED_W),
                big("mask", 6, 0, 0, s + 1), big("image", n, noc, u8, s + 2)]
    return two(gen)


def _plate(source):
    def call(x, s):
        import test_gpu_plate as T
        from flowonthego_amd.plate import background_plate
        W, H, ox, oy = T.CANVAS
        src = dict(flows=x[1]) if source == "flows" else dict(motions=x[2])
        return background_plate(x[0], plate_index(), canvas=(W, H), origin=(ox, oy), occ=x[3], exclude=x[4], ref=x[5], **src, **PLATE)
    return call


def _plate_fused(x, s):
    from flowonthego_amd.plate import upsample_crop_background_plate
    return upsample_crop_background_plate(fused_ctx(), x[1], x[0], plate_index(), occ=x[2], exclude=x[3], ref=x[4], fused=True, **PLATE)


add("fotg_plate", "fotg_plate.hip", plate_gen(False, 1), _plate("flows"))
add("fotg_plate_u8", "fotg_plate.hip", plate_gen(True, 3), _plate("flows"))
add("fotg_plate_motion", "fotg_plate.hip", plate_gen(False, 3), _plate("motions"))
add("fotg_plate_motion_u8", "fotg_plate.hip", plate_gen(True, 1), _plate("motions"))
add("fotg_upsample_crop_plate", "fotg_plate.hip", plate_gen_fused(False, 1), _plate_fused)
add("fotg_upsample_crop_plate_u8", "fotg_plate.hip", plate_gen_fused(True, 3), _plate_fused)


# background subtraction and object removal: case(..., (33, 129), ...); the plate index is a host argument: set A's
SMALL, SMALL_CANVAS = (33, 129), (131, 30, 1, -2)
BIG_CANVAS = (FUSED_W + 4, FUSED_H + 4, 2, -1)
SUBTRACT = dict(low=20.0, high=60.0, window=1, code=True, diff=True, evidence=True, stats=True)
ERASE = dict(grow=2, feather=3, dst=True, code=True, alpha=True, stats=True)


def plate_case(u8, noc, fused):
    def gen(s):
        import test_gpu_subtract as T
        frame, canvas, n = ((FUSED_H, FUSED_W), BIG_CANVAS, 2) if fused else (SMALL, SMALL_CANVAS, 3)
        import test_gpu_erase as E
        frames, plates, _, flows, motions, pcode, mask = T.case(noc, u8, s, frame, canvas, n, 2)
        return [frames, plates, coarse(2, s, 2.0) if fused else flows, motions, pcode, mask, E.removal(frame, n)]
    return two(gen)


def plate_of(fused):
    """(the plate of every frame, the origin)"""
    return ([1, 0] if fused else [0, 1, 1]), (BIG_CANVAS if fused else SMALL_CANVAS)[2:]


def _subtract(source):
    def call(x, s):
        from flowonthego_amd.subtract import subtract_background
        index, origin = plate_of(False)
        src = dict(flows=x[2]) if source == "flows" else dict(motions=x[3])
        return subtract_background(x[0], x[1], index=index, origin=origin, plate_code=x[4], mask=x[5], **src, **SUBTRACT)
    return call


def _subtract_fused(x, s):
    from flowonthego_amd.subtract import upsample_crop_subtract_background
    index, origin = plate_of(True)
    return upsample_crop_subtract_background(fused_ctx(), x[2], x[0], x[1], index=index, origin=origin, plate_code=x[4], mask=x[5], fused=True,
                                             **SUBTRACT)


def _erase(source):
    def call(x, s):
        from flowonthego_amd.erase import remove_objects
        index, origin = plate_of(False)
        src = dict(flows=x[2]) if source == "flows" else dict(motions=x[3])
        return remove_objects(x[0], x[1], x[6], index=index, origin=origin, plate_code=x[4], mask=x[5], **src, **ERASE)
    return call


def _erase_fused(x, s):
    from flowonthego_amd.erase import upsample_crop_remove_objects
    index, origin = plate_of(True)
    return upsample_crop_remove_objects(fused_ctx(), x[2], x[0], x[1], x[6], index=index, origin=origin, plate_code=x[4], mask=x[5], fused=True,
                                        **ERASE)


for _nm, _u8, _noc, _src in (("", False, 1, "flows"), ("_u8", True, 3, "flows"), ("_motion", False, 3, "motions"), ("_motion_u8", True, 1, "motions")):
    add("fotg_subtract" + _nm, "fotg_subtract.hip", plate_case(_u8, _noc, False), _subtract(_src))
    add("fotg_erase" + _nm, "fotg_erase.hip", plate_case(_u8, _noc, False), _erase(_src))
for _nm, _u8, _noc in (("", False, 1), ("_u8", True, 3)):
    add("fotg_upsample_crop_subtract" + _nm, "fotg_subtract.hip", plate_case(_u8, _noc, True), _subtract_fused)
    add("fotg_upsample_crop_erase" + _nm, "fotg_erase.hip", plate_case(_u8, _noc, True), _erase_fused)


# morphology: two stages in one launch
def morph_gen(s):
    import test_gpu_fill as T
    import test_gpu_morph as M
    return [M.as_bytes(T.patterns(139, 150, s)[[19, 20]], (1, 4), s)]          # the two seeded patterns: the sets differ with the seed


def _morph(x, s):
    from flowonthego_amd.morph import chain
    return chain(x[0], [("dilate", 1), ("erode", 1)], fg=(1, 4), out=True, stats=True)


add("fotg_morph", "fotg_morph.hip", two(morph_gen), _morph)


# hole filling: 139 x 150, levels above the tile's
def fill_gen(dtype, ch):
    def gen(s):
        import test_gpu_fill as T
        return [np.stack([T.frame((139, 150), ch, dtype, 10 * s + k) for k in range(2)]), T.as_bytes(T.patterns(139, 150, s)[[9, 18]], None, s)]
    return two(gen)


def _fill(x, s):
    from flowonthego_amd.fill import fill_holes
    return fill_holes(x[0], x[1], dst=True, code=True, stats=True)


def _fill_flow_fused(x, s):
    """the composition fotg_upsample_crop + fotg_fill that test D runs on a shared context; it has no entry point of its own"""
    from flowonthego_amd.fill import upsample_crop_fill_flow
    return tup(upsample_crop_fill_flow(fused_ctx(), x[0], x[1]))


add("fotg_fill", "fotg_fill.hip", fill_gen(f32, 2), _fill)
add("fotg_fill_u8", "fotg_fill.hip", fill_gen(np.uint8, 3), _fill)
FILL_FLOW_FUSED = add("fotg_fill", "fotg_fill.hip", two(lambda s: [coarse(2, s), big("mask", 2, 0, 0, s)]), _fill_flow_fused, name="fill_flow_fused")

assert len({r.name for r in ROWS}) == len(ROWS)
ADDON_ROWS = [r for r in ROWS if not r.core]          # what host threads may share: no row of these owns a context


def files():
    return sorted({r.file for r in ROWS})
