"""Host-side mirror of the reference's flow orchestrator API (src/oflow.h:22-46, src/patchgrid.h:13-86,
src/refine_variational.h:35-57) over the C-ABI of libfotg.so.  Same class and method names, argument meaning and
ownership as the reference; PyTorch is used only to hold device memory and streams.

    ofc = OFClass(op, iparams)                       # src/run_dense.cpp:277
    ofc.calc(I0, I1, iparams, None, outflow)         # src/run_dense.cpp:286

Numerics are those of the reference's kroeger/ CPU implementation, evaluated by hand-written HIP
kernels; nothing here computes on the CPU and there is no fallback path.
"""
import atexit
import ctypes as C
import sys
import weakref

import torch

from ._args import _dev_f32, _ptr, _stream
from ._lib import FotgError, check, lib
from .params import img_params, opt_params, padded_size


_LIVE = weakref.WeakSet()
# id(opt_params handed out by an OFClass) -> that OFClass: how PatGridClass(_i_params, _op) and VarRefClass(.., _op, ..) -- the
# reference's constructor signatures, src/patchgrid.h:16 and src/refine_variational.h:38-39 -- find their engine context
# (the same registry the C++ shim keeps, include/fotg/patchgrid.h)
_REGISTRY = weakref.WeakValueDictionary()


def _context_of(_op):
    ofc = _REGISTRY.get(id(_op))
    if ofc is None or ofc._h is None:
        raise FotgError("these opt_params do not belong to a live OFClass (use the object's own `ofc.op`, as src/oflow.cpp:101,332 do)")
    return ofc


@atexit.register
def _close_all():
    # destroy contexts while the HIP runtime is still alive (not from __del__ during interpreter shutdown)
    for o in list(_LIVE):
        o.close()


class OFClass:
    """src/oflow.h:22-46.  One object = one fixed (size, parameters) configuration, reusable across calc() calls.

    iparams.width/height may be the ORIGINAL frame size: the replicate padding to multiples of 2^coarsest_scale that
    the reference's driver does first (src/run_dense.cpp:231-253) is folded into the pyramid kernel.  Passing already
    padded frames (the reference's calling convention) is the special case pad = 0.
    """

    def __init__(self, _op: opt_params, _i_params: img_params, max_batch: int = 1, device: int = 0):
        self.op = _op.derive()
        self.max_batch = int(max_batch)
        self.width_org, self.height_org = int(_i_params.width), int(_i_params.height)
        self.width, self.height, self.padw, self.padh = padded_size(self.width_org, self.height_org, self.op.coarsest_scale)
        if _i_params.padding not in (0, self.op.patch_size):
            raise FotgError("img_params.padding must equal patch_size (src/run_dense.cpp:263)")
        self.device = torch.device("cuda", device)
        self.nch = 1 if self.op.depth_mode else 2          # flow channels (stereo depth: one displacement, kroeger/oflow.cpp:76-80)
        h = C.c_void_p()
        cp = self.op.to_c()
        check(lib().fotg_create(cp, self.width_org, self.height_org, device, self.max_batch, h))
        self._h = h
        _LIVE.add(self)
        _REGISTRY[id(self.op)] = self
        check(lib().fotg_set_verbosity(self._h, int(self.op.verbosity)))
        # per-scale img_params exactly as src/oflow.cpp:84-95
        self.iparams = []
        ps = self.op.patch_size
        for i in range(self.op.n_scales):
            sl = self.op.finest_scale + i
            w, hh = self.width >> sl, self.height >> sl
            self.iparams.append(img_params(width=w, height=hh, padding=ps, l_bound=-ps / 2.0,
                                           u_bound_width=float(w + ps // 2 - 2), u_bound_height=float(hh + ps // 2 - 2),
                                           width_pad=w + 2 * ps, height_pad=hh + 2 * ps, scale_fact=2.0 ** -sl, curr_lvl=sl))
        self.grid = [PatGridClass(ip, self.op) for ip in self.iparams]        # src/oflow.cpp:101

    # -- geometry -------------------------------------------------------------------------------------------
    def out_size(self):
        w, h = C.c_int(), C.c_int()
        check(lib().fotg_out_size(self._h, w, h))
        return w.value, h.value

    def new_outflow(self, n=1):
        w, h = self.out_size()
        return torch.empty((n, h, w, self.nch), dtype=torch.float32, device=self.device)

    # -- the reference call ---------------------------------------------------------------------------------
    def calc(self, _I0, _I1, _iparams=None, initflow=None, outflow=None):
        """src/oflow.cpp:211-368.  _I0/_I1: device tensors (h, w, channels) or (h, w) float32; outflow: device tensor
        (h/2^finest, w/2^finest, 2), allocated if None.  Returns outflow."""
        single = _I0.dim() == (2 if self.op.channels == 1 else 3)
        I0 = _I0.unsqueeze(0) if single else _I0
        I1 = _I1.unsqueeze(0) if single else _I1
        out = self.calc_batch(I0, I1, initflow, None if outflow is None else (outflow.unsqueeze(0) if single else outflow))
        return out[0] if single else out

    def calc_batch(self, I0, I1, initflow=None, outflow=None):
        """n frame pairs at once: I0, I1 (n, h, w[, channels]); outflow (n, h_l, w_l, 2)"""
        I0, I1 = _dev_f32(I0, "I0", self.device), _dev_f32(I1, "I1", self.device)
        n = I0.shape[0]
        exp = (n, self.height_org, self.width_org) + ((self.op.channels,) if self.op.channels > 1 else ())
        if tuple(I0.shape) != exp and tuple(I0.shape) != exp + (1,):
            raise FotgError("frame shape %s does not match the configured %s" % (tuple(I0.shape), exp))
        if I1.shape != I0.shape:
            raise FotgError("I0 and I1 differ in shape")
        outflow, initflow = self._flow_args(n, outflow, initflow)
        check(lib().fotg_calc_batch(self._h, n, _ptr(I0), _ptr(I1), _ptr(initflow), _ptr(outflow), _stream(self.device)))
        return outflow

    def _flow_args(self, n, outflow, initflow):
        """outflow (n, Hp >> finest, Wp >> finest, nch), allocated if None; initflow None or (n, Hp >> (coarsest+1),
        Wp >> (coarsest+1), nch) -- the sizes fotg_calc_batch reads and writes (include/fotg.h)"""
        if n < 1 or n > self.max_batch:
            raise FotgError("batch of %d pairs, context created for max_batch = %d" % (n, self.max_batch))
        w, h = self.out_size()
        if outflow is None:
            outflow = torch.empty((n, h, w, self.nch), dtype=torch.float32, device=self.device)
        _dev_f32(outflow, "outflow", self.device, (n, h, w, self.nch))
        if initflow is not None:
            sc = self.op.coarsest_scale + 1
            _dev_f32(initflow, "initflow", self.device, (n, self.height >> sc, self.width >> sc, self.nch))
        return outflow, initflow

    def calc_batch_u8(self, I0, I1, initflow=None, outflow=None):
        """n pairs of 8-bit frames (n, h, w[, channels]) uint8 on the device; same result as calc_batch on float frames"""
        for t, nm in ((I0, "I0"), (I1, "I1")):
            _dev_f32(t, nm, self.device, dtype=torch.uint8)
        n = I0.shape[0]
        exp = (n, self.height_org, self.width_org) + self._u8_channels()
        if tuple(I0.shape) != exp or I1.shape != I0.shape:
            raise FotgError("frame shape %s does not match the configured %s" % (tuple(I0.shape), exp))
        outflow, initflow = self._flow_args(n, outflow, initflow)
        check(lib().fotg_calc_batch_u8(self._h, n, _ptr(I0), _ptr(I1), _ptr(initflow), _ptr(outflow), _stream(self.device)))
        return outflow

    def _u8_channels(self):
        """trailing shape of an 8-bit frame: (3,) for colour frames converted to gray on load (op.u8_color)"""
        return (3,) if self.op.u8_color else ((self.op.channels,) if self.op.channels > 1 else ())

    def calc_sequence(self, frames, initflow=None, outflow=None):
        """video mode: frames (n+1, h, w[, channels]) float32 or uint8 on the device -> the n flows frame k -> k+1; every
        frame's pyramid is built once.  Same bits as calc_batch(frames[:-1], frames[1:])"""
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.is_contiguous() and frames.dtype in (torch.float32, torch.uint8)):
            raise FotgError("frames must be a contiguous float32 or uint8 CUDA(HIP) tensor")
        if frames.device != self.device:
            raise FotgError("frames live on %s, the context on %s" % (frames.device, self.device))
        n = frames.shape[0] - 1
        exp = (n + 1, self.height_org, self.width_org) + (self._u8_channels() if frames.dtype == torch.uint8 else ((self.op.channels,) if self.op.channels > 1 else ()))
        if n < 1 or tuple(frames.shape) != exp:
            raise FotgError("frame shape %s does not match the configured %s" % (tuple(frames.shape), exp))
        outflow, initflow = self._flow_args(n, outflow, initflow)
        fn = lib().fotg_calc_sequence if frames.dtype == torch.float32 else lib().fotg_calc_sequence_u8
        check(fn(self._h, n + 1, _ptr(frames), _ptr(initflow), _ptr(outflow), _stream(self.device)))
        return outflow

    # -- both directions (op.bidir) --------------------------------------------------------------------------
    def _bidir_args(self, n, outflow, outflow_bw, initflow, initflow_bw):
        if not self.op.bidir:
            raise FotgError("calc_bidirectional needs a context created with opt_params.bidir = True")
        outflow, initflow = self._flow_args(n, outflow, initflow)
        outflow_bw, initflow_bw = self._flow_args(n, outflow_bw, initflow_bw)
        return outflow, outflow_bw, initflow, initflow_bw

    def calc_bidirectional(self, I0, I1, initflow=None, initflow_bw=None, outflow=None, outflow_bw=None):
        """both directions of n pairs from one pyramid per frame -> (fw, bw): fw == calc_batch(I0, I1, initflow) and
        bw == calc_batch(I1, I0, initflow_bw), bit for bit"""
        I0, I1 = _dev_f32(I0, "I0", self.device), _dev_f32(I1, "I1", self.device)
        n = I0.shape[0]
        exp = (n, self.height_org, self.width_org) + ((self.op.channels,) if self.op.channels > 1 else ())
        if (tuple(I0.shape) != exp and tuple(I0.shape) != exp + (1,)) or I1.shape != I0.shape:
            raise FotgError("frame shape %s does not match the configured %s" % (tuple(I0.shape), exp))
        fw, bw, ifw, ibw = self._bidir_args(n, outflow, outflow_bw, initflow, initflow_bw)
        check(lib().fotg_calc_bidir(self._h, n, _ptr(I0), _ptr(I1), _ptr(ifw), _ptr(ibw), _ptr(fw), _ptr(bw), _stream(self.device)))
        return fw, bw

    def calc_bidirectional_u8(self, I0, I1, initflow=None, initflow_bw=None, outflow=None, outflow_bw=None):
        """calc_bidirectional on 8-bit frames (the layout of calc_batch_u8)"""
        for t, nm in ((I0, "I0"), (I1, "I1")):
            _dev_f32(t, nm, self.device, dtype=torch.uint8)
        n = I0.shape[0]
        exp = (n, self.height_org, self.width_org) + self._u8_channels()
        if tuple(I0.shape) != exp or I1.shape != I0.shape:
            raise FotgError("frame shape %s does not match the configured %s" % (tuple(I0.shape), exp))
        fw, bw, ifw, ibw = self._bidir_args(n, outflow, outflow_bw, initflow, initflow_bw)
        check(lib().fotg_calc_bidir_u8(self._h, n, _ptr(I0), _ptr(I1), _ptr(ifw), _ptr(ibw), _ptr(fw), _ptr(bw), _stream(self.device)))
        return fw, bw

    def calc_sequence_bidirectional(self, frames, initflow=None, initflow_bw=None, outflow=None, outflow_bw=None):
        """video mode, both directions: frames (n+1, ...) float32 or uint8 -> (fw, bw), fw[k] the flow frame k -> k+1 and
        bw[k] the flow frame k+1 -> k; every frame's pyramid is built once"""
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.is_contiguous() and frames.dtype in (torch.float32, torch.uint8)):
            raise FotgError("frames must be a contiguous float32 or uint8 CUDA(HIP) tensor")
        if frames.device != self.device:
            raise FotgError("frames live on %s, the context on %s" % (frames.device, self.device))
        n = frames.shape[0] - 1
        exp = (n + 1, self.height_org, self.width_org) + (self._u8_channels() if frames.dtype == torch.uint8 else ((self.op.channels,) if self.op.channels > 1 else ()))
        if n < 1 or tuple(frames.shape) != exp:
            raise FotgError("frame shape %s does not match the configured %s" % (tuple(frames.shape), exp))
        fw, bw, ifw, ibw = self._bidir_args(n, outflow, outflow_bw, initflow, initflow_bw)
        fn = lib().fotg_calc_sequence_bidir if frames.dtype == torch.float32 else lib().fotg_calc_sequence_bidir_u8
        check(fn(self._h, n + 1, _ptr(frames), _ptr(ifw), _ptr(ibw), _ptr(fw), _ptr(bw), _stream(self.device)))
        return fw, bw

    def upsample_crop(self, flow, out=None):
        """src/run_dense.cpp:293-303: x 2^finest, bilinear upsample, crop the padding -> (n, h_org, w_org, 2)"""
        n = flow.shape[0] if isinstance(flow, torch.Tensor) and flow.dim() == 4 else 0
        if n < 1 or n > self.max_batch:
            raise FotgError("flow must be (n, h_l, w_l, %d) with 1 <= n <= max_batch" % self.nch)
        w, h = self.out_size()
        flow = _dev_f32(flow, "flow", self.device, (n, h, w, self.nch))
        if out is None:
            out = torch.empty((n, self.height_org, self.width_org, self.nch), dtype=torch.float32, device=self.device)
        _dev_f32(out, "out", self.device, (n, self.height_org, self.width_org, self.nch))
        check(lib().fotg_upsample_crop(self._h, n, _ptr(flow), _ptr(out), _stream(self.device)))
        return out

    def upsample_crop_color(self, flow, maxmotion=None, out=None, stats=False):
        """the Middlebury colour code of upsample_crop(flow), fused: uint8 (n, h_org, w_org, 3) -- flowonthego_amd.color"""
        from .color import upsample_crop_color
        return upsample_crop_color(self, flow, maxmotion=maxmotion, out=out, stats=stats)

    def upsample_crop_fb_check(self, flow, flow_bw, alpha1=0.01, alpha2=0.5, stats=False, fused=False):
        """forward-backward consistency masks of upsample_crop(flow) / upsample_crop(flow_bw) -- flowonthego_amd.consistency"""
        from .consistency import upsample_crop_fb_check
        return upsample_crop_fb_check(self, flow, flow_bw, alpha1=alpha1, alpha2=alpha2, stats=stats, fused=fused)

    def upsample_crop_warp(self, flow, src, ref=None, occ=None, fill=None, stats=False, fused=True):
        """src pulled back along upsample_crop(flow), with validity codes and photometric residuals -- flowonthego_amd.warp"""
        from .warp import upsample_crop_warp
        return upsample_crop_warp(self, flow, src, ref=ref, occ=occ, fill=fill, stats=stats, fused=fused)

    def upsample_crop_chain(self, flows, flows_bw=None, alpha1=0.01, alpha2=0.5, stats=False, fused=None):
        """the T coarse flows of one sequence chained: displacement frame 0 -> T, codes, steps -- flowonthego_amd.chain"""
        from .chain import upsample_crop_chain
        return upsample_crop_chain(self, flows, flows_bw, alpha1=alpha1, alpha2=alpha2, stats=stats, fused=fused)

    def upsample_crop_track_points(self, points, flows, flows_bw=None, alpha1=0.01, alpha2=0.5, stats=False, fused=False):
        """points (P, 2) followed through the T coarse flows of one sequence: trajectories, codes, steps -- flowonthego_amd.chain"""
        from .chain import upsample_crop_track_points
        return upsample_crop_track_points(self, points, flows, flows_bw, alpha1=alpha1, alpha2=alpha2, stats=stats, fused=fused)

    def track(self, frames, points=None, alpha1=0.01, alpha2=0.5, stats=False, fused=None):
        """the flows of frames (T+1, ...) and their chain: every pixel of frame 0 (points=None) or the given points followed to
        frame T, with an occlusion test per step on a bidir context -- flowonthego_amd.chain"""
        from .chain import track
        return track(self, frames, points=points, alpha1=alpha1, alpha2=alpha2, stats=stats, fused=fused)

    def upsample_crop_fit_motion(self, flow, mask=None, model="affine", iters=3, thresh=1.0, code=False, residual=False, stats=False,
                                 sums=False, fused=None):
        """the camera motion that explains upsample_crop(flow), and the pixels that do not follow it -- flowonthego_amd.motion"""
        from .motion import upsample_crop_fit_motion
        return upsample_crop_fit_motion(self, flow, mask, model=model, iters=iters, thresh=thresh, code=code, residual=residual,
                                        stats=stats, sums=sums, fused=fused)

    def camera_motion(self, frames, model="affine", iters=3, thresh=1.0, fused=None):
        """the flows of frames (T+1, ...) and the motion fitted to each: (T, 6) float64, occluded pixels left out on a bidir context
        -- flowonthego_amd.motion"""
        from .motion import camera_motion
        return camera_motion(self, frames, model=model, iters=iters, thresh=thresh, fused=fused)

    def stabilize(self, frames, model="similarity", radius=15, fill=None, stats=False, iters=3, thresh=1.0):
        """the flows of frames (T+1, ...), their camera path, and the frames resampled along the smoothed path: (frames, codes[,
        statistics]) -- flowonthego_amd.motion.stabilize"""
        from .motion import ofc_stabilize
        return ofc_stabilize(self, frames, model=model, radius=radius, fill=fill, stats=stats, iters=iters, thresh=thresh)

    def upsample_crop_motion_layers(self, coarse, mask=None, layers=3, model="affine", iters=3, rounds=3, thresh=1.0, init=None,
                                    labels=False, residual=False, records=False, stats=False, sums=False, fused=False):
        """up to `layers` motions fitted to upsample_crop(coarse), every pixel given to the nearest: params (n, K, 6) and what was
        asked for -- flowonthego_amd.layers"""
        from .layers import upsample_crop_motion_layers
        return upsample_crop_motion_layers(self, coarse, mask, layers=layers, model=model, iters=iters, rounds=rounds, thresh=thresh,
                                           init=init, labels=labels, residual=residual, records=records, stats=stats, sums=sums, fused=fused)

    def motion_layers(self, frames, layers=3, model="affine", iters=3, rounds=3, thresh=1.0, labels=False, residual=False, records=False,
                      stats=False, sums=False, fused=False):
        """the flows of frames (T+1, ...) and the motion layers of each: params (T, K, 6) and what was asked for, occluded pixels
        left out on a bidir context -- flowonthego_amd.layers"""
        from .layers import ofc_motion_layers
        return ofc_motion_layers(self, frames, layers=layers, model=model, iters=iters, rounds=rounds, thresh=thresh, labels=labels,
                                 residual=residual, records=records, stats=stats, sums=sums, fused=fused)

    def moving_objects(self, frames, model="affine", iters=3, thresh=1.0, min_area=64, max_objects=256, connectivity=8, ids=False,
                       stats=False):
        """the flows of frames (T+1, ...), the camera motion of each, and the pixels that do not follow it grouped into objects:
        (params (T, 6), objects (T, max_objects, 11)[, ids][, stats]) -- flowonthego_amd.objects"""
        from .objects import ofc_moving_objects
        return ofc_moving_objects(self, frames, model=model, iters=iters, thresh=thresh, min_area=min_area, max_objects=max_objects,
                                  connectivity=connectivity, ids=ids, stats=stats)

    def upsample_crop_temporal_filter(self, flows, frames, center, neighbors, masks=None, tau=30.0, gains=None, ref=None, stats=False,
                                      fused=True):
        """the centre frames filtered with their neighbours pulled onto them along upsample_crop(flows), flows (n K, h_l, w_l, 2)
        of the pairs (centre, neighbour) -- flowonthego_amd.temporal"""
        from .temporal import upsample_crop_temporal_filter
        return upsample_crop_temporal_filter(self, flows, frames, center, neighbors, masks=masks, tau=tau, gains=gains, ref=ref,
                                             stats=stats, fused=fused)

    def temporal_filter(self, frames, radius=1, tau=30.0, gains=None, occlusion=False, ref=None, stats=False):
        """every frame of the stack (T, ...) averaged with its neighbours at distance +-1 .. +-radius, each pulled onto it along
        its own flow and weighted by the local photometric difference (temporal denoising) -- flowonthego_amd.temporal"""
        from .temporal import ofc_temporal_filter
        return ofc_temporal_filter(self, frames, radius=radius, tau=tau, gains=gains, occlusion=occlusion, ref=ref, stats=stats)

    def upsample_crop_filter_flow(self, flow, guide, mask=None, radius=3, sigma=None, spatial=None, tau=20.0, iters=1, code=None,
                                  stats=False, fused=True):
        """upsample_crop(flow) filtered edge- and occlusion-aware with guide (n, h_org, w_org[, c]) and mask, fused: the unfiltered
        full-resolution flow is never written -- flowonthego_amd.flowfilter"""
        from .flowfilter import upsample_crop_filter_flow
        return upsample_crop_filter_flow(self, flow, guide, mask=mask, radius=radius, sigma=sigma, spatial=spatial, tau=tau,
                                         iters=iters, code=code, stats=stats, fused=fused)

    def calc_filtered(self, I0, I1, radius=3, sigma=None, spatial=None, tau=20.0, iters=1, occlusion=True, both=False, code=None,
                      stats=False):
        """the full-resolution flow of n pairs, filtered with I0 as guide; occlusion=True (a bidir context) leaves the vectors the
        forward-backward check rejects out and fills them from their neighbours; both=True also returns the backward flow
        filtered with I1 -- flowonthego_amd.flowfilter"""
        from .flowfilter import ofc_calc_filtered
        return ofc_calc_filtered(self, I0, I1, radius=radius, sigma=sigma, spatial=spatial, tau=tau, iters=iters,
                                 occlusion=occlusion, both=both, code=code, stats=stats)

    def upsample_crop_block_motion(self, flow, cur, ref, mask=None, block=16, refine=2, pred=False, stats=False, fused=True):
        """one quarter-pel motion vector per block x block pixels of cur, predicting it from ref, chosen among the vectors
        upsample_crop(flow) proposes, with its SAD; fused: the full-resolution flow is never written -- flowonthego_amd.blockmotion"""
        from .blockmotion import upsample_crop_block_motion
        return upsample_crop_block_motion(self, flow, cur, ref, mask=mask, block=block, refine=refine, pred=pred, stats=stats,
                                          fused=fused)

    def block_motion(self, I0, I1, block=16, refine=2, occlusion=False, pred=False, stats=False):
        """the flow of n 8-bit frame pairs and the block motion vectors that predict I0 from I1, in one call: (flow, mv, cost,
        kind[, pred][, stats]); occlusion=True (a bidir context) keeps the vectors the forward-backward check rejects from
        proposing candidates -- flowonthego_amd.blockmotion"""
        from .blockmotion import ofc_block_motion
        return ofc_block_motion(self, I0, I1, block=block, refine=refine, occlusion=occlusion, pred=pred, stats=stats)

    def upsample_crop_object_overlap(self, flow, ids_a, ids_b, mask=None, ka=256, kb=256, fused=True):
        """the overlap votes between the objects of two frames along upsample_crop(flow): (votes (n, ka, kb), sent (n, ka, 4)); fused:
        the full-resolution flow is never written -- flowonthego_amd.tracks"""
        from .tracks import upsample_crop_object_overlap
        return upsample_crop_object_overlap(self, flow, ids_a, ids_b, mask=mask, ka=ka, kb=kb, fused=fused)

    def track_objects(self, frames, model="affine", iters=3, thresh=1.0, min_area=64, max_objects=256, connectivity=8, min_votes=16,
                      min_frac=0.25, max_tracks=1024, track_ids=False, stats=False):
        """the moving objects of frames (T+1, ...) as moving_objects finds them, linked across frames by the flow into tracks:
        (params (T, 6), objects (T, max_objects, 11), track (T, max_objects), tracks (max_tracks, 8)[, track_ids][, stats]) --
        flowonthego_amd.tracks"""
        from .tracks import ofc_track_objects
        return ofc_track_objects(self, frames, model=model, iters=iters, thresh=thresh, min_area=min_area, max_objects=max_objects,
                                 connectivity=connectivity, min_votes=min_votes, min_frac=min_frac, max_tracks=max_tracks,
                                 track_ids=track_ids, stats=stats)

    def upsample_crop_motion_histograms(self, flow, mask=None, motion=None, cell=16, thresh=0.4, ids=None, rows=256, cells=True, fused=True):
        """HOF and MBH per cell and/or per object of upsample_crop(flow): int64 records of 32 columns; fused: the full-resolution flow
        is never written -- flowonthego_amd.histograms"""
        from .histograms import upsample_crop_motion_histograms
        return upsample_crop_motion_histograms(self, flow, mask=mask, motion=motion, cell=cell, thresh=thresh, ids=ids, rows=rows,
                                               cells=cells, fused=fused)

    def motion_histograms(self, frames, cell=16, model="affine", occlusion=False, objects=False, thresh=0.4, iters=3, fit_thresh=1.0,
                          min_area=64, max_objects=256, connectivity=8, cells=True):
        """the flows of frames (T+1, ...), the camera motion of each (model=None: none), with occlusion the consistency mask, with
        objects the ids of moving_objects, then the fused histograms: (params, cells[, object histograms, objects, ids]) --
        flowonthego_amd.histograms"""
        from .histograms import ofc_motion_histograms
        return ofc_motion_histograms(self, frames, cell=cell, model=model, occlusion=occlusion, objects=objects, thresh=thresh, iters=iters,
                                     fit_thresh=fit_thresh, min_area=min_area, max_objects=max_objects, connectivity=connectivity,
                                     cells=cells)

    def upsample_crop_motion_blur(self, flow, frame, mask=None, shutter=0.5, max_blur=32, code=False, vectors=False, stats=False, fused=True):
        """frame blurred along upsample_crop(flow), a shutter simulated per frame; fused: the full-resolution flow is never written --
        flowonthego_amd.motionblur"""
        from .motionblur import upsample_crop_motion_blur
        return upsample_crop_motion_blur(self, flow, frame, mask=mask, shutter=shutter, max_blur=max_blur, code=code, vectors=vectors,
                                         stats=stats, fused=fused)

    def motion_blur(self, frames, shutter=0.5, max_blur=32, occlusion=False):
        """frames (T+1, ...) -> frames 0 .. T-1 blurred along their forward flows, in chunks of max_batch; with occlusion (a bidir
        context) the consistency mask says which vectors are unknown -- flowonthego_amd.motionblur"""
        from .motionblur import ofc_motion_blur
        return ofc_motion_blur(self, frames, shutter=shutter, max_blur=max_blur, occlusion=occlusion)

    def upsample_crop_background_plate(self, flows, frames, index=None, occ=None, exclude=None, mode="median", min_count=1, fill=0,
                                       ref=None, count=False, code=False, stats=False, fused=True):
        """the median (or mean) over the frames pulled onto the frame grid along upsample_crop(flows), flows (n K, h_l, w_l, 2) of the
        pairs (reference, frame); fused: the full-resolution flows are never written -- flowonthego_amd.plate"""
        from .plate import upsample_crop_background_plate
        return upsample_crop_background_plate(self, flows, frames, index=index, occ=occ, exclude=exclude, mode=mode, min_count=min_count,
                                              fill=fill, ref=ref, count=count, code=code, stats=stats, fused=fused)

    def background(self, frames, ref=0, model="affine", mosaic=False, mode="median", exclude_moving=True, min_count=1):
        """frames (T+1, ...) -> (plate, code, count): the shot without its moving objects in the coordinates of frame ref, with mosaic
        on the canvas that holds every frame -- flowonthego_amd.plate"""
        from .plate import ofc_background
        return ofc_background(self, frames, ref=ref, model=model, mosaic=mosaic, mode=mode, exclude_moving=exclude_moving,
                              min_count=min_count)

    def upsample_crop_subtract_background(self, flows, frames, plate, index=None, origin=(0, 0), plate_code=None, mask=None, low=8.0,
                                          high=24.0, window=1, code=True, diff=False, evidence=False, stats=False, fused=True):
        """every frame against the plate sampled along upsample_crop(flows), flows (n, h_l, w_l, 2) of the pairs (frame, reference);
        fused: the full-resolution flows are never written -- flowonthego_amd.subtract"""
        from .subtract import upsample_crop_subtract_background
        return upsample_crop_subtract_background(self, flows, frames, plate, index=index, origin=origin, plate_code=plate_code, mask=mask,
                                                 low=low, high=high, window=window, code=code, diff=diff, evidence=evidence, stats=stats,
                                                 fused=fused)

    def foreground(self, frames, ref=0, model="affine", low=8.0, high=24.0, window=1, min_area=64, max_objects=256, mode="median",
                   exclude_moving=True, open=0, close=0):
        """frames (T+1, ...) -> (mask, objects, confirmed, plate, code): the plate of the shot on frame ref's grid, every frame
        subtracted from it, and the components that hold a strong pixel; open, close: the radii 0 .. 8 the foreground is opened and
        closed by before the components are taken (0, 0: as it is) -- flowonthego_amd.subtract, flowonthego_amd.morph"""
        from .subtract import ofc_foreground
        return ofc_foreground(self, frames, ref=ref, model=model, low=low, high=high, window=window, min_area=min_area,
                              max_objects=max_objects, mode=mode, exclude_moving=exclude_moving, open=open, close=close)

    def upsample_crop_remove_objects(self, flows, frames, plate, remove, index=None, origin=(0, 0), plate_code=None, mask=None, grow=2,
                                     feather=3, dst=True, code=False, alpha=False, stats=False, fused=True):
        """the frames with `remove`, grown and feathered, filled from the plate sampled along upsample_crop(flows), flows
        (n, h_l, w_l, 2) of the pairs (frame, reference); fused: the full-resolution flows are never written -- flowonthego_amd.erase"""
        from .erase import upsample_crop_remove_objects
        return upsample_crop_remove_objects(self, flows, frames, plate, remove, index=index, origin=origin, plate_code=plate_code, mask=mask,
                                            grow=grow, feather=feather, dst=dst, code=code, alpha=alpha, stats=stats, fused=fused)

    def remove_objects(self, frames, ref=0, model="affine", low=8.0, high=24.0, window=1, min_area=64, max_objects=256, grow=2, feather=3):
        """frames (T+1, ...) -> (clean, code, mask, plate): OFClass.foreground, then the confirmed objects, grown by `grow` pixels and
        feathered over `feather` more, filled from the plate -- flowonthego_amd.erase"""
        from .erase import ofc_remove_objects
        return ofc_remove_objects(self, frames, ref=ref, model=model, low=low, high=high, window=window, min_area=min_area,
                                  max_objects=max_objects, grow=grow, feather=feather)

    def remove_objects_filled(self, frames, **kw):
        """OFClass.remove_objects(frames, **kw), then the holes it leaves where the plate knows nothing filled from the frame around
        them by pull-push: (clean, code, mask, plate, fill_code) -- flowonthego_amd.fill"""
        from .fill import ofc_remove_objects_filled
        return ofc_remove_objects_filled(self, frames, **kw)

    def upsample_crop_fill_flow(self, flow, mask=None):
        """upsample_crop(flow) with the vectors under mask (and the unknown ones) filled from the others -- flowonthego_amd.fill"""
        from .fill import upsample_crop_fill_flow
        return upsample_crop_fill_flow(self, flow, mask)

    def calc_filled(self, I0, I1, both=False, code=False, stats=False):
        """the full-resolution flow of n pairs with the vectors the forward-backward check rejects filled from the consistent ones by
        pull-push (a bidir context); both=True also returns the backward flow filled -- flowonthego_amd.fill"""
        from .fill import ofc_calc_filled
        return ofc_calc_filled(self, I0, I1, both=both, code=code, stats=stats)

    def bidirectional_flows(self, I0, I1):
        """the coarse (fw, bw) of n pairs for a post-pass that also needs the frames (upsample_crop_fb_check, upsample_crop_warp,
        upsample_crop_interpolate): calc_bidirectional or its 8-bit form, by the frames' dtype"""
        u8 = isinstance(I0, torch.Tensor) and I0.dtype == torch.uint8
        return self.calc_bidirectional_u8(I0, I1) if u8 else self.calc_bidirectional(I0, I1)

    def upsample_crop_interpolate(self, flow, flow_bw, I0, I1, t, mask_fw=None, mask_bw=None, ref=None, stats=False, alpha1=0.01,
                                  alpha2=0.5, fused=True):
        """the frame at time t between I0 and I1 from upsample_crop(flow) / upsample_crop(flow_bw) -- flowonthego_amd.interp"""
        from .interp import upsample_crop_interpolate
        return upsample_crop_interpolate(self, flow, flow_bw, I0, I1, t, mask_fw=mask_fw, mask_bw=mask_bw, ref=ref, stats=stats,
                                         alpha1=alpha1, alpha2=alpha2, fused=fused)

    def interpolate(self, I0, I1, t, ref=None, stats=False, alpha1=0.01, alpha2=0.5, fused=True):
        """the frame(s) at time t (or at every t of a sequence) between I0 and I1: both flows from one pyramid per frame, the
        consistency check and the interpolation -- flowonthego_amd.interp.  Needs opt_params.bidir."""
        from .interp import flow_and_interpolate
        return flow_and_interpolate(self, I0, I1, t, ref=ref, stats=stats, alpha1=alpha1, alpha2=alpha2, fused=fused)

    # -- pyramid (src/oflow.cpp:182-207 ConstructImgPyramids) -----------------------------------------------
    def ConstructImgPyramids(self, I0, I1):
        n = I0.shape[0]
        exp = (n, self.height_org, self.width_org) + ((self.op.channels,) if self.op.channels > 1 else ())
        for t, nm in ((I0, "I0"), (I1, "I1")):
            _dev_f32(t, nm, self.device)
            if tuple(t.shape) != exp and tuple(t.shape) != exp + (1,):
                raise FotgError("%s shape %s does not match the configured %s" % (nm, tuple(t.shape), exp))
        check(lib().fotg_pyramid(self._h, n, _ptr(I0), 0, _stream(self.device)))
        check(lib().fotg_pyramid(self._h, n, _ptr(I1), 1, _stream(self.device)))

    def level(self, which, sl, kind=0, n=1):
        """padded pyramid plane as a tensor VIEW-COPY (n, h+2ps, w+2ps, channels); kind 0 image, 1 dx, 2 dy"""
        p, stride = C.c_void_p(), C.c_long()
        check(lib().fotg_level_ptr(self._h, which, sl, kind, p, stride))
        ip = self.iparams[sl - self.op.finest_scale]
        out = torch.empty((n, ip.height_pad, ip.width_pad, self.op.channels), dtype=torch.float32, device=self.device)
        torch.cuda.synchronize()
        for k in range(n):
            _hip_copy(out[k], p.value + 4 * stride.value * k)
        return out

    def level_ptr(self, which, sl, kind=0):
        p, stride = C.c_void_p(), C.c_long()
        check(lib().fotg_level_ptr(self._h, which, sl, kind, p, stride))
        return p.value, stride.value

    def take_stall(self):
        """for callers of the asynchronous entry points (calc_batch and friends return after enqueueing): AFTER their own
        synchronisation, True = a bounded inter-workgroup wait of this context timed out since the last query (FOTG_ERR_STALL:
        the flows computed since are not valid; re-submit).  Read-and-clear, does not synchronise."""
        return bool(lib().fotg_ctx_counter(self._h, b"take_stall"))

    def synchronize(self):
        """wait for the context's work on the current stream of its device and raise if a stall was flagged"""
        torch.cuda.current_stream(self.device).synchronize()
        if self.take_stall():
            check(5)                                        # FOTG_ERR_STALL

    def close(self):
        """OFClass::~OFClass (src/oflow.cpp:147-179)"""
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            lib().fotg_destroy(h)

    def __del__(self):
        if not sys.is_finalizing():
            try:
                self.close()
            except Exception:
                pass


def gradient_magnitude(frames, coarsest_scale, out=None):
    """The reference's SELECTCHANNEL==2 input (kroeger/run_dense.cpp:138-147): frames (n, h, w[, channels]) float32 or uint8 on
    the device -> (n, Hp, Wp[, channels]) float32, the gradient magnitude of the replicate-padded frames (padding to multiples of
    2^coarsest_scale included).  Feed the result to an OFClass created for Wp x Hp."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.is_contiguous() and frames.dtype in (torch.float32, torch.uint8)):
        raise FotgError("frames must be a contiguous float32 or uint8 CUDA(HIP) tensor")
    if frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] not in (1, 3)):
        raise FotgError("frames must have shape (n, h, w) or (n, h, w, 1|3)")
    n, h, w = frames.shape[:3]
    noc = 1 if frames.ndim == 3 else frames.shape[3]
    from .params import padded_size
    wp, hp = padded_size(w, h, coarsest_scale)[:2]
    shape = (n, hp, wp) + (() if frames.ndim == 3 else (noc,))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    _dev_f32(out, "out", frames.device, shape)
    fn = lib().fotg_gradient_magnitude if frames.dtype == torch.float32 else lib().fotg_gradient_magnitude_u8
    check(fn(frames.device.index or 0, n, _ptr(frames), w, h, noc, coarsest_scale, _ptr(out), _stream(frames.device)))
    return out


def _hip_copy(dst_tensor, src_ptr):
    """device->device copy of a raw library pointer into a tensor (test/inspection helper)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    r = hip.hipMemcpy(C.c_void_p(dst_tensor.data_ptr()), C.c_void_p(src_ptr), dst_tensor.numel() * 4, 3)
    if r != 0:
        raise FotgError("hipMemcpy failed: %d" % r)


class PatGridClass:
    """src/patchgrid.h:13-86: the grid of patches of one scale.  Methods take device tensors in the reference's padded
    level layout (h+2ps, w+2ps, channels) with a leading batch dimension."""

    def __init__(self, _i_params: img_params, _op: opt_params):
        """src/patchgrid.h:16; `_op` is the owning OFClass's `op` (src/oflow.cpp:101 passes &op)"""
        ofc = _context_of(_op)
        self._ofc = ofc
        self.i_params = _i_params
        self.lvl = _i_params.curr_lvl
        a, b = C.c_int(), C.c_int()
        check(lib().fotg_num_patches(ofc._h, self.lvl, a, b))
        self.n_patches_width, self.n_patches_height = a.value, b.value
        self.n_patches = a.value * b.value
        self._n = 1
        self._keep = []

    def GetNumPatches(self): return self.n_patches
    def GetNumPatchesW(self): return self.n_patches_width
    def GetNumPatchesH(self): return self.n_patches_height

    def GetRefPatchPos(self, i):
        """src/patchgrid.cpp:54-63: id = x*n_patches_height + y"""
        steps = self._ofc.op.steps
        offw = (self.i_params.width - (self.n_patches_width - 1) * steps) // 2
        offh = (self.i_params.height - (self.n_patches_height - 1) * steps) // 2
        x, y = divmod(i, self.n_patches_height)
        return (float(x * steps + offw), float(y * steps + offh))

    def InitializeGrid(self, _I0, _I0x, _I0y):
        n = _I0.shape[0] if isinstance(_I0, torch.Tensor) and _I0.dim() == 4 else 0
        if n < 1 or n > self._ofc.max_batch:
            raise FotgError("level images must be (n, h+2ps, w+2ps, channels) with 1 <= n <= max_batch")
        ts = [_dev_f32(t, nm, self._ofc.device, self._lvl_shape(n)) for t, nm in ((_I0, "I0"), (_I0x, "I0x"), (_I0y, "I0y"))]
        self._n = n
        self._keep = ts
        stride = ts[0][0].numel()
        check(lib().fotg_grid_init(self._ofc._h, self.lvl, self._n, _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), stride, _stream(self._ofc.device)))

    def _lvl_shape(self, n):
        return (n, self.i_params.height_pad, self.i_params.width_pad, self._ofc.op.channels)

    def SetTargetImage(self, _I1):
        _dev_f32(_I1, "I1", self._ofc.device, self._lvl_shape(self._n))
        self._keep.append(_I1)
        check(lib().fotg_grid_set_target(self._ofc._h, self.lvl, _ptr(_I1), _I1[0].numel()))

    def InitializeFromCoarserOF(self, flow_prev):
        _dev_f32(flow_prev, "flow_prev", self._ofc.device, (self._n, self.i_params.height // 2, self.i_params.width // 2, self._ofc.nch))
        self._keep.append(flow_prev)
        check(lib().fotg_grid_init_from_coarser(self._ofc._h, self.lvl, self._n, _ptr(flow_prev), _stream(self._ofc.device)))

    def SetCamera(self, camlr):
        """depth mode: camparam::camlr of this grid (kroeger/oflow.h:28; 0 left: displacement <= 0, 1 right: >= 0)"""
        check(lib().fotg_grid_set_camera(self._ofc._h, self.lvl, int(camlr)))

    def Optimize(self):
        check(lib().fotg_grid_optimize(self._ofc._h, self.lvl, self._n, _stream(self._ofc.device)))

    def AggregateFlowDense(self, flowout=None):
        if flowout is None:
            flowout = torch.empty((self._n, self.i_params.height, self.i_params.width, self._ofc.nch), dtype=torch.float32, device=self._ofc.device)
        _dev_f32(flowout, "flowout", self._ofc.device, (self._n, self.i_params.height, self.i_params.width, self._ofc.nch))
        check(lib().fotg_grid_aggregate(self._ofc._h, self.lvl, self._n, _ptr(flowout), _stream(self._ofc.device)))
        return flowout

    def printTimings(self):
        """src/patchgrid.cpp:334-345, from the GPU times of the last flow call with op.verbosity > 0 (HIP events of the stages
        on the launch stream): patch extraction and the initialisation from the coarser flow are part of the LK launch"""
        t = (C.c_float * 5)()
        check(lib().fotg_level_timings(self._ofc._h, self.lvl, t))
        print("\n===============Timings (ms)===============")
        print("[extract]      %g\n[coarse]       %g\n[optiTime]      %g\n[aggregate]    %g\n[flow norm]    %g" % (t[0], t[1], t[2], t[3], 0.0))
        print("==========================================")
        return list(t)

    # test taps
    def read_state(self, pair=0, taps=False):
        import numpy as np
        nv = self._ofc.op.n_vals
        p = np.zeros((self.n_patches, 2), np.float32)
        w = np.zeros((self.n_patches, nv), np.float32)
        vp_ = lambda a: a.ctypes.data_as(C.c_void_p)
        if not taps:
            check(lib().fotg_grid_read(self._ofc._h, self.lvl, pair, vp_(p), vp_(w), None, None, None, None, None))
            return {"p_iter": p, "pweight": w}
        t, tx, ty = (np.zeros((self.n_patches, nv), np.float32) for _ in range(3))
        hes = np.zeros((self.n_patches, 3), np.float32)
        cnt = np.zeros((self.n_patches,), np.int32)
        check(lib().fotg_grid_read(self._ofc._h, self.lvl, pair, vp_(p), vp_(w), vp_(t), vp_(tx), vp_(ty), vp_(hes), vp_(cnt)))
        return {"p_iter": p, "pweight": w, "tmpl": t, "tdx": tx, "tdy": ty, "hes": hes, "cnt": cnt}


class VarRefClass:
    """src/refine_variational.h:35-57: like the reference, the constructor does all the work, in place on flowout.
    _I0/_I1: padded level images (n, h+2ps, w+2ps, channels) on the device; flowout (n, h, w, 2) on the device."""

    def __init__(self, _I0, _I1, _i_params: img_params, _op: opt_params, flowout):
        """src/refine_variational.h:38-39; `_op` is the owning OFClass's `op` (src/oflow.cpp:332 passes &op)"""
        ofc = _context_of(_op)
        n = flowout.shape[0] if isinstance(flowout, torch.Tensor) and flowout.dim() == 4 else 0
        if n < 1 or n > ofc.max_batch:
            raise FotgError("flowout must be (n, h, w, %d) with 1 <= n <= max_batch" % ofc.nch)
        lshape = (n, _i_params.height_pad, _i_params.width_pad, ofc.op.channels)
        _dev_f32(_I0, "I0", ofc.device, lshape); _dev_f32(_I1, "I1", ofc.device, lshape)
        _dev_f32(flowout, "flowout", ofc.device, (n, _i_params.height, _i_params.width, ofc.nch))
        check(lib().fotg_varref(ofc._h, _i_params.curr_lvl, n, _ptr(_I0), _ptr(_I1), _I0[0].numel(),
                                _ptr(flowout), _stream(ofc.device)))
        self.flowout = flowout
