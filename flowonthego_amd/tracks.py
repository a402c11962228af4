"""Object tracks on the GPU: the objects of label_components / moving_objects (flowonthego_amd.objects) linked across the frames of
a sequence by the flow, over fotg_object_overlap / fotg_upsample_crop_object_overlap / fotg_object_links / fotg_object_tracks of
libfotg.so.  Three steps: every pixel of an object of frame a votes for the object of frame b its vector lands on (object_overlap);
two objects are linked when each is the other's best target and the votes pass two thresholds (object_links); the links of a
sequence become track ids that persist over time, with a record per track that says when and why it ended (track_objects).  Exact
integers throughout (no floating-point atomics: the same bytes every run); the definition, in order, is in include/fotg.h and
csrc/objtracks.hip.h.  It runs in HIP only; there is no CPU fallback."""
import torch

from ._args import _dev_f32, _ptr, _stream, batched, coarse_flow, coarse_shape, dense_flow, optional, two_channel, unbatch
from ._lib import FotgError, check, lib
from .objects import OBJECT

TRACK = ("first_frame", "last_frame", "first_row", "last_row", "sum_area", "max_area", "sum_votes", "end")
TRACK_STATS = ("started", "recorded", "links", "alive")
ENDS = ("alive", "threshold", "merged", "lost")              # the values of a track's `end`
SENT = ("voted", "background", "outside", "inadmissible")    # the columns of sent
MAX_ROWS = 1024
MAX_TRACKS = 65536


def _rows(k, name):
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > MAX_ROWS:
        raise FotgError("%s must be an integer in 1 .. %d" % (name, MAX_ROWS))
    return k


def _thresholds(min_votes, min_frac):
    if not isinstance(min_votes, int) or isinstance(min_votes, bool) or min_votes < 1:
        raise FotgError("min_votes must be an integer >= 1")
    if not isinstance(min_frac, (int, float)) or isinstance(min_frac, bool) or not 0 <= min_frac <= 1:
        raise FotgError("min_frac must be in 0 .. 1")
    return min_votes, int(round(min_frac * 256))


def _overlap_outputs(n, ka, kb, device):
    return (torch.empty((n, ka, kb), dtype=torch.int32, device=device), torch.empty((n, ka, 4), dtype=torch.int64, device=device))


def object_overlap(ids_a, ids_b, flow, mask=None, ka=256, kb=256):
    """ids_a, ids_b: device tensors (n, h, w) or (h, w) int32, the `ids` of label_components for the frames a and b (the row of the
    pixel's object, -1 for none; any value outside [0, ka) / [0, kb) is background).  flow: (n, h, w, 2) or (h, w, 2) float32, from a
    to b on a's grid.  mask: None or uint8 (n, h, w) / (h, w), a mask of fb_check (only pixels of code 0 vote).  ka, kb: the rows of
    the two object tables, 1 .. 1024.
    Returns (votes, sent): votes int32 (n, ka, kb), the pixels of object i of a whose vector, rounded to whole pixels, lands on
    object j of b; sent int64 (n, ka, 4) (SENT): per object of a the pixels that voted, landed on background, left the frame, or had
    no admissible vector (masked, not finite, beyond +-4096).  A single pair returns both without the batch dimension.  Asynchronous
    on the current stream."""
    ka, kb = _rows(ka, "ka"), _rows(kb, "kb")
    f, single, n, h, w = dense_flow(flow)
    a = _dev_f32(batched(ids_a, single), "ids_a", f.device, (n, h, w), torch.int32)
    b = _dev_f32(batched(ids_b, single), "ids_b", f.device, (n, h, w), torch.int32)
    m = optional(mask, "mask", f.device, (n, h, w), torch.uint8, single)
    votes, sent = _overlap_outputs(n, ka, kb, f.device)
    check(lib().fotg_object_overlap(f.device.index or 0, n, _ptr(a), _ptr(b), w, h, _ptr(f), _ptr(m), ka, kb, _ptr(votes), _ptr(sent),
                                    _stream(f.device)))
    return unbatch((votes, sent), single, always_tuple=True)


def upsample_crop_object_overlap(ofc, coarse, ids_a, ids_b, mask=None, ka=256, kb=256, fused=True):
    """The context's coarse flow (n, h_l, w_l, 2) and the ids of the frames (n, h_org, w_org) -> bit for bit
    object_overlap(ids_a, ids_b, ofc.upsample_crop(coarse), ...).  fused=True evaluates the upsampling inside the kernel and never
    writes the full-resolution flow; fused=False runs upsample_crop and the dense form."""
    n = coarse_flow(ofc, coarse, "object tracks need a two-channel flow")
    if not fused:
        return object_overlap(ids_a, ids_b, ofc.upsample_crop(coarse), mask=mask, ka=ka, kb=kb)
    ka, kb = _rows(ka, "ka"), _rows(kb, "kb")
    coarse_shape(ofc, coarse, "coarse", n)
    h, w = ofc.height_org, ofc.width_org
    _dev_f32(ids_a, "ids_a", ofc.device, (n, h, w), dtype=torch.int32)
    _dev_f32(ids_b, "ids_b", ofc.device, (n, h, w), dtype=torch.int32)
    optional(mask, "mask", ofc.device, (n, h, w), torch.uint8)
    votes, sent = _overlap_outputs(n, ka, kb, ofc.device)
    check(lib().fotg_upsample_crop_object_overlap(ofc._h, n, _ptr(coarse), _ptr(ids_a), _ptr(ids_b), _ptr(mask), ka, kb, _ptr(votes),
                                                  _ptr(sent), _stream(ofc.device)))
    return votes, sent


def object_links(votes, objects_a, objects_b, min_votes=16, min_frac=0.25):
    """votes: int32 (n, ka, kb) or (ka, kb) of object_overlap; objects_a, objects_b: the object tables of the two frames, int64
    (n, ka, 11) and (n, kb, 11) (label_components; only the area is read).  Object i of a and object j of b are matched iff j is the
    lowest column with the most votes of row i, i the lowest row with the most votes of column j, votes[i][j] >= min_votes and
    256 votes[i][j] >= round(256 min_frac) min(area_a[i], area_b[j]).
    Returns (link_ab, link_ba): int32 (n, ka, 3) and (n, kb, 3), per object (the matched partner or -1, its best target or -1, the
    votes of that best or 0).  The best targets are there whether or not they match: merges and splits can be read from them."""
    if not isinstance(votes, torch.Tensor) or votes.dim() not in (2, 3):
        raise FotgError("votes must be a (n, ka, kb) or (ka, kb) tensor")
    min_votes, frac256 = _thresholds(min_votes, min_frac)
    single = votes.dim() == 2
    v = _dev_f32(batched(votes, single), "votes", dtype=torch.int32)
    n, ka, kb = (int(x) for x in v.shape)
    if n < 1:
        raise FotgError("votes has an empty dimension: %s" % (tuple(votes.shape),))
    _rows(ka, "ka"), _rows(kb, "kb")
    oa = _dev_f32(batched(objects_a, single), "objects_a", v.device, (n, ka, len(OBJECT)), torch.int64)
    ob = _dev_f32(batched(objects_b, single), "objects_b", v.device, (n, kb, len(OBJECT)), torch.int64)
    ab = torch.empty((n, ka, 3), dtype=torch.int32, device=v.device)
    ba = torch.empty((n, kb, 3), dtype=torch.int32, device=v.device)
    check(lib().fotg_object_links(v.device.index or 0, n, _ptr(v), _ptr(oa), _ptr(ob), ka, kb, min_votes, frac256, _ptr(ab), _ptr(ba),
                                  _stream(v.device)))
    return unbatch((ab, ba), single, always_tuple=True)


def link_tracks(objects, link_ab, link_ba, max_tracks=1024, stats=False):
    """objects int64 (T+1, K, 11), link_ab / link_ba int32 (T, K, 3) of object_links over the T pairs of the sequence -> (track,
    tracks[, stats]) as track_objects returns them"""
    if not isinstance(objects, torch.Tensor) or objects.dim() != 3 or objects.shape[0] < 2:
        raise FotgError("objects must be a (T+1, K, 11) tensor with T >= 1")
    if not isinstance(max_tracks, int) or isinstance(max_tracks, bool) or max_tracks < 1 or max_tracks > MAX_TRACKS:
        raise FotgError("max_tracks must be an integer in 1 .. %d" % MAX_TRACKS)
    T, K = int(objects.shape[0]) - 1, _rows(int(objects.shape[1]), "K")
    _dev_f32(objects, "objects", None, (T + 1, K, len(OBJECT)), dtype=torch.int64)
    dev = objects.device
    _dev_f32(link_ab, "link_ab", dev, (T, K, 3), dtype=torch.int32)
    _dev_f32(link_ba, "link_ba", dev, (T, K, 3), dtype=torch.int32)
    track = torch.empty((T + 1, K), dtype=torch.int32, device=dev)
    table = torch.empty((max_tracks, len(TRACK)), dtype=torch.int64, device=dev)
    st = torch.empty((len(TRACK_STATS),), dtype=torch.int64, device=dev) if stats else None
    check(lib().fotg_object_tracks(dev.index or 0, T, K, _ptr(objects), _ptr(link_ab), _ptr(link_ba), max_tracks, _ptr(track), _ptr(table),
                                   _ptr(st), _stream(dev)))
    return (track, table) + ((st,) if stats else ())


def _track_ids(track, ids):
    """the per-pixel map track[t][ids], -1 for background (a torch gather: not the hot path)"""
    T1, K = track.shape
    inside = (ids >= 0) & (ids < K)
    got = torch.gather(track, 1, torch.where(inside, ids, 0).reshape(T1, -1).to(torch.int64)).reshape(ids.shape)
    return torch.where(inside, got, -1).to(torch.int32)


def _finish(ids, objects, votes, min_votes, min_frac, max_tracks, track_ids, stats):
    link_ab, link_ba = object_links(votes, objects[:-1], objects[1:], min_votes, min_frac)
    out = link_tracks(objects, link_ab, link_ba, max_tracks, stats)
    return out[:2] + ((_track_ids(out[0], ids),) if track_ids else ()) + out[2:]


def track_objects(ids, objects, flows, masks=None, min_votes=16, min_frac=0.25, max_tracks=1024, track_ids=False, stats=False):
    """ids: int32 (T+1, h, w) and objects: int64 (T+1, K, 11), what label_components(..., ids=True) returns for the T+1 frames of one
    sequence; flows: float32 (T, h, w, 2), flow t from frame t to frame t+1; masks: None or uint8 (T, h, w).  The overlap votes of
    every pair, their links (min_votes, min_frac) and the tracks: a written row (area > 0) of frame t+1 that is matched inherits the
    track id of its partner in frame t, any other written row starts a new track; ids are handed out in frame order, then row order.
    Returns (track, tracks[, track_ids][, stats]): track int32 (T+1, K), the track id of every row, -1 for an unwritten one; tracks
    int64 (max_tracks, 8) (TRACK), a row per track id below max_tracks, `end` one of ENDS; track_ids int32 (T+1, h, w), the track id of
    every pixel, -1 for background; stats int64 (4) (TRACK_STATS).  Asynchronous on the current stream."""
    if not isinstance(ids, torch.Tensor) or ids.dim() != 3 or ids.shape[0] < 2:
        raise FotgError("ids must be a (T+1, h, w) tensor with T >= 1")
    if not isinstance(objects, torch.Tensor) or objects.dim() != 3:
        raise FotgError("objects must be a (T+1, K, 11) tensor")
    _dev_f32(ids, "ids", None, None, dtype=torch.int32)
    K = _rows(int(objects.shape[1]), "K")
    votes, _ = object_overlap(ids[:-1], ids[1:], flows, masks, K, K)
    return _finish(ids, objects, votes, min_votes, min_frac, max_tracks, track_ids, stats)


def ofc_track_objects(ofc, frames, model="affine", iters=3, thresh=1.0, min_area=64, max_objects=256, connectivity=8, min_votes=16,
                      min_frac=0.25, max_tracks=1024, track_ids=False, stats=False):
    """OFClass.track_objects: the flows of frames (T+1, ...) first (on a bidir context the forward consistency mask is the fit's and
    the votes' mask), the motion fit of each with code and residual, label_components(..., ids=True) of code 1, then for the T-1
    pairs of object maps the fused overlap along the coarse flows, the links and the tracks: (params (T, 6), objects (T,
    max_objects, 11), track (T, max_objects), tracks[, track_ids][, stats]).  The object map of flow t lives on frame t, so T+1 frames
    give T object maps and T-1 links; at least three frames."""
    from .motion import _sequence_flows, upsample_crop_fit_motion
    from .objects import label_components
    two_channel(ofc, "object tracks need a two-channel flow")
    if not isinstance(frames, torch.Tensor) or frames.shape[0] < 3:
        raise FotgError("track_objects needs at least three frames")
    _rows(max_objects, "max_objects")
    fw, mask = _sequence_flows(ofc, frames)
    params, code, residual = upsample_crop_fit_motion(ofc, fw, mask, model, iters, thresh, code=True, residual=True)
    objects, ids = label_components(code, (1,), connectivity, residual, min_area, max_objects, ids=True)
    votes, _ = upsample_crop_object_overlap(ofc, fw[:-1], ids[:-1], ids[1:], None if mask is None else mask[:-1], max_objects, max_objects)
    return (params, objects) + _finish(ids, objects, votes, min_votes, min_frac, max_tracks, track_ids, stats)
