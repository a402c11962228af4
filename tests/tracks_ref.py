"""The object tracks of flowonthego_amd.tracks (fotg_object_overlap / fotg_object_links / fotg_object_tracks, csrc/objtracks.hip.h)
restated in plain numpy / Python, written for clarity from the definition in include/fotg.h.  In order:

Step 1, overlap votes of one pair a -> b: ids_a, ids_b (h, w) int32 (the `ids` of label_components), flow (h, w, 2) float32 on a's
  grid, mask None or (h, w) uint8, ka, kb.  Every pixel (x, y) with i = ids_a[y, x] in [0, ka):
    mask != 0, u or v not finite, |u| > 4096 or |v| > 4096          -> sent[i, 3] += 1
    else xq = x + rint(u), yq = y + rint(v); outside the frame        -> sent[i, 2] += 1
    else j = ids_b[yq, xq]: in [0, kb) -> votes[i, j] += 1, sent[i, 0] += 1;  else sent[i, 1] += 1
Step 2, links: best_b(i) the lowest j with the largest votes[i, :] if that is > 0, best_a(j) alike down the column; i and j are
  matched iff each is the other's best, votes >= min_votes and 256 votes >= min_frac256 min(area_a[i], area_b[j]);
  link_ab[i] = (matched j or -1, best_b(i) or -1, its votes or 0), link_ba[j] alike.
Step 3, tracks: rows with area > 0 are written; frame 0 numbers them in row order; a written row j of frame t + 1 whose
  link_ba[t][j][0] = i in [0, K) inherits track[t][i], any other written row takes the next unused id; tracks (max_tracks, 8) =
  first_frame, last_frame, first_row, last_row, sum area, max area, sum votes of its links, end (0 alive at frame T, 1 mutual best
  but a threshold failed, 2 the best target prefers another, 3 no best target); stats = started, with a table row, links, alive."""
import numpy as np

TRACK = ("first_frame", "last_frame", "first_row", "last_row", "sum_area", "max_area", "sum_votes", "end")
TRACK_STATS = ("started", "recorded", "links", "alive")
AREA = 1


def overlap(ids_a, ids_b, flow, mask, ka, kb):
    """one pair -> votes (ka, kb) int32, sent (ka, 4) int64"""
    h, w = ids_a.shape
    votes = np.zeros((ka, kb), np.int32)
    sent = np.zeros((ka, 4), np.int64)
    for y in range(h):
        for x in range(w):
            i = int(ids_a[y, x])
            if not 0 <= i < ka:
                continue
            u, v = np.float32(flow[y, x, 0]), np.float32(flow[y, x, 1])
            if (mask is not None and mask[y, x] != 0) or not (np.isfinite(u) and np.isfinite(v)) or abs(u) > 4096 or abs(v) > 4096:
                sent[i, 3] += 1
                continue
            xq, yq = x + int(np.rint(u)), y + int(np.rint(v))
            if not (0 <= xq < w and 0 <= yq < h):
                sent[i, 2] += 1
                continue
            j = int(ids_b[yq, xq])
            if 0 <= j < kb:
                votes[i, j] += 1
                sent[i, 0] += 1
            else:
                sent[i, 1] += 1
    return votes, sent


def overlap_batch(ids_a, ids_b, flow, mask, ka, kb):
    res = [overlap(ids_a[k], ids_b[k], flow[k], None if mask is None else mask[k], ka, kb) for k in range(len(ids_a))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def links(votes, objects_a, objects_b, min_votes, min_frac256):
    """one pair: votes (ka, kb), the object tables (k, 11) -> link_ab (ka, 3), link_ba (kb, 3) int32"""
    ka, kb = votes.shape

    def best(col):
        m = int(col.max()) if len(col) else 0
        return (int(np.flatnonzero(col == m)[0]), m) if m > 0 else (-1, 0)

    bb = [best(votes[i]) for i in range(ka)]
    ba = [best(votes[:, j]) for j in range(kb)]

    def matched(i, j):
        t = int(votes[i, j])
        return (bb[i][0] == j and ba[j][0] == i and t >= min_votes
                and 256 * t >= min_frac256 * min(int(objects_a[i, AREA]), int(objects_b[j, AREA])))

    link_ab = np.array([[j if j >= 0 and matched(i, j) else -1, j, t] for i, (j, t) in enumerate(bb)], np.int32).reshape(ka, 3)
    link_ba = np.array([[i if i >= 0 and matched(i, j) else -1, i, t] for j, (i, t) in enumerate(ba)], np.int32).reshape(kb, 3)
    return link_ab, link_ba


def links_batch(votes, objects_a, objects_b, min_votes, min_frac256):
    res = [links(votes[k], objects_a[k], objects_b[k], min_votes, min_frac256) for k in range(len(votes))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def tracks(objects, link_ab, link_ba, max_tracks):
    """objects (T + 1, K, 11), link_ab / link_ba (T, K, 3) -> track (T + 1, K) int32, tracks (max_tracks, 8) int64, stats (4,) int64"""
    T, K = len(link_ab), objects.shape[1]
    track = np.full((T + 1, K), -1, np.int32)
    table = {}
    nxt = nlinks = 0
    for t in range(T + 1):
        for j in range(K):
            area = int(objects[t, j, AREA])
            if area <= 0:
                continue
            m = int(link_ba[t - 1, j, 0]) if t > 0 else -1
            if 0 <= m < K:
                tid = int(track[t - 1, m])
                nlinks += 1
                votes = int(link_ba[t - 1, j, 2])
            else:
                tid, nxt, votes = nxt, nxt + 1, 0
                table[tid] = [t, t, j, j, 0, 0, 0, 0]
            track[t, j] = tid
            if tid not in table:                              # (only with links that name an unwritten row)
                continue
            rec = table[tid]
            rec[1], rec[3] = t, j
            rec[4] += area
            rec[5] = max(rec[5], area)
            rec[6] += votes
            end = 0
            if t < T and link_ab[t, j, 0] < 0:
                b = int(link_ab[t, j, 1])
                end = 3 if not 0 <= b < K else (1 if link_ba[t, b, 1] == j else 2)
            rec[7] = end
    out = np.zeros((max_tracks, 8), np.int64)
    for tid, rec in table.items():
        if 0 <= tid < max_tracks:
            out[tid] = rec
    alive = int((objects[T, :, AREA] > 0).sum())
    return track, out, np.array([nxt, min(nxt, max_tracks), nlinks, alive], np.int64)


def track_objects(ids, objects, flows, masks=None, min_votes=16, min_frac256=64, max_tracks=1024):
    """the three steps over one sequence: ids (T + 1, h, w), objects (T + 1, K, 11), flows (T, h, w, 2) -> dict of every table"""
    K = objects.shape[1]
    votes, sent = overlap_batch(ids[:-1], ids[1:], flows, masks, K, K)
    link_ab, link_ba = links_batch(votes, objects[:-1], objects[1:], min_votes, min_frac256)
    track, table, stats = tracks(objects, link_ab, link_ba, max_tracks)
    return dict(votes=votes, sent=sent, link_ab=link_ab, link_ba=link_ba, track=track, tracks=table, stats=stats)


# ---- the fixed scene of the tests --------------------------------------------------------------------------------------------------
RECTS = ((4, 4, 8, 6, 3, 0), (40, 6, 8, 6, -3, 0), (10, 30, 6, 8, 2, 2), (52, 36, 8, 8, 4, 0))      # x, y, w, h, vx, vy


def fixed_scene(h=48, w=64, frames=8, rects=RECTS):
    """code (frames, h, w) uint8 and flow (frames, h, w, 2) float32: frame t has code 1 and the flow (vx, vy) on each rectangle
    displaced by t v and clipped to the frame; later rectangles overwrite earlier ones; everything else is zero"""
    code = np.zeros((frames, h, w), np.uint8)
    flow = np.zeros((frames, h, w, 2), np.float32)
    for t in range(frames):
        for x, y, rw, rh, vx, vy in rects:
            x0, y0 = x + t * vx, y + t * vy
            xs, ys = slice(max(x0, 0), max(min(x0 + rw, w), 0)), slice(max(y0, 0), max(min(y0 + rh, h), 0))
            code[t, ys, xs] = 1
            flow[t, ys, xs] = (vx, vy)
    return code, flow


def labelled(code, K, connectivity=8, min_area=1):
    """objects_ref.components per frame -> ids (n, h, w) int32, objects (n, K, 11) int64"""
    import objects_ref as O
    res = O.components_batch(code, O.fg_set((1,)), connectivity, None, min_area, K)
    return res["ids"], res["objects"]
