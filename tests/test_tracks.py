"""Properties of the object tracks' definition, checked on its numpy restatement (tests/tracks_ref.py); the labelling comes from
objects_ref.components.  No GPU: tests/test_gpu_tracks.py compares the kernels with the same restatement byte for byte."""
import numpy as np
import pytest

import tracks_ref as R

H, W, FRAMES, K = 48, 64, 8, 8


@pytest.fixture(scope="module")
def fixed():
    code, flow = R.fixed_scene(H, W, FRAMES)
    ids, objects = R.labelled(code, K)
    return ids, objects, R.track_objects(ids, objects, flow[:-1], None, min_votes=1, min_frac256=64, max_tracks=16)


def test_fixed_scene_track_table(fixed):
    _, _, r = fixed
    want = [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, -1], [0, 1, 2, -1], [0, 2, -1, -1], [0, 2, -1, -1], [0, 2, -1, -1]]
    assert r["track"].dtype == np.int32 and r["track"].shape == (FRAMES, K)
    assert r["track"][:, :4].tolist() == want
    assert (r["track"][:, 4:] == -1).all()
    assert r["stats"].tolist() == [4, 4, 7 + 4 + 7 + 2, 2]      # tracks 0 and 2 linked over 7 pairs, 1 over 4, 3 over 2
    assert (r["tracks"][4:] == 0).all()


def test_fixed_scene_track_records(fixed):
    _, objects, r = fixed
    t = r["tracks"]
    # track 1 ends at frame 4 with end 2: the two facing rectangles touch at frame 5, their votes tie at 48, the lower row wins
    assert t[1, :4].tolist() == [0, 4, 1, 1] and t[1, 7] == 2
    assert r["votes"][4, 0, 0] == 48 and r["votes"][4, 1, 0] == 48
    assert r["link_ba"][4, 0].tolist() == [0, 0, 48] and r["link_ab"][4, 1].tolist() == [-1, 0, 48]
    # track 3 ends at frame 2 with end 3: its 32 remaining pixels all leave the frame
    assert t[3, :4].tolist() == [0, 2, 3, 3] and t[3, 7] == 3
    assert r["sent"][2, 3].tolist() == [0, 0, 32, 0] and r["link_ab"][2, 3].tolist() == [-1, -1, 0]
    # tracks 0 and 2 are alive at frame 7
    assert t[0, :2].tolist() == [0, 7] and t[2, :2].tolist() == [0, 7] and t[0, 7] == 0 and t[2, 7] == 0
    assert r["sent"][1, 3].tolist() == [32, 0, 32, 0]
    # sum and maximum of the areas, first and last rows
    for tid in range(4):
        rows = [(f, int(np.flatnonzero(r["track"][f] == tid)[0])) for f in range(FRAMES) if (r["track"][f] == tid).any()]
        areas = [int(objects[f, j, 1]) for f, j in rows]
        assert t[tid, 4] == sum(areas) and t[tid, 5] == max(areas)
        assert (t[tid, 0], t[tid, 2]) == rows[0] and (t[tid, 1], t[tid, 3]) == rows[-1]
        assert rows == [(f, j) for f, j in rows if t[tid, 0] <= f <= t[tid, 1]] and len(rows) == t[tid, 1] - t[tid, 0] + 1


def test_fixed_scene_votes_and_sent(fixed):
    ids, objects, r = fixed
    for p in range(FRAMES - 1):
        # the columns of sent add up to the area, for every row
        assert np.array_equal(r["sent"][p].sum(axis=1), objects[p, :, 1])
        assert np.array_equal(r["sent"][p][:, 0], r["votes"][p].sum(axis=1))
        # every link whose object stays inside the frame carries votes equal to the area
        for i in range(K):
            j = r["link_ab"][p, i, 0]
            if j >= 0 and r["sent"][p, i, 2] == 0:
                assert r["link_ab"][p, i, 2] == objects[p, i, 1] == r["votes"][p, i, j]
        # a match is one-to-one and the two tables agree
        for i in range(K):
            j = r["link_ab"][p, i, 0]
            if j >= 0:
                assert r["link_ba"][p, j, 0] == i
        m = r["link_ab"][p, :, 0]
        assert len(set(m[m >= 0].tolist())) == (m >= 0).sum() == (r["link_ba"][p, :, 0] >= 0).sum()
    # the sum of a track's link votes
    assert r["tracks"][0, 6] == sum(int(r["link_ba"][p, int(np.flatnonzero(r["track"][p + 1] == 0)[0]), 2]) for p in range(FRAMES - 1))


def _blobs(h=20, w=30):
    code = np.zeros((1, h, w), np.uint8)
    code[0, 2:8, 3:9] = 1
    code[0, 11:17, 15:27] = 1
    ids, objects = R.labelled(code, 4)
    return ids[0], objects[0]


def test_zero_flow_and_equal_ids_give_identity_links():
    ids, objects = _blobs()
    flow = np.zeros(ids.shape + (2,), np.float32)
    votes, sent = R.overlap(ids, ids, flow, None, 4, 4)
    assert np.array_equal(votes, np.diag(objects[:, 1]).astype(np.int32))
    assert np.array_equal(sent[:, 0], objects[:, 1]) and (sent[:, 1:] == 0).all()
    ab, ba = R.links(votes, objects, objects, 1, 256)
    assert ab[:2].tolist() == [[0, 0, 36], [1, 1, 72]] and np.array_equal(ab, ba)
    assert ab[2:].tolist() == [[-1, -1, 0]] * 2


def test_thresholds_reject_a_link():
    ids, objects = _blobs()
    flow = np.zeros(ids.shape + (2,), np.float32)
    flow[..., 0] = 1.0                                         # one column of each blob lands on background
    votes, sent = R.overlap(ids, ids, flow, None, 4, 4)
    assert votes[0, 0] == 30 and sent[0].tolist() == [30, 6, 0, 0]
    assert R.links(votes, objects, objects, 1, 256)[0][0].tolist() == [-1, 0, 30]     # 256 * 30 < 256 * 36
    assert R.links(votes, objects, objects, 1, 214)[0][0].tolist() == [-1, 0, 30]     # 7680 < 214 * 36 = 7704
    assert R.links(votes, objects, objects, 1, 213)[0][0].tolist() == [0, 0, 30]      # 7680 >= 213 * 36 = 7668
    assert R.links(votes, objects, objects, 31, 0)[0][0].tolist() == [-1, 0, 30]      # min_votes
    assert R.links(votes, objects, objects, 30, 0)[0][0].tolist() == [0, 0, 30]
    # an end of 1: mutual best, a threshold failed (the larger blob keeps 66 votes and its track)
    obj = np.stack([objects, objects])
    ab, ba = R.links_batch(votes[None], obj[:1], obj[1:], 31, 0)
    track, table, stats = R.tracks(obj, ab, ba, 8)
    assert track.tolist() == [[0, 1, -1, -1], [2, 1, -1, -1]] and table[:3, 7].tolist() == [1, 0, 0] and stats.tolist() == [3, 3, 1, 2]
    assert table[1].tolist() == [0, 1, 1, 1, 144, 72, 66, 0]


def test_mask_nonfinite_and_large_vectors_are_inadmissible():
    ids, objects = _blobs()
    flow = np.zeros(ids.shape + (2,), np.float32)
    mask = np.zeros(ids.shape, np.uint8)
    mask[2, 3:6] = (1, 2, 255)
    flow[3, 3] = (np.nan, 0)
    flow[3, 4] = (0, np.inf)
    flow[3, 5] = (-np.inf, 0)
    flow[3, 6] = (4096.5, 0)
    flow[3, 7] = (0, -5000)
    flow[4, 3] = (4096, 0)                                      # admissible: it leaves the frame
    flow[4, 4] = (0, -4096)
    votes, sent = R.overlap(ids, ids, flow, mask, 4, 4)
    assert sent[0].tolist() == [36 - 10, 0, 2, 8] and votes[0, 0] == 26
    assert sent[1].tolist() == [72, 0, 0, 0]
    votes, sent = R.overlap(ids, ids, flow, None, 4, 4)
    assert sent[0].tolist() == [36 - 7, 0, 2, 5]


def test_rounding_is_half_to_even():
    ids = np.full((1, 8), -1, np.int32)
    ids[0, 2] = 0
    idb = np.arange(8, dtype=np.int32)[None]
    for u, x in ((0.5, 2), (1.5, 4), (2.5, 4), (-0.5, 2), (-1.5, 0), (3.5, 6)):
        flow = np.zeros((1, 8, 2), np.float32)
        flow[0, 2, 0] = u
        votes, _ = R.overlap(ids, idb, flow, None, 1, 8)
        assert votes[0].tolist() == [int(j == x) for j in range(8)], u


def test_ids_beyond_the_row_counts_are_background():
    ids, objects = _blobs()
    flow = np.zeros(ids.shape + (2,), np.float32)
    votes, sent = R.overlap(ids, ids, flow, None, 1, 4)          # ka below the ids present: object 1 is ignored
    assert votes.shape == (1, 4) and votes[0].tolist() == [36, 0, 0, 0] and sent.tolist() == [[36, 0, 0, 0]]
    votes, sent = R.overlap(ids, ids, flow, None, 4, 1)          # kb below: object 1 lands on background
    assert votes[:, 0].tolist() == [36, 0, 0, 0] and sent[1].tolist() == [0, 72, 0, 0]
    big = np.where(ids == 1, 1 << 30, ids).astype(np.int32)
    votes, sent = R.overlap(big, ids, flow, None, 4, 4)
    assert sent.sum() == 36


def test_max_tracks_limits_the_table_not_the_ids():
    code, flow = R.fixed_scene(H, W, FRAMES)
    ids, objects = R.labelled(code, K)
    r = R.track_objects(ids, objects, flow[:-1], None, 1, 64, max_tracks=2)
    assert r["tracks"].shape == (2, 8) and r["stats"].tolist() == [4, 2, 20, 2] and r["track"].max() == 3
