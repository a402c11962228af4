// include/fotg/tracks.h -- object tracks over the C-ABI of libfotg.so (fotg_object_overlap, fotg_upsample_crop_object_overlap,
// fotg_object_links, fotg_object_tracks): the objects of LabelComponents (fotg/objects.h) linked across the frames of a sequence by
// the flow.  Device pointers throughout, asynchronous on `stream` (a hipStream_t, 0 = the null stream); every call returns a FOTG_*
// status.  The definition is in include/fotg.h.
#ifndef FOTG_TRACKS_HEADER
#define FOTG_TRACKS_HEADER
#include <cstddef>
#include "../fotg.h"

namespace OFC {

// sent: per object of frame a four 64-bit integers
enum SentField { SENT_VOTED = 0, SENT_BACKGROUND = 1, SENT_OUTSIDE = 2, SENT_INADMISSIBLE = 3, SENT_FIELDS = 4 };
// link_ab, link_ba: per object three 32-bit integers
enum LinkField { LINK_MATCH = 0, LINK_BEST = 1, LINK_VOTES = 2, LINK_FIELDS = 3 };
// tracks: per track eight 64-bit integers
enum TrackField { TRACK_FIRST_FRAME = 0, TRACK_LAST_FRAME = 1, TRACK_FIRST_ROW = 2, TRACK_LAST_ROW = 3, TRACK_SUM_AREA = 4,
                  TRACK_MAX_AREA = 5, TRACK_SUM_VOTES = 6, TRACK_END = 7, TRACK_FIELDS = 8 };
// the values of TRACK_END
enum TrackEnd { TRACK_ALIVE = 0, TRACK_THRESHOLD = 1, TRACK_MERGED = 2, TRACK_LOST = 3 };
// stats: four 64-bit integers
enum TrackStat { TRACKS_STARTED = 0, TRACKS_RECORDED = 1, TRACKS_LINKS = 2, TRACKS_ALIVE = 3 };

// ids_a, ids_b n x height x width int32 (the ids of LabelComponents for the frames a and b); flow n x height x width x 2 float32, a ->
// b; mask n x height x width uint8 or nullptr; votes n x ka x kb int32; sent n x ka x 4.
inline int ObjectOverlap(const int *ids_a, const int *ids_b, const float *flow, int width, int height, int ka, int kb, int *votes,
                         long long *sent, const unsigned char *mask = nullptr, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_object_overlap(device, n, ids_a, ids_b, width, height, flow, mask, ka, kb, votes, sent, stream);
}

// the same along the coarse flow of a context, upsampled and cropped on the fly
inline int ObjectOverlap(fotg_ctx *ctx, const float *coarse_flow, const int *ids_a, const int *ids_b, int ka, int kb, int *votes,
                         long long *sent, const unsigned char *mask = nullptr, int n = 1, void *stream = nullptr)
{
  return fotg_upsample_crop_object_overlap(ctx, n, coarse_flow, ids_a, ids_b, mask, ka, kb, votes, sent, stream);
}

// votes n x ka x kb; objects_a n x ka x 11, objects_b n x kb x 11; link_ab n x ka x 3, link_ba n x kb x 3 int32
inline int ObjectLinks(const int *votes, const long long *objects_a, const long long *objects_b, int ka, int kb, int *link_ab,
                       int *link_ba, int min_votes = 16, int min_frac256 = 64, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_object_links(device, n, votes, objects_a, objects_b, ka, kb, min_votes, min_frac256, link_ab, link_ba, stream);
}

// objects (T + 1) x K x 11; link_ab, link_ba T x K x 3; track (T + 1) x K int32; tracks max_tracks x 8; stats 4 or nullptr
inline int ObjectTracks(const long long *objects, const int *link_ab, const int *link_ba, int T, int K, int *track, long long *tracks,
                        int max_tracks = 1024, long long *stats = nullptr, int device = 0, void *stream = nullptr)
{
  return fotg_object_tracks(device, T, K, objects, link_ab, link_ba, max_tracks, track, tracks, stats, stream);
}

// the whole sequence: ids (T + 1) x height x width, objects (T + 1) x K x 11, flows T x height x width x 2 (flow t: frame t -> t + 1),
// masks T x height x width or nullptr; votes (T x K x K), sent (T x K x 4), link_ab and link_ba (T x K x 3) are the caller's
inline int TrackObjects(const int *ids, const long long *objects, const float *flows, int width, int height, int T, int K, int *votes,
                        long long *sent, int *link_ab, int *link_ba, int *track, long long *tracks, int max_tracks = 1024,
                        long long *stats = nullptr, const unsigned char *masks = nullptr, int min_votes = 16, int min_frac256 = 64,
                        int device = 0, void *stream = nullptr)
{
  int st = fotg_object_overlap(device, T, ids, ids + (size_t)width * height, width, height, flows, masks, K, K, votes, sent, stream);
  if (st == FOTG_OK)
    st = fotg_object_links(device, T, votes, objects, objects + (size_t)K * 11, K, K, min_votes, min_frac256, link_ab, link_ba, stream);
  if (st == FOTG_OK) st = fotg_object_tracks(device, T, K, objects, link_ab, link_ba, max_tracks, track, tracks, stats, stream);
  return st;
}

}  // namespace OFC
#endif
