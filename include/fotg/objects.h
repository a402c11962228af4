// include/fotg/objects.h -- the connected components of a code map over the C-ABI of libfotg.so (fotg_label_components): the pixels
// of chosen codes (for moving objects: code 1 of the motion fit) grouped into regions, a record of eleven 64-bit integers each.
// Device pointers throughout, asynchronous on `stream` (a hipStream_t, 0 = the null stream); the call returns a FOTG_* status.  The
// definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_OBJECTS_HEADER
#define FOTG_OBJECTS_HEADER
#include "../fotg.h"

namespace OFC {

// objects: per image max_objects rows of eleven 64-bit integers
enum ObjectField { OBJECT_LABEL = 0, OBJECT_AREA = 1, OBJECT_XMIN = 2, OBJECT_YMIN = 3, OBJECT_XMAX = 4, OBJECT_YMAX = 5, OBJECT_SUM_X = 6,
                   OBJECT_SUM_Y = 7, OBJECT_N_VAL = 8, OBJECT_SUM_U = 9, OBJECT_SUM_V = 10, OBJECT_FIELDS = 11 };
// stats: per image four 64-bit integers
enum ObjectStat { OBJECTS_FOREGROUND = 0, OBJECTS_COMPONENTS = 1, OBJECTS_KEPT = 2, OBJECTS_WRITTEN = 3 };

// code n x height x width uint8; fg_codes: bit c set = code c is foreground; values n x height x width x 2 float32 or nullptr;
// objects n x max_objects x 11.  labels, ids n x height x width int32, stats n x 4: each may be nullptr.
inline int LabelComponents(const unsigned char *code, int width, int height, long long *objects, int max_objects = 256,
                           const float *values = nullptr, long long min_area = 1, int fg_codes = 1 << 1, int connectivity = 8,
                           int *labels = nullptr, int *ids = nullptr, long long *stats = nullptr, int n = 1, int device = 0,
                           void *stream = nullptr)
{
  return fotg_label_components(device, n, code, width, height, fg_codes, connectivity, values, min_area, max_objects, labels, ids, objects,
                               stats, stream);
}

}  // namespace OFC
#endif
