// fotg_components.hip -- C-ABI of the connected-component labelling (include/fotg.h fotg_label_components), kernels in
// components.hip.h.  Per call seven launches on the caller's stream; the parent array (unless `labels` is asked for), the per-pixel
// area array and the chunk counts are the call's own memory, taken from and returned to the stream's pool.  Nothing synchronises
// with the host.
#include "host_call.h"
#include "components.hip.h"

using namespace fotg;

namespace {

}  // namespace

extern "C" {

int fotg_label_components(int device, int n, const unsigned char *code, int w, int h, int fg_codes, int connectivity,
                          const float *values, long long min_area, int max_objects, int *labels, int *ids, long long *objects,
                          long long *stats, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > COMP_MAX_DIM || h > COMP_MAX_DIM || !code || !objects) return FOTG_ERR_ARG;
  if (fg_codes < 1 || fg_codes > 255 || (connectivity != 4 && connectivity != 8)) return FOTG_ERR_ARG;
  if (min_area < 1 || max_objects < 1 || max_objects > COMP_MAX_OBJECTS) return FOTG_ERR_ARG;
  const size_t hw = (size_t)w * h;
  const int ntx = (w + COMP_TW - 1) / COMP_TW, nty = (h + COMP_TH - 1) / COMP_TH;
  const int chunks = (int)((hw + COMP_CHUNK - 1) / COMP_CHUNK);                     // <= 2^18
  const size_t tiles = (size_t)ntx * nty * n;
  if (tiles > 0x7fffffffUL) return FOTG_ERR_ARG;
  const Span out[4] = {{labels, n * hw * 4}, {ids, n * hw * 4}, {objects, (size_t)n * max_objects * COMP_NREC * 8},
                       {stats, (size_t)n * COMP_NSTAT * 8}};
  const Span in[2] = {{code, n * hw}, {values, n * hw * 8}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  // the call's memory: [the parents, n h w] the areas, n h w; the chunk counts, n chunks
  const size_t ints = (labels ? 0 : n * hw) + n * hw + (size_t)n * chunks;
  int *ws = nullptr;
  Scratch mem(stream);
  if (!mem.get(&ws, ints * sizeof(int))) return mem.finish(mem.err);
  int *par = labels ? labels : ws;
  int *aux = labels ? ws : ws + n * hw;
  int *chunk_cnt = aux + n * hw;
  hipError_t e = hipMemsetAsync(objects, 0, out[2].bytes, stream);
  if (e == hipSuccess && stats) e = hipMemsetAsync(stats, 0, out[3].bytes, stream);
  if (e == hipSuccess) {
    const bool conn8 = connectivity == 8;
    const dim3 tgrid((unsigned)tiles), cgrid((unsigned)chunks, (unsigned)n);
    comp_tile_kernel<<<tgrid, COMP_THREADS, 0, stream>>>(code, n, w, h, ntx, (unsigned)fg_codes, conn8, par, aux);
    const int nrow = (nty - 1) * w, total = nrow + (ntx - 1) * h;                   // < 2^25
    if (total > 0)
      comp_merge_kernel<<<dim3((unsigned)((total + COMP_THREADS - 1) / COMP_THREADS), (unsigned)n), COMP_THREADS, 0, stream>>>(
          par, w, h, conn8, nrow, total);
    comp_flatten_kernel<<<tgrid, COMP_THREADS, 0, stream>>>(par, aux, n, w, h, ntx);
    comp_count_kernel<<<cgrid, COMP_THREADS, 0, stream>>>(par, aux, (int)hw, min_area, chunk_cnt, stats);
    comp_scan_kernel<<<dim3((unsigned)n), COMP_THREADS, 0, stream>>>(chunk_cnt, chunks, max_objects, stats);
    comp_emit_kernel<<<cgrid, COMP_THREADS, 0, stream>>>(par, aux, w, (int)hw, min_area, chunk_cnt, max_objects, objects);
    if (values)
      comp_reduce_kernel<true><<<tgrid, COMP_THREADS, 0, stream>>>(par, aux, values, n, w, h, ntx, max_objects, objects, ids);
    else
      comp_reduce_kernel<false><<<tgrid, COMP_THREADS, 0, stream>>>(par, aux, nullptr, n, w, h, ntx, max_objects, objects, ids);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

int fotg_components_tile(int *tw, int *th)
{
  if (tw) *tw = COMP_TW;
  if (th) *th = COMP_TH;
  return FOTG_OK;
}

}  // extern "C"
