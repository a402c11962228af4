/*
 * fotg.h -- C-ABI of the MI355X-native Dense-Inverse-Search optical-flow engine (libfotg.so).
 *
 * This is the drop-in boundary for the reference's flow path: the C++ classes of the reference's
 * CUDA build (src/oflow.h:22-46 OFClass, src/patchgrid.h:13-86 PatGridClass,
 * src/refine_variational.h:35-57 VarRefClass, src/params.h:9-65 opt_params/img_params) are thin
 * header-only wrappers over these entry points (include/fotg/oflow.h, include/fotg/patchgrid.h).
 * Plain pointers and sizes only; no C++/torch types.  All image/flow pointers are DEVICE pointers
 * (hipMalloc / any HIP-visible allocation) unless the name says host.  Every call returns a status
 * code (0 = ok); the library never calls exit() -- the C++ shim reproduces the reference's
 * print-and-exit behaviour (src/common/cuda_helper.h:286-299).
 *
 * Numerics follow the reference's kroeger/ CPU implementation (the parity oracle), not the
 * reference's CUDA port, which deviates from it.
 */
#ifndef FOTG_H
#define FOTG_H

#ifdef __cplusplus
extern "C" {
#endif

#define FOTG_OK               0
#define FOTG_ERR_ARG          1   /* bad argument / unsupported parameter combination */
#define FOTG_ERR_HIP          2   /* a HIP runtime call failed (fotg_last_hip_error()) */
#define FOTG_ERR_BATCH        3   /* n > max_batch */
#define FOTG_ERR_UNSUPPORTED  4   /* valid in the reference but not implemented here: patch sizes other than 4 / 8 / 12 / 16; a coarsest
                                     level of fewer than 5 rows or 3 columns; with the refinement on: levels of more than 16 384 rows or whose
                                     skewed system array (w + h) x h x 32 bytes reaches 4 GB per pair (lexicographic solver; an 8K frame at
                                     full resolution is 1.7 GB; the depth mode and sor_coupled_slow_but_readable, FOTG_SOR_POINT, also run to 16 384 rows);
                                     red-black ordering in the depth mode */
#define FOTG_ERR_STALL        5   /* a bounded wait between workgroups of the tile solver (levels of more than 96 rows) timed out (preempted or
                                     starved producer) and the batch could not be recomputed.  The entry points that synchronise with the
                                     host and still have the call's inputs -- fotg_calc, fotg_pipe_wait(host_wait = 1), fotg_pipe_sync,
                                     fotg_node_wait -- recompute a stalled batch on the solver path without such waits and SUCCEED (the
                                     context's "stalls" counter counts them); they return this code only when that fails too, or for
                                     batches whose inputs are gone (fotg_pipe_wait(host_wait = 2), pulled pieces of fotg_node_submit_scatter).
                                     Callers of the asynchronous entry points ask fotg_ctx_counter(ctx, "take_stall") after their own
                                     synchronisation (it does not synchronise; read-and-clear) and re-submit. */

#define FOTG_SOR_LEXICOGRAPHIC 0  /* kroeger FDF1.0.1/solver.c:77-421 order (parity mode, default) */
#define FOTG_SOR_REDBLACK      1  /* red-black ordering of the same 2x2 block update (src/kernels/flowUtil.cu:297-362 ordering) */
#define FOTG_SOR_POINT         2  /* kroeger FDF1.0.1/solver.c:19-72 sor_coupled_slow_but_readable, the solver of the reference's OpenMP
                                     build (refine_variational.cpp:202-206), in the order of its serial loop: point update (du from the
                                     old dv, dv from the new du), no block inverse.  Compatibility mode (levels of <= 1024 rows). */

/* == optparam of kroeger/oflow.h:33-76 / opt_params of src/params.h:23-65 (explicitly set part) */
typedef struct fotg_params {
  int sc_f;            /* coarsest scale            (src: coarsest_scale) */
  int sc_l;            /* finest scale              (src: finest_scale) */
  int ps;              /* patch size 4, 8, 12 or 16 (src: patch_size; the operating points use 8 and 12) */
  int max_iter;        /* LK iterations             (src: grad_descent_iter) */
  int min_iter;
  float dp_thresh;     /* 0.05 (squared internally, kroeger/oflow.cpp:88; src/oflow.cpp:53) */
  float dr_thresh;     /* 0.95 */
  float res_thresh;    /* 0.0  */
  float patove;        /* patch overlap             (src: patch_stride) */
  int patnorm;         /* mean normalisation        (src: use_mean_normalization) */
  int noc;             /* channels: 1 gray (kroeger run_OF_INT), 3 interleaved (src/, run_OF_RGB) */
  int usetvref;        /* variational refinement    (src: use_var_ref) */
  float tv_alpha, tv_gamma, tv_delta;   /* 10, 10, 5 */
  int tv_innerit;      /* 1: inner iterations = tv_innerit*(level+1) */
  int tv_solverit;     /* 3                         (src: var_ref_iter) */
  float tv_sor;        /* 1.6                       (src: var_ref_sor_weight) */
  int sor_mode;        /* FOTG_SOR_* */
  int costfct;         /* patch cost: 0 L2 (all operating points), 1 L1, 2 pseudo-Huber (kroeger/oflow.h:45, patch.cpp:230-261) */
  float normoutlier;   /* 5.0: Huber threshold (kroeger/oflow.h:63; src: norm_outlier) */
  int usefbcon;        /* 0 (all operating points); 1: also compute the backward flow at every scale and merge both in the
                          densification (kroeger/oflow.h:44, oflow.cpp:160-170, patchgrid.cpp:278-375) */
  int depth;           /* 0: optical flow (the reference's SELECTMODE=1 build, run_OF_*); 1: stereo depth (SELECTMODE=2,
                          run_DE_*): ONE horizontal displacement per pixel -- every flow array (initflow, outflow, the
                          per-stage flow arguments, fotg_upsample_crop) has 1 channel instead of 2; forward grid /
                          refinement clamp the displacement to <= 0, the backward ones (usefbcon) to >= 0
                          (kroeger/oflow.cpp:76-80,153-157, patch.cpp:188-193, refine_variational.cpp:243-330) */
  int u8_color;        /* 0: 8-bit frames have `noc` channels.  1 / 2 (noc = 1 only): the 8-bit entry points (fotg_calc_batch_u8,
                          fotg_calc_sequence_u8, fotg_pipe_submit_u8, fotg_node_submit_u8) take THREE-channel frames (n x h_org x
                          w_org x 3 uint8), B,G,R byte order as cv::imread delivers (1) or R,G,B (2), and the flow is computed on
                          their gray value, converted on load with OpenCV's fixed-point formula (1868 B + 9617 G + 4899 R + 8192)
                          >> 14 -- what cv::imread(file, IMREAD_GRAYSCALE) feeds kroeger/run_dense.cpp:199-209 for a colour file.
                          Bit-identical to the gray 8-bit path on the converted frames; the float entry points still take gray. */
  int fast_math;       /* 0 (default): parity mode -- every kernel evaluates the reference's f32 expressions in the reference's order,
                          no fused multiply-add: results bit-identical to the CPU oracle.  1: tolerance mode -- the patch loop
                          (PatClass::OptimizeIter, kroeger/patch.cpp:159-212) runs an algebraically equivalent form with fused
                          multiply-adds, free reduction order and a precomputed inverse Hessian (csrc/lk_fast.hip.h): about a third
                          of the instructions, flows within the north star's 1e-3 px mean endpoint error of the parity mode (the
                          tests state the measured distances).  Applies to L2 cost, min_iter == max_iter, res_thresh <= 0, optical
                          flow -- every operating point; other configurations run the exact patch kernel regardless.  The
                          refinement's cell update (solvers of levels of more than 64 rows) uses fused multiply-adds and its data term
                          (compute_data / compute_smoothness, FDF1.0.1/opticalflow_aux.c:123-165,310-438) v_rcp / v_rsq instead of
                          the IEEE divisions and square roots (csrc/varref_dataterm.inc.h), optical flow only. */
  int bidir;           /* 0 (default, all operating points): one direction.  1: the context also holds the backward grid and flows
                          (the usefbcon buffers) that fotg_calc_bidir / fotg_calc_sequence_bidir need; nothing else changes.
                          FOTG_ERR_UNSUPPORTED with depth. */
} fotg_params;

typedef struct fotg_ctx fotg_ctx;

/* operating points 1..4: kroeger/run_dense.cpp:225-268 == src/run_dense.cpp:168-209 */
int fotg_op_point(int op, int width_org, int channels, fotg_params *out);
/* padding that makes W,H multiples of 2^sc_f: kroeger/run_dense.cpp:298-305 == src/run_dense.cpp:231-237 */
int fotg_padded_size(int w, int h, int sc_f, int *wp, int *hp, int *padw, int *padh);

/* Replaces OFClass::OFClass(opt_params, img_params) (src/oflow.cpp:38-145): allocates pyramids, per-scale
 * flow buffers, patch-grid state and refinement workspace for `max_batch` frame pairs of w_org x h_org
 * (unpadded).  Padding to multiples of 2^sc_f (src/run_dense.cpp:231-253, cu::pad) is folded into the
 * pyramid kernel, so callers pass the ORIGINAL frames; already padded frames work too (pad = 0). */
int fotg_create(const fotg_params *p, int w_org, int h_org, int device, int max_batch, fotg_ctx **out);
/* Replaces OFClass::~OFClass (src/oflow.cpp:147-179) */
void fotg_destroy(fotg_ctx *ctx);

/* Replaces OFClass::calc(I0, I1, iparams, initflow, outflow) (src/oflow.cpp:211-368) for n pairs at once.
 * I0, I1: n contiguous frames, each h_org x w_org x noc float32 interleaved (src/run_dense.cpp:137-162).
 * initflow: NULL (as every reference caller passes, src/run_dense.cpp:286) or n x (h/2^(sc_f+1)) x (w/2^(sc_f+1)) x 2
 *   (patches in the last row / column of an odd-sized coarsest level take the last row / column of it: the reference's
 *   InitializeFromCoarserOF indexes one past the array there).
 * outflow: n x (Hp/2^sc_l) x (Wp/2^sc_l) x 2 float32 interleaved (u,v), row-major (src/run_dense.cpp:280-289).
 * stream: hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing. */
int fotg_calc_batch(fotg_ctx *ctx, int n, const float *I0, const float *I1, const float *initflow,
                    float *outflow, void *stream);
/* The same for 8-bit frames (n x h_org x w_org x noc uint8, device memory): what cv::imread delivers before the
 * reference converts to float (src/run_dense.cpp:137-145).  The conversion is exact and happens on load in the pyramid
 * kernel, which then reads a quarter of the bytes.  Results are bit-identical to fotg_calc_batch on the converted frames. */
int fotg_calc_batch_u8(fotg_ctx *ctx, int n, const unsigned char *I0, const unsigned char *I1, const float *initflow,
                       float *outflow, void *stream);
/* Sequence mode (video): `frames` = n_frames consecutive frames (same layout as I0 above), outflow = the n_frames - 1
 * flows frame k -> frame k+1 (2 <= n_frames <= max_batch + 1).  Each frame's pyramid is built once and serves as the
 * target of pair k-1 and as the template source of pair k -- the reference rebuilds both pyramids for every pair
 * (kroeger/run_dense.cpp:331-336).  Bit-identical to fotg_calc_batch(frames[0..n-2], frames[1..n-1]). */
int fotg_calc_sequence(fotg_ctx *ctx, int n_frames, const float *frames, const float *initflow, float *outflow, void *stream);
int fotg_calc_sequence_u8(fotg_ctx *ctx, int n_frames, const unsigned char *frames, const float *initflow, float *outflow,
                          void *stream);
/* ---- bidirectional flow (contexts created with fotg_params::bidir = 1; FOTG_ERR_ARG otherwise) ----------------------------
 * Both directions of every pair from ONE pyramid per frame: outflow == fotg_calc_batch(I0, I1, initflow) and outflow_bw ==
 * fotg_calc_batch(I1, I0, initflow_bw), bit for bit, in every mode the one-direction call has.  initflow / initflow_bw: NULL or
 * as fotg_calc_batch's initflow, each for its own direction.  With usefbcon the directions are coupled through the merge;
 * the contract still holds, with both initflows NULL (FOTG_ERR_ARG otherwise).  Same stream semantics as fotg_calc_batch. */
int fotg_calc_bidir(fotg_ctx *ctx, int n, const float *I0, const float *I1, const float *initflow, const float *initflow_bw,
                    float *outflow, float *outflow_bw, void *stream);
int fotg_calc_bidir_u8(fotg_ctx *ctx, int n, const unsigned char *I0, const unsigned char *I1, const float *initflow,
                       const float *initflow_bw, float *outflow, float *outflow_bw, void *stream);
/* video mode: pair k = frames k -> k+1 forward into outflow[k], frames k+1 -> k backward into outflow_bw[k] */
int fotg_calc_sequence_bidir(fotg_ctx *ctx, int n_frames, const float *frames, const float *initflow, const float *initflow_bw,
                             float *outflow, float *outflow_bw, void *stream);
int fotg_calc_sequence_bidir_u8(fotg_ctx *ctx, int n_frames, const unsigned char *frames, const float *initflow,
                                const float *initflow_bw, float *outflow, float *outflow_bw, void *stream);
/* ---- batches in flight (no reference equivalent: the reference's calc() is synchronous, one pair at a time) -------------
 * A pipe owns `depth` engine contexts, each on an internal non-blocking stream.  fotg_pipe_submit enqueues one batch exactly
 * like fotg_calc_batch (same arguments, same bits) on the next context in turn and returns at once; up to `depth` batches
 * overlap on the GPU.  The work starts behind everything enqueued so far on `after_stream` (the stream that produced the
 * frames; NULL = default stream), or at once with after_stream = FOTG_NO_STREAM (frames already in place; note that an event
 * on a busy stream is only reached when that stream's queue has drained).  The caller keeps I0 / I1 / outflow alive and
 * untouched until the ticket has been waited for.  A pipe is used from one thread at a time (like a context); batches complete
 * in submission order per slot; every ticket has a completion event of its own for the next 4 * depth submissions (a wait for an
 * older ticket waits for a later batch of the same slot, which covers it). */
#define FOTG_PIPE_MAX_DEPTH 8
#define FOTG_NO_STREAM ((void *)(-1))
typedef struct fotg_pipe fotg_pipe;
int fotg_pipe_create(const fotg_params *p, int w_org, int h_org, int device, int max_batch, int depth, fotg_pipe **out);
void fotg_pipe_destroy(fotg_pipe *pipe);
int fotg_pipe_submit(fotg_pipe *pipe, int n, const float *I0, const float *I1, const float *initflow, float *outflow,
                     void *after_stream, long *ticket);
int fotg_pipe_submit_u8(fotg_pipe *pipe, int n, const unsigned char *I0, const unsigned char *I1, const float *initflow,
                        float *outflow, void *after_stream, long *ticket);
/* The same with the element type as an argument (u8 = 0: float32 frames, 1: 8-bit frames) and flags:
 * FOTG_SUBMIT_NO_RECOMPUTE  the batch's frames or outflow may be gone before the host waits for the ticket (staging buffers that are
 *                           recycled behind a device-side wait): a flagged stall is reported for it (FOTG_ERR_STALL), never recomputed. */
#define FOTG_SUBMIT_NO_RECOMPUTE 1
int fotg_pipe_submit_ex(fotg_pipe *pipe, int n, const void *I0, const void *I1, int u8, const float *initflow, float *outflow,
                        void *after_stream, int flags, long *ticket);
/* RECOMPUTE CONTRACT.  A host wait that finds a context's stall word set recomputes the unverified batches of that context from the
 * pointers of their submits.  That is legal only for tickets whose buffers are still in place, so a ticket is recomputed only if it was
 * submitted without FOTG_SUBMIT_NO_RECOMPUTE AND has not been handed out through fotg_pipe_wait(host_wait = 0) or
 * fotg_pipe_ticket_event: after such a hand-over the waiting stream owns the result and the caller may free or reuse I0 / I1 /
 * outflow as soon as its own wait is over.  Suspects that cannot be recomputed -- those, and tickets older than the 4 * depth
 * submissions the pipe keeps arguments for -- are reported: FOTG_ERR_STALL from every host wait for that ticket and from
 * fotg_pipe_sync (their flows are not valid; re-submit).
 * host_wait = 0: `stream` (NULL = default stream) waits for batch `ticket` on the device, the call returns at once;
 * host_wait = 1: the calling thread waits; if the context of the batch has flagged a timed-out inter-workgroup wait, the batches of
 *   that context that have not been verified yet are recomputed (from the arguments of their submits -- which the caller keeps in
 *   place until a ticket has been waited for) and the call succeeds;
 * host_wait = 2: the calling thread waits; a flagged batch is reported (FOTG_ERR_STALL, on every wait for that ticket) instead of
 *   recomputed -- for callers whose frames are not in place any more.
 * A ticket's verdict never changes once a host wait has settled it: a stalled ticket reports FOTG_ERR_STALL from every later host
 * wait and a good one never does, however many tickets follow (the arguments are kept for the last 4 * depth submissions; the
 * stalled tickets older than that are kept per slot as disjoint ranges).  May be called from another thread than the one that
 * submits. */
int fotg_pipe_wait(fotg_pipe *pipe, long ticket, void *stream, int host_wait);
/* the calling thread waits for everything submitted so far */
int fotg_pipe_sync(fotg_pipe *pipe);
/* the completion event (a hipEvent_t) of batch `ticket` (FOTG_ERR_ARG for a ticket that has not been submitted), for waiting on
 * several pipes at once: valid for the next 4 * depth submissions (afterwards it belongs to a later batch of the same slot).  Note
 * the head-of-line effect of that: with more than 4 * depth newer submissions outstanding, a wait for an old ticket waits for a
 * later batch of its slot (a latency cost, never a correctness one). */
int fotg_pipe_ticket_event(fotg_pipe *pipe, long ticket, void **event);
/* the engine context of a slot (geometry queries, taps, counters) */
int fotg_pipe_context(fotg_pipe *pipe, int slot, fotg_ctx **ctx);
/* HARDWARE QUEUES.  The HIP runtime deals the streams of a process to GPU_MAX_HW_QUEUES hardware queues (default 4) PER STREAM
 * PRIORITY -- three pools: high, normal, low -- and two busy streams on one queue run one after the other.  The null stream and
 * the streams of frameworks live in the normal pool.  fotg_pipe_create reads the budget from the environment (it sets nothing
 * and asks for no more than it finds) and places its slot streams, FOTG_PIPE_QUEUES=auto|normal|high|split, read once at creation:
 *   normal  every slot stream at normal priority: the choice of auto when the budget is >= depth + 1
 *   high    up to `budget` slots in the highest-priority pool, further ones in the lowest-priority pool, the rest normal: the
 *           choice of auto below that budget
 *   split   slots alternate between the highest- and the lowest-priority pool
 * With auto, creation then measures the layout it chose with fotg_pipe_probe_overlap and, if the width is below 0.75 * depth
 * (depth counted up to 4: the probe's kernels of more than four to five queues do not run at once on any layout), tries the
 * remaining layouts in the order high, split, normal and keeps the widest (a few milliseconds, at creation only).
 * No variable needs to be set for depth <= 8; a warning is printed only when some pool still holds more slots than queues. */
#define FOTG_PIPE_QUEUES_NORMAL 0
#define FOTG_PIPE_QUEUES_HIGH   1
#define FOTG_PIPE_QUEUES_SPLIT  2
/* How many slots really run at once: a chain of 8 dependent launches of a spin kernel (64 workgroups of 64 threads, about 30 us
 * each, bounded by an iteration cap: it waits on no memory) on every slot stream at once, then the same chain on slot 0 alone;
 * *width = depth * t_alone / t_together, about `depth` with a queue per slot and about depth / 2 with two slots per queue.
 * Synchronises the pipe's own streams only.  FOTG_ERR_ARG while a ticket has not been settled by a host wait (fotg_pipe_wait with
 * host_wait != 0, or fotg_pipe_sync); such tickets and their results are left alone. */
int fotg_pipe_probe_overlap(fotg_pipe *pipe, float *width);
/* what creation read and chose (any pointer may be NULL): the budget, the layout (FOTG_PIPE_QUEUES_*) and the width of the last
 * probe (0 if none has run: depth 1, or a layout forced through FOTG_PIPE_QUEUES) */
int fotg_pipe_queue_info(fotg_pipe *pipe, int *budget, int *layout, float *width);
/* the priority the runtime reports for a slot's stream (smaller = more urgent, 0 = normal) */
int fotg_pipe_slot_priority(fotg_pipe *pipe, int slot, int *priority);

/* ---- one process, several GPUs (no reference equivalent: src/run_dense.cpp:277-289 drives one device) ------------
 * Frame pairs are independent, so a batch of n pairs is cut into contiguous shards -- slot d gets the pairs [begin, begin + count)
 * with count = n / ndev (+ 1 for the first n % ndev slots) and begin = d * (n / ndev) + min(d, n % ndev); ALWAYS take them from
 * fotg_node_shard -- and every slot runs its shard through a pipe of its own (above) on its device,
 * issued by a host thread of its own; there is no exchange between the GPUs on the data path.  `devices` may name a device more
 * than once (two slots on one GPU).  max_batch = pairs per pipe submission on ONE device (a shard larger than that runs as
 * consecutive pieces on consecutive pipe slots), depth = batches in flight per device.  Up to 16 submitted jobs may be waiting to
 * be waited for (FOTG_ERR_BATCH beyond that).  Results are bit-identical to fotg_calc_batch on the same pairs. */
#define FOTG_NODE_MAX_DEV 16
typedef struct fotg_node fotg_node;
int fotg_node_create(const fotg_params *p, int w_org, int h_org, const int *devices, int ndev, int max_batch, int depth, fotg_node **out);
void fotg_node_destroy(fotg_node *node);
/* [begin, begin + count) of the pairs of slot d */
int fotg_node_shard(int n, int ndev, int d, int *begin, int *count);
/* resident frames: I0[d], I1[d], outflow[d] = the shard of slot d in the memory of devices[d] (frames / flows laid out as in
 * fotg_calc_batch; entries of empty shards are ignored).  Returns at once; the frames must be in place (the work starts
 * immediately) and, like outflow, stay untouched until fotg_node_wait(ticket). */
int fotg_node_submit(fotg_node *node, int n, const float *const *I0, const float *const *I1, float *const *outflow, long *ticket);
int fotg_node_submit_u8(fotg_node *node, int n, const unsigned char *const *I0, const unsigned char *const *I1, float *const *outflow, long *ticket);
/* scatter / gather: I0, I1 (n frames each) and outflow (n flows) live on devices[0].  Slot 0 computes its shard in place; every
 * other slot pulls its shard over xGMI in chunks of `chunk` <= max_batch pairs (hipMemcpyPeerAsync into depth + 1 staging buffers
 * on a copy stream of its own), computes chunk t while chunk t + 1 travels, and writes its flows back into `outflow`. */
int fotg_node_submit_scatter(fotg_node *node, int n, const float *I0, const float *I1, float *outflow, int chunk, long *ticket);
/* the same with 8-bit frames (layout as in fotg_calc_batch_u8, three bytes per pixel with u8_color): the shards travel as bytes */
int fotg_node_submit_scatter_u8(fotg_node *node, int n, const unsigned char *I0, const unsigned char *I1, float *outflow, int chunk, long *ticket);
/* The calling thread waits for job `ticket` and every job before it on all devices.  A piece whose tile solver gave up a bounded
 * wait is recomputed where its frames are still in place (resident shards, the source slot of a scatter: the call then succeeds);
 * pulled pieces of a scatter cannot be (their staging buffers have been recycled): FOTG_ERR_STALL, re-submit the job.  Returns the
 * worst status of the jobs this call covers; every job keeps its own status for later (repeated, out-of-order) waits for it: a job
 * that ended FOTG_ERR_STALL reports it on every later wait, however many jobs followed, and a good job never does (other errors
 * are kept for the next 16 jobs).  fotg_node_last_hip_error: the HIP error behind the last FOTG_ERR_HIP a wait returned (it was raised on a worker
 * thread, where fotg_last_hip_error() of the waiting thread does not see it). */
int fotg_node_wait(fotg_node *node, long ticket);
int fotg_node_last_hip_error(const fotg_node *node);
int fotg_node_sync(fotg_node *node);
int fotg_node_info(const fotg_node *node, int *ndev, int *out_w, int *out_h, int *flow_channels);
int fotg_node_pipe(fotg_node *node, int slot, fotg_pipe **pipe);

/* Single pair, outflow in HOST memory, synchronous -- the exact shape of the reference call. */
int fotg_calc(fotg_ctx *ctx, const float *I0, const float *I1, const float *initflow, float *outflow_host);

/* kroeger/run_dense.cpp:407-414 == src/run_dense.cpp:293-303: flow *= 2^sc_l, bilinear x2^sc_l, crop the
 * padding.  in: n x hl x wl x 2 (device), out: n x h_org x w_org x 2 (device). */
int fotg_upsample_crop(fotg_ctx *ctx, int n, const float *flow, float *out, void *stream);

/* Gradient-magnitude input, the reference's SELECTCHANNEL==2 build (kroeger/run_dense.cpp:138-147): level 0 of the pyramid is
 * sqrt(dx^2 + dy^2) of the padded frame (cv::Sobel ksize 1, REFLECT_101 at the padded edge).  frames: n x h_org x w_org x
 * channels (device, f32 or 8-bit); out: n x Hp x Wp x channels f32 (device), Wp / Hp = fotg_padded_size(w_org, h_org, sc_f) --
 * the replicate padding (run_dense.cpp:306-310) is part of the call, so the flow context for these frames is created with
 * w_org = Wp, h_org = Hp (no further padding) and fotg_upsample_crop of a context of the original size crops the result. */
int fotg_gradient_magnitude(int device, int n, const float *frames, int w_org, int h_org, int channels, int sc_f, float *out, void *stream);
int fotg_gradient_magnitude_u8(int device, int n, const unsigned char *frames, int w_org, int h_org, int channels, int sc_f, float *out, void *stream);

/* STREAM-ORDERED MEMORY.  The add-ons below that keep partial sums, planes or levels "in stream-ordered memory of the call" take it
 * with hipMallocAsync and give it back with hipFreeAsync, both on `stream`; nothing else in them touches the host, and the first such
 * call enqueued behind pending work on a stream returns at once.  A further call on the same stream may wait ON THE HOST until the
 * stream has reached the earlier call's free: the runtime's hipMallocAsync blocks the calling thread when the block it would reuse was
 * freed on that stream and the free has not executed yet (measured on the MI355X; no attribute of the device's pool changes it).
 * Results and stream order are not affected.  Entry points: fotg_flow_color and fotg_upsample_crop_color without `stats` (the
 * per-image keys are then the call's own), fotg_warp*, fotg_interp*, fotg_fit_motion, fotg_motion_layers,
 * fotg_label_components, fotg_temporal_filter*, fotg_flow_filter*, fotg_block_motion, fotg_motion_blur, fotg_plate*, fotg_subtract*,
 * fotg_erase*, fotg_fill* and their fotg_upsample_crop_* forms.  A caller that must not block keeps at most one such call pending
 * per stream, or gives each its own stream. */

/* Middlebury colour code of a flow (flow_code/C/color_flow.cpp MotionToColor + colorcode.cpp computeColor).
 * flow: n x h x w x 2 f32 (device); rgb: n x h x w x 3 uint8 (device), R, G, B per pixel (the byte order of the reference's PNG).
 * Normalised PER IMAGE by maxrad = the largest |(u, v)| over its known vectors, or by maxmotion when maxmotion > 0 (a maxrad of 0
 * becomes 1); unknown vectors (|u| > 1e9, |v| > 1e9 or NaN, flowIO.cpp unknown_flow) are black.
 * stats: NULL or n x 5 f32 (device): maxrad, minu, maxu, minv, maxv over the known vectors -- the values color_flow prints, with
 * its initial values -1 / 999 / -999 where an image has none.  Asynchronous on `stream`.  Bit-identical to the reference's
 * arithmetic except the angle: the correctly rounded f32 of atan2 instead of glibc's atan2f.
 * FOTG_ERR_ARG: n < 1, w or h <= 0, a null flow or rgb. */
int fotg_flow_color(int device, int n, const float *flow, int w, int h, float maxmotion, unsigned char *rgb, float *stats, void *stream);
/* The same from the context's coarse flow (n x hl x wl x 2, the layout of fotg_calc_batch's outflow), upsampled and cropped on the
 * fly: rgb (n x h_org x w_org x 3) == fotg_flow_color(fotg_upsample_crop(flow)) byte for byte, without writing the full-resolution
 * flow.  FOTG_ERR_ARG: n < 1 or n > max_batch, a null pointer, a depth-mode context (one channel: no colour code for it). */
int fotg_upsample_crop_color(fotg_ctx *ctx, int n, const float *flow, float maxmotion, unsigned char *rgb, float *stats, void *stream);

/* ---- forward-backward consistency (Sundaram, Brox & Keutzer, ECCV 2010), csrc/fbcheck.hip.h -----------------------------
 * Per pixel (x, y) of a w x h pair (F, B), all arithmetic f32, each operation rounded on its own (no contraction), in this order:
 *   u, v = F[y][x]
 *   if !isfinite(u) || !isfinite(v):                                   code 3 (unknown)
 *   X = (float)x + u;  Y = (float)y + v
 *   if !(X >= 0 && X <= w-1 && Y >= 0 && Y <= h-1):                    code 2 (leaves the frame)
 *   x0 = min((int)floorf(X), w-1); x1 = min(x0+1, w-1); ax = X - (float)x0      (y0, y1, ay alike)
 *   per channel: r0 = B[y0][x0]*(1-ax) + B[y0][x1]*ax;  r1 = B[y1][x0]*(1-ax) + B[y1][x1]*ax;  b = r0*(1-ay) + r1*ay
 *   du = u + bu;  dv = v + bv
 *   lhs = du*du + dv*dv;  rhs = alpha1*((u*u + v*v) + (bu*bu + bv*bv)) + alpha2
 *   code = lhs < rhs ? 0 (consistent) : 1 (occluded / inconsistent; a NaN in B gives 1)
 * Defaults alpha1 = 0.01, alpha2 = 0.5.
 * flow, flow_bw: n x h x w x 2 f32 on the device.  mask (frame-0 pixels, F against B), mask_bw (frame-1 pixels, B against F):
 * n x h x w uint8, either may be NULL.  counts: NULL or n x 2 x 4 uint32 -- per image and direction (0 = mask, 1 = mask_bw)
 * the number of pixels of each code, zeroed by the call.  Asynchronous on `stream`. */
int fotg_fb_check(int device, int n, const float *flow, const float *flow_bw, int w, int h, float alpha1, float alpha2,
                  unsigned char *mask, unsigned char *mask_bw, unsigned *counts, void *stream);
/* The same from the coarse flows of a context (n x hl x wl x 2 each, fotg_out_size), upsampled and cropped on the fly: masks
 * (n x h_org x w_org) byte-identical to fotg_fb_check(fotg_upsample_crop(flow), fotg_upsample_crop(flow_bw)), without writing
 * either full-resolution flow.  FOTG_ERR_ARG: n < 1 or n > max_batch, a null flow, a depth-mode context. */
int fotg_upsample_crop_fb_check(fotg_ctx *ctx, int n, const float *flow, const float *flow_bw, float alpha1, float alpha2,
                                unsigned char *mask, unsigned char *mask_bw, unsigned *counts, void *stream);

/* ---- warp an image along a flow (the reference's image_warp, kroeger/FDF1.0.1/opticalflow_aux.c:18-60), csrc/warp.hip.h -------
 * Per pixel (x, y) of a w x h image, channel c, all arithmetic f32, every operation rounded on its own, in this order:
 *   u, v = F[y][x]
 *   if !isfinite(u) || !isfinite(v):            own = 3; value = fill            (the reference converts NaN to int: undefined)
 *   xx = (float)x + u;  yy = (float)y + v
 *   fx = floorf(xx);    fy = floorf(yy)         (== (float)(int)floor(xx) wherever the reference's conversion is defined)
 *   dx = xx - fx;       dy = yy - fy
 *   own = (xx >= 0 && xx <= w-1 && yy >= 0 && yy <= h-1) ? 0 : 2                 (image_warp's mask == (own == 0))
 *   xi = fx saturated to [-2, w] as int, yi alike to [-2, h]                     (x + 1 cannot overflow)
 *   x1 = clamp(xi, 0, w-1); x2 = clamp(xi+1, 0, w-1); y1, y2 alike
 *   value_c = S[y1][x1][c]*(1-dx)*(1-dy) + S[y1][x2][c]*dx*(1-dy) + S[y2][x1][c]*(1-dx)*dy + S[y2][x2][c]*dx*dy
 *                                                                                (four products summed left to right)
 *   code = own != 0 ? own : (occ ? occ[y][x] (0, 1 or 3; 2 cannot differ from own) : 0)
 *   fill_mode 0 (reference): dst = value wherever own != 3
 *   fill_mode 1:             dst = code == 0 ? value : fill
 * src (S): the image to warp (frame 1 for a forward flow), n x h x w x channels interleaved, channels 1 or 3, f32 (fotg_warp) or
 * 8-bit (fotg_warp_u8), on the device; flow: n x h x w x 2 f32.  8-bit taps are converted exactly to f32; an 8-bit dst is
 * rintf(value) clamped to [0, 255] (and fill likewise, a NaN becoming 0); the residuals below use the unrounded f32 value.  With
 * fill_mode 0, occ NULL and a finite flow, dst and code == 0 are the reference's dst and mask, bit for bit, for any finite flow
 * however large.  occ: NULL or n x h x w uint8, a mask of fotg_fb_check (a byte above 3 counts as 3).  To warp frame 0 onto
 * frame 1's grid pass frame 0 as src, the backward flow and mask_bw.
 * Outputs, each may be NULL (not all three): dst, of src's layout and type (it must not overlap src); code: n x h x w uint8, the
 * alphabet of fotg_fb_check; stats: n x 6 f64 per image: [0..3] the pixels of code 0, 1, 2, 3 and, when a comparison image ref
 * (frame 0; src's layout and type) is given, over the code-0 pixels and all channels [4] sum (double)|ref - value| and
 * [5] sum (double)|ref - S[y][x]| (the unwarped difference at the same pixels), every term the f32 fabsf of the f32 difference;
 * without ref both are 0.  The sums are added in a fixed order (no floating-point atomics): the same bits every run, and the
 * same from the dense and the fused form.  Asynchronous on `stream`; the partial sums live in stream-ordered memory of the call.
 * FOTG_ERR_ARG: n < 1 (or > 65535), w or h <= 0, channels not 1 or 3, fill_mode not 0 or 1, a null src or flow, all three
 * outputs null, dst overlapping src. */
int fotg_warp(int device, int n, const float *src, const float *flow, int w, int h, int channels, const float *ref,
              const unsigned char *occ, int fill_mode, float fill, float *dst, unsigned char *code, double *stats, void *stream);
int fotg_warp_u8(int device, int n, const unsigned char *src, const float *flow, int w, int h, int channels,
                 const unsigned char *ref, const unsigned char *occ, int fill_mode, float fill, unsigned char *dst,
                 unsigned char *code, double *stats, void *stream);
/* The same along the coarse flow of a context (n x hl x wl x 2, the layout of fotg_calc_batch's outflow), upsampled and cropped on
 * the fly: images of h_org x w_org; every output equals fotg_warp(fotg_upsample_crop(coarse_flow)) bit for bit, the six
 * statistics included, without writing the full-resolution flow.  channels is explicit because a gray context may be fed
 * three-channel frames (u8_color).  FOTG_ERR_ARG also for n > max_batch and a depth-mode context. */
int fotg_upsample_crop_warp(fotg_ctx *ctx, int n, const float *coarse_flow, const float *src, int channels, const float *ref,
                            const unsigned char *occ, int fill_mode, float fill, float *dst, unsigned char *code, double *stats,
                            void *stream);
int fotg_upsample_crop_warp_u8(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *src, int channels,
                               const unsigned char *ref, const unsigned char *occ, int fill_mode, float fill, unsigned char *dst,
                               unsigned char *code, double *stats, void *stream);

/* ---- the frame at time t between two frames, from their bidirectional flow, csrc/interp.hip.h ---------------------------------
 * The interpolation procedure of the Middlebury flow benchmark (Baker et al., "A Database and Evaluation Methodology for Optical
 * Flow", section 3.3).  I0, I1: w x h frames; F (0 -> 1), B (1 -> 0): full-resolution flows; mF, mB: their masks in
 * fotg_fb_check's alphabet; 0 < t < 1; t1 = 1.0f - t.  All arithmetic f32, every operation rounded on its own, in this order;
 * taps(S, xx, yy) and inside(xx, yy) are fotg_warp's value_c (four clamped taps) and its in-frame test (own == 0).
 * 1. Candidates, per direction: forward (Isrc, Idst, V, m, s) = (I0, I1, F, mF, t), backward = (I1, I0, B, mB, t1).
 *    Per source pixel p = (x, y), linear index i = y w + x:
 *      u, v = V[p];  skip unless isfinite(u) && isfinite(v)
 *      c = m[p];     skip unless c <= 1                                   (codes 2 and 3, and any byte above, never project)
 *      val = taps(Idst, (float)x + u, (float)y + v)
 *      e = the sum over the channels, in order, of fabsf(Isrc[p][ch] - val[ch])        (fotg_warp's residual term)
 *      q = e * 256 < 16777215 ? (unsigned)floorf(e * 256) : 16777215                   (a NaN cost is the largest)
 *      tx = floorf(((float)x + s * u) + 0.5f);  ty alike;  skip unless 0 <= tx <= w-1 && 0 <= ty <= h-1
 *      key = (uint64)c << 56 | (uint64)q << 32 | i                                     (hence w h < 2^32)
 *      K[ty][tx] = min(K[ty][tx], key)                  (K starts as all ones = empty; one 64-bit integer atomic min)
 *    A consistent candidate beats an inconsistent one, then the lower cost wins, then the lower source index.  A minimum does not
 *    depend on the order of arrival: the result is deterministic by construction.
 * 2. Resolve, per target pixel (x, y):
 *      a forward key:        p* = its low 32 bits, (Vu, Vv) = F[p*],  origin 0
 *      else a backward key:  p* likewise,          (Vu, Vv) = -B[p*], origin 1
 *      else:                                       (Vu, Vv) = 0,      origin 2 (a hole)
 *      x0 = (float)x - t * Vu;  y0 alike;  x1 = (float)x + t1 * Vu;  y1 alike
 *      v0 = taps(I0, x0, y0);  in0 = inside(x0, y0);  v1 = taps(I1, x1, y1);  in1 = inside(x1, y1)
 *      o0 = mF[clamp(floorf(y0 + 0.5f), 0, h-1)][clamp(floorf(x0 + 0.5f), 0, w-1)] != 0;  o1 alike from mB at (x1, y1)
 *      use0 = in0;  use1 = in1;  for origin != 2:  if (o1 && !o0) use0 = false;  if (o0 && !o1) use1 = false
 *      value = use0 && !use1 ? v0 : use1 && !use0 ? v1 : t1 * v0 + t * v1
 *    -- the weighted mean (w0 v0 + w1 v1) / (w0 + w1) with w0 = use0 ? t1 : 0 and w1 = use1 ? t : 0, or the plain blend when both
 *    are 0, written without the division (the weights sum to t1, t or t1 + t).
 *      an 8-bit dst is rounded as fotg_warp's;  code = origin + 4 (use0 && !use1) + 8 (use1 && !use0)
 * 3. stats, per image six doubles: [0..2] the pixels of origin 0, 1, 2; [3] the one-sided pixels (code >= 4); with a comparison
 *    frame ref (the true frame at t, I0's layout and type) over all pixels and channels [4] sum (double)|ref - value| and
 *    [5] sum (double)|ref - (t1 * I0[y][x] + t * I1[y][x])| (the plain blend), each term the f32 fabsf of the f32 difference of the
 *    unrounded value; without ref both are 0.  Added in fotg_warp's fixed order: the same bits every run and from both forms.
 * I0, I1, ref, dst: n x h x w x channels interleaved, channels 1 or 3, f32 (fotg_interp) or 8-bit (fotg_interp_u8), on the device;
 * flow_fw, flow_bw: n x h x w x 2 f32; mask_fw, mask_bw: n x h x w uint8, both given (e.g. fotg_fb_check's) or both NULL: the call
 * then runs fotg_fb_check's kernel with alpha1, alpha2 into memory of its own (ignored when the masks are given).
 * Outputs, each may be NULL (not all three): dst (it must not overlap I0 or I1), code (n x h x w uint8), stats (n x 6 f64).
 * Asynchronous on `stream`.  Key planes (16 bytes per pixel), the call's own masks and the partial sums live in stream-ordered
 * memory of the call; a batch is processed in chunks of as many images as 256 MiB of key planes hold.
 * FOTG_ERR_ARG: n < 1 (or > 65535), w or h <= 0, w h >= 2^32, channels not 1 or 3, t not inside (0, 1), a null frame or flow,
 * one mask without the other, all three outputs null, dst overlapping a frame. */
int fotg_interp(int device, int n, const float *I0, const float *I1, const float *flow_fw, const float *flow_bw, int w, int h,
                int channels, float t, const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1, float alpha2,
                const float *ref, float *dst, unsigned char *code, double *stats, void *stream);
int fotg_interp_u8(int device, int n, const unsigned char *I0, const unsigned char *I1, const float *flow_fw, const float *flow_bw,
                   int w, int h, int channels, float t, const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1,
                   float alpha2, const unsigned char *ref, unsigned char *dst, unsigned char *code, double *stats, void *stream);
/* The same from the coarse flows of a bidirectional context (n x hl x wl x 2 each, the outflows of fotg_calc_bidir), upsampled and
 * cropped on the fly, frames of h_org x w_org: every output equals fotg_interp on fotg_upsample_crop's outputs (and, with NULL
 * masks, fotg_fb_check's masks of them) byte for byte, the statistics included, without writing a full-resolution flow.
 * FOTG_ERR_UNSUPPORTED: a context created without fotg_params::bidir.  FOTG_ERR_ARG also for n > max_batch. */
int fotg_upsample_crop_interp(fotg_ctx *ctx, int n, const float *coarse_fw, const float *coarse_bw, const float *I0, const float *I1,
                              int channels, float t, const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1,
                              float alpha2, const float *ref, float *dst, unsigned char *code, double *stats, void *stream);
int fotg_upsample_crop_interp_u8(fotg_ctx *ctx, int n, const float *coarse_fw, const float *coarse_bw, const unsigned char *I0,
                                 const unsigned char *I1, int channels, float t, const unsigned char *mask_fw,
                                 const unsigned char *mask_bw, float alpha1, float alpha2, const unsigned char *ref,
                                 unsigned char *dst, unsigned char *code, double *stats, void *stream);

/* ---- flow chaining: a position followed through the T flows of a sequence, csrc/chain.hip.h ----------------------------------
 * A chain has a start position (X0, Y0), T forward flows F_0 .. F_{T-1} of one w x h sequence (F_k: frame k -> k+1) and optionally
 * T backward flows B_k (frame k+1 -> k).  Its state is a displacement (Dx, Dy) = (0, 0), steps = 0 and code = 0.  All arithmetic
 * f32, every operation rounded on its own, in this order; inside is the in-frame test of the warp (own == 0), bilerp the sample of
 * the consistency check (x0 = min((int)floorf(X), w-1), x1 = min(x0+1, w-1), ax = X - (float)x0, y alike; per channel
 * r0 = a*(1-ax) + b*ax, r1 likewise, value = r0*(1-ay) + r1*ay):
 *   start:  !isfinite(X0) || !isfinite(Y0) -> code 3;  else !inside(X0, Y0) -> code 2
 *   for k = 0 .. T-1 while code == 0:
 *     X = X0 + Dx;  Y = Y0 + Dy
 *     u, v = bilerp(F_k, X, Y)
 *     if !isfinite(u) || !isfinite(v):            code 3, stop
 *     Ex = Dx + u;  Ey = Dy + v;  Xn = X0 + Ex;  Yn = Y0 + Ey
 *     if !inside(Xn, Yn):                         code 2, stop
 *     with B:  bu, bv = bilerp(B_k, Xn, Yn);  du = u + bu;  dv = v + bv
 *              lhs = du*du + dv*dv;  rhs = alpha1*((u*u + v*v) + (bu*bu + bv*bv)) + alpha2
 *              if !(lhs < rhs):                   code 1, stop          (a NaN in B gives 1, as in the consistency check)
 *     Dx = Ex;  Dy = Ey;  steps = k + 1
 * A stopped chain keeps its last accepted displacement.  Every tap index comes from a position that has passed inside and is
 * clamped: no input value (NaN, +-inf, 1e30) produces an out-of-range address.  For T = 1 and integer starts the displacement at
 * the code-0 pixels is F_0 (==) and, with B, code is the forward mask of the consistency check byte for byte wherever the taps to
 * the right of, below and diagonally below the pixel are finite (a non-finite tap times the weight 0 is a NaN: code 3).
 * Dense form: one chain per pixel of frame 0.  flows, flows_bw (or NULL): n_seq x T x h x w x 2 f32 on the device.  Outputs, each
 * may be NULL (not all four): total n_seq x h x w x 2 f32 (the displacement), code n_seq x h x w uint8, steps n_seq x h x w int32,
 * stats n_seq x 5 uint64 -- the chains ending with code 0, 1, 2, 3 and the sum of steps, zeroed by the call, integer atomics
 * (the same bits every run).  One launch walks all T steps; no position is written to memory.  Asynchronous on `stream`.
 * FOTG_ERR_ARG: n_seq, T, w or h < 1, n_seq > 65535, n_seq T >= 2^31, a null flows, all outputs null, an output overlapping an
 * input. */
int fotg_flow_chain(int device, int n_seq, int T, const float *flows, const float *flows_bw, int w, int h, float alpha1, float alpha2,
                    float *total, unsigned char *code, int *steps, unsigned long long *stats, void *stream);
/* Point form: pts n_seq x P x 2 f32, (x, y) in pixels, anywhere (outside the frame: code 2 at once, non-finite: code 3).  traj:
 * n_seq x (T+1) x P x 2 f32, X0 + D after every step, traj[0] the start as given, the frozen position repeated once a chain has
 * stopped; code, steps: n_seq x P; stats as above.  Each may be NULL (not all four).  FOTG_ERR_ARG also for P < 1 and a null pts. */
int fotg_track_points(int device, int n_seq, int T, const float *flows, const float *flows_bw, int w, int h, float alpha1,
                      float alpha2, int P, const float *pts, float *traj, unsigned char *code, int *steps, unsigned long long *stats,
                      void *stream);
/* The same along T coarse flows of a context (T x hl x wl x 2, the outflow of fotg_calc_sequence; coarse_bw that of
 * fotg_calc_sequence_bidir, or NULL), upsampled and cropped on the fly: the batch index is the step, the T flows form one sequence
 * of h_org x w_org frames.  Every output equals the dense form run on fotg_upsample_crop's outputs byte for byte, without writing a
 * full-resolution flow.  FOTG_ERR_ARG also for T > max_batch and a depth-mode context. */
int fotg_upsample_crop_flow_chain(fotg_ctx *ctx, int T, const float *coarse_flows, const float *coarse_bw, float alpha1, float alpha2,
                                  float *total, unsigned char *code, int *steps, unsigned long long *stats, void *stream);
int fotg_upsample_crop_track_points(fotg_ctx *ctx, int T, const float *coarse_flows, const float *coarse_bw, float alpha1,
                                    float alpha2, int P, const float *pts, float *traj, unsigned char *code, int *steps,
                                    unsigned long long *stats, void *stream);

/* ---- global motion: the one camera motion that explains a flow, and the pixels that do not follow it, csrc/motion.hip.h -------
 * A robust least-squares fit of u = a00 x + a01 y + tx, v = a10 x + a11 y + ty (x, y in pixels of the w x h image) to a flow.
 * model: 0 translation (A = 0), 1 similarity (a00 = a11, a01 = -a10), 2 affine.  In order:
 * Per pixel, integers and f32: X = 2x - (w-1), Y = 2y - (h-1); known = |u| <= 4096 && |v| <= 4096 (false for a NaN or an
 * infinity); U = (int)rintf(u * 256), V = (int)rintf(v * 256) (exact for a known pixel); admissible = known and mask == 0.
 * Round r = 0 .. iters selects the admissible pixels (r = 0) or those of them that follow the previous round's parameters (r > 0)
 * and reduces twelve int64 sums over them: n, sum X, Y, XX, XY, YY, U, XU, YU, V, XV, YV.  For w, h <= 16384 none can overflow
 * (|sum XU| <= 2^28 x 2^14 x 2^20 = 2^62); integer addition is associative, so the sums are the same bits whatever the order.
 * Solve, f64, every operation rounded on its own, for U ~ c0 X + c1 Y + c2, V ~ c3 X + c4 Y + c5:
 *   translation (n >= 1):  c2 = SU / n;  c5 = SV / n
 *   similarity (n >= 2):   D = n (SXX + SYY) - (SX SX + SY SY) > 0;  a = (n (SXU + SYV) - (SX SU + SY SV)) / D;
 *                          b = (n (SXV - SYU) - (SX SV - SY SU)) / D;  c0 = c4 = a;  c3 = b;  c1 = -b;
 *                          c2 = ((SU - a SX) + b SY) / n;  c5 = ((SV - b SX) - a SY) / n
 *   affine (n >= 3):       A00 = SYY n - SY SY;  A01 = SX SY - SXY n;  A02 = SXY SY - SYY SX;  A11 = SXX n - SX SX;
 *                          A12 = SX SXY - SXX SY;  A22 = SXX SYY - SXY SXY;  det = (SXX A00 + SXY A01) + SX A02 > 0;
 *                          c0 = ((A00 SXU + A01 SYU) + A02 SU) / det;  c1 = ((A01 SXU + A11 SYU) + A12 SU) / det;
 *                          c2 = ((A02 SXU + A12 SYU) + A22 SU) / det;  c3 .. c5 alike with SXV, SYV, SV
 *   to the pixel frame, per row:  q_i = c_i / 256;  a_0 = 2 q0;  a_1 = 2 q1;  t = (q2 - q0 (double)(w-1)) - q1 (double)(h-1)
 * A round whose system is unusable keeps the previous parameters (zeros before round 0) and clears `fitted` for good.
 * Prediction, f32, every operation rounded on its own, per row of the six f64 parameters: h0 = a_0 / 2; h1 = a_1 / 2;
 * k0 = (float)h0; k1 = (float)h1; k2 = (float)((t + h0 (double)(w-1)) + h1 (double)(h-1));  pu = (k0 (float)X + k1 (float)Y) + k2.
 * du = u - pu; dv = v - pv; a pixel follows the model iff du du + dv dv <= thresh thresh.
 * flow: n x h x w x 2 f32; mask: NULL or n x h x w uint8 in the alphabet of the consistency check (only code-0 pixels take part);
 * iters 0 .. 64; thresh >= 0, in pixels.  Outputs on the device, each but params may be NULL:
 *   params   n x 6 f64  [a00 a01 tx a10 a11 ty]
 *   code     n x h x w uint8: 0 follows the model, 1 does not (independent motion), 2 excluded by the mask, 3 unknown
 *   residual n x h x w x 2 f32: (du, dv) against the final parameters
 *   stats    n x 6 int64: pixels of code 0, 1, 2, 3, pixels in the last fit, fitted (1: every round's system was usable)
 *   sums     n x 12 int64: the last round's sums
 * code, residual and the counts come from one final pass, skipped when none of them is asked for.  Asynchronous on `stream`; the
 * parameters never leave the device between rounds.  FOTG_ERR_ARG: n < 1 (or > 65535), w or h < 1 or > 16384, a model, iters or
 * thresh out of range, a null flow or params, an output overlapping an input or another output. */
int fotg_fit_motion(int device, int n, const float *flow, const unsigned char *mask, int w, int h, int model, int iters, float thresh,
                    double *params, unsigned char *code, float *residual, long long *stats, long long *sums, void *stream);
/* The same on the coarse flow of a context (n x hl x wl x 2), upsampled and cropped on the fly; mask at the original size.  Every
 * output equals the dense fit of fotg_upsample_crop's output byte for byte.  FOTG_ERR_ARG also for n > max_batch and a depth-mode
 * context. */
int fotg_upsample_crop_fit_motion(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, int model, int iters,
                                  float thresh, double *params, unsigned char *code, float *residual, long long *stats, long long *sums,
                                  void *stream);
/* The model as a flow: params n x 6 f64 -> flow n x h x w x 2 f32, (pu, pv) of the prediction above, so that a flow minus it is the
 * fit's residual bit for bit.  FOTG_ERR_ARG: n < 1 (or > 65535), w or h < 1, a null pointer, flow overlapping params. */
int fotg_motion_flow(int device, int n, const double *params, int w, int h, float *flow, void *stream);
/* How a pass's sums reach the accumulators: 0 one 64-bit integer atomic per workgroup and sum, 1 per-workgroup partials folded
 * by a second launch.  The results are the same bits; this exists to time both.  Sets the process-wide ending for later
 * calls (any other value only queries) and returns the previous one. */
int fotg_motion_ending(int ending);

/* ---- motion layers: several parametric motions fitted to one flow, every pixel given to the nearest, csrc/layers.hip.h ----------
 * The layered decomposition of Wang and Adelson on the pieces of the global-motion fit above: up to eight motions of one `model`,
 * layer 0 the camera motion fotg_fit_motion finds, each further layer grown from the 32 x 32 tile that the earlier layers explain
 * least, then all of them refined together.  layers: K in 1 .. 8; iters 0 .. 64; rounds 0 .. 64; thresh >= 0; init: NULL or
 * n x K x 6 f64.  In order:
 * Per pixel: X, Y, known, U, V and admissible as above.  For a layer with parameters P: (du, dv) = (u, v) - the prediction of P,
 * r(P) = du du + dv dv, within(P) = r(P) <= thresh thresh (f32, every operation rounded on its own, thresh thresh one product).
 * Every layer starts with zero parameters, live = fitted = 0, seed -1, zero sums.
 * Seeding, k = 0 .. K-1 (skipped with init: every layer is then live and fitted with the caller's parameters, seed -2):
 *   candidates = the admissible pixels within() no live layer j < k (a dead layer removes nothing).
 *   k = 0: no seed tile (seed stays -1); rounds r = 0 .. iters select the candidates (r = 0) or the candidates within the layer's
 *          parameters (r > 0), reduce the twelve sums and solve with `model`: params[0] equals fotg_fit_motion's byte for byte.
 *   k >= 1: the candidates are counted per tile of 32 x 32 pixels (edge tiles partial, tile index = tile row x tiles per row +
 *          tile column).  The seed tile has the most, the lowest index among equals; with no candidate the layer is dead (zeros,
 *          seed -1).  Its first parameters are the translation solve of the seed tile's n, sum U, sum V; then iters + 1 rounds,
 *          each over the candidates within the layer's current parameters, solved with `model`.
 *   An unusable system keeps the previous parameters and clears `fitted`; the later rounds still run.  After the last round
 *   live = fitted (a layer one of whose rounds was unusable is dead; its parameters stay as they are).
 * Refinement, `rounds` times: assign every pixel -- best = none, rb = +infinity, db = (u, v); for the live layers j ascending:
 *   less = r_j < rb; if best is none or less: best = j, db = (du_j, dv_j); if less: rb = r_j (ties go to the lower index, a NaN
 *   never displaces a value); joined = admissible, best a layer, db.u db.u + db.v db.v <= thresh thresh.  Every live layer's twelve
 *   sums run over the pixels joined to it and it is solved with `model`; an unusable system keeps its parameters and clears
 *   `fitted`, the layer stays live.
 * Final pass (skipped when none of its outputs is asked for): assign as above.  Outputs on the device, each but params may be NULL:
 *   params   n x K x 6 f64  [a00 a01 tx a10 a11 ty] per layer, in fotg_fit_motion's convention; layers are not reordered
 *   labels   n x h x w uint8: the layer where joined; 253 admissible but joined to none (or no layer live); 254 excluded by the
 *            mask; 255 unknown (unknown wins over masked)
 *   residual n x h x w x 2 f32: db, the flow minus the assigned layer's motion (the flow itself when no layer is live)
 *   records  n x K x 8 int64: pixels labelled, pixels in the last fit, live, fitted, seed tile (-1 none, -2 init), sum X, sum Y,
 *            sum U over the labelled pixels
 *   stats    n x 4 int64: pixels of label 253, 254, 255, the number of live layers
 *   sums     n x K x 12 int64: the sums of each layer's last fit (zeros for a layer that never had one)
 * Integer sums are the same bits whatever the order and nothing is accumulated in floating point, so every output has one value
 * per input.  Asynchronous on `stream`; the parameters never leave the device between passes.  FOTG_ERR_ARG: n < 1 (or > 65535),
 * w or h < 1 or > 16384, layers outside 1 .. 8, a model, iters, rounds or thresh out of range (a NaN thresh too), a null flow or
 * params, an output overlapping an input (init among them) or another output. */
int fotg_motion_layers(int device, int n, const float *flow, const unsigned char *mask, int w, int h, int layers, int model, int iters,
                       int rounds, float thresh, const double *init, double *params, unsigned char *labels, float *residual,
                       long long *records, long long *stats, long long *sums, void *stream);
/* The same on the coarse flow of a context (n x hl x wl x 2), upsampled and cropped on the fly in every pass; mask at the original
 * size.  Every output equals the dense form on fotg_upsample_crop's output byte for byte.  FOTG_ERR_ARG also for n > max_batch and
 * a depth-mode context. */
int fotg_upsample_crop_motion_layers(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, int layers, int model,
                                     int iters, int rounds, float thresh, const double *init, double *params, unsigned char *labels,
                                     float *residual, long long *records, long long *stats, long long *sums, void *stream);

/* ---- objects: the connected components of a code map, with a record each, csrc/components.hip.h ---------------------------------
 * What turns the per-pixel codes of the motion fit (1 = independent motion), the consistency check or the warp into a list of
 * regions.  In order:
 * Input: code n x h x w uint8, 1 <= w, h <= 16384; fg_codes, an 8-bit set with at least one bit: pixel p is foreground iff
 * code[p] < 8 && ((fg_codes >> code[p]) & 1); connectivity 4 or 8 (links between horizontal and vertical neighbours, at 8 also
 * diagonal ones); components never join across the images of the batch; values NULL or n x h x w x 2 f32 (the fit's residual).
 * Label: the linear index y w + x of the component's first pixel in raster order = the minimum linear index over its pixels; it
 * does not depend on tile shape, launch shape, arrival order or route.
 * Record, eleven int64, each independent of the order of reduction: label, area, xmin, ymin, xmax, ymax, sum x, sum y, n_val,
 * sum U, sum V, with U = (int)rintf(256 u), V = (int)rintf(256 v) of the pixel's vector in `values`, left out unless |u| <= 4096
 * && |v| <= 4096 (false for a NaN or an infinity); n_val counts the admissible pixels; n_val = sum U = sum V = 0 without values.
 * For w, h <= 16384 none can overflow: area <= 2^28, sum x, sum y < 2^28 x 2^14 = 2^42, |sum U|, |sum V| <= 2^28 x 2^20 = 2^48.
 * Selection and order: a component is kept iff area >= min_area (>= 1); the kept ones in ascending label order are the rows of
 * objects, n x max_objects x 11 (1 <= max_objects <= 65536): at most the first max_objects are written, every later row is zero.
 * Outputs on the device, each but objects may be NULL:
 *   labels  n x h x w int32: the component's label, -1 for background (components below min_area keep theirs)
 *   ids     n x h x w int32: the row of the pixel's component in objects, -1 for background, a component too small or one beyond
 *           max_objects
 *   stats   n x 4 int64: foreground pixels, components, components with area >= min_area, rows written
 * Integer atomics only: the same bytes every run.  Asynchronous on `stream`; the scratch (a parent and an area entry per pixel) is
 * taken from and returned to the stream's memory pool.  FOTG_ERR_ARG, decided before the device is touched and before anything is
 * launched or cleared: n < 1 (or > 65535, or more than 2^31 - 1 tiles of 64 x 16 in the batch), w or h < 1 or > 16384, fg_codes
 * < 1 or > 255, a connectivity other than 4 and 8, min_area < 1, max_objects < 1 or > 65536, a null code or objects, an output
 * overlapping an input or another output. */
int fotg_label_components(int device, int n, const unsigned char *code, int w, int h, int fg_codes, int connectivity,
                          const float *values, long long min_area, int max_objects, int *labels, int *ids, long long *objects,
                          long long *stats, void *stream);
/* the tile of the labelling kernels, in pixels (tests place structures on its edges and corners); either pointer may be NULL */
int fotg_components_tile(int *tw, int *th);

/* ---- motion-compensated temporal filtering of a frame sequence (denoising, multi-frame fusion), csrc/temporal.hip.h ------------
 * The frames around a centre frame are pulled onto it along their flows and averaged with it, each with a per-pixel weight that
 * falls with the photometric difference in a 3 x 3 window.  All arithmetic f32, every operation rounded on its own, in this order.
 * Inputs: frames, a stack of T frames w x h x channels, channels 1 or 3 interleaved, f32 (fotg_temporal_filter) or 8-bit
 * (fotg_temporal_filter_u8; taps converted exactly to f32), on the device.  For each of the n output images a centre index c =
 * center[i] and K neighbour indices b_1 .. b_K = neighbors[i K ..], 1 <= K <= 8; a neighbour index of -1 means absent and is
 * skipped entirely.  For each neighbour a flow F_k (centre -> neighbour, full resolution; flows: n x K x h x w x 2 f32) and
 * optionally a mask m_k in fotg_fb_check's alphabet (masks: NULL or n x K x h x w uint8).  tau > 0.  K gains g_k, finite and >= 0
 * (gains NULL: all 1).  scale = 1.0f / (tau * (float)(9 * channels)), computed once on the host in f32.
 * Per neighbour k, per pixel q of the centre C = frame c; taps, own and code are exactly fotg_warp's in its reference fill mode
 * with fill 0, with src = frame b_k, flow = F_k, occ = m_k:
 *   W_k[q][ch] = own != 3 ? taps(frame b_k, q + F_k[q])[ch] : 0
 *   d_k[q]     = the sum over the channels, in order, starting from the first term, of fabsf(C[q][ch] - W_k[q][ch])
 *   r_k[x,y]   = (d_k[cl(x-1),y] + d_k[x,y]) + d_k[cl(x+1),y]
 *   e_k[x,y]   = (r_k[x,cl(y-1)] + r_k[x,y]) + r_k[x,cl(y+1)]       (cl clamps to the image: a 3 x 3 box with replicated edges,
 *                                                                    summed separably)
 *   wt         = g_k * (1.0f - e_k * scale)
 *   use_k      = code_k[x,y] == 0 && wt > 0                           (a NaN fails this test)
 * Per pixel, k in ascending order:
 *   num[ch] = C[ch];  den = 1.0f;  used = 0
 *   for each neighbour with use_k:  num[ch] = num[ch] + wt * W_k[ch];  den = den + wt;  used++
 *   value[ch] = num[ch] / den                                         (a correctly rounded division; den >= 1)
 * Outputs, each may be NULL (not all three): dst, n images of the frames' layout and type (an 8-bit dst is rounded as fotg_warp's;
 * it must not overlap the frames); used: n x h x w uint8; stats: n x 4 f64 per image: [0] the sum of used over the image, [1] the
 * number of pixels with used == 0 and, with a clean comparison stack ref (n images of dst's layout and type) over all pixels and
 * channels [2] sum (double)|ref - value| and [3] sum (double)|ref - C|, each term the f32 fabsf of the f32 difference of the
 * unrounded value; without ref both are 0.  The sums are added in a fixed order (no floating-point atomics): the same bits every
 * run, and the same from the dense and the fused form.
 * center (n ints), neighbors (n x K ints) and gains (K floats) are HOST arrays: validated on the host and consumed before the call
 * returns; the indices reach the kernel by a stream-ordered copy into memory of the call, the gains by value.  Everything else is
 * enqueued on `stream`; the partial sums live in stream-ordered memory of the call.
 * FOTG_ERR_ARG, decided before anything is launched: n < 1 (or > 65535), K outside 1..8, T < 1, w or h <= 0, channels not 1 or 3,
 * tau not finite or <= 0, a gain negative or not finite, a centre index outside [0, T), a neighbour index outside [-1, T), a null
 * frames, flows, center or neighbors, all three outputs null, dst overlapping the frames. */
int fotg_temporal_filter(int device, int n, int K, int T, const float *frames, int w, int h, int channels, const int *center,
                         const int *neighbors, const float *flows, const unsigned char *masks, float tau, const float *gains,
                         const float *ref, float *dst, unsigned char *used, double *stats, void *stream);
int fotg_temporal_filter_u8(int device, int n, int K, int T, const unsigned char *frames, int w, int h, int channels,
                            const int *center, const int *neighbors, const float *flows, const unsigned char *masks, float tau,
                            const float *gains, const unsigned char *ref, unsigned char *dst, unsigned char *used, double *stats,
                            void *stream);
/* The same along the coarse flows of a context (n K x hl x wl x 2, in the order a batch fotg_calc_batch of the pairs (centre,
 * neighbour) returns them: image-major, neighbour-minor), upsampled and cropped on the fly, frames of h_org x w_org: every output
 * equals fotg_temporal_filter on fotg_upsample_crop's output byte for byte, the statistics included, without writing a
 * full-resolution flow.  FOTG_ERR_ARG also for n K > max_batch and a depth-mode context. */
int fotg_upsample_crop_temporal_filter(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows, const float *frames,
                                       int channels, const int *center, const int *neighbors, const unsigned char *masks, float tau,
                                       const float *gains, const float *ref, float *dst, unsigned char *used, double *stats,
                                       void *stream);
int fotg_upsample_crop_temporal_filter_u8(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows,
                                          const unsigned char *frames, int channels, const int *center, const int *neighbors,
                                          const unsigned char *masks, float tau, const float *gains, const unsigned char *ref,
                                          unsigned char *dst, unsigned char *used, double *stats, void *stream);

/* ---- edge- and occlusion-aware filtering of a flow, guided by the frame it belongs to, csrc/flowfilter.hip.h --------------------
 * A joint (cross) bilateral filter of the vectors: a vector becomes the mean of the vectors of nearby pixels of similar colour,
 * which pulls motion boundaries onto image edges; vectors a consistency mask rejects stay out of the mean, and a rejected pixel is
 * filled from the consistent vectors around it.  All arithmetic f32, every operation rounded on its own, in this order.
 * Inputs, per image of w x h: the flow F (flow: n x h x w x 2 f32); a guide G (guide: n x h x w x channels, channels 1 or 3
 * interleaved, f32 (fotg_flow_filter) or 8-bit (fotg_flow_filter_u8; converted exactly to f32)); optionally a mask M (mask: NULL
 * or n x h x w uint8, a mask of fotg_fb_check); a radius R, 1 <= R <= 7; spatial, R + 1 floats s[0 .. R], each finite and in
 * [0, 1], s[0] > 0 (NULL: all 1); tau > 0; iters, 1 <= iters <= 4.  scale = 1.0f / (tau * (float)channels), computed once on the
 * host in f32.
 *   valid(q) = q is inside the image && both components of F(q) are finite && (no mask || M(q) == 0)
 * One pass, pixel p:
 *   nu = nv = den = 0
 *   for dy = -R .. R ascending, inside it dx = -R .. R ascending, q = p + (dx, dy); a q outside the image is skipped (not
 *   replicated):
 *     d   = the sum over the channels, in order, starting from the first term, of fabsf(G(p)[ch] - G(q)[ch])
 *     wt  = (s[|dy|] * s[|dx|]) * (1.0f - d * scale)
 *     use = valid(q) && wt > 0                                            (a NaN fails this test)
 *     if use:  nu = nu + wt * F(q).u;  nv = nv + wt * F(q).v;  den = den + wt     (an unused q contributes nothing)
 *   if den > 0:  out = (nu / den, nv / den)  (correctly rounded divisions);  code = valid(p) ? 0 : 1   (1: filled from neighbours)
 *   otherwise:   out = F(p) bit for bit;  code = 3                                                     (3: no support)
 * A valid centre with a finite guide pixel supports itself (d = 0, wt = s[0]^2 > 0) and gets code 0.
 * Several passes: pass k >= 2 is pass 1 applied to the output of pass k - 1 with the mask (code of pass k - 1 == 3) and the same
 * guide.  The final code is 3 where the last pass says 3, otherwise 0 where pass 1 said 0, otherwise 1; the final vectors are the
 * last pass's.  iters = k equals k calls with iters = 1 composed that way, bit for bit.
 * Outputs, each may be NULL (not all three): out, n x h x w x 2 f32 (it must not overlap the flow; with iters > 1 it also holds
 * intermediate passes before the final one); code, n x h x w uint8; stats, n x 4 f64 per image: the pixels of final code [0] 0,
 * [1] 1 and [2] 3, and [3] over the pixels of final code 0 the sum of (double)fabsf(out.u - F.u) and (double)fabsf(out.v - F.v),
 * F the input of pass 1, each term the f32 fabsf of the f32 difference, terms that are not finite left out.  The sums are added
 * in a fixed order (no floating-point atomics): the same bits every run, and the same from the dense and the fused form.
 * spatial is a HOST array, validated on the host, consumed before the call returns and passed to the kernel by value.
 * Everything else is enqueued on `stream`; the vectors and codes between passes and the partial sums live in stream-ordered
 * memory of the call.
 * FOTG_ERR_ARG, decided before anything is launched: n < 1 (or > 65535), w or h <= 0, channels not 1 or 3, radius outside 1..7,
 * iters outside 1..4, tau not finite or <= 0, a spatial entry not finite or outside [0, 1], s[0] == 0, a null flow or guide, all
 * three outputs null, out overlapping the flow. */
int fotg_flow_filter(int device, int n, const float *flow, const float *guide, int w, int h, int channels, const unsigned char *mask,
                     int radius, const float *spatial, float tau, int iters, float *out, unsigned char *code, double *stats,
                     void *stream);
int fotg_flow_filter_u8(int device, int n, const float *flow, const unsigned char *guide, int w, int h, int channels,
                        const unsigned char *mask, int radius, const float *spatial, float tau, int iters, float *out,
                        unsigned char *code, double *stats, void *stream);
/* The same on the coarse flow of a context (n x hl x wl x 2, as fotg_calc_batch returns it), upsampled and cropped on the fly,
 * guide and mask of h_org x w_org: every output equals fotg_flow_filter on fotg_upsample_crop's output bit for bit, the
 * statistics included, without the unfiltered full-resolution flow ever being written.  FOTG_ERR_ARG also for n > max_batch, a
 * depth-mode context and out overlapping the coarse flow. */
int fotg_upsample_crop_flow_filter(fotg_ctx *ctx, int n, const float *coarse_flow, const float *guide, int channels,
                                   const unsigned char *mask, int radius, const float *spatial, float tau, int iters, float *out,
                                   unsigned char *code, double *stats, void *stream);
int fotg_upsample_crop_flow_filter_u8(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *guide, int channels,
                                      const unsigned char *mask, int radius, const float *spatial, float tau, int iters, float *out,
                                      unsigned char *code, double *stats, void *stream);

/* ---- block motion vectors from a dense flow, for a video encoder, csrc/blockmotion.hip.h ------------------------------------------
 * One quarter-pel vector per B x B block, chosen among the vectors the flow proposes for the block because it makes the
 * motion-compensated prediction cheap, with its SAD.  Integer arithmetic from the first step to the last: the same bytes in any
 * reduction order.
 * Inputs: cur, ref, 8-bit frames n x h x w x channels (channels 1 or 3, interleaved); flow, n x h x w x 2 f32 from cur to ref, so
 * that cur(x) ~ ref(x + flow(x)); mask, NULL or n x h x w uint8 in the alphabet of fotg_fb_check (only a byte equal to 0 is valid;
 * bytes above 3 are invalid like 1 .. 3); block B in {8, 16, 32}; refine in {0, 1, 2, 3}; 1 <= w, h <= 16384.
 * Per pixel:
 *   known = |u| <= 4096 && |v| <= 4096                                    (false for a NaN or an infinity)
 *   Qx = (int)rintf(u * 4), Qy alike, in quarter pixels                   (the product is exact, to nearest even, |Q| <= 16384)
 *   admissible = known && (no mask || mask == 0)
 * Block grid: bw = ceil(w / B), bh = ceil(h / B); block (bx, by) covers x in [bx B, min(bx B + B, w)) and y alike.  Pixels beyond the
 * frame do not exist: they add nothing to any sum.
 * Prediction of pixel (x, y), channel k, by the vector (mx, my), all integers:
 *   ix = 4 x + mx;  X0 = ix >> 2 (arithmetic shift: floor);  fx = ix & 3;  iy, Y0, fy alike
 *   the taps a, b, c, d are ref at (X0, Y0), (X0 + 1, Y0), (X0, Y0 + 1), (X0 + 1, Y0 + 1), every tap coordinate clamped on its own
 *   to [0, w - 1] or [0, h - 1] (the encoder's edge padding)
 *   pred = ((4 - fx)(4 - fy) a + fx (4 - fy) b + (4 - fx) fy c + fx fy d + 8) >> 4
 * SAD(m) = the sum of |cur - pred| over the block's pixels and channels.
 * Candidates, in this order (one with nothing to compute from is absent):
 *   0       the zero vector, always present
 *   1       the block mean: with S = the sum of Q over the block's admissible pixels and m their count, floor((2 S + m) / (2 m)) per
 *           component (a floor division); absent when m = 0
 *   2       Q of the pixel (min(bx B + B/2, w - 1), min(by B + B/2, h - 1)), if that pixel is admissible
 *   3 .. 6  the means, by the same rule, of the four B/2 x B/2 quadrants clipped to the frame, top-left, top-right, bottom-left,
 *           bottom-right, each a candidate for the whole block
 * The winner is the lowest SAD; ties go to the lowest index.
 * Refinement: the steps are the last `refine` entries of (4, 2, 1).  Per step s the eight vectors m + s (dx, dy) are evaluated, (dx,
 * dy) in the order (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1), skipping any with a component beyond +-16384; the
 * vector moves to the lowest SAD only if it is strictly lower than the current one, the earliest in that order among equals.
 * Outputs per block: mv, n x bh x bw x 2 int16, in quarter pixels; cost, n x bh x bw x 2 uint32 = [SAD of the final vector, SAD of
 * the zero vector]; kind, n x bh x bw uint8 = the winning candidate | (8 if a refinement step moved the vector).  Optional (NULL:
 * left out): pred, uint8 shaped like cur, the prediction by each block's final vector (it must not overlap cur or ref); stats, n x
 * 11 int64 per image = [0] sum of SAD, [1] sum of the zero-vector SAD, [2] sum of (cur - pred)^2, [3] the blocks moved, [4 .. 10]
 * the blocks per winning candidate 0 .. 6.  Two identical calls give identical bytes.  Everything is enqueued on `stream`.
 * FOTG_ERR_ARG, decided before anything is launched: n < 1 (or > 65535), w or h outside 1 .. 16384, channels not 1 or 3, block not
 * 8, 16 or 32, refine outside 0 .. 3, a null cur, ref, flow, mv, cost or kind, pred overlapping cur or ref. */
int fotg_block_motion(int device, int n, const unsigned char *cur, const unsigned char *ref, int w, int h, int channels,
                      const float *flow, const unsigned char *mask, int block, int refine, short *mv, unsigned *cost,
                      unsigned char *kind, unsigned char *pred, long long *stats, void *stream);
/* The same on the coarse flow of a context (n x hl x wl x 2, as fotg_calc_batch returns it), upsampled and cropped on the fly, frames
 * and mask of h_org x w_org: every output equals fotg_block_motion on fotg_upsample_crop's output bit for bit, without the
 * full-resolution flow ever being written.  FOTG_ERR_ARG also for n > max_batch and a depth-mode context. */
int fotg_upsample_crop_block_motion(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *cur, const unsigned char *ref,
                                    int channels, const unsigned char *mask, int block, int refine, short *mv, unsigned *cost,
                                    unsigned char *kind, unsigned char *pred, long long *stats, void *stream);

/* ---- object tracks: the objects of fotg_label_components linked across frames by the flow, csrc/objtracks.hip.h -----------------
 * What gives the per-frame objects an identity that persists over time, and says when an object enters, leaves, merges or splits.
 * Integer arithmetic from the first step to the last: the same bytes in any order of reduction.  Three steps, three calls.
 * Step 1, overlap votes, per pair of frames a -> b (fotg_object_overlap).  Inputs: ids_a, ids_b, int32 n x h x w, the `ids` of
 * fotg_label_components (the row of the pixel's object, -1 for none); flow, n x h x w x 2 f32, a -> b on a's grid; mask, NULL or
 * n x h x w uint8 in the alphabet of fotg_fb_check (only a byte equal to 0 votes); the row counts ka, kb in 1 .. 1024; 1 <= w, h <=
 * 16384.  For every pixel (x, y) with i = ids_a in [0, ka), in this order (any other value of ids_a, negative or >= ka, is background
 * and is ignored):
 *   1. the pixel is inadmissible if the mask is non-zero, u or v is not finite, |u| > 4096 or |v| > 4096:  sent[i][3]++
 *   2. otherwise xq = x + (int)rintf(u), yq = y + (int)rintf(v) (round half to even); the target outside the frame:  sent[i][2]++
 *   3. otherwise j = ids_b[yq][xq]:  j in [0, kb): votes[i][j]++ and sent[i][0]++;  otherwise (background): sent[i][1]++
 * Outputs: votes, int32 n x ka x kb; sent, int64 n x ka x 4; both cleared by the call.  The four columns of sent[i] add up to the
 * number of pixels carrying id i.  Pairs of a batch never mix.  For a sequence of T + 1 id maps the caller passes ids and ids + h w
 * with n = T.
 * Step 2, links (fotg_object_links).  Inputs: votes; the two object tables objects_a, objects_b (int64 n x ka x 11 and n x kb x 11 as
 * fotg_label_components writes them; the area is column 1); min_votes >= 1; min_frac256 in 0 .. 256.
 *   best_b(i) = the lowest j that maximises votes[i][.], defined only if that maximum is > 0
 *   best_a(j) = the lowest i that maximises votes[.][j], likewise
 *   i and j are matched iff best_b(i) = j, best_a(j) = i, votes[i][j] >= min_votes and
 *   256 votes[i][j] >= min_frac256 min(area_a[i], area_b[j]), evaluated in 64-bit integers
 * Outputs: link_ab, int32 n x ka x 3 = (the matched j or -1, best_b(i) or -1, the votes of that best or 0); link_ba, int32 n x kb x 3
 * likewise.  A match is one-to-one by construction.
 * Step 3, tracks over one sequence; time is the batch axis (fotg_object_tracks).  T + 1 frames, T pairs, K rows per frame: objects
 * (T + 1) x K x 11, link_ab and link_ba T x K x 3.  A row counts as written iff its area > 0.
 *   frame 0: the written rows get the track ids 0, 1, .. in row order
 *   frame t + 1, rows in ascending order: a written row j whose link_ba[t][j] names a match i (in [0, K)) inherits track[t][i]; any
 *   other written row gets the next unused id;  unwritten rows get -1
 * Outputs: track, int32 (T + 1) x K; tracks, int64 max_tracks x 8, one row per track id < max_tracks, the others zero: first_frame,
 * last_frame, first_row, last_row, the sum of its areas, the largest area, the sum of the votes over its links, end; stats (may be
 * NULL), int64 x 4 = tracks started, tracks with a table row, links made, tracks alive at frame T.  A track has exactly one object
 * per frame from first_frame to last_frame.  end, read at the track's last frame t from its row i:
 *   0  alive at frame T
 *   1  its best target is mutual (best_a(best_b(i)) = i) but a threshold failed
 *   2  its best target prefers another object (a merge, or a tie lost to a lower row)
 *   3  link_ab[t][i] has no best target: no pixel of it landed on an object (it left the frame or vanished)
 * All ties are decided by the lower index.  Two identical calls give identical bytes; there are no floating-point atomics.
 * Everything is enqueued on `stream`.  FOTG_ERR_ARG, decided before anything is launched or cleared: n or T < 1 (or > 65535), w or h
 * outside 1 .. 16384, ka, kb or K outside 1 .. 1024, min_votes < 1, min_frac256 outside 0 .. 256, max_tracks outside 1 .. 65536, a
 * null pointer other than mask and stats, an output overlapping an input or another output. */
int fotg_object_overlap(int device, int n, const int *ids_a, const int *ids_b, int w, int h, const float *flow,
                        const unsigned char *mask, int ka, int kb, int *votes, long long *sent, void *stream);
/* Step 1 on the coarse flow of a context (n x hl x wl x 2, as fotg_calc_batch returns it), upsampled and cropped on the fly, ids and
 * mask of h_org x w_org: both outputs equal fotg_object_overlap on fotg_upsample_crop's output bit for bit, without the
 * full-resolution flow ever being written.  FOTG_ERR_ARG also for n > max_batch and a depth-mode context. */
int fotg_upsample_crop_object_overlap(fotg_ctx *ctx, int n, const float *coarse_flow, const int *ids_a, const int *ids_b,
                                      const unsigned char *mask, int ka, int kb, int *votes, long long *sent, void *stream);
int fotg_object_links(int device, int n, const int *votes, const long long *objects_a, const long long *objects_b, int ka, int kb,
                      int min_votes, int min_frac256, int *link_ab, int *link_ba, void *stream);
int fotg_object_tracks(int device, int T, int K, const long long *objects, const int *link_ab, const int *link_ba, int max_tracks,
                       int *track, long long *tracks, long long *stats, void *stream);

/* ---- motion histograms: HOF and MBH per cell and per object, csrc/histograms.hip.h ------------------------------------------------
 * What turns a flow into features: the histogram of optical flow (HOF) and the motion-boundary histograms (MBHx, MBHy) of the
 * dense-trajectories family, per cell of a regular grid and/or per object of an `ids` map (fotg_label_components).  Integer
 * arithmetic after the first step: every sum is an integer sum, the same bytes in any order of accumulation.  Inputs: flow,
 * n x h x w x 2 f32; mask, NULL or n x h x w uint8 in the alphabet of fotg_fb_check; params, NULL or n x 6 f64, the pixel-frame
 * parameters fotg_fit_motion returns (the camera motion to subtract); ids, NULL or int32 n x h x w.  The definition, in order:
 *   1. Residual.  (u, v) must be known: |u| <= 4096 and |v| <= 4096 (false for a NaN or an infinity).  With params, (pu, pv) is the
 *      model's vector at the pixel exactly as fotg_motion_flow writes it, ru = u - pu, rv = v - pv (one f32 subtraction each), and
 *      (ru, rv) must be known again; without, ru = u, rv = v.
 *   2. A pixel is admissible iff step 1 passes and (mask == NULL or its mask byte is 0).  U = (int)rintf(256 ru), V = (int)rintf(256 rv).
 *   3. M(a, b) = floor(sqrt(a a + b b)), the exact integer square root of the 64-bit sum.
 *   4. The angle index A(a, b) in [0, 2048), in units of 45/256 degrees, for (a, b) != (0, 0).  With ax = |a|, ay = |b|:
 *      phi = T[(ay << 8) / ax] if ax >= ay, else 512 - T[(ax << 8) / ay] (integer division), and by the signs
 *      a >= 0, b >= 0: A = phi;  a < 0, b >= 0: A = 1024 - phi;  a < 0, b < 0: A = 1024 + phi;  a >= 0, b < 0: A = (2048 - phi) mod 2048.
 *      T[k] = rint(256 atan(k / 256) / (pi / 4)) for k = 0 .. 256, a literal table (MH_ATAN of csrc/histograms.hip.h).
 *   5. Soft binning of a weight m at angle A: b0 = A >> 8, f = A & 255, w1 = (m f) >> 8, w0 = m - w1; w0 goes to bin b0, w1 to bin
 *      (b0 + 1) & 7: eight bins centred on the multiples of 45 degrees, linear interpolation between neighbours.
 *   6. HOF, for an admissible pixel with m = M(U, V): m < thresh256 counts one in the zero-bin column and adds no orientation weight;
 *      otherwise m is soft-binned at A(U, V).  thresh256 = 0 sends nothing to the zero bin; a pixel with U = V = 0 then adds nothing.
 *   7. MBH.  Ux = U[y][min(x+1, w-1)] - U[y][max(x-1, 0)], Uy = U[min(y+1, h-1)][x] - U[max(y-1, 0)][x], Vx and Vy alike: clamped
 *      coordinates, so the difference is one-sided at the border.  A pixel takes part iff it and its four clamped neighbours are
 *      admissible.  MBHx soft-bins M(Ux, Uy) at A(Ux, Uy), MBHy M(Vx, Vy) at A(Vx, Vy); a zero gradient counts and adds nothing.
 *   8. The record, 32 int64: [0..7] HOF bins, [8] zero-bin pixels, [9..16] MBHx bins, [17..24] MBHy bins, [25] admissible pixels,
 *      [26] pixels in MBH, [27] pixels of the cell or object that are not admissible, [28] the sum of m, [29] of U, [30] of V over the
 *      admissible pixels, [31] 0.
 *   9. cells (may be NULL), int64 n x ceil(h / cell) x ceil(w / cell) x 32, cell in {8, 16, 32}; edge cells are partial.  objects (may be
 *      NULL; needs ids), int64 n x rows x 32: a pixel with i = ids[y][x] in [0, rows) adds to row i, every other id, -1 included, is
 *      background; a pixel's MBH goes to its own row whatever its neighbours' ids are.  Both are complete after the call, zero rows
 *      included.
 * Two identical calls give identical bytes; there are no floating-point atomics.  Everything is enqueued on `stream`.  FOTG_ERR_ARG,
 * decided before anything is launched or cleared: n < 1 (or > 65535), w or h outside 1 .. 16384, a null flow, cell not 8, 16 or 32,
 * thresh256 < 0, cells and objects both NULL, objects without ids, rows outside 1 .. 1024 (read only with objects), an output
 * overlapping an input or the other output. */
int fotg_motion_histograms(int device, int n, const float *flow, int w, int h, const unsigned char *mask, const double *params, int cell,
                           int thresh256, long long *cells, const int *ids, int rows, long long *objects, void *stream);
/* The same on the coarse flow of a context (n x hl x wl x 2, as fotg_calc_batch returns it), upsampled and cropped on the fly, mask and
 * ids of h_org x w_org: both outputs equal fotg_motion_histograms on fotg_upsample_crop's output bit for bit, without the
 * full-resolution flow ever being written.  FOTG_ERR_ARG also for n > max_batch and a depth-mode context. */
int fotg_upsample_crop_motion_histograms(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, const double *params,
                                         int cell, int thresh256, long long *cells, const int *ids, int rows, long long *objects,
                                         void *stream);

/* ---- motion blur along a flow: a shutter simulated per frame, csrc/motionblur.hip.h ------------------------------------------------
 * Blurs a frame along its flow: the tile-max / neighbour-max scatter-as-gather reconstruction filter (McGuire et al. 2012, the
 * direction test of Guertin et al. 2014, both without depth).  A static pixel is untouched unless something within reach moves
 * across it; a moving object smears over its surroundings by its own half-streak; a fast pixel moving across the line does not
 * smear along it.  One f32 multiply per component, integers after it; lengths in 1/16 pixel.  Inputs: src, n x h x w x channels,
 * 8-bit (type FOTG_BLUR_U8) or f32 (FOTG_BLUR_F32), channels 1 or 3; flow, n x h x w x 2 f32, the flow of src's frame; mask, NULL
 * or n x h x w uint8 in the alphabet of fotg_fb_check.  The definition, in order:
 *   1. Half-vector.  shutter256 in 1 .. 512 is round(256 shutter) (shutter 1 = the exposure lasts the whole frame interval);
 *      s = (float)shutter256 / 32 (exact); hx = (int)rintf(u s), hy = (int)rintf(v s).  A pixel is unknown, H = (0, 0), when u or v
 *      is not finite or |u| or |v| is above 4096, or a mask is given and its byte is non-zero.  len = M(hx, hy), the exact integer
 *      root of the motion histograms (step 3 there); cap16 = 16 max_blur, max_blur in 1 .. 32 pixels; if len > cap16 then
 *      hx = hx cap16 / len, hy = hy cap16 / len (C integer division: towards zero) and len = M(hx, hy) again.
 *   2. Tiles of 32 x 32 pixels, partial at the right and bottom edges.  tilemax = the H of the tile's pixel with the largest
 *      hx hx + hy hy, the lowest linear pixel index on a tie.  D(tile) = the tilemax with the largest squared length among the up to
 *      nine tiles around it, the first in raster order on a tie.  lenD = M(Dx, Dy).
 *   3. Gather, for the pixel X = (x, y) of a tile with D.  lenD < 8: dst = src, code 0, or 3 if X is unknown (the copy path).
 *      Otherwise L = (lenD + 15) / 16 (at most 32) and for k = -L .. L, with a = |k|:
 *        o_k = (ox, oy): ox = sign(Dx k) ((2 |Dx| a + L) / (2 L)), oy alike (half away from zero: o_-k = -o_k)
 *        Y_k = (x + ((ox + 8) >> 4), y + ((oy + 8) >> 4)) (arithmetic shift: the nearest pixel, a half towards +inf), clamped to
 *              the frame; the tap is `clamped` when the clamp moved it
 *        d_k = lenD a / L
 *        r(P) = |Hx(P) Dx + Hy(P) Dy| / lenD                                   (integer division: the reach of P along the line)
 *        w_k = clamp(max(r(Y_k), r(X)) + 16 - d_k, 0, 16)                        (so w_0 = 16)
 *      8-bit frames, per channel: dst = (2 sum w_k c_k + W) / (2 W), W = sum w_k, in integers.  f32 frames: acc = 0, then
 *      acc = acc + (float)w_k c_k for k ascending, every tap (those of weight 0 too), every operation rounded on its own;
 *      dst = acc / (float)W.
 *      code = the first that applies of: 3, X is unknown; 2, a tap with w_k > 0 was clamped; 1, a tap k != 0 had w_k > 0; 0.
 *   4. stats, per image eight int64: the pixels of code 0, 1, 2, 3; the taps with w_k > 0 summed over the pixels of the gather
 *      path (k = 0 included; a pixel of the copy path adds none); the tiles that took the copy path; the largest len; 0.
 * Outputs: dst, of src's shape and type; code, NULL or n x h x w uint8; vectors, NULL or n x h x w x 2 int16, H; stats, NULL or
 * n x 8 int64.  Two identical calls give identical bytes.  Everything is enqueued on `stream`; H and the tile maxima live in
 * stream-ordered memory of the call.  FOTG_ERR_ARG, decided before the device is touched: n outside 1 .. 65535, w or h outside
 * 1 .. 16384, a type or channel count that is none of the above, shutter256 outside 1 .. 512, max_blur outside 1 .. 32, a null src,
 * flow or dst, an output overlapping an input or another output. */
enum { FOTG_BLUR_U8 = 0, FOTG_BLUR_F32 = 1 };
int fotg_motion_blur(int device, int n, const void *src, int type, int channels, const float *flow, int w, int h,
                     const unsigned char *mask, int shutter256, int max_blur, void *dst, unsigned char *code, short *vectors,
                     long long *stats, void *stream);
/* The same on the coarse flow of a context (n x hl x wl x 2, as fotg_calc_batch returns it), upsampled and cropped on the fly, src
 * and mask of h_org x w_org: every output equals fotg_motion_blur on fotg_upsample_crop's output bit for bit, without the
 * full-resolution flow ever being written.  FOTG_ERR_ARG also for n > max_batch and a depth-mode context. */
int fotg_upsample_crop_motion_blur(fotg_ctx *ctx, int n, const void *src, int type, int channels, const float *coarse_flow,
                                   const unsigned char *mask, int shutter256, int max_blur, void *dst, unsigned char *code,
                                   short *vectors, long long *stats, void *stream);

/* ---- background plates and mosaics: a median of frames along their motion, csrc/plate.hip.h -----------------------------------
 * The frames of a shot are pulled into one coordinate system and reduced per pixel by a robust estimate over the frames that see
 * the pixel: the clean plate (the scene without its moving objects), on a canvas larger than the frame the mosaic of a panning
 * shot.  All arithmetic f32, every operation rounded on its own, in this order.
 * Inputs: frames, a stack of T frames w x h x channels, channels 1 or 3 interleaved, f32 or 8-bit (the _u8 forms; taps converted
 * exactly to f32), on the device, 1 <= w, h <= 16384.  n plates on a common W x H canvas, 1 <= W, H <= 16384, with an integer
 * origin (ox, oy), |ox|, |oy| <= 2^20: canvas pixel (X, Y) is the reference coordinate (x, y) = (X - ox, Y - oy).  Per plate i K
 * frame indices b_k = index[i K + k], 1 <= K <= 32, -1 = absent (skipped entirely).
 * Vector per sample (i, k) at every canvas pixel, from one of three sources:
 *   dense   fotg_plate:                flows n x K x H x W x 2 f32
 *   motion  fotg_plate_motion:         params n x K x 6 f64 in fotg_fit_motion's pixel-frame convention for the w x h frame;
 *           (u, v) = motion_predict(motion_coef(P, w, h), 2x - (w-1), 2y - (h-1)): fotg_motion_flow's arithmetic, evaluated at a
 *           reference coordinate that may lie outside the frame
 *   fused   fotg_upsample_crop_plate:  the coarse flows of a context, n K of them, upsampled and cropped on the fly; the canvas is
 *           the frame grid (W = w_org, H = h_org, origin (0, 0)) and n K <= max_batch
 * Admission: the samples are visited in ascending k; a sample is admitted by these tests, in this order:
 *   1. u and v are finite
 *   2. xx = (float)x + u and yy = (float)y + v satisfy fotg_warp's inside test (own == 0; otherwise own = 2)
 *   3. occ is NULL or occ[i][k][Y][X] == 0                     (occ: n x K x H x W uint8 on the canvas grid)
 *   4. exclude is NULL or it is zero at all four clamped tap pixels (x1|x2, y1|y2 of fotg_warp) of frame b_k
 *                                                              (exclude: T x h x w uint8, per source frame)
 *   5. no channel of the value s of fotg_warp's taps of frame b_k at (xx, yy) is NaN
 * The number admitted is m, the number that passed tests 1 and 2 is the coverage.
 * Estimate, per channel over the admitted values:
 *   mode 0, the median: the values ordered by f32 <, ties keeping the k order; s[(m-1)/2] for odd m,
 *           (s[m/2 - 1] + s[m/2]) * 0.5f for even m
 *   mode 1, the mean:   sum = s_0; sum = sum + s_j for j = 1 .. m-1 in k order; sum / (float)m, a correctly rounded division
 * Outputs, each may be NULL (not all of them), 1 <= min_count <= K:
 *   dst    n x H x W x channels of the frames' type: the estimate where code == 0, `fill` elsewhere; an 8-bit dst (and fill) is
 *          rounded as fotg_warp's
 *   count  n x H x W uint8: m
 *   code   n x H x W uint8: 0 where m >= min_count; 2 where fewer than min_count frames cover the pixel (coverage < min_count);
 *          1 otherwise: the masks hid the covering frames
 *   stats  n x 6 f64 per plate: [0..2] the pixels of code 0, 1, 2; [3] the sum of count; with a comparison image ref (n x H x W x
 *          channels of dst's type) over the code-0 pixels and all channels [4] sum (double)|ref - estimate| and [5] sum
 *          (double)|ref - s_0|, the first admitted sample: the overwrite mosaic as a baseline; each term the f32 fabsf of the f32
 *          difference of the unrounded values; without ref both are 0.  The sums are added in a fixed order (no floating-point
 *          atomics): the same bits every run, from every source and every launch shape.
 * index is a HOST array: validated on the host and consumed before the call returns; it reaches the kernel by a stream-ordered
 * copy into memory of the call.  Everything else is enqueued on `stream`; the partial sums live in stream-ordered memory of the call.
 * FOTG_ERR_ARG, decided before the device is touched: n outside 1..65535, K outside 1..32, T < 1, a frame or canvas side outside
 * 1..16384, an origin beyond 2^20, channels not 1 or 3, a mode other than 0 and 1, min_count outside 1..K, an index outside
 * [-1, T), a null frames, source or index, all four outputs null, and by both rules of csrc/spans.h: an output (dst, count, code,
 * stats) overlapping an input (frames, the source, occ, exclude, ref) -- overlap_any -- or another output -- overlap_among.  The
 * fused forms also for a null or depth-mode context and n K > max_batch. */
int fotg_plate(int device, int n, int K, int T, const float *frames, int w, int h, int channels, const int *index, const float *flows,
               int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode, int min_count, float fill,
               const float *ref, float *dst, unsigned char *count, unsigned char *code, double *stats, void *stream);
int fotg_plate_u8(int device, int n, int K, int T, const unsigned char *frames, int w, int h, int channels, const int *index,
                  const float *flows, int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode,
                  int min_count, float fill, const unsigned char *ref, unsigned char *dst, unsigned char *count, unsigned char *code,
                  double *stats, void *stream);
int fotg_plate_motion(int device, int n, int K, int T, const float *frames, int w, int h, int channels, const int *index,
                      const double *params, int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode,
                      int min_count, float fill, const float *ref, float *dst, unsigned char *count, unsigned char *code, double *stats,
                      void *stream);
int fotg_plate_motion_u8(int device, int n, int K, int T, const unsigned char *frames, int w, int h, int channels, const int *index,
                         const double *params, int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude,
                         int mode, int min_count, float fill, const unsigned char *ref, unsigned char *dst, unsigned char *count,
                         unsigned char *code, double *stats, void *stream);
int fotg_upsample_crop_plate(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows, const float *frames, int channels,
                             const int *index, const unsigned char *occ, const unsigned char *exclude, int mode, int min_count, float fill,
                             const float *ref, float *dst, unsigned char *count, unsigned char *code, double *stats, void *stream);
int fotg_upsample_crop_plate_u8(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows, const unsigned char *frames, int channels,
                                const int *index, const unsigned char *occ, const unsigned char *exclude, int mode, int min_count,
                                float fill, const unsigned char *ref, unsigned char *dst, unsigned char *count, unsigned char *code,
                                double *stats, void *stream);
/* Canvas rows per workgroup of the plate kernel (64 lanes each): 1, 2 or 4.  The results are the same bits; this exists to time
 * the launch shapes.  Sets the process-wide value for later calls (any other value only queries) and returns the previous one. */
int fotg_plate_rows(int rows);

/* ---- background subtraction against a plate, with two thresholds for hysteresis, csrc/subtract.hip.h ---------------------------
 * Every frame is compared with the plate (fotg_plate's output) sampled into the frame's own grid; the difference is averaged over
 * a small window and classified by a low and a high threshold.  It finds what fotg_fit_motion's code cannot: an object that
 * stops, one that moves slowly, the untextured inside of a large one.
 * Inputs: n frames w x h x channels, channels 1 or 3 interleaved, f32 or 8-bit (the _u8 forms), 1 <= w, h <= 16384.  P plates of
 * the frames' type and channel count on a W x H canvas, 1 <= W, H <= 16384, with an integer origin (ox, oy), |ox|, |oy| <= 2^20:
 * canvas pixel (X, Y) is the reference coordinate (X - ox, Y - oy), as in fotg_plate.  index[i] in 0 .. P-1 is the plate of
 * frame i, a HOST array of n entries; NULL: plate 0 for P == 1, plate i for P == n.
 * The vector frame i -> reference at every frame pixel (x, y), from one of three sources:
 *   dense   fotg_subtract:                flows n x h x w x 2 f32
 *   motion  fotg_subtract_motion:         params n x 6 f64 in fotg_fit_motion's pixel-frame convention for the w x h frame;
 *           (u, v) = motion_predict(motion_coef(P_i, w, h), 2x - (w-1), 2y - (h-1)): fotg_motion_flow's arithmetic
 *   fused   fotg_upsample_crop_subtract:  the coarse flows of a context, n <= max_batch of them (the pairs (frame i, reference)),
 *           upsampled and cropped on the fly; the frames have the context's original size; a two-channel context
 * Per frame pixel, all arithmetic f32, every operation rounded on its own, in this order:
 *   1. (u, v) not finite, or mask[i][y][x] != 0 (mask: n x h x w uint8 or NULL, fotg_fb_check's):           code 3
 *   2. Xc = (float)(x + ox) + u;  Yc = (float)(y + oy) + v;  fotg_warp's inside test warp_inside(Xc, Yc, W, H) fails:   code 2
 *   3. plate_code (P x H x W uint8 or NULL, fotg_plate's code) of plate index[i] is non-zero at any of the four clamped tap
 *      pixels (x1|x2, y1|y2 of fotg_warp) at (Xc, Yc) -- the test of fotg_plate's exclude:                  code 2
 *   4. s = fotg_warp's taps warp_taps(plate[index[i]], W, H, Xc, Yc); any channel of s or of the frame pixel f is NaN:  code 3
 *   5. otherwise the pixel is admissible:
 *        d  = 0;  per channel in order: e = fabsf(f_ch - s_ch);  d = e > d ? e : d    (the largest channel difference; the frame
 *             value converted to float, the taps of an 8-bit plate left unrounded)
 *        Dq = (int)(fminf(d * 16.f, 32767.f) + 0.5f)           the difference in 1/16 grey levels, saturating at 2047.9 levels
 * Window: r = window in {0, 1, 2} (1 x 1, 3 x 3, 5 x 5); over the pixels of the frame within the window S = the sum of Dq over
 * the admissible pixels and C = their number.  Everything after Dq is integer: no summation order matters.
 * Thresholds: L = lrintf(16 low), Hh = lrintf(16 high), 0 <= L <= Hh <= 32767.
 * Code of an admissible pixel: 4 (strong foreground) if S >= Hh * C, otherwise 1 (foreground) if S >= L * C, otherwise 0.
 * Alphabet: 0 background, 1 foreground, 2 no plate there, 3 unknown, 4 strong foreground; 0 .. 3 mean what they mean in the other
 * code maps, and fotg_label_components with the foreground set {1, 4} takes the map as it is.
 * Outputs, each may be NULL (not all of them):
 *   code      n x h x w uint8
 *   diff      n x h x w int16: Dq at admissible pixels, 0 elsewhere
 *   evidence  n x h x w x 2 f32: (code == 4 ? 1 : 0, Dq / 16), (0, 0) where inadmissible.  As the values of
 *             fotg_label_components it makes a row's sum_u / 256 the number of strong pixels of the component -- a component
 *             counts only if it holds one: the hysteresis -- and sum_v 16 times the sum of Dq, exactly
 *   stats     n x 7 int64 per frame: [0..4] the pixels of code 0 .. 4, [5] the sum of Dq over the admissible pixels, [6] the sum of
 *             Dq over the pixels of code 1 or 4.  Cleared by a stream-ordered memset inside the call and accumulated by integer
 *             atomics: the same value every run.
 * Everything is enqueued on `stream`; index is validated on the host and consumed before the call returns.
 * FOTG_ERR_ARG, decided before the device is touched: n or P outside 1..65535, a frame or canvas side outside 1..16384, an origin
 * beyond 2^20, channels not 1 or 3, a window outside 0..2, thresholds that are not finite or not 0 <= L <= Hh <= 32767, a plate
 * index outside 0 .. P-1 (a NULL index with P other than 1 and n), a null frames, plate or source, all four outputs null, and by
 * both rules of csrc/spans.h: an output (code, diff, evidence, stats) overlapping an input (frames, plate, the source,
 * plate_code, mask) -- overlap_any -- or another output -- overlap_among.  The fused forms also for a null or depth-mode context
 * and n > max_batch. */
int fotg_subtract(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H, int ox,
                  int oy, const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask, float low,
                  float high, int window, unsigned char *code, short *diff, float *evidence, long long *stats, void *stream);
int fotg_subtract_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate, int W,
                     int H, int ox, int oy, const int *index, const float *flows, const unsigned char *plate_code,
                     const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff, float *evidence,
                     long long *stats, void *stream);
int fotg_subtract_motion(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H,
                         int ox, int oy, const int *index, const double *params, const unsigned char *plate_code,
                         const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff, float *evidence,
                         long long *stats, void *stream);
int fotg_subtract_motion_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate,
                            int W, int H, int ox, int oy, const int *index, const double *params, const unsigned char *plate_code,
                            const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff,
                            float *evidence, long long *stats, void *stream);
int fotg_upsample_crop_subtract(fotg_ctx *ctx, int n, const float *coarse_flows, const float *frames, int channels, int P,
                                const float *plate, int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code,
                                const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff,
                                float *evidence, long long *stats, void *stream);
int fotg_upsample_crop_subtract_u8(fotg_ctx *ctx, int n, const float *coarse_flows, const unsigned char *frames, int channels, int P,
                                   const unsigned char *plate, int W, int H, int ox, int oy, const int *index,
                                   const unsigned char *plate_code, const unsigned char *mask, float low, float high, int window,
                                   unsigned char *code, short *diff, float *evidence, long long *stats, void *stream);

/* ---- object removal: a mask grown by a disc, feathered at its rim and filled from the plate, csrc/erase.hip.h -------------------
 * What background subtraction found (fotg_subtract, fotg_label_components), or any other mask, taken out of the frames: under the
 * grown mask the frame is replaced by the plate sampled into the frame's own grid, with a ramp at the rim.
 *
 * n frames of w x h with 1 or 3 interleaved channels, f32 or 8-bit; P plates on a W x H canvas with integer origin (ox, oy), index,
 * plate_code, mask and the three sources of the vector frame i -> reference (dense flows, six f64 parameters per frame through
 * MotionSrc, a context's coarse flows through UpsampleSrc) exactly as in fotg_subtract.  remove: n x h x w bytes, non-zero = take
 * this pixel out.  grow = G and feather = F are integers, 0 <= G <= 8, 0 <= F <= 8; R = G + F.  Per frame pixel (x, y), in this order:
 *   1. Distance (integers).  D2 = the smallest (x - x')^2 + (y - y')^2 over the pixels (x', y') of the frame with remove != 0,
 *      |x - x'| <= R and |y - y'| <= R; without one the pixel is far.  Pixels outside the frame hold nothing.
 *   2. Weight, alpha in 0 .. 256 (integers).  far: alpha = 0;  D2 <= G * G: alpha = 256;  otherwise with F == 0: alpha = 0;  otherwise
 *        D16 = floor(sqrt(256 * D2)), the exact integer root;  E = 16 * (G + F) - D16;
 *        alpha = E <= 0 ? 0 : min(256, (256 * E + 8 * F) / (16 * F))          (integer division)
 *      256 at distance G, 0 from distance G + F on, 16 steps per pixel between.
 *   3. Sample, only where alpha > 0: steps 1 to 4 of fotg_subtract with the same helpers (warp_inside, warp_sat, clampi, warp_taps),
 *      except that a NaN in the frame pixel does not disqualify:
 *        (u, v) not finite, or mask[i][y][x] != 0:                                                            code 3
 *        Xc = (float)(x + ox) + u;  Yc = (float)(y + oy) + v;  !warp_inside(Xc, Yc, W, H):                    code 2
 *        plate_code[index[i]] non-zero at any of the four clamped tap pixels of fotg_warp at (Xc, Yc):        code 2
 *        s = warp_taps(plate[index[i]], W, H, Xc, Yc);  any channel of s is NaN:                              code 3
 *   4. Value, f the frame's pixel.  alpha == 0, or code 2 or 3: dst = f, copied bit for bit.  alpha == 256 and a good sample: dst = s
 *      (8-bit: warp_to_u8(s)), code 1.  0 < alpha < 256 and a good sample: code 4, a = (float)alpha * 0.00390625f and per channel
 *      dst = f + (s - f) * a, every operation rounded on its own (8-bit: through warp_to_u8).
 *      alphabet: 0 untouched, 1 replaced, 2 no plate there (kept), 3 unknown (kept), 4 blended
 *   5. Outputs, each optional, at least one: dst (the frames' type and shape), code (n x h x w uint8), alpha (n x h x w int16),
 *      stats (n x 8 int64 per frame: [0..4] the pixels of code 0 .. 4, [5] the pixels with alpha == 256 and code 2 or 3 -- the holes,
 *      where an object is still visible --, [6] the pixels with remove != 0, [7] the sum of alpha).  stats is cleared by a
 *      stream-ordered memset inside the call and accumulated by integer atomics: the same bytes every run.
 *   With alpha as the only output nothing is sampled: frames, the plate and the source of the vectors are not read and may be null;
 *   alpha == 256 is then the dilation of remove by the disc of radius G (flowonthego_amd.erase.grow_mask).
 *
 * Everything is enqueued on `stream`; index is validated on the host and consumed before the call returns.
 * FOTG_ERR_ARG, decided before the device is touched: n or P outside 1..65535, a frame or canvas side outside 1..16384, an origin
 * beyond 2^20, channels not 1 or 3, grow or feather outside 0..8, a plate index outside 0 .. P-1 (a NULL index with P other than 1
 * and n), a null remove, all four outputs null, a null frames, plate or source unless alpha is the only output, and by both rules
 * of csrc/spans.h: an output (dst, code, alpha, stats) overlapping an input (frames, plate, the source, plate_code, mask, remove)
 * -- overlap_any -- or another output -- overlap_among.  The fused forms also for a null or depth-mode context and n > max_batch. */
int fotg_erase(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H, int ox, int oy,
               const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask, const unsigned char *remove,
               int grow, int feather, float *dst, unsigned char *code, short *alpha, long long *stats, void *stream);
int fotg_erase_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate, int W, int H,
                  int ox, int oy, const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask,
                  const unsigned char *remove, int grow, int feather, unsigned char *dst, unsigned char *code, short *alpha, long long *stats,
                  void *stream);
int fotg_erase_motion(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H, int ox,
                      int oy, const int *index, const double *params, const unsigned char *plate_code, const unsigned char *mask,
                      const unsigned char *remove, int grow, int feather, float *dst, unsigned char *code, short *alpha, long long *stats,
                      void *stream);
int fotg_erase_motion_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate, int W,
                         int H, int ox, int oy, const int *index, const double *params, const unsigned char *plate_code,
                         const unsigned char *mask, const unsigned char *remove, int grow, int feather, unsigned char *dst,
                         unsigned char *code, short *alpha, long long *stats, void *stream);
int fotg_upsample_crop_erase(fotg_ctx *ctx, int n, const float *coarse_flows, const float *frames, int channels, int P, const float *plate,
                             int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code, const unsigned char *mask,
                             const unsigned char *remove, int grow, int feather, float *dst, unsigned char *code, short *alpha,
                             long long *stats, void *stream);
int fotg_upsample_crop_erase_u8(fotg_ctx *ctx, int n, const float *coarse_flows, const unsigned char *frames, int channels, int P,
                                const unsigned char *plate, int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code,
                                const unsigned char *mask, const unsigned char *remove, int grow, int feather, unsigned char *dst,
                                unsigned char *code, short *alpha, long long *stats, void *stream);

/* ---- binary morphology of masks and code maps: erode, dilate, open and close by a disc, csrc/morph.hip.h ----------------------
 * The step between a code map (fotg_subtract, fotg_fit_motion, fotg_fb_check) and what reads masks (fotg_label_components,
 * fotg_erase, fotg_plate's exclude): speckle is opened away, pin-holes are closed.  Exact and in integers.
 *
 * n maps of w x h bytes, 1 <= w, h <= 16384, n <= 65535.  A pixel is set if its byte belongs to the foreground set: with
 * fg_codes == 0 every non-zero byte; otherwise fg_codes is an 8-bit set as in fotg_label_components and byte b is set iff
 * b < 8 && ((fg_codes >> b) & 1), so that a code map goes in unconverted.  The structuring element is the disc
 * dx^2 + dy^2 <= r^2 with r an integer in 0 .. 8, the disc of fotg_erase's grow.  Per map X and stage, on the whole frame:
 *   dilate(X, r): a pixel is set iff some pixel of the frame within the disc around it is set;
 *   erode(X, r):  a pixel is set iff every pixel of the frame within the disc around it is set.
 * Pixels outside the frame take no part in either: the frame border does not erode, and inside the frame exactly
 * erode(X, r) = not dilate(not X, r).  r = 0 is the identity and yields the 0 / 1 map of the foreground set.
 * A call evaluates a chain of nstage = 1 or 2 stages, stage k an erode (ops[k] == 0) or a dilate (ops[k] == 1) with its own radius
 * radii[k], the second on the whole-frame result of the first:
 *   open(X, r) = dilate(erode(X, r), r);  close(X, r) = erode(dilate(X, r), r).
 * Outputs, each optional, at least one: out (n x h x w uint8, 0 or 1), stats (n x 4 int64 per map: [0] the set pixels of the
 * input, [1] the set pixels of the result, [2] the pixels added -- set in the result and not in the input --, [3] the pixels
 * removed).  stats is cleared by a stream-ordered memset inside the call and accumulated by integer atomics: the same bytes every run.
 *
 * One launch per call, whatever the chain: the intermediate map of an opening or a closing never reaches memory.  Everything is
 * enqueued on `stream`; ops and radii are HOST arrays of nstage ints, consumed before the call returns; nothing synchronises.
 * FOTG_ERR_ARG, decided before the device is touched: n outside 1..65535, w or h outside 1..16384, a null src, fg_codes outside
 * 0..255, nstage not 1 or 2, null ops or radii, an op other than 0 (erode) and 1 (dilate), a radius outside 0..8, both outputs null,
 * and by both rules of csrc/spans.h: out or stats overlapping src -- overlap_any -- or each other -- overlap_among. */
int fotg_morph(int device, int n, const unsigned char *src, int w, int h, int fg_codes, int nstage, const int *ops, const int *radii,
               unsigned char *out, long long *stats, void *stream);

/* ---- hole filling by pull-push: frames and flows inpainted from their known pixels, csrc/fill.hip.h --------------------------------
 * What fotg_erase leaves as holes (no plate), what fotg_fb_check marks and fotg_flow_filter cannot reach, the unknown vectors of a
 * .flo file and a sparse set of vectors all become a dense image: a pyramid of sums over the known pixels (pull) is interpolated back
 * down into the holes (push).  Gortler et al., "The Lumigraph", 1996; Kraus, "The pull-push algorithm revisited", 2009.
 *
 * n images of w x h pixels with ch interleaved channels, 1 <= w, h <= 16384, 1 <= n <= 65535.  f32 images take ch in {1, 2, 3}, uint8
 * images ch in {1, 3}.  hole is n x h x w uint8, or NULL (f32 only).  fg_codes in 0 .. 255 follows fotg_morph's rule: with
 * fg_codes == 0 every non-zero byte is a hole; otherwise byte b is a hole iff b < 8 && ((fg_codes >> b) & 1), so that a code map
 * goes in unconverted.
 * Known pixels: a pixel is known iff it is not a hole and, for f32, every channel v is finite with |v| <= 32768.  A NaN, an infinity
 * and the .flo unknown marker 1e9 are therefore holes with no map at all.
 * Pull (exact integers): q = lrintf(256 v) per channel (256 v is exact in f32; for uint8 q = 256 v).  Level 0 has S_0 = q and N_0 = 1
 * at known pixels and 0 elsewhere.  Level l+1 has size w_{l+1} = (w_l + 1) >> 1, h_{l+1} = (h_l + 1) >> 1; S_{l+1}(X, Y) and
 * N_{l+1}(X, Y) are the sums over the children (2X + i, 2Y + j), i, j in {0, 1}, that lie inside level l.  L is the first level of
 * size 1 x 1.  S is an int64 per channel with |S| <= 2^51, N an integer <= 2^28.
 * Empty image: if N_L == 0 the image knows nothing; then dst = src bit for bit and code is 2 at every hole pixel and 0 at every known
 * pixel.
 * Mean of a block with N_l > 0: M_l = (float)((double)S_l / (double)(256 N_l)), one f64 division rounded once to f32 (exact to
 * restate, because |S| < 2^53).
 * Push, for l = L-1 down to 0: F_L = M_L.  At level l a pixel with N_l > 0 and l >= 1 has F_l = M_l.  A pixel with N_l == 0 at (x, y)
 * takes the bilinear value of its four parents: px = x >> 1, px2 = clamp(px + (x & 1 ? 1 : -1), 0, w_{l+1} - 1), py and py2 likewise;
 * a = F_{l+1}(px, py), b = F_{l+1}(px2, py), c = F_{l+1}(px, py2), d = F_{l+1}(px2, py2);
 *   F_l = ((a*9 + b*3) + (c*3 + d)) * 0.0625 in f32, in exactly this order, with no contraction.
 * At level 0 a known pixel keeps its source value bit for bit (it does not become its quantised value); a hole pixel gets F_0, for
 * uint8 rintf, clamped to [0, 255] (fotg_warp's to_u8).
 * Outputs, each optional, at least one: dst (same type and shape as src), code (n x h x w uint8: 0 known (kept), 1 filled, 2 nothing
 * known in this image (kept)), stats (n x 4 int64: known, filled, unfilled, depth).  depth = 1 + the largest l at which some block
 * has N_l == 0, and 0 without holes: the log2 scale of the widest hole.  stats is zeroed by a stream-ordered memset and accumulated
 * with integer atomics and integer maxima: the same bytes every run.
 *
 * Three launches per chunk of images (pull, top, push) over stream-ordered memory of the call: fotg_fill_scratch states its size,
 * host only, the device is not touched.  A batch whose levels would take more than 1 GiB is worked through in chunks of as many
 * images as fit in 1 GiB (at least one) inside the call, so a call takes at most max(the bytes of one image's levels, 1 GiB); one
 * image takes about 0.35 of its f32 size.  Everything is enqueued on `stream`; nothing synchronises.  Not built: filling in place,
 * an edge-aware or guided push, weights other than 0 / 1, inpainting from other frames, more than 3 channels.
 * FOTG_ERR_ARG, decided before the device is touched: n outside 1..65535, w or h outside 1..16384, ch outside {1, 2, 3} (f32) or
 * {1, 3} (uint8), fg_codes outside 0..255, a null src, a null hole with uint8, all three outputs null, and by both rules of
 * csrc/spans.h: an output overlapping src or hole -- overlap_any -- or another output -- overlap_among.  fotg_fill_scratch: the same
 * ranges, and a null bytes. */
int fotg_fill(int device, int n, const float *src, int w, int h, int ch, const unsigned char *hole, int fg_codes, float *dst,
              unsigned char *code, long long *stats, void *stream);
int fotg_fill_u8(int device, int n, const unsigned char *src, int w, int h, int ch, const unsigned char *hole, int fg_codes,
                 unsigned char *dst, unsigned char *code, long long *stats, void *stream);
int fotg_fill_scratch(int n, int w, int h, int ch, long long *bytes);

/* op.verbosity of the reference (src/oflow.cpp:246-365, kroeger/oflow.cpp:298-360).  0 (default): silent, asynchronous.
 * > 0: every flow call (fotg_calc, fotg_calc_batch, ...) waits for its launches and prints "TIME (O.Flow Run-Time   ) (ms): ..."
 * (the flow without the pyramid, like the reference); > 1: also one "TIME (Sc: .., #p: .., pconst, pinit, poptim, cflow, tvopt,
 * total): ..." line per scale, from HIP-event times of the stages on the launch stream (patch construction and initialisation
 * are part of the LK launch: pconst = pinit = 0). */
int fotg_set_verbosity(fotg_ctx *ctx, int verbosity);
/* the five times (ms) of `level` measured by the last flow call with verbosity > 0: pconst, pinit, poptim, cflow, tvopt
 * (PatGridClass::printTimings, src/patchgrid.cpp:334-345, prints from these) */
int fotg_level_timings(fotg_ctx *ctx, int level, float *ms5);

/* geometry queries */
int fotg_level_size(const fotg_ctx *ctx, int level, int *w, int *h);        /* unpadded level size */
int fotg_out_size(const fotg_ctx *ctx, int *w, int *h);                     /* finest-scale flow size */
int fotg_num_patches(const fotg_ctx *ctx, int level, int *nopw, int *noph); /* PatGridClass::GetNumPatches{W,H} */

/* ---- per-stage entry points (what PatGridClass / VarRefClass / the pyramid helpers bind to) ---- */

/* cu::constructImgPyramids (src/kernels/pyramid.cpp:32-223) with kroeger semantics (run_dense.cpp:130-178).
 * which: 0 -> I0 (image + gradients), 1 -> I1 (image only; its gradients are never read, patch.cpp:266). */
int fotg_pyramid(fotg_ctx *ctx, int n, const float *I, int which, void *stream);
/* both frames of n pairs in shared launches (what fotg_calc_batch does).  stages: bit 0 = the HBM-streaming base
 * kernel (frames -> level min(sc_l,4)), bit 1 = coarser levels + borders + gradients; 3 = everything. */
int fotg_pyramid_pair(fotg_ctx *ctx, int n, const float *I0, const float *I1, int stages, void *stream);
/* the same from 8-bit frames (noc channels, or three with fotg_params::u8_color): what the 8-bit flow entry points run first */
int fotg_pyramid_pair_u8(fotg_ctx *ctx, int n, const unsigned char *I0, const unsigned char *I1, int stages, void *stream);
/* device pointer of a pyramid plane of pair 0 (pairs are `*pair_stride` floats apart).
 * kind: 0 image, 1 dx, 2 dy.  Layout (h_l+2ps) x (w_l+2ps) x noc, like the reference's padded levels. */
int fotg_level_ptr(fotg_ctx *ctx, int which, int level, int kind, float **ptr, long *pair_stride);

/* PatGridClass (src/patchgrid.h:13-86).  Grid state lives in the context, one grid per level.
 * All level images use the padded layout above; n pairs, `pair_stride` floats apart. */
int fotg_grid_init(fotg_ctx *ctx, int level, int n, const float *I0, const float *I0x, const float *I0y,
                   long pair_stride, void *stream);                                   /* InitializeGrid */
int fotg_grid_set_target(fotg_ctx *ctx, int level, const float *I1, long pair_stride);  /* SetTargetImage */
int fotg_grid_init_from_coarser(fotg_ctx *ctx, int level, int n, const float *flow_prev, void *stream); /* InitializeFromCoarserOF */
/* depth mode only: camera side of the level's grid and of fotg_varref on that level, camparam::camlr (kroeger/oflow.h:28):
 * 0 = left camera, displacement <= 0 (default; what the forward grid uses), 1 = right camera, displacement >= 0 */
int fotg_grid_set_camera(fotg_ctx *ctx, int level, int camlr);
int fotg_grid_optimize(fotg_ctx *ctx, int level, int n, void *stream);                /* Optimize */
int fotg_grid_aggregate(fotg_ctx *ctx, int level, int n, float *flowout, void *stream); /* AggregateFlowDense */
/* test taps: copy grid state of pair `pair` to host.  Any pointer may be NULL.
 * p_iter: nop x 2, pweight: nop x nv, tmpl/tdx/tdy: nop x nv, hes: nop x 3, cnt: nop ints */
int fotg_grid_read(fotg_ctx *ctx, int level, int pair, float *p_iter, float *pweight, float *tmpl,
                   float *tdx, float *tdy, float *hes, int *cnt);
/* allocate the optional tap buffers (templates, Hessians, iteration counts) that fotg_grid_read returns;
 * off by default so the production path writes nothing it does not need */
int fotg_enable_taps(fotg_ctx *ctx, int on);
/* per-iteration trace for tests: host buffer nop x (max_iter+1) x 4 [p0,p1,mares,cnt] of pair 0; the next
 * fotg_grid_optimize on this level fills it (synchronously).  NULL disables. */
int fotg_grid_set_trace(fotg_ctx *ctx, int level, float *trace_host);

/* VarRefClass::VarRefClass(I0, I1, iparams, op, flowout) (src/refine_variational.cpp:31-145):
 * refines `flow` (n x h_l x w_l x 2, device) in place. */
int fotg_varref(fotg_ctx *ctx, int level, int n, const float *I0, const float *I1, long pair_stride,
                float *flow, void *stream);
/* test tap: copy one refinement workspace plane (stride-padded, FDF image_t layout) of pair `pair` to host.
 * The solver planes (du, dv, a11 .. sv) of levels refined entirely on chip are only written back when
 * fotg_enable_taps(ctx, 1) was called before fotg_varref.
 * name: "wx","wy","mask","du","dv","sh","sv","a11","a12","a22" (block inverse),"b1","b2","avg","Iz","Ix","Iy","Ixx","Ixy","Iyy","Ixz","Iyz"
 * depth mode: "wx","mask","du","uu","s","a11","b1","sh","sv" and the image planes (a11/b1: the scalar system of compute_data_DE) */
int fotg_varref_plane(fotg_ctx *ctx, int pair, const char *name, int level, float *host_out);

/* measurement tap: ONE sor_coupled call (the launch the refinement issues once per inner iteration) of `level` for n pairs on the
 * system the last fotg_varref left in the workspace; bench.py times it for the roofline of the time-dominant kernel */
int fotg_bench_sor_call(fotg_ctx *ctx, int level, int n, void *stream);
/* test tap: how often a kernel variant was launched by this process ("sor_stream", "sor_tiles"); -1 for unknown names */
long fotg_debug_counter(const char *name);
/* per-context counters.  "take_stall" (does NOT synchronise; the query for callers of the asynchronous entry points, AFTER their own
 * synchronisation): 1 = a bounded inter-workgroup wait of this context timed out since the last query / the last FOTG_ERR_STALL
 * -- the flows computed since then are not valid --, 0 = none; it clears the flag.  "stalls" (does NOT synchronise, does not
 * clear): how many such time-outs the host has seen so far (+ 1 while one is pending).  "inject_stall" raises the flag as a timed-out
 * wait would -- only in contexts created with FOTG_TEST_TAPS=1 in the environment (tests), -1 otherwise.
 * Test tap that synchronises the device: "tile_timeouts" = device-side count of those time-outs of the tile solver since the
 * context was created -- 0 unless something is broken; -1 for unknown names */
long fotg_ctx_counter(fotg_ctx *ctx, const char *name);
const char *fotg_strerror(int status);
int fotg_last_hip_error(void);
const char *fotg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOTG_H */
