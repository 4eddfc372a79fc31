/*
 * bf_accel.h -- C-ABI of the MI355X (gfx950) motion-compensation path.
 *
 * This is the drop-in boundary for better-flow's `class AccelLib`
 * (better_flow_core/include/better_flow/accel_lib.h:14-616) as it is consumed by
 * `OptimizerRolling` (optimizer_rolling.h:19,269,294,308,322,327,340) plus the fused
 * on-device form of `OptimizerRolling::run` (optimizer_rolling.h:48-125,305-347).
 * Every entry point cites the reference interface it replaces.  All arguments are
 * plain pointers / sizes / PODs; outputs are caller-allocated; nothing throws.
 *
 * Conventions (same as the reference): fr_x is the sensor ROW, fr_y the COLUMN
 * (bf_motion_compensator.cpp:192,200); t is nanoseconds relative to the slice start
 * (Event::set_local_time, event.h:61-63) and must fit int32 (the reference's own
 * device layout, accel_lib.h:83-85); images are row-major R x C with
 * R = metric_wsizex + scale, C = metric_wsizey + scale.
 *
 * Return values: 0 = BF_OK, 1 = BF_SKIPPED (run() skipped by a guard,
 * optimizer_rolling.h:54,58 -- the reference's own "return 1"), < 0 = error.
 * There is NO CPU fallback: without a usable HIP device bf_create fails with
 * BF_ERR_NODEVICE and every other call fails with BF_ERR_ARG on a NULL ctx.
 *
 * Threading: one bf_ctx per (host thread, GPU).  A ctx is reusable across slices
 * (no per-slice allocation), owns all of its device memory, pinned staging and its HIP
 * stream, and is NOT thread-safe -- with one exception, which the stream engine
 * (better_flow/slice_farm.h) relies on: the asynchronous uploads (bf_upload_events_async,
 * bf_upload_ring_async, bf_upload_ring16_async, bf_upload_ring16t32_async, bf_upload_events16_async) and bf_wait_uploads touch only the
 * context's staging slots and copy stream and may be called from a SECOND thread while
 * the owning thread is inside bf_set_cloud, bf_set_model, bf_run or bf_compute_uv*.  The
 * caller serialises them against each other and against bf_commit_upload (one mutex),
 * and sets "stream_prealloc" first so that no upload allocates device memory in the
 * middle of a solve.  Nothing else may run concurrently on one ctx.  bf_last_error
 * returns a copy of the text private to the calling thread.
 */
#ifndef BF_ACCEL_H
#define BF_ACCEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BF_OK 0
#define BF_SKIPPED 1
#define BF_ERR_ARG (-1)
#define BF_ERR_HIP (-2)
#define BF_ERR_STATE (-3)
#define BF_ERR_NOCONV (-4)   /* hard iteration cap hit (the reference would spin) */
#define BF_ERR_NODEVICE (-5)
#define BF_ERR_CAPACITY (-6)

typedef struct bf_ctx bf_ctx;

/* ObjectModel, object_model.h:10-13. */
typedef struct bf_model {
    double cx, cy, dx, dy, rot, div;
    uint32_t cnt;
    uint32_t _pad;
    double total_dx, total_dy, total_rot, total_div;
} bf_model;

/* Window geometry of OptimizerRolling::set_cloud / set_scale,
 * optimizer_rolling.h:248-283 (members :22-31). */
typedef struct bf_window {
    int32_t scale;
    int32_t x_min, y_min, x_max, y_max;
    int32_t metric_wsizex, metric_wsizey;
    int32_t scale_img_x, scale_img_y;   /* R, C */
    int32_t _pad;
    double x_shift, y_shift;
} bf_window;

/* Options of the fused run; defaults (bf_run_opts_default) are the reference's. */
typedef struct bf_run_opts {
    int32_t max_iter;        /* OptimizerRolling::set_maxiter, :236-238; <= 0: unlimited */
    int32_t min_events;      /* literal 1000 at optimizer_rolling.h:57                  */
    int32_t res_x, res_y;    /* RES_X / RES_Y of the window guard, :49 (common.h:39-40) */
    int32_t hard_iter_cap;   /* not in the reference: give up with BF_ERR_NOCONV        */
    int32_t poll_interval;   /* iterations enqueued between host polls of `done`        */
    int32_t trace_cap;       /* per-iteration records kept for bf_get_trace (0 = none)  */
    int32_t want_uv;         /* 1: also compute per-event (u,v) (Event::compute_uv)     */
} bf_run_opts;

/* What run() leaves behind besides the model (optimizer_rolling.h:36,59). */
typedef struct bf_run_info {
    int32_t rc;              /* 0 optimised, 1 skipped, <0 error                        */
    int32_t iterations;      /* itercount                                               */
    float x_divider, y_divider, rot_divider, div_divider;
    int32_t launches;        /* kernel launches enqueued (diagnostic)                   */
    int32_t polls;           /* host polls of the done flag (diagnostic)                */
    int32_t rebins;          /* counting sorts of the events by image tile (diagnostic)  */
    int32_t overflow_events; /* events that left their bin's LDS tile, summed over the
                                iterations; they take an exact global-atomic path.  The one-kernel loop ("fused") has no
                                such path: there, the passes it repeated after a re-bin    */
} bf_run_info;

/* One record per iteration_step (trajectory tests). */
typedef struct bf_trace_rec {
    bf_model model;
    float x_divider, y_divider, rot_divider, div_divider;
    int32_t iteration;
    int32_t _pad;
} bf_trace_rec;

/* Accumulated per-kernel GPU time, measured with hipEvents on the ctx stream. */
typedef struct bf_profile {
    double warp_scatter_ms;  uint64_t warp_scatter_launches;
    double stencil_ms;       uint64_t stencil_launches;
    double update_ms;        uint64_t update_launches;
    double other_ms;         uint64_t other_launches;
    uint64_t warp_scatter_events;   /* sum over launches of events processed */
} bf_profile;

/* ---- life cycle -------------------------------------------------------------- */

/* Number of visible HIP devices (0 and BF_ERR_NODEVICE if the runtime has none). */
int bf_device_count(int32_t *count);

/* AccelLib::AccelLib (accel_lib.h:44-55) + the allocations of init_gpu (:86-92,
 * :127-144).  Capacity is fixed at creation: up to max_events events and images of
 * up to max_rows x max_cols pixels (R x C).  hip_stream: a hipStream_t to run on, or
 * NULL to let the ctx create (and own) a non-blocking stream. */
int bf_create(int32_t device, int64_t max_events, int32_t max_rows, int32_t max_cols,
              void *hip_stream, bf_ctx **out);

/* AccelLib::~AccelLib / clear_buffers (accel_lib.h:57-69). */
void bf_destroy(bf_ctx *ctx);

/* Text of the last error on this ctx ("" if none).  Never NULL.  Takes the place of the reference's
 * "OpenCL Error: <n>" prints (accel_lib.h:125,138,253,299,361): errors are returned, the text is kept here. */
const char *bf_last_error(const bf_ctx *ctx);

/* Library / build identification, e.g. "bf_accel gfx950 r5" (printed by `bf_motion_compensator --version`
 * next to the reference's version line, bf_motion_compensator.cpp:26-33). */
const char *bf_version(void);

/* The reference's settings of OptimizerRolling::run: no iteration cap (optimizer_rolling.h:25,43, max_itercount = -1),
 * guards of :49-58 (1000 events, window >= scale * RES / 15), sensor 180 x 240 (common.h:39-40). */
void bf_run_opts_default(bf_run_opts *opts);

/* No reference counterpart (the reference has no foreign-language boundary).
 * sizeof() of bf_model, bf_window, bf_run_opts, bf_run_info, bf_trace_rec, bf_profile,
 * bf_local_window, bf_local_state, bf_global_pyramid_opts, bf_global_pyramid_info (in that order; later versions add at
 * the end) as this library was compiled -- lets a foreign-language binding verify its struct layouts.  Writes and returns
 * min(n, 10) entries: a caller that asks for the first 8 gets 8, as before the last two were added.  out NULL: returns 10. */
int bf_abi_struct_sizes(int32_t *out, int32_t n);

/* Tuning / test knobs that have no counterpart in the reference (each takes effect at the
 * next bf_set_cloud).  Keys:
 *   "force_split"  1: keep the event-count and time-sum accumulators in separate planes
 *                  even when they fit one packed 64-bit word.
 *   "binned"       tile-binned LDS scatter inside bf_run: 1 (default) when it pays (fewer than ~12 image pixels per
 *                  event, or an image of at most 9 M pixels -- sparse slices then take its event-list form), 2 whenever
 *                  possible, 0 never (one global atomic per event).  Results are identical.
 *   "fused"        the one-kernel iteration inside bf_run (warp + LDS scatter + stencil + moment sums of one image tile
 *                  per work-group; the events of a tile's edge strips are also read by the neighbouring tiles' work-groups):
 *                  1 (default) where it is the faster loop -- slices of at most one event per two image pixels on images
 *                  of at most 1.2 M pixels, i.e. the reference's 50 000-event ring on a 240x180 or 346x260 sensor --, 2
 *                  whenever possible, 0 never.  A "co_schedule" context takes it only for sparser slices (at most one event
 *                  per eight image pixels: launch-bound even with eight contexts in flight).  Bit-identical to the two-kernel loop;
 *                  bf_run_info::overflow_events then counts the passes that were repeated after a re-bin because an
 *                  event had moved further than the loop's margin of 8 scaled pixels (detected exactly, never a wrong sum).
 *   "persist"      the persistent form of that loop (k_fused_loop, bf_loop.hip): the work-groups stay resident, keep their
 *                  events in registers and run iteration after iteration in ONE launch, exchanging the moment sums through
 *                  tagged records in memory instead of a launch boundary; the launch ends when the loop is over or a re-bin
 *                  is due.  0 never; 1 (default) for warm-started runs (bf_set_model: a stream's chain, where a slice is
 *                  ~100 iterations and one or two re-bins) on a context that is not "co_schedule"d, is the only context of
 *                  this process on its device (two resident kernels could wait for each other's CUs) and whose tiles can
 *                  all be resident at once; 2 for cold runs too (they re-bin a dozen times, each a host round trip: slower).
 *                  Bit-identical to the other loops.
 *   BF_ACCEL_OPTIONS (environment, read by bf_create): "key=value,key=value" applied to every context of the process.
 *   "bin_pack_limit"  bits the per-bin accumulator packing may use (default 64).  The counting sort sizes the
 *                  packed count / time-sum fields from the fullest bin; if they do not fit, every event takes the
 *                  exact unpacked path.  Lower values only serve to exercise that fallback in tests.
 *   "co_schedule"  1: this context shares the GPU with other slice contexts (threads / streams).  The model /
 *                  loop update of the tile-binned loop then runs in the last work-group of the stencil kernel (a
 *                  serial tail on one CU, which the other contexts' kernels fill) instead of at the head of the
 *                  next warp+scatter launch by every work-group (the shortest iteration for a context alone, but
 *                  ~1.5 us on all CUs).  Results are identical bit for bit.  Default 0.
 *   "stream_prealloc"  1: create now what the asynchronous uploads (bf_upload_events_async / bf_upload_ring*_async) create
 *                  on first use -- the copy stream, its events, both staging slots -- so that the first slice of a stream
 *                  does not pay ~20 ms of allocations.
 *   "sep_update"   where the model / loop update of a "co_schedule"d context's two-kernel loop runs: in the stencil kernel's last
 *                  work-group (every work-group drains its accumulator atomics and takes a ticket), or as a one-wave kernel of
 *                  its own ahead of every scatter launch (the stencil kernel then only accumulates).  0 the former, 2 the latter,
 *                  1 (default): the latter for event lists -- thousands of stencil work-groups per launch, each holding its slot
 *                  ~10 % longer for the ticket -- and the former for dense tiles (a few hundred work-groups: the extra launch costs
 *                  more).  Bit-identical results.
 *   "defer_uploads"  1: an asynchronous upload (bf_upload_events_async / bf_upload_events16_async / bf_upload_ring*_async) only takes
 *                  its staging slot and remembers its arguments; the HIP calls behind it -- three copies, the staging kernels, the
 *                  events: ~25 us of host time -- are issued by the next bf_run as soon as that run's first batch of kernels is
 *                  queued (or by bf_commit_upload / bf_wait_uploads, whichever needs the slot first).  For a caller that drives
 *                  ONE warm-started chain from ONE thread (dvs_flow.h:218-224) -- commit k, upload k + 1, set_cloud, run -- that
 *                  host time otherwise falls between two runs with the GPU idle.  The host arrays must stay valid until the
 *                  slice is committed (the asynchronous uploads' contract already).  Not for callers that upload from a second
 *                  thread.  Default 0.
 *   "watchdog_ms"  a cold bf_run whose device iteration counter has not advanced for this long (wall clock, default
 *                  40000) stops with BF_ERR_HIP "device loop makes no progress" instead of waiting for ever.
 *   "bin_predict"  1 (default): re-bin as soon as the model has moved events by 0.6 x the bins' margin (8 scaled pixels;
 *                  bounded analytically), i.e. before they leave their bin's LDS tile and take the exact overflow path;
 *                  0: re-bin only on observed overflow.
 *   "bin_compact"  what the scatter kernel hands to the stencil kernel: 0 dense tiles (the bin's events merged in an LDS
 *                  tile, one accumulator per tile pixel written), 2 event lists (one entry per event: tile-local pixel
 *                  index + packed accumulator, sorted by tile row; no LDS tile); 1 (default): lists when the slice has
 *                  fewer than one event per four pixels, dense tiles otherwise.  With lists, traffic and work follow the
 *                  events instead of the image area.  Bit-identical results in either form.
 * (Round 5 removed eight keys whose sweeps had been flat for two rounds or that only forced what bf_set_cloud / bf_run choose
 * per slice -- tile width / height, margins, scatter work-group size and events per thread, the one-kernel loop's tile rows, the
 * spinning poll -- and the merged-list scatter format; tests reach the paths they forced through geometry, "bin_predict" = 0 and
 * "bin_pack_limit".)
 *   "bin_split"    dense tiles only: 0 the bin writes its whole LDS tile, margin included, and the stencil kernel merges
 *                  up to 2 x 2 such slabs per pixel; 2 the bin writes its own pixels into a tiled image and ADDS the few
 *                  words its events left in the tile's margin to a margin plane (device atomics; the bin clears them again
 *                  at its next launch): 0.6 x the bytes, a quarter of the stencil kernel's loads; 1 (default): the second
 *                  form for a context that has the GPU to itself on an image of >= 1.5 M pixels (640x480 scale 3, 1M
 *                  events: 37.2 -> 32.9 us per iteration), the first otherwise.  Bit-identical results.
 *   "delta_scatter"  the global-atomic loop on ONE plane buffer that is kept from launch to launch: the run's first launch
 *                  scatters every event, every later one warps the events and moves only those whose pixel changed (one atomic
 *                  that takes the event's word off the old pixel, one that adds it to the new one; about one event in twenty
 *                  per iteration of a cold run).  The plane words are exact integers, so the image -- and every bit behind it --
 *                  is the rebuilt one's.  0 never, 2 whenever the slice has no noise mask (it then replaces whichever loop
 *                  the slice would take), 1 (default): where it was measured to be the faster loop -- cold runs of a
 *                  "co_schedule" context on a slice that would otherwise run the two-kernel loop on dense slabs by default
 *                  ("binned" = 1), with packed planes and at least one event per image pixel (config 2 under four contexts:
 *                  218 -> 240 Mevents/s).  A slice with a noise mask keeps the plain global-atomic loop.
 *   "groups_wide"  bf_run_groups only; takes effect at the NEXT bf_run_groups, not at bf_set_cloud.  0 (default): a group whose
 *                  window does not fit one work-group's LDS gets BF_ERR_CAPACITY in its own rc and is not solved.  1: such a
 *                  group is solved inside the call by the chip-wide loop that bf_run is, as long as its window fits the
 *                  context's own image capacity ("event groups", wide groups).  Anything else is BF_ERR_ARG. */
int bf_set_option(bf_ctx *ctx, const char *key, int64_t value);

/* Diagnostics (no reference counterpart).  Keys:
 *   "scatter_format"  what the last bf_set_cloud chose for the tile-binned loop: 0 dense slabs, 2 event
 *                     lists, 3 own pixels + margin plane ("bin_split"); -1 when the slice does not take that loop.
 *   "one_kernel"      1 when bf_run would take the one-kernel iteration for the slice staged now, else 0.
 *   "loop_form"       the loop the last bf_run took (BF_LOOP_*); -1 before the first run and after a skipped one.
 *   "persistent"      1 when bf_run, called now, would run it as the persistent kernel ("persist"), else 0.
 *   "persist_giveups" launches of the persistent kernel on this context that gave up (a work-group waited 0.2 s for others
 *                     that were not resident: something else holds part of the GPU) and undid themselves; the run they
 *                     belonged to went on with one launch per iteration, and the context leaves the kernel alone for the
 *                     next 1, 2, 4 ... 64 runs.
 *   "bin_rows", "bin_cols", "bin_margin", "bins"   the bin grid the last bf_set_cloud planned for the two-kernel tile-binned
 *                     loop: a bin's rows, columns and margin in scaled pixels, and the number of bins; 0 when the slice does
 *                     not take that loop.
 *   "k1_threads", "k1_events_per_thread", "k1_head"   the scatter kernel the last bf_run launched in that loop: its work-group
 *                     size, the events a thread keeps in flight, and 1 when the model update ran at its head (0: the lean
 *                     kernel); -1 when that run launched none (one-kernel or global-atomics loop, no run yet).
 *   "k3_half_scale", "k3_mode", "k3_capped"   ... and its stencil kernel: scale / 2 (at most 4), what it read (0 dense slabs,
 *                     1 event lists, 2 own pixels + margin plane), and 1 for the build with capped scalar registers that a
 *                     launch of >= 8 tiles per CU takes; -1 as above.
 *   "propose_form"    the vote kernel the last bf_propose_models launched: 1 a histogram per work-group in LDS, 2 one global
 *                     atomic per vote; 0 when it launched none (no call yet, or no events).
 *   "groups_wide"     the groups the last bf_run_groups solved on the chip-wide loop ("groups_wide" = 1); 0 before any call.
 *   "groups_held"     the groups K of the grouping held for the uploaded slice (bf_set_groups, bf_set_groups_from_segments,
 *                     bf_assign_groups with install); -1 when none is held.
 *   "tracks_held"     the groups Kp of the owner plane bf_track_keep kept; -1 when none is kept.  An upload does not change it.
 * BF_ERR_ARG for an unknown key. */
int bf_get_stat(bf_ctx *ctx, const char *key, int64_t *value);
#define BF_LOOP_ATOMIC 0      /* one global atomic per event and iteration, two plane buffers */
#define BF_LOOP_BINNED 1      /* the two-kernel tile-binned loop (slabs, lists or own pixels + margin plane) */
#define BF_LOOP_ONE_KERNEL 2  /* the one-kernel iteration */
#define BF_LOOP_PERSISTENT 3  /* ... as the persistent loop kernel (a run whose launch gave up reports the loop that finished it) */
#define BF_LOOP_DELTA 4       /* delta scatter */

/* ---- slice set-up -------------------------------------------------------------- */

/* AccelLib::init_gpu (accel_lib.h:71-115): stage one slice on the device.  Host
 * arrays are borrowed for the duration of the call.  noise may be NULL (no event
 * is noise, the state DVS_flow hands over).  Also resets the per-event warp state
 * (Event::reset, event.h:54-59: pr <- fr, n <- 0).  BF_ERR_STATE while asynchronous
 * uploads (bf_upload_events_async / bf_upload_ring_async) are pending: commit them first. */
int bf_upload_events(bf_ctx *ctx, const int32_t *fr_x, const int32_t *fr_y, const int32_t *t_ns,
                     const uint8_t *noise, int64_t n);

/* Same (accel_lib.h:71-115 without the blocking enqueueWriteBuffer calls of :109-115), but the three arrays are
 * DEVICE pointers (slice already resident in HBM). */
int bf_upload_events_device(bf_ctx *ctx, const int32_t *d_fr_x, const int32_t *d_fr_y,
                            const int32_t *d_t_ns, int64_t n);

/* Streaming front end (BASELINE config 3): stage the NEXT slice while the current one is being
 * optimised -- the reference uploads with blocking writes on its one queue (accel_lib.h:109-115, CL_TRUE) and
 * re-allocates its staging arrays per slice (:82-89).  bf_host_alloc returns pinned host memory; bf_upload_events_async copies a slice from
 * pinned arrays into one of two device staging slots on the ctx's COPY stream and returns at once
 * (the arrays must stay untouched until the matching bf_commit_upload returns);
 * bf_commit_upload makes the compute stream wait for the oldest pending copy and stages it
 * (== bf_upload_events without the blocking copy).  At most two uploads may be pending. */
int bf_host_alloc(bf_ctx *ctx, int64_t bytes, void **out);
int bf_host_free(bf_ctx *ctx, void *ptr);
int bf_upload_events_async(bf_ctx *ctx, const int32_t *fr_x, const int32_t *fr_y, const int32_t *t_ns,
                           int64_t n);
int bf_commit_upload(bf_ctx *ctx);

/* OptimizerRolling::set_cloud + set_scale (optimizer_rolling.h:248-283): bounding
 * box over fr (device reduction), window geometry, Event::reset for every event.
 * res_x / res_y seed x_min / y_min (:252).  scale must be odd (:274). */
int bf_set_cloud(bf_ctx *ctx, int32_t scale, int32_t res_x, int32_t res_y, bf_window *window_out);

/* ---- AccelLib operators -------------------------------------------------------- */

/* AccelLib::project_4param (accel_lib.h:275-281; Event::project_4param, event.h:88-96; project_dn, event.h:72-76): the
 * INCREMENTAL form -- dn from the previous pr as in the reinit form, ADDED to the event's (nx, ny), then apply_project.  The
 * reference's only call is commented out (optimizer_rolling.h:333-339); exported so that every member of SURVEY 8(b)'s
 * signature list exists.  (nx, ny) start at 0 after bf_set_cloud (Event::reset). */
int bf_project_4param(bf_ctx *ctx, double dnx_, double dny_, double cx, double cy, double div, double crl);

/* AccelLib::project_4param_reinit (accel_lib.h:263-267; Event::project_4param_reinit,
 * event.h:99-110; apply_project, event.h:164-168).  cos/sin of crl are evaluated on
 * the host with libm, as the reference does. */
int bf_project_4param_reinit(bf_ctx *ctx, double dnx_, double dny_, double cx, double cy,
                             double div, double crl);

/* AccelLib::get_time_img (accel_lib.h:211-217 -> get_time_img_cpu :147-178) for the
 * current window; x_sh / y_sh are (int)x_shift, (int)y_shift as at :147.  time_out
 * (R*C floats) and count_out (R*C uint32, the event-count image the reference keeps
 * local at :149) may each be NULL.  The time image stays resident for bf_fast_model. */
int bf_get_time_img(bf_ctx *ctx, float *time_out, uint32_t *count_out);

/* AccelLib::Sobel / Sobel_cpu (accel_lib.h:400-432,513-543) on a host image. */
int bf_sobel(bf_ctx *ctx, const float *img, int32_t rows, int32_t cols, float *grad_x,
             float *grad_y);

/* AccelLib::fast_model (accel_lib.h:337-341) = ObjectModel::update
 * (object_model.h:31-34; object_model.cpp:4-39,103-126).  img == NULL: use the time
 * image left on the device by the last bf_get_time_img.  Sets cx, cy, dx, dy, rot,
 * div, cnt of *model; totals are left untouched. */
int bf_fast_model(bf_ctx *ctx, const float *img, int32_t rows, int32_t cols, bf_model *model);

/* AccelLib::writeout_events (accel_lib.h:310-329): copy per-event state back.  Any
 * pointer may be NULL.  Arrays hold n doubles in upload order. */
int bf_writeout_events(bf_ctx *ctx, double *pr_x, double *pr_y, double *nx, double *ny);

/* Event::compute_uv (event.h:135-142) for every event, from the current nx, ny. */
int bf_compute_uv(bf_ctx *ctx, double *u, double *v);

/* ---- fused optimizer ----------------------------------------------------------- */

/* OptimizerRolling::set_model (optimizer_rolling.h:289-299): warm start ("STM",
 * dvs_flow.h:218-219).  model->cx, cy are SENSOR coordinates (:345-346). */
int bf_set_model(bf_ctx *ctx, const bf_model *model);

/* OptimizerRolling::run (optimizer_rolling.h:48-125) with iteration_step (:305-347)
 * executed entirely on the device: per iteration a warp+scatter kernel and a
 * stencil+moments kernel (the scalar model / loop update rides in one of them), no host round trip except a
 * poll of the `done` word every opts->poll_interval iterations.  The starting model is
 * the zero ObjectModel of a fresh optimizer (after bf_set_cloud) or what bf_set_model
 * was given; model_out receives get_model() (:285-287).  opts == NULL: defaults.
 * Returns info->rc.  When bf_run returns, the model and info are final; the last warp of the events (and, with want_uv, their
 * per-event flow) may still be executing on the context's stream -- everything that reads per-event results (bf_compute_uv,
 * bf_compute_uv_ring, bf_writeout_events, the renderers) and every later operation of the context runs on that stream, behind it.
 *
 * Tolerance contract.  The fused loop is NOT bit-identical to the reference's CPU path, and cannot be: (i) the time
 * image is the exact integer-nanosecond sum of a pixel's events rounded to f32 once, where the reference adds f32 seconds
 * event by event in container order (accel_lib.h:162) -- its own result moves by ~1e-7 relative with the event order;
 * (ii) the moments are centred sums reduced in a fixed tree, where object_model.cpp:22-30 adds per pixel in row-major
 * order; (iii) sin / cos of the rotation angle are evaluated on the device (Taylor polynomials for |x| <= 0.25, <= 1 ulp
 * from libm), where event.h:102-103 calls std::cos / std::sin -- bf_project_4param_reinit, the one-to-one operator,
 * evaluates them on the host with libm like the reference, so the two entry points can differ by that ulp.
 * What holds: the event-count image is bit-exact at fixed warp parameters; the time image agrees to 1e-6 relative, the
 * moments to 1e-9; a trajectory agrees with the CPU restatement to rounding until the first event crosses a pixel
 * boundary differently and within the restatement's own event-order spread afterwards; converged per-event flow
 * agrees to 1e-4 relative or 0.02 px/s, iteration counts to +-1 (tests/test_gpu_parity.py, tests/test_gpu_geometries.py
 * bound all of these at full size).  Every scatter / loop mode of this library gives the same bits as every other, and
 * every run is bit-reproducible (integer accumulators). */
int bf_run(bf_ctx *ctx, const bf_run_opts *opts, bf_model *model_out, bf_run_info *info);

/* A grid of independent optimizers over the staged slice (BASELINE config 4; the reference's
 * queue of (events, model) tasks, dvs_flow.h:200-231, with one task per sensor tile).  Events are
 * bucketed by tile (row = fr_x * grid_rows / sensor_res_x, column likewise); every tile gets its
 * own OptimizerRolling: set_cloud (bounding box seeded with sensor_res, optimizer_rolling.h:252),
 * cold start, run() with the guards evaluated against guard_res_x / guard_res_y / min_events (the
 * reference's RES / 15 and 1000 would skip every small tile).  One work-group per tile runs the
 * whole loop on chip.  Needs bf_upload_events first (not bf_set_cloud).  models_out / infos_out
 * hold grid_rows * grid_cols entries (row-major); infos[i].rc is 0, 1 (skipped) or < 0.
 * Afterwards bf_compute_uv / bf_writeout_events return the per-event results of all tiles.
 * Throughput over many slices: a grid's launch lasts as long as its slowest tile (thousands of
 * iterations, while the mean is ~90), so a caller keeps several contexts' grids in flight, one host
 * thread each -- and starts the process with GPU_MAX_HW_QUEUES=16 (the HIP runtime reads it once, at
 * its first call; default 4): with four hardware queues a fifth grid waits behind another grid's
 * straggler (measured, 32 x 32 tiles over 1M-event slices: 189 Mevents/s with 4 queues, 510 with 16
 * queues and 16 grids in flight). */
typedef struct bf_tile_opts {
    int32_t grid_rows, grid_cols;
    int32_t scale;
    int32_t sensor_res_x, sensor_res_y;
    int32_t guard_res_x, guard_res_y;
    int32_t min_events;
    int32_t max_iter;        /* <= 0: unlimited */
    int32_t hard_iter_cap;
} bf_tile_opts;
int bf_run_tiles(bf_ctx *ctx, const bf_tile_opts *opts, bf_model *models_out, bf_run_info *infos_out);

/* The tile grids of n slices in ONE launch: the reference's queue of (events, model) tasks (dvs_flow.h:200-231) holding the
 * tiles of several slices at once.  ctxs: n DISTINCT contexts of one device, each holding its own uploaded slice; opts: the
 * grid, shared by all.  One resident grid of work-groups on ctxs[0]'s stream claims (slice, tile) pairs from a device
 * counter -- slice by slice, a slice's tiles in index order -- so the straggler tiles of the first slices (a grid alone
 * lasts as long as its slowest tile: thousands of iterations against a mean of ~90) run under the bulk of the later ones.
 * No stream and no hardware queue per slice: the sustained rate does not depend on the host process's GPU_MAX_HW_QUEUES
 * (a grid per context in flight needs 16 queues to pass ~180 Mevents/s; the runtime's default is 4).  Every (slice, tile)
 * is the computation of bf_run_tiles -- the same bits.  models_out / infos_out: n * grid_rows * grid_cols entries, slice
 * major (either may be NULL).  Afterwards every context is in the state bf_run_tiles leaves it in (bf_compute_uv etc.
 * read its per-event results).  Blocking; returns the first error (its text on ctxs[0]). */
int bf_run_tiles_many(bf_ctx *const *ctxs, int32_t n, const bf_tile_opts *opts, bf_model *models_out, bf_run_info *infos_out);

/* ---- event groups: the queue of (events, model) tasks over ONE uploaded slice, solved in one launch ----
 *
 * A grouping is a group id per event and a group count: group_id[i] in -1 .. K-1, indexed in UPLOAD order; -1: the event
 * is in no group; K >= 0 groups.  For group g let E_g be its events in upload order.  The group's result is what the
 * reference leaves behind after, on E_g alone and in this order,
 *   1. OptimizerRolling::set_cloud(E_g, scale), its bounding box seeded with sensor_res_x / y as in bf_run_tiles;
 *   2. set_time (the times are already slice-local);
 *   3. set_model(warm_g) when a warm model is given (optimizer_rolling.h:289-299): one
 *      warp_reinit(-total_dx, -total_dy, cx, cy, total_div, -total_rot) from the reset state; the totals carry over;
 *   4. run() with the guards guard_res_x / y, min_events, max_iter, hard_iter_cap:
 * the model, the bf_run_info and (nx, ny) per event.  Afterwards bf_compute_uv / bf_writeout_events read, in upload order:
 * the group's final warp for an event of a group that ran; what set_model left -- (0, 0) cold -- for an event of a group a
 * guard skipped (BF_SKIPPED) or whose window does not fit the LDS (BF_ERR_CAPACITY in that group's rc; the reference
 * applies set_model before run() returns 1); (0, 0) for an event with id -1.  A group's result is a function of its event
 * set only (integer accumulators, as in the tile path): not of K, the other groups, the numbering or the storage order.
 *
 *   bf_set_groups                host ids.  An id outside -1 .. K-1: BF_ERR_ARG; K + 1 beyond the sort's 16384 buckets:
 *                                BF_ERR_CAPACITY; before an upload: BF_ERR_STATE.
 *   bf_set_groups_from_segments  the cl_id of the held segmentation, device to device, into the context's own group plane
 *                                (the grouping outlives the segmentation's invalidation); K = the kept components, also in
 *                                *groups_out.  BF_ERR_STATE when no segmentation of the current window is held (the rule
 *                                of bf_segment_get).
 *   bf_run_groups                warm_count 0: cold (warm may be NULL); 1: every group starts from warm[0]; K: one model per
 *                                group; anything else BF_ERR_ARG.  models_out / infos_out / groups_out: K entries each (any
 *                                may be NULL); groups_out is what the device found per group before solving.  A noise mask
 *                                is BF_ERR_ARG, as in bf_run_tiles.  K == 0 is BF_OK and every event reads (0, 0).  A group
 *                                whose rows * cols * 16 bytes exceed the LDS budget (156 KiB) gets BF_ERR_CAPACITY in its
 *                                own rc; the call still returns BF_OK and the other groups run.  The optimizers' LDS is
 *                                sized to the largest window that runs in THIS call (bf_get_stat "groups_lds",
 *                                "groups_per_cu").  Afterwards the context is in the state bf_run_tiles leaves it in.
 * The grouping holds until the next upload; bf_run_groups may be called again on it, e.g. with other warm models.
 * No membership policy is implied: which events form an object is the caller's decision.
 *
 * Wide groups (bf_set_option "groups_wide" = 1).  A group is WIDE when the guards do not skip it, its
 * rows * cols * 16 bytes exceed the LDS budget, and its window fits the context's own image capacity: rows <= max_rows and
 * cols <= max_cols of bf_create.  A wide group is solved in the same call on the chip-wide loop; a group beyond the image
 * capacity keeps BF_ERR_CAPACITY.  The result of a wide group g is what a FRESH context of the same capacity leaves after
 *   1. bf_upload_events(E_g);  2. bf_set_cloud(scale, sensor_res_x, sensor_res_y);  3. bf_set_model(warm_g) when the call is warm;
 *   4. bf_run with max_iter, min_events, res_x / res_y = guard_res_x / y and hard_iter_cap of the group options, everything
 *      else bf_run_opts_default:
 * the model; the bf_run_info (rc BF_OK or BF_ERR_NOCONV in the group's own rc while the call returns BF_OK, iterations, the
 * four dividers; the diagnostic counters are the inner run's); and per event of the group what bf_writeout_events and
 * bf_compute_uv read there.  Every loop form of bf_run gives the same bits from order-free integer accumulators, so this too
 * is a function of the event set alone.  An inner error that is not a run's own outcome (BF_ERR_HIP, ...) fails the whole call
 * with that code and the inner message.  groups_out[g].reserved is 1 for a group solved wide and 0 otherwise (always 0 with
 * the option off); bf_get_stat "groups_wide" counts them for the last call.  The wide groups run one after the other, longest
 * first, behind the LDS groups' launch, on an inner context the outer one owns (created at the first wide group, same device,
 * capacity and stream; released by bf_destroy; not a context of its own for "persist"'s "only context on its device").  The
 * context is left as by any bf_run_groups; the held grouping, a held flow of bf_hold_groups, the kept track plane, the vote
 * planes and the per-event best state are untouched. */
typedef struct bf_group_opts {            /* 32 bytes */
    int32_t scale;                        /* odd, scale/2 <= 4 */
    int32_t sensor_res_x, sensor_res_y;   /* seeds of set_cloud's bounding box */
    int32_t guard_res_x, guard_res_y;
    int32_t min_events;
    int32_t max_iter;                     /* <= 0: unlimited */
    int32_t hard_iter_cap;
} bf_group_opts;
typedef struct bf_group_info {            /* what the device found per group before solving */
    int32_t events, row_min, row_max, col_min, col_max, rows, cols, reserved;   /* fr bbox (set_cloud's, seeded); window R, C; reserved: 1 solved wide */
} bf_group_info;
int bf_set_groups(bf_ctx *ctx, const int32_t *group_id, int32_t groups);
int bf_set_groups_from_segments(bf_ctx *ctx, int32_t *groups_out);
int bf_run_groups(bf_ctx *ctx, const bf_group_opts *opts, const bf_model *warm, int32_t warm_count,
                  bf_model *models_out, bf_run_info *infos_out, bf_group_info *groups_out);

/* ---- event groups: assignment -- every event to the one of K competing models that explains it best ----
 *
 * The assignment step of motion segmentation by motion compensation (Mitrokhin et al. 2018, Stoffregen et al. 2019): given
 * K candidate models, an event goes to the model under which it lands on the largest pile of OTHER events.  It produces the
 * membership bf_run_groups solves; alternating the two grows a seed to an object's whole event set.
 * Everything after an event's pixel is an integer count, a maximum or a smallest index: the result does not depend on the
 * order events are stored or work-groups run in.
 *
 *   window    OptimizerRolling::set_cloud's window (optimizer_rolling.h:248-283) for a bounding box that is the whole sensor
 *             widened by `margin`: x_min = -margin, x_max = sensor_res_x - 1 + margin, columns likewise.  It does not depend
 *             on the events.  With s = scale: wsx = s (x_max - x_min) (:263), R = wsx + s (:276), x_shift by :279-280, and
 *             the integer x_sh = (int)x_shift (the parameter conversion of accel_lib.h:147); wsy, C, y_sh likewise.
 *   pixel_k(i)  from the reset state (Event::reset: pr = fr) ONE warp_reinit(-total_dx, -total_dy, cx, cy, total_div,
 *             -total_rot) of models[k] (set_model's warp, optimizer_rolling.h:289-299; cx, cy in sensor coordinates; sine
 *             and cosine from the host's libm, as in bf_set_model); per event project_4param_reinit + apply_project
 *             (event.h:99-110,164-168); then X = trunc(pr_x s + x_sh), Y = trunc(pr_y s + y_sh) (accel_lib.h:154-155).
 *             The event is OUTSIDE under k when X >= wsx + s/2 || X < s/2 || Y >= wsy + s/2 || Y < s/2 (accel_lib.h:157).
 *   votes     event i votes under k when it is inside under k and use_prior == 0, or its prior id is k, or its prior id is
 *             -1.  V_k[X, Y] = the number of votes; B_k = the s x s box sum of V_k (the count image of the splat,
 *             accel_lib.h:160-165, gathered).  The prior is the grouping the context holds (bf_set_groups, or an earlier call with install).
 *   score     S_k(i) = B_k[pixel_k(i)] - (1 if i voted under k else 0): leave-one-out; 0 when i is outside under k.
 *   result    best = max_k S_k(i); group_id_out[i] = the smallest k with S_k(i) == best, or -1 when best < min_score;
 *             score_out[i] = best; counts_out[k] = events given k, counts_out[K] = events given -1.  info: models = K,
 *             rows = R, cols = C, assigned, unassigned, changed = events whose id differs from the prior (use_prior == 0:
 *             from -1), max_score = the largest best.  All per-event outputs are in UPLOAD order; any output may be NULL.
 *   state     reads the events' addresses and times only; products, (nx, ny), the time image, a held segmentation, a held
 *             flow and the read-back validity are untouched, and the bytes are the same whether the events are stored in
 *             upload order or sorted (after bf_run_tiles / bf_run_groups).  install == 1: the result becomes the context's
 *             grouping, K groups, as after bf_set_groups (it holds until the next upload); install == 0: the held grouping
 *             is unchanged.
 *   errors    BF_ERR_STATE before an upload, or use_prior without a held grouping; BF_ERR_ARG for an even or too large
 *             scale, a sensor side < 1 or > 65536, a margin < 0 or > 65536, min_score < 1, n_models < 1 or > 64, a NULL
 *             opts or models, a prior whose group count differs from n_models, a noise mask (as bf_run_groups);
 *             BF_ERR_CAPACITY when K R C > 2^27.  Zero events: BF_OK, every output zero (info too).
 * Blocking.  Where candidate models come from is the caller's decision. */
typedef struct bf_assign_opts {        /* 32 bytes */
    int32_t scale;                     /* odd, scale/2 <= 4 */
    int32_t sensor_res_x, sensor_res_y;
    int32_t margin;                    /* >= 0 sensor pixels added on every side of the sensor box */
    int32_t min_score;                 /* >= 1 */
    int32_t use_prior;                 /* 0: every event votes under every model; 1: the held grouping is the prior */
    int32_t install;                   /* 1: the result becomes the context's grouping (K groups) for bf_run_groups */
    int32_t reserved;
} bf_assign_opts;
typedef struct bf_assign_info {        /* 32 bytes */
    int32_t models, rows, cols, assigned, unassigned, changed, max_score, reserved;
} bf_assign_info;
int bf_assign_groups(bf_ctx *ctx, const bf_assign_opts *opts, const bf_model *models, int32_t n_models,
                     int32_t *group_id_out, int32_t *score_out, int32_t *counts_out /* K + 1, last = unassigned */,
                     bf_assign_info *info);

/* ---- event groups: projection -- the slice with every event warped by its own group's model, as an image and a score ----
 *
 * The picture and the objective of motion segmentation by motion compensation: the image in which every object is sharpened
 * by its own model, coloured by object, and its contrast sum N^2 -- the number that says whether one grouping under K models
 * explains the slice better than another.  Everything after an event's pixel is an integer count, a sum,
 * a maximum or a smallest index: the bytes do not depend on the order events are stored or work-groups run in.
 *
 *   grouping  the one the context holds (bf_set_groups, bf_set_groups_from_segments, or bf_assign_groups with install): ids
 *             -1 .. K-1 in upload order.  n_models must equal K; event i of group k is projected under models[k].
 *   window    exactly bf_assign_groups': the whole sensor widened by `margin`; R, C, wsx, wsy, x_sh, y_sh as there.
 *   pixel_k(i)  exactly bf_assign_groups': ONE set_model warp of models[k] from the reset state, sine and cosine from the
 *             host's libm, the scatter kernel's truncation and window test.
 *   planes    V_k[p] = the number of events with id k that are inside under model k at p; B_k = the s x s box sum of V_k,
 *             zero beyond the plane; at scale 1 B_k = V_k.
 *   counts    an event with id -1 is in no plane and counts in info.unassigned; an event of group k that is outside under
 *             model k counts in info.outside (and is scores[k].events - scores[k].inside).
 *   pixel     count_out[p] = N[p] = sum_k B_k[p];  label_out[p] = the smallest k with the largest B_k[p], -1 where N[p] == 0;
 *             bgr_out[3 p + c] = BF_PROJECT_PALETTE[label % 12][c] * min(255, B_label[p] * gain) / 255 (integer division; the
 *             product B * gain in 64 bits), 0 where the label is -1.  p = X * C + Y, planes of R x C.
 *   group     scores_out[k]: events (with id k), inside, pixels_hit = #{p: B_k[p] > 0}, pixels_owned = #{p: label[p] == k},
 *             max = max_p B_k[p], sum_sq = sum_p B_k[p]^2.
 *   info      models = K, rows = R, cols = C, unassigned, outside, pixels = #{p: N[p] > 0}, sum = sum_p N[p] (= s^2 times
 *             the inside events less what the box sums lose beyond the plane's edge), sum_sq = sum_p N[p]^2.
 *   overflow  the uint64 sums wrap by definition.  sum_sq <= sum^2 <= (s^2 n)^2 with s <= 9: none can wrap, and no 32-bit
 *             count or box sum either, while the slice has fewer than 2^32 / 81 = 53 024 287 events.
 *   state     reads the events' addresses and times, the permutation and the held grouping only; products, (nx, ny), the
 *             time image, a held segmentation, a held flow, the per-event best state, the held grouping and the read-back
 *             validity are untouched.  The vote planes are bf_assign_groups' (each call of either clears them first).
 *   errors    BF_ERR_STATE before an upload, or with no held grouping; BF_ERR_ARG for an even or too large scale, a sensor
 *             side < 1 or > 65536, a margin < 0 or > 65536, gain < 1, n_models < 1 or > 64 or different from the held K,
 *             a NULL opts or models, a noise mask; BF_ERR_CAPACITY when K R C > 2^27.  Zero events: BF_OK, scores and info
 *             zero (rows and cols too), count and bgr zero over the R x C window and every label -1 (N == 0 everywhere).
 * Any output may be NULL.  Blocking. */
#define BF_PROJECT_PALETTE_SIZE 12
#define BF_PROJECT_PALETTE /* B, G, R */ \
    {{255, 255, 255}, {0, 0, 255}, {0, 255, 0}, {255, 0, 0}, {0, 255, 255}, {255, 0, 255}, {255, 255, 0}, {0, 128, 255}, \
     {255, 128, 0}, {128, 0, 255}, {0, 255, 128}, {128, 128, 255}}
typedef struct bf_project_opts {       /* 32 bytes */
    int32_t scale;                     /* odd, scale/2 <= 4 */
    int32_t sensor_res_x, sensor_res_y;
    int32_t margin;                    /* >= 0 sensor pixels added on every side of the sensor box */
    int32_t gain;                      /* >= 1: a box sum of 255 / gain or more saturates the colour */
    int32_t reserved[3];
} bf_project_opts;
typedef struct bf_group_score {        /* 32 bytes */
    int32_t events, inside, pixels_hit, pixels_owned, max, reserved;
    uint64_t sum_sq;
} bf_group_score;
typedef struct bf_project_info {       /* 48 bytes */
    int32_t models, rows, cols, unassigned, outside, pixels;
    uint64_t sum, sum_sq;
    int32_t reserved[2];
} bf_project_info;
int bf_project_groups(bf_ctx *ctx, const bf_project_opts *opts, const bf_model *models, int32_t n_models,
                      uint32_t *count_out /* R x C */, int32_t *label_out /* R x C */, uint8_t *bgr_out /* R x C x 3 */,
                      bf_group_score *scores_out /* K */, bf_project_info *info);

/* ---- event groups: merge gains -- how much of a group's contrast survives under another group's model ----
 *
 * The last decision of the object pipeline: which groups are one motion, and with it the number of objects.  For every ordered
 * pair (b, a) of groups it gives the exact change of bf_project_groups' objective, info.sum_sq, under the merge "group b adopts
 * model a" (DESIGN section 18).  Everything after an event's pixel is an integer count or a sum: the bytes do not depend on
 * the order events are stored or work-groups run in, and no tolerance is involved.
 *
 *   grouping  exactly bf_project_groups': the held grouping, ids -1 .. K-1 in upload order; n_models must equal K.
 *   window    exactly bf_project_groups': the whole sensor widened by `margin`.
 *   pixel_k(i)  exactly bf_assign_groups'.
 *   trial     T[b][a][p] = the s x s box sum (zero beyond the plane; at scale 1 the plane itself) of the events with id b that
 *             are inside under MODEL a at p.
 *   base      B_b = T[b][b]: bf_project_groups' planes.  N[p] = sum_k B_k[p].
 *   unassigned  an event with id -1 is in no plane and counts in info.unassigned.
 *   gain      gain_out[b * K + a] = sum_p T[b][a][p] * (2 * (N[p] - B_b[p]) + T[b][a][p]), as uint64.
 *   reading   gain[b][b] is what the objective loses when the events of b are deleted; gain[b][a] is what they add back under
 *             model a: after "b adopts model a" the objective is S - gain[b][b] + gain[b][a], S = info.sum_sq.
 *   inside    inside_out[b * K + a] = the events of b that are inside under model a.
 *   events    events_out[b] = the events with id b.
 *   info      models = K, rows = R, cols = C, unassigned, passes (below), sum = sum_p N[p], sum_sq = S = sum_p N[p]^2.
 *   overflow  the uint64 sums wrap by definition.  A gain is at most the objective after its merge, which is <= (s^2 n)^2 with
 *             s <= 9: none can wrap while the slice has fewer than 2^32 / 81 = 53 024 287 events (bf_project_groups' bound).
 *   passes    one pass holds the trial planes of A = min(K, targets_per_pass or K, floor(2^27 / (K R C))) target models;
 *             info.passes = ceil(K / A).  The result does not depend on A.
 *   state     exactly bf_project_groups' list: reads the events' addresses and times, the permutation and the held grouping
 *             only; nothing of the context's state is written.  The base planes are bf_assign_groups' (each call of the three
 *             entries clears them first); the trial planes are buffers of their own.
 *   errors    those of bf_project_groups (without gain); BF_ERR_ARG for targets_per_pass < 0; BF_ERR_CAPACITY when
 *             K R C > 2^27.  Zero events: BF_OK, every output zero (info too).
 * Any output may be NULL.  Blocking.  Which pair to merge is the caller's policy (bf::ObjectMerger, object_merge.h). */
typedef struct bf_merge_opts {         /* 32 bytes */
    int32_t scale;                     /* odd, scale/2 <= 4 */
    int32_t sensor_res_x, sensor_res_y;
    int32_t margin;                    /* >= 0 sensor pixels added on every side of the sensor box */
    int32_t targets_per_pass;          /* 0: as many target models per launch as fit; >= 1: at most that many */
    int32_t reserved[3];
} bf_merge_opts;
typedef struct bf_merge_info {         /* 48 bytes */
    int32_t models, rows, cols, unassigned, passes, reserved0;
    uint64_t sum, sum_sq;
    int32_t reserved[2];
} bf_merge_info;
int bf_merge_scores(bf_ctx *ctx, const bf_merge_opts *opts, const bf_model *models, int32_t n_models,
                    uint64_t *gain_out /* K x K, [b * K + a] */, int32_t *inside_out /* K x K */,
                    int32_t *events_out /* K */, bf_merge_info *info);

/* ---- event groups: tracks -- which object of the previous slice is which object of this one ----
 *
 * The object pipeline numbers the groups of every slice anew.  To carry an identity from slice to slice, the owner plane of one
 * slice's final grouping is KEPT on the device across the next upload, and the next slice's groups are counted against it: per
 * group, on whose pixels its events land once they are carried back by the time between the two slices.
 * Everything after an event's pixel is an integer count: the bytes do not depend on the order events are stored or work-groups
 * run in.
 *
 * bf_track_keep
 *   plane     R x C words: exactly bf_project_groups' label_out for the held grouping under `models` -- its window (the whole
 *             sensor widened by `margin`), pixel_k(i), box sums B_k, label = the smallest k with the largest B_k[p], -1 where
 *             N[p] == 0 -- and equal to it byte for byte on the same context.  plane_out may be NULL.
 *   kept      the plane, Kp = K = n_models, and the window's options (scale, sensor sides, margin), in a buffer of the plane's
 *             own.  It is NOT slice state: it survives bf_upload_events (that is its purpose), bf_set_cloud,
 *             bf_global_set_window, every run, bf_segment, bf_set_groups and bf_assign_groups.  The next bf_track_keep replaces
 *             it; bf_track_drop and bf_destroy release it.  bf_get_stat "tracks_held" gives Kp, -1 without a plane.
 *   info      models = kept_models = K, rows = R, cols = C, unassigned (ids of -1), outside (events outside under their own
 *             model).
 *   state     writes nothing else: bf_project_groups' untouched list (the vote planes are shared and cleared, as there).
 *   errors    exactly bf_project_groups', without gain.  A refused call leaves the previous plane as it was.  Zero events:
 *             BF_OK, a kept plane of all -1 over the R x C window, info zero.
 * bf_track_overlap
 *   needs     a held grouping of K == n_models groups on the slice uploaded now, and a kept plane of the same window options.
 *   dt_ns     the time origin of the slice uploaded now minus the kept slice's, in ns (the absolute times both slices' local
 *             times were taken from); it may be negative; |dt_ns| <= 2^40.
 *   pixel_k(i; dt)  exactly bf_assign_groups' pixel_k(i) -- ONE set_model warp of models[k] from the reset state, sine and cosine
 *             from the host's libm, the scatter kernel's truncation, the window test -- with one change: the event's time
 *             operand float(t_i) is the f32 nearest (ties to even) to the 64-bit integer t_i + dt_ns.  The event is carried
 *             back, under its own model, to where it was in the kept slice's frame.  dt_ns = 0 gives bf_project_groups' pixel.
 *   overlap   overlap_out[k * (Kp + 1) + j] = the events with id k that are inside and land on a pixel whose kept label is j;
 *             j == Kp: on a pixel whose kept label is -1.  inside_out[k] = the row's sum.
 *   info      models = K, kept_models = Kp, rows, cols, outside = the events of any group that are outside under their own model
 *             and dt, unassigned = the events with id -1.
 *   state     reads the events' addresses and times, the permutation, the held grouping and the kept plane; writes nothing of
 *             the context's state and does not use the vote planes.
 *   errors    BF_ERR_STATE before an upload, with no held grouping, or with no kept plane; BF_ERR_ARG for n_models < 1 or > 64
 *             or different from the held K, NULL opts or models, a noise mask, options that differ from the kept plane's,
 *             |dt_ns| > 2^40.  Zero events: BF_OK, every output zero (info too).
 * All 32-bit counts.  Any output may be NULL.  Blocking.  Which group continues which track is the caller's policy
 * (bf::ObjectTracker::match, object_tracker.h). */
typedef struct bf_track_opts {         /* 32 bytes */
    int32_t scale;                     /* odd, scale/2 <= 4 */
    int32_t sensor_res_x, sensor_res_y;
    int32_t margin;                    /* >= 0 sensor pixels added on every side of the sensor box */
    int32_t reserved[4];
} bf_track_opts;
typedef struct bf_track_info {         /* 32 bytes */
    int32_t models, kept_models, rows, cols, unassigned, outside;
    int32_t reserved[2];
} bf_track_info;
int bf_track_keep(bf_ctx *ctx, const bf_track_opts *opts, const bf_model *models, int32_t n_models,
                  int32_t *plane_out /* R x C */, bf_track_info *info);
int bf_track_overlap(bf_ctx *ctx, const bf_track_opts *opts, const bf_model *models, int32_t n_models, int64_t dt_ns,
                     int32_t *overlap_out /* K x (Kp + 1), [k * (Kp + 1) + j] */, int32_t *inside_out /* K */,
                     bf_track_info *info);
int bf_track_drop(bf_ctx *ctx);

/* A batch of independent slices -- the reference's queue of (events, model) tasks (dvs_flow.h:200-231, executed there
 * one after the other) -- solved together: bf_run on each of the n contexts, all in flight at once (one host thread per
 * context inside the library; the contexts' streams share the GPU, set "co_schedule" on them when n > 1).  Every
 * context must hold its own slice (upload + bf_set_cloud [+ bf_set_model]).  models_out / infos_out: n entries (either
 * may be NULL); infos_out[i].rc is that slice's return code.  Returns BF_OK when every slice returned 0 or 1, else the
 * first error code (the text is on that context: bf_last_error).  For slices spread over several GPUs and for streams
 * of slices, see better_flow/slice_farm.h, which drives the same entry points. */
int bf_run_many(bf_ctx *const *ctxs, int32_t n, const bf_run_opts *opts, bf_model *models_out, bf_run_info *infos_out);

/* Records of the last bf_run (opts->trace_cap > 0): model and dividers after every iteration_step -- what the
 * reference prints under VERBOSE (optimizer_rolling.h:116-118) or shows in manual() (:212).  Returns the number written. */
int bf_get_trace(bf_ctx *ctx, bf_trace_rec *out, int32_t cap, int32_t *written);

/* ---- raw device buffers ----------------------------------------------------------- */

/* EventFile::projection_img(events, scale, show_final) (event_file.h:460-515): the 8-bit image of the
 * non-noise events on the full sensor, (res_x * scale) x (res_y * scale) -- at their current projected
 * positions pr (the motion-compensated image once bf_run has converged) or, with show_final != 0, at their
 * sensor positions.  Saturating count, this build's 8-bit Gaussian for scale > 1 (see above; the reference's
 * cv::GaussianBlur is unpinned), brightness normalised to a non-zero mean of 127 (cv::convertScaleAbs:
 * round-half-even of the float product, saturated).  img_out: host buffer of that many bytes. */
int bf_projection_img(bf_ctx *ctx, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final,
                      uint8_t *img_out);

/* EventFile::color_time_img(events, scale, show_final) (event_file.h:649-747): the colour-coded time image of
 * the non-noise events on the full sensor, (res_x * scale + scale) x (res_y * scale + scale) pixels of B, G, R
 * bytes (3 bytes per pixel, row-major).  Every event adds (1, cos a, sin a) to the scale x scale pixels it
 * covers, a = float(2 * 3.14 * (t - t_min) / (t_max - t_min)) with t_min = min t and t_max = max(0, max t)
 * (:659-662; a = 0 when they are equal -- the reference divides 0 by 0 there).  Per covered pixel: hue =
 * uchar((atan2(mean sin, mean cos) + 3.1416) * 180 / 3.1416 / 2), saturation = uchar(255 * |mean|), value = 255
 * (:712-723); uncovered pixels are black.  Positions are pr (compensated) or, with show_final != 0, the sensor
 * coordinates (:684-687).  scale = 0 means 11 (:650).
 * Two things are this build's own, both stated here: (i) the reference adds the f32 cos / sin in event order,
 * this build adds them as 2^-32 fixed point integers, so the image does not depend on event order and agrees
 * with the f32 sums to their own rounding error (~1e-7) before the 8-bit quantisation; (ii) HSV -> BGR follows the 8-bit convention of
 * cv::cvtColor (H in [0, 180), S and V in [0, 255]) in float32: h = H * (6 / 180), sector = floor(h), f = h -
 * sector, s = S / 255, v = V / 255, p = v (1 - s), q = v (1 - s f), t = v (1 - s (1 - f)), (r, g, b) = (v,t,p),
 * (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q) for sectors 0..5, each channel rint(255 x) -- the reference's
 * cv::cvtColor comes from an un-versioned OpenCV (parity unpinned for that stage). */
int bf_color_time_img(bf_ctx *ctx, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final,
                      uint8_t *bgr_out);

/* The slice hand-off of DVS_flow::recompute (dvs_flow.h:185-216) for a structure-of-arrays event ring kept
 * in pinned memory (bf_host_alloc) -- no AoS -> SoA repack (accel_lib.h:91-99) and no per-slice allocation on
 * the host.  The slice is the n events starting at ring index `first` (wrapping at `cap`), stored oldest ->
 * newest; Event::set_local_time(t0) (event.h:61-63) is applied on the device.  ring_noise (may be NULL: no event
 * is noise) is the ring of Event::noise flags -- the reference sets them for every event of a slice that its
 * small-window guard rejects (optimizer_rolling.h:49-55) and get_time_img leaves flagged events out of later,
 * overlapping slices (accel_lib.h:152).  Asynchronous like bf_upload_events_async (same two staging slots;
 * bf_commit_upload makes the slice current).  The ring slots may be overwritten once bf_wait_uploads has
 * returned. */
int bf_upload_ring_async(bf_ctx *ctx, const int32_t *ring_fr_x, const int32_t *ring_fr_y,
                         const uint64_t *ring_timestamp_ns, const uint8_t *ring_noise, int64_t cap,
                         int64_t first, int64_t n, uint64_t t0_ns);

/* The same hand-off for a ring with 16-bit addresses: 12 bytes per event over the link instead of 16, and the
 * column layout of the binary event file (better_flow/event_reader.h: u64 t_ns[], u16 x[] = column, u16 y[] = row),
 * so that a file block read into the ring is uploaded as it lies.  ring_row = Event::fr_x, ring_col = Event::fr_y. */
int bf_upload_ring16_async(bf_ctx *ctx, const uint16_t *ring_row, const uint16_t *ring_col,
                           const uint64_t *ring_timestamp_ns, const uint8_t *ring_noise, int64_t cap,
                           int64_t first, int64_t n, uint64_t t0_ns);

/* ... and with 32-bit timestamps: 8 bytes per event over the link instead of 12 -- a warm-started stream (a handful of
 * iterations per slice) is bound by that link: 1M-event slices from pinned memory at 47-51 GB/s are 0.25 ms of copy against
 * 0.1-0.2 ms of solve.  ring_t32[i] holds the LOW 32 bits of event i's nanosecond timestamp; t0_ns is the slice start in full.
 * The device forms Event::set_local_time (event.h:61-63) as (int32)(ring_t32[i] - (uint32)t0_ns), which is the exact
 * difference while |timestamp - t0_ns| < 2^31 ns = 2.1 s (the caller's contract: a slice is at most SPAN long, dvs_flow.h:21,156 -- 0.2 s in the
 * command line, bf_motion_compensator.cpp:7,135; the 64-bit forms report a time that does not fit through bf_set_cloud, this one cannot). */
int bf_upload_ring16t32_async(bf_ctx *ctx, const uint16_t *ring_row, const uint16_t *ring_col,
                              const uint32_t *ring_t32, const uint8_t *ring_noise, int64_t cap,
                              int64_t first, int64_t n, uint64_t t0_ns);
/* bf_upload_events_async for a slice whose addresses are held as 16-bit values (AccelLib::init_gpu's int fr_x, fr_y, t,
 * accel_lib.h:83-85,101-103, with the two addresses narrowed: a sensor address fits 16 bits): 8 bytes per event. */
int bf_upload_events16_async(bf_ctx *ctx, const uint16_t *fr_x, const uint16_t *fr_y, const int32_t *t_ns,
                             int64_t n);

/* Event::compute_uv (event.h:135-142) of the current slice written straight into a ring of interleaved (u, v)
 * pairs: event i of the slice goes to uv_ring[2 * ((first + i) % cap)] and [... + 1].  No intermediate host copy:
 * with a pinned ring this is one or two DMA transfers.  Blocks until the data has arrived. */
int bf_compute_uv_ring(bf_ctx *ctx, double *uv_ring, int64_t cap, int64_t first);

/* Block until the host-to-device copies of every pending asynchronous upload have finished. */
int bf_wait_uploads(bf_ctx *ctx);

/* ---- contrast-score optimiser: OptimizerLocal (optimizer_sampler.h:12-68) ------------------
 * The secondary score of the path: saturating 8-bit event-count image, Gaussian blur, mean of
 * the non-zero pixels, coordinate descent on (nx, ny).  The blur is this build's own stated
 * 8-bit Gaussian (binomial taps {1,2,1}/4, {1,4,6,4,1}/16, {2,7,14,18,14,7,2}/64 for
 * scale 3 / 5 / 7, BORDER_REFLECT_101, exact integer sum, one rounding half up): the
 * reference calls cv::GaussianBlur of an unpinned OpenCV, so parity is unpinned there. */
typedef struct bf_local_window {
    int32_t scale;
    int32_t metric_wsizex, metric_wsizey;   /* optimizer_sampler.h:31-32,43-44 */
    int32_t scale_img_x, scale_img_y;       /* optimizer_sampler.cpp:208-209 */
    int32_t c_fr_x, c_fr_y;                 /* event_c, the window centre (optimizer_sampler.h:30,46) */
    int32_t pad_;
    int64_t c_t;                            /* event_c.t */
} bf_local_window;

typedef struct bf_local_state {
    double nx, ny, last_score, dnx, dny, dn_th;   /* optimizer_sampler.h:26-28 */
    int64_t evaluations;                          /* iteration_step calls */
} bf_local_state;

/* The two constructors (optimizer_sampler.h:29-48) + update_fields (optimizer_sampler.cpp:205-212).
 * wsz <= 0: OptimizerLocal(events, scale) -- window = bounding box of the uploaded cloud, centre
 * event in its middle with t = 0 (c_fr_x, c_fr_y, c_t are ignored).  wsz > 0:
 * OptimizerLocal(events, e, scale, wsz) with e = (c_fr_x, c_fr_y, c_t).  scale odd, <= 7. */
int bf_local_set_window(bf_ctx *ctx, int32_t scale, int32_t wsz, int32_t c_fr_x, int32_t c_fr_y,
                        int64_t c_t, bf_local_window *window_out);

/* OptimizerLocal::iteration_step (optimizer_sampler.cpp:120-153): Event::project(nx, ny) of every
 * event, count image, blur, score.  img_out (optional, host, scale_img_x * scale_img_y bytes)
 * receives project_img.  Does not touch the rolling optimizer's per-event state. */
int bf_local_iteration_step(bf_ctx *ctx, double nx, double ny, double *score, uint8_t *img_out);

/* OptimizerLocal::run (optimizer_sampler.cpp:4-38).  Returns BF_OK, BF_SKIPPED (window guard,
 * :9-13, with the sensor size res_x x res_y) or BF_ERR_NOCONV when max_evaluations (> 0) is
 * reached (the reference has no cap). */
int bf_local_run(bf_ctx *ctx, int32_t res_x, int32_t res_y, int64_t max_evaluations, bf_local_state *out);

/* A GRID of OptimizerLocal windows over the uploaded slice -- SURVEY f1's formulation of BASELINE config 4 (per-tile local flow):
 * the sensor is cut into grid_rows x grid_cols tiles (an event belongs to tile (fr_x * grid_rows / sensor_res_x, fr_y *
 * grid_cols / sensor_res_y), as in bf_run_tiles); every tile gets OptimizerLocal(events of the tile, e, scale, wsz)
 * (optimizer_sampler.h:31-34) with the centre event e = (middle row of the tile, middle column of the tile, t = 0) -- "middle"
 * = (first + last) / 2 of the tile's rows / columns, integer division -- and its run() (optimizer_sampler.cpp:4-38): coordinate
 * descent on (nx, ny) for the largest contrast score.  One work-group per window runs the whole descent on chip.  The window
 * guard (:9-13) uses guard_res_x / guard_res_y as RES; max_evaluations > 0 caps a window's iteration_step calls (checked after
 * each ny step, as bf_local_run does).  states_out / rc_out: grid_rows * grid_cols entries (either may be NULL); rc_out[k] is 0,
 * BF_SKIPPED or BF_ERR_NOCONV.  The blur is this build's stated 8-bit Gaussian (above).  Afterwards the slice's events are
 * sorted by tile (as after bf_run_tiles) and hold no per-event result. */
typedef struct bf_local_tile_opts {
    int32_t grid_rows, grid_cols;
    int32_t scale;                        /* odd, <= 7 */
    int32_t wsz;                          /* window side in sensor pixels: metric_wsize = scale * wsz (optimizer_sampler.h:32) */
    int32_t sensor_res_x, sensor_res_y;   /* sensor rows / columns */
    int32_t guard_res_x, guard_res_y;     /* RES_X / RES_Y of the window guard */
    int64_t max_evaluations;              /* <= 0: unlimited */
} bf_local_tile_opts;
int bf_local_run_tiles(bf_ctx *ctx, const bf_local_tile_opts *opts, bf_local_state *states_out, int32_t *rc_out);

/* ---- exhaustive search: OptimizerGlobal (optimizer_global.h:11-57, optimizer_global.cpp) ----------
 * A sweep over a grid of (nx, ny) candidates that scores every event's neighbourhood under each one: for every
 * candidate, Event::project of every event, the saturating scale x scale splat into the bordered 8-bit image, this build's
 * stated 8-bit Gaussian (above: binomial taps, BORDER_REFLECT_101, exact integer sum, one rounding; NOT pinned to any
 * OpenCV -- the reference calls cv::GaussianBlur), and per accepted event the mean of the NON-ZERO blurred pixels in the
 * metric_wsize^2 window centred on it (get_event_score, :82-101).  apply_score (event.h:113-121) then folds that score
 * into the event's running best, strict `>`, in candidate order.  Two definitions of this build ("OptimizerGlobal"):
 *   - the per-event result is the winning candidate (best_nx, best_ny); best_u / best_v are Event::compute_uv of it
 *     (event.h:135-142) -- the reference copies a u / v that apply_project never updates;
 *   - the objective of candidate k is S(k) = sum over the events accepted under k of floor(score * 2^32), an exact int64
 *     (computed as (sum << 32) / count); the slice's best candidate is the first in sweep order (nx outer, ny inner) with
 *     the largest S (candidate 0 when every S is 0).
 * Every result is bit-reproducible: integers and single IEEE operations only.  scale in {1, 3, 5, 7}; metric_wsize odd,
 * 1..63.  Scratch is sized from the window (two 32-bit planes of the bordered image per candidate of a batch), not from
 * bf_create's max_rows / max_cols.  The uploaded events are not moved (their projected positions are untouched). */
typedef struct bf_global_window {       /* optimizer_global.cpp:187-205 */
    int32_t scale, metric_wsize;
    int32_t x_min, y_min, x_max, y_max; /* bounding box of fr_x / fr_y (empty cloud: 0, 0, -1, -1) */
    int32_t scale_img_x, scale_img_y, scale_bordered_img_x, scale_bordered_img_y;
} bf_global_window;

typedef struct bf_global_search_opts {  /* optimizer_global.cpp:106-108 */
    double x_low, x_hi, x_step, y_low, y_hi, y_step, nz;
} bf_global_search_opts;

typedef struct bf_global_result {
    double best_nx, best_ny;   /* first candidate in sweep order with the largest S */
    int64_t best_sum;          /* S(best) */
    int64_t n_x, n_y;          /* candidates swept (180 x 80 for the defaults) */
} bf_global_result;

/* The reference's defaults: x in [-0.09, 0.09), y in [-0.04, 0.04), step 0.001, nz = NZ = 127. */
void bf_global_search_opts_default(bf_global_search_opts *o);

/* The constructors (optimizer_global.h:27-41) + update_fields over the uploaded cloud.  metric_wsize <= 0: 5 * scale.
 * Resets every event's best state (max_score = 0, best (nx, ny) = 0, best_pr = fr).  BF_ERR_ARG for a scale outside
 * {1, 3, 5, 7} or an even / out-of-range metric_wsize; BF_ERR_STATE before bf_upload_events. */
int bf_global_set_window(bf_ctx *ctx, int32_t scale, int32_t metric_wsize, bf_global_window *out);

/* One project_all (optimizer_global.cpp:4-79), folding into the per-event state like the reference.  Any output may be
 * NULL: img_out (scale_bordered_img_x * scale_bordered_img_y bytes) the blurred bordered image; scores_out (float,
 * scale_img_x * scale_img_y) current_scores; sum_out S.  BF_ERR_ARG without a window; BF_ERR_STATE when any upload (of
 * any size, synchronous or committed asynchronous) happened since bf_global_set_window -- the same for bf_global_search and
 * bf_global_get_events. */
int bf_global_project_all(bf_ctx *ctx, double nx, double ny, double nz, uint8_t *img_out, float *scores_out, int64_t *sum_out);

/* compute_flow_bruteforce (optimizer_global.cpp:104-150) over the grid of opts (NULL: the defaults), continuing from the
 * current per-event state.  The host builds the candidate values by the reference's repeated double addition (for (v = lo;
 * v < hi; v += step)).  surface_out (may be NULL) receives S of every candidate, row-major [n_x][n_y]; surface_cap is its
 * length.  BF_ERR_ARG for a step <= 0, lo >= hi, nz <= 0, a surface buffer shorter than n_x * n_y, more than 2^26
 * candidates, or no window. */
int bf_global_search(bf_ctx *ctx, const bf_global_search_opts *opts, bf_global_result *out, int64_t *surface_out,
                     int64_t surface_cap);

/* Per-event state in upload order (n doubles each); any pointer may be NULL.  best_u / best_v: Event::compute_uv of the
 * event's winning candidate (0 for an event never accepted). */
int bf_global_get_events(bf_ctx *ctx, double *max_score, double *best_nx, double *best_ny, double *best_pr_x,
                         double *best_pr_y, double *best_u, double *best_v);

/* The objective per region of the sensor: a third definition of this build ("OptimizerGlobal").
 *   - The grid.  Cells of cell_rows x cell_cols sensor pixels, anchored at sensor pixel (0, 0) -- not at the cloud's
 *     bounding box -- so a cell means the same pixels in every slice.  n_cell_x = ceil(res_x / cell_rows), n_cell_y =
 *     ceil(res_y / cell_cols); the last row and column of cells may be ragged.
 *   - Membership.  An event belongs to the cell of its recorded address, cell = (fr_x / cell_rows) * n_cell_y + fr_y /
 *     cell_cols, wherever a candidate projects it.
 *   - The objective.  S(k, cell) = sum of floor(score * 2^32) over the events of `cell` accepted under candidate k, the
 *     per-event term of S(k) ((sum << 32) / count): an exact int64, order free, and sum over cells of S(k, cell) == S(k).
 *   - A cell's answer is the first candidate in sweep order (nx outer, ny inner) with the largest S(k, cell): candidate 0
 *     when every S(k, cell) is 0, an empty cell included -- the slice rule.
 *   - The per-event best state folds exactly as in bf_global_search. */
typedef struct bf_global_cells {
    int32_t n_cell_x, n_cell_y;
} bf_global_cells;

typedef struct bf_global_cell_result {
    double best_nx, best_ny;   /* the cell's answer */
    double best_u, best_v;     /* Event::compute_uv of it, the expression of bf_global_get_events */
    int64_t best_sum;          /* S(best, cell) */
    int64_t best_index;        /* its place in the sweep: i_x * n_y + i_y */
    int64_t events;            /* events of the slice in the cell, accepted or not */
} bf_global_cell_result;

/* Lays the grid over a res_x x res_y sensor (rows x columns) and orders the slice by cell.  Valid after
 * bf_global_set_window, and invalidated like the window: BF_ERR_STATE when any upload happened since; setting the window
 * again clears the cells.  BF_ERR_ARG for a non-positive size, an event address outside res_x x res_y, more than 65536
 * cells, or no window.  out (may be NULL) reports the grid. */
int bf_global_set_cells(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t cell_rows, int32_t cell_cols, bf_global_cells *out);

/* bf_global_search with the objective kept per cell, continuing from the current per-event state: afterwards
 * bf_global_get_events returns what bf_global_search over the same range would have left.  slice_out (may be NULL) is
 * filled from S(k) = sum over cells, by the slice rule.  cells_out (may be NULL; cells_cap entries) is row-major
 * [n_cell_x][n_cell_y].  cell_surface_out (may be NULL; cell_surface_cap entries) receives S(k, cell) as
 * [cell][n_x][n_y]: at most 2^27 entries, else BF_ERR_CAPACITY; without it the device keeps one batch of candidates per
 * cell only.  BF_ERR_ARG for what bf_global_search refuses, a buffer shorter than the grid, or no cells. */
int bf_global_search_cells(bf_ctx *ctx, const bf_global_search_opts *opts, bf_global_result *slice_out,
                           bf_global_cell_result *cells_out, int64_t cells_cap, int64_t *cell_surface_out,
                           int64_t cell_surface_cap);

/* Coarse-to-fine and seeded forms of bf_global_search_cells: the candidate set is decided on the device from the per-cell
 * results instead of being the whole grid.  Definitions of this build ("OptimizerGlobal"):
 *   - The lattice is what opts describes: x_vals[i], y_vals[j] built by the reference's repeated double addition, n_x x n_y
 *     points, candidate index k = i * n_y + j (the best_index of bf_global_search_cells), at most 2^26 points.  The value
 *     of candidate k, and everything computed from it, is exactly what bf_global_search_cells uses for that k; so every
 *     S(k, cell) computed here is bit for bit an entry of the exhaustive surface over the same opts.
 *   - levels L in 1..8, factor f >= 2, radius r in 1..64.  Level l has the stride s_l = f^(L-1-l) lattice steps; s_0 must
 *     not exceed max(n_x, n_y).
 *   - Level 0 without seeds evaluates every (i, j) with i % s_0 == 0 and j % s_0 == 0.
 *   - Every other level (and level 0 with seeds) takes each cell that has events and a centre: the cell's running best if
 *     that best has S > 0, else its seed.  It evaluates the window (i* + a s_l, j* + b s_l), |a|, |b| <= r, clipped to the
 *     lattice; the level's set is the union over the cells minus everything evaluated before.  A cell without events, a
 *     cell whose best S is 0 and that has no seed, and a cell seeded -1 contribute nothing.
 *   - seed_index (may be NULL; one entry per cell, row-major like cells_out) is a lattice k or -1.  With seeds the strided
 *     pass is skipped: L levels of windows with strides s_0 .. 1.  levels == 1 with seeds is the streaming form: one window
 *     of +-r lattice steps around the previous slice's best_index.
 *   - Evaluation order: level by level, ascending k within a level, in batches of at most 32.  The per-event state folds
 *     in exactly that order with apply_score's strict `>` (evaluation order, not sweep order), continuing from the current
 *     state.  Every evaluated candidate is folded for every cell and for the slice's S(k).
 *   - A cell's answer is the evaluated candidate with the largest S(k, cell), the lowest k among equals (the lowest
 *     evaluated k when all are 0): the exhaustive rule restricted to the evaluated set, whatever the order of the levels.
 *     The slice's answer comes from the sum over cells by the same rule.
 *   - levels == 1 without seeds gives every output of bf_global_search_cells over the same opts, bit for bit. */
typedef struct bf_global_pyramid_opts {
    int32_t levels, factor, radius;
} bf_global_pyramid_opts;

typedef struct bf_global_pyramid_info {
    int64_t n_x, n_y;          /* the lattice */
    int64_t evaluated;         /* candidates evaluated: the sum of level_count */
    int64_t level_count[8];    /* candidates of level l (0 beyond levels_run) */
    int32_t levels_run;
    int32_t reserved;
} bf_global_pyramid_info;

/* pyramid NULL: levels 1 (the exhaustive sweep).  Outputs, any of which may be NULL: slice_out; cells_out (cells_cap
 * entries, [n_cell_x][n_cell_y]); evaluated_out (evaluated_cap entries): the evaluated k in evaluation order;
 * cell_surface_out (cell_surface_cap entries): S(k, cell) as [cell][info->evaluated], columns in the order of evaluated_out,
 * at most 2^27 entries; info.  Preconditions and invalidation are those of bf_global_search_cells.  BF_ERR_ARG for what
 * bf_global_search_cells refuses, levels / factor / radius out of range, a stride beyond the lattice, a seed outside
 * [-1, n_x * n_y), seeds that leave nothing to evaluate (all -1, or only on cells without events), or a buffer too short
 * for what a level adds; BF_ERR_CAPACITY for a surface beyond 2^27 entries.  After either code the per-event state is what
 * it was before the call (a short evaluated_out or surface is found out level by level: the state is put back). */
int bf_global_search_cells_pyramid(bf_ctx *ctx, const bf_global_search_opts *opts, const bf_global_pyramid_opts *pyramid,
                                   const int64_t *seed_index, bf_global_result *slice_out, bf_global_cell_result *cells_out,
                                   int64_t cells_cap, int64_t *evaluated_out, int64_t evaluated_cap, int64_t *cell_surface_out,
                                   int64_t cell_surface_cap, bf_global_pyramid_info *info);

/* The piecewise projection: the slice rendered and scored with every event under the flow of its own cell.  A fifth
 * definition of this build ("OptimizerGlobal"), over the window of bf_global_set_window and the grid of
 * bf_global_set_cells, given one candidate (nx_c, ny_c) per cell and a common nz:
 *   - Projection.  Every event is projected by Event::project in its float form under the candidate of the cell of its
 *     recorded address (the membership of bf_global_set_cells); kx = float(nx_c) / nz and ky are computed once per cell,
 *     on the host, by the expressions of every other candidate of this family.
 *   - Image.  Every later step is bf_global_project_all's, with all events in ONE image: the pixel truncation and the
 *     acceptance test, the saturating scale x scale splat into the bordered image, this build's 8-bit Gaussian, and per
 *     accepted event the mean of the non-zero blurred pixels in its metric_wsize^2 window.
 *   - Objective.  S_pw(cell) = sum of floor(score * 2^32) over the accepted events of the cell, each (sum << 32) / count;
 *     S_pw = sum over the cells of S_pw(cell).  Exact int64, order free.  (Not S(k, cell): that is measured with EVERY
 *     event moved by k, the neighbours from other cells included.)
 *   - State.  The per-event best state is not touched -- a piecewise field is no candidate of the sweep, apply_score has
 *     nothing to record for it -- nor are the cells' running bests or the scratch of the pyramid; the uploaded events are
 *     not moved.  The call may be mixed freely with bf_global_project_all and the searches on one window.
 *   - The entry of a cell without events is never read: it may hold anything, NaN included.
 *   - Identity.  With the same (nx, ny) in every cell, img_out, scores_out and S_pw are bf_global_project_all(nx, ny, nz)'s
 *     outputs bit for bit.
 *   - Interpolating between cell centres (a smooth field) is not part of this definition: bf_global_project_field below.
 * cell_nx / cell_ny: cells_cap entries each, row-major [n_cell_x][n_cell_y] like cells_out.  img_out, scores_out, sum_out
 * (S_pw) as in bf_global_project_all, each may be NULL; cell_sums_out (may be NULL; cell_sums_cap entries) S_pw(cell), row-major.
 * An empty cloud: every sum 0, the images zero, BF_OK.  BF_ERR_ARG without a window or cells, for a buffer shorter than the
 * grid, nz <= 0, or a value in a cell that has events that is not finite in the projection's float form (inf, NaN, or a
 * double past float range such as 1e39: kx or ky would not be finite); nothing ran then and every state is as before.
 * BF_ERR_STATE when an upload happened since bf_global_set_window. */
int bf_global_project_cells(bf_ctx *ctx, const double *cell_nx, const double *cell_ny, int64_t cells_cap, double nz,
                            uint8_t *img_out, float *scores_out, int64_t *sum_out, int64_t *cell_sums_out,
                            int64_t cell_sums_cap);

/* The interpolated field: the slice rendered and scored with every event under the flow interpolated between the cell
 * centres around its recorded address.  A sixth definition of this build ("OptimizerGlobal"), beside
 * bf_global_project_cells, over the same window and grid, given one candidate (nx_c, ny_c) per cell and a common nz.  The
 * arithmetic is stated once, for device and host, in include/bf_global_field.h; every operation is an integer one or a
 * single IEEE double operation (no contraction).
 *   - Cell centres.  Cell a along the rows has its nominal centre at (a + 0.5) * cell_rows - 0.5 sensor pixels, likewise
 *     along the columns; a ragged last cell keeps its nominal centre.
 *   - Corners and weights, per axis, as integers.  For the recorded address x on an axis of n_cell cells of `size` pixels:
 *     p = 2x + 1 - size, D = 2 * size, a0 = floor(p / D), w = p - a0 * D in [0, D); then a0 < 0 -> a0 = 0, w = 0, and
 *     a0 >= n_cell - 1 -> a0 = n_cell - 1, w = 0; a1 = min(a0 + 1, n_cell - 1).  Beyond the outermost centres the field is
 *     constant; an axis with one cell has no interpolation.
 *   - Value per event, for nx and identically for ny, all double: tx = (double)wx / (double)Dx, ty = (double)wy / (double)Dy;
 *     top = n00 + ty * (n01 - n00); bot = n10 + ty * (n11 - n10); nx_e = top + tx * (bot - top), with n_ab the grid value at
 *     (row a_a, column b_b).  This order is part of the definition, for three identities: a uniform grid gives nx_e == n;
 *     an event at a cell centre (w == 0 on both axes) gets its cell's value; cell_rows == cell_cols == 1 gives w == 0
 *     everywhere.  (As values: a grid entry -0.0 comes back as +0.0.)
 *   - Projection.  kx = (float)((double)(float)nx_e / nz), ky likewise: the expressions of every other candidate of this
 *     family, evaluated per event on the device.  Every later step is bf_global_project_cells': the pixel truncation and
 *     the acceptance test, the splat into ONE image, the 8-bit Gaussian, the window score.
 *   - Objective.  S_f(cell) = sum of floor(score * 2^32) over the accepted events of the cell of the event's recorded
 *     address; S_f = sum over the cells.  Exact int64, order free.
 *   - The WHOLE grid is read -- a cell without events is still a corner for its neighbours -- and every one of its entries
 *     must be finite in the projection's float form (as in bf_global_project_cells, but for every cell).
 *     The check is on the entries, and is taken to bound the interpolated values: those lie between their corners up to
 *     rounding.  An event whose own kx or ky still came out infinite or NaN (corners at opposite ends of the float range, a
 *     tiny nz) fails the acceptance test like under any such candidate: it is not drawn and not scored.
 *   - State.  As bf_global_project_cells: the per-event best state, the cells' running bests, the scratch of the pyramid
 *     and the uploaded events are left alone; the call mixes freely with every other call of the family.
 *   - Identities.  With the same (nx, ny) in every cell the outputs are bf_global_project_all(nx, ny, nz)'s bit for bit; with
 *     cell_rows == cell_cols == 1 they are bf_global_project_cells' over the same grid.
 * cell_nx / cell_ny, img_out, scores_out, sum_out (S_f), cell_sums_out (S_f(cell)) as in bf_global_project_cells.  Per-event
 * outputs, n doubles each in upload order, each may be NULL: event_nx_out / event_ny_out the interpolated (nx_e, ny_e) of
 * every event, accepted or not (written on the device, only when one of the four is asked for); event_u_out / event_v_out
 * Event::compute_uv of them with nz, the expression of bf_global_get_events, on the host.  An empty cloud: every sum 0, the
 * images zero, nothing written to the per-event outputs, BF_OK.  BF_ERR_ARG without a window or cells, for a buffer
 * shorter than the grid, nz <= 0, or an entry of ANY cell that is not finite in the projection's float form; nothing ran
 * then and every state and output is as before.  BF_ERR_STATE when an upload happened since bf_global_set_window. */
int bf_global_project_field(bf_ctx *ctx, const double *cell_nx, const double *cell_ny, int64_t cells_cap, double nz,
                            uint8_t *img_out, float *scores_out, int64_t *sum_out, int64_t *cell_sums_out,
                            int64_t cell_sums_cap, double *event_nx_out, double *event_ny_out, double *event_u_out,
                            double *event_v_out);

/* ---- per-event flow table on the device: DVS_flow::get_accumulated (dvs_flow.h:351-389) -----------------------------
 * The -o table (every event once, with the flow of the first slice that solved it) built slice by slice on the device,
 * with the marking rule of bf::StreamEngine::get_accumulated (stream_flow.h), for slices cut from one event ring whose
 * timestamps do not decrease.  A bf_emit holds what carries from slice to slice: a covered byte per ring position
 * (ring_cap of them: event g lives at g % ring_cap), per pixel of a rows x cols sensor the newest timestamp at which an
 * emitted event can still mark later arrivals, and the running row count.  Every event of an emitted slice must lie on that
 * sensor.  The rows go to an output ring of out_rows rows in pinned host memory that the state owns (bf_emit_output: five
 * column arrays, row r at index r % out_rows), written by the device directly.  The state lives on the device of the context
 * it was created with; any context on that device may emit into it.
 *   bf_emit_create   state for a ring of ring_cap positions (>= the largest slice + 1) and a rows x cols sensor.
 *   bf_emit_reset    forget every slice and every row (a new stream).  Waits for the slices in flight.
 *   bf_emit_slice    ENQUEUES the rows of one solved slice on ctx's stream, solving nothing, and returns at once with a ticket
 *                    (0, 1, 2, ...).  n events = the context's committed slice (n == 0: an empty slice, the context is not
 *                    read), the oldest at ring position `first`; start_time its origin in the timestamps' units (an event
 *                    with timestamp start_time - 1 carries the reference's t == -1 mark and is left out); lead != 0: event
 *                    first - 1, which the full ring left out of the slice and no slice has held, is emitted first with zero
 *                    flow (its logical timestamp and address in lead_t / lead_row / lead_col).  Slices run on the device in
 *                    the order of these calls, whatever contexts they come from (the caller makes the calls in slice order,
 *                    one at a time); a context may start its next upload at once.  The flow is what bf_compute_uv_ring reads
 *                    back (zero when no warp ran).  BF_ERR_CAPACITY when the slice's n + (lead != 0) rows might not fit the
 *                    output ring beside the rows not yet released, or 1024 slices wait -- checked first: nothing runs and the
 *                    state is unchanged.  BF_ERR_ARG for a slice starting before the previous one or more elements than
 *                    ring_cap; BF_ERR_STATE when n is not the context's slice.  *ticket_out = -1 for a slice without elements.
 *   bf_emit_wait     waits for slice `ticket` (tickets in order) and gives its rows: [*first_row, *first_row + *rows) of the
 *                    output ring, oldest -> newest.  BF_ERR_ARG if an address lay outside the sensor (then the state is
 *                    undefined until bf_emit_reset).
 *   bf_emit_release  the rows below upto_row have been read: their ring space may be reused.
 * The kernels are in bf_emit.hip; DESIGN.md, "Device-side -o table", states the rule and why the device form is exact. */
typedef struct bf_emit bf_emit;
int bf_emit_create(bf_ctx *ctx, int64_t ring_cap, int32_t rows, int32_t cols, int64_t out_rows, bf_emit **out);
int bf_emit_destroy(bf_emit *emit);
int bf_emit_reset(bf_ctx *ctx, bf_emit *emit);
int bf_emit_output(bf_emit *emit, uint64_t **t, uint16_t **row, uint16_t **col, double **u, double **v, int64_t *out_rows);
int bf_emit_slice(bf_ctx *ctx, bf_emit *emit, int64_t n, uint64_t first, uint64_t start_time, int32_t lead, uint64_t lead_t,
                  int32_t lead_row, int32_t lead_col, int64_t *ticket_out);
int bf_emit_wait(bf_ctx *ctx, bf_emit *emit, int64_t ticket, uint64_t *first_row, int64_t *rows);
int bf_emit_release(bf_emit *emit, uint64_t upto_row);

/* ---- per-slice frames on the device: DVS_flow::render_frame (dvs_flow.h) -----------------------------------------------
 * The frame of --img / --video: the 2 x 2 mosaic of the context's live slice -- projection image (grey) and colour-coded time
 * image, motion compensated on top, as recorded below -- at scale 3 whatever scale the slice was solved at, every tile
 * (3 res_x) x (3 res_y), so the frame is (6 res_x) x (6 res_y) pixels.  It is composed on the device in the byte layouts of the
 * files: BF_FRAME_PPM, the PPM payload (top-down RGB, the bytes after the "P6" header), and BF_FRAME_AVI, the AVI payload
 * (bottom-up BGR rows padded with zeros to a multiple of 4 bytes), both byte for byte those of host/better_flow/frame_writer.h.
 * A bf_frame owns `slots` frames per layout in pinned, device-mapped host memory, which the compose kernel writes directly; it
 * lives on the device of the context it was created with, and its contexts need an image capacity of
 * (3 res_x + 3) x (3 res_y + 3) (bf_create's max_rows / max_cols).
 *   bf_frame_create   state for a res_x x res_y sensor; layouts: a mask of BF_FRAME_PPM and BF_FRAME_AVI.
 *   bf_frame_destroy  waits for the renders in flight, then frees everything.
 *   bf_frame_render   ENQUEUES the frame of ctx's live slice -- as it stands after bf_run, a pending bf_set_model warp applied
 *                     first, like bf_projection_img -- on ctx's stream into a free slot and returns at once with a ticket
 *                     (0, 1, 2, ...).  The context may upload and solve its next slice at once: the frame sees the slice it
 *                     was rendered from.  BF_ERR_CAPACITY when every slot is taken (checked first: nothing runs).
 *   bf_frame_wait     waits for frame `ticket` and gives its payloads (NULL for a layout not created); valid until released.
 *                     BF_ERR_ARG for a ticket released or never issued.
 *   bf_frame_release  the slot of `ticket` may be reused.
 *   bf_render_frame   the synchronous form: one frame of ctx's live slice into ppm_out (res_x * res_y * 108 bytes) and / or
 *                     avi_out (6 res_x rows of ((18 res_y + 3) & ~3) bytes); either may be NULL, not both.
 * The kernel is in bf_frame.hip; DESIGN.md, section 11, states what is bit-exact against what. */
#define BF_FRAME_PPM 1
#define BF_FRAME_AVI 2
typedef struct bf_frame bf_frame;
int bf_frame_create(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t slots, int32_t layouts, bf_frame **out);
int bf_frame_destroy(bf_frame *frame);
int bf_frame_render(bf_ctx *ctx, bf_frame *frame, int64_t *ticket_out);
int bf_frame_wait(bf_ctx *ctx, bf_frame *frame, int64_t ticket, const uint8_t **ppm, const uint8_t **avi);
int bf_frame_release(bf_frame *frame, int64_t ticket);
int bf_render_frame(bf_ctx *ctx, int32_t res_x, int32_t res_y, uint8_t *ppm_out, uint8_t *avi_out);

/* ---- per-pixel flow: EventFile::color_flow_img (event_file.h:318-350) and the field behind it ---------------------------------
 * The picture of the flow that the reference's live front end publishes after every recompute() (bf_visualizer.cpp:249-265),
 * and the same scatter stopped before the colour step: the per-pixel flow field.  On a res_x x res_y sensor, pixel (x, y) at
 * index x * res_y + y (x the row):
 *   - every non-noise event of the live slice lands on pixel (x, y) = ((int)pr_x, (int)pr_y) -- C truncation toward zero of the
 *     double, so pr = -0.7 lands on 0, INSIDE; NaN and anything outside the int range give INT_MIN, as on x86 -- and is left
 *     out unless 0 <= x < res_x and 0 <= y < res_y (:324-328).  pr is the event's current projected position, what
 *     bf_writeout_events returns (a pending bf_set_model warp applied first, as by every renderer);
 *   - the reference assigns (:337-338), so the LAST event of its loop that lands on a pixel owns it.  Ownership is defined here
 *     on the UPLOAD index -- not on where an event sits after the device has re-binned the slice -- and `owner_rule` says which
 *     end wins: BF_FLOW_LAST_UPLOADED, the largest upload index (a container the reference iterates in upload order: DVS_flow
 *     here uploads its ring in iteration order, newest -> oldest), or BF_FLOW_FIRST_UPLOADED, the smallest (a slice uploaded
 *     oldest -> newest, bf_upload_ring*_async, that the reference iterates newest -> oldest, datastructures.h:66-76).  Either
 *     way the owner of a pixel in the command line is the OLDEST non-noise event that lands on it;
 *   - the field of a pixel is its owner's (best_u, best_v) = Event::compute_uv (event.h:135-142): bit for bit what bf_compute_uv
 *     returns at that upload index (0 when no warp has run);
 *   - colour (:330-338, all double): speed = hypot(u, v); angle = speed != 0 ? (atan2(v, u) + 3.1416) * 180 / 3.1416 : 0;
 *     log_spd = std::min(255.0, log(speed) / log(1.025)); H = uchar(angle / 2), S = uchar(log_spd), V = 255; a pixel without an
 *     event is HSV (0, 0, 255): white.  double -> uchar is what the reference's x86-64 build does: truncate to int32
 *     (cvttsd2si: NaN and out-of-range values give INT_MIN), keep the low byte.  So a speed below 1 px/s, whose log_spd is
 *     negative, wraps (0.5 px/s: -28.07 -> -28 -> 228); speed == 0 gives log_spd = -inf -> INT_MIN -> S = 0 (and H = 0);
 *     a NaN flow gives H = 0 (NaN -> INT_MIN) and S = 255 (std::min(255.0, NaN) is 255.0); speeds from 1.025^255 = 543 px/s
 *     up saturate at S = 255.  include/bf_flow_color.h holds this arithmetic for the device and the host alike;
 *   - HSV -> BGR is the float formula stated at bf_color_time_img (the same function); parity with the reference's
 *     un-versioned cv::cvtColor stays unpinned for that stage, as there.  atan2 / log / hypot are the device library's,
 *     which may differ from a host libm in the last place: a pixel whose angle / 2 or log_spd lies within an ulp of an
 *     integer may differ by one H or S step between the two.
 * One deliberate deviation: the reference paints best_pr / best_u / best_v, which a slice stopped by
 * a guard of run() (optimizer_rolling.h:49-58) never assumes; this build paints such a slice's own current state.
 *   bf_flow_field      owner_out[x * res_y + y]: upload index of the owning event, -1 without one; u_out / v_out: its flow,
 *                      0 without one.  Any output may be NULL.
 *   bf_color_flow_img  bgr_out: res_x * res_y * 3 bytes, B, G, R; hs_out (may be NULL): res_x * res_y * 2 bytes, the H and S
 *                      of every pixel before the conversion.
 * Both enqueue on the context stream, copy and synchronise.  BF_ERR_STATE before an upload; BF_ERR_ARG for an unknown rule or
 * a sensor of more pixels than the context's image capacity (bf_create's max_rows x max_cols).
 *
 * The flow frame of --flow-img: three res_x x res_y tiles side by side, left to right bf_projection_img(scale 1, show_final 0)
 * grey -> BGR, bf_color_flow_img, bf_projection_img(scale 1, show_final 1) grey -> BGR -- the visualiser's three topics, not
 * transposed --, res_x x (3 res_y) pixels.  Composed on the device in the byte layouts of the files, byte for byte
 * host/better_flow/frame_writer.h's compose_flow_frame: BF_FRAME_PPM (top-down RGB) and BF_FRAME_AVI (bottom-up BGR rows padded
 * with zeros to a multiple of 4 bytes); BF_FLOW_FRAME_FLO adds the field as the payload of a Middlebury .flo file: per pixel,
 * row-major, two float32 -- horizontal = (float)v, vertical = (float)u, the swap -o makes (event_file.h:274-275) -- and 1e9 in
 * both for a pixel without an event.  A bf_flow_frame owns `slots` frames per layout in pinned, device-mapped host memory;
 * the calls are bf_frame_*'s (tickets 0, 1, 2, ...; BF_ERR_CAPACITY with every slot taken, checked first; BF_ERR_ARG for a ticket
 * released or never issued); every context renders into its own scratch, so contexts of one device may share a bf_flow_frame.
 *   bf_render_flow_frame  the synchronous form: ppm_out (res_x * res_y * 9 bytes), avi_out (res_x rows of ((9 res_y + 3) & ~3)
 *                         bytes), flo_out (res_x * res_y * 2 floats); any may be NULL, not all.
 * The kernels are in bf_flowimg.hip. */
#define BF_FLOW_LAST_UPLOADED 0
#define BF_FLOW_FIRST_UPLOADED 1
#define BF_FLOW_FRAME_FLO 4
typedef struct bf_flow_frame bf_flow_frame;
int bf_flow_field(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, int32_t *owner_out, double *u_out, double *v_out);
int bf_color_flow_img(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t *bgr_out, uint8_t *hs_out);
int bf_flow_frame_create(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t slots, int32_t layouts, bf_flow_frame **out);
int bf_flow_frame_destroy(bf_flow_frame *frame);
int bf_flow_frame_render(bf_ctx *ctx, bf_flow_frame *frame, int32_t owner_rule, int64_t *ticket_out);
int bf_flow_frame_wait(bf_ctx *ctx, bf_flow_frame *frame, int64_t ticket, const uint8_t **ppm, const uint8_t **avi, const float **flo);
int bf_flow_frame_release(bf_flow_frame *frame, int64_t ticket);
int bf_render_flow_frame(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t *ppm_out, uint8_t *avi_out,
                         float *flo_out);

/* ---- the held flow of the exhaustive search: a per-event flow kept on the device, and its outputs -------------------------
 * A seventh definition of this build ("OptimizerGlobal").  A HELD FLOW is, for the n events of the slice
 * bf_global_set_window ran on: (nx, ny) and (u, v) per event in upload order, the two f32 products
 * p = (kx * float(t), ky * float(t)) of Event::apply_project, from which the event's position is pr = float(fr) -
 * (double)p / 10000.0 (the device's pr_from_p, exactly the division).  The nz a flow was formed with -- one for a grid mode,
 * best_nz per event for the snapshot -- is spent when it is formed: p and (u, v) carry it, and it is not kept.  kx =
 * (float)((double)(float)nx / nz), ky likewise, as for every candidate of the family; (u, v) is Event::compute_uv --
 * len = hypot(nx, ny), speed = len / (nz / 100000.0), u = len == 0 ? 0 : speed * nx / len, v likewise -- evaluated on the
 * device with the device's hypot: each of u, v is within 4 * 2^-52 (relative) of the host's value whatever either hypot
 * returns (len cancels: both are three correctly rounded operations away from n / (nz / 100000)), and exactly 0 for a zero flow.
 * There is at most one held flow per context.  It becomes invalid at an upload, at bf_global_set_window and, when it came
 * from bf_global_hold_field, at bf_global_set_cells; every consumer below then returns BF_ERR_STATE, as it does before any hold.
 *
 *   bf_global_hold_field  every event under the candidate bf_global_project_cells (mode BF_GLOBAL_HOLD_CELLS: its cell's) or
 *       bf_global_project_field (BF_GLOBAL_HOLD_FIELD: interpolated at its address) would project it under, with the
 *       arguments, grid checks and error codes of those calls (the piecewise form reads no empty cell, the smooth form reads
 *       and checks the whole grid, nz <= 0 is refused; BF_ERR_ARG also for an unknown mode).  One launch; nothing is rendered
 *       or scored, and the per-event best state, the cells' running bests, the pyramid's scratch and the rolling optimiser's
 *       state are left alone.  A refused call leaves the held flow as it was.
 *   bf_global_hold_best   a snapshot of the searches' per-event state: (nx, ny) = (best_nx, best_ny) with nz = best_nz PER
 *       EVENT; pr comes out as best_pr bit for bit.  An event no candidate was accepted for gets zero flow and pr = fr.  Needs a
 *       window (BF_ERR_ARG without), no cells; searches that run afterwards do not change it.
 *   bf_global_get_flow    the held flow to the host through pinned staging: n doubles each, upload order, each may be NULL.
 *       An empty cloud: BF_OK, nothing written.
 *   bf_global_flow_field, bf_global_color_flow_img, bf_global_render_flow_frame, bf_global_flow_frame_render
 *       bf_flow_field, bf_color_flow_img, bf_render_flow_frame and bf_flow_frame_render (same arguments, layouts, frame
 *       objects, tickets, wait and release) read from the held flow: EVERY event takes part (the family has no noise flags,
 *       and the scaled window's acceptance test plays no role), it lands on pixel ((int)pr_x, (int)pr_y) and is dropped
 *       outside the sensor, ownership is by upload index under owner_rule, and a pixel's field is the held (u, v) of its
 *       owner as bits.  The frame's left tile is the scale-1 projection image of the held positions, its right tile that of
 *       the raw ones.  An empty cloud gives the images of no event (white flow).
 *   bf_global_emit_slice  bf_emit_slice (same arguments, rule, ticket, wait and release) with the rows' (u, v) taken from
 *       the held flow.  BF_ERR_STATE without a held flow or when n is not the number of events it holds. */
#define BF_GLOBAL_HOLD_CELLS 1
#define BF_GLOBAL_HOLD_FIELD 2
int bf_global_hold_field(bf_ctx *ctx, const double *cell_nx, const double *cell_ny, int64_t cells_cap, double nz, int32_t mode);
int bf_global_hold_best(bf_ctx *ctx);
int bf_global_get_flow(bf_ctx *ctx, double *nx, double *ny, double *u, double *v, double *pr_x, double *pr_y);
int bf_global_flow_field(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, int32_t *owner_out, double *u_out, double *v_out);
int bf_global_color_flow_img(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t *bgr_out, uint8_t *hs_out);
int bf_global_flow_frame_render(bf_ctx *ctx, bf_flow_frame *frame, int32_t owner_rule, int64_t *ticket_out);
int bf_global_render_flow_frame(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t *ppm_out, uint8_t *avi_out,
                                float *flo_out);
int bf_global_emit_slice(bf_ctx *ctx, bf_emit *emit, int64_t n, uint64_t first, uint64_t start_time, int32_t lead, uint64_t lead_t,
                         int32_t lead_row, int32_t lead_col, int64_t *ticket_out);

/* ---- the held flow of a grouping: every event under its own object's model, and the per-group median of a held flow ----
 * A further definition of this build.  The object pipeline ends with a grouping (an id per event) and
 * one four-parameter model per group; these two entries turn that into the per-event flow every reader of the held flow
 * above works on unchanged, and into the one per-object figure the host used to compute with K uploads.
 *
 *   bf_hold_groups  a fourth way to fill the context's ONE held flow.  Needs, in this order of checks: an uploaded slice
 *       (BF_ERR_STATE), bf_global_set_window on it (BF_ERR_STATE: the rule every reader is gated on), models != NULL,
 *       1 <= n_models <= 64, no noise mask (BF_ERR_ARG each), a held grouping (BF_ERR_STATE) of exactly n_models groups
 *       (BF_ERR_ARG).  Per event i with id k >= 0, in upload order: from the reset state (pr = fr) ONE
 *       warp_reinit(-total_dx, -total_dy, cx, cy, total_div, -total_rot) of models[k] -- set_model's warp, its sine and
 *       cosine from the host's libm, exactly the (nx, ny) bf_assign_groups and bf_project_groups form for pixel_k(i) -- then
 *       kx = (float)((double)(float)nx / 127), ky likewise, p = (kx * float(t), ky * float(t)) (two f32 products, nz = 127),
 *       pr = float(fr) - (double)p / 10000.0, and (u, v) = Event::compute_uv of (nx, ny): the bits of bf_compute_uv.  An
 *       event with id -1 is held with zero flow, p = 0 and pr = fr -- bf_global_hold_best's convention for an event no
 *       candidate was accepted for; it is still an event for the owner plane.  Zero events: BF_OK and an empty held flow.
 *       Like the snapshot of bf_global_hold_best the hold keeps its own copy of the slot order, so it survives a later
 *       bf_run / bf_run_groups re-sort, bf_set_groups, bf_assign_groups with install and bf_global_set_cells; it is dropped
 *       by bf_global_set_window and invalidated by any upload.  A refused call leaves the previous held flow as it was; a
 *       failure after the checks leaves none.  Nothing else is written: not the events' products, the rolling (nx, ny), the
 *       time image, the grouping, the vote planes or the per-event best state.  Blocking.
 *   bf_group_flow_medians  per group of the held grouping the median of the held u and of the held v over the group's
 *       events.  Needs a held flow of ANY mode and a held grouping of K groups on the same slice (BF_ERR_STATE otherwise);
 *       K > 64: BF_ERR_CAPACITY.  u_med and v_med: K doubles; counts: K + 1 words, counts[k] the events with id k, counts[K]
 *       those with id -1; each may be NULL.  The median orders the values by the total order
 *       key(x) = bits(x) ^ (sign(x) ? ~0 : 1 << 63) on the 64-bit pattern, so -0.0 sorts below +0.0; an odd count c gives
 *       element c / 2, an even count 0.5 * (a[c/2 - 1] + a[c/2]) as one f64 add and one f64 multiply, an empty group 0.0.
 *       The result is a function of the multiset of values alone: whatever order the events are stored in, the bits are
 *       those of sorting the keys.  On the device an 8-pass radix select; the host waits once.  Blocking. */
int bf_hold_groups(bf_ctx *ctx, const bf_model *models, int32_t n_models);
int bf_group_flow_medians(bf_ctx *ctx, double *u_med, double *v_med, int32_t *counts);

/* ---- event groups: candidate models -- the modes of the per-event best flow of the exhaustive search ----
 *
 * After bf_global_search every event holds the lattice candidate under which its neighbourhood was sharpest (best_nx,
 * best_ny, max_score).  The modes of that per-event best flow are the motions present in the slice; this entry turns them
 * into the candidate models bf_assign_groups starts from.  Everything after the index match is an
 * integer count, a maximum or a lowest index: the result does not depend on storage order or scheduling.
 *
 *   lattice   x_vals (n_x values) and y_vals (n_y) of `lattice`, built as bf_global_search builds its candidates (repeated
 *             double addition from x_low while < x_hi; y likewise); NULL: bf_global_search_opts_default.  It must be the
 *             lattice the state was searched over.  n_x * n_y <= 2^22, else BF_ERR_CAPACITY.
 *   votes     event e votes for (i, j) when max_score[e] > 0, best_nx[e] == x_vals[i] and best_ny[e] == y_vals[j]: exact
 *             double equality; the values are strictly increasing, so the index is unique.  max_score == 0 counts in
 *             `unscored`; a best that is on no lattice point (the state was continued from another range or from
 *             bf_global_project_all) counts in `off_lattice`; neither of the two votes.  H[i][j] = the number of votes,
 *             `voted` = its sum: voted + unscored + off_lattice = the events of the slice.
 *   smoothing B[i][j] = the sum of H[i + a][j + b] over |a|, |b| <= radius, zero outside the lattice.
 *   pick      up to max_models times: among the points not within Chebyshev distance `suppress` of an earlier pick the
 *             largest B, among equals the lowest index i * n_y + j; stop when that B is below min_votes.  Proposals are in
 *             pick order, so `votes` is non-increasing.
 *   models    models_out[p] is all zero except total_dx = -nx and total_dy = -ny: the model whose set_model warp
 *             (optimizer_rolling.h:289-299) compensates the flow.  lattice->nz must be 127 for models_out != NULL
 *             (BF_ERR_ARG): the rolling path's Event has no other nz.
 *   state     reads the per-event best state only; that state, a held flow, a held grouping, a segmentation, products, the
 *             time image and the read-back validity are untouched.
 *   outputs   models_out / proposals_out: `cap` entries, the first info->proposals written; hist_out / box_out: H and B,
 *             n_x * n_y words each, row i at i * n_y (planes_cap: the words each holds).  Any output may be NULL.
 *   errors    BF_ERR_ARG for no window, a range error of any option (opts NULL: radius 1, suppress 2, max_models 8,
 *             min_votes 1), cap < max_models with models_out or proposals_out, planes_cap < n_x * n_y with a plane;
 *             BF_ERR_STATE when any upload happened since bf_global_set_window (the rule of bf_global_get_events).  Zero
 *             events: BF_OK, zero proposals, info all zero except n_x and n_y.
 * Blocking.  bf_get_stat "propose_form": what the last call's vote kernel was, 1 a histogram per work-group in LDS (the
 * lattice and its value tables fit 64 KiB), 2 one global atomic per vote, 0 nothing was launched. */
typedef struct bf_propose_opts {   /* 32 bytes */
    int32_t radius;      /* r: box half-width in lattice steps, 0..8 */
    int32_t suppress;    /* half-width of the square suppressed around a pick, 0..64 */
    int32_t max_models;  /* 1..64 */
    int32_t min_votes;   /* >= 1: stop at the first peak whose smoothed count is below it */
    int32_t reserved[4];
} bf_propose_opts;
typedef struct bf_proposal {       /* 48 bytes */
    double nx, ny;       /* the lattice point's values, exactly the candidate bf_global_search used */
    double u, v;         /* Event::compute_uv of it with lattice->nz (the expression of bf_global_get_events) */
    int64_t index;       /* i * n_y + j */
    int32_t votes, peak; /* B and H at the point */
} bf_proposal;
typedef struct bf_propose_info {   /* 32 bytes */
    int64_t n_x, n_y;
    int32_t voted, unscored, off_lattice, proposals;
} bf_propose_info;
int bf_propose_models(bf_ctx *ctx, const bf_global_search_opts *lattice, const bf_propose_opts *opts,
                      bf_model *models_out, bf_proposal *proposals_out, int32_t cap,
                      uint32_t *hist_out, uint32_t *box_out, int64_t planes_cap, bf_propose_info *info);

/* ---- moving-object segmentation: connected components of the compensated time image ---------------------------------------
 * An eighth definition of this build ("Segmentation"); the reference only carries the vocabulary (Event::cl,
 * cl_id = -1, visited: event.h:23-34; Cluster: clustering.h).  Everything is defined on integers, so no result depends on
 * the order work-groups run in.  The image is the current window's time image T (f32 seconds) and count image c (u32),
 * R x C, exactly as bf_get_time_img produces them; a pixel index is p = row * C + col.
 *   1. q(p) = floor((double)T(p) * 2^30) as int64 (conversion and product are exact).
 *   2. n1 = number of pixels with c >= 1; Q = sum of q over them (int64); mu = floor_div(Q, n1) -- a floor, not C's truncation.
 *      n1 == 0: no foreground, zero components, BF_OK.
 *   3. A = floor(above_s * 2^30), B = floor(below_s * 2^30), in double on the host.  A negative threshold is disabled; NaN or
 *      an infinity is BF_ERR_ARG.  p is foreground iff c(p) >= min_count (min_count >= 1) and: both thresholds are disabled,
 *      or above_s >= 0 and q - mu > A, or below_s >= 0 and mu - q > B.
 *   4. Components under 4- or 8-connectivity (anything else: BF_ERR_ARG); a component's provisional name is its smallest
 *      pixel index.  Those with fewer than min_pixels pixels are dropped (their pixels become background); the kept ones are
 *      numbered 0 .. K-1 in ascending order of that smallest index.  labels[p] is the id, or -1.
 *   5. bf_component per kept component: id, first_pixel (the smallest index), pixels, events, the bounding box, and the
 *      int64 sums of row, column and q over its pixels.
 *   6. cl_id[i], upload order: the label of the event's centre pixel -- (int)(pr_x * scale + x_sh), (int)(pr_y * scale + y_sh)
 *      of get_time_img_cpu (accel_lib.h:154-155), the scatter kernel's own pixel -- and -1 when the time image skips the event
 *      (noise, outside the window) or the pixel is background.  A component's `events` counts the events with its cl_id.
 * Thresholds are seconds: the paper's rho > lambda is above_s = lambda * dt, and the caller knows dt.
 *
 *   bf_segment      runs the time-image pass itself (the launches of bf_get_time_img without its read-back: it can never label
 *                   a stale image), then the segmentation; labels, table and cl_id stay on the device.  BF_ERR_STATE before
 *                   bf_set_cloud or on a degenerate window; BF_ERR_ARG for bad options (NULL: the defaults).
 *   bf_segment_get  what the last bf_segment left: labels_out R * C, comps_out at most comps_cap rows, cl_id_out n; any pointer
 *                   may be NULL.  BF_ERR_STATE when no segmentation of the current window is held: an upload, bf_set_cloud
 *                   and every warp invalidate it.
 *   bf_label_image  the labelling alone (4. and 5.; q_sum = events = 0) of a host mask, non-zero = foreground, in the manner of
 *                   bf_sobel.  components_out: K.  BF_ERR_CAPACITY beyond the context's pixel capacity.  Leaves a held
 *                   segmentation invalid (it uses the same planes). */
typedef struct bf_segment_opts {
    double above_s, below_s;   /* seconds; negative: disabled */
    int32_t min_count;         /* >= 1 */
    int32_t connectivity;      /* 4 or 8 */
    int32_t min_pixels;        /* >= 1 */
    int32_t reserved;
} bf_segment_opts;

typedef struct bf_segment_info {
    int32_t rows, cols;
    int64_t n1, q_sum, q_mean;
    int32_t foreground_pixels;   /* before the size filter */
    int32_t components_found;    /* before the size filter */
    int32_t components;          /* kept */
    int32_t reserved;
} bf_segment_info;

typedef struct bf_component {
    int32_t id, first_pixel, pixels, events;
    int32_t row_min, row_max, col_min, col_max;
    int64_t row_sum, col_sum, q_sum;
} bf_component;

/* above_s = below_s = -1 (regions of activity), min_count 1, connectivity 8, min_pixels 1 */
void bf_segment_opts_default(bf_segment_opts *opts);
int bf_segment(bf_ctx *ctx, const bf_segment_opts *opts, bf_segment_info *info);
int bf_segment_get(bf_ctx *ctx, int32_t *labels_out, bf_component *comps_out, int32_t comps_cap, int32_t *cl_id_out);
int bf_label_image(bf_ctx *ctx, const uint8_t *mask, int32_t rows, int32_t cols, int32_t connectivity, int32_t min_pixels,
                   int32_t *labels_out, bf_component *comps_out, int32_t comps_cap, int32_t *components_out);

/* NUMA placement of a feeder thread (no reference counterpart: the reference is single-threaded, SURVEY 8(b) "Threading"; the
 * 8-GPU farm of SURVEY 8(e) wants one feeder thread per GPU with NUMA-local pinned buffers).
 *   bf_device_numa_node          host NUMA node of HIP device `device` (sysfs numa_node of its PCI function); -1: unknown.
 *   bf_bind_thread_to_numa_node  restricts the CALLING thread to the CPUs of `node` that the process may use (a container's
 *                                cpuset wins; no such CPUs, no such node or node < 0: nothing happens) and makes that node the
 *                                preferred one for memory the thread touches or pins from now on.  cpus_out (may be NULL): CPUs
 *                                the thread is bound to, 0 when nothing was done.
 *   bf_bind_thread_to_device_numa  the two together; node_out may be NULL.
 * Call it on a worker thread before the thread's first bf_create / bf_host_alloc.  bf::SliceFarm's workers, the lanes of
 * better_flow_amd/farm.py and every rank of bench.py do. */
int bf_device_numa_node(int32_t device, int32_t *node_out);
int bf_bind_thread_to_numa_node(int32_t node, int32_t *cpus_out);
int bf_bind_thread_to_device_numa(int32_t device, int32_t *node_out);

/* For callers that keep slices resident in HBM (bench.py, the streaming front end) and
 * hand them over with bf_upload_events_device.  bf_memcpy_h2d is synchronous.  (The reference's device buffers are
 * private members of AccelLib, accel_lib.h:15-27; no counterpart.) */
int bf_device_malloc(bf_ctx *ctx, int64_t bytes, void **out);
int bf_device_free(bf_ctx *ctx, void *ptr);
int bf_memcpy_h2d(bf_ctx *ctx, void *dst, const void *src, int64_t bytes);

/* ---- measurement ---------------------------------------------------------------- */

/* Per-kernel hipEvent timing (the reference times whole slices with std::clock in its driver,
 * bf_motion_compensator.cpp:158-177, and the minimiser under VERBOSE, optimizer_rolling.h:116-118).  mode 0: off (default).  mode 1: bracket every kernel
 * launch with events on the ctx stream; totals are read with bf_profile_get, which
 * synchronises the stream. */
int bf_profile_enable(bf_ctx *ctx, int32_t mode);
int bf_profile_reset(bf_ctx *ctx);
int bf_profile_get(bf_ctx *ctx, bf_profile *out);

/* Block until everything enqueued on the ctx stream has finished (the reference's calls are all blocking:
 * CL_TRUE reads / writes and queue->finish(), accel_lib.h:109-115,317-321). */
int bf_synchronize(bf_ctx *ctx);

/* No reference counterpart.  Streaming-copy bandwidth probe on this device: copies `bytes` bytes `reps` times
 * with a float4 kernel and returns the best GB/s (read + write counted).  Used by
 * bench.py to report the measured HBM ceiling next to the 8 TB/s nominal peak. */
int bf_copy_bandwidth(bf_ctx *ctx, int64_t bytes, int32_t reps, double *gbps_out);

/* No reference counterpart.  The sine and cosine the device loops use for the warp's rotation angle
 * (Event::project_4param_reinit evaluates std::cos / std::sin, event.h:102-103; bf_run's update computes them on the device:
 * a polynomial for |x| <= 0.25, the device library beyond), evaluated for `n` host arguments.  table != 0: the variant of the
 * persistent loop kernel, coefficients read from an LDS table -- the same operations in the same order.  For measuring the
 * distance to the host's libm (tests/test_gpu_parity.py; the bound is stated in DESIGN.md, "Oracle"). */
int bf_eval_sincos(bf_ctx *ctx, const double *x, int64_t n, int32_t table, double *sin_out, double *cos_out);

#ifdef __cplusplus
}
#endif
#endif /* BF_ACCEL_H */
