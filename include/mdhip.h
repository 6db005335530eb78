/*
 * mdhip.h — C ABI of libmdhip.so, the MI355X (gfx950) backend for the
 * RDF/CN and MSD/Green-Kubo hot path of molmd/mdproptools.
 *
 * The reference has no plugin/FFI seam of its own: its hot path is a set of
 * private array-in/array-out Python functions. Each entry point below replaces
 * exactly one of them and cites it (paths under /root/reference/mdproptools/).
 * INTEGRATION.md shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *  - plain C types, caller-owned buffers, C-contiguous, float64 unless noted;
 *  - every call returns 0 on success or a negative MDHIP_E* code; the text is
 *    available from mdhip_last_error(); nothing throws across the boundary;
 *  - "host|dev" inputs: the big per-frame planes may live in host memory
 *    (the library stages them) or already in device memory (flag `on_device`);
 *    small tables (relations, cutoffs, offsets, boxes) are always host
 *    pointers; results are written to host pointers, except by the entry points
 *    named *_dev, which write the same values to a DEVICE buffer of the caller
 *    (one process per GPU: the multi-GPU layer hands that buffer to RCCL);
 *  - calls are synchronous on the context's stream: results are complete when
 *    the call returns — except for the entry points named *_async (SURVEY.md
 *    8b: "an _async variant + mdhip_sync"), which return with their work queued
 *    on the stream; see "asynchronous calls" below. One context per thread;
 *    contexts are independent;
 *  - there is NO CPU fallback: without a usable HIP device mdhip_create fails.
 *
 * Integer results (histograms, counts) are exact and independent of the
 * launch geometry. Floating-point reductions use a fixed order per launch
 * geometry (no float atomics), so they are reproducible run to run.
 */
#ifndef MDHIP_H
#define MDHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDHIP_VERSION 610 /* 0.6.1: + mdhip_lag_plan (which spectral path a full-lag MSD call would take, without a device); 0.6.0: + mdhip_pair_plan (which pair kernel a call would run, without a device), mdhip_row_displacement, MDHIP_EUNKNOWN (mdhip_ticket_status of a forgotten ticket), mdhip_lag_msd* finishes on the device at every length; 0.5.0: + mdhip_ticket_status / mdhip_fallbacks / MDHIP_EPENDING (a call's own completion status), mdhip_lag_msd_status_dev; 0.4.0: the *_async entry points with mdhip_sync / mdhip_wait / mdhip_call_stats, mdhip_green_kubo, mdhip_cumtrapz_dev */

#define MDHIP_OK 0
#define MDHIP_EINVAL (-1)  /* bad argument (shape, NULL, unsupported size) */
#define MDHIP_EHIP (-2)    /* a HIP runtime call failed */
#define MDHIP_ENOMEM (-3)  /* device or host allocation failed */
#define MDHIP_ENODEV (-4)  /* no usable gfx950 device */
#define MDHIP_ELIMIT (-5)  /* problem exceeds a kernel limit (e.g. LDS for the histogram rows) */
#define MDHIP_EPENDING (-6) /* mdhip_ticket_status: the call is still in flight */
#define MDHIP_EUNKNOWN (-7) /* mdhip_ticket_status: no such call is remembered (more than 64 completed calls ago) */

typedef struct mdhip_ctx mdhip_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
int mdhip_version(void);
/* Binds `device` (ordinal), creates a stream and a growable device workspace. */
int mdhip_create(mdhip_ctx **out, int device);
void mdhip_destroy(mdhip_ctx *ctx);
/* Last error text of this context (or of mdhip_create when ctx == NULL). */
const char *mdhip_last_error(mdhip_ctx *ctx);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the own stream. */
int mdhip_set_stream(mdhip_ctx *ctx, void *hip_stream);
/*
 * ---- asynchronous calls ----------------------------------------------------
 * A *_async entry point takes the arguments of its synchronous twin (a trailing `*_on_device` flag where the twin
 * comes as a host / _dev pair), queues ALL of its device work — staging of the small tables, kernels, the copy of
 * the results into page-locked staging — on the context's stream and returns. The call COMPLETES later, inside
 * mdhip_sync or mdhip_wait, in issue order: only then are host results in the caller's arrays, device results final
 * (a rare internal re-run may rewrite them at completion), and the error code of the call known — mdhip_sync /
 * mdhip_wait return the first error of the calls they completed (text: mdhip_last_error). Until then every array
 * passed to the call — inputs and outputs, host and device, the small tables too — must stay valid and unchanged.
 * Several calls may be in flight; their kernels run back to back on the stream with no host round trip between
 * them, which is the point: a step of k calls costs its kernels plus ONE wait (reference callers are plain
 * synchronous Python, e.g. dynamical/viscosity.py:178-190, so the overlap has to come from here). Inputs the
 * asynchronous path does not take (frames in pageable host memory, class passes, the edge-table kernels) are
 * handled by completing that part of the work before the call returns: correct, just not overlapped.
 * A synchronous call completes everything issued before it first. mdhip_destroy completes what is still in flight.
 *
 * Two pair calls on the device at once. The context owns a second compute stream with a second set of every buffer a
 * pair call writes (sorted records, boxes, lists, slices, row sums, flag words, results, host-frame staging).
 * Consecutive asynchronous atom-atom pair calls (mdhip_rdf_atomic*_async, mdhip_cn_atomic_async,
 * mdhip_rdf_cn_atomic_async) alternate between the two streams, each call's whole chain in order on its own: the
 * pre-pass of call k + 1 runs while the sweep of call k empties out, and the blocks of sweep k + 1 move in as those of
 * sweep k retire. Results do not change (integer sums). The rule for memory: a call overlaps only when its frames are
 * ONE batch of the pair path (the batches are bounded by ~2 GiB of workspace each, so the second set costs at most
 * that much again) AND two sets of what that batch needs fit the free device memory (asked for whenever a call is
 * larger than any before it). Otherwise — a call of several batches keeps its full-size batches — it runs
 * un-overlapped: alone, behind everything issued before it, as every other kind of call does (ordered by events,
 * without a host wait). So do all calls while the context launches on a caller's stream (mdhip_set_stream): their
 * order against the other work of that stream is the caller's. Growing a buffer waits for the calls of that buffer's
 * own stream only.
 */
/* Completes every call in flight, then waits for the stream. Returns the first error among them, 0 if none. */
int mdhip_sync(mdhip_ctx *ctx);
/* Completes the calls in flight in issue order until at most `keep_in_flight` remain (double buffering: issue step
 * k + 1, then mdhip_wait(ctx, 1) for the results of step k while k + 1 runs). */
int mdhip_wait(mdhip_ctx *ctx, int keep_in_flight);
/* Number of asynchronous calls issued and not yet completed. */
int mdhip_pending(mdhip_ctx *ctx);
/* Kernel time / preparation time / launches / dominant kernel of the call completed `back` calls ago (0 = the last
 * one, as mdhip_last_kernel_ms reports; the last 64 are remembered). Any output pointer may be NULL. */
int mdhip_call_stats(mdhip_ctx *ctx, int back, double *kernel_ms, double *aux_ms, int *n_launches, const char **kernel);
/* The number of the entry-point call issued last on this context (1, 2, ...; calls made by the library itself while it
 * completes another one are not counted), and the same statistics looked up by that number once the call has
 * completed — how a caller with several calls in flight finds the times of each. */
long long mdhip_last_ticket(mdhip_ctx *ctx);
int mdhip_ticket_stats(mdhip_ctx *ctx, long long ticket, double *kernel_ms, double *aux_ms, int *n_launches,
                       const char **kernel);
/* What the COMPLETION of call `ticket` returned: 0, or the negative code of its failure (text: mdhip_last_error) —
 * whoever completed it (its own mdhip_wait, a later mdhip_sync, a synchronous call that drained it). MDHIP_EPENDING
 * while it is in flight, MDHIP_EUNKNOWN for a number more than 64 completed calls old (the context's error text is left as it is: MDHIP_EINVAL
 * can be the completion status of the call itself). An error handed out here is no
 * longer reported by a later mdhip_sync / mdhip_wait. *n_fallbacks (may be NULL): slow-path repeats the call took —
 * the staged full-lag MSD kernel's ring timed out (grid not resident as a whole: a co-tenant on the GPU) and the
 * call was repeated over a transposed copy — results are the same, the call took seconds instead of milliseconds.
 * The wrapper warns when it is non-zero. */
int mdhip_ticket_status(mdhip_ctx *ctx, long long ticket, int *n_fallbacks);
/* Slow-path repeats (see mdhip_ticket_status) since the context was created. */
long long mdhip_fallbacks(mdhip_ctx *ctx);
/* Device time (ms, hipEvent pair on the call's launch stream) of the dominant kernel of the last call,
 * and the number of times that kernel was launched by that call. Each call's time is taken from its own events:
 * launches of two pair calls that overlap share the machine, so the per-call times of a pipeline may add up to more
 * than the wall time it took. */
double mdhip_last_kernel_ms(mdhip_ctx *ctx, int *n_launches);
/* Device time (ms) of the preparation kernels of the last call that are not part of the dominant kernel
 * (the spatial sort / tile lists of the culled pair path); 0 when there were none. */
double mdhip_last_aux_ms(mdhip_ctx *ctx);
/* Name of the dominant kernel the last call launched (as rocprofv3 lists it, without the namespace), "" if none. */
const char *mdhip_last_kernel_name(mdhip_ctx *ctx);
/* Estimated relative rounding-error bound of the last mdhip_lag_msd call when it was answered by the FFT
 * path (lag_variant 2 or 3); 0 when the exact-difference kernel answered. */
double mdhip_last_rel_bound(mdhip_ctx *ctx);
/* Identity of the BUILD: sha256 (first 16 hex digits) of the sources the library was compiled from, as the build
 * recipe computed it (mdproptools_amd/build.py); "unknown" for a library built by other means. bench.py prints it. */
const char *mdhip_build_id(void);
/* Writes the device name (e.g. "gfx950...") into buf. */
int mdhip_device_name(mdhip_ctx *ctx, char *buf, int buflen);
/* Kernel organisation knobs, for A/B measurements only; results never depend on them. Keys:
 *   "rdf_variant"  1 fast pair kernels (default), 0 edge-table lookup per pair
 *   "rdf_cull"     -1 auto, 0 dense sweep, 1 spatially culled sweep (when applicable)
 *   "rdf_sj"       culled sweep: 1 scalar-j kernel (default), 2 the same without the persistent grid,
 *                  0 LDS-tile kernel
 *   "rdf_rows"     scalar-j RDF: -1/1 ordered-pair rows without a class-row table when they fit LDS, 0 class rows
 *   "rdf_pk"       scalar-j RDF with ordered rows: -1/1 packed-f32 classification of the pairs (two per VALU
 *                  instruction) with every pair inside the error band of a bin edge or of the cutoff resolved by
 *                  the exact f64 chain (default whenever the band is narrow enough; ordered rows when they fit LDS,
 *                  else class rows with their row table), 0 all-f64 sweep
 *   "rdf_sort"     spatial sort: -1 auto, 1 one block per frame (LDS counters), 0 multi-block (global counters), 3 as
 *                  auto without the read-once form for frames of <= 12288 atoms
 *   "rdf_inflight" per-frame output: frames in flight per XCD
 *   "rdf_jsplit", "rdf_fpb", "rdf_batch", "rdf_slots"  launch geometry of the pair kernels
 *   "lag_variant"  full-lag MSD: 3 / -1 (default) = autocorrelation theorem (O(F log F)) when the relative error
 *                  bound it computes for the data (mdhip_last_rel_bound) is <= 1e-10, else the exact-difference
 *                  kernel; 1 = always the series-resident difference kernel, 0 = staged difference kernel,
 *                  2 = always the autocorrelation theorem (the one knob that changes results, within that bound)
 *   "lag_fft_kernel" fused full-lag MSD kernel: 3 (default) the 12288-point kernel (radix-12 first pass, twelve waves each a
 *                  512-point transform in registers) where 3072 <= F and F + max_lag <= 12288, else as 2; 2 first pass
 *                  from registers + wave-private sub-transforms of a power-of-two length where the series is long
 *                  enough, 1 block-wide passes, 0 the round-2 kernel (results agree within the bound)
 *   "xcorr_tile"   time slabs of the direct correlation kernel
 *   "fft_logr", "fft_logc"  FFT correlation: largest radix of a pass (log2, default 10) and columns per tile of the
 *                  radix-4 network; "fft_net8" 1 (default) radix-8 network for passes of radix >= 2^9, 0 off, 2 one
 *                  workgroup per CU; "fft_specfuse" 1 (default) spectrum step inside the inverse's first pass;
 *                  "fft_mid" 1 (default) an autocorrelation through a two-pass transform runs in three launches (second
 *                  pass + spectrum step + inverse's first pass in one), 0 four, 2 three with narrower tiles
 *   "seg_frame"    segment COM / flux: 1 (default) one (run, frame) per block, 0 the software-pipelined staged kernel;
 *                  "seg_cap", "seg_vec", "seg_gy" geometry of the staged kernel
 *   "h2d_overlap"  host-resident frames: 1 (default) staged batch by batch under the sweeps, 0 copied first;
 *                  "h2d_ring" 1 (default) pageable sources go through a page-locked ring filled by helper threads
 *   "small_copy"   1 (default) copies of <= 256 KB between page-locked host memory and the device are made by a kernel
 *                  on the launch stream, 0 by hipMemcpyAsync (a blit on another hardware queue)
 *   "rdf_guard", "cn_pk"  overflow guard / coordination counts through the packed sweep ("rdf_relblock": retired in
 *                  round 4, accepted and ignored — the f32 records are relative to their whole tile's centre)
 *   "lag_direct"   fused full-lag MSD path: -1 default (= 2), 0 transposed copy made by a pass of its own, 1 the kernel reads
 *                  the trajectory in place, 2 clusters of 16 workgroups transpose their tiles inside the kernel (results of
 *                  the three agree within the reported bound)
 *   "free_volume_batch"  mdhip_free_volume: frames per batch; 0 (default) what its workspace budget holds
 *   "sync_spin"    waiting for device work: 1 (default) poll the completion event (no interrupt wake-up latency; turns
 *                  into a blocking wait after 100 ms), 0 block at once */
int mdhip_set_option(mdhip_ctx *ctx, const char *key, int value);

/* ---- Non-finite input ("NaN stays home") ------------------------------------------------------ */
/*
 * A run that blew up writes nan, -nan and inf into its dump; the reader passes them on (strtod) and no entry point
 * refuses a non-finite coordinate or sample, as the reference does not. What comes out is defined, per family
 * (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite.py):
 *
 *   Pair counts — RDF, CN, RDF + CN in one sweep, atoms x sites, shell residence, shell members, shell coordination,
 *   contact components, angles, hydration, distinct van Hove (its pairs land in `beyond`). rdf_cn.py:36-69: a non-finite difference leaves rsq at NaN or +inf and
 *   rsq < r_cut^2 false, so the pair is in no cutoff; every pair without such an atom counts as before. The integers of
 *   a frame with K poisoned atoms are those of the frame with the K atoms deleted. This holds on every route: the
 *   spatial sort clamps its keys in the integer domain (a non-finite atom lands in cell 0), bounding boxes leave NaN out
 *   (fmin / fmax) and become unbounded for +-Inf or 1e300 — such a tile is never culled, and the packed-f32 sweep hands
 *   it to its exact f64 chain ("not covered") —, and every bin index is formed under rsq < r_cut^2 only. A finite
 *   coordinate of 1e300 behaves the same (rsq overflows to +inf) except towards an atom at the same value.
 *
 *   Sums — segment COM, charge flux, msd_pairs / origin / windows, lag_msd, correlations, integrals. A non-finite value
 *   enters exactly the sums the value enters in plain numpy, and no others: its segment's COM on its plane in its frame
 *   (its type's flux component); its entity's row, its group's sum on its axis and the total, at the pairs, frames and
 *   windows that touch its frame; every other output is bit-identical to the call on clean data.
 *     lag_msd, difference kernels (lag_variant 0, 1): a sample at frame t* makes the lags k <= max(t*, F - 1 - t*) of its
 *       (group, axis) and of that group's total non-finite, nothing else.
 *     lag_msd, spectral paths forced (lag_variant 2, 4): the transform spreads the sample over every lag, so the affected
 *       (group, axis) column and its total may be NaN THROUGHOUT (lag 0 stays 0); every other column keeps its bound. The
 *       reported bound (mdhip_last_rel_bound, mdhip_lag_msd_status_dev) is +infinity: there is none.
 *     lag_msd, default (lag_variant 3): +infinity misses the 1e-10 bound like any other, so the call is answered by the
 *       difference kernel and the whole result is the difference kernel's.
 *     xcorr, direct: the non-finite lags are those of the plain sums c[k] = sum_t a[t+k] b[t] (a sample of b at t reaches
 *       the lags k < n - t, a sample of a at t the lags k <= t); a row with a non-finite lag is summed once more, every
 *       lag over its own range in time order (the sweep's zero padding times a NaN would reach the other lags too). The
 *       other series of the batch are bit-identical. xcorr, FFT: the poisoned row is non-finite at every lag, as
 *       numpy's rfft / irfft of such a series is; the other rows are bit-identical.
 *     cumtrapz: I[k] is non-finite from the first increment that holds the bad sample on, +-Inf or NaN as a sequential
 *       cumsum of the increments gives (a finite series whose running sum overflows included); the integrals before it,
 *       and the series after it in the batch, are untouched. green_kubo is the chain of the separate calls, masks
 *       included.
 *     velocity_spectrum: as xcorr through the FFT — a non-finite sample of an entity of group g on axis a makes
 *       sums[.][g][a], power[g][a][.], a0[g][a] and that group's totals non-finite THROUGHOUT; every other output is
 *       bit-identical to the call on clean data. An entity of group -1 is never read into a sum, whatever it holds.
 *
 * Not covered: NaN in box lengths, types or masses.
 */

/* ---- R2/R3 binning table ------------------------------------------------ */
/*
 * Exact bin edges of the reference's binning rule
 *     bin = (int64) ( sqrt(rsq) / bin_size )           structural/rdf_cn.py:68,85
 * edges[k] = the smallest double rsq whose bin is >= k, k = 0..nbins (edges[0] = 0).
 * Found by bisection on the bit pattern with IEEE sqrt and divide, so that
 * binning on the device is a pure comparison of rsq against this table and
 * never depends on device sqrt/div rounding. `edges` has nbins+1 entries.
 */
int mdhip_bin_edges(double bin_size, int nbins, double *edges);
/*
 * Bound (in bins) on |g32 - sqrt(rsq_ref)/bin_size - addend| of the packed-f32 bin guess the pair kernel uses to
 * classify pairs: coordinates relative to a tile centre with |xr_i| + |xr_j| <= s_cap per axis, boxes up
 * to l_max, n_rows histogram rows of nbins+1 words riding in the guess. Pairs whose guess is within twice this bound
 * (plus slack) of an integer are resolved by the exact f64 chain instead. Exposed so that the bound can be checked
 * against an emulation of the f32 chain (tests/test_abi_cpu.py); a pure function, no device needed.
 */
double mdhip_pk_error_bound(double r_cut, double bin_size, int nbins, int n_rows, double s_cap, double l_max);

/*
 * Row layout of the table-free ("ordered rows") sweep when the plain n_ti x n_tj rows do not fit LDS:
 * integers a[n_ti], b[n_tj] such that row(ti, tj) = a[ti] + b[tj] never holds two type pairs of different classes
 * (cls[ti * n_tj + tj] >= 0: the class of the ordered pair), with *n_rows = max a + max b + 1 < n_ti * n_tj rows and
 * row_cls[row] the class of every row (-1: unused; at least n_ti * n_tj entries). *n_rows = 0: no layout with fewer
 * rows than the plain one was found (a, b, row_cls untouched). Exposed so that the layout's defining property can be
 * checked without a device (tests/test_abi_cpu.py); a pure function, deterministic.
 */
int mdhip_row_displacement(int n_ti, int n_tj, const int32_t *cls, int32_t *a, int32_t *b, int32_t *row_cls,
                           int *n_rows);

/*
 * What a pair call would launch, decided from its shape alone: the library's own plan function (the one every
 * mdhip_rdf_* / mdhip_cn_* call runs before it stages anything) behind the same label -> class -> row-displacement
 * steps, with no device. ctx: NULL (the defaults of a fresh context), or a context whose options and device limits
 * are read (never changed). op: MDHIP_PLAN_RDF (mdhip_rdf_atomic[_dev] / mdhip_rdf_sites), MDHIP_PLAN_CN
 * (mdhip_cn_atomic / mdhip_cn_sites), MDHIP_PLAN_RDF_CN (mdhip_rdf_cn_atomic); a synchronous call.
 *   type [n_type], site_type [n_site_type]   labels: the type column, or just every label that occurs in it;
 *                      site_type NULL: atom-atom, else atoms x sites with n_sites sites
 *   box                host [n_frames][3]
 *   cn_r_cut_sq        [n_rel] for the two CN ops (r_cut_sq, bin_size, nbins are ignored by MDHIP_PLAN_CN), else NULL
 *   result_on_device   1: the frame-summed RDF stays on the device (mdhip_rdf_atomic_dev)
 *   xyz_on_device      0: host-resident frames, staged batch by batch (counts in the launches)
 *   cu_count, lds_bytes   the two device limits the decision reads (<= 0: the context's; 256 / 65536 without one)
 *   opt_key, opt_value [n_opt] overrides as for mdhip_set_option
 * Out: info[8] = { status, scalar-j mode (-1: an LDS-tile kernel; see sj_kernel in csrc/pair_common.h), class passes
 * per batch, pair-kernel launches of the whole call, ordered rows (0: class rows), rows displaced, BIG block,
 * packed-f32 sweep }; status MDHIP_OK, MDHIP_PLAN_TWO_SWEEPS (an RDF + CN call that takes two sweeps: the RDF sweep is
 * the one described) or a negative MDHIP_E* code. text: the kernel's name as mdhip_last_kernel_name reports it (first
 * batch), or the error text. Returns MDHIP_EINVAL for unusable arguments, else MDHIP_OK. A pure function, deterministic.
 */
#define MDHIP_PLAN_RDF 0
#define MDHIP_PLAN_CN 1
#define MDHIP_PLAN_RDF_CN 2
#define MDHIP_PLAN_TWO_SWEEPS 1
int mdhip_pair_plan(const mdhip_ctx *ctx, int op, int64_t n_frames, int64_t n_atoms, const int32_t *type, int64_t n_type,
                    int64_t n_sites, const int32_t *site_type, int64_t n_site_type, const double *box, int n_rel,
                    const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *cn_r_cut_sq, int per_frame,
                    int result_on_device, int xyz_on_device, int cu_count, int64_t lds_bytes, int n_opt,
                    const char *const *opt_key, const int *opt_value, char *text, int text_cap, int32_t *info);

/*
 * What a full-lag MSD call (mdhip_lag_msd*, lag_variant 2 .. 4) would run on its spectral path, decided from its shape
 * alone: the library's own decision (csrc/lag_plan.h: lag_choose, the function every such call runs first), with no
 * device. ctx: NULL (the defaults of a fresh context), or a context whose options and device limits are read (never
 * changed).
 *   group_off          host [n_groups + 1], as mdhip_lag_msd
 *   r_aligned16        the trajectory's device address is a multiple of 16 (host-resident frames are staged: 1)
 *   cu_count, lds_bytes   the two device limits the decision reads (<= 0: the context's; 256 / 65536 without one)
 *   opt_key, opt_value [n_opt] overrides as for mdhip_set_option
 * Out: info[MDHIP_LAG_PLAN_INFO] = { status, path (MDHIP_LAG_*; -1: nothing runs, or the exact kernels answer),
 *   generation of the power-of-two kernel (1 .. 3) | padded length / 1024 of the one-wave kernel | D of the residue
 *   classes (4, 8) | fuse level of the batched transforms (0 .. 2),
 *   m (fused paths: log2 of the packed points at or above (n_frames + max_lag) / 2),
 *   source of the series (0 the transposed copy, 1 the trajectory in place, 2 / 3 the clusters' staging rings),
 *   rows per cluster member, staging units per lane and tile (0: not staged),
 *   template instance, first parameter (12 288-point kernel: QE; generation 3: JJ; 2: QR2; 1: QR; residue paths: 1 .. 3
 *   msd_power_w1_kernel<n>, 4 msd_power_w12r_kernel<4>, 5 msd_power_w12p_kernel<true>, 6 <false> + msd_power_w12o_kernel),
 *   second parameter (12 288-point kernel: SHORT; generation 3: QE; residue paths: packed),
 *   work items (blocks of the power kernel, all batches), batches of series, timed runs of launches as
 *   mdhip_last_kernel_ms counts them, padded length }; status MDHIP_OK or a negative MDHIP_E* code.
 * text: the name mdhip_last_kernel_name reports after the call, or the error text. The completion step of a call may
 * still hand the answer to the exact kernels (lag_variant 3 with the bound missed) and leave their name. Returns
 * MDHIP_EINVAL for unusable arguments, else MDHIP_OK. A pure function, deterministic.
 */
#define MDHIP_LAG_W1 0
#define MDHIP_LAG_POW2 1
#define MDHIP_LAG_W12 2
#define MDHIP_LAG_RESIDUE 3
#define MDHIP_LAG_BATCHED 4
#define MDHIP_LAG_PLAN_INFO 13
int mdhip_lag_plan(const mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, int max_lag, int n_groups,
                   const int64_t *group_off, int r_aligned16, int cu_count, int64_t lds_bytes, int n_opt,
                   const char *const *opt_key, const int *opt_value, char *text, int text_cap, int32_t *info);

/* ---- R3: _rdf_loop (+ _calc_rsq, _remove_outliers) ------------------------ */
/*
 * structural/rdf_cn.py:72-97 for n_frames frames at once.
 *   xyz        host|dev [n_frames][3][n_atoms]  SoA planes, atoms sorted by id
 *   type       host int32 [n_atoms] labels as in the dump (or altered ids, rdf_cn.py:197-215);
 *              type_frame_stride = 0 when shared by all frames, n_atoms when per frame
 *   box        host [n_frames][3] edge lengths lx, ly, lz (rdf_cn.py:80)
 *   rel        host int32 [n_rel][2] = relation_matrix (rdf_cn.py:484)
 *   r_cut_sq   the value the reference compares against, r_cut**2 (rdf_cn.py:66)
 *   edges      host [nbins+1] from mdhip_bin_edges, or NULL to have it computed from bin_size
 *   hist_full  host uint64 [n_frames][nbins] (per_frame=1) or [nbins] summed over frames (per_frame=0);
 *              +2 per in-cutoff pair (rdf_cn.py:85-86)
 *   hist_part  host uint64 [n_frames][n_rel][nbins] or [n_rel][nbins]; +1 per (head a, other b) and per
 *              (head b, other a) (rdf_cn.py:87-96)
 *   overflow   host uint64 [1]: in-cutoff pairs whose bin index is >= nbins. The reference indexes out of
 *              bounds for them; here they are dropped and counted.
 * Semantics per pair (i < j): d = head - other; one shift by -sign(d)*L iff |d| > L/2;
 * rsq = (dx*dx + dy*dy) + dz*dz with no fused multiply-add; keep iff rsq < r_cut_sq.
 */
int mdhip_rdf_atomic(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                     int on_device, const int32_t *type, int64_t type_frame_stride,
                     const double *box, int n_rel, const int32_t *rel, double r_cut_sq,
                     double bin_size, int nbins, const double *edges, int per_frame,
                     uint64_t *hist_full, uint64_t *hist_part, uint64_t *overflow);

/*
 * The frame-summed form of mdhip_rdf_atomic (per_frame = 0) with the sums left ON THE DEVICE, for the multi-GPU
 * path: frames shard over one process per GPU and the (1 + n_rel) * nbins + 1 words are all-reduced over RCCL
 * straight from this buffer (mdproptools_amd/dist.py), no host round trip.
 *   out_dev    DEVICE uint64 [(1 + n_rel) * nbins + 1] = hist_full | hist_part | overflow (overwritten)
 * Complete (stream synchronised) on return, like every other call.
 */
int mdhip_rdf_atomic_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                         const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                         const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                         uint64_t *out_dev);

int mdhip_rdf_atomic_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                           const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                           const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                           int per_frame, uint64_t *hist_full, uint64_t *hist_part, uint64_t *overflow);
int mdhip_rdf_atomic_dev_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                               const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                               const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                               uint64_t *out_dev);

/* ---- R4: _cn_loop --------------------------------------------------------- */
/*
 * structural/rdf_cn.py:100-119: cn[kl] += #pairs(rsq < r_cut_sq[kl]) with the same a/b double test;
 * every relation has its own cutoff. cn: host uint64 [n_frames][n_rel] or [n_rel].
 */
int mdhip_cn_atomic(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                    int on_device, const int32_t *type, int64_t type_frame_stride,
                    const double *box, int n_rel, const int32_t *rel, const double *r_cut_sq,
                    int per_frame, uint64_t *cn);

/* mdhip_cn_atomic with per_frame = 0 and the n_rel counts written to a DEVICE buffer (all-reduced over RCCL by
 * mdproptools_amd/dist.py: cn_sharded). cn_dev: device uint64 [n_rel]. */
int mdhip_cn_atomic_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                        const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                        const int32_t *rel, const double *r_cut_sq, uint64_t *cn_dev);

/* cn: host [n_frames][n_rel] / [n_rel], or (cn_on_device, per_frame = 0) device [n_rel]. */
int mdhip_cn_atomic_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                          const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                          const int32_t *rel, const double *r_cut_sq, int per_frame, uint64_t *cn, int cn_on_device);

/* ---- R3 + R4 in one sweep ------------------------------------------------------------------ */
/*
 * calc_atomic_rdf and calc_atomic_cn walk the same pairs of the same frames (structural/rdf_cn.py:385-530 and
 * 533-651; BASELINE config 3 asks for both): this call returns the outputs of mdhip_rdf_atomic AND of mdhip_cn_atomic
 * from ONE sweep. The packed-f32 sweep sends every pair that can lie inside the largest coordination cutoff to the
 * exact f64 chain, which bins it and counts it below the cutoffs it is below — the integers are those of the two
 * separate calls. cn_r_cut_sq host [n_rel] (each <= r_cut_sq for the single sweep; otherwise, and for geometries the
 * packed sweep does not cover, the two sweeps run one after the other inside this call).
 */
int mdhip_rdf_cn_atomic(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                        const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                        const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                        const double *cn_r_cut_sq, int per_frame, uint64_t *hist_full, uint64_t *hist_part,
                        uint64_t *overflow, uint64_t *cn);

int mdhip_rdf_cn_atomic_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                              const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                              const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                              const double *cn_r_cut_sq, int per_frame, uint64_t *hist_full, uint64_t *hist_part,
                              uint64_t *overflow, uint64_t *cn);

/* ---- R5: _rdf_mol_loop / _cn_mol_loop (atoms x sites, rectangular) --------- */
/*
 * structural/rdf_cn.py:122-141 and 144-162. Sites are molecule centres of mass
 * (or any second coordinate set): sites host|dev [n_frames][3][n_sites],
 * site_type host int32 [n_sites] (molecule type labels, shared by all frames).
 * +1 per in-cutoff (atom of type rel[kl][0], site of type rel[kl][1]); an atom's
 * own molecule is not excluded. hist_part / cn as above (no hist_full).
 */
int mdhip_rdf_sites(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                    int xyz_on_device, const int32_t *type, int64_t n_sites, const double *sites,
                    int sites_on_device, const int32_t *site_type, const double *box, int n_rel,
                    const int32_t *rel, double r_cut_sq, double bin_size, int nbins,
                    const double *edges, int per_frame, uint64_t *hist_part, uint64_t *overflow);

int mdhip_cn_sites(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                   int xyz_on_device, const int32_t *type, int64_t n_sites, const double *sites,
                   int sites_on_device, const int32_t *site_type, const double *box, int n_rel,
                   const int32_t *rel, const double *r_cut_sq, int per_frame, uint64_t *cn);

/* ---- R6 / M3: per-molecule centre of mass ---------------------------------- */
/*
 * structural/rdf_cn.py:218-241 (_define_mol_cols), common/com_mols.py:58-60 (calc_com),
 * dynamical/diffusion.py:83-89: mass-weighted mean over contiguous atom runs.
 *   attr       host|dev [n_frames][n_attr][n_atoms]
 *   atom_mass  host [n_atoms]; atom_q host [n_atoms] or NULL
 *   seg_off    host int64 [n_seg+1] (atoms of segment s are seg_off[s]..seg_off[s+1]-1)
 *   out        host|dev (out_on_device) [n_frames][n_attr][n_seg]:  sum(m*a) / sum(m), each product
 *              and sum a separate rounding, atoms added in index order
 *   seg_mass   host [n_seg] or NULL; seg_q host [n_seg] or NULL (sum of atom_q), index order from 0.0
 * Floating point: sums are in a different order from pandas' Kahan group sum / BLAS dot; agreement with
 * the reference is to ~1e-15 relative (tests use rtol 1e-13). Every kernel variant and option setting gives the bits
 * of the order stated above (tests/test_gpu_segment_exact.py).
 */
int mdhip_segment_com(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, int n_attr,
                      const double *attr, int attr_on_device, const double *atom_mass,
                      const double *atom_q, int64_t n_seg, const int64_t *seg_off, double *out,
                      int out_on_device, double *seg_mass, double *seg_q);

int mdhip_segment_com_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, int n_attr, const double *attr,
                            int attr_on_device, const double *atom_mass, const double *atom_q, int64_t n_seg,
                            const int64_t *seg_off, double *out, int out_on_device, double *seg_mass, double *seg_q);

/* ---- M1 / M2: frame-pair displacement reductions --------------------------- */
/*
 * dynamical/diffusion.py:212-218 and 225-237 as one primitive over a list of frame pairs.
 *   r          host|dev [n_frames][3][n_ent] entity coordinates (atoms or molecule COMs)
 *   scale      unit factor applied to every coordinate first (r*scale, diffusion.py:201-203)
 *   pairs      host int32 [n_pairs][2] = (t0, t1); M1 is {(0,t)}, M2 is {((k-1)tao, k tao)}
 *   group_off  host int64 [n_groups+1] contiguous entity groups (molecule types; one group for atoms)
 *   sums       host [n_pairs][n_groups][4]: sum over the group's entities of dx2, dy2, dz2 and
 *              (dx2+dy2)+dz2 (the caller divides by the group size: diffusion.py:218)
 *   per_entity host|dev (pe_on_device) [n_pairs][n_ent][4] = msd_all rows, or NULL
 * Tolerance vs the reference: rtol 1e-10 on means (fixed-order tree sums vs pandas' compensated sums).
 * Any number of pairs (n_pairs * n_groups * 4 < 2^31): a launch covers at most 65535 pairs (grid.y), so longer lists
 * run as several launches of one call. A pair's sums and rows are the same bits whichever launch computes it.
 * This holds for every msd_pairs / msd_origin entry point below and their _async twins (one ticket per call).
 */
int mdhip_msd_pairs(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r,
                    int on_device, double scale, int n_pairs, const int32_t *pairs, int n_groups,
                    const int64_t *group_off, double *sums, double *per_entity, int pe_on_device);

/*
 * M1 for a FRAME SHARD (dynamical/diffusion.py:212-218 when the frames are dealt to one process per GPU): every frame
 * t of r against ONE origin frame that need not be among them — the frame at time 0, broadcast by the rank that owns
 * it — i.e. the frame pairs {(origin, t)}, t = 0..n_frames-1. Any number of frames, as mdhip_msd_pairs.
 *   origin     host|dev (origin_on_device) [3][n_ent]
 *   sums       host|dev (sums_on_device) [n_frames][n_groups][4]
 *   cols       NULL, or host|dev (cols_on_device) the four per-entity columns as in mdhip_msd_pairs_cols
 */
int mdhip_msd_origin(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device,
                     const double *origin, int origin_on_device, double scale, int n_groups,
                     const int64_t *group_off, double *sums, int sums_on_device, double *cols, int64_t col_stride,
                     int cols_on_device);

/* mdhip_msd_pairs without per-entity rows and with the sums left in a DEVICE buffer [n_pairs][n_groups][4]: a rank's
 * frame shard of the single-origin MSD, all-gathered over RCCL from there (dist.py: msd_single_origin_sharded;
 * reference: dynamical/diffusion.py:212-218). */
int mdhip_msd_pairs_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device, double scale,
                        int n_pairs, const int32_t *pairs, int n_groups, const int64_t *group_off, double *sums_dev);

/*
 * The same reduction with the per-entity values stored as COLUMNS: dx2, dy2, dz2, msd, each [n_pairs][n_ent],
 * column k at cols + k * col_stride (col_stride >= n_pairs * n_ent, in doubles). These are the column blocks the
 * `msd_all` DataFrame (diffusion.py:212-217, 222) is made of, so the caller wraps them without a transpose.
 *   cols       host|dev (cols_on_device)
 */
int mdhip_msd_pairs_cols(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r,
                         int on_device, double scale, int n_pairs, const int32_t *pairs, int n_groups,
                         const int64_t *group_off, double *sums, double *cols, int64_t col_stride,
                         int cols_on_device);

/*
 * dynamical/diffusion.py:225-237 per entity: frames kept = 0, tao, 2 tao, ...; for every entity the
 * sums over the n_kept-1 windows of (x_k - x_{k-1})^2 per axis and of their total.
 *   win_sums   host [n_ent][4] (the caller applies /(n_kept-1) and, for the total, /n_kept — the
 *              reference's NaN-row quirk)
 */
int mdhip_msd_windows(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r,
                      int on_device, double scale, int tao, double *win_sums);

/* The same with win_sums in a DEVICE buffer [n_ent][4] (a rank's windows of the fixed-lag MSD, all-reduced over RCCL). */
int mdhip_msd_windows_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device,
                          double scale, int tao, double *win_sums_dev);

/*
 * Superset (not in the reference): full lag average
 *   msd[lag][g][c] = mean over t0 in [0, n_frames-lag) and entities of group g of the squared
 *   displacement, c = x, y, z, total; lag = 0..max_lag.   out host [max_lag+1][n_groups][4]
 * Tolerance: rtol 1e-10 against the plain double sum. The default evaluates S1(k) - 2 S2(k) with S2 from the power
 * spectrum (O(F log F)) whenever the rounding bound it computes for the data is <= 1e-10 relative to the MSD
 * (mdhip_last_rel_bound reports it); otherwise — e.g. coordinates far from the origin against a small displacement —
 * the difference kernel sums (r(t0+k) - r(t0))^2 directly. A NaN / Inf sample (or squares that overflow) gives a bound of
 * +infinity, i.e. the difference kernel by default; with lag_variant 2 / 4 its (group, axis) column and that group's total
 * may be NaN at every lag ("Non-finite input" above).
 */
int mdhip_lag_msd(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device,
                  double scale, int max_lag, int n_groups, const int64_t *group_off, double *out);

/* The same with the means in a DEVICE buffer [max_lag+1][n_groups][4] (a rank's entity slice; dist.py: lag_msd_sharded
 * turns them into sums on the device and all-reduces them). */
int mdhip_lag_msd_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device,
                      double scale, int max_lag, int n_groups, const int64_t *group_off, double *out_dev);

/* Asynchronous twins of the MSD calls of a sharded step (dist.py issues them back to back and waits once):
 * mdhip_msd_origin, mdhip_msd_pairs_dev, mdhip_msd_windows[_dev] (out_on_device), mdhip_lag_msd[_dev] (out_on_device;
 * the spectral path's bound check and its fallback to the difference kernel happen at completion). */
int mdhip_msd_origin_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device,
                           const double *origin, int origin_on_device, double scale, int n_groups,
                           const int64_t *group_off, double *sums, int sums_on_device, double *cols, int64_t col_stride,
                           int cols_on_device);
int mdhip_msd_pairs_dev_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device,
                              double scale, int n_pairs, const int32_t *pairs, int n_groups, const int64_t *group_off,
                              double *sums_dev);
int mdhip_msd_windows_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device,
                            double scale, int tao, double *win_sums, int out_on_device);
int mdhip_lag_msd_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int on_device, double scale,
                        int max_lag, int n_groups, const int64_t *group_off, double *out, int out_on_device);
/* The STATUS of the mdhip_lag_msd* call issued last on this context, as one number in DEVICE memory, copied to
 * *dst_dev on the context's stream (behind that call's kernels, no host wait): the relative error bound of the spectral
 * path (what mdhip_last_rel_bound returns once the call has completed), +infinity when the in-kernel transposition of
 * that path did not complete (its result is then rewritten when the call completes), 0 when the exact-difference
 * kernel answered. The multi-GPU step adds this word to the buffer it all-reduces: every rank then knows, from the
 * reduced value alone, whether the lag sums have to be redone — without a host wait between the kernels and the
 * collective (mdproptools_amd/dist.py: msd_step_sharded_async). */
int mdhip_lag_msd_status_dev(mdhip_ctx *ctx, double *dst_dev);

/* ---- G1: per-frame charge flux --------------------------------------------- */
/*
 * dynamical/_conductivity.py:11-35: J[k][type] = sum over molecules of that type of
 * q_mol * v_com,k with v_com = sum(m v)/sum(m), both converted to SI first.
 *   vel        host|dev [n_frames][3][n_atoms]; atom_mass, atom_q host [n_atoms]
 *   seg_off    host int64 [n_seg+1]; seg_type host int32 [n_seg] in 0..n_types-1
 *   flux       host [3][n_types][n_frames] (the layout Conductivity.get_charge_flux returns)
 * Floating point: per molecule ((sum(m v) / sum(m)) * vel_conv) * (sum(q) * charge_conv), the sums as in
 * mdhip_segment_com; then per type 256 partial sums, partial i adding molecules i, i + 256, ... of the type in order,
 * and a fixed tree over them (red[i] += red[i + w], w = 128 .. 1). Every kernel variant and option setting gives these
 * bits (tests/test_gpu_segment_exact.py).
 */
int mdhip_charge_flux(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *vel,
                      int on_device, const double *atom_mass, const double *atom_q, int64_t n_seg,
                      const int64_t *seg_off, const int32_t *seg_type, int n_types,
                      double vel_conv, double charge_conv, double *flux);

/* The same with flux in a DEVICE buffer [3][n_types][n_frames] (a rank's frames; all-gathered over RCCL — the reference's
 * only frame-parallel gather, dynamical/conductivity.py:190-194). */
int mdhip_charge_flux_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *vel,
                          int on_device, const double *atom_mass, const double *atom_q, int64_t n_seg,
                          const int64_t *seg_off, const int32_t *seg_type, int n_types,
                          double vel_conv, double charge_conv, double *flux_dev);

int mdhip_charge_flux_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *vel, int on_device,
                            const double *atom_mass, const double *atom_q, int64_t n_seg, const int64_t *seg_off,
                            const int32_t *seg_type, int n_types, double vel_conv, double charge_conv, double *flux,
                            int flux_on_device);

/* ---- G2 / G3: correlation functions ---------------------------------------- */
#define MDHIP_XCORR_FFT 0    /* zero-padded FFT (reference: length 2n; here the next power of two >= 2n, same linear correlation): conductivity.py:109-114, viscosity.py:111-115 */
#define MDHIP_XCORR_DIRECT 1 /* direct lag sums:           viscosity.py:103-108 ("brute_force")        */
/*
 * out[p][k] = sum_{t=0}^{n-1-k} a_p[t+k] * b_p[t] / (n-k),  k = 0..n_lags-1, for n_pairs series pairs.
 *   a, b       host|dev [n_pairs][n] (b == a for an autocorrelation)
 *   out        host [n_pairs][n_lags]
 * Tolerance vs the reference: |err| <= 1e-10 * out[p][0].
 */
int mdhip_xcorr(mdhip_ctx *ctx, int64_t n, int n_pairs, const double *a, const double *b,
                int on_device, int method, int64_t n_lags, double *out);

/*
 * The lags lag_begin .. lag_begin + n_lags - 1 only (out host [n_pairs][n_lags]): the unit of the multi-GPU split of
 * the direct estimator, whose cost per lag k is n - k products — every GPU owns a lag range and needs the whole
 * series (mdproptools_amd/dist.py: xcorr_direct_sharded). Direct method only unless lag_begin == 0.
 */
int mdhip_xcorr_lags(mdhip_ctx *ctx, int64_t n, int n_pairs, const double *a, const double *b, int on_device,
                     int method, int64_t lag_begin, int64_t n_lags, double *out);

/* The same with out in a DEVICE buffer [n_pairs][n_lags] (a rank's lag range, all-gathered over RCCL). */
int mdhip_xcorr_lags_dev(mdhip_ctx *ctx, int64_t n, int n_pairs, const double *a, const double *b, int on_device,
                         int method, int64_t lag_begin, int64_t n_lags, double *out_dev);

int mdhip_xcorr_async(mdhip_ctx *ctx, int64_t n, int n_pairs, const double *a, const double *b, int on_device,
                      int method, int64_t n_lags, double *out);
int mdhip_xcorr_lags_dev_async(mdhip_ctx *ctx, int64_t n, int n_pairs, const double *a, const double *b, int on_device,
                               int method, int64_t lag_begin, int64_t n_lags, double *out_dev);

/* ---- G4: cumulative trapezoid ---------------------------------------------- */
/*
 * dynamical/viscosity.py:151 (cumtrapz) and conductivity.py:231 (cumulative_trapezoid):
 * I[k] = sum_{m<k} dx*(y[m]+y[m+1])/2. y host|dev [n_series][n];
 * out host [n_series][n-1], or [n_series][n] with a leading 0 when leading_zero != 0.
 * At most 65535 series per call: more fail with MDHIP_EINVAL before anything is written. The same limit holds for
 * mdhip_green_kubo* (tests/test_gpu_launch_limits.py).
 */
int mdhip_cumtrapz(mdhip_ctx *ctx, int64_t n, int n_series, const double *y, int on_device,
                   double dx, int leading_zero, double *out);

/* The same with out in a DEVICE buffer [n_series][n-1 (+1)] (the running integral stays on the GPU). */
int mdhip_cumtrapz_dev(mdhip_ctx *ctx, int64_t n, int n_series, const double *y, int on_device, double dx,
                       int leading_zero, double *out_dev);
int mdhip_cumtrapz_async(mdhip_ctx *ctx, int64_t n, int n_series, const double *y, int on_device, double dx,
                         int leading_zero, double *out);
int mdhip_cumtrapz_dev_async(mdhip_ctx *ctx, int64_t n, int n_series, const double *y, int on_device, double dx,
                             int leading_zero, double *out_dev);

/* ---- G3 -> G4 in one call: the Green-Kubo chain without leaving the device ------------------------------------ */
/*
 * dynamical/viscosity.py:178-190 (_calc_3d_visc: autocorrelate, times PRESSURE_CONVERSION**2, calc_visc = V/(kB T) x
 * cumtrapz, mean over the three tensor components) and dynamical/conductivity.py:109-114 + 229-231 as ONE call: the
 * series go to the device once, the correlation functions never come back to be sent again.
 *   acf[p][k]       = ( sum_t a_p[t+k] b_p[t] / (n-k) ) * acf_scale,  k = 0..n-1     host [n_series][n], or NULL
 *   integral[p][k]  = integral_scale * cumtrapz(acf[p], dx)                          host [n_series][n-1 (+1 with leading_zero)]
 *   integral_mean   = mean over p of integral[p] (numpy's order: ((i0 + i1) + i2 ...) / n_series)   host [n-1 (+1)], or NULL
 * Each factor is applied as one multiplication of the finished value — the roundings of `acf * c**2` and
 * `np.multiply(c, integral)` on the host; 1.0 leaves values untouched. a, b host|dev [n_series][n] (b == a:
 * autocorrelation). Destinations in page-locked memory (mdhip_host_alloc) are written by DMA.
 * At most 65535 series per call, as mdhip_cumtrapz.
 */
int mdhip_green_kubo(mdhip_ctx *ctx, int64_t n, int n_series, const double *a, const double *b, int on_device,
                     int method, double acf_scale, double dx, double integral_scale, int leading_zero, double *acf,
                     double *integral, double *integral_mean);
int mdhip_green_kubo_async(mdhip_ctx *ctx, int64_t n, int n_series, const double *a, const double *b, int on_device,
                           int method, double acf_scale, double dx, double integral_scale, int leading_zero, double *acf,
                           double *integral, double *integral_mean);

/* ---- pinned host staging memory (reader -> pinned buffers -> H2D) -------- */
/*
 * Page-locked host memory for the frame batches a caller parses into (mdproptools_amd/stream.py): host|dev inputs
 * that live in it are copied by DMA at the PCIe rate, asynchronously to the host, instead of through the driver's
 * bounce buffers. MDHIP_ENODEV without a usable HIP runtime.
 */
int mdhip_host_alloc(size_t bytes, void **out);
/* The same from a thread that has made no HIP call yet (a reader thread): `device` is made the thread's current device
 * first, so that a rank bound to GPU k does not open a context on GPU 0; device < 0 = whatever is current. */
int mdhip_host_alloc_on(int device, size_t bytes, void **out);
void mdhip_host_free(void *p);

/* ---- I/O: native LAMMPS text-dump reader (host only, no GPU needed) ---------------------------- */
/* ---- neighbour-shell residence autocorrelation ---- */
/*
 * Replaces the two loops of ResidenceTime.calc_auto_correlation   dynamical/residence_time.py:70-146
 * for one relation: central atoms xi [F][3][n_i], shell atoms xj [F][3][n_j], box [F][3];
 *   h_ij(t) = (rsq > r_lo_sq) && (rsq <= r_hi_sq)                 residence_time.py:101-102
 * with the reference's single-wrap rsq (rdf_cn.py:44-57); exclude_diagonal != 0 (a type with itself; the two
 * sets must then be the same atoms in the same order) clears h_ii (residence_time.py:103-104).
 *   counts[k] = sum_{i,j} sum_t h_ij(t) h_ij(t+k),  k = 0..F-1    exact integers
 * are the numerators of the unbiased autocovariances the reference sums (residence_time.py:124-131):
 *   corr[k] = counts[k] / (F - k) / (n_i n_j) / corr[0]. n_records (optional) = sum_t |{h_ij(t) = 1}|.
 */
int mdhip_shell_residence(mdhip_ctx *ctx, int64_t n_frames, int64_t n_i, const double *xi, int xi_on_device,
                          int64_t n_j, const double *xj, int xj_on_device, const double *box, double r_lo_sq,
                          double r_hi_sq, int exclude_diagonal, uint64_t *counts, uint64_t *n_records);

/* ---- solvation shells of cluster extraction (cluster_analysis.py get_clusters) ---- */
/*
 * Replaces the per-centre pair work of get_clusters            structural/cluster_analysis.py:47-235
 * for a batch of frames: coordinates xyz [F][3][n_atoms] (atoms in ascending-id order), box [F][3], centre atom
 * indices centres[n_centres], mol_of[n_atoms] the molecule index of every atom (molecules are contiguous runs of
 * atoms, as num_mols / num_atoms_per_mol lay them out, cluster_analysis.py:113-120).
 *   shell(f, c) = { mol_of[a] : rsq(centre c, atom a) < r_cut_sq }  cluster_analysis.py:127-142
 * with the reference's single-wrap rsq (rdf_cn.py:36-58: d = centre - atom, wrapped once when d > L/2 or
 * d < -L/2, (dx*dx + dy*dy) + dz*dz unfused); r_cut_sq is the caller's r_cut ** 2.
 *   mols [F][n_centres][cap]: the shell's molecule indices, ascending, padded with -1;
 *   count[F][n_centres]: the number of shell molecules, exact even when it exceeds cap (that row of mols is then
 *   incomplete: call again for its frame with cap >= count). 1 <= cap <= 16384.
 */
int mdhip_shell_members(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                        const double *box, int32_t n_centres, const int32_t *centres, const int32_t *mol_of,
                        double r_cut_sq, int32_t cap, int32_t *mols, int32_t *count);
/*
 * The per-molecule sums of the cluster force filter            cluster_analysis.py:146-152
 * (groupby(["mol_type", "mol_id"]).agg({"fx": "sum", ...})): attr [F][n_attr][n_atoms] -> out [F][n_attr][n_mols],
 * molecule m the atoms [seg_off[m], seg_off[m+1]). Each value is pandas' compensated group sum over the atoms in
 * ascending order: y = v - c; t = s + y; c = (t - s) - y; s = t (bit-identical to pandas, not to a plain sum).
 */
int mdhip_mol_kahan_sums(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, int n_attr, const double *attr,
                         int attr_on_device, int64_t n_mols, const int64_t *seg_off, double *out);
/*
 * The configuration census of get_unique_configurations          structural/cluster_analysis.py:238-457
 * taken from the trajectory instead of from cluster files: inputs as mdhip_shell_members, and the molecule layout in
 * full: seg_off[n_mols + 1] (molecule m is the atoms [seg_off[m], seg_off[m+1]), at most 255 of them, and mol_of
 * agrees), mol_type[n_mols] (>= 0), cls[n_atoms] the coordination class of every atom (0..7, or 255 for an atom that
 * never counts), passes [F][n_mols] (NULL: all ones) the force filter's verdict (cluster_analysis.py:146-152).
 *   members(f, c) = { m : passes[f][m], m is not the centre's own molecule, rsq(centre c, atom a) < r_shell_sq for
 *                         an atom a of m }                          cluster_analysis.py:127-216
 *   word(f, c, m) = sum over the atoms b of m with cls[b] != 255 and rsq(centre c, b) < r_coord_sq of
 *                   1 << (8 * cls[b])                               cluster_analysis.py:347-372
 * (eight 8-bit counters, one per class; the same single-wrap rsq; the two radii are independent).
 *   mols [F][n_centres][cap], words [F][n_centres][cap]: the members and their words in ascending
 *   (mol_type[m], word, m) order, padded with -1 and ~0: two rows are the same configuration exactly when their
 *   (type, word) sequences are equal;
 *   count[F][n_centres]: the number of members, exact even when it exceeds cap (that row is then incomplete: call
 *   again for its frame with cap >= count). 1 <= cap <= 4096.
 */
int mdhip_shell_coordination(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                             const double *box, int32_t n_centres, const int32_t *centres, int64_t n_mols,
                             const int32_t *mol_of, const int64_t *seg_off, const int32_t *mol_type,
                             const uint8_t *cls, const uint8_t *passes, double r_shell_sq, double r_coord_sq,
                             int32_t cap, int32_t *mols, uint64_t *words, int32_t *count);

/* ---- cation-water orientation of the hydration number (hydration_number.py get_hydration_number) ---- */
/*
 * Replaces the per-cation pair work of get_hydration_number      structural/hydration_number.py:13-99
 * for a batch of frames: coordinates xyz [F][3][n_atoms] (atoms in ascending-id order, host or device memory as
 * xyz_on_device says), box [F][3], cation atom indices cations[n_cations], and per water the index of its first atom
 * waters[n_waters] (O; H1 and H2 are the next two atoms). For every (frame f, cation c) the waters w with
 *   rsq(cation c, O of w) < r_cut_sq                               hydration_number.py:17-20
 * (the reference's single-wrap rsq, rdf_cn.py:36-58; r_cut_sq is the caller's r_cut ** 2), and their cosine
 *   d = cation - O wrapped once per axis, v = ((0 + H1) + H2) - 2 O from the raw coordinates,
 *   cos = (((0 + dx vx) + dy vy) + dz vz) / (sqrt((dx dx + dy dy) + dz dz) * sqrt((vx vx + vy vy) + vz vz))
 * unfused, correctly rounded sqrt and division (hydration_number.py:28-32, numpy's double); a zero vector gives NaN.
 *
 * mdhip_hydration_cosines (list mode):
 *   idx [F][n_cations][cap]: the water indices (positions in `waters`), ascending, padded with -1;
 *   cosines [F][n_cations][cap]: their cosines in the same order, padded with NaN;
 *   count [F][n_cations]: the number of waters, exact even when it exceeds cap (that row is then incomplete: call
 *   again for its frame with cap >= count). 1 <= cap <= 16384.
 * mdhip_hydration_counts (counts mode, no capacity limit):
 *   n_water [F][n_cations], n_away [F][n_cations]: the waters, and those with cos < cos_cut (NaN is not);
 *   hist [n_bins] (uint64, summed over all frames and cations): bin trunc((cos + 1.0) / bin_width), clamped to
 *   [0, n_bins - 1]; a NaN cosine is in no bin. 1 <= n_bins <= 4096.
 * Outputs are host memory.
 */
int mdhip_hydration_cosines(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                            const double *box, int32_t n_cations, const int32_t *cations, int32_t n_waters,
                            const int32_t *waters, double r_cut_sq, int32_t cap, int32_t *idx, double *cosines,
                            int32_t *count);
int mdhip_hydration_counts(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                           const double *box, int32_t n_cations, const int32_t *cations, int32_t n_waters,
                           const int32_t *waters, double r_cut_sq, double cos_cut, double bin_width, int32_t n_bins,
                           int32_t *n_water, int32_t *n_away, uint64_t *hist);

/* ---- bond-angle histograms (angular_distribution.py calc_angular_distribution; not in the reference) ---- */
/*
 * The distribution of the angle A-C-B at a centre atom C between two of its shell neighbours, for a batch of frames:
 * coordinates xyz [F][3][n_atoms] (host or device memory as xyz_on_device says), box [F][3], the centre atoms
 * centres[n_centres] with their class centre_class[n_centres], the candidate atoms cand[n_cand] (every atom that can
 * be a neighbour) with their class cand_class[n_cand], mol_of[n_atoms] (NULL: no exclusion), the triplets
 * triplet_class[n_triplets][3] = (class_a, class_c, class_b) with their squared cutoffs triplet_rsq[n_triplets][2] =
 * (r_ca ** 2, r_cb ** 2), and the table cos_edges[n_bins] = cos(m * bin_size), strictly decreasing.
 * For one frame, one centre c of class class_c and one triplet t:
 *   neighbour j of c in role A: j != c, class[j] == class_a, rsq(c, j) < r_ca ** 2 (the reference's single-wrap rsq,
 *     rdf_cn.py:36-58, strict), and mol_of[j] != mol_of[c] under exclusion; role B the same with class_b and r_cb;
 *   d_j = x_j - x_c wrapped once per axis (d > L/2 ? d - L : (d < -L/2 ? d + L : d)), n_j = sqrt((dx dx + dy dy) + dz dz),
 *   cos = ((dxj dxk + dyj dyk) + dzj dzk) / (n_j * n_k), unfused, correctly rounded sqrt and division;
 *   bin = the number of m in [1, n_bins) with cos <= cos_edges[m]: the angle is in [m D, (m + 1) D), the last bin is
 *     closed at 180 degrees, a cosine an ulp outside +-1 falls in the first or last bin; a NaN cosine (a neighbour on
 *     the centre) is in no bin and counts in n_degenerate[t];
 *   a symmetric triplet (class_a == class_b and r_ca ** 2 == r_cb ** 2) counts every unordered pair {j, k}, j != k, of
 *     role-A neighbours once; an asymmetric one every ordered (j, k), j != k, j in role A and k in role B.
 *   hist [n_triplets][n_bins], n_degenerate [n_triplets] (uint64, summed over all frames and centres), exact;
 *   count [F][n_centres]: the candidates other than c (and, under exclusion, its molecule) within the largest cutoff
 *     of the triplets of c's class, exact even when it exceeds cap. A row with count > cap adds NOTHING to hist and
 *     n_degenerate: call again with cap >= the largest count.
 * 1 <= n_triplets <= 8, n_triplets * n_bins <= 4096, 1 <= cap <= 512. Outputs are host memory. The call's aux time
 * (mdhip_last_aux_ms) is that of the gather and the search; the rest of its kernel time is the angle pass.
 */
int mdhip_angle_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                     const double *box, int32_t n_centres, const int32_t *centres, const int32_t *centre_class,
                     int32_t n_cand, const int32_t *cand, const int32_t *cand_class, const int32_t *mol_of,
                     int32_t n_triplets, const int32_t *triplet_class, const double *triplet_rsq, int32_t n_bins,
                     const double *cos_edges, int32_t cap, uint64_t *hist, uint64_t *n_degenerate, int32_t *count);

/* ---- order parameters (order_parameters.py calc_order_parameters; not in the reference) ---- */
/*
 * Per centre and frame the Steinhardt bond-orientational order parameters q_l, the Lechner-Dellago averaged qbar_l and
 * the tetrahedral pair (q_tet, s_k), for a batch of frames: coordinates xyz [F][3][n_atoms] (host or device memory as
 * xyz_on_device says), box [F][3], the centre atoms centres[n_centres], the candidate atoms cand[n_cand] (every atom
 * that can be a neighbour, distinct), mol_of[n_atoms] (NULL: no exclusion), the squared cutoff, the degrees
 * degrees[n_degrees] (distinct, 1 <= l <= 12, at most 4) and n_nearest (0: every neighbour).
 * For one frame and one centre c:
 *   neighbour j of c: a candidate, j != c, rsq(c, j) < r_cut_sq (the reference's single-wrap rsq, rdf_cn.py:36-58,
 *     strict), and mol_of[j] != mol_of[c] under exclusion; with n_nearest = k > 0 the k neighbours smallest by
 *     (rsq, atom index) are selected, else all; a row of fewer than k neighbours (k = 0: of none) is short;
 *   d_j = x_j - x_c wrapped once per axis (d > L/2 ? d - L : (d < -L/2 ? d + L : d)), n_j = sqrt((dx dx + dy dy) + dz dz),
 *     u_j = d_j / n_j; a selected neighbour with n_j == 0 or not finite makes the row degenerate (a short row is short
 *     only);
 *   q_lm = (1 / N) sum_j Y_lm(u_j) over the N selected neighbours in ascending atom index, real spherical harmonics
 *     from the recurrence of the normalised associated Legendre functions in u_z and the powers of rho = sqrt(ux ux +
 *     uy uy) and (ux + i uy) / rho (rho == 0: only m = 0 is not zero); q_l = sqrt(4 pi / (2l + 1) sum_m q_lm q_lm);
 *   qbar_lm(c) = (q_lm(c) + sum_j q_lm(j)) / (N + 1) over the same N neighbours in ascending atom index (averaged:
 *     cand must equal centres, so that a neighbour is a row of its own), qbar_l from qbar_lm as q_l from q_lm; NaN of
 *     any member (the row itself or a neighbour, short or degenerate) propagates, and the row counts as short;
 *   q_tet = 1 - 3/8 sum_{j<k} (cos_jk + 1/3)^2, cos_jk = ((dxj dxk + dyj dyk) + dzj dzk) / (n_j n_k), and
 *     s_k = 1 - 1/3 sum_k ((n_k - rbar)^2 / (4 rbar rbar)), rbar = (((n_0 + n_1) + n_2) + n_3) / 4, over the 4 neighbours
 *     smallest by (rsq, atom index), taken in ascending atom index (pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3));
 *     fewer than 4 neighbours: short; one of the 4 with n == 0 or not finite: degenerate.
 *   q [F][n_centres][n_degrees], qbar the same (averaged != 0, else NULL), tet [F][n_centres][2] = (q_tet, s_k)
 *     (tetrahedral != 0, else NULL): NaN for a short or degenerate row;
 *   flags [F][n_centres]: bit 0 q short, 1 q degenerate, 2 tetrahedral short, 3 tetrahedral degenerate, 4 qbar short;
 *   count [F][n_centres]: the neighbours of the row, exact even when it exceeds cap. A row with count > cap gives NaN
 *     and no flag: call again with cap >= the largest count.
 * The values do not depend on cap, on the order in which the search found the neighbours, or on the launch. 1 <= cap
 * <= 512, 0 <= n_nearest <= 512; at least one degree or tetrahedral. Outputs are host memory. The call's aux time
 * (mdhip_last_aux_ms) is that of the gather and the search; the rest of its kernel time is the row passes.
 */
int mdhip_bond_order(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                     const double *box, int32_t n_centres, const int32_t *centres, int32_t n_cand, const int32_t *cand,
                     const int32_t *mol_of, double r_cut_sq, int32_t n_degrees, const int32_t *degrees,
                     int32_t n_nearest, int32_t averaged, int32_t tetrahedral, int32_t cap, double *q, double *qbar,
                     double *tet, int32_t *flags, int32_t *count);

/* ---- spatial distribution functions (spatial_distribution.py calc_spatial_distribution; not in the reference) ---- */
/*
 * The three-dimensional histogram of observed atoms in the body-fixed frame of a reference molecule, for a batch of
 * frames: coordinates xyz [F][3][n_atoms] (host or device memory as xyz_on_device says), box [F][3], per reference
 * molecule its origin atom origin[n_centres], x-axis atom x_atom[n_centres] and xy-plane atom xy_atom[n_centres], the
 * candidate atoms cand[n_cand] (every atom of an observed species) with their species cand_class[n_cand] in
 * [0, n_species), mol_of[n_atoms] (NULL: no exclusion), r_cut, r_cut_sq = r_cut ** 2 as the caller squares it,
 * bin_size and n_grid = G = ceil(2 * r_cut / bin_size). All arithmetic is unfused f64 with correctly rounded sqrt and
 * division, in exactly this order; wrap(d, L) = d > L/2 ? d - L : (d < -L/2 ? d + L : d), per axis.
 * The body frame of one frame and one molecule with origin atom o, x-axis atom p and xy-plane atom q:
 *   a = wrap(x_p - x_o), b = wrap(x_q - x_o);
 *   na2 = (ax ax + ay ay) + az az, e1 = a / sqrt(na2) component by component;
 *   s = (bx e1x + by e1y) + bz e1z, c_k = b_k - s e1_k;
 *   nc2 = (cx cx + cy cy) + cz cz, e2 = c / sqrt(nc2);
 *   e3 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x): right-handed;
 *   the row (frame, molecule) is DEGENERATE when na2 or nc2 is zero or not finite (p on o, q on the line through o and
 *   p, or a non-finite coordinate): it has no frame.
 * A candidate j of species s is a hit for the origin atom o when j != o, mol_of[j] != mol_of[o] under exclusion, and
 * rsq(o, j) < r_cut_sq (the reference's single-wrap rsq, rdf_cn.py:36-58, strict). For a hit, d = wrap(x_j - x_o),
 *   p_k = (dx ekx + dy eky) + dz ekz for k = 1, 2, 3,
 *   i_k = floor((p_k + r_cut) / bin_size) clamped to [0, G - 1] (the clamp is made on the double: NaN gives 0),
 *   hist[s][i1][i2][i3] += 1; a hit of a degenerate row adds nothing to hist and counts in n_degenerate[s].
 * hist [n_species][G][G][G] and n_degenerate [n_species] (uint64, summed over all frames and molecules, exact: the
 * cells are 64-bit counters), n_hits [F][n_centres] (int32): the hits of the row over all species, n_degenerate_rows
 * (uint64): the degenerate rows. There is no capacity: nothing in this call can overflow and nothing is run again.
 * A non-finite coordinate makes every comparison it enters false: such a candidate is in no shell, an origin atom with
 * one has no hits, a non-finite p or q makes the row degenerate, and no other atom's result changes.
 * 1 <= n_species <= 8, 1 <= n_grid <= 256, n_species * n_grid ** 3 <= 2^25, r_cut and bin_size positive and finite.
 * Outputs are host memory. The call's aux time (mdhip_last_aux_ms) is that of the frame pre-pass and the gather; the
 * rest of its kernel time is the sweep.
 * mdhip_body_frames is the frame pre-pass alone: frames [F][n_mols][10] (host memory), per row e1x e1y e1z e2x e2y e2z
 * e3x e3y e3z and 1.0 for a row that has a frame, 0.0 for a degenerate one (whose nine components then mean nothing),
 * and n_degenerate_rows.
 */
int mdhip_body_frames(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                      const double *box, int32_t n_mols, const int32_t *origin, const int32_t *x_atom,
                      const int32_t *xy_atom, double *frames, uint64_t *n_degenerate_rows);
int mdhip_sdf_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                   const double *box, int32_t n_centres, const int32_t *origin, const int32_t *x_atom,
                   const int32_t *xy_atom, int32_t n_cand, const int32_t *cand, const int32_t *cand_class,
                   int32_t n_species, const int32_t *mol_of, double r_cut, double r_cut_sq, double bin_size,
                   int32_t n_grid, uint64_t *hist, uint64_t *n_degenerate, int32_t *n_hits,
                   uint64_t *n_degenerate_rows);

/* ---- connected components of a contact graph (aggregates.py calc_aggregates; not in the reference) ---- */
/*
 * Which nodes (molecules, or atoms) hang together through contacts between listed atoms, for a batch of frames:
 * coordinates xyz [F][3][n_atoms] (host or device memory as xyz_on_device says), box [F][3], a list A of atoms
 * atoms_a[n_a] with a class class_a[n_a] in [0, n_ca), a list B of atoms atoms_b[n_b] with a class class_b[n_b] in
 * [0, n_cb) (the two lists may share atoms), the squared cutoff of every class pair rsq_cut[n_ca][n_cb] (a value <= 0:
 * that pair never links), and node_of[n_atoms] (read only for listed atoms; values in [0, n_nodes)).
 * In frame f, atom i of A and atom j of B are in contact when
 *   node_of[i] != node_of[j], and
 *   rsq(i, j) < rsq_cut[class_a[i]][class_b[j]] (the reference's single-wrap rsq, rdf_cn.py:36-58, strict, unfused).
 * Each contact makes the two nodes neighbours.
 *   label [F][n_nodes] (int32): the smallest node index of the connected component of that node in that frame; a node
 *     without a contact is its own label;
 *   n_components [F] (int32): the number of nodes with label == index;
 *   n_contacts [F] (uint64): the number of (position in A, position in B) pairs in contact; a pair of atoms listed on
 *     both sides counts once for each position pair in contact (twice when both atoms are in both lists).
 * 1 <= n_ca, n_cb <= 16, n_nodes < 2^31, at least one positive cutoff, every atom index in [0, n_atoms). There is no
 * capacity: nothing in this call can overflow. Outputs are host memory. The call's aux time (mdhip_last_aux_ms) is that
 * of the gather and the union sweep; the rest of its kernel time is the initialisation of the parent rows and the
 * label pass.
 */
int mdhip_contact_components(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                             const double *box, int32_t n_a, const int32_t *atoms_a, const int32_t *class_a,
                             int32_t n_b, const int32_t *atoms_b, const int32_t *class_b, int32_t n_ca, int32_t n_cb,
                             const double *rsq_cut, int64_t n_nodes, const int32_t *node_of, int32_t *label,
                             int32_t *n_components, uint64_t *n_contacts);

/* ---- hydrogen bonds (hydrogen_bonds.py calc_hydrogen_bonds, calc_hbond_lifetime; not in the reference) ---- */
/*
 * Which D-H...A bonds exist in a batch of frames: coordinates xyz [F][3][n_atoms] (host or device memory as
 * xyz_on_device says), box [F][3], the donors donors[n_don] (heavy atoms) with their class don_class[n_don] in
 * [0, n_dc), their hydrogens in CSR form (the hydrogens of donor d are the atoms h_atoms[h_off[d] .. h_off[d + 1]),
 * h_off[0] == 0, h_off[n_don] == n_h), the acceptors acceptors[n_acc] with their class acc_class[n_acc] in [0, n_ac),
 * mol_of[n_atoms] (NULL: no exclusion), the squared cutoffs r_da_sq and r_ha_sq (r_ha_sq <= 0: that test is off) and
 * cos_cut = cos(angle_cut).
 * In frame f, hydrogen h of donor d is bonded to acceptor a when
 *   the atom of a is not the atom of d, and mol_of[a] != mol_of[d] under exclusion;
 *   rsq(d, a) < r_da_sq (the reference's single-wrap rsq, rdf_cn.py:36-58, strict, unfused);
 *   rsq(h, a) < r_ha_sq, when that test is on;
 *   cos <= cos_cut, with u = x_d - x_h and v = x_a - x_h, each wrapped once per axis
 *     (d > L/2 ? d - L : (d < -L/2 ? d + L : d)),
 *     cos = ((ux vx + uy vy) + uz vz) / (sqrt((ux ux + uy uy) + uz uz) * sqrt((vx vx + vy vy) + vz vz)), unfused,
 *     correctly rounded sqrt and division: the angle D-H...A is at least angle_cut.
 * A NaN cosine (H on D or on A) is no bond; it counts in n_degenerate. A non-finite coordinate makes every comparison
 * it enters false: that atom bonds to nothing, and no other atom's result changes (a non-finite hydrogen that is not
 * stopped by the r_ha test has a NaN cosine and counts in n_degenerate).
 *
 * mdhip_hbond_counts (per frame, no capacity: nothing in it can overflow):
 *   n_bonds [F][n_dc][n_ac] (int32): the bonds of every frame and class pair;
 *   n_donated [n_don], n_accepted [n_acc] (uint64): the bonds each donor gives and each acceptor takes, summed over
 *     the frames;
 *   angle_hist [n_dc][n_ac][n_bins] (uint64, summed over the frames): every (h, a) that passes every test but the
 *     angle test, binned by its cosine against cos_edges[n_bins] = cos(m * bin_size), strictly decreasing, with the
 *     rule of mdhip_angle_hist: bin = the number of m in [1, n_bins) with cos <= cos_edges[m]. n_bins == 0: no
 *     histogram (cos_edges and angle_hist may be NULL);
 *   n_degenerate (uint64): the (h, a) with a NaN cosine among them.
 *   1 <= n_dc * n_ac <= 64, n_dc * n_ac * n_bins <= 4096. Any number of frames.
 *
 * mdhip_hbond_lifetime (a whole trajectory, n_frames <= 65535, lags 0 .. max_lag, 0 <= max_lag < n_frames): with
 * h(t) = 1 when the pair (position in h_atoms, position in acceptors) is bonded in frame t,
 *   c_int [max_lag + 1] (uint64): c_int[k] = sum over pairs and t of h(t) h(t + k) (intermittent);
 *   c_cont [max_lag + 1] (uint64): c_cont[k] = sum over pairs of the number of t with h(t) = ... = h(t + k) = 1
 *     (continuous): every run of L consecutive ones adds max(0, L - k);
 *   n_pairs: the distinct pairs that are ever bonded; n_records: the sum of all set bits (= c_int[0] = c_cont[0]).
 *   The pairs' presence masks (one bit per frame) live in a hash table in device memory. table_slots == 0: the
 *   library sizes it, and sweeps once more with a table sized from the bond count when it fills; table_slots > 0:
 *   that many slots (rounded up to a power of two) for the first sweep. The table's byte limit is taken from the free
 *   device memory; a table that cannot fit fails with MDHIP_ELIMIT and a text that names its size. More than 65535
 *   frames: MDHIP_EINVAL before anything is launched. The call's aux time (mdhip_last_aux_ms) is that of the two lag
 *   kernels; the rest of its kernel time is the gather and the sweep (or sweeps).
 * Outputs are host memory.
 */
int mdhip_hbond_counts(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                       const double *box, int32_t n_don, const int32_t *donors, const int32_t *don_class,
                       const int32_t *h_off, int32_t n_h, const int32_t *h_atoms, int32_t n_acc,
                       const int32_t *acceptors, const int32_t *acc_class, int32_t n_dc, int32_t n_ac,
                       const int32_t *mol_of, double r_da_sq, double r_ha_sq, double cos_cut, int32_t n_bins,
                       const double *cos_edges, int32_t *n_bonds, uint64_t *n_donated, uint64_t *n_accepted,
                       uint64_t *angle_hist, uint64_t *n_degenerate);
int mdhip_hbond_lifetime(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                         const double *box, int32_t n_don, const int32_t *donors, const int32_t *h_off, int32_t n_h,
                         const int32_t *h_atoms, int32_t n_acc, const int32_t *acceptors, const int32_t *mol_of,
                         double r_da_sq, double r_ha_sq, double cos_cut, int32_t max_lag, int64_t table_slots,
                         uint64_t *c_int, uint64_t *c_cont, uint64_t *n_pairs, uint64_t *n_records);

/* ---- atom counts along the axis normal to a surface (number_density.py calc_number_density) ---- */
/*
 * Replaces the per-type selections and the counting loop of calc_number_density   structural/number_density.py:76-105
 * for a batch of frames: the axis coordinate x [F][n_atoms] (host or device memory as x_on_device says) and a 16-bit
 * code per atom, codes [n_atoms] shared by the frames or [F][n_atoms] (codes_per_frame != 0), host memory:
 *   code & MDHIP_AP_NONE   the row of the result the atom counts in, 0 .. n_rows - 1; MDHIP_AP_NONE (or any value
 *                          >= n_rows): in none
 *   code & MDHIP_AP_SURFACE  the atom belongs to the surface (it may count in a row as well)
 * Per frame, in float64, unfused, with true division (w = bin_size):
 *   lo, hi = min, max of x over the surface atoms; NaN coordinates are skipped (pandas' min / max), NaN, NaN without
 *   a surface atom; -0.0 orders below +0.0                                          number_density.py:76-82
 *   MDHIP_AP_REF_POS: s = x - lo; the atoms with s < dist: b = s - (hi - lo)        number_density.py:87-96
 *   MDHIP_AP_REF_NEG: s = x - lo; the atoms with s > dist: b = s                    number_density.py:97-105
 *     k = trunc(b / w); counted in bin k when 0 <= k < n_bins, in bin k + n_bins when -n_bins <= k < 0 (the
 *     reference indexes a numpy row with k), else in outside[f] and in no bin (the reference raises IndexError)
 *   MDHIP_AP_PROFILE: s = x - origin_f, origin_f = lo (origin_kind 0), hi (1) or origin[f] (2);
 *     t = (s - dist) / w (dist = the lower end of the binned range); counted in bin trunc(t) when t >= 0 and
 *     trunc(t) < n_bins, else (NaN included) in outside[f]; nothing wraps
 * counts [F][n_rows][n_bins] (uint32), extent [F][2] (lo, hi), outside [F] (uint32): host memory, exact.
 * 1 <= n_rows < MDHIP_AP_NONE, n_bins >= 1, n_rows * n_bins < 2^31, n_atoms < 2^31.
 */
#define MDHIP_AP_REF_POS 0
#define MDHIP_AP_REF_NEG 1
#define MDHIP_AP_PROFILE 2
#define MDHIP_AP_SURFACE 0x4000u
#define MDHIP_AP_NONE 0x3FFFu
int mdhip_axis_profile(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                       const uint16_t *codes, int codes_per_frame, int32_t n_rows, int mode, double bin_size,
                       double dist, int32_t n_bins, int origin_kind, const double *origin, uint32_t *counts,
                       double *extent, uint32_t *outside);

/* ---- displacement over a fixed lag (Displacement.calc_dist; self part of the van Hove function) ---- */
/*
 * Finishes what the reference's Displacement.calc_dist sketches      dynamical/residence_time.py:211-254
 * (the wrapped x y z of the chosen atoms per frame, to be grouped into windows of one residence time): the histogram
 * of the distance travelled over a fixed lag, over all time origins, i.e. G_s(r, t) before normalisation.
 *   r          host|dev (r_on_device) [n_frames][3][n_ent]
 *   box        host [n_frames][3] edge lengths: r is WRAPPED and the image counts are rebuilt; NULL: r is unwrapped
 *   group_off  host int64 [n_groups+1] contiguous entity groups (as mdhip_msd_pairs); empty groups are allowed
 *   jobs       host int32 [n_jobs][3] = (group, lag, stride), 1 <= lag <= n_frames-1, stride >= 1; several jobs may
 *              name one group (a van Hove call asks for many lags that way)
 *   edges      host [nbins+1] from mdhip_bin_edges, or NULL to have it computed from bin_size; 1 <= nbins <= 2^20
 * Anything else is MDHIP_EINVAL before anything is written.
 * Image counts (box != NULL), per entity and axis: n(0) = 0; for f >= 1, d = x(f) - x(f-1), L = box[f][axis]:
 * n(f) = n(f-1) - 1 when d > L/2, n(f-1) + 1 when d < -L/2, else n(f-1) — strict, the reference's single-wrap
 * convention (rdf_cn.py:44-57); a NaN compares false and shifts nothing. xu(f) = x(f) + (double)n(f) * L(f), one
 * multiplication and one addition, unfused; xu = x when box == NULL. Only meaningful when no entity moves more than
 * half a box edge between consecutive frames.
 * Per job (g, k, s): origins t0 = 0, s, 2s, ... with t0 + k <= n_frames-1, entities of group g; for every (origin,
 * entity) d = xu(t0+k) - xu(t0), rsq = (dx*dx + dy*dy) + dz*dz unfused, bin = (int64)(sqrt(rsq) / bin_size) decided by
 * comparing rsq with the edge table (never by device sqrt).
 *   hist       host uint64 [n_jobs][nbins]: +1 in hist[job][bin] when bin < nbins
 *   overflow   host uint64 [n_jobs]: the windows with bin >= nbins or a NaN rsq
 *   windows    host uint64 [n_jobs] = origins * group size
 *   moments    host double [n_jobs][3] = sum sqrt(rsq), sum rsq, sum rsq*rsq over ALL windows of the job (overflowing
 *              ones included; sqrt correctly rounded); fixed order per launch geometry, no float atomics: within
 *              windows * 2^-52 relative of any other summation order, bit-identical from call to call
 *   crossings  host uint64 [1] or NULL: the (frame step, entity, axis) triples that shifted; 0 when box == NULL
 * The integer outputs are exact and independent of the launch geometry. Any number of frames, entities and jobs:
 * launch dimensions over 65535 are split inside the call.
 */
int mdhip_displacement_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                            const double *box, int n_groups, const int64_t *group_off, int n_jobs,
                            const int32_t *jobs, double bin_size, int32_t nbins, const double *edges,
                            uint64_t *hist, uint64_t *overflow, uint64_t *windows, double *moments,
                            uint64_t *crossings);

/* ---- distinct part of the van Hove function (Displacement.calc_van_hove_distinct) ---- */
/*
 * G_d(r, t) before normalisation: per time origin, the histogram of the distances between where the entities of group a
 * were at t0 and where the entities of group b are at t0 + lag. The reference has nothing like it; the conventions are
 * those of mdhip_displacement_hist, whose self part this completes.
 *   r          host|dev (r_on_device) [n_frames][3][n_ent], WRAPPED coordinates (no image counts are rebuilt)
 *   box        host [n_frames][3] edge lengths; required
 *   group_off  host int64 [n_groups+1] contiguous entity groups; empty groups are allowed
 *   jobs       host int32 [n_jobs][4] = (group a, group b, lag, stride), 0 <= lag <= n_frames-1 (lag 0: the pair
 *              counts of g(r)), stride >= 1
 *   edges      host [nbins+1] from mdhip_bin_edges, or NULL to have it computed from bin_size; 1 <= nbins <= 2^20
 * Anything else (NULL box, a group index out of range, a lag outside [0, n_frames-1], stride < 1, nbins out of range,
 * a bin_size that is not positive and finite, a group_off that does not ascend within [0, n_ent]) is MDHIP_EINVAL
 * before anything is written.
 * Per job (a, b, k, s): origins t0 = 0, s, 2s, ... with t0 + k <= n_frames-1; for every origin, every i in a and every
 * j in b with j != i as entity indices (which only bites when a == b): d = r[t0+k][x][j] - r[t0][x][i] per axis, one
 * shift by L = box[t0][x] iff |d| > L/2 — strict, the reference's single-wrap convention (rdf_cn.py:44-57), i.e. the
 * magnitude min(|d|, ||d| - L|) for L >= 0 — rsq = (dx*dx + dy*dy) + dz*dz unfused, bin = (int64)(sqrt(rsq) / bin_size)
 * decided by comparing rsq with the edge table (never by device sqrt).
 *   hist       host uint64 [n_jobs][nbins]: +1 in hist[job][bin] when rsq < edges[nbins]
 *   beyond     host uint64 [n_jobs]: every other pair, a NaN or +inf rsq included
 *   pairs      host uint64 [n_jobs] = origins * (N_a * N_b - (a == b ? N_a : 0)) = sum(hist[job]) + beyond[job]
 * Pairs are ordered: for a == b every unordered pair is visited twice (at lag > 0 those are two different distances;
 * at lag 0 the counts are those of mdhip_rdf_atomic, which adds 2 per pair for a == b); for a != b once.
 * Non-finite input: a pair with a non-finite coordinate at either end lands in `beyond`, every other pair counts as
 * before: hist is that of the trajectory without the entity.
 * The outputs are integers, exact and independent of the launch geometry. Any number of frames, entities and jobs:
 * launch dimensions over 65535 are split inside the call. Complete on return.
 */
int mdhip_van_hove_distinct(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                            const double *box, int n_groups, const int64_t *group_off, int n_jobs,
                            const int32_t *jobs, double bin_size, int32_t nbins, const double *edges, uint64_t *hist,
                            uint64_t *beyond, uint64_t *pairs);

/* ---- structural relaxation (dynamical/relaxation.py, class StructuralRelaxation; no counterpart in the reference) ---- */
/*
 * The self-intermediate scattering function F_s(q, t) = < sin(q |dr|) / (q |dr|) > (isotropic, exact) and the overlap
 * counts behind Q(t) = < theta(a - |dr|) > and chi4(t) = N [<Q^2> - <Q>^2], at EVERY lag 0 .. max_lag and per time
 * origin: the count n(t0, k) of a group's entities that moved less than a is complete before it is squared.
 *   r          host|dev (r_on_device) [n_frames][3][n_ent]: the layout mdhip_displacement_hist reads
 *   box        host [n_frames][3] edge lengths: r is WRAPPED and the image counts are rebuilt by exactly the rule stated
 *              for mdhip_displacement_hist (strict +-L/2, a NaN shifts nothing, xu = x + (double)n * L unfused);
 *              NULL: r is unwrapped, xu = x
 *   group_off  host int64 [n_groups+1] contiguous entity groups, 1 <= n_groups <= 16; empty groups are allowed
 *   max_lag    0 .. n_frames-1: the lags k = 0 .. max_lag
 *   origin_stride  s >= 1: the origins of lag k are t0 = 0, s, 2s, ... with t0 + k <= n_frames-1
 *              (any int64 s >= 1: a stride beyond n_frames-1 leaves the one origin t0 = 0 and is treated as n_frames)
 *   a_sq       host [n_groups]: the squared overlap length a * a per group, formed once by the caller; NULL: no overlap
 *              part
 *   q          host [n_groups][n_q], 0 <= n_q <= 4: wave numbers >= 0 in 1 / length (ignored when n_q == 0)
 * Per (group g, lag k, origin t0, entity e of g), in float64, unfused:
 *   d = xu(t0+k) - xu(t0) per axis, rsq = (dx*dx + dy*dy) + dz*dz
 *   rsq not finite (NaN or Inf): +1 in nonfinite[k][g], and nothing else
 *   else: n(t0, k) += 1 when rsq < a_sq[g] (strict), and for every j < n_q:
 *     x = q[g][j] * sqrt(rsq) (sqrt correctly rounded, one multiplication), v = sinc(x), addend = (int64) rint(v * 2^32)
 *     (half to even). sinc(x) is within 2^-34 absolute of sin(x) / x of the double x (1 at x = 0), for every x >= 0:
 *       x >= 2^36 (an overflow to +inf included): v = 0; |sin(x) / x| <= 2^-36 there
 *       x <  2^-8:  the series v = 1 + x2 * (-1/6 + x2 * (1/120)), x2 = x * x; what it leaves out is below
 *                   x^6 / 5040 <= 2^-48 / 5040 < 2^-60, its roundings below 2^-51
 *       else:       sin(x) from the argument reduced by multiples of pi/2 (pi/2 as two doubles, fused multiply-adds)
 *                   and the Taylor polynomials of sine (degree 13) and cosine (degree 14), within 2^-44; one division
 *                   by x >= 2^-8, where every error is relative while x < pi/4: within 2^-43 (csrc/relaxation_plan.h
 *                   has the derivation, tests/native/relaxation_plan_main.cpp measures it)
 * Results, host memory:
 *   origins    uint64 [max_lag+1]: the number of origins of lag k
 *   count1     uint64 [max_lag+1][n_groups] = sum over t0 of n(t0, k); count2 the same sum of n(t0, k)^2. With
 *              a_sq == NULL both are left UNTOUCHED (and may be NULL)
 *   fs         int64 [max_lag+1][n_groups][n_q] = sum over t0 and e of the addends; untouched (may be NULL) when n_q == 0
 *   nonfinite  uint64 [max_lag+1][n_groups]
 * F_s = fs / 2^32 / W and Q = count1 / W with W = origins * group size; chi4 = (O count2 - count1^2) / (O^2 N).
 * Every result is an integer: exact, independent of the launch geometry and of the order of the entities inside a
 * group, bit-identical from call to call. No floating-point atomics, no floating-point accumulators.
 * MDHIP_EINVAL before anything is written: n_groups outside 1..16, n_q outside 0..4, n_frames outside 1..2^29-1,
 * n_ent outside 0..2^40-1 or n_frames * n_ent >= 2^40 ("trajectory too large"), max_lag outside 0..n_frames-1,
 * origin_stride < 1, a group_off that does not ascend within [0, n_ent], a negative or
 * non-finite q, a negative or NaN a_sq, a_sq == NULL together with n_q == 0, a NULL required array, and any group
 * with origins[0] * size >= 2^30 (fs stays within int64 with the 2^32 unit and count2 within uint64; a larger
 * origin_stride is the remedy, and the error text says so). Launch dimensions over 65535 are split inside the call.
 */
int mdhip_self_relaxation(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                          const double *box, int n_groups, const int64_t *group_off,
                          int64_t max_lag, int64_t origin_stride,
                          const double *a_sq, int n_q, const double *q,
                          uint64_t *origins, uint64_t *count1, uint64_t *count2,
                          int64_t *fs, uint64_t *nonfinite);

/* ---- Einstein-Helfand conductivity (Conductivity.einstein / nernst; `pass` in the reference,
 *      dynamical/conductivity.py:399-403) ---- */
/*
 * The charge-weighted collective displacement of every group, per frame:
 *   P[g][x][t] = sum over the entities e of group g of c_e * (r[t][x][e] - r[0][x][e]),   c_e = weight[e] * scale
 *   r          host|dev (r_on_device) [n_frames][3][n_ent] UNWRAPPED entity coordinates (molecule centres of mass)
 *   weight     host [n_ent] (the charge, already in output units); scale: the coordinates' unit factor. c_e is formed
 *              once on the host, one multiplication.
 *   group_off  host int64 [n_groups+1] contiguous entity groups, 1 <= n_groups <= 16; empty groups give zeros
 *   P          host|dev (P_on_device) [n_groups][3][n_frames], time-major: the input layout of mdhip_cross_msd
 *   weighted_dev  NULL, or DEVICE [n_frames][3][n_ent] that receives c_e * (r[t] - r[0]) per entity (0 for an entity
 *              of no group): fed to mdhip_lag_msd with scale 1 it yields the self part sum_e c_e^2 <|dr_e|^2> (total
 *              column times the group size), so the Nernst-Einstein sum needs no weighting pass of its own
 * Frame 0 is subtracted BEFORE the weighted sum: unwrapped coordinates of tens of angstrom summed over thousands of
 * ions of both signs would otherwise cancel the digits the displacement lives in.
 * Floating point: per entity one subtraction and one multiplication, unfused; per (frame, axis, group) 256 partial
 * sums, partial i adding the entities i, i + 256, ... of the group in order, and a fixed tree over them
 * (red[i] += red[i + w], w = 128 .. 1). The order depends on the group size alone; no floating-point atomics: every
 * call gives the same bits. A NaN stays in its own group and axis. One read of the trajectory: HBM-bound.
 * n_groups outside 1..16, n_frames < 1 or a group_off that does not ascend within [0, n_ent]: MDHIP_EINVAL before
 * anything is written.
 */
int mdhip_collective_displacement(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                                  const double *weight, double scale, int n_groups, const int64_t *group_off,
                                  double *P, int P_on_device, double *weighted_dev);

/*
 * The cross-displacement correlation of the collective series at every lag (the Einstein-Helfand sum):
 *   out[k][a][b] = ( sum_{t=0}^{n-1-k} sum_x (P[a][x][t+k] - P[a][x][t]) * (P[b][x][t+k] - P[b][x][t]) ) / (n - k)
 *   P          host|dev (P_on_device) [n_groups][3][n], 1 <= n_groups <= 16, 1 <= n < 2^29
 *   max_lag    0 .. n-1
 *   out        host|dev (out_on_device) [max_lag+1][n_groups][n_groups]; symmetric bit for bit (a <= b is computed and
 *              mirrored)
 *   abs_out    NULL, or the same shape and place as out: the same sum over |term|, term = one axis' product. It is the
 *              scale of the rounding error: out is within (3 (n - k) + 2) * 2^-53 * abs_out of the exact sum over
 *              the given P (plus one rounding of the division), whatever the order.
 * Difference form throughout: subtract, then one fused multiply-add per term. A product of values is never formed,
 * so a collective dipole that has wandered far from its start costs no digits (composing the sum from
 * mdhip_xcorr results would). No floating-point atomics: the terms of a lag are added in an order fixed by n, max_lag,
 * n_groups and the device's compute-unit count; results are bit-identical from call to call. A NaN in a series of
 * group g reaches rows and columns g only. n * max_lag / 2 window positions of 3 G subtractions and 3 G (G + 1) / 2
 * multiply-adds (twice the latter with abs_out): FP64-bound. Any n; launch dimensions never grow with n beyond the
 * number of lag tiles.
 * n_groups outside 1..16, n < 1, max_lag outside 0..n-1: MDHIP_EINVAL before anything is written.
 */
int mdhip_cross_msd(mdhip_ctx *ctx, int64_t n, int n_groups, const double *P, int P_on_device, int64_t max_lag,
                    double *out, double *abs_out, int out_on_device);

/* ---- molecular reorientation (dynamical/reorientation.py, class Reorientation; no counterpart in the reference) ---- */
/*
 * Molecule-fixed unit vectors, time-major: the input of mdhip_orient_corr.
 *   x          host|dev (x_on_device) [n_frames][3][n_atoms], atoms by id, molecules contiguous: the layout
 *              mdhip_segment_com reads
 *   box        host [n_frames][3] edge lengths, or NULL: x is unwrapped
 *   jobs       job j covers job_mols[j] molecules of job_len[j] atoms each, the first one starting at atom job_atom0[j]
 *              (host [n_jobs]); its terms are the pairs (k, w) = (term_atom[i], term_w[i]), term_off[j] <= i <
 *              term_off[j+1] (host; term_off [n_jobs+1] starts at 0), with 1 <= k < job_len[j], k strictly ascending
 *   U          host|dev (U_on_device) [n_series][3][n_frames], n_series = sum of job_mols: series are numbered job after
 *              job, molecule after molecule
 *   degenerate host uint64 [n_jobs]: the (molecule, frame) pairs of the job whose vector is exactly zero
 * For a molecule whose first atom is a, per axis: d_k = x[a+k] - x[a]; with box, d_k is wrapped once as the reference's
 * pair distances are (rdf_cn.py:44-57): d > L/2 -> d - L, d < -L/2 -> d + L, strict, a NaN shifts nothing;
 * v = sum_k w_k * d_k in ascending k, one multiplication and one addition per term, unfused, starting from w_1 * d_1.
 * Then n2 = (vx*vx + vy*vy) + vz*vz and u = v / sqrt(n2): three divisions by the correctly rounded root, so U is
 * defined bit for bit. n2 == 0 gives u = (0, 0, 0) and +1 in degenerate[j], exactly counted; a non-finite n2 (NaN, or
 * an overflow) gives three NaN components and is not counted. Atoms that no term names, the first atom apart, are
 * never read: a NaN there does not leak.
 * A bond or end-to-end vector tail -> head is the terms (tail, -1), (head, +1), the term of k = 0 dropped because it
 * contributes zero; a dipole is (k, q_k) for every k >= 1. The dipole of a CHARGED molecule depends on the origin: here
 * it is taken about the molecule's first atom. With box, the result is meaningful only when the named atoms lie within
 * half a box edge of the molecule's first atom (one wrap per difference, no connectivity is followed).
 * The trajectory is read frame-major and U written time-major through an LDS tile of 64 molecules x 64 frames, both
 * sides coalesced; one read of the lines that hold named atoms: HBM-bound. Any number of frames, molecules and jobs:
 * launch dimensions over 65535 are split inside the call.
 * n_jobs < 1, a NULL array, a job that runs past n_atoms, a job without terms, k outside [1, job_len) or not strictly
 * ascending: MDHIP_EINVAL before anything is written.
 */
int mdhip_axis_vectors(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                       const double *box, int n_jobs, const int64_t *job_atom0, const int64_t *job_mols,
                       const int32_t *job_len, const int64_t *term_off, const int32_t *term_atom, const double *term_w,
                       double *U, int U_on_device, uint64_t *degenerate);

/*
 * The sums behind the first- and second-rank orientational time-correlation functions, at every lag:
 *   sums[k][g][0] = sum over the series m of group g and t = 0 .. n-1-k of c,   sums[k][g][1] = the same sum of c * c,
 *   c = fma(uz, uz', fma(uy, uy', ux * ux')),  u = U[m][.][t], u' = U[m][.][t+k];  the second sum adds fma(c, c, S2).
 *   U          host|dev (U_on_device) [n_series][3][n], 1 <= n < 2^29
 *   group_off  host int64 [n_groups+1] contiguous series groups, 1 <= n_groups <= 16, ascending within [0, n_series];
 *              an empty group gives zeros
 *   max_lag    0 .. n-1
 *   sums       host|dev (sums_on_device) [max_lag+1][n_groups][2]
 * The caller forms C1 = S1 / W and C2 = 1.5 * S2 / W - 0.5 with W = (n - k) * (size of the group): P1 and P2 of the
 * cosine, averaged over molecules and time origins. Composing C2 from autocorrelations of the nine products u_a u_b
 * would take nine transforms per molecule and subtract large numbers; here every term is formed and squared directly.
 * For any order of summation |S1 - exact| <= (W + 3) * 2^-53 * sum |c| and |S2 - exact| <= (W + 7) * 2^-53 * sum c * c
 * over the given U. No floating-point atomics: the terms of a lag are added in an order fixed by n, max_lag, the
 * groups and the device's compute-unit count; results are bit-identical from call to call. A NaN in a series of group g
 * reaches group g only. n_series * (n * max_lag - max_lag^2 / 2) window positions of five FP64 operations: FP64-bound.
 * Any n_series; launch dimensions stay below 65535 along the series and time slabs.
 * n_groups outside 1..16, n outside 1..2^29-1, max_lag outside 0..n-1, n_series < 0, a group_off that does not ascend
 * within [0, n_series] or a NULL array: MDHIP_EINVAL before anything is written.
 */
int mdhip_orient_corr(mdhip_ctx *ctx, int64_t n, int64_t n_series, const double *U, int U_on_device, int n_groups,
                      const int64_t *group_off, int64_t max_lag, double *sums, int sums_on_device);

/* ---- dihedral angles (structural/dihedral_distribution.py; no counterpart in the reference) ---- */
/*
 * Intramolecular torsions i-j-k-l: their histograms per row and / or their series (cos phi, sin phi, 0), time-major —
 * the input of mdhip_orient_corr, whose S1 then is the sum of cos(phi(t+k) - phi(t)): the torsional autocorrelation.
 *   x          host|dev (x_on_device) [n_frames][3][n_atoms], atoms by id, molecules contiguous (as mdhip_axis_vectors)
 *   box        host [n_frames][3] edge lengths, or NULL: x is unwrapped
 *   jobs       job j covers job_mols[j] molecules of job_len[j] atoms each, the first one starting at atom job_atom0[j]
 *              (host [n_jobs]); job_quad host [n_jobs][4]: the atoms i j k l, 0-based inside the molecule, within
 *              [0, job_len) and pairwise different; job_row host [n_jobs]: the histogram row the job adds to, within
 *              [0, n_rows), 1 <= n_rows <= 16 (several jobs may share a row: pooled torsions)
 *   n_bins     even, 2 .. 1440: bins of D = 360 / n_bins degrees over [-180, 180)
 *   cos_edges  host [n_bins / 2]: cos(m * D) as the host evaluates it, strictly decreasing (entry 0 is not read)
 *   hist       host uint64 [n_rows][n_bins], or NULL: no histogram (cos_edges may be NULL then)
 *   U          host|dev (U_on_device) [n_series][3][n_frames], n_series = sum of job_mols, series numbered job after
 *              job, molecule after molecule; or NULL: no series
 *   degenerate host uint64 [n_jobs]
 * hist and degenerate hold THIS call's counts (they are not accumulated into: the host adds batches).
 * Per (job, molecule, frame), a the molecule's first atom, every operation an IEEE double operation, nothing fused,
 * sqrt and division correctly rounded:
 *   per axis  b1 = w(x[a+j] - x[a+i]),  b2 = w(x[a+k] - x[a+j]),  b3 = w(x[a+l] - x[a+k]);  w is the single strict wrap
 *             of the siblings, w(d) = d > L/2 ? d - L : (d < -L/2 ? d + L : d) (a NaN shifts nothing), the identity when
 *             box == NULL. Each bond difference is wrapped on its own: correct whenever consecutive named atoms lie
 *             within half a box edge of each other, as bonded atoms do; the molecule's first atom is not involved
 *             unless it is named;
 *   n1 = b1 x b2, n2 = b2 x b3, every component p*q - r*s as two products and one subtraction:
 *             (u x v)_x = uy*vz - uz*vy, (u x v)_y = uz*vx - ux*vz, (u x v)_z = ux*vy - uy*vx;
 *   dot(u, v) = (ux*vx + uy*vy) + uz*vz;
 *   l1 = sqrt(dot(n1, n1)), l2 = sqrt(dot(n2, n2)), lb = sqrt(dot(b2, b2)), den = l1 * l2;
 *   c = dot(n1, n2) / den                                                         (cos phi)
 *   s = dot(b1, n2)                  (the sign of sin phi; IUPAC: cis = 0, trans = 180, right-hand rule about j -> k)
 *   sn = (s * lb) / den                                                           (sin phi)
 *   den == 0 (three of the four atoms collinear or coincident): degenerate[job] += 1, no bin, U = (0, 0, 0);
 *   else c or s NaN (non-finite input): no bin, nothing counted, U = (NaN, NaN, 0);
 *   else m = the number of q in [1, n_bins/2) with c <= cos_edges[q] — no acos, no atan2, no clamp: a cosine an ulp
 *             outside +-1 lands in the first or last half-bin —, bin = s >= 0 ? n_bins/2 + m : n_bins/2 - 1 - m,
 *             hist[job_row][bin] += 1 and U = (c, sn, 0).
 * The bins mirror each other about 0: |phi| in [m D, (m+1) D) on either side. The positive half is left-closed as usual,
 * the NEGATIVE HALF IS RIGHT-CLOSED: bin n_bins/2 - 1 - m holds -(m+1) D < phi <= -m D, except that s == +-0 counts as
 * the positive side, so exactly 0 falls in bin n_bins/2 and exactly 180 in the last bin.
 * Atoms that no quadruple names are never read: a NaN there does not leak.
 * A workgroup owns 64 molecules x 64 frames (the tile of mdhip_axis_vectors: lane = molecule while reading, the two
 * components through a padded LDS tile, lane = frame while writing); counts go to an LDS histogram of the workgroup
 * and from there once into 64-bit device bins, with integer atomics only: exact, and independent of the order. Jobs
 * with the same (job_atom0, job_mols, job_len) are worked by the same workgroup one after the other, so their lines
 * come from HBM once (and from the caches for the further jobs). One read of the lines that hold named atoms, one
 * write of U when asked: a single job per molecule type runs at the HBM rate (DESIGN 4.13c has the measured cost of
 * pooled ones). Any number of frames and molecules, up to 2^20 jobs: launch dimensions over 65535 are split inside
 * the call.
 * n_jobs < 1 (or > 2^20), n_rows outside 1..16, a job_row outside [0, n_rows), n_bins odd or outside 2..1440, a
 * quadruple entry outside [0, job_len) or repeated, a job that runs past n_atoms, hist and U both NULL, cos_edges NULL
 * (or not strictly decreasing) while hist is not, any other NULL array: MDHIP_EINVAL before anything is written.
 */
int mdhip_dihedral_angles(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                          const double *box, int n_jobs, const int64_t *job_atom0, const int64_t *job_mols,
                          const int32_t *job_len, const int32_t *job_quad, const int32_t *job_row, int n_rows, int n_bins,
                          const double *cos_edges, uint64_t *hist, double *U, int U_on_device, uint64_t *degenerate);

/* ---- orientational pair correlations and the dielectric constant (structural/orientational_correlation.py,
 *      structural/dielectric.py; no counterpart in the reference) ---- */
/*
 * Per-molecule sites and vectors, FRAME-major — the input of mdhip_vector_pair_hist — and the per-frame totals of the
 * vectors (the total dipole M of a molecule type).
 *   x          host|dev (x_on_device) [n_frames][3][n_atoms], atoms by id, molecules contiguous (as mdhip_axis_vectors)
 *   box        host [n_frames][3] edge lengths, or NULL: x is unwrapped
 *   jobs       job j covers job_mols[j] molecules of job_len[j] atoms each, the first one starting at atom job_atom0[j]
 *              (host [n_jobs]). It has two term lists in the form of mdhip_axis_vectors, the SITE terms (site_off
 *              [n_jobs+1] starting at 0, site_atom, site_w) and the VECTOR terms (vec_off, vec_atom, vec_w): pairs (k, w)
 *              with 1 <= k < job_len[j], k strictly ascending within a list. Either list may be empty.
 *   job_unit   host int32 [n_jobs], 0 or 1: 1 normalises the job's vectors
 *   site, vec  host|dev (out_on_device, one flag for both) [n_frames][3][n_series], n_series = sum of job_mols, series
 *              numbered job after job, molecule after molecule; either may be NULL: not written
 *   total      host [n_jobs][3][n_frames], or NULL: the sum of the job's vectors AS WRITTEN, per frame and axis
 *   sq_total   host [n_jobs][n_frames], or NULL: the sum over the job's molecules of (vx*vx + vy*vy) + vz*vz of the
 *              vectors as written
 *   degenerate host uint64 [n_jobs]: the (molecule, frame) pairs of a job with job_unit set whose vector is exactly zero
 * For a molecule whose first atom is a, per axis, every operation an IEEE double operation, nothing fused:
 *   d_k = w(x[a+k] - x[a]); w is the single strict wrap of the siblings, w(d) = d > L/2 ? d - L : (d < -L/2 ? d + L : d)
 *         with L/2 formed as L / 2 (a NaN shifts nothing), the identity when box == NULL;
 *   o = sum_k w_k * d_k over the site terms in ascending k, one multiplication and one addition per term, starting from
 *         w_1 * d_1;  site = x[a] + o — with no site terms site = x[a] itself, untouched. The site is NOT folded into the
 *         box (mdhip_vector_pair_hist takes the nearest image from any image);
 *   v = the same sum over the vector terms; with no vector terms v = (0, 0, 0), which is never counted as degenerate;
 *   job_unit (and at least one vector term): n2 = (vx*vx + vy*vy) + vz*vz, v = v / sqrt(n2), three divisions by the
 *         correctly rounded root. n2 == 0 gives (0, 0, 0) and +1 in degenerate[j]; a non-finite n2 gives three NaN
 *         components and is not counted: the rules of mdhip_axis_vectors.
 * Atoms that no term names, the first atom apart, are never read: a NaN there does not leak.
 * A centre of mass is the site terms (k, m_k / M), a named atom k is the term (k, 1); a raw dipole about the first atom
 * is the vector terms (k, q_k) with job_unit 0, a unit bond vector (tail, -1), (head, +1) with job_unit 1.
 * Totals: per (job, frame) 256 partial sums per quantity, partial i adding the molecules i, i + 256, ... of the job in
 * order, and a fixed tree over them (red[i] += red[i + w], w = 128 .. 1), as mdhip_collective_displacement: the order
 * depends on the job's size alone, no floating-point atomics, every call gives the same bits. A NaN stays in its own
 * job, frame and axis (and in that job's and frame's sq_total).
 * Lane = molecule on both sides (reads one molecule apart, writes consecutive): one read of the lines that hold named
 * atoms, one write of the two outputs: HBM-bound. Any number of frames, molecules and jobs (up to 2^20): launch
 * dimensions over 65535 are split inside the call.
 * n_jobs < 1, a NULL array among x, the job arrays, the offsets, job_unit and degenerate (a term array may be NULL when
 * its list is empty for every job), a job that runs past n_atoms, a list of job_len terms or more, k outside
 * [1, job_len) or not strictly ascending, a job_unit other than 0 or 1: MDHIP_EINVAL before anything is written.
 */
int mdhip_mol_moments(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                      const double *box, int n_jobs, const int64_t *job_atom0, const int64_t *job_mols,
                      const int32_t *job_len, const int64_t *site_off, const int32_t *site_atom, const double *site_w,
                      const int64_t *vec_off, const int32_t *vec_atom, const double *vec_w, const int32_t *job_unit,
                      double *site, double *vec, int out_on_device, double *total, double *sq_total,
                      uint64_t *degenerate);

/*
 * Distance-resolved orientational pair sums: per bin of the site-site distance the number of pairs and the exact sums
 * of cos(theta), cos^2(theta) between the two vectors and of the cosine of vector j against the direction i -> j.
 *   site, vec  host|dev (in_on_device, one flag for both) [n_frames][3][n_ent], as mdhip_mol_moments writes them
 *   box        host [n_frames][3] edge lengths; required
 *   group_off  host int64 [n_groups+1] contiguous entity groups; empty groups are allowed
 *   jobs       host int32 [n_jobs][2] = (group a, group b)
 *   edges      host [nbins+1] from mdhip_bin_edges, or NULL to have it computed from bin_size; 1 <= nbins <= 4096
 * Per frame f, for every i in a and every j in b with j != i as entity indices; every operation an IEEE double
 * operation, nothing fused, sqrt and division correctly rounded:
 *   per axis  inv = 1.0 / L with L = box[f][axis];  d = site_j - site_i;  d = d - L * rint(d * inv), rint rounding half
 *             to even: the nearest image from ANY image of either site (sites outside the box are fine); at an exact
 *             tie (d * inv = +-0.5) nothing shifts;
 *   rsq = (dx*dx + dy*dy) + dz*dz;
 *   rsq < edges[nbins]: bin = (int64)(sqrt(rsq) / bin_size), decided by comparing rsq with the edge table (never by a
 *             device sqrt), hist[job][bin] += 1; every other pair — a NaN or infinite rsq, hence a NaN site or a box
 *             edge of 0, included — counts in beyond[job] and nowhere else.
 * For a binned pair:
 *   c  = (vxi*vxj + vyi*vyj) + vzi*vzj
 *   c2 = c * c
 *   e  = ((dx*vxj + dy*vyj) + dz*vzj) / sqrt(rsq)          (the vector of j against the direction i -> j)
 * If all three are finite and each has magnitude < 2, the pair adds (int64) rint(value * 4294967296.0) to each of its
 * three sums (fixed point, 32 fractional bits: the product is exact, rint rounds half to even, |addend| < 2^33).
 * Otherwise it adds to none of them and counts in unsummed[job]: coincident sites (rsq == 0, e = 0/0), a NaN vector, a
 * vector far from unit length.
 *   hist       host uint64 [n_jobs][nbins]
 *   sums       host uint64 [n_jobs][3][nbins][2]: (c, c2, e) x bin x (low word, high word) of the exact 128-bit
 *              two's-complement integer sum of the addends; no precondition on sizes is needed
 *   beyond, unsummed, pairs  host uint64 [n_jobs]; pairs = n_frames * (N_a * N_b - (a == b ? N_a : 0))
 *              = sum(hist[job]) + beyond[job]; an unsummed pair is inside hist
 * Pairs are ordered as in mdhip_van_hove_distinct: for a == b every unordered pair is visited twice, and e differs
 * between the two visits (c and c2 do not); for a != b once.
 * Why fixed point: the project adds nothing with floating-point atomics, and a floating-point sum would depend on the
 * order in which workgroups finish. Integer addition is associative: all outputs are integers, exact, and independent
 * of the launch geometry; the caller divides once, on the host.
 * The group that fills its tiles of 64 better lies along the lanes (six values in registers), the other comes through
 * uniform addresses (scalar loads); which is which changes nothing in the results: d, and with it e, change sign
 * exactly. The cutoff compare comes first; the payload, the sqrt and the division run only for pairs inside it. A
 * workgroup holds its job's row in LDS (a uint32 count and three int64 sums per bin, 28 bytes: 112 KiB at 4096 bins),
 * added with LDS integer atomics and flushed with 64-bit integer atomics: low word, carry when the add wrapped, sign
 * extension. At most 2^29 pairs per workgroup between zeroing and flushing: 2^29 * 2^33 < 2^63. Any number of frames,
 * entities and jobs: launch dimensions over 65535 are split inside the call. Complete on return.
 * NULL box, a group index out of range, nbins outside [1, 4096], a bin_size that is not positive and finite, edges that
 * do not start at 0 and ascend, a group_off that does not ascend within [0, n_ent], a NULL array: MDHIP_EINVAL before
 * anything is written.
 */
int mdhip_vector_pair_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *site, const double *vec,
                           int in_on_device, const double *box, int n_groups, const int64_t *group_off, int n_jobs,
                           const int32_t *jobs, double bin_size, int32_t nbins, const double *edges, uint64_t *hist,
                           uint64_t *sums, uint64_t *beyond, uint64_t *unsummed, uint64_t *pairs);

/* ---- molecular shape (structural/molecular_shape.py; no counterpart in the reference) ---- */
/*
 * The shape of flexible molecules: per (job, molecule, frame) the mass-weighted gyration tensor about the centre of mass,
 * the radius of gyration squared Rg2, the end-to-end distance squared Ree2, the second invariant I2, the relative shape
 * anisotropy k2 (kappa^2) and the principal moments l1 >= l2 >= l3; their histograms, per-frame totals and, when asked,
 * the values themselves.
 *   x          host|dev (x_on_device) [n_frames][3][n_atoms], atoms by id, molecules contiguous (as mdhip_axis_vectors)
 *   box        host [n_frames][3] edge lengths, or NULL: x is unwrapped
 *   jobs       job j covers job_mols[j] molecules of job_len[j] >= 1 atoms each, the first one starting at atom
 *              job_atom0[j] (host [n_jobs]): one molecule type
 *   w_off, w   host int64 [n_jobs+1], host double: the weight row of job j — the masses of one molecule's atoms — is
 *              w[w_off[j] .. w_off[j+1]); w_off[0] = 0 and w_off[j+1] - w_off[j] = job_len[j]
 *   job_ends   host int32 [n_jobs][2]: the end atoms (e0, e1), 0-based inside the molecule, within [0, job_len)
 *   unwrap     1: positions follow the chain; 0: every atom against the molecule's first atom (see below)
 *   nbins, bin_size, edges   the histograms of Rg and Ree: 1 <= nbins <= 4096 bins of bin_size; edges host [nbins+1] from
 *              mdhip_bin_edges, or NULL to have it computed from bin_size
 *   n_kbins    1 .. 1024 bins of k2 over [0, 1]
 * Outputs — THIS call's values (nothing is accumulated into: the host adds batches); any may be NULL, not all:
 *   hist_rg, hist_ee  host uint64 [n_jobs][nbins]
 *   hist_k     host uint64 [n_jobs][n_kbins]
 *   beyond     host uint64 [n_jobs][2]: the (molecule, frame) pairs whose Rg2 ([0]) or Ree2 ([1]) has no bin
 *   degenerate host uint64 [n_jobs]: those with Rg2 == 0
 *   totals     host double [n_jobs][9][n_frames]: per frame the sums over the job's molecules of Rg2, sqrt(Rg2), Ree2,
 *              l1, l2, l3, k2, I2 and Rg2 * Rg2
 *   per_mol    host|dev (per_mol_on_device) [n_frames][6][n_series]: Rg2, Ree2, k2, l1, l2, l3; n_series = sum of
 *              job_mols, series numbered job after job, molecule after molecule
 * Per (job, molecule, frame), a the molecule's first atom, w_k its weights, every operation an IEEE double operation,
 * nothing fused, sqrt and division correctly rounded; per axis unless said otherwise:
 *   positions  p_0 = 0.0. unwrap = 1: p_k = p_(k-1) + w(x[a+k] - x[a+k-1]), k = 1, 2, ...: the chain is followed, right
 *              whenever CONSECUTIVE atoms lie within half a box edge of each other, however long the molecule is.
 *              unwrap = 0: p_k = w(x[a+k] - x[a]), the rule of mdhip_axis_vectors: right only while every atom lies
 *              within half an edge of the first. w is the single strict wrap of the siblings, w(d) = d > L/2 ? d - L :
 *              (d < -L/2 ? d + L : d) with L/2 formed as L / 2 (a NaN shifts nothing), the identity when box == NULL;
 *   mass       M = the sum of w_k in ascending k from 0.0, formed on the host;
 *   centre     s = 0.0; s = s + w_k * p_k in ascending k from k = 0;  c = s / M;
 *   tensor     q_k = p_k - c (the p_k formed again by the same operations); with t_a = w_k * q_ka, from 0.0 in ascending
 *              k: Gxx += t_x * q_kx, Gyy += t_y * q_ky, Gzz += t_z * q_kz, Gxy += t_x * q_ky, Gyz += t_y * q_kz,
 *              Gzx += t_z * q_kx; then each of the six is divided by M once;
 *   Rg2 = (Gxx + Gyy) + Gzz  (with weights >= 0 a sum of non-negative terms: never negative, 0 or more unless it is NaN);
 *   I2  = ((Gxx*Gyy + Gyy*Gzz) + Gzz*Gxx) - ((Gxy*Gxy + Gyz*Gyz) + Gzx*Gzx);
 *   k2  = 1.0 - (3.0 * I2) / (Rg2 * Rg2); with Rg2 == 0 (one atom, or all atoms with weight coincide): k2 = 0.0;
 *   Ree2 = (rx*rx + ry*ry) + rz*rz,  r = p_e1 - p_e0;
 *   principal moments: 5 sweeps of cyclic Jacobi over the pairs (x,y), (x,z), (y,z) in that order — +, -, *, / and sqrt
 *     only, no acos or cos. For the pair (p, q), r the third axis: skipped when G_pq == 0.0 exactly; otherwise
 *       theta = (G_qq - G_pp) / (2.0 * G_pq);   root = sqrt(theta * theta + 1.0);
 *       t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (-theta + root);
 *       c = 1.0 / sqrt(t * t + 1.0);  s = t * c;  u = t * G_pq;
 *       G_pp = G_pp - u;  G_qq = G_qq + u;  G_pq = 0.0;
 *       (G_rp, G_rq) = (c * G_rp - s * G_rq,  s * G_rp + c * G_rq), both from the values before the rotation;
 *     then (a, b, d) = (Gxx, Gyy, Gzz) go through `if (a < b) swap(a, b); if (b < d) swap(b, d); if (a < b) swap(a, b)`:
 *     l1 = a, l2 = b, l3 = d. 5 sweeps: four bring every tensor of tests/test_shape_cpu.py — nearly equal moments,
 *     planar and collinear molecules among them — to within 17 * 2^-53 * |G|_F of numpy.linalg.eigvalsh of the tensor
 *     accumulated in extended precision, where further sweeps change nothing; one more is kept in hand.
 *     When neither per_mol nor totals is asked for, the moments are not formed.
 * Counting:
 *   v = Rg2 into hist_rg[job], v = Ree2 into hist_ee[job]: when 0 <= v < edges[nbins] the bin (int)(sqrt(v) / bin_size),
 *     decided by comparing v with the edge table (never by a device sqrt); every other v — NaN and infinities included —
 *     counts in beyond[job][0 | 1] and nowhere else;
 *   Rg2 == 0: degenerate[job] += 1, k2 is not binned; else when k2 is finite: hist_k[job][b] += 1 with
 *     b = (int)(k2 * n_kbins) clamped to [0, n_kbins - 1]; else (NaN, infinite) nothing.
 *   So sum(hist_rg[j]) + beyond[j][0] = sum(hist_ee[j]) + beyond[j][1] = job_mols[j] * n_frames, and sum(hist_k[j]) +
 *   degenerate[j] + (the non-finite k2) the same.
 * per_mol holds the values as computed — a NaN or an infinity where the input gave one.
 * Totals: per (job, frame) 256 partial sums per quantity, partial i adding the values of the molecules i, i + 256, ...
 * of the job in order (sqrt(Rg2) and Rg2 * Rg2 formed from the Rg2 as written), and a fixed tree over them
 * (red[i] += red[i + w], w = 128 .. 1), as mdhip_mol_moments: no floating-point atomics, the same bits from call to call.
 * A NaN stays in its own job and frame.
 * A workgroup owns a run of whole molecules of one job that fits its LDS stage — at most 256 molecules and 1024 atoms —
 * and strides over the frames; per frame the run's three planes come in with coalesced loads into padded LDS, then one
 * lane per molecule walks its atoms there in index order. Molecules of more than 1024 atoms take one lane per
 * (molecule, frame) in global memory: the same operations in the same order, the same bits. Counts go through LDS bins
 * into 64-bit device bins with integer atomics only. Any number of frames (gridDim.y is capped at 65535, frames stride).
 * n_jobs < 1 (or > 2^20), a NULL input array, every output NULL, a job that runs past n_atoms, a weight row that does
 * not hold job_len weights or whose sum is not positive and finite, an end atom outside [0, job_len), nbins outside
 * 1..4096, n_kbins outside 1..1024, unwrap other than 0 or 1, a bin_size that is not positive and finite, edges that do
 * not start at 0 and ascend: MDHIP_EINVAL before anything is written.
 */
int mdhip_mol_shape(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device, const double *box,
                    int n_jobs, const int64_t *job_atom0, const int64_t *job_mols, const int32_t *job_len,
                    const int64_t *w_off, const double *w, const int32_t *job_ends, int unwrap, double bin_size,
                    int32_t nbins, const double *edges, int32_t n_kbins, uint64_t *hist_rg, uint64_t *hist_ee,
                    uint64_t *hist_k, uint64_t *beyond, uint64_t *degenerate, double *totals, double *per_mol,
                    int per_mol_on_device);

/* ---- free volume and cavity sizes (structural/free_volume.py, calc_free_volume; no counterpart in the reference) ---- */
/*
 * For every point of a regular grid laid over the periodic cell of every frame: the distance s to the nearest atom
 * SURFACE (atoms are spheres of their class's radius), which atom that is, and counts of these over all points and frames.
 *   xyz        host|dev (xyz_on_device) [n_frames][3][n_atoms]; wrapped, unwrapped, negative or many boxes away
 *   box        host [n_frames][3]: the orthorhombic edge lengths of every frame, each positive and finite
 *   atom_class host int32 [n_atoms], each in [0, n_classes), or -1: the atom is ignored
 *   radius     host [n_classes], finite and >= 0;  1 <= n_classes <= 16
 *   grid       host int32 [3] = (gx, gy, gz), each >= 1, G = gx * gy * gz <= 2^27; the same for every frame
 *   r_search, r_search_sq   the search radius and its square AS THE CALLER FORMS THEM: r_search positive and finite,
 *              r_search_sq == r_search * r_search as doubles
 *   edges      host [nbins + 1], edges[0] == 0, strictly ascending, finite; 1 <= nbins <= 4096
 *   probe      host [n_probes], each finite, 0 <= probe[k] <= edges[nbins]; 1 <= n_probes <= 8
 * Outputs — THIS call's values; any may be NULL, not all:
 *   hist       host uint64 [n_classes][nbins]
 *   occupied   host uint64 [n_classes]
 *   beyond     host uint64 [1]
 *   n_free     host int64 [n_frames][n_probes]
 *   free_map   host uint32 [G], point (i, j, k) at (i * gy + j) * gz + k
 *   s_out      host|dev (field_on_device) double [n_frames][G];  nearest_out  host|dev (the same flag) int32 [n_frames][G]
 * Every operation is an IEEE double operation, nothing fused, division and sqrt correctly rounded; per frame f with the
 * edges L_a = box[f][a]:
 *   atom       an atom whose class is -1, or with a coordinate that is NaN or infinite, is seen by no point. Every other
 *              atom j is brought into the cell once per axis:  s = x / L;  f = s - floor(s);  f = f < 1 ? f : 0;
 *              xw = f * L  (the wrapped fraction of the spatial sort of the pair path);
 *   point      (i, j, k), 0 <= i_a < g_a, lies at p_a = ((i_a + 0.5) / g_a) * L_a: the grid is fractional and anchored
 *              at coordinate 0 (only edge lengths are known; a rigid shift of the grid changes no statistic);
 *   distance   per axis a = |p - xw|, d = min(a, |a - L|) (the single wrap of the shell searches: for two positions in
 *              [0, L] the exact minimum image at any search radius);  rsq = (dx*dx + dy*dy) + dz*dz.
 *              Atom j is a CANDIDATE of the point iff rsq < r_search_sq, strictly; then s_j = sqrt(rsq) - radius[class_j];
 *   value      s = the minimum of s_j over the candidates, nearest = the LOWEST atom index among those that attain it
 *              (a minimum over the pairs (s_j, j): independent of the order in which atoms are met);
 *              lining = atom_class[nearest]. Without a candidate s = +inf and nearest = -1.
 * Counting over all frames and points, each point in exactly one place:
 *   s < 0:                           occupied[lining] += 1
 *   edges[b] <= s < edges[b + 1]:    hist[lining][b] += 1   (by comparison with the edge table, never by a division)
 *   otherwise (no candidate, or s >= edges[nbins]):  beyond[0] += 1
 * so sum(hist) + sum(occupied) + beyond[0] == n_frames * G.
 *   n_free[f][k] = the points of frame f without a candidate or with s >= probe[k] (probe 0: the geometric free volume;
 *   a point exactly on a sphere's surface is free);  free_map[point] = the frames in which it is free for probe[0].
 * How it runs (csrc/cell_plan.h, csrc/free_volume.hip): per frame the atoms are counting-sorted into a grid of
 * nc_x * nc_y * nc_z cells, nc_a the largest count in [1, 64] whose cell edge L_a / nc_a is at least
 * r_search * (1 + 2^-20) — so nc differs from frame to frame when the box does —; a workgroup takes the grid points that
 * lie in one cell (in bricks of 1024), stages the atoms of the up to 27 DISTINCT neighbouring cells in LDS in chunks of
 * 1024 and every lane carries the running (s, index) minimum of its four points. Counts go through 32-bit LDS bins (when
 * n_classes * nbins + n_classes + 1 <= 6144, else straight) into 64-bit device cells with integer atomics only: the
 * results do not depend on the cells, the bricks or the order of arrival. Frames are worked in batches bounded by the
 * workspace (about 1 GiB, or the option "free_volume_batch"; host-resident xyz is copied batch by batch); no launch dimension grows with n_frames or G.
 * n_frames < 1, n_atoms outside [1, 2^31), n_classes outside 1..16, nbins outside 1..4096, n_probes outside 1..8, a
 * g_a < 1 or G > 2^27, a probe that is negative, not finite or above edges[nbins], a radius that is negative or not
 * finite, a class outside [-1, n_classes), a box edge that is not positive and finite, r_search not positive and finite
 * or r_search_sq not its square, edges that do not start at 0 and ascend, a NULL input array, every output NULL:
 * MDHIP_EINVAL before anything is written.
 */
int mdhip_free_volume(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                      const double *box, const int32_t *atom_class, int32_t n_classes, const double *radius,
                      const int32_t *grid, double r_search, double r_search_sq, int32_t nbins, const double *edges,
                      int32_t n_probes, const double *probe, uint64_t *hist, uint64_t *occupied, uint64_t *beyond,
                      int64_t *n_free, uint32_t *free_map, double *s_out, int32_t *nearest_out, int field_on_device);

/* ---- velocity autocorrelation and power spectrum (dynamical/velocity_correlation.py, class VelocityCorrelation; no
 *      counterpart in the reference) ---- */
/*
 * Per-group lag sums and power spectra of the series s_e,a(t) = coef[e] * v[t][a][e], a = x, y, z:
 *   sums[k][g][a]  = sum over the entities e of group g and t = 0 .. n_frames-1-k of s_e,a(t) * s_e,a(t+k)
 *   power[g][a][j] = sum over the entities e of group g of |sum_t s_e,a(t) e^{-2 pi i j t / L}|^2, unnormalised
 *   a0[g][a]       = sum over the entities e of group g and all t of s_e,a(t)^2
 * Column 3 of each is the total, (x + y) + z of the finished values.
 *   v          host|dev (v_on_device) [n_frames][3][n_ent], frames in time order: the layout every trajectory call reads
 *   coef       host [n_ent], or NULL: 1. One multiplication per sample; the results are those of the rounded products
 *              (sqrt(mass) gives the mass-weighted spectrum)
 *   ent_group  host int32 [n_ent], values -1 .. n_groups-1; -1: the entity is in no group and enters no sum. Groups need
 *              not be contiguous (atom types inside molecules); 1 <= n_groups <= 16; an empty group gives zeros
 *   L          the padded transform length: a power of two, 4 <= L < 2^30, L >= n_frames + max_lag (at equality the
 *              circular correlation is still the linear one); 0 <= max_lag <= n_frames-1
 *   sums       host|dev (out_on_device) [max_lag+1][n_groups][4]
 *   power      NULL, or host|dev (out_on_device) [n_groups][4][L/2+1]
 *   a0         host [n_groups][4]: formed directly, without a transform — the scale of the error bounds; always returned
 * The work goes in batches bounded by the context option lag_batch_mb: a batch is one axis of a range of consecutive
 * entities with ALL their groups, so that every line of the trajectory is read once however the groups are interleaved.
 * The batch is read through 64 x 64 tiles, entities along the lanes, and written as whole time-major rows in the order
 * (group, entity ascending) inside the batch's buffer, every group a contiguous range of rows there. The rows go through
 * the shared FP64 transforms (two passes, the second fused with the column sums of |X|^2 over a group's rows, where the
 * length allows; else the packed transform and its column sums); the partial spectra of splits and batches are added in
 * a fixed order, one inverse transform over the 3 * n_groups summed spectra gives the lag sums. The launches that
 * mdhip_last_kernel_ms reports for this call are its batches (each: one gather, one forward transform, its column sums).
 * Error: |sums[k][g][a] - exact| <= 4 * 2^-52 * log2(L) * a0[g][a] at every lag (|S(k)| <= S(0) = a0: unlike the MSD, the
 * autocorrelation has no conditioning problem and needs no exact fallback); for series without a dominant line
 * |power - exact| <= 4 * 2^-52 * log2(L) * sqrt(n_frames) * a0.
 * No floating-point atomics: the order of every sum is fixed by the shape, the options and the device's compute-unit
 * count; results are bit-identical from call to call. Non-finite samples: see "Non-finite input" above.
 * Any n_frames and n_ent (n_frames * n_ent below 2^40); launch dimensions over 65535 are split inside the call.
 * n_groups outside 1..16, n_frames < 1, n_ent < 0, an ent_group value outside -1..n_groups-1, L no power of two, outside
 * [4, 2^30) or below n_frames + max_lag, max_lag outside 0..n_frames-1, a NULL v, ent_group, sums or a0: MDHIP_EINVAL before
 * anything is written. n_ent == 0 gives zeros.
 */
int mdhip_velocity_spectrum(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *v, int v_on_device,
                            const double *coef, int n_groups, const int32_t *ent_group, int64_t L, int64_t max_lag,
                            double *sums, double *power, int out_on_device, double *a0);

/*
 * Replaces, for the inputs of the path, the un-vendored pymatgen `parse_lammps_dumps` + pandas
 * `read_csv` the reference uses (call sites structural/rdf_cn.py:176, dynamical/diffusion.py:172,
 * dynamical/conductivity.py:87). A file may hold several frames. Numbers are the correctly rounded
 * doubles of their text (identical to pandas for the <= 15 significant digits LAMMPS writes).
 */
typedef struct mdhip_dump mdhip_dump;
int mdhip_dump_open(const char *path, mdhip_dump **out); /* mmap + index the frames */
void mdhip_dump_close(mdhip_dump *d);
const char *mdhip_dump_error(mdhip_dump *d); /* d == NULL: error of the last failed open */
int64_t mdhip_dump_n_frames(mdhip_dump *d);
/* Header of frame f: bounds6 = xlo xhi ylo yhi zlo zhi as written, tilt3 = xy xz yz when triclinic;
 * columns = the names after "ITEM: ATOMS", space separated. Any output pointer may be NULL. */
int mdhip_dump_frame_info(mdhip_dump *d, int64_t f, int64_t *timestep, int64_t *natoms, double *bounds6,
                          double *tilt3, int *triclinic, int *n_cols, char *columns, int columns_len);
/* Columns col_idx[0..n_sel) of frame f as SoA planes out[n_sel][natoms], rows ordered by ascending value
 * of column sort_col (stable; e.g. the id column, as `sort_values("id")` in rdf_cn.py:192) or in file
 * order when sort_col < 0. Parsing is split over n_threads host threads. */
int mdhip_dump_read(mdhip_dump *d, int64_t f, int n_sel, const int32_t *col_idx, int sort_col, double *out,
                    int n_threads);

/* As mdhip_dump_read, with one destination plane [natoms] per selected column: outs[s] may point anywhere — the
 * streaming layer parses x, y, z straight into a slot of a page-locked batch buffer (mdhip_host_alloc) and the ids
 * and types into arrays of their own, so that no copy stands between the text and the H2D transfer. */
int mdhip_dump_read_cols(mdhip_dump *d, int64_t f, int n_sel, const int32_t *col_idx, int sort_col,
                         double *const *outs, int n_threads);

/*
 * MANY single-frame dump files in one call (the per-timestep files LAMMPS writes; the reference's glob pattern,
 * rdf_cn.py:176): file k is opened, indexed and parsed by one of n_threads host threads, column s of its atoms going to
 * dst[s] + k * dst_stride[s] (doubles), rows ordered by ascending sort_name (NULL: file order) — e.g. x, y, z straight
 * into frame slot k of a page-locked batch buffer [n_files][3][n_atoms] and the ids into a table of their own. Columns
 * are found by NAME in every file. timesteps [n_files], bounds6 [n_files][6] (as written), tilt3 [n_files][3],
 * triclinic [n_files]: headers, any may be NULL. Returns MDHIP_OK; a negative MDHIP_E* code with the first failure's
 * text in err; or 1 when some file is not ONE frame of n_atoms atoms with all the requested columns (err says which):
 * the caller then reads that batch frame by frame (mdhip_dump_open / mdhip_dump_read_cols).
 * cmp_equal (may be NULL) [n_files]: 1 where column cmp_sel of the file equals, bit for bit, cmp_ref [n_atoms] — or
 * the same column of the FIRST file when cmp_ref is NULL. The reference re-derives the atom types of every frame
 * (rdf_cn.py:462-470); a caller that knows they did not change skips that per-frame work.
 */
int mdhip_dump_read_files(const char *const *paths, int n_files, int n_sel, const char *const *col_names,
                          const char *sort_name, int64_t n_atoms, double *const *dst, const int64_t *dst_stride,
                          int64_t *timesteps, double *bounds6, double *tilt3, int32_t *triclinic, int n_threads,
                          char *err, int err_len, int cmp_sel, const double *cmp_ref, int32_t *cmp_equal);

/* ---- native LAMMPS log reader (host only) ---------------------------------------------------- */
/*
 * Role of pymatgen's parse_lammps_log (un-vendored; call sites dynamical/viscosity.py:211,
 * utilities/log.py:21, dynamical/diffusion.py:241): one thermo table per `run`, between the line starting with
 * "Memory usage per processor =" / "Per MPI rank memory allocation" and the line starting with "Loop time of";
 * first line = column names; lines starting with "WARNING" and blank lines are skipped. Numbers are parsed as in
 * the dump reader (correctly rounded). `regular` = 0 when some row is not one number per column (the caller then
 * falls back to its text reader for exact pandas behaviour). mdhip_log_read fills column planes
 * out[n_cols][n_rows]; is_int[c] = 1 when every token of column c is a plain integer (pandas makes it int64).
 */
typedef struct mdhip_log mdhip_log;
int mdhip_log_open(const char *path, mdhip_log **out);
void mdhip_log_close(mdhip_log *l);
const char *mdhip_log_error(mdhip_log *l); /* l == NULL: error of the last failed open */
int64_t mdhip_log_n_runs(mdhip_log *l);
int mdhip_log_run_info(mdhip_log *l, int64_t run, int64_t *n_rows, int *n_cols, int *regular, char *names,
                       int names_len);
int mdhip_log_read(mdhip_log *l, int64_t run, double *out, int32_t *is_int, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* MDHIP_H */
