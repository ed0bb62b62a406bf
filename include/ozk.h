/* ozk.h — C ABI of the MI355X-native BN254 MSM / FFT back end.
 *
 * This is the drop-in boundary: one shared library,
 * libozk_hip.so, with plain-C entry points (pointers + sizes, no torch / HIP
 * types).  Each `*_host` function takes exactly the byte buffers the reference's
 * JNI native receives and returns exactly the bytes it returns; the three JNI
 * shim libraries (include/ozk_jni.h) only move bytes between the JVM and these.
 * Each `*_dev` function is the same operation on buffers already resident in HBM
 * (device pointers), asynchronous on `stream`, for callers that keep data on the
 * GPU (bench.py, the prove harness, torch.distributed ranks).
 *
 * Wire formats (all integers canonical, NON-Montgomery, value < modulus):
 *   scalar / Fr element in : 32 B little-endian  (VariableBaseMSM.java:121-131)
 *   G1 point in            : X|Y|Z, 3 x 32 B LE  (VariableBaseMSM.java:221-228)
 *   G2 point in            : X.c0|X.c1|Y.c0|Y.c1|Z.c0|Z.c1, 6 x 32 B LE
 *                                                (bn254a/BN254aG2.java:77-86)
 *   var-MSM / FFT out      : 64 B LE per coordinate, upper 32 B zero
 *                                                (VariableBaseMSM.java:239-258)
 *   fixed-base / field out : 64 B BIG-endian per coordinate
 *                                                (algebra_msm_FixedBaseMSM.cu:783-787)
 * Returned points are affine-normalised Jacobian triples (X/Z^2, Y/Z^3, 1); the
 * point at infinity is (0, 1, 0) as BNG1.toAffineCoordinates (BNG1.java:163-172).
 *
 * Every function returns 0 on success and a negative OZK_E_* code on failure;
 * ozk_last_error() gives the message for the calling thread.  Nothing here ever
 * falls back to a CPU path: without a usable GPU the calls fail with
 * OZK_E_NO_DEVICE.
 */
#ifndef OZK_H
#define OZK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OZK_OK 0
#define OZK_E_INVALID -1    /* bad argument (null pointer, n <= 0, not a power of two ...) */
#define OZK_E_NO_DEVICE -2  /* no HIP device / device call failed */
#define OZK_E_NOMEM -3      /* device or host allocation failed */
#define OZK_E_INTERNAL -4

#define OZK_G1 1 /* `type` / `BNType` value for G1; to the `*_host` entries anything else is G2, as in the reference */
#define OZK_G2 2

const char* ozk_last_error(void);
/* 2.  (1 had one entry per variant of the staged MSM — ozk_var_msm_head_dev, _tail_dev, _sort_dev and _accum_dev
 * took fewer arguments — so a caller bound to those four names must check this before it calls them.) */
int ozk_version(void);
/* number of visible HIP devices (0 if none); `taskID % count` selects the device as
 * the reference does (algebra_msm_VariableBaseMSM.cu:1249-1257). */
int ozk_device_count(void);
/* Streams confined to compute units [first_cu, first_cu + n_cus) of the current device (hipExtStreamCreateWithCUMask;
 * ozk_device_cu_count() = the device's compute units, 256 on an MI355X), for callers that partition the chip between
 * the stages of consecutive MSMs (device.VarMsmPipeline3(tail_cus=...): tails on a few units, the accumulation on the
 * rest).  Such a stream is a BLOCKING stream: it synchronises with the null stream, so nothing of a schedule that
 * uses it may run there.  ozk_stream_destroy gives it back. */
int ozk_device_cu_count(void);
int ozk_stream_create_cu_range(int32_t first_cu, int32_t n_cus, void** stream);
int ozk_stream_destroy(void* stream);
/* The OZK_* tuning environment variables are read once per process and cached (a plan must not change
 * between the workspace-size query and the run); tests and tuning scripts call this after changing one. */
int ozk_tuning_reload(void);
/* The `*_host` entry points keep their streams, device arena and pinned staging buffers in a per-device
 * pool between calls (the reference allocates and frees inside every native call,
 * algebra_msm_VariableBaseMSM.cu:1292-1303,1405-1409).  This gives everything back. */
int ozk_host_cache_release(void);
/* Where the wall time of the calling thread's last `*_host` call went: stats10 = {context acquire, arena growth,
 * waits for a pinned staging buffer, host memcpy into the ring, host memcpy out of it, enqueueing copies,
 * stream synchronisation} in milliseconds, the number of staging waits and of host memcpys, and the call's total
 * time as the library saw it (entry to context release).  (How a call that takes several times its median is
 * attributed — to one of the library's waits, or to the caller's side of the boundary — tools/host_jitter.py.) */
int ozk_host_call_stats(double* stats10);

/* ---------------- VariableBaseMSM ---------------------------------------
 * replaces Java_algebra_msm_VariableBaseMSM_variableBaseSerialMSMNativeHelper
 * (algebra_msm_VariableBaseMSM.h:13-16, .cu:1614-1695).
 * bases: n x 96 B (G1) or n x 192 B (G2); scalars: n x 32 B; out: 192 B / 384 B. */
int ozk_var_msm_host(const uint8_t* bases, const uint8_t* scalars, int32_t n, int32_t type,
                     int32_t task_id, uint8_t* out);
/* replaces ..._variableBaseDoubleMSMNativeHelper (.h:21-24, .cu:1712-1788).
 * out: 576 B = G1 result (192) || G2 result (384). */
int ozk_var_double_msm_host(const uint8_t* bases_g1, const uint8_t* bases_g2,
                            const uint8_t* scalars, int32_t n, int32_t task_id, uint8_t* out);

/* The same MSM spread over several GPUs from ONE call (no counterpart in the reference, whose native uses the
 * one device `taskID % count` selects, algebra_msm_VariableBaseMSM.cu:1249-1257; its multi-GPU form is one
 * Spark partition per device, VariableBaseMSM.java:775-786): the index range is cut into `shards` contiguous
 * slices (<= 0: one per visible device), slice i runs on device i % count from its own host thread, the
 * partial results are added on device 0.  Same bytes out as ozk_var_msm_host.  ozk_var_msm_auto_host is what
 * the JNI shim calls: ozk_var_msm_host on device taskID % count, as the reference; with OZK_SHARD=1 (opt-in, for a
 * serial prover that is the only caller) calls of n >= OZK_SHARD_MIN_N (2^21) pairs are sharded over the visible
 * devices instead.  Unverified on multi-GPU hardware (every box seen so far had one GPU). */
int ozk_var_msm_sharded_host(const uint8_t* bases, const uint8_t* scalars, int32_t n, int32_t type, int32_t shards,
                             uint8_t* out);
int ozk_var_msm_auto_host(const uint8_t* bases, const uint8_t* scalars, int32_t n, int32_t type, int32_t task_id,
                          uint8_t* out);
/* The double MSM the same way (VariableBaseMSM.distributedDoubleMSM, VariableBaseMSM.java:805-818: per-partition
 * doubleMSM + reduce(add)): out = 576 B, G1 (192) || G2 (384); ozk_var_double_msm_auto_host is what the JNI native
 * calls (ozk_var_double_msm_host unless OZK_SHARD=1, as above). */
int ozk_var_double_msm_sharded_host(const uint8_t* bases_g1, const uint8_t* bases_g2, const uint8_t* scalars, int32_t n,
                                    int32_t shards, uint8_t* out);
int ozk_var_double_msm_auto_host(const uint8_t* bases_g1, const uint8_t* bases_g2, const uint8_t* scalars, int32_t n,
                                 int32_t task_id, uint8_t* out);
/* The partial results of a sharded call meet through an RCCL all-gather over xGMI (communicators made once per process
 * by ncclCommInitAll over the devices in use; librccl is bound at run time) followed by a HIP point sum on device 0 —
 * or, when RCCL is absent, fails to initialise, is busy with another sharded call or OZK_SHARD_RCCL=0, through the
 * host.  Same bytes either way.  ozk_shard_last_exchange(): how the calling thread's last sharded call did it
 * (1 = RCCL, 0 = host, -1 = a single shard / no call yet).  ozk_shard_comms_release() drops the communicators. */
int ozk_shard_last_exchange(void);
void ozk_shard_comms_release(void);

/* ---------------- the device-resident MSM --------------------------------
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default); everything is asynchronous on it.
 * n in [1, 2^24].  `type` is OZK_G1 or OZK_G2: any other value is OZK_E_INVALID here (size queries: 0), unlike the
 * `*_host` entries.  From whole to parts:
 *     ozk_var_msm_dev  ==  head | tail  ==  sort | accumulate | tail
 *
 * The whole MSM on one stream.  `d_workspace` must hold ozk_var_msm_workspace_bytes(n, type) bytes. */
size_t ozk_var_msm_workspace_bytes(int32_t n, int32_t type);
int ozk_var_msm_dev(const void* d_bases, const void* d_scalars, int32_t n, int32_t type,
                    void* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* The same MSM in two phases, for callers that keep several MSMs in flight (a Groth16 prove
 * has six independent ones): the HEAD is the throughput-bound part (sort, bucket accumulation,
 * first window-sum level) and leaves its result in `d_tail` (ozk_var_msm_tail_bytes bytes);
 * the TAIL is the latency-bound remainder (upper window-sum levels, Horner over the windows,
 * normalisation; a few lanes busy for ~2 ms) and reads nothing but `d_tail`.  Running the tail
 * on a second stream lets the next MSM's head (which may reuse the same workspace) overlap
 * it.  ozk_var_msm_dev == head + tail on one stream.
 * d_bases: wire-in points, or, with prepared != 0, the records of ozk_var_msm_prepare_dev.  d_workspace:
 * ozk_var_msm_head_workspace_bytes bytes.  previous_levels_done and levels_done are ordering events (below) and may
 * be NULL; mode is the shape of the tail's window sums (below): 0 latency, anything else throughput. */
size_t ozk_var_msm_head_workspace_bytes(int32_t n, int32_t type);
size_t ozk_var_msm_tail_bytes(int32_t n, int32_t type);
int ozk_var_msm_head_dev(const void* d_bases, int32_t prepared, const void* d_scalars, int32_t n, int32_t type,
                         void* d_workspace, size_t workspace_bytes, void* d_tail, size_t tail_bytes, void* stream,
                         void* previous_levels_done);
int ozk_var_msm_tail_dev(int32_t n, int32_t type, void* d_tail, size_t tail_bytes, void* d_out, void* stream,
                         void* levels_done, int32_t mode);

/* The head itself has two stages that stress different units — SORT (base conversion, digits,
 * counting sort: HBM / LDS) and ACCUMULATE (bucket accumulation ... first window-sum level:
 * vector ALU) — so a caller may pipeline three stages (sort of MSM k+2 | accumulate of k+1 |
 * tail of k).  The hand-off between them is the "sorted set" (double-buffer it); sort and
 * accumulate each have private scratch.  ozk_var_msm_head_dev == sort + accumulate.  (On
 * MI355X the three-stage form measures 562-574 Mscalar-mul/s at 2^20 against 576 for head | tail: the
 * sort kernels cannot co-reside with three accumulation blocks per CU and stretch the accumulation
 * when they can — profiles/r02_schedule_experiments.txt.)
 * ozk_var_msm_stage_bytes gives the sizes of the three buffers. */
int ozk_var_msm_stage_bytes(int32_t n, int32_t type, size_t* sorted_bytes, size_t* sort_ws_bytes,
                            size_t* accum_ws_bytes);
/* Where the staged entries put what one stage hands to the next, for tests and diagnostics that read those buffers
 * back.  Host only (no device is needed); the plan and the layouts are the ones the entries below use, under the
 * tuning knobs in force.  Fills fields[0 .. OZK_VAR_MSM_STAGE_LAYOUT_FIELDS), `count` being the room in `fields`:
 *    0 points sorted (n, or 2 n with GLV)   1 glv   2 signed digits   3 c   4 cb (bucket bits per window)   5 W
 *    6 small_sort (the one-launch sort)   7 L1 (entries per level-1 lane)   8 l1_whole as planned
 *    9 lo_bits   10 NH (coarse bins per window)   11 nblk (sort chunks)   12 big_thresh (a coarse bin above it is
 *      split over many blocks)
 *   13 aff (-1 with prepared != 0: the records are the caller's)   14 hist   15 total   16 sent: byte offsets into the
 *      sorted set — affine records of AFF_WORDS words, one count per bucket (W << cb of them, bucket id =
 *      window << cb | bucket), four counters (total[0] = sorted entries), the entries (index | sign << 31, bucket id)
 *   17 buckets   18 hist_t: byte offsets into the tail buffer — records of REC_WORDS words, the copy of the counts
 *   19 AFF_WORDS   20 REC_WORDS   21 REC_TAG (word of a bucket record that says XYZZ = 0 or Jacobian = 1)
 * Bad arguments (n outside [1, 2^24], NULL, count too small, unknown type): OZK_E_INVALID. */
#define OZK_VAR_MSM_STAGE_LAYOUT_FIELDS 22
int ozk_var_msm_stage_layout(int32_t n, int32_t type, int32_t prepared, int64_t* fields, int32_t count);
/* d_bases and prepared as for the head; over prepared bases the sort skips the base conversion */
int ozk_var_msm_sort_dev(const void* d_bases, int32_t prepared, const void* d_scalars, int32_t n, int32_t type,
                         void* d_sorted, size_t sorted_bytes, void* d_sort_ws, size_t sort_ws_bytes, void* stream);
/* d_prepared: the prepared records the sort read, or NULL (bases converted by the sort).
 * part splits the stage for a caller that keeps level 1 (the vector-ALU-bound kernel) back to back on one stream
 * and runs the rest (run merge, the short generic levels, the copy of the bucket counts: ~0.1 ms of low-occupancy work)
 * elsewhere: 0 = all of it, 1 = level 1 only, 2 = the rest (same arguments; it reads the sorted set and the accumulate
 * scratch level 1 wrote, so neither may be reused before it has run).  Any other part: OZK_E_INVALID. */
int ozk_var_msm_accum_dev(const void* d_prepared, int32_t n, int32_t type, void* d_sorted, size_t sorted_bytes,
                          void* d_accum_ws, size_t accum_ws_bytes, void* d_tail, size_t tail_bytes, void* stream,
                          int32_t part);

/* ---- prepared bases (no counterpart in the reference, which re-marshals and
 * re-uploads the proving key for every MSM, VariableBaseMSM.java:224-227).  The bases are converted once
 * to the affine Montgomery records the accumulation kernel gathers (with the GLV plan: both halves,
 * 2n x 64 | 128 B) and stay in HBM; an MSM over them skips the conversion and the 96 | 192 B per base of
 * host-to-device traffic.  Results are byte-identical to ozk_var_msm_host on the same inputs.
 *   device form: ozk_var_msm_prepare_dev once into ozk_var_msm_prepared_bytes bytes, then ozk_var_msm_prepared_dev
 *               (the whole MSM) or the stages above with prepared != 0. */
size_t ozk_var_msm_prepared_bytes(int32_t n, int32_t type);
int ozk_var_msm_prepare_dev(const void* d_bases, int32_t n, int32_t type, void* d_prepared, size_t prepared_size,
                            void* stream);
int ozk_var_msm_prepared_dev(const void* d_prepared, const void* d_scalars, int32_t n, int32_t type, void* d_out,
                             void* d_workspace, size_t workspace_bytes, void* stream);
/*   host form : handle = create(bases) ; msm(handle, scalars) any number of times ; destroy(handle).
 *               A handle serialises its MSMs (internal mutex); use one handle per concurrent caller.  As every
 *               `*_host` entry, create takes any type other than OZK_G1 as G2. */
int ozk_bases_create_host(const uint8_t* bases, int32_t n, int32_t type, int32_t task_id, void** handle);
int ozk_var_msm_bases_host(void* handle, const uint8_t* scalars, int32_t n, uint8_t* out);
int ozk_bases_destroy(void* handle);
/* OZK_G1 / OZK_G2 for a live handle, 0 for a stale or released one.  A handle is a token into a generation-
 * checked table, not a pointer: a late call with a released (or forged) handle fails with OZK_E_INVALID, and
 * ozk_bases_destroy really frees everything — at once, or when the MSM still running on the handle returns. */
int ozk_bases_type(void* handle);

/* Ordering hint for several MSMs in flight on two streams.  A tail given `levels_done` records it after its first
 * window-sum level; a head given the
 * same event as `previous_levels_done` waits for it after its sort and before its bucket accumulation, so that the
 * previous MSM's wave-cooperative level is resident before the accumulation takes three of the four wave slots of
 * every SIMD.  Measured at 2^20: 576 Mscalar-mul/s (538 with the late event; 576 with no event at all — the hint no
 * longer buys throughput since the accumulation kernel leaves a slot free, it only keeps the order deterministic).
 * Events come from ozk_order_event_create (a HIP event underneath). */
int ozk_order_event_create(void** ev);
int ozk_order_event_destroy(void* ev);

/* The tail's window sums come in two shapes (csrc/msm_var_driver.cuh, tail_shape), chosen by the `mode` of
 * ozk_var_msm_tail_dev: LATENCY (mode 0: fused first level + wave-cooperative levels, the fewest dependent additions;
 * also what ozk_var_msm_dev and the host entry points use) and THROUGHPUT (mode 1: serial levels, 3.0 instead of 5.25
 * additions per bucket, ~40 dependent additions longer).  A caller that keeps the chip busy with other
 * work — a prover with five MSMs and a witness map in flight — picks throughput: every addition saved is vector-ALU
 * time for something else (a 2^20-constraint proof: 16.6 -> 16.3 ms). */

/* sum of k affine-normalised partial results in wire-out format (k x 192 B / 384 B), as
 * produced by ozk_var_msm_dev on k ranks -> one normalised point.  The multi-GPU
 * reduce(GroupT::add) of VariableBaseMSM.java:777-783 after the RCCL all-gather. */
int ozk_points_sum_dev(const void* d_points, int32_t k, int32_t type, void* d_out, void* stream);

/* The sharded Groth16 proof from the gathered per-rank partials (zksnark.ShardedProver): d_records holds `world`
 * records of 768 B, A_r (G1, 192) | B_r (G2, 384) | C_r (G1, 192) in wire-out format, in rank order; d_proof receives
 * A | B | C (768 B), each part the normalised sum over the ranks (infinity as (0, 1, 0)) — the bytes three
 * ozk_points_sum_dev calls would write.  One launch, the three sums on their own waves.  world < 1: OZK_E_INVALID. */
int ozk_groth16_combine_dev(const void* d_records, int32_t world, void* d_proof, void* stream);

/* Measurement hooks (bench.py): timing of the dominant kernel (the level-1 bucket accumulation,
 * k_segreduce<.., true> or k_l1_whole) per launch.  ozk_prof_enable(2): the kernel's own waves stamp the device's constant-rate
 * clock (first wave start -> last wave end), which leaves the schedule untouched; ozk_prof_enable(1): HIP start /
 * stop events on the dispatch (16 + k: on every (k+1)-th launch only) — exact too, but an event-carrying dispatch
 * costs the three-stage schedule 4-13 % of its throughput, so bench.py uses it as a cross-check in a second pass;
 * 0: off (the recorded launches stay readable).  ozk_prof_dominant_kernel_ms returns the mean duration over the
 * launches since the last enable, _stats the distribution.  ozk_var_msm_plan reports the window size the library
 * picks for n. */
int ozk_prof_enable(int on);
int ozk_prof_dominant_kernel_ms(double* avg_ms, int* launches);
/* stats4 = {mean, median, min, max} in ms (the box-to-box spread of the pool is ~10 %, so a single mean cannot
 * tell a 5 % gain from a slower box) */
int ozk_prof_dominant_kernel_stats(double* stats4, int* launches);
/* stats4 = {mean, median, min, max} over the launches recorded since ozk_prof_enable(2) of the SHADER clock in MHz
 * each launch ran at (shader-clock / constant-rate ticks stamped inside the kernel): what makes kernel times of two
 * boxes or two rounds comparable.  Profiling is single-device and serialised: launches on other devices than the one
 * current at ozk_prof_enable are not recorded; concurrent callers are safe. */
int ozk_prof_dominant_kernel_clock_mhz(double* stats4, int* launches);
/* ticks per millisecond of the device clock, calibrated against the host's steady clock by the first
 * ozk_prof_enable(2) (MI355X: 100 011.8 kHz for a nominal 100 MHz); 0 before that */
double ozk_prof_clock_khz(void);
int ozk_var_msm_plan(int32_t n, int32_t* window_bits, int32_t* windows);
/* 1 when the MSM of n pairs runs as 2n half-length pairs through the GLV endomorphism (the windows
 * reported above then cover 128 bits); 0 otherwise (n > 2^23 or OZK_MSM_GLV=0). */
int ozk_var_msm_glv(int32_t n);
/* Which level-1 path the calling thread's most recent variable-base MSM (or accumulate stage) took, for tests and
 * profiles: 1 = whole buckets on lane groups, 0 = fixed chunks and the run merge, -1 = no MSM on this thread yet.
 * A whole-bucket plan is decided on the device (a bucket too long for its lane group, or a skewed sort bin, sends
 * the MSM down the chunked path): the call waits for the device and reads the flag from the MSM's sorted set, so ask
 * before the next MSM sorts into the same buffers. */
int ozk_var_msm_last_l1_path(void);
/* Which form of the window sums the calling thread's last variable-base tail launched: 1 = by bucket rows and columns
 * (G1, throughput shape, OZK_MSM_TAIL_RC), 0 = the fused / serial levels, -1 = no call yet.  For tests and profiles. */
int ozk_var_msm_last_tail_form(void);

/* Synthetic inputs for benchmarks / full-size tests (BASELINE.md config 2 generator):
 * writes n G1 bases P_i = k_i * G, k_i = splitmix64(seed + i) (k_i = 1 if that is 0), in the
 * wire-in format (affine, Z = 1).  Not part of the reference's surface. */
int ozk_gen_bases_dev(uint64_t seed, int32_t n, int32_t type, void* d_out_wire, void* stream);

/* ---------------- FixedBaseMSM ------------------------------------------
 * replaces Java_algebra_msm_FixedBaseMSM_batchMSMNativeHelper
 * (algebra_msm_FixedBaseMSM.h:13-16, .cu:1276-1384).  out: n x 192 B / n x 384 B (BE). */
int ozk_fixed_batch_msm_host(int32_t outerc, int32_t window_size, int32_t out_len,
                             int32_t inner_len, int32_t n, int32_t scalar_size,
                             const uint8_t* base, const uint8_t* scalars, int32_t bn_type,
                             int32_t task_id, uint8_t* out);
/* replaces ..._doubleBatchMSMNativeHelper (.h:21-24, .cu:1395-1491).
 * out: n x 576 B, per element G1 (3 x 64 BE) || G2 (6 x 64 BE). */
int ozk_fixed_double_batch_msm_host(int32_t outerc1, int32_t window_size1, int32_t outerc2,
                                    int32_t window_size2, int32_t out_len1, int32_t inner_len1,
                                    int32_t out_len2, int32_t inner_len2, int32_t n,
                                    const uint8_t* base_g1, const uint8_t* base_g2,
                                    const uint8_t* scalars, int32_t task_id, uint8_t* out);
/* replaces ..._fieldBatchMSMNativeHelper (.h:29-32, .cu:1500-1558).
 * in: (n+1) x 32 B LE, element n is the multiplier; out: n x 64 B BE, x_i * b mod r. */
int ozk_field_batch_mul_host(const uint8_t* in, int32_t n, int32_t task_id, uint8_t* out);

/* Scalars are any 256-bit words.  When the caller's windows cover a whole Fr scalar (outerc * window_size >= 254) the
 * result is (s mod r) B in every form of the kernels; with fewer bits of windows it is (s mod 2^(outerc *
 * window_size)) B for the word as written, the reference's rule (FixedBaseMSM.java:146-164). */
size_t ozk_fixed_batch_msm_workspace_bytes(int32_t outerc, int32_t window_size, int32_t n,
                                           int32_t bn_type);
/* The plan a call of this shape runs under the tuning knobs in force, for tests and profiles (host only, no device
 * work): *form = 0 plain windows over the word (outerc * window_size < 254, or OZK_MSM_GLV=0), 1 GLV split with the
 * Jacobian gather-add (OZK_FB_AFFINE=0), 2 GLV split over affine table records (the default); *table_window = the
 * window bits of the table that is built (the caller's in the plain form; in the GLV forms the cost model's choice
 * or OZK_FB_WS, never more than the caller's: a forced value outside [1, window_size] gives window_size);
 * *windows = the windows gathered per digit string (outerc, or ceil(128 / *table_window)).  Any of the three
 * pointers may be null.  OZK_E_INVALID for a shape the entry points reject. */
int ozk_fixed_batch_msm_plan(int32_t outerc, int32_t window_size, int32_t n, int32_t* form, int32_t* table_window,
                             int32_t* windows);
int ozk_fixed_batch_msm_dev(int32_t outerc, int32_t window_size, int32_t n, const void* d_base,
                            const void* d_scalars, int32_t bn_type, void* d_out,
                            void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_field_batch_mul_dev(const void* d_in, int32_t n, void* d_out, void* stream);
/* Compact output (no counterpart in the reference, whose natives return 64-byte
 * big-endian coordinates, algebra_msm_FixedBaseMSM.cu:783-787, i.e. 2x the bytes, and whose Java then
 * re-marshals every key element for each proof, VariableBaseMSM.java:221-228): the same points, written
 * as X|Y|Z 32-byte LITTLE-endian values — n x 96 B (G1) / n x 192 B (G2), exactly the wire-IN format of
 * the variable-base natives, so a proving key goes from the setup to the prover as it is. */
int ozk_fixed_batch_msm_compact_dev(int32_t outerc, int32_t window_size, int32_t n, const void* d_base,
                                    const void* d_scalars, int32_t bn_type, void* d_out, void* d_workspace,
                                    size_t workspace_bytes, void* stream);
int ozk_fixed_batch_msm_compact_host(int32_t outerc, int32_t window_size, int32_t n, const uint8_t* base,
                                     const uint8_t* scalars, int32_t bn_type, int32_t task_id, uint8_t* out);
/* Device-resident scalars and results, the base point given as HOST bytes (wire format, 96 / 192 B): the window
 * table — what the reference's Java side computes once per key element (getWindowTable, FixedBaseMSM.java:71-99) and
 * its native side rebuilds inside every call (algebra_msm_FixedBaseMSM.cu:851-992) — comes from a per-device cache
 * keyed by the base, so the second and later batches over one generator skip the doubling chain and the table
 * (0.65 / 2.1 ms of a 2.0 / 5.5 ms G1 / G2 call at 2^20).  The `*_host` entry points use the same cache.
 * compact != 0: the 32-byte little-endian layout of ozk_fixed_batch_msm_compact_dev.  Workspace:
 * ozk_fixed_batch_msm_workspace_bytes.  ozk_host_cache_release() frees the cached tables. */
int ozk_fixed_batch_msm_base_dev(int32_t outerc, int32_t window_size, int32_t n, const uint8_t* base_host,
                                 const void* d_scalars, int32_t bn_type, void* d_out, int32_t compact,
                                 void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------- radix-2 FFT over Fr -----------------------------------
 * replaces Java_algebra_fft_FFTAuxiliary_serialRadix2FFTNativeHelper
 * (algebra_fft_FFTAuxiliary.h:13-16, .cu:219-260) = FFTAuxiliary.serialRadix2FFT
 * (FFTAuxiliary.java:60-124).  in: n x 32 B LE (the shim flattens the List<byte[]>),
 * omega: 32 B LE, out: n x 64 B LE.  n must be a power of two (n == 1: copy). */
int ozk_fft_host(const uint8_t* in, int32_t n, const uint8_t* omega, int32_t task_id,
                 uint8_t* out);
size_t ozk_fft_workspace_bytes(int32_t n);
/* d_in: n x 32 B LE, d_out: n x 64 B LE (may not alias d_in). */
int ozk_fft_dev(const void* d_in, int32_t n, const uint8_t* omega_host32, void* d_out,
                void* d_workspace, size_t workspace_bytes, void* stream);
/* Compact form: one flat buffer in, n x 32 B LE out (the reference's native walks a
 * java.util.List<byte[]> with one JNI call per element and returns 64-byte values,
 * algebra_fft_FFTAuxiliary.cu:228-255). */
int ozk_fft_compact_host(const uint8_t* in, int32_t n, const uint8_t* omega, int32_t task_id, uint8_t* out);
int ozk_fft_compact_dev(const void* d_in, int32_t n, const uint8_t* omega_host32, void* d_out,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------- QAP witness map (the FFT path's caller) -------------
 * What R1CStoQAP.R1CStoQAPWitness (reductions/r1cs_to_qap/R1CStoQAP.java:163-230) does between the
 * constraint evaluations and the H query of the prover: 3 inverse FFTs, 3 coset FFTs, (A o B - C) / Z on
 * the coset (SerialFFT.java:86-115,158-163; FFTAuxiliary.multiplyByCoset :224-232), 1 coset inverse FFT,
 * one trailing zero — seven transforms and the pointwise stages without leaving HBM.  There is no JNI
 * native for it in the reference (Java loops over List<Fp>); INTEGRATION.md shows the optional binding.
 * A, B, C: m x 32 B LE (evaluations on the domain S, m a power of two >= 2); omega: the domain's root of
 * unity (SerialFFT.java:24-28), g: the coset shift (Fp.multiplicativeGenerator), 32 B LE each;
 * H: (m + 1) x 32 B LE coefficients (canonical).  */
/* The step before: the constraint evaluations themselves (R1CStoQAP.java:143-160,195-199 with
 * LinearCombination.evaluate, relations/objects/LinearCombination.java:39-50 — a term with variable index 0
 * contributes `one` whatever its coefficient).  A sparse matrix in CSR form resident in HBM — row_ptr: rows + 1
 * u32 offsets, index: u32 variable indices, coeff: 32-byte LE coefficients, one per term, or NULL when every
 * coefficient is one — times the assignment (32-byte LE elements): out[i] = sum over row i, rows x 32 B LE,
 * canonical.  long_rows lists the rows with more than 64 terms (n_long of them, u32): each is cut into 64
 * slices summed by one workgroup each (workspace: ozk_r1cs_evaluate_workspace_bytes(n_long)); the caller finds
 * them once per R1CS from row_ptr.  Device pointers; asynchronous on `stream`. */
size_t ozk_r1cs_evaluate_workspace_bytes(int32_t n_long);
int ozk_r1cs_evaluate_dev(const void* d_row_ptr, const void* d_index, const void* d_coeff, const void* d_assignment,
                          int32_t rows, const void* d_long_rows, int32_t n_long, void* d_out, void* d_workspace,
                          size_t workspace_bytes, void* stream);
/* ---------------- QAP instance of the setup (R1CStoQAP.R1CStoQAPRelation,
 * reductions/r1cs_to_qap/R1CStoQAP.java:37-98; SerialSetup.java:50-74,146-151) — pieces, all device-resident:
 *   ozk_qap_lagrange_dev    L_i(t) for the radix-2 domain of size m (FFTAuxiliary.serialRadix2LagrangeCoefficients,
 *                           FFTAuxiliary.java:250-302; one shared inversion per 8 coefficients instead of m inversions)
 *                           and Z(t) = t^m - 1.  t must not lie in the domain (t^m != 1: the caller checks).
 *   ozk_sparse_mat_vec_dev  out = M v for a CSR matrix in HBM: At / Bt / Ct are the TRANSPOSED constraint matrices
 *                           (input-consistency rows appended to A) times the Lagrange vector.  Same layout and
 *                           long-row list as ozk_r1cs_evaluate_dev, without its rule for variable 0.
 *   ozk_fr_powers_dev       out[i] = base^i k  (Ht, and the H query's scalars t^i Z / delta)
 *   ozk_fr_lincomb3_dev     out[i] = (ka a_i + kb b_i + c_i) kk  (the gammaABC / deltaABC scalars)
 * All vectors are n x 32-byte little-endian canonical values; 32-byte host arguments are LE canonical too. */
size_t ozk_qap_lagrange_workspace_bytes(int32_t m);
int ozk_qap_lagrange_dev(const uint8_t* t_host32, const uint8_t* omega_host32, int32_t m, void* d_out, void* d_zt,
                         void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_sparse_mat_vec_dev(const void* d_row_ptr, const void* d_index, const void* d_coeff, const void* d_vec,
                           int32_t rows, const void* d_long_rows, int32_t n_long, void* d_out, void* d_workspace,
                           size_t workspace_bytes, void* stream);
size_t ozk_fr_powers_workspace_bytes(int32_t n);
int ozk_fr_powers_dev(const uint8_t* base_host32, const uint8_t* k_host32, int32_t n, void* d_out, void* d_workspace,
                      size_t workspace_bytes, void* stream);
int ozk_fr_lincomb3_dev(const void* d_a, const void* d_b, const void* d_c, int32_t n, const uint8_t* ka_host32,
                        const uint8_t* kb_host32, const uint8_t* kk_host32, void* d_out, void* d_scratch96, void* stream);
int ozk_qap_witness_host(const uint8_t* A, const uint8_t* B, const uint8_t* C, int32_t m, const uint8_t* omega,
                         const uint8_t* g, int32_t task_id, uint8_t* H);
size_t ozk_qap_witness_workspace_bytes(int32_t m);
int ozk_qap_witness_dev(const void* d_A, const void* d_B, const void* d_C, int32_t m, const uint8_t* omega_host32,
                        const uint8_t* g_host32, void* d_H, void* d_workspace, size_t workspace_bytes,
                        void* stream);

/* The BN254a optimal-ate pairing and the Groth16 verifier (BNPairing.java, zkSNARK/Verifier.java:24-59), one pairing
 * per lane.  No JNI native: the reference's verifier is Java.
 *
 * Formats.  Pairing inputs are wire-in points (G1 96 B, G2 192 B, any Z); they are normalised as toAffineCoordinates
 * does, a point at infinity (Z = 0) becoming (0, 1, 0) (BNG1.java:163-172, BNG2.java:168-177), and the Java's
 * arithmetic then runs on those coordinates: P at infinity gives the Java's value; Q at infinity makes the Miller
 * value zero, where the Java throws, and gives 384 zero bytes.  GT values are 384 B: twelve 32-byte little-endian canonical Fq values in the Java's nesting order
 * c0.c0.c0, c0.c0.c1, c0.c1.c0, c0.c1.c1, c0.c2.c0, c0.c2.c1, c1.c0.c0, ..., c1.c2.c1
 * (Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (9 + u)), Fq2 = Fq[u]/(u^2 + 1)).
 *
 *   ozk_pairing_g2_prepared_bytes  bytes of the line coefficients of n G2 points (102 triples of Fq2, ~22 KB each)
 *   ozk_pairing_g2_prepare_dev     precomputeG2 of n wire-in G2 points into d_prep (opaque layout)
 *   ozk_reduced_pairing_dev        d_gt[i] = reducedPairing(P_i, Q_i) for n pairs; d_q_or_prep holds n wire-in G2
 *                                  points (prepared = 0) or n prepared points (prepared = 1)
 *   ozk_groth16_verify_dev         k proofs: d_proofs k x 768 B records A | B | C in wire-out format (the layout of
 *                                  ozk_groth16_combine_dev), d_abc k x 192 B wire-out evaluationABC points,
 *                                  d_alpha_beta one GT value, d_gamma_prep / d_delta_prep one prepared point each;
 *                                  d_ok[j] = 1 when Verifier.verify would return true, else 0 (also when a Miller
 *                                  value is zero, where the Java throws instead of returning)
 * n or k <= 0: OZK_E_INVALID.  Asynchronous on `stream`. */
size_t ozk_pairing_g2_prepared_bytes(int32_t n);
int ozk_pairing_g2_prepare_dev(const void* d_q, int32_t n, void* d_prep, size_t prep_bytes, void* stream);
int ozk_reduced_pairing_dev(const void* d_p, const void* d_q_or_prep, int32_t prepared, int32_t n, void* d_gt,
                            void* stream);
int ozk_groth16_verify_dev(const void* d_alpha_beta, const void* d_gamma_prep, const void* d_delta_prep,
                           const void* d_proofs, const void* d_abc, int32_t k, int32_t* d_ok, void* stream);

/* Products of pairings, GT powers and randomized batch verification of Groth16 proofs.
 *
 *   ozk_pairing_product_dev     d_gt (one GT value) = FE(prod_i ML(P_i, Q_i)) = prod_i reducedPairing(P_i, Q_i) for n
 *                               pairs in the formats of ozk_reduced_pairing_dev (a Q at infinity: 384 zero bytes)
 *   ozk_gt_pow_dev              d_out[i] = d_gt[i]^e_i for n GT values; d_exp holds n 32-byte little-endian integers
 *                               (any 256-bit value).  The inputs must lie in GT (results of reduced pairings): the
 *                               exponentiation squares with the cyclotomic squaring.
 *   ozk_groth16_wellformed_dev  d_flags[j] = 1 when proof j (768 B record A | B | C, wire-out) is well-formed: every
 *                               coordinate canonical (< q, upper 32 bytes zero), A and C on the curve with Z != 0
 *                               (G1 has cofactor 1), B on the twist with Z != 0 and [r]B = O; else 0
 *   ozk_groth16_verify_rlc_dev  k proofs as one check: d_gamma_abc the key's n wire-in gammaABC points (96 B each),
 *                               d_proofs k records, d_inputs k rows of n 32-byte little-endian primary inputs (taken
 *                               mod r), d_r k 32-byte weights.  Proof j is covered when it is well-formed and
 *                               0 < r_j < 2^128 (d_covered[j] = 1, else 0).  With s_i = sum_j r_j x_ji mod r over the
 *                               covered proofs, ABC* = sum_i s_i gammaABC_i, C* = sum_j r_j C_j and S = sum_j r_j:
 *                               *d_verdict = 1 when FE(prod_j ML(r_j A_j, B_j) (ML(ABC*, gamma) ML(C*, delta))^-1)
 *                               == alphaBeta^S, 0 when not (some covered proof fails Verifier.verify), -1 when the
 *                               check declines (ABC* or C* at infinity, e.g. no proof covered, or a zero Miller
 *                               value).  With the r_j uniform in [1, 2^128) and unknown to the prover, a verdict of 1
 *                               is wrong with probability at most 1 / (2^128 - 1).  Uncovered proofs are not judged.
 *                               stage_ms: nullptr, or five floats that receive the stage times (combination, MSMs,
 *                               Miller loops, product tree, final exponentiation); the call then waits for the stream.
 * n or k <= 0: OZK_E_INVALID.  Otherwise asynchronous on `stream`. */
int ozk_pairing_product_dev(const void* d_p, const void* d_q_or_prep, int32_t prepared, int32_t n, void* d_gt,
                            void* stream);
int ozk_gt_pow_dev(const void* d_gt, const void* d_exp, int32_t n, void* d_out, void* stream);
int ozk_groth16_wellformed_dev(const void* d_proofs, int32_t k, int32_t* d_flags, void* stream);
int ozk_groth16_verify_rlc_dev(const void* d_alpha_beta, const void* d_gamma_prep, const void* d_delta_prep,
                               const void* d_gamma_abc, int32_t n, const void* d_proofs, const void* d_inputs,
                               const void* d_r, int32_t k, int32_t* d_covered, int32_t* d_verdict, float* stage_ms,
                               void* stream);

/* BACE: batch arithmetic-circuit evaluation (the reference's bace/ package).  An instance is a
 * row of n inputs; d_inputs holds N instances row-major (value i n + j is input j of instance i), 32-byte
 * little-endian values (taken mod r).  N is a power of two, D = lowestPowerOfTwo(deg N) with N <= D <= 2^28, n <= 65535.
 * BACE programs (host memory, checked record by record before anything is enqueued): n_ops records of four int32
 * {op, dst, a, b}, run in order at every point:
 *     op 0 INPUT  slot[dst] = input a (0 <= a < n)        op 1 CONST  slot[dst] = consts[a] (0 <= a < n_consts)
 *     op 2 ADD    slot[dst] = slot[a] + slot[b]           op 3 MUL    slot[dst] = slot[a] * slot[b]
 * with 0 <= dst, a, b < n_slots; the value of the last record is the circuit's output.  consts: n_consts 32-byte LE
 * values (host memory).  Slots beyond OZK_BACE_LDS_SLOTS (default 16, at most 28; read once, ozk_tuning_reload) live
 * in the workspace, so query the workspace size after any change of that knob.
 *   ozk_bace_prove_dev        Prover.computeProof: d_proof = the D coefficients (D x 32 B, canonical) of
 *                             R(z) = C(beta_1(z), ..., beta_n(z)), beta_j the interpolant of column j on the N-point
 *                             domain.  Workspace: ozk_bace_workspace_bytes(n, N, D, n_ops, n_slots, n_consts).
 *   ozk_bace_evaluate_dev     NaiveEvaluator.getResult: d_out[i] = C(row i) for `rows` rows of n inputs (rows x 32 B).
 *                             Workspace: ozk_bace_evaluate_workspace_bytes(rows, n_ops, n_slots, n_consts).
 *   ozk_bace_columns_at_dev   d_out[j] = beta_j(r) for the n columns (n x 32 B); r: 32-byte LE host value (mod r).
 *                             Workspace: ozk_bace_workspace_bytes(n, N, N, 0, 0, 0).
 *   ozk_bace_result_dev       Verifier.getResult: d_out[i] = proof(omega_N^i), i < N (N x 32 B) for a proof of D
 *                             coefficients: the proof folded mod z^N - 1, then one transform of size N.
 *                             Workspace: ozk_bace_workspace_bytes(1, N, N, 0, 0, 0).
 *   ozk_fr_poly_eval_dev      d_out[y] = sum_i c_yi r^i (canonical) for npolys polynomials of len coefficients each
 *                             (32-byte LE, any 256-bit word: reduced mod r on load, like the rows of the KZG blocks
 *                             below, whose callers pass theirs here), polynomial y at d_coeffs + 32 y poly_stride
 *                             bytes; poly_stride is 0 (npolys = 1 only) or >= len, 1 <= npolys <= 65535, 1 <= len.
 *                             r: 32-byte LE host value.  Workspace: ozk_fr_poly_eval_workspace_bytes(npolys).
 * A size function returns 0 for a shape it rejects; the entry points return OZK_E_INVALID for it (N not a power of two,
 * D < N, D > 2^28, a malformed program, a short workspace).  All calls are asynchronous on `stream`. */
size_t ozk_bace_workspace_bytes(int32_t n, int32_t N, int32_t D, int32_t n_ops, int32_t n_slots, int32_t n_consts);
size_t ozk_bace_evaluate_workspace_bytes(int32_t rows, int32_t n_ops, int32_t n_slots, int32_t n_consts);
int ozk_bace_prove_dev(const void* d_inputs, int32_t n, int32_t N, const int32_t* program, int32_t n_ops,
                       int32_t n_slots, const uint8_t* consts, int32_t n_consts, int32_t D, void* d_proof,
                       void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_bace_evaluate_dev(const void* d_inputs, int32_t n, int32_t rows, const int32_t* program, int32_t n_ops,
                          int32_t n_slots, const uint8_t* consts, int32_t n_consts, void* d_out, void* d_workspace,
                          size_t workspace_bytes, void* stream);
int ozk_bace_columns_at_dev(const void* d_inputs, int32_t n, int32_t N, const uint8_t* r_host32, void* d_out,
                            void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_bace_result_dev(const void* d_proof, int32_t D, int32_t N, void* d_out, void* d_workspace,
                        size_t workspace_bytes, void* stream);
size_t ozk_fr_poly_eval_workspace_bytes(int32_t npolys);
int ozk_fr_poly_eval_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride,
                         const uint8_t* r_host32, void* d_out, void* d_workspace, size_t workspace_bytes,
                         void* stream);

/* KZG openings over Fr (csrc/kzg.cuh): the quotient (p(X) - p(z)) / (X - z) and the value p(z)
 * of npolys rows at once, and a weighted sum of rows.  Elements are 32-byte little-endian and 16-byte aligned, all in
 * HBM except omega; a value >= r is REDUCED mod r on load (coefficients, evaluations, points and weights alike), and
 * every output is canonical.  Strides count elements.
 *   ozk_fr_poly_open_dev      coefficient form.  Row y: p = the len coefficients at d_coeffs + 32 y poly_stride,
 *                             z = d_points[y]; d_values[y] = p(z), and the row at d_quot + 32 y quot_stride holds
 *                             q_0 .. q_{len-2} with q_{j-1} = p_j + z q_j, and element len - 1 = 0: an MSM scalar vector
 *                             of the same length over the same bases.  poly_stride is 0 (ONE polynomial opened at npolys
 *                             points) or >= len; quot_stride >= len, and elements of a row beyond len are not touched.
 *                             1 <= len, 1 <= npolys, npolys len <= 2^28.  d_quot must not overlap d_coeffs (rejected).
 *                             Workspace: ozk_fr_poly_open_workspace_bytes(npolys, len).
 *   ozk_fr_evals_open_dev     evaluation form.  Row y holds f_i = p(omega^i), i < n, in natural order; n is a power of
 *                             two, 2 <= n <= 2^28, npolys n <= 2^28; omega (32-byte LE, host memory, read before the
 *                             call returns) must have order exactly n (omega^(n/2) = -1 is checked on the host).
 *                             d_values[y] = p(z) and q_i = (f_i - p(z)) / (omega^i - z), the evaluations of the same
 *                             quotient; for z = omega^k: d_values[y] = f_k and q_k = -omega^-k sum_{i != k} q_i omega^i,
 *                             found and finished on the device.  evals_stride is 0 or >= n, quot_stride >= n; d_quot
 *                             must not overlap d_evals (rejected).
 *                             Workspace: ozk_fr_evals_open_workspace_bytes(npolys, n).
 *   ozk_fr_rows_combine_dev   d_out[j] = sum_{i < k} w_i rows[i][j], j < len: row i at d_rows + 32 i row_stride
 *                             (row_stride >= len), w = the k elements at d_weights.  d_out may be d_rows (the first
 *                             row); any other overlap is rejected.  k len <= 2^28.
 * A size function returns 0 for a shape it rejects; the entry points return OZK_E_INVALID for it before any launch (the
 * shape is checked before the pointers).  All calls are asynchronous on `stream`, allocate nothing and synchronise
 * nothing. */
size_t ozk_fr_poly_open_workspace_bytes(int32_t npolys, int32_t len);
int ozk_fr_poly_open_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride, const void* d_points,
                         void* d_quot, int64_t quot_stride, void* d_values, void* d_workspace, size_t workspace_bytes,
                         void* stream);
size_t ozk_fr_evals_open_workspace_bytes(int32_t npolys, int32_t n);
int ozk_fr_evals_open_dev(const void* d_evals, int32_t npolys, int32_t n, int64_t evals_stride,
                          const uint8_t* omega_host32, const void* d_points, void* d_quot, int64_t quot_stride,
                          void* d_values, void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_fr_rows_combine_dev(const void* d_rows, int32_t k, int32_t len, int64_t row_stride, const void* d_weights,
                            void* d_out, void* stream);

/* KZG set openings over Fr (csrc/kzg_set.cuh): for every row the quotient (p - I) / Z_S by the
 * vanishing polynomial Z_S = prod (X - z_i) of t pairwise distinct points, I the interpolant of p on them, and the t
 * values p(z_i).  Elements, reduction on load, canonical outputs, strides and the row layout are those of the block
 * above.  The points are npolys x t elements in HOST memory (32-byte LE, row y uses its own t), read before the call
 * returns; points of a row that are not pairwise distinct mod r are rejected on the host.
 *   ozk_fr_poly_open_set_dev   coefficient form, 1 <= t <= 32.  d_values[y t + i] = p(z_i); the row at
 *                              d_quot + 32 y quot_stride holds q_0 .. q_{len-t-1}, then zeros up to element len - 1 (all
 *                              zeros when len <= t): an MSM scalar vector over the same bases.  Dividing by the linear
 *                              factors in turn, every stage on the lane's registers: a row is read twice and written
 *                              once whatever t.  With t = 1 the bytes are those of ozk_fr_poly_open_dev.  npolys len and
 *                              npolys t <= 2^28; d_quot must not overlap d_coeffs (rejected).
 *                              Workspace: ozk_fr_poly_open_set_workspace_bytes(npolys, len, t).
 *   ozk_fr_evals_open_set_dev  evaluation form, 1 <= t <= 8, n and omega as ozk_fr_evals_open_dev.  q_i = (f_i -
 *                              I(omega^i)) / Z_S(omega^i), one inversion of Z_S(omega^i) per element.  EVERY point must lie
 *                              outside the domain: z^n = 1 is tested on the host and rejected (open such a set in
 *                              coefficient form).  With t = 1 the bytes are those of ozk_fr_evals_open_dev.
 *                              Workspace: ozk_fr_evals_open_set_workspace_bytes(npolys, n, t).
 * Size functions and rejections as above: 0 and OZK_E_INVALID before any launch, the shape (t included) before the
 * pointers.  Asynchronous on `stream`; nothing is allocated or synchronised. */
size_t ozk_fr_poly_open_set_workspace_bytes(int32_t npolys, int32_t len, int32_t t);
int ozk_fr_poly_open_set_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride, int32_t t,
                             const uint8_t* points_host, void* d_quot, int64_t quot_stride, void* d_values,
                             void* d_workspace, size_t workspace_bytes, void* stream);
size_t ozk_fr_evals_open_set_workspace_bytes(int32_t npolys, int32_t n, int32_t t);
int ozk_fr_evals_open_set_dev(const void* d_evals, int32_t npolys, int32_t n, int64_t evals_stride,
                              const uint8_t* omega_host32, int32_t t, const uint8_t* points_host, void* d_quot,
                              int64_t quot_stride, void* d_values, void* d_workspace, size_t workspace_bytes,
                              void* stream);

/* KZG multi-openings over Fr (csrc/kzg_multi.cuh): what a prover that opens many polynomials,
 * each at its own set of points, needs beside the entry points above.  Elements, reduction on load, canonical outputs
 * and strides are those of the two blocks above.
 *   ozk_fr_rows_combine_groups_dev
 *                              d_out[g][j] = sum_{i : group(i) = g} w_i rows[i][j] for g < groups, j < len: row i at
 *                              d_rows + 32 i row_stride, output row g at d_out + 32 g out_stride (both strides >= len;
 *                              elements of an output row beyond len are not touched), w = the k elements at d_weights.
 *                              group_of_row_host: k int32 values in [0, groups) in HOST memory, read before the call
 *                              returns; the groups may interleave in any way, and a group with no row yields a zero
 *                              row.  1 <= k <= 256, 1 <= groups <= 32, k len <= 2^28.  d_out must not overlap d_rows
 *                              (rejected).  Every input element is read once and every output element written once,
 *                              whatever the grouping.  With groups = 1 the bytes are those of ozk_fr_rows_combine_dev.
 *                              No workspace.
 *   ozk_fr_poly_eval_set_dev   d_values[y t + i] = p_y(z_yi), 1 <= t <= 32: the values of ozk_fr_poly_open_set_dev
 *                              without a quotient, from one read of every row.  The points are npolys x t elements in
 *                              HOST memory, laid out and read as there, but the points of a row need NOT be distinct:
 *                              a repeated point gives a repeated value.  poly_stride is 0 (ONE polynomial at npolys
 *                              sets) or >= len; npolys len and npolys t <= 2^28; d_values must not overlap d_coeffs
 *                              (rejected).  For pairwise distinct points the bytes are the values of
 *                              ozk_fr_poly_open_set_dev.
 *                              Workspace: ozk_fr_poly_eval_set_workspace_bytes(npolys, len, t).
 * Size functions and rejections as above: 0 and OZK_E_INVALID before any launch, the shape (k, groups and t included)
 * before the pointers, then the group ids.  Asynchronous on `stream`; nothing is allocated or synchronised. */
int ozk_fr_rows_combine_groups_dev(const void* d_rows, int32_t k, int32_t len, int64_t row_stride, const void* d_weights,
                                   const int32_t* group_of_row_host, int32_t groups, void* d_out, int64_t out_stride,
                                   void* stream);
size_t ozk_fr_poly_eval_set_workspace_bytes(int32_t npolys, int32_t len, int32_t t);
int ozk_fr_poly_eval_set_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride, int32_t t,
                             const uint8_t* points_host, void* d_values, void* d_workspace, size_t workspace_bytes,
                             void* stream);

/* The Fr kernels of the PLONK prover (csrc/plonk.cuh).  Elements, reduction on load, canonical
 * outputs and strides are those of the KZG blocks above; every scalar argument is 32-byte little-endian in HOST memory,
 * taken mod r and read before the call returns.
 *   ozk_fr_rows_coset_dev      d_out[y][i] = c s^i rows[y][i] for i < len and 0 for len <= i < out_len: row y at
 *                              d_rows + 32 y row_stride (>= len), output row y at d_out + 32 y out_stride (>= out_len;
 *                              elements of an output row beyond out_len are not touched).  One call is the way into a
 *                              coset (s = g, zero-extended to the size of the transform that follows), the way out of
 *                              one (s = 1 / g, c = 1 / size) and the 1 / n of an inverse transform (s = 1).
 *                              1 <= k, 1 <= len <= out_len, k out_len <= 2^28.  d_out may be d_rows itself when
 *                              out_len = len and the strides agree; any other overlap is rejected.  No table of len
 *                              powers is written: the workspace holds 256 + ceil(out_len / 1024) elements.
 *                              Workspace: ozk_fr_rows_coset_workspace_bytes(k, len, out_len).
 *   ozk_fr_perm_product_dev    The permutation grand product.  d_wires and d_sigma each hold three rows of len elements
 *                              at `stride` (>= len); the identity label of cell (j, i) is k_j omega^i, k_host96 the
 *                              three k_j.  d_z[0] = 1 and
 *                                d_z[i] = prod_{m < i} prod_j (w_jm + beta k_j omega^m + gamma) / (w_jm + beta s_jm + gamma),
 *                              *d_total (one element) the product over all len rows, *d_zero_dens (int32) the number of
 *                              rows whose denominator is zero: such a row's factor is taken as 1, and the other rows
 *                              are exact.  1 <= len <= 2^28, a power of two or not.  d_z, d_total and d_zero_dens must
 *                              not overlap d_wires, d_sigma or one another (rejected).  Every wire and sigma element
 *                              is read twice (once when len <= 1024) and d_z is written once.
 *                              Workspace: ozk_fr_perm_product_workspace_bytes(len).
 *   ozk_plonk_quotient_dev     d_out[i] = t(g omega_4n^i), i < 4 n, for
 *                                t = (qL a + qR b + qO c + qM a b + qC + PI + alpha P1 + alpha^2 (Z - 1) L_1) / Z_H,
 *                                P1 = Z (a + beta X + gamma)(b + beta k_1 X + gamma)(c + beta k_2 X + gamma)
 *                                     - Z(omega X)(a + beta s1 + gamma)(b + beta s2 + gamma)(c + beta s3 + gamma).
 *                              d_wit: the five rows a, b, c, Z, PI of 4 n values on the coset, at wit_stride; d_key: the
 *                              ten rows qL, qR, qO, qM, qC, s1, s2, s3, L_1 and the coset points themselves, at
 *                              key_stride (both >= 4 n).  k_host96: (k_0, k_1, k_2), of which k_1 and k_2 are used;
 *                              zh_inv_host128: the four values 1 / (g^n i4^m - 1), m < 4, i4 = omega_4n^n, which are
 *                              all that 1 / Z_H takes on the coset (point i has m = i mod 4); Z(omega X) is Z at
 *                              index (i + 4) mod 4 n.  n a power of two, 2 <= n, 4 n <= 2^28.  d_out must not overlap
 *                              d_wit or d_key (rejected).  Every input is read once (Z twice), d_out written once.
 *                              No workspace.
 * Size functions and rejections as above: 0 and OZK_E_INVALID before any launch, the shape before the pointers.
 * Asynchronous on `stream`; nothing is allocated or synchronised. */
size_t ozk_fr_rows_coset_workspace_bytes(int32_t k, int32_t len, int32_t out_len);
int ozk_fr_rows_coset_dev(const void* d_rows, int32_t k, int32_t len, int64_t row_stride, const uint8_t* s_host32,
                          const uint8_t* c_host32, void* d_out, int32_t out_len, int64_t out_stride, void* d_workspace,
                          size_t workspace_bytes, void* stream);
size_t ozk_fr_perm_product_workspace_bytes(int32_t len);
int ozk_fr_perm_product_dev(const void* d_wires, const void* d_sigma, int32_t len, int64_t stride, const uint8_t* omega_host32,
                            const uint8_t* k_host96, const uint8_t* beta_host32, const uint8_t* gamma_host32, void* d_z,
                            void* d_total, int32_t* d_zero_dens, void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_plonk_quotient_dev(const void* d_wit, int64_t wit_stride, const void* d_key, int64_t key_stride, int32_t n,
                           const uint8_t* alpha_host32, const uint8_t* beta_host32, const uint8_t* gamma_host32,
                           const uint8_t* k_host96, const uint8_t* zh_inv_host128, void* d_out, void* stream);

/* The lookup argument of the PLONK prover (csrc/plonk_lookup.cuh): logUp as a running sum over
 * one table of three-column tuples.  Conventions are those of the PLONK block above: plain 32-byte elements, reduced
 * on load, canonical outputs, strides in elements, scalars 32-byte little-endian in HOST memory.  A table is three
 * rows T1, T2, T3 at table_stride, of which the first n_rows elements count.
 *   ozk_plonk_lookup_index_dev  Built once per table.  d_index receives an open-addressing table of uint32 row
 *                              numbers (0xffffffff: empty) over the n_rows tuples; its capacity is the power of two
 *                              >= 2 n_rows, ozk_plonk_lookup_index_bytes(n_rows) bytes.  The key is the canonical
 *                              tuple; the slot of a tuple that several rows hold ends on the LOWEST of them, whatever
 *                              the order of arrival.  1 <= n_rows <= 2^28.  d_index must not overlap d_table.
 *   ozk_plonk_lookup_counts_dev Run once per proof.  d_wires: the rows a, b, c of len elements at `stride`; d_qk: one
 *                              row of len.  d_m (m_len >= n_rows elements) is zeroed, and every row i < len with
 *                              qK_i != 0 mod r adds 1 to the element d_m[row] of the first table row equal to
 *                              (a_i, b_i, c_i) mod r: later copies of a table row and the elements from n_rows to
 *                              m_len stay 0.  Counts stay below 2^28, so an element is its count in word 0.
 *                              *d_missing (int32) is the number of such rows whose tuple is in no table row and
 *                              *d_first_missing (int32) the lowest of them, 0x7fffffff when there is none.  Integer
 *                              atomics only: the result is bitwise reproducible.  1 <= len <= 2^28; the outputs
 *                              must not overlap the inputs or one another (rejected).
 *   ozk_plonk_lookup_sum_dev   d_s[0] = 0 and, with f = a + eta b + eta^2 c and t = T1 + eta T2 + eta^2 T3,
 *                                d_s[i + 1] = d_s[i] + m_i / (theta + t_i) - qK_i / (theta + f_i);
 *                              *d_total (one element) is the sum over all len rows and *d_zero_dens (int32) the
 *                              number of zero denominators among the 2 len: such a fraction counts as 0, the others
 *                              stay exact.  d_key4: the four rows qK, T1, T2, T3 of len elements at key_stride; d_m:
 *                              one row of len.  1 <= len <= 2^28, a power of two or not.  The outputs must not
 *                              overlap the inputs or one another, nor the workspace the inputs or the outputs
 *                              (rejected).  Every input element is read twice
 *                              (once when len <= 1024), d_s written once.
 *                              Workspace: ozk_plonk_lookup_sum_workspace_bytes(len).
 *   ozk_plonk_quotient_lookup_dev  ozk_plonk_quotient_dev with two more terms in the numerator,
 *                                alpha^3 ((S(omega X) - S)(theta + t)(theta + f) - m (theta + f) + qK (theta + t))
 *                                + alpha^4 S L_1.
 *                              d_wit: the seven rows a, b, c, Z, PI, m, S on the coset; d_key: the fourteen rows
 *                              qL, qR, qO, qM, qC, s1, s2, s3, L_1, X, qK, T1, T2, T3.  S(omega X) is S at index
 *                              (i + 4) mod 4 n.  The vanilla terms are the very code of ozk_plonk_quotient_dev: with
 *                              qK = m = S = 0 the outputs agree byte for byte.  No workspace.
 * Size functions and rejections as above: 0 and OZK_E_INVALID before any launch, the shape before the pointers.
 * Asynchronous on `stream`; nothing is allocated or synchronised. */
size_t ozk_plonk_lookup_index_bytes(int32_t n_rows);
int ozk_plonk_lookup_index_dev(const void* d_table, int32_t n_rows, int64_t table_stride, void* d_index, size_t index_bytes,
                               void* stream);
int ozk_plonk_lookup_counts_dev(const void* d_wires, const void* d_qk, int32_t len, int64_t stride, const void* d_table,
                                int32_t n_rows, int64_t table_stride, const void* d_index, size_t index_bytes, void* d_m,
                                int32_t m_len, int32_t* d_missing, int32_t* d_first_missing, void* stream);
size_t ozk_plonk_lookup_sum_workspace_bytes(int32_t len);
int ozk_plonk_lookup_sum_dev(const void* d_wires, int64_t stride, const void* d_key4, int64_t key_stride, const void* d_m,
                             int32_t len, const uint8_t* eta_host32, const uint8_t* theta_host32, void* d_s, void* d_total,
                             int32_t* d_zero_dens, void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_plonk_quotient_lookup_dev(const void* d_wit, int64_t wit_stride, const void* d_key, int64_t key_stride, int32_t n,
                                  const uint8_t* alpha_host32, const uint8_t* beta_host32, const uint8_t* gamma_host32,
                                  const uint8_t* k_host96, const uint8_t* zh_inv_host128, const uint8_t* eta_host32,
                                  const uint8_t* theta_host32, void* d_out, void* stream);

/* The witness of the PLONK prover built on the device (csrc/plonk_r1cs.cuh).  Conventions are
 * those of the PLONK block above: plain 32-byte elements, reduced on load, canonical outputs, strides in elements.
 *   ozk_fr_term_sums_dev       d_out[t] = sum_{u <= t} coeff[u] vec[index[u]] for t < terms: the inclusive running sum
 *                              over the WHOLE stream, not segmented (the sum over terms t0 .. t is
 *                              d_out[t] - d_out[t0 - 1], which ozk_plonk_wires_dev takes).  d_index: `terms` uint32;
 *                              d_vec: n_vec elements; d_coeff: `terms` elements, or NULL when every coefficient is
 *                              one.  A coefficient is stored in the form the kernel multiplies by: the word at
 *                              d_coeff[u] is c_u 2^261 mod r (any 256-bit word is accepted and reduced on load, as
 *                              every element is), so that its product with a plain element is plain.  A term whose
 *                              index is >= n_vec is never read: it counts as zero and adds 1 to *d_bad (int32, zeroed
 *                              by the call); no index makes the call read outside d_vec.  1 <= terms <= 2^28,
 *                              1 <= n_vec < 2^32.  d_index, d_coeff, d_vec and d_out are 16-byte aligned.  The
 *                              outputs must not overlap the inputs or one another, nor the workspace any of them
 *                              (rejected).  No atomics on field data: bitwise reproducible.  Every input is read
 *                              twice (once when terms <= 1024): 4 + 32 bytes a term and pass, + 32 with coefficients;
 *                              d_out is written once.  Workspace: ozk_fr_term_sums_workspace_bytes(terms).
 *   ozk_plonk_wires_dev        d_cells: k rows of len descriptors (hi, lo), two uint32 each, row y at
 *                              d_cells + 8 y cell_stride.  d_out[y][i] = src[hi] - src[lo] mod r, or src[hi] alone when
 *                              lo = 0xFFFFFFFF; output row y at d_out + 32 y out_stride (elements of a row beyond len
 *                              are not touched).  A descriptor whose hi or lo (other than 0xFFFFFFFF) is >= n_src is
 *                              not followed: its element is written as zero and adds 1 to *d_bad (int32, zeroed by
 *                              the call).  1 <= k, 1 <= len, k len <= 2^28, 1 <= n_src < 2^32, both strides >= len.
 *                              d_cells is 8-byte aligned.  d_out must not overlap d_src or d_cells, nor d_bad any of
 *                              them (rejected).  With every descriptor (v, 0xFFFFFFFF) this is the gather of a
 *                              circuit's wire columns from one value per variable.  No workspace.
 * Size functions and rejections as above: 0 and OZK_E_INVALID before any launch, the shape before the pointers.
 * Asynchronous on `stream`; nothing is allocated or synchronised. */
size_t ozk_fr_term_sums_workspace_bytes(int32_t terms);
int ozk_fr_term_sums_dev(const void* d_index, const void* d_coeff, const void* d_vec, int64_t n_vec, int32_t terms,
                         void* d_out, int32_t* d_bad, void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_plonk_wires_dev(const void* d_src, int64_t n_src, const void* d_cells, int32_t k, int32_t len, int64_t cell_stride,
                        void* d_out, int64_t out_stride, int32_t* d_bad, void* stream);

/* What makes a PLONK proof zero-knowledge (csrc/plonk_zk.cuh).  Conventions are those of the
 * PLONK block above: plain 32-byte elements, reduced on load, canonical outputs, strides in elements, scalars 32-byte
 * little-endian in HOST memory, taken mod r and read before the call returns.
 *   ozk_fr_rows_blind_dev      In place on k coefficient rows, row y at d_rows + 32 y stride.  Row y takes
 *                              counts_host[y] blinders r_0, r_1, .. (int32 in host memory, 0 .. 4 each) from
 *                              blinders_host, where the blinders of all rows lie back to back in row order:
 *                                row[j] = row[j] - r_j mod r and row[n + j] = r_j, j < counts_host[y],
 *                              which adds (r_0 + r_1 X + ..)(X^n - 1) to the row's polynomial.  What row[n + j] held is
 *                              not read; no other element is touched.  1 <= k <= 8, 4 <= n, stride >= n + 4,
 *                              k stride <= 2^28.  One launch, no workspace.
 *   ozk_plonk_quotient_split_dev  d_t: the 4 n coefficients of the quotient.  d_out receives three rows at out_stride
 *                              (>= n + 8), each written up to the stride; with blinders_host128 = (u_0, u_1, v_0, v_1):
 *                                t_lo'  = t[0 : n]        + (u_0 + u_1 X) X^n,
 *                                t_mid' = t[n : 2 n]      - (u_0 + u_1 X) + (v_0 + v_1 X) X^n,
 *                                t_hi'  = t[2 n : 3 n + 6] - (v_0 + v_1 X),
 *                              zero beyond, so that t_lo' + X^n t_mid' + X^2n t_hi' = t[0 : 3 n + 6].  *d_nonzero (int32,
 *                              zeroed by the call) is the number of coefficients t[i], 3 n + 6 <= i < 4 n, that are not
 *                              zero mod r: they are in no output row.  n a power of two, 8 <= n <= 2^26,
 *                              3 out_stride <= 2^28.  d_out must not overlap d_t, nor d_nonzero either (rejected).
 *                              Every coefficient is read once, every output element written once.  No workspace.
 * Rejections as above: OZK_E_INVALID before any launch, the shape before the pointers.  Asynchronous on `stream`;
 * nothing is allocated or synchronised. */
int ozk_fr_rows_blind_dev(void* d_rows, int32_t k, int32_t n, int64_t stride, const uint8_t* blinders_host,
                          const int32_t* counts_host, void* stream);
int ozk_plonk_quotient_split_dev(const void* d_t, int32_t n, void* d_out, int64_t out_stride, const uint8_t* blinders_host128,
                                 int32_t* d_nonzero, void* stream);

/* The field side of the batched PLONK verifier (csrc/plonk_verify.cuh): for K proofs under one
 * verifying key, what plonk.verify computes in host integers, one proof per lane.  Conventions are those of the PLONK
 * block above: plain 32-byte elements, canonical outputs.  kind: 0 a vanilla proof (800 bytes, key of 264), 1 a proof
 * with lookups (1088 bytes, key of 392).  d_proofs holds the K proofs back to back, d_public their public inputs,
 * K x n_public x 32 bytes (not read, and may be null, when n_public = 0); n is the key's.
 *   ozk_plonk_verify_challenges_dev  d_out receives one record of 8 (kind 1: 12) scalars per proof:
 *                                kind 0: beta, gamma, alpha, z, the multi-opening's gamma and point, rho_m, 0;
 *                                kind 1: beta, gamma, eta, theta, alpha, z, those two, rho_m, 0, 0, 0,
 *                              the challenges of plonk.challenges / lookup_challenges and kzg.multi_challenges over the
 *                              MultiOpening verify builds, from SHA-256 on the device (csrc/sha256.cuh); rho_m is
 *                              half m % 2 of SHA-256("OZK-plonk-rho" | seed_host32 | m / 2 as 8 bytes LE), 1 if zero:
 *                              transcript.weights.  d_vk_bytes: the key's bytes on the device.  One launch.
 *   ozk_plonk_verify_scalars_dev  d_flags[m] (int32): bit 0 an opened value is >= r, bit 1 a public input is >= r,
 *                              bit 2 z^n = 1, bit 3 the identity on the opened values fails (evaluated when the
 *                              other three are clear).  d_scalars: K x NC scalars of the proofs' commitments in the
 *                              row order of verify's MultiOpening (NC = 7: a b c t_lo t_mid t_hi Z; kind 1, NC = 9:
 *                              a b c m t_lo t_mid t_hi Z S), each the weight of kzg._multi_terms times rho_m; then K
 *                              of W, K of W'; then the NKEY = 8 (12) sums over the batch for the key's commitments
 *                              and the one for g1.  d_rho: the K weights rho_m.  A flagged proof has zero scalars, a
 *                              zero weight, adds nothing to the sums, and nothing is inverted for it.  Sums are
 *                              fixed-shape trees: the output is bitwise reproducible.  Three launches.
 * 1 <= K <= 2^16, K (n_public + 1) <= 2^24, n a power of two in [2, 2^26], 0 <= n_public <= n; every buffer 16-byte
 * aligned (d_flags 4); outputs and workspace may overlap neither inputs nor each other (rejected).  Rejections as
 * above: OZK_E_INVALID before any launch, the shape before the pointers; the size function returns 0 for a bad shape.
 * Asynchronous on `stream`; nothing is allocated or synchronised. */
int ozk_plonk_verify_challenges_dev(int32_t kind, const void* d_vk_bytes, int32_t n, int32_t n_public, const void* d_proofs,
                                    const void* d_public, int32_t K, const uint8_t* seed_host32, void* d_out, void* stream);
size_t ozk_plonk_verify_scalars_workspace_bytes(int32_t kind, int32_t K);
int ozk_plonk_verify_scalars_dev(int32_t kind, int32_t n, int32_t n_public, const void* d_proofs, const void* d_public,
                                 const void* d_challenges, int32_t K, void* d_scalars, void* d_rho, int32_t* d_flags,
                                 void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- batched MSM over shared bases (msm_multi.hip; no counterpart in the reference, whose verifier runs one
 * variable-base MSM per proof): out_i = sum_{j < n} s_ij P_j for k scalar rows over the SAME n bases, G1 only.
 * A window table of every base is built once (ozk_multi_msm_prepare_dev); a run is table gathers and mixed
 * additions, no sort, buckets or doublings.  Results are byte-identical to k calls of ozk_var_msm_dev.
 *   d_bases    n x 96 B wire-in G1 points (X | Y | Z, 32-byte little-endian, as ozk_var_msm_dev; Z = 0 is
 *              infinity, Z != 1 is accepted)
 *   d_table    ozk_multi_msm_table_bytes(n, type) bytes, 64-byte affine records; read-only after the build, may
 *              serve any number of runs and streams ordered after it
 *   d_scalars  k rows of n x 32 B little-endian, row-major, 16-byte aligned.  The contract is canonical scalars
 *              in [0, r); a value >= r is REDUCED mod r first (glv_decompose), which is the group element
 *              ozk_var_msm_dev computes for it too, so both return the same bytes
 *   d_out      k x 192 B wire-out records (64-byte little-endian coordinates, Z = 1; infinity (0, 1, 0))
 *   workspace  ozk_multi_msm_workspace_bytes(n, k, type) covers the build and a run of k rows
 *   plan       window size (signed digits, 2^(bits-1) entries per window) and windows per 128-bit GLV half
 * Limits: 1 <= n <= 4096, k >= 1, k * n <= 2^28, type == OZK_G1.  Outside them (G2 included) the size functions
 * return 0 and the entry points OZK_E_INVALID, as they do for a short table or workspace, and nothing is
 * launched.  Everything is enqueued on `stream`; nothing is allocated or synchronised. */
size_t ozk_multi_msm_table_bytes(int32_t n, int32_t type);
int ozk_multi_msm_prepare_dev(const void* d_bases, int32_t n, int32_t type, void* d_table, size_t table_bytes,
                              void* d_workspace, size_t workspace_bytes, void* stream);
size_t ozk_multi_msm_workspace_bytes(int32_t n, int32_t k, int32_t type);
int ozk_multi_msm_dev(const void* d_table, const void* d_scalars, int32_t n, int32_t k, int32_t type, void* d_out,
                      void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_multi_msm_plan(int32_t n, int32_t* window_bits, int32_t* windows);

/* ---- compressed points and compressed Groth16 proofs (point_codec.hip).
 * A compressed point is its affine x, little-endian, plus two flags in the two top bits of the last byte, which are
 * free because x < q < 2^254: bit 7 Y_LARGER (the canonical y satisfies y > q - y), bit 6 INFINITY (every other bit
 * of the encoding is then zero).  G1: 32 bytes.  G2: 64 bytes, x.c0 | x.c1, the flags in byte 63, Y_LARGER decided
 * on y.c1 unless y.c1 = 0, then on y.c0.  A proof: 128 bytes, A (32) | B (64) | C (32).
 * Decoding is strict; the code of a point is 0 ok, 1 a coordinate >= q, 2 bad infinity encoding (a stray bit next
 * to INFINITY, or Y_LARGER on a point with y = 0), 3 no curve point has this x.  There is NO subgroup check: a G2
 * point that decodes lies on the twist, not necessarily in the order-r subgroup (ozk_groth16_wellformed_dev checks
 * that).
 *   ozk_points_decompress_dev   n encodings of `type` (OZK_G1 / OZK_G2) -> n points X | Y | Z with Z = 1 in
 *                               out_format 0 (wire-in, 32-byte coordinates) or 1 (wire-out, 64-byte coordinates) and
 *                               n codes.  Infinity, and every point whose code is not 0, is written as O:
 *                               (0, 1, 0) for G1, ((0, 0), (1, 0), (0, 0)) for G2.
 *   ozk_points_compress_dev     n points in in_format 0 / 1, any Z (coordinates are taken mod q; of a wire-out
 *                               coordinate only the low 32 bytes are read) -> n encodings.  Z = 0 gives INFINITY.
 *   ozk_groth16_proofs_decompress_dev
 *                               k compressed proofs -> k 768-byte records A | B | C (wire-out), the input of
 *                               ozk_groth16_verify_dev and ozk_groth16_verify_rlc_dev.  d_codes[i] = 0 when the
 *                               three points decoded, else the first non-zero code in the order A, B, C.
 *   ozk_points_decompress_prepared_dev
 *                               n encodings -> the prepared bases of the variable-base MSM over those n points
 *                               (DESIGN.md section 14), byte for byte what ozk_var_msm_prepare_dev writes from the
 *                               wire-in output of ozk_points_decompress_dev, and the same n codes, without the
 *                               wire-in points ever existing: record i = (x, y), record n + i = (beta x, y), canonical
 *                               Montgomery; infinity, and every point whose code is not 0, is the (0, 0) marker in
 *                               both.  prepared_bytes >= ozk_var_msm_prepared_bytes(n, type), else OZK_E_INVALID;
 *                               n > 2^23 (where the MSM leaves the two-record GLV form) is OZK_E_INVALID too.
 *                               check_subgroup != 0 (G2 only; G1 has cofactor 1 and ignores it): a decoded point P
 *                               with [r]P != O gets code 4 and the (0, 0) marker.
 * n or k <= 0, a null pointer, an unknown type or format, a buffer that is not 4-byte aligned: OZK_E_INVALID.
 * Asynchronous on `stream`. */
int ozk_points_decompress_prepared_dev(const void* d_in, int32_t n, int32_t type, void* d_prepared,
                                       size_t prepared_bytes, int32_t* d_codes, int32_t check_subgroup, void* stream);
int ozk_points_decompress_dev(const void* d_in, int32_t n, int32_t type, int32_t out_format, void* d_out,
                              int32_t* d_codes, void* stream);
int ozk_points_compress_dev(const void* d_in, int32_t n, int32_t type, int32_t in_format, void* d_out, void* stream);
int ozk_groth16_proofs_decompress_dev(const void* d_in128, int32_t k, void* d_records768, int32_t* d_codes,
                                      void* stream);

/* ---- n points times one scalar (points_scale.hip; no counterpart in the reference): out_i =
 * [k] P_i, the operation of a phase-2 key contribution (delta_abc_g1 and query_h times 1 / d) and, with k = r - 1 on
 * one point, of the subgroup test of its new delta_g2.
 *   d_in      n wire-in points of `type` (OZK_G1 96 B, OZK_G2 192 B: X | Y | Z, 32-byte little-endian; any Z, Z = 0
 *             is infinity), read as ozk_var_msm_dev reads its bases
 *   k_host32  the scalar, 32 bytes little-endian in HOST memory (as the t of ozk_fr_powers_dev), read before the call
 *             returns.  It must be below r: a value >= r is OZK_E_INVALID and nothing is enqueued.  k = 0 is legal
 *             and gives n points at infinity.
 *   d_out     n wire-in points, affine-normalised (Z = 1, canonical, non-Montgomery); infinity as
 *             ozk_points_decompress_dev writes it: (0, 1, 0) for G1, ((0, 0), (1, 0), (0, 0)) for G2.  d_out == d_in
 *             is allowed (a lane reads its point before it writes); any other overlap is not.
 * The scalar is recoded once on the host and the digit schedule passed in the kernel arguments, one point per lane:
 * G1 runs a GLV split in joint sparse form (about 128 doublings and 64 mixed additions per point), G2 the
 * non-adjacent form of k without the endomorphism, so that the result is exact for EVERY point of the twist, inside
 * the order-r subgroup or not.  Every addition is complete.
 * n <= 0 or n > 2^24, a null pointer, an unknown type, a buffer that is not 4-byte aligned: OZK_E_INVALID.
 * Asynchronous on `stream`; allocates nothing and needs no workspace. */
int ozk_points_scale_dev(const void* d_in, int32_t n, int32_t type, const uint8_t* k_host32, void* d_out,
                         void* stream);

/* ---- n points times n scalars (points_mul.hip; no counterpart in the reference): out_i =
 * [k_i] P_i, the operation of a phase-1 contribution to a powers-of-tau string (tau_g1[i] times s^i and so on).
 *   d_in       n wire-in points of `type`, read exactly as ozk_points_scale_dev reads them
 *   d_scalars  n x 32 bytes little-endian in DEVICE memory: what ozk_fr_powers_dev writes
 *   d_out      n wire-in points exactly as ozk_points_scale_dev writes them (Z = 1, canonical; its infinity).
 *              d_out == d_in is allowed (a lane reads its point and its scalar before it writes); any other overlap
 *              is not.
 *   d_codes    NULL, or n x int32: 0 for a point that was multiplied, 1 where k_i >= r; that point is written as
 *              infinity and its neighbours are not affected.  k_i = 0 and P_i at infinity give infinity with code 0.
 * One point per lane, 64-lane workgroups.  The lane recodes its own scalar in the kernel (G1: the GLV halves in joint
 * sparse form; G2: the non-adjacent form of k without the endomorphism, exact on the whole twist) into 32 words of
 * LDS at a stride of 33 words per lane (8448 bytes per workgroup), and runs the ladder of ozk_points_scale_dev over
 * them.  Every addition is complete: the result is [k_i] P_i for every point of the curve and every k_i in [0, r).
 * n <= 0 or n > 2^24, a null d_in, d_scalars or d_out, an unknown type, a buffer that is not 4-byte aligned:
 * OZK_E_INVALID with nothing enqueued.  Asynchronous on `stream`; allocates nothing and needs no workspace. */
int ozk_points_mul_dev(const void* d_in, const void* d_scalars, int32_t n, int32_t type, void* d_out,
                       int32_t* d_codes, void* stream);

/* ---- point kernels of the setup from a powers-of-tau string (ec_fft.hip; no counterpart in
 * the reference).  All three read wire-in points of `type` (OZK_G1 96 B, OZK_G2 192 B; any Z, Z = 0 is infinity) as
 * ozk_points_scale_dev reads them and write affine-normalised wire-in points (Z = 1, canonical), infinity as
 * ozk_points_decompress_dev writes it.  Every addition is complete, so the result is exact for every input: infinity,
 * repeated points, P with -P.  Asynchronous on `stream`; they allocate nothing; a bad argument (a null pointer, an
 * unknown type, a count out of range, a buffer that is not 4-byte aligned, a workspace that is too small) is
 * OZK_E_INVALID with nothing enqueued.
 *
 *   ozk_ec_fft_dev   the radix-2 transform in the exponent: out[j] = sum_i [omega^(i j)] in[i], in natural order, for
 *                    n a power of two in [1, 2^22].  inverse != 0 uses omega^-1 and multiplies by 1 / n (what
 *                    SerialFFT.radix2InverseFFT does to scalars).  omega_host32: 32 bytes little-endian in HOST
 *                    memory, read before the call returns; it must be below r with omega^n = 1 and omega^(n/2) != 1,
 *                    else OZK_E_INVALID.  d_out must NOT overlap d_in (the first step is a bit-reversing copy).
 *                    d_workspace: ozk_ec_fft_workspace_bytes(n, type) bytes (0 for a bad n or type): the digit
 *                    schedules of the 3 n / 4 twiddles, 132 bytes each, recoded on the device at every call.
 *                    G1 runs the GLV ladder of ozk_points_scale_dev per butterfly, G2 the non-adjacent form without
 *                    the endomorphism: both are exact on the whole curve / twist, no subgroup assumption.
 *   ozk_sparse_mat_points_dev
 *                    out[row] = sum over the row's terms of [coeff] points[index]: the CSR layout, the
 *                    NULL-coefficients-mean-one rule and the long-row list (rows of more than 64 terms) of
 *                    ozk_sparse_mat_vec_dev.  An empty row gives infinity.  Coefficients 1 and r - 1 (and NULL) cost
 *                    one mixed addition, 0 nothing, any other value a per-lane double-and-add over its 254 bits.
 *                    A long row is cut into 4096 strided partial sums, then 64, then one.  d_workspace:
 *                    ozk_sparse_mat_points_workspace_bytes(n_long, type) bytes, unused (may be NULL) for n_long = 0.
 *                    rows in [1, 2^24], n_long in [0, 2^16].  d_out must not overlap an input.
 *   ozk_points_add_dev
 *                    out[i] = a[i] + b[i], or a[i] - b[i] for negate_b != 0; n in [1, 2^24].  d_out may be d_a or d_b. */
size_t ozk_ec_fft_workspace_bytes(int32_t n, int32_t type);
int ozk_ec_fft_dev(const void* d_in, int32_t n, int32_t type, const uint8_t* omega_host32, int32_t inverse,
                   void* d_out, void* d_workspace, size_t workspace_bytes, void* stream);
size_t ozk_sparse_mat_points_workspace_bytes(int32_t n_long, int32_t type);
int ozk_sparse_mat_points_dev(const void* d_row_ptr, const void* d_index, const void* d_coeff, const void* d_points,
                              int32_t rows, int32_t type, const void* d_long_rows, int32_t n_long, void* d_out,
                              void* d_workspace, size_t workspace_bytes, void* stream);
int ozk_points_add_dev(const void* d_a, const void* d_b, int32_t n, int32_t type, int32_t negate_b, void* d_out,
                       void* stream);

/* ---- n sums of products of points and scalars (points_mac.hip; no counterpart in the
 * reference): out[i] = sum over v < terms of [k_v[i]] P_v[i], G1.  The middle step of KZG openings at every coset at
 * once (octopuszk_amd/kzg.py OpenAllKey): the points are fixed per key and prepared once, the scalars change per call.
 * A lane keeps one Jacobian accumulator for its output: one doubling chain of at most 128 steps and one inversion
 * whatever `terms` is, against `terms` of each for ozk_points_mul_dev calls joined by ozk_points_add_dev.
 *   ozk_points_mac_prepared_bytes / ozk_points_mac_workspace_bytes
 *               192 terms n / 68 terms n bytes; 0 for a shape or type the calls refuse.
 *   ozk_points_mac_prepare_dev
 *     d_in        terms x n wire-in G1 points, term-major (term v's n points contiguous), any Z, Z = 0 is infinity,
 *                 read exactly as ozk_points_scale_dev reads them
 *     d_prepared  prepared_bytes >= ozk_points_mac_prepared_bytes(terms, n, type): per point x, beta x, beta^2 x, y
 *                 and the two coordinates of P - phi(P), canonical Montgomery words, element-major so that
 *                 neighbouring lanes read neighbouring elements; infinity is six zero elements.  Valid for calls with
 *                 the same terms and n.
 *   ozk_points_mac_dev
 *     d_scalars   terms x n x 32 bytes little-endian in DEVICE memory, term-major, as ozk_points_mul_dev takes them
 *     d_out       n wire-in points exactly as ozk_points_mul_dev writes them (Z = 1, canonical; its infinity)
 *     d_codes     NULL, or n x int32: 0, or 1 for a lane one of whose scalars was >= r; that lane is written as
 *                 infinity and its neighbours are not affected
 *     d_workspace workspace_bytes >= ozk_points_mac_workspace_bytes(terms, n, type): the digit schedules (the GLV
 *                 halves in joint sparse form, 16 words and a length per scalar), which a first kernel writes and the
 *                 accumulating kernel streams; no buffer may overlap another.
 * Every addition is complete: equal points among the terms, P with -P, infinity as any or every term, k = 0 and
 * k = r - 1 are exact.  1 <= terms <= 32, 1 <= n <= 2^24, type OZK_G1 only (OZK_G2 is OZK_E_INVALID).  A null pointer,
 * a buffer that is not 4-byte aligned, a shape out of range, a buffer that is too small: OZK_E_INVALID with nothing
 * enqueued.  Asynchronous on `stream`; they allocate nothing. */
size_t ozk_points_mac_prepared_bytes(int32_t terms, int32_t n, int32_t type);
int ozk_points_mac_prepare_dev(const void* d_in, int32_t terms, int32_t n, int32_t type, void* d_prepared,
                               size_t prepared_bytes, void* stream);
size_t ozk_points_mac_workspace_bytes(int32_t terms, int32_t n, int32_t type);
int ozk_points_mac_dev(const void* d_prepared, const void* d_scalars, int32_t terms, int32_t n, int32_t type,
                       void* d_out, int32_t* d_codes, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OZK_H */
