/* qkd_ldpc_hip.h — C ABI of libqkdldpc_hip.so, the MI355X (gfx950) LDPC
 * belief-propagation decoder for QKD error reconciliation.
 *
 * This is the drop-in boundary for the hot path of ColdCloudd/QKD_LDPC_V:
 * the six flooding decoders of src/qkd_ldpc_algorithm.cpp:3-1029 (declared at
 * src/qkd_ldpc_algorithm.hpp:28-90), batched over independent trials — the
 * pool.detach_loop seam at src/simulation.cpp:740-746 — plus the per-trial frame
 * construction of QKD_LDPC (src/qkd_ldpc_algorithm.cpp:1031-1087) and the H
 * loaders it reads (src/array_and_matrix_operations.cpp:291-886).
 *
 * Plain C: pointers and sizes only.  Every entry returns 0 on success and a
 * negative QLDPC_E* code on failure; qldpc_last_error() then describes it
 * (thread-local).  The C++ mirror in qkd_ldpc_v_amd/host/qkd_ldpc_algorithm.hpp
 * turns failures into std::runtime_error, as the reference's loaders do.
 */
#ifndef QKD_LDPC_HIP_H
#define QKD_LDPC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLDPC_OK 0
#define QLDPC_EINVAL (-1)   /* bad argument / malformed graph */
#define QLDPC_EHIP (-2)     /* HIP runtime failure */
#define QLDPC_EIO (-3)      /* matrix file cannot be opened / parsed */
#define QLDPC_ENOMEM (-4)
#define QLDPC_EUNSUP (-5)   /* graph shape the GPU path does not accept */

/* Decoder ids: reference src/config.hpp:201 (DEC_SPA=0 ... DEC_AOMSA=5). */
#define QLDPC_SPA 0
#define QLDPC_SPA_LIN 1
#define QLDPC_NMSA 2
#define QLDPC_OMSA 3
#define QLDPC_ANMSA 4
#define QLDPC_AOMSA 5

/* Matrix file formats: reference src/config.hpp:202 (MAT_*). */
#define QLDPC_MAT_UNCOMPRESSED 0
#define QLDPC_MAT_ALIST 1
#define QLDPC_MAT_SPARSE_1 2
#define QLDPC_MAT_SPARSE_2 3

typedef struct qldpc_graph qldpc_graph;

/* Decoder parameters.  Replaces the per-call arguments of the six decoders
 * (src/qkd_ldpc_algorithm.hpp:28-90) plus the global-CFG inputs they read:
 * CFG.DECODING_ALGORITHM (dispatch at src/qkd_ldpc_algorithm.cpp:1056-1085),
 * CFG.DECODING_ALG_MAX_ITERATIONS, CFG.ENABLE_DECODING_ALG_MSG_LLR_THRESHOLD and
 * CFG.DECODING_ALG_MSG_LLR_THRESHOLD; primary/secondary are
 * decoding_scaling_factors (src/config.hpp:50-54). */
typedef struct {
    int32_t algorithm;      /* QLDPC_SPA .. QLDPC_AOMSA */
    int32_t max_iterations; /* >= 1 */
    int32_t thr_enabled;    /* message LLR clipping on/off */
    int32_t reserved;
    double thr;             /* clipping threshold (> 0 when enabled) */
    double primary;         /* alpha (NMSA, ANMSA) or beta (OMSA, AOMSA) */
    double secondary;       /* nu (ANMSA) or sigma (AOMSA) */
} qldpc_params;

/* ---------------------------------------------------------------- loaders */

/* Parse a parity-check matrix file into the reference's H_matrix adjacency
 * (check_nodes -> row_ptr/col_idx, bit_nodes -> col_ptr/row_idx).  Restates
 * read_sparse_uncompressed_matrix / read_sparse_matrix_alist /
 * read_sparse_matrix_1 / read_sparse_matrix_2
 * (src/array_and_matrix_operations.cpp:764-886, 291-468, 478-617, 626-761),
 * including their validation errors.  Files ending in ".gz" are inflated first.
 * Call with NULL arrays to query n, m and nnz; then again with buffers of
 * m+1, nnz, n+1 and nnz entries.  *is_regular mirrors H_matrix::is_regular. */
int qldpc_load_matrix(const char *path, int32_t format, int32_t *n, int32_t *m, int32_t *nnz,
                      int32_t *row_ptr, int32_t *col_idx, int32_t *col_ptr, int32_t *row_idx,
                      int32_t *is_regular);

/* ------------------------------------------------------------------ graph */

/* Build the device-resident Tanner graph from check_nodes in CSR form
 * (row_ptr[m+1], col_idx[nnz]), bit_nodes taken as their ascending transpose.
 * The graph is immutable, replicated on every device of device_mask (bit d =
 * HIP device d; 0 = current device only) and safe to share between host
 * threads.  Rows out of ascending order decode with the reference's occurrence
 * pairing (see qldpc_graph_create_checked); a bit listed twice in one row
 * returns QLDPC_EUNSUP. */
int qldpc_graph_create(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                       int32_t device_mask, qldpc_graph **out);

/* As qldpc_graph_create with the caller's bit_nodes (col_ptr[n+1],
 * row_idx[nnz], the reference's H_matrix::bit_nodes in its own order).  When
 * check_nodes rows are ascending and bit_nodes is their ascending transpose,
 * the reference's slot counters (src/qkd_ldpc_algorithm.cpp:67-69,116-118) pair
 * every message with its own edge; otherwise they pair an edge's b2c with
 * another edge's message, and the graph decodes with that occurrence pairing
 * (the v1 global-slot kernel and a pairing pass).  Lists that disagree on an
 * edge count return QLDPC_EUNSUP. */
int qldpc_graph_create_checked(int32_t n, int32_t m, const int32_t *row_ptr,
                               const int32_t *col_idx, const int32_t *col_ptr,
                               const int32_t *row_idx, int32_t device_mask, qldpc_graph **out);

/* As qldpc_graph_create, on an explicit list of HIP devices, one shard per
 * entry: qldpc_decode_batch splits a batch in ndevices contiguous slices, one
 * host thread, stream and graph replica per entry.  A device may be listed
 * more than once (several concurrent shards on one GPU). */
int qldpc_graph_create_on(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                          const int32_t *devices, int32_t ndevices, qldpc_graph **out);

/* qldpc_graph_create_checked on an explicit device list (one shard per entry,
 * as qldpc_graph_create_on): the C++ drop-in's graphs (the node's GPUs, or
 * logical shards of one GPU for tests). */
int qldpc_graph_create_checked_on(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                                  const int32_t *col_ptr, const int32_t *row_idx, const int32_t *devices,
                                  int32_t ndevices, qldpc_graph **out);

/* Plan only, on the host (no device is touched): the returned graph has no
 * devices and cannot decode; it answers qldpc_graph_info and
 * qldpc_graph_labels.  For inspection and CPU tests of the planner. */
int qldpc_graph_create_host(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                            qldpc_graph **out);

/* Graph creation with options: every entry above through one door, plus the
 * choice of layout.
 *
 * layout QLDPC_LAYOUT_AUTO (or opts == NULL) is the planner's choice, the
 * same graph (plan, labels, tables) as qldpc_graph_create_checked_on builds;
 * col_ptr / row_idx NULL takes bit_nodes as the ascending transpose
 * (qldpc_graph_create_on), host_only != 0 plans without touching a device
 * (qldpc_graph_create_host; devices is ignored).  devices NULL: the current
 * device.
 *
 * QLDPC_LAYOUT_FRAME_PER_LANE ("fpl") decodes 64 frames per wave, lane =
 * frame: the batch is cut into tiles of 64 frames, and every iteration is a
 * short sequence of ordinary kernel launches on the caller's stream (a
 * check-node pass of one wave per row, a settle step, a bit pass).  No kernel
 * of it waits on another workgroup, so unlike the split plan of n = 100k
 * codes it cannot fail to meet: choose it under co-tenancy, CU masks,
 * several ranks on one device or a large max_iterations.  It takes any graph
 * the canonical adjacency allows and any batch size; bit_nodes that need the
 * reference's occurrence pairing return QLDPC_EUNSUP (those graphs stay on
 * the first-generation kernels).  Every decode entry works on it unchanged:
 *   - the launch count is a fixed function of max_iterations and the graph's
 *     row lengths: per iteration one check-node launch per class of row
 *     lengths present (at most 8; 1-3 for the shipped codes), a settle and a
 *     bit-pass launch, plus six launches per chunk; the device entries enqueue the whole sequence,
 *     frames that have exited are masked and finished tiles return at once;
 *   - device memory per tile of 64 frames is 512 nnz + 1024 n + 8 (n + m)
 *     bytes in the (device, stream) workspace; a batch whose tiles exceed a
 *     budget of 4 GiB runs as consecutive chunks of tiles on the same stream;
 *   - the fused entries use the internal LLR workspace when d_llr_ws is NULL;
 *   - qldpc_graph_plan answers variant "fpl", lanes 64, edges_per_lane 0,
 *     lds_bytes 0 and for workgroups the check-node pass's grid for one
 *     tile; qldpc_graph_split_plan parts 1, part_lanes 64, scratch_slots 0;
 *     qldpc_graph_labels the identity;
 *   - qldpc_set_kernel_timing brackets the whole launch sequence of a decode;
 *     qldpc_last_claim_order reports the order in which frames were dealt to
 *     tiles (64 consecutive entries share a tile; count 0: index order).
 * An unknown layout or a nonzero reserved word returns QLDPC_EINVAL. */
#define QLDPC_LAYOUT_AUTO 0
#define QLDPC_LAYOUT_FRAME_PER_LANE 1
typedef struct {
    int32_t layout;
    int32_t host_only;
    int32_t reserved[6];
} qldpc_graph_opts;
int qldpc_graph_create_opts(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                            const int32_t *col_ptr /* nullable */, const int32_t *row_idx /* nullable */,
                            const int32_t *devices /* nullable: current device */, int32_t ndevices,
                            const qldpc_graph_opts *opts /* NULL = all zero */, qldpc_graph **out);

void qldpc_graph_destroy(qldpc_graph *g);

/* n, m, nnz and the number of devices the graph lives on. */
int qldpc_graph_info(const qldpc_graph *g, int32_t *n, int32_t *m, int32_t *nnz,
                     int32_t *num_devices);

/* ----------------------------------------------------------------- decode */

/* Decode `batch` independent frames held in HOST memory; synchronous.
 * Replaces `batch` calls of the decoder selected by p->algorithm, each
 *   decoding_result f(llr, H, syndrome, max_it, [alpha|beta], [nu|sigma], thr, out)
 * (src/qkd_ldpc_algorithm.hpp:28-90).  llr: batch*n doubles (frame-major),
 * syndrome: batch*m bytes in {0,1}, bits_out: batch*n bytes (bit_array_out),
 * iters_out / synd_ok_out: decoding_result {iterations_num, syndromes_match}
 * per frame, posterior_out (nullable): batch*n doubles = the reference's
 * total_bit_llr at return.  Frames are split in contiguous slices over the
 * graph's devices, one host thread per device, no collectives. */
int qldpc_decode_batch(qldpc_graph *g, const qldpc_params *p, int32_t batch, const double *llr,
                       const uint8_t *syndrome, uint8_t *bits_out, uint32_t *iters_out,
                       uint8_t *synd_ok_out, double *posterior_out);

/* Same on DEVICE buffers of the graph's device `device`, enqueued on the HIP
 * stream `stream` (hipStream_t; NULL = default stream).  Asynchronous. */
int qldpc_decode_batch_device(qldpc_graph *g, int32_t device, const qldpc_params *p, int32_t batch,
                              const double *d_llr, const uint8_t *d_syndrome, uint8_t *d_bits_out,
                              uint32_t *d_iters_out, uint8_t *d_synd_ok_out,
                              double *d_posterior_out, void *stream);

/* The same decode with its per-iteration trace: the data the reference prints
 * under TRACE_DECODING_ALG / TRACE_DECODING_ALG_LLR (src/qkd_ldpc_algorithm.cpp:
 * 88-99), as arrays.  Frame-per-lane graphs only (QLDPC_LAYOUT_FRAME_PER_LANE):
 * any other graph returns QLDPC_EUNSUP; build a second graph with that layout.
 *
 * Row `it` of frame f exists when the bit pass of iteration `it` ran for f:
 *   - d_trace_post_out[f][it][0..n) (nullable; batch*max_iterations*n doubles)
 *     is total_bit_llr after that bit pass, in the reference's bit ids;
 *   - d_unsat_out[f][it] (nullable; batch*max_iterations words) is the number
 *     of checks whose parity over the decisions (total <= 0) after that bit
 *     pass differs from the frame's syndrome bit.  Empty checks count: a
 *     syndrome bit of 1 on an empty row is one unsatisfied check.
 * Rows that do not exist read QLDPC_TRACE_NONE and an all-ones NaN (0xFF
 * bytes): both arrays are filled on the stream before the first launch, and
 * no kernel writes a row of a frame that has left the decode.
 *   - SPA / SPA-LIN / NMSA / OMSA: iterations_num rows.
 *   - ANMSA / AOMSA leave after a check-node pass, before the bit pass:
 *     iterations_num - 1 rows when syndromes_match (none for a frame whose
 *     channel decision already matches), max_iterations rows otherwise.
 * A capped ANMSA / AOMSA frame can show 0 unsatisfied checks in its last row
 * and still report syndromes_match = 0: the reference never tests the last
 * decisions of those two (it leaves its loop at the cap).  No other promise
 * is made about zero counts.
 * bits / iterations / syndromes_match / posterior are qldpc_decode_batch[_device]'s;
 * with both trace pointers NULL the call is that decode, launch for launch.
 * Each traced iteration adds two short launches for the counts and one for the
 * totals' row.  Arguments are checked in this order: NULL graph, the
 * parameters, batch < 0, the layout, batch == 0 (OK), NULL buffers; through
 * batch == 0 no device is touched.
 * The host entry shards like qldpc_decode_batch and stages the trace arrays on
 * each shard's device for the call; QLDPC_ENOMEM when they do not fit (then
 * nothing of the call is in flight). */
#define QLDPC_TRACE_NONE 0xFFFFFFFFu
int qldpc_decode_trace_batch_device(qldpc_graph *g, int32_t device, const qldpc_params *p, int32_t batch,
                                    const double *d_llr, const uint8_t *d_syndrome, uint8_t *d_bits_out,
                                    uint32_t *d_iters_out, uint8_t *d_synd_ok_out,
                                    double *d_posterior_out /* nullable */,
                                    uint32_t *d_unsat_out /* nullable: [batch][max_iterations] */,
                                    double *d_trace_post_out /* nullable: [batch][max_iterations][n] */,
                                    void *stream);
int qldpc_decode_trace_batch(qldpc_graph *g, const qldpc_params *p, int32_t batch, const double *llr,
                             const uint8_t *syndrome, uint8_t *bits_out, uint32_t *iters_out,
                             uint8_t *synd_ok_out, double *posterior_out /* nullable */,
                             uint32_t *unsat_out /* nullable */, double *trace_post_out /* nullable */);

/* ------------------------------------------------ per-trial frame (QKD_LDPC) */

/* QKD_LDPC's frame construction on device (src/qkd_ldpc_algorithm.cpp:
 * 1043-1052): llr[i] = bob[i] ? -log_p : log_p, syndrome = H * alice
 * (calculate_syndrome, src/array_and_matrix_operations.cpp:936-950).
 * d_alice/d_bob: batch*n bytes in {0,1}.  d_log_p: batch doubles, each
 * log((1-q)/q) of the trial's accurate QBER q evaluated by the HOST C library
 * (qldpc_log_p below): glibc's log is not correctly rounded, so evaluating it
 * anywhere else could move an LLR by an ulp. */
int qldpc_build_frames_device(qldpc_graph *g, int32_t device, int32_t batch, const uint8_t *d_alice,
                              const uint8_t *d_bob, const double *d_log_p, double *d_llr,
                              uint8_t *d_syndrome, void *stream);

/* log((1. - q) / q) with the host C library, as src/qkd_ldpc_algorithm.cpp:1043. */
double qldpc_log_p(double qber);

/* keys_match = arrays_equal(alice, bob_solution) per frame
 * (src/qkd_ldpc_algorithm.cpp:1087; src/array_and_matrix_operations.cpp:105-118). */
int qldpc_keys_match_device(int32_t batch, int32_t n, const uint8_t *d_alice,
                            const uint8_t *d_bits, uint8_t *d_keys_match, void *stream);

/* The whole per-trial window of QKD_LDPC for `batch` trials on device: frame
 * construction + decode + key comparison.  d_synd_ws: caller-owned workspace
 * of batch*m bytes (Alice's syndromes).  d_llr_ws: batch*n doubles or NULL —
 * when given, the frames' LLRs are written there; NULL skips them where the
 * graph's decoder reads the frame builder's palette codes instead (the
 * register kernels), and uses an internal workspace otherwise. */
int qldpc_qkd_ldpc_batch_device(qldpc_graph *g, int32_t device, const qldpc_params *p,
                                int32_t batch, const uint8_t *d_alice, const uint8_t *d_bob,
                                const double *d_log_p, double *d_llr_ws, uint8_t *d_synd_ws,
                                uint8_t *d_bits_out, uint32_t *d_iters_out,
                                uint8_t *d_synd_ok_out, uint8_t *d_keys_match_out, void *stream);

/* --------------------------------------------------------------- introspection */

/* Launch geometry the decoder uses for this graph on `device`: lanes per frame
 * (threads per workgroup), edges per lane, resident workgroups, dynamic LDS
 * bytes and the kernel variant name (static string).  A host-only graph
 * (qldpc_graph_create_host) answers with workgroups == NULL. */
int qldpc_graph_plan(const qldpc_graph *g, int32_t device, int32_t algorithm, int32_t *lanes,
                     int32_t *edges_per_lane, int32_t *workgroups, int32_t *lds_bytes,
                     const char **variant);

/* Split-frame shape of the plan (n = 100k codes: a frame over several
 * workgroups of one XCD): parts per frame, lanes (threads) per part, and the
 * message slots per lane held in per-workgroup global scratch.  Frames of one
 * workgroup answer parts = 1 (part_lanes = the workgroup's lanes, scratch
 * slots of the hybrid shape included).  Any output pointer may be NULL. */
int qldpc_graph_split_plan(const qldpc_graph *g, int32_t *parts, int32_t *part_lanes, int32_t *scratch_slots);

/* The decoder's bank-aware label of every bit id (labels_out: n entries; the
 * identity when the plan keeps the reference's ids — split, hybrid and
 * first-generation shapes), and stats_out (nullable, 4 entries): summed LDS
 * bank excess of the slot layout before / after the relabelling search, and
 * the summed busiest-bank counts (LDS cycles of the slot groups) before / after.  Labels never change results: inputs and outputs
 * of every entry point use the reference's bit ids. */
int qldpc_graph_labels(const qldpc_graph *g, int32_t *labels_out, int64_t *stats_out);

/* Kernel timing: while enabled on g, every decode kernel launch is bracketed
 * by HIP events on the stream it runs on (nothing else: not the frame build,
 * the claim order or the key compare).  qldpc_last_decode_kernel_ms waits for
 * the last timed launch on (device, stream) and returns its duration in ms. */
int qldpc_set_kernel_timing(qldpc_graph *g, int32_t enabled);
int qldpc_last_decode_kernel_ms(qldpc_graph *g, int32_t device, void *stream, float *ms);

/* Diagnostic: the order in which the last decode on (device, stream) claimed
 * its frames (order.hip: ascending weight |H * z XOR s| of the channel
 * decision z) and each frame's weight, indexed by frame.  *count = the batch,
 * or 0 when that decode claimed frames in index order (QLDPC_ORDER=0, one
 * frame).  Waits for the stream.  No counterpart in the reference (its pool
 * decodes trials one at a time). */
int qldpc_last_claim_order(qldpc_graph *g, int32_t device, void *stream, int32_t *order_out, int32_t *weight_out,
                           int32_t cap, int32_t *count);

/* Diagnostic: evaluate the decoder's device math on `count` inputs on the
 * current device — fn 0 tanh, 1 atanh, 2 expm1, 3 log1p (exact_math.h, the
 * glibc-exact restatement), 4 tanh_lin_approx, 5 atanh_lin_approx
 * (src/qkd_ldpc_algorithm.cpp:146-172), 6 tanh and 7 atanh in the decoder
 * forms the SPA kernel calls, 8 tanh(x / 2.) in the table form of the SPA
 * check-node scan (tanh_half_clip_t; |x| >= 44 gives +-1), 9 clip(2. * atanh(x),
 * 100) in the SPA message pass's form (atanh2_clip). */
int qldpc_selftest_math_device(int32_t fn, int32_t count, const double *d_in, double *d_out, void *stream);

/* The same with the clip threshold of fn 8 and fn 9 given (thr > 0, +inf
 * allowed): fn 8 is tanh(clip(x, thr) / 2.) and fn 9 clip(2. * atanh(x), thr),
 * evaluated with the constants (min(thr, 44), its tanh, the top of 2 atanh)
 * that a decode launch with that threshold enabled hands its kernel, computed
 * by the same host code.  Other fn ignore thr; thr = 100 is the entry above. */
int qldpc_selftest_math_thr_device(int32_t fn, double thr, int32_t count, const double *d_in, double *d_out,
                                   void *stream);

/* Thread-local description of the last failure on this thread. */
const char *qldpc_last_error(void);

/* Library version string. */
const char *qldpc_version(void);

/* Diagnostic, host only: the exit-gate threshold the next decode launch hands
 * its kernel (the SPA register decoder runs a parity-only pass before a
 * check-node scan when the scan before counted at most this many unsatisfied
 * rows).  The library's constant, or QLDPC_EXIT_GATE under
 * QLDPC_DIAG=1.  It moves work, never a result. */
int32_t qldpc_exit_gate(void);

/* Number of HIP devices visible to the process (the C++ drop-in's default
 * device list: every GPU of the node). */
int qldpc_device_count(int32_t *count);

/* ---- Trial generator ------------------------------------
 * qldpc_trial_seeds: the simulation loop's per-trial seeds — `count` draws of
 * uniform_int_distribution<size_t>(0, SIZE_MAX) over Xoshiro256PlusPlus(
 * simulation_seed) (src/simulation.cpp:713-719).  Host only.
 * qldpc_trials_device: for each trial f, run_trial's keys
 * (src/simulation.cpp:540-551): Alice = fill_random_bits, Bob = inject_errors
 * (src/array_and_matrix_operations.cpp:889-933) from a generator seeded with
 * d_seeds[f] + seed_add (the loop's `seeds[n] + curr_sim`, :743), with
 * libstdc++ 11's draw consumption.  d_alice/d_bob: batch*n bytes.  Returns
 * the accurate QBER floor(n*qber)/n; QLDPC_EINVAL (the reference's "too small
 * for QBER" error) when floor(n*qber) == 0. */
int qldpc_trial_seeds(uint64_t simulation_seed, int32_t count, uint64_t *seeds_out);
/* qldpc_xoshiro_jump: the Xoshiro256 state (s0..s3) of a generator seeded
 * like Xoshiro-cpp with `seed`, after `draws` draws, by the GF(2) jump matrix
 * the device trial generator starts its second wave from (draws = n: the state
 * after fill_random_bits).  Host only; the generator's self-check. */
int qldpc_xoshiro_jump(uint64_t seed, uint64_t draws, uint64_t *state_out);
int qldpc_trials_device(int32_t n, double qber, int32_t batch, const uint64_t *d_seeds, uint64_t seed_add,
                        uint8_t *d_alice, uint8_t *d_bob, double *accurate_qber_out, void *stream);

/* ---- Rate adaptation (a15) -----------------------------
 * qldpc_xoshiro_state: the 4-word state of Xoshiro256PlusPlus(seed).
 * qldpc_adapt_code_rate: adapt_code_rate (src/array_and_matrix_operations.cpp:
 * 1131-1223): numbers and ascending positions of punctured / shortened bits
 * for (qber, delta, efficiency), drawing from the generator whose state is
 * prng_state (advanced in place, so successive calls chain like the
 * reference's setup loop, src/simulation.cpp:394-455).  Untainted puncturing
 * takes the first positions of the .untp list.  Out-of-range combinations
 * (the reference's WARNING + skip) return QLDPC_OK with zero counts.
 * punctured_out / shortened_out need capacity n (NULL: counts only).
 * qldpc_rate_plan_create: the position classes of one (punctured, shortened)
 * pair, replicated on the graph's devices (a host-only graph: on none, and no
 * device is touched).
 * qldpc_trials_rate_adapt_device: qldpc_trials_device plus, per trial, the
 * 2 * n_punct further draws QKD_LDPC_RATE_ADAPT takes for punctured positions
 * (src/qkd_ldpc_algorithm.cpp:1148-1157) -> d_punct_alice/bob [batch*n_punct].
 * qldpc_build_frames_rate_adapt_device: the extended frame (:1141-1180):
 * Alice's extended key [batch*n], LLRs (+-log_p / 1e-4 / DBL_MAX) [batch*n]
 * and Alice's syndrome [batch*m].
 * qldpc_qkd_ldpc_rate_adapt_batch_device: QKD_LDPC_RATE_ADAPT's window on
 * device: frame build + decode + keys_match against the extended key (:1216);
 * d_llr_ws nullable as in qldpc_qkd_ldpc_batch_device. */
typedef struct qldpc_rate_plan qldpc_rate_plan;
int qldpc_xoshiro_state(uint64_t seed, uint64_t *state_out);
/* qldpc_select_punctured_untainted: select_punctured_bits_untainted
 * (src/array_and_matrix_operations.cpp:1002-1067, arXiv:1103.6149) — the
 * untainted puncturing list get_punctured_bits_untainted (:1076-1123) writes
 * to a missing .untp file, in selection order.  H as the flattened
 * check_nodes (row_ptr/col_idx) and bit_nodes (col_ptr/row_idx) lists; draws
 * from prng_state (advanced in place, as the reference's setup loop passes
 * its generator).  punctured_out needs capacity n (NULL: count only). */
int qldpc_select_punctured_untainted(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                                     const int32_t *col_ptr, const int32_t *row_idx, uint64_t *prng_state,
                                     int32_t *punctured_out, int32_t *n_punctured);
int qldpc_adapt_code_rate(int32_t n, int32_t m, double qber, double delta, double efficiency,
                          int32_t untainted_enabled, const int32_t *untainted, int32_t n_untainted,
                          uint64_t *prng_state, int32_t *punctured_out, int32_t *n_punctured, int32_t *shortened_out,
                          int32_t *n_shortened, double *adapted_rate_out);
int qldpc_rate_plan_create(qldpc_graph *g, int32_t n_punct, const int32_t *punctured, int32_t n_short,
                           const int32_t *shortened, qldpc_rate_plan **out);
void qldpc_rate_plan_destroy(qldpc_rate_plan *plan);
int qldpc_trials_rate_adapt_device(int32_t n, double qber, int32_t batch, const uint64_t *d_seeds, uint64_t seed_add,
                                   int32_t n_punct, uint8_t *d_alice, uint8_t *d_bob, uint8_t *d_punct_alice,
                                   uint8_t *d_punct_bob, double *accurate_qber_out, void *stream);
int qldpc_build_frames_rate_adapt_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                                         const uint8_t *d_alice, const uint8_t *d_bob, const uint8_t *d_punct_alice,
                                         const uint8_t *d_punct_bob, const double *d_log_p, uint8_t *d_alice_ext,
                                         double *d_llr, uint8_t *d_syndrome, void *stream);
int qldpc_qkd_ldpc_rate_adapt_batch_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device,
                                           const qldpc_params *p, int32_t batch, const uint8_t *d_alice,
                                           const uint8_t *d_bob, const uint8_t *d_punct_alice,
                                           const uint8_t *d_punct_bob, const double *d_log_p, uint8_t *d_alice_ext,
                                           double *d_llr_ws, uint8_t *d_synd_ws, uint8_t *d_bits_out,
                                           uint32_t *d_iters_out, uint8_t *d_synd_ok_out, uint8_t *d_keys_match_out,
                                           void *stream);

/* ---- Two parties: Alice's syndromes, Bob's decode from his own key -------------
 * The entries above restate the reference's simulation, which holds both keys
 * side by side.  In error reconciliation itself neither side sees the other's
 * key: Alice publishes a syndrome, Bob decodes from his key, the received
 * syndrome and a QBER estimate.  These entries are that per-party cut of the
 * frame construction; what they write is byte for byte what the fused entries
 * write for the same inputs.
 *
 * Key bytes must be 0 or 1: only bit 0 of each byte is read, as in the fused
 * builders.
 *
 * Key layout with a plan: d_key is [batch][n] and only the first
 * n_key = n - n_punct - n_short entries of a row are used, exactly as
 * QKD_LDPC_RATE_ADAPT reads alice_bit_array[n]
 * (src/qkd_ldpc_algorithm.cpp:1169-1172), so the buffers
 * qldpc_trials_rate_adapt_device fills pass unchanged.  Without a plan the
 * key is the frame.
 *
 * qldpc_syndrome_batch_device (Alice): d_syndrome_out[f] = H * x_f, where x_f
 * is her key or, with a plan, her extended key: key bits at the plan's key
 * positions in order, d_punct_fill[f][k] at the k-th punctured position (her
 * private randomness, :1148-1157; [batch*n_punct], NULL allowed when there is
 * no plan or n_punct == 0) and 0 at shortened positions.  d_key_ext_out
 * (nullable, [batch*n]) receives x_f when a plan is given (without one it is
 * not written: the key is the frame).
 *
 * qldpc_reconcile_batch_device (Bob): qldpc_qkd_ldpc[_rate_adapt]_batch_device
 * minus Alice — Bob's LLRs from d_key and d_log_p (+-log_p[f]; with a plan
 * 1e-4 at punctured positions whatever he would draw there, :1153-1155, and
 * DBL_MAX at shortened ones), then the decode against d_syndrome ([batch*m],
 * read only).  d_llr_ws nullable as in qldpc_qkd_ldpc_batch_device;
 * d_posterior_out nullable as in qldpc_decode_batch_device.  Works on every
 * graph layout.  d_log_p as in qldpc_build_frames_device (qldpc_log_p).
 *
 * qldpc_extract_key_device: the inverse of the extension — d_key_out[f]
 * ([batch*n_key]) = d_bits[f] ([batch*n], a decoded frame or an extended key)
 * at the plan's key positions, in order.  Needs a plan.
 *
 * qldpc_syndrome_batch / qldpc_reconcile_batch: the same on HOST buffers,
 * synchronous, sharded over the graph's devices like qldpc_decode_batch (the
 * plan must live on every device of the graph).  Only key bytes, log_p and
 * syndromes cross to the device: n + m + 8 bytes per frame instead of the
 * 8 n + m of host-built LLRs.
 *
 * Arguments are checked in this order wherever the step applies: NULL graph,
 * the parameters, batch < 0, batch == 0 (OK), NULL buffers (and the plan of
 * the extract entry), the plan on the device, the device, the LDS fit
 * (QLDPC_EUNSUP beyond n of about 1.3 million; Alice with a plan about 650k).
 * Through batch == 0 no device is touched. */
int qldpc_syndrome_batch_device(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t device,
                                int32_t batch, const uint8_t *d_key, const uint8_t *d_punct_fill /* nullable */,
                                uint8_t *d_key_ext_out /* nullable */, uint8_t *d_syndrome_out, void *stream);
int qldpc_reconcile_batch_device(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t device,
                                 const qldpc_params *p, int32_t batch, const uint8_t *d_key, const double *d_log_p,
                                 const uint8_t *d_syndrome, double *d_llr_ws /* nullable */, uint8_t *d_bits_out,
                                 uint32_t *d_iters_out, uint8_t *d_synd_ok_out,
                                 double *d_posterior_out /* nullable */, void *stream);
int qldpc_extract_key_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                             const uint8_t *d_bits, uint8_t *d_key_out, void *stream);
int qldpc_syndrome_batch(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t batch,
                         const uint8_t *key, const uint8_t *punct_fill /* nullable */,
                         uint8_t *key_ext_out /* nullable */, uint8_t *syndrome_out);
int qldpc_reconcile_batch(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, const qldpc_params *p,
                          int32_t batch, const uint8_t *key, const double *log_p, const uint8_t *syndrome,
                          uint8_t *bits_out, uint32_t *iters_out, uint8_t *synd_ok_out,
                          double *posterior_out /* nullable */);

/* ---- Error estimation at the reconciliation stage ---------------------------------
 * Where the QBER comes from (Kiktenko, Malyshev, Bozhedarov, Pozhar, Anufriev,
 * Fedorov, arXiv:1810.05841): Bob estimates it from data the exchange already
 * holds, before the decode (the log_p of qldpc_reconcile_batch[_device]) and
 * after it (the q of the secret-length formulas).  Both are computed by Bob
 * alone: the estimates need nothing new from the channel.
 *
 * Definitions.  Bob's extended key x~_f: with a plan his key bits at the
 * plan's key positions and 0 at punctured and shortened positions; without a
 * plan his key.  Difference syndrome: z_f = s_A,f XOR H x~_f.  A check row j is
 * INFORMATIVE when it has no punctured neighbour (Alice's private fill makes
 * such a row uniform) and its effective degree d_j = deg_j - #shortened
 * neighbours is >= 1; without a plan every row of degree >= 1 is.  The CLASSES
 * are the distinct effective degrees of the informative rows, ascending,
 * d_1 < ... < d_C, with row counts N_c; R = sum of N_c.  The per-frame
 * statistic K_f (int32) is the number of informative rows with z_f[j] = 1.
 *
 * Estimator: method of moments on the weight.  A row of effective degree d
 * differs with probability (1 - (1 - 2q)^d) / 2, so q^ solves g(q^) = K on
 * [q_min, q_max] with
 *
 *     g(q) = sum over c of  N_c * (1 - (1 - 2q)^d_c) / 2
 *
 * g rises with q: the root is unique.  Only IEEE-754 binary64 add, subtract,
 * multiply and compare take part, in a fixed order (csrc/estimate_math.h, one
 * function for the kernel and the host entry): t = 1 - 2q; the powers t^d by
 * repeated multiplication from 1.0, carried from d_c to d_(c+1); the terms
 * N_c * (0.5 * (1 - t^d_c)) added in ascending class order into an accumulator
 * that starts at 0.0.  With F = frames_per_weight: if F g(q_min) >= K then
 * q^ = q_min; if F g(q_max) <= K then q^ = q_max; otherwise bisect, lo = q_min,
 * hi = q_max, mid = 0.5 (lo + hi), lo = mid when F g(mid) < K, else hi = mid,
 * until mid equals an end or 64 steps are made; q^ = 0.5 (lo + hi).  The same
 * weight gives the same bits on the host and on the device.
 *
 * Bounds: 0 < q_min <= q_max < 0.5, else QLDPC_EINVAL (NaN included): q^ lies
 * in (0, 0.5) and log_p is finite and positive.
 *
 * log_p = log1p((1 - 2 q^) / q^) = log((1 - q^) / q^), with the library's
 * restatement of glibc's log1p (qldpc_selftest_math_device fn 3): bit-identical
 * to the C library's log1p of that argument.  It is NOT claimed to equal
 * qldpc_log_p(q^) bit for bit: that function calls log().
 *
 * R == 0 (for example every row has a punctured neighbour): nothing can be
 * estimated.  Every estimating entry returns QLDPC_EINVAL ("no informative
 * rows") and launches nothing.
 *
 * Corrected errors: E_f = the key positions at which Bob's key differs from
 * the decoded frame.  With a plan #{i : position i is a key position,
 * key[src(i)] != bits[i]}, src(i) the position's index among the key
 * positions: punctured and shortened positions do not count.  Without a plan
 * the Hamming distance of the two n-bit rows.  It is the frame's exact error
 * count when the frame decoded to Alice's key, i.e. for frames that verified.
 * Only bit 0 of every key, syndrome and frame byte is read.
 *
 * qldpc_estimate_classes (host only; works on a qldpc_graph_create_host
 * graph): *n_classes = C, and the first min(C, cap) classes to degree_out /
 * rows_out (NULL allowed when cap == 0).  C == 0 is R == 0.
 *
 * qldpc_qber_from_weight (host only): qber_out[i] (and log_p_out[i]) from
 * weight[i], i < count.  frames_per_weight = 1: per-frame weights; F: each
 * weight is a sum over F frames (a pooled estimate).  A weight outside
 * [0, F R] is refused.
 *
 * qldpc_estimate_qber_device: K_f to d_weight_out, q^_f to d_qber_out, log_p_f
 * to d_log_p_out, [batch] each, each nullable (not all three).  The key layout
 * and strides are those of qldpc_reconcile_batch_device: with a plan d_key is
 * [batch][n] and the first n_key entries of a row are read.  When only
 * d_weight_out is given nothing is solved and the bounds are not looked at.
 * d_log_p_out can be handed to qldpc_reconcile_batch_device on the same stream
 * with no synchronisation in between.  Two launches: one workgroup per frame
 * for the weights, one thread per frame for the solve.  Works on every graph
 * layout; n is bounded by the LDS fit of the key in bit words (as for
 * qldpc_syndrome_batch_device); the solve takes at most 64 classes
 * (QLDPC_EUNSUP beyond; qldpc_qber_from_weight takes any number).
 *
 * qldpc_corrected_errors_device: E_f to d_errors_out [batch]; d_bits is
 * [batch][n], a decoded frame.
 *
 * qldpc_estimate_qber_batch / qldpc_corrected_errors_batch: the same on HOST
 * buffers, synchronous, sharded over the graph's devices like
 * qldpc_reconcile_batch.
 *
 * A plan is tied to the adjacency of the graph it was created for (its row
 * table is built then): with a graph of another adjacency the estimating
 * entries return QLDPC_EINVAL.
 *
 * Arguments are checked in the two-party order: NULL graph, batch < 0,
 * batch == 0 (OK), NULL buffers, then the bounds (when something is solved),
 * the plan's graph and R == 0, then the plan on the device, the device, the
 * LDS fit.  Through batch == 0 no device is touched. */
int qldpc_estimate_classes(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t cap,
                           int32_t *n_classes, int32_t *degree_out, int32_t *rows_out);
int qldpc_qber_from_weight(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t count,
                           const int64_t *weight, int64_t frames_per_weight, double q_min, double q_max,
                           double *qber_out, double *log_p_out /* nullable */);
int qldpc_estimate_qber_device(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t device,
                               int32_t batch, const uint8_t *d_key, const uint8_t *d_syndrome, double q_min,
                               double q_max, int32_t *d_weight_out /* nullable */, double *d_qber_out /* nullable */,
                               double *d_log_p_out /* nullable */, void *stream);
int qldpc_estimate_qber_batch(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t batch,
                              const uint8_t *key, const uint8_t *syndrome, double q_min, double q_max,
                              int32_t *weight_out /* nullable */, double *qber_out /* nullable */,
                              double *log_p_out /* nullable */);
int qldpc_corrected_errors_device(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t device,
                                  int32_t batch, const uint8_t *d_key, const uint8_t *d_bits, int32_t *d_errors_out,
                                  void *stream);
int qldpc_corrected_errors_batch(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t batch,
                                 const uint8_t *key, const uint8_t *bits, int32_t *errors_out);

/* ---- Blind reconciliation: disclosure rounds for frames that failed -------------
 * A frame whose decode ended with syndromes_match == 0 need not be lost, nor
 * the batch be sent again under another rate plan: in blind reconciliation
 * (Martinez-Mateo, Elkouss, Martin, arXiv:1205.5729) Alice discloses the values
 * of some of her punctured bits, Bob pins those positions and decodes the failed
 * frames again, until they decode or nothing is left to disclose.  No round
 * needs a new syndrome or a new plan; the failed-frame list and the disclosed
 * bits are all that crosses the channel.  Every disclosed bit is a leaked bit.
 *
 * qldpc_failed_frames_device: d_list_out[0 .. count) = the frames f with
 * d_synd_ok[f] == 0, ASCENDING (both parties index the round by this order),
 * and *d_count_out = count.  d_list_out holds `batch` entries; those past the
 * count are unspecified.  The caller reads the count (four bytes) between
 * rounds: n_list below is a host integer.
 *
 * qldpc_disclose_device (Alice): d_vals_out[j][i] = d_punct_fill[d_list[j]][d_disc[i]]
 * for j < n_list, i < n_disc.  d_disc holds indices k into the plan's ascending
 * punctured list, the k that index d_punct_fill ([batch][n_punct], the buffer
 * qldpc_syndrome_batch_device read).
 *
 * qldpc_reconcile_round_device (Bob): decodes the frames d_list[0 .. n_list) of
 * the batch again.  For each, the LLRs are exactly qldpc_reconcile_batch_device's
 * (+-log_p[f], 1e-4, DBL_MAX), except that the punctured position of index
 * d_disc[i] holds d_vals[j][i] ? -DBL_MAX : +DBL_MAX (bit 0 of the byte; the
 * builder's sign).  The frames are decoded from these LLRs like
 * qldpc_decode_batch_device's, on every graph layout: a disclosed -DBL_MAX has
 * no code in the register kernels' 2-bit palette, so a round never takes the
 * palette path that qldpc_reconcile_batch_device takes.  Results go to rows
 * d_list[j] of the [batch] outputs — iterations_num and syndromes_match of this
 * round's decode; rows that are not listed are not written, the posterior's
 * included.  n_disc == 0 is a plain re-decode of the listed frames.  The
 * compact frames live in the (device, stream) workspace.
 *
 * The caller's contract, which the device entries cannot check without a
 * synchronisation: d_list entries are distinct and in [0, batch); d_disc
 * entries are distinct and in [0, n_punct).  (Results are unspecified
 * otherwise.)  The host entries do check both.
 *
 * qldpc_disclose_batch / qldpc_reconcile_round_batch: the same on HOST buffers
 * and a host list, synchronous; contiguous slices of the LIST are sharded over
 * the graph's devices.  Only the listed frames' fill rows, or key rows, log_p,
 * syndromes and disclosed bytes, cross to the device.
 *
 * A plan is required (without punctured bits there is nothing to disclose).
 * Arguments are checked in the two-party order: NULL graph, the parameters,
 * batch < 0, n_list outside [0, batch], n_disc outside [0, n_punct],
 * n_list == 0 (OK; batch == 0 for the list entry), NULL plan and buffers, the
 * plan on the device, the device, the LDS fit.  Through n_list == 0 no device
 * is touched. */
int qldpc_failed_frames_device(int32_t batch, const uint8_t *d_synd_ok, int32_t *d_list_out /* batch */,
                               int32_t *d_count_out, void *stream);
int qldpc_disclose_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t n_list,
                          const int32_t *d_list, const uint8_t *d_punct_fill /* [batch][n_punct] */, int32_t n_disc,
                          const int32_t *d_disc, uint8_t *d_vals_out /* [n_list][n_disc] */, void *stream);
int qldpc_reconcile_round_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, const qldpc_params *p,
                                 int32_t batch, const uint8_t *d_key, const double *d_log_p,
                                 const uint8_t *d_syndrome, int32_t n_list, const int32_t *d_list, int32_t n_disc,
                                 const int32_t *d_disc, const uint8_t *d_vals /* [n_list][n_disc] */,
                                 uint8_t *d_bits_out, uint32_t *d_iters_out, uint8_t *d_synd_ok_out,
                                 double *d_posterior_out /* nullable */, void *stream);
int qldpc_disclose_batch(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, int32_t n_list,
                         const int32_t *list, const uint8_t *punct_fill /* [batch][n_punct] */, int32_t n_disc,
                         const int32_t *disc, uint8_t *vals_out /* [n_list][n_disc] */);
int qldpc_reconcile_round_batch(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p, int32_t batch,
                                const uint8_t *key, const double *log_p, const uint8_t *syndrome, int32_t n_list,
                                const int32_t *list, int32_t n_disc, const int32_t *disc,
                                const uint8_t *vals /* [n_list][n_disc] */, uint8_t *bits_out, uint32_t *iters_out,
                                uint8_t *synd_ok_out, double *posterior_out /* nullable */);

/* ---- Symmetric blind reconciliation: disclose each frame's least reliable bits ----
 * The rounds above disclose punctured bits in one order fixed in advance.  In
 * symmetric blind reconciliation (Kiktenko, Trushechkin, Lim, Kurochkin,
 * Fedorov, Phys. Rev. Applied 8, 044017, arXiv:1612.03673) Bob's posteriors of
 * the failed decode say where the decoder is unsure: he names, per frame, the
 * `count` positions of smallest |posterior|, Alice answers with her bits there,
 * and Bob pins those positions and decodes again.  The positions are per FRAME:
 * d_pos is [batch][cap] int32, row f holding frame f's positions in the order
 * they were disclosed.  A frame that still fails has been in every round, so
 * first, count and n_disc are the same for every listed frame.  A plan is
 * optional: without one every position is a key position.  A disclosed bit is
 * one leaked bit whatever its class; disclosed key positions stay in the key.
 *
 * qldpc_select_positions_device (Bob): for each frame f = d_list[j], j < n_list,
 * d_pos[f][first .. first + count) = the `count` smallest candidates of row f of
 * d_posterior ([batch][n]) in the following order, smallest first.  Position i
 * sorts by the pair (u, i), compared lexicographically, u = the 64 bits of the
 * posterior with the sign bit cleared, as an unsigned integer: +-0 lowest, then
 * denormals, normals, +-inf, NaN; equal magnitudes go to the lower index.  The
 * order is total and uses no floating-point compare, so both numpy and the
 * device reproduce it bit for bit, and a shorter selection is a prefix of a
 * longer one.  Candidates are all positions except the plan's shortened ones and
 * the frame's earlier positions d_pos[f][0 .. first).  Punctured positions are
 * candidates.  count is at most QLDPC_SELECT_MAX (QLDPC_EUNSUP beyond, nothing is
 * launched).  Rows of frames that are not listed and columns outside
 * [first, first + count) are not written.
 *
 * qldpc_disclose_positions_device (Alice): d_vals_out[j][i] =
 * d_ext[f][d_pos[f][first + i]] & 1 for f = d_list[j], i < count.  d_ext is her
 * extended key (qldpc_syndrome_batch_device's d_key_ext_out) when there is a
 * plan and her key otherwise, in rows of ext_stride >= n bytes.
 *
 * qldpc_reconcile_positions_round_device (Bob): qldpc_reconcile_round_device
 * with positions.  The LLRs of frame f = d_list[j] are
 * qldpc_reconcile_batch_device's, then position d_pos[f][i] holds
 * d_vals[j][i] ? -DBL_MAX : +DBL_MAX for i < n_disc, whatever the position's
 * class.  d_vals is [n_list][n_disc]: Bob appends each round's answer to his
 * per-frame history.  Decode, scatter and outputs are the fixed-order round's.
 *
 * The caller's contract, which the device entries cannot check without a
 * synchronisation: d_list entries are distinct and in [0, batch); each listed
 * frame's d_pos[f][0 .. first) (select), [first, first + count) (disclose) or
 * [0, n_disc) (round) are distinct and in [0, n); count <= n - n_short - first,
 * the frame's candidates.  (A position outside [0, n) is skipped, and a count
 * beyond the candidates leaves -1 in the entries no candidate fills; results are
 * unspecified otherwise.)  The host entries check all of it (QLDPC_EINVAL).
 *
 * The _batch entries: the same on HOST buffers and a host list, synchronous;
 * contiguous slices of the LIST are sharded over the graph's devices and only
 * the listed frames' rows cross to the device.
 *
 * Arguments are checked in the two-party order: NULL graph, the parameters,
 * batch < 0, n_list outside [0, batch], first / count / n_disc < 0 or past cap
 * (first + count <= cap, n_disc <= cap) and ext_stride < n, n_list == 0 (OK),
 * NULL buffers, the host entries' list and position checks, count >
 * QLDPC_SELECT_MAX, the plan on the device, the device, the LDS fit
 * (QLDPC_EUNSUP beyond n of about 850k).  Through n_list == 0 no device is
 * touched. */
#define QLDPC_SELECT_MAX 4096 /* positions per frame and call: the winners are sorted in LDS */
int qldpc_select_positions_device(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t device,
                                  int32_t batch, const double *d_posterior /* [batch][n] */, int32_t n_list,
                                  const int32_t *d_list, int32_t first, int32_t count,
                                  int32_t *d_pos /* [batch][cap] */, int32_t cap, void *stream);
int qldpc_disclose_positions_device(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t device,
                                    int32_t n_list, const int32_t *d_list, const uint8_t *d_ext, int64_t ext_stride,
                                    const int32_t *d_pos /* [batch][cap] */, int32_t cap, int32_t first,
                                    int32_t count, uint8_t *d_vals_out /* [n_list][count] */, void *stream);
int qldpc_reconcile_positions_round_device(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t device,
                                           const qldpc_params *p, int32_t batch, const uint8_t *d_key,
                                           const double *d_log_p, const uint8_t *d_syndrome, int32_t n_list,
                                           const int32_t *d_list, int32_t n_disc,
                                           const int32_t *d_pos /* [batch][cap] */, int32_t cap,
                                           const uint8_t *d_vals /* [n_list][n_disc] */, uint8_t *d_bits_out,
                                           uint32_t *d_iters_out, uint8_t *d_synd_ok_out,
                                           double *d_posterior_out /* nullable */, void *stream);
int qldpc_select_positions_batch(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t batch,
                                 const double *posterior /* [batch][n] */, int32_t n_list, const int32_t *list,
                                 int32_t first, int32_t count, int32_t *pos /* [batch][cap] */, int32_t cap);
int qldpc_disclose_positions_batch(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */, int32_t batch,
                                   int32_t n_list, const int32_t *list, const uint8_t *ext, int64_t ext_stride,
                                   const int32_t *pos /* [batch][cap] */, int32_t cap, int32_t first, int32_t count,
                                   uint8_t *vals_out /* [n_list][count] */);
int qldpc_reconcile_positions_round_batch(qldpc_graph *g, const qldpc_rate_plan *plan /* nullable */,
                                          const qldpc_params *p, int32_t batch, const uint8_t *key,
                                          const double *log_p, const uint8_t *syndrome, int32_t n_list,
                                          const int32_t *list, int32_t n_disc, const int32_t *pos /* [batch][cap] */,
                                          int32_t cap, const uint8_t *vals /* [n_list][n_disc] */, uint8_t *bits_out,
                                          uint32_t *iters_out, uint8_t *synd_ok_out,
                                          double *posterior_out /* nullable */);

/* ---- Key verification and privacy amplification: a batched Toeplitz hash ---------
 * After reconciliation both sides hold key_len bits per frame.  A universal
 * hash of them closes the protocol twice: a short output (64 bits) is the
 * verification tag the two sides compare, since syndromes_match alone does not
 * prove equal keys; a long output, with a length per frame, is privacy
 * amplification, which takes out what the syndromes and the disclosed bits of
 * the blind rounds leaked.
 *
 * For a frame's key x[0 .. L) (L = key_len), the public seed s[0 .. L + r - 1)
 * shared by the batch, and r = out_len:
 *
 *     y[i] = XOR over j in [0, L) of  s[i + L - 1 - j] & x[j]      for i in [0, r)
 *
 * the Toeplitz matrix T[i][j] = s[i - j + L - 1] over GF(2).
 *
 * Prefix property: row i reads s[i .. i + L) only, so the first r' outputs of a
 * hash are the hash for out_len = r' under the seed's first L + r' - 1 entries.
 * Per-frame output lengths therefore cost nothing: a shorter frame is a prefix
 * of the same hash.
 *
 * All bit arrays are bytes.  Only bit 0 of a key byte or a seed byte is read;
 * outputs are 0 or 1.
 *
 * qldpc_toeplitz_hash_device: d_keys holds `batch` rows, key_stride bytes apart
 * (>= key_len; bytes of a row past key_len are never part of the result), so
 * the [batch][n_key] keys of qldpc_extract_key_device, [batch][n] decoded bits
 * and Alice's [batch][n] key rows of which the first n_key count all pass
 * unchanged.  d_out is [batch][out_len] and is always written whole: with
 * d_out_len NULL every frame gets out_len outputs, otherwise frame f keeps its
 * first d_out_len[f] outputs (a value outside [0, out_len] is clamped into it)
 * and the rest of its row is 0.  No graph, no workspace, no allocation: it runs
 * on the current device, asynchronous on `stream`, and nothing outlives the
 * call.
 *
 * qldpc_toeplitz_hash_batch: the same on HOST buffers, synchronous; the
 * buffers are staged on the current device for the call (QLDPC_ENOMEM when they
 * do not fit).  It refuses an out_lens entry outside [0, out_len] with
 * QLDPC_EINVAL.
 *
 * Arguments are checked in this order: batch < 0, key_len < 1, out_len < 1,
 * key_stride < key_len (QLDPC_EINVAL); batch == 0 (QLDPC_OK); NULL keys, seed
 * or output (QLDPC_EINVAL); the LDS fit — a workgroup keeps the keys of four
 * frames and its window of the seed in LDS as bit words, which limits key_len
 * to 261,888 bits (QLDPC_EUNSUP beyond; also for a batch of 2^26 frames
 * or more, or an out_len of more than 65535 * 1024); the host entry's out_lens.
 * Through these no device is touched. */
int qldpc_toeplitz_hash_device(int32_t batch, int32_t key_len, int64_t key_stride, const uint8_t *d_keys,
                               int32_t out_len, const uint8_t *d_seed /* [key_len + out_len - 1] */,
                               const int32_t *d_out_len /* nullable, [batch] */,
                               uint8_t *d_out /* [batch][out_len] */, void *stream);
int qldpc_toeplitz_hash_batch(int32_t batch, int32_t key_len, int64_t key_stride, const uint8_t *keys,
                              int32_t out_len, const uint8_t *seed /* [key_len + out_len - 1] */,
                              const int32_t *out_lens /* nullable, [batch] */, uint8_t *out /* [batch][out_len] */);

/* ---- Block privacy amplification: one Toeplitz hash over many frames ------------
 * The statistical terms of a finite-key bound fall like 1/sqrt(block length), so
 * keys are verified and amplified in blocks of 10^6 .. 10^8 bits: hundreds to
 * thousands of frames hashed as one key.  The block is the concatenation, in
 * LIST ORDER, of the listed frames' keys,
 *
 *     x[t * key_len + j] = d_keys[d_list[t]][j] & 1      t < n_list, j < key_len
 *
 * with L = n_list * key_len, and the hash is the formula above, unchanged, with
 * r = out_len and a seed of L + r - 1 entries:
 *
 *     y[i] = XOR over j in [0, L) of  s[i + L - 1 - j] & x[j]      for i in [0, r)
 *
 * For a one-frame block it is qldpc_toeplitz_hash_device's row of that frame, bit
 * for bit, and the prefix property holds as it does there.  The cost is
 * O(N log N), N the smallest power of two >= L + r - 1: y[i] is bit 0 of entry
 * i + L - 1 of the integer convolution of s and x, which a number-theoretic
 * transform of length N modulo the prime 15 * 2^27 + 1 computes exactly (every
 * entry is a count <= L).  No floating point takes part.  The limit is
 * L + out_len - 1 <= 2^27 (QLDPC_EUNSUP beyond).
 *
 * qldpc_toeplitz_block_workspace: the bytes of workspace a call with this
 * block length L and out_len needs (two arrays of N words, the table of N
 * twiddles, 16 bytes of alignment slack), or a negative QLDPC_E*: QLDPC_EINVAL
 * for block_len < 1 or out_len < 1, QLDPC_EUNSUP beyond the limit.
 *
 * qldpc_toeplitz_hash_block_device: d_keys holds rows key_stride bytes apart
 * (>= key_len), as for qldpc_toeplitz_hash_device.  n_list is a host integer
 * (the verdicts crossed the channel: both sides know the count); d_list holds
 * n_list frame indices in any order, repeats allowed, or is NULL for the frames
 * 0 .. n_list - 1.  That its entries index rows of d_keys is the caller's
 * contract: the device entry cannot check it.  The call is asynchronous on
 * `stream`, allocates nothing, and writes only d_out[0 .. out_len) and
 * d_ws[0 .. ws_bytes).  The twiddle table is rebuilt by every call: the
 * workspace carries nothing from one call to the next, and what it held before
 * does not matter.
 *
 * qldpc_toeplitz_hash_block: the same on HOST buffers, synchronous.  keys holds
 * `batch` rows; only the listed rows are staged on the current device, with a
 * workspace of the call's own (QLDPC_ENOMEM when they do not fit).  It refuses a
 * list entry outside [0, batch) with QLDPC_EINVAL.
 *
 * Arguments are checked in this order: (1) n_list < 0, key_len < 1, out_len < 1,
 * key_stride < key_len, and for the host entry batch < 0 or n_list > batch
 * (QLDPC_EINVAL); (2) n_list == 0 (QLDPC_OK, nothing is written); (3) NULL keys,
 * seed, output or workspace (QLDPC_EINVAL); (4) L + out_len - 1 > 2^27
 * (QLDPC_EUNSUP); (5) ws_bytes below qldpc_toeplitz_block_workspace(L, out_len)
 * (QLDPC_EINVAL; qldpc_last_error() names the size needed); (6) the host
 * entry's list entries.  Through these no device is touched. */
int64_t qldpc_toeplitz_block_workspace(int64_t block_len, int64_t out_len);
int qldpc_toeplitz_hash_block_device(int32_t n_list, const int32_t *d_list /* nullable: frames 0..n_list-1 */,
                                     int32_t key_len, int64_t key_stride, const uint8_t *d_keys, int64_t out_len,
                                     const uint8_t *d_seed /* [L + out_len - 1] */, uint8_t *d_out /* [out_len] */,
                                     void *d_ws, int64_t ws_bytes, void *stream);
int qldpc_toeplitz_hash_block(int32_t batch, int32_t n_list, const int32_t *list /* nullable */, int32_t key_len,
                              int64_t key_stride, const uint8_t *keys, int64_t out_len,
                              const uint8_t *seed /* [L + out_len - 1] */, uint8_t *out /* [out_len] */);

/* ---- Simulation-driver helpers ----------------------
 * qldpc_sort_permutation: the order std::sort (libstdc++, not stable) leaves a
 * sequence in when comparing only `keys` — how the reference orders its
 * config maps by code_rate (src/config.cpp:43,289,355,389).
 * qldpc_bits_to_remove: privacy-maintenance bit positions
 * (get_bits_positions_to_remove / _rate_adapt,
 * src/array_and_matrix_operations.cpp:138-256), ascending; out needs capacity
 * n (NULL: count only).  The out-key length of the throughput columns is
 * n - count. */
int qldpc_sort_permutation(const double *keys, int32_t n, int32_t *perm_out);
int qldpc_bits_to_remove(int32_t n, int32_t m, const int32_t *col_ptr, const int32_t *row_idx, int32_t n_punct,
                         const int32_t *punctured, int32_t n_short, const int32_t *shortened, int32_t rate_adapt,
                         int32_t *out, int32_t *count);

/* ---- The simulation loop's batch seam --------------
 * qldpc_run_trials: run_trial for `count` trials of one combination
 * (src/simulation.cpp:540-576) — the body of QKD_LDPC_batch_simulation's
 * pool.detach_loop(0, TRIALS_NUMBER) (:721-746) — with host pointers only.
 * Trial t: a generator seeded with seeds[t] + seed_add (the loop's
 * `seeds[n] + curr_sim`), Alice = fill_random_bits, Bob = inject_errors
 * (src/array_and_matrix_operations.cpp:889-933), then QKD_LDPC (plan == NULL,
 * src/qkd_ldpc_algorithm.cpp:1031-1119) or QKD_LDPC_RATE_ADAPT with the plan's
 * punctured / shortened positions (:1121-1258, the punctured draws continuing
 * from the same generator).  Everything happens on device: only the seeds go
 * in and {iterations_num, syndromes_match, keys_match} per trial come back.
 * The trials are split in contiguous slices over the graph's devices, one
 * host thread each, no collectives; on each device chunks alternate over two
 * streams so the next chunk's trials are generated while one decodes.
 * runtime_us_out (nullable): trial_result::runtime — the measured duration of
 * the trial's chunk window (frame build + decode + key compare; trial
 * generation excluded, as :559-568 time only the QKD_LDPC call) shared out
 * over the chunk's trials in proportion to each trial's own decode span (its
 * frame's claim-to-result time on the GPU).  accurate_qber_out (nullable):
 * floor(n * qber) / n, every trial's trial_result::accurate_QBER.
 * Errors: QLDPC_EINVAL with run_trial's message when floor(n * qber) == 0. */
int qldpc_run_trials(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p, double qber,
                     int32_t count, const uint64_t *seeds, uint64_t seed_add, uint32_t *iters_out,
                     uint8_t *synd_ok_out, uint8_t *keys_match_out, double *runtime_us_out,
                     double *accurate_qber_out);
/* qldpc_run_trials in two halves, so the simulation loop can put combination
 * c + 1 on the devices before it collects combination c (the loop over
 * combinations, src/simulation.cpp:725-765): _submit checks the arguments
 * exactly as qldpc_run_trials, copies the seeds and enqueues the trials
 * (blocking only when both of a device's pipeline slots still hold chunks, which
 * it then collects for their own jobs), and returns a job; _wait completes the
 * job's outputs, frees it and returns the first error of any device slice.
 * Between the two the output arrays, the graph and the plan must stay alive;
 * the seeds need not.  Every submitted job must be waited for. */
typedef struct qldpc_trials_job qldpc_trials_job;
int qldpc_run_trials_submit(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p, double qber,
                            int32_t count, const uint64_t *seeds, uint64_t seed_add, uint32_t *iters_out,
                            uint8_t *synd_ok_out, uint8_t *keys_match_out, double *runtime_us_out,
                            double *accurate_qber_out, qldpc_trials_job **job_out);
int qldpc_run_trials_wait(qldpc_trials_job *job);
/* The device slice of the batch seam: trials [*lo, *hi) of `count` for shard
 * `shard` of `shards` (contiguous slices of ceil(count / shards); trailing
 * shards may be short or empty).  Host only. */
int qldpc_shard_range(int32_t count, int32_t shards, int32_t shard, int32_t *lo, int32_t *hi);

#ifdef __cplusplus
}
#endif
#endif
