/* gkr_amd -- C ABI of the MI355X (gfx950) GKR sumcheck prover.
 *
 * Drop-in boundary for ONE path of jeong0982/gkr: the GKR prover's per-layer
 * sumcheck and what feeds it.  The reference has no FFI; its boundary is two
 * crate-internal Rust functions, and every entry point below names the one it
 * replaces.  INTEGRATION.md shows the Rust-side binding.
 *
 *   reference                                                    this library
 *   -----------------------------------------------------------  ----------------------------
 *   prover::prove(&GKRCircuit,&Input) -> Proof                    gkr_prove
 *       rust/src/gkr/prover.rs:6-96 (called aggregator.rs:354,415)
 *   sumcheck::prove_sumcheck_opt(add_wire,mult_wire,add_i,...)    gkr_sumcheck_layer
 *       rust/src/gkr/sumcheck.rs:36-156 (called prover.rs:52-60)
 *   sumcheck::prove_sumcheck(g, v)                                gkr_sumcheck_mle[_batch_device]
 *       rust/src/gkr/sumcheck.rs:158-214 (python/sumcheck.py:6-53)
 *   convert::calculate_input (forward step)                       gkr_layer_eval
 *       rust/src/convert.rs:812-831
 *   wiring predicates add_i/mult_i restricted to z                gkr_predicate_tables
 *       rust/src/convert.rs:715-767 + prover.rs:24-37 (poly.rs:28-62)
 *   poly::reduce_multiple_polynomial / l_function                 inside gkr_prove
 *       rust/src/gkr/poly.rs:469-500, 538-551
 *   Mimc7::new(91).multi_hash(v, &Fr::from(0))  (mimc-rs)         gkr_mimc7_multi_hash
 *       call sites sumcheck.rs:45,84,129,152; prover.rs:10,78
 *
 * Data: a field element is halo2curves bn256::Fr exchanged as its 32-byte
 * little-endian canonical repr (sumcheck.rs:10-22): gkr_fr, 4 LE u64 limbs,
 * value < r.  Never Montgomery at this ABI.
 *
 * Tables are dense evaluation tables over the boolean hypercube, index = the
 * variables' bit string with variable 1 most significant (poly.rs:507).
 *
 * Round vectors: the reference returns Vec<S> of varying length, highest degree
 * first (poly.rs:260-267).  Here every round has a fixed row of slots (2 for the
 * plain sumcheck, 3 for the layer sumcheck), RIGHT-aligned: the last slot is the
 * constant term, out_len says how many trailing slots form the reference's
 * vector, unused leading slots are zero.
 *
 * Ownership: the caller allocates every output; the library owns device memory
 * inside the context.  Errors: the reference panics; this ABI returns a status
 * and never aborts.  Threading: a context is single-owner (one HIP stream);
 * distinct contexts may be used concurrently (the reference calls prove from a
 * rayon par_iter, aggregator.rs:350-355).
 *
 * There is no CPU fallback: every compute entry point needs a gfx950 device and
 * returns GKR_ERR_NO_DEVICE / GKR_ERR_HIP otherwise.
 */
#ifndef GKR_AMD_H
#define GKR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } gkr_fr;

typedef struct gkr_ctx gkr_ctx;

/* ---- limits (every size limit of the library; tests/test_host_library.py checks this table against the code) ----
 * The reference proves any GKRCircuit its compiler emits (prover.rs:6-96; layers padded to whatever 2^k they need,
 * convert.rs:209-214).  The library's limits are those of 32-bit gate indices and device memory, not of a table form:
 *   GKR_MAX_K_NEXT   widest next layer of a layer sumcheck (2^k_next values W; k[i+1] of gkr_prove): U, V, W, the
 *                    c-phase row and eq(u, .) are 2^k_next-entry tables in HBM (9 x 32 B per value and proof);
 *   GKR_MAX_K_I      most gates of a layer, 2^k_i (also the output layer k[0]); sorted gate lists cost 16 B per gate;
 *   GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT   with GKR_TRANSCRIPT_DEVICE the layer sumcheck works on dense 2^(2 k_next)-entry
 *                    predicate tables (the host-free form is complete, not fast): k_next <= 14;
 *   GKR_MAX_MLE_N    plain sumcheck: tables of 2^n values, batch * 2^n <= 2^30 values (32 GiB) per call;
 *   GKR_MAX_BATCH    proofs per gkr_prove_batch call.
 * A call beyond a limit returns GKR_ERR_INVALID and names the limit in gkr_last_error. */
#define GKR_MAX_K_NEXT 24
#define GKR_MAX_K_I 28
#define GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT 14
#define GKR_MAX_MLE_N 30
#define GKR_MAX_BATCH 4096

enum {
    GKR_OK = 0,
    GKR_ERR_INVALID = 1,      /* bad sizes / null pointers / operand index out of range */
    GKR_ERR_NON_CANONICAL = 2,/* a field element >= r (the reference unwrap()s from_repr, sumcheck.rs:16,21) */
    GKR_ERR_NO_DEVICE = 3,
    GKR_ERR_HIP = 4,          /* a HIP runtime call failed; see gkr_last_error */
    GKR_ERR_NOMEM = 5,
    GKR_ERR_DEGENERATE = 6,   /* v == 0: the reference underflows (sumcheck.rs:49) */
    GKR_ERR_UNSUPPORTED = 7   /* an R1CS shape the reference's compiler cannot handle either (it panics or recurses
                                 without end: a constraint with an empty A, B or C, convert.rs:619-622) */
};

/* Transcript placement: where the per-round MiMC7 hash runs.  The hash is a
 * 728-deep serial chain of modular products per round vector with no data
 * parallelism inside it; all table work stays on the GPU in both modes. */
enum {
    GKR_TRANSCRIPT_DEVICE = 0, /* one GPU lane per sumcheck; no host involvement per round */
    GKR_TRANSCRIPT_HOST = 1    /* default: the device publishes the round sums to pinned memory, host
                                  cores hash (one sumcheck per thread), the next launch reads r_j */
};

const char *gkr_strerror(int status);
const char *gkr_version(void);

/* ---- context ---------------------------------------------------------- */
int  gkr_ctx_create(int device_id, gkr_ctx **out);
/* ONE host process driving several GPUs, as the reference is one process whose par_iter fans prover::prove out over the
 * (circuit, input) pairs of a step (aggregator.rs:350-355, 411-416): the context lives on device_ids[0]; gkr_prove_many
 * deals its items, by estimated cost, over child contexts created round-robin on ALL the listed devices (each with its
 * own thread, stream, workspaces and circuit cache; a device listed k times gets k child contexts per round -- which is
 * also how the dealing is tested on a box with one GPU).  Every other entry point runs on device_ids[0].
 * n_devices in [1, 64].  gkr_ctx_device_count: how many devices the context deals over (1 for gkr_ctx_create). */
int  gkr_ctx_create_multi(const int *device_ids, int n_devices, gkr_ctx **out);
int  gkr_ctx_device_count(const gkr_ctx *ctx);
void gkr_ctx_destroy(gkr_ctx *ctx);
const char *gkr_last_error(const gkr_ctx *ctx);
int  gkr_ctx_set_transcript(gkr_ctx *ctx, int mode);
/* Host threads this context may keep busy with the transcript (the calling thread included); 0 = the default:
 * GKR_HOST_THREADS, else (CPUs of the affinity mask and cgroup quota) / LOCAL_WORLD_SIZE - 2.  A process that drives
 * several contexts from several threads (the reference proves its <= 20 sub-circuits from a rayon par_iter,
 * aggregator.rs:350-355) gives each context its share; 1 = hash on the calling thread, no workers. */
int  gkr_ctx_set_host_threads(gkr_ctx *ctx, int threads);
/* The library's switches, per context.  gkr_amd/csrc/options.h holds the ONE table of them (name, default, what it does;
 * gkr_option_count / _name / _doc / _env enumerate it); a context takes the table's defaults -- or, for a test or an A/B
 * script that cannot call in, the value of the environment variable named in the table -- when it is created, and
 * gkr_ctx_set_option changes one value for this context only (cached per-circuit state built under the old value is
 * dropped; resident layers keep the layout they were created with, so set options first).  `name` is the option's name
 * ("rounds_per_pass") or its environment variable ("GKR_ROUNDS_PER_PASS").  No option changes a result: each is a choice
 * between schedules or kernel forms that the parity suite holds bit-exact against each other.  gkr_prove_many's child
 * contexts prove with the options of the context the call was made on. */
int  gkr_ctx_set_option(gkr_ctx *ctx, const char *name, long long value);
int  gkr_ctx_get_option(const gkr_ctx *ctx, const char *name, long long *value);
int  gkr_option_count(void);
const char *gkr_option_name(int index);
const char *gkr_option_doc(int index);
const char *gkr_option_env(int index);
int  gkr_ctx_device_name(const gkr_ctx *ctx, char *buf, size_t len);
/* Contexts proving side by side (one calling thread each -- the reference's par_iter over the (circuit, input) pairs,
 * aggregator.rs:350-355) share their host work: a thread that waits for its own GPU round takes pieces of another
 * context's posted work (a 16-lane hash call, a proof's line restriction).  A thread that has run out of proving
 * calls can lend itself to the others: gkr_host_help_while runs such pieces on the calling thread while *busy != 0
 * (the caller's count of threads still proving) and returns the number of pieces it ran.  GKR_NO_HELP=1 disables
 * the sharing. */
long gkr_host_help_while(const volatile int32_t *busy);
/* Where the proving threads' time goes, summed over every thread of the process while enabled (what GKR_DEBUG_TIMING prints
 * per call, as figures): enable = 1 clears the totals and starts counting, 0 stops.  gkr_host_accounting_read fills, in
 * microseconds: [0] a thread's own host pieces (hashing, incl. waiting for helpers to finish theirs), [1] pieces of other
 * contexts' work taken while waiting for its own GPU round, [2] spinning on the GPU with nothing to take, [3] the rest of
 * its gkr_prove / gkr_prove_batch calls (launches, set-up, copies), [4] pieces run by threads that had no proof left
 * (gkr_host_help_while), [5] their time with nothing to take, [6] the number of proving calls counted, and with
 * count >= 8 [7] the time gkr_prove_many's threads took to start on their items after the call woke them.  count >= 7.
 * With count >= 28 also the hashing PIECES of the layer sumchecks themselves, whoever ran them: [8] how many, [9] their time,
 * [10] the part of it inside the pass function (a piece's J hashes per transcript -- in IFMA lanes, or on the scalar code for
 * fewer than three transcripts -- and the field arithmetic between them; the rest of [9] is copying the round vectors out),
 * [10 + n] the number of pieces that carried n transcripts (n = 1 .. 16: the lanes of an IFMA call that were filled).
 * [0] + [1] + [4] - [9] is what the threads spent posting pieces, looking for them and waiting for the last one of a pass.
 * The reference has no counterpart (rayon hides its scheduling); bench.py reports these for its aggregated-proofs leg. */
int  gkr_host_accounting(int enable);
int  gkr_host_accounting_read(double *out_us, size_t count);

/* Per-kernel timing with HIP events on the stream each kernel is launched on (bench.py's
 * roofline leg).  enable: 0 off, 1 every kernel, 2 only the bandwidth-bound kernels ("mle_multifold",
 * "mle_sub_sums", "mle_fold_sum", "layer_round", ...): the small kernels on the round-trip path are
 * left alone so that the event records do not show in the wall time being measured.
 * kernel: "mle_multifold" (streaming fold passes on the main stream), "mle_multifold_late" (the small late fold
 * passes on the high-priority stream, overlapping other groups' passes), "mle_sub_sums", "mle_sub_reduce", "mle_pass_small", "mle_fold_plan",
 * "mle_fold_sum", "mle_sum_first", "mle_round_hash", "layer_round", "layer_fold", "layer_round_hash", "verify_hash" (the
 * verifier's challenge hashes on the device, gkr_verify_prepared and gkr_mimc7_multi_hash_device: bytes = rows x (96 + 4 + 36);
 * no launches under this name means the host hashed). */
int  gkr_ctx_profile(gkr_ctx *ctx, int enable);
int  gkr_ctx_profile_get(gkr_ctx *ctx, const char *kernel, uint64_t *launches, double *total_ms,
                         double *algorithmic_bytes);
/* the single launches behind a row (duration and algorithmic bytes of each, in launch order; the first 4096 since
 * the last reset): *count = how many there are, at most `capacity` are written */
int  gkr_ctx_profile_samples(gkr_ctx *ctx, const char *kernel, double *ms, double *bytes, size_t capacity, size_t *count);
int  gkr_ctx_profile_reset(gkr_ctx *ctx);

/* ---- MiMC7 (host; no device needed) ------------------------------------ */
/* multi_hash(arr, key): r = key; for a in arr: r += a + hash(a, r) */
int  gkr_mimc7_multi_hash(const gkr_fr *arr, size_t n, const gkr_fr *key, gkr_fr *out);
int  gkr_mimc7_hash(const gkr_fr *x, const gkr_fr *k, gkr_fr *out);
int  gkr_mimc7_constant(int i, gkr_fr *out);     /* i in 0..90 */
/* the device arithmetic (8x32-bit Montgomery) run on the host, for CPU-side unit tests */
int  gkr_selftest_mul(const gkr_fr *a, const gkr_fr *b, gkr_fr *out);
int  gkr_selftest_wide_sum(const gkr_fr *vals, size_t n, gkr_fr *out);
/* the host transcript's batched hash: eight right-aligned 3-slot round vectors at once */
int  gkr_selftest_hash8(const gkr_fr *vecs, const uint32_t *len, gkr_fr *out, int *used_ifma);
/* the host's share of one multi-round pass of the plain sumcheck: `count` <= 16 sumchecks with 2^J <= 32 sub-block
 * sums each (rows of 32: sums[k*32 + b]) -> per round t < J and sumcheck k (index t*count + k) the round polynomial
 * c1 x + c0, the vector's length (final_len non-null: the lengths of the last round are given), the challenge
 * multi_hash(vector); w[k*32 + b], b < 2^J: the weights eq(r, b) of the fold pass that follows (canonical, first
 * challenge = most significant index bit).  Scalar code; its IFMA-lane form runs beside it when the CPU has it and
 * must agree. */
int  gkr_selftest_host_pass(const gkr_fr *sums, int count, int J, const uint32_t *final_len, gkr_fr *c0, gkr_fr *c1,
                            uint32_t *len, gkr_fr *r, gkr_fr *w, int *used_ifma);
/* the host tail of a phase's product passes (once the tables are down to 2^host_tail_log2 entries the host forms the passes'
 * records itself, from tables the last device pass leaves in pinned memory): tables = W, X, Y of 2^m <= 2^12 canonical entries each,
 * weights = the previous pass's 2^jp canonical weights (jp = 0: none pending), J = the rounds of the pass -> rec: the 72 values
 * the device pass would have left (m[a*8 + b] of the folded tables' 2^J sub-blocks, the sub-block sums of Y at 64 + a).  Scalar code;
 * its eight-lane IFMA form runs beside it when the CPU has it (*used_ifma = 1) and must agree. */
int  gkr_selftest_host_tail(const gkr_fr *tables, int m, int jp, const gkr_fr *weights, int J, gkr_fr *rec, int *used_ifma);
/* the host's share of one product pass of the layer sumcheck (h = W X + Y over three tables): `count` <= 16 sumchecks,
 * recs: 72 values each -- the cross sums m[a*8 + b] = sum_i W[aS+i] X[bS+i] of the 2^J <= 8 sub-blocks, then the Y sums
 * at 64 + a; vec_len[t*count + k] = 2 or 3 -> per round t < J (index t*count + k) the coefficients of
 * c2 X^2 + lin X + c0 and the challenge; w[k*8 + b]: the weights eq(r, b) of the fold that follows (canonical).
 * Scalar code; its IFMA-lane form runs beside it when the CPU has it and must agree. */
int  gkr_selftest_host_prod_pass(const gkr_fr *recs, int count, int J, const uint32_t *vec_len, gkr_fr *c2, gkr_fr *lin,
                                 gkr_fr *c0, gkr_fr *r, gkr_fr *w, int *used_ifma);
/* sum_i a_i b_i through the unreduced 544-bit dot-product accumulator of the fused layer kernel */
int  gkr_selftest_dot(const gkr_fr *a, const gkr_fr *b, size_t n, gkr_fr *out);
/* the pass schedule of a 2^n-point plain sumcheck (host logic): rounds covered by each pass; mfma = 1 the matrix-core
 * fold's (up to 5 rounds per pass), 0 the v_mad_u64_u32 fold's (up to 3), 2 the matrix-core fold's with the first fold at
 * two levels where it applies (18 <= n <= 24: 10 | 5 | ..., option first_fold_levels = 2).  *passes = number of passes. */
int  gkr_selftest_pass_schedule(int n, int mfma, uint32_t *rounds, size_t capacity, size_t *passes);
/* The launch plan of gkr_sumcheck_mle_batch_device(n, batch) on the host transcript's multi-round schedule (host logic, from the
 * functions the driver and its launches call; no device work): which kernel reads which table, with how many blocks, on which stream.
 * gkr_selftest_mle_plan: for `hash_threads` hashing threads (the driving one included) and the option table's defaults with
 * option_values[i] laid over option_names[i], i < n_options -- no context, no environment.  gkr_selftest_mle_plan_ctx: for the
 * context's options and thread count.
 * header: GKR_MLE_PLAN_HEADER_WORDS words: 0 jmax, 1 j_first, 2 n_dev (sumchecks hashed on the device), 3 groups, 4 depth, 5 tail_on,
 * 6 two_level, 7 / 8 the two-level first folds that publish flag-in-word records / through a reduce launch (groups - 1 and 1 where
 * the records are in use: the fold launched LAST keeps the reduce, whichever group's it is), 9 hash_threads, 10 .. 42 bound[0 .. 32],
 * 43 .. 74 chunk[0 .. 31] (unused entries 0).
 * rows: GKR_MLE_PLAN_ROW_WORDS words per pass, group by group (the device-hashed chain last, as group `groups`), passes in order:
 * 0 group, 1 pass, 2 kind (GKR_MLE_KIND_*), 3 m_src (log2 entries of the tables read), 4 jin (variables bound; the fine sums: the
 * rounds whose weights they take), 5 jout (rounds the sums cover), 6 blocks per table (the fine sums: partials per table they total),
 * 7 entries per block, 8 publisher (GKR_MLE_PUB_*; a two-level fold: FLAGGED where header word 7 counts it), 9 stream
 * (GKR_MLE_STREAM_*), 10 the fold's digit matrices (GKR_MLE_PLAN_*; with the fine sums: theirs and the two-level fold's), 11 the fold
 * leaves its tables to the host tail, 12 planes its source is the sum of, 13 / 14 the group's first sumcheck / its sumchecks, 15 zero.
 * What depends on the order in which hashes land (which fold is launched last, event waits between streams) is not reported.
 * *n_rows = rows of the plan; rows beyond row_capacity are not written (rows may be NULL with row_capacity 0).
 * GKR_ERR_INVALID: NULL header or n_rows, n outside 2 .. GKR_MAX_MLE_N, batch outside 1 .. 65535, batch * 2^n above 2^30,
 * hash_threads outside 1 .. 256, an unknown option name; the context's form also: a context on the device transcript or with option
 * mle_per_round (another driver runs those). */
enum {
    GKR_MLE_KIND_SMALL0 = 0, GKR_MLE_KIND_SUB_SUMS = 1 /* + form: 1 k_mle_sub_sums, 2 stream<8,1>, 3 stream<16,2>, 4 roll */,
    GKR_MLE_KIND_ROLL_PUB = 5, GKR_MLE_KIND_FINE_SUMS = 6, GKR_MLE_KIND_FOLD2 = 7, GKR_MLE_KIND_FOLD_SMALL = 8, GKR_MLE_KIND_FOLD_MFMA = 9,
    GKR_MLE_KIND_FOLD_VALU = 10, GKR_MLE_KIND_HOST_FOLD = 11
};
enum { GKR_MLE_PUB_SELF = 0, GKR_MLE_PUB_FUSED = 1, GKR_MLE_PUB_REDUCE = 2, GKR_MLE_PUB_FLAGGED = 3, GKR_MLE_PUB_HOST = 4 };
enum { GKR_MLE_STREAM_MAIN = 0, GKR_MLE_STREAM_LATE = 1, GKR_MLE_STREAM_SIDE = 2, GKR_MLE_STREAM_CHAIN = 3, GKR_MLE_STREAM_HOST = 4 };
enum { GKR_MLE_PLAN_NONE = 0, GKR_MLE_PLAN_OWN_STREAM = 1, GKR_MLE_PLAN_SIDE_STREAM = 2 };
#define GKR_MLE_PLAN_HEADER_WORDS 80
#define GKR_MLE_PLAN_ROW_WORDS 16
int  gkr_selftest_mle_plan(int n, int batch, int hash_threads, const char *const *option_names, const long long *option_values,
                           size_t n_options, uint32_t *header, uint32_t *rows, size_t row_capacity, size_t *n_rows);
int  gkr_selftest_mle_plan_ctx(gkr_ctx *ctx, int n, int batch, uint32_t *header, uint32_t *rows, size_t row_capacity, size_t *n_rows);
/* the launch geometry of gkr_sumcheck_product_batch_device (host logic, the process-default options; the degree does not enter):
 * nblk[j] = blocks per sumcheck of round j's pass (j = 0 .. n-1; round 0 the value pass, later rounds the fold-and-value pass),
 * chunk[j] = the entries a block walks, as the kernels derive it: ((items + nblk - 1) / nblk + 255) & ~255 with items = 2^(n-1-j).
 * GKR_ERR_INVALID: NULL pointer, batch outside 1 .. 65535, n outside 2 .. GKR_MAX_MLE_N, batch * 2^n above 2^30. */
int  gkr_selftest_product_geometry(int n, int batch, uint32_t *nblk, uint32_t *chunk);
/* the launch geometry of the dense layer forms (host logic, from the functions the launches call) at round `round` (0-based) of a
 * layer over 2^k_next values cut into 2^log_p trailing-variable shards, N = 2^(2 k_next - log_p) cells per table, h = N >> (round + 1):
 * out[0 .. 3] = column blocks, row chunks, rows per chunk and partials of the device transcript's fused b-phase round (log_p = 0 and
 * round < k_next; otherwise 0); out[4] = the blocks of the session's (and the unfused device transcript's) round kernel over h pairs,
 * bit 31 set in the c-phase (round >= k_next); out[5] = the blocks of the table fold over h pairs; out[6] = the scan blocks of the
 * predicate build, ceil(2 N / 2048); out[7] = the blocks of its sum kernel over 2 N cells.
 * GKR_ERR_INVALID: NULL pointer, k_next outside 1 .. GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT, log_p outside 0 .. k_next, round outside
 * 0 .. 2 k_next - log_p - 1. */
int  gkr_selftest_layer_dense_geometry(int k_next, int log_p, int round, uint32_t out[8]);
/* q(t) = W(b + t (c - b)) (reduce_multiple_polynomial, poly.rs:469-500) as gkr_prove computes it on the host: W = 2^k
 * evaluations; out = k + 1 slots right-aligned, highest degree first; *out_len = 1 + largest monomial degree of W */
int  gkr_selftest_line_restriction(int k, const gkr_fr *W, const gkr_fr *b, const gkr_fr *c, gkr_fr *out, uint32_t *out_len);
/* one item (<= 32 gates) of a gate-list segment and its combine step, on the host twins of the device code
 * (csrc/gate_seg.h): rows = 0: out0 = e_hi * sum_i e_lo[i] (is_mult[i] ? t[i] : 1), out1 = e_hi * sum_{!is_mult} e_lo[i] t[i]
 * (the U, V sums of sumcheck.rs:50-63); rows = 1: out0 over the add gates, out1 over the mult gates (:97-124) */
int  gkr_selftest_seg_item(const gkr_fr *e_lo, const gkr_fr *t, const uint8_t *is_mult, size_t n, const gkr_fr *e_hi, int rows,
                           gkr_fr *out0, gkr_fr *out1);
/* lo + r (hi - lo) through the fixed-multiplier table the fold kernels use */
int  gkr_selftest_fold(const gkr_fr *lo, const gkr_fr *hi, const gkr_fr *r, gkr_fr *out);

/* ---- the device arithmetic ON THE DEVICE, for unit tests (csrc/kernels_selftest.hip) ------------------------------- */
/* Each call copies the inputs to the device, runs one small kernel that calls the kernels' own inline functions, and
 * copies the results back.  Inputs outside a primitive's stated bound: GKR_ERR_INVALID (nothing runs).  Threads are
 * grouped in waves of 64 (element i in wave i / 64); an operand the kernels hold wave-uniform is given once per wave. */
enum {
    /* gkr_devtest_field: canonical a, b (n each); r: one canonical challenge per wave (the fixed-multiplier ops only,
     * the table built on the device by make_fixed_mul).  out: n values; the paired ops write their second results at
     * out[n + i] (MUL_FIXED2: b r; FOLD_FIXED2: b + r (a - b)) */
    GKR_DEVTEST_FR_ADD = 0, GKR_DEVTEST_FR_SUB, GKR_DEVTEST_MONT_MUL, GKR_DEVTEST_FR_MUL, GKR_DEVTEST_TO_MONT,
    GKR_DEVTEST_FROM_MONT, GKR_DEVTEST_MUL_FIXED, GKR_DEVTEST_MUL_FIXED2, GKR_DEVTEST_FOLD_FIXED, GKR_DEVTEST_FOLD_FIXED2
};
enum {
    /* gkr_devtest_lazy: one dot product of `len` terms per row (a[row * len + t], canonical), reduced by `red`.
     * b: per row (b[row * len + t]) for MAC_V, MAC_SEL (term t to the first accumulator iff (row + t) % 3 != 0, else the
     * second), MAC_V_HI (+ a_t 2^256 where row + t is odd); per wave (b[wave * len + t]) for MAC_S, the MACk_S forms
     * (chain c: sum_t a_t b_{(t + c) % len}) and WEIGHTED_SUM_4 / _8 (len = 4 / 8).  ACC_SUM: sum_t a_t through the 288-bit
     * accumulator and acc_reduce (no b, `red` unused).  out[row * 4 + c]: accumulator / chain c (unused slots 0). */
    GKR_DEVTEST_LAZY_MAC_S = 0, GKR_DEVTEST_LAZY_MAC_V, GKR_DEVTEST_LAZY_MAC_SEL, GKR_DEVTEST_LAZY_MAC_V_HI,
    GKR_DEVTEST_LAZY_MAC2_S, GKR_DEVTEST_LAZY_MAC3_S, GKR_DEVTEST_LAZY_MAC4_S, GKR_DEVTEST_WEIGHTED_SUM_4,
    GKR_DEVTEST_WEIGHTED_SUM_8, GKR_DEVTEST_ACC_SUM
};
enum {
    /* the reduction of gkr_devtest_lazy: lazy_reduce (canonical), lazy_reduce_k8 (<= 8 products, canonical),
     * lazy_reduce_partial32 (<= 32 terms; some representative below 2^256) */
    GKR_DEVTEST_RED_FULL = 0, GKR_DEVTEST_RED_K8, GKR_DEVTEST_RED_PARTIAL32
};
enum {
    /* gkr_devtest_reduce: raw little-endian 32-bit limbs, n elements; limbs in -> limbs out per element:
     * MF_REDUCE_274 9 (< 2^274) -> 8; CROSS_REDUCE 17 (< 2^519) -> 8; LAZY_REDUCE 17 -> 8; LAZY_REDUCE_K8 17 (< 8 p^2) -> 8;
     * LAZY_REDUCE_PARTIAL32 17 (< 32 p 2^256) -> 8; LAZY_ADD_HI 26 (acc 17, x 8 below p, on 1) -> 17 (acc + on x 2^256);
     * ACC_ADD_FR9 17 (acc 9, x 8 below p) -> 9; ACC_REDUCE9 9 -> 8; ADD256 16 (a, b) -> 8; SUB256 16 (a, b) -> 9 (a - b,
     * borrow mask); COND_SUB_MOD 8 (< 2p) -> 8 */
    GKR_DEVTEST_MF_REDUCE_274 = 0, GKR_DEVTEST_CROSS_REDUCE, GKR_DEVTEST_LAZY_REDUCE, GKR_DEVTEST_LAZY_REDUCE_K8,
    GKR_DEVTEST_LAZY_REDUCE_PARTIAL32, GKR_DEVTEST_LAZY_ADD_HI, GKR_DEVTEST_ACC_ADD_FR9, GKR_DEVTEST_ACC_REDUCE9,
    GKR_DEVTEST_ADD256, GKR_DEVTEST_SUB256, GKR_DEVTEST_COND_SUB_MOD
};
enum {
    /* gkr_devtest_lanes: the MiMC7 lane code (mimc_lanes.h), eight lanes per element and eight elements per wave as
     * k_mle_pass_hash_lanes lays them out; n elements (the last wave may be ragged).  MONT_MUL x y / 2^256 (operands < 3p;
     * the lanes' representative, < 2.7p); ADD3 x + y + z (< 2^256); COND_SUB_P / _2P (any x); RESOLVE x + y 2^32 with
     * limb j of y the carry lane j holds (< 2^256); PERMUTATION hash(x, key y), both below p, Montgomery form (< 2p);
     * MULTI_HASHk multi_hash of the first k of x, y, z with key 0 (canonical in and out); GROUP_SUM: x holds 8 n
     * canonical values, one per lane, out the modular sum of each element's eight in all eight lanes' slots */
    GKR_DEVTEST_LANES_MONT_MUL = 0, GKR_DEVTEST_LANES_ADD3, GKR_DEVTEST_LANES_COND_SUB_P, GKR_DEVTEST_LANES_COND_SUB_2P,
    GKR_DEVTEST_LANES_RESOLVE, GKR_DEVTEST_LANES_PERMUTATION, GKR_DEVTEST_LANES_MULTI_HASH1, GKR_DEVTEST_LANES_MULTI_HASH2,
    GKR_DEVTEST_LANES_MULTI_HASH3, GKR_DEVTEST_LANES_GROUP_SUM
};
int  gkr_devtest_field(gkr_ctx *ctx, int op, const gkr_fr *a, const gkr_fr *b, const gkr_fr *r, size_t n, gkr_fr *out);
int  gkr_devtest_lazy(gkr_ctx *ctx, int op, int red, const gkr_fr *a, const gkr_fr *b, size_t rows, size_t len, gkr_fr *out);
int  gkr_devtest_reduce(gkr_ctx *ctx, int op, const uint32_t *limbs, size_t n, uint32_t *out);
int  gkr_devtest_lanes(gkr_ctx *ctx, int op, const gkr_fr *x, const gkr_fr *y, const gkr_fr *z, size_t n, gkr_fr *out);
/* The gate lists of one layer (2^k_i gates over 2^k_next values, host arrays) as the layer sumcheck builds them under the
 * context's options, and what the build decided: *form = 0 the bucket kernels, 1 the item plan of wide layers, 2 segments.
 * counts: 2 x 8 words, left-operand half then right-operand half.  Form 1: the half's plan header words 0 .. 5 (items, groups,
 * buckets of 2 .. 64 items, buckets of more, groups of two and more steps, chunks of the long buckets).  Form 2: shift (log2
 * gates per run), runs, m (sort blocks per run), items of the half.  Unused words are 0.  Nothing is proven.
 * GKR_ERR_INVALID: NULL pointer, k_i outside 0 .. GKR_MAX_K_I, k_next outside 1 .. GKR_MAX_K_NEXT, a gate out of range. */
int  gkr_devtest_gate_plan(gkr_ctx *ctx, int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left, const uint32_t *right,
                           uint32_t *form, uint32_t *counts);
/* One shard's dense predicate tables as gkr_layer_session_open builds them under the context's options: shard `shard` of 2^log_p
 * keeps the gates whose right operand has low bits `shard`; out_A, out_M: 2^(2 k_next - log_p) canonical values each, cell
 * (l << (k_next - log_p)) | (r >> log_p).  log_p = 0: gkr_predicate_tables.  GKR_ERR_INVALID: NULL pointer, k_next above
 * GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT, log_p > k_next, shard >= 2^log_p, a gate out of range. */
int  gkr_devtest_predicates(gkr_ctx *ctx, int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left, const uint32_t *right,
                            const gkr_fr *z, uint32_t log_p, uint32_t shard, gkr_fr *out_A, gkr_fr *out_M);

/* ---- plain multilinear sumcheck: prove_sumcheck(g, v), sumcheck.rs:158-161 --- */
/* table: 2^n canonical evaluations on the host.  out_coeffs: n rows x 2 slots;
 * out_len[j] in {1,2}; out_r: n challenges.  n >= 2. */
int  gkr_sumcheck_mle(gkr_ctx *ctx, const gkr_fr *table, int n, gkr_fr *out_coeffs, uint32_t *out_len,
                      gkr_fr *out_r);

/* `batch` independent sumchecks whose tables already sit in device memory,
 * contiguous (table b starts at d_tables + b * 2^n elements).  Inputs are not
 * modified.  Outputs are host arrays of batch x n rows.  Kernel forms behind it, the same bytes whichever is chosen: option
 * first_fold_levels (ten variables bound in the first fold's one read, 18 <= n <= 24) and option pass0_stream (pass 0 of a
 * streaming launch as a pipelined read: 1 a block per partial sum, 2 a wave per partial with its loads kept in flight, 3 the
 * same through one rolling load buffer on the large launches, the default); option
 * fold2_tiles (64-entry tiles a block of that first fold takes: 0 one, k at most k); option stream_publish (how the streaming
 * passes of a batch in several groups hand their sums to the host: 1 through a reduce launch behind every pass, 2 -- the default --
 * as flag-in-word records the blocks store to pinned memory themselves and the hashing threads total, where that applies). */
int  gkr_sumcheck_mle_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int batch,
                                   gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r);

/* ---- sumcheck over a product of resident multilinear tables: prove_sumcheck(g, v) with
 * g = mult_poly(get_multi_ext(T_0), .., get_multi_ext(T_{degree-1})) (sumcheck.rs:158-214, poly.rs:349-386) ----
 * Inner products sum_x A(x) B(x), zero-checks sum_x eq(x) A(x) B(x), a GKR layer written densely.  degree = 1 is the plain
 * sumcheck's transcript.  `batch` independent sumchecks over `degree` tables of 2^n canonical values each (variable 1 = most
 * significant index bit), resident in device memory: factor f of sumcheck b starts at d_tables + (b * degree + f) * 2^n
 * elements.  Inputs are not modified; the folded halves live in context workspace of batch * degree * 2^(n-1) elements.
 *   out_coeffs  batch x n rows of degree + 1 slots, right-aligned, highest degree first, unused slots zero
 *   out_len     batch x n values in 1 .. degree + 1.  Rounds 1 .. n-1: leading zero coefficients dropped, one kept at least
 *               (add_poly merges by exponent, poly.rs:324-327); round n: 1 + the number of factors that depend on x_n (no
 *               merge, sumcheck.rs:206-207)
 *   out_r       batch x n challenges, r_j = multi_hash(round vector j, key 0)
 *   out_evals   batch x degree values T_f~(r_1 .. r_n) -- the one entry each factor has left after the last fold, which the
 *               prover has for free -- or NULL.  A verifier's last check is g_n(r_n) = prod_f T_f~(r): the verifier below
 *               (gkr_sumcheck_product_verify_batch_device) evaluates the resident tables itself and returns the values.
 * A factor that is the zero table makes g the empty term list, on which the reference panics (partial_eval indexes f[0],
 * poly.rs:236); as the library's OWN choice such a sumcheck returns every round vector as [0] with length 1.
 * The challenges are hashed on the device in both transcript modes (one launch per round, no host round trip): the result
 * does not depend on the context's transcript mode.
 * GKR_ERR_INVALID before a device or the context is touched (plain returns; the context's last error is left as it was): NULL
 * ctx or pointer (out_evals excepted), batch outside 1 .. 65535, n outside 2 .. GKR_MAX_MLE_N, degree outside
 * 1 .. GKR_PRODUCT_MAX_DEGREE, batch * degree * 2^n above 2^30 values. */
#define GKR_PRODUCT_MAX_DEGREE 3
int  gkr_sumcheck_product_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int degree, int batch,
                                       gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals);

/* `degree` tables of 2^n values in host memory, one after the other: upload + the call above with batch 1.
 * GKR_ERR_NON_CANONICAL for an entry >= r. */
int  gkr_sumcheck_product(gkr_ctx *ctx, const gkr_fr *tables, int n, int degree,
                          gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals);

/* ---- sumcheck over a SUM OF PRODUCTS of resident multilinear tables: prove_sumcheck(g, v) with
 * g = add_poly over k of c_k * mult_poly(get_multi_ext(T_t(k,0)), ..) (sumcheck.rs:158-214, poly.rs:293-386) ----
 *   g(x) = sum_{k < n_terms} c_k * prod_{j < d_k} T_{t(k,j)}(x)   over n_tables tables of 2^n canonical values each.
 * The R1CS zero-check sum_x eq(x) (A(x) B(x) - C(x)): 4 tables, terms {3, {0, 1, 2}} and {2, {0, 3}} with coefficients 1, r - 1.
 * A GKR layer written densely, add (W_b + W_c) + mult W_b W_c; a random linear combination of inner-product claims.  ONE
 * transcript for all terms; a table that stands in several terms (or several times in one: squares, cubes) is stored once and
 * folded once per round.  Table m of sumcheck b starts at d_tables + (b * n_tables + m) * 2^n elements; the term structure and
 * the coefficients (term_coeffs: n_terms canonical elements, NULL = all 1; zero is allowed) are shared by the batch.  Inputs are
 * not modified; the folded halves live in context workspace of batch * n_tables * 2^(n-1) elements, under slot names of this
 * path's own (a plain or product call on the same context is unaffected).  D = the largest term degree of the call.
 *   out_coeffs  batch x n rows of D + 1 slots, right-aligned, highest degree first, unused slots zero: the sum of the terms'
 *               round polynomials of the current (folded) tables
 *   out_len     batch x n values in 1 .. D + 1.  EVERY round, the last included: leading zero coefficients dropped, one kept at
 *               least.  Rounds 1 .. n-1 this is the reference exactly (add_poly merges by exponent and drops zero sums).  In
 *               round n the reference's length is 1 + deg_{x_n} g as a polynomial; the two differ only where a non-zero
 *               coefficient polynomial of g vanishes at the hashed point (r_1 .. r_{n-1}): probability at most 3 (n - 1) / r.
 *   out_r       batch x n challenges, r_j = multi_hash(used slots of round j, key 0)
 *   out_evals   batch x n_tables values T_m~(r_1 .. r_n), or NULL.  A verifier's last check is
 *               g_n(r_n) = sum_k c_k prod_j out_evals[t(k,j)].
 * g identically zero (terms that cancel, a zero factor in every term) is the empty term list, on which the reference panics;
 * as the library's OWN choice every round vector is then [0] with length 1, as for the product path's zero factor.  With one
 * term of coefficient 1 over distinct tables the transcript is gkr_sumcheck_product_batch_device's byte for byte, wherever that
 * path's structural last-round rule and the value rule above agree (always, up to the probability above).
 * Hashed on the device in both transcript modes; the result does not depend on the context's transcript mode.
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): NULL ctx or pointer (term_coeffs and out_evals
 * excepted), batch outside 1 .. 65535, n outside 2 .. GKR_MAX_MLE_N, n_tables outside 1 .. GKR_SOP_MAX_TABLES, n_terms outside
 * 1 .. GKR_SOP_MAX_TERMS, a term degree outside 1 .. 3, a table index >= n_tables, a table that no term references,
 * batch * n_tables * 2^n above 2^30 values.  GKR_ERR_NON_CANONICAL (through the context) for a coefficient >= r. */
#define GKR_SOP_MAX_TABLES 8
#define GKR_SOP_MAX_TERMS  8
typedef struct { uint8_t degree; uint8_t table[3]; } gkr_sop_term;   /* degree 1..3, table[j] < n_tables for j < degree */
int  gkr_sumcheck_sop_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int n_tables, const gkr_sop_term *terms,
                                   const gkr_fr *term_coeffs /* n_terms, NULL = all 1 */, int n_terms, int batch,
                                   gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals /* batch x n_tables or NULL */);

/* `n_tables` tables of 2^n values in host memory, one after the other: upload + the call above with batch 1.
 * GKR_ERR_NON_CANONICAL also for a table entry >= r. */
int  gkr_sumcheck_sop(gkr_ctx *ctx, const gkr_fr *tables /* host, n_tables x 2^n */, int n, int n_tables, const gkr_sop_term *terms,
                      const gkr_fr *term_coeffs, int n_terms,
                      gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals);

/* ZERO-CHECK: `batch` sumchecks of  sum_x eq(z, x) g(x),  g = sum_k c_k prod_{f < d_k} T_{t(k,f)}  with term degrees d_k in
 * {1, 2} -- the R1CS zero-check eq (A B - C), a dense GKR layer, every "this relation holds on the whole cube" claim -- without
 * eq(z, .) as a table: nothing of 2^n entries is built, uploaded, folded or multiplied in.  Tables, terms and coefficients as
 * gkr_sumcheck_sop_batch_device takes them; z: batch x n canonical elements in host memory, each sumcheck its own point,
 * variable 1 = the most significant index bit.  Entries 0 and 1 are ordinary points (nothing divides by z_j or 1 - z_j).
 * d = the largest term degree, D = d + 1.  Round j = 1 .. n, on the current (folded) tables of 2^(n-j+1) entries, lo_f = T_f[i],
 * hi_f = T_f[i + 2^(n-j)], i < 2^(n-j):
 *     w_j(i) = eq((z_{j+1}, .., z_n), i)                              z_{j+1} against i's top bit; w_n = 1
 *     h_j(X) = sum_i w_j(i) sum_k c_k prod_f (lo_f + X (hi_f - lo_f))                                  degree d
 *     s_j    = prod_{l < j} (z_l r_l + (1 - z_l)(1 - r_l)),  s_1 = 1
 *     g_j(X) = s_j ((1 - z_j) + (2 z_j - 1) X) h_j(X)                                                   degree D
 *   out_coeffs  batch x n rows of D + 1 slots: the coefficients of g_j, right-aligned, highest degree first, unused slots zero
 *   out_len     batch x n values in 1 .. D + 1; EVERY round: leading zero coefficients dropped, one kept at least
 *   out_r       batch x n challenges, r_j = multi_hash(used slots of round j, key 0); every table folds once with r_j
 *   out_evals   batch x n_tables values T_m~(r_1 .. r_n), or NULL
 *   out_eq      batch values s_{n+1} = eq(z, r), or NULL
 * A verifier's last check is  g_n(r_n) = out_eq * sum_k c_k prod_f out_evals[t(k,f)];  a zero-check's claim is zero.
 * g_j is the polynomial gkr_sumcheck_sop_batch_device forms from the n_tables + 1 tables {eq(z, .), T_0 ..} with every term
 * prefixed by table 0, coefficients are canonical and the length rule goes by value: the two transcripts (coefficients, lengths,
 * challenges, the tables' values; out_eq = that call's value of table 0) are EQUAL BYTE FOR BYTE, for every input -- g
 * identically zero (every vector [0]) and boolean z included.  gkr_sumcheck_sop_verify_batch_device on those tables (table 0
 * from gkr_eq_table_device) therefore verifies this call's transcripts.
 * Inputs are not modified; the folded halves (batch * n_tables * 2^(n-1) elements) and the weights of the free variables
 * (2^(n-8) + 511 elements per sumcheck) live in context workspace under slot names of this path's own: a plain, product or SOP
 * call on the same context is unaffected.
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): everything gkr_sumcheck_sop_batch_device refuses
 * (the same table and batch limits), NULL z, and A TERM OF DEGREE 3: inner degree 3 makes g_j a quartic, which needs rows of five
 * slots and a fifth hash slot.  GKR_ERR_NON_CANONICAL (through the context) for a coefficient or a z entry >= r. */
int  gkr_sumcheck_zerocheck_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int n_tables, const gkr_sop_term *terms,
                                         const gkr_fr *term_coeffs /* n_terms, NULL = all 1 */, int n_terms, int batch,
                                         const gkr_fr *z /* host, batch x n */,
                                         gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r,
                                         gkr_fr *out_evals /* batch x n_tables or NULL */, gkr_fr *out_eq /* batch or NULL */);

/* `n_tables` tables of 2^n values in host memory, one after the other, and one point z of n elements: upload + the call above
 * with batch 1.  GKR_ERR_NON_CANONICAL also for a table entry >= r. */
int  gkr_sumcheck_zerocheck(gkr_ctx *ctx, const gkr_fr *tables /* host, n_tables x 2^n */, int n, int n_tables, const gkr_sop_term *terms,
                            const gkr_fr *term_coeffs, int n_terms, const gkr_fr *z /* n */,
                            gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals, gkr_fr *out_eq);

/* The tables eq(z_b, .) of `batch` points, built on the device: d_out[b * stride_elements + i] = prod_j (bit_j(i) ? z_j : 1 - z_j),
 * canonical, variable 1 = the most significant index bit of i < 2^n.  z: batch x n canonical elements in host memory.  With
 * stride_elements = n_tables * 2^n the call fills table 0 of every sumcheck's group of an SOP layout in place; elements between
 * the tables are not touched.  GKR_ERR_INVALID (plain returns): NULL pointer, n outside 1 .. GKR_MAX_MLE_N, batch outside
 * 1 .. 65535, stride_elements < 2^n.  GKR_ERR_NON_CANONICAL (through the context) for a z entry >= r. */
int  gkr_eq_table_device(gkr_ctx *ctx, const gkr_fr *z /* host, batch x n */, int n, int batch,
                         void *d_out, size_t stride_elements /* >= 2^n */);

/* Verifier of gkr_sumcheck_product_batch_device's transcripts: the plain sumcheck's verifier (below; the same driver, the same
 * options) for round polynomials of degree up to 3, one read of every factor.
 * d_tables / coeffs / len / r: exactly the arrays and layout of the prover (factor f of sumcheck b at (b * degree + f) * 2^n
 * elements; batch x n rows of degree + 1 right-aligned slots, highest degree first; len in 1 .. degree + 1; batch x n
 * challenges).  claims: batch elements or NULL.
 * accept[batch] required; failed_round / failed_check / out_claims (batch) / out_evals (batch x degree) may be NULL.
 * Per transcript, in this order, the first failure reported (failed_check: the GKR_VERIFY_* values below):
 *   1. GKR_VERIFY_SHAPE           some len[j] outside 1 .. degree + 1; failed_round = the first such j
 *   2. GKR_VERIFY_NON_CANONICAL   a used slot, an r_j or the claim >= r (unused slots are never read); failed_round = the
 *                                 first such row, 0 for the claim
 *   3. for j = 0 .. n-1:  GKR_VERIFY_ROUND_SUM  g_j(0) + g_j(1) (= 2 c_0 + c_1 + .. + c_D over the used slots) != the running
 *      claim;  GKR_VERIFY_CHALLENGE  r_j != multi_hash(used slots of row j, key 0);  the running claim becomes g_j(r_j)
 *   4. GKR_VERIFY_EVALUATION      g_n(r_n) != prod_f T_f~(r_1 .. r_n); failed_round = n
 * claims == NULL: round 0's sum check is skipped.  out_claims[b] = g_1(0) + g_1(1), the sum the transcript proves, and
 * out_evals[b * degree + f] = T_f~(r) as the device computed it, for every transcript that passes checks 1 and 2; zero for the
 * others (their point is not a point).  A caller that also holds the prover's out_evals compares them itself.  Table entries
 * are read as integers modulo r.  The library's zero-factor transcripts (every vector [0]) need no special case.
 * The return value is the status of the CALL, not the verdict.  GKR_ERR_INVALID before a device or the context is touched
 * (plain returns): NULL ctx or required pointer, and every shape the prover refuses (batch outside 1 .. 65535, n outside
 * 2 .. GKR_MAX_MLE_N, degree outside 1 .. GKR_PRODUCT_MAX_DEGREE, batch * degree * 2^n above 2^30 values).  Chunks are counted
 * in sumchecks (the factors of one sumcheck are never split); verdicts depend neither on verify_workspace_mb nor on
 * verify_device_hash_min. */
int gkr_sumcheck_product_verify_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int degree, int batch,
                                             const gkr_fr *claims, const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r,
                                             int *accept, uint32_t *failed_round, uint32_t *failed_check,
                                             gkr_fr *out_claims, gkr_fr *out_evals);

/* `degree` tables in host memory, one after the other: upload + the call above with batch 1.  GKR_ERR_NON_CANONICAL for a
 * table entry >= r, as gkr_sumcheck_product. */
int gkr_sumcheck_product_verify(gkr_ctx *ctx, const gkr_fr *tables, int n, int degree, const gkr_fr *claim,
                                const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r,
                                int *accept, uint32_t *failed_round, uint32_t *failed_check);

/* Verifier of gkr_sumcheck_sop_batch_device's transcripts: the same driver and options as the product verifier above, with the
 * caller's term structure; one read of every table, all n_tables tables of a sumcheck evaluated at its one point (the point's
 * weights are built once per sumcheck).
 * d_tables / terms / term_coeffs / coeffs / len / r: exactly the arrays and layout of the prover (table m of sumcheck b at
 * (b * n_tables + m) * 2^n elements; batch x n rows of D + 1 right-aligned slots, D the largest term degree; len in 1 .. D + 1;
 * batch x n challenges).  claims: batch elements or NULL; a zero-check passes zeros.
 * accept[batch] required; failed_round / failed_check / out_claims (batch) / out_evals (batch x n_tables) may be NULL.
 * The checks and their order are the product verifier's 1 .. 3 (SHAPE, NON_CANONICAL, per round ROUND_SUM / CHALLENGE), then
 *   4. GKR_VERIFY_EVALUATION      g_n(r_n) != sum_k c_k prod_j T_{t(k,j)}~(r_1 .. r_n); failed_round = n
 * out_claims[b] = g_1(0) + g_1(1) and out_evals[b * n_tables + m] = T_m~(r) as the device computed it, for every transcript that
 * passes checks 1 and 2; zero for the others.  The library's all-[0] transcripts of an identically zero g need no special case.
 * A change of a table shows exactly when it moves the sum of the terms: not behind a zero coefficient or cofactor, not in terms
 * that cancel.  The verifier given other terms or coefficients than the prover's checks the transcript against THOSE.
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): NULL ctx or required pointer (term_coeffs, claims and
 * the optional outputs excepted), and every shape the prover refuses (batch outside 1 .. 65535, n outside 2 .. GKR_MAX_MLE_N,
 * n_tables outside 1 .. GKR_SOP_MAX_TABLES, n_terms outside 1 .. GKR_SOP_MAX_TERMS, a term degree outside 1 .. 3, a table index
 * >= n_tables, a table that no term references, batch * n_tables * 2^n above 2^30 values).  GKR_ERR_NON_CANONICAL (through the
 * context) for a coefficient >= r.  Chunks are counted in sumchecks (the tables of one sumcheck are never split); verdicts depend
 * neither on verify_workspace_mb nor on verify_device_hash_min nor on mle_eval_mfma_min_n. */
int gkr_sumcheck_sop_verify_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int n_tables, const gkr_sop_term *terms,
                                         const gkr_fr *term_coeffs /* n_terms, NULL = all 1 */, int n_terms, int batch,
                                         const gkr_fr *claims /* batch or NULL */, const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r,
                                         int *accept, uint32_t *failed_round, uint32_t *failed_check,
                                         gkr_fr *out_claims /* batch or NULL */, gkr_fr *out_evals /* batch x n_tables or NULL */);

/* `n_tables` tables in host memory, one after the other: upload + the call above with batch 1.  GKR_ERR_NON_CANONICAL also for a
 * table entry >= r, as gkr_sumcheck_sop. */
int gkr_sumcheck_sop_verify(gkr_ctx *ctx, const gkr_fr *tables /* host, n_tables x 2^n */, int n, int n_tables, const gkr_sop_term *terms,
                            const gkr_fr *term_coeffs, int n_terms, const gkr_fr *claim, const gkr_fr *coeffs, const uint32_t *len,
                            const gkr_fr *r, int *accept, uint32_t *failed_round, uint32_t *failed_check);

/* ---- the plain sumcheck's verifier: verify_sumcheck, python/sumcheck.py:55-70, and the relation behind it -------------
 * A transcript of prove_sumcheck proves "sum of the table = claim" only together with g_n(r_n) = T~(r_1 .. r_n), the table's
 * multilinear extension at the challenges: one read of the table (32 * 2^n bytes, where the prover's default schedule moves
 * 66 * 2^n), with every challenge known up front. */

/* W~(point) for `batch` tables resident in device memory (layout of gkr_sumcheck_mle_batch_device: table b at
 * d_tables + b * 2^n elements, variable 1 = most significant index bit).  points: batch x n canonical elements
 * (host), each table its own point; out: batch elements (host).  1 <= n <= 30, batch >= 1.  Tables are not modified. */
int gkr_mle_eval_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int batch, const gkr_fr *points, gkr_fr *out);

/* Verifier of gkr_sumcheck_mle_batch_device's transcripts (python/sumcheck.py:55-70 plus the final evaluation).
 * coeffs / len / r: exactly the arrays the prover wrote (batch x n rows of 2 right-aligned slots, len in {1,2}, batch x n
 * challenges).  claims: batch elements or NULL.
 * accept[batch] required; failed_round / failed_check / out_claims may be NULL.
 * Per transcript, in this order, the first failure reported (failed_check: the GKR_VERIFY_* values below):
 *   1. GKR_VERIFY_SHAPE           some len[j] outside 1..2; failed_round = the first such j
 *   2. GKR_VERIFY_NON_CANONICAL   a used slot, an r_j or the claim >= r (unused slots are never read); failed_round = the
 *                                 first such row, 0 for the claim
 *   3. for j = 0 .. n-1:  GKR_VERIFY_ROUND_SUM  g_j(0) + g_j(1) != the running claim;  GKR_VERIFY_CHALLENGE  r_j !=
 *      multi_hash(used slots of row j, key 0);  the running claim becomes g_j(r_j)
 *   4. GKR_VERIFY_EVALUATION      g_n(r_n) != T~(r_1 .. r_n); failed_round = n
 * claims == NULL: round 0's sum check is skipped.  out_claims[b] = g_1(0) + g_1(1), the sum the transcript proves, for every
 * transcript that passes checks 1 and 2, zero for the others.
 * The return value is the status of the CALL, not the verdict: NULL ctx / required pointer, batch < 1, n outside 2..30 are
 * GKR_ERR_INVALID before a device is touched (gkr_mle_eval_batch_device: n outside 1..30; a point's coordinate >= r is
 * GKR_ERR_NON_CANONICAL).  Table entries are read as integers modulo r.  Processed in chunks of verify_workspace_mb of device
 * workspace; a chunk of verify_device_hash_min round vectors and more hashes them on the device; verdicts depend on neither. */
int gkr_sumcheck_mle_verify_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int batch, const gkr_fr *claims,
                                         const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r,
                                         int *accept, uint32_t *failed_round, uint32_t *failed_check, gkr_fr *out_claims);

/* one table in host memory: upload + the call above with batch 1 */
int gkr_sumcheck_mle_verify(gkr_ctx *ctx, const gkr_fr *table, int n, const gkr_fr *claim, const gkr_fr *coeffs,
                            const uint32_t *len, const gkr_fr *r, int *accept, uint32_t *failed_round, uint32_t *failed_check);

/* ---- GRAND PRODUCT: P = prod_i V[i] over a resident table, proven as GKR on the binary tree of multiplication gates ----
 * Permutation and multiset-equality arguments rest on it (lookups with multiplicities and batched memory checks rest on the
 * FRACTIONAL SUM below).  `batch` independent tables of 2^n canonical
 * values, table b at d_tables + b * 2^n elements, variable 1 = the most significant index bit; 3 <= n <= GKR_MAX_MLE_N,
 * batch in 1 .. 65535, batch * 2^n <= 2^30.  The reference has no such argument; the protocol is the library's own:
 *   tree     L_n = V;  L_k[i] = L_{k+1}[i] * L_{k+1}[i + 2^k] mod r  for k = n-1 .. 0, i < 2^k;  P = L_0[0].  One launch per level
 *            (csrc/kernels_grand_product.hip) stores every level, canonical, in context workspace; the halves of a level are the
 *            two contiguous tables the zero-check of the layer below reads in place: nothing is gathered or copied.
 *   head     the proof opens with L_2 (four values) and P = their product.  zeta_1 = multi_hash(L_2[0..3], key 0),
 *            zeta_2 = multi_hash([zeta_1], key 0), z^(2) = (zeta_1, zeta_2), c_2 = L_2~(z^(2)).
 *   layer k  = 2 .. n-1:  gkr_sumcheck_zerocheck_batch_device with n = k on the tables L_{k+1}[0 .. 2^k), L_{k+1}[2^k .. 2^(k+1)),
 *            the one term {2, {0, 1}} with coefficient 1 and the point z^(k); its claimed sum is c_k.  It yields k round vectors
 *            in rows of 4 slots, their lengths, the challenges r^(k), the values (a_k, b_k) and eq(z^(k), r^(k)) -- byte for byte
 *            that call's on that layer.  Then tau_k = multi_hash([a_k, b_k], key 0), c_{k+1} = a_k + tau_k (b_k - a_k),
 *            z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k): tau in front, the new variable being the top index bit.
 *   end      c_n = V~(z^(n)), which the verifier evaluates itself (no commitment to V, as elsewhere in the library).
 * R = n (n - 1) / 2 - 1 rounds in all, layer k's rows from row k (k - 1) / 2 - 1 on.  Every message is hashed on its own.
 *   out_products  batch values P                                  out_head    batch x 4 values L_2
 *   out_coeffs    batch x R rows of 4 slots, layers k = 2 .. n-1   out_len     batch x R values in 1 .. 4
 *   out_r         batch x R challenges                            out_evals   batch x (n - 2) x 2 values (a_k, b_k), or NULL
 *   out_point     batch x n coordinates z^(n), or NULL            out_claim   batch values c_n, or NULL
 * tau, z and c are formed on the host between the layers.  A table with a zero entry has P = 0 and zero levels from some k
 * down; a zero-check whose g vanishes identically returns every vector as [0] with length 1 (the zero-check's own rule).
 * Inputs are not modified.  The tree (batch * (2^n - 1) elements) lives in context workspace under slot names of this path's
 * own; the layers run through the zero-check's driver and share ITS workspace: a zero-check, SOP or product call on the same
 * context is unaffected.  Hashed on the device by the zero-check's round kernel; the result does not depend on the transcript mode.
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): NULL ctx or pointer (the three optional outputs
 * excepted), batch outside 1 .. 65535, n outside 3 .. GKR_MAX_MLE_N, batch * 2^n above 2^30 values. */
int  gkr_grand_product_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int batch, gkr_fr *out_products, gkr_fr *out_head,
                                    gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals /* or NULL */,
                                    gkr_fr *out_point /* or NULL */, gkr_fr *out_claim /* or NULL */);

/* one table of 2^n values in host memory: upload + the call above with batch 1.  GKR_ERR_NON_CANONICAL (through the context)
 * for a table entry >= r. */
int  gkr_grand_product(gkr_ctx *ctx, const gkr_fr *table, int n, gkr_fr *out_product, gkr_fr *out_head, gkr_fr *out_coeffs,
                       uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals, gkr_fr *out_point, gkr_fr *out_claim);

/* Verifier of gkr_grand_product_batch_device's proofs against the resident tables.  head / coeffs / len / r / evals: exactly the
 * arrays and layout of the prover (evals is required here); products: batch claimed values of P, or NULL (the head's own product
 * is then what the proof proves; out_products returns it).  The round relations of every layer run on host threads
 * (csrc/verify_rounds.h, csrc/grand_product_rounds.h), the round vectors' hashes where the sumcheck verifiers' run (on the
 * device from verify_device_hash_min round vectors on, else on the host threads; zeta and tau always on the host), and V is
 * read ONCE on the device, at z^(n) (gkr_mle_eval_batch_device's kernels).
 * accept[batch] required; failed_layer / failed_round / failed_check / out_products (batch each) may be NULL.
 * Per proof, in this order, the first failure reported (failed_check, at failed_layer, failed_round):
 *   1. GKR_VERIFY_SHAPE           some len outside 1 .. 4; at (k, j) of the first such row
 *   2. GKR_VERIFY_NON_CANONICAL   an element >= r (unused slots are never read): a head entry or the claimed product at (0, 0);
 *                                 else the first layer k with such an element: a used slot or a challenge of row j at (k, j),
 *                                 else a_k or b_k at (k, k)
 *   3. GKR_VERIFY_PRODUCT         with products: the claim != head[0] head[1] head[2] head[3]; at (0, 0)
 *   4. for k = 2 .. n-1, with the running claim c_k:  for j = 0 .. k-1  GKR_VERIFY_ROUND_SUM  g_j(0) + g_j(1) != the running
 *      claim, GKR_VERIFY_CHALLENGE  r_j != multi_hash(used slots of row j, key 0), at (k, j), in the order of the sumcheck
 *      verifiers (the challenges of the rounds before the first failed sum first);  then  GKR_VERIFY_FINAL_CLAIM
 *      g_k(r_k) != eq(z^(k), r^(k)) a_k b_k  at (k, k)
 *   5. GKR_VERIFY_EVALUATION      c_n != V~(z^(n)); at (n, n)
 * An accepted proof reports (0, 0, 0).  out_products[b]: the head's product for every proof that passes checks 1 and 2, zero
 * for the others.  Table entries are read as integers modulo r.  The return value is the status of the CALL, not the verdict;
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): NULL ctx or required pointer and every shape the
 * prover refuses.  Verdicts depend neither on verify_workspace_mb nor on verify_device_hash_min. */
int  gkr_grand_product_verify_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int batch, const gkr_fr *products /* or NULL */,
                                           const gkr_fr *head, const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r,
                                           const gkr_fr *evals, int *accept, uint32_t *failed_layer, uint32_t *failed_round,
                                           uint32_t *failed_check, gkr_fr *out_products /* or NULL */);

/* one table in host memory: upload + the call above with batch 1.  GKR_ERR_NON_CANONICAL for a table entry >= r. */
int  gkr_grand_product_verify(gkr_ctx *ctx, const gkr_fr *table, int n, const gkr_fr *product /* or NULL */, const gkr_fr *head,
                              const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r, const gkr_fr *evals, int *accept,
                              uint32_t *failed_layer, uint32_t *failed_round, uint32_t *failed_check);

/* the launch geometry of the tree (host logic, from the function the launches call): one launch per level k = n-1 .. 0,
 * blocks[k] = its blocks of 256 threads per table, ceil(2^k / 256), a thread per product (k = 0 .. n-1: n words).
 * GKR_ERR_INVALID: NULL pointer, n outside 3 .. GKR_MAX_MLE_N. */
int  gkr_selftest_grand_product_geometry(int n, uint32_t *blocks);
/* The tree alone, into the CALLER's device buffer instead of the context's workspace: d_layers takes batch * (2^n - 1) elements,
 * level k of table b at batch * (2^k - 1) + b * 2^k.  The argument checks of gkr_grand_product_batch_device. */
int  gkr_devtest_grand_product_tree(gkr_ctx *ctx, const void *d_tables, int n, int batch, void *d_layers);
/* The proofs per chunk gkr_grand_product_verify_batch_device works through for (n, batch) under the context's options
 * (verify_workspace_mb, and mle_eval_mfma_min_n through the evaluation's workspace): *out = min(what fits, 32768, batch), at
 * least 1; the last chunk takes what is left.  No device work.  The argument checks of gkr_grand_product_verify_batch_device. */
int  gkr_devtest_grand_product_chunk(gkr_ctx *ctx, int n, int batch, uint32_t *out);

/* ---- FRACTIONAL SUM (LogUp): sum_i N[i] / D[i] = P / Q over a resident pair of tables, proven as GKR on the tree of fraction additions ----
 * Lookups with multiplicities and batched memory checks rest on it.  `batch` independent pairs of tables N (numerators) and D
 * (denominators) of 2^n canonical values each, pair b at d_tables + (2 b) * 2^n (N) and + (2 b + 1) * 2^n (D) elements, variable 1 =
 * the most significant index bit; 3 <= n <= GKR_MAX_MLE_N, batch in 1 .. 65535, batch * 2^(n+1) <= 2^30 (the zero-check's own limit
 * on the top layer's four tables).  The reference has no such argument; the protocol is the library's own:
 *   tree     (p_n, q_n) = (N, D);  for k = n-1 .. 0, i < 2^k, with lo = i, hi = i + 2^k in level k+1:
 *                p_k[i] = p_{k+1}[lo] q_{k+1}[hi] + p_{k+1}[hi] q_{k+1}[lo],   q_k[i] = q_{k+1}[lo] q_{k+1}[hi];
 *            (P, Q) = (p_0[0], q_0[0]) and sum_i N[i] / D[i] = P / Q.  Nothing is inverted.  One launch per level
 *            (csrc/kernels_fraction_sum.hip) stores every level, canonical, in context workspace in the input's own layout: level k
 *            of pair b is p_k (2^k) then q_k (2^k).  The four tables of layer k's sumcheck, T0 = p lo half, T1 = p hi half,
 *            T2 = q lo half, T3 = q hi half of level k+1, lie at (4 b + m) 2^k in place: nothing is gathered or copied.
 *   head     the proof opens with level 2: p_2[0..3], q_2[0..3] (8 values); (P, Q) follow from them by the tree rule.
 *            zeta_1 = multi_hash(those 8 values, key 0), zeta_2 = multi_hash([zeta_1], key 0), z^(2) = (zeta_1, zeta_2),
 *            lambda_2 = multi_hash([zeta_2], key 0), cp_2 = p_2~(z^(2)), cq_2 = q_2~(z^(2)).
 *   layer k  = 2 .. n-1:  the zero-check at z^(k) of g = T0 T3 + T1 T2 + lambda_k T2 T3 (terms {2,{0,3}}, {2,{1,2}}, {2,{2,3}},
 *            coefficients 1, 1, lambda_k), claimed sum cp_k + lambda_k cq_k.  It yields k round vectors in rows of 4 slots, their
 *            lengths, the challenges r^(k), the four values (a0, a1, b0, b1) = T0..T3~(r^(k)) and eq(z^(k), r^(k)) -- byte for byte
 *            what gkr_sumcheck_zerocheck_batch_device returns with batch 1 on that pair's four tables with those coefficients and
 *            that point.  Then tau_k = multi_hash([a0, a1, b0, b1], key 0), cp_{k+1} = a0 + tau_k (a1 - a0),
 *            cq_{k+1} = b0 + tau_k (b1 - b0), z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k), lambda_{k+1} = multi_hash([tau_k], key 0).
 *   end      cp_n = N~(z^(n)) and cq_n = D~(z^(n)), which the verifier evaluates itself (no commitment, as elsewhere).
 * R = n (n - 1) / 2 - 1 rounds in all, layer k's rows from row k (k - 1) / 2 - 1 on: the grand product's bookkeeping.
 *   out_sums      batch x 2 values (P, Q)                         out_head    batch x 8 values p_2, q_2
 *   out_coeffs    batch x R rows of 4 slots, layers k = 2 .. n-1   out_len     batch x R values in 1 .. 4
 *   out_r         batch x R challenges                            out_evals   batch x (n - 2) x 4 values (a0, a1, b0, b1), or NULL
 *   out_point     batch x n coordinates z^(n), or NULL            out_claims  batch x 2 values (cp_n, cq_n), or NULL
 * zeta, tau, lambda and the claims are formed on the host between the layers; the rows are hashed on the device by the round
 * kernel, which reads the layer's lambda per proof (the zero-check's coefficients are one kernel argument for a whole batch).  A
 * D with a zero entry makes Q = 0: the prover still runs and stays exact, the verifier rejects (GKR_VERIFY_ZERO_DENOMINATOR).  A
 * layer whose g vanishes identically returns every vector as [0] with length 1 (the zero-check's own rule).  Inputs are not
 * modified.  The tree (2 batch (2^n - 1) elements) and the layers' buffers live in context workspace under slot names of this
 * path's own (fs.*): a zero-check, SOP, product or grand-product call on the same context is unaffected.
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): NULL ctx or pointer (the three optional outputs
 * excepted), batch outside 1 .. 65535, n outside 3 .. GKR_MAX_MLE_N, batch * 2^(n+1) above 2^30 values. */
int  gkr_fraction_sum_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int batch, gkr_fr *out_sums, gkr_fr *out_head,
                                   gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals /* or NULL */,
                                   gkr_fr *out_point /* or NULL */, gkr_fr *out_claims /* or NULL */);

/* one pair of tables of 2^n values each in host memory: upload + the call above with batch 1.  GKR_ERR_NON_CANONICAL (through
 * the context) for an entry >= r. */
int  gkr_fraction_sum(gkr_ctx *ctx, const gkr_fr *numerators, const gkr_fr *denominators, int n, gkr_fr *out_sum, gkr_fr *out_head,
                      gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals, gkr_fr *out_point, gkr_fr *out_claims);

/* Verifier of gkr_fraction_sum_batch_device's proofs against the resident pairs.  head / coeffs / len / r / evals: exactly the
 * arrays and layout of the prover (evals is required here); sums: batch x 2 claimed values (P, Q), or NULL (the head's own root is
 * then what the proof proves; out_sums returns it).  Built from the pieces of the grand product's verifier: the round relations
 * of every layer run on host threads (csrc/verify_rounds.h, csrc/fraction_sum_rounds.h), the round vectors' hashes on the device
 * from verify_device_hash_min round vectors on, else on the host threads (zeta, tau and lambda always on the host), and N and D
 * are read ONCE on the device, both at the one point z^(n) (gkr_mle_eval_batch_device's kernels, groups of two tables).
 * accept[batch] required; failed_layer / failed_round / failed_check (batch each) and out_sums (batch x 2) may be NULL.
 * Per proof, in this order, the first failure reported (failed_check, at failed_layer, failed_round):
 *   1. GKR_VERIFY_SHAPE             some len outside 1 .. 4; at (k, j) of the first such row
 *   2. GKR_VERIFY_NON_CANONICAL     an element >= r (unused slots are never read): a head entry or a claimed sum at (0, 0); else the
 *                                   first layer k with such an element: a used slot or a challenge of row j at (k, j), else one
 *                                   of its four values at (k, k)
 *   3. GKR_VERIFY_ZERO_DENOMINATOR  the head's Q is 0; at (0, 0).  Always checked
 *   4. GKR_VERIFY_FRACTION_SUM      with sums: (P, Q) claimed != the head's root, as a pair; at (0, 0)
 *   5. for k = 2 .. n-1, with the running claim cp_k + lambda_k cq_k:  for j = 0 .. k-1  GKR_VERIFY_ROUND_SUM, GKR_VERIFY_CHALLENGE
 *      at (k, j), in the order of the sumcheck verifiers;  then  GKR_VERIFY_FINAL_CLAIM
 *      g_k(r_k) != eq(z^(k), r^(k)) (a0 b1 + a1 b0 + lambda_k b0 b1)  at (k, k)
 *   6. GKR_VERIFY_EVALUATION        cp_n != N~(z^(n)) or cq_n != D~(z^(n)); at (n, n)
 * An accepted proof reports (0, 0, 0).  out_sums[b]: the head's root for every proof that passes checks 1 and 2, zeros for the
 * others.  Table entries are read as integers modulo r.  The return value is the status of the CALL, not the verdict;
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): NULL ctx or required pointer and every shape the
 * prover refuses.  Chunks hold min(what fits verify_workspace_mb, 32768, batch) proofs; verdicts depend neither on
 * verify_workspace_mb nor on verify_device_hash_min. */
int  gkr_fraction_sum_verify_batch_device(gkr_ctx *ctx, const void *d_tables, int n, int batch, const gkr_fr *sums /* or NULL */,
                                          const gkr_fr *head, const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r,
                                          const gkr_fr *evals, int *accept, uint32_t *failed_layer, uint32_t *failed_round,
                                          uint32_t *failed_check, gkr_fr *out_sums /* or NULL */);

/* one pair in host memory: upload + the call above with batch 1.  GKR_ERR_NON_CANONICAL for an entry >= r. */
int  gkr_fraction_sum_verify(gkr_ctx *ctx, const gkr_fr *numerators, const gkr_fr *denominators, int n, const gkr_fr *sum /* 2, or NULL */,
                             const gkr_fr *head, const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r, const gkr_fr *evals,
                             int *accept, uint32_t *failed_layer, uint32_t *failed_round, uint32_t *failed_check);

/* the launch geometry of the tree (host logic, from the function the launches call): one launch per level k = n-1 .. 0,
 * blocks[k] = its blocks of 256 threads per pair, ceil(2^k / 256), a thread per node (k = 0 .. n-1: n words).
 * GKR_ERR_INVALID: NULL pointer, n outside 3 .. GKR_MAX_MLE_N. */
int  gkr_selftest_fraction_sum_geometry(int n, uint32_t *blocks);
/* The tree alone, into the CALLER's device buffer instead of the context's workspace: d_layers takes 2 batch (2^n - 1) elements,
 * level k of pair b (p_k then q_k) at 2 batch (2^k - 1) + b 2^(k+1).  The argument checks of gkr_fraction_sum_batch_device. */
int  gkr_devtest_fraction_sum_tree(gkr_ctx *ctx, const void *d_tables, int n, int batch, void *d_layers);
/* The proofs per chunk gkr_fraction_sum_verify_batch_device works through for (n, batch) under the context's options: *out =
 * min(what fits, 32768, batch), at least 1.  No device work.  The argument checks of gkr_fraction_sum_verify_batch_device. */
int  gkr_devtest_fraction_sum_chunk(gkr_ctx *ctx, int n, int batch, uint32_t *out);

/* ---- LOOKUP (LogUp with multiplicities): every value of a resident witness column lies in a resident table -----------------------
 * The first application of the fractional sum above: the multiplicities and the pair (N, D) are built on the device
 * (csrc/kernels_lookup.hip), the proof is gkr_fraction_sum_batch_device's proof of that pair.  The reference has no such argument.
 *   inputs    `batch` witness columns W of 2^n_w canonical values, column b at d_witness + b * 2^n_w elements; tables T of 2^n_t
 *             canonical values: with shared_table != 0 ONE table at d_table for every column, else column b's own at
 *             d_table + b * 2^n_t; a challenge alpha per column, the CALLER's.  The library has no commitments (z and rho of
 *             the R1CS calls are the caller's for the same reason), which is why the multiplicities are a call of their own: a
 *             caller who wants soundness (1) fixes the multiplicities M, (2) commits to W, T and M, (3) derives alpha from the
 *             commitments -- in this order -- and only then proves.
 *   pair      L = max(n_w, n_t) + 1; the pair has 2^L entries, variable 1 = the most significant index bit.  The top-bit-0
 *             half is the witness side: (N, D)[i] = (1, alpha - W[i]) for i < 2^n_w, (0, 1) beyond; the top-bit-1 half is the
 *             table side: (N, D)[2^(L-1) + j] = (-M[j] mod r, alpha - T[j]) for j < 2^n_t, (0, 1) beyond.  Every witness value
 *             lies in T with M its multiplicities iff sum N / D = 0 as a rational function of alpha: the proof is the fractional
 *             sum's proof of this pair (n = L), and the verdict adds P == 0.
 *   M         M[j] = the number of i with W[i] = T[j] if j is the LOWEST index with T's value T[j], else 0: a value T holds
 *             several times gives its whole count to its first copy, so M is a function of (W, T).
 *   index     counting is a join of 256-bit keys.  Per table an open-addressing index, linear probing, 2^(n_t+1) slots of one
 *             uint32_t (load factor <= 1/2), empty = 0xFFFFFFFF.  A thread per table entry j, from slot h(T[j]) on:
 *             atomicCAS(slot, empty, j); claimed: done; the slot holds an index whose entry equals T[j] on all eight limbs:
 *             atomicMin(slot, j), done; else the next slot, wrapping at the end.  A slot's key never changes once claimed, so
 *             value -> lowest index does not depend on the order of arrival.  A launch of its own then counts: a thread per
 *             witness entry probes until the keys are equal and adds one to that index's uint32_t counter (counts <= 2^30); at an
 *             empty slot the entry is a miss.  With a shared table the index is built once; M is per column all the same.
 *   h         the slot of a canonical value v = (v0, v1, v2, v3), 64-bit limbs, least significant first, among 2^s slots,
 *             arithmetic modulo 2^64:  x = 0x9E3779B97F4A7C15;  for i = 0 .. 3: x = (x ^ v_i) * 0xFF51AFD7ED558CCD, x = x ^ (x >> 32);
 *             x = x * 0xC4CEB9FE1A85EC53;  x = x ^ (x >> 29);  h(v, s) = x >> (64 - s).  All four limbs are mixed (witness values are
 *             often small integers, and often differ in high limbs only); csrc/lookup_rules.h, gkr_selftest_lookup_slot.
 * Limits: 2 <= n_w, n_t; L <= GKR_MAX_MLE_N; batch in 1 .. 65535; batch * 2^(L+1) <= 2^30 (the fractional sum's own limit).
 * Anything else, or a NULL ctx or required pointer, is GKR_ERR_INVALID before a device or the context is touched (plain returns).
 * The index, the counters and the pair live in context workspace under slot names of this path's own (lk.*): a fractional-sum,
 * grand-product, zero-check, SOP or product call on the same context is unaffected.  Inputs are not modified. */

/* The multiplicities.  d_mult: batch x 2^n_t canonical elements in device memory, column b's at d_mult + b * 2^n_t -- a PROVER
 * output.  out_missing[b]: the number of entries of column b that are not in its table; out_first_missing[b]: the lowest such
 * index, or 0xFFFFFFFF.  A column with misses is not an error of the call: M counts the hits, the proof still runs and stays
 * exact, and the verifier rejects (GKR_VERIFY_LOOKUP) -- as the fractional sum does with a zero in D. */
int  gkr_lookup_multiplicities_device(gkr_ctx *ctx, const void *d_witness, int n_w, const void *d_table, int n_t, int shared_table,
                                      int batch, void *d_mult, uint32_t *out_missing, uint32_t *out_first_missing);

/* The proofs.  Builds the pairs from W, T, d_mult (as the call above left it, or any batch x 2^n_t canonical elements) and
 * alpha[batch] in context workspace, pair b being N then D -- one launch, a thread per pair entry, one modular subtraction or
 * negation each, the padding included -- then runs gkr_fraction_sum_batch_device on them with n = L.  The outputs are exactly that
 * call's arrays and layouts, byte for byte what it returns on the same pair:
 *   out_sums  batch x 2 (P, Q)    out_head  batch x 8    out_coeffs  batch x R rows of 4 slots, R = L (L - 1) / 2 - 1
 *   out_len   batch x R           out_r     batch x R    out_evals   batch x (L - 2) x 4, or NULL
 *   out_point batch x L, or NULL  out_claims batch x 2, or NULL
 * GKR_ERR_NON_CANONICAL (through the context) for an alpha >= r. */
int  gkr_lookup_batch_device(gkr_ctx *ctx, const void *d_witness, int n_w, const void *d_table, int n_t, int shared_table,
                             const void *d_mult, const gkr_fr *alpha, int batch, gkr_fr *out_sums, gkr_fr *out_head,
                             gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals /* or NULL */,
                             gkr_fr *out_point /* or NULL */, gkr_fr *out_claims /* or NULL */);

/* Verifier of gkr_lookup_batch_device's proofs against the same tables, d_mult and alpha: it reads W, T and M once to rebuild the
 * pair in workspace, runs gkr_fraction_sum_verify_batch_device on it without claimed sums (which reads the pair at z^(L)) and
 * reports that verifier's (failed_check, failed_layer, failed_round) with one addition:
 *   GKR_VERIFY_LOOKUP   the head's P != 0; at (0, 0).  It stands where GKR_VERIFY_FRACTION_SUM stands in that verifier's order --
 *                       after SHAPE, NON_CANONICAL and ZERO_DENOMINATOR, before the layers' relations and EVALUATION -- and is
 *                       decided from the root the inner call returns for every proof that passes SHAPE and NON_CANONICAL.
 * What follows from that:   alpha equal to a witness or table value: ZERO_DENOMINATOR;   M or alpha other than the prover's:
 * EVALUATION at (L, L);   a prover that ran on a wrong M, or on a witness with misses: LOOKUP.
 * accept[batch] required; failed_* (batch each) and out_sums (batch x 2: the heads' roots, zeros for a proof that fails SHAPE or
 * NON_CANONICAL) may be NULL.  The return value is the status of the CALL; GKR_ERR_NON_CANONICAL for an alpha >= r. */
int  gkr_lookup_verify_batch_device(gkr_ctx *ctx, const void *d_witness, int n_w, const void *d_table, int n_t, int shared_table,
                                    const void *d_mult, const gkr_fr *alpha, int batch, const gkr_fr *head, const gkr_fr *coeffs,
                                    const uint32_t *len, const gkr_fr *r, const gkr_fr *evals, int *accept, uint32_t *failed_layer,
                                    uint32_t *failed_round, uint32_t *failed_check, gkr_fr *out_sums /* or NULL */);

/* One column and one table in host memory: upload, count, prove; out_mult takes the 2^n_t multiplicities, out_missing and
 * out_first_missing one word each.  It takes alpha BEFORE M exists, so it is a convenience, not a sound composition (see `inputs`
 * above).  GKR_ERR_NON_CANONICAL for an entry or an alpha >= r. */
int  gkr_lookup(gkr_ctx *ctx, const gkr_fr *witness, int n_w, const gkr_fr *table, int n_t, const gkr_fr *alpha, gkr_fr *out_mult,
                uint32_t *out_missing, uint32_t *out_first_missing, gkr_fr *out_sum, gkr_fr *out_head, gkr_fr *out_coeffs,
                uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals, gkr_fr *out_point, gkr_fr *out_claims);
/* its counterpart: upload + gkr_lookup_verify_batch_device with batch 1.  GKR_ERR_NON_CANONICAL for an entry of witness, table or
 * mult, or an alpha, >= r. */
int  gkr_lookup_verify(gkr_ctx *ctx, const gkr_fr *witness, int n_w, const gkr_fr *table, int n_t, const gkr_fr *mult,
                       const gkr_fr *alpha, const gkr_fr *head, const gkr_fr *coeffs, const uint32_t *len, const gkr_fr *r,
                       const gkr_fr *evals, int *accept, uint32_t *failed_layer, uint32_t *failed_round, uint32_t *failed_check);

/* h (host logic, the function the kernels call): *slot = h(*v, log_slots).  GKR_ERR_INVALID: NULL pointer, log_slots outside 1 .. 32. */
int  gkr_selftest_lookup_slot(const gkr_fr *v, int log_slots, uint32_t *slot);
/* The pair alone, into the CALLER's device buffer instead of the context's workspace: d_pair takes batch x 2 x 2^L elements, pair b
 * (N then D) at d_pair + b * 2^(L+1).  The argument checks of gkr_lookup_batch_device. */
int  gkr_devtest_lookup_pair(gkr_ctx *ctx, const void *d_witness, int n_w, const void *d_table, int n_t, int shared_table,
                             const void *d_mult, const gkr_fr *alpha, int batch, void *d_pair);

/* ---- GKR layer sumcheck: prove_sumcheck_opt, sumcheck.rs:36-44 ----------- */
/* Layer i has 2^k_i gates; gate g is add (0) or mult (1) of entries left[g],
 * right[g] of layer i+1, which has 2^k_next entries W.  z: k_i challenges.
 * out_coeffs: 2*k_next rows x 3 slots; out_len[j] in {2,3}; out_r: 2*k_next. */
int  gkr_sumcheck_layer(gkr_ctx *ctx, int k_i, int k_next, const uint8_t *gate_type,
                        const uint32_t *left, const uint32_t *right, const gkr_fr *z,
                        const gkr_fr *W, gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r);

/* ---- one layer sumcheck split across GPUs by GATES ------------------------------------------------------
 * The reference sums the per-gate terms of a round with a rayon map-reduce over the gate list
 * (sumcheck.rs:50-63 b-rounds, :97-124 c-rounds).  In the linear-time form of the layer sumcheck every table the
 * rounds work on is a SUM OVER GATES: U(b), V(b) (2^k_next entries each) for the k_next rounds that bind b, then
 * the row a_u(c), m_u(c) for the k_next rounds that bind c.  So ANY partition of the gates over ranks works: each
 * rank sums its own gates, two sum-over-ranks exchanges per layer (2 * 2^k_next field elements each) complete the
 * tables, and the 2 k_next rounds run on the completed (tiny) tables identically on every rank -- every rank gets
 * the whole transcript, no broadcast.  Bit-exact: modular sums commute.
 *
 * This rank holds gates gate_first .. gate_first + gate_count - 1 of the layer's 2^k_i (the three arrays have
 * gate_count entries; gate_count may be 0).  z, W and the outputs are as for gkr_sumcheck_layer and identical on
 * all ranks.  Needs the host transcript; k_next <= GKR_MAX_K_NEXT as everywhere.
 *
 * allreduce: called twice per layer (three times never), each time with `count` canonical field elements in host
 * memory that it must replace by their sums over all ranks mod r (the same on every rank); 0 = success.  RCCL has
 * no modular sum: gkr_fr_widen / gkr_fr_narrow turn field elements into eight 32-bit limbs held in int64 (an
 * ordinary integer SUM all-reduce of those is exact for < 2^31 ranks) and back (gkr_amd/parallel.py does exactly
 * that over torch.distributed).  One extra element travels with the first exchange: "some rank saw a bad gate", so
 * that all ranks fail together instead of one leaving the others inside a collective. */
typedef int (*gkr_allreduce_fn)(void *user, gkr_fr *values, size_t count);
int  gkr_sumcheck_layer_sharded(gkr_ctx *ctx, int k_i, int k_next, uint64_t gate_first, uint64_t gate_count,
                                const uint8_t *gate_type, const uint32_t *left, const uint32_t *right, const gkr_fr *z,
                                const gkr_fr *W, gkr_allreduce_fn allreduce, void *user, gkr_fr *out_coeffs,
                                uint32_t *out_len, gkr_fr *out_r);
/* The same sumcheck with the gate arrays already in device memory (gkr_device_alloc + gkr_device_upload; gate_count
 * entries each, gates gate_first .. of the layer) -- nothing but z, W and the transcript crosses PCIe.  allreduce ==
 * NULL: the arrays hold the whole layer (gate_first = 0, gate_count = 2^k_i) and no exchange takes place, i.e.
 * gkr_sumcheck_layer on resident gates; otherwise as gkr_sumcheck_layer_sharded.  Gates are validated on the device. */
int  gkr_sumcheck_layer_device(gkr_ctx *ctx, int k_i, int k_next, uint64_t gate_first, uint64_t gate_count,
                               const void *d_gate_type, const void *d_left, const void *d_right, const gkr_fr *z,
                               const gkr_fr *W, gkr_allreduce_fn allreduce, void *user, gkr_fr *out_coeffs,
                               uint32_t *out_len, gkr_fr *out_r);
/* A layer's gates -- the whole layer, or one rank's contiguous share gate_first .. gate_first + gate_count -- kept in
 * device memory across sumchecks, together with the gate lists sorted from them on first use (what gkr_prove keeps per
 * circuit in its cache, for callers that drive prove_sumcheck_opt themselves: one circuit, many z / W).
 * gkr_resident_layer_sumcheck is gkr_sumcheck_layer_device on that layer: nothing but z, W and the transcript crosses
 * PCIe and no sort runs after the first call.  allreduce == NULL needs the whole layer. */
typedef struct gkr_resident_layer gkr_resident_layer;
int  gkr_resident_layer_create(gkr_ctx *ctx, int k_i, int k_next, uint64_t gate_first, uint64_t gate_count,
                               const uint8_t *gate_type, const uint32_t *left, const uint32_t *right,
                               gkr_resident_layer **out);
/* ... and with W (2^k_next values, canonical) already in DEVICE memory: what prover::prove has (the next layer's values come
 * from the forward evaluation, prover.rs:38-43) and what a host that drives prove_sumcheck_opt itself should do -- the
 * upload of a 2^20-value W is 0.5 ms of PCIe, a quarter of that layer's sumcheck.  Whole layers only (no exchange). */
int  gkr_resident_layer_sumcheck_wdev(gkr_ctx *ctx, gkr_resident_layer *layer, const gkr_fr *z, const void *d_W,
                                      gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r);
int  gkr_resident_layer_sumcheck(gkr_ctx *ctx, gkr_resident_layer *layer, const gkr_fr *z, const gkr_fr *W,
                                 gkr_allreduce_fn allreduce, void *user, gkr_fr *out_coeffs, uint32_t *out_len,
                                 gkr_fr *out_r);
void gkr_resident_layer_free(gkr_ctx *ctx, gkr_resident_layer *layer);
/* The same exchange without leaving the device -- the multi-GPU twin of the rayon reduce at sumcheck.rs:50-63,
 * 97-124 as "one RCCL reduce over xGMI": the caller owns a device buffer of `capacity` int64 (capacity >=
 * gkr_exchange_limbs(k_next)); per exchange the library widens its partial tables into it on the device (eight
 * 32-bit limbs per field element, each in an int64, plus one flag element), calls fn(user, count, hip_stream), which
 * must enqueue an in-place integer SUM all-reduce of d_limbs[0 .. count) ON THAT STREAM (ncclAllReduce(buf, buf, count,
 * ncclInt64, ncclSum, comm, stream); torch.distributed.all_reduce under torch.cuda.ExternalStream(stream)), and
 * reduces the sums mod r on the device.  No host copy, no stream synchronisation: the host next touches the stream
 * when the first round's record lands.  Once a call has passed its argument checks and workspace allocations (which come
 * first and fail alike on every rank given the same arguments), fn is called on every rank the same number of times even
 * when a rank fails locally (the flag element carries "some rank failed", and all ranks then return an error together); fn
 * itself must not fail on one rank only.  (A rank whose device runs out of memory while its peers' do not returns before
 * the first exchange: give every rank the same budget.) */
typedef int (*gkr_allreduce_dev_fn)(void *user, size_t count, void *hip_stream);
typedef struct {
    gkr_allreduce_dev_fn fn;
    void *user;
    int64_t *d_limbs;   /* device memory owned by the caller */
    size_t capacity;    /* in int64 elements */
} gkr_exchange_dev;
size_t gkr_exchange_limbs(int k_next);
int  gkr_resident_layer_sumcheck_dev(gkr_ctx *ctx, gkr_resident_layer *layer, const gkr_fr *z, const gkr_fr *W,
                                     const gkr_exchange_dev *exchange, gkr_fr *out_coeffs, uint32_t *out_len,
                                     gkr_fr *out_r);
/* ---- a sum over ranks the library owns: gkr_exchange_dev backed by RCCL ----------------------------------------------
 * For hosts that are not Python (the reference's Rust binary): no callback of the host's own, no torch.  librccl is
 * loaded on first use (dlopen), not linked.  One rank makes the 128-byte id (gkr_exchange_rccl_unique_id) and hands it
 * to the others by whatever it has; every rank -- a process per GPU, or a thread per GPU of one process, the calls made
 * concurrently -- then calls gkr_exchange_rccl_create(device, id, rank, nranks, capacity), which blocks until all ranks
 * have arrived (ncclCommInitRank) and owns a device buffer of `capacity_limbs` int64.  gkr_exchange_rccl_dev() is the
 * gkr_exchange_dev to pass to gkr_resident_layer_sumcheck_dev / gkr_sumcheck_mle_sharded_dev: its hook queues
 * ncclAllReduce(buf, buf, count, ncclInt64, ncclSum, comm, stream) on the stream the library hands it.  Errors: a status,
 * the text in gkr_exchange_rccl_error() (per thread).  What it stands for in the reference: the rayon reduce at
 * sumcheck.rs:50-63, 97-124 (and :62 for prove_sumcheck), over xGMI instead of over cores.
 *
 * gkr_exchange_rccl_create BLOCKS until all `nranks` ranks have called it with the same id: RCCL's ncclCommInitRank has no
 * timeout, and the library adds none -- a rank that never arrives leaves the others waiting, exactly as in a bare RCCL
 * program; the host that starts the ranks owns that failure mode (tests/test_gpu_sharded.py shows the wait: rank 0 of a
 * world of two, alone, is still inside the call when its parent ends it).  The unit builds without RCCL's development
 * header (the few ABI types are declared locally) and returns GKR_ERR_UNSUPPORTED where librccl cannot be loaded.
 *
 * STATUS: EXPERIMENTAL beyond one device.  The three multi-device mechanisms -- this exchange, gkr_ctx_create_multi and
 * gkr_sumcheck_mle_sharded_dev / gkr_resident_layer_sumcheck_dev across ranks -- are proven bit-exact with logical ranks
 * on one GPU, over gloo with two processes, and through RCCL with ONE rank (torch's communicator and this one); no build
 * of this library has yet had a second physical device (tests/test_gpu_multi_device.py runs the two-device cases and
 * skips where fewer than two GPUs are visible). */
#define GKR_RCCL_ID_BYTES 128
typedef struct gkr_rccl_exchange gkr_rccl_exchange;
int  gkr_exchange_rccl_unique_id(void *id_out /* GKR_RCCL_ID_BYTES */);
int  gkr_exchange_rccl_create(int device_id, const void *unique_id, int rank, int nranks, size_t capacity_limbs,
                              gkr_rccl_exchange **out);
const gkr_exchange_dev *gkr_exchange_rccl_dev(const gkr_rccl_exchange *x);
uint64_t gkr_exchange_rccl_calls(const gkr_rccl_exchange *x);   /* all-reduces queued so far */
void gkr_exchange_rccl_destroy(gkr_rccl_exchange *x);
const char *gkr_exchange_rccl_error(void);

/* ---- one plain sumcheck split over GPUs: prove_sumcheck (sumcheck.rs:158-214), its reduce over the hypercube (the rayon
 * reduce of sumcheck.rs:62) as one RCCL all-reduce per PASS ------------------------------------------------------------
 * A table T of 2^n values is split over P = 2^log2_shards ranks; rank p holds the shard
 *     T_p[h * 2 + x_n] = T[h * 2P + 2p + x_n],   h < 2^(n - log2_shards - 1)
 * (index bits log2_shards .. 1 of an entry are its rank; the last variable stays inside every shard), `batch` shards
 * of 2^(n - log2_shards) values each, contiguous in device memory.  Rounds bind the leading variable, so every pair is
 * rank-local until 2^6 entries per shard are left: the library runs its multi-round passes on the shard (the kernels of
 * gkr_sumcheck_mle_batch_device), and per pass of J <= 5 rounds ONE in-place SUM all-reduce of batch * (2^J + 2) * 8
 * int64 through `exchange` completes the 2^J sub-block sums (they are linear in the table), on the library's stream;
 * every rank then hashes the same round vectors and binds the same challenges.  One more all-reduce gathers the 2^6
 * entries every shard has left, and all ranks finish the last 6 + log2_shards rounds on that tail.  n = 20 on 8 ranks:
 * 3 exchanges + 1 gather instead of 20 per-round reduces.  Every rank returns the whole transcript (outputs as
 * gkr_sumcheck_mle_batch_device: batch x n rows), bit-exact with the unsharded sumcheck.  "Does T depend on x_n" (the
 * last round's length) is a neighbour compare inside the shards, OR-ed over the ranks with the sums.
 * exchange: as for gkr_resident_layer_sumcheck_dev; capacity >= gkr_exchange_limbs_mle(n, log2_shards, batch).  A rank
 * that fails still enters every exchange (the flag travels with the sums) and all ranks return an error together.
 * *out_exchanges (may be NULL): how many times fn was called.  log2_shards = 0 is allowed (one rank; fn may then be a
 * no-op).  Needs the host transcript; 1 <= n - log2_shards <= GKR_MAX_MLE_N. */
size_t gkr_exchange_limbs_mle(int n, int log2_shards, int batch);
int  gkr_sumcheck_mle_sharded_dev(gkr_ctx *ctx, const void *d_shards, int n, int log2_shards, int shard, int batch,
                                  const gkr_exchange_dev *exchange, gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r,
                                  uint32_t *out_exchanges);
/* host only: count field elements <-> count x 8 int64 (32-bit limbs, least significant first); narrow reduces
 * limb sums of up to 2^31 addends mod r */
int  gkr_fr_widen(const gkr_fr *values, size_t count, int64_t *limbs);
int  gkr_fr_narrow(const int64_t *limbs, size_t count, gkr_fr *values);

/* dense predicate tables A, M (2^{2 k_next} each) = add_i / mult_i restricted to z */
int  gkr_predicate_tables(gkr_ctx *ctx, int k_i, int k_next, const uint8_t *gate_type,
                          const uint32_t *left, const uint32_t *right, const gkr_fr *z,
                          gkr_fr *out_A, gkr_fr *out_M);

/* out[g] = prev[left[g]] (+ | *) prev[right[g]] */
int  gkr_layer_eval(gkr_ctx *ctx, size_t gates, const uint8_t *gate_type, const uint32_t *left,
                    const uint32_t *right, const gkr_fr *prev, size_t n_prev, gkr_fr *out);

/* ---- full GKR proof: prover::prove, prover.rs:6-9 ----------------------- */
/* A layered circuit as the reference's GKRCircuit holds it after
 * convert_r1cs_wtns_gkr (gkr.rs:53-114): layer 0 is the output layer; layer i
 * has 2^k[i] gates wired into layer i+1; the input layer has 2^k[depth] values. */
typedef struct {
    uint32_t depth;                 /* number of gate layers L (Proof.depth = L + 1) */
    const uint32_t *k;              /* L + 1 entries: k[0..L-1] gate layers, k[L] input layer */
    const uint8_t *const *gate_type;/* L arrays of 2^k[i] */
    const uint32_t *const *left;    /* L arrays of 2^k[i], values < 2^k[i+1] */
    const uint32_t *const *right;
} gkr_circuit_desc;

/* Caller-allocated proof buffers (sizes from the k list; gkr_proof_sizes fills
 * the counts).  Mirrors gkr.rs:7-19:
 *   sumcheck_coeffs  sum_i 2 k[i+1] rows x 3 slots (layer i's rows contiguous)
 *   sumcheck_len     one per row
 *   sumcheck_r       one per row
 *   q                per layer k[i+1]+1 slots right-aligned; q_len per layer
 *   z                k[0] + k[1] + ... + k[L] values (z[0] = 0s, prover.rs:16-21)
 *   r                L values (r*)
 *   d_coeffs         2^k[0] monomial coefficients of the output layer's MLE
 *                    (index bit pattern = which variables the monomial carries;
 *                    Proof.d is its non-zero entries, get_multi_ext poly.rs:502-536)
 *   input_coeffs     2^k[L] monomial coefficients of the input layer (Proof.input_func)
 */
typedef struct {
    gkr_fr *sumcheck_coeffs;
    uint32_t *sumcheck_len;
    gkr_fr *sumcheck_r;
    gkr_fr *q;
    uint32_t *q_len;
    gkr_fr *z;
    gkr_fr *r;
    gkr_fr *d_coeffs;
    gkr_fr *input_coeffs;
} gkr_proof_buf;

typedef struct {
    size_t rounds;        /* sum_i 2 k[i+1] */
    size_t q_slots;       /* sum_i (k[i+1] + 1) */
    size_t z_values;      /* sum_i k[i], i = 0..L */
    size_t d_coeffs;      /* 2^k[0] */
    size_t input_coeffs;  /* 2^k[L] */
} gkr_proof_sizes_t;

int  gkr_proof_sizes(const gkr_circuit_desc *circuit, gkr_proof_sizes_t *out);

/* input_values: the 2^k[L] values of the input layer (constants and witness
 * entries already gathered, convert.rs:796-810).  require_zero_output != 0
 * reproduces the reference's assert that output 0 is zero (convert.rs:838). */
int  gkr_prove(gkr_ctx *ctx, const gkr_circuit_desc *circuit, const gkr_fr *input_values,
               int require_zero_output, gkr_proof_buf *out);

/* `batch` proofs of ONE circuit for `batch` witnesses, advanced together (every layer's sumcheck runs
 * batched: one set of launches and one host round trip per round for all proofs) -- the reference proves
 * independent (circuit, input) pairs from a rayon par_iter (aggregator.rs:350-355).  input_values:
 * batch x 2^k[L] values; outs: `batch` caller-allocated proof buffers.  Needs the host transcript. */
int  gkr_prove_batch(gkr_ctx *ctx, const gkr_circuit_desc *circuit, const gkr_fr *input_values, int batch,
                     int require_zero_output, gkr_proof_buf *outs);

/* The proving step of one aggregation round in ONE call (aggregator.rs:341-355: prover::prove mapped over the
 * (circuit, input) pairs with a rayon par_iter): every item is a gkr_prove_batch (one circuit, `batch` witnesses); the
 * items are proven side by side, each by its own thread and child context (stream, workspaces, circuit cache) of `ctx`,
 * kept between calls.  A layer round of a small circuit is latency-bound -- launch, a tiny kernel, the hand-off, the
 * hash -- so independent items in flight fill each other's gaps; threads whose items are done, and threads waiting
 * for a round, take pieces of the others' host work (see gkr_host_help_while).  Items are dealt out by estimated cost,
 * the same way for the same list (so a child context finds its circuits in its cache on the next call).
 * LOCKSTEP GROUPS (round 5; option prove_many_lockstep, default on): items whose circuits share their k list -- the <= 20
 * sub-circuits of one compiled R1CS come in a few shapes -- are proven as ONE chain: one launch per pass and one hand-off
 * for the group, the passes over the gates reading each proof's own gate lists through a per-proof table.  A group holds at
 * most lockstep_max_proofs proofs (default 32: beyond that independent chains overlap better); an item that fails in a
 * group is proven again on its own, so statuses stay per item.  Same bytes as item by item.
 * The circuit cache of a context decides a hit by two 64-bit hashes over the k list and the gate arrays AND a comparison
 * with the gate arrays retained when the entry was made -- byte for byte up to 1 MiB of gate data, sampled 4 KiB blocks of
 * every array beyond: a context shared with callers that may hand in CRAFTED circuits larger than that should be given
 * GKR_NO_CIRCUIT_CACHE / no_circuit_cache (the proof would be wrong, not the memory unsafe: indices were range-checked).
 * max_concurrent: threads / child contexts to use at most; 0 = the CPUs this process may use, less two.
 * Every item's `status` is set; the return value is the first status that is not GKR_OK (gkr_last_error has its text). */
typedef struct {
    const gkr_circuit_desc *circuit;
    const gkr_fr *input_values;      /* batch x 2^k[L] */
    int batch;
    int require_zero_output;
    gkr_proof_buf *outs;             /* `batch` proof buffers */
    int status;                      /* out */
} gkr_prove_item;
int  gkr_prove_many(gkr_ctx *ctx, gkr_prove_item *items, size_t n_items, int max_concurrent);

/* ---- the reference's own argument types at `prove` (host only) ----------------------------------------------------
 * prover::prove(&GKRCircuit<S>, &Input<S>) (prover.rs:6-9) does not receive gate arrays and evaluation tables: a Layer
 * holds its wiring as `wire: (Vec<Vec<S>>, Vec<Vec<S>>)` (gkr.rs:35-51) -- per add gate and per mult gate one vector of
 * k_i + 2 k_next field elements 0 / 1, the bits of `gate || left || right`, most significant first (convert.rs:715-767,
 * convert_binary_to_vec) -- and Input.w[i] (gkr.rs:21-33) is layer i's multilinear extension as a TERM LIST: rows
 * [coeff, e_1 .. e_k] with exponents 0 / 1 (get_multi_ext, poly.rs:502-536; non-zero coefficients only, any order).
 * These three turn the one form into the other, so a binding can sit at `prove` itself without touching convert.rs
 * (INTEGRATION.md writes it out; tests/capi_dropin.c drives it from C):
 *   gkr_layer_from_wires   add_wire: n_add rows, mult_wire: n_mult rows of (k_i + 2 k_next) elements -> gate_type / left /
 *                          right of 2^k_i entries.  n_add + n_mult must be 2^k_i and every gate index appear once (every
 *                          slot of a compiled layer is a gate, convert.rs:209-214); an entry that is neither 0 nor 1, a gate
 *                          named twice or a count that does not fill the layer -> GKR_ERR_INVALID.
 *   gkr_values_from_terms  n_terms rows of (1 + k) elements -> the 2^k evaluations over the hypercube (index = the bit
 *                          string, variable 1 most significant): the inverse of get_multi_ext.  Equal monomials add up
 *                          (add_poly); an exponent other than 0 / 1 -> GKR_ERR_INVALID; n_terms = 0 gives the zero table.
 *   gkr_terms_from_coeffs  a table of 2^k monomial coefficients (gkr_proof_buf.d_coeffs / input_coeffs) -> the term list
 *                          Proof.d / Proof.input_func holds: the non-zero coefficients, ascending monomial index, rows of
 *                          (1 + k) elements.  *n_terms = how many there are; out_terms == NULL only counts;
 *                          GKR_ERR_NOMEM if capacity_terms is too small. */
int  gkr_layer_from_wires(int k_i, int k_next, const gkr_fr *add_wire, size_t n_add, const gkr_fr *mult_wire, size_t n_mult,
                          uint8_t *gate_type, uint32_t *left, uint32_t *right);
int  gkr_values_from_terms(int k, const gkr_fr *terms, size_t n_terms, gkr_fr *out_values);
int  gkr_terms_from_coeffs(int k, const gkr_fr *coeffs, gkr_fr *out_terms, size_t capacity_terms, size_t *n_terms);

/* prover::prove on exactly the reference's argument types, in ONE call (the three adapters above + gkr_prove): per layer i
 * the wire vectors of Layer.wire (add_wire[i]: n_add[i] rows, mult_wire[i]: n_mult[i] rows of k[i] + 2 k[i+1] elements; a
 * pointer may be NULL where its count is 0) and the input layer's term list Input.w[depth] (n_input_terms rows of 1 + k[depth]
 * elements).  Everything else as gkr_prove.  The statuses of the adapters pass through (GKR_ERR_INVALID: wire vectors that do
 * not describe a layer, a term that is not multilinear). */
typedef struct {
    uint32_t depth;                      /* number of gate layers L */
    const uint32_t *k;                   /* L + 1 entries (GKRCircuit::get_k_list) */
    const gkr_fr *const *add_wire;       /* L pointers */
    const size_t *n_add;                 /* L counts */
    const gkr_fr *const *mult_wire;
    const size_t *n_mult;
} gkr_wire_circuit;
int  gkr_prove_wires(gkr_ctx *ctx, const gkr_wire_circuit *circuit, const gkr_fr *input_terms, size_t n_input_terms,
                     int require_zero_output, gkr_proof_buf *out);

/* ---- verifier (host only, no device) ------------------------------------------------------------------------------
 * The relations the reference's verifier checks (python/gkr.py:202-231 with python/sumcheck.py:55-70; verifier.circom:39-71
 * holds the same inside a circuit) on the Rust prover's Proof, which carries no `f` / `add` / `mult` fields: per layer
 * every round's g_j(0) + g_j(1) = the running claim and r_j = multi_hash(g_j); the last claim =
 * add_i(z, b*, c*) (q(0) + q(1)) + mult_i(z, b*, c*) q(0) q(1) with the wiring predicates summed over the circuit's gates
 * (eq tables, O(gates) products on `threads` host threads; 0 = the CPUs this process may use); r* = multi_hash of the last
 * round vector; z[i+1] = l(r*); finally q(r*) of the last layer = input_func(z[L]).  z[0] must be zero (prover.rs:16-21).
 * *accept = 1 / 0; on a rejection *failed_layer / *failed_check (either may be NULL) name the first relation that failed.
 * The return value is a status of the CALL (GKR_ERR_INVALID: null pointers, a gate operand out of range), not the verdict. */
enum {
    GKR_VERIFY_OK = 0,
    GKR_VERIFY_SHAPE = 1,          /* a round vector / q length outside its range */
    GKR_VERIFY_NON_CANONICAL = 2,  /* a proof element >= r */
    GKR_VERIFY_Z0 = 3,             /* z[0] is not the zero vector */
    GKR_VERIFY_ROUND_SUM = 4,      /* g_j(0) + g_j(1) != claim */
    GKR_VERIFY_CHALLENGE = 5,      /* r_j != multi_hash(g_j) */
    GKR_VERIFY_FINAL_CLAIM = 6,    /* g_v(r_v) != add (q0 + q1) + mult q0 q1 */
    GKR_VERIFY_R_STAR = 7,         /* r* != multi_hash(last round vector) */
    GKR_VERIFY_NEXT_Z = 8,         /* z[i+1] != b* + r* (c* - b*) */
    GKR_VERIFY_INPUT = 9,          /* q(r*) of the last layer != input_func(z[L]) */
    GKR_VERIFY_EVALUATION = 10,    /* plain, product and sum-of-products sumcheck (gkr_sumcheck_*_verify*): g_n(r_n) != the tables'
                                      values at r combined as the sumcheck combines them: T~(r), prod_f T_f~(r), sum_k c_k prod_j T_t(k,j)~(r);
                                      gkr_r1cs_verify*: g_n(r_n) != the transcript's own evaluations combined */
    GKR_VERIFY_MATRIX = 11,        /* gkr_r1cs_verify*: e_T != sum_m rho_m M_m~(r_x, r_y) from the public matrices */
    GKR_VERIFY_WITNESS = 12,       /* gkr_r1cs_verify* with a witness: e_w != w~(r_y) */
    GKR_VERIFY_PRODUCT = 13,       /* gkr_grand_product_verify* with claimed products: a claim != the product of the proof's head */
    GKR_VERIFY_ZERO_DENOMINATOR = 14,  /* gkr_fraction_sum_verify*: the head's Q is 0 -- the sum P / Q is undefined */
    GKR_VERIFY_FRACTION_SUM = 15,  /* gkr_fraction_sum_verify* with claimed sums: a claimed (P, Q) != the root of the proof's head */
    GKR_VERIFY_LOOKUP = 16         /* gkr_lookup_verify*: the head's P is not 0 -- the fractions of witness and table do not cancel */
};
int  gkr_verify(const gkr_circuit_desc *circuit, const gkr_proof_buf *proof, int threads, int *accept, uint32_t *failed_layer,
                uint32_t *failed_check);

/* ---- verifier on the device ------------------------------------------------------------------------------------------
 * The same verdicts as gkr_verify with the three sums that take its time on the GPU: the wiring predicates over every gate,
 * the coefficient tables at z[0] / z[L], and the tables' canonical scans.  A verifier reads every challenge out of the proof,
 * so all layers of all proofs are launched at once and the call synchronises once per chunk.  The challenge hashes of a chunk
 * of proofs are independent of one another for the same reason: a chunk with at least verify_device_hash_min round vectors
 * (context option; 0 the measured default, -1 never, 1 always) hashes them on the device too, on a second stream beside the
 * sums; a smaller chunk hashes on the context's host threads (gkr_ctx_set_host_threads) while the device works.  Verdicts do
 * not depend on where the hashes ran.  After that the relations
 * themselves -- round sums, q, r*, next z, in gkr_verify's order -- are evaluated proof by proof on the calling thread, from the
 * hashes and the device's sums.  A verifier checks many proofs of one circuit: the gate arrays reach the device once, through
 * a handle the caller holds.
 *   gkr_verify_prepare   the argument checks of gkr_verify (depth, k limits, GKR_ERR_DEGENERATE for k[i] == 0, i >= 1), then
 *                        the gate arrays go to the device, packed to 8 bytes per gate, and every operand and gate type is
 *                        range-checked there: GKR_ERR_INVALID for a bad gate (no handle is returned; no pass over the gates
 *                        ever runs for such a circuit).  The handle keeps its own copy of the k list: the caller's arrays need
 *                        not outlive the call.  It belongs to the context's device.
 *   gkr_verify_prepared  proofs: `batch` proof buffers in host memory; accept[batch] is required, failed_layer[batch] and
 *                        failed_check[batch] may be NULL.  For every proof the triple (accept, failed_layer, failed_check) is
 *                        what gkr_verify returns for that proof and circuit.  ONE difference: a malformed circuit is
 *                        GKR_ERR_INVALID at prepare time whatever the proof says, where gkr_verify would report a rejection it
 *                        meets before the bad gate.  The batch is processed in chunks of as many proofs as fit the context
 *                        option verify_workspace_mb of device workspace (at least one); verdicts do not depend on the chunking.
 *   gkr_verify_circuit_free   releases a handle (NULL is allowed, for the handle and for the context).
 *   gkr_verify_device    prepare + verify + free in one call.
 * The return value is the status of the CALL (GKR_ERR_NO_DEVICE, GKR_ERR_HIP, GKR_ERR_NOMEM as everywhere).  What needs no
 * device is checked before the device is touched: NULL pointers and batch < 1 (GKR_ERR_INVALID), a NULL ctx
 * (GKR_ERR_INVALID), a degenerate k list (GKR_ERR_DEGENERATE; decided from the circuit alone, before ctx or a proof is looked at).
 *   gkr_mimc7_multi_hash_device   the verifier's hash kernel for a caller's own round vectors (below).
 */
typedef struct gkr_verify_circuit gkr_verify_circuit;
int  gkr_verify_prepare(gkr_ctx *ctx, const gkr_circuit_desc *circuit, gkr_verify_circuit **out);
int  gkr_verify_prepared(gkr_ctx *ctx, const gkr_verify_circuit *vc, const gkr_proof_buf *proofs, int batch,
                         int *accept, uint32_t *failed_layer, uint32_t *failed_check);
void gkr_verify_circuit_free(gkr_ctx *ctx, gkr_verify_circuit *vc);
int  gkr_verify_device(gkr_ctx *ctx, const gkr_circuit_desc *circuit, const gkr_proof_buf *proofs, int batch,
                       int *accept, uint32_t *failed_layer, uint32_t *failed_check);   /* prepare + verify + free */
/* n independent Mimc7 multi_hash calls (key 0) on the device: rows of 3 slots, right-aligned as in gkr_proof_buf.sumcheck_coeffs;
 * len[i] in 1..3.  out[i] = multi_hash of row i's trailing len[i] slots, valid[i] = 1; a row whose length is outside 1..3 or whose
 * used slots hold an element >= r gets valid[i] = 0 and out[i] = 0 (the call still returns GKR_OK: a verifier meets such rows).
 * Processed in pieces of the device workspace; n >= 1.  NULL pointers, a NULL ctx and n == 0 are GKR_ERR_INVALID before the
 * device is touched.  The kernel and its launcher are gkr_verify_prepared's ("verify_hash" in the context's profile). */
int gkr_mimc7_multi_hash_device(gkr_ctx *ctx, const gkr_fr *rows, const uint32_t *len, size_t n, gkr_fr *out, uint32_t *valid);

/* ---- the proof as input signals of verifier.circom (host only) -----------
 * What the reference does with a Proof right after the path: pad its ragged vectors to the dimensions of
 * the generated verifier component (get_meta aggregator.rs:92-146, modify_proof_for_circom :148-213), print
 * field elements as decimal strings (file_utils.rs:20-28) and merge them into the circuit's input JSON
 * under keys suffixed with the proof's index (CircomInputProof aggregator.rs:20-82, file_utils.rs:49-67).
 * circuit: only depth and k are read.
 * gkr_circom_meta: [depth, largest k, k[0], #terms of D, longest round vector, longest q, #terms of the
 *   input function, k[L], k[0..L]] -- the VerifyGKR template arguments; *count = 8 + L + 1.
 * gkr_circom_input_json: one JSON object with the keys sumcheckProof<i>, sumcheckr<i>, q<i>, D<i>, z<i>,
 *   r<i>, inputFunc<i> (NUL-terminated).  *needed = bytes including the terminator; with out == NULL only
 *   the size is returned; GKR_ERR_NOMEM if capacity is too small.  Term order of D / inputFunc: ascending
 *   monomial index (the reference's order is HashMap order, i.e. unspecified). */
int  gkr_circom_meta(const gkr_circuit_desc *circuit, const gkr_proof_buf *proof, uint32_t *meta, size_t capacity,
                     size_t *count);
int  gkr_circom_input_json(const gkr_circuit_desc *circuit, const gkr_proof_buf *proof, int proof_index, char *out,
                           size_t capacity, size_t *needed);

/* The circom source the reference adds to the user's circuit for the next aggregation round (modify_circom_file,
 * aggregator.rs:215-314), as pure text functions (no circom is run): gkr_circom_verifier_source = the
 * `component verifier[n]` declaration and, per proof, the VerifyGKR(meta) instance, its input signals and the
 * wiring loops; metas = the proofs' meta vectors back to back, meta_len[i] entries each.  gkr_circom_inject = the
 * circuit text with the verifier include after the line `pragma circom 2.0.0;` and the source in front of the
 * first line that is exactly `}`.  Size protocol as gkr_circom_input_json. */
int  gkr_circom_verifier_source(const uint32_t *metas, const size_t *meta_len, size_t proofs, char *out, size_t capacity,
                                size_t *needed);
int  gkr_circom_inject(const char *circuit_text, const char *verifier_source, char *out, size_t capacity, size_t *needed);

/* ---- in front of the path: R1CS + witness -> layered circuits (host only) ------------------------------
 * What the reference does between circom's output files and prover::prove: read the iden3 `.r1cs` and `.wtns`
 * containers (third-party r1cs-file / wtns-file crates; aggregator.rs:341,345,399,404), turn every constraint
 * <A,w> * <B,w> - <C,w> = 0 into an expression tree (convert_constraints_to_nodes, convert.rs:360-632), and
 * compile the trees into at most 20 layered circuits whose every layer has 2^k add / mult gates over the next
 * one (compile, convert.rs:154-358; get_k :140-152).  gkr_layered_circuit hands out the gkr_circuit_desc that
 * gkr_prove / gkr_prove_batch take; gkr_layered_input_values gathers a witness into the input layer's values
 * (calculate_input, convert.rs:796-810) -- the forward evaluation and the "output 0 is zero" assertion
 * (:812-838) happen inside gkr_prove (require_zero_output).
 * Formats: `.r1cs` = magic "r1cs", version 1, sections (type u32, size u64): 1 header {field size 32, prime,
 * nWires, nPubOut, nPubIn, nPrvIn, nLabels u64, nConstraints}, 2 constraints {per constraint three linear
 * combinations: nTerms, then (wire u32, coefficient 32 B LE) per term}, 3 wire2label; `.wtns` = magic "wtns",
 * version 2, sections 1 {field size, prime, nWitness} and 2 {values, 32 B LE}.  Only BN254 Fr is accepted.
 * The writers exist because there is no circom in the build image: test fixtures have to be written. */
typedef struct gkr_r1cs gkr_r1cs;
typedef struct gkr_layered gkr_layered;
typedef struct {
    uint32_t n_wires, n_pub_out, n_pub_in, n_prv_in;
    uint64_t n_labels;
    size_t n_constraints, n_terms;   /* n_terms: over all A, B, C of all constraints */
} gkr_r1cs_info_t;

int  gkr_r1cs_parse(const void *bytes, size_t len, gkr_r1cs **out);
/* flat form: term_counts has 3 entries per constraint (A, B, C), wires / coeffs list all terms in that order */
int  gkr_r1cs_build(uint32_t n_wires, uint32_t n_pub_out, uint32_t n_pub_in, uint32_t n_prv_in, size_t n_constraints,
                    const uint32_t *term_counts, const uint32_t *wires, const gkr_fr *coeffs, gkr_r1cs **out);
int  gkr_r1cs_info(const gkr_r1cs *r1cs, gkr_r1cs_info_t *out);
int  gkr_r1cs_export(const gkr_r1cs *r1cs, uint32_t *term_counts, uint32_t *wires, gkr_fr *coeffs);
/* *needed = size of the file image; with out == NULL only the size is returned; GKR_ERR_NOMEM if too small */
int  gkr_r1cs_serialize(const gkr_r1cs *r1cs, void *out, size_t capacity, size_t *needed);
void gkr_r1cs_free(gkr_r1cs *r1cs);
int  gkr_wtns_parse(const void *bytes, size_t len, gkr_fr *out, size_t capacity, size_t *count);
int  gkr_wtns_serialize(const gkr_fr *values, size_t count, void *out, size_t capacity, size_t *needed);

/* bad_constraint (may be NULL): index of the constraint behind GKR_ERR_UNSUPPORTED */
int  gkr_r1cs_compile(const gkr_r1cs *r1cs, gkr_layered **out, size_t *bad_constraint);
int  gkr_layered_count(const gkr_layered *layered, uint32_t *circuits);
/* the arrays *out points to stay owned by `layered` */
int  gkr_layered_circuit(const gkr_layered *layered, uint32_t index, gkr_circuit_desc *out);
/* input layer of circuit `index`: slot s holds witness[wire[s]], or constant[s] where wire[s] == UINT32_MAX */
int  gkr_layered_input_layer(const gkr_layered *layered, uint32_t index, const uint32_t **wire, const gkr_fr **constant,
                             size_t *slots);
int  gkr_layered_input_values(const gkr_layered *layered, uint32_t index, const gkr_fr *witness, size_t n_witness,
                              gkr_fr *out_values);
void gkr_layered_free(gkr_layered *layered);

/* ---- R1CS zero-check: Az, Bz, Cz built on the device, then eq (A B - C) ---------------------------------
 * A witness w satisfies an R1CS iff  sum_x eq(z, x) (Az(x) Bz(x) - Cz(x)) = 0  for a random z, with Az(i) = <A_i, w> the value
 * of constraint i's first linear combination (Bz, Cz alike) and zero for i >= n_constraints.  The three tables are sparse
 * matrix-vector products; they are computed on the device from the witness and handed to the zero-check above.
 *
 * Host side (no device, no context): the matrices A, B, C = matrix 0, 1, 2 in CSR form.  row_ptr: n_constraints + 1 offsets into
 * the matrix's term records; a record is {wire, coeff}, coeff an index into ONE pool of distinct canonical coefficients shared by
 * the three matrices: pool[0] = 1 and pool[1] = r - 1 always, the other values in order of first appearance (constraint by
 * constraint, A before B before C, a row's terms in the file's order).  A term with coefficient 0 is dropped; a wire that
 * appears twice in a row stays as two terms; an empty combination is an empty row.  long_rows: the ascending indices of the rows
 * with more than GKR_R1CS_LONG_ROW terms (the device gives those a wave each instead of a thread).
 * n = max(2, ceil(log2(n_constraints))): the tables have 2^n entries.
 * GKR_ERR_INVALID: NULL r1cs or out, n_constraints == 0, n > GKR_MAX_MLE_N, n_wires == 0, a matrix outside 0 .. 2.
 * GKR_ERR_UNSUPPORTED: more than 2^32 - 1 terms in one matrix. */
#define GKR_R1CS_LONG_ROW 32
typedef struct { uint32_t wire, coeff; } gkr_r1cs_term;
typedef struct {
    uint32_t n, n_wires;
    size_t n_constraints, n_terms[3], n_long_rows[3], n_pool;   /* n_terms: without the dropped ones */
} gkr_r1cs_csr_info_t;
int  gkr_r1cs_csr_info(const gkr_r1cs *r1cs, gkr_r1cs_csr_info_t *out);
/* any output pointer may be NULL; sizes from the info call (row_ptr n_constraints + 1, terms n_terms[matrix], long_rows
 * n_long_rows[matrix], pool n_pool) */
int  gkr_r1cs_csr_export(const gkr_r1cs *r1cs, int matrix, uint32_t *row_ptr, gkr_r1cs_term *terms, uint32_t *long_rows,
                         gkr_fr *pool);

/* The CSR form resident on ONE context's device (row offsets, records, long-row lists, the pool in Montgomery form): made once
 * per R1CS, used for witness after witness.  Free it before its context is destroyed.  GKR_ERR_INVALID (plain return) for a NULL
 * pointer and whatever the info call refuses. */
typedef struct gkr_r1cs_rows gkr_r1cs_rows;
int  gkr_r1cs_rows_prepare(gkr_ctx *ctx, const gkr_r1cs *r1cs, gkr_r1cs_rows **out);
int  gkr_r1cs_rows_info(const gkr_r1cs_rows *rows, gkr_r1cs_csr_info_t *out);
void gkr_r1cs_rows_free(gkr_r1cs_rows *rows);

/* d_out[(b * 3 + m) * 2^n + i] = sum_t pool[coeff_t] * w_b[wire_t] over row i of matrix m, canonical; rows >= n_constraints are
 * zero: batch x 3 tables of 2^n values, the n_tables = 3 layout of the zero-check.  Witness b: the n_wires canonical elements at
 * d_witness + b * stride_elements (canonical by precondition, as every resident table is); not modified.
 * out_first_bad: batch values, the lowest constraint index with a * b != c, or UINT32_MAX; NULL = no check pass.
 * GKR_ERR_INVALID (plain returns, before a device is touched): NULL ctx, rows, d_witness or d_out; batch outside 1 .. 65535;
 * stride_elements < n_wires; batch * 3 * 2^n above 2^30; rows prepared on another context. */
int  gkr_r1cs_rows_device(gkr_ctx *ctx, const gkr_r1cs_rows *rows, const void *d_witness, size_t stride_elements, int batch,
                          void *d_out, uint32_t *out_first_bad);

/* The rows into context workspace (slots of this path's own: a plain, product, SOP or zero-check call on the same context is
 * unaffected), then the zero-check with terms {2, {0, 1}} coefficient 1 and {1, {2}} coefficient r - 1: the outputs of the
 * zero-check's batch call with n_tables = 3 (rows of 4 slots), byte for byte what that call returns on the tables the call above
 * writes.  An unsatisfied witness is NOT an error: its transcript has a non-zero claim g_1(0) + g_1(1), and out_first_bad says
 * where.  The verifier is left with claims on the three tables' values at r (out_evals); reducing those to the witness is the
 * inner sumcheck below (gkr_r1cs_inner_batch_device), a call of its own.
 * GKR_ERR_INVALID as above, and for NULL z, out_coeffs, out_len or out_r; GKR_ERR_NON_CANONICAL (through the context) for a z
 * entry >= r. */
int  gkr_r1cs_zerocheck_batch_device(gkr_ctx *ctx, const gkr_r1cs_rows *rows, const void *d_witness, size_t stride_elements, int batch,
                                     const gkr_fr *z /* host, batch x n */, gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r,
                                     gkr_fr *out_evals /* batch x 3 or NULL */, gkr_fr *out_eq /* batch or NULL */,
                                     uint32_t *out_first_bad /* batch or NULL */);

/* A host witness of n_witness >= n_wires values: prepare + upload + the call above with batch 1 + free.  GKR_ERR_INVALID also for
 * n_witness < n_wires and for 3 * 2^n above 2^30; GKR_ERR_NON_CANONICAL also for a witness entry >= r. */
int  gkr_r1cs_zerocheck(gkr_ctx *ctx, const gkr_r1cs *r1cs, const gkr_fr *witness, size_t n_witness, const gkr_fr *z /* n */,
                        gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals, gkr_fr *out_eq,
                        uint32_t *out_first_bad);

/* ---- R1CS inner sumcheck: the claims on Az, Bz, Cz at r_x reduced to ONE claim on the witness ------------------
 * The zero-check above leaves v_A = Az~(r_x), v_B = Bz~(r_x), v_C = Cz~(r_x) (its out_evals at its out_r).  For any
 * rho = (rho_A, rho_B, rho_C) and EVERY witness, satisfied or not,
 *     rho_A v_A + rho_B v_B + rho_C v_C = sum_y T(y) w(y),    T(y) = sum_m rho_m sum_i M_m[i][y] eq(r_x, i),
 * with M_0, M_1, M_2 = A, B, C, w the witness zero-padded to 2^n_y entries and n_y = max(2, ceil(log2 n_wires)): the second
 * sumcheck of a Spartan-style argument.  T is a transposed sparse matrix-vector product, built on the device; the sumcheck is the
 * product path's at degree 2 over (T, w).  It leaves w~(r_y) -- one evaluation of the witness, gkr_mle_eval_batch_device -- and
 * T~(r_y) = sum_m rho_m M_m~(r_x, r_y), a sum over the non-zeros of the public matrices (gkr_amd/verifier.py, on integers).
 * The points x and the weights rho are the CALLER's, as z is in the zero-check: nothing derives Fiat-Shamir challenges across
 * calls.
 *
 * Host side (no device, no context): the matrices in COLUMN-major form, one column per wire.  col_ptr: n_wires + 1 offsets into
 * the matrix's records; a record is the CSR form's gkr_r1cs_term with the ROW (the constraint index) in its first field (`wire`)
 * and the same pool index: the pool is the CSR form's entry for entry, the same terms are dropped (coefficient 0), a wire that
 * appears twice in a row gives two records with the same row.  A column's records are in ascending row order, within a row in the
 * CSR order (a stable counting sort of the CSR records by wire).  long_cols: the ascending indices of the columns with more than
 * GKR_R1CS_LONG_COL records.  n_x = the CSR form's n.  Refusals: the CSR info call's, GKR_ERR_UNSUPPORTED included. */
#define GKR_R1CS_LONG_COL 32
typedef struct {
    uint32_t n_x, n_y, n_wires;
    size_t n_constraints, n_terms[3], n_long_cols[3], n_pool;
} gkr_r1cs_csc_info_t;
int  gkr_r1cs_csc_info(const gkr_r1cs *r1cs, gkr_r1cs_csc_info_t *out);
/* any output pointer may be NULL; sizes from the info call (col_ptr n_wires + 1, terms n_terms[matrix], long_cols
 * n_long_cols[matrix], pool n_pool) */
int  gkr_r1cs_csc_export(const gkr_r1cs *r1cs, int matrix, uint32_t *col_ptr, gkr_r1cs_term *terms, uint32_t *long_cols,
                         gkr_fr *pool);

/* The column-major form resident on ONE context's device (column offsets, records, long-column lists, the segments the long
 * columns are cut into, the pool in Montgomery form): made once per R1CS and context, a type of its own beside the rows handle: a
 * caller that never runs the inner sumcheck never pays for it.  Free it before its context is destroyed.  GKR_ERR_INVALID
 * (plain return) for a NULL pointer and whatever the info call refuses.
 * gkr_r1cs_cols_prepare_segment: the same with long columns cut into segments of at most `segment` records instead of
 * GKR_R1CS_COL_SEGMENT (0: no cut, a wave per long column); results do not depend on it.  For measurements. */
#define GKR_R1CS_COL_SEGMENT 2048
typedef struct gkr_r1cs_cols gkr_r1cs_cols;
int  gkr_r1cs_cols_prepare(gkr_ctx *ctx, const gkr_r1cs *r1cs, gkr_r1cs_cols **out);
int  gkr_r1cs_cols_prepare_segment(gkr_ctx *ctx, const gkr_r1cs *r1cs, uint32_t segment, gkr_r1cs_cols **out);
int  gkr_r1cs_cols_info(const gkr_r1cs_cols *cols, gkr_r1cs_csc_info_t *out);
void gkr_r1cs_cols_free(gkr_r1cs_cols *cols);

/* d_out[b * out_stride_elements + y] = sum_m rho_{b,m} sum_{records (i, c) of column y of M_m} pool[c] eq(x_b, i), canonical, for
 * y < 2^n_y; zero for y >= n_wires.  eq(x_b, .): the canonical eq table of sumcheck b's own point of n_x coordinates (variable 1 =
 * the most significant index bit, gkr_eq_table_device's order), built in context workspace under slot names of this path's own
 * ("r1cs.cols.*").  Elements between the tables are not touched.  Exact: the order of summation is the library's.
 * GKR_ERR_INVALID (plain returns, before a device is touched): NULL ctx, cols, x, rho or d_out; batch outside 1 .. 65535;
 * out_stride_elements < 2^n_y; batch * 2 * 2^n_y or batch * 2^n_x above 2^30 values; cols prepared on another context.
 * GKR_ERR_NON_CANONICAL (through the context) for an x or rho entry >= r. */
int  gkr_r1cs_cols_device(gkr_ctx *ctx, const gkr_r1cs_cols *cols, const gkr_fr *x /* host, batch x n_x */,
                          const gkr_fr *rho /* host, batch x 3 */, int batch, void *d_out, size_t out_stride_elements /* >= 2^n_y */);

/* The tables {T_b, w_b zero-padded to 2^n_y} of every sumcheck into context workspace, laid out as the product path takes them
 * (factor f of sumcheck b at (b * 2 + f) * 2^n_y), then that path at degree 2: the outputs are byte for byte what
 * gkr_sumcheck_product_batch_device(.., n_y, 2, batch, ..) returns on those tables -- rows of 3 slots, its length rules, its
 * all-[0] transcript when T is the zero table (rho = 0).  g_1(0) + g_1(1) = sum_m rho_m Mz_m~(x): with x = the zero-check's out_r,
 * sum_m rho_m out_evals[m] of that call.  Witness b: the n_wires canonical elements at d_witness + b * stride_elements (canonical
 * by precondition); not modified.
 *   out_evals   batch x 2: T_b~(r_y), w_b~(r_y); or NULL
 * GKR_ERR_INVALID as above, and for NULL d_witness, out_coeffs, out_len or out_r and stride_elements < n_wires;
 * GKR_ERR_NON_CANONICAL as above. */
int  gkr_r1cs_inner_batch_device(gkr_ctx *ctx, const gkr_r1cs_cols *cols, const void *d_witness, size_t stride_elements, int batch,
                                 const gkr_fr *x /* host, batch x n_x */, const gkr_fr *rho /* host, batch x 3 */,
                                 gkr_fr *out_coeffs /* batch x n_y rows of 3 slots */, uint32_t *out_len, gkr_fr *out_r /* batch x n_y */,
                                 gkr_fr *out_evals /* batch x 2 or NULL */);

/* A host witness of n_witness >= n_wires values: prepare + upload + the call above with batch 1 + free.  GKR_ERR_INVALID also for
 * n_witness < n_wires; GKR_ERR_NON_CANONICAL also for a witness entry >= r. */
int  gkr_r1cs_inner(gkr_ctx *ctx, const gkr_r1cs *r1cs, const gkr_fr *witness, size_t n_witness, const gkr_fr *x /* n_x */,
                    const gkr_fr *rho /* 3 */, gkr_fr *out_coeffs, uint32_t *out_len, gkr_fr *out_r, gkr_fr *out_evals);

/* ---- R1CS verifier: the two transcripts above against z, rho and the public matrices --------------------------
 * A verifier of the two calls holds no table: it has the matrices, its own z and rho, and the proof.  What ties the proof to the
 * R1CS is T~(r_y) = sum_m rho_m M_m~(r_x, r_y) with
 *     M_m~(x, y) = sum over the records (row i, wire w, coefficient c) of matrix m of  c eq(x, i) eq(y, w),
 * one pass over the non-zeros: the CSR form of the rows handle, eq(x, .) and eq(y, .) as tables of 2^n and 2^n_y entries in context
 * workspace (slot names of this path's own, "r1cs.mat.*"), nothing else of 2^n entries written, the padding rows never visited.
 * n_y = max(2, ceil(log2 n_wires)), the CSC info's rule, from the handle's n_wires.
 *
 * out[b * 3 + m] = M_m~(x_b, y_b), canonical; variable 1 = the most significant index bit on both sides.  A boolean (x, y) gives
 * the sum of the coefficients at that (row, wire): zero for a row >= n_constraints or a wire >= n_wires.  Equal, value for value,
 * to gkr_eq_table_device(y) -> gkr_r1cs_rows_device (that table as the witness) -> gkr_mle_eval_batch_device(x).
 * GKR_ERR_INVALID before a device or the context is touched (plain returns): NULL pointer; batch outside 1 .. 65535; rows
 * prepared on another context; n or n_y above 28; batch * (2^n + 2^n_y) above 2^30 values.  GKR_ERR_NON_CANONICAL (through the
 * context) for a coordinate >= r.  Processed in chunks of verify_workspace_mb of device workspace. */
int  gkr_r1cs_matrix_evals_device(gkr_ctx *ctx, const gkr_r1cs_rows *rows, const gkr_fr *x /* host, batch x n */,
                                  const gkr_fr *y /* host, batch x n_y */, int batch, gkr_fr *out /* host, batch x 3 */);

/* Verifier of gkr_r1cs_zerocheck_batch_device's and gkr_r1cs_inner_batch_device's transcripts, tied together.  Per proof b:
 *   z          n elements, the zero-check's point                          rho        3 elements, the inner call's weights
 *   coeffs_x   n rows of 4 slots, len_x, r_x: the zero-check's outputs     evals_abc  3 elements, its out_evals (v_A, v_B, v_C)
 *   coeffs_y   n_y rows of 3 slots, len_y, r_y: the inner call's outputs   evals_tw   2 elements, its out_evals (e_T, e_w)
 * all in host memory, batch of each one after the other.  d_witness: NULL, or witness b's n_wires canonical elements at
 * d_witness + b * stride_elements in device memory (not modified).
 * accept[batch] required; failed_stage / failed_round / failed_check (batch each) may be NULL.  The first failure in this order
 * (failed_stage 1 .. 4, 0 for an accepted proof; failed_check: the GKR_VERIFY_* values):
 *   stage 1, the zero-check's transcript (degree 3):
 *     GKR_VERIFY_SHAPE          some len_x[j] outside 1 .. 4; failed_round = the first such j
 *     GKR_VERIFY_NON_CANONICAL  a used slot or r_x[j] >= r: failed_round = the first such j; an evals_abc entry: failed_round = n
 *     for j = 0 .. n-1:  GKR_VERIFY_ROUND_SUM  g_j(0) + g_j(1) != the running claim, which starts at ZERO;
 *                        GKR_VERIFY_CHALLENGE  r_x[j] != multi_hash(used slots of row j, key 0)
 *     GKR_VERIFY_EVALUATION     g_n(r_n) != eq(z, r_x) (v_A v_B - v_C), eq(z, r_x) the product of n factors; failed_round = n
 *   stage 2, the inner transcript (degree 2): the same checks on rows of 3 slots, the running claim starting at sum_m rho_m v_m,
 *     NON_CANONICAL also for an evals_tw entry (failed_round = n_y), EVALUATION for g(r) != e_T e_w (failed_round = n_y)
 *   stage 3  GKR_VERIFY_MATRIX  e_T != sum_m rho_m M_m~(r_x, r_y), the three values from the call above's kernels; failed_round = n_y
 *   stage 4  GKR_VERIFY_WITNESS only with d_witness: e_w != w~(r_y), the witness zero-padded to 2^n_y entries and evaluated on the
 *            device; failed_round = n_y
 * With d_witness == NULL the claim (r_y, e_w) on the witness is the CALLER's to settle: this library has no commitment to a
 * witness, and an accepted proof then says "IF w~(r_y) = e_w".  A proof that fails SHAPE or NON_CANONICAL in either transcript
 * never sends its point to the device: its slot is evaluated at zeros and its verdict is decided without that value.
 * z and rho are the verifier's own inputs: an entry >= r is GKR_ERR_NON_CANONICAL for the whole call (through the context), not a
 * verdict.  The return value is the status of the CALL, not the verdict.  GKR_ERR_INVALID (plain returns): what
 * gkr_r1cs_matrix_evals_device refuses, NULL for any required array, stride_elements < n_wires when a witness is given.
 * The round relations run on the context's host threads; both transcripts' round vectors are hashed on the device from
 * verify_device_hash_min of them per chunk on, on the host threads below; chunks of verify_workspace_mb.  Verdicts depend on
 * neither option. */
int  gkr_r1cs_verify_batch_device(gkr_ctx *ctx, const gkr_r1cs_rows *rows, int batch, const gkr_fr *z /* batch x n */,
                                  const gkr_fr *coeffs_x /* batch x n rows of 4 slots */, const uint32_t *len_x, const gkr_fr *r_x,
                                  const gkr_fr *evals_abc /* batch x 3 */, const gkr_fr *rho /* batch x 3 */,
                                  const gkr_fr *coeffs_y /* batch x n_y rows of 3 slots */, const uint32_t *len_y, const gkr_fr *r_y,
                                  const gkr_fr *evals_tw /* batch x 2 */, const void *d_witness /* or NULL */, size_t stride_elements,
                                  int *accept, uint32_t *failed_stage, uint32_t *failed_round, uint32_t *failed_check);

/* A host gkr_r1cs and an optional host witness of n_witness >= n_wires values (NULL: none): prepare + upload + the call above
 * with batch 1 + free.  GKR_ERR_INVALID also for n_witness < n_wires; GKR_ERR_NON_CANONICAL also for a witness entry >= r. */
int  gkr_r1cs_verify(gkr_ctx *ctx, const gkr_r1cs *r1cs, const gkr_fr *z, const gkr_fr *coeffs_x, const uint32_t *len_x, const gkr_fr *r_x,
                     const gkr_fr *evals_abc, const gkr_fr *rho, const gkr_fr *coeffs_y, const uint32_t *len_y, const gkr_fr *r_y,
                     const gkr_fr *evals_tw, const gkr_fr *witness /* or NULL */, size_t n_witness,
                     int *accept, uint32_t *failed_stage, uint32_t *failed_round, uint32_t *failed_check);

/* ---- step-wise sessions: one sumcheck split across GPUs -------------------
 * The reference reduces each round's per-assignment polynomials with a rayon
 * map-reduce (sumcheck.rs:50-63,65-78,97-124); across GPUs that reduce is one
 * tiny all-reduce per round.  The hypercube is partitioned by its TRAILING
 * log2(P) variables (rank p owns index low bits == p), so every pair of a
 * leading-variable round is rank-local.  A session does one rank's table work;
 * the caller owns the collective and the transcript (gkr_amd/parallel.py).
 * P = 1 gives the whole sumcheck with an external transcript. */
typedef struct gkr_layer_session gkr_layer_session;
typedef struct gkr_mle_session gkr_mle_session;

/* shard `shard` of `nshards` (power of two, <= 2^k_next) of the layer sumcheck:
 * keeps the gates whose right operand % nshards == shard; runs 2 k_next - log2(nshards) rounds */
int  gkr_layer_session_open(gkr_ctx *ctx, int k_i, int k_next, const uint8_t *gate_type,
                            const uint32_t *left, const uint32_t *right, const gkr_fr *z,
                            const gkr_fr *W, uint32_t nshards, uint32_t shard,
                            gkr_layer_session **out);
/* the redundant tail after the all-gather of the shards' last entries: tables of 2^kc entries */
int  gkr_layer_session_open_tables(gkr_ctx *ctx, int kc, const gkr_fr *A, const gkr_fr *M,
                                   const gkr_fr *wb, const gkr_fr *Wc, gkr_layer_session **out);
int  gkr_layer_session_dep(gkr_ctx *ctx, const gkr_layer_session *s, uint32_t *out_dep, uint32_t count);
int  gkr_layer_session_rounds(const gkr_layer_session *s, uint32_t *done, uint32_t *total);
/* this shard's partial sums of the current round: out[0] = c0, out[1] = g(1), out[2] = c2 */
int  gkr_layer_session_sums(gkr_ctx *ctx, gkr_layer_session *s, gkr_fr *out);
int  gkr_layer_session_bind(gkr_ctx *ctx, gkr_layer_session *s, const gkr_fr *r);
/* after the last local round: out = { A, M, Wc, W(b*) } of this shard */
int  gkr_layer_session_tail(gkr_ctx *ctx, gkr_layer_session *s, gkr_fr *out);
void gkr_layer_session_close(gkr_ctx *ctx, gkr_layer_session *s);

/* plain multilinear sumcheck on a device-resident table of 2^n entries (a shard or the whole table) */
int  gkr_mle_session_open(gkr_ctx *ctx, const void *d_table, int n, gkr_mle_session **out);
/* out[0] = sum of the low half, out[1] = sum of the high half of the current table */
int  gkr_mle_session_sums(gkr_ctx *ctx, gkr_mle_session *s, gkr_fr *out, uint32_t *out_dep);
int  gkr_mle_session_bind(gkr_ctx *ctx, gkr_mle_session *s, const gkr_fr *r);
int  gkr_mle_session_value(gkr_ctx *ctx, gkr_mle_session *s, gkr_fr *out);
void gkr_mle_session_close(gkr_ctx *ctx, gkr_mle_session *s);
int  gkr_device_tables_differ(gkr_ctx *ctx, const void *d_a, const void *d_b, size_t count,
                              uint32_t *out_differ);

/* ---- device memory helpers (so callers need no HIP of their own) -------- */
int  gkr_device_alloc(gkr_ctx *ctx, size_t bytes, void **d_ptr);
int  gkr_device_free(gkr_ctx *ctx, void *d_ptr);
int  gkr_device_upload(gkr_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int  gkr_device_download(gkr_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* synthetic table generator used by bench.py and the full-size parity tests
 * (definition: element i, limb j = mix64(seed + (4 i + j + 1) * 0x9E3779B97F4A7C15),
 * top limb masked to 61 bits; mix64 = splitmix64's finaliser) */
int  gkr_device_fill_table(gkr_ctx *ctx, void *d_table, size_t count, uint64_t seed);
/* the same stream of values, the 2^(n - log2_shards) entries rank `shard` of gkr_sumcheck_mle_sharded_dev holds of the
 * 2^n-entry table gkr_device_fill_table would write (bench.py --mode mle-split; no table ever exists in one piece) */
int  gkr_device_fill_shard(gkr_ctx *ctx, void *d_shard, int n, int log2_shards, int shard, uint64_t seed);
int  gkr_device_synchronize(gkr_ctx *ctx);
/* What this box itself gives, measured now (SURVEY section 8d asks bench.py to quote them beside the vendor
 * peaks): a plain device-to-device copy of `bytes` (>= 64 MiB; read + write counted) and a read-only stream, in
 * GB/s, and the chip-wide rate of 254-bit Montgomery products (dependent chains, 16 waves per SIMD) -- the
 * arithmetic ceiling of the gate passes of prove_sumcheck_opt (sumcheck.rs:50-63, 97-124).  No reference
 * counterpart: measurement only. */
/* host only: microseconds per Mimc7::multi_hash (sumcheck.rs:84,129,152) of a len-element round vector on ONE thread
 * of this host: sixteen transcripts side by side in AVX-512 IFMA lanes (time per hash; 0 without IFMA), and one
 * transcript on the scalar code.  The legs of the bench that are bound by the transcript quote their floor from it. */
int  gkr_ubench_host_hash(int len, double *us_per_hash_lanes16, double *us_per_hash_scalar);
int  gkr_ubench_ceilings(gkr_ctx *ctx, size_t bytes, double *copy_GBps, double *read_GBps, double *modmul_per_sec);

#ifdef __cplusplus
}
#endif
#endif /* GKR_AMD_H */
