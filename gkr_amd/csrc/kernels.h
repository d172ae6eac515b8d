// Launchers of the CDNA4 kernels (kernels.hip).  Internal to the library; the
// public surface is include/gkr_amd.h.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "flagged_rec.h"
#include "fr32.h"

namespace gkr {

constexpr uint32_t kMaxBlocksPerTable = 2048;
constexpr uint32_t kMaxLayerBlocks = 2048;

struct MlePartial {
    Acc<9> lo, hi;
    uint32_t dep, pad;
};

// a batch of layer sumchecks that share their gates (proofs of one circuit): per-proof strides of the
// predicate tables, the W copies and the partials; batch = 1 with zero strides is the single sumcheck
struct LayerBatch {
    uint32_t batch;
    uint32_t pstride;
    size_t tstride, wstride;
};
inline LayerBatch single_layer() { return LayerBatch{1u, 0u, 0, 0}; }

struct LayerPartial {
    Acc<9> c0, g1, c2;
    uint32_t pad;
};

// pinned-host hand-off records of the host transcript (128 B each, seq written last)
struct MleHostRec {
    Fr c0, c1;
    uint32_t dep, seq;
    uint32_t pad[14];
};
struct LayerHostRec {
    Fr c0, g1, c2;
    uint32_t seq;
    uint32_t pad[7];
};
static_assert(sizeof(MleHostRec) == 128 && sizeof(LayerHostRec) == 128, "hand-off records are one 128-byte line");

// Multi-round passes of the layer sumcheck's product form (kernels.hip, "product passes"): a pass hands the host the
// 4^J cross sums of the sub-blocks of W and X and the 2^J sub-block sums of Y, J <= kProdMaxJ rounds' worth.
constexpr int kProdMaxJ = 3;
constexpr int kProdRecValues = 72;   // m[a * 8 + b], a, b < 2^J; then sy[a] at 64 + a
struct ProdPassRec {
    Fr v[kProdRecValues];
    uint32_t seq;
    uint32_t pad[7];
};
static_assert(sizeof(ProdPassRec) == kProdRecValues * 32 + 32, "product-pass record layout");
// entries per block of a pass (one tile) and blocks per proof for tables whose sub-blocks have S entries
constexpr uint32_t kProdTile = 8, kProdTileWide = 32;
inline uint32_t prod_pass_tile(uint32_t S) { return S >= 1024u ? kProdTileWide : kProdTile; }
inline uint32_t prod_pass_blocks(uint32_t S) { return S <= kProdTile ? 1u : S / prod_pass_tile(S); }
// most blocks per proof any pass over tables of 2^k entries takes (sub-blocks of 1 .. 2^(k-1) entries)
inline uint32_t prod_pass_max_blocks(uint32_t k) {
    uint32_t m = 1;
    for (uint32_t l = 0; l < k; ++l) m = prod_pass_blocks(1u << l) > m ? prod_pass_blocks(1u << l) : m;
    return m;
}
// Fr values of pass scratch per proof for tables of 2^k entries (the blocks' partials, and behind them the first-level
// totals of passes with more than 1024 blocks)
inline size_t prod_pass_scratch_values(uint32_t k) { return ((size_t)prod_pass_max_blocks(k) + 64u) * kProdRecValues; }
// One pass on the tables W (Montgomery), X, Y (canonical) of 2^m_in entries per proof (stride wstride): bind the jp
// variables of the previous pass with the 2^jp Montgomery weights at weights + proof * 8 (in place; jp = 0: none), then
// the cross sums for the next J rounds -> the pinned records (seq = ticket, system-scope release); partials: scratch of
// batch x prod_pass_blocks(2^(m_in - jp - 1)) x 72 values for passes that span several blocks per proof.
// arrivals (may be null): `batch` zeroed words; passes of 2 .. kProdFuseBlocks blocks per proof then publish from their last
// block instead of a second launch (the words are zero again when the kernel ends).
// tail (may be null; pinned host memory, batch x 3 tables x tail_stride entries): the pass also leaves there the tables its
// rounds work on (2^(m_in - jp) <= tail_stride entries each, the pending fold applied) -- the host runs the rest of the
// phase's passes itself (capi_layer.hip, host tail).
// fold_plans (may be null): batch * prod_fold_plan_bytes() of device memory; passes with three variables pending over tables
// of 2^kProdFoldMinM entries and more then fold on the matrix cores first (unless the option no_mfma_cross is set).
constexpr uint32_t kProdFuseBlocks = 64;
constexpr uint32_t kProdFoldMinM = 17;
size_t prod_fold_plan_bytes();
void launch_prod_pass(Fr* W, Fr* X, Fr* Y, uint32_t m_in, uint32_t jp, const Fr* weights, uint32_t J, Fr* partials, uint32_t wstride,
                      ProdPassRec* rec, uint32_t ticket, uint32_t batch, hipStream_t s, uint32_t* arrivals = nullptr, void* fold_plans = nullptr,
                      Fr* tail = nullptr, uint32_t tail_stride = 0);
// start of the c-phase: W(u) = sum_b w_b Wb[b] over the 2^jp entries left of Wb, then X = A + W(u) M, Y = W(u) A over
// the 2^k entries of the rows A, M (gate_rows), per proof
void launch_prod_c_setup(const Fr* Wb, uint32_t jp, const Fr* weights, const Fr* A, const Fr* M, Fr* X, Fr* Y, uint32_t k, uint32_t wstride,
                         uint32_t batch, hipStream_t s);

constexpr uint32_t kSmallFoldQuarter = 2048;   // rounds whose output half has <= this many entries use one block per sumcheck
void launch_mle_fold_sum_small(const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                               const FixedMul* rtab, MleHostRec* host_rec, uint32_t ticket, hipStream_t s);
void launch_mle_round_reduce(const MlePartial* partials, uint32_t nblk, uint32_t batch, MleHostRec* host_rec,
                             uint32_t ticket, hipStream_t s);

// multi-round passes (see kernels.hip)
struct MleSubPartial {
    Acc<9> sum;
    uint32_t dep, pad[2];
};
constexpr int kMlePassMaxRounds = 5;                   // rounds one pass can cover (matrix-core fold: mfma_fold.h)
constexpr int kMleMaxSub = 1 << kMlePassMaxRounds;     // sub-block sums / fold weights per sumcheck and pass
struct MleHostRecSub {   // pinned hand-off record: up to 32 sub-block sums, seq written last
    Fr sums[kMleMaxSub];
    uint32_t dep, seq;
    uint32_t pad[14];
};
static_assert(sizeof(MleHostRecSub) == 1088, "hand-off record layout");
// a pass that publishes its own sums (latency-bound passes: the last block to arrive totals the partials; arrivals == nullptr:
// launch_mle_sub_reduce does it)
struct MlePublish {
    MleHostRecSub* rec = nullptr;   // the first sumcheck of the launch
    uint32_t* arrivals = nullptr;   // one zeroed counter per sumcheck of the launch; left zero
    uint32_t ticket = 0, jout = 0;
};
constexpr uint32_t kSmallPassEntries = 512;   // passes whose output has <= this many entries run as one block per sumcheck
uint32_t mle_pass_blocks(uint32_t items, uint32_t jout, uint32_t batch);
uint32_t mle_multifold_blocks(uint32_t S, uint32_t jout, uint32_t batch);
bool mle_multifold_uses_mfma(uint32_t S, uint32_t nblk);
// pass 0 (launch_mle_sub_sums): k_mle_sub_sums, or for streaming launches (no publish, chunk = len / nblk a multiple of 256 entries, nblk a
// multiple of 4) its pipelined form k_mle_sub_sums_stream (a wave per one or two partials, its loads in flight in two sets), or, for
// the launches of the two-partial form, k_mle_sub_sums_roll (a wave per partial, ONE buffer of sixteen loads each reloaded as soon as
// it is added, the blocks of an XCD on one contiguous eighth of the launch) -- the same partials, bit for bit
constexpr int kMlePass0Stream = 3;   // what option pass0_stream = 0 means: 1 k_mle_sub_sums always, 2 the pipelined form where it applies, 3 the rolling form where the deeper pipelined form applies
// launches of at least this many partials (and chunks of whole 512 entries) take the form with sixteen loads per lane and two partials per
// wave: 2 partials x 12 resident waves x 256 CUs x 4 generations.  Reasoned, not tuned: only 128 tables x 1024 partials was measured
// (profiles/r22); what smaller launches take is a guess that keeps their block count at the chip's size or above
constexpr uint64_t kMlePass0DeepMinPartials = 2u * 12u * 256u * 4u;
// Host arithmetic only (the launch and the launch plan, capi_mle_passes.hip, both call them): the form launch_mle_sub_sums gives a launch
// -- 0 k_mle_sub_sums, 1 k_mle_sub_sums_stream<8, 1>, 2 k_mle_sub_sums_stream<16, 2>, 3 k_mle_sub_sums_roll -- and whether a launch of that
// form that is offered flag-in-word records publishes there (k_mle_sub_sums_roll_pub)
int mle_sub_sums_stream_form(uint32_t len, uint32_t batch, uint32_t nblk, bool publishes);
bool mle_sub_sums_publishes_flagged(int form, uint32_t nblk);
// Every pass: per-block partial sums, then a reduce kernel that writes the pinned host record.
// flagged != nullptr (pinned: batch x kFlagRecsPerTable flag-in-word records, flagged_rec.h): the rolling form with kFlagRecsPerTable
// blocks per table publishes its blocks' sums there under flag_ticket and returns true -- the host totals them, no reduce launch
bool launch_mle_sub_sums(const Fr* tables, size_t stride, uint32_t len, uint32_t batch, uint32_t nblk, MleSubPartial* partials,
                         hipStream_t s, const MlePublish* publish = nullptr, uint64_t* flagged = nullptr, uint32_t flag_ticket = 0);
void launch_mle_sub_reduce(const MleSubPartial* partials, uint32_t nblk, uint32_t jout, uint32_t batch, MleHostRecSub* host_rec,
                           uint32_t ticket, hipStream_t s);
size_t mle_fold_plan_bytes();
void launch_mle_fold_plan(int jin, const Fr* weights, void* plans, uint32_t batch, hipStream_t s, uint32_t threads = 0);
void launch_mle_multifold(int jin, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t S, uint32_t batch,
                          uint32_t nblk, const Fr* weights, const void* plans, MleSubPartial* partials, hipStream_t s,
                          const MlePublish* publish = nullptr);
// the host's share of a pass ON THE DEVICE (kernels_transcript.hip): J rounds of `count` sumchecks from their records
void launch_mle_pass_hash_lanes(const MleHostRecSub* rec, uint32_t count, uint32_t J, uint32_t round0, uint32_t n_out, bool final_pass,
                                bool first_pass, const Fr* cts, uint32_t* dep_last, Fr* weights, Fr* out_coeffs, uint32_t* out_len, Fr* out_r,
                                hipStream_t s);
// tail (may be null; pinned host memory, tail_stride entries per sumcheck): the folded table (S <= tail_stride entries) is left there
// too -- the host binds the remaining variables itself (capi_mle.hip, the host tail of a lone sumcheck).
void launch_mle_multifold_small(int jin, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t S, uint32_t jout,
                                uint32_t batch, const Fr* weights, MleHostRecSub* host_rec, uint32_t ticket, hipStream_t s, Fr* tail = nullptr, uint32_t tail_stride = 0,
                                uint32_t planes = 1, uint32_t plane_stride = 0);
// The first fold at two levels (kernels.hip): launch_mle_fine_sums turns pass 0's partials (nblk a multiple of 1024 per table) and the
// weights of rounds 1-5 into the 32 sums of rounds 6-10; launch_mle_multifold2 binds the ten variables in one read of the table
// (S = 2^(n-5), plans: launch_mle_fold_plan(5) of the first five, w2: the other 32 weights copied to device memory by
// launch_mle_copy_weights) and leaves eight partial planes of S / 32 entries and mle_multifold2_partials(S) partials per table.
constexpr uint32_t kMleFold2Planes = 8;
uint32_t mle_multifold2_partials(uint32_t S);
// host arithmetic only: a launch_mle_multifold2 that is offered flag-in-word records publishes there
bool mle_multifold2_publishes_flagged(uint32_t S);
// tiles of 64 entries a block of the fold takes: one, or what option fold2_tiles forces
uint32_t mle_multifold2_tiles(uint32_t S);
uint32_t mle_multifold2_blocks(uint32_t S);   // the launch's blocks per table: (S / 256) / tiles
void launch_mle_fine_sums(const MleSubPartial* partials, uint32_t nblk, const Fr* weights, uint32_t batch, MleHostRecSub* host_rec, uint32_t ticket,
                          hipStream_t s);
void launch_mle_copy_weights(const Fr* src, Fr* dst, uint32_t batch, hipStream_t s);
// (flagged, flag_ticket, return value: as launch_mle_sub_sums', for launches of kFlagRecsPerTable partials of >= 16 entries per table; ended,
// may be null: fired by a publishing kernel's completion)
bool launch_mle_multifold2(const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t S, uint32_t batch, const void* plans, const Fr* w2,
                           MleSubPartial* partials, hipStream_t s, uint64_t* flagged = nullptr, uint32_t flag_ticket = 0, hipEvent_t ended = nullptr);
void launch_layer_round_reduce(const LayerPartial* partials, uint32_t nblk, LayerHostRec* host_rec, uint32_t ticket,
                               LayerBatch lb, hipStream_t s);
void launch_fold_small(Fr* W, uint32_t hw, const FixedMul* rtab, LayerBatch lb, hipStream_t s);
// gate lists by left / right operand and the 2^k-entry tables summed straight from them (no dense predicate tables).
// GateSpan: the gate arrays hold gates base .. base + count - 1 of the layer (the whole layer, or one rank's shard).
struct GateSpan {
    uint64_t base, count;
};
// lds_scratch: gate_lists_lds_scratch_words(gates, k) words (or null): large layers sort with block-private LDS
// histograms instead of one global atomic per gate and operand
uint32_t gate_lists_lds_blocks(uint64_t gates, uint32_t k);
size_t gate_lists_lds_scratch_words(uint64_t gates, uint32_t k);
// `list`: 2 * gate_list_words(gates) words -- the gate indices of every bucket (left-operand buckets, then right-operand
// buckets), and after them, entry for entry, what the sums over a bucket need of the gate besides its index: the OTHER
// operand in the low bits, the gate type in bit 31 (read in list order instead of gathered by gate index)
inline size_t gate_list_words(uint64_t gates) { return 2 * (size_t)gates + 1; }
// Segments of the sorted lists (gate_seg.h): the bucket lists cut where gate >> shift changes, so that E_hi is a common
// factor of a segment; segments cut into items of <= kSegCap gates, both halves (left-operand buckets, right-operand
// buckets) in one item array, `order` = the items of each half by decreasing length.  Built once per circuit by
// launch_gate_lists right after the block-private sort (whose per-block starts ARE the segment bounds).
struct GateSegs {
    uint32_t shift = 0;      // log2 gates per run; 0: no segments (small layer, unaligned shard): the bucket kernels run
    uint32_t runs = 0;       // runs the span covers
    uint32_t run_base = 0;   // the span's first run in the layer (index into E_hi)
    uint32_t bound = 0;      // capacity of items / order (both halves together)
    uint32_t half_bound = 0; // most items one half can have
    uint32_t groups = 0;     // most groups (64 items, one wave's work) one half can have
    uint32_t nb = 0;         // 2^k buckets per half
    uint64_t packed_half = 0;   // capacity of one half of `packed`, in entries
    uint32_t* words = nullptr;  // one allocation of gate_segs_words()
    // items | order | bucket_begin | group_len | group_off | packed
    uint2* items() const { return reinterpret_cast<uint2*>(words); }      // {first list entry, len | run << 8}
    uint32_t* order() const { return words + 2 * (size_t)bound; }          // the items of each half by decreasing length
    uint32_t* bucket_begin() const { return order() + bound; }             // 2 nb + 1 item offsets (+ 1 pad)
    uint32_t* group_len() const { return bucket_begin() + 2 * (size_t)nb + 2; }   // 2 * groups: gates of a group's longest item
    uint32_t* group_off() const { return group_len() + 2 * (size_t)groups; }      // 2 * groups + 1: first entry / 64 of the group in `packed`
    // The list entries once more, in the order the pass reads them: group after group, inside a group step-major --
    // entry (step j, lane l) = gate j of the group's item l -- so that a wave's load of one step is 256 contiguous bytes
    // (per-lane walks through list / meta cost one cache line per gate and array).
    // entry = (gate & mask) | other operand << shift | type << 31   (shift + k <= 31)
    uint32_t* packed() const { return group_off() + 2 * (size_t)groups + 2; }
};
// the split point of eq(z, g) = E_hi[g >> shift] * E_lo[g & mask] the gate passes of this span use: k_i / 2 for the
// bucket kernels, the segment shift where segments apply (a function of the span and the widths only)
uint32_t gate_seg_shift(GateSpan span, uint32_t k_i, uint32_t k);
size_t gate_segs_words(GateSpan span, uint32_t k_i, uint32_t k);           // u32 words of GateSegs::words (0: no segments)
size_t gate_segs_scratch_words(GateSpan span, uint32_t k_i, uint32_t k);   // u32 words of build scratch
size_t gate_seg_partial_elems(GateSpan span, uint32_t k_i, uint32_t k);    // Fr elements of pass scratch per proof
void launch_gate_lists(GateSpan span, uint32_t k_i, uint32_t k, const uint8_t* gate_type, const uint32_t* left, const uint32_t* right,
                       uint32_t* counts, uint32_t* offsets, uint32_t* cursor, uint32_t* block_sums, uint32_t* list, uint32_t* bad,
                       uint32_t* lds_scratch, GateSegs* segs, uint32_t* seg_scratch, hipStream_t s);
// The sorted gate lists (and gate arrays) of ONE circuit layer on the device, as the passes over the gates read them.  A pass
// over a batch of proofs of one circuit takes the pointers as launch arguments; a pass over proofs of DIFFERENT circuits whose
// layers have the same shape (gkr_prove_many's lockstep groups: the reference's par_iter over the (circuit, input) pairs of a
// step, aggregator.rs:411-416, as ONE launch per pass) takes `sets`, a device table with one entry per proof of the launch,
// and ignores the pointer arguments.
struct GateSet {
    const uint32_t* offsets;      // 2 * 2^k bucket starts
    const uint32_t* cursor;       // 2 * 2^k bucket ends
    const uint32_t* list;         // gate indices by bucket; the entries' meta words follow at list + gate_list_words(gates)
    const uint32_t* plan;         // the wide layers' item plan (gate_plan_words; may be null)
    const uint8_t* gate_type;     // the layer's gate arrays (layer evaluation)
    const uint32_t* left;
    const uint32_t* right;
    uint64_t pad;
};
static_assert(sizeof(GateSet) == 64, "one cache line per proof");
// e_hi / e_lo_mont split at `kl` = gate_seg_shift() when segs->shift != 0 (partials: gate_seg_partial_elems() * batch
// elements of scratch), else at any kl
void launch_gate_uv(GateSpan span, uint32_t k_i, uint32_t k, const uint32_t* offsets, const uint32_t* cursor, const uint32_t* list,
                    const Fr* e_hi, const Fr* e_lo_mont, uint32_t kl, const Fr* W, Fr* U, Fr* V, LayerBatch lb, const GateSegs* segs,
                    Fr* partials, hipStream_t s, const GateSet* sets = nullptr);
// the c-phase's set-up done by the row pass itself (launch_prod_c_setup's arguments; Wb null: not fused)
struct CPhaseFuse {
    const Fr* Wb = nullptr;
    const Fr* weights = nullptr;
    Fr* X = nullptr;
    Fr* Y = nullptr;
    uint32_t jp = 0;
};
// fuse (may be null): also write X = a_u + W(u) m_u, Y = W(u) a_u; returns true when it did (the segment form), false when
// the caller still has to launch_prod_c_setup (the bucket form)
bool launch_gate_rows(GateSpan span, uint32_t k_i, uint32_t k, const uint32_t* offsets, const uint32_t* cursor, const uint32_t* list,
                      const Fr* e_hi, const Fr* e_lo_mont, uint32_t kl, const Fr* eq_mont, Fr* A_row, Fr* M_row, LayerBatch lb,
                      const GateSegs* segs, Fr* partials, hipStream_t s, const CPhaseFuse* fuse = nullptr, const GateSet* sets = nullptr);
void launch_fill_table(Fr* table, size_t count, uint64_t seed, hipStream_t s);
void launch_fill_shard(Fr* shard_table, size_t count, uint32_t lp, uint32_t shard, uint64_t seed, hipStream_t s);
// sum over ranks without leaving the device: a, b (each `each` elements) + one flag element <-> (2 each + 1) x 8 int64 limbs
void launch_exchange_widen(const Fr* a, const Fr* b, uint32_t each, const uint32_t* flag, uint32_t local_flag, long long* limbs, hipStream_t s);
void launch_exchange_narrow(const long long* limbs, Fr* a, Fr* b, uint32_t each, uint32_t* flag_out, hipStream_t s);
// ceilings of the box (gkr_ubench_ceilings): a plain copy, a read-only stream, chains of Montgomery products
void launch_ubench_copy(const void* in, void* out, size_t bytes, hipStream_t s);
void launch_ubench_read(const void* in, void* out, size_t bytes, hipStream_t s);
void launch_ubench_modmul(Fr* io, uint32_t entries_pow2, uint32_t waves, int reps, hipStream_t s);

uint32_t mle_blocks_per_table(uint32_t items, uint32_t batch);
void launch_mle_sum_first(const Fr* tables, size_t stride, uint32_t h, uint32_t batch, uint32_t nblk,
                          MlePartial* partials, hipStream_t s);
void launch_mle_fold_sum(const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                         uint32_t nblk, const FixedMul* rtab, uint32_t r_stride, MlePartial* partials, hipStream_t s);
void launch_mle_round_hash(const MlePartial* partials, uint32_t nblk, uint32_t round, uint32_t n, uint32_t batch,
                           const Fr* cts, Fr* out_coeffs, uint32_t* out_len, Fr* out_r, FixedMul* rtab,
                           uint32_t* dep_last, hipStream_t s);

// ---- sumcheck over a product of `degree` <= kProductMaxDegree resident tables (kernels_product.hip) ----
// One pass leaves per block degree + 1 exact values of the round polynomial (scaled, see the kernels) and, in round 1, the
// factors' flags; one wave per sumcheck and round turns them into the round vector, hashes it and publishes r.
// Launch geometry: mle_blocks_per_table(h or q, batch) blocks per sumcheck, as the plain sumcheck's passes.
constexpr int kProductMaxDegree = 3;
struct ProductPartial {
    Acc<9> s[kProductMaxDegree + 1];
    uint32_t flags, pad[3];
};
// factor f of sumcheck b at tables + (b * degree + f) * table_stride; h = half a table
void launch_product_first(int degree, const Fr* tables, size_t table_stride, uint32_t h, uint32_t batch, uint32_t nblk,
                          ProductPartial* partials, hipStream_t s);
// src: 4q entries per factor, dst: 2q (dst == src with equal strides: in place); rtab[b * r_stride]: r of the round before
void launch_product_fold_sum(int degree, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                             uint32_t nblk, const FixedMul* rtab, uint32_t r_stride, ProductPartial* partials, hipStream_t s);
// out_coeffs: batch x n rows of degree + 1 slots; out_len, out_r, rtab: batch x n; meta: batch words (written in round 0, read
// in round n - 1); evals: batch x degree, written in round n - 1 from the factors' two remaining entries at work + (b * degree +
// f) * work_stride
void launch_product_round(int degree, const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n, uint32_t batch,
                          const Fr* cts, const Fr* work, size_t work_stride, Fr* out_coeffs, uint32_t* out_len, Fr* out_r,
                          FixedMul* rtab, uint32_t* meta, Fr* evals, hipStream_t s);

// ---- sumcheck over a sum of products of resident tables (kernels_sop.hip): g = sum_k c_k prod_j T_{t(k, j)} ----
// The term structure travels as kernel arguments (wave-uniform).  A pass folds each of the n_tables tables once and leaves per
// block and term one ProductPartial (partials: batch x nblk x n_terms); the geometry is the product path's.
constexpr int kSopMaxTables = 8, kSopMaxTerms = 8;
struct SopTerms {
    uint32_t n_tables, n_terms, max_degree;
    uint32_t term[kSopMaxTerms];   // degree | table 0 << 8 | table 1 << 16 | table 2 << 24
};
struct SopCoeffs {
    Fr c[kSopMaxTerms];            // canonical
};
// table m of sumcheck b at tables + (b * n_tables + m) * table_stride; h = half a table
void launch_sop_first(const SopTerms& ts, const Fr* tables, size_t table_stride, uint32_t h, uint32_t batch, uint32_t nblk,
                      ProductPartial* partials, hipStream_t s);
// src: 4q entries per table, dst: 2q (dst == src with equal strides: in place); rtab[b * r_stride]: r of the round before
void launch_sop_fold_sum(const SopTerms& ts, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                         uint32_t nblk, const FixedMul* rtab, uint32_t r_stride, ProductPartial* partials, hipStream_t s);
// out_coeffs: batch x n rows of max_degree + 1 slots; out_len, out_r, rtab: batch x n; evals: batch x n_tables, written in round
// n - 1 from the tables' two remaining entries at work + (b * n_tables + m) * work_stride
void launch_sop_round(const SopTerms& ts, const SopCoeffs& cf, const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n,
                      uint32_t batch, const Fr* cts, const Fr* work, size_t work_stride, Fr* out_coeffs, uint32_t* out_len, Fr* out_r,
                      FixedMul* rtab, Fr* evals, hipStream_t s);

// ---- zero-check sumcheck (kernels_zerocheck.hip): eq(z, .) * sum_k c_k prod_j T_{t(k, j)}, term degrees <= 2, eq never a table ----
// The weights of the variables still free, w_j(i) = E_hi,j[i >> 8] * E_lo[i & 255], as eq tables of launch_eq_table (Montgomery):
// hi table m (m variables in front of the last eight) of all sumchecks at hi + batch * (2^m - 1), sumcheck b at + (b << m);
// lo table k (the last k <= 8 variables) at lo + batch * (2^k - 1).  zc_weight_elements(n, batch) <= batch * (2^(n-8) + 511).
struct ZcWeights {
    Fr *hi, *lo;
    uint32_t batch;
    const Fr* hi_table(uint32_t m) const { return hi + (size_t)batch * ((1u << m) - 1u); }
    const Fr* lo_table(uint32_t k) const { return lo + (size_t)batch * ((1u << k) - 1u); }
};
size_t zc_weight_elements(uint32_t n, uint32_t batch);
ZcWeights zc_weights_layout(Fr* base, uint32_t n, uint32_t batch);
// points: batch x n canonical elements in device (or pinned host) memory
void launch_zc_weights(const Fr* points, uint32_t n, uint32_t batch, const ZcWeights& w, hipStream_t s);
// as launch_sop_first / launch_sop_fold_sum; the round has 2^(kh + kl) entries per half table, kl = min(free variables, 8)
void launch_zc_first(const SopTerms& ts, const Fr* tables, size_t table_stride, uint32_t h, uint32_t batch, uint32_t nblk, const ZcWeights& w,
                     uint32_t kh, uint32_t kl, ProductPartial* partials, hipStream_t s);
void launch_zc_fold_sum(const SopTerms& ts, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                        uint32_t nblk, const FixedMul* rtab, uint32_t r_stride, const ZcWeights& w, uint32_t kh, uint32_t kl,
                        ProductPartial* partials, hipStream_t s);
// out_coeffs: batch x n rows of max_degree + 2 slots; z: batch x n canonical; s_slot: batch elements (s_j, Montgomery); evals
// (batch x n_tables) and eq_out (batch: eq(z, r)) are written in round n - 1
void launch_zc_round(const SopTerms& ts, const SopCoeffs& cf, const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n,
                     uint32_t batch, const Fr* cts, const Fr* z, Fr* s_slot, const Fr* work, size_t work_stride, Fr* out_coeffs,
                     uint32_t* out_len, Fr* out_r, FixedMul* rtab, Fr* evals, Fr* eq_out, hipStream_t s);

// ---- the grand product's tree (kernels_grand_product.hip): L_k[i] = L_{k+1}[i] * L_{k+1}[i + 2^k], every level stored ----
// One launch per level k = n-1 .. 0, gp_level_blocks(k) = ceil(2^k / 256) blocks of 256 threads per table, a thread per product.
uint32_t gp_level_blocks(uint32_t k);
// level k (2^k entries per table) of a batch's trees starts at this element of `layers`, table b at + b * 2^k
__host__ __device__ inline size_t gp_layer_offset(uint32_t level, uint32_t batch) { return (size_t)batch * (((size_t)1 << level) - 1); }
// tables: batch x 2^n canonical values, table b at + b * 2^n, not modified; layers: batch * (2^n - 1) elements, levels 0 .. n-1
void launch_gp_tree(const Fr* tables, uint32_t n, uint32_t batch, Fr* layers, hipStream_t s);

// ---- the fractional sum's tree and round (kernels_fraction_sum.hip): (p, q)_k[i] = (p lo q hi + p hi q lo, q lo q hi) of level k + 1 ----
// One launch per level k = n-1 .. 0, fs_level_blocks(k) = ceil(2^k / 256) blocks of 256 threads per pair, a thread per node.
uint32_t fs_level_blocks(uint32_t k);
// level k (p_k then q_k, 2^k entries each, per pair) of a batch's trees starts at this element of `layers`, pair b at + b * 2^(k+1)
__host__ __device__ inline size_t fs_layer_offset(uint32_t level, uint32_t batch) { return 2 * (size_t)batch * (((size_t)1 << level) - 1); }
// tables: batch pairs (N then D, 2^n canonical values each), pair b at + b * 2^(n+1), not modified; layers: 2 batch (2^n - 1)
// elements, levels 0 .. n-1
void launch_fs_tree(const Fr* tables, uint32_t n, uint32_t batch, Fr* layers, hipStream_t s);
// launch_zc_round for the layer's three terms T0 T3 + T1 T2 + lambda[b] T2 T3 over four tables: lambda: batch canonical elements;
// partials: batch x nblk x 3; out_coeffs: batch x n rows of 4 slots; evals: batch x 4
void launch_fs_round(const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n, uint32_t batch, const Fr* lambda, const Fr* cts,
                     const Fr* z, Fr* s_slot, const Fr* work, size_t work_stride, Fr* out_coeffs, uint32_t* out_len, Fr* out_r, FixedMul* rtab,
                     Fr* evals, Fr* eq_out, hipStream_t s);

// ---- the lookup argument's preparation (kernels_lookup.hip): the table's index, the multiplicities, the pair (N, D) ----
// Every launch: blocks of 256 threads, a thread per item, lk_blocks(log2 items) = ceil(2^log2 / 256) blocks per table / column / pair.
uint32_t lk_blocks(uint32_t log2_items);
// index: tables x 2^(n_t+1) words, all 0xFFFFFFFF before the launch; table t at + t * 2^n_t
void launch_lk_build(const Fr* table, uint32_t n_t, uint32_t tables, uint32_t* index, hipStream_t s);
// counts: batch x 2^n_t words and missing: batch words, zero before the launch; first_missing: batch words, 0xFFFFFFFF before it;
// witness column b at + b * 2^n_w; shared_table: one table and one index for every column
void launch_lk_count(const Fr* witness, uint32_t n_w, const Fr* table, uint32_t n_t, bool shared_table, const uint32_t* index, uint32_t batch,
                     uint32_t* counts, uint32_t* missing, uint32_t* first_missing, hipStream_t s);
// mult: batch x 2^n_t canonical elements
void launch_lk_mult(const uint32_t* counts, uint32_t n_t, uint32_t batch, Fr* mult, hipStream_t s);
// pair: batch x 2 x 2^L elements (N then D), L = max(n_w, n_t) + 1; alpha: batch canonical elements in device memory
void launch_lk_pair(const Fr* witness, uint32_t n_w, const Fr* table, uint32_t n_t, bool shared_table, const Fr* mult, const Fr* alpha, uint32_t L,
                    uint32_t batch, Fr* pair, hipStream_t s);

void launch_layer_eval(uint32_t gates, const uint8_t* gate_type, const uint32_t* left, const uint32_t* right,
                       const Fr* prev, Fr* out, uint32_t batch, uint32_t prev_stride, hipStream_t s, const GateSet* sets = nullptr);
// words 32-bit words src -> dst (16-byte aligned when words >= 4); either side may be pinned host memory
void launch_copy_words(const void* src, void* dst, size_t words, hipStream_t s);
// rows x words: row r from src + r * src_stride_words to dst + r * dst_stride_words (32-bit words)
void launch_copy_rows(const void* src, size_t src_stride_words, void* dst, size_t dst_stride_words, uint32_t words, uint32_t rows, hipStream_t s);
// out[proof][g] = eq(points[proof * stride + first ..+nvars), g), nvars <= 28; points may be pinned host memory
// wu_job / wu_out (both or neither): the launch also leaves W(u) = sum_{i < 2^jp} Wb[i] * weights[i] of every proof (Montgomery;
// k_prod_c_setup's scalar) in wu_out[proof] -- the wide layers' row pass writes the c-phase's tables with it (WideCFuse)
void launch_eq_table(const Fr* points, uint32_t stride, uint32_t first, uint32_t nvars, Fr* out, bool montgomery, uint32_t batch,
                     hipStream_t s, const CPhaseFuse* wu_job = nullptr, Fr* wu_out = nullptr, uint32_t wstride = 0);
// one launch for a layer's set-up: E_hi (canonical, kh leading coordinates of the proof's point), E_lo (Montgomery, kl
// trailing ones), the two Montgomery copies of W (Wb null: none) and the 32 dependence flags per proof, in dep and -- when not null -- in
// pinned host memory host_dep (k_layer_prologue)
void launch_layer_prologue(const Fr* points, uint32_t k_i, uint32_t kh, uint32_t kl, Fr* e_hi, Fr* e_lo, const Fr* W, Fr* Wb, Fr* Wc,
                           uint32_t k, uint32_t* dep, uint32_t* host_dep, uint32_t batch, hipStream_t s, uint32_t* wide_bits = nullptr);
// q(t) = W(b + t (c - b)) per proof: W batch x 2^k, bc batch x 2k (b then c), scratch batch x 3 * 2^k, deg_scratch batch
// words (device), out batch x (k + 1) highest degree first, out_len batch
// bcm: batch * 2k elements of device scratch (the line's coefficients in Montgomery form; unused for k <= 9)
// part (layers of more than 2^12 values only; smaller ones ignore it and must be called with `all`): `prepare` issues what needs
// W alone (the copy, the Moebius transform, the largest degree), `finish` the rest (the line's coefficients, the steps, q).
enum class LinePart { all, prepare, finish };
void launch_line_restriction(const Fr* W, uint32_t k, const Fr* bc, Fr* scratch, uint32_t* deg_scratch, Fr* bcm, Fr* out, uint32_t* out_len,
                             uint32_t batch, hipStream_t s, LinePart part = LinePart::all);

// ---- wide layers (kernels_wide.hip): next-layer tables of 2^14 values and more -------------------------------------------
// The gate passes over ITEMS: the buckets of the sorted lists cut into pieces of at most sixteen gates, sorted by length, a
// lane per item; eq(z, .) gathered from a materialised 2^k_i-entry table E (canonical).  The plan (items, their order, the
// step-major entries) is built once per circuit layer by launch_gate_plan, right after the sort.
constexpr uint32_t kWideMinK = 13;        // layers with k_next >= this take the item passes
size_t gate_plan_words(uint64_t gates, uint32_t k);             // u32 words of the plan (both halves)
size_t gate_plan_partial_elems(uint64_t gates, uint32_t k);     // Fr elements of pass scratch per proof
void launch_gate_plan(GateSpan span, uint32_t k, const uint32_t* offsets, const uint32_t* cursor, const uint32_t* list, uint32_t* plan, hipStream_t s);
// eq(z, .) for the passes: E (batch x 2^k_i entries, canonical) when materialised, else null and the two half tables of the
// layer's prologue (e_hi canonical, batch x 2^(k_i - kl); e_lo_mont Montgomery, batch x 2^kl): one reduced product per gate.
// W / eq_mont: batch tables of 2^k entries in Montgomery form (stride lb.wstride).
struct GateEq {
    const Fr* E;
    const Fr* e_hi;
    const Fr* e_lo_mont;
    uint32_t kl;
};
// eq(z, g) per gate: gathered from the materialised 2^k_i-entry table up to 2^20 gates (32 MiB per proof), formed from the two
// half tables (one reduced product per gate, both halves cache-resident) beyond.  Same-box A/B, ms of gate passes + table
// build per sumcheck, table / halves (profiles/r06/e_wide_eq_source_*): (20,15) 0.113 / 0.134, (20,20) 0.174 / 0.155, circom-
// shaped (20,20) 0.195 / 0.204, (21,16) 0.184 / 0.153, (21,21) 0.327 / 0.288, (22,16) 0.306 / 0.238, (22,22) 0.697 / 0.575 -- the
// table's random 32-byte reads move 128-byte lines, and from 64 MiB on that costs more than the product (round 5 kept the table
// up to k_i = 22, while it stays in the 256 MiB Infinity Cache).
constexpr uint32_t kGateEqTableMaxKi = 20;
// The plan's counts as the host read them back when the plan was built (hdr[half]: [1] groups, [2] buckets of 2 .. 64 items, [3]
// buckets of more, [5] their chunks): exact grids, and no combine launch for a half whose buckets are all one item.  In a lockstep
// group: the largest count over the members.
struct GatePlanCounts {
    uint32_t hdr[2][8];
    bool known;
};
size_t gate_plan_arrive_words(uint64_t gates, uint32_t k);     // zeroed u32 counters per proof (the combine step's long buckets)
void gate_plan_counts_offsets(uint64_t gates, uint32_t k, size_t* half1_word_offset);   // where the second half's header starts in the plan
void launch_gate_uv_wide(GateSpan span, uint32_t k_i, uint32_t k, const uint32_t* plan, const GateEq& eq, const Fr* W, Fr* U, Fr* V, LayerBatch lb, Fr* partials,
                         uint32_t* arrive, hipStream_t s, const GateSet* sets = nullptr, const GatePlanCounts* counts = nullptr);
// fuse (may be null): the rows are not written; every bucket's (a_u, m_u) goes straight into the c-phase's tables
// X = a_u + W(u) m_u, Y = W(u) a_u (k_prod_c_setup's arithmetic: one launch and 64 B of traffic per bucket less per sumcheck)
struct WideCFuse {
    const Fr* wu = nullptr;   // W(u) per proof, Montgomery, device memory (launch_eq_table's wu_out)
    Fr* X = nullptr;
    Fr* Y = nullptr;
};
void launch_gate_rows_wide(GateSpan span, uint32_t k_i, uint32_t k, const uint32_t* plan, const GateEq& eq, const Fr* eq_mont, Fr* A_row, Fr* M_row, LayerBatch lb,
                           Fr* partials, uint32_t* arrive, hipStream_t s, const GateSet* sets = nullptr, const GatePlanCounts* counts = nullptr,
                           const WideCFuse* fuse = nullptr);
// E (batch x 2^k_i, canonical) = the outer product of the prologue's half tables (e_hi canonical, e_lo_mont Montgomery, split at kl)
void launch_eq_outer(const Fr* e_hi, const Fr* e_lo_mont, uint32_t k_i, uint32_t kl, Fr* E, uint32_t batch, hipStream_t s);
// exclusive scan of n 32-bit counts (block_sums: n / 2048 + 1 words of scratch)
void launch_exclusive_scan(const uint32_t* in, uint32_t* out, uint32_t* block_sums, size_t n, hipStream_t s);
// *flag |= 1 if some entry of t[0 .. n) is >= r (flag zeroed by the caller)
void launch_check_canonical(const Fr* t, size_t n, uint32_t* flag, hipStream_t s);
// dependence flags over a grid: bits = one word of scratch per proof, zeroed by the launcher unless `bits_preset` (the layer's
// prologue stored what a first look found: launch_layer_prologue's wide_bits); dep / host_dep as launch_layer_prologue
void launch_depends_wide(const Fr* W, uint32_t k, uint32_t* bits, uint32_t* dep, uint32_t* host_dep, uint32_t batch, hipStream_t s, bool bits_preset = false);
// in-place Moebius transform (evaluations -> monomial coefficients, MSB-first) of `batch` tables of 2^k, `stride` apart
void launch_mobius(Fr* tables, uint32_t k, size_t stride, uint32_t batch, hipStream_t s);
void launch_line_setup_wide(const Fr* W, uint32_t k, Fr* scratch, uint32_t* maxdeg_scratch, uint32_t batch, hipStream_t s);

// ---- one plain sumcheck split over ranks (kernels_wide.hip): the per-pass exchange of the sub-block sums and the final gather
// rec: the pass's records in DEVICE memory; limbs: batch x (2^J + 2) x 8 int64 (sums | dep | fail per table)
void launch_mle_xwiden(const MleHostRecSub* rec, uint32_t J, uint32_t batch, uint32_t local_fail, long long* limbs, hipStream_t s);
void launch_mle_xnarrow(const long long* limbs, uint32_t J, uint32_t batch, MleHostRecSub* host_rec, uint32_t ticket, uint32_t* fail_out,
                        hipStream_t s);
// the 2^t entries every shard has left -> the tail table of 2^(t + lp) entries (limbs: batch x 2^(t+lp) x 8 + 8 int64)
void launch_mle_gather_widen(const Fr* src, size_t stride, uint32_t t, uint32_t lp, uint32_t shard, uint32_t local_fail, uint32_t batch,
                             long long* limbs, hipStream_t s);
void launch_mle_gather_narrow(const long long* limbs, uint32_t tn, uint32_t batch, Fr* tail, uint32_t* fail_out, hipStream_t s);
void launch_to_mont(const Fr* in, Fr* out, uint32_t count, hipStream_t s);
void launch_depends(const Fr* W, uint32_t k, uint32_t* dep, uint32_t batch, hipStream_t s);
void launch_predicate_scatter(uint32_t k_i, uint32_t k_next, const uint8_t* gate_type, const uint32_t* left,
                              const uint32_t* right, const Fr* e_hi, const Fr* e_lo_mont, uint32_t kl,
                              unsigned long long* wideA, unsigned long long* wideM, uint32_t* bad, uint32_t log_p,
                              uint32_t shard, hipStream_t s);
void launch_to_mont_strided(const Fr* in, Fr* out, uint32_t count, uint32_t stride, uint32_t offset, hipStream_t s);
void launch_tables_differ(const Fr* a, const Fr* b, size_t count, uint32_t* flag, hipStream_t s);
void launch_fold_pair(const Fr* src, Fr* dst, const FixedMul* rtab, hipStream_t s);
void launch_predicate_sorted(uint32_t k_i, uint32_t k_next, const uint8_t* gate_type, const uint32_t* left,
                             const uint32_t* right, const Fr* e_hi, const Fr* e_lo_mont, uint32_t kl, uint32_t log_p,
                             uint32_t shard, size_t ncells, uint32_t* counts, uint32_t* offsets, uint32_t* cursor,
                             uint32_t* block_sums, uint32_t* list, uint32_t* bad, Fr* out_A, Fr* out_M, uint32_t batch,
                             hipStream_t s);
void launch_predicate_normalise(const unsigned long long* wide, Fr* out, size_t cells, hipStream_t s);

// ---- device verifier (kernels_verify.hip) ------------------------------------------------------------------------------------
// prepare: gate arrays of 2^k_i gates -> packed records {left | type << 31, right}; *bad |= 1 (zeroed by the caller) on an
// operand >= 2^k or a type > 1
void launch_verify_pack(const uint8_t* gate_type, const uint32_t* left, const uint32_t* right, uint32_t gates, uint32_t k, uint2* packed,
                        uint32_t* bad, hipStream_t s);
// One layer of the wiring pass, as the launch over all layers and proofs of a chunk reads it from device memory: the packed
// gates and the chunk's tables of this layer (all Montgomery; proof p's table at base + (p << log2 entries)): eq(z_i, .) as the
// half tables e_hi (k_i - kl leading variables) and e_lo (kl trailing ones), eq(b*, .) and eq(c*, .) of 2^k entries.
struct VerifyLayer {
    const uint2* gates;
    const Fr* e_hi;
    const Fr* e_lo;
    const Fr* eq_b;
    const Fr* eq_c;
    uint32_t k_i, kl, k, pad;
};
static_assert(sizeof(VerifyLayer) == 56, "layer table entry");
uint32_t verify_wiring_blocks(uint32_t max_k_i);   // blocks per (layer, proof) of the wiring pass
// out[(proof * n_layers + layer) * 2 + (0 add | 1 mult)] = the wiring predicate at (z, b*, c*), Montgomery; partials: batch x
// n_layers x 2 x verify_wiring_blocks(max_k_i) elements of scratch.  One launch for the pass, one for the second-level sums.
void launch_verify_wiring(const VerifyLayer* layers, uint32_t n_layers, uint32_t max_k_i, uint32_t batch, Fr* partials, Fr* out, hipStream_t s);
// flags[p * flag_stride] |= 1 when proof p's table (2^k coefficients, proofs contiguous) holds an element >= r.  One launch.
void launch_verify_canonical(const Fr* coeffs, uint32_t k, uint32_t* flags, uint32_t flag_stride, uint32_t batch, hipStream_t s);
uint32_t verify_mono_blocks(uint32_t k);
// out[proof] = sum_S coeffs[proof][S] prod_{j in S} x_j (canonical) for `batch` tables of 2^k monomial coefficients (index
// MSB-first), x = points[proof * stride + first ..+k) canonical.  t_hi: batch x 2^(k - k/2), t_lo: batch x 2^(k/2), partials:
// batch x verify_mono_blocks(k) elements of scratch.
void launch_verify_mono_eval(const Fr* points, uint32_t stride, uint32_t first, uint32_t k, const Fr* coeffs, Fr* t_hi, Fr* t_lo, Fr* partials,
                             Fr* out, uint32_t batch, hipStream_t s);
// ---- the verifier's challenge hashes (kernels_verify_hash.hip) -----------------------------------------------------------------
// One row's result: the canonical hash as eight little-endian limbs and whether the row was well-formed (36 bytes written, 40
// with the padding of capi_verify.hip's HashSlot {gkr_fr, uint32_t}, whose layout this is: the relations read what the kernel
// wrote without a conversion).
struct VerifyHashSlot {
    uint32_t h[8];
    uint32_t valid;
    uint32_t pad;
};
static_assert(sizeof(VerifyHashSlot) == 40, "hash slot");
// out[i] = {multi_hash(row i's trailing len[i] slots, key 0), 1} for n >= 1 rows of `slots` (3 or 4) right-aligned slots (8 * slots
// words per row; 3: the layout of gkr_proof_buf.sumcheck_coeffs, 4: the degree-3 product sumcheck's rows); {0, 0} when len[i] is
// outside 1 .. slots or a used slot holds an element >= r (an unused leading slot is never looked at).  cts: the 91 round
// constants in Montgomery form.  Eight lanes per row, one launch.
void launch_verify_hash(int slots, const uint32_t* rows, const uint32_t* len, uint32_t n, const Fr* cts, VerifyHashSlot* out, hipStream_t s);

// ---- multilinear evaluation at a point (kernels_mle_eval.hip) ---------------------------------------------------------------------
// The streaming matrix-core form binds five variables per pass over 2^(n-5) outputs in wave tiles of 64: it applies from
// kMleEvalMfmaValidN on.  From kMleEvalMfmaMinN on it is used (option mle_eval_mfma_min_n overrides; below, one block per table
// does the whole sum: one launch instead of six, and a table of 2^12 entries is 16 entries per thread).  Above kMleEvalSmallMaxN the
// streaming form is used whatever the option says: one block walking a table of gigabytes would hold the device for minutes.
constexpr uint32_t kMleEvalMfmaValidN = 11, kMleEvalMfmaMinN = 13, kMleEvalSmallMaxN = 24;
bool mle_eval_uses_mfma(uint32_t n);
uint32_t mle_eval_blocks(uint32_t n, uint32_t batch);      // blocks per table of the streaming form
size_t mle_eval_ws_bytes(uint32_t n, uint32_t groups, uint32_t G);   // device workspace of one launch_mle_eval
// groups x G tables of 2^n entries, 1 <= n <= 30; the G tables of a group share a point (G = 1: every table its own):
// out[t] = sum_i eq(points[g * n ..+n), i) tables[(t << n) + i] (canonical) for t = g G + m, m < G.  points: groups x n canonical
// elements in device memory, variable 1 = most significant index bit.  What depends on the point alone is built once per group;
// every value is bit for bit the one G = 1 gives with the point repeated.  ws: mle_eval_ws_bytes().
void launch_mle_eval(const Fr* tables, uint32_t n, uint32_t groups, uint32_t G, const Fr* points, void* ws, Fr* out, hipStream_t s);

// ---- the R1CS zero-check's tables (kernels_r1cs.hip) -------------------------------------------------------------------------------
// The three matrices of an R1CS in CSR form, resident: matrix m's n_constraints + 1 row offsets, its records {x: wire, y: pool
// index}, the ascending list of its rows with more than kR1csLongRow records; the coefficient pool in Montgomery form (entries
// 0 and 1, one and r - 1, are never read).  Tables of 2^n entries.
constexpr uint32_t kR1csLongRow = 32;   // (= GKR_R1CS_LONG_ROW: the host's long-row lists are cut at the same length)
struct R1csCsr {
    const uint32_t* row_ptr[3];
    const uint2* terms[3];
    const uint32_t* long_rows[3];
    uint32_t n_long[3];
    const Fr* pool_mont;
    uint32_t n_constraints, n;
};
// out[(b * 3 + m) * 2^n + i] = row i of matrix m times witness b (witness + b * witness_stride elements, canonical), canonical;
// rows >= n_constraints zero.  One launch over all rows, one more over the long rows where a matrix has any.
void launch_r1cs_rows(const R1csCsr& csr, const Fr* witness, size_t witness_stride, uint32_t batch, Fr* out, hipStream_t s);
// first_bad[b] = the lowest row < n_constraints of sumcheck b's tables (a, b, c at (b * 3 + m) * 2^n) with a * b != c, UINT32_MAX if none
hipError_t launch_r1cs_check(const Fr* tables, uint32_t n, uint32_t n_constraints, uint32_t batch, uint32_t* first_bad, hipStream_t s);

// ---- the R1CS inner sumcheck's table (kernels_r1cs.hip) ----------------------------------------------------------------------------
// The three matrices in column-major form, resident: matrix m's n_wires + 1 column offsets and its records {x: row, y: pool
// index}; the pool in Montgomery form.  A column of more than kR1csLongCol records of a matrix is cut into segments of at most
// kR1csColSegment records (the host's lists): segs[s] = {x: column, y: matrix, z: first record, w: one past the last}, sorted by
// column, so that the segments of one column -- of all three matrices -- are neighbours; comb_cols[k] is the k-th column that has
// any, comb_ptr[k] .. comb_ptr[k + 1] its segments.  Tables of 2^n_y entries.
constexpr uint32_t kR1csLongCol = 32;        // (= GKR_R1CS_LONG_COL)
constexpr uint32_t kR1csColSegment = 2048;   // (= GKR_R1CS_COL_SEGMENT)
struct R1csCsc {
    const uint32_t* col_ptr[3];
    const uint2* terms[3];
    const Fr* pool_mont;
    const uint4* segs;
    const uint32_t* comb_cols;
    const uint32_t* comb_ptr;
    uint32_t n_segs, n_comb, n_wires, n_y;
};
// out[b * out_stride + y] = sum_m rho_{b,m} sum_{records (i, c) of column y of matrix m} pool[c] * eq[b << n_x | i], canonical, for
// y < 2^n_y; zero for y >= n_wires.  eq: batch canonical tables of 2^n_x entries; rho_mont: batch x 3, Montgomery; partials:
// batch * n_segs elements of scratch (unused without segments).  Three launches in stream order: a thread per column, a wave per
// segment, a wave per column that has segments.
void launch_r1cs_cols(const R1csCsc& csc, const Fr* eq, uint32_t n_x, const Fr* rho_mont, uint32_t batch, Fr* partials, Fr* out,
                      size_t out_stride, hipStream_t s);
// dst[b * dst_stride + y] = y < n_wires ? witness[b * witness_stride + y] : 0 for y < 2^n_y (the witness as a factor of the product path)
void launch_r1cs_pad_witness(const Fr* witness, size_t witness_stride, uint32_t n_wires, uint32_t n_y, uint32_t batch, Fr* dst,
                             size_t dst_stride, hipStream_t s);

// ---- the R1CS verifier's last relation (kernels_r1cs.hip) --------------------------------------------------------------------------
// out[b * 3 + m] = M_m~(x_b, y_b) = sum over the records (row i, wire w, coefficient c) of matrix m of c eq(x_b, i) eq(y_b, w),
// canonical, from the resident CSR form in one pass: ex_mont = batch tables eq(x_b, .) of 2^n entries in MONTGOMERY form, ey =
// batch tables eq(y_b, .) of 2^n_y >= n_wires entries, canonical (launch_eq_table's two forms).  partials: batch * 3 *
// r1cs_matrix_eval_slots(csr) elements of scratch, every one written before it is read.  Three launches in stream order (two
// where no matrix has a long row): a thread per row, a wave per long row, a block per (matrix, proof).
uint32_t r1cs_matrix_eval_slots(const R1csCsr& csr);
void launch_r1cs_matrix_evals(const R1csCsr& csr, const Fr* ex_mont, const Fr* ey, uint32_t n_y, uint32_t batch, Fr* partials, Fr* out,
                              hipStream_t s);

uint32_t layer_blocks(uint32_t h);
// The grid of the fused b-phase round (launch_layer_round_b) over hb row pairs of 2^kc columns: ~1024 blocks per table over the
// whole batch, every block at least one row pair.  grid = (col_blocks, chunks * batch, 2); partials = the slots one proof writes.
// Host arithmetic only: the launch and gkr_selftest_layer_dense_geometry both call it.
struct LayerRoundBGrid {
    uint32_t col_blocks, chunks, rows_per_chunk, partials;
};
inline LayerRoundBGrid layer_round_b_grid(uint32_t hb, uint32_t kc, uint32_t batch) {
    LayerRoundBGrid g;
    g.col_blocks = ((1u << kc) + 255u) / 256u;
    uint32_t chunks = 1024u / (g.col_blocks * batch);
    if (chunks < 1) chunks = 1;
    if (chunks > hb) chunks = hb;
    g.rows_per_chunk = (hb + chunks - 1) / chunks;
    g.chunks = (hb + g.rows_per_chunk - 1) / g.rows_per_chunk;
    g.partials = g.col_blocks * g.chunks * 2;
    return g;
}
uint32_t layer_fold_blocks(uint32_t h, uint32_t batch);   // blocks per proof of k_layer_fold over h pairs
uint32_t pred_scan_blocks(size_t n);                      // blocks of k_scan_blocks / k_scan_add over n counters (launch_predicate_sorted)
uint32_t pred_sum_blocks(size_t n);                       // blocks per proof of k_pred_sum over n cells
void launch_layer_round(const Fr* A, const Fr* M, uint32_t h, uint32_t k, uint32_t phase, uint32_t hb, const Fr* Wb,
                        const Fr* Wc, uint32_t nblk, LayerPartial* partials, LayerBatch lb, hipStream_t s);
uint32_t launch_layer_round_b(bool fold, const Fr* A_src, const Fr* M_src, Fr* A_dst, Fr* M_dst, uint32_t hb, uint32_t kc,
                              const FixedMul* rtab, const Fr* Wb, const Fr* Wc, LayerPartial* partials, LayerBatch lb,
                              hipStream_t s);
void launch_layer_fold(Fr* A, Fr* M, uint32_t h, const FixedMul* rtab, LayerBatch lb, hipStream_t s);
void launch_layer_round_hash(const LayerPartial* partials, uint32_t nblk, uint32_t round, uint32_t k,
                             const uint32_t* dep, const Fr* cts, Fr* out_coeffs, uint32_t* out_len, Fr* out_r,
                             FixedMul* rtab, Fr* Wb, Fr* Wc, hipStream_t s);

}  // namespace gkr
