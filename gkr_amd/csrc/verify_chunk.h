// The pieces every batch verifier builds a chunk of proofs from: capi_verify.hip (whole GKR proofs), capi_mle_verify.hip (the plain,
// product and sum-of-products sumchecks), capi_r1cs_verify.hip and tree_argument.h's one chunk verifier of the grand product and
// the fractional sum (capi_grand_product.hip, capi_fraction_sum.hip).  All of them follow one plan per chunk --
// hash the round vectors, on the side stream or on the host threads; run the relations that need neither a hash nor a device
// value; read the tables once on the device; synchronise ONCE; decide a verdict per proof -- and each calls these pieces in an
// order of its own, which is what its overlap of host and device rests on:
//   verify_chunk_size, for_chunks    how many proofs fit verify_workspace_mb, and the loop over a call's chunks;
//   for_pieces (hostpool.h: PieceJob, its two-step form)    host work in numbered pieces on this thread and the context's pool;
//   RowSet, RoundHashes              the hash slots of a chunk's round vectors, from the device or from the host;
//   queue_eval                       points up, launch_mle_eval, values down, on the main stream.
// Not a public header.
#pragma once
#include "capi_internal.h"

namespace gkr_host {

// ---- chunks

// Items (proofs, sumchecks) of a chunk: what fits verify_workspace_mb (0: 2 GiB) at bytes_per_item, at most `cap` (the item is a
// grid dimension of the launches) and at least one.  The price of an item is its caller's; verdicts do not depend on the chunking.
inline size_t verify_chunk_size(size_t bytes_per_item, size_t cap, int batch) {
    long long mb = gkr::opt(gkr::OPT_verify_workspace_mb);
    if (mb <= 0) mb = 2048;
    return std::max<size_t>(1, std::min<size_t>({((size_t)mb << 20) / bytes_per_item, cap, (size_t)batch}));
}
// fn(b, nb) for every chunk [b, b + nb) of a batch, up to the first status that is not GKR_OK
template <class Fn>
int for_chunks(int batch, size_t chunk, Fn&& fn) {
    for (size_t b = 0; b < (size_t)batch; b += chunk)
        if (const int rc = fn(b, (uint32_t)std::min(chunk, (size_t)batch - b))) return rc;
    return GKR_OK;
}

// ---- host work in pieces

// piece(a) once for every a < pieces, on the calling thread and -- from pool_from pieces on: waking the pool is worth some tens
// of hashes or transcripts -- on the context's host threads; returns when all have been run to their end
template <class Piece>
void for_pieces(gkr_ctx* ctx, size_t pieces, size_t pool_from, Piece&& piece) {
    gkr::PieceJob job(pieces >= pool_from ? ctx->host_pool() : nullptr, pieces, std::forward<Piece>(piece));
    job.drain();
}

// ---- the hashes of a chunk's round vectors

// Smallest number of round vectors in a chunk that are hashed on the device when verify_device_hash_min is 0; 0: never.
// Measured (profiles/r08, tools/bench_verify.py --hash both --sweep: the demo circuit k = [5,6,7,7,7,7], 68 vectors per proof,
// MI355X, 16 host CPUs, median (interquartile range) of 20 alternating calls, ms):
//     vectors      68     136     272     544    1088    4352   17408   69632  278528
//     host      0.305   0.318   0.499   0.761   1.616   4.826  18.411  70.622 285.474
//     device    0.483   0.489   0.518   0.563   0.630   1.058   2.960  10.478  59.930
// From 544 vectors on, at every larger point, the device median is below the host median by more than the sum of the two
// interquartile ranges (at 272: 0.019 ms in favour of the host); rounded up to a power of two.
constexpr long long kVerifyDeviceHashMinRows = 1024;
constexpr size_t kHashLaunchRows = (size_t)1 << 24;   // rows per launch: the grid stays far below 2^31 blocks
constexpr double kHashRowBytes = 96.0 + 4.0 + 36.0;   // a row of three slots in, its length, hash and valid word out
constexpr size_t kHashPiece = 16;                     // round vectors per piece of host hashing

inline bool verify_device_hash_wanted(size_t rows) {
    long long min_rows = gkr::opt(gkr::OPT_verify_device_hash_min);
    if (min_rows == 0) min_rows = kVerifyDeviceHashMinRows;
    return min_rows > 0 && rows >= (size_t)min_rows;
}

// THE launcher of the hash kernel: n rows of `slots` (3 or 4) right-aligned slots and their lengths, in device memory -> their
// hash slots in device memory, on stream s
inline int verify_hash_rows_device(gkr_ctx* ctx, int slots, const uint32_t* d_rows, const uint32_t* d_len, size_t n, gkr::VerifyHashSlot* d_slots,
                                   hipStream_t s) {
    const size_t row_words = (size_t)slots * 8;
    for (size_t a = 0; a < n; a += kHashLaunchRows) {
        const size_t m = std::min(kHashLaunchRows, n - a);
        {
            Timed t(ctx, "verify_hash", (double)m * (kHashRowBytes + 32.0 * (slots - 3)), s);
            gkr::launch_verify_hash(slots, d_rows + a * row_words, d_len + a, (uint32_t)m, ctx->d_cts, d_slots + a, s);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    return GKR_OK;
}

static_assert(sizeof(gkr::verify::HashSlot) == sizeof(gkr::VerifyHashSlot) &&
                  offsetof(gkr::verify::HashSlot, valid) == offsetof(gkr::VerifyHashSlot, valid),
              "the kernel writes the slots the relations read");
static_assert(gkr::verify::kMaxRowWidth == 4, "the hash kernel has rows of three and of four slots");

// A run of round vectors of one width in the caller's arrays: spans of rows_per_span rows each (equal lengths: the span of a row
// is a division), every row `width` right-aligned slots, 2 .. 4, as the caller stores them.
struct RowSet {
    struct Span {
        const gkr_fr* coeffs;
        const uint32_t* len;
    };
    uint32_t width = 0;
    size_t rows_per_span = 0;
    std::vector<Span> spans;
    size_t rows() const { return rows_per_span * spans.size(); }
    size_t kernel_width() const { return std::max<size_t>(3, width); }   // the hash kernel's rows have three slots or four
};

// The hash slots of a chunk's round vectors, in the order set, span, row.  A chunk of at least verify_device_hash_min round
// vectors has them from the device (start(): k_verify_hash on the context's side stream, beside whatever the caller queues on the
// main stream), a smaller one from the host (hash_piece(a) for a < host_pieces(), the caller's to run through for_pieces).  Both
// fill the same slots by the same rule (verify_rounds.h: hash_slot; the kernel restates it), so verdicts do not depend on where
// the hashes ran.
//
// The side stream's work is joined on EVERY way out of the chunk: nothing may still read or write a workspace or a pinned buffer
// the next chunk or call reuses.  The good way out is join(), which makes the main stream wait for the side stream's last event,
// and then sync_main(), the chunk's one synchronisation; on every other way the destructor synchronises the side stream itself.
class RoundHashes {
   public:
    // prefix: of the workspace and pinned slots *hash_in and *hash_out
    RoundHashes(gkr_ctx* ctx, const char* prefix, std::vector<RowSet> sets) : ctx_(ctx), prefix_(prefix), sets_(std::move(sets)) {
        for (const RowSet& s : sets_) rows_ += s.rows();
        device_ = verify_device_hash_wanted(rows_);
        if (!device_) host_slots_.resize(rows_);
        slots_ = host_slots_.data();
    }
    ~RoundHashes() {
        if (forked_) (void)hipStreamSynchronize(forked_);
    }
    RoundHashes(const RoundHashes&) = delete;
    RoundHashes& operator=(const RoundHashes&) = delete;

    size_t rows() const { return rows_; }
    const gkr::verify::HashSlot* slots() const { return slots_; }   // (the device's: filled once sync_main() has returned)

    // host side: pieces of kHashPiece rows; none where the device hashes
    size_t host_pieces() const { return device_ ? 0 : (rows_ + kHashPiece - 1) / kHashPiece; }
    void hash_piece(size_t a) {
        size_t s = a * kHashPiece;
        const size_t end = std::min(rows_, s + kHashPiece);
        size_t first = 0;   // of the set s lies in
        for (const RowSet& set : sets_) {
            for (const size_t set_end = first + set.rows(); s < std::min(end, set_end); ++s) {
                const RowSet::Span& span = set.spans[(s - first) / set.rows_per_span];
                const size_t row = (s - first) % set.rows_per_span;
                host_hash_slot(span.coeffs + set.width * row, set.width, span.len[row], &host_slots_[s]);
            }
            first += set.rows();
        }
    }

    // device side (nothing to do where the host hashes): all rows, then all lengths, in ONE staging buffer; the side stream is
    // forked from the main stream, takes one copy up, one launch per maximal run of sets of one kernel width and one copy of the
    // slots down into pinned memory, and records the event join() waits for.  Rows narrower than the kernel's get leading zero
    // words, which the kernel never looks at for len <= width.
    int start() {
        if (!device_) return GKR_OK;
        size_t row_words = 0;
        for (const RowSet& s : sets_) row_words += s.rows() * s.kernel_width() * 8;
        const size_t words = row_words + rows_;
        const std::string in = prefix_ + "hash_in", out = prefix_ + "hash_out";
        uint32_t *d_in = nullptr, *h_in = nullptr;
        gkr::VerifyHashSlot *d_out = nullptr, *h_out = nullptr;
        WS_OR_NOMEM(ctx_, in.c_str(), uint32_t, words, d_in);
        WS_OR_NOMEM(ctx_, out.c_str(), gkr::VerifyHashSlot, rows_, d_out);
        HIP_TRY(ctx_, ctx_->pinned_host(in.c_str(), words * sizeof(uint32_t), reinterpret_cast<void**>(&h_in)));
        HIP_TRY(ctx_, ctx_->pinned_host(out.c_str(), rows_ * sizeof(gkr::VerifyHashSlot), reinterpret_cast<void**>(&h_out)));
        uint32_t *h_row = h_in, *h_len = h_in + row_words;
        for (const RowSet& s : sets_) {
            const size_t hw = s.kernel_width() * 8, lead = hw - (size_t)s.width * 8;
            for (const RowSet::Span& span : s.spans) {
                if (lead == 0) {
                    memcpy(h_row, span.coeffs, s.rows_per_span * hw * sizeof(uint32_t));
                } else {
                    for (size_t r = 0; r < s.rows_per_span; ++r) {
                        memset(h_row + r * hw, 0, lead * sizeof(uint32_t));
                        memcpy(h_row + r * hw + lead, span.coeffs + s.width * r, s.width * sizeof(gkr_fr));
                    }
                }
                memcpy(h_len, span.len, s.rows_per_span * sizeof(uint32_t));
                h_row += s.rows_per_span * hw;
                h_len += s.rows_per_span;
            }
        }
        HIP_TRY(ctx_, ctx_->aux_stream(2));
        const hipStream_t aux = ctx_->aux;
        HIP_TRY(ctx_, hipEventRecord(ctx_->aux_events[0], ctx_->stream));   // fork: after whatever the main stream still holds
        HIP_TRY(ctx_, hipStreamWaitEvent(aux, ctx_->aux_events[0], 0));
        forked_ = aux;
        HIP_TRY(ctx_, hipMemcpyAsync(d_in, h_in, words * sizeof(uint32_t), hipMemcpyHostToDevice, aux));
        size_t word = 0, row = 0;
        for (size_t i = 0; i < sets_.size();) {
            const size_t kw = sets_[i].kernel_width();
            size_t n = 0;
            for (; i < sets_.size() && sets_[i].kernel_width() == kw; ++i) n += sets_[i].rows();
            if (const int rc = verify_hash_rows_device(ctx_, (int)kw, d_in + word, d_in + row_words + row, n, d_out + row, aux)) return rc;
            word += n * kw * 8;
            row += n;
        }
        HIP_TRY(ctx_, hipMemcpyAsync(h_out, d_out, rows_ * sizeof(gkr::VerifyHashSlot), hipMemcpyDeviceToHost, aux));
        HIP_TRY(ctx_, hipEventRecord(ctx_->aux_events[1], aux));
        slots_ = reinterpret_cast<const gkr::verify::HashSlot*>(h_out);
        return GKR_OK;
    }
    // the main stream's end becomes the side stream's too: in front of the caller's last copy back
    int join() {
        if (forked_) HIP_TRY(ctx_, hipStreamWaitEvent(ctx_->stream, ctx_->aux_events[1], 0));
        joined_ = forked_ != nullptr;
        return GKR_OK;
    }
    // the chunk's ONE synchronisation; behind a join() it is the side stream's as well
    int sync_main() {
        HIP_TRY(ctx_, hipStreamSynchronize(ctx_->stream));
        if (joined_) forked_ = nullptr;
        return GKR_OK;
    }

   private:
    gkr_ctx* ctx_;
    const std::string prefix_;
    const std::vector<RowSet> sets_;
    size_t rows_ = 0;
    bool device_ = false, joined_ = false;
    std::vector<gkr::verify::HashSlot> host_slots_;
    const gkr::verify::HashSlot* slots_ = nullptr;
    hipStream_t forked_ = nullptr;
};

// ---- the one read of the tables

// The evaluation of a chunk's groups x G tables of 2^n entries, queued on the main stream: points up (h_pts: pinned, ONE per group
// of G tables: groups x n), launch_mle_eval, values down (h_out: pinned, one per table).  prefix: of the workspace slots *pts,
// *out and *ws.
inline int queue_eval(gkr_ctx* ctx, const char* prefix, const Fr* d_tables, int n, uint32_t groups, uint32_t G, const Fr* h_pts, Fr* h_out) {
    Fr *d_pts = nullptr, *d_out = nullptr;
    unsigned char* d_ws = nullptr;
    const size_t nt = (size_t)groups * G;
    const std::string pts = std::string(prefix) + "pts", out = std::string(prefix) + "out", ws = std::string(prefix) + "ws";
    WS_OR_NOMEM(ctx, pts.c_str(), Fr, (size_t)groups * n, d_pts);
    WS_OR_NOMEM(ctx, out.c_str(), Fr, nt, d_out);
    WS_OR_NOMEM(ctx, ws.c_str(), unsigned char, gkr::mle_eval_ws_bytes((uint32_t)n, groups, G), d_ws);
    HIP_TRY(ctx, hipMemcpyAsync(d_pts, h_pts, (size_t)groups * n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    {
        Timed t(ctx, "mle_eval", (double)nt * 32.0 * (double)((size_t)1 << n));
        gkr::launch_mle_eval(d_tables, (uint32_t)n, groups, G, d_pts, d_ws, d_out, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, nt * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    return GKR_OK;
}

}  // namespace gkr_host
