/* Plain-C dense oracle for the GKR sumcheck hot path -- TEST INFRASTRUCTURE ONLY.
 *
 * Never linked into, loaded by or called from the product library
 * (gkr_amd/csrc).  Users: tests/, __graft_entry__.smoke(), and the
 * cpu_baseline leg of bench.py.
 *
 * Restates, on dense evaluation tables, the reference's
 *   prove_sumcheck_opt   rust/src/gkr/sumcheck.rs:36-156
 *   prove_sumcheck       rust/src/gkr/sumcheck.rs:158-214
 *   reduce_multiple_polynomial / l_function   rust/src/gkr/poly.rs:469-500,538-551
 *   calculate_input (forward step)            rust/src/convert.rs:812-831
 *   MiMC7 multi_hash (third-party mimc-rs; call sites sumcheck.rs:45,84)
 * It is the C twin of oracle/dense.py, which tests/test_oracle_equivalence.py
 * shows equal to the term-list restatement oracle/termlist.py and
 * tests/test_oracle_golden.py pins to fixtures made by the reference's own
 * Python prover.  Pinning status of each piece: oracle/__init__.py.
 *
 * All field elements cross this API as 4 little-endian 64-bit limbs of the
 * canonical value (32-byte LE repr, sumcheck.rs:10-22).
 */
#ifndef OGKR_H
#define OGKR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } ogkr_fr;

void ogkr_fr_add(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out);
void ogkr_fr_sub(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out);
void ogkr_fr_mul(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out);
int  ogkr_fr_is_canonical(const ogkr_fr *a);

void ogkr_keccak256(const uint8_t *data, size_t len, uint8_t out[32]);
void ogkr_mimc7_constant(int i, ogkr_fr *out);                 /* i in 0..90 */
void ogkr_mimc7_hash(const ogkr_fr *x, const ogkr_fr *k, ogkr_fr *out);
void ogkr_multi_hash(const ogkr_fr *arr, size_t n, const ogkr_fr *key, ogkr_fr *out);

/* Synthetic workload generator shared (by definition, not by code) with the
 * product: element i of stream `seed` is four splitmix64 outputs of the state
 * seed + 4 i + {1,2,3,4} golden-ratio steps, top limb masked to 61 bits, so the
 * value is < 2^253 < r and needs no rejection. */
void ogkr_fill_table(ogkr_fr *table, size_t count, uint64_t seed);

/* prove_sumcheck on the 2^n evaluations of a multilinear g.  out_coeffs holds
 * n rows of 2 slots, right-aligned (slot 1 = constant term); out_len[j] is the
 * reference's vector length for round j.  threads <= 0: all cores. */
int ogkr_sumcheck_mle(const ogkr_fr *table, int n, ogkr_fr *out_coeffs, uint32_t *out_len,
                      ogkr_fr *out_r, int threads);

/* the same, overwriting the caller's table (no copy: for tables of tens of GiB) */
int ogkr_sumcheck_mle_inplace(ogkr_fr *table, int n, ogkr_fr *out_coeffs, uint32_t *out_len,
                              ogkr_fr *out_r, int threads);

/* prove_sumcheck on the product of `degree` (1 .. 3) multilinear tables of 2^n evaluations each, factor f at
 * tables + f * 2^n: the C twin of tests/product_model.py (its docstring has the rules), coefficients by multiplying
 * the factors out per index.  out_coeffs: n rows of degree + 1 slots, right-aligned, highest degree first, unused
 * slots zero; out_evals: the degree entries left after the last fold.  -1: n < 2 or degree outside 1 .. 3;
 * -2: no memory. */
int ogkr_sumcheck_product(const ogkr_fr *tables, int n, int degree, ogkr_fr *out_coeffs, uint32_t *out_len,
                          ogkr_fr *out_r, ogkr_fr *out_evals, int threads);

/* prove_sumcheck on g = sum_k c_k prod_f T_t(k,f) over n_tables (1 .. 8) multilinear tables of 2^n evaluations, table m at
 * tables + m * 2^n: the C twin of tests/sop_model.py (its docstring has the rules).  Term k is the product of `degree`
 * (1 .. 3) tables table[0 .. degree - 1], scaled by the canonical term_coeffs[k]; 1 .. 8 terms.  Per index every term is
 * multiplied out and scaled, the sums are taken coefficient by coefficient; the length rule is by value in every round.
 * out_coeffs: n rows of D + 1 slots (D the largest term degree), right-aligned, highest degree first, unused slots
 * zero; out_evals: the n_tables entries left after the last fold.  -1: a bad shape, term or coefficient; -2: no memory. */
#define OGKR_SOP_MAX_TABLES 8
#define OGKR_SOP_MAX_TERMS  8
typedef struct { uint8_t degree; uint8_t table[3]; } ogkr_sop_term;
int ogkr_sumcheck_sop(const ogkr_fr *tables, int n, int n_tables, const ogkr_sop_term *terms, const ogkr_fr *term_coeffs,
                      int n_terms, ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, ogkr_fr *out_evals, int threads);

/* The zero-check sum_x eq(z, x) g(x), g as above with term degrees 1 .. 2, in the EXPLICIT form: eq(z, .) is materialised
 * (2^n entries) and ogkr_sumcheck_sop's rounds run on {eq, T_0 ..} with every term prefixed by table 0.  z: n canonical
 * elements, variable 1 = the most significant index bit.  out_coeffs: n rows of D + 2 slots (D the largest term degree);
 * out_evals: the n_tables tables' entries left; out_eq: the eq table's.  Errors as above. */
int ogkr_sumcheck_zerocheck(const ogkr_fr *tables, int n, int n_tables, const ogkr_sop_term *terms, const ogkr_fr *term_coeffs,
                            int n_terms, const ogkr_fr *z, ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r,
                            ogkr_fr *out_evals, ogkr_fr *out_eq, int threads);

/* The grand product P = prod_i table[i] of 2^n canonical values as GKR on the binary tree of products (include/gkr_amd.h,
 * gkr_grand_product*): the C twin of tests/grand_product_model.py.  The tree L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k] is a loop of
 * ogkr_fr_mul; the head is L_2, z^(2) = (multi_hash(L_2), multi_hash([zeta_1])); layer k = 2 .. n - 1 is ogkr_sumcheck_zerocheck
 * with the one term T_0 T_1 (coefficient 1) on the two halves of level k + 1 at z^(k), then tau_k = multi_hash([a_k, b_k]),
 * c_{k+1} = a_k + tau_k (b_k - a_k), z^(k+1) = (tau_k, r^(k)).  With R = n (n - 1) / 2 - 1 and layer k's rows from
 * k (k - 1) / 2 - 1 on: out_head 4, out_coeffs R rows of 4 slots (right-aligned, highest degree first, unused slots zero),
 * out_len R, out_r R, out_evals (n - 2) x 2 the (a_k, b_k), out_point n the point z^(n), out_claim c_n.  out_levels, if not
 * NULL, takes the levels 0 .. n - 1, level k at 2^k - 1 (2^n - 1 elements: the library's layout for one table).
 * -1: n < 3, n > 30 or a NULL pointer (out_levels apart); -2: no memory. */
int ogkr_grand_product(const ogkr_fr *table, int n, ogkr_fr *out_product, ogkr_fr *out_head, ogkr_fr *out_coeffs, uint32_t *out_len,
                       ogkr_fr *out_r, ogkr_fr *out_evals, ogkr_fr *out_point, ogkr_fr *out_claim, ogkr_fr *out_levels, int threads);

/* The fractional sum sum_i num[i] / den[i] = P / Q of 2^n pairs of canonical values as GKR on the binary tree of fractions
 * (include/gkr_amd.h, gkr_fraction_sum*): the C twin of tests/fraction_sum_model.fraction_sum.  The tree
 * p_k[i] = p_{k+1}[i] q_{k+1}[i + 2^k] + p_{k+1}[i + 2^k] q_{k+1}[i], q_k[i] = q_{k+1}[i] q_{k+1}[i + 2^k] is a loop of
 * ogkr_fr_mul / ogkr_fr_add; the head is (p_2, q_2), z^(2) = (zeta_1, zeta_2) = (multi_hash(head), multi_hash([zeta_1])),
 * lambda_2 = multi_hash([zeta_2]); layer k = 2 .. n - 1 is ogkr_sumcheck_zerocheck with the terms T0 T3 + T1 T2 + lambda_k T2 T3 on
 * the halves of p_{k+1} (T0, T1) and q_{k+1} (T2, T3) at z^(k), then tau_k = multi_hash([a0, a1, b0, b1]),
 * cp = a0 + tau_k (a1 - a0), cq = b0 + tau_k (b1 - b0), z^(k+1) = (tau_k, r^(k)), lambda_{k+1} = multi_hash([tau_k]).  With
 * R = n (n - 1) / 2 - 1 and layer k's rows from k (k - 1) / 2 - 1 on: out_sums 2 (P, Q), out_head 8, out_coeffs R rows of 4 slots
 * (right-aligned, highest degree first, unused slots zero), out_len R, out_r R, out_evals (n - 2) x 4, out_point n the point
 * z^(n), out_claims 2 (cp_n, cq_n).  out_levels, if not NULL, takes the levels 0 .. n - 1, level k at 2 (2^k - 1), p_k then q_k
 * (2 (2^n - 1) elements: the library's layout for one pair).  -1: n < 3, n > 29 or a NULL pointer (out_levels apart); -2: no memory. */
int ogkr_fraction_sum(const ogkr_fr *num, const ogkr_fr *den, int n, ogkr_fr *out_sums, ogkr_fr *out_head, ogkr_fr *out_coeffs,
                      uint32_t *out_len, ogkr_fr *out_r, ogkr_fr *out_evals, ogkr_fr *out_point, ogkr_fr *out_claims, ogkr_fr *out_levels,
                      int threads);

/* The lookup argument's inputs (include/gkr_amd.h, gkr_lookup*): the C twins of tests/lookup_model.multiplicities and .pair.
 *   multiplicities: out_mult[j] = #{i: witness[i] = table[j]} if j is the lowest index with table's value table[j], else 0 --
 *                   counted by sorting the table's indices by (value, index) and a binary search per witness entry (no hash
 *                   table); *out_missing the witness entries outside the table, *out_first_missing the lowest such index or
 *                   0xFFFFFFFF.  Not thread-safe (one sort at a time).
 *   pair:           out_pair = N then D, 2^L each, L = max(n_w, n_t) + 1: (1, alpha - witness[i]) for i < 2^n_w, (0, 1) up to
 *                   2^(L-1), then (-mult[j], alpha - table[j]) for j < 2^n_t, (0, 1) up to 2^L.
 * -1: n_w or n_t outside 0 .. 30 or a NULL pointer; -2: no memory. */
int ogkr_lookup_multiplicities(const ogkr_fr *witness, int n_w, const ogkr_fr *table, int n_t, ogkr_fr *out_mult, uint32_t *out_missing,
                               uint32_t *out_first_missing);
int ogkr_lookup_pair(const ogkr_fr *witness, int n_w, const ogkr_fr *table, int n_t, const ogkr_fr *mult, const ogkr_fr *alpha,
                     ogkr_fr *out_pair);

/* The tables of the R1CS zero-check and inner sumcheck on the flat form of an R1CS: counts[3 * n_constraints] (the records of A,
 * B, C per constraint), wires[] and canonical coeffs[], one record after the other -- the C twins of tests/r1cs_rows_model.rows,
 * tests/r1cs_cols_model.cols_table and verifier.r1cs_matrix_evals, as loops over the records as they stand.  A zero coefficient
 * contributes nothing, a repeated wire adds; variable 1 of a point is the most significant index bit.
 *   rows:          out[m * 2^n + i] = sum coeff * witness[wire] over the combination of constraint i in matrix m, zero for
 *                  i >= n_constraints; witness: n_wires canonical elements; out: 3 * 2^n.
 *   cols:          out[y] = sum_m rho[m] sum_i M_m[i][y] eq(x, i), eq(x, .) written out as a table of 2^n_x entries and the
 *                  records scattered one by one; zero for y >= n_wires; out: 2^n_y.
 *   matrix_evals:  out[m] = sum over the records (c, wire w) of constraint i in matrix m of c eq(x, i) eq(y, w), both eq tables
 *                  written out; out: 3.
 * -1: a wire >= n_wires, n_constraints > 2^n (2^n_x), n_wires > 2^n_y, or an element that is not canonical; -2: no memory. */
int ogkr_r1cs_rows(size_t n_constraints, uint32_t n_wires, const uint32_t *counts, const uint32_t *wires, const ogkr_fr *coeffs,
                   const ogkr_fr *witness, int n, ogkr_fr *out, int threads);
int ogkr_r1cs_cols(size_t n_constraints, uint32_t n_wires, const uint32_t *counts, const uint32_t *wires, const ogkr_fr *coeffs,
                   const ogkr_fr *x, int n_x, const ogkr_fr *rho, int n_y, ogkr_fr *out, int threads);
int ogkr_r1cs_matrix_evals(size_t n_constraints, uint32_t n_wires, const uint32_t *counts, const uint32_t *wires, const ogkr_fr *coeffs,
                           const ogkr_fr *x, int n_x, const ogkr_fr *y, int n_y, ogkr_fr *out, int threads);

/* out[i] = a[i] * b[i], a[i] + b[i] for i < count (out may be a or b): for witnesses and first_bad at sizes where a Python
 * integer per entry costs too much */
void ogkr_fr_mul_many(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out, size_t count);
void ogkr_fr_add_many(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out, size_t count);

/* prove_sumcheck_opt for one layer: gates g = 0..2^k_i-1 of type gate_type[g]
 * (0 add, 1 mult) with operands left[g], right[g] in [0, 2^k_next); z has k_i
 * entries; W has 2^k_next evaluations.  out_coeffs: 2*k_next rows of 3 slots,
 * right-aligned, highest degree first. */
int ogkr_sumcheck_layer(int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left,
                        const uint32_t *right, const ogkr_fr *z, const ogkr_fr *W,
                        ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, int threads);

/* The same transcript in time linear in the gates (no 2^{2 k_next}-entry tables; k_next up to 28): U, V and the
 * c-phase row summed over the gate list -- the C twin of oracle/gatesum.py, the checker for wide layers. */
int ogkr_sumcheck_layer_lin(int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left,
                            const uint32_t *right, const ogkr_fr *z, const ogkr_fr *W,
                            ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, int threads);

/* eq(z, .) weights scattered into the dense predicate tables A, M (2^{2 k_next} each). */
int ogkr_predicate_tables(int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left,
                          const uint32_t *right, const ogkr_fr *z, ogkr_fr *A, ogkr_fr *M);

/* forward gate evaluation of one layer */
void ogkr_layer_eval(size_t gates, const uint8_t *gate_type, const uint32_t *left,
                     const uint32_t *right, const ogkr_fr *prev, ogkr_fr *out);

/* q(t) = W(b + t (c - b)); out has k+1 slots right-aligned, *out_len = 1 + max
 * total degree of a non-zero monomial of W. */
int ogkr_line_restriction(int k, const ogkr_fr *b, const ogkr_fr *c, const ogkr_fr *W,
                          ogkr_fr *out, uint32_t *out_len);

/* evaluation table -> monomial coefficients (MSB-first Moebius transform), in place */
void ogkr_mobius(ogkr_fr *vals, int k);

/* default thread count of every parallel loop below (OpenMP's own default is one per visible CPU) */
void ogkr_set_threads(int threads);
int ogkr_max_threads(void);

#ifdef __cplusplus
}
#endif
#endif
