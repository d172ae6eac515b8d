/* Stand-alone check of ogkr_r1cs_rows, ogkr_r1cs_cols and ogkr_r1cs_matrix_evals (TEST INFRASTRUCTURE ONLY), meant to be built with
 * ogkr.c under -fsanitize=address,undefined (make r1cs_selfcheck): systems of 1 .. 2^n constraints for n = 2 .. 9 with empty rows,
 * rows of up to 70 records, zero coefficients, repeated wires and wire 0 in most rows, with 1 and with 4 threads.  The two runs
 * must give equal bytes; with eq tables built here entry by entry,
 *     sum_y T[y] w[y] == sum_m rho_m sum_i eq(x, i) (M_m w)[i]       and
 *     matrix_evals(x, y)[m] == sum_w eq(y, w) T_m[w], T_m the cols table with rho the m-th unit vector;
 * rows past the constraints and entries past the wires are zero; the bad shapes are refused.  Exit status 1 on a mismatch. */
#include "ogkr.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_N 9
#define MAX_ROW 70

static const ogkr_fr ONE = {{1, 0, 0, 0}};

static uint64_t state = 0x9E3779B97F4A7C15ULL;
static uint64_t next_u64(void) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
}

static void small(ogkr_fr *x, uint64_t v) {
    memset(x, 0, sizeof *x);
    x->l[0] = v;
}

static void eq_at(const ogkr_fr *z, int n, size_t i, ogkr_fr *out) {
    ogkr_fr e = ONE, f;
    for (int v = 0; v < n; ++v) {
        if ((i >> (n - 1 - v)) & 1) f = z[v];
        else ogkr_fr_sub(&ONE, &z[v], &f);
        ogkr_fr_mul(&e, &f, &e);
    }
    *out = e;
}

static int is_zero(const ogkr_fr *x) { return !(x->l[0] | x->l[1] | x->l[2] | x->l[3]); }

int main(void) {
    int bad = 0;
    const size_t max_len = (size_t)1 << MAX_N, max_records = 3 * max_len * MAX_ROW;
    uint32_t *counts = malloc(3 * max_len * sizeof(uint32_t)), *wires = malloc(max_records * sizeof(uint32_t));
    ogkr_fr *coeffs = malloc(max_records * sizeof(ogkr_fr)), *w = malloc(max_len * sizeof(ogkr_fr));
    ogkr_fr *rows = malloc(3 * max_len * sizeof(ogkr_fr)), *rows4 = malloc(3 * max_len * sizeof(ogkr_fr));
    ogkr_fr *T = malloc(max_len * sizeof(ogkr_fr)), *T4 = malloc(max_len * sizeof(ogkr_fr));
    if (!counts || !wires || !coeffs || !w || !rows || !rows4 || !T || !T4) return 2;
    ogkr_fr minus_one, x[MAX_N], y[MAX_N], rho[3], unit[3], me[3], me4[3];
    small(&minus_one, 0);
    ogkr_fr_sub(&minus_one, &ONE, &minus_one);
    for (int n = 2; n <= MAX_N; ++n) {
        for (int n_y = 2; n_y <= MAX_N; n_y += (n % 3) + 1) {
            const size_t len = (size_t)1 << n, len_y = (size_t)1 << n_y;
            /* sizes: full tables, one past half, a single constraint / wire */
            const size_t n_constraints = (n + n_y) % 3 == 0 ? len : (n + n_y) % 3 == 1 ? len / 2 + 1 : 1;
            const uint32_t n_wires = (uint32_t)((n * n_y) % 3 == 0 ? len_y : (n * n_y) % 3 == 1 ? len_y / 2 + 1 : 1);
            size_t records = 0;
            for (size_t i = 0; i < 3 * n_constraints; ++i) {
                const uint64_t pick = next_u64() % 16;
                const uint32_t count = pick == 0 ? MAX_ROW : pick == 1 ? 33 : pick == 2 ? 65 : (uint32_t)(pick % 5);   /* 0 .. 4, or long */
                counts[i] = count;
                for (uint32_t t = 0; t < count; ++t, ++records) {
                    wires[records] = (t == 0 && pick % 2) ? 0 : (uint32_t)(next_u64() % n_wires);
                    const uint64_t kind = next_u64() % 8;
                    if (kind == 0) small(&coeffs[records], 0);
                    else if (kind < 3) coeffs[records] = ONE;
                    else if (kind < 5) coeffs[records] = minus_one;
                    else ogkr_fill_table(&coeffs[records], 1, next_u64());
                }
            }
            ogkr_fill_table(w, n_wires, 100u + (unsigned)n);
            ogkr_fill_table(x, (size_t)n, 200u + (unsigned)n);
            ogkr_fill_table(y, (size_t)n_y, 300u + (unsigned)n_y);
            ogkr_fill_table(rho, 3, 400u + (unsigned)(n + n_y));
            if (n % 2) small(&x[0], 1);
            if (n_y % 2) small(&y[n_y - 1], 0);
            /* -- 1 and 4 threads */
            memset(rows, 0xab, 3 * len * sizeof(ogkr_fr));
            memset(T, 0xab, len_y * sizeof(ogkr_fr));
            if (ogkr_r1cs_rows(n_constraints, n_wires, counts, wires, coeffs, w, n, rows, 1) ||
                ogkr_r1cs_rows(n_constraints, n_wires, counts, wires, coeffs, w, n, rows4, 4) ||
                ogkr_r1cs_cols(n_constraints, n_wires, counts, wires, coeffs, x, n, rho, n_y, T, 1) ||
                ogkr_r1cs_cols(n_constraints, n_wires, counts, wires, coeffs, x, n, rho, n_y, T4, 4) ||
                ogkr_r1cs_matrix_evals(n_constraints, n_wires, counts, wires, coeffs, x, n, y, n_y, me, 1) ||
                ogkr_r1cs_matrix_evals(n_constraints, n_wires, counts, wires, coeffs, x, n, y, n_y, me4, 4)) {
                printf("n=%d n_y=%d: error return\n", n, n_y);
                bad = 1;
                continue;
            }
            if (memcmp(rows, rows4, 3 * len * sizeof(ogkr_fr)) || memcmp(T, T4, len_y * sizeof(ogkr_fr)) || memcmp(me, me4, sizeof me)) {
                printf("n=%d n_y=%d: 1 and 4 threads differ\n", n, n_y);
                bad = 1;
            }
            /* -- padding */
            for (int m = 0; m < 3; ++m)
                for (size_t i = n_constraints; i < len; ++i)
                    if (!is_zero(&rows[(size_t)m * len + i])) bad = 1, printf("n=%d: row %zu of matrix %d is not zero\n", n, i, m);
            for (size_t v = n_wires; v < len_y; ++v)
                if (!is_zero(&T[v])) bad = 1, printf("n_y=%d: entry %zu of T is not zero\n", n_y, v);
            /* -- sum_y T[y] w[y] == sum_m rho_m sum_i eq(x, i) (M_m w)[i] */
            ogkr_fr lhs, rhs, p, e;
            small(&lhs, 0);
            small(&rhs, 0);
            for (size_t v = 0; v < n_wires; ++v) {
                ogkr_fr_mul(&T[v], &w[v], &p);
                ogkr_fr_add(&lhs, &p, &lhs);
            }
            for (size_t i = 0; i < n_constraints; ++i) {
                eq_at(x, n, i, &e);
                for (int m = 0; m < 3; ++m) {
                    ogkr_fr_mul(&e, &rows[(size_t)m * len + i], &p);
                    ogkr_fr_mul(&p, &rho[m], &p);
                    ogkr_fr_add(&rhs, &p, &rhs);
                }
            }
            if (memcmp(&lhs, &rhs, sizeof lhs)) {
                printf("n=%d n_y=%d: <T, w> differs from the weighted rows\n", n, n_y);
                bad = 1;
            }
            /* -- matrix_evals against the cols table of a unit rho, extended at y */
            for (int m = 0; m < 3; ++m) {
                for (int k = 0; k < 3; ++k) small(&unit[k], k == m);
                if (ogkr_r1cs_cols(n_constraints, n_wires, counts, wires, coeffs, x, n, unit, n_y, T4, 4)) {
                    printf("n=%d n_y=%d: error return\n", n, n_y);
                    bad = 1;
                    continue;
                }
                small(&lhs, 0);
                for (size_t v = 0; v < len_y; ++v) {
                    eq_at(y, n_y, v, &e);
                    ogkr_fr_mul(&e, &T4[v], &p);
                    ogkr_fr_add(&lhs, &p, &lhs);
                }
                if (memcmp(&lhs, &me[m], sizeof lhs)) {
                    printf("n=%d n_y=%d matrix %d: matrix_evals differs from the cols table's extension\n", n, n_y, m);
                    bad = 1;
                }
            }
        }
    }
    /* the vector product and sum */
    ogkr_fill_table(T, 100, 7);
    ogkr_fill_table(T4, 100, 8);
    ogkr_fr_mul_many(T, T4, rows, 100);
    ogkr_fr_add_many(T, T4, rows4, 100);
    for (size_t i = 0; i < 100; ++i) {
        ogkr_fr p, s;
        ogkr_fr_mul(&T[i], &T4[i], &p);
        ogkr_fr_add(&T[i], &T4[i], &s);
        if (memcmp(&p, &rows[i], sizeof p) || memcmp(&s, &rows4[i], sizeof s)) bad = 1, printf("mul_many / add_many differ at %zu\n", i);
    }
    /* the refusals: three constraints of one record each per matrix over four wires */
    ogkr_fr big;
    memset(&big, 0xff, sizeof big);
    for (size_t i = 0; i < 9; ++i) {
        counts[i] = 1;
        wires[i] = (uint32_t)(i % 4);
        small(&coeffs[i], i + 1);
    }
    ogkr_fill_table(w, 4, 1);
    ogkr_fill_table(x, 2, 2);
    ogkr_fill_table(y, 2, 3);
    if (ogkr_r1cs_rows(3, 4, counts, wires, coeffs, w, 2, rows, 1) || ogkr_r1cs_cols(3, 4, counts, wires, coeffs, x, 2, rho, 2, T, 1) ||
        ogkr_r1cs_matrix_evals(3, 4, counts, wires, coeffs, x, 2, y, 2, me, 1)) {
        printf("the good shape beside the bad ones was refused\n");
        bad = 1;
    }
    if (ogkr_r1cs_rows(3, 4, counts, wires, coeffs, w, 1, rows, 1) != -1 ||                      /* n_constraints > 2^n */
        ogkr_r1cs_rows(3, 3, counts, wires, coeffs, w, 2, rows, 1) != -1 ||                      /* a wire >= n_wires */
        ogkr_r1cs_cols(3, 4, counts, wires, coeffs, x, 1, rho, 2, T, 1) != -1 ||                 /* n_constraints > 2^n_x */
        ogkr_r1cs_cols(3, 4, counts, wires, coeffs, x, 2, rho, 1, T, 1) != -1 ||                 /* n_wires > 2^n_y */
        ogkr_r1cs_cols(3, 3, counts, wires, coeffs, x, 2, rho, 2, T, 1) != -1 ||
        ogkr_r1cs_matrix_evals(3, 4, counts, wires, coeffs, x, 1, y, 2, me, 1) != -1 ||
        ogkr_r1cs_matrix_evals(3, 4, counts, wires, coeffs, x, 2, y, 1, me, 1) != -1 ||
        ogkr_r1cs_matrix_evals(3, 3, counts, wires, coeffs, x, 2, y, 2, me, 1) != -1) {
        printf("a bad shape was accepted\n");
        bad = 1;
    }
    coeffs[5] = big;
    if (ogkr_r1cs_rows(3, 4, counts, wires, coeffs, w, 2, rows, 1) != -1 || ogkr_r1cs_cols(3, 4, counts, wires, coeffs, x, 2, rho, 2, T, 1) != -1 ||
        ogkr_r1cs_matrix_evals(3, 4, counts, wires, coeffs, x, 2, y, 2, me, 1) != -1) {
        printf("a coefficient that is not canonical was accepted\n");
        bad = 1;
    }
    free(counts);
    free(wires);
    free(coeffs);
    free(w);
    free(rows);
    free(rows4);
    free(T);
    free(T4);
    printf(bad ? "r1cs_selfcheck: FAILED\n" : "r1cs_selfcheck: ok\n");
    return bad;
}
