/* Stand-alone check of ogkr_sumcheck_sop and ogkr_sumcheck_zerocheck (TEST INFRASTRUCTURE ONLY), meant to be built with ogkr.c
 * under -fsanitize=address,undefined (make sop_selfcheck): n = 2 .. 10, a term list that uses every degree, a shared table and
 * the full eight terms, with 1 and with 4 threads.  The two runs must give equal bytes, one term of coefficient 1 must equal
 * ogkr_sumcheck_product, and the zero-check must equal the SOP oracle on an eq table built here.  Exit status 1 on a mismatch. */
#include "ogkr.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_N 10
#define MAX_SLOTS 4
#define TABLES 4

typedef struct {
    ogkr_fr coeffs[MAX_N * MAX_SLOTS];
    uint32_t len[MAX_N];
    ogkr_fr r[MAX_N];
    ogkr_fr evals[OGKR_SOP_MAX_TABLES + 1];
    ogkr_fr eq;
} transcript;

static const ogkr_fr ONE = {{1, 0, 0, 0}};

/* ABC - AD + 5 BB + 7 D, then four more terms to fill the list: 3 AB, C, 2 CD, (r - 1) A */
static const ogkr_sop_term SOP_TERMS[8] = {{3, {0, 1, 2}}, {2, {0, 3, 0}}, {2, {1, 1, 0}}, {1, {3, 0, 0}},
                                           {2, {0, 1, 0}}, {1, {2, 0, 0}}, {2, {2, 3, 0}}, {1, {0, 0, 0}}};
/* AB - C + 5 DD + 7 A (degrees 1 and 2 only) */
static const ogkr_sop_term ZC_TERMS[4] = {{2, {0, 1, 0}}, {1, {2, 0, 0}}, {2, {3, 3, 0}}, {1, {0, 0, 0}}};

static void small(ogkr_fr *x, uint64_t v) {
    memset(x, 0, sizeof *x);
    x->l[0] = v;
}

int main(void) {
    int bad = 0;
    const size_t max_len = (size_t)1 << MAX_N;
    ogkr_fr *tables = malloc((TABLES + 1) * max_len * sizeof(ogkr_fr));   /* one more for the eq table */
    transcript *a = calloc(1, sizeof *a), *b = calloc(1, sizeof *b);
    if (!tables || !a || !b) return 2;
    ogkr_fr coeffs[8], minus_one, z[MAX_N];
    small(&minus_one, 0);
    ogkr_fr_sub(&minus_one, &ONE, &minus_one);
    small(&coeffs[0], 1);
    coeffs[1] = minus_one;
    small(&coeffs[2], 5);
    small(&coeffs[3], 7);
    small(&coeffs[4], 3);
    small(&coeffs[5], 1);
    small(&coeffs[6], 2);
    coeffs[7] = minus_one;
    for (int n = 2; n <= MAX_N; ++n) {
        const size_t len = (size_t)1 << n;
        ogkr_fill_table(tables, TABLES * len, 3000u + 16u * (unsigned)n);
        /* table B ignores x_n, table C ignores x_1 */
        for (size_t m = 0; m < len / 2; ++m) tables[len + 2 * m + 1] = tables[len + 2 * m];
        memcpy(tables + 2 * len + len / 2, tables + 2 * len, len / 2 * sizeof(ogkr_fr));
        /* -- the SOP oracle: 4 and 8 terms, 1 and 4 threads */
        for (int n_terms = 4; n_terms <= 8; n_terms += 4) {
            memset(a, 0, sizeof *a);
            memset(b, 0, sizeof *b);
            if (ogkr_sumcheck_sop(tables, n, TABLES, SOP_TERMS, coeffs, n_terms, a->coeffs, a->len, a->r, a->evals, 1) ||
                ogkr_sumcheck_sop(tables, n, TABLES, SOP_TERMS, coeffs, n_terms, b->coeffs, b->len, b->r, b->evals, 4)) {
                printf("n=%d terms=%d: error return\n", n, n_terms);
                bad = 1;
            } else if (memcmp(a, b, sizeof *a) != 0) {
                printf("n=%d terms=%d: 1 and 4 threads differ\n", n, n_terms);
                bad = 1;
            }
        }
        /* -- one term of coefficient 1 is the product */
        for (int d = 1; d <= 3; ++d) {
            const ogkr_sop_term one_term = {(uint8_t)d, {0, 1, 2}};
            memset(a, 0, sizeof *a);
            memset(b, 0, sizeof *b);
            if (ogkr_sumcheck_sop(tables, n, d, &one_term, &ONE, 1, a->coeffs, a->len, a->r, a->evals, 4) ||
                ogkr_sumcheck_product(tables, n, d, b->coeffs, b->len, b->r, b->evals, 4)) {
                printf("n=%d degree=%d: error return\n", n, d);
                bad = 1;
            } else if (memcmp(a, b, sizeof *a) != 0) {
                printf("n=%d degree=%d: one term differs from ogkr_sumcheck_product\n", n, d);
                bad = 1;
            }
        }
        /* -- the zero-check: 1 and 4 threads; z_1 = 0, z_n = 1, the rest from the generator */
        ogkr_fill_table(z, (size_t)n, 4000u + (unsigned)n);
        small(&z[0], 0);
        small(&z[n - 1], 1);
        memset(a, 0, sizeof *a);
        memset(b, 0, sizeof *b);
        if (ogkr_sumcheck_zerocheck(tables, n, TABLES, ZC_TERMS, coeffs, 4, z, a->coeffs, a->len, a->r, a->evals, &a->eq, 1) ||
            ogkr_sumcheck_zerocheck(tables, n, TABLES, ZC_TERMS, coeffs, 4, z, b->coeffs, b->len, b->r, b->evals, &b->eq, 4)) {
            printf("n=%d: zero-check error return\n", n);
            bad = 1;
            continue;
        }
        if (memcmp(a, b, sizeof *a) != 0) {
            printf("n=%d: zero-check, 1 and 4 threads differ\n", n);
            bad = 1;
        }
        /* ... and the SOP oracle on {eq, A, B, C, D} with the eq table built here entry by entry */
        memmove(tables + len, tables, TABLES * len * sizeof(ogkr_fr));
        for (size_t i = 0; i < len; ++i) {
            ogkr_fr e = ONE, f;
            for (int v = 0; v < n; ++v) {
                if ((i >> (n - 1 - v)) & 1) f = z[v];
                else ogkr_fr_sub(&ONE, &z[v], &f);
                ogkr_fr_mul(&e, &f, &e);
            }
            tables[i] = e;
        }
        ogkr_sop_term lifted[4];
        for (int k = 0; k < 4; ++k) {
            lifted[k].degree = (uint8_t)(ZC_TERMS[k].degree + 1);
            lifted[k].table[0] = 0;
            lifted[k].table[1] = (uint8_t)(ZC_TERMS[k].table[0] + 1);
            lifted[k].table[2] = (uint8_t)(ZC_TERMS[k].table[1] + 1);
        }
        memset(b, 0, sizeof *b);
        if (ogkr_sumcheck_sop(tables, n, TABLES + 1, lifted, coeffs, 4, b->coeffs, b->len, b->r, b->evals, 4)) {
            printf("n=%d: error return on the explicit form\n", n);
            bad = 1;
        } else if (memcmp(a->coeffs, b->coeffs, sizeof a->coeffs) != 0 || memcmp(a->len, b->len, sizeof a->len) != 0 ||
                   memcmp(a->r, b->r, sizeof a->r) != 0 || memcmp(&a->eq, &b->evals[0], sizeof a->eq) != 0 ||
                   memcmp(a->evals, b->evals + 1, TABLES * sizeof(ogkr_fr)) != 0) {
            printf("n=%d: zero-check differs from the SOP oracle on the eq table built here\n", n);
            bad = 1;
        }
    }
    /* the argument checks */
    const ogkr_sop_term cube = {3, {0, 0, 0}}, far = {2, {0, 4, 0}}, none = {0, {0, 0, 0}};
    ogkr_fr big;
    memset(&big, 0xff, sizeof big);
    small(&z[0], 3);
    small(&z[1], 5);
    small(&z[2], 7);
    small(&z[3], 9);
    if (ogkr_sumcheck_sop(tables, 1, 1, &cube, &ONE, 1, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_sop(tables, 4, 0, &cube, &ONE, 1, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_sop(tables, 4, 9, &cube, &ONE, 1, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_sop(tables, 4, 4, &cube, &ONE, 0, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_sop(tables, 4, 4, SOP_TERMS, coeffs, 9, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_sop(tables, 4, 4, &far, &ONE, 1, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_sop(tables, 4, 4, &none, &ONE, 1, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_sop(tables, 4, 4, &cube, &big, 1, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_zerocheck(tables, 4, 4, &cube, &ONE, 1, z, a->coeffs, a->len, a->r, a->evals, &a->eq, 1) == 0 ||
        ogkr_sumcheck_zerocheck(tables, 4, 4, ZC_TERMS, coeffs, 4, NULL, a->coeffs, a->len, a->r, a->evals, &a->eq, 1) == 0) {
        printf("a bad shape was accepted\n");
        bad = 1;
    }
    z[2] = big;
    if (ogkr_sumcheck_zerocheck(tables, 4, 4, ZC_TERMS, coeffs, 4, z, a->coeffs, a->len, a->r, a->evals, &a->eq, 1) == 0) {
        printf("a point that is not canonical was accepted\n");
        bad = 1;
    }
    free(tables);
    free(a);
    free(b);
    printf(bad ? "sop_selfcheck: FAILED\n" : "sop_selfcheck: ok\n");
    return bad;
}
