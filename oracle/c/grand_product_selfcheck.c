/* Stand-alone check of ogkr_grand_product (TEST INFRASTRUCTURE ONLY), meant to be built with ogkr.c under
 * -fsanitize=address,undefined (make grand_product_selfcheck): n = 3 .. 10 on a random table, a table with one zero entry and a
 * table whose upper half is zero, with 1 and with 4 threads, with and without the levels.  The runs must give equal bytes; the
 * product must be the plain product; the levels, the head, every layer and the chain of points and claims must be what this
 * program gets from a tree of its own and one ogkr_sumcheck_zerocheck call per layer; a zero upper half gives vectors [0] of
 * length 1 throughout.  Every output buffer is allocated at its exact size, so a write past a row is a report.  Exit status 1
 * on a mismatch. */
#include "ogkr.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_N 10

typedef struct {
    ogkr_fr product, head[4], claim;
    ogkr_fr *coeffs, *r, *evals, *point;
    uint32_t *len;
} proof;

static const ogkr_fr ZERO = {{0, 0, 0, 0}}, ONE = {{1, 0, 0, 0}};

static size_t rounds(int n) { return (size_t)n * (size_t)(n - 1) / 2 - 1; }

static int proof_alloc(proof *p, int n) {
    const size_t R = rounds(n);
    memset(p, 0, sizeof *p);
    p->coeffs = calloc(4 * R, sizeof(ogkr_fr));
    p->r = calloc(R, sizeof(ogkr_fr));
    p->evals = calloc(2 * (size_t)(n - 2), sizeof(ogkr_fr));
    p->point = calloc((size_t)n, sizeof(ogkr_fr));
    p->len = calloc(R, sizeof(uint32_t));
    return p->coeffs && p->r && p->evals && p->point && p->len;
}

static void proof_free(proof *p) {
    free(p->coeffs);
    free(p->r);
    free(p->evals);
    free(p->point);
    free(p->len);
}

static int proof_run(proof *p, const ogkr_fr *table, int n, ogkr_fr *levels, int threads) {
    return ogkr_grand_product(table, n, &p->product, p->head, p->coeffs, p->len, p->r, p->evals, p->point, &p->claim, levels, threads);
}

static int proof_same(const proof *a, const proof *b, int n) {
    const size_t R = rounds(n);
    return !memcmp(&a->product, &b->product, sizeof a->product) && !memcmp(a->head, b->head, sizeof a->head) &&
           !memcmp(&a->claim, &b->claim, sizeof a->claim) && !memcmp(a->coeffs, b->coeffs, 4 * R * sizeof(ogkr_fr)) &&
           !memcmp(a->r, b->r, R * sizeof(ogkr_fr)) && !memcmp(a->evals, b->evals, 2 * (size_t)(n - 2) * sizeof(ogkr_fr)) &&
           !memcmp(a->point, b->point, (size_t)n * sizeof(ogkr_fr)) && !memcmp(a->len, b->len, R * sizeof(uint32_t));
}

/* the chain once more, on a tree built here level by level (each level its own allocation) */
static int chain_matches(const proof *p, const ogkr_fr *table, int n, const ogkr_fr *levels) {
    ogkr_fr *lv[MAX_N + 1];
    int ok = 1;
    lv[n] = malloc(((size_t)1 << n) * sizeof(ogkr_fr));
    if (!lv[n]) return 0;
    memcpy(lv[n], table, ((size_t)1 << n) * sizeof(ogkr_fr));
    for (int k = n - 1; k >= 0; --k) {
        const size_t h = (size_t)1 << k;
        lv[k] = malloc(h * sizeof(ogkr_fr));
        if (!lv[k]) return 0;
        for (size_t i = 0; i < h; ++i) ogkr_fr_mul(&lv[k + 1][i], &lv[k + 1][i + h], &lv[k][i]);
        if (memcmp(lv[k], levels + (h - 1), h * sizeof(ogkr_fr)) != 0) ok = 0;
    }
    ogkr_fr plain = ONE;
    for (size_t i = 0; i < (size_t)1 << n; ++i) ogkr_fr_mul(&plain, &table[i], &plain);
    if (memcmp(&plain, &p->product, sizeof plain) != 0 || memcmp(lv[2], p->head, 4 * sizeof(ogkr_fr)) != 0) ok = 0;
    ogkr_fr z[MAX_N + 1], claim = ZERO;
    ogkr_multi_hash(lv[2], 4, &ZERO, &z[0]);
    ogkr_multi_hash(&z[0], 1, &ZERO, &z[1]);
    const ogkr_sop_term term = {2, {0, 1, 0}};
    for (int k = 2; k < n; ++k) {
        const size_t row = (size_t)k * (size_t)(k - 1) / 2 - 1;
        ogkr_fr *c = calloc(4 * (size_t)k, sizeof(ogkr_fr)), *r = calloc((size_t)k, sizeof(ogkr_fr)), ab[2], eq, tau, d;
        uint32_t *len = calloc((size_t)k, sizeof(uint32_t));
        if (!c || !r || !len) return 0;
        if (ogkr_sumcheck_zerocheck(lv[k + 1], k, 2, &term, &ONE, 1, z, c, len, r, ab, &eq, 1)) ok = 0;
        if (memcmp(c, p->coeffs + 4 * row, 4 * (size_t)k * sizeof(ogkr_fr)) != 0 || memcmp(len, p->len + row, (size_t)k * sizeof(uint32_t)) != 0 ||
            memcmp(r, p->r + row, (size_t)k * sizeof(ogkr_fr)) != 0 || memcmp(ab, p->evals + 2 * (size_t)(k - 2), sizeof ab) != 0)
            ok = 0;
        ogkr_multi_hash(ab, 2, &ZERO, &tau);
        ogkr_fr_sub(&ab[1], &ab[0], &d);
        ogkr_fr_mul(&tau, &d, &d);
        ogkr_fr_add(&ab[0], &d, &claim);
        z[0] = tau;
        memcpy(z + 1, r, (size_t)k * sizeof(ogkr_fr));
        free(c);
        free(r);
        free(len);
    }
    if (memcmp(z, p->point, (size_t)n * sizeof(ogkr_fr)) != 0 || memcmp(&claim, &p->claim, sizeof claim) != 0) ok = 0;
    for (int k = 0; k <= n; ++k) free(lv[k]);
    return ok;
}

int main(void) {
    int bad = 0;
    for (int n = 3; n <= MAX_N; ++n) {
        const size_t size = (size_t)1 << n, R = rounds(n);
        for (int kind = 0; kind < 3; ++kind) {
            ogkr_fr *table = malloc(size * sizeof(ogkr_fr)), *levels = malloc((size - 1) * sizeof(ogkr_fr));
            proof a, b, c;
            if (!table || !levels || !proof_alloc(&a, n) || !proof_alloc(&b, n) || !proof_alloc(&c, n)) return 2;
            ogkr_fill_table(table, size, 5000u + 16u * (unsigned)n + (unsigned)kind);
            if (kind == 1) table[size - 1 - (size_t)n] = ZERO;
            if (kind == 2) memset(table + size / 2, 0, size / 2 * sizeof(ogkr_fr));
            if (proof_run(&a, table, n, NULL, 1) || proof_run(&b, table, n, levels, 4) || proof_run(&c, table, n, NULL, 4)) {
                printf("n=%d kind=%d: error return\n", n, kind);
                bad = 1;
            } else {
                if (!proof_same(&a, &b, n) || !proof_same(&a, &c, n)) {
                    printf("n=%d kind=%d: 1 and 4 threads, or with and without levels, differ\n", n, kind);
                    bad = 1;
                }
                if (!chain_matches(&b, table, n, levels)) {
                    printf("n=%d kind=%d: the tree or the chain differs from the one built here\n", n, kind);
                    bad = 1;
                }
                if (kind != 0 && (a.product.l[0] | a.product.l[1] | a.product.l[2] | a.product.l[3])) {
                    printf("n=%d kind=%d: a table with a zero has a non-zero product\n", n, kind);
                    bad = 1;
                }
                if (kind == 2)
                    for (size_t j = 0; j < R; ++j)
                        if (a.len[j] != 1) {
                            printf("n=%d: a zero upper half, but row %zu has length %u\n", n, j, a.len[j]);
                            bad = 1;
                            break;
                        }
            }
            proof_free(&a);
            proof_free(&b);
            proof_free(&c);
            free(table);
            free(levels);
        }
    }
    /* the argument checks */
    {
        const int n = 3;
        ogkr_fr table[8], x[16];
        uint32_t len[2];
        ogkr_fill_table(table, 8, 1);
        void *out[9] = {x, x, x, len, x, x, x, x, NULL};
        if (ogkr_grand_product(table, 2, x, x, x, len, x, x, x, x, NULL, 1) != -1 || ogkr_grand_product(table, 31, x, x, x, len, x, x, x, x, NULL, 1) != -1 ||
            ogkr_grand_product(table, 0, x, x, x, len, x, x, x, x, NULL, 1) != -1 || ogkr_grand_product(table, -1, x, x, x, len, x, x, x, x, NULL, 1) != -1 ||
            ogkr_grand_product(NULL, n, x, x, x, len, x, x, x, x, NULL, 1) != -1) {
            printf("a bad shape was accepted\n");
            bad = 1;
        }
        for (int at = 0; at < 8; ++at) {
            void *o[9];
            memcpy(o, out, sizeof o);
            o[at] = NULL;
            if (ogkr_grand_product(table, n, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], NULL, 1) != -1) {
                printf("a NULL output %d was accepted\n", at);
                bad = 1;
            }
        }
    }
    printf(bad ? "grand_product_selfcheck: FAILED\n" : "grand_product_selfcheck: ok\n");
    return bad;
}
