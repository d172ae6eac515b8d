/* Stand-alone check of ogkr_sumcheck_product (TEST INFRASTRUCTURE ONLY), meant to be built with ogkr.c under
 * -fsanitize=address,undefined (make product_selfcheck): n = 2 .. 10 at degree 1 .. 3, with 1 and with 4 threads.
 * The two runs must give equal bytes, and degree 1 must equal ogkr_sumcheck_mle.  Exit status 1 on a mismatch. */
#include "ogkr.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_N 10
#define MAX_D 3

typedef struct {
    ogkr_fr coeffs[MAX_N * (MAX_D + 1)];
    uint32_t len[MAX_N];
    ogkr_fr r[MAX_N];
    ogkr_fr evals[MAX_D];
} transcript;

static int run(const ogkr_fr *tables, int n, int d, int threads, transcript *out) {
    memset(out, 0, sizeof *out);
    return ogkr_sumcheck_product(tables, n, d, out->coeffs, out->len, out->r, out->evals, threads);
}

int main(void) {
    int bad = 0;
    ogkr_fr *tables = malloc(((size_t)MAX_D << MAX_N) * sizeof(ogkr_fr));
    transcript *a = malloc(sizeof *a), *b = malloc(sizeof *b);
    if (!tables || !a || !b) return 2;
    for (int n = 2; n <= MAX_N; ++n) {
        const size_t len = (size_t)1 << n;
        for (int d = 1; d <= MAX_D; ++d) {
            ogkr_fill_table(tables, (size_t)d * len, 1000u + 16u * (unsigned)n + (unsigned)d);
            /* structure the length rules act on: the second factor ignores x_n, the third ignores x_1 */
            if (d >= 2)
                for (size_t m = 0; m < len / 2; ++m) tables[len + 2 * m + 1] = tables[len + 2 * m];
            if (d >= 3) memcpy(tables + 2 * len + len / 2, tables + 2 * len, len / 2 * sizeof(ogkr_fr));
            if (run(tables, n, d, 1, a) || run(tables, n, d, 4, b)) {
                printf("n=%d degree=%d: error return\n", n, d);
                bad = 1;
                continue;
            }
            if (memcmp(a, b, sizeof *a) != 0) {
                printf("n=%d degree=%d: 1 and 4 threads differ\n", n, d);
                bad = 1;
            }
            if (a->len[n - 1] != (uint32_t)(d >= 2 ? d : 2)) {   /* every factor but the second depends on x_n */
                printf("n=%d degree=%d: last length %u\n", n, d, a->len[n - 1]);
                bad = 1;
            }
            if (d == 1) {
                ogkr_fr c[MAX_N * 2], r[MAX_N];
                uint32_t l[MAX_N];
                if (ogkr_sumcheck_mle(tables, n, c, l, r, 4) || memcmp(c, a->coeffs, (size_t)n * 2 * sizeof(ogkr_fr)) != 0 ||
                    memcmp(l, a->len, (size_t)n * sizeof(uint32_t)) != 0 || memcmp(r, a->r, (size_t)n * sizeof(ogkr_fr)) != 0) {
                    printf("n=%d: degree 1 differs from ogkr_sumcheck_mle\n", n);
                    bad = 1;
                }
            }
        }
    }
    /* the argument checks */
    if (ogkr_sumcheck_product(tables, 1, 1, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_product(tables, 4, 0, a->coeffs, a->len, a->r, a->evals, 1) == 0 ||
        ogkr_sumcheck_product(tables, 4, 4, a->coeffs, a->len, a->r, a->evals, 1) == 0) {
        printf("a bad shape was accepted\n");
        bad = 1;
    }
    free(tables);
    free(a);
    free(b);
    printf(bad ? "product_selfcheck: FAILED\n" : "product_selfcheck: ok\n");
    return bad;
}
