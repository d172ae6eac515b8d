/* Stand-alone check of ogkr_fraction_sum, ogkr_lookup_multiplicities and ogkr_lookup_pair (TEST INFRASTRUCTURE ONLY), meant to be
 * built with ogkr.c under -fsanitize=address,undefined (make fraction_sum_selfcheck): n = 3 .. 10 on a random pair, a pair with
 * zero numerators, a pair with one zero denominator and a lookup's pair (built by the two lookup functions, the witness side
 * padded), with 1 and with 4 threads, with and without the levels.  The runs must give equal bytes; the levels, the head, every
 * layer and the chain of points, lambdas and claims must be what this program gets from a tree of its own and one
 * ogkr_sumcheck_zerocheck call per layer; a lookup's sum is P = 0.  The multiplicities are held to a count by comparing every
 * witness entry with every table entry, the pair to its rule entry by entry.  Every output buffer is allocated at its exact size,
 * so a write past a row is a report.  Exit status 1 on a mismatch. */
#include "ogkr.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_N 10

typedef struct {
    ogkr_fr sums[2], head[8], claims[2];
    ogkr_fr *coeffs, *r, *evals, *point;
    uint32_t *len;
} proof;

static const ogkr_fr ZERO = {{0, 0, 0, 0}}, ONE = {{1, 0, 0, 0}};

static size_t rounds(int n) { return (size_t)n * (size_t)(n - 1) / 2 - 1; }

static int is_zero(const ogkr_fr *a) { return !(a->l[0] | a->l[1] | a->l[2] | a->l[3]); }

static int proof_alloc(proof *p, int n) {
    const size_t R = rounds(n);
    memset(p, 0, sizeof *p);
    p->coeffs = calloc(4 * R, sizeof(ogkr_fr));
    p->r = calloc(R, sizeof(ogkr_fr));
    p->evals = calloc(4 * (size_t)(n - 2), sizeof(ogkr_fr));
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

static int proof_run(proof *p, const ogkr_fr *pair, int n, ogkr_fr *levels, int threads) {
    return ogkr_fraction_sum(pair, pair + ((size_t)1 << n), n, p->sums, p->head, p->coeffs, p->len, p->r, p->evals, p->point, p->claims, levels,
                             threads);
}

static int proof_same(const proof *a, const proof *b, int n) {
    const size_t R = rounds(n);
    return !memcmp(a->sums, b->sums, sizeof a->sums) && !memcmp(a->head, b->head, sizeof a->head) &&
           !memcmp(a->claims, b->claims, sizeof a->claims) && !memcmp(a->coeffs, b->coeffs, 4 * R * sizeof(ogkr_fr)) &&
           !memcmp(a->r, b->r, R * sizeof(ogkr_fr)) && !memcmp(a->evals, b->evals, 4 * (size_t)(n - 2) * sizeof(ogkr_fr)) &&
           !memcmp(a->point, b->point, (size_t)n * sizeof(ogkr_fr)) && !memcmp(a->len, b->len, R * sizeof(uint32_t));
}

/* a + t (b - a) */
static void lerp(const ogkr_fr *a, const ogkr_fr *b, const ogkr_fr *t, ogkr_fr *out) {
    ogkr_fr d;
    ogkr_fr_sub(b, a, &d);
    ogkr_fr_mul(t, &d, &d);
    ogkr_fr_add(a, &d, out);
}

/* the chain once more, on a tree built here level by level (each level its own allocation: p_k then q_k) */
static int chain_matches(const proof *p, const ogkr_fr *pair, int n, const ogkr_fr *levels) {
    ogkr_fr *lv[MAX_N + 1];
    int ok = 1;
    lv[n] = malloc(((size_t)2 << n) * sizeof(ogkr_fr));
    if (!lv[n]) return 0;
    memcpy(lv[n], pair, ((size_t)2 << n) * sizeof(ogkr_fr));
    for (int k = n - 1; k >= 0; --k) {
        const size_t h = (size_t)1 << k;
        const ogkr_fr *up = lv[k + 1], *uq = lv[k + 1] + 2 * h;
        lv[k] = malloc(2 * h * sizeof(ogkr_fr));
        if (!lv[k]) return 0;
        for (size_t i = 0; i < h; ++i) {
            ogkr_fr x, y;
            ogkr_fr_mul(&up[i], &uq[i + h], &x);
            ogkr_fr_mul(&up[i + h], &uq[i], &y);
            ogkr_fr_add(&x, &y, &lv[k][i]);
            ogkr_fr_mul(&uq[i], &uq[i + h], &lv[k][h + i]);
        }
        if (memcmp(lv[k], levels + 2 * (h - 1), 2 * h * sizeof(ogkr_fr)) != 0) ok = 0;
    }
    if (memcmp(lv[0], p->sums, sizeof p->sums) != 0 || memcmp(lv[2], p->head, sizeof p->head) != 0) ok = 0;
    ogkr_fr z[MAX_N + 1], lam, claims[2], t[2];
    ogkr_multi_hash(lv[2], 8, &ZERO, &z[0]);
    ogkr_multi_hash(&z[0], 1, &ZERO, &z[1]);
    ogkr_multi_hash(&z[1], 1, &ZERO, &lam);
    for (int w = 0; w < 2; ++w) {
        const ogkr_fr *v = lv[2] + 4 * w;
        lerp(&v[0], &v[2], &z[0], &t[0]);
        lerp(&v[1], &v[3], &z[0], &t[1]);
        lerp(&t[0], &t[1], &z[1], &claims[w]);
    }
    const ogkr_sop_term terms[3] = {{2, {0, 3, 0}}, {2, {1, 2, 0}}, {2, {2, 3, 0}}};
    for (int k = 2; k < n; ++k) {
        const size_t row = (size_t)k * (size_t)(k - 1) / 2 - 1;
        ogkr_fr *c = calloc(4 * (size_t)k, sizeof(ogkr_fr)), *r = calloc((size_t)k, sizeof(ogkr_fr)), v[4], eq, tau;
        uint32_t *len = calloc((size_t)k, sizeof(uint32_t));
        const ogkr_fr cf[3] = {ONE, ONE, lam};
        if (!c || !r || !len) return 0;
        if (ogkr_sumcheck_zerocheck(lv[k + 1], k, 4, terms, cf, 3, z, c, len, r, v, &eq, 1)) ok = 0;
        if (memcmp(c, p->coeffs + 4 * row, 4 * (size_t)k * sizeof(ogkr_fr)) != 0 || memcmp(len, p->len + row, (size_t)k * sizeof(uint32_t)) != 0 ||
            memcmp(r, p->r + row, (size_t)k * sizeof(ogkr_fr)) != 0 || memcmp(v, p->evals + 4 * (size_t)(k - 2), sizeof v) != 0)
            ok = 0;
        ogkr_multi_hash(v, 4, &ZERO, &tau);
        lerp(&v[0], &v[1], &tau, &claims[0]);
        lerp(&v[2], &v[3], &tau, &claims[1]);
        z[0] = tau;
        memcpy(z + 1, r, (size_t)k * sizeof(ogkr_fr));
        ogkr_multi_hash(&tau, 1, &ZERO, &lam);
        free(c);
        free(r);
        free(len);
    }
    if (memcmp(z, p->point, (size_t)n * sizeof(ogkr_fr)) != 0 || memcmp(claims, p->claims, sizeof claims) != 0) ok = 0;
    for (int k = 0; k <= n; ++k) free(lv[k]);
    return ok;
}

/* a lookup's pair of 2^n entries from the two lookup functions: n_t = n - 1, n_w = n - 2 (the witness half is half padding), the
 * table with repeated values, and (with_miss) one witness value outside it.  Both are held to their rules here. */
static int lookup_pair(ogkr_fr *pair, int n, unsigned seed, int with_miss) {
    const int n_w = n - 2, n_t = n - 1;
    const size_t nw = (size_t)1 << n_w, nt = (size_t)1 << n_t, size = (size_t)1 << n;
    ogkr_fr *W = malloc(nw * sizeof(ogkr_fr)), *T = malloc((nt + 2) * sizeof(ogkr_fr)), *M = malloc(nt * sizeof(ogkr_fr)), alpha, outside;
    uint32_t missing = 7, first = 7;
    int ok = 1;
    if (!W || !T || !M) return 0;
    ogkr_fill_table(T, nt + 2, seed);
    alpha = T[nt];
    outside = T[nt + 1];
    T[nt - 1] = T[0];                                       /* a value at the first and the last index */
    if (nt >= 4) T[2] = T[1];
    for (size_t i = 0; i < nw; ++i) W[i] = T[(i * 7 + 3) % nt];
    if (with_miss) W[nw - 1] = outside;
    if (ogkr_lookup_multiplicities(W, n_w, T, n_t, M, &missing, &first)) ok = 0;
    size_t sum = 0;
    for (size_t j = 0; j < nt; ++j) {
        size_t want = 0, lowest = j;
        for (size_t u = 0; u < j; ++u)
            if (!memcmp(&T[u], &T[j], sizeof T[j])) {
                lowest = u;
                break;
            }
        if (lowest == j)
            for (size_t i = 0; i < nw; ++i) want += !memcmp(&W[i], &T[j], sizeof T[j]);
        if (M[j].l[0] != want || M[j].l[1] || M[j].l[2] || M[j].l[3]) ok = 0;
        sum += want;
    }
    if (sum + (size_t)with_miss != nw || missing != (uint32_t)with_miss || first != (with_miss ? (uint32_t)(nw - 1) : 0xFFFFFFFFu)) ok = 0;
    if (ogkr_lookup_pair(W, n_w, T, n_t, M, &alpha, pair)) ok = 0;
    const ogkr_fr *N = pair, *D = pair + size;
    for (size_t i = 0; i < size / 2; ++i) {
        ogkr_fr d, m;
        ogkr_fr_sub(&alpha, i < nw ? &W[i] : &ZERO, &d);
        if (memcmp(&N[i], i < nw ? &ONE : &ZERO, sizeof N[i]) != 0 || memcmp(&D[i], i < nw ? &d : &ONE, sizeof d) != 0) ok = 0;
        ogkr_fr_sub(&alpha, &T[i], &d);                    /* (n_t = n - 1: the table half has no padding) */
        ogkr_fr_add(&N[size / 2 + i], &M[i], &m);
        if (!is_zero(&m) || memcmp(&D[size / 2 + i], &d, sizeof d) != 0) ok = 0;
    }
    free(W);
    free(T);
    free(M);
    return ok;
}

int main(void) {
    int bad = 0;
    for (int n = 3; n <= MAX_N; ++n) {
        const size_t size = (size_t)1 << n;
        for (int kind = 0; kind < 5; ++kind) {
            ogkr_fr *pair = malloc(2 * size * sizeof(ogkr_fr)), *levels = malloc(2 * (size - 1) * sizeof(ogkr_fr));
            proof a, b, c;
            if (!pair || !levels || !proof_alloc(&a, n) || !proof_alloc(&b, n) || !proof_alloc(&c, n)) return 2;
            ogkr_fill_table(pair, 2 * size, 6000u + 16u * (unsigned)n + (unsigned)kind);
            if (kind == 1) memset(pair, 0, size * sizeof(ogkr_fr));
            if (kind == 2) pair[2 * size - 1 - (size_t)n] = ZERO;
            if (kind >= 3 && !lookup_pair(pair, n, 6100u + (unsigned)n, kind == 4)) {
                printf("n=%d kind=%d: the multiplicities or the pair differ from their rules\n", n, kind);
                bad = 1;
            }
            if (proof_run(&a, pair, n, NULL, 1) || proof_run(&b, pair, n, levels, 4) || proof_run(&c, pair, n, NULL, 4)) {
                printf("n=%d kind=%d: error return\n", n, kind);
                bad = 1;
            } else {
                if (!proof_same(&a, &b, n) || !proof_same(&a, &c, n)) {
                    printf("n=%d kind=%d: 1 and 4 threads, or with and without levels, differ\n", n, kind);
                    bad = 1;
                }
                if (!chain_matches(&b, pair, n, levels)) {
                    printf("n=%d kind=%d: the tree or the chain differs from the one built here\n", n, kind);
                    bad = 1;
                }
                if ((kind == 1 && !is_zero(&a.sums[0])) || (kind == 2 && !is_zero(&a.sums[1]))) {
                    printf("n=%d kind=%d: zero numerators or a zero denominator, but a non-zero sum\n", n, kind);
                    bad = 1;
                }
                if (kind >= 3 && (is_zero(&a.sums[0]) != (kind == 3) || is_zero(&a.sums[1]))) {
                    printf("n=%d kind=%d: P = 0 exactly for the lookup that holds, Q != 0\n", n, kind);
                    bad = 1;
                }
            }
            proof_free(&a);
            proof_free(&b);
            proof_free(&c);
            free(pair);
            free(levels);
        }
    }
    /* the argument checks */
    {
        const int n = 3;
        ogkr_fr pair[16], x[16];
        uint32_t len[2], u;
        ogkr_fill_table(pair, 16, 1);
        void *out[8] = {x, x, x, len, x, x, x, x};
        const int shapes[] = {2, 30, 0, -1};
        for (size_t s = 0; s < sizeof shapes / sizeof shapes[0]; ++s)
            if (ogkr_fraction_sum(pair, pair + 8, shapes[s], x, x, x, len, x, x, x, x, NULL, 1) != -1) {
                printf("n = %d was accepted\n", shapes[s]);
                bad = 1;
            }
        if (ogkr_fraction_sum(NULL, pair + 8, n, x, x, x, len, x, x, x, x, NULL, 1) != -1 ||
            ogkr_fraction_sum(pair, NULL, n, x, x, x, len, x, x, x, x, NULL, 1) != -1) {
            printf("a NULL table was accepted\n");
            bad = 1;
        }
        for (int at = 0; at < 8; ++at) {
            void *o[8];
            memcpy(o, out, sizeof o);
            o[at] = NULL;
            if (ogkr_fraction_sum(pair, pair + 8, n, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], NULL, 1) != -1) {
                printf("a NULL output %d was accepted\n", at);
                bad = 1;
            }
        }
        if (ogkr_lookup_multiplicities(NULL, 2, pair, 2, x, &u, &u) != -1 || ogkr_lookup_multiplicities(pair, 2, NULL, 2, x, &u, &u) != -1 ||
            ogkr_lookup_multiplicities(pair, 2, pair, 2, NULL, &u, &u) != -1 || ogkr_lookup_multiplicities(pair, 2, pair, 2, x, NULL, &u) != -1 ||
            ogkr_lookup_multiplicities(pair, 2, pair, 2, x, &u, NULL) != -1 || ogkr_lookup_multiplicities(pair, -1, pair, 2, x, &u, &u) != -1 ||
            ogkr_lookup_multiplicities(pair, 2, pair, 31, x, &u, &u) != -1 || ogkr_lookup_pair(NULL, 2, pair, 2, pair, pair, x) != -1 ||
            ogkr_lookup_pair(pair, 2, NULL, 2, pair, pair, x) != -1 || ogkr_lookup_pair(pair, 2, pair, 2, NULL, pair, x) != -1 ||
            ogkr_lookup_pair(pair, 2, pair, 2, pair, NULL, x) != -1 || ogkr_lookup_pair(pair, 2, pair, 2, pair, pair, NULL) != -1 ||
            ogkr_lookup_pair(pair, 31, pair, 2, pair, pair, x) != -1 || ogkr_lookup_pair(pair, 2, pair, -1, pair, pair, x) != -1) {
            printf("a bad argument of a lookup function was accepted\n");
            bad = 1;
        }
    }
    printf(bad ? "fraction_sum_selfcheck: FAILED\n" : "fraction_sum_selfcheck: ok\n");
    return bad;
}
