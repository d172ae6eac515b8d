/* Plain-C dense oracle -- see ogkr.h.  TEST INFRASTRUCTURE ONLY. */
#include "ogkr.h"

#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef unsigned __int128 u128;
typedef uint64_t u64;

/* BN254 scalar modulus r (halo2curves bn256::Fr, rust/Cargo.toml:21) */
static const u64 MOD[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL,
                           0x30644e72e131a029ULL};
static const u64 INV = 0xc2e1f593efffffffULL;                       /* -r^{-1} mod 2^64 */
static const u64 R2[4] = {0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL,
                          0x0216d0b17f4e44a5ULL};                   /* 2^512 mod r */
static const u64 ONE[4] = {1, 0, 0, 0};

static inline int geq_mod(const u64 a[4]) {
    for (int i = 3; i >= 0; --i) {
        if (a[i] > MOD[i]) return 1;
        if (a[i] < MOD[i]) return 0;
    }
    return 1;
}

static inline void sub_mod_inplace(u64 a[4]) {
    u64 borrow = 0;
    for (int i = 0; i < 4; ++i) {
        u128 d = (u128)a[i] - MOD[i] - borrow;
        a[i] = (u64)d;
        borrow = (u64)(d >> 64) & 1;
    }
}

static inline void fr_add(const u64 a[4], const u64 b[4], u64 out[4]) {
    u64 carry = 0;
    for (int i = 0; i < 4; ++i) {
        u128 s = (u128)a[i] + b[i] + carry;
        out[i] = (u64)s;
        carry = (u64)(s >> 64);
    }
    /* a, b < r < 2^254 so no carry out of 256 bits */
    if (geq_mod(out)) sub_mod_inplace(out);
}

static inline void fr_sub(const u64 a[4], const u64 b[4], u64 out[4]) {
    u64 borrow = 0;
    for (int i = 0; i < 4; ++i) {
        u128 d = (u128)a[i] - b[i] - borrow;
        out[i] = (u64)d;
        borrow = (u64)(d >> 64) & 1;
    }
    if (borrow) {
        u64 carry = 0;
        for (int i = 0; i < 4; ++i) {
            u128 s = (u128)out[i] + MOD[i] + carry;
            out[i] = (u64)s;
            carry = (u64)(s >> 64);
        }
    }
}

/* Montgomery product a*b*2^-256 mod r (coarsely integrated operand scanning) */
static inline void mont_mul(const u64 a[4], const u64 b[4], u64 out[4]) {
    u64 t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        u64 carry = 0;
        for (int j = 0; j < 4; ++j) {
            u128 p = (u128)a[j] * b[i] + t[j] + carry;
            t[j] = (u64)p;
            carry = (u64)(p >> 64);
        }
        u128 s = (u128)t[4] + carry;
        t[4] = (u64)s;
        t[5] = (u64)(s >> 64);
        u64 m = t[0] * INV;
        u128 p = (u128)m * MOD[0] + t[0];
        carry = (u64)(p >> 64);
        for (int j = 1; j < 4; ++j) {
            p = (u128)m * MOD[j] + t[j] + carry;
            t[j - 1] = (u64)p;
            carry = (u64)(p >> 64);
        }
        s = (u128)t[4] + carry;
        t[3] = (u64)s;
        t[4] = t[5] + (u64)(s >> 64);
    }
    memcpy(out, t, 32);
    if (t[4] || geq_mod(out)) sub_mod_inplace(out);
}

static inline void to_mont(const u64 a[4], u64 out[4]) { mont_mul(a, R2, out); }
static inline void from_mont(const u64 a[4], u64 out[4]) { mont_mul(a, ONE, out); }

/* canonical * canonical -> canonical */
static inline void fr_mul(const u64 a[4], const u64 b[4], u64 out[4]) {
    u64 am[4];
    to_mont(a, am);          /* a R */
    mont_mul(am, b, out);    /* a R b R^-1 = a b */
}

void ogkr_fr_add(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out) { fr_add(a->l, b->l, out->l); }
void ogkr_fr_sub(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out) { fr_sub(a->l, b->l, out->l); }
void ogkr_fr_mul(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out) { fr_mul(a->l, b->l, out->l); }
int ogkr_fr_is_canonical(const ogkr_fr *a) { return !geq_mod(a->l); }

void ogkr_set_threads(int threads) {
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
}

int ogkr_max_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* ---------------------------------------------------------------- keccak-256 */

static const u64 KRC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
    0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
    0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
    0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
static const int KROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
static const int KPIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};

static inline u64 rol64(u64 x, int n) { return (x << n) | (x >> (64 - n)); }

static void keccak_f(u64 st[25]) {
    for (int round = 0; round < 24; ++round) {
        u64 bc[5];
        for (int i = 0; i < 5; ++i) bc[i] = st[i] ^ st[i + 5] ^ st[i + 10] ^ st[i + 15] ^ st[i + 20];
        for (int i = 0; i < 5; ++i) {
            u64 t = bc[(i + 4) % 5] ^ rol64(bc[(i + 1) % 5], 1);
            for (int j = 0; j < 25; j += 5) st[j + i] ^= t;
        }
        u64 t = st[1];
        for (int i = 0; i < 24; ++i) {
            int j = KPIL[i];
            u64 b = st[j];
            st[j] = rol64(t, KROT[i]);
            t = b;
        }
        for (int j = 0; j < 25; j += 5) {
            for (int i = 0; i < 5; ++i) bc[i] = st[j + i];
            for (int i = 0; i < 5; ++i) st[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
        }
        st[0] ^= KRC[round];
    }
}

void ogkr_keccak256(const uint8_t *data, size_t len, uint8_t out[32]) {
    const size_t rate = 136;
    u64 st[25];
    memset(st, 0, sizeof st);
    uint8_t block[136];
    while (len >= rate) {
        for (size_t i = 0; i < rate / 8; ++i) {
            u64 w;
            memcpy(&w, data + 8 * i, 8);
            st[i] ^= w;
        }
        keccak_f(st);
        data += rate;
        len -= rate;
    }
    memset(block, 0, rate);
    memcpy(block, data, len);
    block[len] ^= 0x01;           /* original Keccak padding, not SHA-3's 0x06 */
    block[rate - 1] ^= 0x80;
    for (size_t i = 0; i < rate / 8; ++i) {
        u64 w;
        memcpy(&w, block + 8 * i, 8);
        st[i] ^= w;
    }
    keccak_f(st);
    memcpy(out, st, 32);
}

/* -------------------------------------------------------------------- MiMC7 */

#define MIMC_ROUNDS 91
static u64 CTS_MONT[MIMC_ROUNDS][4];
static int cts_ready = 0;

static void reduce_be32(const uint8_t be[32], u64 out[4]) {
    /* int_big_endian(be) mod r; 2^256 < 6 r so at most five subtractions */
    for (int i = 0; i < 4; ++i) {
        u64 w = 0;
        for (int j = 0; j < 8; ++j) w = (w << 8) | be[8 * (3 - i) + j];
        out[i] = w;
    }
    while (geq_mod(out)) sub_mod_inplace(out);
}

static void init_constants(void) {
#pragma omp critical(ogkr_cts)
    {
        if (!cts_ready) {
            uint8_t h[32];
            ogkr_keccak256((const uint8_t *)"mimc", 4, h);
            memset(CTS_MONT[0], 0, 32);
            for (int i = 1; i < MIMC_ROUNDS; ++i) {
                uint8_t nh[32];
                ogkr_keccak256(h, 32, nh);
                memcpy(h, nh, 32);
                u64 c[4];
                reduce_be32(h, c);
                to_mont(c, CTS_MONT[i]);
            }
            cts_ready = 1;
        }
    }
}

void ogkr_mimc7_constant(int i, ogkr_fr *out) {
    if (!cts_ready) init_constants();
    from_mont(CTS_MONT[i], out->l);
}

/* x, k in Montgomery form; out in Montgomery form */
static void mimc7_hash_mont(const u64 x[4], const u64 k[4], u64 out[4]) {
    u64 h[4] = {0, 0, 0, 0}, t[4], t2[4], t4[4], t6[4];
    for (int i = 0; i < MIMC_ROUNDS; ++i) {
        if (i == 0) {
            fr_add(x, k, t);
        } else {
            fr_add(h, k, t);
            fr_add(t, CTS_MONT[i], t);
        }
        mont_mul(t, t, t2);
        mont_mul(t2, t2, t4);
        mont_mul(t4, t2, t6);
        mont_mul(t6, t, h);
    }
    fr_add(h, k, out);
}

void ogkr_mimc7_hash(const ogkr_fr *x, const ogkr_fr *k, ogkr_fr *out) {
    if (!cts_ready) init_constants();
    u64 xm[4], km[4], hm[4];
    to_mont(x->l, xm);
    to_mont(k->l, km);
    mimc7_hash_mont(xm, km, hm);
    from_mont(hm, out->l);
}

void ogkr_multi_hash(const ogkr_fr *arr, size_t n, const ogkr_fr *key, ogkr_fr *out) {
    if (!cts_ready) init_constants();
    u64 r[4], a[4], h[4];
    to_mont(key->l, r);
    for (size_t i = 0; i < n; ++i) {
        to_mont(arr[i].l, a);
        mimc7_hash_mont(a, r, h);
        fr_add(r, a, r);
        fr_add(r, h, r);
    }
    from_mont(r, out->l);
}

/* ------------------------------------------------------- synthetic workload */

static inline u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

void ogkr_fill_table(ogkr_fr *table, size_t count, uint64_t seed) {
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < count; ++i) {
        for (int j = 0; j < 4; ++j)
            table[i].l[j] = mix64(seed + (4 * (u64)i + (u64)j + 1) * 0x9E3779B97F4A7C15ULL);
        table[i].l[3] &= 0x1FFFFFFFFFFFFFFFULL;
    }
}

/* --------------------------------------------------------- dense sumchecks */

static int set_threads(int threads) {
#ifdef _OPENMP
    int t = threads > 0 ? threads : omp_get_max_threads();
    return t;
#else
    (void)threads;
    return 1;
#endif
}

static void fold_table(u64 (*t)[4], size_t h, const u64 r_mont[4], int nt) {
    /* T[i] <- T[i] + r (T[i+h] - T[i]) */
    (void)nt;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < h; ++i) {
        u64 d[4], p[4];
        fr_sub(t[i + h], t[i], d);
        mont_mul(d, r_mont, p);
        fr_add(t[i], p, t[i]);
    }
}

static int sumcheck_mle_on(u64 (*t)[4], int n, ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, int threads);

int ogkr_sumcheck_mle(const ogkr_fr *table, int n, ogkr_fr *out_coeffs, uint32_t *out_len,
                      ogkr_fr *out_r, int threads) {
    if (n < 2 || n > 40) return -1;
    size_t len = (size_t)1 << n;
    u64(*t)[4] = malloc(len * 32);
    if (!t) return -2;
    memcpy(t, table, len * 32);
    int rc = sumcheck_mle_on(t, n, out_coeffs, out_len, out_r, threads);
    free(t);
    return rc;
}

/* the same on the caller's table, which is overwritten (a 2^30-entry table is 32 GiB: no room for a copy) */
int ogkr_sumcheck_mle_inplace(ogkr_fr *table, int n, ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, int threads) {
    if (n < 2 || n > 40) return -1;
    return sumcheck_mle_on((u64(*)[4])table, n, out_coeffs, out_len, out_r, threads);
}

static int sumcheck_mle_on(u64 (*t)[4], int n, ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, int threads) {
    if (!cts_ready) init_constants();
    int nt = set_threads(threads);
    size_t len = (size_t)1 << n;
    int dep_last = 0;
#pragma omp parallel for schedule(static) num_threads(nt) reduction(| : dep_last)
    for (size_t i = 0; i < len / 2; ++i)
        dep_last |= memcmp(t[2 * i], t[2 * i + 1], 32) != 0;
    const ogkr_fr zero = {{0, 0, 0, 0}};
    for (int j = 0; j < n; ++j) {
        size_t h = len >> (j + 1);
        u64 c0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
#pragma omp parallel num_threads(nt)
        {
            u64 l0[4] = {0, 0, 0, 0}, l1[4] = {0, 0, 0, 0};
#pragma omp for schedule(static) nowait
            for (size_t i = 0; i < h; ++i) {
                fr_add(l0, t[i], l0);
                fr_add(l1, t[i + h], l1);
            }
#pragma omp critical(ogkr_acc)
            {
                fr_add(c0, l0, c0);
                fr_add(s1, l1, s1);
            }
        }
        u64 c1[4];
        fr_sub(s1, c0, c1);
        int c1_zero = !(c1[0] | c1[1] | c1[2] | c1[3]);
        int length = (j < n - 1) ? (c1_zero ? 1 : 2) : (dep_last ? 2 : 1);
        out_len[j] = (uint32_t)length;
        out_coeffs[2 * j] = zero;
        memcpy(out_coeffs[2 * j + 1].l, c0, 32);
        if (length == 2) memcpy(out_coeffs[2 * j].l, c1, 32);
        ogkr_multi_hash(&out_coeffs[2 * j + (2 - length)], (size_t)length, &zero, &out_r[j]);
        u64 rm[4];
        to_mont(out_r[j].l, rm);
        fold_table(t, h, rm, nt);
    }
    return 0;
}

/* prove_sumcheck on g = the product of `degree` multilinear tables (tests/product_model.py restates the rules): round j's
 * polynomial sum_{i<h} prod_f (lo_f + t (hi_f - lo_f)) by EXPANSION -- per index the factors are multiplied out into
 * degree + 1 coefficients, which are summed coefficient by coefficient.  No evaluation points, no interpolation, no
 * division; every sum and product is reduced at once.  The working tables are held in Montgomery form, so a product is
 * one mont_mul; the modular sums are exact, so the result does not depend on the thread count. */
int ogkr_sumcheck_product(const ogkr_fr *tables, int n, int degree, ogkr_fr *out_coeffs, uint32_t *out_len,
                          ogkr_fr *out_r, ogkr_fr *out_evals, int threads) {
    if (n < 2 || n > 40 || degree < 1 || degree > 3) return -1;
    if (!cts_ready) init_constants();
    const int nt = set_threads(threads), d = degree;
    const size_t len = (size_t)1 << n;
    u64(*t)[4] = malloc((size_t)d * len * 32);
    if (!t) return -2;
    /* the structural facts of the input: factors that depend on x_n, and whether a factor is the zero table */
    int ndep = 0, zero_factor = 0;
    for (int f = 0; f < d; ++f) {
        const ogkr_fr *tf = tables + (size_t)f * len;
        int dep = 0, any = 0;
#pragma omp parallel for schedule(static) num_threads(nt) reduction(| : dep, any)
        for (size_t m = 0; m < len / 2; ++m) {
            dep |= memcmp(tf[2 * m].l, tf[2 * m + 1].l, 32) != 0;
            any |= (tf[2 * m].l[0] | tf[2 * m].l[1] | tf[2 * m].l[2] | tf[2 * m].l[3] | tf[2 * m + 1].l[0] | tf[2 * m + 1].l[1] |
                    tf[2 * m + 1].l[2] | tf[2 * m + 1].l[3]) != 0;
        }
        ndep += dep;
        zero_factor |= !any;
    }
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < (size_t)d * len; ++i) to_mont(tables[i].l, t[i]);
    const ogkr_fr zero = {{0, 0, 0, 0}};
    for (int j = 0; j < n; ++j) {
        const size_t h = len >> (j + 1);
        u64 c[4][4];   /* c[k]: coefficient of t^k, Montgomery form */
        memset(c, 0, sizeof c);
#pragma omp parallel num_threads(nt)
        {
            u64 local[4][4];
            memset(local, 0, sizeof local);
#pragma omp for schedule(static) nowait
            for (size_t i = 0; i < h; ++i) {
                u64 poly[4][4], nxt[4][4], diff[4], a[4], b[4];
                /* factor 0: lo + t (hi - lo) */
                memcpy(poly[0], t[i], 32);
                fr_sub(t[i + h], t[i], poly[1]);
                for (int f = 1; f < d; ++f) {   /* poly (degree f) times (lo + t diff) */
                    const u64 *lo = t[(size_t)f * len + i];
                    fr_sub(t[(size_t)f * len + i + h], lo, diff);
                    mont_mul(poly[0], lo, nxt[0]);
                    for (int k = 1; k <= f; ++k) {
                        mont_mul(poly[k], lo, a);
                        mont_mul(poly[k - 1], diff, b);
                        fr_add(a, b, nxt[k]);
                    }
                    mont_mul(poly[f], diff, nxt[f + 1]);
                    memcpy(poly, nxt, (size_t)(f + 2) * 32);
                }
                for (int k = 0; k <= d; ++k) fr_add(local[k], poly[k], local[k]);
            }
#pragma omp critical(ogkr_prod)
            for (int k = 0; k <= d; ++k) fr_add(c[k], local[k], c[k]);
        }
        ogkr_fr *row = out_coeffs + (size_t)j * (d + 1);   /* highest degree first */
        for (int k = 0; k <= d; ++k) from_mont(c[d - k], row[k].l);
        int length;
        if (j < n - 1) {
            length = d + 1;
            while (length > 1 && !(row[d + 1 - length].l[0] | row[d + 1 - length].l[1] | row[d + 1 - length].l[2] | row[d + 1 - length].l[3]))
                --length;
        } else {
            length = zero_factor ? 1 : 1 + ndep;
        }
        for (int k = 0; k < d + 1 - length; ++k) row[k] = zero;   /* (zero already in the last round, by the length rule's own argument) */
        out_len[j] = (uint32_t)length;
        ogkr_multi_hash(row + (d + 1 - length), (size_t)length, &zero, &out_r[j]);
        u64 rm[4];
        to_mont(out_r[j].l, rm);
        for (int f = 0; f < d; ++f) fold_table(t + (size_t)f * len, h, rm, nt);
    }
    for (int f = 0; f < d; ++f) from_mont(t[(size_t)f * len], out_evals[f].l);
    free(t);
    return 0;
}

static void eq_table(int k, const ogkr_fr *z, u64 (*e)[4]) {
    /* e[g] = prod_i (bit_i(g) ? z_i : 1 - z_i), variable 1 = most significant bit */
    memcpy(e[0], ONE, 32);
    size_t cur = 1;
    for (int i = 0; i < k; ++i) {
        u64 zm[4];
        to_mont(z[i].l, zm);
        for (size_t g = cur; g-- > 0;) {
            u64 hi[4], lo[4];
            mont_mul(e[g], zm, hi);      /* e * z (canonical) */
            fr_sub(e[g], hi, lo);        /* e * (1 - z) */
            memcpy(e[2 * g], lo, 32);
            memcpy(e[2 * g + 1], hi, 32);
        }
        cur <<= 1;
    }
}

/* prove_sumcheck on g = sum_k c_k prod_f T_t(k,f) (tests/sop_model.py restates the rules), in ogkr_sumcheck_product's way: per
 * index EVERY term is multiplied out into its degree + 1 coefficients and scaled by c_k, the scaled coefficients are summed
 * exponent by exponent over the terms and the indices, every sum and product reduced at once.  No evaluation points, no
 * interpolation, no division.  The length rule is BY VALUE in every round, the last included: leading zero coefficients are
 * dropped, one is kept at least, so g == 0 gives [0].  Every table folds once per round, whatever number of terms name it.
 * t: the M working tables of `len` entries each in Montgomery form, overwritten; cm: the coefficients in Montgomery form. */
static void sop_on(u64 (*t)[4], size_t len, int n, int M, const ogkr_sop_term *terms, u64 (*cm)[4], int n_terms, int D,
                   ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, ogkr_fr *out_evals, int nt) {
    const ogkr_fr zero = {{0, 0, 0, 0}};
    for (int j = 0; j < n; ++j) {
        const size_t h = len >> (j + 1);
        u64 c[4][4];   /* c[e]: coefficient of X^e, Montgomery form */
        memset(c, 0, sizeof c);
#pragma omp parallel num_threads(nt)
        {
            u64 local[4][4];
            memset(local, 0, sizeof local);
#pragma omp for schedule(static) nowait
            for (size_t i = 0; i < h; ++i) {
                for (int k = 0; k < n_terms; ++k) {
                    const int dk = terms[k].degree;
                    u64 poly[4][4], nxt[4][4], diff[4], a[4], b[4];
                    size_t at = (size_t)terms[k].table[0] * len + i;
                    memcpy(poly[0], t[at], 32);
                    fr_sub(t[at + h], t[at], poly[1]);
                    for (int f = 1; f < dk; ++f) {   /* poly (degree f) times (lo + X diff) */
                        at = (size_t)terms[k].table[f] * len + i;
                        const u64 *lo = t[at];
                        fr_sub(t[at + h], lo, diff);
                        mont_mul(poly[0], lo, nxt[0]);
                        for (int e = 1; e <= f; ++e) {
                            mont_mul(poly[e], lo, a);
                            mont_mul(poly[e - 1], diff, b);
                            fr_add(a, b, nxt[e]);
                        }
                        mont_mul(poly[f], diff, nxt[f + 1]);
                        memcpy(poly, nxt, (size_t)(f + 2) * 32);
                    }
                    for (int e = 0; e <= dk; ++e) {
                        mont_mul(poly[e], cm[k], a);
                        fr_add(local[e], a, local[e]);
                    }
                }
            }
#pragma omp critical(ogkr_sop)
            for (int e = 0; e <= D; ++e) fr_add(c[e], local[e], c[e]);
        }
        ogkr_fr *row = out_coeffs + (size_t)j * (D + 1);   /* highest degree first */
        for (int e = 0; e <= D; ++e) from_mont(c[D - e], row[e].l);
        int length = D + 1;
        while (length > 1 && !(row[D + 1 - length].l[0] | row[D + 1 - length].l[1] | row[D + 1 - length].l[2] | row[D + 1 - length].l[3]))
            --length;
        out_len[j] = (uint32_t)length;
        ogkr_multi_hash(row + (D + 1 - length), (size_t)length, &zero, &out_r[j]);
        u64 rm[4];
        to_mont(out_r[j].l, rm);
        for (int m = 0; m < M; ++m) fold_table(t + (size_t)m * len, h, rm, nt);
    }
    for (int m = 0; m < M; ++m) from_mont(t[(size_t)m * len], out_evals[m].l);
}

/* the largest term degree, or 0 for a term list sop_on must not see */
static int sop_check_terms(int n_tables, const ogkr_sop_term *terms, const ogkr_fr *term_coeffs, int n_terms, int max_degree) {
    if (!terms || !term_coeffs || n_terms < 1 || n_terms > OGKR_SOP_MAX_TERMS) return 0;
    int D = 0;
    for (int k = 0; k < n_terms; ++k) {
        if (terms[k].degree < 1 || terms[k].degree > max_degree || geq_mod(term_coeffs[k].l)) return 0;
        for (int f = 0; f < terms[k].degree; ++f)
            if (terms[k].table[f] >= n_tables) return 0;
        if (terms[k].degree > D) D = terms[k].degree;
    }
    return D;
}

int ogkr_sumcheck_sop(const ogkr_fr *tables, int n, int n_tables, const ogkr_sop_term *terms, const ogkr_fr *term_coeffs,
                      int n_terms, ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, ogkr_fr *out_evals, int threads) {
    if (n < 2 || n > 40 || n_tables < 1 || n_tables > OGKR_SOP_MAX_TABLES) return -1;
    const int D = sop_check_terms(n_tables, terms, term_coeffs, n_terms, 3);
    if (!D) return -1;
    if (!cts_ready) init_constants();
    const int nt = set_threads(threads);
    const size_t len = (size_t)1 << n;
    u64(*t)[4] = malloc((size_t)n_tables * len * 32);
    if (!t) return -2;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < (size_t)n_tables * len; ++i) to_mont(tables[i].l, t[i]);
    u64 cm[OGKR_SOP_MAX_TERMS][4];
    for (int k = 0; k < n_terms; ++k) to_mont(term_coeffs[k].l, cm[k]);
    sop_on(t, len, n, n_tables, terms, cm, n_terms, D, out_coeffs, out_len, out_r, out_evals, nt);
    free(t);
    return 0;
}

/* The zero-check sum_x eq(z, x) g(x) in its EXPLICIT form: eq(z, .) is written out as a table of 2^n entries (eq_table above),
 * put in front of the caller's tables, and ogkr_sumcheck_sop's rounds run on the M + 1 tables with table 0 in front of every
 * term.  (The library and tests/zerocheck_model.py never hold that table; holding it is what makes this an oracle for them.) */
int ogkr_sumcheck_zerocheck(const ogkr_fr *tables, int n, int n_tables, const ogkr_sop_term *terms, const ogkr_fr *term_coeffs,
                            int n_terms, const ogkr_fr *z, ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r,
                            ogkr_fr *out_evals, ogkr_fr *out_eq, int threads) {
    if (n < 2 || n > 40 || n_tables < 1 || n_tables > OGKR_SOP_MAX_TABLES || !z) return -1;
    const int d = sop_check_terms(n_tables, terms, term_coeffs, n_terms, 2);
    if (!d) return -1;
    for (int j = 0; j < n; ++j)
        if (geq_mod(z[j].l)) return -1;
    if (!cts_ready) init_constants();
    const int nt = set_threads(threads), M = n_tables + 1;
    const size_t len = (size_t)1 << n;
    u64(*t)[4] = malloc((size_t)M * len * 32);
    if (!t) return -2;
    eq_table(n, z, t);   /* canonical values */
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < len; ++i) to_mont(t[i], t[i]);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < (size_t)n_tables * len; ++i) to_mont(tables[i].l, t[len + i]);
    ogkr_sop_term lifted[OGKR_SOP_MAX_TERMS];
    u64 cm[OGKR_SOP_MAX_TERMS][4];
    for (int k = 0; k < n_terms; ++k) {
        lifted[k].degree = (uint8_t)(terms[k].degree + 1);
        lifted[k].table[0] = 0;
        for (int f = 0; f < terms[k].degree; ++f) lifted[k].table[f + 1] = (uint8_t)(terms[k].table[f] + 1);
        to_mont(term_coeffs[k].l, cm[k]);
    }
    ogkr_fr evals[OGKR_SOP_MAX_TABLES + 1];
    sop_on(t, len, n, M, lifted, cm, n_terms, d + 1, out_coeffs, out_len, out_r, evals, nt);
    *out_eq = evals[0];
    memcpy(out_evals, evals + 1, (size_t)n_tables * sizeof(ogkr_fr));
    free(t);
    return 0;
}

/* The grand product argument (include/gkr_amd.h, gkr_grand_product*; tests/grand_product_model.py restates the rules) from its
 * parts above: the tree is a loop of ogkr_fr_mul over every level, L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k]; the head is L_2 with
 * zeta_1 = multi_hash(L_2), zeta_2 = multi_hash([zeta_1]); layer k = 2 .. n - 1 is ogkr_sumcheck_zerocheck (the EXPLICIT form)
 * with the one term 1 * T_0 T_1 on the two halves of level k + 1 at z^(k); tau_k = multi_hash([a_k, b_k]),
 * c_{k+1} = a_k + tau_k (b_k - a_k), z^(k+1) = (tau_k, r^(k)).  The levels are kept in one buffer, level k at 2^k - 1: the
 * library's layout for one table, so that level k + 1 IS the layer's two tables one after the other. */
int ogkr_grand_product(const ogkr_fr *table, int n, ogkr_fr *out_product, ogkr_fr *out_head, ogkr_fr *out_coeffs, uint32_t *out_len,
                       ogkr_fr *out_r, ogkr_fr *out_evals, ogkr_fr *out_point, ogkr_fr *out_claim, ogkr_fr *out_levels, int threads) {
    if (n < 3 || n > 30 || !table || !out_product || !out_head || !out_coeffs || !out_len || !out_r || !out_evals || !out_point ||
        !out_claim)
        return -1;
    const ogkr_fr zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}};
    const int nt = set_threads(threads);
    (void)nt;
    const size_t size = (size_t)1 << n;
    ogkr_fr *levels = out_levels ? out_levels : malloc((size - 1) * sizeof(ogkr_fr));
    if (!levels) return -2;
    for (int k = n - 1; k >= 0; --k) {
        const size_t h = (size_t)1 << k;
        const ogkr_fr *up = k + 1 == n ? table : levels + (2 * h - 1);
        ogkr_fr *lvl = levels + (h - 1);
#pragma omp parallel for schedule(static) num_threads(nt)
        for (size_t i = 0; i < h; ++i) ogkr_fr_mul(&up[i], &up[i + h], &lvl[i]);
    }
    *out_product = levels[0];
    memcpy(out_head, levels + 3, 4 * sizeof(ogkr_fr));
    ogkr_fr z[31], eq;
    ogkr_multi_hash(out_head, 4, &zero, &z[0]);
    ogkr_multi_hash(&z[0], 1, &zero, &z[1]);
    const ogkr_sop_term term = {2, {0, 1, 0}};
    int rc = 0;
    for (int k = 2; k < n && !rc; ++k) {
        const size_t row = (size_t)k * (size_t)(k - 1) / 2 - 1;
        const ogkr_fr *up = k + 1 == n ? table : levels + (((size_t)2 << k) - 1);
        ogkr_fr *ab = out_evals + 2 * (size_t)(k - 2), tau, d;
        rc = ogkr_sumcheck_zerocheck(up, k, 2, &term, &one, 1, z, out_coeffs + 4 * row, out_len + row, out_r + row, ab, &eq, threads);
        if (rc) break;
        ogkr_multi_hash(ab, 2, &zero, &tau);
        ogkr_fr_sub(&ab[1], &ab[0], &d);
        ogkr_fr_mul(&tau, &d, &d);
        ogkr_fr_add(&ab[0], &d, out_claim);
        z[0] = tau;
        memcpy(z + 1, out_r + row, (size_t)k * sizeof(ogkr_fr));
    }
    if (!rc) memcpy(out_point, z, (size_t)n * sizeof(ogkr_fr));
    if (!out_levels) free(levels);
    return rc;
}

/* The fractional sum argument (include/gkr_amd.h, gkr_fraction_sum*; tests/fraction_sum_model.py restates the rules) from the
 * parts above, as ogkr_grand_product: the tree is a loop of ogkr_fr_mul / ogkr_fr_add over every level,
 * p_k[i] = p_{k+1}[i] q_{k+1}[i + 2^k] + p_{k+1}[i + 2^k] q_{k+1}[i], q_k[i] = q_{k+1}[i] q_{k+1}[i + 2^k]; the head is
 * (p_2, q_2) with zeta_1 = multi_hash(those 8), zeta_2 = multi_hash([zeta_1]), lambda_2 = multi_hash([zeta_2]); layer k is
 * ogkr_sumcheck_zerocheck (the EXPLICIT form) on T0, T1 = the halves of p_{k+1}, T2, T3 = the halves of q_{k+1} with the terms
 * T0 T3 + T1 T2 + lambda_k T2 T3; tau_k = multi_hash([a0, a1, b0, b1]), cp = a0 + tau (a1 - a0), cq = b0 + tau (b1 - b0),
 * z^(k+1) = (tau_k, r^(k)), lambda_{k+1} = multi_hash([tau_k]).  The levels are kept in one buffer, level k at 2 (2^k - 1), p_k
 * then q_k: the library's layout for one pair, so that level k + 1 IS the layer's four tables one after the other -- as the
 * caller's pair (N then D) is for the last layer. */
int ogkr_fraction_sum(const ogkr_fr *num, const ogkr_fr *den, int n, ogkr_fr *out_sums, ogkr_fr *out_head, ogkr_fr *out_coeffs,
                      uint32_t *out_len, ogkr_fr *out_r, ogkr_fr *out_evals, ogkr_fr *out_point, ogkr_fr *out_claims, ogkr_fr *out_levels,
                      int threads) {
    if (n < 3 || n > 29 || !num || !den || !out_sums || !out_head || !out_coeffs || !out_len || !out_r || !out_evals || !out_point ||
        !out_claims)
        return -1;
    const ogkr_fr zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}};
    const int nt = set_threads(threads);
    (void)nt;
    const size_t size = (size_t)1 << n;
    ogkr_fr *levels = out_levels ? out_levels : malloc(2 * (size - 1) * sizeof(ogkr_fr));
    ogkr_fr *top = malloc(2 * size * sizeof(ogkr_fr));      /* N then D: the last layer's four tables */
    if (!levels || !top) {
        if (!out_levels) free(levels);
        free(top);
        return -2;
    }
    memcpy(top, num, size * sizeof(ogkr_fr));
    memcpy(top + size, den, size * sizeof(ogkr_fr));
    for (int k = n - 1; k >= 0; --k) {
        const size_t h = (size_t)1 << k;
        const ogkr_fr *up = k + 1 == n ? top : levels + 2 * (2 * h - 1), *uq = up + 2 * h;
        ogkr_fr *p = levels + 2 * (h - 1), *q = p + h;
#pragma omp parallel for schedule(static) num_threads(nt)
        for (size_t i = 0; i < h; ++i) {
            ogkr_fr x, y;
            ogkr_fr_mul(&up[i], &uq[i + h], &x);
            ogkr_fr_mul(&up[i + h], &uq[i], &y);
            ogkr_fr_add(&x, &y, &p[i]);
            ogkr_fr_mul(&uq[i], &uq[i + h], &q[i]);
        }
    }
    out_sums[0] = levels[0];
    out_sums[1] = levels[1];
    memcpy(out_head, levels + 6, 8 * sizeof(ogkr_fr));
    ogkr_fr z[30], lam, eq, t[4];
    ogkr_multi_hash(out_head, 8, &zero, &z[0]);
    ogkr_multi_hash(&z[0], 1, &zero, &z[1]);
    ogkr_multi_hash(&z[1], 1, &zero, &lam);
    /* cp_2, cq_2 = p_2~(z^(2)), q_2~(z^(2)): variable 1 is the most significant index bit */
    for (int w = 0; w < 2; ++w) {
        const ogkr_fr *v = out_head + 4 * w;
        for (int i = 0; i < 2; ++i) {
            ogkr_fr d;
            ogkr_fr_sub(&v[i + 2], &v[i], &d);
            ogkr_fr_mul(&z[0], &d, &d);
            ogkr_fr_add(&v[i], &d, &t[i]);
        }
        ogkr_fr_sub(&t[1], &t[0], &t[2]);
        ogkr_fr_mul(&z[1], &t[2], &t[2]);
        ogkr_fr_add(&t[0], &t[2], &out_claims[w]);
    }
    const ogkr_sop_term terms[3] = {{2, {0, 3, 0}}, {2, {1, 2, 0}}, {2, {2, 3, 0}}};
    int rc = 0;
    for (int k = 2; k < n && !rc; ++k) {
        const size_t row = (size_t)k * (size_t)(k - 1) / 2 - 1;
        const ogkr_fr *up = k + 1 == n ? top : levels + 2 * (((size_t)2 << k) - 1);
        const ogkr_fr cf[3] = {one, one, lam};
        ogkr_fr *v = out_evals + 4 * (size_t)(k - 2), tau, d;
        rc = ogkr_sumcheck_zerocheck(up, k, 4, terms, cf, 3, z, out_coeffs + 4 * row, out_len + row, out_r + row, v, &eq, threads);
        if (rc) break;
        ogkr_multi_hash(v, 4, &zero, &tau);
        for (int w = 0; w < 2; ++w) {
            ogkr_fr_sub(&v[2 * w + 1], &v[2 * w], &d);
            ogkr_fr_mul(&tau, &d, &d);
            ogkr_fr_add(&v[2 * w], &d, &out_claims[w]);
        }
        z[0] = tau;
        memcpy(z + 1, out_r + row, (size_t)k * sizeof(ogkr_fr));
        ogkr_multi_hash(&tau, 1, &zero, &lam);
    }
    if (!rc) memcpy(out_point, z, (size_t)n * sizeof(ogkr_fr));
    if (!out_levels) free(levels);
    free(top);
    return rc;
}

/* The lookup argument's multiplicities and pair (include/gkr_amd.h, gkr_lookup*; tests/lookup_model.py restates the rules).
 * Counting is by ORDER: the table's indices sorted by (value, index), a binary search per witness entry for the first index of
 * its value.  No hash table, no slot function, no probe chain. */
static int cmp_fr(const ogkr_fr *a, const ogkr_fr *b) {
    for (int i = 3; i >= 0; --i)
        if (a->l[i] != b->l[i]) return a->l[i] < b->l[i] ? -1 : 1;
    return 0;
}

static const ogkr_fr *sort_table;
static int cmp_index(const void *x, const void *y) {
    const uint32_t a = *(const uint32_t *)x, b = *(const uint32_t *)y;
    const int c = cmp_fr(&sort_table[a], &sort_table[b]);
    return c ? c : (a < b ? -1 : a > b);
}

int ogkr_lookup_multiplicities(const ogkr_fr *witness, int n_w, const ogkr_fr *table, int n_t, ogkr_fr *out_mult, uint32_t *out_missing,
                               uint32_t *out_first_missing) {
    if (n_w < 0 || n_w > 30 || n_t < 0 || n_t > 30 || !witness || !table || !out_mult || !out_missing || !out_first_missing) return -1;
    const size_t nw = (size_t)1 << n_w, nt = (size_t)1 << n_t;
    uint32_t *order = malloc(nt * sizeof(uint32_t));
    uint64_t *count = calloc(nt, sizeof(uint64_t));
    if (!order || !count) {
        free(order);
        free(count);
        return -2;
    }
    for (size_t j = 0; j < nt; ++j) order[j] = (uint32_t)j;
    sort_table = table;       /* (one sort at a time: the callers are single-threaded tests) */
    qsort(order, nt, sizeof(uint32_t), cmp_index);
    uint32_t missing = 0, first = 0xFFFFFFFFu;
    for (size_t i = 0; i < nw; ++i) {
        size_t lo = 0, hi = nt;                    /* the first position whose value is >= W[i] */
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (cmp_fr(&table[order[mid]], &witness[i]) < 0) lo = mid + 1;
            else hi = mid;
        }
        if (lo < nt && cmp_fr(&table[order[lo]], &witness[i]) == 0) {
            ++count[order[lo]];                    /* equal values are in index order: this is the lowest index */
        } else {
            ++missing;
            if (first == 0xFFFFFFFFu) first = (uint32_t)i;
        }
    }
    for (size_t j = 0; j < nt; ++j) {
        const ogkr_fr m = {{count[j], 0, 0, 0}};
        out_mult[j] = m;
    }
    *out_missing = missing;
    *out_first_missing = first;
    free(order);
    free(count);
    return 0;
}

int ogkr_lookup_pair(const ogkr_fr *witness, int n_w, const ogkr_fr *table, int n_t, const ogkr_fr *mult, const ogkr_fr *alpha,
                     ogkr_fr *out_pair) {
    if (n_w < 0 || n_w > 30 || n_t < 0 || n_t > 30 || !witness || !table || !mult || !alpha || !out_pair) return -1;
    const ogkr_fr zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}};
    const size_t nw = (size_t)1 << n_w, nt = (size_t)1 << n_t, half = nw > nt ? nw : nt, size = 2 * half;
    ogkr_fr *N = out_pair, *D = out_pair + size;
    for (size_t i = 0; i < half; ++i) {
        N[i] = i < nw ? one : zero;
        D[i] = one;
        if (i < nw) ogkr_fr_sub(alpha, &witness[i], &D[i]);
        N[half + i] = zero;
        D[half + i] = one;
        if (i < nt) {
            ogkr_fr_sub(&zero, &mult[i], &N[half + i]);
            ogkr_fr_sub(alpha, &table[i], &D[half + i]);
        }
    }
    return 0;
}

/* ------------------------------------------------------------------ R1CS tables
 * The tables of the R1CS zero-check and inner sumcheck (tests/r1cs_rows_model.py, tests/r1cs_cols_model.py and
 * verifier.r1cs_matrix_evals restate the rules) on the flat records as they stand: counts[3 i + m] records for the combination
 * of constraint i in matrix m (A, B, C), one after the other in wires[] / coeffs[].  No row pointers, no column-major form, no
 * coefficient pool, no case for 1 or r - 1; a zero coefficient adds zero and a repeated wire adds twice by itself.  The modular
 * sums are exact, so no result depends on how the constraints are dealt over the threads. */

void ogkr_fr_mul_many(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out, size_t count) {
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < count; ++i) fr_mul(a[i].l, b[i].l, out[i].l);
}

void ogkr_fr_add_many(const ogkr_fr *a, const ogkr_fr *b, ogkr_fr *out, size_t count) {
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < count; ++i) fr_add(a[i].l, b[i].l, out[i].l);
}

/* every wire below n_wires, every coefficient canonical: the number of records, or (size_t)-1 */
static size_t r1cs_check(size_t n_constraints, uint32_t n_wires, const uint32_t *counts, const uint32_t *wires, const ogkr_fr *coeffs) {
    size_t total = 0;
    for (size_t i = 0; i < 3 * n_constraints; ++i) total += counts[i];
    int bad = 0;
#pragma omp parallel for schedule(static) reduction(| : bad)
    for (size_t t = 0; t < total; ++t) bad |= wires[t] >= n_wires || geq_mod(coeffs[t].l);
    return bad ? (size_t)-1 : total;
}

static int all_canonical(const ogkr_fr *v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (geq_mod(v[i].l)) return 0;
    return 1;
}

/* thread `id` of `nt` takes the constraints [*first, *last); *pos is the index of its first record */
static void r1cs_share(size_t n_constraints, const uint32_t *counts, int id, int nt, size_t *first, size_t *last, size_t *pos) {
    *first = n_constraints * (size_t)id / (size_t)nt;
    *last = n_constraints * ((size_t)id + 1) / (size_t)nt;
    size_t p = 0;
    for (size_t i = 0; i < 3 * *first; ++i) p += counts[i];
    *pos = p;
}

int ogkr_r1cs_rows(size_t n_constraints, uint32_t n_wires, const uint32_t *counts, const uint32_t *wires, const ogkr_fr *coeffs,
                   const ogkr_fr *witness, int n, ogkr_fr *out, int threads) {
    if (n < 0 || n > 40 || n_constraints > (size_t)1 << n) return -1;
    if (r1cs_check(n_constraints, n_wires, counts, wires, coeffs) == (size_t)-1 || !all_canonical(witness, n_wires)) return -1;
    const int nt = set_threads(threads);
    const size_t len = (size_t)1 << n;
    u64(*wm)[4] = malloc(((size_t)n_wires + 1) * 32);
    if (!wm) return -2;
    for (size_t y = 0; y < n_wires; ++y) to_mont(witness[y].l, wm[y]);
    memset(out, 0, 3 * len * 32);
#pragma omp parallel num_threads(nt)
    {
#ifdef _OPENMP
        const int id = omp_get_thread_num(), team = omp_get_num_threads();
#else
        const int id = 0, team = 1;
#endif
        size_t first, last, pos;
        r1cs_share(n_constraints, counts, id, team, &first, &last, &pos);
        for (size_t i = first; i < last; ++i)
            for (int m = 0; m < 3; ++m) {
                u64 *dst = out[(size_t)m * len + i].l, p[4];
                for (uint32_t t = 0; t < counts[3 * i + m]; ++t, ++pos) {
                    mont_mul(coeffs[pos].l, wm[wires[pos]], p);   /* c (w R) / R = c w */
                    fr_add(dst, p, dst);
                }
            }
    }
    free(wm);
    return 0;
}

int ogkr_r1cs_cols(size_t n_constraints, uint32_t n_wires, const uint32_t *counts, const uint32_t *wires, const ogkr_fr *coeffs,
                   const ogkr_fr *x, int n_x, const ogkr_fr *rho, int n_y, ogkr_fr *out, int threads) {
    if (n_x < 0 || n_x > 40 || n_y < 0 || n_y > 40 || n_constraints > (size_t)1 << n_x || n_wires > (size_t)1 << n_y) return -1;
    if (r1cs_check(n_constraints, n_wires, counts, wires, coeffs) == (size_t)-1 || !all_canonical(x, (size_t)n_x) || !all_canonical(rho, 3))
        return -1;
    const int nt = set_threads(threads);
    const size_t len = (size_t)1 << n_y;
    u64(*e)[4] = malloc(((size_t)1 << n_x) * 32);
    if (!e) return -2;
    eq_table(n_x, x, e);
    u64 rm[3][4];
    for (int m = 0; m < 3; ++m) to_mont(rho[m].l, rm[m]);
    memset(out, 0, len * 32);
    int no_memory = 0;
#pragma omp parallel num_threads(nt)
    {
#ifdef _OPENMP
        const int id = omp_get_thread_num(), team = omp_get_num_threads();
#else
        const int id = 0, team = 1;
#endif
        /* a table per thread (the cells collide), added into out one thread at a time */
        u64(*mine)[4] = calloc(len, 32);
        if (!mine) {
#pragma omp atomic write
            no_memory = 1;
        } else {
            size_t first, last, pos;
            r1cs_share(n_constraints, counts, id, team, &first, &last, &pos);
            for (size_t i = first; i < last; ++i)
                for (int m = 0; m < 3; ++m) {
                    u64 f[4], fm[4], p[4];
                    mont_mul(e[i], rm[m], f);                     /* rho_m eq(x, i) */
                    to_mont(f, fm);
                    for (uint32_t t = 0; t < counts[3 * i + m]; ++t, ++pos) {
                        mont_mul(coeffs[pos].l, fm, p);
                        fr_add(mine[wires[pos]], p, mine[wires[pos]]);
                    }
                }
#pragma omp critical(ogkr_r1cs_cols)
            for (size_t y = 0; y < n_wires; ++y) fr_add(out[y].l, mine[y], out[y].l);
            free(mine);
        }
    }
    free(e);
    return no_memory ? -2 : 0;
}

int ogkr_r1cs_matrix_evals(size_t n_constraints, uint32_t n_wires, const uint32_t *counts, const uint32_t *wires, const ogkr_fr *coeffs,
                           const ogkr_fr *x, int n_x, const ogkr_fr *y, int n_y, ogkr_fr *out, int threads) {
    if (n_x < 0 || n_x > 40 || n_y < 0 || n_y > 40 || n_constraints > (size_t)1 << n_x || n_wires > (size_t)1 << n_y) return -1;
    if (r1cs_check(n_constraints, n_wires, counts, wires, coeffs) == (size_t)-1 || !all_canonical(x, (size_t)n_x) ||
        !all_canonical(y, (size_t)n_y))
        return -1;
    const int nt = set_threads(threads);
    const size_t len_x = (size_t)1 << n_x, len_y = (size_t)1 << n_y;
    u64(*ex)[4] = malloc(len_x * 32), (*ey)[4] = malloc(len_y * 32);
    if (!ex || !ey) {
        free(ex);
        free(ey);
        return -2;
    }
    eq_table(n_x, x, ex);
    eq_table(n_y, y, ey);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < len_x; ++i) to_mont(ex[i], ex[i]);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t w = 0; w < len_y; ++w) to_mont(ey[w], ey[w]);
    u64 acc[3][4];
    memset(acc, 0, sizeof acc);
#pragma omp parallel num_threads(nt)
    {
#ifdef _OPENMP
        const int id = omp_get_thread_num(), team = omp_get_num_threads();
#else
        const int id = 0, team = 1;
#endif
        u64 local[3][4];
        memset(local, 0, sizeof local);
        size_t first, last, pos;
        r1cs_share(n_constraints, counts, id, team, &first, &last, &pos);
        for (size_t i = first; i < last; ++i)
            for (int m = 0; m < 3; ++m)
                for (uint32_t t = 0; t < counts[3 * i + m]; ++t, ++pos) {
                    u64 p[4], q[4];
                    mont_mul(ex[i], ey[wires[pos]], p);           /* (ex R)(ey R) / R = ex ey R */
                    mont_mul(coeffs[pos].l, p, q);                /* c ex ey */
                    fr_add(local[m], q, local[m]);
                }
#pragma omp critical(ogkr_r1cs_mat)
        for (int m = 0; m < 3; ++m) fr_add(acc[m], local[m], acc[m]);
    }
    for (int m = 0; m < 3; ++m) memcpy(out[m].l, acc[m], 32);
    free(ex);
    free(ey);
    return 0;
}

int ogkr_predicate_tables(int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left,
                          const uint32_t *right, const ogkr_fr *z, ogkr_fr *A, ogkr_fr *M) {
    if (k_i < 0 || k_i > 30 || k_next < 1 || k_next > 15) return -1;
    size_t G = (size_t)1 << k_i, N = (size_t)1 << (2 * k_next);
    u64(*e)[4] = malloc(G * 32);
    if (!e) return -2;
    eq_table(k_i, z, e);
    memset(A, 0, N * 32);
    memset(M, 0, N * 32);
    for (size_t g = 0; g < G; ++g) {
        if (left[g] >> k_next || right[g] >> k_next) {
            free(e);
            return -1;
        }
        size_t idx = ((size_t)left[g] << k_next) | right[g];
        ogkr_fr *dst = gate_type[g] ? &M[idx] : &A[idx];
        fr_add(dst->l, e[g], dst->l);
    }
    free(e);
    return 0;
}

static void depends_on(int k, const ogkr_fr *W, int *dep) {
    size_t n = (size_t)1 << k;
    for (int b = 0; b < k; ++b) {
        size_t bit = (size_t)1 << (k - 1 - b);
        dep[b] = 0;
        for (size_t i = 0; i < n && !dep[b]; ++i)
            if (!(i & bit) && memcmp(W[i].l, W[i ^ bit].l, 32)) dep[b] = 1;
    }
}

int ogkr_sumcheck_layer(int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left,
                        const uint32_t *right, const ogkr_fr *z, const ogkr_fr *W,
                        ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, int threads) {
    if (k_i < 0 || k_i > 30 || k_next < 1 || k_next > 15) return -1;
    if (!cts_ready) init_constants();
    int nt = set_threads(threads);
    const int k = k_next;
    const size_t N = (size_t)1 << (2 * k), mask = ((size_t)1 << k) - 1;
    ogkr_fr *A = malloc(N * 32), *M = malloc(N * 32);
    u64(*F1)[4] = malloc(N * 32), (*F2)[4] = malloc(N * 32);
    if (!A || !M || !F1 || !F2) return -2;
    int rc = ogkr_predicate_tables(k_i, k, gate_type, left, right, z, A, M);
    if (rc) return rc;
    /* F1, F2 hold W in Montgomery form so that mont_mul(canonical, F) is canonical */
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < N; ++i) {
        to_mont(W[i >> k].l, F1[i]);
        to_mont(W[i & mask].l, F2[i]);
    }
    int dep[16];
    depends_on(k, W, dep);
    u64(*a)[4] = (u64(*)[4])A, (*m)[4] = (u64(*)[4])M;
    const ogkr_fr zero = {{0, 0, 0, 0}};
    for (int j = 0; j < 2 * k; ++j) {
        size_t h = N >> (j + 1);
        u64 c0[4] = {0}, c1[4] = {0}, c2[4] = {0};
#pragma omp parallel num_threads(nt)
        {
            u64 l0[4] = {0}, l1[4] = {0}, l2[4] = {0};
#pragma omp for schedule(static) nowait
            for (size_t i = 0; i < h; ++i) {
                u64 da[4], dm[4], dp[4], dq[4], s0[4], ds[4], pq0[4], pq1[4], pq2[4], t0[4], t1[4];
                fr_sub(a[i + h], a[i], da);
                fr_sub(m[i + h], m[i], dm);
                fr_sub(F1[i + h], F1[i], dp);
                fr_sub(F2[i + h], F2[i], dq);
                fr_add(F1[i], F2[i], s0);
                fr_add(dp, dq, ds);
                mont_mul(F1[i], F2[i], pq0);          /* (pR)(qR)/R = pq R */
                mont_mul(F1[i], dq, t0);
                mont_mul(dp, F2[i], t1);
                fr_add(t0, t1, pq1);
                mont_mul(dp, dq, pq2);
                /* c0 += a0 s0 + m0 pq0 */
                mont_mul(a[i], s0, t0);
                mont_mul(m[i], pq0, t1);
                fr_add(l0, t0, l0);
                fr_add(l0, t1, l0);
                /* c1 += a0 ds + da s0 + m0 pq1 + dm pq0 */
                mont_mul(a[i], ds, t0);
                fr_add(l1, t0, l1);
                mont_mul(da, s0, t0);
                fr_add(l1, t0, l1);
                mont_mul(m[i], pq1, t0);
                fr_add(l1, t0, l1);
                mont_mul(dm, pq0, t0);
                fr_add(l1, t0, l1);
                /* c2 += da ds + m0 pq2 + dm pq1 */
                mont_mul(da, ds, t0);
                fr_add(l2, t0, l2);
                mont_mul(m[i], pq2, t0);
                fr_add(l2, t0, l2);
                mont_mul(dm, pq1, t0);
                fr_add(l2, t0, l2);
            }
#pragma omp critical(ogkr_acc3)
            {
                fr_add(c0, l0, c0);
                fr_add(c1, l1, c1);
                fr_add(c2, l2, c2);
            }
        }
        int length = 2 + (dep[j % k] ? 1 : 0);
        out_len[j] = (uint32_t)length;
        memcpy(out_coeffs[3 * j].l, c2, 32);
        memcpy(out_coeffs[3 * j + 1].l, c1, 32);
        memcpy(out_coeffs[3 * j + 2].l, c0, 32);
        if (length == 2) out_coeffs[3 * j] = zero;   /* provably zero; kept zero for a stable layout */
        ogkr_multi_hash(&out_coeffs[3 * j + (3 - length)], (size_t)length, &zero, &out_r[j]);
        u64 rm[4];
        to_mont(out_r[j].l, rm);
        fold_table(a, h, rm, nt);
        fold_table(m, h, rm, nt);
        fold_table(F1, h, rm, nt);
        fold_table(F2, h, rm, nt);
    }
    free(A);
    free(M);
    free(F1);
    free(F2);
    return 0;
}

/* ---------------------------------------- the layer sumcheck in linear time
 * The same transcript as ogkr_sumcheck_layer (prove_sumcheck_opt, rust/src/gkr/sumcheck.rs:36-156) without the
 * 2^{2k}-entry tables, so that it can follow layers of 2^15 .. 2^24 values: the C twin of oracle/gatesum.py.
 *     sum_c f(b, c) = W(b) U(b) + V(b),  U(b) = sum_c [a(b,c) + m(b,c) W(c)],  V(b) = sum_c a(b,c) W(c)
 * are sums over the gate list (sumcheck.rs:50-63 reduces over the same list); with b bound to u the rounds over c
 * run on the single row a_u(c) = sum_b eq(u,b) a(b,c), m_u(c) (sumcheck.rs:97-124).  Field arithmetic is exact, so
 * the round vectors are the field elements the dense form gives: tests/test_oracle_c.py holds the two against each
 * other for every k the dense form can reach. */
static void depends_on_wide(int k, const ogkr_fr *W, int *dep, int nt) {
    size_t n = (size_t)1 << k;
    (void)nt;
    for (int b = 0; b < k; ++b) {
        size_t bit = (size_t)1 << (k - 1 - b);
        int d = 0;
#pragma omp parallel for schedule(static) num_threads(nt) reduction(| : d)
        for (size_t i = 0; i < n; ++i)
            if (!(i & bit) && memcmp(W[i].l, W[i ^ bit].l, 32)) d |= 1;
        dep[b] = d;
    }
}

static void publish_round(int j, int dep_j, const u64 c2[4], const u64 g1[4], const u64 c0[4], ogkr_fr *out_coeffs,
                          uint32_t *out_len, ogkr_fr *out_r) {
    const ogkr_fr zero = {{0, 0, 0, 0}};
    u64 c1[4];
    fr_sub(g1, c0, c1);
    fr_sub(c1, c2, c1);
    int length = 2 + (dep_j ? 1 : 0);
    out_len[j] = (uint32_t)length;
    memcpy(out_coeffs[3 * j].l, c2, 32);
    memcpy(out_coeffs[3 * j + 1].l, c1, 32);
    memcpy(out_coeffs[3 * j + 2].l, c0, 32);
    if (length == 2) out_coeffs[3 * j] = zero;
    ogkr_multi_hash(&out_coeffs[3 * j + (3 - length)], (size_t)length, &zero, &out_r[j]);
}

int ogkr_sumcheck_layer_lin(int k_i, int k_next, const uint8_t *gate_type, const uint32_t *left,
                            const uint32_t *right, const ogkr_fr *z, const ogkr_fr *W,
                            ogkr_fr *out_coeffs, uint32_t *out_len, ogkr_fr *out_r, int threads) {
    if (k_i < 0 || k_i > 30 || k_next < 1 || k_next > 28) return -1;
    if (!cts_ready) init_constants();
    int nt = set_threads(threads);
    const int k = k_next;
    const size_t G = (size_t)1 << k_i, n = (size_t)1 << k;
    for (size_t g = 0; g < G; ++g)
        if (left[g] >> k || right[g] >> k || gate_type[g] > 1) return -1;
    u64(*e)[4] = malloc(G * 32), (*eu)[4] = malloc(n * 32);
    u64(*Wm)[4] = malloc(n * 32), (*Wt)[4] = malloc(n * 32);
    u64(*X)[4] = calloc(n, 32), (*Y)[4] = calloc(n, 32);
    if (!e || !eu || !Wm || !Wt || !X || !Y) return -2;
    eq_table(k_i, z, e);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < n; ++i) {
        to_mont(W[i].l, Wm[i]);
        memcpy(Wt[i], Wm[i], 32);
    }
    int dep[32];
    depends_on_wide(k, W, dep, nt);
    /* U = X, V = Y: one pass over the gates (serial: the cells collide) */
    for (size_t g = 0; g < G; ++g) {
        u64 t[4];
        mont_mul(e[g], Wm[right[g]], t);                 /* eq(z, g) W(right) */
        if (gate_type[g]) {
            fr_add(X[left[g]], t, X[left[g]]);
        } else {
            fr_add(X[left[g]], e[g], X[left[g]]);
            fr_add(Y[left[g]], t, Y[left[g]]);
        }
    }
    /* the k rounds that bind b: g(x) = sum_i W_i(x) U_i(x) + V_i(x) */
    for (int j = 0; j < k; ++j) {
        size_t h = n >> (j + 1);
        u64 c0[4] = {0}, g1[4] = {0}, c2[4] = {0};
#pragma omp parallel num_threads(nt)
        {
            u64 l0[4] = {0}, l1[4] = {0}, l2[4] = {0};
#pragma omp for schedule(static) nowait
            for (size_t i = 0; i < h; ++i) {
                u64 t[4], dw[4], du[4];
                mont_mul(X[i], Wt[i], t);
                fr_add(l0, t, l0);
                fr_add(l0, Y[i], l0);
                mont_mul(X[i + h], Wt[i + h], t);
                fr_add(l1, t, l1);
                fr_add(l1, Y[i + h], l1);
                fr_sub(Wt[i + h], Wt[i], dw);
                fr_sub(X[i + h], X[i], du);
                mont_mul(du, dw, t);
                fr_add(l2, t, l2);
            }
#pragma omp critical(ogkr_lin_b)
            {
                fr_add(c0, l0, c0);
                fr_add(g1, l1, g1);
                fr_add(c2, l2, c2);
            }
        }
        publish_round(j, dep[j], c2, g1, c0, out_coeffs, out_len, out_r);
        u64 rm[4];
        to_mont(out_r[j].l, rm);
        fold_table(X, h, rm, nt);
        fold_table(Y, h, rm, nt);
        fold_table(Wt, h, rm, nt);
    }
    u64 wu[4];                       /* W(u), Montgomery form */
    memcpy(wu, Wt[0], 32);
    /* the rows a_u (X), m_u (Y) */
    eq_table(k, out_r, eu);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (size_t i = 0; i < n; ++i) {
        to_mont(eu[i], eu[i]);
        memset(X[i], 0, 32);
        memset(Y[i], 0, 32);
        memcpy(Wt[i], Wm[i], 32);
    }
    for (size_t g = 0; g < G; ++g) {
        u64 t[4];
        mont_mul(e[g], eu[left[g]], t);                  /* eq(z, g) eq(u, left) */
        u64 *dst = gate_type[g] ? Y[right[g]] : X[right[g]];
        fr_add(dst, t, dst);
    }
    /* the k rounds that bind c on the row at b = u */
    for (int j = 0; j < k; ++j) {
        size_t h = n >> (j + 1);
        u64 c0[4] = {0}, g1[4] = {0}, c2[4] = {0};
#pragma omp parallel num_threads(nt)
        {
            u64 l0[4] = {0}, l1[4] = {0}, l2[4] = {0};
#pragma omp for schedule(static) nowait
            for (size_t i = 0; i < h; ++i) {
                u64 s0[4], s1[4], pq0[4], pq1[4], da[4], dm[4], ds[4], dpq[4], t[4];
                fr_add(wu, Wt[i], s0);
                fr_add(wu, Wt[i + h], s1);
                mont_mul(wu, Wt[i], pq0);
                mont_mul(wu, Wt[i + h], pq1);
                mont_mul(X[i], s0, t);
                fr_add(l0, t, l0);
                mont_mul(Y[i], pq0, t);
                fr_add(l0, t, l0);
                mont_mul(X[i + h], s1, t);
                fr_add(l1, t, l1);
                mont_mul(Y[i + h], pq1, t);
                fr_add(l1, t, l1);
                fr_sub(X[i + h], X[i], da);
                fr_sub(Y[i + h], Y[i], dm);
                fr_sub(s1, s0, ds);
                fr_sub(pq1, pq0, dpq);
                mont_mul(da, ds, t);
                fr_add(l2, t, l2);
                mont_mul(dm, dpq, t);
                fr_add(l2, t, l2);
            }
#pragma omp critical(ogkr_lin_c)
            {
                fr_add(c0, l0, c0);
                fr_add(g1, l1, g1);
                fr_add(c2, l2, c2);
            }
        }
        publish_round(k + j, dep[j], c2, g1, c0, out_coeffs, out_len, out_r);
        u64 rm[4];
        to_mont(out_r[k + j].l, rm);
        fold_table(X, h, rm, nt);
        fold_table(Y, h, rm, nt);
        fold_table(Wt, h, rm, nt);
    }
    free(e);
    free(eu);
    free(Wm);
    free(Wt);
    free(X);
    free(Y);
    return 0;
}

void ogkr_layer_eval(size_t gates, const uint8_t *gate_type, const uint32_t *left,
                     const uint32_t *right, const ogkr_fr *prev, ogkr_fr *out) {
#pragma omp parallel for schedule(static)
    for (size_t g = 0; g < gates; ++g) {
        if (gate_type[g])
            fr_mul(prev[left[g]].l, prev[right[g]].l, out[g].l);
        else
            fr_add(prev[left[g]].l, prev[right[g]].l, out[g].l);
    }
}

void ogkr_mobius(ogkr_fr *vals, int k) {
    size_t n = (size_t)1 << k;
    for (int b = 0; b < k; ++b) {
        size_t bit = (size_t)1 << (k - 1 - b);
#pragma omp parallel for schedule(static)
        for (size_t i = 0; i < n; ++i)
            if (i & bit) fr_sub(vals[i].l, vals[i ^ bit].l, vals[i].l);   /* (reads only entries without the bit) */
    }
}

int ogkr_line_restriction(int k, const ogkr_fr *b, const ogkr_fr *c, const ogkr_fr *W,
                          ogkr_fr *out, uint32_t *out_len) {
    if (k < 0 || k > 24) return -1;
    size_t n = (size_t)1 << k;
    ogkr_fr *co = malloc(n * 32);
    u64(*res)[4] = calloc((size_t)(k + 1), 32);
    u64(*grad)[4] = malloc((size_t)(k + 1) * 32), (*cst)[4] = malloc((size_t)(k + 1) * 32);
    if (!co || !res || !grad || !cst) return -2;
    memcpy(co, W, n * 32);
    ogkr_mobius(co, k);
    for (int j = 0; j < k; ++j) {
        u64 g[4];
        fr_sub(c[j].l, b[j].l, g);
        to_mont(g, grad[j]);
        to_mont(b[j].l, cst[j]);
    }
    /* res[d] = coefficient of t^d (ascending while accumulating); every monomial expanded along the line, as the
     * reference does (poly.rs:476-497); the monomials are independent, so they are dealt over the threads */
    int maxdeg = 0;
#pragma omp parallel
    {
        u64 poly[32][4], lres[32][4];
        int lmax = 0;
        memset(lres, 0, sizeof lres);
#pragma omp for schedule(dynamic, 1024) nowait
        for (size_t mono = 0; mono < n; ++mono) {
            const u64 *cf = co[mono].l;
            if (!(cf[0] | cf[1] | cf[2] | cf[3])) continue;
            int deg = 0;
            memcpy(poly[0], cf, 32);
            for (int j = 0; j < k; ++j) {
                if (!((mono >> (k - 1 - j)) & 1)) continue;
                /* poly *= (grad_j t + cst_j) */
                memset(poly[deg + 1], 0, 32);
                for (int d = deg + 1; d >= 1; --d) {
                    u64 x[4], y[4];
                    mont_mul(poly[d - 1], grad[j], x);
                    mont_mul(poly[d], cst[j], y);
                    fr_add(x, y, poly[d]);
                }
                u64 y0[4];
                mont_mul(poly[0], cst[j], y0);
                memcpy(poly[0], y0, 32);
                ++deg;
            }
            if (deg > lmax) lmax = deg;
            for (int d = 0; d <= deg; ++d) fr_add(lres[d], poly[d], lres[d]);
        }
#pragma omp critical(ogkr_line)
        {
            if (lmax > maxdeg) maxdeg = lmax;
            for (int d = 0; d <= k; ++d) fr_add(res[d], lres[d], res[d]);
        }
    }
    *out_len = (uint32_t)(maxdeg + 1);
    for (int d = 0; d <= k; ++d) memcpy(out[k - d].l, res[d], 32);   /* highest first, right-aligned */
    free(co);
    free(res);
    free(grad);
    free(cst);
    return 0;
}
