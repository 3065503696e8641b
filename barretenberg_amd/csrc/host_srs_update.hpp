// host_srs_update.hpp -- the host side of the SRS update (include/bbgpu.h, bbgpu_srs_update): what the GPU entry and its host twin share -- the verdict on
// y, the report, the G2 half (y G2 and y * g2_x, one g2_scalar_mul_affine each) -- the twin's own rows (a curve loop, then a plain double-and-add per row on
// host_g1.hpp: deliberately NOT the split ladder of srs_update.hip, so that the two check each other bit for bit), the proof that an update was one
// (bbgpu_host_srs_update_check: one pairing check of two pairs), and the transcript writer for a string whose secret nobody holds.
// Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_pairing.hpp"
#include "host_srs_check.hpp"

namespace bbgpu {
namespace host {

static const Fq FQ_BETA = { { 0x71930c11d782e155ULL, 0xa6bb947cffbe3323ULL, 0xaa303344d4741444ULL, 0x2c3b3f0d26594943ULL } }; // fq.hpp:53-56 (Montgomery)

// y given in Montgomery form, any representative below 2^256 -> the canonical Montgomery residue; false when y == 0 (mod r)
static inline bool srs_update_secret(const uint64_t y_mont[4], Fr* y)
{
    Fr v;
    memcpy(v.d, y_mont, 32);
    *y = fr_mul(v, fr_one());
    return !fr_is_zero(*y);
}

static inline void g2_to_words(const G2Affine& q, uint64_t out[16])
{
    memcpy(out, q.x.c0.d, 32);
    memcpy(out + 4, q.x.c1.d, 32);
    memcpy(out + 8, q.y.c0.d, 32);
    memcpy(out + 12, q.y.c1.d, 32);
}

// the report with the G2 half filled in: y_g2 = y G2; g2_ok and g2_x_out = y * g2_x when g2_x is given and is what bbgpu_srs_check accepts
static inline void srs_update_report_init(bbgpu_srs_update_report* R, size_t n, size_t first_power, const Fr& y, const uint64_t* g2_x)
{
    memset(R, 0, sizeof(*R));
    R->n = n;
    R->first_power = first_power;
    R->first_bad_point = UINT64_MAX;
    G2Affine q;
    if (g2_scalar_mul_affine(G2_ONE, y, &q)) g2_to_words(q, R->y_g2); // y != 0: never infinity
    R->g2_ok = srs_check_g2_ok(g2_x) ? 1 : 0;
    if (R->g2_ok && g2_scalar_mul_affine(g2_from_words(g2_x), y, &q)) g2_to_words(q, R->g2_x_out);
}

// bbgpu_host_srs_update: rows are the even entries of a 2n-entry endo table; table_out may alias table
static inline int srs_update_host(const uint64_t* table, size_t n, size_t first_power, const Fr& y, uint64_t* table_out, bbgpu_srs_update_report* R)
{
    // the curve test of canonical_rows (host_random_check.hpp): canonical coordinates, y^2 = x^3 + 3
    std::vector<Fq> rows(2 * n);
    for (size_t i = 0; i < n; i++) {
        g1_words_canonical(table + 16 * i, &rows[2 * i], &rows[2 * i + 1]);
        if (!g1_on_curve(rows[2 * i], rows[2 * i + 1]) && R->bad_points++ == 0) R->first_bad_point = i;
    }
    if (R->bad_points) return BBGPU_ERR_ARG;
    fallback_parallel(n, 16, [&](size_t lo, size_t hi) {
        Fr s = fr_pow(y, (uint64_t)first_power + lo);
        for (size_t i = lo; i < hi; i++, s = fr_mul(s, y)) {
            const Fr k = fr_from_mont(s);
            const Xyzz p = { rows[2 * i], rows[2 * i + 1], FQ_ONE, FQ_ONE };
            Xyzz acc = g1_infinity();
            for (int b = 253; b >= 0; --b) {
                acc = g1_dbl(acc);
                if ((k.d[b >> 6] >> (b & 63)) & 1) acc = g1_add(acc, p);
            }
            uint64_t o[12];
            g1_to_normalised(acc, o); // finite: r is prime and k != 0
            Fq x, yy;
            memcpy(x.d, o, 32);
            memcpy(yy.d, o + 4, 32);
            const Fq bx = fq_mul(x, FQ_BETA), ny = fq_neg(yy);
            uint64_t* e = table_out + 16 * i;
            memcpy(e, x.d, 32);
            memcpy(e + 4, yy.d, 32);
            memcpy(e + 8, bx.d, 32);
            memcpy(e + 12, ny.d, 32);
        }
    });
    return BBGPU_OK;
}

// is new_p1 = y old_p1 for the y behind y_g2?  e(old_p1, y G2) e(-new_p1, G2) == 1
static inline bool srs_update_check(const uint64_t old_p1[8], const uint64_t new_p1[8], const uint64_t y_g2[16])
{
    if (!srs_check_g2_ok(y_g2) || g1_words_is_inf(old_p1) || g1_words_is_inf(new_p1)) return false;
    return pair_is_one(old_p1, new_p1, y_g2, &G2_ONE); // (new_p1's y is made canonical before it is negated)
}

// io.hpp:36-135,159-181 restated for WRITING (see bbgpu_transcript_write): the G1 records of entries 2 .. 2 (degree - 1) of the endo table, then G2 and the
// given x G2, then the 64-byte checksum slot.  Returns false on a file error (why: a static string).
static inline bool transcript_write_file(const char* path, const uint64_t* points_endo_table, size_t degree, const G2Affine& xg2, const char** why)
{
    FILE* f = fopen(path, "wb");
    if (!f) {
        *why = "cannot create transcript";
        return false;
    }
    const Fq one_raw = { { 1, 0, 0, 0 } };
    auto put_fq = [&](unsigned char* dst, const uint64_t* mont) {
        Fq v;
        memcpy(v.d, mont, 32);
        v = fq_mul(v, one_raw); // out of Montgomery form
        for (int l = 0; l < 4; l++)
            for (int b = 0; b < 8; b++) dst[l * 8 + b] = (unsigned char)(v.d[l] >> (8 * (7 - b)));
    };
    const uint32_t man[7] = { 0, 1, (uint32_t)(degree - 1), 2, (uint32_t)(degree - 1), 2, 0 };
    unsigned char mb[28];
    for (int i = 0; i < 7; i++)
        for (int b = 0; b < 4; b++) mb[4 * i + b] = (unsigned char)(man[i] >> (8 * (3 - b)));
    bool ok = fwrite(mb, 1, 28, f) == 28;
    std::vector<unsigned char> buf(64 * 4096);
    for (size_t done = 1; ok && done < degree;) {
        const size_t chunk = std::min<size_t>(4096, degree - done);
        for (size_t k = 0; k < chunk; k++) {
            const uint64_t* e = points_endo_table + (done + k) * 16;
            put_fq(&buf[k * 64], e);
            put_fq(&buf[k * 64 + 32], e + 4);
        }
        ok = fwrite(buf.data(), 64, chunk, f) == chunk;
        done += chunk;
    }
    unsigned char g2b[2 * 128 + 64];
    memset(g2b, 0, sizeof(g2b));
    const G2Affine pts[2] = { G2_ONE, xg2 };
    for (int i = 0; i < 2; i++) { // g2::affine_element = {x.c0, x.c1, y.c0, y.c1} (io.hpp:100-135)
        put_fq(g2b + 128 * i, pts[i].x.c0.d);
        put_fq(g2b + 128 * i + 32, pts[i].x.c1.d);
        put_fq(g2b + 128 * i + 64, pts[i].y.c0.d);
        put_fq(g2b + 128 * i + 96, pts[i].y.c1.d);
    }
    ok = ok && fwrite(g2b, 1, sizeof(g2b), f) == sizeof(g2b);
    ok = (fclose(f) == 0) && ok;
    if (!ok) *why = "short write to transcript";
    return ok;
}

} // namespace host
} // namespace bbgpu
