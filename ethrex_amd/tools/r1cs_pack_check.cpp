// Host check of the R1CS matrix packing (csrc/r1cs_pack.h).  For random and
// edge CSR matrices and several (T, chunk) geometries:
//   - unpacking the packed form gives back exactly the multiset of
//     (row, col, coeff) of the CSR;
//   - every row < n_rows sits in exactly one bin (short lane or long list),
//     short rows have length <= T, long rows length > T, and the chunks of
//     a long row tile its entries with no gap and no overlap;
//   - padding is inert: stored as {0, 0} and beyond the lane's length guard;
//   - dictionary ids 0 and 1 are +1 and r-1, and ids are distinct values;
//   - every malformed input the ABI lists is rejected.
//
//   hipcc -x hip --offload-host-only -O2 -std=c++17 -I ../csrc \
//         r1cs_pack_check.cpp -o r1cs_pack_check
//
// Exit status 0 and "all cases agree" when everything holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "r1cs_pack.h"

using namespace em_r1cs;
typedef uint64_t u64;

static u64 rng_s = 0x9e3779b97f4a7c15ull;
static u64 rnd() {
    rng_s ^= rng_s << 13;
    rng_s ^= rng_s >> 7;
    rng_s ^= rng_s << 17;
    return rng_s;
}

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static void to_be(const r1cs_word4 &w, uint8_t *be) {
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 8; b++)
            be[8 * (3 - i) + b] = (uint8_t)(w[i] >> (8 * (7 - b)));
}

static bool lt_r(const r1cs_word4 &w) {
    for (int i = 3; i >= 0; i--) {
        if (w[i] < R1CS_R[i]) return true;
        if (w[i] > R1CS_R[i]) return false;
    }
    return false;
}

static const r1cs_word4 ONE = {1, 0, 0, 0};
static const r1cs_word4 MINUS_ONE = {R1CS_R[0] - 1, R1CS_R[1], R1CS_R[2],
                                     R1CS_R[3]};

// coefficient mix: +1, -1, 0, small, full width
static r1cs_word4 rnd_coeff(int mode) {
    u64 k = mode >= 0 ? (u64)mode : rnd() % 8;
    if (k <= 2) return ONE;
    if (k <= 4) return MINUS_ONE;
    if (k == 5) return r1cs_word4{0, 0, 0, 0};
    if (k == 6) return r1cs_word4{rnd() % 17, 0, 0, 0};
    r1cs_word4 w;
    do {
        w = {rnd(), rnd(), rnd(), rnd() >> 2};
    } while (!lt_r(w));
    return w;
}

struct csr {
    std::vector<u64> offs;
    std::vector<uint32_t> cols;
    std::vector<uint8_t> coeffs;
    std::vector<r1cs_word4> words;
    size_t n_rows() const { return offs.size() - 1; }
};

static csr make_csr(const std::vector<size_t> &lens, size_t n_vars, int mode) {
    csr m;
    m.offs.push_back(0);
    for (size_t len : lens) {
        for (size_t k = 0; k < len; k++) {
            m.cols.push_back((uint32_t)(rnd() % n_vars));
            m.words.push_back(rnd_coeff(mode));
        }
        m.offs.push_back(m.cols.size());
    }
    m.coeffs.resize(32 * m.cols.size() + 32);
    for (size_t e = 0; e < m.words.size(); e++)
        to_be(m.words[e], &m.coeffs[32 * e]);
    m.cols.push_back(0);   // keep data() non-null for empty matrices
    return m;
}

typedef std::tuple<uint32_t, uint32_t, r1cs_word4> term;

static void check_matrix(const char *name, const csr &m, size_t n,
                         size_t n_vars, uint32_t T, uint32_t chunk) {
    r1cs_packed p;
    int rc = r1cs_pack(m.offs.data(), m.cols.data(), m.coeffs.data(),
                       m.n_rows(), n, n_vars, T, chunk, p);
    CHECK(rc == 0, "%s: pack rc %d", name, rc);
    if (rc) return;
    const size_t nnz = (size_t)m.offs.back();
    CHECK(p.nnz == nnz && p.n_rows == m.n_rows(), "%s: counts", name);

    // dictionary
    CHECK(p.dict.size() >= 2 && p.dict[R1CS_ID_ONE] == ONE &&
              p.dict[R1CS_ID_MINUS_ONE] == MINUS_ONE, "%s: ids 0/1", name);
    std::set<r1cs_word4> distinct(p.dict.begin(), p.dict.end());
    CHECK(distinct.size() == p.dict.size(), "%s: duplicate dictionary value",
          name);

    // multiset of terms
    std::vector<term> want, got;
    for (size_t i = 0; i < m.n_rows(); i++)
        for (u64 e = m.offs[i]; e < m.offs[i + 1]; e++)
            want.emplace_back((uint32_t)i, m.cols[e], m.words[e]);
    std::vector<r1cs_triple> un;
    r1cs_unpack(p, un);
    for (const r1cs_triple &t : un) got.emplace_back(t.row, t.col, t.coeff);
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    CHECK(want == got, "%s: unpacked terms differ (%zu vs %zu)", name,
          got.size(), want.size());

    // every row in exactly one bin, on the right side of T
    std::vector<int> seen(m.n_rows(), 0);
    size_t live_lanes = 0;
    for (size_t j = 0; j < p.s_perm.size(); j++) {
        uint32_t row = p.s_perm[j];
        if (row == R1CS_NO_ROW) {
            CHECK(p.s_len[j] == 0, "%s: unused lane with a length", name);
            continue;
        }
        live_lanes++;
        CHECK(row < m.n_rows(), "%s: perm out of range", name);
        if (row >= m.n_rows()) continue;
        seen[row]++;
        u64 len = m.offs[row + 1] - m.offs[row];
        CHECK(p.s_len[j] == len && len <= T, "%s: short row %u len", name, row);
    }
    CHECK(live_lanes == p.n_short, "%s: n_short", name);
    CHECK(p.l_chunk_off.size() == p.l_row.size() + 1, "%s: chunk_off", name);
    size_t pos = 0;
    for (size_t j = 0; j < p.l_row.size(); j++) {
        uint32_t row = p.l_row[j];
        CHECK(row < m.n_rows(), "%s: long row out of range", name);
        if (row >= m.n_rows()) continue;
        seen[row]++;
        u64 len = m.offs[row + 1] - m.offs[row];
        CHECK(len > T, "%s: long row %u is short", name, row);
        u64 sum = 0;
        for (uint32_t c = p.l_chunk_off[j]; c < p.l_chunk_off[j + 1]; c++) {
            CHECK(p.l_chunk[c].off == pos + sum, "%s: chunk gap", name);
            CHECK(p.l_chunk[c].len >= 1 && p.l_chunk[c].len <= chunk,
                  "%s: chunk size", name);
            sum += p.l_chunk[c].len;
        }
        CHECK(sum == len, "%s: chunks of row %u cover %llu of %llu", name, row,
              (unsigned long long)sum, (unsigned long long)len);
        pos += (size_t)len;
    }
    CHECK(pos == p.l_ent.size(), "%s: long entries", name);
    CHECK(p.l_chunk_off.back() == p.l_chunk.size(), "%s: chunk count", name);
    for (size_t i = 0; i < m.n_rows(); i++)
        CHECK(seen[i] == 1, "%s: row %zu in %d bins", name, i, seen[i]);

    // slices: width = longest row, lengths non-increasing, padding {0, 0}
    CHECK(p.s_off.size() == p.n_slices() + 1 && p.s_off[0] == 0, "%s: s_off",
          name);
    size_t padding = 0;
    for (size_t s = 0; s < p.n_slices(); s++) {
        u64 span = p.s_off[s + 1] - p.s_off[s];
        CHECK(span % R1CS_SLICE == 0, "%s: slice span", name);
        u64 width = span / R1CS_SLICE;
        uint32_t longest = 0;
        for (uint32_t lane = 0; lane < R1CS_SLICE; lane++) {
            size_t j = s * R1CS_SLICE + lane;
            longest = std::max(longest, p.s_len[j]);
            if (j) CHECK(p.s_len[j] <= p.s_len[j - 1], "%s: order", name);
            for (u64 k = p.s_len[j]; k < width; k++) {
                const r1cs_entry &e =
                    p.s_ent[(size_t)(p.s_off[s] + k * R1CS_SLICE + lane)];
                CHECK(e.col == 0 && e.id == 0, "%s: padding not blank", name);
                padding++;
            }
        }
        CHECK(width == longest, "%s: slice %zu padded past its longest row",
              name, s);
    }
    CHECK(p.s_off.back() == p.s_ent.size(), "%s: short entries", name);
    CHECK(p.nnz_stored() == nnz + padding, "%s: stored count", name);

    // class order within every stored row: ids 0, then 1, then the rest
    auto cls = [](uint32_t id) { return id < 2 ? (int)id : 2; };
    for (size_t j = 0; j < p.s_perm.size(); j++) {
        size_t s = j / R1CS_SLICE, lane = j % R1CS_SLICE;
        for (uint32_t k = 1; k < p.s_len[j]; k++) {
            const r1cs_entry *b = &p.s_ent[(size_t)p.s_off[s] + lane];
            CHECK(cls(b[(k - 1) * R1CS_SLICE].id) <= cls(b[k * R1CS_SLICE].id),
                  "%s: class order", name);
        }
    }
}

static void expect_reject(const char *name, const u64 *offs,
                          const uint32_t *cols, const uint8_t *coeffs,
                          size_t n_rows, size_t n, size_t n_vars) {
    r1cs_packed p;
    int rc = r1cs_pack(offs, cols, coeffs, n_rows, n, n_vars, 64, 1024, p);
    CHECK(rc == R1CS_ERR_INPUT, "%s: accepted (rc %d)", name, rc);
}

int main() {
    const uint32_t geoms[][2] = {{64, 1024}, {0, 64}, {0xffffffffu, 64},
                                 {7, 64}, {1, 1}, {128, 4096}};
    int cases = 0;
    for (const auto &g : geoms) {
        const uint32_t T = g[0], chunk = g[1];
        // edges
        check_matrix("empty", make_csr({}, 4, -1), 16, 4, T, chunk);
        check_matrix("one", make_csr({1}, 1, -1), 1, 1, T, chunk);
        check_matrix("zero rows", make_csr({0, 0, 0}, 3, -1), 4, 3, T, chunk);
        std::vector<size_t> ramp;
        for (size_t i = 0; i < 64; i++) ramp.push_back(i);
        check_matrix("ramp", make_csr(ramp, 5, -1), 64, 5, T, chunk);
        check_matrix("boundaries",
                     make_csr({1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000,
                               1023, 1024, 1025, 4097, 0, 2},
                              300, -1), 32, 300, T, chunk);
        check_matrix("plus ones", make_csr({3, 3, 70, 3}, 9, 0), 4, 9, T, chunk);
        check_matrix("minus ones", make_csr({3, 3, 70, 3}, 9, 3), 4, 9, T,
                     chunk);
        check_matrix("all distinct", make_csr({50, 50, 200}, 1000, 7), 4, 1000,
                     T, chunk);
        for (size_t rows : {63u, 65u, 321u}) {
            std::vector<size_t> l(rows, 3);
            check_matrix("tails", make_csr(l, 77, -1), 512, 77, T, chunk);
        }
        cases += 11;
        // random
        for (int it = 0; it < 40; it++) {
            size_t rows = rnd() % 300, n_vars = 1 + rnd() % 500;
            std::vector<size_t> l(rows);
            for (size_t &x : l) {
                u64 k = rnd() % 16;
                x = k == 0 ? rnd() % 3000 : k < 4 ? rnd() % 100 : rnd() % 6;
            }
            check_matrix("random", make_csr(l, n_vars, -1), 512, n_vars, T,
                         chunk);
            cases++;
        }
    }

    // malformed inputs
    csr ok = make_csr({2, 3}, 4, -1);
    expect_reject("null offs", nullptr, ok.cols.data(), ok.coeffs.data(), 2, 4, 4);
    expect_reject("null cols", ok.offs.data(), nullptr, ok.coeffs.data(), 2, 4, 4);
    expect_reject("null coeffs", ok.offs.data(), ok.cols.data(), nullptr, 2, 4, 4);
    expect_reject("n_rows > n", ok.offs.data(), ok.cols.data(),
                  ok.coeffs.data(), 2, 1, 4);
    expect_reject("n_vars == 0", ok.offs.data(), ok.cols.data(),
                  ok.coeffs.data(), 2, 4, 0);
    expect_reject("n_vars == 2^32", ok.offs.data(), ok.cols.data(),
                  ok.coeffs.data(), 2, 4, (size_t)1 << 32);
    {
        std::vector<u64> o = ok.offs;
        o[0] = 1;
        expect_reject("offs[0] = 1", o.data(), ok.cols.data(),
                      ok.coeffs.data(), 2, 4, 4);
        o = ok.offs;
        o[1] = 4, o[2] = 3;
        expect_reject("decreasing", o.data(), ok.cols.data(),
                      ok.coeffs.data(), 2, 4, 4);
        // rejected on the offsets alone: no entry array is that long
        o = {0, 1, (u64)1 << 32};
        expect_reject("nnz = 2^32", o.data(), ok.cols.data(),
                      ok.coeffs.data(), 2, 4, 4);
    }
    {
        std::vector<uint32_t> c = ok.cols;
        c[4] = 4;
        expect_reject("col = n_vars", ok.offs.data(), c.data(),
                      ok.coeffs.data(), 2, 4, 4);
        std::vector<uint8_t> k = ok.coeffs;
        r1cs_word4 r = {R1CS_R[0], R1CS_R[1], R1CS_R[2], R1CS_R[3]};
        to_be(r, &k[32 * 3]);
        expect_reject("coeff = r", ok.offs.data(), ok.cols.data(), k.data(), 2,
                      4, 4);
        std::memset(&k[32 * 3], 0xff, 32);
        expect_reject("coeff = 2^256-1", ok.offs.data(), ok.cols.data(),
                      k.data(), 2, 4, 4);
        r[0] -= 1;   // r - 1 is canonical
        to_be(r, &k[32 * 3]);
        r1cs_packed p;
        CHECK(r1cs_pack(ok.offs.data(), ok.cols.data(), k.data(), 2, 4, 4, 64,
                        1024, p) == 0 && p.s_ent.size() == 3 * 64,
              "r - 1 refused");
    }

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("%d matrices packed and unpacked, 12 malformed inputs rejected\n",
                cases);
    std::printf("all cases agree\n");
    return 0;
}
