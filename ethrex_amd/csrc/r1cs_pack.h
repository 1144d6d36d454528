// ============================================================================
// Host packing of one sparse R1CS matrix (CSR in, device layout out) for the
// A*z / B*z / C*z kernels of r1cs_kernels.h.  Plain C++: no HIP, no device
// types — ethrex_amd/tools/r1cs_pack_check.cpp runs it on the host alone.
//
// Packed form (DESIGN.md "R1CS evaluation"):
//   dictionary  distinct coefficient values, canonical, 4 x u64 little-endian
//               words; id 0 = +1 and id 1 = r-1 are always present.  A stored
//               nonzero is {u32 col, u32 id}: 8 B.
//   short bin   rows of length <= T, ordered by length (longest first, ties
//               by row index) and cut into slices of 64 rows = one wave.
//               Slice s holds width_s = its longest row entries per lane,
//               stored [k][lane]: s_ent[s_off[s] + 64*k + lane].  s_len is
//               the true length of the lane's row — entries at k >= s_len
//               are padding ({0, 0}) and are never read as terms (length
//               guard).  s_perm is the lane's original row, R1CS_NO_ROW for
//               the unused lanes of the last slice.  Empty rows are short.
//   long bin    rows of length > T.  Their entries are stored row after row
//               in l_ent and cut into chunks of at most `chunk` entries; the
//               chunks of long row j are l_chunk[l_chunk_off[j] ..
//               l_chunk_off[j+1]).  One wave sums a chunk, a second step
//               sums the partials of a row.
// Within a row the entries are ordered by class: id 0, id 1, then the rest
// in CSR order, so the lanes of a wave tend to branch alike at equal k.
// ============================================================================
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace em_r1cs {

constexpr uint32_t R1CS_NO_ROW = 0xffffffffu;
constexpr uint32_t R1CS_SLICE = 64;          // rows per slice = one wave
constexpr uint32_t R1CS_ID_ONE = 0;          // +1
constexpr uint32_t R1CS_ID_MINUS_ONE = 1;    // r - 1
constexpr int R1CS_ERR_INPUT = 2;            // EM_ERR_INPUT

// BN254 Fr modulus r, little-endian u64 words
constexpr uint64_t R1CS_R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull,
                                0xb85045b68181585dull, 0x30644e72e131a029ull};

using r1cs_word4 = std::array<uint64_t, 4>;

struct r1cs_entry {
    uint32_t col, id;
};
struct r1cs_chunk {
    uint32_t off, len;   // entries l_ent[off, off + len)
};

struct r1cs_packed {
    size_t n_rows = 0, nnz = 0;
    uint32_t T = 0, chunk = 0;
    std::vector<r1cs_word4> dict;
    // short bin
    uint32_t n_short = 0;
    std::vector<uint32_t> s_perm, s_len;   // n_slices * 64
    std::vector<uint64_t> s_off;           // n_slices + 1
    std::vector<r1cs_entry> s_ent;
    // long bin
    std::vector<uint32_t> l_row;           // n_long
    std::vector<uint32_t> l_chunk_off;     // n_long + 1
    std::vector<r1cs_chunk> l_chunk;
    std::vector<r1cs_entry> l_ent;

    size_t n_slices() const { return s_perm.size() / R1CS_SLICE; }
    size_t nnz_stored() const { return s_ent.size() + l_ent.size(); }
};

struct r1cs_triple {
    uint32_t row, col;
    r1cs_word4 coeff;
};

struct r1cs_word4_hash {
    size_t operator()(const r1cs_word4 &w) const {
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (uint64_t x : w) h = (h ^ x) * 0xff51afd7ed558ccdull + (h >> 29);
        return (size_t)h;
    }
};

// 32 big-endian bytes -> little-endian words; false if the value is >= r
static inline bool r1cs_parse_be(const uint8_t *be, r1cs_word4 &out) {
    for (int i = 0; i < 4; i++) {
        uint64_t w = 0;
        for (int b = 0; b < 8; b++) w = (w << 8) | be[8 * (3 - i) + b];
        out[i] = w;
    }
    for (int i = 3; i >= 0; i--) {
        if (out[i] < R1CS_R[i]) return true;
        if (out[i] > R1CS_R[i]) return false;
    }
    return false;
}

// Validate a CSR matrix and pack it.  Returns 0, or R1CS_ERR_INPUT for: a
// null pointer, n_rows > n, n_vars == 0 or >= 2^32, row_offs[0] != 0, a
// decreasing offset, nnz >= 2^32, a column >= n_vars, a coefficient >= r.
// The offsets are checked before any entry is read.  T: longest short row;
// chunk >= 1: entries per long-row chunk.  `out` is meaningful on 0 only.
static inline int r1cs_pack(const uint64_t *row_offs, const uint32_t *cols,
                            const uint8_t *coeffs32, size_t n_rows, size_t n,
                            size_t n_vars, uint32_t T, uint32_t chunk,
                            r1cs_packed &out) {
    if (!row_offs || !cols || !coeffs32) return R1CS_ERR_INPUT;
    if (n_rows > n || n_vars == 0 || n_vars >= ((size_t)1 << 32) || chunk == 0)
        return R1CS_ERR_INPUT;
    if (row_offs[0] != 0) return R1CS_ERR_INPUT;
    for (size_t i = 0; i < n_rows; i++)
        if (row_offs[i + 1] < row_offs[i]) return R1CS_ERR_INPUT;
    const uint64_t nnz = row_offs[n_rows];
    if (nnz >= ((uint64_t)1 << 32)) return R1CS_ERR_INPUT;

    out = r1cs_packed();
    out.n_rows = n_rows;
    out.nnz = (size_t)nnz;
    out.T = T;
    out.chunk = chunk;

    // dictionary + per-entry ids
    std::unordered_map<r1cs_word4, uint32_t, r1cs_word4_hash> ids;
    r1cs_word4 one = {1, 0, 0, 0};
    r1cs_word4 minus_one = {R1CS_R[0] - 1, R1CS_R[1], R1CS_R[2], R1CS_R[3]};
    out.dict = {one, minus_one};
    ids.emplace(one, R1CS_ID_ONE);
    ids.emplace(minus_one, R1CS_ID_MINUS_ONE);
    std::vector<uint32_t> id_of((size_t)nnz);
    for (size_t e = 0; e < (size_t)nnz; e++) {
        if (cols[e] >= n_vars) return R1CS_ERR_INPUT;
        r1cs_word4 w;
        if (!r1cs_parse_be(coeffs32 + 32 * e, w)) return R1CS_ERR_INPUT;
        auto it = ids.find(w);
        if (it == ids.end()) {
            it = ids.emplace(w, (uint32_t)out.dict.size()).first;
            out.dict.push_back(w);
        }
        id_of[e] = it->second;
    }

    // the entries of row i in class order: +1, -1, general (CSR order within)
    auto emit_row = [&](size_t i, r1cs_entry *dst, size_t stride) {
        size_t k = 0;
        for (int cls = 0; cls < 3; cls++)
            for (uint64_t e = row_offs[i]; e < row_offs[i + 1]; e++) {
                uint32_t id = id_of[(size_t)e];
                if ((id < 2 ? (int)id : 2) != cls) continue;
                dst[k * stride] = {cols[e], id};
                k++;
            }
    };

    // bins
    std::vector<uint32_t> shorts;
    for (size_t i = 0; i < n_rows; i++) {
        uint64_t len = row_offs[i + 1] - row_offs[i];
        if (len <= T) shorts.push_back((uint32_t)i);
        else out.l_row.push_back((uint32_t)i);
    }
    std::stable_sort(shorts.begin(), shorts.end(),
                     [&](uint32_t a, uint32_t b) {
                         return row_offs[a + 1] - row_offs[a] >
                                row_offs[b + 1] - row_offs[b];
                     });
    out.n_short = (uint32_t)shorts.size();
    const size_t n_slices = (shorts.size() + R1CS_SLICE - 1) / R1CS_SLICE;
    out.s_perm.assign(n_slices * R1CS_SLICE, R1CS_NO_ROW);
    out.s_len.assign(n_slices * R1CS_SLICE, 0);
    out.s_off.assign(n_slices + 1, 0);
    for (size_t s = 0; s < n_slices; s++) {
        // longest row of the slice is its first (sorted by length)
        uint32_t r0 = shorts[s * R1CS_SLICE];
        uint64_t width = row_offs[r0 + 1] - row_offs[r0];
        out.s_off[s + 1] = out.s_off[s] + width * R1CS_SLICE;
    }
    out.s_ent.assign((size_t)out.s_off[n_slices], r1cs_entry{0, 0});
    for (size_t j = 0; j < shorts.size(); j++) {
        uint32_t i = shorts[j];
        out.s_perm[j] = i;
        out.s_len[j] = (uint32_t)(row_offs[i + 1] - row_offs[i]);
        size_t s = j / R1CS_SLICE, lane = j % R1CS_SLICE;
        if (out.s_len[j])
            emit_row(i, &out.s_ent[(size_t)out.s_off[s] + lane], R1CS_SLICE);
    }

    // long rows: contiguous entries, fixed-size chunks
    out.l_chunk_off.assign(out.l_row.size() + 1, 0);
    size_t total_long = 0;
    for (uint32_t i : out.l_row) total_long += (size_t)(row_offs[i + 1] - row_offs[i]);
    out.l_ent.resize(total_long);
    size_t pos = 0;
    for (size_t j = 0; j < out.l_row.size(); j++) {
        uint32_t i = out.l_row[j];
        size_t len = (size_t)(row_offs[i + 1] - row_offs[i]);
        emit_row(i, &out.l_ent[pos], 1);
        for (size_t c = 0; c < len; c += chunk)
            out.l_chunk.push_back({(uint32_t)(pos + c),
                                   (uint32_t)std::min<size_t>(chunk, len - c)});
        out.l_chunk_off[j + 1] = (uint32_t)out.l_chunk.size();
        pos += len;
    }
    return 0;
}

// The (row, col, coeff) terms the packed form stands for — what the kernels
// sum: short entries under the length guard, long entries chunk by chunk.
static inline void r1cs_unpack(const r1cs_packed &p,
                               std::vector<r1cs_triple> &out) {
    out.clear();
    for (size_t s = 0; s < p.n_slices(); s++) {
        uint64_t width = (p.s_off[s + 1] - p.s_off[s]) / R1CS_SLICE;
        for (uint32_t lane = 0; lane < R1CS_SLICE; lane++) {
            size_t j = s * R1CS_SLICE + lane;
            if (p.s_perm[j] == R1CS_NO_ROW) continue;
            for (uint64_t k = 0; k < width && k < p.s_len[j]; k++) {
                const r1cs_entry &e =
                    p.s_ent[(size_t)(p.s_off[s] + k * R1CS_SLICE + lane)];
                out.push_back({p.s_perm[j], e.col, p.dict[e.id]});
            }
        }
    }
    for (size_t j = 0; j < p.l_row.size(); j++)
        for (uint32_t c = p.l_chunk_off[j]; c < p.l_chunk_off[j + 1]; c++)
            for (uint32_t k = 0; k < p.l_chunk[c].len; k++) {
                const r1cs_entry &e = p.l_ent[p.l_chunk[c].off + k];
                out.push_back({p.l_row[j], e.col, p.dict[e.id]});
            }
}

}  // namespace em_r1cs
