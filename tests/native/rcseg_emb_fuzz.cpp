// rcseg_emb_fuzz.cpp — sanitizer harness for the embedded-table container ("TICA" version 1:
// tic_rcseg_count_nbr, tic_rcseg_fit_tables, tic_rcseg_*_emb in range_coder.cpp), built by
// `make asan-rcseg-emb` with -fsanitize=address,undefined and run by tests/test_entropy_emb_asan.py
// on the CPU.  A container is input a user hands in.
//
// Every buffer is a heap block of exactly the size passed, so a read or write one byte outside is a
// report.  Cases: round trips and ranges against the slice of the full decode for all neighbours
// values, the table block against the fit of the counts, the extent from the head alone, a copy
// with every payload byte outside the extent overwritten, truncated and bit-flipped containers
// (rejected, or in-range symbols), pure noise, every error path.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "tic.h"

static int g_fail = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)

// exact-size heap copy (std::vector may over-allocate)
struct Block {
  std::unique_ptr<uint8_t[]> p;
  size_t n = 0;
  explicit Block(size_t n_) : p(new uint8_t[n_ ? n_ : 1]), n(n_) {}
  Block(const uint8_t* src, size_t n_) : Block(n_) {
    if (n_) memcpy(p.get(), src, n_);
  }
};

struct Model {
  size_t K0, nsym;
  uint32_t nbrs, eh, ew, C;
  size_t M() const { return nbrs == 0 ? 1 : nbrs == 1 ? 3 : 9; }
  size_t rows() const { return K0 * M(); }
  size_t T() const { return rows() * (nsym - 1) * 2; }
};

static std::vector<uint8_t> pack(const Model& m, const std::vector<uint8_t>& sym, uint32_t L) {
  size_t cap = 0, w = 0;
  CHECK(tic_rcseg_bound_emb(sym.size(), L, m.K0, m.nbrs, m.nsym, &cap) == TIC_OK);
  Block in(sym.data(), sym.size()), out(cap);
  CHECK(tic_rcseg_encode_emb(in.p.get(), in.n, L, m.K0, m.nbrs, m.nsym, m.eh, m.ew, m.C, out.p.get(), cap, &w) == TIC_OK);
  CHECK(w <= cap && w >= 40 + m.T());
  if (cap) {  // one byte less than the bound is refused before anything is written
    Block small(cap - 1);
    size_t w2 = 7;
    CHECK(tic_rcseg_encode_emb(in.p.get(), in.n, L, m.K0, m.nbrs, m.nsym, m.eh, m.ew, m.C, small.p.get(), cap - 1, &w2) ==
          TIC_EINVAL);
    CHECK(w2 == 0);
  }
  return std::vector<uint8_t>(out.p.get(), out.p.get() + w);
}

static void check_container(const Model& m, const std::vector<uint8_t>& c, const std::vector<uint8_t>& sym, uint32_t L,
                            std::mt19937_64& g) {
  const size_t n = sym.size(), S = (n + L - 1) / L, hdr = 40 + m.T();
  Block in(c.data(), c.size());
  uint32_t hL = 0, K0 = 0, eh = 0, ew = 0, C = 0, nb = 9, nsym = 0;
  uint64_t hn = 0;
  Block tab(m.rows() * (m.nsym + 1) * 8);
  int64_t* tables = reinterpret_cast<int64_t*>(tab.p.get());
  CHECK(tic_rcseg_parse_emb(in.p.get(), in.n, &hL, &hn, &K0, &eh, &ew, &C, &nb, &nsym, tables) == TIC_OK);
  CHECK(hL == L && hn == n && K0 == m.K0 && eh == m.eh && ew == m.ew && C == m.C && nb == m.nbrs && nsym == m.nsym);
  CHECK(tic_rcseg_parse_emb(in.p.get(), in.n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr) == TIC_OK);
  // the tables are the fit of the counts
  {
    Block s(sym.data(), n), cnt(m.rows() * m.nsym * 8), fit(m.rows() * (m.nsym + 1) * 8);
    uint64_t* counts = reinterpret_cast<uint64_t*>(cnt.p.get());
    CHECK(tic_rcseg_count_nbr(s.p.get(), n, L, m.K0, m.nbrs, m.nsym, m.eh, m.ew, m.C, counts) == TIC_OK);
    uint64_t total = 0;
    for (size_t k = 0; k < m.rows() * m.nsym; ++k) total += counts[k];
    CHECK(total == n);
    CHECK(tic_rcseg_fit_tables(counts, m.rows(), m.nsym, reinterpret_cast<int64_t*>(fit.p.get())) == TIC_OK);
    CHECK(memcmp(fit.p.get(), tab.p.get(), fit.n) == 0);
    for (size_t r = 0; r < m.rows(); ++r) {
      CHECK(tables[r * (m.nsym + 1)] == 0 && tables[r * (m.nsym + 1) + m.nsym] == 4096);
      for (size_t s2 = 0; s2 < m.nsym; ++s2) CHECK(tables[r * (m.nsym + 1) + s2 + 1] > tables[r * (m.nsym + 1) + s2]);
    }
  }
  Block full(n);
  CHECK(tic_rcseg_decode_emb(in.p.get(), in.n, full.p.get(), n) == TIC_OK);
  CHECK(memcmp(full.p.get(), sym.data(), n) == 0);
  CHECK(tic_rcseg_decode_emb(in.p.get(), in.n, full.p.get(), n + 1) == TIC_EINVAL);
  for (int rep = 0; rep < 6; ++rep) {
    size_t first = rep == 0 ? 0 : rep == 1 ? n - 1 : (size_t)(g() % n);
    size_t count = rep == 0 ? n : rep == 1 ? 1 : 1 + (size_t)(g() % (n - first));
    Block out(count);
    CHECK(tic_rcseg_decode_range_emb(in.p.get(), in.n, out.p.get(), n, first, count) == TIC_OK);
    CHECK(memcmp(out.p.get(), sym.data() + first, count) == 0);
    // the extent from the head alone; the range from a copy whose other payload bytes are overwritten
    Block head(c.data(), hdr + 2 * S);
    size_t j0 = 0, nj = 0, off = 0, len = 0;
    CHECK(tic_rcseg_range_extent_emb(head.p.get(), head.n, first, count, &j0, &nj, &off, &len) == TIC_OK);
    CHECK(j0 == first / L && nj == (first + count - 1) / L - first / L + 1);
    CHECK(off >= hdr + 2 * S && off + len <= c.size());
    CHECK(tic_rcseg_range_extent_emb(head.p.get(), head.n, first, count, nullptr, nullptr, nullptr, nullptr) == TIC_OK);
    Block shortHead(c.data(), hdr + 2 * S - 1);
    CHECK(tic_rcseg_range_extent_emb(shortHead.p.get(), shortHead.n, first, count, &j0, &nj, &off, &len) == TIC_EINVAL);
    Block other(c.data(), c.size());
    for (size_t k = hdr + 2 * S; k < c.size(); ++k)
      if (k < off || k >= off + len) other.p.get()[k] ^= 0xA7;
    memset(out.p.get(), 0xEE, count);
    CHECK(tic_rcseg_decode_range_emb(other.p.get(), other.n, out.p.get(), n, first, count) == TIC_OK);
    CHECK(memcmp(out.p.get(), sym.data() + first, count) == 0);
  }
  // ranges outside the stream
  Block one(1);
  CHECK(tic_rcseg_decode_range_emb(in.p.get(), in.n, one.p.get(), n, n, 1) == TIC_EINVAL);
  CHECK(tic_rcseg_decode_range_emb(in.p.get(), in.n, one.p.get(), n, 0, 0) == TIC_EINVAL);
  CHECK(tic_rcseg_decode_range_emb(in.p.get(), in.n, one.p.get(), n, n - 1, 2) == TIC_EINVAL);
  CHECK(tic_rcseg_range_extent_emb(in.p.get(), in.n, n, 1, nullptr, nullptr, nullptr, nullptr) == TIC_EINVAL);
  // truncated at every boundary and at random places
  const size_t cuts[] = {0, 3, 4, 39, 40, hdr - 1, hdr, hdr + 2 * S - 1, hdr + 2 * S, c.size() - 1};
  for (size_t cut : cuts) {
    if (cut >= c.size()) continue;
    Block t(c.data(), cut);
    Block out(n);
    CHECK(tic_rcseg_parse_emb(t.p.get(), t.n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_emb(t.p.get(), t.n, out.p.get(), n) == TIC_EINVAL);
  }
  // bit flips anywhere: rejected, or n symbols below nsym
  for (int rep = 0; rep < 60; ++rep) {
    Block t(c.data(), c.size());
    const size_t at = rep < 40 ? (size_t)(g() % std::min<size_t>(c.size(), hdr + 2 * S)) : (size_t)(g() % c.size());
    t.p.get()[at] ^= (uint8_t)(1u << (g() % 8));
    Block out(n);
    memset(out.p.get(), 0xFF, n);
    const int rc = tic_rcseg_decode_emb(t.p.get(), t.n, out.p.get(), n);
    CHECK(rc == TIC_OK || rc == TIC_EINVAL);
    if (rc == TIC_OK)
      for (size_t k = 0; k < n; ++k) CHECK(out.p.get()[k] < m.nsym);
    size_t j0, nj, off, len;
    (void)tic_rcseg_range_extent_emb(t.p.get(), std::min(t.n, hdr + 2 * S), 0, 1, &j0, &nj, &off, &len);
  }
  // the payloads replaced by noise under an intact head: defined symbols
  {
    Block t(c.data(), c.size());
    for (size_t k = hdr + 2 * S; k < c.size(); ++k) t.p.get()[k] = (uint8_t)g();
    Block out(n);
    CHECK(tic_rcseg_decode_emb(t.p.get(), t.n, out.p.get(), n) == TIC_OK);
    for (size_t k = 0; k < n; ++k) CHECK(out.p.get()[k] < m.nsym);
  }
}

static void set_crc(std::vector<uint8_t>& c, size_t T) {
  const uint32_t crc = tic_crc32c(c.data() + 40, T, 0);
  for (int b = 0; b < 4; ++b) c[36 + b] = (uint8_t)(crc >> (8 * b));
}

static void error_paths() {
  const Model m{4, 3, 2, 2, 3, 4};
  std::vector<uint8_t> sym(61);
  for (size_t k = 0; k < sym.size(); ++k) sym[k] = (uint8_t)((k * 7 + k / 5) % 3);
  const std::vector<uint8_t> c = pack(m, sym, 8);
  const size_t T = m.T();
  auto rejected = [&](const std::vector<uint8_t>& v) {
    Block t(v.data(), v.size());
    Block out(sym.size());
    return tic_rcseg_parse_emb(t.p.get(), t.n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr) == TIC_EINVAL &&
           tic_rcseg_decode_emb(t.p.get(), t.n, out.p.get(), sym.size()) == TIC_EINVAL;
  };
  auto with = [&](size_t at, std::initializer_list<uint8_t> bytes, bool fix) {
    std::vector<uint8_t> v = c;
    size_t k = at;
    for (uint8_t b : bytes) v[k++] = b;
    if (fix) set_crc(v, T);
    return v;
  };
  CHECK(rejected(with(0, {'T', 'I', 'C', 'S'}, false)));
  CHECK(rejected(with(4, {2}, false)));
  CHECK(rejected(with(5, {3}, false)));
  CHECK(rejected(with(5, {1}, false)));            // T of another model
  CHECK(rejected(with(6, {1, 0}, false)));         // nsym 1
  CHECK(rejected(with(6, {1, 1}, false)));         // nsym 257
  CHECK(rejected(with(8, {6, 0, 0, 0}, false)));   // L
  CHECK(rejected(with(12, {0, 0, 0, 0, 0, 0, 0, 0}, false)));
  CHECK(rejected(with(20, {0, 0, 0, 0}, false)));  // K0 0
  CHECK(rejected(with(20, {0, 0, 16, 0}, false))); // too many rows
  CHECK(rejected(with(24, {0, 0}, false)));        // eh 0
  CHECK(rejected(with(30, {1}, false)));
  CHECK(rejected(with(31, {1}, false)));
  CHECK(rejected(with(32, {(uint8_t)(T + 2)}, false)));
  CHECK(rejected(with(36, {(uint8_t)(c[36] ^ 1)}, false)));
  CHECK(rejected(with(41, {(uint8_t)(c[41] ^ 1)}, false)));      // a table bit, the CRC differs
  CHECK(rejected(with(40 + 6, {0, 0}, true)));                   // a zero frequency under a matching CRC
  CHECK(rejected(with(40, {0xA0, 0x0F, 0x60, 0x00}, true)));     // 4000 + 96: the row sums to 4096
  CHECK(rejected(with(40, {0xFF, 0x0F, 0xFF, 0x0F}, true)));
  CHECK(rejected(with(40 + T, {29, 0}, false)));                 // a segment of 8 symbols claims 29 bytes
  std::vector<uint8_t> longer = c;
  longer.push_back(0);
  CHECK(rejected(longer));
  // arguments
  size_t b = 1, w = 1;
  uint8_t out[4096];
  uint64_t counts[4 * 9 * 3];
  int64_t tables[4 * 9 * 4];
  CHECK(tic_rcseg_bound_emb(0, 8, 4, 2, 3, &b) == TIC_EINVAL && b == 0);
  CHECK(tic_rcseg_bound_emb(61, 6, 4, 2, 3, &b) == TIC_EINVAL);
  CHECK(tic_rcseg_bound_emb(61, 8, 4, 3, 3, &b) == TIC_EINVAL && b == 0);
  CHECK(tic_rcseg_bound_emb(61, 8, 0, 2, 3, &b) == TIC_EINVAL);
  CHECK(tic_rcseg_bound_emb(61, 8, 4, 2, 1, &b) == TIC_EINVAL);
  CHECK(tic_rcseg_bound_emb(61, 8, 4, 2, 257, &b) == TIC_EINVAL);
  CHECK(tic_rcseg_bound_emb(61, 8, 9710, 2, 2, &b) == TIC_EINVAL);  // 9710 * 9 * 3 > 262144
  CHECK(tic_rcseg_bound_emb(61, 8, 4, 2, 3, nullptr) == TIC_EINVAL);
  CHECK(tic_rcseg_encode_emb(nullptr, 61, 8, 4, 2, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
  CHECK(tic_rcseg_encode_emb(sym.data(), 61, 8, 4, 2, 3, 2, 0, 4, out, sizeof(out), &w) == TIC_EINVAL && w == 0);
  CHECK(tic_rcseg_encode_emb(sym.data(), 61, 8, 4, 2, 3, 2, 3, 65536, out, sizeof(out), &w) == TIC_EINVAL);
  std::vector<uint8_t> badsym = sym;
  badsym[60] = 3;
  CHECK(tic_rcseg_encode_emb(badsym.data(), 61, 8, 4, 2, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL && w == 0);
  CHECK(tic_rcseg_count_nbr(badsym.data(), 61, 8, 4, 2, 3, 2, 3, 4, counts) == TIC_EINVAL);
  CHECK(tic_rcseg_count_nbr(sym.data(), 61, 8, 4, 2, 3, 2, 3, 4, nullptr) == TIC_EINVAL);
  CHECK(tic_rcseg_count_nbr(sym.data(), 61, 7, 4, 2, 3, 2, 3, 4, counts) == TIC_EINVAL);
  CHECK(tic_rcseg_count_nbr(sym.data(), 61, 8, 4, 2, 3, 2, 3, 4, counts) == TIC_OK);
  CHECK(tic_rcseg_fit_tables(counts, 36, 3, tables) == TIC_OK);
  CHECK(tic_rcseg_fit_tables(nullptr, 36, 3, tables) == TIC_EINVAL);
  CHECK(tic_rcseg_fit_tables(counts, 0, 3, tables) == TIC_EINVAL);
  CHECK(tic_rcseg_fit_tables(counts, 36, 1, tables) == TIC_EINVAL);
  counts[5] = (1ull << 40) + 1;
  CHECK(tic_rcseg_fit_tables(counts, 36, 3, tables) == TIC_EINVAL);
  counts[5] = 1ull << 40;  // the largest count the format promises
  CHECK(tic_rcseg_fit_tables(counts, 36, 3, tables) == TIC_OK);
  CHECK(tic_rcseg_parse_emb(nullptr, 100, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr) == TIC_EINVAL);
  CHECK(tic_rcseg_decode_emb(c.data(), c.size(), nullptr, 61) == TIC_EINVAL);
  CHECK(tic_rcseg_range_extent_emb(nullptr, 100, 0, 1, nullptr, nullptr, nullptr, nullptr) == TIC_EINVAL);
  // the two magics do not cross
  uint32_t L = 0;
  uint64_t n = 0;
  CHECK(tic_rcseg_parse(c.data(), c.size(), &L, &n) == TIC_EINVAL);
  CHECK(tic_rcseg_range_extent(c.data(), c.size(), 0, 1, nullptr, nullptr, nullptr, nullptr) == TIC_EINVAL);
}

int main() {
  std::mt19937_64 g(20240607);
  const Model models[] = {
      {1, 2, 0, 2, 3, 4},  {4, 2, 0, 2, 3, 4},  {4, 2, 1, 2, 3, 4},  {4, 2, 2, 2, 3, 4},   {3, 2, 2, 2, 2, 3},
      {1, 3, 2, 2, 2, 3},  {64, 2, 1, 4, 4, 64}, {64, 2, 2, 4, 4, 64}, {4, 256, 2, 4, 4, 4}, {7, 5, 1, 3, 2, 5},
  };
  const uint32_t Ls[] = {4, 8, 16, 2048};
  for (const Model& m : models)
    for (uint32_t L : Ls) {
      const size_t patch = (size_t)m.eh * m.ew * m.C;
      const size_t lens[] = {1, L - 1, L, L + 1, 3 * (size_t)L + 2, 2 * patch + 7};
      for (size_t n : lens) {
        if (n > 9000) continue;
        std::vector<uint8_t> sym(n);
        uint8_t cur = 0;
        for (size_t k = 0; k < n; ++k) {
          if (g() % 5 == 0) cur = (uint8_t)(g() % m.nsym);
          sym[k] = cur;
        }
        const std::vector<uint8_t> c = pack(m, sym, L);
        check_container(m, c, sym, L, g);
      }
    }
  error_paths();
  // pure noise, and noise behind the magic
  for (int rep = 0; rep < 400; ++rep) {
    const size_t n = (size_t)(g() % 300);
    Block t(n);
    for (size_t k = 0; k < n; ++k) t.p.get()[k] = (uint8_t)g();
    if (rep % 2 && n >= 6) {
      memcpy(t.p.get(), "TICA", 4);
      t.p.get()[4] = 1;
      t.p.get()[5] = (uint8_t)(g() % 3);
    }
    Block out(64);
    CHECK(tic_rcseg_decode_emb(t.p.get(), t.n, out.p.get(), 64) == TIC_EINVAL);
    CHECK(tic_rcseg_range_extent_emb(t.p.get(), t.n, 0, 1, nullptr, nullptr, nullptr, nullptr) == TIC_EINVAL);
  }
  if (g_fail) {
    fprintf(stderr, "rcseg_emb_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  printf("rcseg_emb_fuzz ok\n");
  return 0;
}
