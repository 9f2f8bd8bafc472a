// rcseg_range_fuzz.cpp — sanitizer harness for the symbol-range entries of the segmented container
// (tic_rcseg_range_extent, tic_rcseg_decode_range / _ctx / _nbr in range_coder.cpp), built by
// `make asan-rcseg-range` with -fsanitize=address,undefined and run by
// tests/test_entropy_range_asan.py on the CPU.  A container is input a user hands in.
//
// Every buffer is a heap block of exactly the size passed, so a read or write one byte outside is
// a report: the output of a range holds `count` bytes, and tic_rcseg_range_extent gets the header
// and the length table only.  Cases, for all three versions: ranges against the slice of the full
// decode (one symbol, inside a segment, up to a border, across segments, everything); the extent
// against the length table; a copy with every payload byte outside the extent overwritten;
// truncated and bit-flipped containers (rejected, or in-range symbols); every error path.
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

// One model of any version: ver 1 uses row 0 of the tables, ver 2 K = K0 rows, ver 3 K0 * M rows.
struct Model {
  int ver = 1;
  std::unique_ptr<int64_t[]> p;
  size_t K0 = 1, M = 1, ncum = 0;
  uint32_t nbrs = 1, eh = 1, ew = 1, C = 1;
  size_t rows() const { return ver == 1 ? 1 : ver == 2 ? K0 : K0 * M; }
  size_t header() const { return ver == 1 ? 20 : ver == 2 ? 28 : 36; }
};

static void fill_tables(std::mt19937_64& g, Model& m) {
  const int nsym = (int)m.ncum - 1;
  m.p.reset(new int64_t[m.rows() * m.ncum]);
  for (size_t k = 0; k < m.rows(); ++k) {
    int64_t* cum = m.p.get() + k * m.ncum;
    cum[0] = 0;
    for (int i = 0; i < nsym; ++i) cum[i + 1] = cum[i] + 1 + (int64_t)(g() % 40);
    if (g() % 2) cum[nsym] = 4096;  // a power-of-two total
  }
}

static int encode(const Model& m, const uint8_t* sym, size_t n, uint32_t L, uint8_t* out, size_t cap, size_t* w) {
  if (m.ver == 1) return tic_rcseg_encode(sym, n, L, m.p.get(), m.ncum, out, cap, w);
  if (m.ver == 2) return tic_rcseg_encode_ctx(sym, n, L, m.p.get(), m.K0, m.ncum, out, cap, w);
  return tic_rcseg_encode_nbr(sym, n, L, m.p.get(), m.K0, m.nbrs, m.ncum, m.eh, m.ew, m.C, out, cap, w);
}
static int decode(const Model& m, const uint8_t* buf, size_t nbytes, uint8_t* out, size_t n) {
  if (m.ver == 1) return tic_rcseg_decode(buf, nbytes, m.p.get(), m.ncum, out, n);
  if (m.ver == 2) return tic_rcseg_decode_ctx(buf, nbytes, m.p.get(), m.K0, m.ncum, out, n);
  return tic_rcseg_decode_nbr(buf, nbytes, m.p.get(), m.K0, m.nbrs, m.ncum, m.eh, m.ew, m.C, out, n);
}
static int decode_range(const Model& m, const uint8_t* buf, size_t nbytes, uint8_t* out, size_t n, size_t first,
                        size_t count) {
  if (m.ver == 1) return tic_rcseg_decode_range(buf, nbytes, m.p.get(), m.ncum, out, n, first, count);
  if (m.ver == 2) return tic_rcseg_decode_range_ctx(buf, nbytes, m.p.get(), m.K0, m.ncum, out, n, first, count);
  return tic_rcseg_decode_range_nbr(buf, nbytes, m.p.get(), m.K0, m.nbrs, m.ncum, m.eh, m.ew, m.C, out, n, first,
                                    count);
}

// a range of container c against the slice of the full decode `sym`, the extent against the
// length table, and the same range from a copy whose other payload bytes are overwritten
static void check_range(const Model& m, const std::vector<uint8_t>& c, const std::vector<uint8_t>& sym, uint32_t L,
                        size_t first, size_t count) {
  const size_t n = sym.size(), S = (n + L - 1) / L, hdr = m.header();
  Block in(c.data(), c.size());
  Block out(count);
  CHECK(decode_range(m, in.p.get(), in.n, out.p.get(), n, first, count) == TIC_OK);
  CHECK(memcmp(out.p.get(), sym.data() + first, count) == 0);

  size_t j0 = 0, nj = 0, off = 0, len = 0;
  Block head(c.data(), hdr + 2 * S);  // the header and the length table, not a byte more
  CHECK(tic_rcseg_range_extent(head.p.get(), head.n, first, count, &j0, &nj, &off, &len) == TIC_OK);
  CHECK(tic_rcseg_range_extent(head.p.get(), head.n, first, count, nullptr, nullptr, nullptr, nullptr) == TIC_OK);
  size_t want_off = hdr + 2 * S, want_len = 0;
  const size_t wj0 = first / L, wj1 = (first + count - 1) / L;
  for (size_t j = 0; j <= wj1; ++j) {
    const size_t l = c[hdr + 2 * j] | (size_t)c[hdr + 2 * j + 1] << 8;
    if (j < wj0) want_off += l;
    else want_len += l;
  }
  CHECK(j0 == wj0 && nj == wj1 - wj0 + 1 && off == want_off && len == want_len && off + len <= c.size());

  Block poisoned(c.data(), c.size());
  for (size_t i = hdr + 2 * S; i < c.size(); ++i)
    if (i < off || i >= off + len) poisoned.p[i] = 0xA5;
  Block out2(count);
  CHECK(decode_range(m, poisoned.p.get(), poisoned.n, out2.p.get(), n, first, count) == TIC_OK);
  CHECK(memcmp(out2.p.get(), sym.data() + first, count) == 0);
}

// arbitrary bytes: rejected, or count in-range symbols
static void try_range(const Model& m, const std::vector<uint8_t>& bytes, size_t n, size_t first, size_t count) {
  Block b(bytes.data(), bytes.size());
  Block o(count);
  const int rc = decode_range(m, b.p.get(), b.n, o.p.get(), n, first, count);
  CHECK(rc == TIC_OK || rc == TIC_EINVAL);
  if (rc == TIC_OK)
    for (size_t i = 0; i < count; ++i) CHECK(o.p[i] < m.ncum - 1);
  size_t j0, nj, off, len;
  const int re = tic_rcseg_range_extent(b.p.get(), b.n, first, count, &j0, &nj, &off, &len);
  CHECK(re == TIC_OK || re == TIC_EINVAL);
  if (rc == TIC_OK) CHECK(re == TIC_OK && off + len <= b.n);
}

int main() {
  std::mt19937_64 g(20261021);
  const uint32_t Ls[] = {4, 8, 16, 64, 2048, 16384};
  const uint32_t geos[][3] = {{2, 3, 4}, {4, 4, 64}, {1, 1, 1}, {1, 5, 2}, {16, 16, 64}, {2, 300, 64}};

  for (int it = 0; it < 90; ++it) {
    Model m;
    m.ver = 1 + it % 3;
    const int nsym = 1 + (int)(g() % (it % 5 == 0 ? 256 : 6));
    m.ncum = (size_t)nsym + 1;
    const uint32_t* ge = geos[g() % 6];
    m.eh = ge[0], m.ew = ge[1], m.C = ge[2];
    m.nbrs = 1 + (uint32_t)(g() % 2);
    m.M = m.nbrs == 1 ? 3 : 9;
    const size_t patch = (size_t)ge[0] * ge[1] * ge[2];
    const size_t k0s[] = {1, ge[2], 3, patch <= 1024 ? patch : 7};
    m.K0 = std::min<size_t>(k0s[g() % 4], 262144 / (9 * m.ncum));
    fill_tables(g, m);
    const uint32_t L = Ls[g() % 6];
    const size_t lens[] = {1, (size_t)L - 1, L, (size_t)L + 1, 3 * (size_t)L + 2, 2 * patch + 7};
    const size_t n = it % 4 == 0 ? 1 + g() % 40000 : std::min<size_t>(lens[g() % 6], 60000);
    std::vector<uint8_t> sym(n);
    for (auto& s : sym) s = (uint8_t)(g() % 5 == 0 ? g() % nsym : (g() % 2) * (nsym - 1));
    size_t cap = 0, w = 0;
    if (m.ver == 1) CHECK(tic_rcseg_bound(n, L, &cap) == TIC_OK);
    if (m.ver == 2) CHECK(tic_rcseg_bound_ctx(n, L, &cap) == TIC_OK);
    if (m.ver == 3) CHECK(tic_rcseg_bound_nbr(n, L, &cap) == TIC_OK);
    Block enc(cap);
    CHECK(encode(m, sym.data(), n, L, enc.p.get(), cap, &w) == TIC_OK);
    const std::vector<uint8_t> c(enc.p.get(), enc.p.get() + w);
    Block full(n);
    CHECK(decode(m, c.data(), c.size(), full.p.get(), n) == TIC_OK);
    CHECK(memcmp(full.p.get(), sym.data(), n) == 0);

    // --- the ranges: one symbol at each end, inside a segment, up to a border, across, everything ---
    check_range(m, c, sym, L, 0, 1);
    check_range(m, c, sym, L, n - 1, 1);
    check_range(m, c, sym, L, 0, n);
    if (n > 2) check_range(m, c, sym, L, 1, std::min<size_t>(n - 1, L - 2));
    if (n >= 2 * (size_t)L) check_range(m, c, sym, L, L / 2, 2 * (size_t)L - L / 2);  // ends on a border
    if (n > 2 * (size_t)L + 1) check_range(m, c, sym, L, L - 1, L + 2);                // three segments
    for (int k = 0; k < 8; ++k) {
      const size_t first = g() % n, count = 1 + g() % (n - first);
      check_range(m, c, sym, L, first, count);
    }

    // --- truncated and bit-flipped containers ---
    const size_t S = (n + L - 1) / L;
    for (int k = 0; k < 8; ++k) {
      const size_t first = g() % n, count = 1 + g() % std::min<size_t>(n - first, 500);
      std::vector<uint8_t> tr(c.begin(), c.begin() + g() % (c.size() + 1));
      try_range(m, tr, n, first, count);
      std::vector<uint8_t> fl = c;
      const size_t where = k < 4 ? g() % std::min<size_t>(fl.size(), m.header() + 2 * S) : g() % fl.size();
      fl[where] ^= (uint8_t)(1u << (g() % 8));
      try_range(m, fl, n, first, count);
    }

    // --- the range's own error paths, each with the container intact ---
    Block o(4);
    CHECK(decode_range(m, c.data(), c.size(), o.p.get(), n, 0, 0) == TIC_EINVAL);
    CHECK(decode_range(m, c.data(), c.size(), o.p.get(), n, n, 1) == TIC_EINVAL);
    CHECK(decode_range(m, c.data(), c.size(), o.p.get(), n, n - 1, 2) == TIC_EINVAL);
    CHECK(decode_range(m, c.data(), c.size(), o.p.get(), n, 1, SIZE_MAX) == TIC_EINVAL);
    CHECK(decode_range(m, c.data(), c.size(), nullptr, n, 0, 1) == TIC_EINVAL);
    CHECK(decode_range(m, c.data(), c.size(), o.p.get(), n + 1, 0, 1) == TIC_EINVAL);
    CHECK(decode_range(m, nullptr, c.size(), o.p.get(), n, 0, 1) == TIC_EINVAL);
    size_t j0, nj, off, len;
    CHECK(tic_rcseg_range_extent(c.data(), c.size(), 0, 0, &j0, &nj, &off, &len) == TIC_EINVAL);
    CHECK(tic_rcseg_range_extent(c.data(), c.size(), n, 1, &j0, &nj, &off, &len) == TIC_EINVAL);
    CHECK(tic_rcseg_range_extent(c.data(), c.size(), 0, n + 1, &j0, &nj, &off, &len) == TIC_EINVAL);
    CHECK(tic_rcseg_range_extent(nullptr, c.size(), 0, 1, &j0, &nj, &off, &len) == TIC_EINVAL);
    {
      Block cut(c.data(), m.header() + 2 * S - 1);  // the length table not wholly present
      CHECK(tic_rcseg_range_extent(cut.p.get(), cut.n, 0, 1, &j0, &nj, &off, &len) == TIC_EINVAL);
      Block hd(c.data(), m.header() - 1);
      CHECK(tic_rcseg_range_extent(hd.p.get(), hd.n, 0, 1, &j0, &nj, &off, &len) == TIC_EINVAL);
      Block bad(c.data(), c.size());
      bad.p[4] = 4;
      CHECK(tic_rcseg_range_extent(bad.p.get(), bad.n, 0, 1, &j0, &nj, &off, &len) == TIC_EINVAL);
      bad.p[4] = c[4], bad.p[0] = 'X';
      CHECK(tic_rcseg_range_extent(bad.p.get(), bad.n, 0, 1, &j0, &nj, &off, &len) == TIC_EINVAL);
    }
    // the wrong version for the entry
    Model other;
    other.ver = 1 + m.ver % 3;
    other.ncum = m.ncum, other.K0 = m.K0, other.M = m.M, other.nbrs = m.nbrs, other.eh = m.eh, other.ew = m.ew,
    other.C = m.C;
    std::mt19937_64 g2(it);
    fill_tables(g2, other);
    CHECK(decode_range(other, c.data(), c.size(), o.p.get(), n, 0, 1) == TIC_EINVAL);
  }

  // --- pure noise ---
  Model m2;
  m2.ver = 1;
  m2.ncum = 3;
  fill_tables(g, m2);
  for (int it = 0; it < 300; ++it) {
    std::vector<uint8_t> b(g() % 120);
    for (auto& v : b) v = (uint8_t)g();
    if (it % 2 == 0 && b.size() >= 20) {
      memcpy(b.data(), "TICS\x01\0\0\0", 8);
      const uint32_t L = 4 * (1 + (uint32_t)(g() % 4));
      memcpy(b.data() + 8, &L, 4);
      const uint64_t n = it % 8 < 6 ? g() % 60 : g();
      memcpy(b.data() + 12, &n, 8);
    }
    try_range(m2, b, 10, g() % 10, 1);
  }

  if (g_fail) {
    fprintf(stderr, "rcseg_range_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  printf("rcseg_range_fuzz ok\n");
  return 0;
}
