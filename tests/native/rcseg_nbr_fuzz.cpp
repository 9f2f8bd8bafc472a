// rcseg_nbr_fuzz.cpp — sanitizer harness for the version-3 (causal-neighbour) container entries
// (tic_rcseg_*_nbr in range_coder.cpp), built by `make asan-rcseg-nbr` with
// -fsanitize=address,undefined and run by tests/test_entropy_nbr_asan.py on the CPU.  A container
// is input a user hands in.
//
// Every buffer is a heap block of exactly the size passed, so a read or write one byte outside
// is a report (the neighbour reads sym[k - C] and sym[k - ew*C] are the new ones).  Cases: round
// trips over random geometries, K0, neighbours, alphabets, counts and segment lengths, the first
// segments compared with the file coder fed one symbol per call under the row the definition in
// tic.h gives (computed here without counters); random bytes, truncated, bit-flipped and
// length-inconsistent containers through parse and decode (rejected, or decoded to in-range
// symbols); containers with valid framing and random payloads; every error path.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
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
struct Model {  // exact-size int64 block of K0 * M rows, and what else a container carries
  std::unique_ptr<int64_t[]> p;
  size_t K0 = 0, M = 0, ncum = 0;
  uint32_t nbrs = 0, eh = 0, ew = 0, C = 0;
  Model(size_t K0_, uint32_t nbrs_, size_t ncum_, uint32_t eh_, uint32_t ew_, uint32_t C_)
      : p(new int64_t[K0_ * (nbrs_ == 1 ? 3 : 9) * ncum_]), K0(K0_), M(nbrs_ == 1 ? 3 : 9), ncum(ncum_), nbrs(nbrs_),
        eh(eh_), ew(ew_), C(C_) {}
  size_t rows() const { return K0 * M; }
  int64_t* row(size_t k) { return p.get() + k * ncum; }
};

static void fill_tables(std::mt19937_64& g, Model& m, bool mixed) {
  const int nsym = (int)m.ncum - 1;
  const int64_t totals[3] = {4096, 5000, 1 << 24};
  for (size_t k = 0; k < m.rows(); ++k) {
    const int64_t total = mixed ? totals[g() % 3] : 70000;
    const int64_t top = std::max<int64_t>(1, std::min<int64_t>(2000, total / nsym - 1));
    int64_t* cum = m.row(k);
    cum[0] = 0;
    for (int i = 0; i < nsym; ++i)
      cum[i + 1] = cum[i] + 1 + (int64_t)(g() % (uint64_t)(g() % 3 == 0 ? top : std::min<int64_t>(top, 20)));
    if (mixed && cum[nsym] < total) cum[nsym] = total;
  }
}

// the row of symbol k from the text of the definition
static size_t def_row(const Model& m, const std::vector<uint8_t>& sym, size_t k, uint32_t L) {
  const size_t nsym = m.ncum - 1, rowC = (size_t)m.ew * m.C, p = k % ((size_t)m.eh * rowC);
  const size_t h = p / rowC, w = (p / m.C) % m.ew, seg0 = (size_t)L * (k / L);
  auto t = [&](bool valid, size_t j) -> size_t { return valid ? 1 + (2 * (size_t)sym[j] >= nsym ? 1 : 0) : 0; };
  size_t nb = t(w >= 1 && k >= m.C && k - m.C >= seg0, k - m.C);
  if (m.nbrs == 2) nb += 3 * t(h >= 1 && k >= rowC && k - rowC >= seg0, k - rowC);
  return (k % m.K0) * m.M + nb;
}

static int encode(const Model& m, const uint8_t* sym, size_t n, uint32_t L, uint8_t* out, size_t cap, size_t* w) {
  return tic_rcseg_encode_nbr(sym, n, L, m.p.get(), m.K0, m.nbrs, m.ncum, m.eh, m.ew, m.C, out, cap, w);
}
static int decode(const Model& m, const uint8_t* buf, size_t nbytes, uint8_t* out, size_t n) {
  return tic_rcseg_decode_nbr(buf, nbytes, m.p.get(), m.K0, m.nbrs, m.ncum, m.eh, m.ew, m.C, out, n);
}

static std::vector<uint8_t> encode_ok(const std::vector<uint8_t>& sym, uint32_t L, const Model& m) {
  size_t cap = 0, v1 = 0, w = 0;
  CHECK(tic_rcseg_bound_nbr(sym.size(), L, &cap) == TIC_OK);
  CHECK(tic_rcseg_bound(sym.size(), L, &v1) == TIC_OK && cap == v1 + 16);
  Block out(cap);
  Block in(sym.data(), sym.size());
  CHECK(encode(m, in.p.get(), in.n, L, out.p.get(), cap, &w) == TIC_OK);
  CHECK(w <= cap && w >= 36);
  return std::vector<uint8_t>(out.p.get(), out.p.get() + w);
}

// parse + decode of arbitrary bytes: either rejected, or n in-range symbols
static void try_decode(const std::vector<uint8_t>& bytes, const Model& m, size_t n_hint) {
  Block b(bytes.data(), bytes.size());
  uint32_t L = 0, K0 = 0, crc = 0, eh = 0, ew = 0, C = 0, nb = 0;
  uint64_t n = 0;
  const int rc = tic_rcseg_parse_nbr(b.p.get(), b.n, &L, &n, &K0, &crc, &eh, &ew, &C, &nb);
  CHECK(rc == TIC_OK || rc == TIC_EINVAL);
  if (rc != TIC_OK) {
    CHECK(strlen(tic_rc_last_error()) > 0);
    Block o(n_hint);
    CHECK(decode(m, b.p.get(), b.n, o.p.get(), n_hint) == TIC_EINVAL);
    return;
  }
  CHECK(n > 0 && K0 >= 1 && (nb == 1 || nb == 2) && eh >= 1 && ew >= 1 && C >= 1 && b.p[35] == 0);
  if (n > (1u << 22)) return;  // segments of length zero: many symbols from few bytes
  Block o((size_t)n);
  const int drc = decode(m, b.p.get(), b.n, o.p.get(), (size_t)n);
  CHECK(drc == TIC_OK || drc == TIC_EINVAL);  // EINVAL: the flip hit K0, the CRC, the geometry or neighbours
  if (drc == TIC_OK)
    for (size_t i = 0; i < n; ++i) CHECK(o.p[i] < m.ncum - 1);
  Block o2((size_t)n + 1);
  CHECK(decode(m, b.p.get(), b.n, o2.p.get(), (size_t)n + 1) == TIC_EINVAL);
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : "/tmp";
  std::mt19937_64 g(20261021);
  const uint32_t Ls[] = {4, 8, 16, 64, 2048, 4096, 16384};
  const uint32_t geos[][3] = {{2, 3, 4}, {2, 2, 3}, {1, 1, 1}, {1, 5, 2}, {4, 4, 64}, {8, 8, 80}, {16, 16, 64},
                              {2, 300, 64}, {3, 1, 7}, {65535, 65535, 65535}};

  // --- round trips, the first segments against the file coder, one symbol per call ---
  for (int it = 0; it < 60; ++it) {
    const int nsym = 1 + (int)(g() % (it % 5 == 0 ? 256 : 6));
    const uint32_t* ge = geos[g() % 10];
    const size_t patch = (size_t)ge[0] * ge[1] * ge[2];
    const uint32_t nbrs = 1 + (uint32_t)(g() % 2);
    const size_t k0s[] = {1, ge[2], 3, patch <= 1024 ? patch : 7};
    const size_t K0 = std::min<size_t>(k0s[g() % 4], 262144 / (9 * ((size_t)nsym + 1)));
    Model m(K0, nbrs, (size_t)nsym + 1, ge[0], ge[1], ge[2]);
    fill_tables(g, m, it % 3 == 0 && nsym <= 64);
    const uint32_t L = Ls[g() % 7];
    const size_t n = 1 + g() % (it % 4 == 0 ? 40000 : 300);
    std::vector<uint8_t> sym(n);
    for (auto& s : sym) s = (uint8_t)(g() % 11 == 0 ? g() % nsym : 0 + (g() % 2) * (nsym - 1));
    const std::vector<uint8_t> c = encode_ok(sym, L, m);
    uint32_t pl = 0, pk = 0, pc = 0, peh = 0, pew = 0, pC = 0, pnb = 0;
    uint64_t pn = 0;
    CHECK(tic_rcseg_parse_nbr(c.data(), c.size(), &pl, &pn, &pk, &pc, &peh, &pew, &pC, &pnb) == TIC_OK);
    CHECK(pl == L && pn == n && pk == K0 && peh == ge[0] && pew == ge[1] && pC == ge[2] && pnb == nbrs);
    CHECK(tic_rcseg_parse_nbr(c.data(), c.size(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == TIC_OK);
    CHECK(pc == tic_crc32c(m.p.get(), m.rows() * m.ncum * sizeof(int64_t), 0));  // this harness runs little-endian
    CHECK(tic_rcseg_parse(c.data(), c.size(), &pl, &pn) == TIC_EINVAL);           // version 3 is not version 1
    CHECK(tic_rcseg_parse_ctx(c.data(), c.size(), &pl, &pn, &pk, &pc) == TIC_EINVAL);  // nor version 2
    Block back(n);
    CHECK(decode(m, c.data(), c.size(), back.p.get(), n) == TIC_OK);
    CHECK(memcmp(back.p.get(), sym.data(), n) == 0);
    // segment payloads are the file coder's bytes under the definition's rows
    const size_t S = (n + L - 1) / L;
    size_t at = 36 + 2 * S;
    for (size_t j = 0; j < S && j < 4; ++j) {
      const size_t len = c[36 + 2 * j] | (size_t)c[36 + 2 * j + 1] << 8;
      const size_t b = j * L, e = std::min(n, b + L);
      const std::string path = std::string(dir) + "/rcseg_nbr_seg.bin";
      tic_rc_encoder* enc = nullptr;
      CHECK(tic_rc_encoder_open(path.c_str(), &enc) == TIC_OK);
      for (size_t i = b; i < e; ++i) {
        const int64_t one = sym[i];
        CHECK(tic_rc_encode(enc, &one, 1, m.row(def_row(m, sym, i, L)), m.ncum) == TIC_OK);
      }
      CHECK(tic_rc_encoder_close(enc) == TIC_OK);
      tic_rc_encoder_free(enc);
      std::vector<uint8_t> fb;
      FILE* f = fopen(path.c_str(), "rb");
      int ch;
      while ((ch = fgetc(f)) != EOF) fb.push_back((uint8_t)ch);
      fclose(f);
      CHECK(fb.size() == len && (len == 0 || memcmp(fb.data(), c.data() + at, len) == 0));
      at += len;
    }

    // --- decode under something else: K0, geometry, neighbours, one table entry ---
    {
      Model o(K0, nbrs, m.ncum, m.eh, m.ew, m.C);
      memcpy(o.p.get(), m.p.get(), m.rows() * m.ncum * sizeof(int64_t));
      if (K0 > 1) {
        o.K0 = K0 - 1;
        CHECK(decode(o, c.data(), c.size(), back.p.get(), n) == TIC_EINVAL);
        o.K0 = K0;
      }
      o.ew = m.ew == 65535 ? 1 : m.ew + 1;
      CHECK(decode(o, c.data(), c.size(), back.p.get(), n) == TIC_EINVAL &&
            strstr(tic_rc_last_error(), "geometry") != nullptr);
      o.ew = m.ew;
      if (nbrs == 2) {  // the first K0 * 3 rows as neighbours = 1 tables
        o.nbrs = 1, o.M = 3;
        CHECK(decode(o, c.data(), c.size(), back.p.get(), n) == TIC_EINVAL &&
              strstr(tic_rc_last_error(), "neighbours") != nullptr);
        o.nbrs = 2, o.M = 9;
      }
      int64_t& total = o.row(g() % o.rows())[nsym];
      if (total < (1 << 24)) {  // one larger: still a valid table, but not the one the stream was coded under
        total += 1;
        CHECK(decode(o, c.data(), c.size(), back.p.get(), n) == TIC_EINVAL &&
              strstr(tic_rc_last_error(), "CRC") != nullptr);
      }
    }

    // --- truncated, bit-flipped, extended ---
    for (int k = 0; k < 12; ++k) {
      std::vector<uint8_t> tr(c.begin(), c.begin() + g() % (c.size() + 1));
      try_decode(tr, m, n);
      std::vector<uint8_t> fl = c;
      const size_t where = k < 6 ? g() % std::min<size_t>(fl.size(), 36 + 2 * S) : g() % fl.size();
      fl[where] ^= (uint8_t)(1u << (g() % 8));
      try_decode(fl, m, n);
    }
    std::vector<uint8_t> ext = c;
    ext.push_back(0);
    try_decode(ext, m, n);

    // --- inconsistent lengths: move a byte from one segment's length to another's, overflow one ---
    if (S >= 2) {
      std::vector<uint8_t> mv = c;
      const size_t a = g() % S, b2 = (a + 1 + g() % (S - 1)) % S;
      auto rd = [&](size_t j) { return (uint32_t)(mv[36 + 2 * j] | mv[36 + 2 * j + 1] << 8); };
      auto wr = [&](size_t j, uint32_t v) {
        mv[36 + 2 * j] = (uint8_t)v;
        mv[36 + 2 * j + 1] = (uint8_t)(v >> 8);
      };
      if (rd(a) > 0) {
        wr(a, rd(a) - 1);
        wr(b2, rd(b2) + 1);
        try_decode(mv, m, n);  // still sums right: valid framing or a length above its limit
      }
      wr(a, 0xFFFF);
      try_decode(mv, m, n);
    }

    // --- valid framing, random payload: decodes, in range ---
    std::vector<uint8_t> rp = c;
    for (size_t i = 36 + 2 * S; i < rp.size(); ++i) rp[i] = (uint8_t)g();
    try_decode(rp, m, n);
  }

  // --- random bytes behind a plausible header, and pure noise ---
  Model m2(2, 1, 3, 2, 3, 4);
  {
    std::mt19937_64 g2(7);
    fill_tables(g2, m2, true);
  }
  for (int it = 0; it < 400; ++it) {
    std::vector<uint8_t> b(g() % 200);
    for (auto& v : b) v = (uint8_t)g();
    if (it % 2 == 0 && b.size() >= 36) {
      memcpy(b.data(), "TICS\x03\0\0\0", 8);
      const uint32_t L = it % 4 == 0 ? 4 * (1 + (uint32_t)(g() % 8)) : (uint32_t)g();
      memcpy(b.data() + 8, &L, 4);
      const uint64_t n = it % 8 < 6 ? g() % 100 : g();
      memcpy(b.data() + 12, &n, 8);
      const uint32_t K0 = it % 6 < 4 ? 2 : (uint32_t)g();
      memcpy(b.data() + 20, &K0, 4);
      if (it % 3 == 0) {
        const uint32_t crc = tic_crc32c(m2.p.get(), 6 * 3 * sizeof(int64_t), 0);
        memcpy(b.data() + 24, &crc, 4);
      }
      if (it % 10 < 8) {
        const uint8_t geo[8] = {2, 0, 3, 0, 4, 0, (uint8_t)(it % 14 == 0 ? g() % 4 : 1), (uint8_t)(it % 22 == 0)};
        memcpy(b.data() + 28, geo, 8);
      }
    }
    try_decode(b, m2, 10);
  }
  try_decode({}, m2, 1);

  // --- error paths ---
  {
    size_t cap = 0, w = 0;
    uint32_t L = 0, K0 = 0, crc = 0, eh = 0, ew = 0, C = 0, nb = 0;
    uint64_t n = 0;
    uint8_t sym[8] = {0, 1, 0, 1, 1, 0, 0, 2};
    uint8_t out[160];
    int64_t tab[18];  // K0 = 2, neighbours = 1
    for (int k = 0; k < 6; ++k) tab[3 * k] = 0, tab[3 * k + 1] = 3 + k, tab[3 * k + 2] = k % 2 ? 4096 : 9;
    auto enc = [&](const uint8_t* s, size_t n_, uint32_t L_, const int64_t* t, size_t K0_, uint32_t nb_, size_t ncum,
                   uint32_t eh_, uint32_t ew_, uint32_t C_, uint8_t* o, size_t cap_, size_t* w_) {
      return tic_rcseg_encode_nbr(s, n_, L_, t, K0_, nb_, ncum, eh_, ew_, C_, o, cap_, w_);
    };
    CHECK(tic_rcseg_bound_nbr(8, 4, nullptr) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_nbr(0, 4, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_nbr(8, 0, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_nbr(8, 6, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_nbr(8, 16388, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_nbr(SIZE_MAX, 4, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_nbr(8, 4, &cap) == TIC_OK && cap == 36 + 4 + 24 + 8);
    CHECK(enc(nullptr, 7, 4, tab, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 2, 3, 4, nullptr, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 2, 3, 4, out, sizeof(out), nullptr) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, nullptr, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 0, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 0, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 3, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "neighbours") != nullptr);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 0, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 2, 0, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 2, 3, 0, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 65536, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "geometry") != nullptr);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 1, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 258, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 30000, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);  // K * ncum
    CHECK(strstr(tic_rc_last_error(), "262144") != nullptr);
    CHECK(enc(sym, 7, 4, tab, 50000, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "context count") != nullptr);
    CHECK(enc(sym, 0, 4, tab, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 5, tab, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 8, 4, tab, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);  // symbol 2
    CHECK(strstr(tic_rc_last_error(), "outside the table") != nullptr);
    size_t need = 0;
    CHECK(tic_rcseg_bound_nbr(7, 4, &need) == TIC_OK);
    {
      Block o(need - 1);
      CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 2, 3, 4, o.p.get(), need - 1, &w) == TIC_EINVAL);
    }
    // a bad row anywhere in the set, reachable or not (row 5: context 1, neighbours 2)
    int64_t zero_freq[18], big[18], wide[18], down[18], off[18];
    for (int64_t* t : {zero_freq, big, wide, down, off}) memcpy(t, tab, sizeof(tab));
    zero_freq[16] = 4096;
    big[17] = (int64_t)1 << 32;
    wide[2] = (1 << 24) + 1;
    down[16] = 5, down[17] = 4;
    off[15] = 1;
    CHECK(enc(sym, 7, 4, zero_freq, 2, 1, 3, 1, 1, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "context 1, neighbours 2") != nullptr);
    CHECK(enc(sym, 7, 4, big, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EOVERFLOW);
    CHECK(enc(sym, 7, 4, wide, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "context 0, neighbours 0") != nullptr);
    CHECK(enc(sym, 7, 4, down, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, off, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(enc(sym, 7, 4, tab, 2, 1, 3, 2, 3, 4, out, sizeof(out), &w) == TIC_OK && w > 40);
    CHECK(tic_rcseg_parse_nbr(nullptr, w, &L, &n, &K0, &crc, &eh, &ew, &C, &nb) == TIC_EINVAL);
    CHECK(tic_rcseg_parse_nbr(out, w, &L, &n, &K0, &crc, &eh, &ew, &C, &nb) == TIC_OK);
    CHECK(L == 4 && n == 7 && K0 == 2 && eh == 2 && ew == 3 && C == 4 && nb == 1);
    CHECK(crc == tic_crc32c(tab, sizeof(tab), 0));
    for (size_t cut : {(size_t)0, (size_t)19, (size_t)20, (size_t)35, (size_t)36, (size_t)39, w - 1})
      CHECK(tic_rcseg_parse_nbr(out, cut, &L, &n, &K0, &crc, &eh, &ew, &C, &nb) == TIC_EINVAL);
    {  // the reserved byte, neighbours, a zero geometry field, K0
      const struct { size_t at; uint8_t v; const char* why; } bad[] = {
          {35, 1, "reserved byte"}, {34, 0, "neighbours"}, {34, 3, "neighbours"}, {5, 1, "reserved bytes"}};
      for (const auto& b : bad) {
        Block cp(out, w);
        cp.p[b.at] = b.v;
        CHECK(tic_rcseg_parse_nbr(cp.p.get(), w, &L, &n, &K0, &crc, &eh, &ew, &C, &nb) == TIC_EINVAL);
        CHECK(strstr(tic_rc_last_error(), b.why) != nullptr);
      }
      for (size_t at : {(size_t)28, (size_t)30, (size_t)32, (size_t)20}) {
        Block cp(out, w);
        memset(cp.p.get() + at, 0, at == 20 ? 4 : 2);
        CHECK(tic_rcseg_parse_nbr(cp.p.get(), w, &L, &n, &K0, &crc, &eh, &ew, &C, &nb) == TIC_EINVAL);
      }
    }
    {  // version-1 and version-2 containers
      uint8_t v[64];
      size_t wv = 0;
      CHECK(tic_rcseg_encode(sym, 7, 4, tab, 3, v, sizeof(v), &wv) == TIC_OK);
      CHECK(tic_rcseg_parse_nbr(v, wv, &L, &n, &K0, &crc, &eh, &ew, &C, &nb) == TIC_EINVAL);
      CHECK(strstr(tic_rc_last_error(), "version 1") != nullptr);
      CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 2, 3, v, sizeof(v), &wv) == TIC_OK);
      CHECK(tic_rcseg_parse_nbr(v, wv, &L, &n, &K0, &crc, &eh, &ew, &C, &nb) == TIC_EINVAL);
      CHECK(strstr(tic_rc_last_error(), "version 2") != nullptr);
    }
    uint8_t back[8];
    auto dec = [&](const int64_t* t, size_t K0_, uint32_t nb_, uint32_t eh_, uint32_t ew_, uint32_t C_, uint8_t* o,
                   size_t n_) { return tic_rcseg_decode_nbr(out, w, t, K0_, nb_, 3, eh_, ew_, C_, o, n_); };
    CHECK(dec(tab, 2, 1, 2, 3, 4, nullptr, 7) == TIC_EINVAL);
    CHECK(dec(tab, 2, 1, 2, 3, 4, back, 6) == TIC_EINVAL);
    CHECK(dec(tab, 2, 1, 2, 3, 4, back, 8) == TIC_EINVAL);
    CHECK(dec(nullptr, 2, 1, 2, 3, 4, back, 7) == TIC_EINVAL);
    CHECK(dec(tab, 1, 1, 2, 3, 4, back, 7) == TIC_EINVAL);
    CHECK(dec(tab, 0, 1, 2, 3, 4, back, 7) == TIC_EINVAL);
    CHECK(dec(tab, 2, 1, 3, 2, 4, back, 7) == TIC_EINVAL);
    CHECK(dec(tab, 2, 1, 2, 3, 5, back, 7) == TIC_EINVAL);
    CHECK(dec(tab, 2, 0, 2, 3, 4, back, 7) == TIC_EINVAL);
    CHECK(dec(zero_freq, 2, 1, 2, 3, 4, back, 7) == TIC_EINVAL);
    CHECK(dec(big, 2, 1, 2, 3, 4, back, 7) == TIC_EOVERFLOW);
    CHECK(dec(wide, 2, 1, 2, 3, 4, back, 7) == TIC_EINVAL);
    int64_t other[18];
    memcpy(other, tab, sizeof(tab));
    other[16] += 1;
    CHECK(dec(other, 2, 1, 2, 3, 4, back, 7) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "CRC") != nullptr);
    CHECK(dec(tab, 2, 1, 2, 3, 4, back, 7) == TIC_OK && memcmp(back, sym, 7) == 0);
  }

  if (g_fail) {
    fprintf(stderr, "rcseg_nbr_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  printf("rcseg_nbr_fuzz ok\n");
  return 0;
}
