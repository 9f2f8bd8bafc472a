// rcseg_ctx_fuzz.cpp — sanitizer harness for the version-2 (context) container entries
// (tic_rcseg_*_ctx in range_coder.cpp), built by `make asan-rcseg-ctx` with
// -fsanitize=address,undefined and run by tests/test_entropy_ctx_asan.py on the CPU.  A container
// is input a user hands in.
//
// Every buffer is a heap block of exactly the size passed, so a read or write one byte outside
// is a report.  Cases: round trips over random table sets (K, ncum, mixed totals), counts and
// segment lengths, each segment compared with the file coder fed one symbol per call; random
// bytes, truncated, bit-flipped and length-inconsistent containers through parse and decode
// (rejected, or decoded to in-range symbols); containers with valid framing and random payloads
// (must decode, in range); every error path.
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
struct Tables {  // exact-size int64 block of K rows
  std::unique_ptr<int64_t[]> p;
  size_t K = 0, ncum = 0;
  Tables(size_t K_, size_t ncum_) : p(new int64_t[K_ * ncum_]), K(K_), ncum(ncum_) {}
  int64_t* row(size_t k) { return p.get() + k * ncum; }
};

static Tables random_tables(std::mt19937_64& g, size_t K, int nsym, bool mixed) {
  Tables t(K, (size_t)nsym + 1);
  const int64_t totals[3] = {4096, 5000, 1 << 24};
  for (size_t k = 0; k < K; ++k) {
    const int64_t total = mixed ? totals[g() % 3] : 70000;
    const int64_t top = std::max<int64_t>(1, std::min<int64_t>(2000, total / nsym - 1));
    int64_t* cum = t.row(k);
    cum[0] = 0;
    for (int i = 0; i < nsym; ++i)
      cum[i + 1] = cum[i] + 1 + (int64_t)(g() % (uint64_t)(g() % 3 == 0 ? top : std::min<int64_t>(top, 20)));
    if (mixed && cum[nsym] < total) cum[nsym] = total;  // the row's total exactly (last frequency grows)
  }
  return t;
}

static std::vector<uint8_t> encode_ok(const std::vector<uint8_t>& sym, uint32_t L, Tables& t) {
  size_t cap = 0, v1 = 0, w = 0;
  CHECK(tic_rcseg_bound_ctx(sym.size(), L, &cap) == TIC_OK);
  CHECK(tic_rcseg_bound(sym.size(), L, &v1) == TIC_OK && cap == v1 + 8);
  Block out(cap);
  Block in(sym.data(), sym.size());
  CHECK(tic_rcseg_encode_ctx(in.p.get(), in.n, L, t.p.get(), t.K, t.ncum, out.p.get(), cap, &w) == TIC_OK);
  CHECK(w <= cap && w >= 28);
  return std::vector<uint8_t>(out.p.get(), out.p.get() + w);
}

// parse + decode of arbitrary bytes: either rejected, or n in-range symbols
static void try_decode(const std::vector<uint8_t>& bytes, Tables& t, size_t n_hint) {
  Block b(bytes.data(), bytes.size());
  uint32_t L = 0, K = 0, crc = 0;
  uint64_t n = 0;
  const int rc = tic_rcseg_parse_ctx(b.p.get(), b.n, &L, &n, &K, &crc);
  CHECK(rc == TIC_OK || rc == TIC_EINVAL);
  if (rc != TIC_OK) {
    CHECK(strlen(tic_rc_last_error()) > 0);
    Block o(n_hint);
    CHECK(tic_rcseg_decode_ctx(b.p.get(), b.n, t.p.get(), t.K, t.ncum, o.p.get(), n_hint) == TIC_EINVAL);
    return;
  }
  CHECK(n > 0 && K >= 1 && K <= 65536);
  if (n > (1u << 22)) return;  // segments of length zero: many symbols from few bytes
  Block o((size_t)n);
  const int drc = tic_rcseg_decode_ctx(b.p.get(), b.n, t.p.get(), t.K, t.ncum, o.p.get(), (size_t)n);
  CHECK(drc == TIC_OK || drc == TIC_EINVAL);  // EINVAL: the flip hit K or the CRC
  if (drc == TIC_OK)
    for (size_t i = 0; i < n; ++i) CHECK(o.p[i] < t.ncum - 1);
  Block o2((size_t)n + 1);
  CHECK(tic_rcseg_decode_ctx(b.p.get(), b.n, t.p.get(), t.K, t.ncum, o2.p.get(), (size_t)n + 1) == TIC_EINVAL);
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : "/tmp";
  std::mt19937_64 g(20261021);
  const uint32_t Ls[] = {4, 8, 64, 1024, 4096, 16384};
  const size_t Ks[] = {1, 2, 3, 5, 64, 80, 1000};

  // --- round trips, each segment against the file coder, one symbol per call ---
  for (int it = 0; it < 60; ++it) {
    const int nsym = 1 + (int)(g() % (it % 5 == 0 ? 256 : 6));
    const size_t K = Ks[g() % 7];
    Tables t = random_tables(g, K, nsym, it % 3 == 0 && nsym <= 64);
    const uint32_t L = Ls[g() % 6];
    const size_t n = 1 + g() % (it % 4 == 0 ? 40000 : 300);
    std::vector<uint8_t> sym(n);
    for (auto& s : sym) s = (uint8_t)(g() % 11 == 0 ? g() % nsym : 0 + (g() % 2) * (nsym - 1));
    const std::vector<uint8_t> c = encode_ok(sym, L, t);
    uint32_t pl = 0, pk = 0, pc = 0;
    uint64_t pn = 0;
    CHECK(tic_rcseg_parse_ctx(c.data(), c.size(), &pl, &pn, &pk, &pc) == TIC_OK && pl == L && pn == n && pk == K);
    CHECK(tic_rcseg_parse_ctx(c.data(), c.size(), nullptr, nullptr, nullptr, nullptr) == TIC_OK);
    CHECK(pc == tic_crc32c(t.p.get(), K * t.ncum * sizeof(int64_t), 0));  // this harness runs little-endian
    CHECK(tic_rcseg_parse(c.data(), c.size(), &pl, &pn) == TIC_EINVAL);   // version 2 is not version 1
    Block back(n);
    CHECK(tic_rcseg_decode_ctx(c.data(), c.size(), t.p.get(), K, t.ncum, back.p.get(), n) == TIC_OK);
    CHECK(memcmp(back.p.get(), sym.data(), n) == 0);
    // segment payloads are the file coder's bytes
    const size_t S = (n + L - 1) / L;
    size_t at = 28 + 2 * S;
    for (size_t j = 0; j < S && j < 4; ++j) {
      const size_t len = c[28 + 2 * j] | (size_t)c[28 + 2 * j + 1] << 8;
      const size_t b = j * L, e = std::min(n, b + L);
      const std::string path = std::string(dir) + "/rcseg_ctx_seg.bin";
      tic_rc_encoder* enc = nullptr;
      CHECK(tic_rc_encoder_open(path.c_str(), &enc) == TIC_OK);
      for (size_t i = b; i < e; ++i) {
        const int64_t one = sym[i];
        CHECK(tic_rc_encode(enc, &one, 1, t.row(i % K), t.ncum) == TIC_OK);
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

    // --- other tables: K, one entry ---
    if (K > 1) {
      CHECK(tic_rcseg_decode_ctx(c.data(), c.size(), t.p.get(), K - 1, t.ncum, back.p.get(), n) == TIC_EINVAL);
    }
    {
      Tables o(K, t.ncum);
      memcpy(o.p.get(), t.p.get(), K * t.ncum * sizeof(int64_t));
      int64_t& total = o.row(g() % K)[nsym];
      if (total < (1 << 24)) {  // one larger: still a valid table, but not the one the stream was coded under
        total += 1;
        CHECK(tic_rcseg_decode_ctx(c.data(), c.size(), o.p.get(), K, t.ncum, back.p.get(), n) == TIC_EINVAL &&
              strstr(tic_rc_last_error(), "CRC") != nullptr);
      }
    }

    // --- truncated, bit-flipped, extended ---
    for (int k = 0; k < 12; ++k) {
      std::vector<uint8_t> tr(c.begin(), c.begin() + g() % (c.size() + 1));
      try_decode(tr, t, n);
      std::vector<uint8_t> fl = c;
      const size_t where = k < 6 ? g() % std::min<size_t>(fl.size(), 28 + 2 * S) : g() % fl.size();
      fl[where] ^= (uint8_t)(1u << (g() % 8));
      try_decode(fl, t, n);
    }
    std::vector<uint8_t> ext = c;
    ext.push_back(0);
    try_decode(ext, t, n);

    // --- inconsistent lengths: move a byte from one segment's length to another's, overflow one ---
    if (S >= 2) {
      std::vector<uint8_t> m = c;
      const size_t a = g() % S, b2 = (a + 1 + g() % (S - 1)) % S;
      auto rd = [&](size_t j) { return (uint32_t)(m[28 + 2 * j] | m[28 + 2 * j + 1] << 8); };
      auto wr = [&](size_t j, uint32_t v) {
        m[28 + 2 * j] = (uint8_t)v;
        m[28 + 2 * j + 1] = (uint8_t)(v >> 8);
      };
      if (rd(a) > 0) {
        wr(a, rd(a) - 1);
        wr(b2, rd(b2) + 1);
        try_decode(m, t, n);  // still sums right: valid framing or a length above its limit
      }
      wr(a, 0xFFFF);
      try_decode(m, t, n);
    }

    // --- valid framing, random payload: decodes, in range ---
    std::vector<uint8_t> rp = c;
    for (size_t i = 28 + 2 * S; i < rp.size(); ++i) rp[i] = (uint8_t)g();
    try_decode(rp, t, n);
  }

  // --- random bytes behind a plausible header, and pure noise ---
  Tables t2(2, 3);
  const int64_t rows2[6] = {0, 2457, 4096, 0, 100, 5000};
  memcpy(t2.p.get(), rows2, sizeof(rows2));
  for (int it = 0; it < 300; ++it) {
    std::vector<uint8_t> b(g() % 200);
    for (auto& v : b) v = (uint8_t)g();
    if (it % 2 == 0 && b.size() >= 28) {
      memcpy(b.data(), "TICS\x02\0\0\0", 8);
      const uint32_t L = it % 4 == 0 ? 4 * (1 + (uint32_t)(g() % 8)) : (uint32_t)g();
      memcpy(b.data() + 8, &L, 4);
      const uint64_t n = it % 8 < 6 ? g() % 100 : g();
      memcpy(b.data() + 12, &n, 8);
      const uint32_t K = it % 6 < 4 ? 2 : (uint32_t)g();
      memcpy(b.data() + 20, &K, 4);
      if (it % 3 == 0) {
        const uint32_t crc = tic_crc32c(rows2, sizeof(rows2), 0);
        memcpy(b.data() + 24, &crc, 4);
      }
    }
    try_decode(b, t2, 10);
  }
  try_decode({}, t2, 1);

  // --- error paths ---
  {
    size_t cap = 0, w = 0;
    uint32_t L = 0, K = 0, crc = 0;
    uint64_t n = 0;
    uint8_t sym[8] = {0, 1, 0, 1, 1, 0, 0, 2};
    uint8_t out[160];
    const int64_t tab[6] = {0, 3, 8, 0, 4000, 4096};
    CHECK(tic_rcseg_bound_ctx(8, 4, nullptr) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_ctx(0, 4, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_ctx(8, 0, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_ctx(8, 6, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_ctx(8, 16388, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_ctx(SIZE_MAX, 4, &cap) == TIC_EINVAL);
    CHECK(tic_rcseg_bound_ctx(8, 4, &cap) == TIC_OK && cap == 28 + 4 + 24 + 8);
    CHECK(tic_rcseg_encode_ctx(nullptr, 7, 4, tab, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 2, 3, nullptr, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 2, 3, out, sizeof(out), nullptr) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, nullptr, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 0, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 65537, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 2, 1, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 2, 258, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 65536, 5, out, sizeof(out), &w) == TIC_EINVAL);  // K * ncum
    CHECK(strstr(tic_rc_last_error(), "262144") != nullptr);
    CHECK(tic_rcseg_encode_ctx(sym, 0, 4, tab, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 5, tab, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 8, 4, tab, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);  // symbol 2
    CHECK(strstr(tic_rc_last_error(), "outside the table") != nullptr);
    size_t need = 0;
    CHECK(tic_rcseg_bound_ctx(7, 4, &need) == TIC_OK);
    {
      Block o(need - 1);
      CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 2, 3, o.p.get(), need - 1, &w) == TIC_EINVAL);
    }
    // a bad row anywhere in the set
    const int64_t zero_freq[6] = {0, 3, 8, 0, 8, 8}, big[6] = {0, 3, 8, 0, 1, (int64_t)1 << 32};
    const int64_t wide[6] = {0, 1, (1 << 24) + 1, 0, 3, 8}, down[6] = {0, 3, 8, 0, 5, 4}, off[6] = {0, 3, 8, 1, 2, 3};
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, zero_freq, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "context 1") != nullptr);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, big, 2, 3, out, sizeof(out), &w) == TIC_EOVERFLOW);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, wide, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "context 0") != nullptr);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, down, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, off, 2, 3, out, sizeof(out), &w) == TIC_EINVAL);
    CHECK(tic_rcseg_encode_ctx(sym, 7, 4, tab, 2, 3, out, sizeof(out), &w) == TIC_OK && w > 32);
    CHECK(tic_rcseg_parse_ctx(nullptr, w, &L, &n, &K, &crc) == TIC_EINVAL);
    CHECK(tic_rcseg_parse_ctx(out, w, &L, &n, &K, &crc) == TIC_OK && L == 4 && n == 7 && K == 2);
    CHECK(crc == tic_crc32c(tab, sizeof(tab), 0));
    CHECK(tic_rcseg_parse_ctx(out, 27, &L, &n, &K, &crc) == TIC_EINVAL);
    {  // a version-1 container
      uint8_t v1[64];
      size_t w1 = 0;
      CHECK(tic_rcseg_encode(sym, 7, 4, tab, 3, v1, sizeof(v1), &w1) == TIC_OK);
      CHECK(tic_rcseg_parse_ctx(v1, w1, &L, &n, &K, &crc) == TIC_EINVAL);
      CHECK(strstr(tic_rc_last_error(), "version 1") != nullptr);
    }
    uint8_t back[8];
    CHECK(tic_rcseg_decode_ctx(out, w, tab, 2, 3, nullptr, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_ctx(out, w, tab, 2, 3, back, 6) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_ctx(out, w, tab, 2, 3, back, 8) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_ctx(out, w, nullptr, 2, 3, back, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_ctx(out, w, tab, 1, 3, back, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_ctx(out, w, tab, 0, 3, back, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_ctx(out, w, zero_freq, 2, 3, back, 7) == TIC_EINVAL);
    CHECK(tic_rcseg_decode_ctx(out, w, big, 2, 3, back, 7) == TIC_EOVERFLOW);
    CHECK(tic_rcseg_decode_ctx(out, w, wide, 2, 3, back, 7) == TIC_EINVAL);
    const int64_t other[6] = {0, 3, 8, 0, 4001, 4096};
    CHECK(tic_rcseg_decode_ctx(out, w, other, 2, 3, back, 7) == TIC_EINVAL);
    CHECK(strstr(tic_rc_last_error(), "CRC") != nullptr);
    CHECK(tic_rcseg_decode_ctx(out, w, tab, 2, 3, back, 7) == TIC_OK && memcmp(back, sym, 7) == 0);
  }

  if (g_fail) {
    fprintf(stderr, "rcseg_ctx_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  printf("rcseg_ctx_fuzz ok\n");
  return 0;
}
