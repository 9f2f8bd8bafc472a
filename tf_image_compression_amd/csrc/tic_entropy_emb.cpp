// tic_entropy_emb.cpp — "TICA" version 1 on the device (include/tic.h): version 3's context model
// under tables fitted to each stream's own symbols and carried in its container.
//
// The encoder is two passes over the symbols, all on the handle's stream:
//
//   emb_histogram_kernel   per-stream counts [stream][K0*M][nsym].  A workgroup counts into LDS
//                          (64-bit counters, when a stream's counts fit 32 KiB) and adds what it
//                          counted to the stream's counts in the scratch once; integer adds only.
//   emb_fit_kernel         one thread per table row: the integer fit rule of include/tic.h, the
//                          row's cumulative table (u32, nsym + 1 words) and its u16 frequencies of
//                          the container's table block, both into the scratch
//   emb_crc_kernel         one wave per stream: CRC-32C of the table block.  Every lane takes a
//                          run of bytes, the 64 values are combined in a tree by multiplying with
//                          x^(8*len) modulo the polynomial; the result is tic_crc32c's.
//   emb_encode_kernel      tic_entropy.cpp's neighbour coder, one segment per lane, reading ITS
//                          STREAM'S tables.  The work items give every stream whole workgroups
//                          (wg_base), so a workgroup stages one stream's tables in LDS when they
//                          fit 64 KiB and reads them from the scratch otherwise.
//   emb_seg_scan_kernel, ent_stream_scan_kernel, emb_gather_kernel
//                          as tic_entropy.cpp's; the gather also writes the 40-byte header and the
//                          table block.
//
// The decoder: emb_dec_header_kernel checks every header against the caller's model, count and
// size, emb_dec_tables_kernel rebuilds the cumulative tables from the table block (one thread per
// row; a zero frequency or a row sum above 4095 marks the container), emb_crc_kernel checks the
// block's CRC, emb_dec_scan_kernel finds the payload offsets and zero-fills what cannot be decoded,
// emb_decode_kernel decodes one segment per lane with version 3's class-bit rings.  RNG = 1 is the
// symbol-range form, as in tic_entropy.cpp.
//
// Every row's total is 4096, so range / total is a shift by 12 everywhere.  The coder arithmetic is
// a further copy of ent_encode_kernel's / ent_decode_kernel's (the measured kernels stay as they
// are): a fix to the carry, flush or renormalisation goes into every copy.
//
// Nothing is kept on the handle: the model comes with every call, and the tables of
// tic_entropy_set_* stay as they are.  This file closes the one translation unit of the host
// runtime: it includes tic_region.cpp, which includes tic_entropy.cpp and so on.
#include "tic_region.cpp"

namespace tic {

constexpr uint32_t kEmbTotal = 4096;
constexpr int kEmbShift = 12;
constexpr uint32_t kEmbHeader = 40;
constexpr uint32_t kEmbPoly = 0x82F63B78u;  // CRC-32C, reflected

struct EmbModel {
  EntNbr q;       // ncum = nsym + 1 words a table row; ring as version 3's (0 when no neighbour counts)
  uint32_t useW;  // neighbours >= 1
  uint32_t nbrs;  // the header's neighbours byte
  uint32_t nsym, rows, words;  // rows = K0 * M, words = rows * ncum
  uint32_t T;     // bytes of a table block
};

// The by-value records of one chunk of streams; wg_base: workgroups (of `lanes` segments) in front
// of each stream.
struct EmbChunk {
  long long in_off[kEntStreams], in_size[kEntStreams], count[kEntStreams], out_off[kEntStreams];
  long long seg_base[kEntStreams + 1], wg_base[kEntStreams + 1];
  int n, first, last;
};

__global__ void __launch_bounds__(64) emb_put_kernel(const EmbChunk t, uint32_t L, EntRec* __restrict__ rec,
                                                     unsigned long long* __restrict__ seg_base,
                                                     unsigned long long* __restrict__ wg_base) {
  const int k = threadIdx.x;
  if (k < t.n) {
    EntRec r;
    r.in_off = t.in_off[k];
    r.in_size = t.in_size[k];
    r.count = t.count[k];
    r.out_off = t.out_off[k];
    r.L = L;
    r.valid = 1;
    rec[t.first + k] = r;
    seg_base[t.first + k] = (unsigned long long)t.seg_base[k];
    wg_base[t.first + k] = (unsigned long long)t.wg_base[k];
  }
  if (k == 0 && t.last) {
    seg_base[t.first + t.n] = (unsigned long long)t.seg_base[t.n];
    wg_base[t.first + t.n] = (unsigned long long)t.wg_base[t.n];
  }
}

// blockIdx.y: stream t.first + y of the chunk; pieces of 64 symbols as ent_histogram_nbr_kernel.  A
// symbol >= nsym counts nowhere (its class, as a neighbour, is 1).  LDS: the workgroup's own
// counters, added to the stream's once.
template <int LDS>
__global__ void __launch_bounds__(256) emb_histogram_kernel(const EntChunk t, const EmbModel m,
                                                            const uint8_t* __restrict__ sym, uint32_t L,
                                                            unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned long long s_cnt[];
  const int i = blockIdx.y;
  if (i >= t.n) return;
  const uint32_t nsym = m.nsym, entries = m.rows * nsym;
  if (LDS) {
    for (uint32_t e = threadIdx.x; e < entries; e += 256) s_cnt[e] = 0;
    __syncthreads();
  }
  unsigned long long* mine = counts + (size_t)(t.first + i) * entries;
  const unsigned long long n = (unsigned long long)t.count[i];
  const uint8_t* src = sym + t.in_off[i];
  const unsigned long long per = (L + 63) / 64, pieces = ((n + L - 1) / L) * per;
  EntNbr q = m.q;
  q.ncum = 1;  // `row` then counts table rows, not words
  for (unsigned long long pc = (unsigned long long)blockIdx.x * 256 + threadIdx.x; pc < pieces;
       pc += (unsigned long long)gridDim.x * 256) {
    const unsigned long long seg0 = (pc / per) * L, a = seg0 + (pc % per) * 64;
    unsigned long long e = a + 64;
    if (e > seg0 + L) e = seg0 + L;
    if (e > n) e = n;
    if (a >= e) continue;
    EntNbrPos at;
    at.start(q, a);
    for (unsigned long long k = a; k < e; ++k) {
      uint32_t nb = 0;
      if (m.useW && at.w && k - seg0 >= q.C) nb = 1u + (2u * src[k - q.C] >= nsym ? 1u : 0u);
      if (q.two && at.h && k - seg0 >= q.rowC) nb += 3u * (1u + (2u * src[k - q.rowC] >= nsym ? 1u : 0u));
      const uint32_t row = at.row + nb;
      at.advance(q, m.rows);
      const uint32_t v = src[k];
      if (v < nsym) {
        if (LDS) atomicAdd(&s_cnt[row * nsym + v], 1ull);
        else atomicAdd(&mine[(size_t)row * nsym + v], 1ull);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < entries; e += 256)
      if (s_cnt[e]) atomicAdd(&mine[e], s_cnt[e]);
  }
}

// Thread (blockIdx.y * 256 + x) of stream blockIdx.x: one table row by the fit rule.
__global__ void __launch_bounds__(256) emb_fit_kernel(const EmbModel m, const unsigned long long* __restrict__ counts,
                                                      uint32_t* __restrict__ tabs, uint8_t* __restrict__ tblk) {
  const uint32_t r = blockIdx.y * 256 + threadIdx.x;
  if (r >= m.rows) return;
  const size_t i = blockIdx.x;
  const uint32_t nsym = m.nsym;
  const unsigned long long* c = counts + (i * m.rows + r) * nsym;
  unsigned long long nr = 0;
  uint32_t best = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    nr += c[s];
    if (c[s] > c[best]) best = s;
  }
  const unsigned long long scale = kEmbTotal - nsym;
  uint32_t deficit = 0;
  if (nr) {
    uint32_t sum = 0;
    for (uint32_t s = 0; s < nsym; ++s) sum += 1u + (uint32_t)(c[s] * scale / nr);
    deficit = kEmbTotal - sum;
  }
  uint32_t* row = tabs + i * m.words + (size_t)r * (nsym + 1);
  uint8_t* blk = tblk + i * m.T + (size_t)r * (nsym - 1) * 2;
  uint32_t cum = 0;
  row[0] = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    uint32_t f;
    if (nr) f = 1u + (uint32_t)(c[s] * scale / nr) + (s == best ? deficit : 0u);
    else f = kEmbTotal * (s + 1) / nsym - kEmbTotal * s / nsym;
    if (s + 1 < nsym) {
      blk[2 * s] = (uint8_t)(f & 0xFFu);
      blk[2 * s + 1] = (uint8_t)(f >> 8);
    }
    cum += f;
    row[s + 1] = cum;
  }
}

// --- CRC-32C of a block by one wave ---
// a * b modulo the polynomial, operands bit-reflected (bit 31 is x^0), as zlib's crc32_combine does it.
__host__ __device__ inline uint32_t emb_multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t mask = 1u << 31; mask; mask >>= 1) {
    if (a & mask) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kEmbPoly : b >> 1;
  }
  return p;
}
// x2n[k] = x^(2^k) modulo the polynomial
__host__ __device__ inline void emb_x2n_table(uint32_t* x2n) {
  uint32_t p = 1u << 30;  // x^1
  x2n[0] = p;
  for (int k = 1; k < 32; ++k) x2n[k] = p = emb_multmodp(p, p);
}
// x^(8 * n) modulo the polynomial
__host__ __device__ inline uint32_t emb_x8n(const uint32_t* x2n, unsigned long long n) {
  uint32_t p = 1u << 31;  // x^0
  for (unsigned k = 3; n; n >>= 1, ++k)
    if (n & 1) p = emb_multmodp(x2n[k & 31], p);
  return p;
}
// tic_crc32c(p, n, 0), a bit at a time
__host__ __device__ inline uint32_t emb_crc_bytes(const uint8_t* p, size_t n) {
  uint32_t c = ~0u;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (kEmbPoly & (0u - (c & 1u)));
  }
  return ~c;
}

// Workgroup i (one wave): the CRC-32C of stream i's table block of T bytes.  ENC: the block lies at
// tblk + i*T and the CRC goes to crc[i].  Else the block lies in container i at byte 40 (only
// looked at when the record is valid, which says that it lies inside the container) and a CRC that
// differs from the header's sets flag[i].
template <int ENC>
__global__ void __launch_bounds__(64) emb_crc_kernel(const uint8_t* __restrict__ base, const EntRec* __restrict__ rec,
                                                     uint32_t T, uint32_t* __restrict__ out) {
  __shared__ uint32_t s_x2n[32], s_crc[64];
  __shared__ unsigned long long s_len[64];
  const int i = blockIdx.x, l = threadIdx.x;
  if (!ENC && !rec[i].valid) return;
  const uint8_t* blk = ENC ? base + (size_t)i * T : base + rec[i].in_off + kEmbHeader;
  if (l == 0) emb_x2n_table(s_x2n);
  const uint32_t cs = (T + 63) / 64;
  const uint32_t a = min(T, (uint32_t)l * cs), e = min(T, (uint32_t)(l + 1) * cs);
  s_crc[l] = emb_crc_bytes(blk + a, e - a);
  s_len[l] = e - a;
  __syncthreads();
  for (int d = 1; d < 64; d <<= 1) {
    if ((l & (2 * d - 1)) == 0) {
      s_crc[l] = emb_multmodp(emb_x8n(s_x2n, s_len[l + d]), s_crc[l]) ^ s_crc[l + d];
      s_len[l] += s_len[l + d];
    }
    __syncthreads();
  }
  if (l == 0) {
    if (ENC) {
      out[i] = s_crc[0];
    } else {
      const uint8_t* p = base + rec[i].in_off + 36;
      const uint32_t want = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
      if (want != s_crc[0]) out[i] = 1;
    }
  }
}

// Workgroup b belongs to one stream: segment (b - wg_base[i]) * 64 + lane of stream i.
template <int LDS>
__global__ void __launch_bounds__(64) emb_encode_kernel(const uint32_t* __restrict__ tabs, const EmbModel m,
                                                        const uint8_t* __restrict__ sym,
                                                        const EntRec* __restrict__ rec,
                                                        const unsigned long long* __restrict__ seg_base,
                                                        const unsigned long long* __restrict__ wg_base,
                                                        int n_streams, uint32_t L, uint8_t* __restrict__ slots,
                                                        uint32_t* __restrict__ seg_len) {
  extern __shared__ uint32_t s_dyn[];
  const EntNbr q = m.q;
  const uint32_t ncum = q.ncum, words = m.words;
  const int i = ent_find(wg_base, n_streams, blockIdx.x);
  const uint32_t* g_tab = tabs + (size_t)i * words;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < words; k += 64) s_dyn[k] = g_tab[k];
    __syncthreads();
  }
  auto tab = [&](uint32_t k) -> uint32_t { return LDS ? s_dyn[k] : g_tab[k]; };
  const unsigned long long j = (blockIdx.x - wg_base[i]) * 64 + threadIdx.x;
  if (j >= seg_base[i + 1] - seg_base[i]) return;
  const unsigned long long g = seg_base[i] + j;
  const long long left = rec[i].count - (long long)(j * L);
  const uint32_t cnt = left < (long long)L ? (uint32_t)left : L;
  const uint8_t* src = sym + rec[i].in_off + (long long)(j * L);
  uint32_t* out = reinterpret_cast<uint32_t*>(slots + (size_t)g * ent_stride(L));

  const uint32_t nsym = m.nsym;
  EntNbrPos at;
  at.start(q, j * L);  // every stream starts at position 0 of a patch
  unsigned long long low = 0, range = 1ull << 32;
  int cache = -1;
  uint32_t pending = 0, nout = 0, acc = 0;
  bool bad = false;

  auto put = [&](uint32_t b) {
    acc |= (b & 0xFFu) << (8 * (nout & 3));
    ++nout;
    if ((nout & 3) == 0) {
      out[(nout >> 2) - 1] = acc;
      acc = 0;
    }
  };
  auto emit_top = [&]() {
    if (low < 0xFF000000ull || low >= (1ull << 32)) {
      const uint32_t carry = low >= (1ull << 32) ? 1u : 0u;
      if (cache >= 0) put((uint32_t)cache + carry);
      for (; pending; --pending) put(0xFFu + carry);
      cache = (int)((low >> 24) & 0xFF);
    } else {
      ++pending;
    }
    low = (low << 8) & 0xFFFFFFFFull;
  };
  // symbol s at segment-local index k; clsW, clsN: the classes of the symbols at k - C and k - ew*C
  // (read only where that index lies inside the segment)
  auto step = [&](uint32_t k, uint32_t s, uint32_t clsW, uint32_t clsN) {
    uint32_t nb = 0;
    if (m.useW && at.w && k >= q.C) nb = 1u + clsW;
    if (q.two && at.h && k >= q.rowC) nb += 3u * (1u + clsN);
    const uint32_t r0 = at.row + nb * ncum;
    at.advance(q, words);
    if (s >= nsym) {
      bad = true;
      return;
    }
    const uint32_t start = tab(r0 + s), next = tab(r0 + s + 1);
    const unsigned long long r = range >> kEmbShift;
    const unsigned long long sr = (unsigned long long)start * r;
    low += sr;
    range = next == kEmbTotal ? range - sr : (unsigned long long)(next - start) * r;
    while (range < (1ull << 24)) {
      range <<= 8;
      emit_top();
    }
  };

  auto cls = [&](uint32_t at_k) -> uint32_t { return 2u * src[at_k] >= nsym ? 1u : 0u; };
  auto one = [&](uint32_t k) {
    step(k, src[k], m.useW && k >= q.C ? cls(k - q.C) : 0u, q.two && k >= q.rowC ? cls(k - q.rowC) : 0u);
  };
  uint32_t k = 0;
  for (; k < cnt && ((uintptr_t)(src + k) & 15) != 0; ++k) one(k);
  for (; k + 16 <= cnt; k += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + k);
    // the block's 16 + 16 neighbour classes as bit masks: independent loads, all in flight before
    // the chain of 16 symbols starts
    uint32_t mW = 0, mN = 0;
    if (m.useW && k + 15 >= q.C) {
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (k + b >= q.C) mW |= cls(k + b - q.C) << b;
    }
    if (q.two && k + 15 >= q.rowC) {
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (k + b >= q.rowC) mN |= cls(k + b - q.rowC) << b;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      uint32_t x = w[qq];
#pragma unroll 1
      for (int b = 0; b < 4; ++b) {
        step(k + 4 * qq + b, x & 0xFFu, mW & 1u, mN & 1u);
        x >>= 8;
        mW >>= 1;
        mN >>= 1;
      }
    }
  }
  for (; k < cnt; ++k) one(k);

  // the minimal flush (range_coder.cpp EncCore::finish)
  int nb = 0;
  unsigned long long v = low;
  for (; nb <= 4; ++nb) {
    if (nb == 4) {
      v = low;
    } else {
      const unsigned long long unit = 1ull << (32 - 8 * nb);
      v = (low + unit - 1) & ~(unit - 1);
    }
    if (v < low + range) break;
  }
  low = v;
  for (int qq = 0; qq < nb; ++qq) emit_top();
  if (nb > 0) {
    if (cache >= 0) put((uint32_t)cache);
    for (; pending; --pending) put(0xFFu);
  } else if (cache >= 0) {
    const uint32_t carry = v >= (1ull << 32) ? 1u : 0u;
    put((uint32_t)cache + carry);
    for (; pending; --pending) put(0xFFu + carry);
  }
  if (nout & 3) out[nout >> 2] = acc;  // the slot is a multiple of 4 bytes
  seg_len[g] = bad ? kEntBad : nout;
}

// ent_seg_scan_kernel with the header's size (40 + T) as an argument.
__global__ void __launch_bounds__(256) emb_seg_scan_kernel(const unsigned long long* __restrict__ seg_base,
                                                           const uint32_t* __restrict__ seg_len, uint32_t hdr,
                                                           unsigned long long* __restrict__ seg_off,
                                                           unsigned long long* __restrict__ sizes) {
  __shared__ unsigned long long s[256];
  __shared__ int s_bad;
  const int i = blockIdx.x, t = threadIdx.x;
  const unsigned long long b = seg_base[i], S = seg_base[i + 1] - b;
  if (t == 0) s_bad = 0;
  __syncthreads();
  unsigned long long carry = 0;
  bool bad = false;
  for (unsigned long long j0 = 0; j0 < S; j0 += 256) {
    const unsigned long long j = j0 + t;
    uint32_t len = j < S ? seg_len[b + j] : 0;
    if (len == kEntBad) {
      bad = true;
      len = 0;
    }
    const unsigned long long inc = ent_block_scan(len, s);
    if (j < S) seg_off[b + j] = carry + inc - len;
    carry += s[255];
    __syncthreads();
  }
  if (bad) s_bad = 1;  // every writer stores the same value
  __syncthreads();
  if (t == 0) sizes[i] = s_bad ? ~0ull : (unsigned long long)hdr + 2ull * S + carry;
}

// Workgroup g: segment g's payload and its length to their places; the first segment's workgroup
// also writes the header and the table block.
__global__ void __launch_bounds__(256) emb_gather_kernel(const EmbModel m, const EntRec* __restrict__ rec,
                                                         const unsigned long long* __restrict__ seg_base,
                                                         int n_streams, uint32_t L, const uint8_t* __restrict__ slots,
                                                         const uint32_t* __restrict__ seg_len,
                                                         const unsigned long long* __restrict__ seg_off,
                                                         const unsigned long long* __restrict__ sizes,
                                                         const unsigned long long* __restrict__ out_off,
                                                         const uint8_t* __restrict__ tblk,
                                                         const uint32_t* __restrict__ crc, uint8_t* __restrict__ out) {
  const unsigned long long g = blockIdx.x;
  const int i = ent_find(seg_base, n_streams, g);
  if (sizes[i] == ~0ull) return;
  const unsigned long long j = g - seg_base[i], S = seg_base[i + 1] - seg_base[i];
  uint8_t* base = out + out_off[i];
  const uint32_t t = threadIdx.x, hdr = kEmbHeader + m.T;
  const uint32_t len = seg_len[g];
  if (j == 0) {
    if (t < kEmbHeader) {
      const unsigned long long n = (unsigned long long)rec[i].count;
      uint32_t b;
      if (t < 4) b = (0x41434954u >> (8 * t)) & 0xFFu;  // "TICA"
      else if (t == 4) b = 1u;
      else if (t == 5) b = m.nbrs;
      else if (t < 8) b = (m.nsym >> (8 * (t - 6))) & 0xFFu;
      else if (t < 12) b = (L >> (8 * (t - 8))) & 0xFFu;
      else if (t < 20) b = (uint32_t)(n >> (8 * (t - 12))) & 0xFFu;
      else if (t < 24) b = (m.q.K0 >> (8 * (t - 20))) & 0xFFu;
      else if (t < 26) b = (m.q.eh >> (8 * (t - 24))) & 0xFFu;
      else if (t < 28) b = (m.q.ew >> (8 * (t - 26))) & 0xFFu;
      else if (t < 30) b = (m.q.C >> (8 * (t - 28))) & 0xFFu;
      else if (t < 32) b = 0u;
      else if (t < 36) b = (m.T >> (8 * (t - 32))) & 0xFFu;
      else b = (crc[i] >> (8 * (t - 36))) & 0xFFu;
      base[t] = (uint8_t)b;
    }
    const uint8_t* tb = tblk + (size_t)i * m.T;
    for (uint32_t k = t; k < m.T; k += 256) base[kEmbHeader + k] = tb[k];
  }
  if (t < 2) base[hdr + 2 * j + t] = (uint8_t)(len >> (8 * t));
  const uint8_t* src = slots + (size_t)g * ent_stride(L);
  uint8_t* dst = base + hdr + 2 * S + seg_off[g];
  for (uint32_t k = t; k < len; k += 256) dst[k] = src[k];
}

// Lane k: the header of container first + k against the caller's model, count and size.  seg_cnt
// receives its segments (RNG: those its range touches), wg_cnt the workgroups of `lanes` segments
// they need, flag a zero that the table and CRC kernels may set.
template <int RNG>
__global__ void __launch_bounds__(64) emb_dec_header_kernel(const EntChunk t, const EmbModel m, uint32_t lanes,
                                                            const uint8_t* __restrict__ blob,
                                                            EntRec* __restrict__ rec,
                                                            unsigned long long* __restrict__ seg_cnt,
                                                            unsigned long long* __restrict__ wg_cnt,
                                                            uint32_t* __restrict__ flag, const EntRngChunk<RNG> rg,
                                                            EntRng* __restrict__ rng) {
  const int k = threadIdx.x;
  if (k >= t.n) return;
  EntRec r;
  r.in_off = t.in_off[k];
  r.in_size = t.in_size[k];
  r.count = t.count[k];
  r.out_off = t.out_off[k];
  r.L = 0;
  r.valid = 0;
  unsigned long long S = 0;
  const unsigned long long hdr = (unsigned long long)kEmbHeader + m.T;
  if ((unsigned long long)r.in_size >= hdr) {
    const uint8_t* p = blob + r.in_off;
    auto u16 = [&](int at) { return (uint32_t)p[at] | (uint32_t)p[at + 1] << 8; };
    auto u32 = [&](int at) { return u16(at) | u16(at + 2) << 16; };
    const uint32_t L = u32(8);
    const unsigned long long n = (unsigned long long)u32(12) | (unsigned long long)u32(16) << 32;
    bool ok = p[0] == 'T' && p[1] == 'I' && p[2] == 'C' && p[3] == 'A' && p[4] == 1 && p[5] == m.nbrs &&
              u16(6) == m.nsym && u32(20) == m.q.K0 && u16(24) == m.q.eh && u16(26) == m.q.ew && u16(28) == m.q.C &&
              !p[30] && !p[31] && u32(32) == m.T;
    ok = ok && L >= 4 && L <= kEntMaxL && (L & 3) == 0 && n == (unsigned long long)r.count;
    if (ok) {
      S = (n + L - 1) / L;
      if (S > ((unsigned long long)r.in_size - hdr) / 2) ok = false;
    }
    if constexpr (RNG != 0) {
      const unsigned long long a = (unsigned long long)rg.first[k], c = (unsigned long long)rg.count[k];
      if (ok && (c == 0 || a >= n || c > n - a)) ok = false;
      if (ok) S = (a + c - 1) / L - a / L + 1;
    }
    if (ok) {
      r.L = L;
      r.valid = 1;
    } else {
      S = 0;
    }
  }
  rec[t.first + k] = r;
  seg_cnt[t.first + k] = S;
  wg_cnt[t.first + k] = (S + lanes - 1) / lanes;
  flag[t.first + k] = 0;
  if constexpr (RNG != 0) {
    EntRng q;
    q.first = rg.first[k];
    q.count = rg.count[k];
    rng[t.first + k] = q;
  }
}

// Thread (blockIdx.y * 256 + x) of container blockIdx.x: one row of its table block to a cumulative
// row in the scratch.  A zero frequency or a row sum above 4095 sets flag (the row written then is
// never used).
__global__ void __launch_bounds__(256) emb_dec_tables_kernel(const EmbModel m, const uint8_t* __restrict__ blob,
                                                             const EntRec* __restrict__ rec,
                                                             uint32_t* __restrict__ tabs, uint32_t* __restrict__ flag) {
  const uint32_t r = blockIdx.y * 256 + threadIdx.x;
  const size_t i = blockIdx.x;
  if (r >= m.rows || !rec[i].valid) return;
  const uint32_t nsym = m.nsym;
  const uint8_t* blk = blob + rec[i].in_off + kEmbHeader + (size_t)r * (nsym - 1) * 2;
  uint32_t* row = tabs + i * m.words + (size_t)r * (nsym + 1);
  uint32_t cum = 0;
  bool bad = false;
  row[0] = 0;
  for (uint32_t s = 0; s + 1 < nsym; ++s) {
    const uint32_t f = (uint32_t)blk[2 * s] | (uint32_t)blk[2 * s + 1] << 8;
    if (f == 0) bad = true;
    cum += f;
    if (cum >= kEmbTotal) {
      bad = true;
      cum = kEmbTotal - 1;
    }
    row[s + 1] = cum;
  }
  row[nsym] = kEmbTotal;
  if (bad) flag[i] = 1;  // every writer stores the same value
}

// ent_dec_scan_kernel with the header's size as an argument; a container whose flag is set becomes
// zeros like one whose header does not fit.
template <int RNG>
__global__ void __launch_bounds__(256) emb_dec_scan_kernel(const uint8_t* __restrict__ blob, EntRec* __restrict__ rec,
                                                           const uint32_t* __restrict__ flag, uint32_t hdr,
                                                           const unsigned long long* __restrict__ seg_base,
                                                           unsigned long long cap,
                                                           unsigned long long* __restrict__ seg_off,
                                                           uint8_t* __restrict__ d_sym,
                                                           const EntRng* __restrict__ rng) {
  __shared__ unsigned long long s[256];
  const int i = blockIdx.x, t = threadIdx.x;
  const EntRec r = rec[i];
  const unsigned long long b = seg_base[i], S = seg_base[i + 1] - b;
  const long long fill = RNG ? rng[i].count : r.count;
  if (!r.valid || flag[i] || b + S > cap) {
    uint8_t* dst = d_sym + r.out_off;
    for (long long k = t; k < fill; k += 256) dst[k] = 0;
    __syncthreads();  // every thread has read rec[i]
    if (t == 0) rec[i].valid = 0;
    return;
  }
  const uint8_t* lens = blob + r.in_off + hdr;
  const unsigned long long Sc = RNG ? ((unsigned long long)r.count + r.L - 1) / r.L : S;
  const unsigned long long j0 = RNG ? (unsigned long long)rng[i].first / r.L : 0, je = j0 + S;
  unsigned long long carry = (unsigned long long)hdr + 2ull * Sc;
  for (unsigned long long jb = 0; jb < je; jb += 256) {
    const unsigned long long j = jb + t;
    const uint32_t len = j < je ? (uint32_t)lens[2 * j] | (uint32_t)lens[2 * j + 1] << 8 : 0;
    const unsigned long long inc = ent_block_scan(len, s);
    if (j < je && j >= j0) seg_off[b + j - j0] = carry + inc - len;
    carry += s[255];
    __syncthreads();
  }
  if (RNG && carry > (unsigned long long)r.in_size) {  // uniform: every thread holds the same carry
    uint8_t* dst = d_sym + r.out_off;
    for (long long k = t; k < fill; k += 256) dst[k] = 0;
    if (t == 0) rec[i].valid = 0;
  }
}

// ent_decode_nbr_kernel under per-stream tables.  The work items are workgroups of LN segments of
// one stream (wg_base), grid-stride; a workgroup stages its stream's tables (LDS) before it decodes.
// Dynamic LDS: the tables (LDS), then the rings (RING, or RNG).
template <int LDS, int RING, int RNG>
__global__ void __launch_bounds__(64) emb_decode_kernel(const uint32_t* __restrict__ tabs, const EmbModel m,
                                                        uint32_t hdr, const uint8_t* __restrict__ blob,
                                                        const EntRec* __restrict__ rec,
                                                        const unsigned long long* __restrict__ seg_base,
                                                        const unsigned long long* __restrict__ wg_base,
                                                        int n_streams,
                                                        const unsigned long long* __restrict__ seg_off,
                                                        uint8_t* d_sym, const EntRng* __restrict__ rng) {
  constexpr int LN = (RNG != 0 && !RING) ? 32 : 64;  // working lanes; ring words of a lane lie LN apart
  constexpr bool kRing = RING || RNG != 0;
  extern __shared__ uint32_t s_dyn[];
  const EntNbr q = m.q;
  const unsigned long long W = wg_base[n_streams];
  const uint32_t ncum = q.ncum, words = m.words, nsym = m.nsym;
  uint32_t* ring = s_dyn + (LDS ? words : 0) + threadIdx.x;  // this lane's words, LN apart
  const uint32_t R = q.ring;
  const bool useN = q.two && q.rowC == R;  // else no segment reaches its N neighbour
  const bool two = nsym == 2;
  int staged = -1;

  for (unsigned long long wb = blockIdx.x; wb < W; wb += gridDim.x) {  // wb, i: the same in every lane
    const int i = ent_find(wg_base, n_streams, wb);
    const uint32_t* g_tab = tabs + (size_t)i * words;
    if (LDS) {
      __syncthreads();  // the lanes of the previous item have finished with the tables
      if (i != staged)
        for (uint32_t k = threadIdx.x; k < words; k += 64) s_dyn[k] = g_tab[k];
      staged = i;
      __syncthreads();
    }
    auto tab = [&](uint32_t k) -> uint32_t { return LDS ? s_dyn[k] : g_tab[k]; };
    const EntRec r = rec[i];
    if (!r.valid) continue;
    if (LN < 64 && threadIdx.x >= LN) continue;  // these lanes only help to stage the tables
    const unsigned long long jl = (wb - wg_base[i]) * LN + threadIdx.x;
    if (jl >= seg_base[i + 1] - seg_base[i]) continue;
    const unsigned long long g = seg_base[i] + jl;
    unsigned long long j = jl;
    if constexpr (RNG != 0) j += (unsigned long long)rng[i].first / r.L;
    const long long left = r.count - (long long)(j * r.L);
    uint32_t cnt = left < (long long)r.L ? (uint32_t)left : r.L;
    const uint8_t* cont = blob + r.in_off;
    const uint32_t len = (uint32_t)cont[hdr + 2 * j] | (uint32_t)cont[hdr + 2 * j + 1] << 8;
    // the segment's extent, clamped to the container
    const unsigned long long size = (unsigned long long)r.in_size;
    unsigned long long pos = seg_off[g];
    if (pos > size) pos = size;
    unsigned long long end = pos + len;
    if (end > size) end = size;
    uint8_t* dst = d_sym + r.out_off + (long long)(j * r.L);
    uint32_t lo = 0;  // the first symbol of the segment that is stored
    if constexpr (RNG != 0) {
      const long long first = rng[i].first, b = (long long)(j * r.L), stop = first + rng[i].count - b;
      if (stop < (long long)cnt) cnt = (uint32_t)stop;
      if (first > b) lo = (uint32_t)(first - b);
      dst = d_sym + (r.out_off + b - first);  // dst[k] is touched for k >= lo only
    }
    EntNbrPos at;
    at.start(q, j * r.L);
    uint32_t rp = 0, rw = R ? (R - q.C % R) % R : 0;  // ring places of symbol k - R and of symbol k - C
    // the ring word that holds place rp, kept in a register and written back when rp leaves it
    uint32_t far = kRing && R ? ring[0] : 0u;

    auto get = [&]() -> uint32_t { return pos < end ? (uint32_t)cont[pos++] : 0u; };
    uint32_t code = 0;
    for (int b = 0; b < 4; ++b) code = (code << 8) | get();
    unsigned long long range = 1ull << 32;
    // symbol at segment-local index k
    auto dec = [&](uint32_t k) -> uint32_t {
      uint32_t nb = 0;
      if (kRing) {
        if (R) {
          // a place in the word under rp is read from the register: the word in LDS is older
          const uint32_t near = (rw >> 5) == (rp >> 5) ? far : ring[(rw >> 5) * LN];
          if (at.w && k >= q.C) nb = 1u + ((near >> (rw & 31)) & 1u);
          if (useN && at.h && k >= R) nb += 3u * (1u + ((far >> (rp & 31)) & 1u));
        }
      } else {
        if (m.useW && at.w && k >= q.C) nb = 1u + (2u * dst[k - q.C] >= nsym ? 1u : 0u);
        if (q.two && at.h && k >= q.rowC) nb += 3u * (1u + (2u * dst[k - q.rowC] >= nsym ? 1u : 0u));
      }
      const uint32_t r0 = at.row + nb * ncum;
      at.advance(q, words);
      const unsigned long long rr = range >> kEmbShift;
      uint32_t val = (rr >> 32) ? 0u : code / (uint32_t)rr;
      if (val >= kEmbTotal) val = kEmbTotal - 1;
      uint32_t s;
      if (two) {
        s = val >= tab(r0 + 1) ? 1u : 0u;
      } else {
        uint32_t a = 0, hi = nsym - 1;  // last s with cum[s] <= val
        while (a < hi) {
          const uint32_t mid = (a + hi + 1) >> 1;
          if (tab(r0 + mid) <= val) a = mid;
          else hi = mid - 1;
        }
        s = a;
      }
      const uint32_t start = tab(r0 + s), next = tab(r0 + s + 1);
      const unsigned long long sr = (unsigned long long)start * rr;
      code -= (uint32_t)sr;
      range = next == kEmbTotal ? range - sr : (unsigned long long)(next - start) * rr;
      while (range < (1ull << 24)) {
        range <<= 8;
        code = (code << 8) | get();
      }
      if (kRing && R) {  // this symbol's class replaces that of symbol k - R
        const uint32_t bit = 1u << (rp & 31), word = rp >> 5;
        far = 2u * s >= nsym ? far | bit : far & ~bit;
        if (++rp == R) rp = 0;
        if (++rw == R) rw = 0;
        if ((rp >> 5) != word) {
          ring[word * LN] = far;
          far = ring[(rp >> 5) * LN];
        }
      }
      return s;
    };

    if (kRing) {
      uint32_t k = 0;
      for (; k < lo; ++k) (void)dec(k);  // RNG: in front of the range
      for (; k < cnt && ((uintptr_t)(dst + k) & 3) != 0; ++k) dst[k] = (uint8_t)dec(k);
      for (; k + 4 <= cnt; k += 4) {
        uint32_t w = 0;
#pragma unroll 1
        for (int b = 0; b < 4; ++b) w |= dec(k + b) << (8 * b);
        *reinterpret_cast<uint32_t*>(dst + k) = w;
      }
      for (; k < cnt; ++k) dst[k] = (uint8_t)dec(k);
    } else {
      for (uint32_t k = 0; k < cnt; ++k) dst[k] = (uint8_t)dec(k);
    }
  }
}

}  // namespace tic

namespace {

int emb_model(size_t K0, uint32_t neighbours, size_t nsym, uint32_t eh, uint32_t ew, uint32_t C, tic::EmbModel* m) {
  size_t b = 0;
  if (tic_rcseg_bound_emb(1, 4, K0, neighbours, nsym, &b)) return fail(TIC_EINVAL, "%s", tic_rc_last_error());
  if (eh < 1 || ew < 1 || C < 1 || eh > 65535 || ew > 65535 || C > 65535)
    return fail(TIC_EINVAL, "code geometry %u x %u x %u must be in [1, 65535] each", eh, ew, C);
  memset(m, 0, sizeof(*m));
  tic::EntNbr& q = m->q;
  q.K0 = (uint32_t)K0;
  q.M = neighbours == 0 ? 1 : neighbours == 1 ? 3 : 9;
  q.ncum = (uint32_t)nsym + 1;
  q.two = neighbours == 2;
  q.eh = eh, q.ew = ew, q.C = C;
  q.rowC = ew * C;
  q.ring = neighbours == 0 ? 0 : q.two && q.rowC < tic::kEntMaxL ? q.rowC : (C < tic::kEntMaxL ? C : 0);
  m->useW = neighbours >= 1;
  m->nbrs = neighbours;
  m->nsym = (uint32_t)nsym;
  m->rows = q.K0 * q.M;
  m->words = m->rows * q.ncum;
  m->T = m->rows * ((uint32_t)nsym - 1) * 2;
  return TIC_OK;
}

size_t emb_align(size_t b) { return (b + 15) & ~(size_t)15; }
// seg_base, aux, wg_base, aux2: u64[n + 1] each; the records; a u32 per stream (CRC / flag)
size_t emb_fixed(int n) { return emb_align(4 * ((size_t)n + 1) * 8 + (size_t)n * sizeof(tic::EntRec) + (size_t)n * 4); }

struct EmbScratch {
  unsigned long long *seg_base, *aux, *wg_base, *aux2, *seg_off, *counts;
  tic::EntRec* rec;
  uint32_t *word, *tabs, *seg_len;  // word: the stream's CRC (encoder) or flag (decoder)
  uint8_t *tblk, *slots;
  tic::EntRng* rng;
};
size_t emb_enc_bytes(const tic::EmbModel& m, int n, long long T, uint32_t L) {
  return emb_fixed(n) + (size_t)n * m.rows * m.nsym * 8 + emb_align((size_t)n * m.words * 4) + emb_align((size_t)n * m.T) +
         emb_align((size_t)T * 12) + (size_t)T * tic::ent_stride(L);
}
// what the decoder needs in front of its per-segment offsets
size_t emb_dec_fixed(const tic::EmbModel& m, int n, bool rng) {
  return emb_fixed(n) + emb_align((size_t)n * m.words * 4) + (rng ? (size_t)n * sizeof(tic::EntRng) : 0);
}
EmbScratch emb_carve(void* d_scratch, const tic::EmbModel& m, int n, long long T, bool enc, bool rng) {
  EmbScratch s;
  memset(&s, 0, sizeof(s));
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  s.seg_base = reinterpret_cast<unsigned long long*>(p);
  s.aux = s.seg_base + n + 1;
  s.wg_base = s.aux + n + 1;
  s.aux2 = s.wg_base + n + 1;
  s.rec = reinterpret_cast<tic::EntRec*>(s.aux2 + n + 1);
  s.word = reinterpret_cast<uint32_t*>(s.rec + n);
  p += emb_fixed(n);
  if (enc) {
    s.counts = reinterpret_cast<unsigned long long*>(p);
    p += (size_t)n * m.rows * m.nsym * 8;
  }
  s.tabs = reinterpret_cast<uint32_t*>(p);
  p += emb_align((size_t)n * m.words * 4);
  if (enc) {
    s.tblk = p;
    p += emb_align((size_t)n * m.T);
  }
  if (rng) {
    s.rng = reinterpret_cast<tic::EntRng*>(p);
    p += (size_t)n * sizeof(tic::EntRng);
  }
  s.seg_off = reinterpret_cast<unsigned long long*>(p);
  if (enc) {
    s.seg_len = reinterpret_cast<uint32_t*>(s.seg_off + T);
    s.slots = p + emb_align((size_t)T * 12);
  }
  return s;
}

// The per-stream histogram launches.
int emb_histogram(tic_handle* h, const tic::EmbModel& m, const uint8_t* d_sym, const int64_t* sym_offsets,
                  const int64_t* counts, int n_streams, uint32_t L, unsigned long long* d_counts) {
  const size_t lds = (size_t)m.rows * m.nsym * 8;
  const bool in_lds = lds <= 32 * 1024;
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EntChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    long long most = 0;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = sym_offsets[f + k];
      t.count[k] = counts[f + k];
      most = std::max(most, (long long)counts[f + k]);
    }
    // pieces of 64 symbols, 256 to a workgroup
    const unsigned gx = (unsigned)std::min<long long>((most / 64 + 256) / 256, (long long)h->num_cus * 8);
    touch(h);
    if (in_lds)
      hipLaunchKernelGGL(tic::emb_histogram_kernel<1>, dim3(gx, (unsigned)t.n), dim3(256), lds, h->stream, t, m, d_sym,
                         L, d_counts);
    else
      hipLaunchKernelGGL(tic::emb_histogram_kernel<0>, dim3(gx, (unsigned)t.n), dim3(256), 0, h->stream, t, m, d_sym, L,
                         d_counts);
    const int rc = check_launch();
    if (rc) return rc;
  }
  return TIC_OK;
}

template <int RNG>
int emb_decode_t(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets, const int64_t* blob_sizes,
                 const int64_t* counts, const int64_t* firsts, const int64_t* rcounts, int n_streams, size_t K0,
                 uint32_t neighbours, size_t nsym, uint32_t eh, uint32_t ew, uint32_t C, uint8_t* d_sym,
                 const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  tic::EmbModel m;
  int rc = emb_model(K0, neighbours, nsym, eh, ew, C, &m);
  if (rc) return rc;
  if (n_streams == 0) return TIC_OK;
  if (!d_blob || !d_scratch || !d_sym) return fail(TIC_EINVAL, "null device pointer");
  if (!blob_offsets || !blob_sizes || !counts || !sym_offsets) return fail(TIC_EINVAL, "null per-stream array");
  if (RNG && (!firsts || !rcounts)) return fail(TIC_EINVAL, "null per-range array");
  const char* why = "";
  long long Tmin = ent_segments(counts, n_streams, tic::kEntMaxL, &why);
  if (Tmin < 0) return fail(TIC_EINVAL, "%s", why);
  if (RNG) {
    Tmin = n_streams;  // a range touches at least one segment
    for (int i = 0; i < n_streams; ++i)
      if (firsts[i] < 0 || rcounts[i] <= 0 || firsts[i] >= counts[i] || rcounts[i] > counts[i] - firsts[i])
        return fail(TIC_EINVAL, "range %d: [%lld, %lld + %lld) is empty or not inside the stream's %lld symbols", i,
                    (long long)firsts[i], (long long)firsts[i], (long long)rcounts[i], (long long)counts[i]);
  }
  for (int i = 0; i < n_streams; ++i)
    if (blob_offsets[i] < 0 || blob_sizes[i] < 0 || sym_offsets[i] < 0)
      return fail(TIC_EINVAL, "stream %d: negative offset or size", i);
  if (((uintptr_t)d_scratch & 15) != 0) return fail(TIC_EINVAL, "d_scratch must be 16-byte aligned");
  const size_t fixed = emb_dec_fixed(m, n_streams, RNG != 0);
  if (scratch_bytes < fixed + (size_t)Tmin * 8)
    return fail(TIC_EINVAL, "scratch of %zu bytes is too small (tic_entropy_%semb_scratch_bytes)", scratch_bytes,
                RNG ? "ranges_" : "");
  // segments the scratch has room for: the containers' own L decides how many there are
  const unsigned long long cap = std::min<unsigned long long>((scratch_bytes - fixed) / 8, INT_MAX);

  const size_t tab_bytes = (size_t)m.words * 4;
  const bool in_lds = tab_bytes <= kEntLdsTables;
  size_t ring_bytes = ((size_t)m.q.ring + 31) / 32 * 4 * 64;
  const bool ring = ring_bytes <= kEntLdsRings;
  const uint32_t lanes = RNG && !ring ? 32 : 64;
  if (RNG && !ring) ring_bytes /= 2;
  const size_t lds = (in_lds ? tab_bytes : 0) + (ring || RNG ? ring_bytes : 0);
  const void* fn = in_lds ? (ring ? reinterpret_cast<const void*>(tic::emb_decode_kernel<1, 1, RNG>)
                                  : reinterpret_cast<const void*>(tic::emb_decode_kernel<1, 0, RNG>))
                          : (ring ? reinterpret_cast<const void*>(tic::emb_decode_kernel<0, 1, RNG>)
                                  : reinterpret_cast<const void*>(tic::emb_decode_kernel<0, 0, RNG>));
  HIP_TRY(hipSetDevice(h->device));
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const EmbScratch s = emb_carve(d_scratch, m, n_streams, 0, false, RNG != 0);
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EntChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = blob_offsets[f + k];
      t.in_size[k] = blob_sizes[f + k];
      t.count[k] = counts[f + k];
      t.out_off[k] = sym_offsets[f + k];
    }
    tic::EntRngChunk<RNG> rg;
    if constexpr (RNG != 0) {
      memset(&rg, 0, sizeof(rg));
      for (int k = 0; k < t.n; ++k) rg.first[k] = firsts[f + k], rg.count[k] = rcounts[f + k];
    }
    touch(h);
    hipLaunchKernelGGL((tic::emb_dec_header_kernel<RNG>), dim3(1), dim3(64), 0, h->stream, t, m, lanes, d_blob, s.rec,
                       s.aux, s.aux2, s.word, rg, s.rng);
    if ((rc = check_launch())) return rc;
  }
  const tic::EntRec* rec = s.rec;
  const unsigned row_wgs = (m.rows + 255) / 256;
  hipLaunchKernelGGL(tic::emb_dec_tables_kernel, dim3((unsigned)n_streams, row_wgs), dim3(256), 0, h->stream, m, d_blob,
                     rec, s.tabs, s.word);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::emb_crc_kernel<0>, dim3((unsigned)n_streams), dim3(64), 0, h->stream, d_blob, rec, m.T,
                     s.word);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::ent_stream_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)s.aux,
                     n_streams, s.seg_base);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::ent_stream_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)s.aux2,
                     n_streams, s.wg_base);
  if ((rc = check_launch())) return rc;
  const unsigned long long *seg_base = s.seg_base, *wg_base = s.wg_base;
  const uint32_t hdr = tic::kEmbHeader + m.T;
  const tic::EntRng* crng = s.rng;
  hipLaunchKernelGGL((tic::emb_dec_scan_kernel<RNG>), dim3((unsigned)n_streams), dim3(256), 0, h->stream, d_blob, s.rec,
                     (const uint32_t*)s.word, hdr, seg_base, cap, s.seg_off, d_sym, crng);
  if ((rc = check_launch())) return rc;
  // every stream wastes less than one workgroup of lanes
  const unsigned wgs = (unsigned)std::min<unsigned long long>((cap + lanes - 1) / lanes + (unsigned)n_streams, 1u << 16);
  const uint32_t* tabs = s.tabs;
  const unsigned long long* seg_off = s.seg_off;
  if (in_lds && ring)
    hipLaunchKernelGGL((tic::emb_decode_kernel<1, 1, RNG>), dim3(wgs), dim3(64), lds, h->stream, tabs, m, hdr, d_blob,
                       rec, seg_base, wg_base, n_streams, seg_off, d_sym, crng);
  else if (in_lds)
    hipLaunchKernelGGL((tic::emb_decode_kernel<1, 0, RNG>), dim3(wgs), dim3(64), lds, h->stream, tabs, m, hdr, d_blob,
                       rec, seg_base, wg_base, n_streams, seg_off, d_sym, crng);
  else if (ring)
    hipLaunchKernelGGL((tic::emb_decode_kernel<0, 1, RNG>), dim3(wgs), dim3(64), lds, h->stream, tabs, m, hdr, d_blob,
                       rec, seg_base, wg_base, n_streams, seg_off, d_sym, crng);
  else
    hipLaunchKernelGGL((tic::emb_decode_kernel<0, 0, RNG>), dim3(wgs), dim3(64), lds, h->stream, tabs, m, hdr, d_blob,
                       rec, seg_base, wg_base, n_streams, seg_off, d_sym, crng);
  return check_launch();
}

}  // namespace

extern "C" {

int tic_histogram_streams_nbr_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                     const int64_t* counts, int n_streams, size_t nsym, uint32_t L, size_t K0,
                                     uint32_t neighbours, uint32_t eh, uint32_t ew, uint32_t C, uint64_t* d_counts) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  tic::EmbModel m;
  int rc = emb_model(K0, neighbours, nsym, eh, ew, C, &m);
  if (rc) return rc;
  if (n_streams == 0) return TIC_OK;
  if (!d_sym || !d_counts) return fail(TIC_EINVAL, "null device pointer");
  if (!sym_offsets || !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (((uintptr_t)d_counts & 7) != 0) return fail(TIC_EINVAL, "d_counts must be 8-byte aligned");
  const char* why = "";
  if (ent_segments(counts, n_streams, L, &why) < 0) return fail(TIC_EINVAL, "%s", why);
  for (int i = 0; i < n_streams; ++i)
    if (sym_offsets[i] < 0) return fail(TIC_EINVAL, "stream %d: negative offset %lld", i, (long long)sym_offsets[i]);
  HIP_TRY(hipSetDevice(h->device));
  return emb_histogram(h, m, d_sym, sym_offsets, counts, n_streams, L, reinterpret_cast<unsigned long long*>(d_counts));
}

int tic_entropy_emb_scratch_bytes(const int64_t* counts, int n_streams, uint32_t L, size_t K0, uint32_t neighbours,
                                  size_t nsym, size_t* bytes) {
  if (!bytes) return fail(TIC_EINVAL, "null bytes");
  *bytes = 0;
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (n_streams > 0 && !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  tic::EmbModel m;
  const int rc = emb_model(K0, neighbours, nsym, 1, 1, 1, &m);
  if (rc) return rc;
  const char* why = "";
  const long long T = ent_segments(counts, n_streams, L, &why);
  if (T < 0) return fail(TIC_EINVAL, "%s", why);
  *bytes = emb_enc_bytes(m, n_streams, T, L);
  return TIC_OK;
}

int tic_entropy_encode_emb_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                  const int64_t* counts, int n_streams, uint32_t L, size_t K0, uint32_t neighbours,
                                  size_t nsym, uint32_t eh, uint32_t ew, uint32_t C, void* d_scratch,
                                  size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  tic::EmbModel m;
  int rc = emb_model(K0, neighbours, nsym, eh, ew, C, &m);
  if (rc) return rc;
  if (n_streams == 0) return TIC_OK;
  if (!d_sym || !d_scratch || !d_out || !d_sizes) return fail(TIC_EINVAL, "null device pointer");
  if (!sym_offsets || !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  const char* why = "";
  const long long T = ent_segments(counts, n_streams, L, &why);
  if (T < 0) return fail(TIC_EINVAL, "%s", why);
  const size_t hdr = tic::kEmbHeader + m.T;
  size_t bound = 0;
  for (int i = 0; i < n_streams; ++i) {
    if (sym_offsets[i] < 0) return fail(TIC_EINVAL, "stream %d: negative offset %lld", i, (long long)sym_offsets[i]);
    const size_t S = ((size_t)counts[i] + L - 1) / L;
    bound += hdr + 2 * S + 3 * (size_t)counts[i] + 4 * S;
  }
  if (((uintptr_t)d_scratch & 15) != 0 || ((uintptr_t)d_sizes & 7) != 0)
    return fail(TIC_EINVAL, "d_scratch must be 16-byte and d_sizes 8-byte aligned");
  const size_t need = emb_enc_bytes(m, n_streams, T, L);
  if (scratch_bytes < need)
    return fail(TIC_EINVAL, "scratch of %zu bytes is too small (tic_entropy_emb_scratch_bytes: %zu)", scratch_bytes, need);
  if (out_cap < bound) return fail(TIC_EINVAL, "out_cap %zu is below the sum of tic_rcseg_bound_emb (%zu)", out_cap, bound);
  const size_t tab_bytes = (size_t)m.words * 4;
  const bool in_lds = tab_bytes <= kEntLdsTables;

  HIP_TRY(hipSetDevice(h->device));
  if (in_lds && tab_bytes > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tic::emb_encode_kernel<1>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes));
  const EmbScratch s = emb_carve(d_scratch, m, n_streams, T, true, false);
  long long segs = 0, wgs = 0;
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EmbChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    t.last = f + t.n == n_streams;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = sym_offsets[f + k];
      t.count[k] = counts[f + k];
      t.seg_base[k] = segs;
      t.wg_base[k] = wgs;
      const long long S = (counts[f + k] + L - 1) / L;
      segs += S;
      wgs += (S + 63) / 64;
    }
    t.seg_base[t.n] = segs;
    t.wg_base[t.n] = wgs;
    touch(h);
    hipLaunchKernelGGL(tic::emb_put_kernel, dim3(1), dim3(64), 0, h->stream, t, L, s.rec, s.seg_base, s.wg_base);
    if ((rc = check_launch())) return rc;
  }
  HIP_TRY(hipMemsetAsync(s.counts, 0, (size_t)n_streams * m.rows * m.nsym * 8, h->stream));
  if ((rc = emb_histogram(h, m, d_sym, sym_offsets, counts, n_streams, L, s.counts))) return rc;
  const unsigned row_wgs = (m.rows + 255) / 256;
  hipLaunchKernelGGL(tic::emb_fit_kernel, dim3((unsigned)n_streams, row_wgs), dim3(256), 0, h->stream, m,
                     (const unsigned long long*)s.counts, s.tabs, s.tblk);
  if ((rc = check_launch())) return rc;
  const tic::EntRec* rec = s.rec;
  hipLaunchKernelGGL(tic::emb_crc_kernel<1>, dim3((unsigned)n_streams), dim3(64), 0, h->stream, (const uint8_t*)s.tblk,
                     rec, m.T, s.word);
  if ((rc = check_launch())) return rc;
  const unsigned long long *seg_base = s.seg_base, *wg_base = s.wg_base;
  const uint32_t* tabs = s.tabs;
  if (in_lds)
    hipLaunchKernelGGL(tic::emb_encode_kernel<1>, dim3((unsigned)wgs), dim3(64), tab_bytes, h->stream, tabs, m, d_sym,
                       rec, seg_base, wg_base, n_streams, L, s.slots, s.seg_len);
  else
    hipLaunchKernelGGL(tic::emb_encode_kernel<0>, dim3((unsigned)wgs), dim3(64), 0, h->stream, tabs, m, d_sym, rec,
                       seg_base, wg_base, n_streams, L, s.slots, s.seg_len);
  if ((rc = check_launch())) return rc;
  unsigned long long* sizes = reinterpret_cast<unsigned long long*>(d_sizes);
  const uint32_t* seg_len = s.seg_len;
  hipLaunchKernelGGL(tic::emb_seg_scan_kernel, dim3((unsigned)n_streams), dim3(256), 0, h->stream, seg_base, seg_len,
                     (uint32_t)hdr, s.seg_off, sizes);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::ent_stream_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)sizes,
                     n_streams, s.aux);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::emb_gather_kernel, dim3((unsigned)T), dim3(256), 0, h->stream, m, rec, seg_base, n_streams, L,
                     (const uint8_t*)s.slots, seg_len, (const unsigned long long*)s.seg_off,
                     (const unsigned long long*)sizes, (const unsigned long long*)s.aux, (const uint8_t*)s.tblk,
                     (const uint32_t*)s.word, d_out);
  return check_launch();
}

int tic_entropy_decode_emb_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                  const int64_t* blob_sizes, const int64_t* counts, int n_streams, size_t K0,
                                  uint32_t neighbours, size_t nsym, uint32_t eh, uint32_t ew, uint32_t C, uint8_t* d_sym,
                                  const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  return emb_decode_t<0>(h, d_blob, blob_offsets, blob_sizes, counts, nullptr, nullptr, n_streams, K0, neighbours, nsym,
                         eh, ew, C, d_sym, sym_offsets, d_scratch, scratch_bytes);
}

int tic_entropy_ranges_emb_scratch_bytes(const int64_t* firsts, const int64_t* counts, int n_ranges, uint32_t L,
                                         size_t K0, uint32_t neighbours, size_t nsym, size_t* bytes) {
  if (!bytes) return fail(TIC_EINVAL, "null bytes");
  *bytes = 0;
  if (n_ranges < 0) return fail(TIC_EINVAL, "n_ranges %d is negative", n_ranges);
  if (n_ranges > 0 && (!firsts || !counts)) return fail(TIC_EINVAL, "null per-range array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  tic::EmbModel m;
  const int rc = emb_model(K0, neighbours, nsym, 1, 1, 1, &m);
  if (rc) return rc;
  long long T = 0;
  for (int i = 0; i < n_ranges; ++i) {
    if (firsts[i] < 0 || counts[i] <= 0 || counts[i] > (1ll << 40))
      return fail(TIC_EINVAL, "range %d: first %lld, count %lld", i, (long long)firsts[i], (long long)counts[i]);
    T += ent_range_segments(counts[i], L);
    if (T > INT_MAX) return fail(TIC_EINVAL, "more than 2^31 - 1 segments");
  }
  *bytes = emb_dec_fixed(m, n_ranges, true) + (size_t)T * 8;
  return TIC_OK;
}

int tic_entropy_decode_ranges_emb_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                         const int64_t* blob_sizes, const int64_t* stream_counts,
                                         const int64_t* firsts, const int64_t* counts, int n_ranges, size_t K0,
                                         uint32_t neighbours, size_t nsym, uint32_t eh, uint32_t ew, uint32_t C,
                                         uint8_t* d_sym, const int64_t* sym_offsets, void* d_scratch,
                                         size_t scratch_bytes) {
  return emb_decode_t<1>(h, d_blob, blob_offsets, blob_sizes, stream_counts, firsts, counts, n_ranges, K0, neighbours,
                         nsym, eh, ew, C, d_sym, sym_offsets, d_scratch, scratch_bytes);
}

}  // extern "C"
